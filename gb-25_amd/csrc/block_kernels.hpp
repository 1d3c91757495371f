// block_kernels.hpp -- block sums (gb25_get_block_sums, gb25_compute_block_sums, gb25_get_derived_block_sums: include/gb25.h): the
// interior of a field, or of a packed derived field, cut into boxes of bx x by x bz points; per box sum mu', sum mu' x and
// sum mu' x^2 in fp64 with mu THE MEASURE of gb25_integrate_field (k_field_moments: the same tables, the same expression --
// measure_column, measure_level of diagnostics_kernels.hpp, shared with the moving-window filter of filter_kernels.hpp) and
// mu' = mu * level_weight[k].  Coarse fields (block means), column integrals, heat content.
//
//   k_block_sums<T, LOC, ONE>  a workgroup takes one tile of W = (256 / bx) bx consecutive columns of one block row J and one block
//                     level K: grid = (ceil(Nx / W), Ny / by, k_count / bz).  ONE THREAD PER FINE COLUMN i, so that the loads of a
//                     level are coalesced along i; bx divides both W and Nx, so a segment of bx columns never straddles a tile.
//                     A thread walks the block's by rows; in each it marches the bz levels upward with the column partial
//                     c(i, j) in registers -- the loads of BLK_AHEAD levels are issued before the first of them is added: the
//                     march is bound by the latency of a load, not by its arithmetic --, writes the partial to LDS (three
//                     planes of 256 doubles, 6 KB), and after one barrier the first thread of every segment adds its bx
//                     partials in ascending i: s(I, j), which it adds to the block's sums in ascending j.  A second barrier
//                     precedes the next row's writes.  The lead threads store the planes that were asked for.
//                     ONE (bx == 1, the column integrals): a column partial IS a segment; no LDS, no barrier.
//
// Every sum starts from +0.0; a point that does not count adds nothing.  fp64 with floating-point contraction OFF: t = mu' * x
// and q = t * x round by themselves (k_field_moments forms `second` with an FMA; this kernel must not, numpy restates it).  Plain
// vector stores, no floating-point atomics: the order of every sum is a function of the box alone, so the result is bitwise
// repeatable.  The three counts of the info record are integers: a wave adds its lanes' by the shuffle tree and lane 0 stores
// them to the wave's own slot (plain stores); k_block_counts adds the slots and its few workgroups add their sums to the record
// with integer atomics, whose order cannot matter.  (One atomic per wave of k_block_sums on ONE word was the first form: a word
// takes an atomic every ~11 ns, which made 2.4 ms of the 207 360 waves of a 4 x 4 x 1 call at 1440 x 720 x 48.)  Offsets into the
// source are 64-bit.
#pragma once
#include "diagnostics_kernels.hpp"

namespace gb25 {

constexpr int BLK_THREADS = 256;   // four waves; also the largest bx
constexpr int BLK_AHEAD = 8;       // levels whose loads are in flight before the first add

struct BlockCounts {   // the device's part of gb25_block_info
  unsigned long long points, nonfinite, empty_blocks;
};
struct BlockSlot {     // the counts of one wave
  unsigned points, nonfinite, empty_blocks;
};
struct BlockArgs {
  int bx, by, bz;                       // the extents of a block
  int k_first;                          // the window's first level, in the field's own level count (metrics, weights, wetness)
  int nI, nJ, nK;                       // the result's dims
  const double* level_weight;           // by level of the field; null: mu' = mu
  double *measure, *first, *second;     // the planes, nI nJ nK each; null: not stored
  BlockSlot* slots;                     // one per wave of the launch: 4 per workgroup, workgroups in x, y, z order
};

// box: bx = Nx; pitch, plane, origin of the array's element (0, 0, k_first): a parent (the interior of the window's first
// level) or a packed derived result (whose level 0 is the window's first)
template <class T, int LOC, bool ONE>
__global__ __launch_bounds__(BLK_THREADS) void k_block_sums(Grid g, MomentsTables tab, const T* __restrict__ a, DiagBox box, BlockArgs A) {
#pragma clang fp contract(off)
  constexpr int HL = (LOC == LOC_FCC || LOC == LOC_FC) ? 1 : (LOC == LOC_CFC || LOC == LOC_CF) ? 2 : 0;
  __shared__ double lds[ONE ? 1 : 3 * BLK_THREADS];
  const int t = threadIdx.x;
  const int W = ONE ? BLK_THREADS : (BLK_THREADS / A.bx) * A.bx;
  const int i = blockIdx.x * W + t;
  const bool active = t < W && i < box.bx;
  const bool lead = active && (ONE || t % A.bx == 0);
  const int J = blockIdx.y, K = blockIdx.z;
  const int ka = K * A.bz;          // the block's first level in the array
  const int k0 = A.k_first + ka;    // ... and in the field
  double bm = 0.0, bt = 0.0, bq = 0.0;   // the block's sums (lead threads)
  unsigned points = 0, nonfinite = 0;
  for (int jj = 0; jj < A.by; jj++) {
    const int j = J * A.by + jj;
    double cm = 0.0, ct = 0.0, cq = 0.0;   // the column partial c(i, j)
    if (active && !measure_wall_row<HL>(g, j)) {
      const MeasureColumn mc = measure_column<HL>(g, tab, i, j);
      const T* col = a + (box.origin + i + box.pitch * j + box.plane * ka);
      for (int kk0 = 0; kk0 < A.bz; kk0 += BLK_AHEAD) {
        T e[BLK_AHEAD];
#pragma unroll
        for (int s = 0; s < BLK_AHEAD; s++)
          if (kk0 + s < A.bz) e[s] = col[box.plane * (kk0 + s)];
#pragma unroll
        for (int s = 0; s < BLK_AHEAD; s++) {
          if (kk0 + s >= A.bz) break;
          const int k = k0 + kk0 + s;
          double mu = measure_level<LOC>(g, mc, k);
          if (A.level_weight) mu = mu * A.level_weight[k];
          if (!(mu > 0.0)) continue;
          const double x = (double)e[s];
          if (__builtin_isfinite(x)) {
            const double tm = mu * x;
            const double q = tm * x;
            cm += mu;
            ct += tm;
            cq += q;
            points++;
          } else {
            nonfinite++;
          }
        }
      }
    }
    if (ONE) {
      bm += cm; bt += ct; bq += cq;
    } else {
      if (active) {
        lds[t] = cm;
        lds[BLK_THREADS + t] = ct;
        lds[2 * BLK_THREADS + t] = cq;
      }
      __syncthreads();
      if (lead) {
        double sm = 0.0, st = 0.0, sq = 0.0;   // the segment s(I, j)
        for (int s = 0; s < A.bx; s++) {
          sm += lds[t + s];
          st += lds[BLK_THREADS + t + s];
          sq += lds[2 * BLK_THREADS + t + s];
        }
        bm += sm; bt += st; bq += sq;
      }
      __syncthreads();
    }
  }
  unsigned empty = 0;
  if (lead) {
    const long long o = (long long)(ONE ? i : i / A.bx) + (long long)A.nI * ((long long)J + (long long)A.nJ * K);
    if (A.measure) A.measure[o] = bm;
    if (A.first) A.first[o] = bt;
    if (A.second) A.second[o] = bq;
    empty = bm == 0.0 ? 1u : 0u;
  }
  // the counts: whole waves run (the block is a multiple of 64 lanes, nobody has returned)
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    points += __shfl_down(points, off, 64);
    nonfinite += __shfl_down(nonfinite, off, 64);
    empty += __shfl_down(empty, off, 64);
  }
  if ((t & 63) == 0) {
    const long long wg = (long long)blockIdx.x + (long long)gridDim.x * ((long long)blockIdx.y + (long long)gridDim.y * blockIdx.z);
    A.slots[wg * (BLK_THREADS / 64) + (t >> 6)] = {points, nonfinite, empty};
  }
}

// the record = the sum of the n slots; a few workgroups, each adds its sum to the record (zeroed in front of the launch)
__global__ __launch_bounds__(BLK_THREADS) void k_block_counts(const BlockSlot* __restrict__ slots, long long n, BlockCounts* out) {
  unsigned long long s[3] = {0, 0, 0};
  for (long long q = (long long)blockIdx.x * BLK_THREADS + threadIdx.x; q < n; q += (long long)gridDim.x * BLK_THREADS) {
    const BlockSlot c = slots[q];
    s[0] += c.points;
    s[1] += c.nonfinite;
    s[2] += c.empty_blocks;
  }
#pragma unroll
  for (int q = 0; q < 3; q++) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s[q] += __shfl_down(s[q], off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    if (s[0]) atomicAdd(&out->points, s[0]);
    if (s[1]) atomicAdd(&out->nonfinite, s[1]);
    if (s[2]) atomicAdd(&out->empty_blocks, s[2]);
  }
}

}  // namespace gb25
