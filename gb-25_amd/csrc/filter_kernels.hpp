// filter_kernels.hpp -- the moving-window filter (gb25_get_filter_sums, gb25_compute_filter_sums, gb25_get_derived_filter_sums:
// include/gb25.h): per level the window of (2 rx + 1) x (2 ry + 1) points around every sx-th column and sy-th row of the interior
// of a field, or of a packed derived field; per window sum w mu, sum w mu x and sum w mu x^2 in fp64 with mu THE MEASURE of
// gb25_integrate_field (measure_column, measure_level of diagnostics_kernels.hpp: the expression of k_block_sums) and w the
// product of the optional weights.  The filtered field, the eddy part, the variance below the filter scale.  Separable, two passes:
//
//   k_filter_x<T, LOC, WEIGHTED>  a workgroup takes one tile of FLT_TILE = 256 consecutive columns of one row j and one level K:
//                     grid = (ceil(Nx / 256), Ny, k_count).  It forms m, t, q of the tile's columns and of R = the row's rx
//                     columns on either side ONCE, into LDS (three planes of 256 + 2 x 32 doubles, 7.7 KB): loads coalesced along i,
//                     the periodic wrap by index (2 rx + 1 <= Nx: one conditional add), no halo of the parent is read.  After one
//                     barrier thread u takes the u-th column of the tile that is a multiple of sx and adds its 2 R + 1 LDS values
//                     in ascending d: s(I, j), stored to the scratch planes [Nx / sx, Ny, k_count].  A row that no y window
//                     contains (sy > 2 ry + 1) is read for its count alone.
//   k_filter_y<WEIGHTED>  one thread per output column I: grid = (ceil(nI / 256), Ny / sy, k_count).  It adds s of the rows
//                     j - ry .. j + ry that exist in ascending e; at a fixed e the loads of a wave are consecutive in I, so this pass
//                     needs no LDS.  It stores the planes that were asked for.
//
// Every sum starts from +0.0; a point that does not count is +0.0 in m, t and q.  fp64 with floating-point contraction OFF:
// t = mu * x, q = t * x, a weight times a term and every addition round by themselves (numpy restates them: gb-25_amd/filters.py).
// Plain vector stores, no floating-point atomics: the order of every sum is a function of the window alone, so the result is
// bitwise repeatable.  The counts are integers and go the way of the block sums': a wave adds its lanes' by the shuffle tree and
// lane 0 stores them to the wave's own BlockSlot -- k_filter_x the points with mu > 0 whose value is not finite (each source
// point once: the tile's own columns, not the wings), k_filter_y the outputs whose measure is 0 --, k_block_counts adds the
// slots.  Offsets into the source and into the planes are 64-bit.
#pragma once
#include "block_kernels.hpp"

namespace gb25 {

constexpr int FLT_TILE = 256;                            // columns of a tile of the x pass = threads of a workgroup (four waves)
constexpr int FLT_MAX_R = 32;                            // the largest radius (GB25_FILTER_MAX_RADIUS)
constexpr int FLT_SPAN = FLT_TILE + 2 * FLT_MAX_R;       // LDS columns of a plane

struct FilterArgs {
  int rx, ry, sx, sy;                   // radii and strides
  int k_first;                          // the window's first level, in the field's own level count
  int Nx, Ny;                           // the fine extents: columns, rows of cell centres
  int nI, nJ, nK;                       // the result's dims
  const double *wx, *wy;                // 2 rx + 1 and 2 ry + 1 weights; null: the box (WEIGHTED says which pass has them)
  const int* rx_of_row;                 // by row; null: rx for every row
  double* s[3];                         // the x pass's m, t, q: nI Ny nK each; null: the plane was not asked for (m always is)
  double* out[3];                       // measure, first, second: nI nJ nK each; null: not stored
  BlockSlot *slots_x, *slots_y;         // one per wave of each launch: 4 per workgroup, workgroups in x, y, z order
};

__device__ __forceinline__ void filter_store_counts(BlockSlot* slots, unsigned nonfinite, unsigned empty) {
  // whole waves run (the block is a multiple of 64 lanes, nobody has returned)
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    nonfinite += __shfl_down(nonfinite, off, 64);
    empty += __shfl_down(empty, off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    const long long wg = (long long)blockIdx.x + (long long)gridDim.x * ((long long)blockIdx.y + (long long)gridDim.y * blockIdx.z);
    slots[wg * (FLT_TILE / 64) + (threadIdx.x >> 6)] = {0u, nonfinite, empty};
  }
}

// box: bx = Nx; pitch, plane, origin of the array's element (0, 0, k_first), as for k_block_sums
template <class T, int LOC, bool WEIGHTED>
__global__ __launch_bounds__(FLT_TILE) void k_filter_x(Grid g, MomentsTables tab, const T* __restrict__ a, DiagBox box, FilterArgs A) {
#pragma clang fp contract(off)
  constexpr int HL = (LOC == LOC_FCC || LOC == LOC_FC) ? 1 : (LOC == LOC_CFC || LOC == LOC_CF) ? 2 : 0;
  __shared__ double lds[3 * FLT_SPAN];
  const int t = threadIdx.x;
  const int j = blockIdx.y, K = blockIdx.z;
  const int k = A.k_first + K;                                            // the level in the field
  const int tile0 = blockIdx.x * FLT_TILE;
  const int W = A.Nx - tile0 < FLT_TILE ? A.Nx - tile0 : FLT_TILE;        // the tile's own columns
  const int R = A.rx_of_row ? A.rx_of_row[j] : A.rx;                      // <= FLT_MAX_R and 2 R + 1 <= Nx (checked on the host)
  const bool wall = measure_wall_row<HL>(g, j);
  const T* row = a + (box.origin + box.pitch * j + box.plane * K);
  unsigned nonfinite = 0;
  for (int l = t; l < W + 2 * R; l += FLT_TILE) {                         // LDS column l holds fine column tile0 - R + l, wrapped
    int i = tile0 - R + l;
    i = i < 0 ? i + A.Nx : (i >= A.Nx ? i - A.Nx : i);
    double pm = 0.0, pt = 0.0, pq = 0.0;
    if (!wall) {
      const T e = row[i];
      const MeasureColumn mc = measure_column<HL>(g, tab, i, j);
      const double mu = measure_level<LOC>(g, mc, k);
      if (mu > 0.0) {
        const double x = (double)e;
        if (__builtin_isfinite(x)) {
          pm = mu;
          pt = mu * x;
          pq = pt * x;
        } else if (l >= R && l < R + W) {
          nonfinite++;
        }
      }
    }
    lds[l] = pm;
    lds[FLT_SPAN + l] = pt;
    lds[2 * FLT_SPAN + l] = pq;
  }
  __syncthreads();
  // is row j in the y window of an output row?  the nearest output rows are J0 sy <= j and (J0 + 1) sy
  const int J0 = j / A.sy;
  const bool needed = j - J0 * A.sy <= A.ry || (J0 + 1 < A.nJ && (J0 + 1) * A.sy - j <= A.ry);
  // the u-th output column of the tile: the multiples of sx in [tile0, tile0 + W)
  const long long I = (long long)((tile0 + A.sx - 1) / A.sx) + t;
  const long long i = I * A.sx;
  if (needed && i < tile0 + W) {
    const int base = (int)(i - tile0);                                     // LDS column of fine column i - R
    const long long o = I + (long long)A.nI * ((long long)j + (long long)A.Ny * K);
#pragma unroll
    for (int p = 0; p < 3; p++) {
      if (!A.s[p]) continue;
      const double* v = lds + p * FLT_SPAN + base;
      double s = 0.0;
      for (int d = 0; d <= 2 * R; d++) s += WEIGHTED ? A.wx[d] * v[d] : v[d];
      A.s[p][o] = s;
    }
  }
  filter_store_counts(A.slots_x, nonfinite, 0u);
}

template <bool WEIGHTED>
__global__ __launch_bounds__(FLT_TILE) void k_filter_y(FilterArgs A) {
#pragma clang fp contract(off)
  const long long I = (long long)blockIdx.x * FLT_TILE + threadIdx.x;
  const int J = blockIdx.y, K = blockIdx.z;
  const int j = J * A.sy;
  const int e0 = -A.ry > -j ? -A.ry : -j;                                   // rows outside 0 .. Ny - 1 are skipped
  const int e1 = A.ry < A.Ny - 1 - j ? A.ry : A.Ny - 1 - j;
  unsigned empty = 0;
  if (I < A.nI) {
    const long long o = I + (long long)A.nI * ((long long)J + (long long)A.nJ * K);
#pragma unroll
    for (int p = 0; p < 3; p++) {
      if (!A.s[p]) continue;
      const double* s = A.s[p] + (I + (long long)A.nI * ((long long)A.Ny * K));
      double b = 0.0;
      for (int e = e0; e <= e1; e++) {
        const double v = s[(long long)A.nI * (j + e)];
        b += WEIGHTED ? A.wy[e + A.ry] * v : v;
      }
      if (A.out[p]) A.out[p][o] = b;
      if (p == 0) empty = b == 0.0 ? 1u : 0u;
    }
  }
  filter_store_counts(A.slots_y, 0u, empty);
}

}  // namespace gb25
