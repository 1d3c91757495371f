// zonal_eddy_kernels.hpp -- zonal-mean and eddy statistics (gb25_get_zonal_eddy, include/gb25.h): for every interior line (row j,
// level k, along i) the measure-weighted first moments of six variables brought to the cell centre -- U, V, W, T, S and the
// potential density -- and the 21 comoments of their deviations from the line's mean.  Included by gb25_api.hip, launched from
// zonal_eddy_host.hpp.
//
//   k_zonal_eddy<CURV, IMM>  ONE WAVE takes ONE LINE (j, kk), four lines per block.  The line is cut into chunks of four cells
//                     exactly as k_field_moments cuts a row of T (aligned to 16 / 32 bytes in MEMORY, diag_misalignment of the row of
//                     T); a lane takes every 64th chunk and adds in the order of its cells, the lanes are combined by the fixed
//                     shuffle tree of diag_wave_reduce (lane l <- lane l + lane l + off, off = 1, 2, ... 32), every sum starts from
//                     +0.0 and a cell that does not count adds nothing: no atomics, bitwise repeatable, and `measure` and `points`
//                     ARE the ROWS record of gb25_integrate_field(GB25_T).
//                     Pass 1: measure, first[6], points, nonfinite.  Every lane then holds lane 0's sums and forms mean[q] = first[q]
//                     / measure with one IEEE division (+0.0 for an empty line), or takes the caller's.  Pass 2 walks the line again
//                     -- the five fields of the line were just read by this wave: the second read is served by the caches -- and adds
//                     co[p, q] += (mu d_p) d_q, d_q = x_q - mean[q].  The equation of state is evaluated once per cell and pass.
//                     CURV: the areas come from diagnostics' 2-D table, else from the row table; IMM: the first wet level of every
//                     column comes from diagnostics' table, else every level is wet.  Both through measure_column / measure_level,
//                     THE MEASURE of diagnostics_kernels.hpp.
// Arithmetic: fp64 on (double) of the stored values with floating-point contraction OFF (every product, sum and difference rounds by
// itself); the potential density is derived_density_value rounded to `real`, the bits gb25_get_derived hands out (the pragma is
// lexical: the density lives in its own function).  numpy restates the records bit for bit (gb-25_amd/eddies.py).  Plain vector
// loads and stores, no LDS, every offset into a 3-D array 64-bit.  Reads: the interior of the line, u one column beyond it (the x
// halo), v one row beyond it, w one level above it -- the reach of k_stability_faces.
#pragma once

namespace gb25 {

constexpr int ZE_VARS = 6;    // U, V, W, T, S, SIGMA
constexpr int ZE_CO = 21;     // p <= q, row-major over (p, q)

struct ZonalEddyRecord {   // = gb25_zonal_eddy_row
  double measure, first[ZE_VARS], mean[ZE_VARS], co[ZE_CO];
  long long points, nonfinite;
};
struct ZonalEddyIn {
  const real *u, *v, *w, *T, *S;   // parents
  const double* eos0;              // the TEOS-10 table folded at Z = 0
  const double* means;             // null, or [k_count][by][ZE_VARS]: the means the deviations are taken about
  int by, k_first, k_count;
};

// lane 0 ends with the sum of the wave in the association of diag_wave_reduce
__device__ __forceinline__ double ze_wave_sum(double x) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) x = x + __shfl_down(x, off, 64);
  return x;
}
__device__ __forceinline__ long long ze_wave_count(long long n) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) n += __shfl_down(n, off, 64);
  return n;
}

// The rows a line reads and how it is cut (wave-uniform)
struct ZeLine {
  const real *T, *S, *U, *V, *V1, *W, *W1;
  int mis, nchunks;
};
__device__ __forceinline__ ZeLine ze_line(const Grid& g, const ZonalEddyIn& in, int j, int k) {
  const long long oc = der_off(g, g.pl_c, 0, j, k), ov = der_off(g, g.pl_v, 0, j, k);
  ZeLine L;
  L.T = in.T + oc;
  L.S = in.S + oc;
  L.U = in.u + oc;
  L.W = in.w + oc;
  L.W1 = L.W + g.pl_c;
  L.V = in.v + ov;
  L.V1 = L.V + g.sx;
  L.mis = diag_misalignment(L.T);
  L.nchunks = (L.mis + g.Nx + 3) >> 2;
  return L;
}
// what a chunk of four cells reads: cells [x0, x0 + 4) of which [0, Nx) exist; u one face further (the halo column behind cell Nx - 1)
struct ZeChunk {
  real T[4], S[4], U[5], V[4], V1[4], W[4], W1[4];
};
__device__ __forceinline__ void ze_load(const ZeLine& L, int x0, int bx, ZeChunk& e) {
  diag_load4(L.T, x0, bx, e.T);
  diag_load4(L.S, x0, bx, e.S);
  diag_load4(L.U, x0, bx + 1, e.U);
  e.U[4] = x0 + 4 <= bx ? L.U[x0 + 4] : real(0);
  diag_load4(L.V, x0, bx, e.V);
  diag_load4(L.V1, x0, bx, e.V1);
  diag_load4(L.W, x0, bx, e.W);
  diag_load4(L.W1, x0, bx, e.W1);
}
// cell s of the chunk: 0 = it does not exist or mu is not > 0, 1 = it counts (mu and the six values), 2 = wet with a value that is
// not finite
enum { ZE_NONE = 0, ZE_COUNTS = 1, ZE_SKIPPED = 2 };
__device__ __forceinline__ int ze_cell(const Grid& g, const MomentsTables& tab, const double* __restrict__ eos0, const ZeChunk& e, int x0,
                                       int s, int j, int k, double& mu, double v[ZE_VARS]) {
#pragma clang fp contract(off)
  const int x = x0 + s;
  if (x < 0 || x >= g.Nx) return ZE_NONE;
  mu = measure_level<LOC_CCC>(g, measure_column<0>(g, tab, x, j), k);
  if (!(mu > 0.0)) return ZE_NONE;
  v[0] = 0.5 * ((double)e.U[s] + (double)e.U[s + 1]);
  v[1] = 0.5 * ((double)e.V[s] + (double)e.V1[s]);
  v[2] = 0.5 * ((double)e.W[s] + (double)e.W1[s]);
  v[3] = (double)e.T[s];
  v[4] = (double)e.S[s];
  v[5] = (double)(real)derived_density_value(eos0, e.T[s], e.S[s]);
  bool finite = true;
#pragma unroll
  for (int q = 0; q < ZE_VARS; q++) finite = finite && __builtin_isfinite(v[q]);
  return finite ? ZE_COUNTS : ZE_SKIPPED;
}

template <bool CURV, bool IMM>
__global__ __launch_bounds__(DIAG_THREADS) void k_zonal_eddy(Grid g, MomentsTables tab_in, ZonalEddyIn in, ZonalEddyRecord* __restrict__ out) {
#pragma clang fp contract(off)
  const long long r = (long long)blockIdx.x * (DIAG_THREADS / 64) + (threadIdx.x >> 6);
  if (r >= (long long)in.by * in.k_count) return;   // (the whole wave)
  const int lane = threadIdx.x & 63;
  const int kk = __builtin_amdgcn_readfirstlane((int)(r / in.by)), j = __builtin_amdgcn_readfirstlane((int)(r - (long long)kk * in.by));
  const int k = in.k_first + kk, bx = g.Nx;
  MomentsTables tab = tab_in;
  if (!CURV) tab.area[0] = nullptr;
  if (!IMM) tab.first[0] = nullptr;
  const ZeLine L = ze_line(g, in, j, k);

  // pass 1
  double measure = 0.0, first[ZE_VARS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  long long points = 0, nonfinite = 0;
  for (int c = lane; c < L.nchunks; c += 64) {
    const int x0 = 4 * c - L.mis;
    ZeChunk e;
    ze_load(L, x0, bx, e);
#pragma unroll
    for (int s = 0; s < 4; s++) {
      double mu, v[ZE_VARS];
      const int what = ze_cell(g, tab, in.eos0, e, x0, s, j, k, mu, v);
      nonfinite += what == ZE_SKIPPED ? 1 : 0;
      if (what != ZE_COUNTS) continue;
      measure = measure + mu;
#pragma unroll
      for (int q = 0; q < ZE_VARS; q++) {
        const double t = mu * v[q];
        first[q] = first[q] + t;
      }
      points++;
    }
  }
  measure = ze_wave_sum(measure);
  points = ze_wave_count(points);
  nonfinite = ze_wave_count(nonfinite);
#pragma unroll
  for (int q = 0; q < ZE_VARS; q++) first[q] = ze_wave_sum(first[q]);

  // the means, the same bits in every lane
  double mean[ZE_VARS];
  const double m0 = __shfl(measure, 0, 64);
#pragma unroll
  for (int q = 0; q < ZE_VARS; q++) {
    const double f0 = __shfl(first[q], 0, 64);
    mean[q] = in.means ? in.means[r * ZE_VARS + q] : (m0 == 0.0 ? 0.0 : f0 / m0);
  }

  // pass 2
  double co[ZE_CO];
#pragma unroll
  for (int n = 0; n < ZE_CO; n++) co[n] = 0.0;
  for (int c = lane; c < L.nchunks; c += 64) {
    const int x0 = 4 * c - L.mis;
    ZeChunk e;
    ze_load(L, x0, bx, e);
#pragma unroll
    for (int s = 0; s < 4; s++) {
      double mu, v[ZE_VARS], d[ZE_VARS];
      if (ze_cell(g, tab, in.eos0, e, x0, s, j, k, mu, v) != ZE_COUNTS) continue;
#pragma unroll
      for (int q = 0; q < ZE_VARS; q++) d[q] = v[q] - mean[q];
#pragma unroll
      for (int p = 0; p < ZE_VARS; p++) {
        const double t = mu * d[p];
#pragma unroll
        for (int q = p; q < ZE_VARS; q++) {
          const double x = t * d[q];
          co[p * (11 - p) / 2 + q] = co[p * (11 - p) / 2 + q] + x;
        }
      }
    }
  }
#pragma unroll
  for (int n = 0; n < ZE_CO; n++) co[n] = ze_wave_sum(co[n]);

  if (lane == 0) {
    ZonalEddyRecord* o = out + r;
    o->measure = measure;
#pragma unroll
    for (int q = 0; q < ZE_VARS; q++) {
      o->first[q] = first[q];
      o->mean[q] = mean[q];
    }
#pragma unroll
    for (int n = 0; n < ZE_CO; n++) o->co[n] = co[n];
    o->points = points;
    o->nonfinite = nonfinite;
  }
}

}  // namespace gb25
