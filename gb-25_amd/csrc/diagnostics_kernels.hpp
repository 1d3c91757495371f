// diagnostics_kernels.hpp -- reductions over the model's fields where the fields live (gb25_get_field_stats,
// gb25_compare_field, gb25_get_state_monitor: include/gb25.h).  Three streaming reads and one tiny second launch:
//
//   k_field_stats     one pass over a box of a field's parent array: min, max, max|x| and where, sum x, sum x^2 (fp64), the
//                     number of non-finite values and where the first one is.  4 (Float32) / 8 (Float64) bytes per element.
//   k_field_diff      the same pass over two arrays a, b (b: float or double, dims of its own, an origin of its own):
//                     max|a|, max|b|, sum a^2, sum b^2, d = a - b in fp64, max|d| and where, sum d^2.  sizeof a + sizeof b.
//   k_advective_cfl   over the interior cells max of |u|/dx(u point) + |v|/dy(v point) + |w|/dz(w face) in fp64, IEEE
//                     divisions, the three values at the same index (i, j, k), summed left to right.  The metrics are the
//                     numbers gb25_get_metric / gb25_get_metric2 return:
//                       LatitudeLongitudeGrid:  dx = GB25_M_DXC(j),  dy = GB25_M_DY,        dz = GB25_M_DZF(k)
//                       curvilinear grids:      dx = GB25_M2_DXFC,   dy = GB25_M2_DYCF,     dz = GB25_M_DZF(k)
//                     12 / 24 bytes per cell.
//   k_diag_finish<P>  combines the per-block records of any of the three in a fixed order.
//
// Bitwise repeatable, whatever the order in which blocks run: the assignment of elements to lanes is a function of the box
// alone (a block = DIAG_ROWS rows of the box, a wave = every fourth of them, a lane = every 64th chunk of four elements of a
// row), a lane accumulates in the order of its elements, lanes are combined by a fixed shuffle tree, the four waves through LDS
// in wave order, the blocks' records (plain vector stores into the model's scratch buffer) by one block of the second launch in
// the same manner.  No atomics.  Extrema do not depend on any order; ties in a position go to the smallest linear offset in
// memory order (i fastest), Julia's findmax.  Offsets are 64-bit.
//
// Loads: a row is cut into chunks of four elements aligned to 4 sizeof(T) in MEMORY (the interior of a row starts H elements
// into a row of Nx + 2H: whatever that does to the alignment, the body of a row goes through one 16-byte (Float32) or two
// 16-byte (Float64) loads per lane and only the cut chunks at its two ends through element loads).  Nothing outside the box
// is read.
#pragma once
#include "device_common.hpp"

namespace gb25 {

constexpr int DIAG_THREADS = 256;   // four waves
constexpr int DIAG_ROWS = 16;       // rows of the box per block
constexpr long long DIAG_NONE = 0x7fffffffffffffffLL;

// a box of an array: extent, the array's pitches, the box's first element
struct DiagBox {
  int bx, by, bz;
  long long pitch, plane, origin;
};

struct StatsPartial {
  double mn, mx, amax, sum, sumsq;
  long long at, nonfinite, first;
};
struct DiffPartial {
  double amax_a, amax_b, amax_d, ss_a, ss_b, ss_d;
  long long at, nonfinite;
};
struct CflPartial {
  double cfl;
  long long at;
};

__device__ __forceinline__ StatsPartial diag_identity(const StatsPartial*) {
  return {__builtin_inf(), -__builtin_inf(), -1.0, 0.0, 0.0, DIAG_NONE, 0, DIAG_NONE};
}
__device__ __forceinline__ DiffPartial diag_identity(const DiffPartial*) { return {-1.0, -1.0, -1.0, 0.0, 0.0, 0.0, DIAG_NONE, 0}; }
__device__ __forceinline__ CflPartial diag_identity(const CflPartial*) { return {-1.0, DIAG_NONE}; }

// larger value wins; equal values: the smaller offset
__device__ __forceinline__ void diag_take_max(double& best, long long& at, double v, long long o) {
  const bool take = v > best || (v == best && o < at);
  best = take ? v : best;
  at = take ? o : at;
}
// a (the earlier in the fixed order) combined with b
__device__ __forceinline__ StatsPartial diag_combine(StatsPartial a, const StatsPartial& b) {
  a.mn = __builtin_fmin(a.mn, b.mn);
  a.mx = __builtin_fmax(a.mx, b.mx);
  diag_take_max(a.amax, a.at, b.amax, b.at);
  a.sum += b.sum;
  a.sumsq += b.sumsq;
  a.nonfinite += b.nonfinite;
  a.first = b.first < a.first ? b.first : a.first;
  return a;
}
__device__ __forceinline__ DiffPartial diag_combine(DiffPartial a, const DiffPartial& b) {
  a.amax_a = __builtin_fmax(a.amax_a, b.amax_a);
  a.amax_b = __builtin_fmax(a.amax_b, b.amax_b);
  diag_take_max(a.amax_d, a.at, b.amax_d, b.at);
  a.ss_a += b.ss_a;
  a.ss_b += b.ss_b;
  a.ss_d += b.ss_d;
  a.nonfinite += b.nonfinite;
  return a;
}
__device__ __forceinline__ CflPartial diag_combine(CflPartial a, const CflPartial& b) {
  diag_take_max(a.cfl, a.at, b.cfl, b.at);
  return a;
}

// lane l <- combine(lane l, lane l + off), off = 1, 2, ... 32: lane 0 ends with the whole wave in a fixed association
template <class P>
__device__ __forceinline__ P diag_wave_reduce(P p) {
  constexpr int W = sizeof(P) / sizeof(int);
  static_assert(sizeof(P) % sizeof(int) == 0, "records are whole dwords");
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    int w[W];
    __builtin_memcpy(w, &p, sizeof(P));
#pragma unroll
    for (int q = 0; q < W; q++) w[q] = __shfl_down(w[q], off, 64);
    P o;
    __builtin_memcpy(&o, w, sizeof(P));
    p = diag_combine(p, o);
  }
  return p;
}
// the block's record, in thread 0
template <class P>
__device__ __forceinline__ P diag_block_reduce(P p) {
  __shared__ P lds[DIAG_THREADS / 64];
  p = diag_wave_reduce(p);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) lds[wave] = p;
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < DIAG_THREADS / 64; w++) p = diag_combine(p, lds[w]);
  return p;
}

// Four elements of a row: in-row positions [x0, x0 + 4), of which [0, bx) exist.  `row` points at position 0.  A chunk that
// lies inside the row and is aligned in memory is one vector load; any other is element loads of what exists (0 elsewhere).
template <class T>
__device__ __forceinline__ void diag_load4(const T* row, int x0, int bx, T out[4]) {
  using V4 = T __attribute__((ext_vector_type(4)));
  const T* p = row + x0;
  if (x0 >= 0 && x0 + 4 <= bx && ((unsigned long long)p & (4 * sizeof(T) - 1)) == 0) {
    const V4 v = *reinterpret_cast<const V4*>(p);
    out[0] = v.x; out[1] = v.y; out[2] = v.z; out[3] = v.w;
  } else {
#pragma unroll
    for (int s = 0; s < 4; s++) out[s] = (x0 + s >= 0 && x0 + s < bx) ? p[s] : T(0);
  }
}
// how many elements the row's first element lies beyond a 4 sizeof(T) boundary
template <class T>
__device__ __forceinline__ int diag_misalignment(const T* row) {
  return (int)(((unsigned long long)row / sizeof(T)) & 3);
}

// The rows of a block: row r of the box is (j, k) = (r % by, r / by); the wave takes every fourth row of the block's DIAG_ROWS,
// a lane every 64th chunk of the row.  body(row offset into the array, box offset of the row's first element, j, k).
template <class Body>
__device__ __forceinline__ void diag_for_rows(const DiagBox& box, Body body) {
  const long long rows = (long long)box.by * box.bz;
  const long long r0 = (long long)blockIdx.x * DIAG_ROWS;
  const int wave = threadIdx.x >> 6;
  for (int q = wave; q < DIAG_ROWS; q += DIAG_THREADS / 64) {
    const long long r = r0 + q;
    if (r >= rows) break;
    const int k = (int)(r / box.by), j = (int)(r - (long long)k * box.by);
    body(box.origin + box.pitch * j + box.plane * k, r * box.bx, j, k);
  }
}

template <class T>
__global__ __launch_bounds__(DIAG_THREADS) void k_field_stats(const T* __restrict__ a, DiagBox box, StatsPartial* __restrict__ partials) {
  StatsPartial p = diag_identity((StatsPartial*)nullptr);
  const int lane = threadIdx.x & 63;
  diag_for_rows(box, [&](long long row_off, long long box_off, int, int) {
    const T* row = a + row_off;
    const int mis = diag_misalignment(row), nchunks = (mis + box.bx + 3) >> 2;
    for (int c = lane; c < nchunks; c += 64) {
      const int x0 = 4 * c - mis;
      T e[4];
      diag_load4(row, x0, box.bx, e);
#pragma unroll
      for (int s = 0; s < 4; s++) {
        const int x = x0 + s;
        if (x < 0 || x >= box.bx) continue;
        const double v = (double)e[s];
        const long long o = box_off + x;
        if (__builtin_isfinite(v)) {
          p.mn = __builtin_fmin(p.mn, v);
          p.mx = __builtin_fmax(p.mx, v);
          diag_take_max(p.amax, p.at, __builtin_fabs(v), o);
          p.sum += v;
          p.sumsq = __builtin_fma(v, v, p.sumsq);
        } else {
          p.nonfinite++;
          p.first = o < p.first ? o : p.first;
        }
      }
    }
  });
  p = diag_block_reduce(p);
  if (threadIdx.x == 0) partials[blockIdx.x] = p;
}

// a: box `box` of the model's field; b: the box of the same extent of another array (pitches and first element in bbox)
template <class TA, class TB>
__global__ __launch_bounds__(DIAG_THREADS) void k_field_diff(const TA* __restrict__ a, DiagBox box, const TB* __restrict__ b, DiagBox bbox,
                                                             DiffPartial* __restrict__ partials) {
  DiffPartial p = diag_identity((DiffPartial*)nullptr);
  const int lane = threadIdx.x & 63;
  diag_for_rows(box, [&](long long row_off, long long box_off, int j, int k) {
    const TA* row = a + row_off;
    const TB* rowb = b + (bbox.origin + bbox.pitch * j + bbox.plane * k);
    const int mis = diag_misalignment(row), nchunks = (mis + box.bx + 3) >> 2;
    for (int c = lane; c < nchunks; c += 64) {
      const int x0 = 4 * c - mis;
      TA ea[4];
      TB eb[4];
      diag_load4(row, x0, box.bx, ea);
      diag_load4(rowb, x0, box.bx, eb);   // (chunks cut like a's: a vector load where b happens to be aligned as well)
#pragma unroll
      for (int s = 0; s < 4; s++) {
        const int x = x0 + s;
        if (x < 0 || x >= box.bx) continue;
        const double va = (double)ea[s], vb = (double)eb[s], d = va - vb;
        const bool fa = __builtin_isfinite(va), fb = __builtin_isfinite(vb);
        if (fa) {
          p.amax_a = __builtin_fmax(p.amax_a, __builtin_fabs(va));
          p.ss_a = __builtin_fma(va, va, p.ss_a);
        }
        if (fb) {
          p.amax_b = __builtin_fmax(p.amax_b, __builtin_fabs(vb));
          p.ss_b = __builtin_fma(vb, vb, p.ss_b);
        }
        if (fa && fb && __builtin_isfinite(d)) {
          diag_take_max(p.amax_d, p.at, __builtin_fabs(d), box_off + x);
          p.ss_d = __builtin_fma(d, d, p.ss_d);
        } else {
          p.nonfinite++;
        }
      }
    }
  });
  p = diag_block_reduce(p);
  if (threadIdx.x == 0) partials[blockIdx.x] = p;
}

// box: the interior of u (w has the same pitches; v the plane g.pl_v)
__global__ __launch_bounds__(DIAG_THREADS) void k_advective_cfl(Grid g, const real* __restrict__ u, const real* __restrict__ v,
                                                                const real* __restrict__ w, DiagBox box, CflPartial* __restrict__ partials) {
  CflPartial p = diag_identity((CflPartial*)nullptr);
  const int lane = threadIdx.x & 63;
  diag_for_rows(box, [&](long long row_off, long long box_off, int j, int k) {
    const real *ru = u + row_off, *rw = w + row_off;
    const real* rv = v + (box.origin + box.pitch * j + (long long)g.pl_v * k + ((long long)g.pl_v - g.pl_c) * g.H);
    const real *rdx = nullptr, *rdy = nullptr;
    double dx = 0, dy = (double)g.dy;
    if (g.cv.on) {
      rdx = g.cv.dxfc + i2(g, 0, j);
      rdy = g.cv.dycf + i2(g, 0, j);
    } else {
      dx = (double)g.dxc[j];
    }
    const double dz = (double)g.dzf[k];
    const int mis = diag_misalignment(ru), nchunks = (mis + box.bx + 3) >> 2;
    for (int c = lane; c < nchunks; c += 64) {
      const int x0 = 4 * c - mis;
      real eu[4], ev[4], ew[4], ex[4], ey[4];
      diag_load4(ru, x0, box.bx, eu);
      diag_load4(rv, x0, box.bx, ev);
      diag_load4(rw, x0, box.bx, ew);
      if (g.cv.on) {
        diag_load4(rdx, x0, box.bx, ex);
        diag_load4(rdy, x0, box.bx, ey);
      }
#pragma unroll
      for (int s = 0; s < 4; s++) {
        const int x = x0 + s;
        if (x < 0 || x >= box.bx) continue;
        if (g.cv.on) {
          dx = (double)ex[s];
          dy = (double)ey[s];
        }
        const double c3 = (__builtin_fabs((double)eu[s]) / dx + __builtin_fabs((double)ev[s]) / dy) + __builtin_fabs((double)ew[s]) / dz;
        if (__builtin_isfinite(c3)) diag_take_max(p.cfl, p.at, c3, box_off + x);
      }
    }
  });
  p = diag_block_reduce(p);
  if (threadIdx.x == 0) partials[blockIdx.x] = p;
}

// ---- integrals (gb25_integrate_field, gb25_get_budget): sums weighted by the measure mu = A dz fold wet of include/gb25.h.
//   k_field_moments<T, LOC>  one pass over the interior box of a field at location LOC: ONE WAVE takes ONE ROW (j, k); a lane takes
//                     every 64th chunk of four elements (diag_load4, cut like k_field_stats' chunks) and accumulates sum mu,
//                     sum mu x, sum mu x^2 in fp64 in the order of its elements; the fixed shuffle tree combines the lanes and
//                     lane 0 stores the row's record (plain vector stores): rows[j + by k].  The area comes from the row tables
//                     of the LatitudeLongitudeGrid (one number per row) or from a 2-D table of diagnostics' own (curvilinear
//                     grids), the first wet level per column and location from a 2-D table of 16-bit numbers of diagnostics' own
//                     (none on a grid without a bottom); all of them in the parent layout of a (c,f) field, so that a row of a
//                     table is cut into the same chunks as the row of the field.  4 / 8 bytes per element plus the tables.
//   k_moments_fold    one wave per level: the level's row records, 64 at a time through LDS, added by lane 0 LEFT TO RIGHT in j;
//                     launched a second time over the levels it adds them left to right in k: the total.
enum MomentLoc { LOC_CCC = 0, LOC_FCC, LOC_CFC, LOC_CCF, LOC_CC, LOC_FC, LOC_CF };
constexpr unsigned short MOMENTS_DRY = 0xffff;   // first wet level of a column that has none
constexpr int MOMENTS_SLOTS = 5;                  // fields a budget reduces before one fold

struct MomentsPartial {   // = gb25_moments
  double measure, first, second;
  long long points, nonfinite;
};
__device__ __forceinline__ MomentsPartial diag_combine(MomentsPartial a, const MomentsPartial& b) {
  a.measure += b.measure;
  a.first += b.first;
  a.second += b.second;
  a.points += b.points;
  a.nonfinite += b.nonfinite;
  return a;
}
// diagnostics' own tables, by horizontal location (c,c), (f,c), (c,f): parent layout of a (c,f) field (pitch g.sx, row j + H)
struct MomentsTables {
  const real* area[3];              // null: the row tables of the LatitudeLongitudeGrid
  const unsigned short* first[3];   // first wet level of the column (MOMENTS_DRY: none); null: every level of every column is wet
  int pivot_row;                    // local row of the GLOBAL pivot row of a folded grid on this rank, else -1
};

// THE MEASURE point by point, for the kernels that keep it apart from the value (k_block_sums, k_filter_x: ONE expression, so
// that their planes agree bit for bit): the part of a column -- its area, its first wet level, the pivot row's 1/2 --, then the
// level's.  HL: the horizontal location of the tables, 0 (c,c), 1 (f,c), 2 (c,f).  Pure products: nothing here can contract.
struct MeasureColumn {
  double area, fold;
  int first_wet;
};
template <int HL>
__device__ __forceinline__ bool measure_wall_row(const Grid& g, int j) {   // (a y face on a wall of the GLOBAL grid: mu = 0)
  return HL == 2 && (j == g.jws || (j == g.jwn && !g.cv.north_fold));
}
template <int HL>
__device__ __forceinline__ MeasureColumn measure_column(const Grid& g, const MomentsTables& tab, int i, int j) {
  const int o2 = i2(g, i, j);
  MeasureColumn c;
  c.fold = (HL != 2 && j == tab.pivot_row) ? 0.5 : 1.0;
  c.area = tab.area[HL] ? (double)tab.area[HL][o2] : (double)(HL == 2 ? g.azf[j] : g.azc[j]);
  c.first_wet = tab.first[HL] ? (int)tab.first[HL][o2] : 0;
  return c;
}
// k: the level in the field's own count, wave-uniform
template <int LOC>
__device__ __forceinline__ double measure_level(const Grid& g, const MeasureColumn& c, int k) {
  constexpr bool FLAT = LOC >= LOC_CC;
  const double dz = FLAT ? 1.0 : (double)uniform_at(LOC == LOC_CCF ? g.dzf : g.dzc, k);
  const int level = FLAT ? g.Nz - 1 : k;   // wet: level >= the column's first wet level
  return level < c.first_wet ? 0.0 : (c.area * dz) * c.fold;
}

template <class T, int LOC>
__global__ __launch_bounds__(DIAG_THREADS) void k_field_moments(Grid g, MomentsTables tab, const T* __restrict__ a, DiagBox box,
                                                                MomentsPartial* __restrict__ rows) {
  constexpr int HL = (LOC == LOC_FCC || LOC == LOC_FC) ? 1 : (LOC == LOC_CFC || LOC == LOC_CF) ? 2 : 0;
  constexpr bool FLAT = LOC >= LOC_CC;
  const long long r = (long long)blockIdx.x * (DIAG_THREADS / 64) + (threadIdx.x >> 6);
  if (r >= (long long)box.by * box.bz) return;
  const int lane = threadIdx.x & 63;
  const int k = (int)(r / box.by), j = (int)(r - (long long)k * box.by);
  MomentsPartial p = {0.0, 0.0, 0.0, 0, 0};
  const bool wall = HL == 2 && (j == g.jws || (j == g.jwn && !g.cv.north_fold));   // (a y face on a wall of the GLOBAL grid)
  if (!wall) {
    const T* row = a + (box.origin + box.pitch * j + box.plane * k);
    const double dz = FLAT ? 1.0 : (double)(LOC == LOC_CCF ? g.dzf[k] : g.dzc[k]);
    const double fold = (HL != 2 && j == tab.pivot_row) ? 0.5 : 1.0;
    const int level = FLAT ? g.Nz - 1 : k;   // wet: level >= the column's first wet level
    const real* ra = tab.area[HL] ? tab.area[HL] + i2(g, 0, j) : nullptr;
    const unsigned short* rf = tab.first[HL] ? tab.first[HL] + i2(g, 0, j) : nullptr;
    const double mu_row = ra ? 0.0 : ((double)(HL == 2 ? g.azf[j] : g.azc[j]) * dz) * fold;
    const int mis = diag_misalignment(row), nchunks = (mis + box.bx + 3) >> 2;
    for (int c = lane; c < nchunks; c += 64) {
      const int x0 = 4 * c - mis;
      T e[4];
      real ea[4];
      unsigned short ef[4];
      diag_load4(row, x0, box.bx, e);
      if (ra) diag_load4(ra, x0, box.bx, ea);
      if (rf) diag_load4(rf, x0, box.bx, ef);
#pragma unroll
      for (int s = 0; s < 4; s++) {
        const int x = x0 + s;
        if (x < 0 || x >= box.bx) continue;
        const double mu = (rf && level < (int)ef[s]) ? 0.0 : (ra ? ((double)ea[s] * dz) * fold : mu_row);
        if (!(mu > 0.0)) continue;
        const double v = (double)e[s];
        if (__builtin_isfinite(v)) {
          const double t = mu * v;
          p.measure += mu;
          p.first += t;
          p.second = __builtin_fma(t, v, p.second);
          p.points++;
        } else {
          p.nonfinite++;
        }
      }
    }
    p = diag_wave_reduce(p);
  }
  if (lane == 0) rows[r] = p;
}

// slot s (blockIdx.y) holds n[s] groups (blockIdx.x) of len[s] records each, group q at in + in_stride s + len[s] q; its sum,
// left to right, goes to out[out_stride s + q].  One wave per group.
struct MomentsFold {
  int len[MOMENTS_SLOTS], n[MOMENTS_SLOTS];
};
__global__ __launch_bounds__(64) void k_moments_fold(const MomentsPartial* __restrict__ in, long long in_stride, MomentsFold f,
                                                     MomentsPartial* __restrict__ out, long long out_stride) {
  __shared__ MomentsPartial lds[64];
  const int s = blockIdx.y, q = blockIdx.x, lane = threadIdx.x;
  if (q >= f.n[s]) return;   // (uniform for the block)
  const int len = f.len[s];
  const MomentsPartial* src = in + in_stride * s + (long long)len * q;
  MomentsPartial p = {0.0, 0.0, 0.0, 0, 0};
  for (int base = 0; base < len; base += 64) {
    if (base + lane < len) lds[lane] = src[base + lane];
    __syncthreads();
    if (lane == 0) {
      const int m = len - base < 64 ? len - base : 64;
      for (int t = 0; t < m; t++) p = diag_combine(p, lds[t]);
    }
    __syncthreads();
  }
  if (lane == 0) out[out_stride * s + q] = p;
}

// one block: the records of the first launch in index order -- thread t takes t, t + 256, ... --, then the block's tree
template <class P>
__global__ __launch_bounds__(DIAG_THREADS) void k_diag_finish(const P* __restrict__ partials, int n, P* __restrict__ out) {
  P p = diag_identity((P*)nullptr);
  for (int q = threadIdx.x; q < n; q += DIAG_THREADS) p = diag_combine(p, partials[q]);
  p = diag_block_reduce(p);
  if (threadIdx.x == 0) *out = p;
}

// ---- derived fields (gb25_compute_derived, gb25_get_derived, gb25_get_derived_stats, gb25_get_field_levels): relative vorticity,
// kinetic energy per cell, in-situ and potential density, mixed-layer depth, and a gather of levels of an ordinary field.
// Definitions: include/gb25.h.  Common shape: a block is 64 x 4 threads, ONE WAVE = 64 consecutive i of one row j (u, v, T, S and
// the 2-D metrics load coalesced), and marches DER_LEVELS levels, so that the 2-D metrics, the first wet level and the row tables
// are loaded once per block; the row and level tables (dxc, azf, the 28 coefficients of a level) are wave-uniform and go through
// scalar loads.  The result is PACKED: out[i + bx (j + by kk)], kk = 0 .. k_count - 1 for level k_first + kk, so that only the
// requested levels are computed, stored and copied.  Plain vector stores, no atomics, every offset into a 3-D array 64-bit.
// Vorticity, kinetic energy and the mixed-layer depth are fp64 on (double) of the stored values with floating-point contraction
// OFF (every product and sum rounds by itself, divisions are IEEE), rounded once to the float type: numpy restates them bit for
// bit (gb-25_amd/derived.py).  The densities are teos10_level on s, t formed as k_compute_p forms them, compiled like it.
constexpr int DER_LEVELS = 4;
struct DerivedOut {
  real* out;
  int bx, by, k_first, k_count;
};
__device__ __forceinline__ long long der_off(const Grid& g, int plane, int i, int j, int k) {
  return (long long)(i + g.H) + (long long)g.sx * (j + g.H) + (long long)plane * (k + g.H);
}
__device__ __forceinline__ long long der_out(const DerivedOut& d, int i, int j, int kk) {
  return (long long)i + (long long)d.bx * ((long long)j + (long long)d.by * kk);
}

// zeta(i,j,k) = ((dy v(i,j) - dy' v(i-1,j)) - (dx u(i,j) - dx' u(i,j-1))) / Az at (f,f,c); box = the interior of v.
// CURV: dy = DYCF(i,j), dy' = DYCF(i-1,j), dx = DXFC(i,j), dx' = DXFC(i,j-1), Az = AZFF(i,j) (azff: diagnostics' own table);
// else dy = dy' = GB25_M_DY, dx = DXC(j), dx' = DXC(j-1), Az = AZF(j).  Az == 0 gives 0.
template <bool CURV>
__global__ __launch_bounds__(256) void k_derived_vorticity(Grid g, const real* __restrict__ u, const real* __restrict__ v,
                                                            const real* __restrict__ azff, DerivedOut d) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 64 + threadIdx.x;
  const int j = blockIdx.y * 4 + __builtin_amdgcn_readfirstlane(threadIdx.y);
  if (j >= d.by) return;   // (the whole wave)
  const bool in = i < d.bx;
  const int ii = in ? i : d.bx - 1;   // (addresses stay in the box)
  double dyc, dyw, dxc, dxs, az;
  if (CURV) {
    const int o = i2(g, ii, j);
    dyc = (double)g.cv.dycf[o];
    dyw = (double)g.cv.dycf[o - 1];
    dxc = (double)g.cv.dxfc[o];
    dxs = (double)g.cv.dxfc[o - g.sx];
    az = (double)azff[o];
  } else {
    dyc = dyw = (double)g.dy;
    dxc = (double)uniform_at(g.dxc, j);
    dxs = (double)uniform_at(g.dxc, j - 1);
    az = (double)uniform_at(g.azf, j);
  }
  const int kk0 = blockIdx.z * DER_LEVELS;
  for (int q = 0; q < DER_LEVELS && kk0 + q < d.k_count; q++) {
    const int k = d.k_first + kk0 + q;
    const long long ou = der_off(g, g.pl_c, ii, j, k), ov = der_off(g, g.pl_v, ii, j, k);
    const double vc = (double)v[ov], vw = (double)v[ov - 1], uc = (double)u[ou], us = (double)u[ou - g.sx];
    const double a = dyc * vc, b = dyw * vw, c = dxc * uc, e = dxs * us;
    const double z = ((a - b) - (c - e)) / az;
    if (in) d.out[der_out(d, i, j, kk0 + q)] = (real)(az == 0.0 ? 0.0 : z);
  }
}

// KE(i,j,k) = 0.25 ((u(i)^2 + u(i+1)^2) + (v(j)^2 + v(j+1)^2)) at (c,c,c): Oceananigans' (Ix u^2 + Iy v^2) / 2
__global__ __launch_bounds__(256) void k_derived_kinetic_energy(Grid g, const real* __restrict__ u, const real* __restrict__ v,
                                                                 DerivedOut d) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 64 + threadIdx.x;
  const int j = blockIdx.y * 4 + __builtin_amdgcn_readfirstlane(threadIdx.y);
  if (j >= d.by) return;
  const bool in = i < d.bx;
  const int ii = in ? i : d.bx - 1;
  const int kk0 = blockIdx.z * DER_LEVELS;
  for (int q = 0; q < DER_LEVELS && kk0 + q < d.k_count; q++) {
    const int k = d.k_first + kk0 + q;
    const long long ou = der_off(g, g.pl_c, ii, j, k), ov = der_off(g, g.pl_v, ii, j, k);
    const double u0 = (double)u[ou], u1 = (double)u[ou + 1], v0 = (double)v[ov], v1 = (double)v[ov + g.sx];
    const double a = u0 * u0, b = u1 * u1, c = v0 * v0, e = v1 * v1;
    const double ke = 0.25 * ((a + b) + (c + e));
    if (in) d.out[der_out(d, i, j, kk0 + q)] = (real)ke;
  }
}

// rho - rho0 of one cell from the table `c` of its level: teos10_level on s, t formed as k_compute_p forms them.  Shared by
// k_derived_density and the class sums (class_kernels.hpp), which must bin the very bits the former stores.
__device__ __forceinline__ double derived_density_value(const double* __restrict__ c, real t, real s) {
  const double sc = 0.875 / 35.16504;
  return teos10_level(c, sqrt_pos(((double)s + 32.0) * sc), (double)t * 0.025);
}

// rho(T, S, z_k) - rho0 (POT: rho(T, S, 0) - rho0, one table `eos0` folded at Z = 0) at (c,c,c); 0 in the immersed cells
// (first_wet: diagnostics' table of the (c,c) columns, null on a grid without a bottom table)
template <bool POT>
__global__ __launch_bounds__(256) void k_derived_density(Grid g, const real* __restrict__ T, const real* __restrict__ S,
                                                          const double* __restrict__ eos0, const unsigned short* __restrict__ first_wet,
                                                          DerivedOut d) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  const int j = blockIdx.y * 4 + __builtin_amdgcn_readfirstlane(threadIdx.y);
  if (j >= d.by) return;
  const bool in = i < d.bx;
  const int ii = in ? i : d.bx - 1;
  const int kb = first_wet ? (int)first_wet[i2(g, ii, j)] : 0;
  const int kk0 = blockIdx.z * DER_LEVELS;
  for (int q = 0; q < DER_LEVELS && kk0 + q < d.k_count; q++) {
    const int k = d.k_first + kk0 + q;
    const double* c = POT ? eos0 : g.eos + 28 * k;
    const long long o = der_off(g, g.pl_c, ii, j, k);
    const double rho = derived_density_value(c, T[o], S[o]);
    if (in) d.out[der_out(d, i, j, kk0 + q)] = k < kb ? real(0) : (real)rho;
  }
}

// Mixed-layer depth, one thread per column, coalesced in i.  sigma: the potential density of every level as k_derived_density<true>
// stored it (packed bx x by x Nz, values of the float type: the same bits gb25_get_derived hands out).  zt: (double) of the
// model's zc[0 .. Nz) followed by zf[0 .. Nz].  d(k) = sigma(k) - sigma(Nz - 1); marching down from Nz - 2, at the first wet k with
// d(k) >= param: -(zc(k+1) + (zc(k) - zc(k+1)) ((param - d(k+1)) / (d(k) - d(k+1)))); never: -zf(first wet level); dry column: 0.
__global__ __launch_bounds__(256) void k_derived_mixed_layer(Grid g, const real* __restrict__ sigma, const unsigned short* __restrict__ first_wet,
                                                              const double* __restrict__ zt, double param, real* __restrict__ out, int bx, int by) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 64 + threadIdx.x;
  const int j = blockIdx.y * 4 + threadIdx.y;
  if (i >= bx || j >= by) return;
  const int Nz = g.Nz;
  const int kb = first_wet ? (int)first_wet[i2(g, i, j)] : 0;
  const long long col = (long long)i + (long long)bx * j, plane = (long long)bx * by;
  double depth = 0.0;
  if (kb < Nz) {
    const double* zc = zt;
    const double* zf = zt + Nz;
    const double s0 = (double)sigma[col + plane * (Nz - 1)];
    double dprev = 0.0;
    depth = -zf[kb];
    for (int k = Nz - 2; k >= kb; k--) {
      const double dk = (double)sigma[col + plane * k] - s0;
      if (dk >= param) {
        const double frac = (param - dprev) / (dk - dprev);
        const double step = (zc[k] - zc[k + 1]) * frac;
        depth = -(zc[k + 1] + step);
        break;
      }
      dprev = dk;
    }
  }
  out[col] = (real)depth;
}

// Levels of the interior of an ordinary field into the packed scratch array.  box: the interior box whose first level is the
// first requested one, bz = the number of levels.  One wave per row; the row is cut into 16-byte chunks aligned in the DESTINATION:
// a whole chunk is one vector store, fed by one vector load where the source happens to be aligned as well and by element loads
// where it is not; the cut chunks at the two ends of a row go element by element.
template <class T>
__global__ __launch_bounds__(256) void k_gather_levels(const T* __restrict__ src, DiagBox box, T* __restrict__ dst) {
  constexpr int VW = 16 / sizeof(T);
  using V = T __attribute__((ext_vector_type(VW)));
  const int j = blockIdx.y * 4 + __builtin_amdgcn_readfirstlane(threadIdx.y);
  if (j >= box.by) return;
  const int kk = blockIdx.z;
  const T* s = src + (box.origin + box.pitch * j + box.plane * kk);
  T* t = dst + (long long)box.bx * ((long long)j + (long long)box.by * kk);
  const int mis = (int)(((unsigned long long)t / sizeof(T)) & (VW - 1));
  const int nchunks = (mis + box.bx + VW - 1) / VW;
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= nchunks) return;
  const int x0 = VW * c - mis;
  if (x0 >= 0 && x0 + VW <= box.bx) {
    V v;
    if (((unsigned long long)(s + x0) & 15) == 0) {
      v = *reinterpret_cast<const V*>(s + x0);
    } else {
#pragma unroll
      for (int q = 0; q < VW; q++) v[q] = s[x0 + q];
    }
    *reinterpret_cast<V*>(t + x0) = v;
  } else {
#pragma unroll
    for (int q = 0; q < VW; q++)
      if (x0 + q >= 0 && x0 + q < box.bx) t[x0 + q] = s[x0 + q];
  }
}

// ---- transports (gb25_get_transport): how much water, heat and salt crosses the faces of v (GB25_ACROSS_Y) or of u
// (GB25_ACROSS_X), summed along a window of i or of j.  Definitions: include/gb25.h.  A face's terms are formed in fp64 on (double)
// of the stored values with floating-point contraction OFF, in the written order; gb-25_amd/transports.py restates them bit for bit.
//   k_transport_rows<CURV>     y faces: ONE WAVE takes ONE ROW (j, k) of v's interior, cut into chunks of four like k_field_moments'
//                     rows; v is read once, T and S twice (rows j - 1 and j), every load of a chunk ahead of its arithmetic; the
//                     fixed shuffle tree; lines[j + by k].  The sum of a row is fixed but not sequential.
//   k_transport_columns<CURV>  x faces: ONE THREAD per (i, k) walks j south to north and adds in that order; lanes run along i, so
//                     u, T(i - 1), T(i), S(i - 1), S(i) and the tables are five coalesced loads a row and more; TR_UNROLL rows'
//                     loads are issued ahead of their arithmetic.  lines[i + bx k] is the sequential sum of the terms.
//   k_transport_fold           one lane per line n: psi[n] = 0, psi[n + N (k + 1)] = psi[n + N k] + lines[n + N k] member by member,
//                     profile[n] = psi[n + N Nz].
struct TransportPartial {   // = gb25_transport
  double area, volume, heat, salt;
  long long faces, nonfinite;
};
__device__ __forceinline__ TransportPartial diag_combine(TransportPartial a, const TransportPartial& b) {
  a.area += b.area;
  a.volume += b.volume;
  a.heat += b.heat;
  a.salt += b.salt;
  a.faces += b.faces;
  a.nonfinite += b.nonfinite;
  return a;
}
// diagnostics' own tables of the faces of one direction, parent layout of a (c,f) field like MomentsTables'
struct TransportTables {
  const real* length;             // DXCF (y faces) / DYFC (x faces); null: GB25_M_DXF(j) / GB25_M_DY of the LatitudeLongitudeGrid
  const unsigned short* first;    // first wet level of the face's column (MOMENTS_DRY: none); null: every level is wet
  int pivot_row;                  // x faces: local row of the GLOBAL pivot row of a folded grid on this rank, else -1
};
// one face of area a: skipped whole when one of its five values is not finite
__device__ __forceinline__ void transport_face(TransportPartial& p, double a, double vel, double t0, double t1, double s0, double s1) {
#pragma clang fp contract(off)
  const bool wet = a > 0.0;
  const bool finite = __builtin_isfinite(vel) && __builtin_isfinite(t0) && __builtin_isfinite(t1) && __builtin_isfinite(s0) && __builtin_isfinite(s1);
  if (wet && finite) {
    const double q = a * vel;
    const double tm = 0.5 * (t0 + t1), sm = 0.5 * (s0 + s1);
    const double qt = q * tm, qs = q * sm;
    p.area += a;
    p.volume += q;
    p.heat += qt;
    p.salt += qs;
  }
  p.faces += (wet && finite) ? 1 : 0;   // (two counters by value: an if / else here becomes an indexed update in scratch memory)
  p.nonfinite += (wet && !finite) ? 1 : 0;
}

// columns [i0, i0 + bx) of the by rows of v's interior
template <bool CURV>
__global__ __launch_bounds__(DIAG_THREADS) void k_transport_rows(Grid g, TransportTables tab, const real* __restrict__ v,
                                                                 const real* __restrict__ T, const real* __restrict__ S, int i0, int bx,
                                                                 int by, TransportPartial* __restrict__ lines) {
#pragma clang fp contract(off)
  const long long r = (long long)blockIdx.x * (DIAG_THREADS / 64) + (threadIdx.x >> 6);
  if (r >= (long long)by * g.Nz) return;
  const int lane = threadIdx.x & 63;
  const int k = (int)(r / by), j = (int)(r - (long long)k * by);
  TransportPartial p = {0.0, 0.0, 0.0, 0.0, 0, 0};
  const bool wall = j == g.jws || (j == g.jwn && !g.cv.north_fold);   // (a wall of the GLOBAL grid: dry, nothing is read)
  if (!wall) {
    const real* rv = v + der_off(g, g.pl_v, i0, j, k);
    const real *rt1 = T + der_off(g, g.pl_c, i0, j, k), *rt0 = rt1 - g.sx;
    const real *rs1 = S + der_off(g, g.pl_c, i0, j, k), *rs0 = rs1 - g.sx;
    const real* rl = CURV ? tab.length + i2(g, i0, j) : nullptr;
    const unsigned short* rf = tab.first ? tab.first + i2(g, i0, j) : nullptr;
    const double dz = (double)g.dzc[k];
    const double a_row = CURV ? 0.0 : (double)g.dxf[j] * dz;
    const int mis = diag_misalignment(rv), nchunks = (mis + bx + 3) >> 2;
    for (int c = lane; c < nchunks; c += 64) {
      const int x0 = 4 * c - mis;
      real ev[4], et0[4], et1[4], es0[4], es1[4], el[4];
      unsigned short ef[4];
      diag_load4(rv, x0, bx, ev);
      diag_load4(rt0, x0, bx, et0);
      diag_load4(rt1, x0, bx, et1);
      diag_load4(rs0, x0, bx, es0);
      diag_load4(rs1, x0, bx, es1);
      if (CURV) diag_load4(rl, x0, bx, el);
      if (rf) diag_load4(rf, x0, bx, ef);
#pragma unroll
      for (int s = 0; s < 4; s++) {
        const int x = x0 + s;
        if (x < 0 || x >= bx) continue;
        const double a = (rf && k < (int)ef[s]) ? 0.0 : (CURV ? (double)el[s] * dz : a_row);
        transport_face(p, a, (double)ev[s], (double)et0[s], (double)et1[s], (double)es0[s], (double)es1[s]);
      }
    }
    p = diag_wave_reduce(p);
  }
  if (lane == 0) lines[r] = p;
}

// rows [j0, j0 + nj) of u's interior; block 64 x 4: a wave = 64 consecutive i of one level
constexpr int TR_UNROLL = 4;
template <bool CURV>
__global__ __launch_bounds__(256) void k_transport_columns(Grid g, TransportTables tab, const real* __restrict__ u,
                                                           const real* __restrict__ T, const real* __restrict__ S, int j0, int nj,
                                                           TransportPartial* __restrict__ lines) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 64 + threadIdx.x;
  const int k = blockIdx.y * 4 + __builtin_amdgcn_readfirstlane(threadIdx.y);
  if (i >= g.Nx || k >= g.Nz) return;
  const real* length = tab.length;
  const unsigned short* first = tab.first;
  const int pivot_row = tab.pivot_row;
  const double dz = (double)uniform_at(g.dzc, k);
  const double a_all = CURV ? 0.0 : (double)g.dy * dz;
  TransportPartial p = {0.0, 0.0, 0.0, 0.0, 0, 0};
  for (int jb = 0; jb < nj; jb += TR_UNROLL) {
    real eu[TR_UNROLL], et0[TR_UNROLL], et1[TR_UNROLL], es0[TR_UNROLL], es1[TR_UNROLL], el[TR_UNROLL];
    unsigned short ef[TR_UNROLL];
#pragma unroll
    for (int q = 0; q < TR_UNROLL; q++) {
      const int j = j0 + (jb + q < nj ? jb + q : jb);   // (addresses stay in the window)
      const long long o = der_off(g, g.pl_c, i, j, k);
      eu[q] = u[o];
      et0[q] = T[o - 1];
      et1[q] = T[o];
      es0[q] = S[o - 1];
      es1[q] = S[o];
      el[q] = CURV ? length[i2(g, i, j)] : real(0);
      ef[q] = first ? first[i2(g, i, j)] : (unsigned short)0;
    }
#pragma unroll
    for (int q = 0; q < TR_UNROLL; q++) {
      if (jb + q >= nj) break;
      const double fold = (j0 + jb + q == pivot_row) ? 0.5 : 1.0;
      const double a = k < (int)ef[q] ? 0.0 : (CURV ? (double)el[q] * dz : a_all) * fold;
      transport_face(p, a, (double)eu[q], (double)et0[q], (double)et1[q], (double)es0[q], (double)es1[q]);
    }
  }
  lines[(long long)i + (long long)g.Nx * k] = p;
}

__global__ __launch_bounds__(64) void k_transport_fold(const TransportPartial* __restrict__ lines, int N, int Nz,
                                                       TransportPartial* __restrict__ psi, TransportPartial* __restrict__ profile) {
  const int n = blockIdx.x * 64 + threadIdx.x;
  if (n >= N) return;
  TransportPartial p = {0.0, 0.0, 0.0, 0.0, 0, 0};
  psi[n] = p;
  for (int k = 0; k < Nz; k++) {
    p = diag_combine(p, lines[n + (long long)N * k]);
    psi[n + (long long)N * (k + 1)] = p;
  }
  profile[n] = p;
}

}  // namespace gb25
