// class_kernels.hpp -- sums in classes of T, S or potential density (gb25_get_class_sums, include/gb25.h): the transport through
// every row of y faces sorted by the class of the water that crosses (the overturning in density classes), and the census of
// volume, heat and salt per class and row of cells.  Included by gb25_api.hip, launched from diagnostics_host.hpp.
//
// The order of every sum is part of the ABI (numpy restates it bit for bit, gb-25_amd/classes.py), so there are no floating-point
// atomics and no tree over the summed index:
//   k_class_rows<WHAT, CURV, VAR>  ONE BLOCK of four waves per row n; wave w takes the levels k = w, w + 4, ...  For a level the
//                     wave walks the window in chunks of 64 adjacent faces (cells): lane l loads face i0 + 64 c + l -- every load of
//                     the chunk ahead of its arithmetic --, forms the four terms and the bin, and PARKS them in the wave's own part
//                     of LDS.  Then LANES OWN BINS: lane l keeps the partial sums of the bins l, l + 64, l + 128, l + 192 in named
//                     registers.  The wave scans the parked entries in i order; the bin of an entry is wave-uniform (a broadcast
//                     read made scalar), an entry that does not contribute is skipped by a uniform branch, and the one lane that
//                     owns the bin adds the terms: the partial p(n, k, b) is the SEQUENTIAL sum over i ascending, starting from +0.
//                     After the level the wave writes its B partials to LDS; after a barrier thread b adds the (up to) four
//                     partials of the round to its running total in k order: ROWS[n, b] = ((0 + p(n,0,b)) + p(n,1,b)) + ...
//                     LDS: 4 waves x 256 bins x (4 doubles + 1 count) = 36 KB of level partials, 9 KB of parked chunks, 2 KB of
//                     edges, 1 KB of counters: 48 KB, static.
//   k_class_fold      thread n: psi[n, 0] = 0, psi[n, e + 1] = psi[n, e] + ROWS[n, e]; thread b: TOTAL[b] = the sum of ROWS[n, b]
//                     over n ascending; member by member.
// Terms: those of transport_face (FACES_Y) and the (c,c,c) measure of k_field_moments (CELLS), fp64 on (double) of the stored
// values, contraction OFF; the potential density is derived_density_value, the function k_derived_density<true> stores from,
// rounded to `real` as there.  Plain vector loads and stores; every offset into a 3-D array is 64-bit.
#pragma once

namespace gb25 {

constexpr int CLASS_MAX_BINS = 256;   // = GB25_CLASS_MAX_BINS
constexpr int CLASS_THREADS = 256;
enum ClassWhat { CL_FACES_Y = 0, CL_CELLS = 1 };
enum ClassVar { CLV_T = 0, CLV_S = 1, CLV_SIGMA = 2 };

struct ClassPartial {   // = gb25_class_sum
  double measure, flow, heat, salt;
  long long count, nonfinite;
};
__device__ __forceinline__ ClassPartial diag_combine(ClassPartial a, const ClassPartial& b) {
  a.measure += b.measure;
  a.flow += b.flow;
  a.heat += b.heat;
  a.salt += b.salt;
  a.count += b.count;
  a.nonfinite += b.nonfinite;
  return a;
}
// diagnostics' own tables (parent layout of a (c,f) field) and the class edges
struct ClassTables {
  const real* metric;             // FACES_Y: DXCF, CELLS: AZCC; unused on the LatitudeLongitudeGrid (row tables)
  const unsigned short* first;    // first wet level of the face's / the cell's column (MOMENTS_DRY: none); null: every level is wet
  const double* eos0;             // the TEOS-10 table folded at Z = 0
  const double* edges;            // CLASS_MAX_BINS doubles: the n_edges edges, then +Inf
  int pivot_row;                  // CELLS: local row of the GLOBAL pivot row of a folded grid on this rank, else -1
};

template <int VAR>
__device__ __forceinline__ double class_value(const double* __restrict__ eos0, real t, real s) {
  if (VAR == CLV_T) return (double)t;
  if (VAR == CLV_S) return (double)s;
  return (double)(real)derived_density_value(eos0, t, s);
}

// the number of edges e <= c, c finite: edges[0 .. 255] ascending, +Inf behind the last edge (so the answer is at most 255)
__device__ __forceinline__ int class_bin(const double* edges, double c) {
  int b = 0;
#pragma unroll
  for (int step = CLASS_MAX_BINS / 2; step >= 1; step >>= 1)
    if (edges[b + step - 1] <= c) b += step;
  return b;
}

#define GB25_CLASS_ADD(s)      \
  {                            \
    m##s = m##s + tm;          \
    q##s = q##s + tq;          \
    h##s = h##s + th;          \
    x##s = x##s + tx;          \
    c##s = c##s + 1;           \
  }
#define GB25_CLASS_PUT(s)                        \
  if (lane + 64 * s < B) {                       \
    s_lvl[w][0][lane + 64 * s] = m##s;           \
    s_lvl[w][1][lane + 64 * s] = q##s;           \
    s_lvl[w][2][lane + 64 * s] = h##s;           \
    s_lvl[w][3][lane + 64 * s] = x##s;           \
    s_cnt[w][lane + 64 * s] = c##s;              \
  }

// rows [0, N) of v's interior (FACES_Y) or of T's (CELLS), columns [i0, i0 + bx), B = n_edges + 1 bins; rows[n B + b]
template <int WHAT, bool CURV, int VAR>
__global__ __launch_bounds__(CLASS_THREADS) void k_class_rows(Grid g, ClassTables tab, const real* __restrict__ v,
                                                              const real* __restrict__ T, const real* __restrict__ S, int i0, int bx,
                                                              int B, ClassPartial* __restrict__ rows) {
#pragma clang fp contract(off)
  __shared__ double s_edges[CLASS_MAX_BINS];
  __shared__ double s_term[4][64][4];               // [wave][entry of the chunk][measure, flow, heat, salt]
  __shared__ int s_bin[4][64];                      // the entry's bin, -1: it does not contribute
  __shared__ double s_lvl[4][4][CLASS_MAX_BINS];    // [wave][member][bin]: the partials of the wave's level
  __shared__ int s_cnt[4][CLASS_MAX_BINS];
  __shared__ int s_nf[CLASS_THREADS];
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = blockIdx.x;
  ClassPartial tot = {0.0, 0.0, 0.0, 0.0, 0, 0};
  // (a row of y faces on a wall of the GLOBAL grid: dry, nothing is read; uniform for the block)
  const bool wall = WHAT == CL_FACES_Y && (j == g.jws || (j == g.jwn && !g.cv.north_fold));
  if (wall) {
    if (tid < B) rows[(long long)j * B + tid] = tot;
    return;
  }
  s_edges[tid] = tab.edges[tid];
  __syncthreads();
  const real* metric = tab.metric;
  const unsigned short* first = tab.first;
  const double* eos0 = tab.eos0;
  const double fold = (WHAT == CL_CELLS && j == tab.pivot_row) ? 0.5 : 1.0;
  const int nchunks = (bx + 63) >> 6;
  int nf = 0;
  for (int kr = 0; kr < g.Nz; kr += 4) {
    const int k = kr + w;
    if (k < g.Nz) {
      double m0 = 0.0, q0 = 0.0, h0 = 0.0, x0 = 0.0, m1 = 0.0, q1 = 0.0, h1 = 0.0, x1 = 0.0;
      double m2 = 0.0, q2 = 0.0, h2 = 0.0, x2 = 0.0, m3 = 0.0, q3 = 0.0, h3 = 0.0, x3 = 0.0;
      int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
      const double dz = (double)g.dzc[k];
      const double row_measure = CURV ? 0.0 : (WHAT == CL_FACES_Y ? (double)g.dxf[j] * dz : ((double)g.azc[j] * dz) * fold);
      for (int c = 0; c < nchunks; c++) {
        const int n_in = bx - 64 * c < 64 ? bx - 64 * c : 64;   // entries of this chunk
        const bool in = lane < n_in;
        const int i = i0 + 64 * c + (in ? lane : n_in - 1);     // (addresses stay in the window)
        const long long o = der_off(g, g.pl_c, i, j, k);
        const int o2 = i2(g, i, j);
        real ev = real(0), et0 = real(0), es0 = real(0), em = real(0);
        if (WHAT == CL_FACES_Y) {
          ev = v[der_off(g, g.pl_v, i, j, k)];
          et0 = T[o - g.sx];
          es0 = S[o - g.sx];
        }
        const real et1 = T[o], es1 = S[o];
        if (CURV) em = metric[o2];
        const int kb = first ? (int)first[o2] : 0;
        double tm, tq, th, tx, cls;
        bool finite;
        if (WHAT == CL_FACES_Y) {
          const double a = k < kb ? 0.0 : (CURV ? (double)em * dz : row_measure);
          const double vel = (double)ev, t0 = (double)et0, t1 = (double)et1, s0 = (double)es0, s1 = (double)es1;
          const double q = a * vel;
          const double tmid = 0.5 * (t0 + t1), smid = 0.5 * (s0 + s1);
          cls = 0.5 * (class_value<VAR>(eos0, et0, es0) + class_value<VAR>(eos0, et1, es1));
          finite = __builtin_isfinite(vel) && __builtin_isfinite(t0) && __builtin_isfinite(t1) && __builtin_isfinite(s0) && __builtin_isfinite(s1);
          tm = a;
          tq = q;
          th = q * tmid;
          tx = q * smid;
        } else {
          const double mu = k < kb ? 0.0 : (CURV ? ((double)em * dz) * fold : row_measure);
          const double t1 = (double)et1, s1 = (double)es1;
          cls = class_value<VAR>(eos0, et1, es1);
          finite = __builtin_isfinite(t1) && __builtin_isfinite(s1);
          tm = mu;
          tq = 0.0;
          th = mu * t1;
          tx = mu * s1;
        }
        finite = finite && __builtin_isfinite(cls);
        const bool wet = in && tm > 0.0;
        nf += (wet && !finite) ? 1 : 0;
        // park the entry; the wave's own part of LDS: the wave's LDS operations execute in order, no barrier of the block is needed
        s_bin[w][lane] = (wet && finite) ? class_bin(s_edges, finite ? cls : 0.0) : -1;
        s_term[w][lane][0] = tm;
        s_term[w][lane][1] = tq;
        s_term[w][lane][2] = th;
        s_term[w][lane][3] = tx;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        for (int e = 0; e < n_in; e++) {
          const int b = __builtin_amdgcn_readfirstlane(s_bin[w][e]);
          if (b < 0) continue;   // (uniform)
          if ((b & 63) == lane) {
            tm = s_term[w][e][0];
            tq = s_term[w][e][1];
            th = s_term[w][e][2];
            tx = s_term[w][e][3];
            switch (b >> 6) {   // (uniform)
              case 0: GB25_CLASS_ADD(0) break;
              case 1: GB25_CLASS_ADD(1) break;
              case 2: GB25_CLASS_ADD(2) break;
              default: GB25_CLASS_ADD(3) break;
            }
          }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      }
      GB25_CLASS_PUT(0)
      GB25_CLASS_PUT(1)
      GB25_CLASS_PUT(2)
      GB25_CLASS_PUT(3)
    }
    __syncthreads();
    if (tid < B) {
#pragma unroll
      for (int ww = 0; ww < 4; ww++) {
        if (kr + ww >= g.Nz) break;
        tot.measure = tot.measure + s_lvl[ww][0][tid];
        tot.flow = tot.flow + s_lvl[ww][1][tid];
        tot.heat = tot.heat + s_lvl[ww][2][tid];
        tot.salt = tot.salt + s_lvl[ww][3][tid];
        tot.count += s_cnt[ww][tid];
      }
    }
    __syncthreads();
  }
  // the skipped faces (cells) of the row: integers, any order; they go to bin 0
  s_nf[tid] = nf;
  __syncthreads();
  if (tid == 0) {
    long long n = 0;
    for (int t = 0; t < CLASS_THREADS; t++) n += s_nf[t];
    tot.nonfinite = n;
  }
  if (tid < B) rows[(long long)j * B + tid] = tot;
}
#undef GB25_CLASS_ADD
#undef GB25_CLASS_PUT

// rows [N, B] -> psi [N, B + 1] (the running sums over the bins) and total [B] (the sum over the rows, south to north)
__global__ __launch_bounds__(64) void k_class_fold(const ClassPartial* __restrict__ rows, int N, int B, ClassPartial* __restrict__ psi,
                                                   ClassPartial* __restrict__ total) {
  const int q = blockIdx.x * 64 + threadIdx.x;
  if (q < N) {
    ClassPartial p = {0.0, 0.0, 0.0, 0.0, 0, 0};
    psi[(long long)q * (B + 1)] = p;
    for (int e = 0; e < B; e++) {
      p = diag_combine(p, rows[(long long)q * B + e]);
      psi[(long long)q * (B + 1) + e + 1] = p;
    }
  }
  if (q < B) {
    ClassPartial p = {0.0, 0.0, 0.0, 0.0, 0, 0};
    for (int n = 0; n < N; n++) p = diag_combine(p, rows[(long long)n * B + q]);
    total[q] = p;
  }
}

}  // namespace gb25
