// surface_kernels.hpp -- fields on surfaces (gb25_compute_on_surfaces, gb25_get_on_surfaces, include/gb25.h): the depth of an
// isopycnal, an isotherm or an isohaline, a field on it, and a field at fixed depths.  Included by gb25_api.hip, launched from
// surfaces_host.hpp.
//
//   k_on_surfaces<SV, SC>  a block is 64 x 4 threads, ONE WAVE = 64 consecutive i of one row j (T, S, u, v, e load coalesced), ONE
//                     THREAD per column; blockIdx.z runs over groups of SURF_TG targets.  The targets of the group are wave-uniform
//                     (scalar loads from the padded target buffer: SURF_MAX doubles, NaN behind the last one, and a NaN never
//                     crosses; a short group tests its own targets only).  The thread marches ONCE down its column: it forms the search variable q and the carried
//                     quantity f of a level once and tests every target of the group against the pair (k + 1, k); a target's
//                     result and its found flag stay in registers (one `real` and one bit per target), the interpolation runs
//                     under a branch only where a target crosses.  When every target of the lane is found the lane leaves the
//                     march.  The targets without a crossing take the face of the bottom or of the top (GROUNDED, OUTCROP).
// q and f of a level: T, S, e as stored; the densities are derived_density_value (diagnostics_kernels.hpp: the function
// k_derived_density stores from, compiled with the contraction of k_compute_p) and the kinetic energy the expression of
// k_derived_kinetic_energy, each rounded to `real` -- the bits gb25_get_derived hands out, no 3-D scratch array, no extra pass.
// The interpolation is fp64 with floating-point contraction OFF (the pragma is lexical: the density lives in its own function),
// IEEE division, rounded once to `real`: numpy restates it bit for bit (gb-25_amd/surfaces.py).
// The result is PACKED: out[i + bx (j + by n)], the status bytes likewise.  Plain vector stores, no atomics, every offset into a
// 3-D array 64-bit.
#pragma once

namespace gb25 {

constexpr int SURF_MAX = 64;   // = GB25_SURFACE_MAX_VALUES
#ifndef GB25_SURF_TG
#define GB25_SURF_TG 16
#endif
constexpr int SURF_TG = GB25_SURF_TG;   // targets per march; SURF_MAX is a multiple of it
static_assert(SURF_TG >= 1 && SURF_TG <= 32 && SURF_MAX % SURF_TG == 0, "groups of targets tile the padded buffer");

enum SurfVar { SV_T = 0, SV_S = 1, SV_SIGMA = 2, SV_DEPTH = 3, SV_COUNT = 4 };
enum SurfCarried { SC_DEPTH = 0, SC_T = 1, SC_S = 2, SC_E = 3, SC_KE = 4, SC_RHO = 5, SC_SIGMA = 6, SC_COUNT = 7 };
enum SurfStatus : unsigned char { SURF_FOUND = 0, SURF_OUTCROP = 1, SURF_GROUNDED = 2, SURF_DRY = 3 };

struct SurfIn {
  const real *T, *S, *u, *v, *e;      // parents; those the instance does not read are null
  const double* eos0;                 // the TEOS-10 table folded at Z = 0
  const unsigned short* first_wet;    // first wet level of the (c,c) column (MOMENTS_DRY: none); null: every level is wet
  const double* zt;                   // (double) zc[0 .. Nz) | zf[0 .. Nz]
  const double* targets;              // SURF_MAX doubles: the n values, then NaN
};
struct SurfOut {
  real* value;
  unsigned char* status;
  int bx, by, n;
};

// KE of k_derived_kinetic_energy, rounded to `real` as it stores it
__device__ __forceinline__ double surf_kinetic_energy(const Grid& g, const real* __restrict__ u, const real* __restrict__ v, int i, int j,
                                                      int k) {
#pragma clang fp contract(off)
  const long long ou = der_off(g, g.pl_c, i, j, k), ov = der_off(g, g.pl_v, i, j, k);
  const double u0 = (double)u[ou], u1 = (double)u[ou + 1], v0 = (double)v[ov], v1 = (double)v[ov + g.sx];
  const double a = u0 * u0, b = u1 * u1, c = v0 * v0, e = v1 * v1;
  const double ke = 0.25 * ((a + b) + (c + e));
  return (double)(real)ke;
}

// q and f of level k of column (i, j)
template <int SV, int SC>
__device__ __forceinline__ void surf_level(const Grid& g, const SurfIn& in, int i, int j, int k, double* q, double* f) {
  constexpr bool need_t = SV == SV_T || SV == SV_SIGMA || SC == SC_T || SC == SC_RHO || SC == SC_SIGMA;
  constexpr bool need_s = SV == SV_S || SV == SV_SIGMA || SC == SC_S || SC == SC_RHO || SC == SC_SIGMA;
  const long long o = der_off(g, g.pl_c, i, j, k);
  real t = real(0), s = real(0);
  if (need_t) t = in.T[o];
  if (need_s) s = in.S[o];
  double sigma = 0.0;
  if (SV == SV_SIGMA || SC == SC_SIGMA) sigma = (double)(real)derived_density_value(in.eos0, t, s);
  if (SV == SV_T) *q = (double)t;
  else if (SV == SV_S) *q = (double)s;
  else if (SV == SV_SIGMA) *q = sigma;
  else *q = -in.zt[k];
  if (SC == SC_T) *f = (double)t;
  else if (SC == SC_S) *f = (double)s;
  else if (SC == SC_E) *f = (double)in.e[o];
  else if (SC == SC_KE) *f = surf_kinetic_energy(g, in.u, in.v, i, j, k);
  else if (SC == SC_RHO) *f = (double)(real)derived_density_value(g.eos + 28 * k, t, s);
  else if (SC == SC_SIGMA) *f = sigma;
  else *f = 0.0;
}

// the target c between qa (level k + 1: za, fa) and qb (level k: zb, fb); the two-product form is exact at both ends
template <int SC>
__device__ __forceinline__ real surf_interpolate(double c, double qa, double qb, double za, double zb, double fa, double fb) {
#pragma clang fp contract(off)
  const double frac = (qa == qb) ? 0.0 : (c - qa) / (qb - qa);
  const double gq = 1.0 - frac;
  if (SC == SC_DEPTH) {
    const double a = za * gq, b = zb * frac;
    return (real)(-(a + b));
  }
  const double a = fa * gq, b = fb * frac;
  return (real)(a + b);
}

__device__ __forceinline__ bool surf_finite(double x) { return __builtin_fabs(x) < __builtin_inf(); }

template <int SV, int SC>
__global__ __launch_bounds__(256) void k_on_surfaces(Grid g, SurfIn in, SurfOut d) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 64 + threadIdx.x;
  const int j = blockIdx.y * 4 + __builtin_amdgcn_readfirstlane(threadIdx.y);
  if (j >= d.by) return;   // (the whole wave)
  const bool inside = i < d.bx;
  const int ii = inside ? i : d.bx - 1;   // (addresses stay in the box)
  const int t0 = blockIdx.z * SURF_TG;
  const int Nz = g.Nz, ks = Nz - 1;
  const int kb = in.first_wet ? (int)in.first_wet[i2(g, ii, j)] : 0;
  const double* tg = in.targets + t0;   // (wave-uniform: SURF_TG of the SURF_MAX padded values)
  const double* zc = in.zt;
  const double* zf = in.zt + Nz;
  real res[SURF_TG];
#pragma unroll
  for (int t = 0; t < SURF_TG; t++) res[t] = real(0);
  constexpr unsigned all = SURF_TG == 32 ? 0xffffffffu : (1u << SURF_TG) - 1u;
  const int nt = d.n - t0 < SURF_TG ? d.n - t0 : SURF_TG;   // targets of this group (uniform)
  unsigned found = nt < SURF_TG ? all & ~((1u << nt) - 1u) : 0u;   // (the padding counts as found: it is never stored)
  const bool wet = kb < Nz;
  double qs = 0.0, fs = 0.0, qa = 0.0, fa = 0.0;
  if (wet) {
    surf_level<SV, SC>(g, in, ii, j, ks, &qs, &fs);
    qa = qs;
    fa = fs;
    for (int k = ks - 1; k >= kb; k--) {
      double qb, fb;
      surf_level<SV, SC>(g, in, ii, j, k, &qb, &fb);
      if (surf_finite(qa) && surf_finite(qb)) {
#pragma unroll
        for (int t = 0; t < SURF_TG; t++) {
          if (t >= nt) break;   // (uniform: a short group pays for its own targets only)
          const double c = tg[t];
          const bool cross = (qa <= c && c <= qb) || (qb <= c && c <= qa);
          if (cross && !(found & (1u << t))) {
            res[t] = surf_interpolate<SC>(c, qa, qb, zc[k + 1], zc[k], fa, fb);
            found |= 1u << t;
          }
        }
      }
      qa = qb;
      fa = fb;
      if (found == all) break;
    }
  }
  // (here qa, fa are q and f of the first wet level wherever a target is still not found)
  const bool down = qa >= qs;
#pragma unroll
  for (int t = 0; t < SURF_TG; t++) {
    if (t0 + t >= d.n) break;   // (uniform)
    const double c = tg[t];
    real r = res[t];
    unsigned char st = SURF_FOUND;
    if (!wet) {
      st = SURF_DRY;
      r = real(0);
    } else if (!(found & (1u << t))) {
      const bool grounded = (c > qs) == down;
      st = grounded ? SURF_GROUNDED : SURF_OUTCROP;
      if (SC == SC_DEPTH) r = (real)(grounded ? -zf[kb] : -zf[Nz]);
      else r = (real)(grounded ? fa : fs);
    }
    if (inside) {
      const long long o = (long long)i + (long long)d.bx * ((long long)j + (long long)d.by * (t0 + t));
      d.value[o] = r;
      d.status[o] = st;
    }
  }
}

}  // namespace gb25
