// stability_kernels.hpp -- stability diagnostics (gb25_compute_stability, gb25_get_stability, include/gb25.h): what the flow is
// about to do -- N^2, the squared shear, the Richardson number, the Eady growth rate and the Ertel potential vorticity at
// (Center, Center, Face), and the first baroclinic gravity-wave speed per column.  Included by gb25_api.hip, launched from
// stability_host.hpp.
//
//   k_stability_faces<Q, CURV>  a block is 64 x 4 threads, ONE WAVE = 64 consecutive i of one row j (T, S, u, v load coalesced), ONE
//                     THREAD per column; blockIdx.z runs over chunks of STAB_FACES requested faces.  The thread marches UP its
//                     chunk and carries level k - 1 in registers (StabLevel: sigma of the cell and of its four neighbours, the
//                     two averaged velocities, the four corner vorticities -- only what Q reads), so that every T, S, u, v value
//                     is loaded once per level and the equation of state is evaluated once per cell-level per thread; a chunk
//                     pays one extra level, the one below its first face.  The horizontal metrics of the column (StabHoriz)
//                     are loaded once.  Template parameters: the quantity, and CURV (2-D metrics / the row tables of the
//                     LatitudeLongitudeGrid).  The bottom needs no instance of its own: a null table means kb = 0 everywhere.
//   k_stability_wave_speed      ONE THREAD per column marches once from the first wet level to the top and adds in that order.
// sigma is derived_density_value (diagnostics_kernels.hpp: the function k_derived_density stores from, compiled with the
// contraction of k_compute_p) on the one table folded at Z = 0, rounded to `real`, and the corner vorticities are the expression
// of k_derived_vorticity rounded to `real` -- the bits gb25_get_derived hands out, in the halo column and row too; no 3-D scratch
// array, no extra pass.  Everything else is fp64 with floating-point contraction OFF (the pragma is lexical: the density lives in
// its own function), IEEE divisions and square roots, rounded once to `real`: numpy restates it bit for bit
// (gb-25_amd/stability.py).  The result is PACKED: out[i + bx (j + by kk)], kk = 0 .. k_count - 1 for face k_first + kk.  Plain
// vector stores, no atomics, no LDS, every offset into a 3-D array 64-bit.
#pragma once

namespace gb25 {

enum StabKind { ST_N2 = 0, ST_SHEAR2 = 1, ST_RI = 2, ST_EADY = 3, ST_PV = 4, ST_WAVE = 5, ST_COUNT = 6 };
constexpr int STAB_FACES = 16;   // faces a thread marches

struct StabIn {
  const real *T, *S, *u, *v;       // parents; those the instance does not read are null
  const double* eos0;              // the TEOS-10 table folded at Z = 0
  const unsigned short* wet;       // first wet level of the (c,c) columns AND of the ring of columns around the interior
                                   // (MOMENTS_DRY: none); null: every level is wet
  const double* zt;                // (double) zc[0 .. Nz) | zf[0 .. Nz]
  const real *azff, *fff;          // diagnostics' own tables of a curvilinear grid (null on the LatitudeLongitudeGrid)
  double ngr;                      // -(g / rho0): b = ngr sigma
  double param;
  int jtop;                        // local row of the y faces beyond the last row of cells of the GLOBAL grid (a wall or the fold)
};

// the metrics of one column that no level changes.  CURV: DYCF of the rows j, j + 1 and the columns i - 1, i, i + 1, DXFC of the
// rows j - 1, j, j + 1 and the columns i, i + 1, AZFF and the Coriolis parameter of the four corners; else DXC of the rows j - 1,
// j, j + 1 in dx[.][0], AZF and GB25_M_FCOR of the rows j, j + 1 in az[.][0], f[.][0], GB25_M_DY in dy[0][0]
struct StabHoriz {
  real dy[2][3], dx[3][2], az[2][2], f[2][2];
};
template <bool CURV>
__device__ __forceinline__ void stab_horiz(const Grid& g, const StabIn& in, int i, int j, bool pv, StabHoriz* h) {
  if (CURV) {
    const int o = i2(g, i, j);
#pragma unroll
    for (int b = 0; b < 2; b++)
#pragma unroll
      for (int a = 0; a < 2; a++) h->f[b][a] = in.fff[o + a + b * g.sx];
    if (!pv) return;
#pragma unroll
    for (int b = 0; b < 2; b++) {
#pragma unroll
      for (int a = 0; a < 3; a++) h->dy[b][a] = g.cv.dycf[o + (a - 1) + b * g.sx];
#pragma unroll
      for (int a = 0; a < 2; a++) h->az[b][a] = in.azff[o + a + b * g.sx];
    }
#pragma unroll
    for (int b = 0; b < 3; b++)
#pragma unroll
      for (int a = 0; a < 2; a++) h->dx[b][a] = g.cv.dxfc[o + a + (b - 1) * g.sx];
  } else {
    h->dy[0][0] = g.dy;
#pragma unroll
    for (int b = 0; b < 3; b++) h->dx[b][0] = uniform_at(g.dxc, j - 1 + b);
#pragma unroll
    for (int b = 0; b < 2; b++) {
      h->az[b][0] = uniform_at(g.azf, j + b);
      h->f[b][0] = uniform_at(g.fcor, j + b);
    }
  }
}

// one level of one column, as far as Q reads it
struct StabLevel {
  double sc, sw, se, ss, sn;         // sigma of the cell and of its western, eastern, southern, northern neighbour
  double ub, vb;                     // 0.5 (u(i) + u(i+1)), 0.5 (v(j) + v(j+1))
  double z[2][2];                    // the corner vorticities [b][a]: corner (i + a, j + b)
};

__device__ __forceinline__ double stab_sigma(const StabIn& in, long long o) {
  return (double)(real)derived_density_value(in.eos0, in.T[o], in.S[o]);
}

// zeta of k_derived_vorticity at corner (i + a, j + b), rounded to `real` as it stores it
template <bool CURV>
__device__ __forceinline__ double stab_zeta(const StabHoriz& h, int a, int b, double vc, double vw, double uc, double us) {
#pragma clang fp contract(off)
  const double dyc = (double)(CURV ? h.dy[b][a + 1] : h.dy[0][0]), dyw = (double)(CURV ? h.dy[b][a] : h.dy[0][0]);
  const double dxc = (double)(CURV ? h.dx[b + 1][a] : h.dx[b + 1][0]), dxs = (double)(CURV ? h.dx[b][a] : h.dx[b][0]);
  const double az = (double)(CURV ? h.az[b][a] : h.az[b][0]);
  const double p = dyc * vc, q = dyw * vw, r = dxc * uc, s = dxs * us;
  const double z = ((p - q) - (r - s)) / az;
  return (double)(real)(az == 0.0 ? 0.0 : z);
}

template <int Q, bool CURV>
__device__ __forceinline__ void stab_level(const Grid& g, const StabIn& in, const StabHoriz& h, int i, int j, int k, StabLevel* L) {
#pragma clang fp contract(off)
  constexpr bool need_sigma = Q != ST_SHEAR2, need_shear = Q != ST_N2, pv = Q == ST_PV;
  const long long oc = der_off(g, g.pl_c, i, j, k), ov = der_off(g, g.pl_v, i, j, k);
  if (need_sigma) L->sc = stab_sigma(in, oc);
  if (pv) {
    L->sw = stab_sigma(in, oc - 1);
    L->se = stab_sigma(in, oc + 1);
    L->ss = stab_sigma(in, oc - g.sx);
    L->sn = stab_sigma(in, oc + g.sx);
    double u[3][2], v[2][3];   // u[row j - 1 + b][column i + a], v[row j + b][column i - 1 + a]
#pragma unroll
    for (int b = 0; b < 3; b++)
#pragma unroll
      for (int a = 0; a < 2; a++) u[b][a] = (double)in.u[oc + a + (long long)(b - 1) * g.sx];
#pragma unroll
    for (int b = 0; b < 2; b++)
#pragma unroll
      for (int a = 0; a < 3; a++) v[b][a] = (double)in.v[ov + (a - 1) + (long long)b * g.sx];
    L->ub = 0.5 * (u[1][0] + u[1][1]);
    L->vb = 0.5 * (v[0][1] + v[1][1]);
#pragma unroll
    for (int b = 0; b < 2; b++)
#pragma unroll
      for (int a = 0; a < 2; a++) L->z[b][a] = stab_zeta<CURV>(h, a, b, v[b][a + 1], v[b][a], u[b + 1][a], u[b][a]);
  } else if (need_shear) {
    const double u0 = (double)in.u[oc], u1 = (double)in.u[oc + 1], v0 = (double)in.v[ov], v1 = (double)in.v[ov + g.sx];
    L->ub = 0.5 * (u0 + u1);
    L->vb = 0.5 * (v0 + v1);
  }
}

// the first wet levels the instance tests: of the cell and, for the potential vorticity, of its four neighbours
struct StabWet {
  int c, w, e, s, n;
};

// a horizontal buoyancy gradient across one face at one level; 0 where `open` is false
__device__ __forceinline__ double stab_gradient(bool open, double ngr, double s_far, double s_near, double d) {
#pragma clang fp contract(off)
  const double b1 = ngr * s_far, b0 = ngr * s_near;
  const double gq = (b1 - b0) / d;
  return open ? gq : 0.0;
}

// the four gradients of level k: x faces i and i + 1, y faces j and j + 1
template <bool CURV>
__device__ __forceinline__ void stab_gradients(const StabIn& in, const StabHoriz& h, const StabLevel& L, const StabWet& w, int k,
                                               bool wall_s, bool wall_n, double* gx, double* gy) {
  const double dxw = (double)(CURV ? h.dx[1][0] : h.dx[1][0]), dxe = (double)(CURV ? h.dx[1][1] : h.dx[1][0]);
  const double dys = (double)(CURV ? h.dy[0][1] : h.dy[0][0]), dyn = (double)(CURV ? h.dy[1][1] : h.dy[0][0]);
  gx[0] = stab_gradient(k >= w.c && k >= w.w, in.ngr, L.sc, L.sw, dxw);
  gx[1] = stab_gradient(k >= w.c && k >= w.e, in.ngr, L.se, L.sc, dxe);
  gy[0] = stab_gradient(!wall_s && k >= w.c && k >= w.s, in.ngr, L.sc, L.ss, dys);
  gy[1] = stab_gradient(!wall_n && k >= w.c && k >= w.n, in.ngr, L.sn, L.sc, dyn);
}

template <int Q, bool CURV>
__global__ __launch_bounds__(256) void k_stability_faces(Grid g, StabIn in, DerivedOut d) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 64 + threadIdx.x;
  const int j = blockIdx.y * 4 + __builtin_amdgcn_readfirstlane(threadIdx.y);
  if (j >= d.by) return;   // (the whole wave)
  const bool inside = i < d.bx;
  const int ii = inside ? i : d.bx - 1;   // (addresses stay in the box)
  const int Nz = g.Nz;
  const int kk0 = blockIdx.z * STAB_FACES;
  const int kk1 = kk0 + STAB_FACES < d.k_count ? kk0 + STAB_FACES : d.k_count;
  const double* zc = in.zt;
  StabWet w = {0, 0, 0, 0, 0};
  if (in.wet) {
    const int o = i2(g, ii, j);
    w.c = (int)in.wet[o];
    if (Q == ST_PV) {
      w.w = (int)in.wet[o - 1];
      w.e = (int)in.wet[o + 1];
      w.s = (int)in.wet[o - g.sx];
      w.n = (int)in.wet[o + g.sx];
    }
  }
  StabHoriz h;
  double fc = 0.0;
  if (Q == ST_EADY || Q == ST_PV) {
    stab_horiz<CURV>(g, in, ii, j, Q == ST_PV, &h);
    const double f00 = (double)h.f[0][0], f10 = (double)(CURV ? h.f[0][1] : h.f[0][0]);
    const double f01 = (double)h.f[1][0], f11 = (double)(CURV ? h.f[1][1] : h.f[1][0]);
    fc = 0.25 * ((f00 + f10) + (f01 + f11));
  }
  const bool wall_s = j == g.jws, wall_n = j + 1 == in.jtop;
  StabLevel lo = {}, hi = {};
  bool have_lo = false;
  for (int kk = kk0; kk < kk1; kk++) {
    const int k = d.k_first + kk;   // the face between the cells k - 1 and k
    real r = real(0);
    if (k >= 1 && k < Nz) {
      if (!have_lo) stab_level<Q, CURV>(g, in, h, ii, j, k - 1, &lo);
      have_lo = true;
      stab_level<Q, CURV>(g, in, h, ii, j, k, &hi);
      const double dz = zc[k] - zc[k - 1];
      double n2 = 0.0, s2 = 0.0, du = 0.0, dv = 0.0;
      if (Q != ST_SHEAR2) n2 = (in.ngr * (hi.sc - lo.sc)) / dz;
      if (Q != ST_N2) {
        du = (hi.ub - lo.ub) / dz;
        dv = (hi.vb - lo.vb) / dz;
        const double a = du * du, b = dv * dv;
        s2 = a + b;
      }
      double x;
      if (Q == ST_N2) {
        x = n2;
      } else if (Q == ST_SHEAR2) {
        x = s2;
      } else if (Q == ST_RI) {
        x = n2 / (s2 > in.param ? s2 : in.param);
      } else if (Q == ST_EADY) {
        const double num = (0.31 * __builtin_fabs(fc)) * __builtin_sqrt(s2);
        const double e = num / __builtin_sqrt(n2);
        x = n2 > in.param ? e : 0.0;
      } else {
        double gxl[2], gyl[2], gxh[2], gyh[2];
        stab_gradients<CURV>(in, h, lo, w, k - 1, wall_s, wall_n, gxl, gyl);
        stab_gradients<CURV>(in, h, hi, w, k, wall_s, wall_n, gxh, gyh);
        const double bx = 0.25 * ((gxl[0] + gxl[1]) + (gxh[0] + gxh[1]));
        const double by = 0.25 * ((gyl[0] + gyl[1]) + (gyh[0] + gyh[1]));
        const double zl = (lo.z[0][0] + lo.z[0][1]) + (lo.z[1][0] + lo.z[1][1]);
        const double zh = (hi.z[0][0] + hi.z[0][1]) + (hi.z[1][0] + hi.z[1][1]);
        const double zb = 0.125 * (zl + zh);
        const double t1 = (fc + zb) * n2, t2 = du * by, t3 = dv * bx;
        x = t1 + (t2 - t3);
      }
      r = k > w.c ? (real)x : real(0);   // (faces at or below the lower face of the first wet cell: 0; a dry column: MOMENTS_DRY)
      lo = hi;
    }
    if (inside) d.out[der_out(d, i, j, kk)] = r;
  }
}

// c1 = (1 / pi) sum_k sqrt(max(N2(k), 0)) (zc(k) - zc(k-1)) over the wet interior faces, bottom to top
__global__ __launch_bounds__(256) void k_stability_wave_speed(Grid g, StabIn in, real* __restrict__ out, int bx, int by) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 64 + threadIdx.x;
  const int j = blockIdx.y * 4 + threadIdx.y;
  if (i >= bx || j >= by) return;
  const int Nz = g.Nz;
  const int kb = in.wet ? (int)in.wet[i2(g, i, j)] : 0;
  const double* zc = in.zt;
  double sum = 0.0;
  if (kb < Nz) {
    double sl = stab_sigma(in, der_off(g, g.pl_c, i, j, kb));
    for (int k = kb + 1; k < Nz; k++) {
      const double sh = stab_sigma(in, der_off(g, g.pl_c, i, j, k));
      const double dz = zc[k] - zc[k - 1];
      const double n2 = (in.ngr * (sh - sl)) / dz;
      const double term = __builtin_sqrt(n2 > 0.0 ? n2 : 0.0) * dz;
      sum = sum + term;
      sl = sh;
    }
  }
  out[(long long)i + (long long)bx * j] = (real)(sum / 3.141592653589793);
}

}  // namespace gb25
