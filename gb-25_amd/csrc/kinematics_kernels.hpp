// kinematics_kernels.hpp -- flow kinematics (gb25_compute_kinematics, gb25_get_kinematics, include/gb25.h): the horizontal velocity
// gradient beyond zeta -- divergence, normal and shear strain, the Okubo-Weiss parameter, the local Rossby number -- and the
// horizontal gradient of T, S or the potential density with the frontogenesis function.  Included by gb25_api.hip, launched from
// kinematics_host.hpp, ONE launch per request.
//
//   k_kinematics_corner<Q, CURV>             the two quantities at (f,f,c), the shear strain and zeta / f: the shape of
//                     k_derived_vorticity (diagnostics_kernels.hpp) -- a block is 64 x 4 threads, one wave = 64 consecutive i of one
//                     row, one thread per corner, KIN_LEVELS levels per block with the metrics loaded once.  No LDS.
//   k_kinematics_centre<Q, CURV, IMM, DENS>  the five quantities at (c,c,c).  A block is 64 x 4 threads and owns the 64 x 4 cells
//                     (i0 .., j0 ..); blockIdx.z runs over chunks of KIN_LEVELS requested levels.  What an instance stages is
//                     named by kin_flags(Q) (KinFlags below), so that an instance carries nothing it does not read:
//                       tile_uv   u and v of the level on the 66 x 6 tile (i0 - 1 .., j0 - 1 ..) in LDS, (double) of the stored
//                                 values, every point loaded ONCE per block and level;
//                       corners   s_s and zeta in fp64 at the 65 x 5 corners of the block's cells, each formed ONCE from the tile
//                                 (two divisions per corner instead of eight per cell) into a second pair of LDS tiles;
//                       tile_x    the tracer on the same 66 x 6 tile; with DENS the potential density is evaluated once per tile
//                                 point and level, never once per use, and never stored to memory;
//                       direct_uv the divergence and the normal strain alone read their four faces straight from memory: their
//                                 stencil has no ring, so nothing would be shared.
//                     CURV: the 2-D metrics of a curvilinear grid / the row tables of the LatitudeLongitudeGrid (that instance
//                     has no 2-D metric load).  IMM: the table of first wet levels with its ring (a grid without a bottom has the
//                     instance without the five loads and the tests).  The metrics and the first wet levels of a thread's cell,
//                     and of the (at most two) corners it forms, are loaded once per block, before the levels.
// Arithmetic: fp64 on (double) of the stored values with floating-point contraction OFF (the pragma is lexical: the density lives
// in its own function, compiled like k_derived_density), IEEE divisions and square roots, in the order include/gb25.h writes,
// rounded once to `real`: numpy restates it bit for bit (gb-25_amd/kinematics.py).  Every value is a function of its own stencil
// alone -- no sum runs across threads -- so the block shape changes no bit.  The result is PACKED: out[i + bx (j + by kk)], kk = 0 ..
// k_count - 1 for level k_first + kk; only the requested levels are computed and written.  Plain vector stores, one thread per
// element, no atomics, every offset into a 3-D array 64-bit.  Addresses of a partial block are clamped into the box plus its ring.
#pragma once

namespace gb25 {

enum KinKind { KIN_DIV = 0, KIN_NSTRAIN = 1, KIN_SSTRAIN = 2, KIN_OW = 3, KIN_RO = 4, KIN_GRAD = 5, KIN_FRONT = 6, KIN_COUNT = 7 };
constexpr int KIN_LEVELS = 4;                    // levels a block marches
constexpr int KIN_TX = 64, KIN_TY = 4;           // the block
constexpr int KIN_TW = KIN_TX + 2, KIN_TH = KIN_TY + 2, KIN_TILE = KIN_TW * KIN_TH;     // the tile with its one-point ring
constexpr int KIN_CW = KIN_TX + 1, KIN_CH = KIN_TY + 1, KIN_CORNERS = KIN_CW * KIN_CH;  // the corners of the block's cells
constexpr int KIN_CP = KIN_TW;                   // pitch of the corner tiles

// what an instance of k_kinematics_centre stages, by name
struct KinFlags {
  bool tile_uv, corners, zeta, tile_x, direct_uv;
};
constexpr KinFlags kin_flags(int Q) {
  return Q == KIN_OW      ? KinFlags{true, true, true, false, false}
         : Q == KIN_FRONT ? KinFlags{true, true, false, true, false}
         : Q == KIN_GRAD  ? KinFlags{false, false, false, true, false}
                          : KinFlags{false, false, false, false, true};
}

struct KinIn {
  const real *u, *v;               // parents; null where the instance does not read them
  const real *x, *S;               // the tracer (T or S); with DENS: T and S
  const double* eos0;              // the TEOS-10 table folded at Z = 0
  const unsigned short* wet;       // first wet level of the (c,c) columns AND of the ring of columns around the interior
                                   // (MOMENTS_DRY: none); null: every level is wet
  const real *azff, *fff;          // diagnostics' own tables of a curvilinear grid (null on the LatitudeLongitudeGrid)
  int jtop;                        // local row of the y faces beyond the last row of cells of the GLOBAL grid (a wall or the fold)
};

// the metrics of one corner: dy, dy' (of v(i), v(i-1)), dx, dx' (of u(j), u(j-1)), Az, f -- those of k_derived_vorticity
struct KinCornerMetrics {
  double dyc, dyw, dxc, dxs, az, f;
};
template <bool CURV>
__device__ __forceinline__ KinCornerMetrics kin_corner_metrics(const Grid& g, const KinIn& in, int i, int j, bool want_f) {
  KinCornerMetrics m;
  if (CURV) {
    const int o = i2(g, i, j);
    m.dyc = (double)g.cv.dycf[o];
    m.dyw = (double)g.cv.dycf[o - 1];
    m.dxc = (double)g.cv.dxfc[o];
    m.dxs = (double)g.cv.dxfc[o - g.sx];
    m.az = (double)in.azff[o];
    m.f = want_f ? (double)in.fff[o] : 0.0;
  } else {
    m.dyc = m.dyw = (double)g.dy;
    m.dxc = (double)g.dxc[j];
    m.dxs = (double)g.dxc[j - 1];
    m.az = (double)g.azf[j];
    m.f = want_f ? (double)g.fcor[j] : 0.0;
  }
  return m;
}
// s_s and zeta of one corner: the operands and the order of k_derived_vorticity, the inner sign apart
__device__ __forceinline__ void kin_corner_values(const KinCornerMetrics& m, double vc, double vw, double uc, double us, double* ss,
                                                  double* zeta) {
#pragma clang fp contract(off)
  const double a = m.dyc * vc, b = m.dyw * vw, c = m.dxc * uc, e = m.dxs * us;
  const double dv = a - b, du = c - e;
  const double s = (dv + du) / m.az, z = (dv - du) / m.az;
  *ss = m.az == 0.0 ? 0.0 : s;
  *zeta = m.az == 0.0 ? 0.0 : z;
}

// s_s (KIN_SSTRAIN) or zeta / f (KIN_RO) at (f,f,c); box = the interior of v
template <int Q, bool CURV>
__global__ __launch_bounds__(256) void k_kinematics_corner(Grid g, KinIn in, DerivedOut d) {
#pragma clang fp contract(off)
  static_assert(Q == KIN_SSTRAIN || Q == KIN_RO, "the corner quantities");
  const int i = blockIdx.x * KIN_TX + threadIdx.x;
  const int j = blockIdx.y * KIN_TY + __builtin_amdgcn_readfirstlane(threadIdx.y);
  if (j >= d.by) return;   // (the whole wave; the kernel has no barrier)
  const bool inside = i < d.bx;
  const int ii = inside ? i : d.bx - 1;   // (addresses stay in the box)
  const KinCornerMetrics m = kin_corner_metrics<CURV>(g, in, ii, j, Q == KIN_RO);
  const int kk0 = blockIdx.z * KIN_LEVELS;
  for (int q = 0; q < KIN_LEVELS && kk0 + q < d.k_count; q++) {
    const int k = d.k_first + kk0 + q;
    const long long ou = der_off(g, g.pl_c, ii, j, k), ov = der_off(g, g.pl_v, ii, j, k);
    double ss, zeta;
    kin_corner_values(m, (double)in.v[ov], (double)in.v[ov - 1], (double)in.u[ou], (double)in.u[ou - g.sx], &ss, &zeta);
    double r = ss;
    if (Q == KIN_RO) {
      const double ro = zeta / m.f;
      r = m.f == 0.0 ? 0.0 : ro;
    }
    if (inside) d.out[der_out(d, i, j, kk0 + q)] = (real)r;
  }
}

// the metrics of one cell: dy of its x faces i and i + 1 (DYFC), dx of its y faces j and j + 1 (DXCF), its area (AZCC); the
// spacings ACROSS its x faces i and i + 1 (DXFC) and across its y faces j and j + 1 (DYCF)
struct KinCellMetrics {
  double dyw, dye, dxs, dxn, az;
  double gxw, gxe, gys, gyn;
};
template <bool CURV>
__device__ __forceinline__ KinCellMetrics kin_cell_metrics(const Grid& g, int i, int j, bool strain, bool gradient) {
  KinCellMetrics m = {};
  if (CURV) {
    const int o = i2(g, i, j);
    if (strain) {
      m.dyw = (double)g.cv.dyfc[o];
      m.dye = (double)g.cv.dyfc[o + 1];
      m.dxs = (double)g.cv.dxcf[o];
      m.dxn = (double)g.cv.dxcf[o + g.sx];
      m.az = (double)g.cv.azcc[o];
    }
    if (gradient) {
      m.gxw = (double)g.cv.dxfc[o];
      m.gxe = (double)g.cv.dxfc[o + 1];
      m.gys = (double)g.cv.dycf[o];
      m.gyn = (double)g.cv.dycf[o + g.sx];
    }
  } else {
    if (strain) {
      m.dyw = m.dye = (double)g.dy;
      m.dxs = (double)g.dxf[j];
      m.dxn = (double)g.dxf[j + 1];
      m.az = (double)g.azc[j];
    }
    if (gradient) {
      m.gxw = m.gxe = (double)g.dxc[j];
      m.gys = m.gyn = (double)g.dy;
    }
  }
  return m;
}
// delta and s_n of one cell from its four faces
__device__ __forceinline__ void kin_cell_strain(const KinCellMetrics& m, double uw, double ue, double vs, double vn, double* delta,
                                                double* sn) {
#pragma clang fp contract(off)
  const double a = m.dye * ue, b = m.dyw * uw, c = m.dxn * vn, e = m.dxs * vs;
  const double ax = a - b, ay = c - e;
  const double dl = (ax + ay) / m.az, st = (ax - ay) / m.az;
  *delta = m.az == 0.0 ? 0.0 : dl;
  *sn = m.az == 0.0 ? 0.0 : st;
}
// a difference across one face; 0 where `open` is false
__device__ __forceinline__ double kin_face_difference(bool open, double x_far, double x_near, double d) {
#pragma clang fp contract(off)
  const double q = (x_far - x_near) / d;
  return open ? q : 0.0;
}
// the mean of the four corners of a cell
__device__ __forceinline__ double kin_corner_mean(double a00, double a10, double a01, double a11) {
#pragma clang fp contract(off)
  return 0.25 * ((a00 + a10) + (a01 + a11));
}

template <int Q, bool CURV, bool IMM, bool DENS>
__global__ __launch_bounds__(256) void k_kinematics_centre(Grid g, KinIn in, DerivedOut d) {
#pragma clang fp contract(off)
  constexpr KinFlags F = kin_flags(Q);
  static_assert(Q == KIN_DIV || Q == KIN_NSTRAIN || Q == KIN_OW || Q == KIN_GRAD || Q == KIN_FRONT, "the centre quantities");
  static_assert(F.tile_x || !DENS, "only the tracer instances evaluate the density");
  constexpr bool strain = F.tile_uv || F.direct_uv;
  __shared__ double tu[F.tile_uv ? KIN_TILE : 1], tv[F.tile_uv ? KIN_TILE : 1], tx[F.tile_x ? KIN_TILE : 1];
  __shared__ double cs[F.corners ? KIN_CP * KIN_CH : 1], cz[F.zeta ? KIN_CP * KIN_CH : 1];
  const int i0 = blockIdx.x * KIN_TX, j0 = blockIdx.y * KIN_TY;
  const int ty = __builtin_amdgcn_readfirstlane(threadIdx.y);
  const int tid = ty * KIN_TX + threadIdx.x;
  const int i = i0 + threadIdx.x, j = j0 + ty;
  const bool inside = i < d.bx && j < d.by;
  const int ii = i < d.bx ? i : d.bx - 1, jj = j < d.by ? j : d.by - 1;   // (addresses stay in the box and its ring)
  // once per block: the cell's metrics and first wet levels, the metrics of the corners this thread forms
  const KinCellMetrics cm = kin_cell_metrics<CURV>(g, ii, jj, strain, F.tile_x);
  int wc = 0, ww = 0, we = 0, ws = 0, wn = 0;
  if (IMM) {
    const int o = i2(g, ii, jj);
    wc = (int)in.wet[o];
    if (F.tile_x) {
      ww = (int)in.wet[o - 1];
      we = (int)in.wet[o + 1];
      ws = (int)in.wet[o - g.sx];
      wn = (int)in.wet[o + g.sx];
    }
  }
  const bool wall_s = jj == g.jws, wall_n = jj + 1 == in.jtop;
  KinCornerMetrics km[2] = {};
  if (F.corners) {
#pragma unroll
    for (int p = 0; p < 2; p++) {
      const int t = tid + 256 * p;
      if (t < KIN_CORNERS) {
        const int ci = i0 + t % KIN_CW, cj = j0 + t / KIN_CW;
        km[p] = kin_corner_metrics<CURV>(g, in, ci < d.bx ? ci : d.bx, cj < d.by ? cj : d.by, false);
      }
    }
  }
  const int kk0 = blockIdx.z * KIN_LEVELS;
  for (int q = 0; q < KIN_LEVELS && kk0 + q < d.k_count; q++) {   // (uniform over the block: every thread meets every barrier)
    const int k = d.k_first + kk0 + q;
    if (F.tile_uv || F.tile_x) {
      if (q) __syncthreads();   // (the last level's readers are done with the tiles)
      for (int t = tid; t < KIN_TILE; t += 256) {
        const int c = t % KIN_TW, r = t / KIN_TW;
        const int ti = i0 - 1 + c < d.bx ? i0 - 1 + c : d.bx, tj = j0 - 1 + r < d.by ? j0 - 1 + r : d.by;
        const long long oc = der_off(g, g.pl_c, ti, tj, k);
        if (F.tile_uv) {
          tu[t] = (double)in.u[oc];
          tv[t] = (double)in.v[der_off(g, g.pl_v, ti, tj, k)];
        }
        if (F.tile_x) tx[t] = DENS ? (double)(real)derived_density_value(in.eos0, in.x[oc], in.S[oc]) : (double)in.x[oc];
      }
      __syncthreads();
    }
    if (F.corners) {
#pragma unroll
      for (int p = 0; p < 2; p++) {
        const int t = tid + 256 * p;
        if (t < KIN_CORNERS) {
          const int c = t % KIN_CW, r = t / KIN_CW;   // corner (i0 + c, j0 + r): tile column c + 1, tile row r + 1
          double ss, zeta;
          kin_corner_values(km[p], tv[(r + 1) * KIN_TW + c + 1], tv[(r + 1) * KIN_TW + c], tu[(r + 1) * KIN_TW + c + 1],
                            tu[r * KIN_TW + c + 1], &ss, &zeta);
          cs[r * KIN_CP + c] = ss;
          if (F.zeta) cz[r * KIN_CP + c] = zeta;
        }
      }
      __syncthreads();
    }
    const int at = (ty + 1) * KIN_TW + threadIdx.x + 1;   // the cell on the tiles
    double delta = 0.0, sn = 0.0;
    if (F.tile_uv) kin_cell_strain(cm, tu[at], tu[at + 1], tv[at], tv[at + KIN_TW], &delta, &sn);
    if (F.direct_uv) {
      const long long ou = der_off(g, g.pl_c, ii, jj, k), ov = der_off(g, g.pl_v, ii, jj, k);
      kin_cell_strain(cm, (double)in.u[ou], (double)in.u[ou + 1], (double)in.v[ov], (double)in.v[ov + g.sx], &delta, &sn);
    }
    double gx = 0.0, gy = 0.0;
    if (F.tile_x) {
      const double xc = tx[at];
      const bool wet = k >= wc;
      const double dw = kin_face_difference(wet && k >= ww, xc, tx[at - 1], cm.gxw);
      const double de = kin_face_difference(wet && k >= we, tx[at + 1], xc, cm.gxe);
      const double ds = kin_face_difference(!wall_s && wet && k >= ws, xc, tx[at - KIN_TW], cm.gys);
      const double dn = kin_face_difference(!wall_n && wet && k >= wn, tx[at + KIN_TW], xc, cm.gyn);
      gx = 0.5 * (dw + de);
      gy = 0.5 * (ds + dn);
    }
    const int ca = ty * KIN_CP + threadIdx.x;   // the cell's south-western corner on the corner tiles
    double x;
    if (Q == KIN_DIV) {
      x = delta;
    } else if (Q == KIN_NSTRAIN) {
      x = sn;
    } else if (Q == KIN_OW) {
      const double s00 = cs[ca], s10 = cs[ca + 1], s01 = cs[ca + KIN_CP], s11 = cs[ca + KIN_CP + 1];
      const double z00 = cz[ca], z10 = cz[ca + 1], z01 = cz[ca + KIN_CP], z11 = cz[ca + KIN_CP + 1];
      const double ms = kin_corner_mean(s00 * s00, s10 * s10, s01 * s01, s11 * s11);
      const double mz = kin_corner_mean(z00 * z00, z10 * z10, z01 * z01, z11 * z11);
      const double n2 = sn * sn;
      const double w = (n2 + ms) - mz;
      x = cm.az == 0.0 ? 0.0 : w;
    } else if (Q == KIN_GRAD) {
      const double a = gx * gx, b = gy * gy;
      x = __builtin_sqrt(a + b);
    } else {
      const double ms = kin_corner_mean(cs[ca], cs[ca + 1], cs[ca + KIN_CP], cs[ca + KIN_CP + 1]);
      const double a1 = gx * gx, b1 = 0.5 * (delta + sn), t1 = a1 * b1;
      const double c2 = gx * gy, t2 = c2 * ms;
      const double a3 = gy * gy, b3 = 0.5 * (delta - sn), t3 = a3 * b3;
      const double f = -((t1 + t2) + t3);
      x = cm.az == 0.0 ? 0.0 : f;
    }
    if (inside) d.out[der_out(d, i, j, kk0 + q)] = k >= wc ? (real)x : real(0);   // (an immersed cell: 0)
  }
}

}  // namespace gb25
