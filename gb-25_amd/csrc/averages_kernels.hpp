// averages_kernels.hpp -- time averages and eddy fluxes accumulated on the device (gb25_averages_*, include/gb25.h): the running sums
// acc = acc + weight * term of u, v, w, T, S, eta (MEANS), their squares (SQUARES) and the products u T, u S, v T, v S, w T, w S at
// the faces (FLUXES).  Definitions: include/gb25.h.  Every term is fp64 on (double) of the stored values with floating-point
// contraction OFF (every product and sum rounds by itself; weight * term and the addition are two roundings):
// gb-25_amd/averages.py restates them with numpy bit for bit.
//
// ONE LAUNCH PER SAMPLE, k_averages_accumulate<GROUPS, VW>.  A block is 64 x 4 threads; a lane owns VW adjacent i of one row j
// (VW = 2 where Nx and the halo are even: every parent row and every packed accumulator row then starts on a multiple of two elements, so the
// inputs are one 8-byte (Float32) or 16-byte (Float64) load and the read-modify-write of an accumulator is one 16-byte load and
// one 16-byte store per lane; VW = 1 otherwise) and marches AVG_LEVELS faces of the window upwards, carrying T(k-1), S(k-1) in
// registers for the z fluxes (the first face of a chunk loads them once more: 1/AVG_LEVELS of a field, from the cache the chunk
// below filled).  The tile covers the largest box -- the rows of v (Ny + 1 below a wall), the faces of w (k_count + 1) -- and
// every quantity is guarded by its own dims.  u, v, w, T, S are loaded once per cell; the western tracer neighbour is one more
// element per lane out of the line the neighbouring lane loads, the southern one is the row the wave below loads (three of four
// rows inside the block): cache hits, no second pass.  Each active accumulator is read once and written once.  GROUPS is a
// template parameter, so an inactive group costs no instruction and no register.  eta and its square ride on the blocks of the
// first chunk.  Plain vector loads and stores, no atomics, every offset into a 3-D array 64-bit.
//
// GB25_AVG_NONTEMPORAL = 1 compiles the accumulator accesses as non-temporal loads and stores (the A/B of DESIGN.md).
#pragma once

#ifndef GB25_AVG_NONTEMPORAL
#define GB25_AVG_NONTEMPORAL 0
#endif

namespace gb25 {

constexpr int AVG_LEVELS = 8;

struct AvgArgs {
  double* acc[GB25_A_COUNT];   // packed interior arrays, i fastest; null: the quantity's group is not active
  const real *u, *v, *w, *T, *S, *eta;
  double weight;
  int bx, by, byv;             // columns; rows of cells; rows of y faces (>= by)
  int k_first, k_count;        // the window of cell levels; faces k_first .. k_first + k_count
  int Nz, H, sx, pl_c, pl_v;   // levels of the model, halo, row pitch, plane strides of the parents ((c,c) rows; (c,f) rows)
};

template <int VW> struct AvgVec;
template <> struct AvgVec<1> {
  using D = double;
  using R = real;
};
template <> struct AvgVec<2> {
  using D = double __attribute__((ext_vector_type(2)));
  using R = real __attribute__((ext_vector_type(2)));
};
__device__ __forceinline__ double avg_widen(real x) { return (double)x; }
__device__ __forceinline__ AvgVec<2>::D avg_widen(AvgVec<2>::R x) {
  AvgVec<2>::D d;
  d.x = (double)x.x;
  d.y = (double)x.y;
  return d;
}
// VW stored values from p, as double
template <int VW>
__device__ __forceinline__ typename AvgVec<VW>::D avg_load(const real* p) {
  return avg_widen(*reinterpret_cast<const typename AvgVec<VW>::R*>(p));
}
// the values one element to the west of x = (p[0], p[1]): (p[-1], p[0])
__device__ __forceinline__ double avg_west(const real* p, double) { return (double)p[-1]; }
__device__ __forceinline__ AvgVec<2>::D avg_west(const real* p, AvgVec<2>::D x) {
  AvgVec<2>::D d;
  d.x = (double)p[-1];
  d.y = x.x;
  return d;
}
// acc[q] = acc[q] + weight * term[q] at element `off` of N accumulators of one location: two roundings per element.  All N loads
// are issued ahead of the first store (the compiler may not move a load above a store that could alias it).
template <int N, class D>
__device__ __forceinline__ void avg_add(double* const (&acc)[N], long long off, double weight, const D (&term)[N]) {
#pragma clang fp contract(off)
  D old[N];
#pragma unroll
  for (int q = 0; q < N; q++) {
    D* p = reinterpret_cast<D*>(acc[q] + off);
#if GB25_AVG_NONTEMPORAL
    old[q] = __builtin_nontemporal_load(p);
#else
    old[q] = *p;
#endif
  }
#pragma unroll
  for (int q = 0; q < N; q++) {
    D* p = reinterpret_cast<D*>(acc[q] + off);
    const D add = weight * term[q];
    const D sum = old[q] + add;
#if GB25_AVG_NONTEMPORAL
    __builtin_nontemporal_store(sum, p);
#else
    *p = sum;
#endif
  }
}

template <int GROUPS, int VW>
__global__ __launch_bounds__(256) void k_averages_accumulate(AvgArgs a) {
#pragma clang fp contract(off)
  using D = typename AvgVec<VW>::D;
  constexpr bool SQ = (GROUPS & GB25_AVG_SQUARES) != 0, FL = (GROUPS & GB25_AVG_FLUXES) != 0;
  constexpr int NE = 1 + SQ, NV = 1 + SQ + 2 * FL, NC = 3 + 3 * SQ + 2 * FL, NW = 1 + 2 * FL;   // accumulators by location
  const int i = (blockIdx.x * 64 + threadIdx.x) * VW;
  const int j = blockIdx.y * 4 + __builtin_amdgcn_readfirstlane(threadIdx.y);
  if (i >= a.bx || j >= a.byv) return;   // (bx is even where VW = 2: i + 1 is inside as well)
  const bool cells = j < a.by;           // (false: the wall row of v alone)
  const double weight = a.weight;
  const long long row = (long long)(i + a.H) + (long long)a.sx * (j + a.H);
  const long long out_c = (long long)i + (long long)a.bx * j;   // into a plane of bx x by; the planes of v have byv rows
  const long long plane_out_c = (long long)a.bx * a.by, plane_out_v = (long long)a.bx * a.byv;
  // the accumulators of a location, in the order of the terms below (the counts are compile-time: NE, NV, NC, NW)
  double *acc_e[2], *acc_v[4], *acc_c[8], *acc_w[3];
  {
    int n = 0;
    acc_e[n++] = a.acc[GB25_A_ETA];
    if (SQ) acc_e[n++] = a.acc[GB25_A_ETAETA];
    n = 0;
    acc_v[n++] = a.acc[GB25_A_V];
    if (SQ) acc_v[n++] = a.acc[GB25_A_VV];
    if (FL) {
      acc_v[n++] = a.acc[GB25_A_VT];
      acc_v[n++] = a.acc[GB25_A_VS];
    }
    n = 0;
    acc_c[n++] = a.acc[GB25_A_U];
    acc_c[n++] = a.acc[GB25_A_T];
    acc_c[n++] = a.acc[GB25_A_S];
    if (SQ) {
      acc_c[n++] = a.acc[GB25_A_UU];
      acc_c[n++] = a.acc[GB25_A_TT];
      acc_c[n++] = a.acc[GB25_A_SS];
    }
    if (FL) {
      acc_c[n++] = a.acc[GB25_A_UT];
      acc_c[n++] = a.acc[GB25_A_US];
    }
    n = 0;
    acc_w[n++] = a.acc[GB25_A_W];
    if (FL) {
      acc_w[n++] = a.acc[GB25_A_WT];
      acc_w[n++] = a.acc[GB25_A_WS];
    }
  }

  if (blockIdx.z == 0 && cells) {
    const D e = avg_load<VW>(a.eta + row);
    const D te[2] = {e, e * e};
    avg_add(reinterpret_cast<double* const(&)[NE]>(acc_e), out_c, weight, reinterpret_cast<const D(&)[NE]>(te));
  }

  const int f0 = a.k_first + blockIdx.z * AVG_LEVELS, top = a.k_first + a.k_count;   // faces [f0, fend) of k_first .. top
  const int fend = f0 + AVG_LEVELS < top + 1 ? f0 + AVG_LEVELS : top + 1;
  const D zero = 0.0;
  D Tm = zero, Sm = zero;   // T, S of the level below
  if (FL && cells && f0 >= 1) {
    const long long o = row + (long long)a.pl_c * (f0 - 1 + a.H);
    Tm = avg_load<VW>(a.T + o);
    Sm = avg_load<VW>(a.S + o);
  }
  for (int kf = f0; kf < fend; kf++) {
    const int kk = kf - a.k_first;
    const bool level = kf < top;                        // a cell level of the window (the last face has none)
    const bool zflux = FL && kf >= 1 && kf < a.Nz;      // an interior face: bottom and top carry exactly 0
    const long long oc = row + (long long)a.pl_c * (kf + a.H), ov = row + (long long)a.pl_v * (kf + a.H);
    // every input of the level ahead of the first accumulator
    D Tc = zero, Sc = zero, Ts = zero, Ss = zero, Tw = zero, Sw = zero, uc = zero, vc = zero, wc = zero;
    if ((level && (cells || FL)) || (zflux && cells)) {   // (never a halo level: kf < Nz here)
      Tc = avg_load<VW>(a.T + oc);
      Sc = avg_load<VW>(a.S + oc);
    }
    if (level) {
      vc = avg_load<VW>(a.v + ov);
      if (FL) {
        Ts = avg_load<VW>(a.T + oc - a.sx);
        Ss = avg_load<VW>(a.S + oc - a.sx);
      }
      if (cells) {
        uc = avg_load<VW>(a.u + oc);
        if (FL) {
          Tw = avg_west(a.T + oc, Tc);
          Sw = avg_west(a.S + oc, Sc);
        }
      }
    }
    if (cells) wc = avg_load<VW>(a.w + oc);

    if (level) {
      D tv[4];
      int n = 0;
      tv[n++] = vc;
      if (SQ) tv[n++] = vc * vc;
      if (FL) {
        const D tm = 0.5 * (Ts + Tc), sm = 0.5 * (Ss + Sc);
        tv[n++] = vc * tm;
        tv[n++] = vc * sm;
      }
      avg_add(reinterpret_cast<double* const(&)[NV]>(acc_v), out_c + plane_out_v * kk, weight, reinterpret_cast<const D(&)[NV]>(tv));
      if (cells) {
        D tc[8];
        n = 0;
        tc[n++] = uc;
        tc[n++] = Tc;
        tc[n++] = Sc;
        if (SQ) {
          tc[n++] = uc * uc;
          tc[n++] = Tc * Tc;
          tc[n++] = Sc * Sc;
        }
        if (FL) {
          const D tm = 0.5 * (Tw + Tc), sm = 0.5 * (Sw + Sc);
          tc[n++] = uc * tm;
          tc[n++] = uc * sm;
        }
        avg_add(reinterpret_cast<double* const(&)[NC]>(acc_c), out_c + plane_out_c * kk, weight,
                reinterpret_cast<const D(&)[NC]>(tc));
      }
    }
    if (cells) {   // (c,c,f): k_count + 1 planes of bx x by
      D tw[3] = {wc, zero, zero};
      if (zflux) {
        const D tm = 0.5 * (Tm + Tc), sm = 0.5 * (Sm + Sc);
        tw[1] = wc * tm;
        tw[2] = wc * sm;
      }
      avg_add(reinterpret_cast<double* const(&)[NW]>(acc_w), out_c + plane_out_c * kk, weight, reinterpret_cast<const D(&)[NW]>(tw));
    }
    Tm = Tc;
    Sm = Sc;
  }
}

// out = acc / weight_sum, one IEEE division per element (gb25_get_average, normalized)
__global__ __launch_bounds__(256) void k_averages_normalize(const double* __restrict__ acc, double weight_sum, double* __restrict__ out,
                                                            long long n) {
  const long long o = (long long)blockIdx.x * 256 + threadIdx.x;
  if (o < n) out[o] = acc[o] / weight_sum;
}

}  // namespace gb25
