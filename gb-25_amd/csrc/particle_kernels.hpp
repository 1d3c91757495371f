// particle_kernels.hpp -- Lagrangian particles advected and sampled on the device (gb25_particles_*, include/gb25.h, which states the
// position, the rate, the midpoint substep, the re-celling and the boundary rules; gb-25_amd/particles.py restates them with numpy
// bit for bit).  All of the arithmetic is fp64 on (double) of the stored values with floating-point contraction OFF, IEEE
// divisions by the metrics as `real` widened (the numbers gb25_get_metric / gb25_get_metric2 return), in the written order.
//
// k_particles_advance<CURV>: ONE LAUNCH PER CALL.  One lane per particle, structure-of-arrays state; a lane loads its particle,
// makes `substeps` midpoint substeps in registers and stores it into the OTHER copy of the state (the host exchanges the copies
// when the call is accepted: a refused call has moved nothing).  The kernel is bound by the latency of its gathers, not by
// arithmetic: a rate evaluation computes its three offsets first and issues the six velocity loads and the metric loads
// back to back ahead of the first use; the two kbot loads of a move go out together.  The counters are reduced per wave by
// shuffles and lane 0 stores them to the wave's slot with ordinary vector stores; k_particles_fold adds the slots (integers: the
// sum has no order).  No atomics at all.  Every cell index is clamped into the parent arrays before it enters an address.
//
// k_particles_sample: the value of a (c,c,c) field in each particle's cell, widened to double: a copy, no arithmetic.
#pragma once

namespace gb25 {

constexpr int PART_BLOCK = 256;
constexpr double PART_BELOW_ONE = 0x1.fffffffffffffp-1;   // the largest double below 1
constexpr double PART_FAR = 1073741824.0;                 // 2^30 cells: a displacement not below it counts as not finite
enum : unsigned { PART_EV_BLOCKED = 1, PART_EV_CLAMPED_Y = 2, PART_EV_CLAMPED_Z = 4, PART_EV_TOO_FAR = 8 };

struct PartState {
  int *i, *j, *k, *status;
  double *a, *b, *c;
};

struct PartArgs {
  PartState in, out;
  const real *u, *v, *w;
  const real *dxu;       // CURV: DXFC, parent layout of a (c,f) 2-D field; else DXC by j (index 0 = the first interior row)
  const real *dyv;       // CURV: DYCF; else unused (dy)
  const real *dzc;       // by k (index 0 = the first interior level)
  const int* kbot;       // first wet level of every column the parent holds, parent layout of a (c,f) 2-D field
  unsigned* slots;       // [wave][GB25_PC_COUNT]
  double dy, h;
  long long n;
  int substeps;
  int Nx, Ny, Nz, H, sx, pl_c, pl_v;
  int x_periodic;        // 1: i wraps modulo Nx; 0: a particle may leave in x (a neighbour owns the halo columns)
  int j_south, j_north;  // rows [j_south, j_north) are allowed: the global walls (the pivot row is the last one on a folded grid)
  int fold;              // 1: the last row of this rank is the pivot row of a folded grid
};

struct PartPos {
  int i, j, k;
  double a, b, c;
};
struct PartRate {
  double x, y, z;
};

__device__ __forceinline__ int part_clamp(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }

template <bool CURV>
__device__ __forceinline__ PartRate part_rate(const PartArgs& A, const PartPos& p) {
#pragma clang fp contract(off)
  const int H = A.H;
  const int ic = part_clamp(p.i, -H, A.Nx + H - 2), jc = part_clamp(p.j, -H, A.Ny + H - 2), kc = part_clamp(p.k, -H, A.Nz + H - 2);
  const int o2 = (ic + H) + A.sx * (jc + H);
  const long long oc = o2 + (long long)A.pl_c * (kc + H), ov = o2 + (long long)A.pl_v * (kc + H);
  // the gathers, all of them ahead of the first use
  const real u0 = A.u[oc], u1 = A.u[oc + 1];
  const real v0 = A.v[ov], v1 = A.v[ov + A.sx];
  const real w0 = A.w[oc], w1 = A.w[oc + A.pl_c];
  real dx0, dx1, dy0, dy1;
  if (CURV) {
    dx0 = A.dxu[o2]; dx1 = A.dxu[o2 + 1];
    dy0 = A.dyv[o2]; dy1 = A.dyv[o2 + A.sx];
  } else {
    dx0 = dx1 = A.dxu[jc];
  }
  const double dz = (double)A.dzc[kc];
  const double y0 = CURV ? (double)dy0 : A.dy, y1 = CURV ? (double)dy1 : A.dy;
  PartRate r;
  r.x = (1.0 - p.a) * ((double)u0 / (double)dx0) + p.a * ((double)u1 / (double)dx1);
  r.y = (1.0 - p.b) * ((double)v0 / y0) + p.b * ((double)v1 / y1);
  r.z = ((1.0 - p.c) * (double)w0 + p.c * (double)w1) / dz;
  return r;
}

__device__ __forceinline__ void part_recell(int& i, double& a, double d) {
#pragma clang fp contract(off)
  double x = a + d;
  const double n = __builtin_floor(x);
  i += (int)n;           // (|d| < 2^30 and a cell index within a few cells of the rank: no overflow)
  x = x - n;
  if (x >= 1.0) {
    i += 1;
    x = 0.0;
  }
  a = x;
}

__device__ __forceinline__ int part_kbot(const PartArgs& A, int i, int j) {
  return A.kbot[(part_clamp(i, -A.H, A.Nx + A.H - 1) + A.H) + A.sx * (part_clamp(j, -A.H, A.Ny + A.H) + A.H)];
}

// move(p, d) of include/gb25.h; returns the events
__device__ __forceinline__ unsigned part_move(const PartArgs& A, const PartPos& p, double dx, double dy, double dz, PartPos& q) {
  unsigned ev = 0;
  q = p;
  part_recell(q.i, q.a, dx);
  part_recell(q.j, q.b, dy);
  part_recell(q.k, q.c, dz);
  if (A.x_periodic) {
    q.i %= A.Nx;
    if (q.i < 0) q.i += A.Nx;
  }
  if (q.j < A.j_south) {
    q.j = A.j_south; q.b = 0.0; ev |= PART_EV_CLAMPED_Y;
  } else if (q.j >= A.j_north) {
    q.j = A.j_north - 1; q.b = PART_BELOW_ONE; ev |= PART_EV_CLAMPED_Y;
  }
  const int kb0 = part_kbot(A, p.i, p.j), kb1 = part_kbot(A, q.i, q.j);
  if (q.k < kb0) {
    q.k = kb0; q.c = 0.0; ev |= PART_EV_CLAMPED_Z;
  }
  if (q.k >= A.Nz) {
    q.k = A.Nz - 1; q.c = PART_BELOW_ONE; ev |= PART_EV_CLAMPED_Z;
  }
  if (kb1 > q.k) {
    q.i = p.i; q.j = p.j; q.a = p.a; q.b = p.b; ev |= PART_EV_BLOCKED;
  }
  if (q.i < -1 || q.i > A.Nx || q.j < -1 || q.j > A.Ny) ev |= PART_EV_TOO_FAR;
  return ev;
}

__device__ __forceinline__ bool part_small(double x, double y, double z) {
  return __builtin_fabs(x) < PART_FAR && __builtin_fabs(y) < PART_FAR && __builtin_fabs(z) < PART_FAR;   // (false for a NaN)
}

__device__ __forceinline__ unsigned part_wave_sum(unsigned x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
  return x;
}

template <bool CURV>
__global__ __launch_bounds__(PART_BLOCK) void k_particles_advance(const PartArgs A) {
#pragma clang fp contract(off)
  const long long n = (long long)blockIdx.x * PART_BLOCK + threadIdx.x;
  const bool live = n < A.n;
  PartPos p = {0, 0, 0, 0.0, 0.0, 0.0};
  int status = GB25_PARTICLE_OUTSIDE;   // (a lane beyond the last particle does nothing)
  if (live) {
    p.i = A.in.i[n]; p.j = A.in.j[n]; p.k = A.in.k[n];
    p.a = A.in.a[n]; p.b = A.in.b[n]; p.c = A.in.c[n];
    status = A.in.status[n];
  }
  unsigned cnt[GB25_PC_COUNT] = {};
  const double hh = 0.5 * A.h;
  for (int s = 0; s < A.substeps; s++) {
    if (status != GB25_PARTICLE_ACTIVE) break;
    if (A.fold && (p.j > A.Ny - 1 || (p.j == A.Ny - 1 && p.b >= 0.5))) {   // (set there, or handed over there)
      status = GB25_PARTICLE_AT_FOLD;
      cnt[GB25_PC_AT_FOLD]++;
      break;
    }
    const PartRate r0 = part_rate<CURV>(A, p);
    const double d0x = hh * r0.x, d0y = hh * r0.y, d0z = hh * r0.z;
    if (!part_small(d0x, d0y, d0z)) {
      status = GB25_PARTICLE_NONFINITE;
      cnt[GB25_PC_NONFINITE]++;
      break;
    }
    PartPos pm, q;
    const unsigned evm = part_move(A, p, d0x, d0y, d0z, pm);
    const PartRate r1 = part_rate<CURV>(A, pm);
    const double d1x = A.h * r1.x, d1y = A.h * r1.y, d1z = A.h * r1.z;
    if (!part_small(d1x, d1y, d1z)) {
      status = GB25_PARTICLE_NONFINITE;
      cnt[GB25_PC_NONFINITE]++;
      break;
    }
    const unsigned ev = part_move(A, p, d1x, d1y, d1z, q);
    if ((ev | evm) & PART_EV_TOO_FAR) {   // (the host refuses the call: nothing of it is kept)
      cnt[GB25_PC_TOO_FAR] = 1;
      break;
    }
    p = q;
    cnt[GB25_PC_BLOCKED] += (ev & PART_EV_BLOCKED) ? 1u : 0u;
    cnt[GB25_PC_CLAMPED_Y] += (ev & PART_EV_CLAMPED_Y) ? 1u : 0u;
    cnt[GB25_PC_CLAMPED_Z] += (ev & PART_EV_CLAMPED_Z) ? 1u : 0u;
    if (A.fold && p.j == A.Ny - 1 && p.b >= 0.5) {
      status = GB25_PARTICLE_AT_FOLD;
      cnt[GB25_PC_AT_FOLD]++;
    } else if (p.i < 0 || p.i >= A.Nx || p.j < 0 || p.j >= A.Ny) {
      status = GB25_PARTICLE_OUTSIDE;
      cnt[GB25_PC_OUTSIDE]++;
    }
  }
  if (live) {
    A.out.i[n] = p.i; A.out.j[n] = p.j; A.out.k[n] = p.k;
    A.out.a[n] = p.a; A.out.b[n] = p.b; A.out.c[n] = p.c;
    A.out.status[n] = status;
  }
  // per wave: lane 0 stores the wave's sums to its slot (whole waves run: the block is a multiple of 64 lanes)
  const long long wave = ((long long)blockIdx.x * PART_BLOCK + threadIdx.x) >> 6;
#pragma unroll
  for (int q = 0; q < GB25_PC_COUNT; q++) {
    const unsigned s = part_wave_sum(cnt[q]);
    if ((threadIdx.x & 63) == 0) A.slots[wave * GB25_PC_COUNT + q] = s;
  }
}

// totals[q] = the sum of slot q of every wave; one block
__global__ __launch_bounds__(PART_BLOCK) void k_particles_fold(const unsigned* slots, long long waves, unsigned long long* totals) {
  __shared__ unsigned long long part[PART_BLOCK / 64][GB25_PC_COUNT];
  unsigned long long s[GB25_PC_COUNT] = {};
  for (long long wv = threadIdx.x; wv < waves; wv += PART_BLOCK)
#pragma unroll
    for (int q = 0; q < GB25_PC_COUNT; q++) s[q] += slots[wv * GB25_PC_COUNT + q];
#pragma unroll
  for (int q = 0; q < GB25_PC_COUNT; q++) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s[q] += __shfl_down(s[q], off, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][q] = s[q];
  }
  __syncthreads();
  if (threadIdx.x < GB25_PC_COUNT) {
    unsigned long long t = 0;
    for (int wv = 0; wv < PART_BLOCK / 64; wv++) t += part[wv][threadIdx.x];
    totals[threadIdx.x] = t;
  }
}

// out[n] = (double) f(i, j, k) of particle n's cell, the indices clamped into the parent
__global__ __launch_bounds__(PART_BLOCK) void k_particles_sample(const PartState P, const real* f, double* out, long long count, int Nx,
                                                                 int Ny, int Nz, int H, int sx, int pl_c) {
  const long long n = (long long)blockIdx.x * PART_BLOCK + threadIdx.x;
  if (n >= count) return;
  const int ic = part_clamp(P.i[n], -H, Nx + H - 1), jc = part_clamp(P.j[n], -H, Ny + H - 1), kc = part_clamp(P.k[n], -H, Nz + H - 1);
  out[n] = (double)f[(ic + H) + sx * (jc + H) + (long long)pl_c * (kc + H)];
}

}  // namespace gb25
