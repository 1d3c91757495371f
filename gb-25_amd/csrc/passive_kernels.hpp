// passive_kernels.hpp -- the device side of the passive tracers carried beside a run (gb25_tracers_*, include/gb25.h; host:
// passive_host.hpp).  The advective tendency of a passive tracer is the one-tracer kernel's (k_tracer_tendencies_single,
// tendency_kernels.hpp); what is new here is k_passive_update: the quasi-AB2 update of EVERY tracer of a set in one launch, with
// the source, the surface reset, the clip, the zeros of immersed cells and the halo cells the next tendency reads.
// gb-25_amd/passive.py (passive_update_host) restates it in numpy bit for bit: no fused multiply-add, in the written order.
#pragma once
#include "device_common.hpp"

namespace gb25 {

constexpr int PASSIVE_MAX = 8;   // (GB25_TRACERS_MAX, include/gb25.h)

struct PassiveArgs {
  real* c[PASSIVE_MAX];
  const real* Gn[PASSIVE_MAX];
  const real* Gm[PASSIVE_MAX];
  real source[PASSIVE_MAX], surface[PASSIVE_MAX];   // dt * source; the value of the top level
  int reset[PASSIVE_MAX], clip[PASSIVE_MAX];
  real dt, C1, C2;   // C1 = 1.5 + chi, C2 = 0.5 + chi (an Euler step: 1 and 0)
  int count;
  int fold;          // the rows beyond a zipper fold are images; else row Ny is the layer beyond a wall
};

// One thread per interior cell (i, j, k) of tracer blockIdx.z / Nz.  The thread writes its cell AND every halo cell that is an
// image of it, as the FOLD variants of the model's producers do -- no cell is written by two threads, none is read by another:
//   the layer beyond the southern wall (row -1 <- row 0), beyond the northern wall (row Ny <- row Ny - 1) unless it is the fold line,
//   the layer below the bottom (level -1 <- level 0) and above the top (level Nz <- level Nz - 1) of interior rows,
//   on a folded grid cell (Nx - 1 - i, Ny - 1 + q) <- cell (i, Ny - 1 - q), q = 1 .. H, with its bottom / top layer,
//   and of each of those the periodic x images (column a < H also at a + Nx, column a >= Nx - H also at a - Nx).
// UPDATE = false: nothing is advanced -- the mask and the halo cells of what the host has set (gb25_tracers_set).
// grid: (ceil(Nx / 64), ceil(Ny / 4), Nz * count), block (64, 4)
template <bool IMM, bool UPDATE>
__global__ __launch_bounds__(256) void k_passive_update(Grid g, PassiveArgs A) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y * 4 + threadIdx.y;
  const int n = (int)blockIdx.z / g.Nz, k = (int)blockIdx.z - n * g.Nz;
  if (i >= g.Nx || j >= g.Ny || n >= A.count) return;
  real* __restrict__ c = A.c[n];
  const long o = (long)(i + g.H) + (long)g.sx * (j + g.H) + (long)g.pl_c * (k + g.H);
  real x = c[o];
  if (UPDATE) {
    const real t = A.C1 * A.Gn[n][o] - A.C2 * A.Gm[n][o];
    x = (x + A.dt * t) + A.source[n];
    if (A.reset[n] && k == g.Nz - 1) x = A.surface[n];
    if (A.clip[n]) x = x < real(0.) ? real(0.) : x;   // (a NaN stays a NaN)
  }
  if (IMM && k < (int)(g.im.ordA[i2(g, i, j)] & 255u)) x = real(0.);
  const bool bottom = k == 0, top = k == g.Nz - 1;
  // a value, its bottom / top layer and the periodic x images of all three, at the cell of column a whose offset is at
  auto put = [&](long at, int a) {
    const bool xw = a < g.H, xe = a >= g.Nx - g.H;
    for (int l = -1; l <= 1; l++) {
      if ((l < 0 && !bottom) || (l > 0 && !top)) continue;
      const long p = at + (long)l * g.pl_c;
      c[p] = x;
      if (xw) c[p + g.Nx] = x;
      if (xe) c[p - g.Nx] = x;
    }
  };
  put(o, i);
  // (the layers beyond the walls hold interior levels only, as the model's fills leave them: no bottom / top layer of theirs)
  auto put_row = [&](long at) {
    c[at] = x;
    if (i < g.H) c[at + g.Nx] = x;
    if (i >= g.Nx - g.H) c[at - g.Nx] = x;
  };
  if (j == 0) put_row(o - g.sx);
  if (A.fold) {
    const int q = g.Ny - 1 - j;
    if (q >= 1 && q <= g.H) {
      const int a = g.Nx - 1 - i;
      put(o + (long)(a - i) + (long)g.sx * (2 * q), a);
    }
  } else if (j == g.Ny - 1) {
    put_row(o + g.sx);
  }
}

}  // namespace gb25
