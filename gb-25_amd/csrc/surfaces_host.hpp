// surfaces_host.hpp -- host side of gb25_compute_on_surfaces / gb25_get_on_surfaces (include/gb25.h); included by gb25_api.hip
// behind diagnostics_host.hpp, whose shared helpers (diag_*) and tables (moments_tables: first wet levels, (double) zc | zf) it
// uses.  Kernel: surface_kernels.hpp; the memory: surfaces (a result buffer), surf_targets of DiagState (diagnostics_state.hpp).  Like the other
// diagnostics nothing here writes model memory or a schedule flag: the only memory written is the results' own buffer.
#pragma once

namespace {

static_assert(SURF_MAX == GB25_SURFACE_MAX_VALUES, "the kernels' cap is the header's");
// (the kernels' ids, written as ints: two enumerations do not compare)
static_assert((int)SV_COUNT == (int)GB25_SV_COUNT && (int)SC_COUNT == (int)GB25_SC_COUNT, "the kernels' ids are the header's");
static_assert((int)SV_T == (int)GB25_SV_T && (int)SV_S == (int)GB25_SV_S && (int)SV_SIGMA == (int)GB25_SV_POTENTIAL_DENSITY &&
                  (int)SV_DEPTH == (int)GB25_SV_DEPTH, "search variables");
static_assert((int)SC_DEPTH == (int)GB25_SC_DEPTH && (int)SC_T == (int)GB25_SC_T && (int)SC_S == (int)GB25_SC_S && (int)SC_E == (int)GB25_SC_E &&
                  (int)SC_KE == (int)GB25_SC_KINETIC_ENERGY && (int)SC_RHO == (int)GB25_SC_DENSITY_ANOMALY &&
                  (int)SC_SIGMA == (int)GB25_SC_POTENTIAL_DENSITY, "carried quantities");
static_assert((int)SURF_FOUND == (int)GB25_SURF_FOUND && (int)SURF_OUTCROP == (int)GB25_SURF_OUTCROP && (int)SURF_GROUNDED == (int)GB25_SURF_GROUNDED &&
                  (int)SURF_DRY == (int)GB25_SURF_DRY, "status bytes");

// the padded targets, then the values [Nx Ny n] and the status bytes [Nx Ny n]
gb25_status surfaces_buffer(gb25_model* m, const char* what, int n) {
  const size_t elems = (size_t)m->Nx * m->Ny * n;
  return m->diag.surfaces.grow(m, what, "the values and status bytes", SURF_MAX * sizeof(double) + elems * (sizeof(real) + 1));
}
inline double* surfaces_targets(gb25_model* m) { return (double*)m->diag.surfaces.p; }
// (the status bytes lie behind the values of the CALL's n: the two arrays are packed, whatever the buffer has room for)
inline real* surfaces_values(gb25_model* m) { return (real*)(surfaces_targets(m) + SURF_MAX); }

template <int SV>
void surfaces_launch_carried(gb25_model* m, int carried, const dim3& grd, const SurfIn& in, const SurfOut& out) {
  const dim3 blk(64, 4);
  switch (carried) {
    case GB25_SC_DEPTH: hipLaunchKernelGGL((k_on_surfaces<SV, SC_DEPTH>), grd, blk, 0, m->stream, m->g, in, out); break;
    case GB25_SC_T: hipLaunchKernelGGL((k_on_surfaces<SV, SC_T>), grd, blk, 0, m->stream, m->g, in, out); break;
    case GB25_SC_S: hipLaunchKernelGGL((k_on_surfaces<SV, SC_S>), grd, blk, 0, m->stream, m->g, in, out); break;
    case GB25_SC_E: hipLaunchKernelGGL((k_on_surfaces<SV, SC_E>), grd, blk, 0, m->stream, m->g, in, out); break;
    case GB25_SC_KINETIC_ENERGY: hipLaunchKernelGGL((k_on_surfaces<SV, SC_KE>), grd, blk, 0, m->stream, m->g, in, out); break;
    case GB25_SC_DENSITY_ANOMALY: hipLaunchKernelGGL((k_on_surfaces<SV, SC_RHO>), grd, blk, 0, m->stream, m->g, in, out); break;
    default: hipLaunchKernelGGL((k_on_surfaces<SV, SC_SIGMA>), grd, blk, 0, m->stream, m->g, in, out); break;
  }
}

// What the two entry points share: the checks, the parents, the buffer, the upload of the targets, the launch.  The results lie
// at surfaces_values and behind them, packed Nx x Ny x n, when the stream has run.
gb25_status surfaces_run(gb25_model* m, const char* what, gb25_surface_variable v, gb25_surface_carried c, const double* values, int32_t n) {
  if (v < 0 || v >= GB25_SV_COUNT) return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: no search variable %d (0 .. %d)", what, (int)v, GB25_SV_COUNT - 1);
  if (c < 0 || c >= GB25_SC_COUNT) return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: no carried quantity %d (0 .. %d)", what, (int)c, GB25_SC_COUNT - 1);
  if (n < 1 || n > GB25_SURFACE_MAX_VALUES)
    return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: %d values, must be 1 .. %d", what, (int)n, GB25_SURFACE_MAX_VALUES);
  if (!values) return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: values is NULL", what);
  for (int t = 0; t < n; t++)
    if (!std::isfinite(values[t])) return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: the values must be finite (value %d is %g)", what, t, values[t]);
  if (c == GB25_SC_E && !m->catke)
    return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: carried GB25_SC_E needs closure = CATKEVerticalDiffusivity(): this model has no e", what);
  if (gb25_status s = diag_need_device(m, what)) return s;
  const bool sigma = v == GB25_SV_POTENTIAL_DENSITY || c == GB25_SC_DENSITY_ANOMALY || c == GB25_SC_POTENTIAL_DENSITY;
  SurfIn in = {};
  if (sigma || v == GB25_SV_T || c == GB25_SC_T)
    if (gb25_status s = diag_source(m, GB25_T, &in.T)) return s;
  if (sigma || v == GB25_SV_S || c == GB25_SC_S)
    if (gb25_status s = diag_source(m, GB25_S, &in.S)) return s;
  if (c == GB25_SC_KINETIC_ENERGY) {
    if (gb25_status s = diag_source(m, GB25_U, &in.u)) return s;
    if (gb25_status s = diag_source(m, GB25_V, &in.v)) return s;
  }
  if (c == GB25_SC_E)
    if (gb25_status s = diag_source(m, GB25_E, &in.e)) return s;
  if (gb25_status s = surfaces_buffer(m, what, n)) return s;
  if (gb25_status s = wait_for_model(m)) return s;
  if (gb25_status s = moments_tables(m)) return s;
  DiagState& D = m->diag;
  for (int t = 0; t < SURF_MAX; t++) D.surf_targets[t] = t < n ? values[t] : (double)NAN;
  HIPCHK(hipMemcpyAsync(surfaces_targets(m), D.surf_targets, sizeof D.surf_targets, hipMemcpyHostToDevice, m->stream));
  in.eos0 = D.eos0;
  in.first_wet = D.first_wet[0];
  in.zt = D.zt;
  in.targets = surfaces_targets(m);
  real* val = surfaces_values(m);
  const SurfOut out = {val, (unsigned char*)(val + (size_t)m->Nx * m->Ny * n), m->Nx, m->Ny, (int)n};
  const dim3 grd((m->Nx + 63) / 64, (m->Ny + 3) / 4, (n + SURF_TG - 1) / SURF_TG);
  Timed t(m, GB25_K_DIAGNOSTICS);
  switch (v) {
    case GB25_SV_T: surfaces_launch_carried<SV_T>(m, (int)c, grd, in, out); break;
    case GB25_SV_S: surfaces_launch_carried<SV_S>(m, (int)c, grd, in, out); break;
    case GB25_SV_POTENTIAL_DENSITY: surfaces_launch_carried<SV_SIGMA>(m, (int)c, grd, in, out); break;
    default: surfaces_launch_carried<SV_DEPTH>(m, (int)c, grd, in, out); break;
  }
  LAUNCHCHK();
  return GB25_OK;
}

}  // namespace

extern "C" {

gb25_status gb25_compute_on_surfaces(gb25_model* m, gb25_surface_variable v, gb25_surface_carried c, const double* values, int32_t n,
                                     const void** dev, const uint8_t** dev_status, int32_t device_dims[3]) {
  if (!m) return GB25_ERR_INVALID_ARGUMENT;
  if (!dev) return fail(m, GB25_ERR_INVALID_ARGUMENT, "gb25_compute_on_surfaces: dev is NULL");
  if (gb25_status s = surfaces_run(m, "gb25_compute_on_surfaces", v, c, values, n)) return s;
  HIPCHK(hipStreamSynchronize(m->stream));
  const real* val = surfaces_values(m);
  *dev = val;
  if (dev_status) *dev_status = (const uint8_t*)(val + (size_t)m->Nx * m->Ny * n);
  if (device_dims) device_dims[0] = m->Nx, device_dims[1] = m->Ny, device_dims[2] = n;
  return GB25_OK;
}

gb25_status gb25_get_on_surfaces(gb25_model* m, gb25_surface_variable v, gb25_surface_carried c, const double* values, int32_t n,
                                 void* host, uint8_t* host_status) {
  if (!m) return GB25_ERR_INVALID_ARGUMENT;
  if (!host) return fail(m, GB25_ERR_INVALID_ARGUMENT, "gb25_get_on_surfaces: host is NULL");
  if (gb25_status s = surfaces_run(m, "gb25_get_on_surfaces", v, c, values, n)) return s;
  const size_t elems = (size_t)m->Nx * m->Ny * n;
  const real* val = surfaces_values(m);
  if (host_status) HIPCHK(hipMemcpyAsync(host_status, val + elems, elems, hipMemcpyDeviceToHost, m->stream));
  return diag_download(m, host, val, elems * sizeof(real));
}

}  // extern "C"
