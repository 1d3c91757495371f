// kinematics_host.hpp -- host side of gb25_kinematics_dims / gb25_compute_kinematics / gb25_get_kinematics / gb25_get_kinematics_stats
// (include/gb25.h); included by gb25_api.hip behind diagnostics_host.hpp, whose shared helpers (diag_*), tables (moments_tables: the
// first wet levels with their ring, AZFF and the Coriolis parameter of a curvilinear grid) and result array (derived_scratch: the
// 3-D part of the derived fields' array, room for the largest interior a field has) it uses.  Kernels: kinematics_kernels.hpp.  Like
// the other diagnostics nothing here writes model memory or a schedule flag: the only memory written is the result array.
#pragma once

namespace {

// (the kernels' ids, written as ints: two enumerations do not compare)
static_assert((int)KIN_COUNT == (int)GB25_KIN_COUNT && (int)KIN_DIV == (int)GB25_KIN_DIVERGENCE && (int)KIN_NSTRAIN == (int)GB25_KIN_NORMAL_STRAIN &&
                  (int)KIN_SSTRAIN == (int)GB25_KIN_SHEAR_STRAIN && (int)KIN_OW == (int)GB25_KIN_OKUBO_WEISS &&
                  (int)KIN_RO == (int)GB25_KIN_ROSSBY_NUMBER && (int)KIN_GRAD == (int)GB25_KIN_GRADIENT &&
                  (int)KIN_FRONT == (int)GB25_KIN_FRONTOGENESIS, "the kernels' ids are the header's");

inline bool kinematics_at_corners(gb25_kinematics q) { return q == GB25_KIN_SHEAR_STRAIN || q == GB25_KIN_ROSSBY_NUMBER; }
inline bool kinematics_of_a_tracer(gb25_kinematics q) { return q == GB25_KIN_GRADIENT || q == GB25_KIN_FRONTOGENESIS; }

// extents of a quantity, from the configuration alone (no device): the corner quantities have the rows of v, as the vorticity has
void kinematics_extents(const gb25_model* m, gb25_kinematics q, int32_t d[3]) {
  d[0] = m->Nx;
  d[1] = m->Ny + ((kinematics_at_corners(q) && has_north_wall(m)) ? 1 : 0);
  d[2] = m->cfg.Nz;
}
gb25_status kinematics_check(gb25_model* m, const char* what, gb25_kinematics q, int32_t param) {
  if (q < 0 || q >= GB25_KIN_COUNT) return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: no kinematics quantity %d (0 .. %d)", what, (int)q, GB25_KIN_COUNT - 1);
  if (kinematics_of_a_tracer(q) && (param < 0 || param > 2))
    return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: param selects the tracer of the gradient: 0 = T, 1 = S, 2 = the potential density, got %d", what, (int)param);
  if (!kinematics_of_a_tracer(q) && param != 0)
    return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: param is the tracer of the gradient and of the frontogenesis function; quantity %d takes 0, got %d",
                what, (int)q, (int)param);
  return GB25_OK;
}

template <int Q, bool DENS>
void kinematics_launch_centre(gb25_model* m, const dim3& grd, const KinIn& in, const DerivedOut& d) {
  const dim3 blk(KIN_TX, KIN_TY);
  const bool curv = m->g.cv.on, imm = in.wet != nullptr;
  if (curv && imm) hipLaunchKernelGGL((k_kinematics_centre<Q, true, true, DENS>), grd, blk, 0, m->stream, m->g, in, d);
  else if (curv) hipLaunchKernelGGL((k_kinematics_centre<Q, true, false, DENS>), grd, blk, 0, m->stream, m->g, in, d);
  else if (imm) hipLaunchKernelGGL((k_kinematics_centre<Q, false, true, DENS>), grd, blk, 0, m->stream, m->g, in, d);
  else hipLaunchKernelGGL((k_kinematics_centre<Q, false, false, DENS>), grd, blk, 0, m->stream, m->g, in, d);
}
template <int Q>
void kinematics_launch_corner(gb25_model* m, const dim3& grd, const KinIn& in, const DerivedOut& d) {
  const dim3 blk(KIN_TX, KIN_TY);
  if (m->g.cv.on) hipLaunchKernelGGL((k_kinematics_corner<Q, true>), grd, blk, 0, m->stream, m->g, in, d);
  else hipLaunchKernelGGL((k_kinematics_corner<Q, false>), grd, blk, 0, m->stream, m->g, in, d);
}

// The ONE launch of a quantity, levels [k0, k0 + kc), on m->stream behind the model; *result: where the packed result lies when
// the stream has run.
gb25_status kinematics_run(gb25_model* m, gb25_kinematics q, int32_t param, int k0, int kc, const real** result) {
  KinIn in = {};
  if (q != GB25_KIN_GRADIENT) {
    if (gb25_status s = diag_source(m, GB25_U, &in.u)) return s;
    if (gb25_status s = diag_source(m, GB25_V, &in.v)) return s;
  }
  const bool dens = kinematics_of_a_tracer(q) && param == 2;
  if (kinematics_of_a_tracer(q)) {
    if (gb25_status s = diag_source(m, param == 1 ? GB25_S : GB25_T, &in.x)) return s;
    if (dens)
      if (gb25_status s = diag_source(m, GB25_S, &in.S)) return s;
  }
  if (gb25_status s = derived_scratch(m)) return s;
  if (gb25_status s = wait_for_model(m)) return s;
  if (gb25_status s = moments_tables(m)) return s;
  const DiagState& D = m->diag;
  in.eos0 = D.eos0;
  in.wet = D.first_wet_ring;
  in.azff = D.azff;
  in.fff = D.fff;
  in.jtop = m->cfg.Ny - m->j0;
  int32_t e[3];
  kinematics_extents(m, q, e);
  real* out = m->diag.derived + m->diag.derived_plane;
  const DerivedOut d{out, e[0], e[1], k0, kc};
  const dim3 grd((e[0] + KIN_TX - 1) / KIN_TX, (e[1] + KIN_TY - 1) / KIN_TY, (kc + KIN_LEVELS - 1) / KIN_LEVELS);
  Timed t(m, GB25_K_DIAGNOSTICS);
  switch (q) {
    case GB25_KIN_DIVERGENCE: kinematics_launch_centre<KIN_DIV, false>(m, grd, in, d); break;
    case GB25_KIN_NORMAL_STRAIN: kinematics_launch_centre<KIN_NSTRAIN, false>(m, grd, in, d); break;
    case GB25_KIN_SHEAR_STRAIN: kinematics_launch_corner<KIN_SSTRAIN>(m, grd, in, d); break;
    case GB25_KIN_OKUBO_WEISS: kinematics_launch_centre<KIN_OW, false>(m, grd, in, d); break;
    case GB25_KIN_ROSSBY_NUMBER: kinematics_launch_corner<KIN_RO>(m, grd, in, d); break;
    case GB25_KIN_GRADIENT:
      if (dens) kinematics_launch_centre<KIN_GRAD, true>(m, grd, in, d);
      else kinematics_launch_centre<KIN_GRAD, false>(m, grd, in, d);
      break;
    default:
      if (dens) kinematics_launch_centre<KIN_FRONT, true>(m, grd, in, d);
      else kinematics_launch_centre<KIN_FRONT, false>(m, grd, in, d);
      break;
  }
  LAUNCHCHK();
  *result = out;
  return GB25_OK;
}

// What gb25_compute_kinematics and gb25_get_kinematics share: the checks, the window of levels, the launch.  e: the packed dims
// of the result (e[2]: the levels of the window).
gb25_status kinematics_window_run(gb25_model* m, const char* what, gb25_kinematics q, int32_t param, int32_t k_first, int32_t k_count,
                                  int32_t e[3], const real** result) {
  if (gb25_status s = kinematics_check(m, what, q, param)) return s;
  int kc = 0;
  kinematics_extents(m, q, e);
  if (gb25_status s = diag_window(m, what, k_first, k_count, e[2], "levels (k_first, k_count)", &kc)) return s;
  if (gb25_status s = diag_need_device(m, what)) return s;
  if (gb25_status s = kinematics_run(m, q, param, k_first, kc, result)) return s;
  e[2] = kc;
  return GB25_OK;
}

}  // namespace

extern "C" {

gb25_status gb25_kinematics_dims(const gb25_model* m, gb25_kinematics q, int32_t dims[3]) {
  if (!m || !dims || q < 0 || q >= GB25_KIN_COUNT) return GB25_ERR_INVALID_ARGUMENT;
  kinematics_extents(m, q, dims);
  return GB25_OK;
}

gb25_status gb25_compute_kinematics(gb25_model* m, gb25_kinematics q, int32_t param, int32_t k_first, int32_t k_count, const void** dev,
                                    int32_t device_dims[3]) {
  if (!m) return GB25_ERR_INVALID_ARGUMENT;
  if (!dev) return fail(m, GB25_ERR_INVALID_ARGUMENT, "gb25_compute_kinematics: dev is NULL");
  int32_t e[3];
  const real* result = nullptr;
  if (gb25_status s = kinematics_window_run(m, "gb25_compute_kinematics", q, param, k_first, k_count, e, &result)) return s;
  HIPCHK(hipStreamSynchronize(m->stream));
  *dev = result;
  if (device_dims) memcpy(device_dims, e, sizeof e);
  return GB25_OK;
}

gb25_status gb25_get_kinematics(gb25_model* m, gb25_kinematics q, int32_t param, int32_t k_first, int32_t k_count, void* host) {
  if (!m) return GB25_ERR_INVALID_ARGUMENT;
  if (!host) return fail(m, GB25_ERR_INVALID_ARGUMENT, "gb25_get_kinematics: host is NULL");
  int32_t e[3];
  const real* result = nullptr;
  if (gb25_status s = kinematics_window_run(m, "gb25_get_kinematics", q, param, k_first, k_count, e, &result)) return s;
  return diag_download(m, host, result, (size_t)e[0] * e[1] * e[2] * sizeof(real));
}

gb25_status gb25_get_kinematics_stats(gb25_model* m, gb25_kinematics q, int32_t param, gb25_field_stats* out) {
  if (!m) return GB25_ERR_INVALID_ARGUMENT;
  if (!out) return fail(m, GB25_ERR_INVALID_ARGUMENT, "gb25_get_kinematics_stats: out is NULL");
  if (gb25_status s = kinematics_check(m, "gb25_get_kinematics_stats", q, param)) return s;
  if (gb25_status s = diag_need_device(m, "gb25_get_kinematics_stats")) return s;
  int32_t e[3];
  kinematics_extents(m, q, e);
  const DiagBox b{e[0], e[1], e[2], (long long)e[0], (long long)e[0] * e[1], 0};
  if (gb25_status s = diag_scratch(m)) return s;
  if (gb25_status s = diag_check_box(m, b)) return s;
  const real* result = nullptr;
  if (gb25_status s = kinematics_run(m, q, param, 0, e[2], &result)) return s;
  // (interior: the offsets are those of a field of the rank at the quantity's location, 0 in k)
  return diag_stats_of(m, kinematics_at_corners(q) ? GB25_V : GB25_T, result, b, 0, out);
}

}  // extern "C"
