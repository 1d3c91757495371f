// stability_host.hpp -- host side of gb25_stability_dims / gb25_compute_stability / gb25_get_stability / gb25_get_stability_stats
// (include/gb25.h); included by gb25_api.hip behind diagnostics_host.hpp, whose shared helpers (diag_*) and tables
// (moments_tables: the first wet levels with their ring, (double) zc | zf, AZFF and the Coriolis parameter of a curvilinear grid)
// it uses.  Kernels: stability_kernels.hpp; the memory: stability of DiagState (diagnostics_state.hpp).  Like the other
// diagnostics nothing here writes model memory or a schedule flag: the only memory written is the results' own buffer.
#pragma once

namespace {

// (the kernels' ids, written as ints: two enumerations do not compare)
static_assert((int)ST_COUNT == (int)GB25_ST_COUNT && (int)ST_N2 == (int)GB25_ST_N2 && (int)ST_SHEAR2 == (int)GB25_ST_SHEAR2 &&
                  (int)ST_RI == (int)GB25_ST_RICHARDSON && (int)ST_EADY == (int)GB25_ST_EADY_RATE && (int)ST_PV == (int)GB25_ST_ERTEL_PV &&
                  (int)ST_WAVE == (int)GB25_ST_WAVE_SPEED, "the kernels' ids are the header's");

// extents of a stability diagnostic, from the configuration alone (no device)
void stability_extents(const gb25_model* m, gb25_stability q, int32_t d[3]) {
  d[0] = m->Nx;
  d[1] = m->Ny;
  d[2] = q == GB25_ST_WAVE_SPEED ? 1 : m->cfg.Nz + 1;
}
gb25_status stability_check(gb25_model* m, const char* what, gb25_stability q, double param) {
  if (q < 0 || q >= GB25_ST_COUNT) return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: no stability diagnostic %d (0 .. %d)", what, (int)q, GB25_ST_COUNT - 1);
  if (q == GB25_ST_RICHARDSON && !(param > 0.0))
    return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: the Richardson number needs a floor > 0 s^-2 on the squared shear as param, got %g", what, param);
  if (q == GB25_ST_EADY_RATE && !(param >= 0.0))
    return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: the Eady growth rate needs a floor >= 0 s^-2 on N^2 as param, got %g", what, param);
  return GB25_OK;
}
// once per model: room for the largest result, Nx x Ny x (Nz + 1)
gb25_status stability_buffer(gb25_model* m, const char* what) {
  DiagState& D = m->diag;
  if (D.stability) return GB25_OK;
  const size_t bytes = (size_t)m->Nx * m->Ny * ((size_t)m->cfg.Nz + 1) * sizeof(real);
  if (gb25_status s = diag_room_for(m, what, "the result array", (double)bytes)) return s;
  HIPCHK(hipMalloc(&D.stability, bytes));
  return GB25_OK;
}

template <int Q>
void stability_launch(gb25_model* m, const dim3& grd, const StabIn& in, const DerivedOut& d) {
  const dim3 blk(64, 4);
  if (m->g.cv.on) hipLaunchKernelGGL((k_stability_faces<Q, true>), grd, blk, 0, m->stream, m->g, in, d);
  else hipLaunchKernelGGL((k_stability_faces<Q, false>), grd, blk, 0, m->stream, m->g, in, d);
}

// The launch of one diagnostic, faces [k0, k0 + kc), on m->stream behind the model; the packed result lies at m->diag.stability
// when the stream has run.
gb25_status stability_run(gb25_model* m, const char* what, gb25_stability q, double param, int k0, int kc) {
  StabIn in = {};
  if (q != GB25_ST_SHEAR2) {
    if (gb25_status s = diag_source(m, GB25_T, &in.T)) return s;
    if (gb25_status s = diag_source(m, GB25_S, &in.S)) return s;
  }
  if (q != GB25_ST_N2 && q != GB25_ST_WAVE_SPEED) {
    if (gb25_status s = diag_source(m, GB25_U, &in.u)) return s;
    if (gb25_status s = diag_source(m, GB25_V, &in.v)) return s;
  }
  if (gb25_status s = stability_buffer(m, what)) return s;
  if (gb25_status s = wait_for_model(m)) return s;
  if (gb25_status s = moments_tables(m)) return s;
  const DiagState& D = m->diag;
  in.eos0 = D.eos0;
  in.wet = D.first_wet_ring;
  in.zt = D.zt;
  in.azff = D.azff;
  in.fff = D.fff;
  in.ngr = -(m->cfg.g / m->cfg.rho0);
  in.param = param;
  in.jtop = m->cfg.Ny - m->j0;
  Timed t(m, GB25_K_DIAGNOSTICS);
  if (q == GB25_ST_WAVE_SPEED) {
    hipLaunchKernelGGL(k_stability_wave_speed, dim3((m->Nx + 63) / 64, (m->Ny + 3) / 4), dim3(64, 4), 0, m->stream, m->g, in, D.stability,
                       m->Nx, m->Ny);
  } else {
    const DerivedOut d{D.stability, m->Nx, m->Ny, k0, kc};
    const dim3 grd((m->Nx + 63) / 64, (m->Ny + 3) / 4, (kc + STAB_FACES - 1) / STAB_FACES);
    switch (q) {
      case GB25_ST_N2: stability_launch<ST_N2>(m, grd, in, d); break;
      case GB25_ST_SHEAR2: stability_launch<ST_SHEAR2>(m, grd, in, d); break;
      case GB25_ST_RICHARDSON: stability_launch<ST_RI>(m, grd, in, d); break;
      case GB25_ST_EADY_RATE: stability_launch<ST_EADY>(m, grd, in, d); break;
      default: stability_launch<ST_PV>(m, grd, in, d); break;
    }
  }
  LAUNCHCHK();
  return GB25_OK;
}

// What gb25_compute_stability and gb25_get_stability share: the checks, the window of faces, the launch.  e: the packed dims
// of the result (e[2]: the faces of the window).
gb25_status stability_window_run(gb25_model* m, const char* what, gb25_stability q, double param, int32_t k_first, int32_t k_count,
                                 int32_t e[3]) {
  if (gb25_status s = stability_check(m, what, q, param)) return s;
  int kc = 0;
  stability_extents(m, q, e);
  if (gb25_status s = diag_window(m, what, k_first, k_count, e[2], "faces (k_first, k_count)", &kc)) return s;
  if (gb25_status s = diag_need_device(m, what)) return s;
  if (gb25_status s = stability_run(m, what, q, param, k_first, kc)) return s;
  e[2] = kc;
  return GB25_OK;
}

}  // namespace

extern "C" {

gb25_status gb25_stability_dims(const gb25_model* m, gb25_stability q, int32_t dims[3]) {
  if (!m || !dims || q < 0 || q >= GB25_ST_COUNT) return GB25_ERR_INVALID_ARGUMENT;
  stability_extents(m, q, dims);
  return GB25_OK;
}

gb25_status gb25_compute_stability(gb25_model* m, gb25_stability q, double param, int32_t k_first, int32_t k_count, const void** dev,
                                   int32_t device_dims[3]) {
  if (!m) return GB25_ERR_INVALID_ARGUMENT;
  if (!dev) return fail(m, GB25_ERR_INVALID_ARGUMENT, "gb25_compute_stability: dev is NULL");
  int32_t e[3];
  if (gb25_status s = stability_window_run(m, "gb25_compute_stability", q, param, k_first, k_count, e)) return s;
  HIPCHK(hipStreamSynchronize(m->stream));
  *dev = m->diag.stability;
  if (device_dims) memcpy(device_dims, e, sizeof e);
  return GB25_OK;
}

gb25_status gb25_get_stability(gb25_model* m, gb25_stability q, double param, int32_t k_first, int32_t k_count, void* host) {
  if (!m) return GB25_ERR_INVALID_ARGUMENT;
  if (!host) return fail(m, GB25_ERR_INVALID_ARGUMENT, "gb25_get_stability: host is NULL");
  int32_t e[3];
  if (gb25_status s = stability_window_run(m, "gb25_get_stability", q, param, k_first, k_count, e)) return s;
  return diag_download(m, host, m->diag.stability, (size_t)e[0] * e[1] * e[2] * sizeof(real));
}

gb25_status gb25_get_stability_stats(gb25_model* m, gb25_stability q, double param, gb25_field_stats* out) {
  if (!m) return GB25_ERR_INVALID_ARGUMENT;
  if (!out) return fail(m, GB25_ERR_INVALID_ARGUMENT, "gb25_get_stability_stats: out is NULL");
  if (gb25_status s = stability_check(m, "gb25_get_stability_stats", q, param)) return s;
  if (gb25_status s = diag_need_device(m, "gb25_get_stability_stats")) return s;
  int32_t e[3];
  stability_extents(m, q, e);
  const DiagBox b{e[0], e[1], e[2], (long long)e[0], (long long)e[0] * e[1], 0};
  if (gb25_status s = diag_scratch(m)) return s;
  if (gb25_status s = diag_check_box(m, b)) return s;
  if (gb25_status s = stability_run(m, "gb25_get_stability_stats", q, param, 0, e[2])) return s;
  return diag_stats_of(m, GB25_T, m->diag.stability, b, 0, out);   // (interior: the offsets are those of any field of the rank, 0 in k)
}

}  // extern "C"
