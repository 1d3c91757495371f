// zonal_eddy_host.hpp -- host side of gb25_get_zonal_eddy / gb25_zonal_eddy_dims / gb25_zonal_eddy_bytes (include/gb25.h); included
// by gb25_api.hip behind diagnostics_host.hpp, whose shared helpers (diag_*) and tables (moments_tables, diag_measure_tables) it
// uses.  Kernel: zonal_eddy_kernels.hpp; the memory: zonal_eddy (a result buffer) of DiagState (diagnostics_state.hpp).  Like the
// other diagnostics nothing here writes model memory or a schedule flag: the only memory written is the records' own buffer.
#pragma once

namespace {

static_assert(sizeof(ZonalEddyRecord) == sizeof(gb25_zonal_eddy_row), "a line record is a gb25_zonal_eddy_row");
static_assert(ZE_VARS == GB25_ZE_COUNT && ZE_CO == GB25_ZE_COUNT * (GB25_ZE_COUNT + 1) / 2, "the kernels' counts are the header's");

// the records [kc][Ny] of one call, then the caller's means [kc][Ny][6]
inline ZonalEddyRecord* zonal_eddy_records(gb25_model* m) { return (ZonalEddyRecord*)m->diag.zonal_eddy.p; }
inline double* zonal_eddy_means(gb25_model* m, size_t lines) { return (double*)(zonal_eddy_records(m) + lines); }

}  // namespace

extern "C" {

int32_t gb25_zonal_eddy_bytes(void) { return (int32_t)sizeof(gb25_zonal_eddy_row); }

gb25_status gb25_zonal_eddy_dims(const gb25_model* m, int32_t dims[2]) {
  if (!m || !dims) return GB25_ERR_INVALID_ARGUMENT;
  dims[0] = m->Ny;
  dims[1] = m->cfg.Nz;
  return GB25_OK;
}

gb25_status gb25_get_zonal_eddy(gb25_model* m, int32_t k_first, int32_t k_count, const double* means, gb25_zonal_eddy_row* out) {
  if (!m) return GB25_ERR_INVALID_ARGUMENT;
  const char* what = "gb25_get_zonal_eddy";
  if (!out) return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: out is NULL", what);
  int kc = 0;
  if (gb25_status s = diag_window(m, what, k_first, k_count, m->cfg.Nz, "levels (k_first, k_count)", &kc)) return s;
  const size_t lines = (size_t)kc * m->Ny;
  if (means)
    for (size_t n = 0; n < lines * ZE_VARS; n++)
      if (!std::isfinite(means[n]))
        return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: every entry of means must be finite; variable %d of row %d of level %d of the window is %g",
                    what, (int)(n % ZE_VARS), (int)((n / ZE_VARS) % m->Ny), (int)(n / ZE_VARS / m->Ny), means[n]);
  if (gb25_status s = diag_need_device(m, what)) return s;
  ZonalEddyIn in = {};
  if (gb25_status s = diag_source(m, GB25_U, &in.u)) return s;
  if (gb25_status s = diag_source(m, GB25_V, &in.v)) return s;
  if (gb25_status s = diag_source(m, GB25_W, &in.w)) return s;
  if (gb25_status s = diag_source(m, GB25_T, &in.T)) return s;
  if (gb25_status s = diag_source(m, GB25_S, &in.S)) return s;
  if (gb25_status s = m->diag.zonal_eddy.grow(m, what, "the zonal-eddy records", lines * (sizeof(ZonalEddyRecord) + ZE_VARS * sizeof(double))))
    return s;
  if (gb25_status s = wait_for_model(m)) return s;
  if (gb25_status s = moments_tables(m)) return s;
  if (means) {   // (the caller's array is alive until the stream is synchronised below)
    HIPCHK(hipMemcpyAsync(zonal_eddy_means(m, lines), means, lines * ZE_VARS * sizeof(double), hipMemcpyHostToDevice, m->stream));
    in.means = zonal_eddy_means(m, lines);
  }
  in.eos0 = m->diag.eos0;
  in.by = m->Ny;
  in.k_first = k_first;
  in.k_count = kc;
  const MomentsTables tab = diag_measure_tables(m, true);
  ZonalEddyRecord* rec = zonal_eddy_records(m);
  {
    Timed t(m, GB25_K_DIAGNOSTICS);
    const dim3 grd((unsigned)((lines + DIAG_THREADS / 64 - 1) / (DIAG_THREADS / 64))), blk(DIAG_THREADS);
    const bool curv = tab.area[0] != nullptr, imm = tab.first[0] != nullptr;
    if (curv && imm) hipLaunchKernelGGL((k_zonal_eddy<true, true>), grd, blk, 0, m->stream, m->g, tab, in, rec);
    else if (curv) hipLaunchKernelGGL((k_zonal_eddy<true, false>), grd, blk, 0, m->stream, m->g, tab, in, rec);
    else if (imm) hipLaunchKernelGGL((k_zonal_eddy<false, true>), grd, blk, 0, m->stream, m->g, tab, in, rec);
    else hipLaunchKernelGGL((k_zonal_eddy<false, false>), grd, blk, 0, m->stream, m->g, tab, in, rec);
    LAUNCHCHK();
  }
  return diag_download(m, out, rec, lines * sizeof(gb25_zonal_eddy_row));
}

}  // extern "C"
