// averages_host.hpp -- host side of gb25_averages_begin / gb25_averages_accumulate / gb25_averages_get_info / gb25_average_dims /
// gb25_get_average / gb25_average_device_ptr / gb25_averages_end (include/gb25.h); included by gb25_api.hip behind
// diagnostics_host.hpp, whose shared helpers (diag_*) it uses.  Kernels: averages_kernels.hpp; the memory: the avg_* members of
// DiagState (diagnostics_state.hpp), freed by its release_averages().  Like the other diagnostics nothing here writes model
// memory or a schedule flag: the only memory written is the accumulators' own allocation.
#pragma once

namespace {

inline int avg_group_of(int q) { return q <= GB25_A_ETA ? GB25_AVG_MEANS : q <= GB25_A_ETAETA ? GB25_AVG_SQUARES : GB25_AVG_FLUXES; }

// packed dims of quantity q for a window of kc cell levels, from the configuration alone (no device)
void avg_extents(const gb25_model* m, int q, int kc, int32_t d[3]) {
  d[0] = m->Nx;
  d[1] = m->Ny;
  d[2] = kc;
  switch (q) {
    case GB25_A_V: case GB25_A_VV: case GB25_A_VT: case GB25_A_VS: d[1] = m->Ny + (has_north_wall(m) ? 1 : 0); break;
    case GB25_A_W: case GB25_A_WT: case GB25_A_WS: d[2] = kc + 1; break;
    case GB25_A_ETA: case GB25_A_ETAETA: d[2] = 1; break;
    default: break;
  }
}
inline size_t avg_elems(const gb25_model* m, int q, int kc) {
  int32_t d[3];
  avg_extents(m, q, kc, d);
  return (size_t)d[0] * d[1] * d[2];
}

template <int VW>
void averages_launch(gb25_model* m, const AvgArgs& a, dim3 grd) {
  const dim3 blk(64, 4);
  switch (m->diag.avg_info.groups) {
    case GB25_AVG_MEANS:
      hipLaunchKernelGGL((k_averages_accumulate<GB25_AVG_MEANS, VW>), grd, blk, 0, m->stream, a);
      break;
    case GB25_AVG_MEANS | GB25_AVG_SQUARES:
      hipLaunchKernelGGL((k_averages_accumulate<GB25_AVG_MEANS | GB25_AVG_SQUARES, VW>), grd, blk, 0, m->stream, a);
      break;
    case GB25_AVG_MEANS | GB25_AVG_FLUXES:
      hipLaunchKernelGGL((k_averages_accumulate<GB25_AVG_MEANS | GB25_AVG_FLUXES, VW>), grd, blk, 0, m->stream, a);
      break;
    default:
      hipLaunchKernelGGL((k_averages_accumulate<GB25_AVG_MEANS | GB25_AVG_SQUARES | GB25_AVG_FLUXES, VW>), grd, blk, 0, m->stream, a);
      break;
  }
}

gb25_status averages_quantity(gb25_model* m, const char* what, gb25_average q) {
  if (q < 0 || q >= GB25_A_COUNT) return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: no average %d (0 .. %d)", what, (int)q, GB25_A_COUNT - 1);
  if (!m->diag.avg_on) return fail(m, GB25_ERR_STATE, "%s: no averages are being accumulated (call gb25_averages_begin first)", what);
  if (!(m->diag.avg_info.groups & avg_group_of(q)))
    return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: average %d belongs to group %d, which gb25_averages_begin was not asked for (groups = %d)",
                what, (int)q, avg_group_of(q), (int)m->diag.avg_info.groups);
  return GB25_OK;
}

}  // namespace

extern "C" {

int32_t gb25_averages_info_bytes(void) { return (int32_t)sizeof(gb25_averages_info); }

gb25_status gb25_averages_begin(gb25_model* m, int32_t groups, int32_t k_first, int32_t k_count) {
  if (!m) return GB25_ERR_INVALID_ARGUMENT;
  const int all = GB25_AVG_MEANS | GB25_AVG_SQUARES | GB25_AVG_FLUXES;
  if (groups <= 0 || (groups & ~all) || !(groups & GB25_AVG_MEANS))
    return fail(m, GB25_ERR_INVALID_ARGUMENT, "gb25_averages_begin: groups = %d must be a sum of GB25_AVG_MEANS (1), GB25_AVG_SQUARES (2), "
                "GB25_AVG_FLUXES (4) that contains GB25_AVG_MEANS (the eddy parts need the means)", (int)groups);
  int kc = 0;
  if (gb25_status s = diag_window(m, "gb25_averages_begin", k_first, k_count, m->cfg.Nz, "levels (k_first, k_count)", &kc)) return s;
  if (gb25_status s = diag_need_device(m, "gb25_averages_begin")) return s;
  if (gb25_status s = wait_for_model(m)) return s;
  m->diag.release_averages();   // (a model that already has averages starts over)
  // one allocation: every active accumulator, then the array a normalized read-out is divided into (the largest quantity);
  // each part starts on a multiple of two doubles
  size_t off[GB25_A_COUNT + 1], total = 0, largest = 0;
  for (int q = 0; q < GB25_A_COUNT; q++) {
    off[q] = total;
    if (!(groups & avg_group_of(q))) continue;
    const size_t n = avg_elems(m, q, kc);
    largest = std::max(largest, n);
    total += (n + 1) & ~(size_t)1;
  }
  off[GB25_A_COUNT] = total;
  total += largest;
  const size_t bytes = total * sizeof(double);
  char of[128];
  snprintf(of, sizeof of, "the accumulators of groups %d over %d level%s (fewer groups or a smaller window of levels need less)", (int)groups, kc,
           kc == 1 ? "" : "s");
  void* made = nullptr;
  if (gb25_status s = diag_room_for(m, "gb25_averages_begin", of, (double)bytes)) return s;
  if (gb25_status s = diag_alloc_zeroed(m, "gb25_averages_begin", of, bytes, &made)) return s;
  double* base = (double*)made;
  for (int q = 0; q < GB25_A_COUNT; q++) m->diag.avg_acc[q] = (groups & avg_group_of(q)) ? base + off[q] : nullptr;   // (MEANS is always active: avg_acc[0] is the allocation)
  m->diag.avg_out = base + off[GB25_A_COUNT];
  m->diag.avg_info.groups = groups;
  m->diag.avg_info.k_first = k_first;
  m->diag.avg_info.k_count = kc;
  m->diag.avg_on = true;
  return GB25_OK;
}

gb25_status gb25_averages_accumulate(gb25_model* m, double weight) {
  if (!m) return GB25_ERR_INVALID_ARGUMENT;
  if (!m->diag.avg_on) return fail(m, GB25_ERR_STATE, "gb25_averages_accumulate: no averages are being accumulated (call gb25_averages_begin first)");
  if (!(std::isfinite(weight) && weight > 0.0))
    return fail(m, GB25_ERR_INVALID_ARGUMENT, "gb25_averages_accumulate: weight must be finite and > 0, got %g", weight);
  static const gb25_field ids[6] = {GB25_U, GB25_V, GB25_W, GB25_T, GB25_S, GB25_ETA};
  const real* src[6];
  for (int q = 0; q < 6; q++)
    if (gb25_status s = diag_source(m, ids[q], &src[q])) return s;
  if (gb25_status s = wait_for_model(m)) return s;
  const Grid& g = m->g;
  AvgArgs a;
  for (int q = 0; q < GB25_A_COUNT; q++) a.acc[q] = m->diag.avg_acc[q];
  a.u = src[0]; a.v = src[1]; a.w = src[2]; a.T = src[3]; a.S = src[4]; a.eta = src[5];
  a.weight = weight;
  int32_t d[3];
  avg_extents(m, GB25_A_V, m->diag.avg_info.k_count, d);
  a.bx = m->Nx; a.by = m->Ny; a.byv = d[1];
  a.k_first = m->diag.avg_info.k_first; a.k_count = m->diag.avg_info.k_count;
  a.Nz = g.Nz; a.H = g.H; a.sx = g.sx; a.pl_c = g.pl_c; a.pl_v = g.pl_v;
  const int vw = (a.bx % 2 == 0 && a.H % 2 == 0) ? 2 : 1;   // (pairs: every parent row and accumulator row starts on an even element)
  const dim3 grd((a.bx + 64 * vw - 1) / (64 * vw), (a.byv + 3) / 4, (a.k_count + 1 + AVG_LEVELS - 1) / AVG_LEVELS);
  {
    Timed t(m, GB25_K_DIAGNOSTICS);
    if (vw == 2) averages_launch<2>(m, a, grd);
    else averages_launch<1>(m, a, grd);
    LAUNCHCHK();
  }
  HIPCHK(hipStreamSynchronize(m->stream));   // (the sources are free for the next step when the call returns)
  gb25_averages_info& I = m->diag.avg_info;
  if (I.samples == 0) {
    I.first_iteration = m->iteration;
    I.first_time = m->time;
  }
  I.last_iteration = m->iteration;
  I.last_time = m->time;
  I.samples++;
  I.weight_sum = I.weight_sum + weight;
  return GB25_OK;
}

gb25_status gb25_averages_get_info(const gb25_model* m, gb25_averages_info* info) {
  if (!m || !info) return GB25_ERR_INVALID_ARGUMENT;
  *info = m->diag.avg_info;   // (all zero, groups = 0, while no averages are being accumulated)
  return GB25_OK;
}

gb25_status gb25_average_dims(const gb25_model* m, gb25_average q, int32_t dims[3]) {
  if (!m || !dims || q < 0 || q >= GB25_A_COUNT) return GB25_ERR_INVALID_ARGUMENT;
  avg_extents(m, q, m->diag.avg_on ? m->diag.avg_info.k_count : m->cfg.Nz, dims);   // (before gb25_averages_begin: the whole column)
  return GB25_OK;
}

gb25_status gb25_get_average(gb25_model* m, gb25_average q, int32_t normalized, double* host, int64_t count) {
  if (!m) return GB25_ERR_INVALID_ARGUMENT;
  if (!host) return fail(m, GB25_ERR_INVALID_ARGUMENT, "gb25_get_average: host is NULL");
  if (gb25_status s = averages_quantity(m, "gb25_get_average", q)) return s;
  const size_t n = avg_elems(m, q, m->diag.avg_info.k_count);
  if (count != (int64_t)n)
    return fail(m, GB25_ERR_INVALID_ARGUMENT, "gb25_get_average: this average has %zu elements over the active window, count is %lld", n, (long long)count);
  if (normalized && m->diag.avg_info.samples == 0)
    return fail(m, GB25_ERR_STATE, "gb25_get_average: normalized = %d before the first sample (weight_sum is 0)", (int)normalized);
  const double* from = m->diag.avg_acc[q];
  if (normalized) {
    Timed t(m, GB25_K_DIAGNOSTICS);
    hipLaunchKernelGGL(k_averages_normalize, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, m->stream, from, m->diag.avg_info.weight_sum,
                       m->diag.avg_out, (long long)n);
    LAUNCHCHK();
    from = m->diag.avg_out;
  }
  return diag_download(m, host, from, n * sizeof(double));
}

gb25_status gb25_average_device_ptr(gb25_model* m, gb25_average q, const double** dev, int32_t device_dims[3]) {
  if (!m) return GB25_ERR_INVALID_ARGUMENT;
  if (!dev) return fail(m, GB25_ERR_INVALID_ARGUMENT, "gb25_average_device_ptr: dev is NULL");
  if (gb25_status s = averages_quantity(m, "gb25_average_device_ptr", q)) return s;
  HIPCHK(hipStreamSynchronize(m->stream));
  *dev = m->diag.avg_acc[q];
  if (device_dims) avg_extents(m, q, m->diag.avg_info.k_count, device_dims);
  return GB25_OK;
}

gb25_status gb25_averages_end(gb25_model* m) {
  if (!m) return GB25_ERR_INVALID_ARGUMENT;
  if (m->diag.avg_on) HIPCHK(hipStreamSynchronize(m->stream));
  m->diag.release_averages();
  return GB25_OK;
}

}  // extern "C"
