// filters_host.hpp -- host side of gb25_filter_dims / gb25_derived_filter_dims / gb25_get_filter_sums / gb25_compute_filter_sums /
// gb25_get_derived_filter_sums / gb25_filter_info_bytes (include/gb25.h); included by gb25_api.hip behind diagnostics_host.hpp,
// whose shared pieces it is built from exactly as blocks_host.hpp is (its k_block_counts folds the counts here too).  Kernels:
// filter_kernels.hpp; the memory: filters (a result buffer), filter_* of DiagState (diagnostics_state.hpp).  Like the other
// diagnostics nothing here writes model memory or a schedule flag: the only memory written is the results' own buffer.
#pragma once

namespace {

static_assert(FLT_MAX_R == GB25_FILTER_MAX_RADIUS, "the kernel's LDS wings are the header's largest radius");
constexpr size_t FILTER_WEIGHTS = 2 * GB25_FILTER_MAX_RADIUS + 1;   // doubles of wx, and of wy

// What is specific to a call of the filter, beside its source's plan: the window, the result, which planes go beyond the x
// pass, and where everything lies in the buffer
struct FilterPlan {
  int kc;                                // the resolved k_count
  int32_t e[3];                          // the result's dims
  bool want[3];                          // measure, first, second stored
  size_t elems, selems;                  // of a result plane, of a scratch plane
  long long waves_x, waves_y;
  dim3 grid_x, grid_y;
  int64_t clipped;
};

// the checks that need no device, over the source S: Nx columns and Ny rows of cell centres, ITS levels
gb25_status filters_check(gb25_model* m, const char* what, const SourcePlan& S, const gb25_filter* F, const double* wx, const double* wy,
                          const int32_t* rx_of_row, FilterPlan* P) {
  if (!F) return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: filter is NULL", what);
  const int Nx = m->Nx, Ny = m->Ny, levels = S.dims[2];
  if (F->rx < 0 || F->rx > GB25_FILTER_MAX_RADIUS)
    return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: rx = %d must be 0 .. %d", what, (int)F->rx, GB25_FILTER_MAX_RADIUS);
  if (F->ry < 0 || F->ry > GB25_FILTER_MAX_RADIUS)
    return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: ry = %d must be 0 .. %d", what, (int)F->ry, GB25_FILTER_MAX_RADIUS);
  if (2 * F->rx + 1 > Nx)
    return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: rx = %d: a window of 2 rx + 1 = %d columns exceeds Nx = %d (a point would enter it twice)", what,
                (int)F->rx, 2 * (int)F->rx + 1, Nx);
  if (F->sx <= 0 || Nx % F->sx) return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: sx = %d must be > 0 and divide Nx = %d", what, (int)F->sx, Nx);
  if (F->sy <= 0 || Ny % F->sy)
    return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: sy = %d must be > 0 and divide Ny = %d (rows of cell centres)", what, (int)F->sy, Ny);
  if (gb25_status s = diag_window(m, what, F->k_first, F->k_count, levels, "levels (k_first, k_count)", &P->kc)) return s;
  if (wx && rx_of_row) return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: wx and rx_of_row exclude each other: with a radius per row x is the box", what);
  const double* w[2] = {wx, wy};
  const int r[2] = {F->rx, F->ry};
  for (int q = 0; q < 2; q++) {
    if (!w[q]) continue;
    const char* name = q ? "wy" : "wx";
    double sum = 0.0;
    for (int d = 0; d <= 2 * r[q]; d++) {
      if (!std::isfinite(w[q][d]) || w[q][d] < 0.0)
        return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: %s[%d] = %g must be finite and >= 0", what, name, d, w[q][d]);
      sum += w[q][d];
    }
    if (!(sum > 0.0) || !std::isfinite(sum)) return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: %s: the %d weights sum to %g, not to a positive number", what, name, 2 * r[q] + 1, sum);
  }
  if (rx_of_row)
    for (int j = 0; j < Ny; j++)
      if (rx_of_row[j] < 0 || rx_of_row[j] > GB25_FILTER_MAX_RADIUS || 2 * rx_of_row[j] + 1 > Nx)
        return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: rx_of_row[%d] = %d must be 0 .. %d with 2 rx + 1 <= Nx = %d", what, j, (int)rx_of_row[j],
                    GB25_FILTER_MAX_RADIUS, Nx);
  P->e[0] = Nx / F->sx;
  P->e[1] = Ny / F->sy;
  P->e[2] = P->kc;
  return GB25_OK;
}
// the source's own checks, those of the families that weigh with the measure, then the call's
gb25_status filters_plan(gb25_model* m, const char* what, const DiagSource& S, const gb25_filter* F, const double* wx, const double* wy,
                         const int32_t* rx_of_row, SourcePlan* SP, FilterPlan* P) {
  if (gb25_status s = diag_source_plan(m, what, S, SP)) return s;
  if (gb25_status s = diag_source_measured(m, what, S)) return s;
  return filters_check(m, what, *SP, F, wx, wy, rx_of_row, P);
}

// the counts, the weights, the rows' radii, the planes, the scratch planes, then the waves' slots
inline size_t filters_rows_bytes(const gb25_model* m) { return (((size_t)m->Ny * sizeof(int32_t)) + 7) / 8 * 8; }
inline BlockCounts* filters_counts(gb25_model* m) { return (BlockCounts*)m->diag.filters.p; }
inline double* filters_weights(gb25_model* m, int q) { return (double*)((char*)m->diag.filters.p + COUNTS_HEAD) + q * FILTER_WEIGHTS; }
inline int* filters_rows(gb25_model* m) { return (int*)(filters_weights(m, 2)); }
inline double* filters_planes(gb25_model* m) { return (double*)((char*)filters_rows(m) + filters_rows_bytes(m)); }
gb25_status filters_buffer(gb25_model* m, const char* what, const FilterPlan& P) {
  int nscratch = 0;
  for (int q = 0; q < 3; q++) nscratch += (q == 0 || P.want[q]) ? 1 : 0;
  const size_t bytes = COUNTS_HEAD + 2 * FILTER_WEIGHTS * sizeof(double) + filters_rows_bytes(m) +
                       (3 * P.elems + (size_t)nscratch * P.selems) * sizeof(double) + (size_t)(P.waves_x + P.waves_y) * sizeof(BlockSlot);
  return m->diag.filters.grow(m, what, "the planes and the scratch planes of the filter", bytes);
}

// The launches over src, whose element (0, 0, k_first) is box.origin, on m->stream behind whatever made src; the model has been
// waited for.  The planes lie at filters_planes, the counts at filters_counts, when the stream has run.
gb25_status filters_run(gb25_model* m, const char* what, const SourcePlan& S, FilterPlan& P, const gb25_filter& F, const double* wx,
                        const double* wy, const int32_t* rx_of_row, const real* src, const DiagBox& box) {
  const int Nx = m->Nx, Ny = m->Ny;
  P.elems = (size_t)P.e[0] * P.e[1] * P.e[2];
  P.selems = (size_t)P.e[0] * Ny * P.e[2];
  P.grid_x = dim3((Nx + FLT_TILE - 1) / FLT_TILE, Ny, P.e[2]);
  P.grid_y = dim3((P.e[0] + FLT_TILE - 1) / FLT_TILE, P.e[1], P.e[2]);
  P.waves_x = (long long)P.grid_x.x * P.grid_x.y * P.grid_x.z * (FLT_TILE / 64);
  P.waves_y = (long long)P.grid_y.x * P.grid_y.y * P.grid_y.z * (FLT_TILE / 64);
  long long cut = 0;   // output rows whose y window leaves 0 .. Ny - 1
  for (int J = 0; J < P.e[1]; J++) cut += (J * F.sy - F.ry < 0 || J * F.sy + F.ry > Ny - 1) ? 1 : 0;
  P.clipped = (int64_t)cut * P.e[0] * P.e[2];
  if (gb25_status s = filters_buffer(m, what, P)) return s;
  if (gb25_status s = moments_tables(m)) return s;
  DiagState& D = m->diag;
  HIPCHK(hipMemsetAsync(filters_counts(m), 0, COUNTS_HEAD, m->stream));
  if (wx) {
    D.filter_wx.assign(wx, wx + 2 * F.rx + 1);
    HIPCHK(hipMemcpyAsync(filters_weights(m, 0), D.filter_wx.data(), D.filter_wx.size() * sizeof(double), hipMemcpyHostToDevice, m->stream));
  }
  if (wy) {
    D.filter_wy.assign(wy, wy + 2 * F.ry + 1);
    HIPCHK(hipMemcpyAsync(filters_weights(m, 1), D.filter_wy.data(), D.filter_wy.size() * sizeof(double), hipMemcpyHostToDevice, m->stream));
  }
  if (rx_of_row) {
    D.filter_rows.assign(rx_of_row, rx_of_row + Ny);
    HIPCHK(hipMemcpyAsync(filters_rows(m), D.filter_rows.data(), (size_t)Ny * sizeof(int32_t), hipMemcpyHostToDevice, m->stream));
  }
  const MomentsTables tab = diag_measure_tables(m, true);
  double* planes = filters_planes(m);
  FilterArgs A = {};
  A.rx = F.rx; A.ry = F.ry; A.sx = F.sx; A.sy = F.sy;
  A.k_first = F.k_first;
  A.Nx = Nx; A.Ny = Ny;
  A.nI = P.e[0]; A.nJ = P.e[1]; A.nK = P.e[2];
  A.wx = wx ? filters_weights(m, 0) : nullptr;
  A.wy = wy ? filters_weights(m, 1) : nullptr;
  A.rx_of_row = rx_of_row ? filters_rows(m) : nullptr;
  double* scratch = planes + 3 * P.elems;
  for (int q = 0; q < 3; q++) {
    A.out[q] = P.want[q] ? planes + q * P.elems : nullptr;
    A.s[q] = nullptr;
    if (q == 0 || P.want[q]) {   // (the measure always: `empty` is counted from it)
      A.s[q] = scratch;
      scratch += P.selems;
    }
  }
  A.slots_x = (BlockSlot*)scratch;
  A.slots_y = A.slots_x + P.waves_x;
  Timed t(m, GB25_K_DIAGNOSTICS);
  diag_with_loc(S.loc, [&](auto loc) {
    constexpr int LOC = decltype(loc)::value;
    if (A.wx) hipLaunchKernelGGL((k_filter_x<real, LOC, true>), P.grid_x, dim3(FLT_TILE), 0, m->stream, m->g, tab, src, box, A);
    else hipLaunchKernelGGL((k_filter_x<real, LOC, false>), P.grid_x, dim3(FLT_TILE), 0, m->stream, m->g, tab, src, box, A);
  });
  LAUNCHCHK();
  if (A.wy) hipLaunchKernelGGL(k_filter_y<true>, P.grid_y, dim3(FLT_TILE), 0, m->stream, A);
  else hipLaunchKernelGGL(k_filter_y<false>, P.grid_y, dim3(FLT_TILE), 0, m->stream, A);
  LAUNCHCHK();
  const long long waves = P.waves_x + P.waves_y;
  const unsigned folders = (unsigned)std::min<long long>(64, (waves + BLK_THREADS - 1) / BLK_THREADS);
  hipLaunchKernelGGL(k_block_counts, dim3(folders), dim3(BLK_THREADS), 0, m->stream, (const BlockSlot*)A.slots_x, waves, filters_counts(m));
  LAUNCHCHK();
  return GB25_OK;
}

gb25_status filters_single_domain(gb25_model* m, const char* what) {
  if (m->slab)
    return fail(m, GB25_ERR_STATE,
                "%s: this model is a rank of a decomposition: a window reaches beyond the rank's columns and rows, and the halo exchanges are not "
                "widened for it; gather on the host (LocalSlabEnsemble.filter_sums of gb-25_amd/distributed.py)", what);
  return GB25_OK;
}

// checks, source, launches
gb25_status filters_of(gb25_model* m, const char* what, const DiagSource& S, const gb25_filter* F, const double* wx, const double* wy,
                       const int32_t* rx_of_row, FilterPlan* P) {
  SourcePlan SP;
  if (gb25_status s = filters_plan(m, what, S, F, wx, wy, rx_of_row, &SP, P)) return s;
  if (gb25_status s = filters_single_domain(m, what)) return s;
  if (gb25_status s = diag_need_device(m, what)) return s;
  const real* src = nullptr;
  DiagBox b;
  if (gb25_status s = diag_source_resolve(m, S, SP, F->k_first, P->kc, &src, &b)) return s;
  return filters_run(m, what, SP, *P, *F, wx, wy, rx_of_row, src, b);
}

// the planes asked for and the counts to the host, then the record
gb25_status filters_download(gb25_model* m, const FilterPlan& P, double* measure, double* first, double* second, gb25_filter_info* info) {
  double* const host[3] = {measure, first, second};
  BlockCounts c = {};
  if (gb25_status s = diag_download_planes(m, host, filters_planes(m), P.elems, filters_counts(m), &c)) return s;
  if (!info) return GB25_OK;
  memset(info, 0, sizeof *info);
  memcpy(info->dims, P.e, sizeof P.e);
  info->nonfinite = (int64_t)c.nonfinite;
  info->empty = (int64_t)c.empty_blocks;
  info->clipped = P.clipped;
  diag_global_offset(m, GB25_T, 0, info->global_offset);   // (interior: the offsets are those of any field, 0 in k)
  return GB25_OK;
}

// gb25_filter_dims and its derived twin
gb25_status filters_dims(const gb25_model* m, const char* what, const DiagSource& S, const gb25_filter* F, int32_t dims[3]) {
  if (!m || !dims) return GB25_ERR_INVALID_ARGUMENT;
  SourcePlan SP;
  FilterPlan P = {};
  if (gb25_status s = filters_plan(const_cast<gb25_model*>(m), what, S, F, nullptr, nullptr, nullptr, &SP, &P)) return s;   // (the error string alone is written)
  memcpy(dims, P.e, sizeof P.e);
  return GB25_OK;
}

}  // namespace

extern "C" {

int32_t gb25_filter_info_bytes(void) { return (int32_t)sizeof(gb25_filter_info); }

gb25_status gb25_filter_dims(const gb25_model* m, gb25_field f, const gb25_filter* filter, int32_t dims[3]) {
  return filters_dims(m, "gb25_filter_dims", DiagSource(f), filter, dims);
}

gb25_status gb25_derived_filter_dims(const gb25_model* m, gb25_derived q, const gb25_filter* filter, int32_t dims[3]) {
  return filters_dims(m, "gb25_derived_filter_dims", DiagSource(q, 1.0), filter, dims);   // (the dims do not depend on the parameter)
}

gb25_status gb25_get_filter_sums(gb25_model* m, gb25_field f, const gb25_filter* filter, const double* wx, const double* wy,
                                 const int32_t* rx_of_row, double* measure, double* first, double* second, gb25_filter_info* info) {
  if (!m) return GB25_ERR_INVALID_ARGUMENT;
  const char* what = "gb25_get_filter_sums";
  if (!measure && !first && !second) return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: measure, first and second are all NULL: no output requested", what);
  FilterPlan P = {};
  P.want[0] = measure != nullptr; P.want[1] = first != nullptr; P.want[2] = second != nullptr;
  if (gb25_status s = filters_of(m, what, DiagSource(f), filter, wx, wy, rx_of_row, &P)) return s;
  return filters_download(m, P, measure, first, second, info);
}

gb25_status gb25_compute_filter_sums(gb25_model* m, gb25_field f, const gb25_filter* filter, const double* wx, const double* wy,
                                     const int32_t* rx_of_row, gb25_filter_info* info, const double** dev, int32_t device_dims[3]) {
  if (!m) return GB25_ERR_INVALID_ARGUMENT;
  const char* what = "gb25_compute_filter_sums";
  if (!dev) return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: dev is NULL: no output requested", what);
  FilterPlan P = {};
  P.want[0] = P.want[1] = P.want[2] = true;
  if (gb25_status s = filters_of(m, what, DiagSource(f), filter, wx, wy, rx_of_row, &P)) return s;
  if (gb25_status s = filters_download(m, P, nullptr, nullptr, nullptr, info)) return s;   // (the counts; the stream is quiet behind it)
  *dev = filters_planes(m);
  if (device_dims) memcpy(device_dims, P.e, sizeof P.e);
  return GB25_OK;
}

gb25_status gb25_get_derived_filter_sums(gb25_model* m, gb25_derived q, double param, const gb25_filter* filter, const double* wx,
                                         const double* wy, const int32_t* rx_of_row, double* measure, double* first, double* second,
                                         gb25_filter_info* info) {
  if (!m) return GB25_ERR_INVALID_ARGUMENT;
  const char* what = "gb25_get_derived_filter_sums";
  if (!measure && !first && !second) return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: measure, first and second are all NULL: no output requested", what);
  FilterPlan P = {};
  P.want[0] = measure != nullptr; P.want[1] = first != nullptr; P.want[2] = second != nullptr;
  if (gb25_status s = filters_of(m, what, DiagSource(q, param), filter, wx, wy, rx_of_row, &P)) return s;
  return filters_download(m, P, measure, first, second, info);
}

}  // extern "C"
