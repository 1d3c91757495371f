// filters_host.hpp -- host side of gb25_filter_dims / gb25_derived_filter_dims / gb25_get_filter_sums / gb25_compute_filter_sums /
// gb25_get_derived_filter_sums / gb25_filter_info_bytes (include/gb25.h); included by gb25_api.hip behind blocks_host.hpp, whose
// plans of a source (blocks_plan_field, blocks_plan_derived: the fine extents and the location of the measure) it shares, as it
// shares diagnostics_host.hpp's helpers (diag_*), measure (moments_tables) and derived fields (derived_run).  Kernels:
// filter_kernels.hpp; the memory: filters, filter_* of DiagState (diagnostics_state.hpp).  Like the other diagnostics nothing
// here writes model memory or a schedule flag: the only memory written is the results' own buffer.
#pragma once

namespace {

static_assert(FLT_MAX_R == GB25_FILTER_MAX_RADIUS, "the kernel's LDS wings are the header's largest radius");
constexpr size_t FILTER_HEAD = 32;                              // bytes in front of the weights: BlockCounts, padded
constexpr size_t FILTER_WEIGHTS = 2 * GB25_FILTER_MAX_RADIUS + 1;   // doubles of wx, and of wy
static_assert(sizeof(BlockCounts) <= FILTER_HEAD, "the counts fit their slot");

// What a call filters: the source (BlockPlan: fine extents, location, resolved k_count; e = the result's dims), which planes
// go beyond the x pass, and where everything lies in the buffer
struct FilterPlan {
  BlockPlan src;
  bool want[3];                          // measure, first, second stored
  size_t elems, selems;                  // of a result plane, of a scratch plane
  long long waves_x, waves_y;
  dim3 grid_x, grid_y;
  int64_t clipped;
};

// the checks that need no device; P.src.fine and P.src.loc are given
gb25_status filters_check(gb25_model* m, const char* what, const gb25_filter* F, const double* wx, const double* wy, const int32_t* rx_of_row,
                          FilterPlan* P) {
  if (!F) return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: filter is NULL", what);
  const int Nx = P->src.fine[0], Ny = P->src.fine[1], levels = P->src.fine[2];
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
  if (gb25_status s = diag_window(m, what, F->k_first, F->k_count, levels, "levels (k_first, k_count)", &P->src.kc)) return s;
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
  P->src.e[0] = Nx / F->sx;
  P->src.e[1] = Ny / F->sy;
  P->src.e[2] = P->src.kc;
  return GB25_OK;
}

// the counts, the weights, the rows' radii, the planes, the scratch planes, then the waves' slots; made by the first call, made
// anew when a call needs more bytes
inline size_t filters_rows_bytes(const gb25_model* m) { return (((size_t)m->Ny * sizeof(int32_t)) + 7) / 8 * 8; }
inline BlockCounts* filters_counts(gb25_model* m) { return (BlockCounts*)m->diag.filters; }
inline double* filters_weights(gb25_model* m, int q) { return (double*)((char*)m->diag.filters + FILTER_HEAD) + q * FILTER_WEIGHTS; }
inline int* filters_rows(gb25_model* m) { return (int*)(filters_weights(m, 2)); }
inline double* filters_planes(gb25_model* m) { return (double*)((char*)filters_rows(m) + filters_rows_bytes(m)); }
gb25_status filters_buffer(gb25_model* m, const char* what, const FilterPlan& P) {
  DiagState& D = m->diag;
  int nscratch = 0;
  for (int q = 0; q < 3; q++) nscratch += (q == 0 || P.want[q]) ? 1 : 0;
  const size_t bytes = FILTER_HEAD + 2 * FILTER_WEIGHTS * sizeof(double) + filters_rows_bytes(m) +
                       (3 * P.elems + (size_t)nscratch * P.selems) * sizeof(double) + (size_t)(P.waves_x + P.waves_y) * sizeof(BlockSlot);
  if (D.filters && bytes <= D.filter_bytes) return GB25_OK;
  D.drop(D.filters);
  D.filter_bytes = 0;
  if (gb25_status s = diag_room_for(m, what, "the planes and the scratch planes of the filter", (double)bytes)) return s;
  const hipError_t e = hipMalloc(&D.filters, bytes);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    D.filters = nullptr;
    return fail(m, GB25_ERR_OUT_OF_MEMORY, "%s: hipMalloc of %zu bytes for the planes and the scratch planes of the filter failed: %s", what, bytes,
                hipGetErrorString(e));
  }
  D.filter_bytes = bytes;
  return GB25_OK;
}

template <int LOC>
void filters_launch_loc(gb25_model* m, const dim3& grd, const MomentsTables& tab, const real* src, const DiagBox& b, const FilterArgs& A) {
  if (A.wx) hipLaunchKernelGGL((k_filter_x<real, LOC, true>), grd, dim3(FLT_TILE), 0, m->stream, m->g, tab, src, b, A);
  else hipLaunchKernelGGL((k_filter_x<real, LOC, false>), grd, dim3(FLT_TILE), 0, m->stream, m->g, tab, src, b, A);
}

// The launches over src, whose element (0, 0, k_first) is box.origin, on m->stream behind whatever made src; the model has been
// waited for.  The planes lie at filters_planes, the counts at filters_counts, when the stream has run.
gb25_status filters_run(gb25_model* m, const char* what, FilterPlan& P, const gb25_filter& F, const double* wx, const double* wy,
                        const int32_t* rx_of_row, const real* src, const DiagBox& box) {
  const BlockPlan& S = P.src;
  const int Nx = S.fine[0], Ny = S.fine[1];
  P.elems = (size_t)S.e[0] * S.e[1] * S.e[2];
  P.selems = (size_t)S.e[0] * Ny * S.e[2];
  P.grid_x = dim3((Nx + FLT_TILE - 1) / FLT_TILE, Ny, S.e[2]);
  P.grid_y = dim3((S.e[0] + FLT_TILE - 1) / FLT_TILE, S.e[1], S.e[2]);
  P.waves_x = (long long)P.grid_x.x * P.grid_x.y * P.grid_x.z * (FLT_TILE / 64);
  P.waves_y = (long long)P.grid_y.x * P.grid_y.y * P.grid_y.z * (FLT_TILE / 64);
  long long cut = 0;   // output rows whose y window leaves 0 .. Ny - 1
  for (int J = 0; J < S.e[1]; J++) cut += (J * F.sy - F.ry < 0 || J * F.sy + F.ry > Ny - 1) ? 1 : 0;
  P.clipped = (int64_t)cut * S.e[0] * S.e[2];
  if (gb25_status s = filters_buffer(m, what, P)) return s;
  if (gb25_status s = moments_tables(m)) return s;
  DiagState& D = m->diag;
  HIPCHK(hipMemsetAsync(filters_counts(m), 0, FILTER_HEAD, m->stream));
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
  MomentsTables tab;
  for (int q = 0; q < 3; q++) {
    tab.area[q] = D.area[q];
    tab.first[q] = D.first_wet[q];
  }
  tab.pivot_row = is_folded(m) ? m->Ny - 1 : -1;
  double* planes = filters_planes(m);
  FilterArgs A = {};
  A.rx = F.rx; A.ry = F.ry; A.sx = F.sx; A.sy = F.sy;
  A.k_first = F.k_first;
  A.Nx = Nx; A.Ny = Ny;
  A.nI = S.e[0]; A.nJ = S.e[1]; A.nK = S.e[2];
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
  switch (S.loc) {
    case LOC_CCC: filters_launch_loc<LOC_CCC>(m, P.grid_x, tab, src, box, A); break;
    case LOC_FCC: filters_launch_loc<LOC_FCC>(m, P.grid_x, tab, src, box, A); break;
    case LOC_CFC: filters_launch_loc<LOC_CFC>(m, P.grid_x, tab, src, box, A); break;
    case LOC_CCF: filters_launch_loc<LOC_CCF>(m, P.grid_x, tab, src, box, A); break;
    case LOC_CC: filters_launch_loc<LOC_CC>(m, P.grid_x, tab, src, box, A); break;
    case LOC_FC: filters_launch_loc<LOC_FC>(m, P.grid_x, tab, src, box, A); break;
    case LOC_CF: filters_launch_loc<LOC_CF>(m, P.grid_x, tab, src, box, A); break;
  }
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

// checks, source, launches: a field
gb25_status filters_of_field(gb25_model* m, const char* what, gb25_field f, const gb25_filter* F, const double* wx, const double* wy,
                             const int32_t* rx_of_row, FilterPlan* P) {
  if (gb25_status s = blocks_plan_field(m, what, f, &P->src)) return s;
  if (gb25_status s = filters_check(m, what, F, wx, wy, rx_of_row, P)) return s;
  if (gb25_status s = filters_single_domain(m, what)) return s;
  if (gb25_status s = diag_need_device(m, what)) return s;
  const real* src = nullptr;
  DiagBox b;
  if (gb25_status s = diag_source(m, f, &src)) return s;
  if (gb25_status s = diag_box(m, f, 0, &b)) return s;
  if (gb25_status s = wait_for_model(m)) return s;
  b.origin += b.plane * F->k_first;
  return filters_run(m, what, *P, *F, wx, wy, rx_of_row, src, b);
}
// ... a derived field: gb25_compute_derived's launches into the model's packed array, then the same kernels over that array
gb25_status filters_of_derived(gb25_model* m, const char* what, gb25_derived q, double param, const gb25_filter* F, const double* wx,
                               const double* wy, const int32_t* rx_of_row, FilterPlan* P) {
  if (gb25_status s = blocks_plan_derived(m, what, q, &P->src)) return s;
  if (gb25_status s = derived_check(m, what, q, param)) return s;
  if (gb25_status s = filters_check(m, what, F, wx, wy, rx_of_row, P)) return s;
  if (gb25_status s = filters_single_domain(m, what)) return s;
  if (gb25_status s = diag_need_device(m, what)) return s;
  const real* src = nullptr;
  if (gb25_status s = derived_run(m, q, param, F->k_first, P->src.kc, &src)) return s;
  const BlockPlan& S = P->src;
  const DiagBox b{S.fine[0], S.fine[1], S.kc, (long long)S.fine[0], (long long)S.fine[0] * S.fine[1], 0};   // (packed: the levels of the window alone)
  return filters_run(m, what, *P, *F, wx, wy, rx_of_row, src, b);
}

// the planes asked for and the counts to the host (behind the launches; the last copy synchronizes), then the record
gb25_status filters_download(gb25_model* m, const FilterPlan& P, double* measure, double* first, double* second, gb25_filter_info* info) {
  double* host[3] = {measure, first, second};
  for (int q = 0; q < 3; q++)
    if (host[q]) HIPCHK(hipMemcpyAsync(host[q], filters_planes(m) + q * P.elems, P.elems * sizeof(double), hipMemcpyDeviceToHost, m->stream));
  BlockCounts c = {};
  if (gb25_status s = diag_download(m, &c, filters_counts(m), sizeof c)) return s;
  if (info) {
    memset(info, 0, sizeof *info);
    memcpy(info->dims, P.src.e, sizeof P.src.e);
    info->nonfinite = (int64_t)c.nonfinite;
    info->empty = (int64_t)c.empty_blocks;
    info->clipped = P.clipped;
    diag_global_offset(m, GB25_T, 0, info->global_offset);   // (interior: the offsets are those of any field, 0 in k)
  }
  return GB25_OK;
}

gb25_status filters_dims(gb25_model* m, const char* what, const gb25_filter* F, FilterPlan* P, int32_t dims[3]) {
  if (gb25_status s = filters_check(m, what, F, nullptr, nullptr, nullptr, P)) return s;
  memcpy(dims, P->src.e, sizeof P->src.e);
  return GB25_OK;
}

}  // namespace

extern "C" {

int32_t gb25_filter_info_bytes(void) { return (int32_t)sizeof(gb25_filter_info); }

gb25_status gb25_filter_dims(const gb25_model* m, gb25_field f, const gb25_filter* filter, int32_t dims[3]) {
  if (!m || !dims) return GB25_ERR_INVALID_ARGUMENT;
  gb25_model* mm = const_cast<gb25_model*>(m);   // (the error string alone is written)
  FilterPlan P = {};
  if (gb25_status s = blocks_plan_field(mm, "gb25_filter_dims", f, &P.src)) return s;
  return filters_dims(mm, "gb25_filter_dims", filter, &P, dims);
}

gb25_status gb25_derived_filter_dims(const gb25_model* m, gb25_derived q, const gb25_filter* filter, int32_t dims[3]) {
  if (!m || !dims) return GB25_ERR_INVALID_ARGUMENT;
  gb25_model* mm = const_cast<gb25_model*>(m);
  FilterPlan P = {};
  if (gb25_status s = blocks_plan_derived(mm, "gb25_derived_filter_dims", q, &P.src)) return s;
  return filters_dims(mm, "gb25_derived_filter_dims", filter, &P, dims);
}

gb25_status gb25_get_filter_sums(gb25_model* m, gb25_field f, const gb25_filter* filter, const double* wx, const double* wy,
                                 const int32_t* rx_of_row, double* measure, double* first, double* second, gb25_filter_info* info) {
  if (!m) return GB25_ERR_INVALID_ARGUMENT;
  const char* what = "gb25_get_filter_sums";
  if (!measure && !first && !second) return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: measure, first and second are all NULL: no output requested", what);
  FilterPlan P = {};
  P.want[0] = measure != nullptr; P.want[1] = first != nullptr; P.want[2] = second != nullptr;
  if (gb25_status s = filters_of_field(m, what, f, filter, wx, wy, rx_of_row, &P)) return s;
  return filters_download(m, P, measure, first, second, info);
}

gb25_status gb25_compute_filter_sums(gb25_model* m, gb25_field f, const gb25_filter* filter, const double* wx, const double* wy,
                                     const int32_t* rx_of_row, gb25_filter_info* info, const double** dev, int32_t device_dims[3]) {
  if (!m) return GB25_ERR_INVALID_ARGUMENT;
  const char* what = "gb25_compute_filter_sums";
  if (!dev) return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: dev is NULL: no output requested", what);
  FilterPlan P = {};
  P.want[0] = P.want[1] = P.want[2] = true;
  if (gb25_status s = filters_of_field(m, what, f, filter, wx, wy, rx_of_row, &P)) return s;
  if (gb25_status s = filters_download(m, P, nullptr, nullptr, nullptr, info)) return s;   // (the counts; the stream is quiet behind it)
  *dev = filters_planes(m);
  if (device_dims) memcpy(device_dims, P.src.e, sizeof P.src.e);
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
  if (gb25_status s = filters_of_derived(m, what, q, param, filter, wx, wy, rx_of_row, &P)) return s;
  return filters_download(m, P, measure, first, second, info);
}

}  // extern "C"
