// region_host.hpp -- host side of gb25_region_dims / gb25_label_regions / gb25_get_regions / gb25_region_bytes /
// gb25_regions_info_bytes (include/gb25.h); included by gb25_api.hip behind kinematics_host.hpp, whose kinematics_run (and
// diagnostics_host.hpp's derived_run, diag_source) make the criterion.  Kernels: region_kernels.hpp; the memory: regions (a result
// buffer of DiagState, diagnostics_state.hpp).  Like the other diagnostics nothing here writes model memory or a schedule flag:
// the only memory written is the results' own buffer (and, for a derived or kinematics criterion, the model's packed array).
#pragma once

namespace {

static_assert(sizeof(RegionRecord) == sizeof(gb25_region), "a record is a gb25_region");

struct RegionPlan {
  gb25_region_source kind;
  int32_t id, param, carried;
  int above;
  double threshold;
  int k_first, kc, max_regions;
  int Nx, Ny, n, blocks;
  // where everything lies in the buffer: the counts of the levels, the label planes, the records, then one level's scratch
  size_t off_labels, off_records, off_work, off_num, off_roots, bytes;
};

inline size_t region_align(size_t b) { return (b + 255) & ~(size_t)255; }

gb25_status regions_single_domain(gb25_model* m, const char* what) {
  if (m->slab)
    return fail(m, GB25_ERR_STATE,
                "%s: this model is a rank of a decomposition: a region reaches beyond the rank's columns and rows; gather the criterion on the "
                "host (label_host, region_records_host of gb-25_amd/regions.py)", what);
  return GB25_OK;
}

// the checks that need no device
gb25_status regions_check(gb25_model* m, const char* what, gb25_region_source kind, int32_t id, int32_t param, int32_t carried, gb25_region_cmp cmp,
                          double threshold, int32_t k_first, int32_t k_count, int32_t max_regions, RegionPlan* P) {
  switch (kind) {
    case GB25_REGION_FIELD:
      if (id < 0 || id >= GB25_FIELD_COUNT) return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: id: no field %d", what, (int)id);
      if (id != GB25_T && id != GB25_S && id != GB25_E)
        return fail(m, GB25_ERR_INVALID_ARGUMENT,
                    "%s: id: field %d is not a tracer at (Center, Center, Center): the criterion takes GB25_T, GB25_S or GB25_E (a face field "
                    "has no cell to label)", what, (int)id);
      if (param != 0) return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: param: a field takes 0, got %d", what, (int)param);
      break;
    case GB25_REGION_DERIVED:
      if (gb25_status s = derived_check(m, what, (gb25_derived)id, 1.0)) return s;
      if (id == GB25_D_VORTICITY)
        return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: id: derived GB25_D_VORTICITY is a corner quantity, at (f,f,c): it has no cell to label", what);
      if (id == GB25_D_MIXED_LAYER_DEPTH)
        return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: id: derived GB25_D_MIXED_LAYER_DEPTH is 2-D: the criterion is a 3-D quantity at (c,c,c)", what);
      if (param != 0) return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: param: a derived field takes 0, got %d", what, (int)param);
      break;
    case GB25_REGION_KINEMATICS:
      if (gb25_status s = kinematics_check(m, what, (gb25_kinematics)id, param)) return s;
      if (kinematics_at_corners((gb25_kinematics)id))
        return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: id: kinematics quantity %d is a corner quantity, at (f,f,c): it has no cell to label", what, (int)id);
      break;
    default:
      return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: source_kind must be GB25_REGION_FIELD, GB25_REGION_DERIVED or GB25_REGION_KINEMATICS, got %d", what, (int)kind);
  }
  if (carried != -1 && carried != GB25_T && carried != GB25_S && carried != GB25_E)
    return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: carried_field must be GB25_T, GB25_S, GB25_E or -1 (none), got %d", what, (int)carried);
  for (int f : {kind == GB25_REGION_FIELD ? (int)id : -1, (int)carried})
    if (f >= 0 && m->own_stream && !m->f[f].d)
      return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: this model has no such field (closure = CATKEVerticalDiffusivity() only)", what);
  if (cmp != GB25_REGION_BELOW && cmp != GB25_REGION_ABOVE)
    return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: cmp must be GB25_REGION_BELOW or GB25_REGION_ABOVE, got %d", what, (int)cmp);
  if (threshold != threshold) return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: threshold is NaN", what);
  if (gb25_status s = diag_window(m, what, k_first, k_count, m->cfg.Nz, "levels (k_first, k_count)", &P->kc)) return s;
  if (max_regions < 1) return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: max_regions = %d must be >= 1", what, (int)max_regions);
  if ((long long)m->Nx * m->Ny > 0x7fffffffLL) return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: a level of %d x %d cells exceeds the 32-bit labels", what, m->Nx, m->Ny);
  P->kind = kind; P->id = id; P->param = param; P->carried = carried;
  P->above = cmp == GB25_REGION_ABOVE;
  P->threshold = threshold;
  P->k_first = k_first; P->max_regions = max_regions;
  P->Nx = m->Nx; P->Ny = m->Ny; P->n = m->Nx * m->Ny;
  P->blocks = (P->n + REG_THREADS - 1) / REG_THREADS;
  P->off_labels = region_align((size_t)P->kc * sizeof(RegionCounts));
  P->off_records = P->off_labels + region_align((size_t)P->n * P->kc * sizeof(int));
  P->off_work = P->off_records + region_align((size_t)max_regions * P->kc * sizeof(RegionRecord));
  P->off_num = P->off_work + region_align((size_t)P->n * sizeof(int));
  P->off_roots = P->off_num + region_align((size_t)P->n * sizeof(int));
  P->bytes = P->off_roots + region_align((size_t)P->blocks * sizeof(int));
  return GB25_OK;
}

inline RegionCounts* regions_counts(gb25_model* m) { return (RegionCounts*)m->diag.regions.p; }
inline int* regions_labels(gb25_model* m, const RegionPlan& P) { return (int*)((char*)m->diag.regions.p + P.off_labels); }
inline RegionRecord* regions_records(gb25_model* m, const RegionPlan& P) { return (RegionRecord*)((char*)m->diag.regions.p + P.off_records); }

// The criterion, then the launches of every level of the window, on m->stream; labels, records and counts lie in the buffer when
// the stream has run.
gb25_status regions_run(gb25_model* m, const char* what, const RegionPlan& P) {
  const real *x = nullptr, *y = nullptr;
  DiagBox box, ybox = {};
  if (P.carried >= 0) {
    if (gb25_status s = diag_source(m, (gb25_field)P.carried, &y)) return s;
    if (gb25_status s = diag_box(m, (gb25_field)P.carried, 0, &ybox)) return s;
  }
  if (P.kind == GB25_REGION_FIELD) {
    if (gb25_status s = diag_source(m, (gb25_field)P.id, &x)) return s;
    if (gb25_status s = diag_box(m, (gb25_field)P.id, 0, &box)) return s;
    box.origin += box.plane * P.k_first;
    if (gb25_status s = wait_for_model(m)) return s;
  } else {
    if (P.kind == GB25_REGION_DERIVED) {
      if (gb25_status s = derived_run(m, (gb25_derived)P.id, 0.0, P.k_first, P.kc, &x)) return s;
    } else {
      if (gb25_status s = kinematics_run(m, (gb25_kinematics)P.id, P.param, P.k_first, P.kc, &x)) return s;
    }
    box = DiagBox{P.Nx, P.Ny, P.kc, (long long)P.Nx, (long long)P.n, 0};   // (packed: the levels of the window alone)
  }
  if (gb25_status s = m->diag.regions.grow(m, what, "the labels, the records and the scratch of the regions", P.bytes)) return s;
  if (gb25_status s = moments_tables(m)) return s;
  const MomentsTables tab = diag_measure_tables(m, true);
  char* base = (char*)m->diag.regions.p;
  HIPCHK(hipMemsetAsync(base, 0, P.off_labels, m->stream));
  HIPCHK(hipMemsetAsync(base + P.off_records, 0, (size_t)P.max_regions * P.kc * sizeof(RegionRecord), m->stream));
  RegionArgs A = {};
  A.Nx = P.Nx; A.Ny = P.Ny; A.n = P.n;
  A.above = P.above;
  A.periodic = m->g.x_periodic ? 1 : 0;
  A.max_regions = P.max_regions;
  A.threshold = (real)P.threshold;
  A.work = (int*)(base + P.off_work);
  A.num = (int*)(base + P.off_num);
  A.block_roots = (int*)(base + P.off_roots);
  const dim3 cells((unsigned)P.blocks), blk(REG_THREADS);
  // (a region has at least one cell and two regions never touch: a level holds at most ceil(n / 2))
  const unsigned most = (unsigned)std::min<long long>(P.max_regions, ((long long)P.n + 1) / 2);
  Timed t(m, GB25_K_DIAGNOSTICS);
  for (int K = 0; K < P.kc; K++) {
    A.k = P.k_first + K;
    A.labels = regions_labels(m, P) + (size_t)P.n * K;
    A.records = regions_records(m, P) + (size_t)P.max_regions * K;
    A.counts = regions_counts(m) + K;
    DiagBox yb = ybox;
    yb.origin += yb.plane * A.k;
    hipLaunchKernelGGL(k_region_init<real>, cells, blk, 0, m->stream, m->g, tab, x, box, K, A);
    LAUNCHCHK();
    hipLaunchKernelGGL(k_region_flatten<false>, cells, blk, 0, m->stream, A);
    LAUNCHCHK();
    hipLaunchKernelGGL(k_region_merge, cells, blk, 0, m->stream, A);
    LAUNCHCHK();
    hipLaunchKernelGGL(k_region_flatten<true>, cells, blk, 0, m->stream, A);
    LAUNCHCHK();
    hipLaunchKernelGGL(k_region_scan, dim3(1), blk, 0, m->stream, A, P.blocks);
    LAUNCHCHK();
    hipLaunchKernelGGL(k_region_number, cells, blk, 0, m->stream, A);
    LAUNCHCHK();
    hipLaunchKernelGGL(k_region_rewrite, cells, blk, 0, m->stream, A);
    LAUNCHCHK();
    hipLaunchKernelGGL(k_region_records<real>, dim3(most), dim3(64), 0, m->stream, m->g, tab, x, box, K, y, yb, A);
    LAUNCHCHK();
  }
  return GB25_OK;
}

// checks, criterion, launches; then the counts to the host (the stream is quiet behind it) and the info records
gb25_status regions_of(gb25_model* m, const char* what, gb25_region_source kind, int32_t id, int32_t param, int32_t carried, gb25_region_cmp cmp,
                       double threshold, int32_t k_first, int32_t k_count, int32_t max_regions, gb25_regions_info* info, RegionPlan* P) {
  if (!info) return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: info is NULL", what);
  if (gb25_status s = regions_check(m, what, kind, id, param, carried, cmp, threshold, k_first, k_count, max_regions, P)) return s;
  if (gb25_status s = regions_single_domain(m, what)) return s;
  if (gb25_status s = diag_need_device(m, what)) return s;
  if (gb25_status s = regions_run(m, what, *P)) return s;
  std::vector<RegionCounts> c((size_t)P->kc);
  if (gb25_status s = diag_download(m, c.data(), regions_counts(m), c.size() * sizeof(RegionCounts))) return s;
  for (int K = 0; K < P->kc; K++) {
    if (c[K].gave_up)
      return fail(m, GB25_ERR_STATE, "%s: level %d: a union-find walk exhausted its %d hops; the labels of this level are not complete", what,
                  P->k_first + K, P->n);
    info[K].regions = c[K].regions;
    info[K].stored = std::min(c[K].regions, P->max_regions);
    info[K].foreground_cells = c[K].foreground;
    info[K].nonfinite_cells = c[K].nonfinite;
  }
  return GB25_OK;
}

}  // namespace

extern "C" {

int32_t gb25_region_bytes(void) { return (int32_t)sizeof(gb25_region); }
int32_t gb25_regions_info_bytes(void) { return (int32_t)sizeof(gb25_regions_info); }

gb25_status gb25_region_dims(const gb25_model* m, int32_t dims[3]) {
  if (!m || !dims) return GB25_ERR_INVALID_ARGUMENT;
  dims[0] = m->Nx; dims[1] = m->Ny; dims[2] = m->cfg.Nz;
  return GB25_OK;
}

gb25_status gb25_label_regions(gb25_model* m, gb25_region_source source_kind, int32_t id, int32_t param, int32_t carried_field,
                               gb25_region_cmp cmp, double threshold, int32_t k_first, int32_t k_count, int32_t max_regions,
                               const void** dev_labels, const void** dev_records, gb25_regions_info* info) {
  if (!m) return GB25_ERR_INVALID_ARGUMENT;
  const char* what = "gb25_label_regions";
  if (!dev_labels && !dev_records) return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: dev_labels and dev_records are both NULL: no output requested", what);
  RegionPlan P = {};
  if (gb25_status s = regions_of(m, what, source_kind, id, param, carried_field, cmp, threshold, k_first, k_count, max_regions, info, &P)) return s;
  if (dev_labels) *dev_labels = regions_labels(m, P);
  if (dev_records) *dev_records = regions_records(m, P);
  return GB25_OK;
}

gb25_status gb25_get_regions(gb25_model* m, gb25_region_source source_kind, int32_t id, int32_t param, int32_t carried_field,
                             gb25_region_cmp cmp, double threshold, int32_t k_first, int32_t k_count, int32_t max_regions, int32_t* labels,
                             gb25_region* records, gb25_regions_info* info) {
  if (!m) return GB25_ERR_INVALID_ARGUMENT;
  const char* what = "gb25_get_regions";
  if (!records) return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: records is NULL", what);
  RegionPlan P = {};
  if (gb25_status s = regions_of(m, what, source_kind, id, param, carried_field, cmp, threshold, k_first, k_count, max_regions, info, &P)) return s;
  // of every level the stored records alone, the planes where they were asked for
  memset(records, 0, (size_t)P.max_regions * P.kc * sizeof(gb25_region));
  for (int K = 0; K < P.kc; K++)
    if (info[K].stored)
      HIPCHK(hipMemcpyAsync(records + (size_t)P.max_regions * K, regions_records(m, P) + (size_t)P.max_regions * K,
                            (size_t)info[K].stored * sizeof(gb25_region), hipMemcpyDeviceToHost, m->stream));
  if (labels) HIPCHK(hipMemcpyAsync(labels, regions_labels(m, P), (size_t)P.n * P.kc * sizeof(int32_t), hipMemcpyDeviceToHost, m->stream));
  HIPCHK(hipStreamSynchronize(m->stream));
  return GB25_OK;
}

}  // extern "C"
