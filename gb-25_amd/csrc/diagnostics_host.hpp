// diagnostics_host.hpp -- host side of gb25_get_field_stats / gb25_compare_field / gb25_get_state_monitor /
// gb25_field_device_ptr_readonly / gb25_integrate_field / gb25_get_budget / gb25_compute_derived / gb25_get_derived /
// gb25_get_derived_stats / gb25_get_field_levels / gb25_get_transport (include/gb25.h); the last part of gb25_api.hip, which includes it.  Kernels:
// diagnostics_kernels.hpp; the memory: DiagState (diagnostics_state.hpp), m->diag.  Nothing here writes model memory or a schedule
// flag: the calls may sit between any two steps.  The first section holds what every diagnostic shares, averages_host.hpp,
// classes_host.hpp and particles_host.hpp included: diag_need_device, diag_window, diag_download, diag_upload, diag_room_for /
// diag_malloc / diag_alloc_zeroed, DiagBuffer::grow, diag_source; wait_for_model: gb25_api.hip (is_folded, has_north_wall and
// first_wet_level: gb25_api.hip, beside is_2d).  Three more pieces are written ONCE here for the families that reduce a field or a
// derived field (integrals, block sums, filters, spectra; DESIGN.md, "The host layer of the diagnostics"): the measure of a
// launch (diag_measure_tables, diag_with_loc), what a call reads (DiagSource: diag_source_plan without the device,
// diag_source_resolve with it), and the copy of planes and counts to the host (diag_download_planes).
#pragma once

namespace {

// ---- shared by every diagnostic
gb25_status diag_need_device(gb25_model* m, const char* what) {
  if (!m->own_stream) return fail(m, GB25_ERR_NO_DEVICE, "%s: this model has no device (gb25_create failed); libgb25hip has no CPU fallback", what);
  return GB25_OK;
}
// the window [first, first + count) of 0-based local interior indices of an extent; count = -1: all from first on.  noun: what
// the extent counts and what the caller names the two arguments
gb25_status diag_window(gb25_model* m, const char* what, int32_t first, int32_t count, int extent, const char* noun, int* n) {
  const long long c = count == -1 ? (long long)extent - first : (long long)count;
  if (first < 0 || first >= extent || count < -1 || count == 0 || first + c > extent)
    return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: window first = %d, count = %d of %d %s; 0-based local interior indices, count = -1: to the end",
                what, (int)first, (int)count, extent, noun);
  *n = (int)c;
  return GB25_OK;
}
// the tail of most entry points: the result to the host behind the launches, then the stream is quiet
gb25_status diag_download(gb25_model* m, void* host, const void* dev, size_t bytes) {
  HIPCHK(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, m->stream));
  HIPCHK(hipStreamSynchronize(m->stream));
  return GB25_OK;
}
// one of diagnostics' own tables: the values of h as T in a new allocation (*dst holds nothing: DiagState::release_tables)
template <class T, class S>
gb25_status diag_upload(gb25_model* m, const std::vector<S>& h, T** dst) {
  std::vector<T> a(h.size());
  for (size_t o = 0; o < h.size(); o++) a[o] = (T)h[o];
  HIPCHK(hipMalloc(dst, a.size() * sizeof(T)));
  HIPCHK(hipMemcpy(*dst, a.data(), a.size() * sizeof(T), hipMemcpyHostToDevice));
  return GB25_OK;
}
// An allocation that grows with what the caller asks for (gb25_averages_begin, gb25_particles_begin) is refused BEFORE hipMalloc
// when the device has fewer bytes free: nothing is allocated, nothing is evicted.  of: what the bytes are for.
gb25_status diag_room_for(gb25_model* m, const char* what, const char* of, double need) {
  size_t free_bytes = 0, device_bytes = 0;
  HIPCHK(hipMemGetInfo(&free_bytes, &device_bytes));
  if (need > (double)free_bytes) return fail(m, GB25_ERR_OUT_OF_MEMORY, "%s: %s need %.0f bytes, the device has %zu free", what, of, need, free_bytes);
  return GB25_OK;
}
// ... and then made: a failure is out of memory, not a HIP error that sticks, and leaves nothing allocated
gb25_status diag_malloc(gb25_model* m, const char* what, const char* of, size_t bytes, void** base) {
  const hipError_t e = hipMalloc(base, bytes);
  if (e == hipSuccess) return GB25_OK;
  (void)hipGetLastError();
  *base = nullptr;
  return fail(m, GB25_ERR_OUT_OF_MEMORY, "%s: hipMalloc of %zu bytes for %s failed: %s", what, bytes, of, hipGetErrorString(e));
}
// ... and zeroed
gb25_status diag_alloc_zeroed(gb25_model* m, const char* what, const char* of, size_t bytes, void** base) {
  if (gb25_status s = diag_malloc(m, what, of, bytes, base)) return s;
  if (hipMemsetAsync(*base, 0, bytes, m->stream) != hipSuccess || hipStreamSynchronize(m->stream) != hipSuccess) {
    (void)hipFree(*base);
    *base = nullptr;
    return fail(m, GB25_ERR_HIP, "%s: zeroing %s failed: %s", what, of, hipGetErrorString(hipGetLastError()));
  }
  return GB25_OK;
}

// a result buffer (diagnostics_state.hpp) with room for `need` bytes: the one it has, or a new one
gb25_status DiagBuffer::grow(gb25_model* m, const char* what, const char* of, size_t need) {
  if (p && need <= bytes) return GB25_OK;
  drop();
  if (gb25_status s = diag_room_for(m, what, of, (double)need)) return s;
  if (gb25_status s = diag_malloc(m, what, of, need, &p)) return s;
  bytes = need;
  return GB25_OK;
}

constexpr size_t DIAG_RECORD = 64;   // bytes of a slot of the scratch buffer: the largest per-block record
constexpr int DIAG_RESULTS = 8;      // result slots behind the per-block records (a state monitor fills seven)
static_assert(sizeof(StatsPartial) <= DIAG_RECORD && sizeof(DiffPartial) <= DIAG_RECORD && sizeof(CflPartial) <= DIAG_RECORD, "slot size");

inline long long diag_blocks(const DiagBox& b) { return ((long long)b.by * b.bz + DIAG_ROWS - 1) / DIAG_ROWS; }

// once per model: per-block records for the tallest box a field of this model has (w's parent), plus the result slots
gb25_status diag_scratch(gb25_model* m) {
  if (m->diag.scratch) return GB25_OK;
  const int H = m->cfg.halo;
  const long long rows = (long long)(m->Ny + 2 * H + 1) * (m->cfg.Nz + 2 * H + 1);
  const size_t records = (size_t)((rows + DIAG_ROWS - 1) / DIAG_ROWS);
  HIPCHK(hipMalloc(&m->diag.scratch, (records + DIAG_RESULTS) * DIAG_RECORD));
  m->diag.scratch_records = records;
  return GB25_OK;
}
inline void* diag_result_slot(gb25_model* m, int q) { return (char*)m->diag.scratch + (m->diag.scratch_records + q) * DIAG_RECORD; }

// The array that holds what gb25_get_field(id) would return, without moving anything: previous_velocities are read where they
// live (prev_uv_src), a stale pHY' is recomputed from the T, S it belongs to (the launch is filed under GB25_K_DIAGNOSTICS).
gb25_status diag_source(gb25_model* m, gb25_field id, const real** src) {
  if (id < 0 || id >= GB25_FIELD_COUNT) return GB25_ERR_INVALID_ARGUMENT;
  if (!m->f[id].d) return fail(m, GB25_ERR_INVALID_ARGUMENT, "this model has no such field (closure = CATKEVerticalDiffusivity() only)");
  if (m->route.memory_lacks_correction())   // (only after a composite call that failed half-way)
    if (gb25_status s = materialize_uv(m)) return s;
  if (id == GB25_PHY && m->phy_stale) {
    m->prof_redirect = GB25_K_DIAGNOSTICS;
    const gb25_status s = compute_p_impl(m, PressureBox::whole(launch_facts(m)));
    m->prof_redirect = -1;
    if (s) return s;
  }
  *src = m->f[id].d;
  if ((id == GB25_PREV_U || id == GB25_PREV_V) && m->catke && m->prev_uv_src != 0) {
    const int q = id - GB25_PREV_U;
    *src = m->prev_uv_src == 1 ? m->f[GB25_U + q].d : m->ahead_uv[q].d;
  }
  return GB25_OK;
}

gb25_status diag_box(const gb25_model* m, gb25_field id, int include_halos, DiagBox* b) {
  int32_t d[3];
  if (gb25_field_dims(m, id, include_halos, d)) return GB25_ERR_INVALID_ARGUMENT;
  const Field& F = m->f[id];
  const long long H = include_halos ? 0 : m->cfg.halo;
  b->bx = d[0]; b->by = d[1]; b->bz = d[2];
  b->pitch = F.nx;
  b->plane = (long long)F.nx * F.ny;
  b->origin = H + b->pitch * H + b->plane * (is_2d(id) ? 0 : H);
  return GB25_OK;
}
// position + global_offset = 1-based index into the global interior
void diag_global_offset(const gb25_model* m, gb25_field id, int include_halos, int32_t off[3]) {
  const int H = include_halos ? m->cfg.halo : 0;
  off[0] = m->rx * m->Nx - H;
  off[1] = m->j0 - H;
  off[2] = is_2d(id) ? 0 : -H;
}
void diag_position(long long at, const DiagBox& b, int32_t pos[3]) {
  if (at == DIAG_NONE) {
    pos[0] = pos[1] = pos[2] = 0;
    return;
  }
  pos[0] = (int32_t)(at % b.bx) + 1;
  pos[1] = (int32_t)((at / b.bx) % b.by) + 1;
  pos[2] = (int32_t)(at / ((long long)b.bx * b.by)) + 1;
}

template <class P>
gb25_status diag_finish(gb25_model* m, long long nblocks, int slot) {
  hipLaunchKernelGGL(k_diag_finish<P>, dim3(1), dim3(DIAG_THREADS), 0, m->stream, (const P*)m->diag.scratch, (int)nblocks,
                     (P*)diag_result_slot(m, slot));
  LAUNCHCHK();
  return GB25_OK;
}
gb25_status diag_launch_stats(gb25_model* m, const real* src, const DiagBox& b, int slot) {
  const long long nb = diag_blocks(b);
  hipLaunchKernelGGL(k_field_stats<real>, dim3((unsigned)nb), dim3(DIAG_THREADS), 0, m->stream, src, b, (StatsPartial*)m->diag.scratch);
  LAUNCHCHK();
  return diag_finish<StatsPartial>(m, nb, slot);
}
void diag_fill_stats(const gb25_model* m, gb25_field id, const StatsPartial& p, const DiagBox& b, int include_halos, gb25_field_stats* out) {
  memset(out, 0, sizeof *out);
  out->min = p.mn; out->max = p.mx;
  out->max_abs = p.amax < 0 ? 0.0 : p.amax;
  out->sum = p.sum; out->sum_sq = p.sumsq;
  out->count = (int64_t)b.bx * b.by * b.bz;
  out->nonfinite = p.nonfinite;
  diag_position(p.amax < 0 ? DIAG_NONE : p.at, b, out->at_max_abs);
  diag_position(p.first, b, out->first_nonfinite);
  diag_global_offset(m, id, include_halos, out->global_offset);
}
gb25_status diag_check_box(gb25_model* m, const DiagBox& b) {
  if (b.bx <= 0 || b.by <= 0 || b.bz <= 0) return fail(m, GB25_ERR_INVALID_ARGUMENT, "the field has an empty box");
  if ((size_t)diag_blocks(b) > m->diag.scratch_records) return fail(m, GB25_ERR_STATE, "diagnostics: the box needs more per-block records than the model's scratch buffer holds");
  return GB25_OK;
}

// launch, finish, download and fill: the statistics of the box b of src (gb25_get_field_stats, gb25_get_derived_stats)
gb25_status diag_stats_of(gb25_model* m, gb25_field id, const real* src, const DiagBox& b, int include_halos, gb25_field_stats* out) {
  {
    Timed t(m, GB25_K_DIAGNOSTICS);
    if (gb25_status s = diag_launch_stats(m, src, b, 0)) return s;
  }
  StatsPartial p;
  if (gb25_status s = diag_download(m, &p, diag_result_slot(m, 0), sizeof p)) return s;
  diag_fill_stats(m, id, p, b, include_halos, out);
  return GB25_OK;
}

// ---- integrals: the measure's location of a field, diagnostics' own tables, the records' buffer
static_assert(sizeof(MomentsPartial) == sizeof(gb25_moments), "a row record is a gb25_moments");

MomentLoc moments_loc(int id) {
  const bool flat = is_2d(id);
  if (is_v_shaped(id)) return flat ? LOC_CF : LOC_CFC;
  switch (id) {
    case GB25_U: case GB25_GN_U: case GB25_GM_U: case GB25_PREV_U: return LOC_FCC;
    case GB25_BT_U: case GB25_U_BAR: case GB25_GN_BT_U: return LOC_FC;
    case GB25_W: case GB25_KAPPA_U: case GB25_KAPPA_C: case GB25_KAPPA_E: return LOC_CCF;
    default: return flat ? LOC_CC : LOC_CCC;
  }
}

// areas by location as `real` (what gb25_get_metric2 returns, rounded back: exact) and the first wet level per column and
// location, from the host's tables; parent layout of a (c,f) field
gb25_status moments_tables(gb25_model* m) {
  if (m->diag.tables_valid) return GB25_OK;
  const int Nx = m->Nx, Ny = m->Ny, Nz = m->cfg.Nz, H = m->cfg.halo, sx = Nx + 2 * H, sy = Ny + 2 * H + 1;
  const size_t n2 = (size_t)sx * sy;
  DiagState& D = m->diag;
  D.release_tables();
  // the derived fields' own: (double) of zc[0 .. Nz) | zf[0 .. Nz] as gb25_get_metric returns them
  std::vector<double> zt((size_t)2 * Nz + 1);
  for (int k = 0; k < Nz; k++) zt[k] = (double)(real)m->h_metric[GB25_M_ZC][m->metric_off_k + k];
  for (int k = 0; k <= Nz; k++) zt[Nz + k] = (double)(real)m->h_metric[GB25_M_ZF][m->metric_off_k + k];
  if (gb25_status s = diag_upload(m, zt, &D.zt)) return s;
  if (m->g.cv.on) {
    // of a curvilinear grid: the derived fields' AZFF, the integrals' areas by location, the transports' lengths of the y faces
    // (DXCF) and of the x faces (DYFC), the stability diagnostics' Coriolis parameter at (f,f)
    const struct { int id; const char* name; real** dst; } metrics[] = {
        {GB25_M2_AZFF, "AZFF", &D.azff},    {GB25_M2_AZCC, "AZCC", &D.area[0]},        {GB25_M2_AZFC, "AZFC", &D.area[1]},
        {GB25_M2_AZCF, "AZCF", &D.area[2]}, {GB25_M2_DXCF, "DXCF", &D.face_length[0]}, {GB25_M2_DYFC, "DYFC", &D.face_length[1]},
        {GB25_M2_FFF, "FFF", &D.fff}};
    for (const auto& c : metrics) {
      if (m->h_curv[c.id].size() != n2) return fail(m, GB25_ERR_STATE, "diagnostics: the curvilinear metric %s is not built", c.name);
      if (gb25_status s = diag_upload(m, m->h_curv[c.id], c.dst)) return s;
    }
  }
  if (!m->kbot.empty()) {
    auto kb = [&](int ii, int jj) { return first_wet_level(m, ii, jj); };
    std::vector<unsigned short> f(n2);
    for (int q = 0; q < 3; q++) {
      std::fill(f.begin(), f.end(), MOMENTS_DRY);
      for (int j = 0; j <= Ny; j++) {
        if (j == Ny && q != 2) continue;   // (only y faces have a row Ny)
        for (int i = 0; i < Nx; i++) {
          const int k = q == 0 ? kb(i, j) : q == 1 ? std::max(kb(i - 1, j), kb(i, j)) : std::max(kb(i, j - 1), kb(i, j));
          f[(size_t)(i + H) + (size_t)sx * (j + H)] = k < Nz ? (unsigned short)k : MOMENTS_DRY;
        }
      }
      if (gb25_status s = diag_upload(m, f, &D.first_wet[q])) return s;
    }
    // the stability diagnostics' own: the (c,c) columns and the ring around them, [-1, Nx] x [-1, Ny]
    std::fill(f.begin(), f.end(), MOMENTS_DRY);
    for (int j = -1; j <= Ny; j++)
      for (int i = -1; i <= Nx; i++) {
        const int k = kb(i, j);
        f[(size_t)(i + H) + (size_t)sx * (j + H)] = k < Nz ? (unsigned short)k : MOMENTS_DRY;
      }
    if (gb25_status s = diag_upload(m, f, &D.first_wet_ring)) return s;
  }
  D.tables_valid = true;
  return GB25_OK;
}

// once per model: MOMENTS_SLOTS sets of row records for the tallest interior a field of this model has, their level records,
// their totals
gb25_status moments_buffer(gb25_model* m) {
  if (m->diag.moments) return GB25_OK;
  const size_t levels = (size_t)m->cfg.Nz + 1, rows = (size_t)(m->Ny + 1) * levels;
  HIPCHK(hipMalloc(&m->diag.moments, (size_t)MOMENTS_SLOTS * (rows + levels + 1) * sizeof(MomentsPartial)));
  m->diag.moments_rows = rows;
  m->diag.moments_levels = levels;
  return GB25_OK;
}
inline MomentsPartial* moments_rows(gb25_model* m, int slot) { return (MomentsPartial*)m->diag.moments + m->diag.moments_rows * slot; }
inline MomentsPartial* moments_levels(gb25_model* m, int slot) {
  return (MomentsPartial*)m->diag.moments + m->diag.moments_rows * MOMENTS_SLOTS + m->diag.moments_levels * slot;
}
inline MomentsPartial* moments_totals(gb25_model* m) {
  return (MomentsPartial*)m->diag.moments + (m->diag.moments_rows + m->diag.moments_levels) * MOMENTS_SLOTS;
}
gb25_status moments_check_box(gb25_model* m, const DiagBox& b) {
  if (b.bx <= 0 || b.by <= 0 || b.bz <= 0) return fail(m, GB25_ERR_INVALID_ARGUMENT, "the field has an empty box");
  if ((size_t)b.by * b.bz > m->diag.moments_rows || (size_t)b.bz > m->diag.moments_levels)
    return fail(m, GB25_ERR_STATE, "integrals: the box needs more row records than the model's buffer holds");
  return GB25_OK;
}

// What a kernel reads of them (moments_tables has run): the areas and the first wet levels by horizontal location, and the local
// row of the pivot row of a folded grid.  fold_applies: the points of the launch lie ON that row (cells, x faces) -- the y faces
// of the transports and of the class sums do not, and pass false.  (TransportTables and ClassTables take their parts from it.)
MomentsTables diag_measure_tables(const gb25_model* m, bool fold_applies) {
  MomentsTables tab;
  for (int q = 0; q < 3; q++) {
    tab.area[q] = m->diag.area[q];
    tab.first[q] = m->diag.first_wet[q];
  }
  tab.pivot_row = (fold_applies && is_folded(m)) ? m->Ny - 1 : -1;
  return tab;
}
// f(std::integral_constant<int, LOC>) for the location loc: how a MomentLoc becomes the template argument of a kernel
template <class F>
void diag_with_loc(MomentLoc loc, F&& f) {
  switch (loc) {
    case LOC_CCC: f(std::integral_constant<int, LOC_CCC>()); break;
    case LOC_FCC: f(std::integral_constant<int, LOC_FCC>()); break;
    case LOC_CFC: f(std::integral_constant<int, LOC_CFC>()); break;
    case LOC_CCF: f(std::integral_constant<int, LOC_CCF>()); break;
    case LOC_CC: f(std::integral_constant<int, LOC_CC>()); break;
    case LOC_FC: f(std::integral_constant<int, LOC_FC>()); break;
    case LOC_CF: f(std::integral_constant<int, LOC_CF>()); break;
  }
}

// the row records of field id into slot `slot`
gb25_status moments_launch(gb25_model* m, gb25_field id, const real* src, const DiagBox& b, int slot) {
  const MomentsTables tab = diag_measure_tables(m, true);
  MomentsPartial* rows = moments_rows(m, slot);
  const long long nb = ((long long)b.by * b.bz + DIAG_THREADS / 64 - 1) / (DIAG_THREADS / 64);
  diag_with_loc(moments_loc(id), [&](auto loc) {
    hipLaunchKernelGGL((k_field_moments<real, decltype(loc)::value>), dim3((unsigned)nb), dim3(DIAG_THREADS), 0, m->stream, m->g, tab, src, b, rows);
  });
  LAUNCHCHK();
  return GB25_OK;
}
// rows -> levels -> totals of the first n slots, two launches
gb25_status moments_fold(gb25_model* m, const DiagBox* b, int n) {
  MomentsFold f = {}, t = {};
  int most = 0;
  for (int s = 0; s < n; s++) {
    f.len[s] = b[s].by; f.n[s] = b[s].bz;
    t.len[s] = b[s].bz; t.n[s] = 1;
    most = std::max(most, b[s].bz);
  }
  hipLaunchKernelGGL(k_moments_fold, dim3(most, n), dim3(64), 0, m->stream, (const MomentsPartial*)moments_rows(m, 0),
                     (long long)m->diag.moments_rows, f, moments_levels(m, 0), (long long)m->diag.moments_levels);
  LAUNCHCHK();
  hipLaunchKernelGGL(k_moments_fold, dim3(1, n), dim3(64), 0, m->stream, (const MomentsPartial*)moments_levels(m, 0),
                     (long long)m->diag.moments_levels, t, moments_totals(m), 1LL);
  LAUNCHCHK();
  return GB25_OK;
}


// ---- derived fields
// interior extents of a derived field, from the configuration alone (no device): zeta has the rows of v -- one more than the
// cells below a wall, as many on a folded grid and below a northern neighbour rank
void derived_extents(const gb25_model* m, gb25_derived q, int32_t d[3]) {
  d[0] = m->Nx;
  d[1] = m->Ny + ((q == GB25_D_VORTICITY && has_north_wall(m)) ? 1 : 0);
  d[2] = q == GB25_D_MIXED_LAYER_DEPTH ? 1 : m->cfg.Nz;
}
gb25_status derived_check(gb25_model* m, const char* what, gb25_derived q, double param) {
  if (q < 0 || q >= GB25_D_COUNT) return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: no derived field %d (0 .. %d)", what, (int)q, GB25_D_COUNT - 1);
  if (q == GB25_D_MIXED_LAYER_DEPTH && !(param > 0.0))
    return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: the mixed-layer depth needs a density threshold > 0 kg/m^3 as param, got %g", what, param);
  return GB25_OK;
}
// once per model: one 2-D plane, then room for the largest interior a field has (w: Nz + 1 levels; v: Ny + 1 rows)
gb25_status derived_scratch(gb25_model* m) {
  if (m->diag.derived) return GB25_OK;
  const size_t plane = (size_t)m->Nx * (m->Ny + 1);
  m->diag.derived_plane = (plane + 3) & ~(size_t)3;   // (the 3-D part starts on a 16-byte boundary)
  m->diag.derived_elems = m->diag.derived_plane + plane * ((size_t)m->cfg.Nz + 1);
  HIPCHK(hipMalloc(&m->diag.derived, m->diag.derived_elems * sizeof(real)));
  return GB25_OK;
}
inline dim3 derived_grid(int bx, int by, int kc) { return dim3((bx + 63) / 64, (by + 3) / 4, (kc + DER_LEVELS - 1) / DER_LEVELS); }

// The launches of one derived field, levels [k0, k0 + kc), on m->stream behind the model; *result: where the packed result lies.
gb25_status derived_run(gb25_model* m, gb25_derived q, double param, int k0, int kc, const real** result) {
  const bool vel = q == GB25_D_VORTICITY || q == GB25_D_KINETIC_ENERGY;
  const real *a = nullptr, *b = nullptr;
  if (gb25_status s = diag_source(m, vel ? GB25_U : GB25_T, &a)) return s;
  if (gb25_status s = diag_source(m, vel ? GB25_V : GB25_S, &b)) return s;
  if (gb25_status s = derived_scratch(m)) return s;
  if (gb25_status s = wait_for_model(m)) return s;
  if (gb25_status s = moments_tables(m)) return s;
  int32_t e[3];
  derived_extents(m, q, e);
  const Grid& g = m->g;
  const dim3 blk(64, 4);
  Timed t(m, GB25_K_DIAGNOSTICS);
  if (q == GB25_D_MIXED_LAYER_DEPTH) {
    // sigma of every level into the 3-D part (the very values gb25_get_derived(GB25_D_POTENTIAL_DENSITY) hands out), then the march
    real* sigma = m->diag.derived + m->diag.derived_plane;
    const DerivedOut d{sigma, e[0], e[1], 0, g.Nz};
    hipLaunchKernelGGL(k_derived_density<true>, derived_grid(e[0], e[1], g.Nz), blk, 0, m->stream, g, a, b, m->diag.eos0, m->diag.first_wet[0], d);
    LAUNCHCHK();
    hipLaunchKernelGGL(k_derived_mixed_layer, dim3((e[0] + 63) / 64, (e[1] + 3) / 4), blk, 0, m->stream, g, (const real*)sigma,
                       m->diag.first_wet[0], (const double*)m->diag.zt, param, m->diag.derived, e[0], e[1]);
    LAUNCHCHK();
    *result = m->diag.derived;
    return GB25_OK;
  }
  real* out = m->diag.derived + m->diag.derived_plane;
  const DerivedOut d{out, e[0], e[1], k0, kc};
  const dim3 grd = derived_grid(e[0], e[1], kc);
  switch (q) {
    case GB25_D_VORTICITY:
      if (g.cv.on) hipLaunchKernelGGL(k_derived_vorticity<true>, grd, blk, 0, m->stream, g, a, b, (const real*)m->diag.azff, d);
      else hipLaunchKernelGGL(k_derived_vorticity<false>, grd, blk, 0, m->stream, g, a, b, (const real*)nullptr, d);
      break;
    case GB25_D_KINETIC_ENERGY: hipLaunchKernelGGL(k_derived_kinetic_energy, grd, blk, 0, m->stream, g, a, b, d); break;
    case GB25_D_DENSITY_ANOMALY:
      hipLaunchKernelGGL(k_derived_density<false>, grd, blk, 0, m->stream, g, a, b, m->diag.eos0, m->diag.first_wet[0], d);
      break;
    default:
      hipLaunchKernelGGL(k_derived_density<true>, grd, blk, 0, m->stream, g, a, b, m->diag.eos0, m->diag.first_wet[0], d);
      break;
  }
  LAUNCHCHK();
  *result = out;
  return GB25_OK;
}

// What gb25_compute_derived and gb25_get_derived share: the checks, the window of levels, the launches.  e: the packed dims of
// the result (e[2]: the levels of the window).
gb25_status derived_window_run(gb25_model* m, const char* what, gb25_derived q, double param, int32_t k_first, int32_t k_count, int32_t e[3],
                               const real** result) {
  if (gb25_status s = derived_check(m, what, q, param)) return s;
  int kc = 0;
  derived_extents(m, q, e);
  if (gb25_status s = diag_window(m, what, k_first, k_count, e[2], "levels (k_first, k_count)", &kc)) return s;
  if (gb25_status s = diag_need_device(m, what)) return s;
  if (gb25_status s = derived_run(m, q, param, k_first, kc, result)) return s;
  e[2] = kc;
  return GB25_OK;
}

// ---- what a call reads: a field of the model, or a derived field with its parameter (block sums, filters, spectra)
struct DiagSource {
  bool is_derived;
  gb25_field field;
  gb25_derived derived;
  double param;
  DiagSource(gb25_field f) : is_derived(false), field(f), derived(GB25_D_VORTICITY), param(0.0) {}
  DiagSource(gb25_derived q, double par) : is_derived(true), field(GB25_T), derived(q), param(par) {}
};
// what its plan says without the device: the interior extents of the source itself (columns; ITS rows -- a y-face field and the
// vorticity have one more than the cells below a wall --; its levels) and where its measure lives
struct SourcePlan {
  int32_t dims[3];
  MomentLoc loc;   // (of GB25_D_VORTICITY, at (f,f,c): none -- diag_source_measured)
};
// The checks of the source that need no device -- the id, "this model has no such field", the parameter -- and its plan
gb25_status diag_source_plan(gb25_model* m, const char* what, const DiagSource& S, SourcePlan* P) {
  if (S.is_derived) {
    if (gb25_status s = derived_check(m, what, S.derived, S.param)) return s;
    derived_extents(m, S.derived, P->dims);
    P->loc = S.derived == GB25_D_MIXED_LAYER_DEPTH ? LOC_CC : LOC_CCC;
    return GB25_OK;
  }
  const gb25_field f = S.field;
  if (f < 0 || f >= GB25_FIELD_COUNT) return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: no field %d", what, (int)f);
  if (m->own_stream && !m->f[f].d)
    return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: this model has no such field (closure = CATKEVerticalDiffusivity() only)", what);
  // (from the configuration alone, what gb25_field_dims says of the interior)
  P->loc = moments_loc(f);
  P->dims[0] = m->Nx;
  P->dims[1] = m->Ny + ((is_v_shaped(f) && has_north_wall(m)) ? 1 : 0);
  P->dims[2] = P->loc >= LOC_CC ? 1 : m->cfg.Nz + (P->loc == LOC_CCF ? 1 : 0);
  return GB25_OK;
}
// ... for the families that weigh with the measure (not the spectra): every source but one has it
gb25_status diag_source_measured(gb25_model* m, const char* what, const DiagSource& S) {
  if (S.is_derived && S.derived == GB25_D_VORTICITY)
    return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: derived GB25_D_VORTICITY lives at (f,f,c), for which the measure is not defined", what);
  return GB25_OK;
}
// The source on the device, levels [k_first, k_first + kc) of it: *src and the box whose origin is element (0, 0, k_first).  A
// field is read where it lies (diag_source), in its parent's pitch and plane, all its levels behind the origin, once the model
// has been waited for; a derived field is gb25_compute_derived's launches on m->stream behind the model (derived_run) into the
// model's packed array, which holds the kc levels of the window alone.
gb25_status diag_source_resolve(gb25_model* m, const DiagSource& S, const SourcePlan& P, int k_first, int kc, const real** src, DiagBox* b) {
  if (S.is_derived) {
    if (gb25_status s = derived_run(m, S.derived, S.param, k_first, kc, src)) return s;
    *b = DiagBox{P.dims[0], P.dims[1], kc, (long long)P.dims[0], (long long)P.dims[0] * P.dims[1], 0};
    return GB25_OK;
  }
  if (gb25_status s = diag_source(m, S.field, src)) return s;
  if (gb25_status s = diag_box(m, S.field, 0, b)) return s;
  if (gb25_status s = wait_for_model(m)) return s;
  b->origin += b->plane * k_first;
  return GB25_OK;
}

// ---- planes and counts (block sums, filters): the counts' slot in front of a family's buffer, and the way to the host
constexpr size_t COUNTS_HEAD = 32;   // bytes: BlockCounts, padded
static_assert(sizeof(BlockCounts) <= COUNTS_HEAD, "the counts fit their slot");
// those of the planes measure | first | second (elems doubles each, one after another from `planes`) that host[] asks for,
// then the counts: behind the launches, and the stream is quiet when it returns
gb25_status diag_download_planes(gb25_model* m, double* const host[3], const double* planes, size_t elems, const BlockCounts* counts, BlockCounts* c) {
  for (int q = 0; q < 3; q++)
    if (host[q]) HIPCHK(hipMemcpyAsync(host[q], planes + q * elems, elems * sizeof(double), hipMemcpyDeviceToHost, m->stream));
  return diag_download(m, c, counts, sizeof *c);
}

// ---- transports
static_assert(sizeof(TransportPartial) == sizeof(gb25_transport), "a line record is a gb25_transport");

// once per model: LINES [N Nz], the running sums [N (Nz + 1)] and PROFILE [N] for the longest set of lines a call can ask for
// (N = by of v for the y faces, Nx for the x faces); the three parts start at multiples of that longest N
gb25_status transport_buffer(gb25_model* m) {
  if (m->diag.transport) return GB25_OK;
  const size_t lines = (size_t)std::max(m->Nx, m->Ny + 1);
  HIPCHK(hipMalloc(&m->diag.transport, lines * (2 * (size_t)m->cfg.Nz + 2) * sizeof(TransportPartial)));
  m->diag.transport_lines = lines;
  return GB25_OK;
}
inline TransportPartial* transport_lines(gb25_model* m) { return (TransportPartial*)m->diag.transport; }
inline TransportPartial* transport_psi(gb25_model* m) { return transport_lines(m) + m->diag.transport_lines * m->cfg.Nz; }
inline TransportPartial* transport_profile(gb25_model* m) { return transport_psi(m) + m->diag.transport_lines * (m->cfg.Nz + 1); }

}  // namespace

extern "C" {

int32_t gb25_transport_bytes(void) { return (int32_t)sizeof(gb25_transport); }

gb25_status gb25_get_transport(gb25_model* m, gb25_transport_faces faces, gb25_transport_shape shape, int32_t along_first,
                               int32_t along_count, gb25_transport* out, int64_t count) {
  if (!m || !out) return GB25_ERR_INVALID_ARGUMENT;
  if (faces != GB25_ACROSS_Y && faces != GB25_ACROSS_X)
    return fail(m, GB25_ERR_INVALID_ARGUMENT, "gb25_get_transport: faces must be GB25_ACROSS_Y or GB25_ACROSS_X, got %d", (int)faces);
  if (shape != GB25_TR_LINES && shape != GB25_TR_PROFILE && shape != GB25_TR_STREAMFUNCTION)
    return fail(m, GB25_ERR_INVALID_ARGUMENT, "gb25_get_transport: shape must be GB25_TR_LINES, GB25_TR_PROFILE or GB25_TR_STREAMFUNCTION, got %d", (int)shape);
  const bool ay = faces == GB25_ACROSS_Y;
  int32_t d[3];
  if (gb25_field_dims(m, ay ? GB25_V : GB25_U, 0, d)) return GB25_ERR_INVALID_ARGUMENT;
  const int Nz = d[2], N = ay ? d[1] : d[0], along = ay ? d[0] : d[1];   // lines; the extent of the summed index
  int n = 0;
  if (gb25_status s = diag_window(m, "gb25_get_transport", along_first, along_count, along,
                                  ay ? "columns (along_first, along_count)" : "rows (along_first, along_count)", &n))
    return s;
  const int64_t want = shape == GB25_TR_LINES ? (int64_t)N * Nz : shape == GB25_TR_PROFILE ? (int64_t)N : (int64_t)N * (Nz + 1);
  if (count != want)
    return fail(m, GB25_ERR_INVALID_ARGUMENT, "gb25_get_transport: this shape has %lld records (lines %d, levels %d), count is %lld",
                (long long)want, N, Nz, (long long)count);
  if (gb25_status s = diag_need_device(m, "gb25_get_transport")) return s;
  const real *vel = nullptr, *T = nullptr, *S = nullptr;
  if (gb25_status s = diag_source(m, ay ? GB25_V : GB25_U, &vel)) return s;
  if (gb25_status s = diag_source(m, GB25_T, &T)) return s;
  if (gb25_status s = diag_source(m, GB25_S, &S)) return s;
  if (gb25_status s = transport_buffer(m)) return s;
  if ((size_t)N > m->diag.transport_lines) return fail(m, GB25_ERR_STATE, "gb25_get_transport: more lines than the model's buffer holds");
  if (gb25_status s = wait_for_model(m)) return s;
  if (gb25_status s = moments_tables(m)) return s;
  const Grid& g = m->g;
  const MomentsTables measure = diag_measure_tables(m, !ay);
  const TransportTables tab = {m->diag.face_length[ay ? 0 : 1], measure.first[ay ? 2 : 1], measure.pivot_row};
  TransportPartial* lines = transport_lines(m);
  {
    Timed t(m, GB25_K_DIAGNOSTICS);
    if (ay) {
      const long long nb = ((long long)N * Nz + DIAG_THREADS / 64 - 1) / (DIAG_THREADS / 64);
      if (g.cv.on) hipLaunchKernelGGL(k_transport_rows<true>, dim3((unsigned)nb), dim3(DIAG_THREADS), 0, m->stream, g, tab, vel, T, S, (int)along_first, n, N, lines);
      else hipLaunchKernelGGL(k_transport_rows<false>, dim3((unsigned)nb), dim3(DIAG_THREADS), 0, m->stream, g, tab, vel, T, S, (int)along_first, n, N, lines);
    } else {
      const dim3 grd((N + 63) / 64, (Nz + 3) / 4), blk(64, 4);
      if (g.cv.on) hipLaunchKernelGGL(k_transport_columns<true>, grd, blk, 0, m->stream, g, tab, vel, T, S, (int)along_first, n, lines);
      else hipLaunchKernelGGL(k_transport_columns<false>, grd, blk, 0, m->stream, g, tab, vel, T, S, (int)along_first, n, lines);
    }
    LAUNCHCHK();
    if (shape != GB25_TR_LINES) {
      hipLaunchKernelGGL(k_transport_fold, dim3((N + 63) / 64), dim3(64), 0, m->stream, (const TransportPartial*)lines, N, Nz,
                         transport_psi(m), transport_profile(m));
      LAUNCHCHK();
    }
  }
  const TransportPartial* from = shape == GB25_TR_LINES ? lines : shape == GB25_TR_PROFILE ? transport_profile(m) : transport_psi(m);
  return diag_download(m, out, from, (size_t)count * sizeof(gb25_transport));
}

gb25_status gb25_derived_dims(const gb25_model* m, gb25_derived q, int32_t dims[3]) {
  if (!m || !dims || q < 0 || q >= GB25_D_COUNT) return GB25_ERR_INVALID_ARGUMENT;
  derived_extents(m, q, dims);
  return GB25_OK;
}

gb25_status gb25_compute_derived(gb25_model* m, gb25_derived q, double param, int32_t k_first, int32_t k_count, const void** dev,
                                 int32_t device_dims[3]) {
  if (!m) return GB25_ERR_INVALID_ARGUMENT;
  if (!dev) return fail(m, GB25_ERR_INVALID_ARGUMENT, "gb25_compute_derived: dev is NULL");
  int32_t e[3];
  const real* out = nullptr;
  if (gb25_status s = derived_window_run(m, "gb25_compute_derived", q, param, k_first, k_count, e, &out)) return s;
  HIPCHK(hipStreamSynchronize(m->stream));
  *dev = out;
  if (device_dims) memcpy(device_dims, e, sizeof e);
  return GB25_OK;
}

gb25_status gb25_get_derived(gb25_model* m, gb25_derived q, double param, int32_t k_first, int32_t k_count, void* host) {
  if (!m) return GB25_ERR_INVALID_ARGUMENT;
  if (!host) return fail(m, GB25_ERR_INVALID_ARGUMENT, "gb25_get_derived: host is NULL");
  int32_t e[3];
  const real* out = nullptr;
  if (gb25_status s = derived_window_run(m, "gb25_get_derived", q, param, k_first, k_count, e, &out)) return s;
  return diag_download(m, host, out, (size_t)e[0] * e[1] * e[2] * sizeof(real));
}

gb25_status gb25_get_derived_stats(gb25_model* m, gb25_derived q, double param, gb25_field_stats* out) {
  if (!m) return GB25_ERR_INVALID_ARGUMENT;
  if (!out) return fail(m, GB25_ERR_INVALID_ARGUMENT, "gb25_get_derived_stats: out is NULL");
  if (gb25_status s = derived_check(m, "gb25_get_derived_stats", q, param)) return s;
  if (gb25_status s = diag_need_device(m, "gb25_get_derived_stats")) return s;
  int32_t e[3];
  derived_extents(m, q, e);
  const DiagBox b{e[0], e[1], e[2], (long long)e[0], (long long)e[0] * e[1], 0};
  if (gb25_status s = diag_scratch(m)) return s;
  if (gb25_status s = diag_check_box(m, b)) return s;
  const real* src = nullptr;
  if (gb25_status s = derived_run(m, q, param, 0, e[2], &src)) return s;
  return diag_stats_of(m, GB25_T, src, b, 0, out);   // (interior: the offsets are those of any field of the rank, 0 in k)
}

gb25_status gb25_get_field_levels(gb25_model* m, gb25_field f, int32_t k_first, int32_t k_count, void* host) {
  if (!m) return GB25_ERR_INVALID_ARGUMENT;
  if (f < 0 || f >= GB25_FIELD_COUNT) return fail(m, GB25_ERR_INVALID_ARGUMENT, "gb25_get_field_levels: no field %d", (int)f);
  if (!host) return fail(m, GB25_ERR_INVALID_ARGUMENT, "gb25_get_field_levels: host is NULL");
  if (k_first < 0 || k_count < -1 || k_count == 0)   // (what no extent can make right: refused before the device is asked for, a stale pHY' recomputed)
    return fail(m, GB25_ERR_INVALID_ARGUMENT, "gb25_get_field_levels: levels k_first = %d, k_count = %d (0-based interior levels; k_count = -1: all)",
                (int)k_first, (int)k_count);
  if (gb25_status s = diag_need_device(m, "gb25_get_field_levels")) return s;
  const real* src = nullptr;
  DiagBox b;
  int kc = 0;
  if (gb25_status s = diag_source(m, f, &src)) return s;
  if (gb25_status s = diag_box(m, f, 0, &b)) return s;
  if (gb25_status s = diag_window(m, "gb25_get_field_levels", k_first, k_count, b.bz, "levels (k_first, k_count)", &kc)) return s;
  if (gb25_status s = derived_scratch(m)) return s;
  const size_t n = (size_t)b.bx * b.by * kc;
  if (n > m->diag.derived_elems - m->diag.derived_plane) return fail(m, GB25_ERR_STATE, "gb25_get_field_levels: the levels need more room than the model's result array has");
  if (gb25_status s = wait_for_model(m)) return s;
  b.origin += b.plane * k_first;
  b.bz = kc;
  real* out = m->diag.derived + m->diag.derived_plane;
  {
    Timed t(m, GB25_K_DIAGNOSTICS);
    constexpr int VW = 16 / sizeof(real);
    const int chunks = (b.bx + VW - 1) / VW + 1;
    hipLaunchKernelGGL(k_gather_levels<real>, dim3((chunks + 63) / 64, (b.by + 3) / 4, kc), dim3(64, 4), 0, m->stream, src, b, out);
    LAUNCHCHK();
  }
  return diag_download(m, host, out, n * sizeof(real));
}

int32_t gb25_field_stats_bytes(void) { return (int32_t)sizeof(gb25_field_stats); }
int32_t gb25_field_diff_bytes(void) { return (int32_t)sizeof(gb25_field_diff); }
int32_t gb25_state_monitor_bytes(void) { return (int32_t)sizeof(gb25_state_monitor); }

gb25_status gb25_get_field_stats(gb25_model* m, gb25_field f, int include_halos, gb25_field_stats* out) {
  if (!m || !out) return GB25_ERR_INVALID_ARGUMENT;
  const real* src = nullptr;
  DiagBox b;
  if (gb25_status s = diag_source(m, f, &src)) return s;
  if (gb25_status s = diag_scratch(m)) return s;
  if (gb25_status s = diag_box(m, f, include_halos, &b)) return s;
  if (gb25_status s = diag_check_box(m, b)) return s;
  if (gb25_status s = wait_for_model(m)) return s;
  return diag_stats_of(m, f, src, b, include_halos, out);
}

gb25_status gb25_compare_field(gb25_model* m, gb25_field f, int include_halos, const void* other_dev, int32_t other_real_bytes,
                               const int32_t other_dims[3], const int32_t other_origin[3], gb25_field_diff* out) {
  if (!m || !out || !other_dev || !other_dims) return GB25_ERR_INVALID_ARGUMENT;
  if (other_real_bytes != 4 && other_real_bytes != 8)
    return fail(m, GB25_ERR_INVALID_ARGUMENT, "other_real_bytes must be 4 (float) or 8 (double), got %d", other_real_bytes);
  const real* src = nullptr;
  DiagBox b, ob;
  if (gb25_status s = diag_source(m, f, &src)) return s;
  if (gb25_status s = diag_scratch(m)) return s;
  if (gb25_status s = diag_box(m, f, include_halos, &b)) return s;
  if (gb25_status s = diag_check_box(m, b)) return s;
  const int32_t zero[3] = {0, 0, 0};
  const int32_t* o = other_origin ? other_origin : zero;
  const int ext[3] = {b.bx, b.by, b.bz};
  for (int q = 0; q < 3; q++)
    if (other_dims[q] <= 0 || o[q] < 0 || (long long)o[q] + ext[q] > other_dims[q])
      return fail(m, GB25_ERR_INVALID_ARGUMENT, "the other array (%d x %d x %d from %d %d %d) does not hold the %d x %d x %d box of this field",
                  other_dims[0], other_dims[1], other_dims[2], o[0], o[1], o[2], b.bx, b.by, b.bz);
  ob = b;
  ob.pitch = other_dims[0];
  ob.plane = (long long)other_dims[0] * other_dims[1];
  ob.origin = o[0] + ob.pitch * o[1] + ob.plane * o[2];
  if (gb25_status s = wait_for_model(m)) return s;
  const long long nb = diag_blocks(b);
  {
    Timed t(m, GB25_K_DIAGNOSTICS);
    DiffPartial* part = (DiffPartial*)m->diag.scratch;
    if (other_real_bytes == 4)
      hipLaunchKernelGGL((k_field_diff<real, float>), dim3((unsigned)nb), dim3(DIAG_THREADS), 0, m->stream, src, b, (const float*)other_dev, ob, part);
    else
      hipLaunchKernelGGL((k_field_diff<real, double>), dim3((unsigned)nb), dim3(DIAG_THREADS), 0, m->stream, src, b, (const double*)other_dev, ob, part);
    LAUNCHCHK();
    if (gb25_status s = diag_finish<DiffPartial>(m, nb, 0)) return s;
  }
  DiffPartial p;
  if (gb25_status s = diag_download(m, &p, diag_result_slot(m, 0), sizeof p)) return s;
  memset(out, 0, sizeof *out);
  out->max_abs_a = p.amax_a < 0 ? 0.0 : p.amax_a;
  out->max_abs_b = p.amax_b < 0 ? 0.0 : p.amax_b;
  out->max_abs_delta = p.amax_d < 0 ? 0.0 : p.amax_d;
  out->sum_sq_a = p.ss_a; out->sum_sq_b = p.ss_b; out->sum_sq_delta = p.ss_d;
  out->count = (int64_t)b.bx * b.by * b.bz;
  out->nonfinite = p.nonfinite;
  diag_position(p.amax_d < 0 ? DIAG_NONE : p.at, b, out->at_max_abs_delta);
  diag_global_offset(m, f, include_halos, out->global_offset);
  return GB25_OK;
}

gb25_status gb25_get_state_monitor(gb25_model* m, gb25_state_monitor* out) {
  if (!m || !out) return GB25_ERR_INVALID_ARGUMENT;
  static const gb25_field ids[6] = {GB25_U, GB25_V, GB25_W, GB25_ETA, GB25_T, GB25_S};
  const real* src[6];
  DiagBox b[6];
  for (int q = 0; q < 6; q++) {
    if (gb25_status s = diag_source(m, ids[q], &src[q])) return s;
    if (gb25_status s = diag_box(m, ids[q], 0, &b[q])) return s;
  }
  if (gb25_status s = diag_scratch(m)) return s;
  for (int q = 0; q < 6; q++)
    if (gb25_status s = diag_check_box(m, b[q])) return s;
  if (gb25_status s = wait_for_model(m)) return s;
  {
    Timed t(m, GB25_K_DIAGNOSTICS);
    for (int q = 0; q < 6; q++)
      if (gb25_status s = diag_launch_stats(m, src[q], b[q], q)) return s;
    const long long nb = diag_blocks(b[0]);   // (the interior of u: Nx x Ny x Nz, the cells)
    hipLaunchKernelGGL(k_advective_cfl, dim3((unsigned)nb), dim3(DIAG_THREADS), 0, m->stream, m->g, src[0], src[1], src[2], b[0],
                       (CflPartial*)m->diag.scratch);
    LAUNCHCHK();
    if (gb25_status s = diag_finish<CflPartial>(m, nb, 6)) return s;
  }
  char host[7 * DIAG_RECORD];
  if (gb25_status s = diag_download(m, host, diag_result_slot(m, 0), sizeof host)) return s;
  memset(out, 0, sizeof *out);
  gb25_field_stats* dst[6] = {&out->u, &out->v, &out->w, &out->eta, &out->T, &out->S};
  for (int q = 0; q < 6; q++) {
    StatsPartial p;
    memcpy(&p, host + q * DIAG_RECORD, sizeof p);
    diag_fill_stats(m, ids[q], p, b[q], 0, dst[q]);
    out->nonfinite_total += p.nonfinite;
  }
  CflPartial c;
  memcpy(&c, host + 6 * DIAG_RECORD, sizeof c);
  out->cfl = c.cfl < 0 ? 0.0 : c.cfl;
  diag_position(c.cfl < 0 ? DIAG_NONE : c.at, b[0], out->at_cfl);
  out->iteration = m->iteration;
  out->time = m->time;
  return GB25_OK;
}

int32_t gb25_moments_bytes(void) { return (int32_t)sizeof(gb25_moments); }
int32_t gb25_budget_bytes(void) { return (int32_t)sizeof(gb25_budget); }

gb25_status gb25_integrate_field(gb25_model* m, gb25_field f, gb25_sum_shape shape, gb25_moments* out, int64_t count) {
  if (!m || !out) return GB25_ERR_INVALID_ARGUMENT;
  if (shape != GB25_SUM_ROWS && shape != GB25_SUM_LEVELS && shape != GB25_SUM_TOTAL)
    return fail(m, GB25_ERR_INVALID_ARGUMENT, "gb25_integrate_field: shape must be GB25_SUM_ROWS, GB25_SUM_LEVELS or GB25_SUM_TOTAL, got %d", (int)shape);
  const real* src = nullptr;
  DiagBox b;
  if (gb25_status s = diag_source(m, f, &src)) return s;
  if (gb25_status s = diag_box(m, f, 0, &b)) return s;
  const int64_t want = shape == GB25_SUM_ROWS ? (int64_t)b.by * b.bz : shape == GB25_SUM_LEVELS ? (int64_t)b.bz : 1;
  if (count != want)
    return fail(m, GB25_ERR_INVALID_ARGUMENT, "gb25_integrate_field: this shape of this field has %lld records (rows %d, levels %d), count is %lld",
                (long long)want, b.by, b.bz, (long long)count);
  if (gb25_status s = moments_buffer(m)) return s;
  if (gb25_status s = moments_check_box(m, b)) return s;
  if (gb25_status s = wait_for_model(m)) return s;
  if (gb25_status s = moments_tables(m)) return s;
  {
    Timed t(m, GB25_K_DIAGNOSTICS);
    if (gb25_status s = moments_launch(m, f, src, b, 0)) return s;
    if (shape != GB25_SUM_ROWS)
      if (gb25_status s = moments_fold(m, &b, 1)) return s;
  }
  const MomentsPartial* from = shape == GB25_SUM_ROWS ? moments_rows(m, 0) : shape == GB25_SUM_LEVELS ? moments_levels(m, 0) : moments_totals(m);
  return diag_download(m, out, from, (size_t)count * sizeof(gb25_moments));
}

gb25_status gb25_get_budget(gb25_model* m, gb25_budget* out) {
  if (!m || !out) return GB25_ERR_INVALID_ARGUMENT;
  static const gb25_field ids[MOMENTS_SLOTS] = {GB25_T, GB25_S, GB25_U, GB25_V, GB25_ETA};
  const real* src[MOMENTS_SLOTS];
  DiagBox b[MOMENTS_SLOTS];
  for (int q = 0; q < MOMENTS_SLOTS; q++) {
    if (gb25_status s = diag_source(m, ids[q], &src[q])) return s;
    if (gb25_status s = diag_box(m, ids[q], 0, &b[q])) return s;
  }
  if (gb25_status s = moments_buffer(m)) return s;
  for (int q = 0; q < MOMENTS_SLOTS; q++)
    if (gb25_status s = moments_check_box(m, b[q])) return s;
  if (gb25_status s = wait_for_model(m)) return s;
  if (gb25_status s = moments_tables(m)) return s;
  {
    Timed t(m, GB25_K_DIAGNOSTICS);
    for (int q = 0; q < MOMENTS_SLOTS; q++)
      if (gb25_status s = moments_launch(m, ids[q], src[q], b[q], q)) return s;
    if (gb25_status s = moments_fold(m, b, MOMENTS_SLOTS)) return s;
  }
  gb25_moments tot[MOMENTS_SLOTS];
  if (gb25_status s = diag_download(m, tot, moments_totals(m), sizeof tot)) return s;
  memset(out, 0, sizeof *out);
  out->T = tot[0]; out->S = tot[1]; out->u = tot[2]; out->v = tot[3]; out->eta = tot[4];
  out->volume = out->T.measure;
  out->surface_area = out->eta.measure;
  out->kinetic_energy = 0.5 * (out->u.second + out->v.second);
  out->eta_potential_energy = 0.5 * m->cfg.g * out->eta.second;
  out->iteration = m->iteration;
  out->time = m->time;
  diag_global_offset(m, GB25_T, 0, out->global_offset);
  return GB25_OK;
}

gb25_status gb25_field_device_ptr_readonly(gb25_model* m, gb25_field f, const void** dev, int32_t device_dims[3]) {
  if (!m || !dev) return GB25_ERR_INVALID_ARGUMENT;
  const real* src = nullptr;
  if (gb25_status s = diag_source(m, f, &src)) return s;
  if (gb25_status s = wait_for_model(m)) return s;
  *dev = src;
  if (device_dims) {
    device_dims[0] = m->f[f].nx; device_dims[1] = m->f[f].ny; device_dims[2] = m->f[f].nz;
  }
  return GB25_OK;
}

}  // extern "C"
