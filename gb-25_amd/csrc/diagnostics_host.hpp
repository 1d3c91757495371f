// diagnostics_host.hpp -- host side of gb25_get_field_stats / gb25_compare_field / gb25_get_state_monitor /
// gb25_field_device_ptr_readonly / gb25_integrate_field / gb25_get_budget / gb25_compute_derived / gb25_get_derived /
// gb25_get_derived_stats / gb25_get_field_levels / gb25_get_transport (include/gb25.h); the last part of gb25_api.hip, which includes it.  Kernels:
// diagnostics_kernels.hpp.  Nothing here writes model memory or a schedule flag: the calls may sit between any two steps.
#pragma once

namespace {

constexpr size_t DIAG_RECORD = 64;   // bytes of a slot of the scratch buffer: the largest per-block record
constexpr int DIAG_RESULTS = 8;      // result slots behind the per-block records (a state monitor fills seven)
static_assert(sizeof(StatsPartial) <= DIAG_RECORD && sizeof(DiffPartial) <= DIAG_RECORD && sizeof(CflPartial) <= DIAG_RECORD, "slot size");

inline long long diag_blocks(const DiagBox& b) { return ((long long)b.by * b.bz + DIAG_ROWS - 1) / DIAG_ROWS; }

// once per model: per-block records for the tallest box a field of this model has (w's parent), plus the result slots
gb25_status diag_scratch(gb25_model* m) {
  if (m->diag_scratch) return GB25_OK;
  const int H = m->cfg.halo;
  const long long rows = (long long)(m->Ny + 2 * H + 1) * (m->cfg.Nz + 2 * H + 1);
  const size_t records = (size_t)((rows + DIAG_ROWS - 1) / DIAG_ROWS);
  HIPCHK(hipMalloc(&m->diag_scratch, (records + DIAG_RESULTS) * DIAG_RECORD));
  m->diag_scratch_records = records;
  return GB25_OK;
}
inline void* diag_result_slot(gb25_model* m, int q) { return (char*)m->diag_scratch + (m->diag_scratch_records + q) * DIAG_RECORD; }

// the whole model is quiet (what gb25_synchronize waits for)
gb25_status diag_wait_for_model(gb25_model* m) {
  HIPCHK(hipStreamSynchronize(m->stream));
  HIPCHK(hipStreamSynchronize(m->side_stream));
  if (m->baro_stream) HIPCHK(hipStreamSynchronize(m->baro_stream));
  if (m->group) HIPCHK(m->group->sync_side());
  return GB25_OK;
}

// The array that holds what gb25_get_field(id) would return, without moving anything: previous_velocities are read where they
// live (prev_uv_src), a stale pHY' is recomputed from the T, S it belongs to (the launch is filed under GB25_K_DIAGNOSTICS).
gb25_status diag_source(gb25_model* m, gb25_field id, const real** src) {
  if (id < 0 || id >= GB25_FIELD_COUNT) return GB25_ERR_INVALID_ARGUMENT;
  if (!m->f[id].d) return fail(m, GB25_ERR_INVALID_ARGUMENT, "this model has no such field (closure = CATKEVerticalDiffusivity() only)");
  if (m->uv_lazy)   // (only after a composite call that failed half-way)
    if (gb25_status s = materialize_uv(m)) return s;
  if (id == GB25_PHY && m->phy_stale) {
    m->prof_redirect = GB25_K_DIAGNOSTICS;
    const gb25_status s = compute_p_impl(m);
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
  hipLaunchKernelGGL(k_diag_finish<P>, dim3(1), dim3(DIAG_THREADS), 0, m->stream, (const P*)m->diag_scratch, (int)nblocks,
                     (P*)diag_result_slot(m, slot));
  LAUNCHCHK();
  return GB25_OK;
}
gb25_status diag_launch_stats(gb25_model* m, const real* src, const DiagBox& b, int slot) {
  const long long nb = diag_blocks(b);
  hipLaunchKernelGGL(k_field_stats<real>, dim3((unsigned)nb), dim3(DIAG_THREADS), 0, m->stream, src, b, (StatsPartial*)m->diag_scratch);
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
  if ((size_t)diag_blocks(b) > m->diag_scratch_records) return fail(m, GB25_ERR_STATE, "diagnostics: the box needs more per-block records than the model's scratch buffer holds");
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
  if (m->diag_tables_valid) return GB25_OK;
  const int Nx = m->Nx, Ny = m->Ny, Nz = m->cfg.Nz, H = m->cfg.halo, sx = Nx + 2 * H, sy = Ny + 2 * H + 1;
  const size_t n2 = (size_t)sx * sy;
  for (int q = 0; q < 3; q++) {
    if (m->diag_area[q]) HIPCHK(hipFree(m->diag_area[q]));
    if (m->diag_first_wet[q]) HIPCHK(hipFree(m->diag_first_wet[q]));
    m->diag_area[q] = nullptr;
    m->diag_first_wet[q] = nullptr;
  }
  if (m->diag_azff) HIPCHK(hipFree(m->diag_azff));
  if (m->diag_zt) HIPCHK(hipFree(m->diag_zt));
  m->diag_azff = nullptr;
  m->diag_zt = nullptr;
  for (int q = 0; q < 2; q++) {
    if (m->diag_face_length[q]) HIPCHK(hipFree(m->diag_face_length[q]));
    m->diag_face_length[q] = nullptr;
  }
  {
    // the derived fields' own: (double) of zc[0 .. Nz) | zf[0 .. Nz] as gb25_get_metric returns them, AZFF of a curvilinear grid
    std::vector<double> zt((size_t)2 * Nz + 1);
    for (int k = 0; k < Nz; k++) zt[k] = (double)(real)m->h_metric[GB25_M_ZC][m->metric_off_k + k];
    for (int k = 0; k <= Nz; k++) zt[Nz + k] = (double)(real)m->h_metric[GB25_M_ZF][m->metric_off_k + k];
    HIPCHK(hipMalloc(&m->diag_zt, zt.size() * sizeof(double)));
    HIPCHK(hipMemcpy(m->diag_zt, zt.data(), zt.size() * sizeof(double), hipMemcpyHostToDevice));
    if (m->g.cv.on) {
      const std::vector<double>& h = m->h_curv[GB25_M2_AZFF];
      if (h.size() != n2) return fail(m, GB25_ERR_STATE, "derived fields: the curvilinear metrics are not built");
      std::vector<real> a(n2);
      for (size_t o = 0; o < n2; o++) a[o] = (real)h[o];
      HIPCHK(hipMalloc(&m->diag_azff, n2 * sizeof(real)));
      HIPCHK(hipMemcpy(m->diag_azff, a.data(), n2 * sizeof(real), hipMemcpyHostToDevice));
    }
  }
  if (m->g.cv.on) {
    static const int ids[3] = {GB25_M2_AZCC, GB25_M2_AZFC, GB25_M2_AZCF};
    std::vector<real> a(n2);
    for (int q = 0; q < 3; q++) {
      const std::vector<double>& h = m->h_curv[ids[q]];
      if (h.size() != n2) return fail(m, GB25_ERR_STATE, "integrals: the curvilinear metrics are not built");
      for (size_t o = 0; o < n2; o++) a[o] = (real)h[o];
      HIPCHK(hipMalloc(&m->diag_area[q], n2 * sizeof(real)));
      HIPCHK(hipMemcpy(m->diag_area[q], a.data(), n2 * sizeof(real), hipMemcpyHostToDevice));
    }
  }
  if (m->g.cv.on) {
    // the transports' own: the lengths of the y faces (DXCF) and of the x faces (DYFC)
    static const int ids[2] = {GB25_M2_DXCF, GB25_M2_DYFC};
    std::vector<real> a(n2);
    for (int q = 0; q < 2; q++) {
      const std::vector<double>& h = m->h_curv[ids[q]];
      if (h.size() != n2) return fail(m, GB25_ERR_STATE, "transports: the curvilinear metrics are not built");
      for (size_t o = 0; o < n2; o++) a[o] = (real)h[o];
      HIPCHK(hipMalloc(&m->diag_face_length[q], n2 * sizeof(real)));
      HIPCHK(hipMemcpy(m->diag_face_length[q], a.data(), n2 * sizeof(real), hipMemcpyHostToDevice));
    }
  }
  if (!m->kbot.empty()) {
    const int E = m->kb_E, ksx = Nx + 2 * E;
    auto kb = [&](int ii, int jj) {   // (gb25_get_bottom_info's: clamped at the walls, a neighbour's row otherwise)
      const int jl = std::min(std::max(jj + m->j0, 0), m->cfg.Ny - 1) - m->j0;
      return m->kbot[(size_t)(ii + E) + (size_t)ksx * (std::min(std::max(jl, -m->kb_Ey), Ny + m->kb_Ey - 1) + m->kb_Ey)];
    };
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
      HIPCHK(hipMalloc(&m->diag_first_wet[q], n2 * sizeof(unsigned short)));
      HIPCHK(hipMemcpy(m->diag_first_wet[q], f.data(), n2 * sizeof(unsigned short), hipMemcpyHostToDevice));
    }
  }
  m->diag_tables_valid = true;
  return GB25_OK;
}

// once per model: MOMENTS_SLOTS sets of row records for the tallest interior a field of this model has, their level records,
// their totals
gb25_status moments_buffer(gb25_model* m) {
  if (m->diag_moments) return GB25_OK;
  const size_t levels = (size_t)m->cfg.Nz + 1, rows = (size_t)(m->Ny + 1) * levels;
  HIPCHK(hipMalloc(&m->diag_moments, (size_t)MOMENTS_SLOTS * (rows + levels + 1) * sizeof(MomentsPartial)));
  m->diag_moments_rows = rows;
  m->diag_moments_levels = levels;
  return GB25_OK;
}
inline MomentsPartial* moments_rows(gb25_model* m, int slot) { return (MomentsPartial*)m->diag_moments + m->diag_moments_rows * slot; }
inline MomentsPartial* moments_levels(gb25_model* m, int slot) {
  return (MomentsPartial*)m->diag_moments + m->diag_moments_rows * MOMENTS_SLOTS + m->diag_moments_levels * slot;
}
inline MomentsPartial* moments_totals(gb25_model* m) {
  return (MomentsPartial*)m->diag_moments + (m->diag_moments_rows + m->diag_moments_levels) * MOMENTS_SLOTS;
}
gb25_status moments_check_box(gb25_model* m, const DiagBox& b) {
  if (b.bx <= 0 || b.by <= 0 || b.bz <= 0) return fail(m, GB25_ERR_INVALID_ARGUMENT, "the field has an empty box");
  if ((size_t)b.by * b.bz > m->diag_moments_rows || (size_t)b.bz > m->diag_moments_levels)
    return fail(m, GB25_ERR_STATE, "integrals: the box needs more row records than the model's buffer holds");
  return GB25_OK;
}

template <int LOC>
void moments_launch_loc(gb25_model* m, const MomentsTables& tab, const real* src, const DiagBox& b, MomentsPartial* rows) {
  const long long nb = ((long long)b.by * b.bz + DIAG_THREADS / 64 - 1) / (DIAG_THREADS / 64);
  hipLaunchKernelGGL((k_field_moments<real, LOC>), dim3((unsigned)nb), dim3(DIAG_THREADS), 0, m->stream, m->g, tab, src, b, rows);
}
// the row records of field id into slot `slot`
gb25_status moments_launch(gb25_model* m, gb25_field id, const real* src, const DiagBox& b, int slot) {
  MomentsTables tab;
  for (int q = 0; q < 3; q++) {
    tab.area[q] = m->diag_area[q];
    tab.first[q] = m->diag_first_wet[q];
  }
  tab.pivot_row = (m->cfg.grid_type >= GB25_GRID_TRIPOLAR && !m->yn_open) ? m->Ny - 1 : -1;
  MomentsPartial* rows = moments_rows(m, slot);
  switch (moments_loc(id)) {
    case LOC_CCC: moments_launch_loc<LOC_CCC>(m, tab, src, b, rows); break;
    case LOC_FCC: moments_launch_loc<LOC_FCC>(m, tab, src, b, rows); break;
    case LOC_CFC: moments_launch_loc<LOC_CFC>(m, tab, src, b, rows); break;
    case LOC_CCF: moments_launch_loc<LOC_CCF>(m, tab, src, b, rows); break;
    case LOC_CC: moments_launch_loc<LOC_CC>(m, tab, src, b, rows); break;
    case LOC_FC: moments_launch_loc<LOC_FC>(m, tab, src, b, rows); break;
    case LOC_CF: moments_launch_loc<LOC_CF>(m, tab, src, b, rows); break;
  }
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
                     (long long)m->diag_moments_rows, f, moments_levels(m, 0), (long long)m->diag_moments_levels);
  LAUNCHCHK();
  hipLaunchKernelGGL(k_moments_fold, dim3(1, n), dim3(64), 0, m->stream, (const MomentsPartial*)moments_levels(m, 0),
                     (long long)m->diag_moments_levels, t, moments_totals(m), 1LL);
  LAUNCHCHK();
  return GB25_OK;
}


// ---- derived fields
// interior extents of a derived field, from the configuration alone (no device): zeta has the rows of v -- one more than the
// cells below a wall, as many on a folded grid and below a northern neighbour rank
void derived_extents(const gb25_model* m, gb25_derived q, int32_t d[3]) {
  const bool no_wall = m->cfg.grid_type >= GB25_GRID_TRIPOLAR || m->yn_open;
  d[0] = m->Nx;
  d[1] = m->Ny + ((q == GB25_D_VORTICITY && !no_wall) ? 1 : 0);
  d[2] = q == GB25_D_MIXED_LAYER_DEPTH ? 1 : m->cfg.Nz;
}
// interior levels [k_first, k_first + k_count) of nz; k_count = -1: all from k_first on
gb25_status derived_levels(gb25_model* m, const char* what, int nz, int32_t k_first, int32_t k_count, int* kc) {
  const long long n = k_count == -1 ? (long long)nz - k_first : (long long)k_count;
  if (k_first < 0 || k_first >= nz || k_count < -1 || k_count == 0 || k_first + n > nz)
    return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: levels k_first = %d, k_count = %d of a result with %d level%s (0-based interior levels; k_count = -1: all)",
                what, (int)k_first, (int)k_count, nz, nz == 1 ? "" : "s");
  *kc = (int)n;
  return GB25_OK;
}
gb25_status derived_check(gb25_model* m, const char* what, gb25_derived q, double param) {
  if (q < 0 || q >= GB25_D_COUNT) return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: no derived field %d (0 .. %d)", what, (int)q, GB25_D_COUNT - 1);
  if (q == GB25_D_MIXED_LAYER_DEPTH && !(param > 0.0))
    return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: the mixed-layer depth needs a density threshold > 0 kg/m^3 as param, got %g", what, param);
  return GB25_OK;
}
gb25_status derived_need_device(gb25_model* m, const char* what) {
  if (!m->own_stream) return fail(m, GB25_ERR_NO_DEVICE, "%s: this model has no device (gb25_create failed); libgb25hip has no CPU fallback", what);
  return GB25_OK;
}
// once per model: one 2-D plane, then room for the largest interior a field has (w: Nz + 1 levels; v: Ny + 1 rows)
gb25_status derived_scratch(gb25_model* m) {
  if (m->diag_derived) return GB25_OK;
  const size_t plane = (size_t)m->Nx * (m->Ny + 1);
  m->diag_derived_plane = (plane + 3) & ~(size_t)3;   // (the 3-D part starts on a 16-byte boundary)
  m->diag_derived_elems = m->diag_derived_plane + plane * ((size_t)m->cfg.Nz + 1);
  HIPCHK(hipMalloc(&m->diag_derived, m->diag_derived_elems * sizeof(real)));
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
  if (gb25_status s = diag_wait_for_model(m)) return s;
  if (gb25_status s = moments_tables(m)) return s;
  int32_t e[3];
  derived_extents(m, q, e);
  const Grid& g = m->g;
  const dim3 blk(64, 4);
  Timed t(m, GB25_K_DIAGNOSTICS);
  if (q == GB25_D_MIXED_LAYER_DEPTH) {
    // sigma of every level into the 3-D part (the very values gb25_get_derived(GB25_D_POTENTIAL_DENSITY) hands out), then the march
    real* sigma = m->diag_derived + m->diag_derived_plane;
    const DerivedOut d{sigma, e[0], e[1], 0, g.Nz};
    hipLaunchKernelGGL(k_derived_density<true>, derived_grid(e[0], e[1], g.Nz), blk, 0, m->stream, g, a, b, m->diag_eos0, m->diag_first_wet[0], d);
    LAUNCHCHK();
    hipLaunchKernelGGL(k_derived_mixed_layer, dim3((e[0] + 63) / 64, (e[1] + 3) / 4), blk, 0, m->stream, g, (const real*)sigma,
                       m->diag_first_wet[0], (const double*)m->diag_zt, param, m->diag_derived, e[0], e[1]);
    LAUNCHCHK();
    *result = m->diag_derived;
    return GB25_OK;
  }
  real* out = m->diag_derived + m->diag_derived_plane;
  const DerivedOut d{out, e[0], e[1], k0, kc};
  const dim3 grd = derived_grid(e[0], e[1], kc);
  switch (q) {
    case GB25_D_VORTICITY:
      if (g.cv.on) hipLaunchKernelGGL(k_derived_vorticity<true>, grd, blk, 0, m->stream, g, a, b, (const real*)m->diag_azff, d);
      else hipLaunchKernelGGL(k_derived_vorticity<false>, grd, blk, 0, m->stream, g, a, b, (const real*)nullptr, d);
      break;
    case GB25_D_KINETIC_ENERGY: hipLaunchKernelGGL(k_derived_kinetic_energy, grd, blk, 0, m->stream, g, a, b, d); break;
    case GB25_D_DENSITY_ANOMALY:
      hipLaunchKernelGGL(k_derived_density<false>, grd, blk, 0, m->stream, g, a, b, m->diag_eos0, m->diag_first_wet[0], d);
      break;
    default:
      hipLaunchKernelGGL(k_derived_density<true>, grd, blk, 0, m->stream, g, a, b, m->diag_eos0, m->diag_first_wet[0], d);
      break;
  }
  LAUNCHCHK();
  *result = out;
  return GB25_OK;
}

// ---- transports
static_assert(sizeof(TransportPartial) == sizeof(gb25_transport), "a line record is a gb25_transport");

// once per model: LINES [N Nz], the running sums [N (Nz + 1)] and PROFILE [N] for the longest set of lines a call can ask for
// (N = by of v for the y faces, Nx for the x faces); the three parts start at multiples of that longest N
gb25_status transport_buffer(gb25_model* m) {
  if (m->diag_transport) return GB25_OK;
  const size_t lines = (size_t)std::max(m->Nx, m->Ny + 1);
  HIPCHK(hipMalloc(&m->diag_transport, lines * (2 * (size_t)m->cfg.Nz + 2) * sizeof(TransportPartial)));
  m->diag_transport_lines = lines;
  return GB25_OK;
}
inline TransportPartial* transport_lines(gb25_model* m) { return (TransportPartial*)m->diag_transport; }
inline TransportPartial* transport_psi(gb25_model* m) { return transport_lines(m) + m->diag_transport_lines * m->cfg.Nz; }
inline TransportPartial* transport_profile(gb25_model* m) { return transport_psi(m) + m->diag_transport_lines * (m->cfg.Nz + 1); }

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
  const long long n = along_count == -1 ? (long long)along - along_first : (long long)along_count;
  if (along_first < 0 || along_first >= along || along_count < -1 || along_count == 0 || along_first + n > along)
    return fail(m, GB25_ERR_INVALID_ARGUMENT, "gb25_get_transport: window along_first = %d, along_count = %d of %d %s (0-based local interior indices; along_count = -1: to the end)",
                (int)along_first, (int)along_count, along, ay ? "columns" : "rows");
  const int64_t want = shape == GB25_TR_LINES ? (int64_t)N * Nz : shape == GB25_TR_PROFILE ? (int64_t)N : (int64_t)N * (Nz + 1);
  if (count != want)
    return fail(m, GB25_ERR_INVALID_ARGUMENT, "gb25_get_transport: this shape has %lld records (lines %d, levels %d), count is %lld",
                (long long)want, N, Nz, (long long)count);
  if (gb25_status s = derived_need_device(m, "gb25_get_transport")) return s;
  const real *vel = nullptr, *T = nullptr, *S = nullptr;
  if (gb25_status s = diag_source(m, ay ? GB25_V : GB25_U, &vel)) return s;
  if (gb25_status s = diag_source(m, GB25_T, &T)) return s;
  if (gb25_status s = diag_source(m, GB25_S, &S)) return s;
  if (gb25_status s = transport_buffer(m)) return s;
  if ((size_t)N > m->diag_transport_lines) return fail(m, GB25_ERR_STATE, "gb25_get_transport: more lines than the model's buffer holds");
  if (gb25_status s = diag_wait_for_model(m)) return s;
  if (gb25_status s = moments_tables(m)) return s;
  const Grid& g = m->g;
  TransportTables tab;
  tab.length = m->diag_face_length[ay ? 0 : 1];
  tab.first = m->diag_first_wet[ay ? 2 : 1];
  tab.pivot_row = (!ay && m->cfg.grid_type >= GB25_GRID_TRIPOLAR && !m->yn_open) ? m->Ny - 1 : -1;
  TransportPartial* lines = transport_lines(m);
  {
    Timed t(m, GB25_K_DIAGNOSTICS);
    if (ay) {
      const long long nb = ((long long)N * Nz + DIAG_THREADS / 64 - 1) / (DIAG_THREADS / 64);
      if (g.cv.on) hipLaunchKernelGGL(k_transport_rows<true>, dim3((unsigned)nb), dim3(DIAG_THREADS), 0, m->stream, g, tab, vel, T, S, (int)along_first, (int)n, N, lines);
      else hipLaunchKernelGGL(k_transport_rows<false>, dim3((unsigned)nb), dim3(DIAG_THREADS), 0, m->stream, g, tab, vel, T, S, (int)along_first, (int)n, N, lines);
    } else {
      const dim3 grd((N + 63) / 64, (Nz + 3) / 4), blk(64, 4);
      if (g.cv.on) hipLaunchKernelGGL(k_transport_columns<true>, grd, blk, 0, m->stream, g, tab, vel, T, S, (int)along_first, (int)n, lines);
      else hipLaunchKernelGGL(k_transport_columns<false>, grd, blk, 0, m->stream, g, tab, vel, T, S, (int)along_first, (int)n, lines);
    }
    LAUNCHCHK();
    if (shape != GB25_TR_LINES) {
      hipLaunchKernelGGL(k_transport_fold, dim3((N + 63) / 64), dim3(64), 0, m->stream, (const TransportPartial*)lines, N, Nz,
                         transport_psi(m), transport_profile(m));
      LAUNCHCHK();
    }
  }
  const TransportPartial* from = shape == GB25_TR_LINES ? lines : shape == GB25_TR_PROFILE ? transport_profile(m) : transport_psi(m);
  HIPCHK(hipMemcpyAsync(out, from, (size_t)count * sizeof(gb25_transport), hipMemcpyDeviceToHost, m->stream));
  HIPCHK(hipStreamSynchronize(m->stream));
  return GB25_OK;
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
  if (gb25_status s = derived_check(m, "gb25_compute_derived", q, param)) return s;
  int32_t e[3];
  int kc = 0;
  derived_extents(m, q, e);
  if (gb25_status s = derived_levels(m, "gb25_compute_derived", e[2], k_first, k_count, &kc)) return s;
  if (gb25_status s = derived_need_device(m, "gb25_compute_derived")) return s;
  const real* out = nullptr;
  if (gb25_status s = derived_run(m, q, param, k_first, kc, &out)) return s;
  HIPCHK(hipStreamSynchronize(m->stream));
  *dev = out;
  if (device_dims) {
    device_dims[0] = e[0]; device_dims[1] = e[1]; device_dims[2] = kc;
  }
  return GB25_OK;
}

gb25_status gb25_get_derived(gb25_model* m, gb25_derived q, double param, int32_t k_first, int32_t k_count, void* host) {
  if (!m) return GB25_ERR_INVALID_ARGUMENT;
  if (!host) return fail(m, GB25_ERR_INVALID_ARGUMENT, "gb25_get_derived: host is NULL");
  if (gb25_status s = derived_check(m, "gb25_get_derived", q, param)) return s;
  int32_t e[3];
  int kc = 0;
  derived_extents(m, q, e);
  if (gb25_status s = derived_levels(m, "gb25_get_derived", e[2], k_first, k_count, &kc)) return s;
  if (gb25_status s = derived_need_device(m, "gb25_get_derived")) return s;
  const real* out = nullptr;
  if (gb25_status s = derived_run(m, q, param, k_first, kc, &out)) return s;
  HIPCHK(hipMemcpyAsync(host, out, (size_t)e[0] * e[1] * kc * sizeof(real), hipMemcpyDeviceToHost, m->stream));
  HIPCHK(hipStreamSynchronize(m->stream));
  return GB25_OK;
}

gb25_status gb25_get_derived_stats(gb25_model* m, gb25_derived q, double param, gb25_field_stats* out) {
  if (!m) return GB25_ERR_INVALID_ARGUMENT;
  if (!out) return fail(m, GB25_ERR_INVALID_ARGUMENT, "gb25_get_derived_stats: out is NULL");
  if (gb25_status s = derived_check(m, "gb25_get_derived_stats", q, param)) return s;
  if (gb25_status s = derived_need_device(m, "gb25_get_derived_stats")) return s;
  int32_t e[3];
  derived_extents(m, q, e);
  const DiagBox b{e[0], e[1], e[2], (long long)e[0], (long long)e[0] * e[1], 0};
  if (gb25_status s = diag_scratch(m)) return s;
  if (gb25_status s = diag_check_box(m, b)) return s;
  const real* src = nullptr;
  if (gb25_status s = derived_run(m, q, param, 0, e[2], &src)) return s;
  {
    Timed t(m, GB25_K_DIAGNOSTICS);
    if (gb25_status s = diag_launch_stats(m, src, b, 0)) return s;
  }
  StatsPartial p;
  HIPCHK(hipMemcpyAsync(&p, diag_result_slot(m, 0), sizeof p, hipMemcpyDeviceToHost, m->stream));
  HIPCHK(hipStreamSynchronize(m->stream));
  diag_fill_stats(m, GB25_T, p, b, 0, out);   // (interior: the offsets are those of any field of the rank, 0 in k)
  return GB25_OK;
}

gb25_status gb25_get_field_levels(gb25_model* m, gb25_field f, int32_t k_first, int32_t k_count, void* host) {
  if (!m) return GB25_ERR_INVALID_ARGUMENT;
  if (f < 0 || f >= GB25_FIELD_COUNT) return fail(m, GB25_ERR_INVALID_ARGUMENT, "gb25_get_field_levels: no field %d", (int)f);
  if (!host) return fail(m, GB25_ERR_INVALID_ARGUMENT, "gb25_get_field_levels: host is NULL");
  if (k_first < 0 || k_count < -1 || k_count == 0)
    return fail(m, GB25_ERR_INVALID_ARGUMENT, "gb25_get_field_levels: levels k_first = %d, k_count = %d (0-based interior levels; k_count = -1: all)",
                (int)k_first, (int)k_count);
  if (gb25_status s = derived_need_device(m, "gb25_get_field_levels")) return s;
  const real* src = nullptr;
  DiagBox b;
  int kc = 0;
  if (gb25_status s = diag_source(m, f, &src)) return s;
  if (gb25_status s = diag_box(m, f, 0, &b)) return s;
  if (gb25_status s = derived_levels(m, "gb25_get_field_levels", b.bz, k_first, k_count, &kc)) return s;
  if (gb25_status s = derived_scratch(m)) return s;
  const size_t n = (size_t)b.bx * b.by * kc;
  if (n > m->diag_derived_elems - m->diag_derived_plane) return fail(m, GB25_ERR_STATE, "gb25_get_field_levels: the levels need more room than the model's result array has");
  if (gb25_status s = diag_wait_for_model(m)) return s;
  b.origin += b.plane * k_first;
  b.bz = kc;
  real* out = m->diag_derived + m->diag_derived_plane;
  {
    Timed t(m, GB25_K_DIAGNOSTICS);
    constexpr int VW = 16 / sizeof(real);
    const int chunks = (b.bx + VW - 1) / VW + 1;
    hipLaunchKernelGGL(k_gather_levels<real>, dim3((chunks + 63) / 64, (b.by + 3) / 4, kc), dim3(64, 4), 0, m->stream, src, b, out);
    LAUNCHCHK();
  }
  HIPCHK(hipMemcpyAsync(host, out, n * sizeof(real), hipMemcpyDeviceToHost, m->stream));
  HIPCHK(hipStreamSynchronize(m->stream));
  return GB25_OK;
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
  if (gb25_status s = diag_wait_for_model(m)) return s;
  {
    Timed t(m, GB25_K_DIAGNOSTICS);
    if (gb25_status s = diag_launch_stats(m, src, b, 0)) return s;
  }
  StatsPartial p;
  HIPCHK(hipMemcpyAsync(&p, diag_result_slot(m, 0), sizeof p, hipMemcpyDeviceToHost, m->stream));
  HIPCHK(hipStreamSynchronize(m->stream));
  diag_fill_stats(m, f, p, b, include_halos, out);
  return GB25_OK;
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
  if (gb25_status s = diag_wait_for_model(m)) return s;
  const long long nb = diag_blocks(b);
  {
    Timed t(m, GB25_K_DIAGNOSTICS);
    DiffPartial* part = (DiffPartial*)m->diag_scratch;
    if (other_real_bytes == 4)
      hipLaunchKernelGGL((k_field_diff<real, float>), dim3((unsigned)nb), dim3(DIAG_THREADS), 0, m->stream, src, b, (const float*)other_dev, ob, part);
    else
      hipLaunchKernelGGL((k_field_diff<real, double>), dim3((unsigned)nb), dim3(DIAG_THREADS), 0, m->stream, src, b, (const double*)other_dev, ob, part);
    LAUNCHCHK();
    if (gb25_status s = diag_finish<DiffPartial>(m, nb, 0)) return s;
  }
  DiffPartial p;
  HIPCHK(hipMemcpyAsync(&p, diag_result_slot(m, 0), sizeof p, hipMemcpyDeviceToHost, m->stream));
  HIPCHK(hipStreamSynchronize(m->stream));
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
  if (gb25_status s = diag_wait_for_model(m)) return s;
  {
    Timed t(m, GB25_K_DIAGNOSTICS);
    for (int q = 0; q < 6; q++)
      if (gb25_status s = diag_launch_stats(m, src[q], b[q], q)) return s;
    const long long nb = diag_blocks(b[0]);   // (the interior of u: Nx x Ny x Nz, the cells)
    hipLaunchKernelGGL(k_advective_cfl, dim3((unsigned)nb), dim3(DIAG_THREADS), 0, m->stream, m->g, src[0], src[1], src[2], b[0],
                       (CflPartial*)m->diag_scratch);
    LAUNCHCHK();
    if (gb25_status s = diag_finish<CflPartial>(m, nb, 6)) return s;
  }
  char host[7 * DIAG_RECORD];
  HIPCHK(hipMemcpyAsync(host, diag_result_slot(m, 0), sizeof host, hipMemcpyDeviceToHost, m->stream));
  HIPCHK(hipStreamSynchronize(m->stream));
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
  if (gb25_status s = diag_wait_for_model(m)) return s;
  if (gb25_status s = moments_tables(m)) return s;
  {
    Timed t(m, GB25_K_DIAGNOSTICS);
    if (gb25_status s = moments_launch(m, f, src, b, 0)) return s;
    if (shape != GB25_SUM_ROWS)
      if (gb25_status s = moments_fold(m, &b, 1)) return s;
  }
  const MomentsPartial* from = shape == GB25_SUM_ROWS ? moments_rows(m, 0) : shape == GB25_SUM_LEVELS ? moments_levels(m, 0) : moments_totals(m);
  HIPCHK(hipMemcpyAsync(out, from, (size_t)count * sizeof(gb25_moments), hipMemcpyDeviceToHost, m->stream));
  HIPCHK(hipStreamSynchronize(m->stream));
  return GB25_OK;
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
  if (gb25_status s = diag_wait_for_model(m)) return s;
  if (gb25_status s = moments_tables(m)) return s;
  {
    Timed t(m, GB25_K_DIAGNOSTICS);
    for (int q = 0; q < MOMENTS_SLOTS; q++)
      if (gb25_status s = moments_launch(m, ids[q], src[q], b[q], q)) return s;
    if (gb25_status s = moments_fold(m, b, MOMENTS_SLOTS)) return s;
  }
  gb25_moments tot[MOMENTS_SLOTS];
  HIPCHK(hipMemcpyAsync(tot, moments_totals(m), sizeof tot, hipMemcpyDeviceToHost, m->stream));
  HIPCHK(hipStreamSynchronize(m->stream));
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
  if (gb25_status s = diag_wait_for_model(m)) return s;
  *dev = src;
  if (device_dims) {
    device_dims[0] = m->f[f].nx; device_dims[1] = m->f[f].ny; device_dims[2] = m->f[f].nz;
  }
  return GB25_OK;
}

}  // extern "C"
