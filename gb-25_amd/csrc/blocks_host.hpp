// blocks_host.hpp -- host side of gb25_block_dims / gb25_derived_block_dims / gb25_get_block_sums / gb25_compute_block_sums /
// gb25_get_derived_block_sums / gb25_block_info_bytes (include/gb25.h); included by gb25_api.hip behind diagnostics_host.hpp, whose
// shared helpers (diag_*), measure (moments_loc, moments_tables: the areas and first wet levels of gb25_integrate_field) and derived
// fields (derived_run) it uses.  Kernel: block_kernels.hpp; the memory: blocks, block_* of DiagState (diagnostics_state.hpp).
// Like the other diagnostics nothing here writes model memory or a schedule flag: the only memory written is the results' own
// buffer.
#pragma once

namespace {

static_assert(BLK_THREADS == GB25_BLOCK_MAX_BX, "the kernel's tile is the header's largest bx");
constexpr size_t BLOCK_HEAD = 32;   // bytes in front of the weights: BlockCounts, padded
static_assert(sizeof(BlockCounts) <= BLOCK_HEAD, "the counts fit their slot");

// What a call reduces: the fine extents (columns, rows of cell centres, the levels of the source), its location, the window
struct BlockPlan {
  int32_t fine[3];   // Nx, Ny, the source's own level count
  MomentLoc loc;
  int kc;            // the resolved k_count
  int32_t e[3];      // the result's dims
};

// the checks that need no device; P.fine and P.loc are given
gb25_status blocks_check(gb25_model* m, const char* what, const gb25_blocks* B, const double* level_weight, BlockPlan* P) {
  if (!B) return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: blocks is NULL", what);
  const int Nx = P->fine[0], Ny = P->fine[1], levels = P->fine[2];
  if (B->bx <= 0 || B->bx > GB25_BLOCK_MAX_BX || Nx % B->bx)
    return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: bx = %d must be 1 .. %d and divide the rank's Nx = %d", what, (int)B->bx, GB25_BLOCK_MAX_BX, Nx);
  if (B->by <= 0 || Ny % B->by)
    return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: by = %d must be > 0 and divide the rank's Ny = %d (rows of cell centres)", what, (int)B->by, Ny);
  if (gb25_status s = diag_window(m, what, B->k_first, B->k_count, levels, "levels (k_first, k_count)", &P->kc)) return s;
  if (B->bz <= 0 || P->kc % B->bz)
    return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: bz = %d must be > 0 and divide the %d levels of the window", what, (int)B->bz, P->kc);
  if (level_weight) {
    if (P->loc >= LOC_CC) return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: level_weight must be NULL for a 2-D field", what);
    for (int k = 0; k < levels; k++)
      if (!std::isfinite(level_weight[k]) || level_weight[k] < 0.0)
        return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: level_weight[%d] = %g must be finite and >= 0", what, k, level_weight[k]);
  }
  P->e[0] = Nx / B->bx;
  P->e[1] = Ny / B->by;
  P->e[2] = P->kc / B->bz;
  return GB25_OK;
}
gb25_status blocks_plan_field(gb25_model* m, const char* what, gb25_field f, BlockPlan* P) {
  if (f < 0 || f >= GB25_FIELD_COUNT) return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: no field %d", what, (int)f);
  if (m->own_stream && !m->f[f].d)
    return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: this model has no such field (closure = CATKEVerticalDiffusivity() only)", what);
  // (from the configuration alone: the dims need no device)
  P->loc = moments_loc(f);
  P->fine[0] = m->Nx; P->fine[1] = m->Ny;
  P->fine[2] = P->loc >= LOC_CC ? 1 : m->cfg.Nz + (P->loc == LOC_CCF ? 1 : 0);
  return GB25_OK;
}
gb25_status blocks_plan_derived(gb25_model* m, const char* what, gb25_derived q, BlockPlan* P) {
  if (q < 0 || q >= GB25_D_COUNT) return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: no derived field %d (0 .. %d)", what, (int)q, GB25_D_COUNT - 1);
  if (q == GB25_D_VORTICITY)
    return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: derived GB25_D_VORTICITY lives at (f,f,c), for which the measure is not defined", what);
  int32_t d[3];
  derived_extents(m, q, d);
  P->fine[0] = m->Nx; P->fine[1] = m->Ny; P->fine[2] = d[2];
  P->loc = q == GB25_D_MIXED_LAYER_DEPTH ? LOC_CC : LOC_CCC;
  return GB25_OK;
}

// the counts, the weights, the planes, then the waves' slots; made by the first call, made anew when a call needs more bytes
gb25_status blocks_buffer(gb25_model* m, const char* what, size_t elems, size_t waves) {
  DiagState& D = m->diag;
  const size_t bytes = BLOCK_HEAD + ((size_t)m->cfg.Nz + 1 + 3 * elems) * sizeof(double) + waves * sizeof(BlockSlot);
  if (D.blocks && bytes <= D.block_bytes) return GB25_OK;
  D.drop(D.blocks);
  D.block_bytes = 0;
  if (gb25_status s = diag_room_for(m, what, "the planes of the block sums", (double)bytes)) return s;
  HIPCHK(hipMalloc(&D.blocks, bytes));
  D.block_bytes = bytes;
  return GB25_OK;
}
inline BlockCounts* blocks_counts(gb25_model* m) { return (BlockCounts*)m->diag.blocks; }
inline double* blocks_weights(gb25_model* m) { return (double*)((char*)m->diag.blocks + BLOCK_HEAD); }
// (the planes of the CALL lie one after another, the slots of its waves behind them, whatever the buffer has room for)
inline double* blocks_planes(gb25_model* m) { return blocks_weights(m) + m->cfg.Nz + 1; }

template <int LOC>
void blocks_launch_loc(gb25_model* m, const dim3& grd, const MomentsTables& tab, const real* src, const DiagBox& b, const BlockArgs& A) {
  if (A.bx == 1) hipLaunchKernelGGL((k_block_sums<real, LOC, true>), grd, dim3(BLK_THREADS), 0, m->stream, m->g, tab, src, b, A);
  else hipLaunchKernelGGL((k_block_sums<real, LOC, false>), grd, dim3(BLK_THREADS), 0, m->stream, m->g, tab, src, b, A);
}

// The launch over src, whose element (0, 0, k_first) is box.origin, on m->stream behind whatever made src; the model has been
// waited for.  The planes lie at blocks_planes, the counts at blocks_counts, when the stream has run.
gb25_status blocks_run(gb25_model* m, const char* what, const BlockPlan& P, const gb25_blocks& B, const double* level_weight, const real* src,
                       const DiagBox& box) {
  const size_t elems = (size_t)P.e[0] * P.e[1] * P.e[2];
  const int W = (BLK_THREADS / B.bx) * B.bx;
  const dim3 grd((P.fine[0] + W - 1) / W, P.e[1], P.e[2]);
  const long long waves = (long long)grd.x * grd.y * grd.z * (BLK_THREADS / 64);
  if (gb25_status s = blocks_buffer(m, what, elems, (size_t)waves)) return s;
  if (gb25_status s = moments_tables(m)) return s;
  DiagState& D = m->diag;
  HIPCHK(hipMemsetAsync(blocks_counts(m), 0, BLOCK_HEAD, m->stream));
  if (level_weight) {
    D.block_weights.assign(level_weight, level_weight + P.fine[2]);
    HIPCHK(hipMemcpyAsync(blocks_weights(m), D.block_weights.data(), (size_t)P.fine[2] * sizeof(double), hipMemcpyHostToDevice, m->stream));
  }
  MomentsTables tab;
  for (int q = 0; q < 3; q++) {
    tab.area[q] = D.area[q];
    tab.first[q] = D.first_wet[q];
  }
  tab.pivot_row = is_folded(m) ? m->Ny - 1 : -1;
  double* planes = blocks_planes(m);
  BlockArgs A = {};
  A.bx = B.bx; A.by = B.by; A.bz = B.bz;
  A.k_first = B.k_first;
  A.nI = P.e[0]; A.nJ = P.e[1]; A.nK = P.e[2];
  A.level_weight = level_weight ? blocks_weights(m) : nullptr;
  A.measure = planes; A.first = planes + elems; A.second = planes + 2 * elems;
  A.slots = (BlockSlot*)(planes + 3 * elems);
  Timed t(m, GB25_K_DIAGNOSTICS);
  switch (P.loc) {
    case LOC_CCC: blocks_launch_loc<LOC_CCC>(m, grd, tab, src, box, A); break;
    case LOC_FCC: blocks_launch_loc<LOC_FCC>(m, grd, tab, src, box, A); break;
    case LOC_CFC: blocks_launch_loc<LOC_CFC>(m, grd, tab, src, box, A); break;
    case LOC_CCF: blocks_launch_loc<LOC_CCF>(m, grd, tab, src, box, A); break;
    case LOC_CC: blocks_launch_loc<LOC_CC>(m, grd, tab, src, box, A); break;
    case LOC_FC: blocks_launch_loc<LOC_FC>(m, grd, tab, src, box, A); break;
    case LOC_CF: blocks_launch_loc<LOC_CF>(m, grd, tab, src, box, A); break;
  }
  LAUNCHCHK();
  const unsigned folders = (unsigned)std::min<long long>(64, (waves + BLK_THREADS - 1) / BLK_THREADS);
  hipLaunchKernelGGL(k_block_counts, dim3(folders), dim3(BLK_THREADS), 0, m->stream, (const BlockSlot*)A.slots, waves, blocks_counts(m));
  LAUNCHCHK();
  return GB25_OK;
}

// checks, source, launch: a field
gb25_status blocks_of_field(gb25_model* m, const char* what, gb25_field f, const gb25_blocks* B, const double* level_weight, BlockPlan* P) {
  if (gb25_status s = blocks_plan_field(m, what, f, P)) return s;
  if (gb25_status s = blocks_check(m, what, B, level_weight, P)) return s;
  if (gb25_status s = diag_need_device(m, what)) return s;
  const real* src = nullptr;
  DiagBox b;
  if (gb25_status s = diag_source(m, f, &src)) return s;
  if (gb25_status s = diag_box(m, f, 0, &b)) return s;
  if (gb25_status s = wait_for_model(m)) return s;
  b.origin += b.plane * B->k_first;
  return blocks_run(m, what, *P, *B, level_weight, src, b);
}
// ... a derived field: gb25_compute_derived's launches into the model's packed array, then the same kernel over that array
gb25_status blocks_of_derived(gb25_model* m, const char* what, gb25_derived q, double param, const gb25_blocks* B, const double* level_weight,
                              BlockPlan* P) {
  if (gb25_status s = blocks_plan_derived(m, what, q, P)) return s;
  if (gb25_status s = derived_check(m, what, q, param)) return s;
  if (gb25_status s = blocks_check(m, what, B, level_weight, P)) return s;
  if (gb25_status s = diag_need_device(m, what)) return s;
  const real* src = nullptr;
  if (gb25_status s = derived_run(m, q, param, B->k_first, P->kc, &src)) return s;
  const DiagBox b{P->fine[0], P->fine[1], P->kc, (long long)P->fine[0], (long long)P->fine[0] * P->fine[1], 0};   // (packed: the levels of the window alone)
  return blocks_run(m, what, *P, *B, level_weight, src, b);
}

// the counts to the host (behind the launch; the caller's last copy synchronizes), then the record
void blocks_fill_info(const gb25_model* m, const BlockPlan& P, const BlockCounts& c, gb25_block_info* info) {
  memset(info, 0, sizeof *info);
  memcpy(info->dims, P.e, sizeof P.e);
  info->points = (int64_t)c.points;
  info->nonfinite = (int64_t)c.nonfinite;
  info->empty_blocks = (int64_t)c.empty_blocks;
  diag_global_offset(m, GB25_T, 0, info->global_offset);   // (interior: the offsets are those of any field of the rank, 0 in k)
}
gb25_status blocks_download(gb25_model* m, const BlockPlan& P, double* measure, double* first, double* second, gb25_block_info* info) {
  const size_t elems = (size_t)P.e[0] * P.e[1] * P.e[2];
  double* host[3] = {measure, first, second};
  for (int q = 0; q < 3; q++)
    if (host[q]) HIPCHK(hipMemcpyAsync(host[q], blocks_planes(m) + q * elems, elems * sizeof(double), hipMemcpyDeviceToHost, m->stream));
  BlockCounts c = {};
  if (gb25_status s = diag_download(m, &c, blocks_counts(m), sizeof c)) return s;
  if (info) blocks_fill_info(m, P, c, info);
  return GB25_OK;
}

}  // namespace

extern "C" {

int32_t gb25_block_info_bytes(void) { return (int32_t)sizeof(gb25_block_info); }

gb25_status gb25_block_dims(const gb25_model* m, gb25_field f, const gb25_blocks* blocks, int32_t dims[3]) {
  if (!m || !dims) return GB25_ERR_INVALID_ARGUMENT;
  gb25_model* mm = const_cast<gb25_model*>(m);   // (the error string alone is written)
  BlockPlan P;
  if (gb25_status s = blocks_plan_field(mm, "gb25_block_dims", f, &P)) return s;
  if (gb25_status s = blocks_check(mm, "gb25_block_dims", blocks, nullptr, &P)) return s;
  memcpy(dims, P.e, sizeof P.e);
  return GB25_OK;
}

gb25_status gb25_derived_block_dims(const gb25_model* m, gb25_derived q, const gb25_blocks* blocks, int32_t dims[3]) {
  if (!m || !dims) return GB25_ERR_INVALID_ARGUMENT;
  gb25_model* mm = const_cast<gb25_model*>(m);
  BlockPlan P;
  if (gb25_status s = blocks_plan_derived(mm, "gb25_derived_block_dims", q, &P)) return s;
  if (gb25_status s = blocks_check(mm, "gb25_derived_block_dims", blocks, nullptr, &P)) return s;
  memcpy(dims, P.e, sizeof P.e);
  return GB25_OK;
}

gb25_status gb25_get_block_sums(gb25_model* m, gb25_field f, const gb25_blocks* blocks, const double* level_weight, double* measure,
                                double* first, double* second, gb25_block_info* info) {
  if (!m) return GB25_ERR_INVALID_ARGUMENT;
  const char* what = "gb25_get_block_sums";
  if (!measure && !first && !second) return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: measure, first and second are all NULL: no output requested", what);
  BlockPlan P;
  if (gb25_status s = blocks_of_field(m, what, f, blocks, level_weight, &P)) return s;
  return blocks_download(m, P, measure, first, second, info);
}

gb25_status gb25_compute_block_sums(gb25_model* m, gb25_field f, const gb25_blocks* blocks, const double* level_weight, gb25_block_info* info,
                                    const double** dev, int32_t device_dims[3]) {
  if (!m) return GB25_ERR_INVALID_ARGUMENT;
  const char* what = "gb25_compute_block_sums";
  if (!dev) return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: dev is NULL: no output requested", what);
  BlockPlan P;
  if (gb25_status s = blocks_of_field(m, what, f, blocks, level_weight, &P)) return s;
  if (gb25_status s = blocks_download(m, P, nullptr, nullptr, nullptr, info)) return s;   // (the counts; the stream is quiet behind it)
  *dev = blocks_planes(m);
  if (device_dims) memcpy(device_dims, P.e, sizeof P.e);
  return GB25_OK;
}

gb25_status gb25_get_derived_block_sums(gb25_model* m, gb25_derived q, double param, const gb25_blocks* blocks, const double* level_weight,
                                        double* measure, double* first, double* second, gb25_block_info* info) {
  if (!m) return GB25_ERR_INVALID_ARGUMENT;
  const char* what = "gb25_get_derived_block_sums";
  if (!measure && !first && !second) return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: measure, first and second are all NULL: no output requested", what);
  BlockPlan P;
  if (gb25_status s = blocks_of_derived(m, what, q, param, blocks, level_weight, &P)) return s;
  return blocks_download(m, P, measure, first, second, info);
}

}  // extern "C"
