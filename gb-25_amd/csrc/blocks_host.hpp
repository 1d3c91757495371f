// blocks_host.hpp -- host side of gb25_block_dims / gb25_derived_block_dims / gb25_get_block_sums / gb25_compute_block_sums /
// gb25_get_derived_block_sums / gb25_block_info_bytes (include/gb25.h); included by gb25_api.hip behind diagnostics_host.hpp, whose
// shared pieces it is built from: what a call reads (DiagSource), the measure (moments_tables, diag_measure_tables, diag_with_loc),
// the way of planes and counts to the host, diag_*.  Kernel: block_kernels.hpp; the memory: blocks (a result buffer),
// block_weights of DiagState (diagnostics_state.hpp).  Like the other diagnostics nothing here writes model memory or a schedule
// flag: the only memory written is the results' own buffer.
#pragma once

namespace {

static_assert(BLK_THREADS == GB25_BLOCK_MAX_BX, "the kernel's tile is the header's largest bx");

// What is specific to a call of the block sums, beside its source's plan: the window and the result
struct BlockPlan {
  int kc;            // the resolved k_count
  int32_t e[3];      // the result's dims
};

// the checks that need no device, over the source S: Nx columns and Ny rows of cell centres, ITS levels
gb25_status blocks_check(gb25_model* m, const char* what, const SourcePlan& S, const gb25_blocks* B, const double* level_weight, BlockPlan* P) {
  if (!B) return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: blocks is NULL", what);
  const int Nx = m->Nx, Ny = m->Ny, levels = S.dims[2];
  if (B->bx <= 0 || B->bx > GB25_BLOCK_MAX_BX || Nx % B->bx)
    return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: bx = %d must be 1 .. %d and divide the rank's Nx = %d", what, (int)B->bx, GB25_BLOCK_MAX_BX, Nx);
  if (B->by <= 0 || Ny % B->by)
    return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: by = %d must be > 0 and divide the rank's Ny = %d (rows of cell centres)", what, (int)B->by, Ny);
  if (gb25_status s = diag_window(m, what, B->k_first, B->k_count, levels, "levels (k_first, k_count)", &P->kc)) return s;
  if (B->bz <= 0 || P->kc % B->bz)
    return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: bz = %d must be > 0 and divide the %d levels of the window", what, (int)B->bz, P->kc);
  if (level_weight) {
    if (S.loc >= LOC_CC) return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: level_weight must be NULL for a 2-D field", what);
    for (int k = 0; k < levels; k++)
      if (!std::isfinite(level_weight[k]) || level_weight[k] < 0.0)
        return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: level_weight[%d] = %g must be finite and >= 0", what, k, level_weight[k]);
  }
  P->e[0] = Nx / B->bx;
  P->e[1] = Ny / B->by;
  P->e[2] = P->kc / B->bz;
  return GB25_OK;
}
// the source's own checks, those of the families that weigh with the measure, then the call's
gb25_status blocks_plan(gb25_model* m, const char* what, const DiagSource& S, const gb25_blocks* B, const double* level_weight, SourcePlan* SP,
                        BlockPlan* P) {
  if (gb25_status s = diag_source_plan(m, what, S, SP)) return s;
  if (gb25_status s = diag_source_measured(m, what, S)) return s;
  return blocks_check(m, what, *SP, B, level_weight, P);
}

// the counts, the weights, the planes, then the waves' slots
gb25_status blocks_buffer(gb25_model* m, const char* what, size_t elems, size_t waves) {
  const size_t bytes = COUNTS_HEAD + ((size_t)m->cfg.Nz + 1 + 3 * elems) * sizeof(double) + waves * sizeof(BlockSlot);
  return m->diag.blocks.grow(m, what, "the planes of the block sums", bytes);
}
inline BlockCounts* blocks_counts(gb25_model* m) { return (BlockCounts*)m->diag.blocks.p; }
inline double* blocks_weights(gb25_model* m) { return (double*)((char*)m->diag.blocks.p + COUNTS_HEAD); }
// (the planes of the CALL lie one after another, the slots of its waves behind them, whatever the buffer has room for)
inline double* blocks_planes(gb25_model* m) { return blocks_weights(m) + m->cfg.Nz + 1; }

// The launch over src, whose element (0, 0, k_first) is box.origin, on m->stream behind whatever made src; the model has been
// waited for.  The planes lie at blocks_planes, the counts at blocks_counts, when the stream has run.
gb25_status blocks_run(gb25_model* m, const char* what, const SourcePlan& S, const BlockPlan& P, const gb25_blocks& B, const double* level_weight,
                       const real* src, const DiagBox& box) {
  const size_t elems = (size_t)P.e[0] * P.e[1] * P.e[2];
  const int W = (BLK_THREADS / B.bx) * B.bx, levels = S.dims[2];
  const dim3 grd((m->Nx + W - 1) / W, P.e[1], P.e[2]);
  const long long waves = (long long)grd.x * grd.y * grd.z * (BLK_THREADS / 64);
  if (gb25_status s = blocks_buffer(m, what, elems, (size_t)waves)) return s;
  if (gb25_status s = moments_tables(m)) return s;
  DiagState& D = m->diag;
  HIPCHK(hipMemsetAsync(blocks_counts(m), 0, COUNTS_HEAD, m->stream));
  if (level_weight) {
    D.block_weights.assign(level_weight, level_weight + levels);
    HIPCHK(hipMemcpyAsync(blocks_weights(m), D.block_weights.data(), (size_t)levels * sizeof(double), hipMemcpyHostToDevice, m->stream));
  }
  const MomentsTables tab = diag_measure_tables(m, true);
  double* planes = blocks_planes(m);
  BlockArgs A = {};
  A.bx = B.bx; A.by = B.by; A.bz = B.bz;
  A.k_first = B.k_first;
  A.nI = P.e[0]; A.nJ = P.e[1]; A.nK = P.e[2];
  A.level_weight = level_weight ? blocks_weights(m) : nullptr;
  A.measure = planes; A.first = planes + elems; A.second = planes + 2 * elems;
  A.slots = (BlockSlot*)(planes + 3 * elems);
  Timed t(m, GB25_K_DIAGNOSTICS);
  diag_with_loc(S.loc, [&](auto loc) {
    constexpr int LOC = decltype(loc)::value;
    if (A.bx == 1) hipLaunchKernelGGL((k_block_sums<real, LOC, true>), grd, dim3(BLK_THREADS), 0, m->stream, m->g, tab, src, box, A);
    else hipLaunchKernelGGL((k_block_sums<real, LOC, false>), grd, dim3(BLK_THREADS), 0, m->stream, m->g, tab, src, box, A);
  });
  LAUNCHCHK();
  const unsigned folders = (unsigned)std::min<long long>(64, (waves + BLK_THREADS - 1) / BLK_THREADS);
  hipLaunchKernelGGL(k_block_counts, dim3(folders), dim3(BLK_THREADS), 0, m->stream, (const BlockSlot*)A.slots, waves, blocks_counts(m));
  LAUNCHCHK();
  return GB25_OK;
}

// checks, source, launch
gb25_status blocks_of(gb25_model* m, const char* what, const DiagSource& S, const gb25_blocks* B, const double* level_weight, BlockPlan* P) {
  SourcePlan SP;
  if (gb25_status s = blocks_plan(m, what, S, B, level_weight, &SP, P)) return s;
  if (gb25_status s = diag_need_device(m, what)) return s;
  const real* src = nullptr;
  DiagBox b;
  if (gb25_status s = diag_source_resolve(m, S, SP, B->k_first, P->kc, &src, &b)) return s;
  return blocks_run(m, what, SP, *P, *B, level_weight, src, b);
}

// the planes asked for and the counts to the host, then the record
gb25_status blocks_download(gb25_model* m, const BlockPlan& P, double* measure, double* first, double* second, gb25_block_info* info) {
  double* const host[3] = {measure, first, second};
  BlockCounts c = {};
  if (gb25_status s = diag_download_planes(m, host, blocks_planes(m), (size_t)P.e[0] * P.e[1] * P.e[2], blocks_counts(m), &c)) return s;
  if (!info) return GB25_OK;
  memset(info, 0, sizeof *info);
  memcpy(info->dims, P.e, sizeof P.e);
  info->points = (int64_t)c.points;
  info->nonfinite = (int64_t)c.nonfinite;
  info->empty_blocks = (int64_t)c.empty_blocks;
  diag_global_offset(m, GB25_T, 0, info->global_offset);   // (interior: the offsets are those of any field of the rank, 0 in k)
  return GB25_OK;
}

// gb25_block_dims and its derived twin
gb25_status blocks_dims(const gb25_model* m, const char* what, const DiagSource& S, const gb25_blocks* B, int32_t dims[3]) {
  if (!m || !dims) return GB25_ERR_INVALID_ARGUMENT;
  SourcePlan SP;
  BlockPlan P;
  if (gb25_status s = blocks_plan(const_cast<gb25_model*>(m), what, S, B, nullptr, &SP, &P)) return s;   // (the error string alone is written)
  memcpy(dims, P.e, sizeof P.e);
  return GB25_OK;
}

}  // namespace

extern "C" {

int32_t gb25_block_info_bytes(void) { return (int32_t)sizeof(gb25_block_info); }

gb25_status gb25_block_dims(const gb25_model* m, gb25_field f, const gb25_blocks* blocks, int32_t dims[3]) {
  return blocks_dims(m, "gb25_block_dims", DiagSource(f), blocks, dims);
}

gb25_status gb25_derived_block_dims(const gb25_model* m, gb25_derived q, const gb25_blocks* blocks, int32_t dims[3]) {
  return blocks_dims(m, "gb25_derived_block_dims", DiagSource(q, 1.0), blocks, dims);   // (the dims do not depend on the parameter)
}

gb25_status gb25_get_block_sums(gb25_model* m, gb25_field f, const gb25_blocks* blocks, const double* level_weight, double* measure,
                                double* first, double* second, gb25_block_info* info) {
  if (!m) return GB25_ERR_INVALID_ARGUMENT;
  const char* what = "gb25_get_block_sums";
  if (!measure && !first && !second) return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: measure, first and second are all NULL: no output requested", what);
  BlockPlan P;
  if (gb25_status s = blocks_of(m, what, DiagSource(f), blocks, level_weight, &P)) return s;
  return blocks_download(m, P, measure, first, second, info);
}

gb25_status gb25_compute_block_sums(gb25_model* m, gb25_field f, const gb25_blocks* blocks, const double* level_weight, gb25_block_info* info,
                                    const double** dev, int32_t device_dims[3]) {
  if (!m) return GB25_ERR_INVALID_ARGUMENT;
  const char* what = "gb25_compute_block_sums";
  if (!dev) return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: dev is NULL: no output requested", what);
  BlockPlan P;
  if (gb25_status s = blocks_of(m, what, DiagSource(f), blocks, level_weight, &P)) return s;
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
  if (gb25_status s = blocks_of(m, what, DiagSource(q, param), blocks, level_weight, &P)) return s;
  return blocks_download(m, P, measure, first, second, info);
}

}  // extern "C"
