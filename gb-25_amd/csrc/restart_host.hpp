// restart_host.hpp -- host side of checkpoint and restart (included by gb25_api.hip behind wait_for_model).  What the set is:
// restart_plan.hpp; the kernel: restart_kernels.hpp; the file: restart_file.hpp.  The arena, the pinned host buffer, the copy
// stream and the two events belong to the model (RestartState, made by the first snapshot, freed by gb25_checkpoint_release and
// gb25_destroy).  A snapshot is one launch on the model's stream, filed under GB25_K_DIAGNOSTICS; it moves no buffer and voids
// nothing; the drain to the host runs on a stream of its own behind an event.  DESIGN.md, "Checkpoint and restart".
#include "restart_plan.hpp"
#include "restart_file.hpp"

struct RestartState {
  RestartPlan plan;
  RestartScalars scalars;
  std::vector<std::vector<RestartSpan>> pieces;
  std::vector<RestartSeg> segs;          // of every piece, one after the other (block0: within its piece)
  std::vector<size_t> piece_seg0;        // first segment of piece q; one more entry at the end
  std::vector<size_t> piece_block0;      // first pair of partial sums of piece q in h_partials; one more entry at the end
  bool taken = false;                    // a snapshot waits to be written or released
  unsigned char* d_arena = nullptr;
  size_t arena_cap = 0;
  RestartSeg* d_segs = nullptr;
  size_t d_segs_cap = 0;
  RestartSeg* h_segs = nullptr;          // pinned: the table of a launch goes up without a staging copy the host would wait for
  size_t h_segs_cap = 0;
  unsigned long long* d_partials = nullptr;
  size_t d_partials_cap = 0;             // pairs
  unsigned char* h_set = nullptr;        // pinned: the whole set, members at the offsets of the plan
  size_t h_set_cap = 0;
  unsigned long long* h_partials = nullptr;   // pinned
  size_t h_partials_cap = 0;             // pairs
  hipStream_t copy_stream = nullptr;
  hipEvent_t ev_packed = nullptr, ev_drained = nullptr;
  void release() {
    if (copy_stream) (void)hipStreamSynchronize(copy_stream);
    if (d_arena) (void)hipFree(d_arena);
    if (d_segs) (void)hipFree(d_segs);
    if (d_partials) (void)hipFree(d_partials);
    if (h_set) (void)hipHostFree(h_set);
    if (h_partials) (void)hipHostFree(h_partials);
    if (h_segs) (void)hipHostFree(h_segs);
    if (ev_packed) (void)hipEventDestroy(ev_packed);
    if (ev_drained) (void)hipEventDestroy(ev_drained);
    if (copy_stream) (void)hipStreamDestroy(copy_stream);
    *this = RestartState();
  }
};

namespace {

void restart_release(gb25_model* m) {
  if (!m->restart) return;
  m->restart->release();
  delete m->restart;
  m->restart = nullptr;
}

RestartSwitches restart_switches(const gb25_model* m) {
  RestartSwitches sw;
  sw.catke = m->catke;
  sw.phy_stored = !m->phy_stale;
  for (int q = 0; q < 4; q++) sw.top_flux[q] = m->g.top_flux[q] != nullptr;
  sw.ahead_ts = m->valid.ahead_valid;
  sw.ahead_uv = m->valid.ahead_uv_valid;
  sw.ahead_baro = m->valid.ahead_baro_valid;
  sw.colsums = m->valid.colsum_valid;
  return sw;
}

// The two checksums over what gb25_get_metric (z faces, the row tables), gb25_get_metric2 and gb25_get_bottom_info (immersed cells,
// depths at the U and V faces) hand out, and over the host's bottom height where one was set.  Made once and kept: every call that
// changes the grid goes through quiesce_for_grid_change, which drops it.
void grid_fingerprint(gb25_model* m, uint64_t* s1, uint64_t* s2) {
  if (!m->grid_print_valid) {
    std::vector<double> v;
    double x = 0;
    for (int k = 1; k <= m->cfg.Nz + 1; k++)
      if (gb25_get_metric(m, GB25_M_ZF, k, &x) == GB25_OK) v.push_back(x);
    for (int id = GB25_M_PHIF; id <= GB25_M_FCOR; id++)
      for (int j = 1; j <= m->Ny + 1; j++)
        if (gb25_get_metric(m, (gb25_metric)id, j, &x) == GB25_OK) v.push_back(x);
    for (int id = 0; id < GB25_M2_COUNT; id++) {
      const size_t n = m->h_curv[id].size(), at = v.size();
      if (!n) continue;
      v.resize(at + n);
      gb25_get_metric2(m, (gb25_metric2)id, v.data() + at, (int64_t)n);
    }
    v.reserve(v.size() + (size_t)3 * m->Nx * m->Ny + m->host_bottom.size());
    for (int which = 0; which < 3; which++)
      for (int j = 0; j < m->Ny; j++)
        for (int i = 0; i < m->Nx; i++)
          if (gb25_get_bottom_info(m, which, i, j, &x) == GB25_OK) v.push_back(x);
    v.insert(v.end(), m->host_bottom.begin(), m->host_bottom.end());
    m->grid_print[0] = m->grid_print[1] = 0;
    restart_checksums(v.data(), v.size(), 8, 0, &m->grid_print[0], &m->grid_print[1]);
    m->grid_print_valid = true;
  }
  *s1 = m->grid_print[0];
  *s2 = m->grid_print[1];
}

RestartScalars restart_scalars(gb25_model* m, const RestartSwitches& sw) {
  RestartScalars s;
  memset(static_cast<void*>(&s), 0, sizeof s);   // (padding too: a snapshot of the same state gives the same file byte for byte)
  s.time = m->time; s.last_dt = m->last_dt; s.iteration = m->iteration;
  s.real_bytes = (int32_t)sizeof(real); s.config_bytes = (int32_t)sizeof(gb25_config); s.scalars_bytes = (int32_t)sizeof(RestartScalars);
  s.next_step_is_euler = m->iteration == 0;
  s.dt_config = m->cfg.dt; s.chi = m->cfg.chi; s.catke_prev_time = m->catke_prev_time;
  s.nu = m->nu; s.kappa = m->kappa; s.bottom_drag = m->bottom_drag;
  s.catke = m->catke; s.coupled = m->coupled; s.tracer_order = m->tracer_order; s.tracer_rows_forced = m->tracer_rows_forced;
  s.phy_stored = sw.phy_stored;
  for (int q = 0; q < 4; q++) s.top_flux_mask |= sw.top_flux[q] ? 1 << q : 0;
  for (int q = 0; q < kRestartOptionCount; q++) gb25_get_option(m, (gb25_option)kRestartOptions[q], &s.options[q]);
  const Validity<real>& v = m->valid;
  s.ahead_valid = v.ahead_valid; s.ahead_uv_valid = v.ahead_uv_valid; s.ahead_baro_valid = v.ahead_baro_valid;
  s.colsum_valid = v.colsum_valid; s.halo_colsum_valid = v.halo_colsum_valid; s.tend_forkable = v.tend_forkable; s.complete_fills_needed = v.complete_fills_needed;
  s.ahead_ts_folded = m->ahead_ts_folded; s.ahead_eta_folded = m->ahead_eta_folded;
  s.ahead_dt = (double)v.ahead_dt; s.ahead_chi = (double)v.ahead_chi; s.ahead_uv_dt = (double)v.ahead_uv_dt; s.ahead_uv_chi = (double)v.ahead_uv_chi;
  grid_fingerprint(m, &s.grid_s1, &s.grid_s2);
  s.cfg = m->cfg;
  s.catke_par = m->catke_par;
  return s;
}

// where member q lives on the device: for a snapshot the buffer that holds it NOW (CATKE's previous velocities wherever
// prev_uv_src says, without moving them); for a restore its own field.  partner: the other buffer of an alternating pair, which a
// restore fills too, so that the halo layers no kernel rewrites are the same in both (as gb25_set_field does).
unsigned char* restart_member_ptr(gb25_model* m, const RestartMember& mem, bool for_restore, unsigned char** partner, const RestartSwitches& sw) {
  *partner = nullptr;
  if (mem.field < 0) {
    const int x = mem.extra;
    real* p = x <= RESTART_TOP_FLUX_S ? m->d_top_flux[x - RESTART_TOP_FLUX_U]
            : x <= RESTART_AHEAD_S ? m->ahead[x - RESTART_AHEAD_T].d
            : x <= RESTART_AHEAD_V ? m->ahead_uv[x - RESTART_AHEAD_U].d
            : x <= RESTART_AHEAD_GV ? m->ahead_G[x - RESTART_AHEAD_GU].d
            : x <= RESTART_AHEAD_COLSUM_V ? m->ahead_colsum[x - RESTART_AHEAD_COLSUM_U].d
            : x == RESTART_AHEAD_PARTIALS ? m->uv_partials
            : x <= RESTART_AHEAD_BT_V ? m->ahead_eta[x - RESTART_AHEAD_ETA].d
            : x <= RESTART_AHEAD_V_BAR ? m->ahead_bar[x - RESTART_AHEAD_ETA_BAR].d
            : m->colsum[x - RESTART_COLSUM_U].d;
    return reinterpret_cast<unsigned char*>(p);
  }
  const int id = mem.field;
  real* p = m->f[id].d;
  if (!for_restore && m->catke && (id == GB25_PREV_U || id == GB25_PREV_V) && m->prev_uv_src != 0) {
    const int q = id - GB25_PREV_U;
    p = m->prev_uv_src == 1 ? m->f[GB25_U + q].d : m->ahead_uv[q].d;
  }
  if (for_restore) {
    real* other = nullptr;
    // (a partner that is a member itself gets its own bytes)
    if (id == GB25_T || id == GB25_S) other = sw.ahead_ts ? nullptr : m->ahead[id - GB25_T].d;
    else if (id == GB25_U || id == GB25_V) other = sw.ahead_uv ? nullptr : m->ahead_uv[id - GB25_U].d;
    else if (id >= GB25_ETA && id <= GB25_BT_V) other = sw.ahead_baro ? nullptr : m->ahead_eta[id - GB25_ETA].d;
    else if (id >= GB25_ETA_BAR && id <= GB25_V_BAR) other = sw.ahead_baro ? nullptr : m->ahead_bar[id - GB25_ETA_BAR].d;
    *partner = reinterpret_cast<unsigned char*>(other);
  }
  return reinterpret_cast<unsigned char*>(p);
}

// the bytes of the array member `mem` lives in, as it was allocated
size_t restart_member_bytes(const gb25_model* m, const RestartMember& mem) {
  if (mem.field >= 0) return m->f[mem.field].elems() * sizeof(real);
  const int x = mem.extra;
  const size_t elems = x <= RESTART_TOP_FLUX_S ? m->top_flux_elems[x - RESTART_TOP_FLUX_U]
                     : x <= RESTART_AHEAD_S ? m->ahead[x - RESTART_AHEAD_T].elems()
                     : x <= RESTART_AHEAD_V ? m->ahead_uv[x - RESTART_AHEAD_U].elems()
                     : x <= RESTART_AHEAD_GV ? m->ahead_G[x - RESTART_AHEAD_GU].elems()
                     : x <= RESTART_AHEAD_COLSUM_V ? m->ahead_colsum[x - RESTART_AHEAD_COLSUM_U].elems()
                     : x == RESTART_AHEAD_PARTIALS ? 4 * chunk_columns(m->layout)
                     : x <= RESTART_AHEAD_BT_V ? m->ahead_eta[x - RESTART_AHEAD_ETA].elems()
                     : x <= RESTART_AHEAD_V_BAR ? m->ahead_bar[x - RESTART_AHEAD_ETA_BAR].elems()
                     : m->colsum[x - RESTART_COLSUM_U].elems();
  return elems * sizeof(real);
}

// the segments of every piece.  to_fields: arena -> fields (restore), else fields -> arena; copy = false: checksums of the arena only
gb25_status restart_build_segments(gb25_model* m, RestartState& R, bool to_fields, bool copy, const RestartSwitches& sw) {
  R.segs.clear();
  R.piece_seg0.assign(1, 0);
  R.piece_block0.assign(1, 0);
  for (const auto& piece : R.pieces) {
    unsigned block = 0;
    for (const RestartSpan& sp : piece) {
      const RestartMember& mem = R.plan.members[sp.member];
      unsigned char* partner = nullptr;
      unsigned char* field = restart_member_ptr(m, mem, to_fields, &partner, sw);
      // (the plan's bytes against the array that is there: a span never leaves it.  A top flux array may be larger than its member:
      // the coupling allocates the rows of a y-face field for all four.)  A pass that only sums the arena touches no array.
      const size_t have = restart_member_bytes(m, mem);
      const bool fits = mem.field < 0 && mem.extra <= RESTART_TOP_FLUX_S ? have >= mem.bytes : have == mem.bytes;
      if (to_fields && !copy) field = nullptr;
      else if (!field) return fail(m, GB25_ERR_STATE, "internal: member %s of the restart set has no array", mem.name.c_str());
      if ((field && !fits) || sp.begin + sp.bytes > mem.bytes)
        return fail(m, GB25_ERR_STATE, "internal: member %s has %zu bytes on the device, the restart plan says %llu", mem.name.c_str(), have,
                    (unsigned long long)mem.bytes);
      RestartSeg g{};
      unsigned char* in_arena = R.d_arena + sp.arena_offset;
      if (to_fields) {
        g.src = in_arena;
        g.dst = copy ? field + sp.begin : nullptr;
        g.dst2 = copy && partner ? partner + sp.begin : nullptr;
      } else {
        g.src = field + sp.begin;
        g.dst = in_arena;
      }
      g.bytes = sp.bytes;
      g.elem0 = sp.begin / (uint64_t)mem.elem_bytes;
      g.elem_bytes = (unsigned)mem.elem_bytes;
      g.member = (unsigned)sp.member;
      const uintptr_t off16 = reinterpret_cast<uintptr_t>(g.src) | reinterpret_cast<uintptr_t>(g.dst) | reinterpret_cast<uintptr_t>(g.dst2);
      g.scalar = (off16 & 15) != 0;
      const uint64_t work = g.scalar ? (g.bytes + kRestartBlockBytes - 1) / kRestartBlockBytes
                                     : (g.bytes / 16 + kRestartVectorsPerBlock - 1) / kRestartVectorsPerBlock;
      g.block0 = block;
      g.nblocks = (unsigned)std::max<uint64_t>(1, work);
      block += g.nblocks;
      R.segs.push_back(g);
    }
    R.piece_seg0.push_back(R.segs.size());
    R.piece_block0.push_back(R.piece_block0.back() + block);
  }
  return GB25_OK;
}

template <class T>
gb25_status restart_grow_device(gb25_model* m, T*& p, size_t& cap, size_t need) {
  if (cap >= need) return GB25_OK;
  if (p) (void)hipFree(p);
  p = nullptr; cap = 0;
  if (hipMalloc(reinterpret_cast<void**>(&p), need * sizeof(T)) != hipSuccess) {
    (void)hipGetLastError();
    return fail(m, GB25_ERR_OUT_OF_MEMORY, "checkpoint: cannot allocate %zu bytes on the device", need * sizeof(T));
  }
  cap = need;
  return GB25_OK;
}
template <class T>
gb25_status restart_grow_pinned(gb25_model* m, T*& p, size_t& cap, size_t need) {
  if (cap >= need) return GB25_OK;
  if (p) (void)hipHostFree(p);
  p = nullptr; cap = 0;
  if (hipHostMalloc(reinterpret_cast<void**>(&p), need * sizeof(T), hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();
    return fail(m, GB25_ERR_OUT_OF_MEMORY, "checkpoint: cannot allocate %zu bytes of pinned host memory", need * sizeof(T));
  }
  cap = need;
  return GB25_OK;
}

// the plan, the pieces under `cap`, and every buffer they need
gb25_status restart_prepare(gb25_model* m, const RestartSwitches& sw, uint64_t cap) {
  RestartPlan plan = plan_restart(m->layout, sw, (int)sizeof(real));
  if (plan.status) return fail(m, plan.status, "%s", plan.refusal.c_str());
  if (!m->restart) m->restart = new RestartState();
  RestartState& R = *m->restart;
  R.plan = plan;
  if (!R.copy_stream) HIPCHK(hipStreamCreateWithFlags(&R.copy_stream, hipStreamNonBlocking));
  if (!R.ev_packed) HIPCHK(hipEventCreateWithFlags(&R.ev_packed, hipEventDisableTiming));
  if (!R.ev_drained) HIPCHK(hipEventCreateWithFlags(&R.ev_drained, hipEventDisableTiming));
  // the arena: the whole set, or what the cap allows, or -- when the device has no room for that -- half of it, and half again
  uint64_t want = cap > 0 ? std::min<uint64_t>(R.plan.arena_bytes, std::max<uint64_t>(16, cap & ~(uint64_t)15)) : R.plan.arena_bytes;
  if (R.arena_cap < want || (cap > 0 && R.arena_cap > want)) {
    if (R.d_arena) (void)hipFree(R.d_arena);
    R.d_arena = nullptr; R.arena_cap = 0;
    while (hipMalloc(reinterpret_cast<void**>(&R.d_arena), want) != hipSuccess) {
      (void)hipGetLastError();
      R.d_arena = nullptr;
      if (cap > 0 || want <= (1u << 20)) return fail(m, GB25_ERR_OUT_OF_MEMORY, "checkpoint: cannot allocate an arena of %llu bytes", (unsigned long long)want);
      want = (want / 2) & ~(uint64_t)15;
    }
    R.arena_cap = want;
  }
  R.pieces = restart_pieces(R.plan, R.arena_cap >= R.plan.arena_bytes ? 0 : R.arena_cap);
  return GB25_OK;
}
gb25_status restart_size_buffers(gb25_model* m, RestartState& R) {
  size_t most_segs = 0, most_blocks = 0;
  for (size_t q = 0; q + 1 < R.piece_seg0.size(); q++) {
    most_segs = std::max(most_segs, R.piece_seg0[q + 1] - R.piece_seg0[q]);
    most_blocks = std::max(most_blocks, R.piece_block0[q + 1] - R.piece_block0[q]);
  }
  if (gb25_status s = restart_grow_device(m, R.d_segs, R.d_segs_cap, most_segs)) return s;
  if (gb25_status s = restart_grow_device(m, R.d_partials, R.d_partials_cap, 2 * most_blocks)) return s;
  HIPCHK(hipStreamSynchronize(m->restart->copy_stream));   // (nothing reads the pinned tables of an earlier call any more)
  if (gb25_status s = restart_grow_pinned(m, R.h_segs, R.h_segs_cap, R.segs.size())) return s;
  std::copy(R.segs.begin(), R.segs.end(), R.h_segs);
  return restart_grow_pinned(m, R.h_partials, R.h_partials_cap, 2 * R.piece_block0.back());
}

// ONE launch over the segments of piece q on the model's stream; its partial sums land in d_partials
gb25_status restart_launch_piece(gb25_model* m, RestartState& R, size_t q) {
  const size_t s0 = R.piece_seg0[q], ns = R.piece_seg0[q + 1] - s0;
  const size_t nb = R.piece_block0[q + 1] - R.piece_block0[q];
  HIPCHK(hipMemcpyAsync(R.d_segs, R.h_segs + s0, ns * sizeof(RestartSeg), hipMemcpyHostToDevice, m->stream));
  Timed t(m, GB25_K_DIAGNOSTICS);
  hipLaunchKernelGGL(k_restart_pack, dim3((unsigned)nb), dim3(kRestartThreads), 0, m->stream, R.d_segs, (int)ns, R.d_partials);
  LAUNCHCHK();
  return GB25_OK;
}
// the sums of every member from the partial sums of its blocks (h_partials: complete)
void restart_sum_partials(const RestartState& R, std::vector<uint64_t>& s1, std::vector<uint64_t>& s2) {
  s1.assign(R.plan.members.size(), 0);
  s2.assign(R.plan.members.size(), 0);
  for (size_t q = 0; q + 1 < R.piece_seg0.size(); q++)
    for (size_t s = R.piece_seg0[q]; s < R.piece_seg0[q + 1]; s++) {
      const RestartSeg& g = R.segs[s];
      const unsigned long long* part = R.h_partials + 2 * (R.piece_block0[q] + g.block0);
      for (unsigned b = 0; b < g.nblocks; b++) { s1[g.member] += part[2 * b]; s2[g.member] += part[2 * b + 1]; }
    }
}

std::string restart_path(const gb25_model* m, const char* directory, const char* label, bool make_dirs) {
  const std::string dir = std::string(directory) + "/" + (label && *label ? label : "checkpoint");
  if (make_dirs)
    for (size_t q = 1; q <= dir.size(); q++)   // mkpath
      if (q == dir.size() || dir[q] == '/') mkdir(dir.substr(0, q).c_str(), 0777);
  return dir + "/restart_rank" + std::to_string(m->cfg.rank) + ".gb25";
}

}  // namespace

extern "C" {

int32_t gb25_checkpoint_info_bytes(void) { return (int32_t)sizeof(gb25_checkpoint_info); }
int32_t gb25_restore_info_bytes(void) { return (int32_t)sizeof(gb25_restore_info); }

gb25_status gb25_checkpoint_snapshot(gb25_model* m, int64_t max_arena_bytes) {
  CHECK_MODEL(m);
  if (max_arena_bytes < 0) return fail(m, GB25_ERR_INVALID_ARGUMENT, "gb25_checkpoint_snapshot: max_arena_bytes must be >= 0 (0: no cap)");
  if (m->restart && m->restart->taken)
    return fail(m, GB25_ERR_STATE, "a snapshot waits to be written: gb25_checkpoint_write or gb25_checkpoint_release first");
  if (m->route.memory_lacks_correction() || m->route.w_field_stale())
    return fail(m, GB25_ERR_STATE, "a composite call failed half-way: memory does not hold the corrected velocities and their w, nothing to checkpoint");
  // (a look-ahead sub-cycle on a stream of its own writes members: the snapshot runs behind it)
  if (m->baro_inflight) HIPCHK(hipStreamWaitEvent(m->stream, m->ev_baro, 0));
  // (a rank of a decomposition: the chain of the sub-cycle look-ahead runs on the exchange streams; the host waits for it here)
  if (m->group) HIPCHK(m->group->sync_side());
  const RestartSwitches sw = restart_switches(m);
  if (gb25_status s = restart_prepare(m, sw, (uint64_t)max_arena_bytes)) return s;
  RestartState& R = *m->restart;
  R.scalars = restart_scalars(m, sw);
  if (gb25_status s = restart_build_segments(m, R, false, true, sw)) return s;
  if (gb25_status s = restart_size_buffers(m, R)) return s;
  if (gb25_status s = restart_grow_pinned(m, R.h_set, R.h_set_cap, (size_t)R.plan.arena_bytes)) return s;
  const bool whole = R.pieces.size() == 1;
  for (size_t q = 0; q < R.pieces.size(); q++) {
    if (gb25_status s = restart_launch_piece(m, R, q)) return s;
    HIPCHK(hipEventRecord(R.ev_packed, m->stream));
    HIPCHK(hipStreamWaitEvent(R.copy_stream, R.ev_packed, 0));
    const size_t nb = R.piece_block0[q + 1] - R.piece_block0[q];
    HIPCHK(hipMemcpyAsync(R.h_partials + 2 * R.piece_block0[q], R.d_partials, 2 * nb * sizeof(unsigned long long), hipMemcpyDeviceToHost, R.copy_stream));
    if (whole) {
      HIPCHK(hipMemcpyAsync(R.h_set, R.d_arena, (size_t)R.plan.arena_bytes, hipMemcpyDeviceToHost, R.copy_stream));
    } else {
      // a bounded arena: every span to its place in the set, and the model waits until the piece has drained
      for (const RestartSpan& sp : R.pieces[q])
        HIPCHK(hipMemcpyAsync(R.h_set + R.plan.members[sp.member].offset + sp.begin, R.d_arena + sp.arena_offset, (size_t)sp.bytes,
                              hipMemcpyDeviceToHost, R.copy_stream));
      HIPCHK(hipStreamSynchronize(R.copy_stream));
    }
  }
  HIPCHK(hipEventRecord(R.ev_drained, R.copy_stream));
  R.taken = true;
  return GB25_OK;
}

gb25_status gb25_checkpoint_get_info(const gb25_model* m, gb25_checkpoint_info* info) {
  if (!m || !info) return GB25_ERR_INVALID_ARGUMENT;
  memset(info, 0, sizeof *info);
  info->averages_open_not_saved = m->diag.avg_on ? 1 : 0;
  info->particles_open_not_saved = m->diag.part_on ? 1 : 0;
  if (!m->restart) return GB25_OK;
  const RestartState& R = *m->restart;
  info->taken = R.taken ? 1 : 0;
  info->members = (int32_t)R.plan.members.size();
  info->pieces = (int32_t)R.pieces.size();
  info->bytes = (int64_t)R.plan.arena_bytes;
  info->arena_bytes = (int64_t)R.arena_cap;
  info->drained = R.taken && hipEventQuery(R.ev_drained) == hipSuccess ? 1 : 0;
  return GB25_OK;
}

gb25_status gb25_checkpoint_write(gb25_model* m, const char* directory, const char* label) {
  CHECK_MODEL(m);
  if (!directory || !*directory) return GB25_ERR_INVALID_ARGUMENT;
  if (!m->restart || !m->restart->taken) return fail(m, GB25_ERR_STATE, "gb25_checkpoint_write: no snapshot has been taken (gb25_checkpoint_snapshot first)");
  RestartState& R = *m->restart;
  HIPCHK(hipEventSynchronize(R.ev_drained));   // (the drain only: the model's stream is not waited for)
  std::vector<uint64_t> s1, s2;
  restart_sum_partials(R, s1, s2);
  std::vector<RestartFileRow> rows(R.plan.members.size());
  for (size_t q = 0; q < rows.size(); q++) {
    const RestartMember& mem = R.plan.members[q];
    RestartFileRow& r = rows[q];
    memset(&r, 0, sizeof r);
    snprintf(r.name, sizeof r.name, "%s", mem.name.c_str());
    r.field = mem.field; r.extra = mem.extra;
    r.dims[0] = mem.dims.nx; r.dims[1] = mem.dims.ny; r.dims[2] = mem.dims.nz;
    r.elem_bytes = mem.elem_bytes; r.bytes = mem.bytes; r.arena_offset = mem.offset;
    r.s1 = s1[q]; r.s2 = s2[q];
  }
  std::string err;
  const std::string path = restart_path(m, directory, label, true);
  if (!restart_write_file(path, (uint32_t)sizeof(real), &R.scalars, (uint32_t)sizeof R.scalars, rows, R.h_set, &err))
    return fail(m, GB25_ERR_STATE, "%s", err.c_str());
  R.taken = false;
  return GB25_OK;
}

gb25_status gb25_checkpoint_release(gb25_model* m) {
  CHECK_MODEL(m);
  restart_release(m);
  return GB25_OK;
}

gb25_status gb25_set_clock(gb25_model* m, double time, int64_t iteration, double last_dt) {
  CHECK_MODEL(m);
  if (!(last_dt > 0) || iteration < 0 || !std::isfinite(time)) return fail(m, GB25_ERR_INVALID_ARGUMENT, "gb25_set_clock: a finite time, iteration >= 0, last_dt > 0");
  if (gb25_status s = collective_guard(m, 4, 1, time)) return s;
  m->time = time;
  m->iteration = iteration;
  m->last_dt = last_dt;
  return GB25_OK;
}

gb25_status gb25_restore(gb25_model* m, const char* directory, const char* label, gb25_restore_info* info) {
  CHECK_MODEL(m);
  if (!directory || !*directory) return GB25_ERR_INVALID_ARGUMENT;
  if (info) memset(info, 0, sizeof *info);
  if (m->restart && m->restart->taken) return fail(m, GB25_ERR_STATE, "a snapshot waits to be written: gb25_checkpoint_write or gb25_checkpoint_release first");
  if (gb25_status s = wait_for_model(m)) return s;
  // ---- 1. the file, and every reason to refuse it that needs no device
  const std::string path = restart_path(m, directory, label, false);
  RestartFile file;
  std::string err;
  if (!file.open(path, &err)) return fail(m, GB25_ERR_STATE, "%s", err.c_str());
  if (file.header.real_bytes != sizeof(real))
    return fail(m, GB25_ERR_STATE, "%s holds %s numbers, this library steps %s", path.c_str(), file.header.real_bytes == 8 ? "Float64" : "Float32",
                sizeof(real) == 8 ? "Float64" : "Float32");
  if (file.scalars.size() != sizeof(RestartScalars))
    return fail(m, GB25_ERR_STATE, "%s: a scalar block of %zu bytes, this library's has %zu", path.c_str(), file.scalars.size(), sizeof(RestartScalars));
  RestartScalars sc;
  memcpy(&sc, file.scalars.data(), sizeof sc);
  if (sc.real_bytes != (int32_t)sizeof(real) || sc.config_bytes != (int32_t)sizeof(gb25_config) || sc.scalars_bytes != (int32_t)sizeof(RestartScalars))
    return fail(m, GB25_ERR_STATE, "%s: written by a library with other struct sizes", path.c_str());
  {
    const gb25_config &a = sc.cfg, &b = m->cfg;
    std::string diff;
    auto cmp = [&diff](const char* name, double x, double y) {
      if (x != y) { char buf[96]; snprintf(buf, sizeof buf, " %s %g (file) / %g (model)", name, x, y); diff += buf; }
    };
    cmp("Nx", a.Nx, b.Nx); cmp("Ny", a.Ny, b.Ny); cmp("Nz", a.Nz, b.Nz); cmp("halo", a.halo, b.halo); cmp("substeps", a.substeps, b.substeps);
    cmp("rank", a.rank, b.rank); cmp("nranks", a.nranks, b.nranks); cmp("ranks_y", a.ranks_y > 1 ? a.ranks_y : 1, b.ranks_y > 1 ? b.ranks_y : 1);
    cmp("slab_mode", a.slab_mode, b.slab_mode); cmp("grid_type", a.grid_type, b.grid_type);
    if (!diff.empty()) {
      const bool decomposition = a.rank != b.rank || a.nranks != b.nranks || a.ranks_y != b.ranks_y || a.slab_mode != b.slab_mode;
      return fail(m, GB25_ERR_STATE, "%s was written by another configuration%s:%s", path.c_str(),
                  decomposition ? " (restarting on another decomposition is not supported)" : "", diff.c_str());
    }
    cmp("chi", a.chi, b.chi); cmp("lat_south", a.lat_south, b.lat_south); cmp("lat_north", a.lat_north, b.lat_north);
    cmp("lon_west", a.lon_west, b.lon_west); cmp("lon_east", a.lon_east, b.lon_east); cmp("depth", a.depth, b.depth); cmp("zexp_h", a.zexp_h, b.zexp_h);
    cmp("g", a.g, b.g); cmp("Omega", a.Omega, b.Omega); cmp("radius", a.radius, b.radius); cmp("rho0", a.rho0, b.rho0);
    if (!diff.empty()) return fail(m, GB25_ERR_STATE, "%s was written by another configuration:%s", path.c_str(), diff.c_str());
  }
  if ((sc.catke != 0) != m->catke)
    return fail(m, GB25_ERR_STATE, "%s: closure = CATKEVerticalDiffusivity() is %s in the file and %s in the model", path.c_str(), sc.catke ? "on" : "off", m->catke ? "on" : "off");
  if ((sc.coupled != 0) != m->coupled)
    return fail(m, GB25_ERR_STATE, "%s: the data-free coupling (prescribed atmosphere) is %s in the file and %s in the model", path.c_str(), sc.coupled ? "on" : "off", m->coupled ? "on" : "off");
  if (sc.nu != m->nu || sc.kappa != m->kappa || sc.bottom_drag != m->bottom_drag || sc.tracer_order != m->tracer_order ||
      memcmp(&sc.catke_par, &m->catke_par, sizeof sc.catke_par) != 0)
    return fail(m, GB25_ERR_STATE, "%s: another closure or forcing: nu %g / %g, kappa %g / %g, Cd %g / %g, tracer advection order %d / %d (file / model), or other CATKE parameters",
                path.c_str(), sc.nu, m->nu, sc.kappa, m->kappa, sc.bottom_drag, m->bottom_drag, (int)sc.tracer_order, m->tracer_order);
  {
    uint64_t g1 = 0, g2 = 0;
    grid_fingerprint(m, &g1, &g2);
    if (g1 != sc.grid_s1 || g2 != sc.grid_s2)
      return fail(m, GB25_ERR_STATE, "%s was written on another grid: the fingerprint of z faces, bottom height and metrics differs (set the grid and the bottom "
                  "of the run that wrote it before gb25_restore)", path.c_str());
  }
  // ---- 2. the set the file's switches give on THIS model's layout must be the file's table
  RestartSwitches sw;
  sw.catke = sc.catke != 0;
  sw.phy_stored = sc.phy_stored != 0;
  for (int q = 0; q < 4; q++) sw.top_flux[q] = (sc.top_flux_mask >> q) & 1;
  sw.ahead_ts = sc.ahead_valid != 0; sw.ahead_uv = sc.ahead_uv_valid != 0; sw.ahead_baro = sc.ahead_baro_valid != 0; sw.colsums = sc.colsum_valid != 0;
  if (gb25_status s = restart_prepare(m, sw, 0)) return s;
  RestartState& R = *m->restart;
  if (R.plan.members.size() != file.rows.size())
    return fail(m, GB25_ERR_STATE, "%s lists %zu members, this model's restart set has %zu", path.c_str(), file.rows.size(), R.plan.members.size());
  for (size_t q = 0; q < file.rows.size(); q++) {
    const RestartMember& mem = R.plan.members[q];
    const RestartFileRow& r = file.rows[q];
    if (mem.name != r.name || mem.field != r.field || mem.extra != r.extra || mem.bytes != r.bytes || mem.elem_bytes != r.elem_bytes ||
        mem.dims.nx != r.dims[0] || mem.dims.ny != r.dims[1] || mem.dims.nz != r.dims[2])
      return fail(m, GB25_ERR_STATE, "%s: member %zu is %s of %llu bytes, this model's restart set has %s of %llu bytes there", path.c_str(), q, r.name,
                  (unsigned long long)r.bytes, mem.name.c_str(), (unsigned long long)mem.bytes);
  }
  // ---- 3. upload and verify, piece by piece: the checksums of the arena against the file's, nothing of the model written yet
  if (gb25_status s = restart_build_segments(m, R, true, false, sw)) return s;
  if (gb25_status s = restart_size_buffers(m, R)) return s;
  if (gb25_status s = restart_grow_pinned(m, R.h_set, R.h_set_cap, (size_t)R.plan.arena_bytes)) return s;
  for (size_t q = 0; q < file.rows.size(); q++)
    if (!file.read_member(q, 0, file.rows[q].bytes, R.h_set + R.plan.members[q].offset))
      return fail(m, GB25_ERR_STATE, "%s: cannot read member %s", path.c_str(), file.rows[q].name);
  auto upload_piece = [&](size_t q) -> gb25_status {
    for (const RestartSpan& sp : R.pieces[q])
      HIPCHK(hipMemcpyAsync(R.d_arena + sp.arena_offset, R.h_set + R.plan.members[sp.member].offset + sp.begin, (size_t)sp.bytes,
                            hipMemcpyHostToDevice, m->stream));
    return GB25_OK;
  };
  for (size_t q = 0; q < R.pieces.size(); q++) {
    if (gb25_status s = upload_piece(q)) return s;
    if (gb25_status s = restart_launch_piece(m, R, q)) return s;
    const size_t nb = R.piece_block0[q + 1] - R.piece_block0[q];
    HIPCHK(hipMemcpyAsync(R.h_partials + 2 * R.piece_block0[q], R.d_partials, 2 * nb * sizeof(unsigned long long), hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
  }
  {
    std::vector<uint64_t> s1, s2;
    restart_sum_partials(R, s1, s2);
    for (size_t q = 0; q < file.rows.size(); q++)
      if (s1[q] != file.rows[q].s1 || s2[q] != file.rows[q].s2)
        return fail(m, GB25_ERR_STATE, "%s: checksum mismatch in member %s (s1 %016llx / %016llx, s2 %016llx / %016llx: read / recorded); the model is untouched",
                    path.c_str(), file.rows[q].name, (unsigned long long)s1[q], (unsigned long long)file.rows[q].s1, (unsigned long long)s2[q],
                    (unsigned long long)file.rows[q].s2);
  }
  // ---- 4. the recorded result-changing options (all or none: what was changed is put back when one is refused)
  int32_t before[kRestartOptionCount];
  for (int q = 0; q < kRestartOptionCount; q++) gb25_get_option(m, (gb25_option)kRestartOptions[q], &before[q]);
  for (int q = 0; q < kRestartOptionCount; q++) {
    if (before[q] == sc.options[q]) continue;
    if (gb25_status s = gb25_set_option(m, (gb25_option)kRestartOptions[q], sc.options[q])) {
      const std::string why = m->err;
      for (int b = 0; b < q; b++) gb25_set_option(m, (gb25_option)kRestartOptions[b], before[b]);
      return fail(m, s, "%s: the recorded option %s = %d is refused: %s", path.c_str(), restart_option_name(q), (int)sc.options[q], why.c_str());
    }
    if (info) info->options_changed |= 1u << q;
  }
  if (info) info->tracer_rows_differ = sc.tracer_rows_forced != m->tracer_rows_forced ? 1 : 0;
  // ---- 5. scatter: the second launch per piece (a bounded arena is uploaded again), then the scalar state and the validity
  // (the top flux arrays a restore fills, made only now that nothing can refuse the file any more; zeroed like gb25_set_top_flux's)
  for (int q = 0; q < 4; q++)
    if (sw.top_flux[q] && !m->d_top_flux[q]) {
      m->top_flux_elems[q] = (size_t)m->g.sx * m->g.sy_v;
      HIPCHK(m->mem.alloc(&m->d_top_flux[q], m->top_flux_elems[q] * sizeof(real), true));
    }
  if (gb25_status s = restart_build_segments(m, R, true, true, sw)) return s;
  if (gb25_status s = restart_size_buffers(m, R)) return s;   // (and the new table into the pinned copy the launches read)
  for (size_t q = 0; q < R.pieces.size(); q++) {
    if (R.pieces.size() > 1)
      if (gb25_status s = upload_piece(q)) return s;
    if (gb25_status s = restart_launch_piece(m, R, q)) return s;
    if (R.pieces.size() > 1) HIPCHK(hipStreamSynchronize(m->stream));
  }
  for (int q = 0; q < 4; q++) m->g.top_flux[q] = sw.top_flux[q] ? m->d_top_flux[q] : nullptr;
  m->time = sc.time;
  m->iteration = sc.iteration;
  m->last_dt = sc.last_dt;
  m->catke_prev_time = sc.catke_prev_time;
  m->prev_uv_src = 0;   // (CATKE's previous velocities are in their own fields now)
  m->baro_inflight = m->baro_adopted = false;
  m->strips_issued = false;
  m->route = StepRoute();
  m->implicit_key[0][0] = m->implicit_key[1][0] = -1.0;
  {
    Validity<real> made;
    made.ahead_valid = sc.ahead_valid != 0; made.ahead_uv_valid = sc.ahead_uv_valid != 0; made.ahead_baro_valid = sc.ahead_baro_valid != 0;
    made.colsum_valid = sc.colsum_valid != 0; made.halo_colsum_valid = sc.halo_colsum_valid != 0; made.tend_forkable = false; made.complete_fills_needed = sc.complete_fills_needed;
    made.ahead_dt = (real)sc.ahead_dt; made.ahead_chi = (real)sc.ahead_chi; made.ahead_uv_dt = (real)sc.ahead_uv_dt; made.ahead_uv_chi = (real)sc.ahead_uv_chi;
    m->valid.state_restored(made);
  }
  m->ahead_ts_folded = sc.ahead_ts_folded != 0 && m->valid.ahead_valid;
  m->ahead_eta_folded = sc.ahead_eta_folded != 0 && m->valid.ahead_baro_valid;
  if (sw.phy_stored) {
    m->phy_stale = false;
    if (gb25_status s = widen_phy(m)) return s;
  } else {
    m->phy_stale = true;
  }
  HIPCHK(hipStreamSynchronize(m->stream));
  if (info) {
    info->members = (int32_t)R.plan.members.size();
    info->pieces = (int32_t)R.pieces.size();
    info->bytes = (int64_t)R.plan.arena_bytes;
    info->phy_stale = m->phy_stale ? 1 : 0;
  }
  return GB25_OK;
}

}  // extern "C"
