// restart_plan.hpp -- what a checkpoint holds: the table of its members (whole parent arrays, halos included, bits as they are in
// memory), the scalar state that goes with them, and how the set passes through a bounded arena in pieces.  plan_restart() is the
// ONLY place the set is decided; restart_host.hpp packs, writes, reads and scatters what it lists.  Plain C++, no HIP, no gb25_model:
// a host compiler can include this file alone (tests/test_restart_plan.py).  In prose: DESIGN.md, "Checkpoint and restart".
#pragma once
#include "model_layout.hpp"

#include <cstdint>

namespace {

// a member that is no gb25_field: the top flux boundary conditions of u, v, T, S (2-D, rows of the field they belong to)
// ... and what the tendency kernels of the last step made ahead of time for the next one (the look-aheads: T, S; u, v, G.U, G.V,
// the column integrals and the partial sums; eta, U, V and the filtered state) and the column integrals of the u, v in memory.
// They are members while they are valid: a restored model then takes the very route the run that went on takes -- the steps that
// keep the corrector in its consumers and carry w in the tendency kernels start from adopted look-aheads, and their w differs from
// the stand-alone one in the last bits.
enum RestartExtra {
  RESTART_NO_EXTRA = -1, RESTART_TOP_FLUX_U = 0, RESTART_TOP_FLUX_V, RESTART_TOP_FLUX_T, RESTART_TOP_FLUX_S,
  RESTART_AHEAD_T, RESTART_AHEAD_S, RESTART_AHEAD_U, RESTART_AHEAD_V, RESTART_AHEAD_GU, RESTART_AHEAD_GV, RESTART_AHEAD_COLSUM_U,
  RESTART_AHEAD_COLSUM_V, RESTART_AHEAD_PARTIALS, RESTART_AHEAD_ETA, RESTART_AHEAD_BT_U, RESTART_AHEAD_BT_V, RESTART_AHEAD_ETA_BAR,
  RESTART_AHEAD_U_BAR, RESTART_AHEAD_V_BAR, RESTART_COLSUM_U, RESTART_COLSUM_V, RESTART_EXTRA_COUNT
};

// the switches of a model that decide the set (restart_host.hpp reads them off the model; a restore reads them off the file)
struct RestartSwitches {
  bool catke = false;        // closure = CATKEVerticalDiffusivity(): e, its tendencies, the diffusivity fields, the previous velocities
  bool phy_stored = false;   // pHY' is in memory (not only its differences): a member; else the restored model marks it stale
  bool top_flux[4] = {false, false, false, false};   // a top flux array of u, v, T, S is in use (set by the host, or by the coupling)
  bool ahead_ts = false, ahead_uv = false, ahead_baro = false;   // the look-ahead is valid (validity.hpp)
  bool colsums = false;                                          // the column integrals of u, v are
};

struct RestartMember {
  std::string name;
  int field = -1;                  // gb25_field, or -1 ...
  int extra = RESTART_NO_EXTRA;    // ... and then which extra array
  Dims dims{0, 0, 0};              // parent dims
  int elem_bytes = 0;
  uint64_t offset = 0, bytes = 0;  // 16-byte-aligned offset in the arena
  uint64_t elems() const { return bytes / (uint64_t)elem_bytes; }
};

// the options that change results: a restore applies the recorded values (gb25_option ids)
constexpr int kRestartOptions[] = {GB25_OPT_KERNELS, GB25_OPT_PRESSURE_PRECISION, GB25_OPT_MOMENTUM_CHUNK_LEVELS, GB25_OPT_TRACER_CHUNK_LEVELS,
                                   GB25_OPT_W_ON_THE_FLY, GB25_OPT_SUBSTEP_ORDER, GB25_OPT_FOLD_PIVOT_SLAVED, GB25_OPT_CATKE_STALE_E_HALOS};
constexpr int kRestartOptionCount = sizeof kRestartOptions / sizeof kRestartOptions[0];
inline const char* restart_option_name(int q) {
  static const char* const names[] = {"KERNELS", "PRESSURE_PRECISION", "MOMENTUM_CHUNK_LEVELS", "TRACER_CHUNK_LEVELS",
                                      "W_ON_THE_FLY", "SUBSTEP_ORDER", "FOLD_PIVOT_SLAVED", "CATKE_STALE_E_HALOS"};
  return q >= 0 && q < kRestartOptionCount ? names[q] : "?";
}

// The scalar state, stored as these bytes (a file is read by the library that wrote it, or by one built alike: real_bytes and
// config_bytes come first after the clock and are checked before anything else is believed).
struct RestartScalars {
  double time = 0, last_dt = 0;
  int64_t iteration = 0;
  int32_t real_bytes = 0, config_bytes = 0, scalars_bytes = 0;
  int32_t next_step_is_euler = 0;   // nothing has been stepped yet: gb25_first_time_step is still to come
  double dt_config = 0, chi = 0, catke_prev_time = 0;
  double nu = 0, kappa = 0, bottom_drag = 0;
  int32_t catke = 0, coupled = 0, tracer_order = 5, tracer_rows_forced = 0;
  int32_t phy_stored = 0, top_flux_mask = 0;
  int32_t options[kRestartOptionCount] = {0};
  // the validity of what was made ahead of time (validity.hpp) and who wrote which halo cells, as they were at the snapshot
  int32_t ahead_valid = 0, ahead_uv_valid = 0, ahead_baro_valid = 0, colsum_valid = 0, halo_colsum_valid = 0, tend_forkable = 0, complete_fills_needed = 0;
  int32_t ahead_ts_folded = 0, ahead_eta_folded = 0, reserved = 0;   // (no padding in front of the doubles: the block is written as bytes)
  double ahead_dt = 0, ahead_chi = 0, ahead_uv_dt = 0, ahead_uv_chi = 0;
  uint64_t grid_s1 = 0, grid_s2 = 0;   // fingerprint of z faces, bottom and metrics (restart_host.hpp: grid_fingerprint)
  gb25_config cfg{};
  gb25_catke_parameters catke_par{};
};

struct RestartPlan {
  gb25_status status = GB25_OK;
  std::string refusal;
  std::vector<RestartMember> members;
  uint64_t arena_bytes = 0;   // the whole set, every member at its offset
};

inline uint64_t restart_align16(uint64_t b) { return (b + 15) & ~(uint64_t)15; }

inline const char* restart_field_name(int id) {
  static const char* const names[GB25_FIELD_COUNT] = {
      "u", "v", "w", "T", "S", "pHY", "Gn.u", "Gn.v", "Gn.T", "Gn.S", "Gm.u", "Gm.v", "Gm.T", "Gm.S", "eta", "U", "V",
      "eta_bar", "U_bar", "V_bar", "Gn.U", "Gn.V", "e", "Gn.e", "Gm.e", "kappa_u", "kappa_c", "kappa_e", "Le", "Jb", "previous_u", "previous_v"};
  return names[id];
}

// Every array a step reads and a step wrote, in the order of the gb25_field enum, then the extras.  Scratch a step rewrites
// before it reads it (the ping-pong partners, the pressure differences, CATKE's N^2 and e*, du, dv and the chunk bases of w) is not
// state; a look-ahead or a column sum that is not valid at the snapshot is no member, and the restored model makes it anew.
inline RestartPlan plan_restart(const ModelLayout& L, const RestartSwitches& sw, int real_bytes) {
  RestartPlan p;
  auto add = [&](const std::string& name, int field, int extra, Dims d) {
    RestartMember m;
    m.name = name; m.field = field; m.extra = extra; m.dims = d; m.elem_bytes = real_bytes;
    m.bytes = (uint64_t)d.elems() * (uint64_t)real_bytes;
    m.offset = p.arena_bytes;
    p.arena_bytes = restart_align16(p.arena_bytes + m.bytes);
    p.members.push_back(m);
  };
  for (int id = 0; id < GB25_FIELD_COUNT; id++) {
    if (is_catke_field(id) && !sw.catke) continue;
    if (id == GB25_PHY && !sw.phy_stored) continue;
    add(restart_field_name(id), id, RESTART_NO_EXTRA, parent_dims(L, id));
  }
  for (int q = 0; q < 4; q++) {
    if (!sw.top_flux[q]) continue;
    const int of_field[4] = {GB25_U, GB25_V, GB25_T, GB25_S};
    const Dims d = parent_dims(L, of_field[q]);
    add(std::string("top_flux.") + restart_field_name(of_field[q]), -1, RESTART_TOP_FLUX_U + q, Dims{d.nx, d.ny, 1});
  }
  auto add_like = [&](const char* prefix, int extra, int like) { add(std::string(prefix) + restart_field_name(like), -1, extra, parent_dims(L, like)); };
  if (sw.ahead_ts)
    for (int q = 0; q < 2; q++) add_like("ahead.", RESTART_AHEAD_T + q, GB25_T + q);
  if (sw.ahead_uv) {
    for (int q = 0; q < 2; q++) add_like("ahead.", RESTART_AHEAD_U + q, GB25_U + q);
    for (int q = 0; q < 2; q++) add_like("ahead.", RESTART_AHEAD_GU + q, GB25_GN_BT_U + q);
    for (int q = 0; q < 2; q++) add_like("ahead.colsum.", RESTART_AHEAD_COLSUM_U + q, GB25_BT_U + q);
    add("ahead.partials", -1, RESTART_AHEAD_PARTIALS, Dims{(int)(4 * chunk_columns(L)), 1, 1});   // (k_ab2_velocities_finish's partial sums)
  }
  if (sw.ahead_baro) {
    for (int q = 0; q < 3; q++) add_like("ahead.", RESTART_AHEAD_ETA + q, GB25_ETA + q);
    for (int q = 0; q < 3; q++) add_like("ahead.", RESTART_AHEAD_ETA_BAR + q, GB25_ETA_BAR + q);
  }
  if (sw.colsums)
    for (int q = 0; q < 2; q++) add_like("colsum.", RESTART_COLSUM_U + q, GB25_BT_U + q);
  return p;
}

// A part of a member that passes through the arena in one piece: `bytes` bytes from byte `begin` of member `member`, at
// `arena_offset` of the (bounded) arena.  begin and arena_offset are multiples of 16.
struct RestartSpan {
  int member;
  uint64_t begin, bytes, arena_offset;
};
// The set in pieces of at most `cap` bytes of arena (cap = 0: one piece, the spans at the members' own offsets).  A member larger
// than what is left of a piece is split on a 16-byte boundary.  Every byte of every member is in exactly one span, in order.
inline std::vector<std::vector<RestartSpan>> restart_pieces(const RestartPlan& p, uint64_t cap) {
  std::vector<std::vector<RestartSpan>> pieces(1);
  if (cap == 0 || cap >= p.arena_bytes) {
    for (size_t q = 0; q < p.members.size(); q++) pieces[0].push_back({(int)q, 0, p.members[q].bytes, p.members[q].offset});
    return pieces;
  }
  cap = std::max<uint64_t>(16, cap & ~(uint64_t)15);
  uint64_t used = 0;
  for (size_t q = 0; q < p.members.size(); q++) {
    uint64_t begin = 0;
    const uint64_t bytes = p.members[q].bytes;
    while (begin < bytes) {
      if (used == cap) { pieces.emplace_back(); used = 0; }
      const uint64_t take = std::min(bytes - begin, cap - used);   // (cap - used is a multiple of 16: so is every begin)
      pieces.back().push_back({(int)q, begin, take, used});
      begin += take;
      used = std::min(cap, restart_align16(used + take));
    }
  }
  return pieces;
}
inline uint64_t restart_piece_bytes(const std::vector<RestartSpan>& piece) {
  return piece.empty() ? 0 : restart_align16(piece.back().arena_offset + piece.back().bytes);
}

}  // namespace
