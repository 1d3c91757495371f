// validity.hpp -- may state made ahead of time, or cached, be trusted?  ONE member of gb25_model (`valid`) holds every such flag and
// key; the buffers (ahead[], ahead_uv[], colsum[] ...) stay in the model.  Plain C++, no HIP.  The members are assigned here and nowhere
// else: callers name the CAUSE.  Who calls what, and the guard a narrower reset relies on: DESIGN.md, "Validity of look-aheads and caches".
#pragma once
namespace {
template <class Real> struct Validity {
  // look-aheads: T, S of the next time level (tracer kernel); u, v, G.U, G.V and the column integrals (momentum kernel), each made
  // for one (dt, chi); eta, U, V and the filtered state of the next step (the sub-cycle run early, from the velocity look-ahead)
  bool ahead_valid = false, ahead_uv_valid = false, ahead_baro_valid = false;
  Real ahead_dt = 0, ahead_chi = 0, ahead_uv_dt = 0, ahead_uv_chi = 0;
  bool colsum_valid = false;        // colsum[] holds the column integrals of the u, v in memory
  bool halo_colsum_valid = false;   // slab: ... and its x-halo columns hold their owner's (packed with group 0)
  bool tend_forkable = false;       // the last tendency evaluation was a composite step's, tracers first: ev_tend covers both kernels
  int complete_fills_needed = 2;    // steps that still owe complete halo fills, one per buffer of each alternating pair (fold_fills)
  bool ptr_exposed = false;         // a prognostic field's address is out: the host may write behind our back, no look-ahead ever again
  void void_lookaheads() { ahead_valid = ahead_uv_valid = ahead_baro_valid = false; }   // an input of all of them changed
  void void_tracer_lookahead() { ahead_valid = false; }
  void void_velocity_lookaheads() { ahead_uv_valid = ahead_baro_valid = false; }
  void void_velocity_lookahead_alone() { ahead_uv_valid = false; }   // (the sub-cycle made from it stays: its adoption asks for both)
  void void_subcycle_lookahead() { ahead_baro_valid = false; }
  void void_colsums() { colsum_valid = false; }   // u, v changed under them, or their consumer used them up
  // the host wrote into one buffer of an alternating pair, or a switch changed who writes the halo cells of what a look-ahead makes
  void complete_fills_owed() { complete_fills_needed = 2; }
  void option_changes() { void_lookaheads(); tend_forkable = false; }
  void pointer_handed_out() { ptr_exposed = true; void_lookaheads(); }
  void grid_changes() { option_changes(); colsum_valid = halo_colsum_valid = false; complete_fills_owed(); }
  // gb25_restore wrote every array of the restart set behind every cache: nothing made ahead of time or summed earlier belongs to this state
  // -- except what the snapshot held as members and recorded as valid (`made`), which is this state's own; a model whose pointers
  // are out keeps no look-ahead, and the early fork of the tracer branch rests on an event of the old run (tend_forkable stays false)
  void state_restored(const Validity& made) {
    grid_changes();   // (everything void, complete fills owed) -- then, by name, what the snapshot recorded
    if (ptr_exposed) return;
    ahead_valid = made.ahead_valid; ahead_dt = made.ahead_dt; ahead_chi = made.ahead_chi;
    ahead_uv_valid = made.ahead_uv_valid; ahead_uv_dt = made.ahead_uv_dt; ahead_uv_chi = made.ahead_uv_chi;
    ahead_baro_valid = made.ahead_baro_valid;
    colsum_valid = made.colsum_valid;
    halo_colsum_valid = made.halo_colsum_valid;
    complete_fills_needed = made.complete_fills_needed;
  }
  // a tendency kernel is about to run; from_new_state: the momentum kernel STARTS an evaluation (the edge pass of a split one does not)
  void tendency_kernel_runs(bool from_new_state) { tend_forkable = false; if (from_new_state) void_velocity_lookaheads(); }
  // ---- causes that validate; what a step consumes; predicates
  void record_tracer_lookahead(bool made, Real dt, Real chi) { ahead_valid = made; ahead_dt = dt; ahead_chi = chi; }
  void record_velocity_lookahead(Real dt, Real chi) { ahead_uv_valid = true; ahead_uv_dt = dt; ahead_uv_chi = chi; }
  void record_subcycle_lookahead() { ahead_baro_valid = true; }
  void record_colsums() { colsum_valid = true; }
  void halo_colsums_packed() { halo_colsum_valid = colsum_valid; }
  void tendencies_forkable() { tend_forkable = true; }
  bool take_tend_forkable() { const bool was = tend_forkable; tend_forkable = false; return was; }
  bool take_complete_fill() { return complete_fills_needed > 0 ? (complete_fills_needed -= 1, true) : false; }
  bool tracers_adoptable(Real dt, Real chi) const { return ahead_valid && dt == ahead_dt && chi == ahead_chi; }
  bool velocities_adoptable(Real dt, Real chi) const { return ahead_uv_valid && dt == ahead_uv_dt && chi == ahead_uv_chi; }
  // the velocity look-ahead exists and the sub-cycle may run from it (the option SUBCYCLE_LOOKAHEAD is the caller's)
  bool velocities_ready(int subcycle_lookahead) const { return ahead_uv_valid && subcycle_lookahead && !ptr_exposed; }
};
}  // namespace
