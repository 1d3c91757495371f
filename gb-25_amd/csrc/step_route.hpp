// step_route.hpp -- in what form do u, v and w sit in memory, and which kernel applies the barotropic correction this step?  ONE member
// of gb25_model (`route`) holds every such flag; the buffers (corr[], uvc[], wbase) stay in the model.  Plain C++, no HIP.  The members
// are assigned here and nowhere else: callers say what HAPPENED.  The four routes, what each requires, who enters and who leaves each
// state: DESIGN.md, "Which kernel corrects u, v: the route of a step".
#pragma once
namespace {
enum class Corrector {
  Sweep,           // k_corrector / k_corrector_cells over u, v; w from k_compute_w
  SweepWFly,       // the sweep, which also leaves du, dv behind; w from k_w_bases + the WFLY instances of the tendency kernels
  InConsumers,     // nobody in memory: k_corrector_2d leaves du, dv and the LAZY instances add them ("lazy")
  ThroughTracers,  // the WCORR tracer instance adds du, dv and writes corrected arrays, which then become u, v (pointer exchange)
};
struct StepRoute {
  // u and v in memory lack du, dv = corr[0], corr[1], and every kernel that reads them adds them (only between the steps of one
  // composite call: gb25_loop applies them before it returns)
  bool uv_lazy = false;
  bool uv_corr_pending = false;   // this step's tracer kernel adds du, dv and writes the corrected velocities into uvc[]
  bool w_fly_now = false;         // this step's tendency kernels carry w up their chunks of levels from wbase: no k_compute_w launch
  bool w_stale = false;           // the field w in memory is the one of an earlier step (made again with the velocities: materialize_uv)
  bool corr_out = false;          // the sweep of this step also writes du, dv of the own columns into corr[] (for k_w_bases)
  bool step_lazy = false;         // this step keeps the corrector inside its consumers (a slab asks in every stage after stage 0)
  bool lazy_head_done = false;    // slab: ... and its du, dv and chunk bases of w are made already (stage 20 ran ahead of stage 2)
  // ---- what happens.  begin: the step's decision (time_step_impl; a slab: stage 0), taken once memory holds what the corrector expects
  void begin(Corrector c, bool w_fly) {
    step_lazy = c == Corrector::InConsumers;
    uv_corr_pending = c == Corrector::ThroughTracers;
    corr_out = c == Corrector::SweepWFly;
    w_fly_now = w_fly;
    lazy_head_done = false;
  }
  void head_done() { lazy_head_done = true; }
  void sweep_done() { corr_out = false; }                        // (a sweep outside a step leaves no increments)
  void correction_left_in_2d() { uv_lazy = true; }               // du, dv are made and nobody sweeps: memory now lacks them
  void tracer_kernel_wrote_corrected() { uv_corr_pending = false; }
  void w_carried_in_kernels() { w_stale = true; }                // the chunk bases are made: no kernel writes the field w this step
  // u += du, v += dv ran where memory lacked them, and with w_too the field w was made again: what every phase entry point, every
  // host read and every sweeping step expects
  void materialized(bool w_too) { uv_lazy = w_fly_now = false; if (w_too) w_stale = false; }
  // ---- predicates
  bool memory_lacks_correction() const { return uv_lazy; }
  bool kernels_add_correction() const { return uv_lazy; }        // (the LAZY instances, k_compute_w<false, true>)
  bool tracer_kernel_corrects() const { return uv_corr_pending; }
  bool kernels_carry_w() const { return w_fly_now; }
  bool sweep_leaves_increments() const { return corr_out; }
  bool w_field_stale() const { return w_stale; }
  bool corrector_in_consumers() const { return step_lazy; }
  bool head_is_done() const { return lazy_head_done; }
};
}  // namespace
