// gb25_api.hip -- host side of libgb25hip.so: the C ABI declared in include/gb25.h.
//
// Owns the device state of one model (one x-slab on one GPU), builds the grid metrics,
// sequences the kernels of kernels.hpp in the reference's phase order
// (GB-25 src/precompile.jl:31-42) and exposes the per-phase entry points.
// There is no CPU fallback: without a HIP device gb25_create fails with GB25_ERR_NO_DEVICE.
#include "../../include/gb25.h"
#include <dlfcn.h>
#include "kernels.hpp"
#include "tendency_kernels.hpp"
#include "diagnostics_kernels.hpp"
#include "averages_kernels.hpp"
#include "class_kernels.hpp"
#include "particle_kernels.hpp"
#include "passive_kernels.hpp"
#include "spectrum_kernels.hpp"
#include "surface_kernels.hpp"
#include "stability_kernels.hpp"
#include "kinematics_kernels.hpp"
#include "zonal_eddy_kernels.hpp"
#include "block_kernels.hpp"
#include "filter_kernels.hpp"
#include "region_kernels.hpp"
#include "restart_kernels.hpp"
#include "diagnostics_state.hpp"
#include "validity.hpp"
#include "step_route.hpp"
#include "subcycle_plan.hpp"
#include "model_layout.hpp"
#include "launch_plan.hpp"
#include "tendency_plan.hpp"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <array>
#include <chrono>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <atomic>
#include <vector>

using namespace gb25;

namespace {

constexpr int PAD = 2;  // metric tables extend 2 entries beyond the halo

struct Field {
  real* d = nullptr;
  int nx = 0, ny = 0, nz = 0;  // parent dims
  size_t elems() const { return (size_t)nx * ny * nz; }
};

struct EventPair {
  hipEvent_t a, b;
};

// Every block of device memory a model allocates, remembered where it is made and freed by gb25_destroy in one loop: whichever
// member holds a pointer by then (the look-aheads exchange them) and however many Fields share a block.  A block is remembered
// before it is zeroed, so a failing hipMemset loses nothing.  (DiagState frees in mid-life and keeps its own memory.)
// The zeros are IN the block when zeroed() returns: hipMemset of device memory goes to the null stream and returns before the device
// has run it, and the model's streams are non-blocking, so nothing else orders a kernel launched next behind it -- a block allocated
// in mid-run (the corrected velocities of a step through the tracer kernel) was zeroed AFTER its first kernels had written it
// whenever the device was busy enough ("Reproducibility of a step").
inline hipError_t zeroed(void* d, size_t bytes) {
  const hipError_t e = hipMemset(d, 0, bytes);
  return e != hipSuccess ? e : hipStreamSynchronize(nullptr);
}
struct DeviceBlocks {
  std::vector<void*> blocks;
  template <class T>
  hipError_t alloc(T** p, size_t bytes, bool zero = false) {
    void* d = nullptr;
    const hipError_t e = hipMalloc(&d, bytes);
    if (e != hipSuccess) return e;
    blocks.push_back(d);
    *p = static_cast<T*>(d);
    return zero ? zeroed(d, bytes) : hipSuccess;
  }
  template <class T>
  void release(T*& p) {   // one block before the end (a field of the prescribed atmosphere that is taken away again)
    blocks.erase(std::remove(blocks.begin(), blocks.end(), static_cast<void*>(p)), blocks.end());
    (void)hipFree(p);
    p = nullptr;
  }
  void release_all() {
    for (void* d : blocks) (void)hipFree(d);
    blocks.clear();
  }
};

}  // namespace

struct gb25_model {
  gb25_config cfg;
  // What plan_layout (model_layout.hpp) decided at creation, never changed afterwards: the argument of parent_dims and its kin.  The
  // members below that carry a name of the layout (Nx .. yn_open, slab, Ns, dtau_frac, weights, W, Wy, Wys, tracer_rows_forced) are
  // copies of it, made by adopt_layout and nowhere else; so are the starting values of the options it has a default for.
  ModelLayout layout;
  int Nx = 0, Ny = 0;  // local slab width and rows
  int Rx = 1, Ry = 1, rx = 0, ry = 0, j0 = 0;
  bool ys_open = false, yn_open = false;
  Grid g;
  Field f[GB25_FIELD_COUNT];
  Field pp[3];                   // ping-pong partners of eta, U, V
  Field dpx, dpy;                // p'(i)-p'(i-1), p'(j)-p'(j-1), differenced in fp64 by k_compute_p, stored fp32
  Field colsum[2];               // column integrals of u, v after the AB2 update (consumed by the corrector)
  // The look-aheads' buffers, adopted by pointer exchange; whether each may be trusted: `valid` (validity.hpp).  T, S of the next time
  // level, written by the tracer tendency kernel (Ab2Ahead) ...
  Field ahead[2];
  // ... u, v, G.U, G.V, the corrector's column integrals and the partial sums for k_ab2_velocities_finish, by the momentum kernel (UvAhead) ...
  Field ahead_uv[2], ahead_G[2], ahead_colsum[2];
  real* uv_partials = nullptr;
  // ... and the split-explicit sub-cycle of the next step runs from those into partners of eta, U, V and of the filtered state
  Field pp2[3];                      // second scratch set: the sub-cycle never writes the arrays it starts from
  Field ahead_eta[3], ahead_bar[3];  // partners of eta, U, V and of eta_bar, U_bar, V_bar
  real* bars_ahead = nullptr;        // (the three partners of the averages are one allocation, like `bars`)
  Validity<real> valid;
  // pHY' is a diagnostic: inside a composite step only its differences are stored (4 of the kernel's 20 B/cell
  // saved) and the field is recomputed when the host asks for it; pinned to "always stored" once its pointer is out
  bool phy_stale = false;
  int phy_pinned = 0;                // option STORE_PRESSURE (0 or 1, as every option flag below)
  bool baro_inflight = false;        // a look-ahead sub-cycle is on the side stream and nobody has waited for it yet
  bool baro_adopted = false;         // staged path: stage 0 of this step adopted the sub-cycle look-ahead
  int baro_ahead = 1;                // option SUBCYCLE_LOOKAHEAD = 0: sub-cycle inside the step, on the critical path
  hipEvent_t ev_baro = nullptr, ev_mom = nullptr;
  int fill_fused = 1;                // y, z and periodic-x fills of a single slab in one launch (option FILL_FUSED = 0: two)
  int ab2_ahead = 1;                 // option AB2_LOOKAHEAD: 0 = stand-alone AB2 kernels, 1 = both look-aheads, 2 = tracers only
  real* bars = nullptr;         // contiguous etabar | Ubar | Vbar
  DeviceBlocks mem;             // owner of every device allocation below (not of DiagState's, not of the exchange context's)
  std::vector<double> h_metric[11];
  // orthogonal curvilinear grid (grid_type >= 2): the 14 horizontal metrics by location, fp64, parent layout of a (c,f)
  // field (gb25_get_metric2); cell-centre coordinates in degrees for analytic bottoms
  std::vector<double> h_curv[GB25_M2_COUNT];
  // The HOST's grid (gb25_set_curvilinear_grid, gb25_set_vertical_faces, gb25_set_bottom_height): the 14 horizontal metrics
  // over the GLOBAL parent extent ((Nx_global + 2H) x (Ny + 2H + 1) doubles each, i fastest), the Nz + 1 vertical faces, the
  // bottom height at the global cell centres.  Empty: the built-in generators of cfg.grid_type.
  std::vector<double> host_curv[GB25_M2_COUNT];
  std::vector<double> host_zf, host_bottom;
  int metric_off_j = 0, metric_off_k = 0;
  // substepping
  int Ns = 0;
  double dtau_frac = 0;
  std::vector<double> weights;
  // work arrays of the sub-cycle: widened by W columns either side on a slab (wide halos, filled once per step), tall by Wy
  // rows beyond the pivot row on a folded grid (images of the rows south of it, filled once per step); a single folded
  // domain has W = 0
  int W = 0, Wy = 0, Wys = 0;        // (Wys: rows below row 0 -- the southern neighbour's, 2-D decomposition)
  real* tall_buf = nullptr;          // single folded domain: the buffer its image rows pass through (k_tall_rows)
  Field wide[2][3];  // [pingpong][eta,U,V]
  Field wideG[2];    // GU, GV
  Field wideBar[3];  // running averages on the wide domain
  // clock
  double time = 0, last_dt = 0;
  int64_t iteration = 0;
  // streams / timing
  hipStream_t own_stream = nullptr, stream = nullptr, side_stream = nullptr;
  hipStream_t baro_stream = nullptr;   // the look-ahead sub-cycle of a single domain: a stream of its own, so that the
                                       // pressure of the next step (side stream) need not queue behind its tail
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  // Order of the two tendency kernels inside a composite step of a single domain (option TRACERS_FIRST, default 1): with the
  // tracer kernel first, T and S of the next time level (its look-ahead) exist before the momentum kernel runs, so the next
  // step's pressure -- forked off `ev_tend`, recorded right behind the momentum kernel's finish launch -- runs beside the
  // next step's sub-cycle (a chain of short LDS phases that leaves HBM idle) instead of beside w.  ev_ts: T, S of this step
  // and their halo cells are complete (side stream); the tracer kernel waits for it, the momentum kernel for ev_join.
  hipEvent_t ev_ts = nullptr, ev_tend = nullptr;
  hipEvent_t ev_strips = nullptr;    // slab: the pressure strips next to the x halos are done (exchange stream, stage 33)
  // the lists gb25_create and gb25_destroy loop over (baro_stream is created on demand: time_step_impl)
  std::array<hipEvent_t*, 7> events() { return {&ev_fork, &ev_join, &ev_baro, &ev_mom, &ev_ts, &ev_tend, &ev_strips}; }
  std::array<hipStream_t*, 3> streams() { return {&own_stream, &side_stream, &baro_stream}; }
  bool strips_issued = false;
  int early_strips = 1;              // option EARLY_STRIPS
  int tracers_first = 1;
  int two_streams = 1;              // option TWO_STREAMS = 0: strictly sequential phases on one stream
  bool profile = false;
  int profile_only = -1;             // >= 0: time this kernel id alone (keeps the event records out of the other launches)
  std::vector<EventPair> pending[GB25_K_COUNT];
  std::vector<EventPair> free_events;
  int64_t prof_count[GB25_K_COUNT] = {0};
  int64_t prof_seen[GB25_K_COUNT] = {0};
  double prof_ms[GB25_K_COUNT] = {0};
  std::string err;
  int baro_block = 5;                // substeps per barotropic launch (option SUBCYCLE_BLOCK = 1: one launch per substep; 5: 64 x 17 tiles,
                                     // four blocks per CU, every block of a 1440 x 720 launch resident at once: 0.16 ms for 21 substeps against 0.21 with 7)
  int kernel_gen = 2;                // 2: LDS / flux-sharing tendency kernels (tendency_kernels.hpp); 1: direct-stencil kernels
  int pressure_form = 0;             // option PRESSURE_FORM: 0 = the rule of plan_pressure; 1 tiles, 2 one row, 3 four rows per thread
  int spectrum_table_where = 0;      // option SPECTRUM_TABLE: 0 = the rule of spectrum_run (LDS where it fits); 1 global memory
  int pressure_bits = 64;            // option PRESSURE_PRECISION: 64 = fp64 EOS + integral (default); 32 = the float type's own
  // single periodic domain: the last writers of u, v (corrector), T, S (tracer look-ahead) and eta, U, V (last barotropic
  // launch) also write the halo cells the fills derive from them, and the fill launches leave the step.  Halo cells
  // deeper than one layer in y / z are static while stepping, so their x images only need the complete fills of the two
  // steps (one per buffer of each alternating pair) that follow a host write (valid.complete_fills_needed).
  int n_cu = 256;                    // compute units of the device
  int fold_fills = 1;
  bool composite = false;            // inside gb25_time_step / gb25_loop (the phase entry points leave halos alone, as the
                                     // reference's phases do: there the producers do not fold)
  bool ahead_ts_folded = false, ahead_eta_folded = false;
  int split_tendencies = 1;          // slab of a decomposition: interior tile columns before the x-halo bundle has arrived
  int baro_whole = 1;                // narrow slab: the whole sub-cycle in one launch (option SUBCYCLE_WHOLE)
  int sub_priority = 0;              // slab: the stream of the look-ahead's substeps is a high-priority one (read when the exchange context is built)
  // immersed boundary (GridFittedBottom): first active level per column on the columns [-kb_E, Nx + kb_E) x [0, Ny)
  // (host), the folded tables of device_common.hpp (device), the depths of the wide barotropic arrays of a slab
  int immersed = 0;                  // some cell is immersed: the IMM kernel variants run
  int kb_E = 0, kb_Ey = 0;           // (kbot: pitch Nx + 2 kb_E, row of local row j: j + kb_Ey)
  std::vector<int> kbot;
  unsigned* d_ord[4] = {nullptr, nullptr, nullptr, nullptr};
  real* d_H[4] = {nullptr, nullptr, nullptr, nullptr};   // Hfc, Hcf, rHfc, rHcf (parent layout of a (c,f) field)
  real* d_wideH[2] = {nullptr, nullptr};                 // Hfc, Hcf on the wide barotropic layout of a slab
  // curvilinear slab: dyfc, dxcf, 1/azcc, 1/dxfc, 1/dycf on the wide barotropic layout, and (zipper fold) the metrics of
  // the cells row Ny-1 mirrors onto, by own wide column (CurvBaro::mir, kernels.hpp)
  real* d_wideM[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  real* d_top_flux[4] = {nullptr, nullptr, nullptr, nullptr};   // FluxBoundaryCondition at the top of u, v, T, S
  // PrescribedAtmosphere at the cell centres (data-free forcing); all seven set: the composites compute the
  // atmosphere-ocean fluxes after every step.  d_tau: the stress components at the centres.
  double* d_atm[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  double* d_tau[2] = {nullptr, nullptr};
  bool coupled = false;
  int tracer_order = 5;              // tracer_advection = WENO(order = 5 | 7)
  double bottom_drag = 0.0;          // quadratic bottom drag coefficient (0: none); the two flux arrays behind Grid.bottom_flux
  real* d_bottom_flux[2] = {nullptr, nullptr};
  // Which kernel corrects u, v this step, and in what form u, v and w sit in memory meanwhile (step_route.hpp; chosen once per step
  // by choose_corrector).  corr: du, dv of the current step as 2-D fields (k_corrector_2d, or a by-product of the sweep).
  StepRoute route;
  Field corr[2];
  int lazy_corrector = 1;            // option LAZY_CORRECTOR
  // ... and with it w ON THE FLY (option W_ON_THE_FLY): in those steps the tendency kernels carry w up their chunks of levels
  // from the divergence of the transports they hold; no k_compute_w launch, no w traffic.  wbase: w at the first level of every
  // chunk (k_w_bases).  Results agree with the stand-alone w to round-off, not to the last bit.
  real* wbase = nullptr;
  int w_fly = 1;
  // The corrector through the tracer kernel (round 4; grids with a bottom / curvilinear / folded, single domain): du, dv as 2-D
  // fields; the tracer kernel -- first in the step, and every u, v is some cell's west / south face -- adds them as it loads and
  // writes the corrected velocities into this second pair of arrays, which then BECOME u, v (pointer exchange) and get their halo
  // cells from the ordinary fill; the momentum kernel reads corrected velocities like any other.  No sweep over u and v.
  Field uvc[2];
  // levels a block of the momentum / tracer tendency kernel marches through (options MOMENTUM_CHUNK_LEVELS,
  // TRACER_CHUNK_LEVELS): fewer, longer chunks amortise the start-up of the vertical windows, more chunks fill the chip.
  // The momentum chunking is also the association of every column integral of u, v (all their producers share it).
  int mom_chunk_levels = 12, trc_chunk_levels = 12;
  // rows per lane of the tracer tendency kernel (tracer_rows): 0 = the rule decides; 1, 2 = GB25_TRACER_ROWS in the environment of
  // gb25_create forced it (the A/B switch of a form with the same bits; not an option: the option table is pinned)
  int tracer_rows_forced = 0;
  // closure = VerticalScalarDiffusivity(VerticallyImplicitTimeDiscretization(), kappa, nu); both zero: closure = nothing
  double nu = 0, kappa = 0;
  bool catke = false;                // closure = CATKEVerticalDiffusivity(): the fields GB25_E .. GB25_JB exist
  Field catke_b, catke_scratch;      // N^2 on the faces; the unused half of the two-wide tracer kernel's output
  gb25_catke_parameters catke_par;   // (gb25_default_catke_parameters at creation)
  Field catke_src;                   // 2-D: the top boundary condition of e (surface TKE flux / dz of the top cell)
  real* catke_e_star = nullptr;   // where the last k_catke_tke_step left e* (e, or catke_scratch)
  bool implicit_lds_raised[2] = {false, false};   // k_implicit_vertical's dynamic-LDS attribute (Nz > 128), likewise
  bool whole_attr_set[4] = {false, false, false, false};   // k_barotropic_whole's dynamic-LDS attribute, per instance (SubcyclePlan::instance()), on THIS model's device
  int comm_timeout_s = 180;          // option COMM_TIMEOUT_SECONDS
  int roctx_ranges = 1;              // option ROCTX_RANGES
  int substep_order = 0;             // option SUBSTEP_ORDER
  double catke_prev_time = 0;        // diffusivity_fields.previous_compute_time
  // where diffusivity_fields.previous_velocities live (single domain: no copies in the steady state).  0: in their fields
  // (GB25_PREV_U/V).  1: they ARE the current u, v (compute_diffusivities! just ended: u- <- u is pending).  2: in the
  // look-ahead's partner buffers -- the AB2 step that followed adopted the look-ahead by exchanging pointers, and the buffers
  // it left hold u, v as they were at the last compute_diffusivities!, halos included.  materialize_prev_uv brings them home.
  int prev_uv_src = 0;
  int catke_stale_e_halos = 0;       // option CATKE_STALE_E_HALOS
  Field catke_gam[2];                // Nz > 64: the elimination factors of the streamed implicit solve
  real* d_implicit[2] = {nullptr, nullptr};   // elimination tables of the implicit solve for (u, v) and (T, S): lo | 1/beta | gamma
  double implicit_key[2][2] = {{0, 0}, {0, 0}};   // the (dt, K) they were built for
  bool slab = false;                 // x halos come from a neighbour (nranks > 1, or the self-ring of slab_mode = 1)
  struct SlabGroup* group = nullptr; // exchange context (transport, buffers, comm stream) once gb25_comm_init_* was called
  int group_index = 0;               // this slab's position in group->slabs
  int fold_flip = 0;                 // folded slab: which of the two widened state sets the next substep reads
  // the read-only diagnostics' buffers, tables and bookkeeping (diagnostics_state.hpp: who makes and who frees each); prof_redirect
  // >= 0: every timed launch is filed under that kernel id instead of its own (the pressure recomputed for the statistics of
  // a stale pHY' is a diagnostic)
  DiagState diag;
  int prof_redirect = -1;
  // checkpoint and restart: the arena, the pinned host buffer, the copy stream (restart_host.hpp; made by the first snapshot or
  // restore, freed by gb25_checkpoint_release and gb25_destroy)
  struct RestartState* restart = nullptr;
  size_t top_flux_elems[4] = {0, 0, 0, 0};   // (what each d_top_flux was allocated with)
  uint64_t grid_print[2] = {0, 0};           // the grid fingerprint of a checkpoint, made once per grid (restart_host.hpp)
  bool grid_print_valid = false;
  // passive tracers carried beside the run (passive_host.hpp): the sets begun on this model and not ended yet.  Each set owns its
  // memory; gb25_destroy frees the ones still here
  std::vector<struct gb25_tracers*> tracer_sets;
};

namespace {

gb25_status fail(gb25_model* m, gb25_status s, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (m) m->err = buf;
  return s;
}

#define HIPCHK(call)                                                                                  \
  do {                                                                                                \
    hipError_t e_ = (call);                                                                           \
    if (e_ != hipSuccess)                                                                             \
      return fail(m, GB25_ERR_HIP, "%s:%d: %s failed: %s", __FILE__, __LINE__, #call, hipGetErrorString(e_)); \
  } while (0)
#define CHECK_MODEL(m) \
  if (!(m)) return GB25_ERR_INVALID_ARGUMENT
#define LAUNCHCHK() HIPCHK(hipGetLastError())

// (is_v_shaped, is_2d, is_catke_field: model_layout.hpp, over its table of field shapes)
inline bool is_folded(const gb25_model* m) { return m->layout.north_fold; }
inline bool has_north_wall(const gb25_model* m) { return m->layout.north_wall; }
// First wet level (= number of immersed cells) of LOCAL column (i, j) on the host; 0 without a bottom table.  Rows beyond a global
// wall read the wall's row, rows beyond the rank read a neighbour's as far as the table holds them (kb_Ey).  The clamp of i and
// the cap at Nz are there for safety and change no result: build_bottom stores the columns [-E, Nx + E) with E = kb_E >=
// halo + 4, and the callers ask for i in [-1, Nx) (gb25_get_bottom_info, moments_tables: a cell and its western neighbour), [0, Nx)
// (gb25_particles_set) and [-halo, Nx + halo) (particles_tables); every row the two row clamps can land on lies inside the global
// grid, where build_bottom has stored level(), a count of at most Nz cells (its filler 255 stays in the rows beyond the walls,
// which are never read here).
inline int first_wet_level(const gb25_model* m, int i, int j) {
  if (m->kbot.empty()) return 0;
  const int E = m->kb_E, Ey = m->kb_Ey, ksx = m->Nx + 2 * E;
  const int il = std::min(std::max(i, -E), m->Nx + E - 1);
  const int jl = std::min(std::max(j + m->j0, 0), m->cfg.Ny - 1) - m->j0;
  const int kb = m->kbot[(size_t)(il + E) + (size_t)ksx * (std::min(std::max(jl, -Ey), m->Ny + Ey - 1) + Ey)];
  return std::min(kb, (int)m->cfg.Nz);
}

// --- profiling helpers -----------------------------------------------------------------------
// Named ranges for a profiler's timeline, as the reference wraps its entry points in Reactant.Profiler.annotate("first_time_step" /
// "time_step" / "loop") (GB-25 src/timestepping_utils.jl:22,30,38): roctx ranges around the composites and around the issue of
// every phase of src/precompile.jl:31-42, so that a `rocprofv3 --kernel-trace --marker-trace` of gb25_loop shows which phase a
// kernel belongs to.  The marker library is resolved at run time (rocprofv3 preloads librocprofiler-sdk-roctx; the legacy
// libroctx64 serves the older tools); without one the ranges cost a null-pointer test.  Option ROCTX_RANGES = 0 turns them off.
struct RoctxApi {
  int (*push)(const char*) = nullptr;
  int (*pop)() = nullptr;
  RoctxApi() {
    for (const char* name : {"librocprofiler-sdk-roctx.so.1", "librocprofiler-sdk-roctx.so", "libroctx64.so.4", "libroctx64.so"}) {
      void* lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
      if (!lib) continue;
      push = (int (*)(const char*))dlsym(lib, "roctxRangePushA");
      pop = (int (*)())dlsym(lib, "roctxRangePop");
      if (push && pop) return;
      push = nullptr; pop = nullptr;
    }
  }
};
inline RoctxApi& roctx() {
  static RoctxApi api;
  return api;
}
struct Range {
  bool on;
  Range(const gb25_model* m, const char* name) : on(m->roctx_ranges && roctx().push != nullptr) {
    if (on) roctx().push(name);
  }
  ~Range() {
    if (on) roctx().pop();
  }
};
// the model's launches go to another stream while this lives (the side stream of a step, the streams of an exchange context);
// whichever way the scope is left, the model is back on the stream it had
struct OnStream {
  gb25_model* m;
  hipStream_t saved;
  OnStream(gb25_model* m_, hipStream_t st) : m(m_), saved(m_->stream) { m->stream = st; }
  ~OnStream() { m->stream = saved; }
};
// the phase a kernel timer belongs to (src/precompile.jl:31-42; ":" + what inside the phase)
inline const char* phase_name(int k) {
  switch (k) {
    case GB25_K_FILL_HALOS: return "tupled_fill_halo_regions";
    case GB25_K_COMPUTE_W: return "compute_auxiliaries:w";
    case GB25_K_COMPUTE_P: return "compute_auxiliaries:pHY";
    case GB25_K_CLOSURE: return "compute_auxiliaries:diffusivities";
    case GB25_K_GU: case GB25_K_GV: return "compute_tendencies:momentum";
    case GB25_K_TRACERS: return "compute_tendencies:tracers";
    case GB25_K_AB2_VELOCITIES: return "ab2_step:velocities";
    case GB25_K_AB2_TRACERS: return "ab2_step:tracers";
    case GB25_K_BAROTROPIC: return "ab2_step:free_surface";
    case GB25_K_IMPLICIT: return "ab2_step:implicit_step";
    case GB25_K_CORRECTOR: return "correct_velocities_and_cache_previous_tendencies";
    case GB25_K_FLUXES: return "compute_atmosphere_ocean_fluxes";
    case GB25_K_DIAGNOSTICS: return "diagnostics";
    default: return "gb25";
  }
}
struct Timed {
  gb25_model* m;
  int k;
  EventPair ev;
  bool on;
  Range range;
  Timed(gb25_model* m_, int k_) : m(m_), k(m_->prof_redirect >= 0 ? m_->prof_redirect : k_), on(m_->profile && (m_->profile_only < 0 || m_->profile_only == k)), range(m_, phase_name(k)) {
    // one kernel alone: every fourth launch is timed (the event records cost the step ~1.6 % when every launch carries them)
    if (on && m->profile_only == k && (m->prof_seen[k]++ & 3) != 0) on = false;
    if (!on) return;
    if (!m->free_events.empty()) {
      ev = m->free_events.back();
      m->free_events.pop_back();
    } else {
      hipEventCreate(&ev.a);
      hipEventCreate(&ev.b);
    }
    hipEventRecord(ev.a, m->stream);
  }
  void stop() {
    if (!on) return;
    hipEventRecord(ev.b, m->stream);
    m->pending[k].push_back(ev);
    on = false;
  }
  ~Timed() { stop(); }
};

void resolve_profile(gb25_model* m) {
  for (int k = 0; k < GB25_K_COUNT; k++) {
    for (auto& ev : m->pending[k]) {
      hipEventSynchronize(ev.b);
      float ms = 0;
      if (hipEventElapsedTime(&ms, ev.a, ev.b) == hipSuccess) {
        m->prof_ms[k] += ms;
        m->prof_count[k] += 1;
      }
      m->free_events.push_back(ev);
    }
    m->pending[k].clear();
  }
}

// --- grid ------------------------------------------------------------------------------------
// simple_latitude_longitude_grid (GB-25 src/model_utils.jl:56-65): regular lat-lon spacing,
// exponential_z_faces(Nz, depth, h) vertical faces, spherical-shell metrics.
gb25_status upload_table(gb25_model* m, const std::vector<double>& h, int off, const real** out) {
  std::vector<real> f(h.size());
  for (size_t a = 0; a < h.size(); a++) f[a] = (real)h[a];
  real* d = nullptr;
  HIPCHK(m->mem.alloc(&d, f.size() * sizeof(real)));
  HIPCHK(hipMemcpy(d, f.data(), f.size() * sizeof(real), hipMemcpyHostToDevice));
  *out = d + off;
  return GB25_OK;
}

gb25_status build_grid(gb25_model* m) {
  m->diag.invalidate_tables();   // (the diagnostics' own tables follow the grid: rebuilt by the next call that needs them)
  const gb25_config& c = m->cfg;
  const int H = c.halo, Ny = m->Ny, Nz = c.Nz;
  // (the row tables of a rank of a 2-D decomposition also cover the rows its sub-cycle is widened by)
  const int padj = PAD + (m->Ry > 1 ? c.substeps + 2 + H + 8 : 0);
  const int nj = Ny + 2 * H + 2 * padj + 2, nk = Nz + 2 * H + 2 * PAD + 2;
  const int offj = H + padj, offk = H + PAD;  // table index of 0-based logical index 0
  m->metric_off_j = offj;
  m->metric_off_k = offk;
  const double d2r = M_PI / 180.0;
  const double dlam = (c.lon_east - c.lon_west) / c.Nx, dphi = (c.lat_north - c.lat_south) / c.Ny, R = c.radius;
  std::vector<double>&phif = m->h_metric[GB25_M_PHIF], &phic = m->h_metric[GB25_M_PHIC],
  &dxc = m->h_metric[GB25_M_DXC], &dxf = m->h_metric[GB25_M_DXF], &azc = m->h_metric[GB25_M_AZC],
  &azf = m->h_metric[GB25_M_AZF], &fcor = m->h_metric[GB25_M_FCOR];
  phif.assign(nj, 0); phic.assign(nj, 0); dxc.assign(nj, 0); dxf.assign(nj, 0);
  azc.assign(nj, 0); azf.assign(nj, 0); fcor.assign(nj, 0);
  for (int a = 0; a < nj; a++) {
    int j = a - offj + m->j0;  // 0-based GLOBAL face / centre index
    phif[a] = c.lat_south + j * dphi;
    phic[a] = c.lat_south + (j + 0.5) * dphi;
  }
  for (int a = 0; a < nj; a++) {
    dxc[a] = R * std::cos(phic[a] * d2r) * dlam * d2r;
    dxf[a] = R * std::cos(phif[a] * d2r) * dlam * d2r;
    fcor[a] = 2.0 * c.Omega * std::sin(phif[a] * d2r);
    if (a + 1 < nj) azc[a] = R * R * dlam * d2r * (std::sin(phif[a + 1] * d2r) - std::sin(phif[a] * d2r));
    if (a > 0) azf[a] = R * R * dlam * d2r * (std::sin(phic[a] * d2r) - std::sin(phic[a - 1] * d2r));
  }
  // vertical faces: z_k ~ exp(k/h), k = 1..Nz+1, mapped to [0, -depth] and reversed (exponential_z_faces, src/model_utils.jl:
  // 56-62) -- or the host's own faces (gb25_set_vertical_faces)
  std::vector<double> zint(Nz + 1);
  const double h = c.zexp_h, e1 = std::exp(1.0 / h), eN = std::exp((Nz + 1.0) / h);
  for (int k = 1; k <= Nz + 1; k++) zint[Nz + 1 - k] = -c.depth * (std::exp(k / h) - e1) / (eN - e1);
  zint[Nz] = 0.0;
  if (!m->host_zf.empty()) zint = m->host_zf;
  // the faces are numbers of the model's float type (a Float32 host holds Float32 faces); centres and spacings derive from them
  for (double& z : zint) z = (double)(real)z;
  std::vector<double>&zf = m->h_metric[GB25_M_ZF], &zc = m->h_metric[GB25_M_ZC], &dzc = m->h_metric[GB25_M_DZC],
  &dzf = m->h_metric[GB25_M_DZF];
  zf.assign(nk + 1, 0); zc.assign(nk, 0); dzc.assign(nk, 0); dzf.assign(nk, 0);
  const double dlo = zint[1] - zint[0], dhi = zint[Nz] - zint[Nz - 1];
  for (int a = 0; a <= nk; a++) {
    int k = a - offk;  // 0-based face index
    zf[a] = k < 0 ? zint[0] + k * dlo : (k > Nz ? zint[Nz] + (k - Nz) * dhi : zint[k]);
  }
  for (int a = 0; a < nk; a++) zc[a] = 0.5 * (zf[a] + zf[a + 1]);
  for (int a = 0; a < nk; a++) {
    dzc[a] = zf[a + 1] - zf[a];
    dzf[a] = a > 0 ? zc[a] - zc[a - 1] : zc[1] - zc[0];
  }
  Grid& g = m->g;
  g.Nx = m->Nx; g.Ny = Ny; g.Nz = Nz; g.H = H;
  g.sx = m->Nx + 2 * H;
  g.sy_c = Ny + 2 * H; g.sy_v = Ny + 2 * H + 1;
  g.pl_c = g.sx * g.sy_c; g.pl_v = g.sx * g.sy_v;
  g.x_periodic = !m->slab;
  g.jws = -m->j0;
  g.jwn = c.grid_type >= GB25_GRID_TRIPOLAR ? (1 << 20) : c.Ny - m->j0;
  g.dy = (real)(R * dphi * d2r);
  g.g = (real)c.g; g.rho0 = (real)c.rho0; g.Lz = (real)(zint[Nz] - zint[0]);
  gb25_status s;
  if ((s = upload_table(m, dxc, offj, &g.dxc))) return s;
  if ((s = upload_table(m, dxf, offj, &g.dxf))) return s;
  if ((s = upload_table(m, azc, offj, &g.azc))) return s;
  if ((s = upload_table(m, azf, offj, &g.azf))) return s;
  if ((s = upload_table(m, fcor, offj, &g.fcor))) return s;
  if ((s = upload_table(m, phic, offj, &g.phic))) return s;
  {
    auto recip = [](const std::vector<double>& a) {
      std::vector<double> r(a.size());
      for (size_t q = 0; q < a.size(); q++) r[q] = a[q] != 0.0 ? 1.0 / a[q] : 0.0;
      return r;
    };
    if ((s = upload_table(m, recip(dxc), offj, &g.rdxc))) return s;
    if ((s = upload_table(m, recip(azc), offj, &g.razc))) return s;
    if ((s = upload_table(m, recip(azf), offj, &g.razf))) return s;
    if ((s = upload_table(m, recip(dzc), offk, &g.rdzc))) return s;
    if ((s = upload_table(m, recip(dzf), offk, &g.rdzf))) return s;
    g.rdy = (real)(1.0 / (R * dphi * d2r));
    g.rLz = (real)(1.0 / (zint[Nz] - zint[0]));
  }
  if ((s = upload_table(m, zc, offk, &g.zc))) return s;
  if ((s = upload_table(m, dzc, offk, &g.dzc))) return s;
  if ((s = upload_table(m, dzf, offk, &g.dzf))) return s;
  return GB25_OK;
}

// --- orthogonal curvilinear grids ---------------------------------------------------------------------------------
// TripolarGrid(arch; size, halo, z) (GB-25 src/model_utils.jl:134-137), restated as an analytic bipolar cap after Murray
// (1996): first pole at 70 E, both at 55 N, southern edge as configured, northern edge the fold line between the poles
// [UPSTREAM-UNVERIFIED: Oceananigans builds its cap numerically; topology, poles and fold agree, the interior coordinate
// lines of the cap need not].  South of 55 N the grid is the lat-lon grid.  In the polar stereographic plane the cap
// carries bipolar coordinates with the foci at the poles, chosen so that the rim keeps its longitudes and the meridian
// halfway between the poles its latitudes.  Metrics: great-circle distances between neighbouring nodes, spherical areas
// of the quadrilaterals they span.  oracle/gb25_oracle.c states the same construction; tests compare the two.
struct GNode { double x, y, z, lam, phi; };
GNode sphere_node(double lam, double phi) {
  const double d2r = M_PI / 180.0;
  phi = std::max(phi, -89.999);   // (halo rows of coarse grids beyond the south pole: never used)
  return {std::cos(phi * d2r) * std::cos(lam * d2r), std::cos(phi * d2r) * std::sin(lam * d2r), std::sin(phi * d2r), lam, phi};
}
// f(j) for every row j of [j_lo, j_hi) on the host's cores (rows in blocks of eight from a shared counter).  The grid and bottom
// tables of a curvilinear model are elliptic-function work per column -- 20 s on one core for config 5's 4320 x 2160 columns.
template <class F>
void parallel_rows(int j_lo, int j_hi, F f) {
  const unsigned hw = std::thread::hardware_concurrency();
  const int nt = (int)std::min<unsigned>(hw ? hw : 1u, 32u);
  if (j_hi - j_lo < 64 || nt <= 1) {
    for (int j = j_lo; j < j_hi; j++) f(j);
    return;
  }
  std::atomic<int> next{j_lo};
  std::vector<std::thread> th;
  for (int t = 0; t < nt; t++)
    th.emplace_back([&]() {
      for (;;) {
        const int j = next.fetch_add(8);
        if (j >= j_hi) break;
        for (int q = j; q < std::min(j + 8, j_hi); q++) f(q);
      }
    });
  for (auto& t : th) t.join();
}
GNode tripolar_node(double lamt, double phit) {
  const double d2r = M_PI / 180.0, lamP = 70.0, phiP = 55.0;
  if (phit > 90.0) {   // beyond the fold: the image point
    phit = 180.0 - phit;
    lamt = 2 * lamP - lamt;
  }
  if (phit <= phiP) return sphere_node(lamt, phit);
  const double rP = std::tan((90.0 - phiP) / 2 * d2r), rt = std::tan((90.0 - phit) / 2 * d2r) / rP;
  const double th = (lamt - lamP) * d2r, ct = std::cos(th), sth = std::sin(th), st = std::fabs(sth);
  const double sg = 2 * std::atan2(1.0, rt), D = 1.0 - std::cos(sg) * st;
  const double xw = ct / D, yw = (sth < 0 ? -1.0 : 1.0) * std::sin(sg) * st / D;
  const double rz = rP * std::sqrt(xw * xw + yw * yw);
  return sphere_node(lamP + std::atan2(yw, xw) / d2r, 90.0 - 2 * std::atan(rz) / d2r);
}
double gc_dist(const GNode& a, const GNode& b, double R) {
  const double cx = a.y * b.z - a.z * b.y, cy = a.z * b.x - a.x * b.z, cz = a.x * b.y - a.y * b.x;
  const double d = R * std::atan2(std::sqrt(cx * cx + cy * cy + cz * cz), a.x * b.x + a.y * b.y + a.z * b.z);
  return std::max(d, 100.0);   // the coordinate lines meet at the poles: keep the metrics finite there
}
double tri_area(const GNode& a, const GNode& b, const GNode& c) {
  const double t = a.x * (b.y * c.z - b.z * c.y) + a.y * (b.z * c.x - b.x * c.z) + a.z * (b.x * c.y - b.y * c.x);
  const double d = 1.0 + (a.x * b.x + a.y * b.y + a.z * b.z) + (b.x * c.x + b.y * c.y + b.z * c.z) + (c.x * a.x + c.y * a.y + c.z * a.z);
  return 2 * std::atan2(std::fabs(t), d);
}
double quad_area(const GNode& a, const GNode& b, const GNode& c, const GNode& d, double R) {
  return std::max(R * R * (tri_area(a, b, c) + tri_area(a, c, d)), 1e4);
}

// The 14 horizontal metrics (gb25_metric2 order) and the physical coordinates of the cell centre at GLOBAL column ig,
// row j (any integers: halo rows and columns are generated like interior ones).  grid_type 2: the lat-lon metrics; 3, 4: the
// tripolar grid, whose Ny rows of cell centres run from the southern edge to 90 degrees (Oceananigans' TripolarGrid:
// range(southernmost_latitude, 90, length = Ny); "the north pole is a Center point"), the y faces half a spacing south of them.
// `own` rows only (j <= Ny - 1 on the tripolar grid): curv_metrics_at maps the rows beyond the pivot row onto their images.
void curv_metrics_own(const gb25_model* m, int ig, int j, double out[GB25_M2_COUNT], double* lam_c, double* phi_c) {
  const gb25_config& c = m->cfg;
  const bool tri = c.grid_type >= GB25_GRID_TRIPOLAR;
  const double d2r = M_PI / 180.0, R = c.radius;
  const double lam0 = tri ? 70.0 : c.lon_west, dlam = (tri ? 360.0 : (c.lon_east - c.lon_west)) / c.Nx;
  const double phiN = tri ? 90.0 : c.lat_north, dphi = (phiN - c.lat_south) / (tri ? c.Ny - 1 : c.Ny);
  if (!m->host_curv[0].empty()) {
    // the host's arrays: halo columns as the host holds them (its periodic images), columns beyond them wrapped
    const int H = c.halo, gsx = c.Nx + 2 * H;
    const int col = (ig >= -H && ig < c.Nx + H) ? ig + H : ((ig % c.Nx) + c.Nx) % c.Nx + H;
    const size_t o = (size_t)col + (size_t)gsx * (size_t)(std::min(std::max(j, -H), c.Ny + H) + H);
    for (int q = 0; q < GB25_M2_COUNT; q++) out[q] = m->host_curv[q][o];
    if (lam_c) *lam_c = 0.0;   // (not among the metrics: an analytic bottom cannot be placed on a host grid -- gb25_set_bottom_height)
    if (phi_c) *phi_c = out[GB25_M2_PHICC];
    return;
  }
  if (!tri) {
    const int a = m->metric_off_j + j - m->j0;   // (the row tables are indexed by LOCAL row)
    out[GB25_M2_DXFC] = out[GB25_M2_DXCC] = m->h_metric[GB25_M_DXC][a];
    out[GB25_M2_DXCF] = out[GB25_M2_DXFF] = m->h_metric[GB25_M_DXF][a];
    out[GB25_M2_DYFC] = out[GB25_M2_DYCC] = out[GB25_M2_DYCF] = out[GB25_M2_DYFF] = R * dphi * d2r;
    out[GB25_M2_AZCC] = out[GB25_M2_AZFC] = m->h_metric[GB25_M_AZC][a];
    out[GB25_M2_AZCF] = out[GB25_M2_AZFF] = m->h_metric[GB25_M_AZF][a];
    out[GB25_M2_FFF] = m->h_metric[GB25_M_FCOR][a];
    out[GB25_M2_PHICC] = m->h_metric[GB25_M_PHIC][a];
    if (lam_c) *lam_c = c.lon_west + (ig + 0.5) * dlam;
    // (the row tables were rounded to the float type when they were uploaded: the same value here)
    if (phi_c) *phi_c = (double)(real)m->h_metric[GB25_M_PHIC][a];
    return;
  }
  // computational coordinates of the four node families around the 0-based (ig, j)
  const double lf = lam0 + ig * dlam, lc = lam0 + (ig + 0.5) * dlam;
  const double pc = c.lat_south + j * dphi, pf = pc - 0.5 * dphi;
  auto N = [](double l, double p) { return tripolar_node(l, p); };
  const GNode cc = N(lc, pc), fc = N(lf, pc), cf = N(lc, pf), ff = N(lf, pf);
  const GNode fc_e = N(lf + dlam, pc), ff_e = N(lf + dlam, pf), cc_w = N(lc - dlam, pc), cf_w = N(lc - dlam, pf);
  const GNode cf_n = N(lc, pf + dphi), ff_n = N(lf, pf + dphi), ff_ne = N(lf + dlam, pf + dphi);
  const GNode cc_s = N(lc, pc - dphi), fc_s = N(lf, pc - dphi), cc_sw = N(lc - dlam, pc - dphi);
  const GNode cf_nw = N(lc - dlam, pf + dphi), fc_se = N(lf + dlam, pc - dphi);
  out[GB25_M2_DXCC] = gc_dist(fc, fc_e, R);
  out[GB25_M2_DXFC] = gc_dist(cc_w, cc, R);
  out[GB25_M2_DXCF] = gc_dist(ff, ff_e, R);
  out[GB25_M2_DXFF] = gc_dist(cf_w, cf, R);
  out[GB25_M2_DYCC] = gc_dist(cf, cf_n, R);
  out[GB25_M2_DYFC] = gc_dist(ff, ff_n, R);
  out[GB25_M2_DYCF] = gc_dist(cc_s, cc, R);
  out[GB25_M2_DYFF] = gc_dist(fc_s, fc, R);
  out[GB25_M2_AZCC] = quad_area(ff, ff_e, ff_ne, ff_n, R);
  out[GB25_M2_AZFC] = quad_area(cf_w, cf, cf_n, cf_nw, R);
  out[GB25_M2_AZCF] = quad_area(fc_s, fc_se, fc_e, fc, R);
  out[GB25_M2_AZFF] = quad_area(cc_sw, cc_s, cc, cc_w, R);
  out[GB25_M2_FFF] = 2.0 * c.Omega * std::sin(ff.phi * d2r);
  out[GB25_M2_PHICC] = cc.phi;
  if (lam_c) *lam_c = cc.lam;
  if (phi_c) *phi_c = cc.phi;
}
// ... at any row: beyond the pivot row of a folded grid (j >= Ny) the metric of a location is the metric of its image --
// cell rows and y-face rows mirror about the centres of row Ny-1, x faces as ig -> (Nx - ig) mod Nx (kernels.hpp, k_fill_fold).
// The images are COPIES of interior numbers (a host-supplied grid is treated the same way), so a metric and its image agree
// to the last bit whatever generated them.
void curv_metrics_at(const gb25_model* m, int ig, int j, double out[GB25_M2_COUNT], double* lam_c, double* phi_c) {
  const gb25_config& c = m->cfg;
  if (c.grid_type < GB25_GRID_TRIPOLAR || j < c.Ny) {
    curv_metrics_own(m, ig, j, out, lam_c, phi_c);
    return;
  }
  const int iw = ((ig % c.Nx) + c.Nx) % c.Nx, icc = c.Nx - 1 - iw, ifc = iw == 0 ? 0 : c.Nx - iw;
  const int jc = 2 * (c.Ny - 1) - j, jf = 2 * c.Ny - 1 - j;
  double A[GB25_M2_COUNT], B[GB25_M2_COUNT], C[GB25_M2_COUNT], D[GB25_M2_COUNT];
  curv_metrics_own(m, icc, jc, A, lam_c, phi_c);   // (c,c)
  curv_metrics_own(m, ifc, jc, B, nullptr, nullptr);   // (f,c)
  curv_metrics_own(m, icc, jf, C, nullptr, nullptr);   // (c,f)
  curv_metrics_own(m, ifc, jf, D, nullptr, nullptr);   // (f,f)
  out[GB25_M2_DXCC] = A[GB25_M2_DXCC]; out[GB25_M2_DYCC] = A[GB25_M2_DYCC]; out[GB25_M2_AZCC] = A[GB25_M2_AZCC]; out[GB25_M2_PHICC] = A[GB25_M2_PHICC];
  out[GB25_M2_DXFC] = B[GB25_M2_DXFC]; out[GB25_M2_DYFC] = B[GB25_M2_DYFC]; out[GB25_M2_AZFC] = B[GB25_M2_AZFC];
  out[GB25_M2_DXCF] = C[GB25_M2_DXCF]; out[GB25_M2_DYCF] = C[GB25_M2_DYCF]; out[GB25_M2_AZCF] = C[GB25_M2_AZCF];
  out[GB25_M2_DXFF] = D[GB25_M2_DXFF]; out[GB25_M2_DYFF] = D[GB25_M2_DYFF]; out[GB25_M2_AZFF] = D[GB25_M2_AZFF]; out[GB25_M2_FFF] = D[GB25_M2_FFF];
}

// Fills m->h_curv (the local slab's columns, halo columns by their own global index) and uploads what the kernels read
// (device_common.hpp, Curv).
gb25_status build_curv_grid(gb25_model* m) {
  m->diag.invalidate_tables();   // (the diagnostics' own tables follow the grid: rebuilt by the next call that needs them)
  const gb25_config& c = m->cfg;
  const int Nx = m->Nx, Ny = m->Ny, H = c.halo, sx = Nx + 2 * H, sy = Ny + 2 * H + 1;
  const size_t n2 = (size_t)sx * sy;
  // (the fold is the northern edge of the top row of ranks only)
  const bool tri = is_folded(m);
  for (auto& a : m->h_curv) a.assign(n2, 0.0);
  auto at = [&](int id) -> std::vector<double>& { return m->h_curv[id]; };
  parallel_rows(-H, Ny + H + 1, [&](int j) {
    for (int i = -H; i < Nx + H; i++) {
      const size_t o = (size_t)(i + H) + (size_t)sx * (j + H);
      double v[GB25_M2_COUNT];
      curv_metrics_at(m, i + m->rx * Nx, j + m->j0, v, nullptr, nullptr);
      // (numbers of the model's float type, as a host's grid holds them: reciprocals below are those of the rounded values, so
      // that what gb25_get_metric2 hands out, fed back through gb25_set_curvilinear_grid, is the same grid to the last bit)
      for (int q = 0; q < GB25_M2_COUNT; q++) at(q)[o] = (double)(real)v[q];
    }
  });
  Curv& cv = m->g.cv;
  gb25_status s;
  auto up = [&](const std::vector<double>& h, const real** out) { return upload_table(m, h, 0, out); };
  auto recip = [&](int id) {
    std::vector<double> r(n2);
    for (size_t q = 0; q < n2; q++) r[q] = at(id)[q] != 0.0 ? 1.0 / at(id)[q] : 0.0;
    return r;
  };
  if ((s = up(at(GB25_M2_DXFC), &cv.dxfc)) || (s = up(at(GB25_M2_DXCF), &cv.dxcf)) || (s = up(at(GB25_M2_DYFC), &cv.dyfc)) ||
      (s = up(at(GB25_M2_DYCF), &cv.dycf)) || (s = up(at(GB25_M2_AZCC), &cv.azcc)) || (s = up(at(GB25_M2_PHICC), &cv.phicc)) ||
      (s = up(recip(GB25_M2_DXFC), &cv.rdxfc)) || (s = up(recip(GB25_M2_DYCF), &cv.rdycf)) ||
      (s = up(recip(GB25_M2_AZCC), &cv.razcc)) || (s = up(recip(GB25_M2_AZFC), &cv.razfc)) ||
      (s = up(recip(GB25_M2_AZCF), &cv.razcf)) || (s = up(recip(GB25_M2_AZFF), &cv.razff)))
    return s;
  {
    // Coriolis parameter at the u and v points: the mean of the two (f,f) values either side, formed in the float type
    // from the rounded values exactly as the plain kernels form it from their row table
    std::vector<double> fu(n2, 0.0), fv(n2, 0.0);
    const std::vector<double>& F = at(GB25_M2_FFF);
    for (int j = -H; j < Ny + H; j++)
      for (int i = -H; i < Nx + H - 1; i++) {
        const size_t o = (size_t)(i + H) + (size_t)sx * (j + H);
        fu[o] = (double)(real(0.5) * ((real)F[o] + (real)F[o + sx]));
        fv[o] = (double)(real(0.5) * ((real)F[o] + (real)F[o + 1]));
      }
    if ((s = up(fu, &cv.fbar_u)) || (s = up(fv, &cv.fbar_v))) return s;
  }
  cv.on = 1;
  cv.north_fold = tri ? 1 : 0;
  return GB25_OK;
}
// The metrics of the split-explicit sub-cycle on the work arrays of a slab (WIDENED: columns [-W, Nx + W), pitch Nx + 2W) and
// of a folded grid (TALL: Wy more rows beyond the pivot row, whose metrics are those of their images; a single folded domain
// has W = 0).  Global columns are wrapped into [0, Nx_global): the sub-cycle of a single domain wraps its indices the same
// way, so that a decomposition reads the very numbers the single domain reads.
gb25_status build_curv_wide(gb25_model* m) {
  const gb25_config& c = m->cfg;
  const int Nx = m->Nx, Ny = m->Ny, H = c.halo, W = m->W, wsx = Nx + 2 * W, sy = Ny + 2 * H + 1 + m->Wy + m->Wys;
  auto wrap = [&](int ig) { return ((ig % c.Nx) + c.Nx) % c.Nx; };
  std::vector<real> t[5];
  for (auto& a : t) a.assign((size_t)wsx * sy, real(0.));
  parallel_rows(-H - m->Wys, Ny + H + m->Wy + 1, [&](int j) {
    for (int i = -W; i < Nx + W; i++) {
      const size_t o = (size_t)(i + W) + (size_t)wsx * (j + H + m->Wys);
      double v[GB25_M2_COUNT];
      curv_metrics_at(m, wrap(i + m->rx * Nx), j + m->j0, v, nullptr, nullptr);
      t[0][o] = (real)v[GB25_M2_DYFC];
      t[1][o] = (real)v[GB25_M2_DXCF];
      t[2][o] = (real)(1.0 / (double)(real)v[GB25_M2_AZCC]);
      t[3][o] = (real)(1.0 / (double)(real)v[GB25_M2_DXFC]);
      t[4][o] = (real)(1.0 / (double)(real)v[GB25_M2_DYCF]);
    }
  });
  for (int q = 0; q < 5; q++) {
    if (!m->d_wideM[q]) HIPCHK(m->mem.alloc(&m->d_wideM[q], t[q].size() * sizeof(real)));
    HIPCHK(hipMemcpy(m->d_wideM[q], t[q].data(), t[q].size() * sizeof(real), hipMemcpyHostToDevice));
  }
  return GB25_OK;
}

// TEOS-10 (Roquet et al. 2015) coefficient table R[i][j][k] of s^i t^j zeta^k and the reference profile r0(zeta),
// folded per model level: rho - rho0 = sum_{i+j<=6} C_ij(k) s^i t^j with
// C_ij(k) = sum_m R_ijm zeta_k^m  (+ r0(zeta_k) - rho0 on the constant term).
struct EosTerm { int i, j, k; double v; };
const EosTerm kEos[] = {
    {0,0,0, 8.0189615746e+02}, {1,0,0, 8.6672408165e+02}, {2,0,0,-1.7864682637e+03}, {3,0,0, 2.0375295546e+03},
    {4,0,0,-1.2849161071e+03}, {5,0,0, 4.3227585684e+02}, {6,0,0,-6.0579916612e+01}, {0,1,0, 2.6010145068e+01},
    {1,1,0,-6.5281885265e+01}, {2,1,0, 8.1770425108e+01}, {3,1,0,-5.6888046321e+01}, {4,1,0, 1.7681814114e+01},
    {5,1,0,-1.9193502195e+00}, {0,2,0,-3.7074170417e+01}, {1,2,0, 6.1548258127e+01}, {2,2,0,-6.0362551501e+01},
    {3,2,0, 2.9130021253e+01}, {4,2,0,-5.4723692739e+00}, {0,3,0, 2.1661789529e+01}, {1,3,0,-3.3449108469e+01},
    {2,3,0, 1.9717078466e+01}, {3,3,0,-3.1742946532e+00}, {0,4,0,-8.3627885467e+00}, {1,4,0, 1.1311538584e+01},
    {2,4,0,-5.3563304045e+00}, {0,5,0, 5.4048723791e-01}, {1,5,0, 4.8169980163e-01}, {0,6,0,-1.9083568888e-01},
    {0,0,1, 1.9681925209e+01}, {1,0,1,-4.2549998214e+01}, {2,0,1, 5.0774768218e+01}, {3,0,1,-3.0938076334e+01},
    {4,0,1, 6.6051753097e+00}, {0,1,1,-1.3336301113e+01}, {1,1,1,-4.4870114575e+00}, {2,1,1, 5.0042598061e+00},
    {3,1,1,-6.5399043664e-01}, {0,2,1, 6.7080479603e+00}, {1,2,1, 3.5063081279e+00}, {2,2,1,-1.8795372996e+00},
    {0,3,1,-2.4649669534e+00}, {1,3,1,-5.5077101279e-01}, {0,4,1, 5.5927935970e-01}, {0,0,2, 2.0660924175e+00},
    {1,0,2,-4.9527603989e+00}, {2,0,2, 2.5019633244e+00}, {0,1,2, 2.0564311499e+00}, {1,1,2,-2.1311365518e-01},
    {0,2,2,-1.2419983026e+00}, {0,0,3,-2.3342758797e-02}, {1,0,3,-1.8507636718e-02}, {0,1,3, 3.7969820455e-01}};
const double kEosR0[6] = {4.6494977072e+01, -5.2099962525e+00, 2.2601900708e-01,
                          6.4326772569e-02, 1.5616995503e-02, -1.7243708991e-03};

gb25_status build_eos_tables(gb25_model* m) {
  const int Nz = m->cfg.Nz, offk = m->metric_off_k;
  const std::vector<double>&zc = m->h_metric[GB25_M_ZC], &dzf = m->h_metric[GB25_M_DZF], &zf = m->h_metric[GB25_M_ZF];
  // [28 (Nz+1): levels][28 (Nz+1): faces][Nz+1: dzf][28: the surface, Z = 0 -- the potential density of the derived fields]
  std::vector<double> tab((size_t)56 * (Nz + 1), 0.0), dz(Nz + 1), surf(28, 0.0);
  auto fold = [&](double Z, double* c) {
    const double zeta = -Z * 1e-4;
    for (const EosTerm& t : kEos) {
      int base = 0;
      for (int j = 0; j < t.j; j++) base += 7 - j;
      c[base + t.i] += t.v * std::pow(zeta, t.k);
    }
    double r0 = 0;
    for (int q = 5; q >= 0; q--) r0 = (r0 + kEosR0[q]) * zeta;
    c[0] += r0 - m->cfg.rho0;
  };
  for (int k = 0; k <= Nz; k++) {
    // geopotential height of level k; the halo level above the surface is mirrored (Oceananigans Z^ccc)
    fold((k < Nz) ? zc[offk + k] : zc[offk + Nz - 1] - dzf[offk + Nz - 1], &tab[(size_t)28 * k]);
    fold((double)(real)zf[offk + k], &tab[(size_t)28 * (Nz + 1 + k)]);   // (Z^ccf: the face itself, a number of the model's float type)
    dz[k] = dzf[offk + k];
  }
  fold(0.0, surf.data());
  double* d = nullptr;
  HIPCHK(m->mem.alloc(&d, (tab.size() + dz.size() + surf.size()) * sizeof(double)));
  HIPCHK(hipMemcpy(d + tab.size() + dz.size(), surf.data(), surf.size() * sizeof(double), hipMemcpyHostToDevice));
  m->diag.eos0 = d + tab.size() + dz.size();
  HIPCHK(hipMemcpy(d, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(d + tab.size(), dz.data(), dz.size() * sizeof(double), hipMemcpyHostToDevice));
  m->g.eos = d;
  m->g.eosf = d + (size_t)28 * (Nz + 1);
  m->g.dzf_d = d + tab.size();
  return GB25_OK;
}

// GridFittedBottom(bottom_height) -> first active level per column -> the folded tables (device_common.hpp, Immersed).
// zb(i, j): bottom height at the centre of LOCAL column i (any i in [-E, Nx + E)), GLOBAL row j in [0, Ny_global).
// Restated from Oceananigans.ImmersedBoundaries [UPSTREAM-UNVERIFIED]; oracle/gb25_oracle.c states the same rules cell
// by cell (inactive_cell / stencil_active) and tests/test_gpu_immersed.py compares the two.
template <class ZB>
gb25_status build_bottom(gb25_model* m, ZB zb) {
  m->diag.invalidate_tables();   // (the diagnostics' own tables follow the grid: rebuilt by the next call that needs them)
  const gb25_config& c = m->cfg;
  const int Nx = m->Nx, Ny = m->Ny, Nz = c.Nz, H = c.halo, offk = m->metric_off_k, j0 = m->j0;
  const int E = std::max(H, m->W) + 4, ksx = Nx + 2 * E;
  // (rows: the own ones and, on a rank of a 2-D decomposition, the neighbours' rows its stencils and its widened sub-cycle reach)
  const int Ey = m->Ry > 1 ? H + std::max(m->Wy, m->Wys) + 6 : 0;
  const std::vector<double>&zc = m->h_metric[GB25_M_ZC], &zf = m->h_metric[GB25_M_ZF];
  m->kb_E = E;
  m->kb_Ey = Ey;
  m->kbot.assign((size_t)ksx * (Ny + 2 * Ey), 255);
  std::atomic<bool> any{false};
  auto level = [&](double b) {   // number of immersed cells of a column whose bottom is at height b
    int kb = 0;
    for (int k = 0; k < Nz; k++)
      if ((double)(real)zc[offk + k] <= b) kb = k + 1;   // z_center <= bottom: immersed (CenterImmersedCondition)
    return kb;
  };
  parallel_rows(-Ey, Ny + Ey, [&](int j) {
    if (j + j0 < 0 || j + j0 >= c.Ny) return;   // (beyond the walls / the fold: below)
    bool row_any = false;
    for (int i = -E; i < Nx + E; i++) {
      const int kb = level(zb(i, j + j0));
      m->kbot[(size_t)(i + E) + (size_t)ksx * (j + Ey)] = kb;
      row_any = row_any || (kb > 0 && j >= 0 && j < Ny);
    }
    if (row_any) any = true;
  });
  m->immersed = any.load();
  // level from which cell (i, j) is active; rows beyond the walls never are; rows beyond the zipper fold are the images
  // of the cells they mirror
  const bool nfold = m->g.cv.north_fold != 0;
  auto thr = [&](int i, int j) -> int {
    if (nfold && j >= Ny) {
      // the mirrored cell: GLOBAL column Nx_global - 1 - ig, usually another rank's -- the bottom is a function of the
      // global position, evaluated here (a slab sees its partner's bottom without any exchange)
      const int il = c.Nx - 1 - (i + m->rx * Nx) - m->rx * Nx, jm = 2 * (c.Ny - 1) - (j + j0);   // (the fold pivots on the centres of row Ny-1)
      return jm < 0 ? 255 : level(zb(il, jm));
    }
    if (j + j0 < 0 || j + j0 >= c.Ny) return 255;
    return m->kbot[(size_t)(std::min(std::max(i, -E), Nx + E - 1) + E) + (size_t)ksx * (j + Ey)];
  };
  auto node_x = [&](int q, int j) { return std::min(thr(q - 1, j), thr(q, j)); };   // face node: inactive when BOTH cells are
  auto node_y = [&](int i, int q) { return std::min(thr(i, q - 1), thr(i, q)); };
  auto depth = [&](int i, int j) -> double {   // static column depth: top face - materialised bottom
    const int jj = (nfold && j >= Ny) ? j : std::min(std::max(j + j0, 0), c.Ny - 1) - j0;
    const int kb = thr(i, jj);
    return (double)(real)zf[offk + Nz] - (double)(real)zf[offk + kb];
  };
  const int sx = Nx + 2 * H, sy = Ny + 2 * H + 1;
  std::vector<unsigned> A((size_t)sx * sy, 0), B(A.size(), 0), C(A.size(), 0), D(A.size(), 0);
  std::vector<real> Hf(A.size(), 0), Hc(A.size(), 0), rHf(A.size(), 0), rHc(A.size(), 0);
  // (rows: the own ones; with a neighbour rank on a side, that side's halo rows too -- the corrector runs there as well)
  parallel_rows(m->ys_open ? -H : 0, (m->yn_open ? Ny + H : Ny) + 1, [&](int j) {
    for (int i = -H; i < Nx + H; i++) {
      const size_t o = (size_t)(i + H) + (size_t)sx * (j + H);
      int KX5 = 0, KX3 = 0, KY5 = 0, KY3 = 0, KXC5 = 0, KXC3 = 0, KYC5 = 0, KYC3 = 0;
      for (int q = -3; q <= 2; q++) { KX5 = std::max(KX5, thr(i + q, j)); KY5 = std::max(KY5, thr(i, j + q)); }
      for (int q = -2; q <= 1; q++) { KX3 = std::max(KX3, thr(i + q, j)); KY3 = std::max(KY3, thr(i, j + q)); }
      for (int q = -2; q <= 3; q++) { KXC5 = std::max(KXC5, node_x(i + q, j)); KYC5 = std::max(KYC5, node_y(i, j + q)); }
      for (int q = -1; q <= 2; q++) { KXC3 = std::max(KXC3, node_x(i + q, j)); KYC3 = std::max(KYC3, node_y(i, j + q)); }
      const int kc = std::min(thr(i, j), Nz);   // (the extra face row j = Ny has no cells: its kc is never used)
      const int KPU = std::max(thr(i - 1, j), thr(i, j));
      // wall faces: the plain grid's business (the fold line is no wall)
      const int KPV = (j + j0 == 0 || (j + j0 >= c.Ny && !nfold)) ? 0 : std::min(std::max(thr(i, j - 1), thr(i, j)), 255);
      A[o] = (unsigned)kc | (unsigned)KX5 << 8 | (unsigned)KX3 << 16 | (unsigned)KY5 << 24;
      B[o] = (unsigned)KY3 | (unsigned)KXC5 << 8 | (unsigned)KXC3 << 16 | (unsigned)KYC5 << 24;
      C[o] = (unsigned)KYC3 | (unsigned)std::min(KPU, 255) << 8 | (unsigned)KPV << 16;
      int KX7 = 0, KY7 = 0;   // WENO(order = 7) tracer advection: the eight cells around the x face / the y face
      for (int q = -4; q <= 3; q++) { KX7 = std::max(KX7, thr(i + q, j)); KY7 = std::max(KY7, thr(i, j + q)); }
      D[o] = (unsigned)std::min(KX7, 255) | (unsigned)std::min(KY7, 255) << 8 |
             (unsigned)std::min(node_x(i, j), 255) << 16 | (unsigned)std::min(node_y(i, j), 255) << 24;
      const double hf = std::min(depth(i - 1, j), depth(i, j)), hc = std::min(depth(i, j - 1), depth(i, j));
      Hf[o] = (real)hf;
      Hc[o] = (real)hc;
      rHf[o] = hf > 0 ? (real)(1.0 / hf) : real(0.);
      // (the v face on the southern wall never moves; its correction divides by the full depth as on the plain grid)
      rHc[o] = j + j0 == 0 ? (real)(1.0 / ((double)(real)zf[offk + Nz] - (double)(real)zf[offk])) : (hc > 0 ? (real)(1.0 / hc) : real(0.));
    }
  });
  auto upload = [&](const void* h, size_t bytes, void** d) -> gb25_status {
    if (!*d) HIPCHK(m->mem.alloc(d, bytes));
    HIPCHK(hipMemcpy(*d, h, bytes, hipMemcpyHostToDevice));
    return GB25_OK;
  };
  gb25_status s;
  if ((s = upload(A.data(), A.size() * sizeof(unsigned), (void**)&m->d_ord[0]))) return s;
  if ((s = upload(B.data(), B.size() * sizeof(unsigned), (void**)&m->d_ord[1]))) return s;
  if ((s = upload(C.data(), C.size() * sizeof(unsigned), (void**)&m->d_ord[2]))) return s;
  if ((s = upload(D.data(), D.size() * sizeof(unsigned), (void**)&m->d_ord[3]))) return s;
  if ((s = upload(Hf.data(), Hf.size() * sizeof(real), (void**)&m->d_H[0]))) return s;
  if ((s = upload(Hc.data(), Hc.size() * sizeof(real), (void**)&m->d_H[1]))) return s;
  if ((s = upload(rHf.data(), rHf.size() * sizeof(real), (void**)&m->d_H[2]))) return s;
  if ((s = upload(rHc.data(), rHc.size() * sizeof(real), (void**)&m->d_H[3]))) return s;
  m->g.im.ordA = m->d_ord[0]; m->g.im.ordB = m->d_ord[1]; m->g.im.ordC = m->d_ord[2]; m->g.im.ordD = m->d_ord[3];
  m->g.im.Hfc = m->d_H[0]; m->g.im.Hcf = m->d_H[1]; m->g.im.rHfc = m->d_H[2]; m->g.im.rHcf = m->d_H[3];
  if (m->slab || nfold) {   // the same depths on the work arrays of the sub-cycle: widened slab / tall folded grid
    const int W = m->W, wsx = Nx + 2 * W;
    std::vector<real> wf((size_t)wsx * (sy + m->Wy + m->Wys), 0), wc(wf.size(), 0);
    for (int j = -m->Wys; j <= Ny + m->Wy; j++)
      for (int i = -W; i < Nx + W; i++) {
        const size_t o = (size_t)(i + W) + (size_t)wsx * (j + H + m->Wys);
        wf[o] = (real)std::min(depth(i - 1, j), depth(i, j));
        wc[o] = (real)std::min(depth(i, j - 1), depth(i, j));
      }
    if ((s = upload(wf.data(), wf.size() * sizeof(real), (void**)&m->d_wideH[0]))) return s;
    if ((s = upload(wc.data(), wc.size() * sizeof(real), (void**)&m->d_wideH[1]))) return s;
  }
  m->valid.void_lookaheads();
  return GB25_OK;
}
// gaussian_islands(lambda, phi) = zb + h (mtn1 + mtn2), zb = z[1], h = -zb + 100; mountains 5 degrees wide at (70 E,
// 55 N) and (250 E, 55 N) (GB-25 src/model_utils.jl:67-80,138-140).  A function of the GLOBAL longitude: the halo
// columns of a slab see the neighbour's bottom without any exchange.
double gaussian_islands_bottom(const gb25_model* m, int i_local, int j) {
  const gb25_config& c = m->cfg;
  const double dlam = (c.lon_east - c.lon_west) / c.Nx, dphi = (c.lat_north - c.lat_south) / c.Ny;
  int ig = (i_local + m->rx * m->Nx) % c.Nx;
  if (ig < 0) ig += c.Nx;
  auto mtn = [](double l, double p, double l1, double p1) {
    const double d = 5;
    return std::exp(-((l - l1) * (l - l1) + (p - p1) * (p - p1)) / (2 * d * d));
  };
  const double z1 = -c.depth, h = -z1 + 100.0;
  if (m->g.cv.on) {
    // physical coordinates of the cell centre, the longitude brought next to each mountain (the tripolar grid starts AT
    // the first mountain's longitude: without this only its eastern half would exist)
    double lam, phi;
    if (c.grid_type >= GB25_GRID_TRIPOLAR) {   // (the centre node alone: this runs for every column of the bottom tables)
      const GNode cc = tripolar_node(70.0 + (ig + 0.5) * (360.0 / c.Nx), c.lat_south + j * ((90.0 - c.lat_south) / (c.Ny - 1)));
      lam = cc.lam;
      phi = cc.phi;
    } else {
      double v[GB25_M2_COUNT];
      curv_metrics_at(m, ig, j, v, &lam, &phi);
    }
    const double l1 = lam - 360.0 * std::floor((lam - 70.0 + 180.0) / 360.0), l2 = lam - 360.0 * std::floor((lam - 250.0 + 180.0) / 360.0);
    return z1 + h * (mtn(l1, phi, 70, 55) + mtn(l2, phi, 70 + 180, 55));
  }
  const double lam = c.lon_west + (ig + 0.5) * dlam;
  // (the centre latitude as the model's float type holds it: phi_c is a metric of the grid)
  const double phi = (double)(real)(c.lat_south + (j + 0.5) * dphi);
  return z1 + h * (mtn(lam, phi, 70, 55) + mtn(lam, phi, 70 + 180, 55));
}

gb25_status alloc_field(gb25_model* m, Field& F, int nx, int ny, int nz) {
  F.nx = nx; F.ny = ny; F.nz = nz;
  hipError_t e = m->mem.alloc(&F.d, F.elems() * sizeof(real));
  if (e != hipSuccess)
    return fail(m, GB25_ERR_OUT_OF_MEMORY, "hipMalloc of %zu bytes failed: %s", F.elems() * sizeof(real),
                hipGetErrorString(e));
  HIPCHK(zeroed(F.d, F.elems() * sizeof(real)));
  return GB25_OK;
}
inline gb25_status alloc_field(gb25_model* m, Field& F, Dims d) { return alloc_field(m, F, d.nx, d.ny, d.nz); }
// an array with the parent extents of field id (model_layout.hpp)
inline gb25_status alloc_like(gb25_model* m, Field& F, int id) { return alloc_field(m, F, parent_dims(m->layout, id)); }
// three arrays in ONE zeroed block, F[q] with the extents dims(layout, id0 + q): the filtered state and its partners, the running
// averages on the wide domain (one memset per step)
gb25_status alloc_three(gb25_model* m, Field F[3], Dims (*dims)(const ModelLayout&, int), int id0, real** base) {
  size_t tot = 0;
  for (int q = 0; q < 3; q++) tot += dims(m->layout, id0 + q).elems();
  HIPCHK(m->mem.alloc(base, tot * sizeof(real), true));
  real* d = *base;
  for (int q = 0; q < 3; q++) {
    const Dims e = dims(m->layout, id0 + q);
    F[q] = Field{d, e.nx, e.ny, e.nz};
    d += e.elems();
  }
  return GB25_OK;
}

inline int mom_kchunks(const gb25_model* m) { return std::max(1, m->g.Nz / m->mom_chunk_levels); }
inline int trc_kchunks(const gb25_model* m) { return std::max(1, m->g.Nz / m->trc_chunk_levels); }   // (>= 12 levels: z-carry start-up ~3 %)
// w on the fly: the chunkings of the two tendency kernels must be the one the look-ahead's chunk sums were made with
inline bool chunkings_match(const gb25_model* m) { return trc_kchunks(m) == mom_kchunks(m); }
inline dim3 grid2(int nx, int ny, dim3 b) { return dim3((nx + b.x - 1) / b.x, (ny + b.y - 1) / b.y); }

Halo3 halo3(gb25_model* m, Fields3 sel) {
  Halo3 h{};
  int n = 0;
  if (has(sel, Fields3::UV)) {   // (xf, neg: how the field crosses the zipper fold -- on x faces, changing sign)
    h.p[n] = m->f[GB25_U].d; h.xf[n] = 1; h.neg[n] = 1; h.is_v[n++] = 0;
    h.p[n] = m->f[GB25_V].d; h.neg[n] = 1; h.is_v[n++] = 1;
  }
  if (has(sel, Fields3::TS)) {
    h.p[n] = m->f[GB25_T].d; h.is_v[n++] = 0;
    h.p[n] = m->f[GB25_S].d; h.is_v[n++] = 0;
  }
  if (has(sel, Fields3::E)) h.p[n] = m->f[GB25_E].d, h.is_v[n++] = 0;   // (the TKE tracer of CATKE: a launch of its own)
  h.n = n;
  return h;
}
Halo2 halo2_prognostic(gb25_model* m) {
  Halo2 h{};
  h.p[0] = m->f[GB25_ETA].d; h.is_v[0] = 0;
  h.p[1] = m->f[GB25_BT_U].d; h.is_v[1] = 0; h.xf[1] = 1; h.neg[1] = 1;
  h.p[2] = m->f[GB25_BT_V].d; h.is_v[2] = 1; h.neg[2] = 1;
  h.n = 3;
  return h;
}
Halo2 halo2_G(gb25_model* m) {   // the barotropic forcing G.U, G.V
  Halo2 h{};
  h.p[0] = m->f[GB25_GN_BT_U].d; h.is_v[0] = 0; h.xf[0] = 1; h.neg[0] = 1;
  h.p[1] = m->f[GB25_GN_BT_V].d; h.is_v[1] = 1; h.neg[1] = 1;
  h.n = 2;
  return h;
}
// the single-domain producers write the halo cells derived from their output themselves (option FOLD_FILLS) -- not across
// the zipper fold, whose images live in other threads' columns, and not with a closure (the implicit solve comes after
// the look-aheads' writes)
inline bool producers_fold(const gb25_model* m) {
  return !m->slab && m->fold_fills && !m->g.cv.north_fold && m->nu == 0 && m->kappa == 0 && !m->catke && m->tracer_order == 5;
}
// rows of y faces a launch covers (face 0 is the southern wall; the faces beyond the last row of cells are a wall or, on a
// folded grid, halo cells)
inline int v_rows(const Grid& g) { return g.Ny; }

// what the plans of launch_plan.hpp need to know of the model: the one place that reads it
inline LaunchFacts launch_facts(const gb25_model* m) {
  const Grid& g = m->g;
  return {g.Nx, g.Ny, g.Nz, g.H, g.sy_c, g.sy_v, g.x_periodic != 0, g.cv.north_fold != 0, g.cv.pivot_slaved, m->slab, m->ys_open, m->yn_open,
          m->fill_fused != 0, g.cv.on != 0, g.pl_c, g.pl_v, (long)m->f[GB25_W].elems(), (int)sizeof(real), m->mom_chunk_levels,
          m->trc_chunk_levels, v_rows(g), m->Ry, m->immersed != 0, m->tracer_order, m->tracer_rows_forced};
}

// Binds the model's arrays to a fill request, plans it (plan_fill) and issues the planned launches in order on the model's stream.
// given: the 2-D fields of a Fields2::Given request.  The timer is the caller's.
gb25_status issue_fill(gb25_model* m, FillRequest rq, const Halo2& given) {
  const Grid& g = m->g;
  const Halo3 h3 = halo3(m, rq.f3);
  const Halo2 h2 = rq.f2 == Fields2::Given ? given : rq.f2 == Fields2::Prognostic ? halo2_prognostic(m) : Halo2{};
  rq.n_given = given.n;
  const FillPlan p = plan_fill(rq, launch_facts(m));
  const dim3 b(256);
  auto launch = [&](const Grid& gl, const FillLaunch& L) {
    const dim3 gr(L.gx, L.gy, L.gz);
    switch (L.kernel) {
      case FillKernel::Y: hipLaunchKernelGGL(k_fill_y, gr, b, 0, m->stream, gl, h3, h2, L.i0, L.ni); break;
      case FillKernel::YZ: hipLaunchKernelGGL(k_fill_yz, gr, b, 0, m->stream, gl, h3, h2, L.i0, L.ni, L.jlo); break;
      case FillKernel::Fold: hipLaunchKernelGGL(k_fill_fold, gr, b, 0, m->stream, gl, h3, h2); break;
      case FillKernel::X: hipLaunchKernelGGL(k_fill_x, gr, b, 0, m->stream, gl, h3, h2, L.rows_c, L.rows_v); break;
      case FillKernel::Fused:
        hipLaunchKernelGGL(k_fill_fused, gr, b, 0, m->stream, gl, h3, h2, L.nbx, L.nb_yz, L.nbr, L.rows_c, L.rows_v);
        break;
    }
  };
  for (int q = 0; q < p.n; q++) {
    if (p.l[q].flat) {
      Grid g2 = g;
      g2.Nz = 0;
      launch(g2, p.l[q]);
    } else {
      launch(g, p.l[q]);
    }
  }
  LAUNCHCHK();
  return GB25_OK;
}
// y / z boundary layers (always local), the rows beyond a single domain's zipper fold and the periodic x copy of the fields and
// columns the request names (launch_plan.hpp)
gb25_status fill_halos_impl(gb25_model* m, FillRequest rq, const Halo2& given = Halo2{}) {
  Timed t(m, GB25_K_FILL_HALOS);
  return issue_fill(m, rq, given);
}
// the caller's 2-D fields alone, with the periodic x copy; no timer of its own
gb25_status fill_halos_2d(gb25_model* m, Halo2 h2) { return issue_fill(m, FillRequest::flat(Fields2::Given, Columns::OwnWithPeriodicX), h2); }

gb25_status compute_w_impl(gb25_model* m, Pass pass = Pass::Whole) {
  const Grid& g = m->g;
  Timed t(m, GB25_K_COMPUTE_W);
  const WColumns w = w_columns(pass, launch_facts(m));
  const dim3 b(w.bx, w.by);
  const LazyCorr lz{m->corr[0].d, m->corr[1].d, m->wbase, m->g.sx * m->g.sy_v};
  auto kw = k_compute_w<false, false>;
  if (m->route.kernels_add_correction()) kw = k_compute_w<false, true>;
  else if (g.cv.on) kw = k_compute_w<true, false>;
  hipLaunchKernelGGL(kw, grid2(w.cols.ni, w.rows, b), b, 0, m->stream, g, m->f[GB25_U].d, m->f[GB25_V].d, m->f[GB25_W].d, w.cols.i0,
                     w.cols.na(), w.cols.b0(), w.cols.nb(), lz);
  LAUNCHCHK();
  return GB25_OK;
}
// Hydrostatic pressure and its differences on the columns and rows of `box`, in the form plan_pressure chooses (launch_plan.hpp).
// may_skip_p: pHY' itself need not be stored (nobody reads it inside a composite step unless it is pinned).
static_assert(PR == PRESSURE_ROWS, "the plan counts the rows per thread of k_compute_p<PR>");
gb25_status compute_p_impl(gb25_model* m, PressureBox box, bool may_skip_p = false) {
  const Grid& g = m->g;
  if (m->pressure_bits == 32) {
    // the model float type's own arithmetic, whole extended range, pHY' stored, differences from the stored values
    Timed t(m, GB25_K_COMPUTE_P);
    dim3 b(64, 4);
    const int nx = g.Nx + 2 * g.H - 2, ny = g.Ny + 2 * g.H - 2;
    hipLaunchKernelGGL(k_compute_p_literal, grid2(nx, ny, b), b, 0, m->stream, g, m->f[GB25_T].d, m->f[GB25_S].d,
                       m->f[GB25_PHY].d, -g.H + 1, nx, 0, 0);
    const long n = (long)m->f[GB25_PHY].elems();
    hipLaunchKernelGGL(k_pressure_differences, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, m->stream, g,
                       m->f[GB25_PHY].d, m->dpx.d, m->dpy.d, n);
    m->phy_stale = false;
    LAUNCHCHK();
    return GB25_OK;
  }
  const bool write_p = !may_skip_p || m->phy_pinned;
  m->phy_stale = !write_p;
  Timed t(m, GB25_K_COMPUTE_P);
  const PressurePlan p = plan_pressure(box, launch_facts(m), m->pressure_form);
  auto kern = write_p ? k_compute_p_tile<true> : k_compute_p_tile<false>;
  if (p.form == 2) kern = write_p ? k_compute_p<1, true> : k_compute_p<1, false>;
  if (p.form == 3) kern = write_p ? k_compute_p<PR, true> : k_compute_p<PR, false>;
  const Cols& c = box.cols;
  // (the kernels' N^2 output is unused: CATKE's N^2 is SeawaterBuoyancy's dz_b -- alpha dzT - beta dzS -- not a difference of buoyancies: k_catke_n2)
  hipLaunchKernelGGL(kern, dim3(p.gx, p.gy), dim3(64, 4), 0, m->stream, g, m->f[GB25_T].d, m->f[GB25_S].d, m->f[GB25_PHY].d, m->dpx.d,
                     m->dpy.d, c.i0, c.i0 + c.na() - 1, c.b0(), c.b0() + c.nb() - 1, p.tiles_a, (real*)nullptr, box.j_first, box.j_last);
  LAUNCHCHK();
  return GB25_OK;
}

void tile_grid(const Grid& g, int* nbx, int* nb) {
  *nbx = (g.Nx + TX - 1) / TX;
  int nby = (g.Ny + TY - 1) / TY;
  *nb = *nbx * nby * g.Nz;
}

// the options' half of the split of a slab's tendencies into the Interior and Edges passes; the geometry's: momentum_splittable
inline bool tendencies_split(const gb25_model* m) {
  return m->slab && m->split_tendencies && m->two_streams && m->pressure_bits == 64 && m->kernel_gen >= 2 &&
         momentum_splittable(launch_facts(m));
}

// ---- which template instance of a tendency kernel runs.  A family's flags are in the order of the kernel's template
// parameters; pick_instance turns their values into the instance and instantiates only the variants the family's rule admits
// (the rule is also the kernel's static_assert: tendency_kernels.hpp).  A state no variant exists for is an error.
template <class Fam, bool... B>
typename Fam::kernel_t pick_instance(const std::array<bool, Fam::n>& f) {
  if constexpr (sizeof...(B) < Fam::n)
    return f[sizeof...(B)] ? pick_instance<Fam, B..., true>(f) : pick_instance<Fam, B..., false>(f);
  else if constexpr (Fam::admits(B...))
    return Fam::template instance<B...>();
  else
    return nullptr;
}
template <class Fam>
gb25_status tendency_instance(gb25_model* m, const std::array<bool, Fam::n>& f, typename Fam::kernel_t* k) {
  if ((*k = pick_instance<Fam>(f))) return GB25_OK;
  std::string bits;
  for (bool b : f) bits += b ? '1' : '0';
  return fail(m, GB25_ERR_STATE, "the %s kernel has no variant for the flags %s", Fam::name, bits.c_str());
}

struct MomentumKernels {   // k_momentum_tendencies_v5
  // waves/SIMD the register allocator is held to: 4 (128 VGPRs) in fp32; fp64 operands are register pairs,
  // so the Float64 build asks for 2 (256 VGPRs) instead of spilling.  TYm: rows (= waves) per block (tile_sizes.hpp)
  static constexpr int MW = sizeof(real) == 8 ? 2 : 4, TYm = MOMENTUM_TY, n = 6;
  static constexpr const char* name = "momentum (AHEAD IMM CURV LAZY DRAG WFLY)";
  using kernel_t = decltype(&k_momentum_tendencies_v5<MW, TYm, false, false>);
  static constexpr bool admits(bool a, bool i, bool c, bool l, bool d, bool w) { return momentum_variant(a, i, c, l, d, w); }
  template <bool... B> static kernel_t instance() { return k_momentum_tendencies_v5<MW, TYm, B...>; }
};
// pass: see Pass (launch_plan.hpp).  WFLY: w on the fly in a lazy step, or beside the corrector's sweep (memory holds the corrected
// velocities, only w is not read) -- in the passes over the whole domain
std::array<bool, MomentumKernels::n> momentum_flags(const gb25_model* m, Pass pass) {
  const bool ahead = m->ab2_ahead == 1 && !m->valid.ptr_exposed, curv = m->g.cv.on;
  const StepRoute& r = m->route;
  return {ahead, m->immersed || curv, curv, r.kernels_add_correction(), m->bottom_drag != 0,
          ahead && r.kernels_carry_w() && (r.kernels_add_correction() || pass == Pass::Whole)};
}

struct TracerKernels {   // k_tracer_tendencies_v5; the flags O7: ORD = 7 (WENO(order = 7)), else 5; R2: ROWS = 2 (two rows per lane), else 1
  static constexpr int TW = sizeof(real) == 8 ? 3 : 6;    // see MomentumKernels::MW (Float32: held to 80 VGPRs, six waves per SIMD)
  static constexpr int TW7 = sizeof(real) == 8 ? 2 : 5;   // (the order-7 windows: 9 register pairs per direction; 90-96 VGPRs without a spill)
  // (two rows per lane: three waves per SIMD.  133 VGPRs without a spill; held to four waves -- 127 VGPRs -- the headline instance
  // reloads three spilled pairs inside the level loop and is 0.3 % slower; held to five -- 96 VGPRs, 47 spilled dwords -- the step
  // is 32 % slower: DESIGN section 4)
  static constexpr int TW2 = sizeof(real) == 8 ? 2 : 3;
  static constexpr int n = 9;
  static constexpr const char* name = "tracer (AHEAD IMM FOLD CURV LAZY O7 WFLY WCORR R2)";
  using kernel_t = decltype(&k_tracer_tendencies_v5<TW, false, false, false>);
  static constexpr bool admits(bool a, bool i, bool f, bool c, bool l, bool o7, bool w, bool wc, bool r2) {
    return tracer_variant(a, i, f, c, l, o7 ? 7 : 5, w, wc, r2 ? 2 : 1);
  }
  template <bool A, bool I, bool F, bool C, bool L, bool O7, bool W, bool WC, bool R2>
  static kernel_t instance() { return k_tracer_tendencies_v5<R2 ? TW2 : O7 ? TW7 : TW, A, I, F, C, L, O7 ? 7 : 5, W, WC, R2 ? 2 : 1>; }
};
// rows: the rows per lane plan_tracers chose.
// WCORR: the corrector through the tracer kernel -- it adds du, dv as it loads (LAZY) and writes the corrected u, v; the halo
// cells of the next T, S are then left to the fill (no FOLD)
std::array<bool, TracerKernels::n> tracer_flags(const gb25_model* m, int rows) {
  const bool ahead = m->ab2_ahead && !m->valid.ptr_exposed, curv = m->g.cv.on, wcorr = m->route.tracer_kernel_corrects();
  return {ahead, m->immersed || curv, ahead && producers_fold(m) && !wcorr, curv, m->route.kernels_add_correction() || wcorr,
          m->tracer_order == 7, ahead && m->route.kernels_carry_w(), wcorr, rows == 2};
}

struct SingleKernels {   // k_tracer_tendencies_single (CATKE's e); O7 as in TracerKernels
  static constexpr int TW = sizeof(real) == 8 ? 2 : 4, n = 4;
  static constexpr const char* name = "one-tracer (IMM CURV O7 WFLY)";
  using kernel_t = decltype(&k_tracer_tendencies_single<TW, false, false, 5>);
  static constexpr bool admits(bool i, bool c, bool o7, bool w) { return single_variant(i, c, o7 ? 7 : 5, w); }
  template <bool I, bool C, bool O7, bool W> static kernel_t instance() { return k_tracer_tendencies_single<TW, I, C, O7 ? 7 : 5, W>; }
};
// (WFLY: the field w is stale, the kernel carries w up its chunks like the two others)
std::array<bool, SingleKernels::n> single_flags(const gb25_model* m) {
  const bool curv = m->g.cv.on;
  return {m->immersed || curv, curv, m->tracer_order == 7, m->route.kernels_carry_w()};
}

// pass (launch_plan.hpp): every tile column; the interior tile columns (a12: launched before the x-halo bundle has arrived); the edge
// tile columns, then whatever follows the complete evaluation (the look-ahead's finish kernel).
gb25_status materialize_prev_uv(gb25_model* m);
gb25_status momentum_impl(gb25_model* m, Pass pass = Pass::Whole) {
  const Grid& g = m->g;
  int nbx, nb;
  m->valid.tendency_kernel_runs(pass != Pass::Edges);   // look-aheads made from the previous tendencies are void
  if (m->kernel_gen >= 2) {
    Timed t(m, GB25_K_GU);   // the fused G_u + G_v kernel is accounted under the "gu" timer
    const MomentumPlan p = plan_momentum(pass, launch_facts(m));
    TileCols tc{p.n, p.nlead, p.bx0, p.bx1};
    const std::array<bool, MomentumKernels::n> flags = momentum_flags(m, pass);
    const bool ahead = flags[0];
    UvAhead nx{};
    const real dt = (real)m->last_dt, chi = (real)m->cfg.chi;
    if (ahead && m->prev_uv_src == 2)   // (the partner buffers still hold CATKE's previous velocities: a caller of the single phases)
      if (gb25_status s_ = materialize_prev_uv(m)) return s_;
    if (ahead) {   // predicted parameters of the next ab2_step!: the clock's dt and the model's chi
      nx.GmU = m->f[GB25_GM_U].d; nx.GmV = m->f[GB25_GM_V].d;
      nx.un = m->ahead_uv[0].d; nx.vn = m->ahead_uv[1].d;
      nx.P = m->uv_partials;
      nx.dt = dt; nx.C1 = real(1.5) + chi; nx.C2 = real(0.5) + chi;
      nx.plane2 = g.sx * g.sy_v;
      nx.fold = (producers_fold(m) && !m->immersed) ? 1 : 0;   // (with a bottom the corrector's own halo writes do it)
    }
    if (m->bottom_drag != 0) {
      // the bottom flux boundary condition of u, v from the (corrected) velocities this evaluation sees
      dim3 b(64, 4);
      hipLaunchKernelGGL(m->immersed ? k_bottom_drag_flux<true> : k_bottom_drag_flux<false>, grid2(p.drag_n, v_rows(g), b), b, 0,
                         m->stream, g, m->f[GB25_U].d, m->f[GB25_V].d, m->d_bottom_flux[0], m->d_bottom_flux[1],
                         (real)m->bottom_drag, p.drag_i_first, p.drag_n);
    }
    const LazyCorr lz{m->corr[0].d, m->corr[1].d, m->wbase, m->g.sx * m->g.sy_v};
    // (single domain: the kernel also writes the halo images of the next u, v; a slab's come with the next bundle)
    if (m->route.memory_lacks_correction() && !(m->slab || (nx.fold && pass == Pass::Whole)))
      return fail(m, GB25_ERR_STATE, "internal: uncorrected velocities in a step whose momentum kernel cannot correct them");
    MomentumKernels::kernel_t k5;
    if (gb25_status s_ = tendency_instance<MomentumKernels>(m, flags, &k5)) return s_;
    // one launch per run of chunks of levels within the kernel's reach (tendency_plan.hpp).  Normally: one launch, kofs = 0
    for (int c0 = 0; p.nb() > 0 && c0 < p.kchunks;) {
      const ChunkRun run = chunk_run(p.chunks, c0);
      tc.cr = ChunkRange{run.first, run.count, run.kofs};
      const long oc_ = (long)g.pl_c * run.kofs, ov_ = (long)g.pl_v * run.kofs;
      UvAhead nr = nx;
      if (ahead) { nr.GmU += oc_; nr.GmV += ov_; nr.un += oc_; nr.vn += ov_; }
      const int nbr = p.n * p.nby * run.count;
      hipLaunchKernelGGL(k5, dim3(nbr), dim3(V2_TX, MomentumKernels::TYm), 0, m->stream, g, m->f[GB25_U].d + oc_, m->f[GB25_V].d + ov_,
                         m->f[GB25_W].d + oc_, m->dpx.d + oc_, m->dpy.d + oc_, m->f[GB25_GN_U].d + oc_, m->f[GB25_GN_V].d + ov_,
                         tc, p.kchunks, nbr, nr, lz);
      c0 = run.first + run.count;
    }
    t.stop();   // the timer covers the tendency kernel alone
    if (ahead && p.finish) {
      dim3 b(64, 4);
      hipLaunchKernelGGL(k_ab2_velocities_finish, grid2(g.Nx, v_rows(g), b), b, 0, m->stream, g, m->uv_partials, p.kchunks,
                         nx.plane2, m->ahead_G[0].d, m->ahead_G[1].d, m->ahead_colsum[0].d, m->ahead_colsum[1].d);
      m->valid.record_velocity_lookahead(dt, chi);
    }
    LAUNCHCHK();
    return GB25_OK;
  }
  if (pass == Pass::Interior) return GB25_OK;   // the direct-stencil kernels are not split: everything after the halos arrived
  if (m->immersed || g.cv.on) return fail(m, GB25_ERR_STATE, "the direct-stencil kernels (GB25_OPT_KERNELS = 1) know neither immersed boundaries nor curvilinear grids");
  if (g.top_flux[0] || g.top_flux[1] || g.bottom_flux[0]) return fail(m, GB25_ERR_STATE, "the direct-stencil kernels (GB25_OPT_KERNELS = 1) know no flux boundary conditions");
  tile_grid(g, &nbx, &nb);
  dim3 b(TX, TY);
  {
    Timed t(m, GB25_K_GU);
    hipLaunchKernelGGL(k_gu, dim3(nb), b, 0, m->stream, g, m->f[GB25_U].d, m->f[GB25_V].d, m->f[GB25_W].d,
                       m->dpx.d, m->f[GB25_GN_U].d, nbx, nb);
  }
  {
    Timed t(m, GB25_K_GV);
    hipLaunchKernelGGL(k_gv, dim3(nb), b, 0, m->stream, g, m->f[GB25_U].d, m->f[GB25_V].d, m->f[GB25_W].d,
                       m->dpy.d, m->f[GB25_GN_V].d, nbx, nb);
  }
  LAUNCHCHK();
  return GB25_OK;
}
gb25_status tracers_impl(gb25_model* m) {
  const Grid& g = m->g;
  int nbx, nb;
  m->valid.tendency_kernel_runs(false);
  if (m->kernel_gen >= 2) {
    Timed t(m, GB25_K_TRACERS);
    const TracerPlan p = plan_tracers(launch_facts(m));
    const std::array<bool, TracerKernels::n> flags = tracer_flags(m, p.rows);
    const bool ahead = flags[0], fold = flags[2];
    Ab2Ahead nx{};
    if (ahead) {   // predicted parameters of the next ab2_step!: the clock's dt and the model's chi
      nx.GmT = m->f[GB25_GM_T].d; nx.GmS = m->f[GB25_GM_S].d;
      nx.Tn = m->ahead[0].d; nx.Sn = m->ahead[1].d;
      nx.dt = (real)m->last_dt;
      nx.C1 = real(1.5) + (real)m->cfg.chi; nx.C2 = real(0.5) + (real)m->cfg.chi;
    }
    const LazyCorr lz{m->corr[0].d, m->corr[1].d, m->wbase, m->g.sx * m->g.sy_v};
    if (m->route.memory_lacks_correction() && !(fold || m->slab))
      return fail(m, GB25_ERR_STATE, "internal: uncorrected velocities in a step whose tracer kernel cannot correct them");
    TracerKernels::kernel_t kern;
    if (gb25_status s_ = tendency_instance<TracerKernels>(m, flags, &kern)) return s_;
    const bool wcorr = m->route.tracer_kernel_corrects();
    if (wcorr) {
      if (!m->uvc[0].d) return fail(m, GB25_ERR_STATE, "internal: the corrected velocities have no arrays");
      nx.uc = m->uvc[0].d;
      nx.vc = m->uvc[1].d;
    }
    m->ahead_ts_folded = fold;
    hipLaunchKernelGGL(kern, dim3(p.nb), dim3(64, 4), 0, m->stream, g, m->f[GB25_U].d,
                       m->f[GB25_V].d, m->f[GB25_W].d, m->f[GB25_T].d, m->f[GB25_S].d, m->f[GB25_GN_T].d,
                       m->f[GB25_GN_S].d, p.nbx, p.kchunks, p.nb, nx, lz);
    LAUNCHCHK();
    m->valid.record_tracer_lookahead(ahead, nx.dt, (real)m->cfg.chi);
    if (wcorr) {
      // the arrays the kernel wrote ARE u, v from here on (the uncorrected ones become the scratch pair of the next step), and
      // their halo cells come from the ordinary fill -- y / z layers, the rows beyond a zipper fold, the periodic x copy
      m->route.tracer_kernel_wrote_corrected();
      for (int q = 0; q < 2; q++) std::swap(m->f[GB25_U + q].d, m->uvc[q].d);
      if (gb25_status s = fill_halos_impl(m, FillRequest::uv(Columns::OwnWithPeriodicX))) return s;
    }
    return GB25_OK;
  }
  m->valid.void_tracer_lookahead();   // only the packed kernel looks ahead
  if (m->immersed || g.cv.on) return fail(m, GB25_ERR_STATE, "the direct-stencil kernels (GB25_OPT_KERNELS = 1) know neither immersed boundaries nor curvilinear grids");
  if (g.top_flux[2] || g.top_flux[3]) return fail(m, GB25_ERR_STATE, "the direct-stencil kernels (GB25_OPT_KERNELS = 1) know no flux boundary conditions");
  tile_grid(g, &nbx, &nb);
  Timed t(m, GB25_K_TRACERS);
  hipLaunchKernelGGL(k_tracer_tendencies, dim3(nb), dim3(TX, TY), 0, m->stream, g, m->f[GB25_U].d, m->f[GB25_V].d,
                     m->f[GB25_W].d, m->f[GB25_T].d, m->f[GB25_S].d, m->f[GB25_GN_T].d, m->f[GB25_GN_S].d, nbx, nb);
  LAUNCHCHK();
  return GB25_OK;
}

gb25_status catke_implicit_impl(gb25_model* m, int mode, real dt, real chi = real(0.), int z0 = 0, int nz = -1);   // (with CATKE's diffusivity fields: below)
// implicit_step! of a pair of fields (kind 0: u, v with nu, the corrector's column integrals rewritten; 1: T, S with kappa)
gb25_status implicit_tables(gb25_model* m, int kind, double dt, double K) {
  if (m->d_implicit[kind] && m->implicit_key[kind][0] == dt && m->implicit_key[kind][1] == K) return GB25_OK;
  const int Nz = m->cfg.Nz, offk = m->metric_off_k;
  const std::vector<double>&dzc = m->h_metric[GB25_M_DZC], &dzf = m->h_metric[GB25_M_DZF];
  // (the spacings as the float type holds them; the chains in fp64, rounded once)
  auto Dc = [&](int k) { return (double)(real)dzc[offk + k]; };
  auto Df = [&](int k) { return (double)(real)dzf[offk + k]; };
  const double dK = (double)(real)dt * (double)(real)K;
  std::vector<real> tab((size_t)Nz + 2 * (size_t)Nz * Nz, real(0.));
  real *lo = tab.data(), *rb = lo + Nz, *gm = rb + (size_t)Nz * Nz;
  for (int k = 1; k < Nz; k++) lo[k] = (real)(-dK / (Dc(k) * Df(k)));
  for (int kf = 0; kf < Nz; kf++) {
    double bet = 1.0;
    for (int k = kf; k < Nz; k++) {
      const double l = k == kf ? 0.0 : -dK / (Dc(k) * Df(k)), u = k == Nz - 1 ? 0.0 : -dK / (Dc(k) * Df(k + 1));
      double gk = 0.0;
      if (k > kf) gk = (-dK / (Dc(k - 1) * Df(k))) / bet;
      bet = (1.0 - l - u) - l * gk;
      rb[(size_t)kf * Nz + k] = (real)(1.0 / bet);
      gm[(size_t)kf * Nz + k] = (real)gk;
    }
  }
  HIPCHK(hipStreamSynchronize(m->stream));   // (a solve with the old tables may still be running, on either stream)
  HIPCHK(hipStreamSynchronize(m->own_stream));
  HIPCHK(hipStreamSynchronize(m->side_stream));
  if (!m->d_implicit[kind]) HIPCHK(m->mem.alloc(&m->d_implicit[kind], tab.size() * sizeof(real)));
  HIPCHK(hipMemcpy(m->d_implicit[kind], tab.data(), tab.size() * sizeof(real), hipMemcpyHostToDevice));
  m->implicit_key[kind][0] = dt;
  m->implicit_key[kind][1] = K;
  return GB25_OK;
}
gb25_status implicit_vertical_impl(gb25_model* m, int kind, real dt) {
  const Grid& g = m->g;
  const real K = (real)(kind == 0 ? m->nu : m->kappa);
  if (K == real(0.)) return GB25_OK;
  Timed t_implicit(m, GB25_K_IMPLICIT);
  real *a = m->f[kind == 0 ? GB25_U : GB25_T].d, *b = m->f[kind == 0 ? GB25_V : GB25_S].d;
  real *sa = kind == 0 ? m->colsum[0].d : nullptr, *sb = kind == 0 ? m->colsum[1].d : nullptr;
  const int kchunks = mom_kchunks(m);
  if (g.Nz <= 128) {   // the column in registers, the elimination factors from tables
    if (gb25_status s = implicit_tables(m, kind, (double)dt, (double)K)) return s;
    ImplicitFields A{};
    const real* t = m->d_implicit[kind];
    for (int f = 0; f < 2; f++) {
      A.f[f] = f ? b : a;
      A.vshape[f] = kind == 0 && f == 1;
      A.first[f] = kind == 0 ? f : 2;
      A.lo[f] = t; A.rb[f] = t + g.Nz; A.gm[f] = t + g.Nz + (size_t)g.Nz * g.Nz;
      A.sum[f] = f ? sb : sa;
    }
    const bool imm = m->immersed;
    void (*kern)(Grid, ImplicitFields, int) =
        g.Nz <= 32 ? (imm ? k_implicit_vertical_reg<32, true> : k_implicit_vertical_reg<32, false>)
        : g.Nz <= 48 ? (imm ? k_implicit_vertical_reg<48, true> : k_implicit_vertical_reg<48, false>)
        : g.Nz <= 64 ? (imm ? k_implicit_vertical_reg<64, true> : k_implicit_vertical_reg<64, false>)
                     : (imm ? k_implicit_vertical_reg<128, true> : k_implicit_vertical_reg<128, false>);
    Timed tm(m, kind == 0 ? GB25_K_AB2_VELOCITIES : GB25_K_AB2_TRACERS);   // (accounted with the update it completes)
    dim3 b(64, 4);
    hipLaunchKernelGGL(kern, dim3((g.Nx + 63) / 64, ((kind == 0 ? v_rows(g) : g.Ny) + 3) / 4, 2), b, 0, m->stream, g, A, kchunks);
    LAUNCHCHK();
    if (kind == 0) m->valid.record_colsums();
    return GB25_OK;
  }
  // deeper columns: the column and the per-thread elimination factors in LDS
  int T = 256;
  auto lds_of = [&](int t) { return (size_t)(2 * t + 2) * g.Nz * sizeof(real); };
  while (T > 64 && lds_of(T) > 64 * 1024) T /= 2;
  if (lds_of(T) > 160 * 1024) T = 32;   // (half a wave per block before the solve is refused: Float64 fits 157 levels at 64 threads, 310 at 32)
  const size_t lds = lds_of(T);
  if (lds > 160 * 1024) return fail(m, GB25_ERR_INVALID_ARGUMENT, "the implicit vertical solve keeps a column in LDS: Nz = %d is too deep", g.Nz);
  auto kern = m->immersed ? k_implicit_vertical<true> : k_implicit_vertical<false>;
  // (a function attribute is set per device: the flag lives in the model, not in the process)
  if (lds > 64 * 1024 && !m->implicit_lds_raised[m->immersed ? 1 : 0]) {
    HIPCHK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    m->implicit_lds_raised[m->immersed ? 1 : 0] = true;
  }
  Timed tm(m, kind == 0 ? GB25_K_AB2_VELOCITIES : GB25_K_AB2_TRACERS);
  hipLaunchKernelGGL(kern, dim3((g.Nx + T - 1) / T, kind == 0 ? v_rows(g) : g.Ny, 2), dim3(T), lds, m->stream, g, a, b, kind, K, K,
                     dt, sa, sb, kchunks);
  LAUNCHCHK();
  if (kind == 0) m->valid.record_colsums();
  return GB25_OK;
}

// previous_velocities into their own fields (before anything writes the buffer they live in, and before the host looks)
gb25_status materialize_prev_uv(gb25_model* m) {
  if (m->prev_uv_src == 0 || !m->catke) return GB25_OK;
  for (int q = 0; q < 2; q++) {
    const real* src = m->prev_uv_src == 1 ? m->f[GB25_U + q].d : m->ahead_uv[q].d;
    HIPCHK(hipMemcpyAsync(m->f[GB25_PREV_U + q].d, src, m->f[GB25_U + q].elems() * sizeof(real), hipMemcpyDeviceToDevice, m->stream));
  }
  m->prev_uv_src = 0;
  return GB25_OK;
}
// Adoption of the sub-cycle look-ahead: eta, U, V and the filtered state of the step that begins were made beside the last tracer
// kernel; a pointer exchange on the host (time_step_impl; a slab: stage Update).  The velocities and T, S are adopted below.
void adopt_subcycle(gb25_model* m) {
  for (int q = 0; q < 3; q++) {
    std::swap(m->f[GB25_ETA + q].d, m->ahead_eta[q].d);
    std::swap(m->f[GB25_ETA_BAR + q].d, m->ahead_bar[q].d);
  }
  std::swap(m->bars, m->bars_ahead);
}
gb25_status ab2_velocities_impl(gb25_model* m, real dt, real chi) {
  const Grid& g = m->g;
  if (m->valid.velocities_adoptable(dt, chi)) {
    // the last momentum evaluation already advanced u and v with exactly these parameters: adopt its buffers
    // (closure = CATKE: the buffers given up hold the velocities of the last compute_diffusivities!: its previous_velocities)
    if (m->prev_uv_src == 2)
      if (gb25_status s_ = materialize_prev_uv(m)) return s_;
    if (m->prev_uv_src == 1) m->prev_uv_src = 2;
    for (int q = 0; q < 2; q++) {
      std::swap(m->f[GB25_U + q].d, m->ahead_uv[q].d);
      std::swap(m->f[GB25_GN_BT_U + q].d, m->ahead_G[q].d);
      std::swap(m->colsum[q].d, m->ahead_colsum[q].d);
    }
    m->valid.record_colsums();
    m->valid.void_velocity_lookahead_alone();
    if (m->catke) return catke_implicit_impl(m, 0, dt);
    return implicit_vertical_impl(m, 0, dt);
  }
  m->valid.void_velocity_lookahead_alone();
  if (m->prev_uv_src == 1)   // (u, v are about to be advanced in place)
    if (gb25_status s_ = materialize_prev_uv(m)) return s_;
  dim3 b(64, 4);
  Timed t(m, GB25_K_AB2_VELOCITIES);
  hipLaunchKernelGGL(k_ab2_velocities, grid2(g.Nx, v_rows(g), b), b, 0, m->stream, g, m->f[GB25_U].d, m->f[GB25_V].d,
                     m->f[GB25_GN_U].d, m->f[GB25_GM_U].d, m->f[GB25_GN_V].d, m->f[GB25_GM_V].d,
                     m->f[GB25_GN_BT_U].d, m->f[GB25_GN_BT_V].d, m->colsum[0].d, m->colsum[1].d, dt, chi,
                     mom_kchunks(m));   // the momentum kernel's chunking (momentum_impl)
  m->valid.record_colsums();
  LAUNCHCHK();
  if (m->catke) return catke_implicit_impl(m, 0, dt);
  return implicit_vertical_impl(m, 0, dt);
}
// the implicit solve of T, S (one elimination) with CATKE's kappa_c.  e is NOT stepped here: ab2_step! skips it, it is
// stepped inside compute_diffusivities! (catke_diffusivities_impl)
gb25_status catke_tracers_impl(gb25_model* m, real dt, real chi) { return catke_implicit_impl(m, 1, dt, chi); }
gb25_status ab2_tracers_impl(gb25_model* m, real dt, real chi) {
  const Grid& g = m->g;
  if (m->valid.tracers_adoptable(dt, chi)) {
    // the last tendency evaluation already advanced T and S with exactly these parameters
    std::swap(m->f[GB25_T].d, m->ahead[0].d);
    std::swap(m->f[GB25_S].d, m->ahead[1].d);
    m->valid.void_tracer_lookahead();
    if (m->catke) return catke_tracers_impl(m, dt, chi);
    return implicit_vertical_impl(m, 1, dt);
  }
  m->valid.void_tracer_lookahead();
  Timed t(m, GB25_K_AB2_TRACERS);
  const real C1 = real(1.5) + chi, C2 = real(0.5) + chi;
  size_t off = (size_t)g.H * g.pl_c;
  long n = (long)g.Nz * g.pl_c;
  real *T = m->f[GB25_T].d + off, *S = m->f[GB25_S].d + off;
  const real *a = m->f[GB25_GN_T].d + off, *bb = m->f[GB25_GM_T].d + off, *c = m->f[GB25_GN_S].d + off,
              *d = m->f[GB25_GM_S].d + off;
  bool aligned = (n % 4 == 0) && (((uintptr_t)T | (uintptr_t)S | (uintptr_t)a | (uintptr_t)bb | (uintptr_t)c |
                                   (uintptr_t)d) % sizeof(real4) == 0);
  if (aligned) {
    long n4 = n / 4;
    int blocks = (int)std::min<long>((n4 + 255) / 256, 256 * 16);
    // (nontemporal tendency reads: every byte of this stream is touched once per step)
    hipLaunchKernelGGL(k_ab2_tracers4<true>, dim3(blocks), dim3(256), 0, m->stream, (real4*)T, (real4*)S, (const real4*)a,
                       (const real4*)bb, (const real4*)c, (const real4*)d, n4, dt, C1, C2);
  } else {
    int blocks = (int)std::min<long>((n + 255) / 256, 256 * 16);
    hipLaunchKernelGGL(k_ab2_tracers1, dim3(blocks), dim3(256), 0, m->stream, T, S, a, bb, c, d, n, dt, C1, C2);
  }
  LAUNCHCHK();
  if (m->catke) return catke_tracers_impl(m, dt, chi);
  return implicit_vertical_impl(m, 1, dt);
}
gb25_status ab2_local_impl(gb25_model* m, real dt, real chi) {
  gb25_status s = ab2_velocities_impl(m, dt, chi);
  return s ? s : ab2_tracers_impl(m, dt, chi);
}

// step_free_surface!: Ns fused forward-backward substeps.  Single slab: canonical arrays, periodic x wrapped
// in-kernel.  Slab of a decomposition: wide-halo work arrays (halo W >= Ns filled once by the exchange of
// group 1), every substep computes on [-W+1, Nx+W-1) and the invalid rim never reaches the interior.
// ahead (single slab only): read eta, U, V where they are and G.U, G.V from the momentum look-ahead, write the new
// eta, U, V and the averages into the partner buffers.
// the image rows of the sub-cycle's tall work arrays (folded grid): pack the rows south of the pivot row / unpack into the rows
// beyond it.  A slab exchanges the buffer with its partner rank in between (slab_step.hpp, group 8); a single domain unpacks
// what it packed.
int64_t tall_buffer_elems(const gb25_model* m) { return (int64_t)5 * (m->Wy + 1) * (m->Nx + 2 * m->W); }
gb25_status tall_rows_impl(gb25_model* m, real* buf, bool pack) {
  const Grid& g = m->g;
  TallRows T{};
  for (int q = 0; q < 3; q++) T.p[q] = m->wide[0][q].d;
  T.p[3] = m->wideG[0].d;
  T.p[4] = m->wideG[1].d;
  T.sx = g.Nx + 2 * m->W; T.xo = m->W; T.yo = g.H + m->Wys; T.Wy = m->Wy; T.wrap = m->slab ? 0 : 1;
  const dim3 gr((T.sx + 255) / 256, m->Wy + 1, 5);
  if (pack) hipLaunchKernelGGL(k_tall_rows<true>, gr, dim3(256), 0, m->stream, g, T, buf, m->rx * g.Nx, m->cfg.Nx);
  else hipLaunchKernelGGL(k_tall_rows<false>, gr, dim3(256), 0, m->stream, g, T, buf, m->rx * g.Nx, m->cfg.Nx);
  LAUNCHCHK();
  return GB25_OK;
}

// ---- WHAT the sub-cycle runs is decided in one place, plan_subcycle (subcycle_plan.hpp; DESIGN.md, "The forms of the sub-cycle").
// barotropic_impl builds the plan's setting from the model, binds the model's buffers to the plan, and carries the plan out.

// the argument of k_copy_interior_columns, built piece by piece (up to five), and its launch
struct ColumnCopies {
  InteriorCopies C{};
  int rmax = 0;   // the most rows of any piece
  void add(real* dst, int dsx, int dxo, const real* src, int ssx, int sxo, int rows) {
    const int q = C.n++;
    C.dst[q] = dst; C.dsx[q] = dsx; C.dxo[q] = dxo;
    C.src[q] = src; C.ssx[q] = ssx; C.sxo[q] = sxo; C.rows[q] = rows;
    rmax = std::max(rmax, rows);
  }
  void launch(gb25_model* m, int rows) const {
    hipLaunchKernelGGL(k_copy_interior_columns, dim3((m->g.Nx + 255) / 256, rows, C.n), dim3(256), 0, m->stream, C, m->g.Nx);
  }
};
// the kernel instances of a form, in the order of SubcyclePlan::instance()
struct SubstepKernels {   // k_barotropic_substep<IMM, ORDER>
  using kernel_t = void (*)(Grid, Baro, real, real);
  static kernel_t at(int i) {
    static const kernel_t table[4] = {k_barotropic_substep<false, 0>, k_barotropic_substep<false, 1>,
                                      k_barotropic_substep<true, 0>, k_barotropic_substep<true, 1>};
    return table[i];
  }
};
struct BlockedKernels {   // k_barotropic_multi<S, TY, IMM>
  using kernel_t = void (*)(Grid, BaroMulti, real);
  static kernel_t at(int i) {
    static const kernel_t table[6] = {k_barotropic_multi<3, 16, false>, k_barotropic_multi<5, 17, false>, k_barotropic_multi<7, 16, false>,
                                      k_barotropic_multi<3, 16, true>, k_barotropic_multi<5, 17, true>, k_barotropic_multi<7, 16, true>};
    return table[i];
  }
};
struct WholeKernels {   // k_barotropic_whole<BW_NS, IMM, TY>
  using kernel_t = void (*)(Grid, BaroMulti, real);
  static kernel_t at(int i) {
    static const kernel_t table[4] = {k_barotropic_whole<BW_NS, false, 17>, k_barotropic_whole<BW_NS, false, 24>,
                                      k_barotropic_whole<BW_NS, true, 17>, k_barotropic_whole<BW_NS, true, 24>};
    return table[i];
  }
};

// own: (slab) the pieces of the interior columns of eta, U, V, G.U, G.V, which still sit in the canonical arrays
SubcycleSetting subcycle_setting(const gb25_model* m, bool ahead, const ColumnCopies* own) {
  const Grid& g = m->g;
  SubcycleSetting c{};
  c.Nx = g.Nx; c.Ny = g.Ny; c.H = g.H; c.W = m->W; c.Wy = m->Wy; c.Wys = m->Wys;
  c.slab = m->slab; c.curv = g.cv.on; c.north_fold = g.cv.north_fold; c.ys_open = m->ys_open; c.yn_open = m->yn_open;
  c.immersed = m->immersed;
  c.Ns = m->Ns;
  c.subcycle_block = m->baro_block; c.substep_order = m->substep_order; c.subcycle_whole = m->baro_whole;
  c.n_cu = m->n_cu; c.real_bytes = (int)sizeof(real);
  c.ahead = ahead; c.own_given = own != nullptr; c.own_five = own && own->C.n == 5;
  c.composite = m->composite; c.producers_fold = producers_fold(m);
  return c;
}

// the model's buffers in the roles of the plan, each chosen by the array set and by `ahead` (the look-ahead reads G.U, G.V of the
// momentum look-ahead and writes the partner buffers of eta, U, V and of the filtered state)
struct SubcycleBuffers {
  // eta, U, V: what the next launch reads and writes, the second scratch set, and where the results go.  The state the sub-cycle
  // starts from is only read; the launches alternate between two scratch sets
  real *cur[3], *nxt[3], *other[3], *out[3];
  real* bar[3];         // the running averages ...
  size_t bar_elems;     // (one allocation)
  Field* filtered[3];   // ... and the canonical filtered-state arrays (compared by compare_states), where the wide ones are published
  const real *GU, *GV, *Hfc, *Hcf;
  CurvBaro cb;
  void rotate() {
    for (int q = 0; q < 3; q++) { real* w_ = nxt[q]; nxt[q] = other[q]; other[q] = w_; cur[q] = w_; }
  }
  Baro baro(const SubcyclePlan& p) const {
    Baro b;
    b.eta0 = cur[0]; b.U0 = cur[1]; b.V0 = cur[2];
    b.eta1 = nxt[0]; b.U1 = nxt[1]; b.V1 = nxt[2];
    b.etab = bar[0]; b.Ub = bar[1]; b.Vb = bar[2];
    b.GU = GU; b.GV = GV; b.Hfc = Hfc; b.Hcf = Hcf;
    b.sx = p.sx; b.xo = p.xo; b.ilo = p.ilo; b.ihi = p.ihi; b.wrap = p.wrap;
    b.jlo = p.jlo; b.jhi = p.jhi; b.yo = p.yo; b.top_open = p.top_open;
    return b;
  }
};
SubcycleBuffers bind_subcycle(gb25_model* m, const SubcyclePlan& p, bool ahead) {
  const Grid& g = m->g;
  const bool wide = p.arrays == SubcycleArrays::Wide;
  SubcycleBuffers B{};
  for (int q = 0; q < 3; q++) {
    B.cur[q] = wide ? m->wide[0][q].d : m->f[GB25_ETA + q].d;
    B.nxt[q] = wide ? m->wide[1][q].d : m->pp[q].d;
    B.other[q] = wide ? m->wide[0][q].d : m->pp2[q].d;
    B.out[q] = ahead ? m->ahead_eta[q].d : m->f[GB25_ETA + q].d;
    B.filtered[q] = ahead ? &m->ahead_bar[q] : &m->f[GB25_ETA_BAR + q];
    B.bar[q] = wide ? m->wideBar[q].d : B.filtered[q]->d;
    B.bar_elems += wide ? m->wideBar[q].elems() : B.filtered[q]->elems();
  }
  B.GU = wide ? m->wideG[0].d : (ahead ? m->ahead_G[0].d : m->f[GB25_GN_BT_U].d);
  B.GV = wide ? m->wideG[1].d : (ahead ? m->ahead_G[1].d : m->f[GB25_GN_BT_V].d);
  B.Hfc = wide ? m->d_wideH[0] : m->d_H[0];
  B.Hcf = wide ? m->d_wideH[1] : m->d_H[1];
  B.cb = wide ? CurvBaro{m->d_wideM[0], m->d_wideM[1], m->d_wideM[2], m->d_wideM[3], m->d_wideM[4]}
              : CurvBaro{g.cv.dyfc, g.cv.dxcf, g.cv.razcc, g.cv.rdxfc, g.cv.rdycf};
  return B;
}

struct SubcycleDone {   // what barotropic_impl did (a failure has done neither)
  gb25_status status;
  bool halo_images_written;   // the last launch wrote every halo cell of the new eta, U, V: no fill for them in the step
  bool layers_written;        // the kernel wrote the y layers of the new eta, U, V: no fill after the sub-cycle of a slab
  SubcycleDone(gb25_status s, bool h = false, bool l = false) : status(s), halo_images_written(h), layers_written(l) {}
};
SubcycleDone barotropic_impl(gb25_model* m, real dt, bool ahead = false, const ColumnCopies* own = nullptr) {
  const Grid& g = m->g;
  if (m->baro_inflight && !ahead) {
    // a look-ahead that is not being adopted (changed dt, ...) may still be running on the side stream, and it uses
    // the same scratch sets
    HIPCHK(hipStreamWaitEvent(m->stream, m->ev_baro, 0));
    m->baro_inflight = false;
  }
  Timed t(m, GB25_K_BAROTROPIC);
  const SubcyclePlan p = plan_subcycle(subcycle_setting(m, ahead, own));
  SubcycleBuffers B = bind_subcycle(m, p, ahead);
  const real dtau = (real)m->dtau_frac * dt;
  // ---- before the kernels
  if (p.copy_state_in) {
    ColumnCopies C;
    for (int q = 0; q < 5; q++) {
      const Field& src = q < 3 ? m->f[GB25_ETA + q] : (ahead ? m->ahead_G[q - 3] : m->f[GB25_GN_BT_U + q - 3]);
      C.add(q < 3 ? m->wide[0][q].d : m->wideG[q - 3].d, p.sx, p.xo, src.d, g.sx, g.H, src.ny);
    }
    C.launch(m, C.rmax);
    gb25_status s;
    if ((s = tall_rows_impl(m, m->tall_buf, true))) return s;
    if ((s = tall_rows_impl(m, m->tall_buf, false))) return s;
  }
  if (p.zero_averages) HIPCHK(hipMemsetAsync(B.bar[0], 0, B.bar_elems * sizeof(real), m->stream));
  if (p.copy_own_first) own->launch(m, g.sy_v);
  // ---- the kernels
  auto multi = [&](int i) {
    const SubcycleLaunch L = p.launch(i);
    BaroMulti bm;
    bm.b = B.baro(p);
    for (int q = 0; q < BT_SMAX; q++) bm.w[q] = (L.s0 + q < m->Ns) ? (real)m->weights[L.s0 + q] : real(0.);
    bm.ns = L.ns; bm.first = L.first; bm.last = L.last;
    bm.eta_out = B.out[0]; bm.U_out = B.out[1]; bm.V_out = B.out[2];
    bm.eb_out = p.publish_through_eb_out ? B.filtered[0]->d : nullptr;
    bm.ub_out = p.publish_through_eb_out ? B.filtered[1]->d : nullptr;
    bm.vb_out = p.publish_through_eb_out ? B.filtered[2]->d : nullptr;
    bm.fold = (p.halo_images_on_last && L.last) ? 1 : 0;
    bm.out_halo = p.out_halo; bm.out_js = p.out_js; bm.out_jn = p.out_jn;
    for (int q = 0; q < 5; q++) bm.own_src[q] = p.own_in_place ? own->C.src[q] : nullptr;
    bm.layers = p.write_layers ? 1 : 0;
    return bm;
  };
  const dim3 grid(p.grid_x, p.grid_y), block(p.block_x, p.block_y);
  // (the attribute belongs to the DEVICE: kept per model, not per process -- a host driving several GPUs from one process, or
  // two threads, must not skip it on the second device)
  if (p.form == SubcycleForm::Whole && !m->whole_attr_set[p.instance()]) {
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(WholeKernels::at(p.instance())),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_bytes));
    m->whole_attr_set[p.instance()] = true;
  }
  for (int i = 0; i < p.n_launches; i++) {
    switch (p.form) {
      case SubcycleForm::PerSubstep:
        hipLaunchKernelGGL(SubstepKernels::at(p.instance()), grid, block, 0, m->stream, g, B.baro(p), dtau, (real)m->weights[i]);
        break;
      case SubcycleForm::PerSubstepCurv:
        hipLaunchKernelGGL(k_barotropic_substep_curv, grid, block, 0, m->stream, g, B.baro(p), B.cb, dtau, (real)m->weights[i]);
        break;
      case SubcycleForm::Blocked:
        hipLaunchKernelGGL(BlockedKernels::at(p.instance()), grid, block, 0, m->stream, g, multi(i), dtau);
        break;
      case SubcycleForm::BlockedCurv:
        hipLaunchKernelGGL((k_barotropic_multi_curv<5, 17>), grid, block, 0, m->stream, g, multi(i), B.cb, dtau);
        break;
      case SubcycleForm::Whole:
        hipLaunchKernelGGL(WholeKernels::at(p.instance()), grid, block, p.lds_bytes, m->stream, g, multi(i), dtau);
        break;
    }
    B.rotate();
  }
  // ---- after them (the last launch of several substeps wrote eta, U, V and published the averages itself)
  if (p.finalize_after) {
    const dim3 b(64, 4);
    hipLaunchKernelGGL(k_barotropic_finalize, grid2(p.fin_nx, p.fin_ny, b), b, 0, m->stream, g, B.out[0], B.out[1], B.out[2],
                       B.bar[0], B.bar[1], B.bar[2], p.sx, p.xo, p.fin_yo, p.out_halo, p.out_js, p.out_jn);
  }
  if (p.publish_after) {
    ColumnCopies C;
    for (int q = 0; q < 3; q++)
      C.add(B.filtered[q]->d, B.filtered[q]->nx, g.H, B.bar[q] + (size_t)m->Wys * p.sx, p.sx, p.xo, B.filtered[q]->ny);
    C.launch(m, C.rmax);
  }
  LAUNCHCHK();
  return {GB25_OK, p.halo_images_on_last, p.write_layers};
}

// cache_previous_tendencies!: G^- <- G^n is a pointer exchange; the next tendency evaluation overwrites the (old G^-) buffers
// that now carry the G^n name.  (closure = CATKE: G^-.e is written by the e step itself -- cache_previous_tendencies! skips e)
void cache_previous_tendencies(gb25_model* m) {
  for (int q = 0; q < 4; q++) std::swap(m->f[GB25_GN_U + q].d, m->f[GB25_GM_U + q].d);
  m->valid.void_lookaheads();   // the look-aheads used the tendency pairs as they were before
}
// the corrector inside its consumers: du, dv (k_corrector_2d) on the columns c, rows jr0 + [0, nj)
gb25_status corrector_2d_impl(gb25_model* m, dim3 b, Cols c, int jr0, int nj) {
  hipLaunchKernelGGL(m->immersed ? k_corrector_2d<true> : k_corrector_2d<false>, grid2(c.ni, nj, b), b, 0, m->stream, m->g,
                     m->f[GB25_BT_U].d, m->f[GB25_BT_V].d, m->colsum[0].d, m->colsum[1].d, m->f[GB25_U_BAR].d, m->f[GB25_V_BAR].d,
                     m->corr[0].d, m->corr[1].d, c.i0, c.ni, c.skip_from, c.skip, jr0, nj);
  LAUNCHCHK();
  return GB25_OK;
}
// w on the fly: w at the chunk boundaries (k_w_bases) on the columns c, rows -2 .. Ny + 1
gb25_status w_bases_impl(gb25_model* m, dim3 b, Cols c) {
  const Grid& g = m->g;
  auto kb = g.cv.on ? k_w_bases<true, true> : (m->immersed ? k_w_bases<true, false> : k_w_bases<false, false>);
  hipLaunchKernelGGL(kb, grid2(c.ni, g.Ny + 4, b), b, 0, m->stream, g, m->uv_partials, mom_kchunks(m), g.sx * g.sy_v,
                     LazyCorr{m->corr[0].d, m->corr[1].d, nullptr, 0}, m->wbase, c.i0, c.ni, c.skip_from, c.skip);
  LAUNCHCHK();
  return GB25_OK;
}

// The barotropic corrector on the columns the request names, in the form plan_corrector chooses (tendency_plan.hpp)
gb25_status corrector_impl(gb25_model* m, CorrectorRequest rq) {
  const Grid& g = m->g;
  {
    Timed t(m, GB25_K_CORRECTOR);
    const CorrectorPlan p = plan_corrector(rq, launch_facts(m), m->valid.colsum_valid, m->valid.halo_colsum_valid);
    if (p.form == CorrectorForm::Nothing) return GB25_OK;
    const dim3 b(64, 4);
    const Cols& c = p.cols;
    if (p.form == CorrectorForm::Cells) {
      hipLaunchKernelGGL(m->immersed ? k_corrector_cells<true> : k_corrector_cells<false>,
                         dim3((c.ni + 63) / 64, (p.nj + 3) / 4, g.Nz), b, 0, m->stream, g, m->f[GB25_U].d, m->f[GB25_V].d,
                         m->f[GB25_BT_U].d, m->f[GB25_BT_V].d, m->f[GB25_U_BAR].d, m->f[GB25_V_BAR].d, m->colsum[0].d,
                         m->colsum[1].d, c.i0, c.ni, c.skip_from, c.skip, p.j0, p.nj, INT_MAX, 0);
    } else {
      const bool fold = producers_fold(m) && m->composite, leaves = m->route.sweep_leaves_increments();
      auto kern = m->immersed ? (fold ? k_corrector<true, true> : k_corrector<true, false>)
                              : (fold ? k_corrector<false, true> : k_corrector<false, false>);
      hipLaunchKernelGGL(kern, grid2(c.ni, p.nj, b), b, 0, m->stream, g, m->f[GB25_U].d, m->f[GB25_V].d,
                         m->f[GB25_BT_U].d, m->f[GB25_BT_V].d, m->f[GB25_U_BAR].d, m->f[GB25_V_BAR].d,
                         p.reads_colsum ? m->colsum[0].d : nullptr, p.reads_colsum ? m->colsum[1].d : nullptr, c.i0, c.ni, mom_kchunks(m),
                         c.skip_from, c.skip, p.j0, p.nj, INT_MAX, 0, leaves ? m->corr[0].d : nullptr, leaves ? m->corr[1].d : nullptr);
    }
    LAUNCHCHK();
    if (!p.caches) return GB25_OK;
  }
  m->valid.void_colsums();
  cache_previous_tendencies(m);
  return GB25_OK;
}

// mask_immersed_model_fields! (src/precompile.jl:34): a sweep of its own only where the kernels of a composite step do
// not already guarantee the zeros (update_state!, initialize!, after host writes)
gb25_status mask_impl(gb25_model* m) {
  if (!m->immersed) return GB25_OK;
  Range r_mask(m, "mask_immersed_model_fields");   // (the wall faces of v are the halo fill's business on the plain grid)
  const Grid& g = m->g;
  dim3 b(64, 4);
  hipLaunchKernelGGL(k_mask_immersed, grid2(g.Nx, g.Ny + 1, b), b, 0, m->stream, g, m->f[GB25_U].d, m->f[GB25_V].d,
                     m->f[GB25_T].d, m->f[GB25_S].d, m->f[GB25_BT_U].d, m->f[GB25_BT_V].d);
  LAUNCHCHK();
  // the look-ahead partners of u, v, T, S hold the same zeros from the kernels' own masks; nothing else to do
  return GB25_OK;
}

// closure = CATKEVerticalDiffusivity(): what update_state! adds -- the advection of e (the two-wide tracer kernel with e in
// both halves: a first version, the second half is thrown away), the buoyancy field, J^b, then the diffusivity fields with
// their halo cells and the explicit TKE terms added to G^n.e.  After the tendencies of T, S (same stream).
CatkePar catke_parameters(const gb25_model* m) {
  const gb25_catke_parameters& p = m->catke_par;
  CatkePar c;
  c.Cs = (real)p.Cs; c.Cb = (real)p.Cb; c.Csp = (real)p.Csp; c.CRid = (real)p.CRid; c.CRi0 = (real)p.CRi0;
  for (int q = 0; q < 4; q++) {
    c.Chi[q] = (real)p.Chi[q]; c.Clo[q] = (real)p.Clo[q]; c.Cun[q] = (real)p.Cun[q]; c.Cc[q] = (real)p.Cc[q]; c.Ce[q] = (real)p.Ce[q];
  }
  c.CWu = (real)p.CWu; c.CWw = (real)p.CWw; c.emin = (real)p.minimum_tke; c.Jbmin = (real)p.minimum_convective_buoyancy_flux;
  c.tau_neg = (real)p.negative_tke_damping_time_scale;
  c.CWeps = (real)p.CWeps;
  c.rCRid = (real)(1.0 / p.CRid);
  c.rtau_neg = (real)(1.0 / p.negative_tke_damping_time_scale);
  return c;
}
// The extended range on which a rank of a decomposition COMPUTES N^2 and the diffusivities: the first halo column on either
// side, the first halo row of an open side and the row beyond a zipper fold (single domain: the interior, halos by images)
struct CatkeRange { int i_lo, i_hi, j_lo, j_hi; };
// chunks of levels of the CATKE column kernels: enough threads for ~10 waves per SIMD, at least 8 levels per chunk
inline int catke_level_chunks(const gb25_model* m, long columns) {
  int kch = 1;
  while (kch < 8 && columns * kch < 600000L && m->g.Nz / (kch + 1) >= 8) kch++;
  return kch;
}
inline CatkeRange catke_range(const gb25_model* m) {
  const Grid& g = m->g;
  CatkeRange r;
  r.i_lo = m->slab ? -1 : 0;
  r.i_hi = g.Nx + (m->slab ? 1 : 0);
  r.j_lo = m->ys_open ? -1 : 0;
  r.j_hi = g.Ny + ((m->yn_open || (m->slab && g.cv.north_fold)) ? 1 : 0);
  return r;
}
gb25_status catke_implicit_impl(gb25_model* m, int mode, real dt, real chi, int z0, int nz);
// compute_diffusivities!(diffusivities, closure::CATKE, model), first part: N^2 of the current T, S, the e step
// (time_step_catke_equation!: k_catke_tke_step + the implicit solve of e) on the own columns, J^b filtered.
// What follows needs the halos of e and J^b: catke_diffusivities_finish_impl.
gb25_status catke_tke_step_impl(gb25_model* m) {
  if (!m->catke) return GB25_OK;
  Timed t_closure(m, GB25_K_CLOSURE);
  const Grid& g = m->g;
  const CatkeRange r = catke_range(m);
  dim3 b(64, 4);
  {
    const int ni = r.i_hi - r.i_lo, nj = r.j_hi - r.j_lo;
    hipLaunchKernelGGL(m->immersed ? k_catke_n2<true> : k_catke_n2<false>, dim3((ni + 63) / 64, (nj + 3) / 4, g.Nz - 1), b, 0,
                       m->stream, g, m->f[GB25_T].d, m->f[GB25_S].d, m->catke_b.d, r.i_lo, r.j_lo, ni, nj);
  }
  // dt = clock.last_dt (finite from the model's construction on: GB-25 src/baroclinic_instability_model.jl:82), chi = 0.1 always
  const real dt = (real)m->last_dt, chi = (real)m->cfg.chi;
  const real* prev_uv[2];   // previous_velocities, wherever they are (prev_uv_src)
  for (int q = 0; q < 2; q++)
    prev_uv[q] = m->prev_uv_src == 1 ? m->f[GB25_U + q].d : m->prev_uv_src == 2 ? m->ahead_uv[q].d : m->f[GB25_PREV_U + q].d;
  // chunks of levels (catke_kernels.hpp): with fewer than ~600 k columns a thread per column leaves the chip short of waves
  const int kch = catke_level_chunks(m, (long)g.Nx * g.Ny);
  m->catke_e_star = kch > 1 ? m->catke_scratch.d : m->f[GB25_E].d;   // (where the implicit solve of e finds e*)
  dim3 gt = grid2(g.Nx, g.Ny, b);
  gt.z = kch;
  hipLaunchKernelGGL(m->immersed ? k_catke_tke_step<true> : k_catke_tke_step<false>, gt, b, 0, m->stream, g,
                     catke_parameters(m), dt, real(1.5) + chi, real(0.5) + chi, m->f[GB25_U].d, m->f[GB25_V].d,
                     prev_uv[0], prev_uv[1], m->f[GB25_E].d, m->catke_e_star, m->catke_b.d, m->f[GB25_JB].d,
                     m->f[GB25_KAPPA_U].d, m->f[GB25_KAPPA_C].d, m->f[GB25_KAPPA_E].d, m->f[GB25_LE].d, m->f[GB25_GN_E].d,
                     m->f[GB25_GM_E].d);
  LAUNCHCHK();
  if (gb25_status s = catke_implicit_impl(m, 1, dt, chi, 1, 1)) return s;   // (the e slice alone)
  // previous velocities <- velocities (parents).  Single domain with the look-ahead of u, v: nothing moves -- the next AB2 step
  // adopts the look-ahead's buffers and leaves these behind untouched, which is where the next compute_diffusivities! finds them
  // (prev_uv_src; 0.8 GB of copies per step at 1440x720x48 otherwise).  A rank of a decomposition, whose stages write the
  // partner buffers ahead of this one, and models without the look-ahead: D2D copies behind the kernel that read them.
  m->prev_uv_src = 1;
  if (m->slab || m->ab2_ahead != 1 || m->valid.ptr_exposed || !m->two_streams)
    if (gb25_status s_ = materialize_prev_uv(m)) return s_;
  const double dt_since = m->time - m->catke_prev_time;
  m->catke_prev_time = m->time;
  hipLaunchKernelGGL(m->immersed ? k_catke_surface_flux<true> : k_catke_surface_flux<false>, grid2(g.Nx, g.Ny, b), b, 0, m->stream,
                     g, catke_parameters(m), (real)dt_since, m->f[GB25_U].d, m->f[GB25_V].d, m->f[GB25_T].d, m->f[GB25_S].d,
                     m->f[GB25_E].d, m->catke_b.d, m->f[GB25_JB].d, m->catke_src.d);
  LAUNCHCHK();
  return GB25_OK;
}
// ... second part, once the halo cells of the new e (and, on a rank of a decomposition, of J^b) are in place: kappa_u, kappa_c,
// kappa_e with the halo cells their fill derives (a14).
gb25_status catke_diffusivities_finish_impl(gb25_model* m) {
  if (!m->catke) return GB25_OK;
  Timed t_closure(m, GB25_K_CLOSURE);
  const Grid& g = m->g;
  const CatkeRange r = catke_range(m);
  dim3 b(64, 4);
  dim3 gd = grid2(r.i_hi - r.i_lo, r.j_hi - r.j_lo, b);
  gd.z = catke_level_chunks(m, (long)(r.i_hi - r.i_lo) * (r.j_hi - r.j_lo));
  hipLaunchKernelGGL(m->immersed ? k_catke_diffusivities<true> : k_catke_diffusivities<false>,
                     gd, b, 0, m->stream, g, catke_parameters(m), m->f[GB25_U].d,
                     m->f[GB25_V].d, m->f[GB25_E].d, m->catke_b.d, m->f[GB25_JB].d, m->f[GB25_KAPPA_U].d,
                     m->f[GB25_KAPPA_C].d, m->f[GB25_KAPPA_E].d, r.i_lo, r.i_hi, r.j_lo, r.j_hi);
  if (g.cv.north_fold && !m->slab)   // the rows beyond the zipper
    hipLaunchKernelGGL(k_catke_fold, dim3((g.sx + 255) / 256, g.H, g.Nz + 3), dim3(256), 0, m->stream, g,
                       m->f[GB25_KAPPA_U].d, m->f[GB25_KAPPA_C].d, m->f[GB25_KAPPA_E].d, m->f[GB25_LE].d, m->f[GB25_JB].d);
  LAUNCHCHK();
  return GB25_OK;
}
// compute_diffusivities! on a single domain: the two parts with the halo fill of the new e between them (option
// CATKE_STALE_E_HALOS: without it -- Oceananigans as recalled; the bottom / top layers of e are never read)
gb25_status catke_diffusivities_impl(gb25_model* m) {
  if (!m->catke) return GB25_OK;
  gb25_status s;
  if ((s = catke_tke_step_impl(m))) return s;
  if (!m->catke_stale_e_halos && (s = fill_halos_impl(m, FillRequest::e(Columns::OwnWithPeriodicX)))) return s;
  return catke_diffusivities_finish_impl(m);
}
// what compute_tendencies! leaves in G^n.e: the SLOW tendency of e -- -div(u e) (one tracer, the two halves of the packed
// arithmetic on two columns of it: k_tracer_tendencies_single) and the top boundary condition of e (the surface TKE flux)
gb25_status catke_tendency_impl(gb25_model* m) {
  if (!m->catke) return GB25_OK;
  Timed t_closure(m, GB25_K_CLOSURE);
  const Grid& g = m->g;
  {
    const TracerPlan p = plan_single(launch_facts(m));
    SingleKernels::kernel_t kt;
    if (gb25_status s_ = tendency_instance<SingleKernels>(m, single_flags(m), &kt)) return s_;
    const LazyCorr lz{m->corr[0].d, m->corr[1].d, m->wbase, g.sx * g.sy_v};
    hipLaunchKernelGGL(kt, dim3(p.nb), dim3(64, 4), 0, m->stream, g, m->f[GB25_U].d, m->f[GB25_V].d, m->f[GB25_W].d, m->f[GB25_E].d,
                       m->f[GB25_GN_E].d, p.nbx, p.kchunks, p.nb, lz);
  }
  dim3 b(64, 4);
  hipLaunchKernelGGL(k_catke_add_top_source, grid2(g.Nx, g.Ny, b), b, 0, m->stream, g, m->catke_src.d, m->f[GB25_GN_E].d);
  LAUNCHCHK();
  return GB25_OK;
}
// single domain: compute_diffusivities! followed by the slow tendency of e (where update_state! has both at its end)
gb25_status catke_update_impl(gb25_model* m) {
  if (!m->catke) return GB25_OK;
  gb25_status s = catke_diffusivities_impl(m);
  return s ? s : catke_tendency_impl(m);
}
// implicit_step! with CATKE's diffusivity fields.  mode 0: u, v (and the corrector's column integrals); 1: slice 0 = T with S
// (ab2_step!), slice 1 = e (inside compute_diffusivities!: e holds e* already).  z0, nz: the slices of this launch
// (default: both of mode 0, slice 0 of mode 1)
gb25_status catke_implicit_impl(gb25_model* m, int mode, real dt, real chi, int z0, int nz) {
  if (nz < 0) nz = mode == 0 ? 2 : 1;
  const Grid& g = m->g;
  Timed t_implicit(m, GB25_K_IMPLICIT);
  ImplicitVarFields A{};
  A.f[0] = m->f[GB25_U].d; A.f[1] = m->f[GB25_V].d; A.f[2] = m->f[GB25_T].d; A.f[3] = m->f[GB25_S].d; A.f[4] = m->f[GB25_E].d;
  A.KU = m->f[GB25_KAPPA_U].d; A.KC = m->f[GB25_KAPPA_C].d; A.KE = m->f[GB25_KAPPA_E].d; A.Le = m->f[GB25_LE].d;
  A.dt = dt;
  A.GnE = A.GmE = nullptr;   // (e arrives with its AB2 update done: k_catke_tke_step)
  A.src_e = (mode == 1 && z0 == 1) ? m->catke_e_star : nullptr;   // (... in e itself, or in the scratch array when the step ran in chunks of levels)
  A.C1 = real(1.5) + chi; A.C2 = real(0.5) + chi;
  A.z0 = z0;
  A.sum[0] = mode == 0 ? m->colsum[0].d : nullptr;
  A.sum[1] = mode == 0 ? m->colsum[1].d : nullptr;
  A.kchunks = mom_kchunks(m);
  A.P = mode == 0 ? m->uv_partials : nullptr;   // (null without the look-ahead of u, v)
  A.plane2 = g.sx * g.sy_v;
  const bool imm = m->immersed;
  void (*kern)(Grid, ImplicitVarFields);
#define VARK(NZT) (mode == 0 ? (imm ? k_implicit_vertical_var<NZT, true, 0> : k_implicit_vertical_var<NZT, false, 0>) \
                             : (imm ? k_implicit_vertical_var<NZT, true, 1> : k_implicit_vertical_var<NZT, false, 1>))
  constexpr int REG_LEVELS = sizeof(real) == 8 ? 32 : 64;   // three per-thread arrays of that many values fit the VGPRs
  if (g.Nz <= 32) kern = VARK(32);
  else if (g.Nz <= 48 && REG_LEVELS >= 48) kern = VARK(48);
  else if (g.Nz <= 64 && REG_LEVELS >= 64) kern = VARK(64);
  else {   // deeper columns stream through HBM with the factors in two scratch arrays
    gb25_status s;
    for (int q = 0; q < 2; q++) {
      if (!m->catke_gam[q].d && (s = alloc_field(m, m->catke_gam[q], g.sx, g.sy_v, g.Nz + 2 * g.H))) return s;
      A.gam[q] = m->catke_gam[q].d;
    }
    kern = mode == 0 ? (imm ? k_implicit_vertical_var_stream<true, 0> : k_implicit_vertical_var_stream<false, 0>)
                     : (imm ? k_implicit_vertical_var_stream<true, 1> : k_implicit_vertical_var_stream<false, 1>);
  }
#undef VARK
  dim3 b(64, 4);
  const int rows = mode == 0 ? v_rows(g) : g.Ny;   // (with the zipper fold v has the fold line too)
  hipLaunchKernelGGL(kern, dim3((g.Nx + 63) / 64, (rows + 3) / 4, nz), b, 0, m->stream, g, A);
  LAUNCHCHK();
  if (mode == 0) m->valid.record_colsums();
  return GB25_OK;
}

// compute_atmosphere_ocean_fluxes! + the net ocean fluxes of ClimaOcean's OceanSeaIceModel (data-free forcing): similarity
// theory per surface cell, then the top flux boundary conditions of u, v, T, S (allocated here if the host set none)
gb25_status atmosphere_ocean_fluxes_impl(gb25_model* m) {
  if (!m->coupled) return GB25_OK;
  Timed t_fluxes(m, GB25_K_FLUXES);
  const Grid& g = m->g;
  const size_t n2 = (size_t)g.sx * g.sy_v;
  for (int q = 0; q < 4; q++) {
    if (!m->d_top_flux[q]) {
      HIPCHK(m->mem.alloc(&m->d_top_flux[q], n2 * sizeof(real)));
      m->top_flux_elems[q] = n2;
      HIPCHK(hipMemsetAsync(m->d_top_flux[q], 0, n2 * sizeof(real), m->stream));
    }
    m->g.top_flux[q] = m->d_top_flux[q];
  }
  for (int q = 0; q < 2; q++)
    if (!m->d_tau[q]) {
      HIPCHK(m->mem.alloc(&m->d_tau[q], n2 * sizeof(double)));
      HIPCHK(hipMemsetAsync(m->d_tau[q], 0, n2 * sizeof(double), m->stream));
    }
  Atmosphere A;
  for (int q = 0; q < 7; q++) A.a[q] = m->d_atm[q];
  const int j_hi = g.Ny;
  dim3 b(64, 4);
  hipLaunchKernelGGL(m->immersed ? k_similarity_fluxes<true> : k_similarity_fluxes<false>, grid2(g.Nx + 1, j_hi + 1, b), b, 0,
                     m->stream, m->g, A, m->f[GB25_U].d, m->f[GB25_V].d, m->f[GB25_T].d, m->f[GB25_S].d, m->d_tau[0],
                     m->d_tau[1], m->d_top_flux[2], m->d_top_flux[3], j_hi, 5);
  hipLaunchKernelGGL(k_stress_to_faces, grid2(g.Nx, j_hi, b), b, 0, m->stream, m->g, m->d_tau[0], m->d_tau[1],
                     m->d_top_flux[0], m->d_top_flux[1], j_hi);
  LAUNCHCHK();
  return GB25_OK;
}

gb25_status update_state_impl(gb25_model* m) {
  gb25_status s;
  if ((s = mask_impl(m))) return s;
  if ((s = fill_halos_impl(m, FillRequest::everything_periodic_x()))) return s;
  if (m->catke && (s = fill_halos_impl(m, FillRequest::e(Columns::OwnWithPeriodicX)))) return s;   // the TKE tracer
  if ((s = compute_w_impl(m))) return s;
  if ((s = compute_p_impl(m, PressureBox::whole(launch_facts(m))))) return s;
  // (compute_diffusivities! ahead of the tendencies, as update_state! has them: neither reads what the other writes, and the
  // e step must have read CATKE's previous velocities before the momentum kernel's look-ahead reuses their buffers)
  if ((s = catke_update_impl(m))) return s;
  if ((s = momentum_impl(m))) return s;
  return tracers_impl(m);
}

gb25_status ab2_step_impl(gb25_model* m, double dt, int euler) {
  gb25_status s;
  m->valid.void_subcycle_lookahead();   // this route always runs the sub-cycle itself
  const real chi = euler ? -real(0.5) : (real)m->cfg.chi;
  if ((s = ab2_local_impl(m, (real)dt, chi))) return s;
  Halo2 hG = halo2_G(m);
  if ((s = fill_halos_2d(m, hG))) return s;
  return barotropic_impl(m, (real)dt).status;
}

// u, v <- u + du, v + dv: ends the state in which the corrector lives inside its consumers (before a composite call returns)
// need_w = false: the step that follows carries w inside its tendency kernels as well (w on the fly beside the corrector's sweep):
// the field w stays stale
gb25_status materialize_uv(gb25_model* m, bool need_w = true) {
  if (m->route.memory_lacks_correction()) {
    const Grid& g = m->g;
    dim3 b(64, 4);
    hipLaunchKernelGGL(k_apply_correction, grid2(g.sx, g.sy_v, b), b, 0, m->stream, g, m->f[GB25_U].d, m->f[GB25_V].d,
                       LazyCorr{m->corr[0].d, m->corr[1].d, nullptr, 0});
    LAUNCHCHK();
  }
  // the steps behind carried w inside their tendency kernels: the field itself, from the corrected velocities
  const bool w_too = need_w && m->route.w_field_stale();
  m->route.materialized(w_too);
  return w_too ? compute_w_impl(m) : GB25_OK;
}
// What each route of a step requires ("Which kernel corrects u, v: the route of a step", one row per term).  The LAZY
// instances of the tendency kernels exist for the flat lat-lon grid; a single domain also needs look-aheads that write their halos
inline bool lazy_instances_ok(const gb25_model* m) {
  return m->lazy_corrector && !m->coupled && m->bottom_drag == 0 && m->tracer_order == 5 && m->two_streams && !m->immersed &&
         !m->g.cv.on && m->kernel_gen >= 2 && m->ab2_ahead == 1 && !m->valid.ptr_exposed && m->pressure_bits == 64;
}
inline bool lazy_corrector_ok(const gb25_model* m) { return lazy_instances_ok(m) && producers_fold(m); }
// w on the fly beside the corrector's sweep: every other grid of a single domain (the sweep leaves corrected velocities, so drag,
// fluxes and WENO(order = 7) are fine; not with a closure, whose implicit solve rewrites the chunk sums k_w_bases starts from)
inline bool wfly_sweep_ok(const gb25_model* m) {
  return m->w_fly && m->baro_ahead != 0 && !m->slab && m->two_streams && m->kernel_gen >= 2 &&
         m->ab2_ahead == 1 && !m->valid.ptr_exposed && m->nu == 0 && m->kappa == 0 && chunkings_match(m);
}
// ... and the sweep itself through the tracer kernel, first in the step (not with a closure: its kernels read u, v ahead of it)
inline bool lazy_through_tracers_ok(const gb25_model* m) {
  return m->lazy_corrector && wfly_sweep_ok(m) && !m->catke && !m->coupled && m->bottom_drag == 0 && m->tracer_order == 5 &&
         (m->immersed || m->g.cv.on) && m->tracers_first != 0 && m->pressure_bits == 64;
}
// a slab or a rank of a mesh: the LAZY instances without the halo images (du, dv of the halo columns / rows are computed locally)
inline bool slab_lazy_ok(const gb25_model* m) { return m->slab && lazy_instances_ok(m) && m->nu == 0 && m->kappa == 0 && !m->catke; }
inline bool slab_wfly_ok(const gb25_model* m) { return slab_lazy_ok(m) && m->w_fly && chunkings_match(m); }

// Which kernel corrects u, v this step: the one decision of a step (time_step_impl; stage 0 of a slab) and the only caller of the four
// _ok functions.  more: a step of a composite call (gb25_loop), which materialises u, v, w when it returns; uv_adopted, baro_adopted:
// the step adopted the velocity / the sub-cycle look-ahead
Corrector choose_corrector(const gb25_model* m, bool more, bool uv_adopted, bool baro_adopted) {
  if (m->slab)   // a slab asks for neither `more` nor complete_fills_needed == 0, and never takes ThroughTracers or SweepWFly
    return uv_adopted && baro_adopted && slab_lazy_ok(m) ? Corrector::InConsumers : Corrector::Sweep;
  if (!(more && uv_adopted && m->valid.complete_fills_needed == 0)) return Corrector::Sweep;
  if (baro_adopted && lazy_corrector_ok(m)) return Corrector::InConsumers;
  if (baro_adopted && lazy_through_tracers_ok(m)) return Corrector::ThroughTracers;
  if (wfly_sweep_ok(m)) return Corrector::SweepWFly;   // does not ask for baro_adopted: it asks for baro_ahead != 0 (wfly_sweep_ok)
  return Corrector::Sweep;
}
// ... and whether that step's tendency kernels carry w: in the consumers, a slab follows slab_wfly_ok, a single domain the option and
// the chunkings; the two other routes away from the plain sweep exist only with w on the fly
inline bool route_carries_w(const gb25_model* m, Corrector c) {
  if (c == Corrector::InConsumers) return m->slab ? slab_wfly_ok(m) : (m->w_fly && chunkings_match(m));
  return c != Corrector::Sweep;
}

// The head of a step whose corrector is not the sweep, as the request names it (HeadRequest, tendency_plan.hpp): du, dv, the chunk
// bases of w, G^- <- G^n.  An empty range (ni = 0) launches nothing; the column integrals are used up once du, dv of the OWN columns
// are made (a slab's halo columns skip them).  The timer is the caller's.
gb25_status unswept_head(gb25_model* m, const HeadRequest& rq) {
  gb25_status s;
  const dim3 b(rq.bx, rq.by);
  if (rq.cols.ni > 0) {
    if ((s = corrector_2d_impl(m, b, rq.cols, rq.j0, rq.nj))) return s;
    if (rq.cols.skip == 0) m->valid.void_colsums();
  }
  // (through the tracer kernel: memory lacks du, dv only until that kernel has run, and no other kernel reads u, v before it)
  if (!m->route.tracer_kernel_corrects()) m->route.correction_left_in_2d();
  if (rq.bases.ni > 0) {
    if ((s = w_bases_impl(m, b, rq.bases))) return s;
    m->route.w_carried_in_kernels();
  }
  if (rq.cache) cache_previous_tendencies(m);
  return GB25_OK;
}

// One time step on a single slab.  Two HIP streams: the tracer branch (AB2 of T,S -> their halos -> hydrostatic
// pressure: HBM- then fp64-bound) is independent of the velocity branch (AB2 of u,v -> split-explicit sub-cycle,
// which is latency-bound -> halos -> corrector -> halos -> w) until the tendencies need both, so it runs on a
// side stream and overlaps.  The phase order within each branch is the reference's (src/precompile.jl:31-42);
// T and S are untouched between the two halo fills of the reference sequence, so they are filled once.
gb25_status time_step_impl(gb25_model* m, int euler, bool more = false) {
  gb25_status s;
  const double dt = m->last_dt;
  struct Composite {
    gb25_model* m;
    explicit Composite(gb25_model* m_) : m(m_) { m->composite = true; }
    ~Composite() { m->composite = false; }
  } composite_scope(m);
  if (!m->two_streams) {
    if ((s = materialize_uv(m))) return s;
    if ((s = ab2_step_impl(m, dt, euler))) return s;
    m->time += dt;
    m->iteration += 1;
    if ((s = fill_halos_impl(m, FillRequest::everything_periodic_x()))) return s;
    if ((s = corrector_impl(m, CorrectorRequest::all(true)))) return s;
    if ((s = update_state_impl(m))) return s;
    return atmosphere_ocean_fluxes_impl(m);
  }
  const real chi = euler ? -real(0.5) : (real)m->cfg.chi;
  hipStream_t main = m->stream, side = m->side_stream;
  // ---- AB2 of u, v: normally the adoption of the look-ahead (a pointer exchange on the host, no kernel)
  const bool adopted = m->valid.velocities_adoptable((real)dt, chi);
  const bool baro_adopted = adopted && m->valid.ahead_baro_valid;   // (made from that very look-ahead, same dt)
  m->valid.void_subcycle_lookahead();
  // When everything this step needs was made ahead of time (u, v, the sub-cycle) and another step follows, no sweep over u and v:
  // a 2-D kernel leaves du, dv and the consumers add them, or the tracer kernel writes corrected arrays; or only w leaves the step
  const Corrector corrector = choose_corrector(m, more, adopted, baro_adopted);
  // (every route but the first expects corrected velocities in memory; the plain sweep the field w as well)
  if (corrector != Corrector::InConsumers && (s = materialize_uv(m, corrector == Corrector::Sweep))) return s;
  m->route.begin(corrector, route_carries_w(m, corrector));
  if ((s = ab2_velocities_impl(m, (real)dt, chi))) return s;
  Halo2 hG = halo2_G(m);
  // the sub-cycle reads G.U, G.V at interior points only (periodic wrap and walls are in the kernel): their halo
  // fill is for the state's sake and leaves the critical path when no kernel on this stream produced them
  if (!adopted && (s = fill_halos_2d(m, hG))) return s;
  const bool ts_adopted = m->valid.tracers_adoptable((real)dt, chi);
  // Everything the tracer branch reads was complete when the previous step's momentum kernel had finished (both
  // look-aheads adopted, the tracer kernel ran before the momentum kernel, no closure whose implicit solve sits in between):
  // the branch then starts behind THAT kernel -- beside this step's sub-cycle look-ahead, which is still in the queue of
  // the main stream -- and not behind everything the main stream holds.  (Not across the zipper fold: the fill of G.U, G.V
  // rewrites the eastern half of the fold line, which the sub-cycle reads.)
  const bool early_fork = m->valid.take_tend_forkable() && adopted && ts_adopted && !m->catke && m->nu == 0 && m->kappa == 0 &&
                          !m->coupled && !m->g.cv.north_fold;
  HIPCHK(hipEventRecord(m->ev_fork, main));
  HIPCHK(hipStreamWaitEvent(side, early_fork ? m->ev_tend : m->ev_fork, 0));
  // ---- tracer branch (side stream)
  // (complete fills for the two steps after a host write, one per buffer of each alternating pair: see fold_fills)
  const bool complete = m->valid.take_complete_fill();
  {
    OnStream on(m, side);
    if ((s = ab2_tracers_impl(m, (real)dt, chi))) return s;
    // y/z/x halos of T, S -- unless the look-ahead that was just adopted wrote them itself
    if ((complete || !(ts_adopted && m->ahead_ts_folded)) && (s = fill_halos_impl(m, FillRequest::ts(Columns::OwnWithPeriodicX)))) return s;
    // (closure = CATKE: e is not stepped by ab2_step!; its halos were refilled after its step inside compute_diffusivities! --
    // unless the option keeps them stale there, as Oceananigans does as recalled: then they are filled here, with the others)
    if (m->catke && m->catke_stale_e_halos && (s = fill_halos_impl(m, FillRequest::e(Columns::OwnWithPeriodicX)))) return s;
    HIPCHK(hipEventRecord(m->ev_ts, side));
    if ((s = compute_p_impl(m, PressureBox::whole(launch_facts(m)), true))) return s;
    if (adopted && (s = fill_halos_2d(m, hG))) return s;
  }
  HIPCHK(hipEventRecord(m->ev_join, side));
  // ---- velocity branch (main stream)
  bool eta_halos_fresh;   // the last launch of this step's sub-cycle wrote the halo cells of eta, U, V
  if (baro_adopted) {
    // the sub-cycle of this step ran in the previous one: adopt eta, U, V and the filtered state
    if (m->baro_inflight) HIPCHK(hipStreamWaitEvent(main, m->ev_baro, 0));
    m->baro_inflight = false;
    adopt_subcycle(m);
    eta_halos_fresh = m->ahead_eta_folded;
  } else {
    const SubcycleDone done = barotropic_impl(m, (real)dt);
    if (done.status) return done.status;
    eta_halos_fresh = done.halo_images_written;
  }
  m->time += dt;
  m->iteration += 1;
  // The reference fills the halos of u, v, eta, U, V here as well as after the corrector.  On a single slab the
  // corrector reads and writes its own columns only, and the fill after it rewrites exactly the same halo cells from
  // the corrected interior, so the first fill has no effect on any later value: it is left out (3 launches).
  const Grid& g = m->g;
  const LaunchFacts facts = launch_facts(m);
  switch (corrector) {
    case Corrector::InConsumers: {
      Timed t(m, GB25_K_CORRECTOR);
      if ((s = unswept_head(m, HeadRequest::in_consumers(facts, m->route.kernels_carry_w())))) return s;
      break;
    }
    case Corrector::ThroughTracers: {
      Timed t(m, GB25_K_CORRECTOR);
      for (int q = 0; q < 2; q++)
        if (!m->uvc[q].d && (s = alloc_field(m, m->uvc[q], m->f[GB25_U + q].nx, m->f[GB25_U + q].ny, m->f[GB25_U + q].nz))) return s;
      // du, dv on the own faces (rows of y faces: [0, Ny) on a folded grid, [0, Ny] below a wall) ...
      if ((s = unswept_head(m, HeadRequest::through_tracers_faces(facts)))) return s;
      // ... and their halo cells as the fills derive them (the rows beyond a zipper fold: images with the sign of a vector component)
      if (g.cv.north_fold) {
        Halo2 hc{};
        hc.p[0] = m->corr[0].d; hc.is_v[0] = 0; hc.xf[0] = 1; hc.neg[0] = 1;
        hc.p[1] = m->corr[1].d; hc.is_v[1] = 1; hc.xf[1] = 0; hc.neg[1] = 1;
        hc.n = 2;
        if ((s = fill_halos_2d(m, hc))) return s;
      }
      if ((s = unswept_head(m, HeadRequest::through_tracers_bases(facts)))) return s;
      // (the two strips of halo cells of the uncorrected u, v the tracer kernel reads: k_uncorrected_edges)
      hipLaunchKernelGGL(k_uncorrected_edges, dim3((std::max(g.Nx, g.Ny) + 255) / 256, g.Nz, g.cv.north_fold ? 3 : 2), dim3(256), 0, main, g,
                         m->f[GB25_U].d, m->f[GB25_V].d);
      LAUNCHCHK();
      cache_previous_tendencies(m);
      break;
    }
    case Corrector::SweepWFly:   // (the sweep leaves du, dv of the own columns behind for k_w_bases)
    case Corrector::Sweep:
      s = corrector_impl(m, CorrectorRequest::all(true));
      m->route.sweep_done();
      if (s) return s;
      if (corrector == Corrector::SweepWFly && (s = w_bases_impl(m, dim3(64, 4), wide_bases(facts)))) return s;
      if (corrector == Corrector::SweepWFly) m->route.w_carried_in_kernels();
      break;
  }
  {
    // u, v and eta, U, V -- whatever their last writers (the corrector, the sub-cycle's last launch) did not fill
    // (through the tracer kernel: u, v get their halo cells behind that kernel, which writes their corrected interior: tracers_impl)
    const bool unswept = corrector == Corrector::InConsumers || corrector == Corrector::ThroughTracers;
    const bool uv_fresh = unswept || (producers_fold(m) && m->composite && !complete);
    const FillRequest stale{uv_fresh ? Fields3::None : Fields3::UV, (eta_halos_fresh && !complete) ? Fields2::None : Fields2::Prognostic,
                            Columns::OwnWithPeriodicX};
    if (!stale.empty() && (s = fill_halos_impl(m, stale))) return s;
  }
  if (!m->route.kernels_carry_w() && (s = compute_w_impl(m))) return s;
  if (corrector == Corrector::ThroughTracers && !m->tracers_first) return fail(m, GB25_ERR_STATE, "internal: the corrector through the tracer kernel needs the tracer kernel first");
  // ---- join: the tendencies need w, u, v and T, S (the tracers) / the pressure differences (the momentum)
  const bool tracers_first = m->tracers_first != 0;
  if (m->catke) {   // compute_diffusivities! + the slow tendency of e, ahead of the tendency kernels (see update_state_impl)
    HIPCHK(hipStreamWaitEvent(main, m->ev_ts, 0));
    if ((s = catke_update_impl(m))) return s;
  }
  if (tracers_first) {
    HIPCHK(hipStreamWaitEvent(main, m->ev_ts, 0));
    if ((s = tracers_impl(m))) return s;
  }
  HIPCHK(hipStreamWaitEvent(main, m->ev_join, 0));
  if ((s = momentum_impl(m))) return s;
  if (tracers_first) {
    HIPCHK(hipEventRecord(m->ev_tend, main));
    m->valid.tendencies_forkable();
  }
  if (m->valid.velocities_ready(m->baro_ahead)) {
    // G.U, G.V of the next step exist now, and with them everything its split-explicit sub-cycle needs: it runs here,
    // into the partner buffers, and leaves the head of the next step (where the corrector waits for it).
    if (m->baro_ahead == 2) {
      // ... on a stream of its own beside the tracer tendency kernel.  (Measured on MI355X, profiles/r02b: the first of
      // its three launches is dispatched 7 us after the tracer kernel's 16 560 blocks and does not become resident until
      // they have drained -- 800 us instead of 60 -- so the "beside" is mostly an "after", and the other two launches
      // then compete with the next step's pressure kernel.  Kept as a schedule; not the default.)
      if (!m->baro_stream) HIPCHK(hipStreamCreateWithFlags(&m->baro_stream, hipStreamNonBlocking));
      HIPCHK(hipEventRecord(m->ev_mom, main));
      HIPCHK(hipStreamWaitEvent(m->baro_stream, m->ev_mom, 0));
      {
        OnStream on(m, m->baro_stream);
        const SubcycleDone done = barotropic_impl(m, m->valid.ahead_uv_dt, true);
        s = done.status;
        m->ahead_eta_folded = done.halo_images_written;
      }
      if (s) return s;
      HIPCHK(hipEventRecord(m->ev_baro, m->baro_stream));
      m->baro_inflight = true;
    } else {
      // ... on the main stream, between the momentum and the tracer tendencies: three launches of 60 us with the GPU to
      // themselves, no cross-stream dependency at all.
      const SubcycleDone done = barotropic_impl(m, m->valid.ahead_uv_dt, true);
      if (done.status) return done.status;
      m->ahead_eta_folded = done.halo_images_written;
    }
    m->valid.record_subcycle_lookahead();
  }
  if (!tracers_first && (s = tracers_impl(m))) return s;
  return atmosphere_ocean_fluxes_impl(m);   // (a coupled model: the fluxes the NEXT evaluation of the tendencies sees)
}
// a coupled model at iteration 0: the fluxes of the initial state, then the tendencies again, which now see them
gb25_status first_fluxes_impl(gb25_model* m) {
  if (!m->coupled) return GB25_OK;
  gb25_status s;
  if ((s = atmosphere_ocean_fluxes_impl(m))) return s;
  if ((s = catke_update_impl(m))) return s;
  if ((s = momentum_impl(m))) return s;
  return tracers_impl(m);
}

gb25_status initialize_impl(gb25_model* m) {
  const Grid& g = m->g;
  dim3 b(64, 4);
  hipLaunchKernelGGL(k_barotropic_mode, grid2(g.Nx, v_rows(g), b), b, 0, m->stream, g, m->f[GB25_U].d, m->f[GB25_V].d,
                     m->f[GB25_BT_U].d, m->f[GB25_BT_V].d);
  LAUNCHCHK();
  return fill_halos_2d(m, halo2_prognostic(m));
}

// The bottom tables from whatever the bottom currently is: the host's bottom height (gb25_set_bottom_height, global cell centres),
// the analytic mountains of grid_type, or nothing (flat: tables only where the kernels take everything from tables).
gb25_status rebuild_bottom(gb25_model* m) {
  const gb25_config& c = m->cfg;
  const bool islands = c.grid_type == GB25_GRID_LAT_LON_GAUSSIAN_ISLANDS || c.grid_type == GB25_GRID_TRIPOLAR_GAUSSIAN_ISLANDS;
  if (!m->host_bottom.empty() || islands || m->g.cv.on) {
    if (c.Nz > 254) return fail(m, GB25_ERR_INVALID_ARGUMENT, "an immersed boundary / a curvilinear grid needs Nz <= 254 (8-bit level tables)");
  }
  if (!m->host_bottom.empty()) {
    const int Nxg = c.Nx, i0 = m->rx * m->Nx;
    gb25_status s = build_bottom(m, [&](int i, int j) { return m->host_bottom[(size_t)((((i + i0) % Nxg) + Nxg) % Nxg) + (size_t)Nxg * j]; });
    if (s) return s;
    if (m->slab) m->immersed = true;   // (every slab of a decomposition runs the kernel variants its neighbours run)
    return GB25_OK;
  }
  if (islands) {
    if (!m->host_curv[0].empty())
      return fail(m, GB25_ERR_STATE, "grid_type = gaussian_islands places its mountains by the built-in generator's coordinates: "
                                     "with a host grid pass the bottom height too (gb25_set_bottom_height)");
    gb25_status s = build_bottom(m, [&](int i, int j) { return gaussian_islands_bottom(m, i, j); });
    m->immersed = true;   // (every slab of a decomposition runs the kernel variants the single domain runs, mountains or not)
    return s;
  }
  // the curvilinear kernels take every reconstruction order and mask from the tables (that is also where the fold's
  // "north is not a wall" lives): a flat bottom is a bottom nothing touches
  if (m->g.cv.on) return build_bottom(m, [&](int, int) { return -1e30; });
  return GB25_OK;
}
// everything in flight finishes and every look-ahead is void: the grid under the model is about to change
gb25_status quiesce_for_grid_change(gb25_model* m) {
  HIPCHK(hipStreamSynchronize(m->stream));
  HIPCHK(hipStreamSynchronize(m->own_stream));
  HIPCHK(hipStreamSynchronize(m->side_stream));
  if (m->baro_stream) HIPCHK(hipStreamSynchronize(m->baro_stream));
  m->valid.grid_changes();
  m->grid_print_valid = false;
  m->implicit_key[0][0] = m->implicit_key[1][0] = -1.0;   // (the elimination tables of a closure hold the old spacings)
  return GB25_OK;
}

}  // namespace

#include "slab_step.hpp"
#include "state_io.hpp"

// everything a model has in flight finishes (quiesce_for_grid_change and implicit_tables wait for stream lists of their own)
static gb25_status wait_for_model(gb25_model* m) {
  HIPCHK(hipStreamSynchronize(m->stream));
  HIPCHK(hipStreamSynchronize(m->side_stream));
  if (m->baro_stream) HIPCHK(hipStreamSynchronize(m->baro_stream));
  if (m->group) HIPCHK(m->group->sync_side());
  return GB25_OK;
}

namespace { void restart_release(gb25_model* m); }   // (restart_host.hpp)
namespace { void passive_release_all(gb25_model* m); }   // (passive_host.hpp)

// =============================================================================================
extern "C" {

const char* gb25_version(void) { return sizeof(real) == 8 ? "gb25hip 0.2 (gfx950, Float64)" : "gb25hip 0.2 (gfx950, Float32)"; }
int32_t gb25_real_bytes(void) { return (int32_t)sizeof(real); }
int32_t gb25_config_bytes(void) { return (int32_t)sizeof(gb25_config); }
int32_t gb25_catke_parameters_bytes(void) { return (int32_t)sizeof(gb25_catke_parameters); }

void gb25_default_config(gb25_config* c, int32_t Nx, int32_t Ny, int32_t Nz) {
  memset(c, 0, sizeof *c);
  c->Nx = Nx; c->Ny = Ny; c->Nz = Nz;
  c->halo = 8; c->substeps = 30; c->rank = 0; c->nranks = 1; c->device = 0;
  c->dt = 60.0; c->chi = 0.1;
  c->lat_south = -80; c->lat_north = 80; c->lon_west = 0; c->lon_east = 360;
  c->depth = 4000; c->zexp_h = 30;
  c->g = 9.80665; c->Omega = 7.292115e-5; c->radius = 6371e3; c->rho0 = 1020.0;
  c->slab_mode = 0; c->grid_type = GB25_GRID_LAT_LON; c->ranks_y = 1;
}

// What plan_layout decided, into the members that carry its names and into the options it has a default for: the one place
static void adopt_layout(gb25_model* m, const ModelLayout& L) {
  m->layout = L;
  m->Nx = L.Nx; m->Ny = L.Ny;
  m->Rx = L.Rx; m->Ry = L.Ry; m->rx = L.rx; m->ry = L.ry; m->j0 = L.j0;
  m->ys_open = L.ys_open; m->yn_open = L.yn_open; m->slab = L.slab;
  m->Ns = L.sub.Ns; m->dtau_frac = L.sub.dtau_frac; m->weights = L.sub.weights;
  m->W = L.W; m->Wy = L.Wy; m->Wys = L.Wys;
  m->tracer_rows_forced = L.tracer_rows_forced;
  // (gb25_set_option changes any of these defaults; nothing else is read from the environment)
  m->mom_chunk_levels = m->trc_chunk_levels = L.chunk_levels;
  m->baro_ahead = L.baro_ahead;
  m->split_tendencies = L.split_tendencies;
}

gb25_status gb25_create(const gb25_config* cfg, gb25_model** out) {
  if (!cfg || !out) return GB25_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  gb25_model* m = new gb25_model();
  gb25_default_catke_parameters(&m->catke_par);
  *out = m;  // returned even on failure so the caller can read the error string, then destroy
  m->cfg = *cfg;
  m->last_dt = cfg->dt;

  // ---- 1. plan, and refuse (model_layout.hpp): nothing of HIP, so a refused configuration allocates nothing
  {
    const LayoutPlan plan = plan_layout(*cfg, (int)sizeof(real), getenv("GB25_TRACER_ROWS"));
    if (plan.status) return fail(m, plan.status, "%s", plan.refusal.c_str());
    adopt_layout(m, plan.layout);
  }

  // ---- 2. the device, the streams, the events
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(m, GB25_ERR_NO_DEVICE, "no HIP device visible; libgb25hip has no CPU fallback");
  if (cfg->device < 0 || cfg->device >= ndev)
    return fail(m, GB25_ERR_INVALID_ARGUMENT, "device ordinal %d out of range (%d devices)", cfg->device, ndev);
  HIPCHK(hipSetDevice(cfg->device));
  {
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, cfg->device));
    m->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  }
  // (few streams on purpose: HIP multiplexes streams onto a handful of hardware queues, and two streams that share one
  // run in order -- a rocprof trace of eight slabs in one process, 25 streams, shows the exchange stream and the main
  // stream taking turns.  A slab has three: own, side, and the exchange stream of its context; the stream of
  // SUBCYCLE_LOOKAHEAD = 2 is created on demand.)
  for (hipStream_t* st : m->streams())
    if (st != &m->baro_stream) HIPCHK(hipStreamCreateWithFlags(st, hipStreamNonBlocking));
  for (hipEvent_t* ev : m->events()) HIPCHK(hipEventCreateWithFlags(ev, hipEventDisableTiming));
  m->stream = m->own_stream;

  // ---- 3. the grid's tables, then every array: each has the extents of a field (alloc_like: parent_dims) or of the sub-cycle's work
  // array that stands for one (wide_dims: W columns either side, Wy + Wys more rows).  The order of allocation is kept as it was.
  const ModelLayout& L = m->layout;
  gb25_status s;
  if ((s = build_grid(m))) return s;
  if ((s = build_eos_tables(m))) return s;
  if (cfg->grid_type >= GB25_GRID_LAT_LON_AS_CURVILINEAR && (s = build_curv_grid(m))) return s;
  for (int id = 0; id < GB25_FIELD_COUNT; id++) {
    if (id >= GB25_ETA_BAR && id <= GB25_V_BAR) continue;  // allocated contiguously below
    if (is_catke_field(id)) continue;   // (allocated when the closure is switched on)
    if ((s = alloc_like(m, m->f[id], id))) return s;
  }
  if ((s = alloc_three(m, &m->f[GB25_ETA_BAR], parent_dims, GB25_ETA_BAR, &m->bars))) return s;   // contiguous etabar | Ubar | Vbar
  for (int q = 0; q < 3; q++) {
    if ((s = alloc_like(m, m->pp[q], GB25_ETA + q))) return s;
    if ((s = alloc_like(m, m->pp2[q], GB25_ETA + q))) return s;
    if ((s = alloc_like(m, m->ahead_eta[q], GB25_ETA + q))) return s;
  }
  if ((s = alloc_three(m, m->ahead_bar, parent_dims, GB25_ETA_BAR, &m->bars_ahead))) return s;   // partners of the filtered state, laid out like `bars`
  if ((s = alloc_like(m, m->dpx, GB25_PHY))) return s;
  if ((s = alloc_like(m, m->dpy, GB25_PHY))) return s;
  for (int q = 0; q < 2; q++) {
    if ((s = alloc_like(m, m->ahead[q], GB25_T + q))) return s;
    if ((s = alloc_like(m, m->ahead_uv[q], GB25_U + q))) return s;
    if ((s = alloc_like(m, m->ahead_G[q], GB25_GN_BT_U + q))) return s;
    if ((s = alloc_like(m, m->ahead_colsum[q], GB25_BT_U + q))) return s;
  }
  HIPCHK(m->mem.alloc(&m->uv_partials, 4 * chunk_columns(L) * sizeof(real), true));
  HIPCHK(m->mem.alloc(&m->wbase, chunk_columns(L) * sizeof(real), true));
  if ((s = alloc_like(m, m->corr[0], GB25_BT_V))) return s;   // (du and dv: both with the row of a y-face field)
  if ((s = alloc_like(m, m->corr[1], GB25_BT_V))) return s;
  if ((s = alloc_like(m, m->colsum[0], GB25_BT_U))) return s;
  if ((s = alloc_like(m, m->colsum[1], GB25_BT_V))) return s;
  if (L.wide()) {
    for (int a = 0; a < 2; a++)
      for (int q = 0; q < 3; q++)
        if ((s = alloc_field(m, m->wide[a][q], wide_dims(L, GB25_ETA + q)))) return s;
    real* wide_bars = nullptr;   // the three running averages are one allocation, zeroed by one memset per step
    if ((s = alloc_three(m, m->wideBar, wide_dims, GB25_ETA, &wide_bars))) return s;
    if ((s = alloc_field(m, m->wideG[0], wide_dims(L, GB25_GN_BT_U)))) return s;
    if ((s = alloc_field(m, m->wideG[1], wide_dims(L, GB25_GN_BT_V)))) return s;
    if (m->g.cv.on && (s = build_curv_wide(m))) return s;
    if (L.Wy && !L.slab) HIPCHK(m->mem.alloc(&m->tall_buf, tall_buf_elems(L) * sizeof(real)));
  }
  if ((s = rebuild_bottom(m))) return s;
  HIPCHK(hipDeviceSynchronize());
  return GB25_OK;
}

void gb25_destroy(gb25_model* m) {
  if (!m) return;
  restart_release(m);
  passive_release_all(m);
  if (m->group) group_destroy(m->group);   // (the exchange context of every slab it holds)
  if (m->own_stream) hipStreamSynchronize(m->own_stream);
  m->diag.release();
  m->mem.release_all();
  resolve_profile(m);
  for (auto& ev : m->free_events) {
    hipEventDestroy(ev.a);
    hipEventDestroy(ev.b);
  }
  for (hipStream_t* st : m->streams())
    if (*st) {
      hipStreamSynchronize(*st);
      hipStreamDestroy(*st);
    }
  for (hipEvent_t* ev : m->events())
    if (*ev) hipEventDestroy(*ev);
  delete m;
}

const char* gb25_last_error_string(const gb25_model* m) { return m ? m->err.c_str() : "null model"; }

gb25_status gb25_set_stream(gb25_model* m, void* s) {
  CHECK_MODEL(m);
  if (m->group) return fail(m, GB25_ERR_STATE, "the slabs of an exchange context run on the context's own two streams");
  m->stream = (hipStream_t)s;  // NULL = HIP's default stream; ordering between streams is the caller's business
  return GB25_OK;
}
gb25_status gb25_use_own_stream(gb25_model* m) {
  CHECK_MODEL(m);
  if (m->group) return GB25_OK;
  HIPCHK(hipStreamSynchronize(m->stream));
  m->stream = m->own_stream;
  return GB25_OK;
}
gb25_status gb25_synchronize(gb25_model* m) {
  CHECK_MODEL(m);
  return wait_for_model(m);
}

gb25_status gb25_field_dims(const gb25_model* m, gb25_field id, int include_halos, int32_t d[3]) {
  if (!m || id < 0 || id >= GB25_FIELD_COUNT || !d) return GB25_ERR_INVALID_ARGUMENT;
  if (!m->f[id].d) return GB25_ERR_INVALID_ARGUMENT;   // (a field of CATKE on a model whose closure is not CATKE)
  // A y-face field of a folded grid has Ny rows ((Periodic, RightConnected, Bounded): the faces beyond the last row of cells are
  // halo cells), so its parent has Ny + 2H rows like a cell-centred one, likewise below a northern neighbour rank; the device
  // arrays keep the row a Bounded grid needs (host_dims and parent_dims, model_layout.hpp).
  const Dims h = host_dims(m->layout, id, include_halos != 0);
  d[0] = h.nx; d[1] = h.ny; d[2] = h.nz;
  return GB25_OK;
}

static gb25_status copy_field(gb25_model* m, gb25_field id, real* host, int include_halos, bool to_device) {
  if (!m || id < 0 || id >= GB25_FIELD_COUNT || !host) return GB25_ERR_INVALID_ARGUMENT;
  if (!m->f[id].d) return fail(m, GB25_ERR_INVALID_ARGUMENT, "this model has no such field (closure = CATKEVerticalDiffusivity() only)");
  if (to_device && (id == GB25_U || id == GB25_V)) m->valid.void_colsums();  // cached column integrals are stale
  if (m->route.memory_lacks_correction())   // (only after a composite call that failed half-way: memory must hold the corrected velocities)
    if (gb25_status s = materialize_uv(m)) return s;
  if (gb25_status s = materialize_prev_uv(m)) return s;   // (CATKE's previous velocities into their fields before the host reads or writes)
  Field& F = m->f[id];
  if (!to_device) HIPCHK(hipStreamSynchronize(m->stream));
  else if (gb25_status s = wait_for_model(m)) return s;   // a look-ahead may still be reading the old values
  int32_t d[3];
  gb25_field_dims(m, id, include_halos, d);
  if (include_halos && d[1] == F.ny) {
    if (to_device) HIPCHK(hipMemcpy(F.d, host, F.elems() * sizeof(real), hipMemcpyHostToDevice));
    else HIPCHK(hipMemcpy(host, F.d, F.elems() * sizeof(real), hipMemcpyDeviceToHost));
    return GB25_OK;
  }
  const Dims skip = include_halos ? Dims{0, 0, 0} : halo_depth(m->layout, id);
  hipMemcpy3DParms p = {};
  hipPitchedPtr dev = make_hipPitchedPtr(F.d, (size_t)F.nx * sizeof(real), F.nx, F.ny);
  hipPitchedPtr hst = make_hipPitchedPtr(host, (size_t)d[0] * sizeof(real), d[0], d[1]);
  hipPos dpos = make_hipPos((size_t)skip.nx * sizeof(real), skip.ny, skip.nz), zero = make_hipPos(0, 0, 0);
  p.extent = make_hipExtent((size_t)d[0] * sizeof(real), d[1], d[2]);
  if (to_device) {
    p.srcPtr = hst; p.srcPos = zero; p.dstPtr = dev; p.dstPos = dpos; p.kind = hipMemcpyHostToDevice;
  } else {
    p.srcPtr = dev; p.srcPos = dpos; p.dstPtr = hst; p.dstPos = zero; p.kind = hipMemcpyDeviceToHost;
  }
  HIPCHK(hipMemcpy3D(&p));
  return GB25_OK;
}
static gb25_status widen_phy(gb25_model* m) {   // the host uploaded pHY': rebuild the differences from it
  long n = (long)m->f[GB25_PHY].elems();
  hipLaunchKernelGGL(k_pressure_differences, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, m->stream, m->g,
                     m->f[GB25_PHY].d, m->dpx.d, m->dpy.d, n);
  LAUNCHCHK();
  return GB25_OK;
}
// T and S alternate between two buffers (AB2 look-ahead).  Whatever the host writes into one, halos included, goes
// into the partner too, so that the halo layers no kernel ever rewrites are the same in both.
static gb25_status mirror_tracers(gb25_model* m) {
  m->valid.void_tracer_lookahead();
  m->valid.complete_fills_owed();
  for (int q = 0; q < 2; q++)
    HIPCHK(hipMemcpyAsync(m->ahead[q].d, m->f[GB25_T + q].d, m->f[GB25_T + q].elems() * sizeof(real),
                          hipMemcpyDeviceToDevice, m->stream));
  return GB25_OK;
}
static gb25_status mirror_velocities(gb25_model* m) {   // u and v alternate between two buffers likewise
  m->valid.void_velocity_lookahead_alone();
  m->valid.complete_fills_owed();
  for (int q = 0; q < 2; q++)
    HIPCHK(hipMemcpyAsync(m->ahead_uv[q].d, m->f[GB25_U + q].d, m->f[GB25_U + q].elems() * sizeof(real),
                          hipMemcpyDeviceToDevice, m->stream));
  return GB25_OK;
}
gb25_status gb25_set_field(gb25_model* m, gb25_field f, const void* host, int include_halos) {
  CHECK_MODEL(m);
  gb25_status s = collective_guard(m, 1, (unsigned)f, 0.0);
  if (s) return s;
  s = copy_field(m, f, static_cast<real*>(const_cast<void*>(host)), include_halos, true);
  if (s == GB25_OK && f == GB25_PHY) {
    m->phy_stale = false;
    s = widen_phy(m);
  }
  if (s == GB25_OK && m->immersed && (f == GB25_U || f == GB25_V || f == GB25_T || f == GB25_S || f == GB25_BT_U || f == GB25_BT_V))
    s = mask_impl(m);   // set!(model, ...) masks what it has set (as Oceananigans' set! does on an immersed grid)
  if (s == GB25_OK) {
    m->valid.void_lookaheads();   // any input of the look-aheads may have changed
    m->valid.complete_fills_owed();
    if (f == GB25_T || f == GB25_S) s = mirror_tracers(m);
    if (f == GB25_U || f == GB25_V) s = mirror_velocities(m);
    if (s == GB25_OK && f >= GB25_ETA && f <= GB25_V_BAR) {   // eta, U, V and the filtered state alternate likewise
      Field& P = (f <= GB25_BT_V) ? m->ahead_eta[f - GB25_ETA] : m->ahead_bar[f - GB25_ETA_BAR];
      HIPCHK(hipMemcpyAsync(P.d, m->f[f].d, m->f[f].elems() * sizeof(real), hipMemcpyDeviceToDevice, m->stream));
    }
  }
  return s;
}
gb25_status gb25_get_field(gb25_model* m, gb25_field f, void* host_, int include_halos) {
  real* host = static_cast<real*>(host_);
  if (m && f == GB25_PHY && m->phy_stale) {   // the step stored only the differences: T, S are those it was made from
    gb25_status s = compute_p_impl(m, PressureBox::whole(launch_facts(m)));
    if (s) return s;
  }
  return copy_field(m, f, host, include_halos, false);
}
gb25_status gb25_field_device_ptr(gb25_model* m, gb25_field id, void** dev) {
  if (!m || id < 0 || id >= GB25_FIELD_COUNT || !dev) return GB25_ERR_INVALID_ARGUMENT;
  if (!m->f[id].d) return fail(m, GB25_ERR_INVALID_ARGUMENT, "this model has no such field (closure = CATKEVerticalDiffusivity() only)");
  if (gb25_status s = collective_guard(m, 2, (unsigned)id, 0.0)) return s;
  if (m->route.memory_lacks_correction())
    if (gb25_status s = materialize_uv(m)) return s;
  if (gb25_status s = materialize_prev_uv(m)) return s;
  if (id == GB25_U || id == GB25_V || id == GB25_T || id == GB25_S || (id >= GB25_GN_U && id <= GB25_GM_S) ||
      (id >= GB25_ETA && id <= GB25_GN_BT_V)) {
    // the host can now write prognostic fields or their tendencies behind our back: no more look-ahead for this
    // model, u, v, T, S stay in the buffers whose addresses are handed out
    m->valid.pointer_handed_out();
  }
  if (id == GB25_PHY) {
    m->phy_pinned = true;
    if (m->phy_stale) {
      gb25_status s = compute_p_impl(m, PressureBox::whole(launch_facts(m)));
      if (s) return s;
    }
  }
  *dev = m->f[id].d;
  return GB25_OK;
}
gb25_status gb25_get_metric(const gb25_model* m, gb25_metric id, int32_t logical_index, double* v) {
  if (!m || id < 0 || id > GB25_M_DY || !v) return GB25_ERR_INVALID_ARGUMENT;
  if (id == GB25_M_DY) {   // (one number: the spacing of a regular latitude grid)
    *v = (double)m->g.dy;
    return GB25_OK;
  }
  int off = (id <= GB25_M_FCOR) ? m->metric_off_j : m->metric_off_k;
  long a = (long)logical_index - 1 + off;  // logical_index is 1-based like the Julia sources
  if (a < 0 || a >= (long)m->h_metric[id].size()) return GB25_ERR_INVALID_ARGUMENT;
  *v = (double)(real)m->h_metric[id][a];
  return GB25_OK;
}
gb25_status gb25_get_metric2(const gb25_model* m, gb25_metric2 id, double* v, int64_t count) {
  if (!m || id < 0 || id >= GB25_M2_COUNT || !v) return GB25_ERR_INVALID_ARGUMENT;
  const std::vector<double>& a = m->h_curv[id];
  if (a.empty() || count != (int64_t)a.size()) return GB25_ERR_INVALID_ARGUMENT;   // (not a curvilinear grid, or a wrong size)
  for (size_t q = 0; q < a.size(); q++) v[q] = (double)(real)a[q];
  return GB25_OK;
}
gb25_status gb25_get_substepping(const gb25_model* m, int32_t* n, double* frac, double* w) {
  if (!m) return GB25_ERR_INVALID_ARGUMENT;
  if (n) *n = m->Ns;
  if (frac) *frac = m->dtau_frac;
  if (w) for (int k = 0; k < m->Ns; k++) w[k] = (double)(real)m->weights[k];
  return GB25_OK;
}

gb25_status gb25_set_baroclinic_instability(gb25_model* m) {
  CHECK_MODEL(m);
  if (gb25_status s = collective_guard(m, 3, 0, 0.0)) return s;
  const Grid& g = m->g;
  hipLaunchKernelGGL(k_set_baroclinic_instability, dim3((g.Nx + 255) / 256, g.Ny, g.Nz), dim3(256), 0, m->stream, g,
                     m->f[GB25_T].d, m->f[GB25_S].d);
  LAUNCHCHK();
  if (gb25_status s = mask_impl(m)) return s;
  return mirror_tracers(m);
}

gb25_status gb25_get_clock(const gb25_model* m, double* time, int64_t* it, double* last_dt) {
  if (!m) return GB25_ERR_INVALID_ARGUMENT;
  if (time) *time = m->time;
  if (it) *it = m->iteration;
  if (last_dt) *last_dt = m->last_dt;
  return GB25_OK;
}
gb25_status gb25_set_dt(gb25_model* m, double dt) {
  CHECK_MODEL(m);
  if (gb25_status s = collective_guard(m, 4, 0, dt)) return s;
  m->last_dt = dt;
  return GB25_OK;
}

// closure = VerticalScalarDiffusivity(VerticallyImplicitTimeDiscretization(), kappa, nu) (src/baroclinic_instability_model.jl:
// 31); nu = kappa = 0 is closure = nothing.  Collective on a decomposed model.
gb25_status gb25_set_vertical_diffusivity(gb25_model* m, double nu, double kappa) {
  CHECK_MODEL(m);
  if (!(nu >= 0) || !(kappa >= 0)) return fail(m, GB25_ERR_INVALID_ARGUMENT, "viscosity and diffusivity must be >= 0");
  if ((nu != 0 || kappa != 0) && !m->tracer_sets.empty())
    return fail(m, GB25_ERR_STATE, "gb25_set_vertical_diffusivity: %zu set(s) of passive tracers are open, and they are built for closure = nothing "
                "(gb25_tracers_end first)", m->tracer_sets.size());
  if (gb25_status s = collective_guard(m, 7, 0, nu)) return s;
  if (gb25_status s = collective_guard(m, 7, 1, kappa)) return s;
  m->nu = nu;
  m->kappa = kappa;
  m->valid.void_tracer_lookahead();   // (a look-ahead of T, S written with its halos predates the solve)
  if (!m->slab) m->valid.complete_fills_owed();
  return GB25_OK;
}
gb25_status gb25_set_closure_catke(gb25_model* m, int32_t on) {
  CHECK_MODEL(m);
  if (gb25_status s = collective_guard(m, 8, (unsigned)(on != 0), 0.0)) return s;
  if (on && (m->nu != 0 || m->kappa != 0)) return fail(m, GB25_ERR_STATE, "one closure at a time: the vertical diffusivity is set");
  if (on && !m->tracer_sets.empty())
    return fail(m, GB25_ERR_STATE, "gb25_set_closure_catke: %zu set(s) of passive tracers are open, and they are built for closure = nothing "
                "(gb25_tracers_end first)", m->tracer_sets.size());
  if (on && m->cfg.Nz < 2) return fail(m, GB25_ERR_INVALID_ARGUMENT, "CATKE needs at least two levels (it lives on the faces between them)");
  if (gb25_status s = wait_for_model(m)) return s;
  if (on && !m->f[GB25_E].d) {
    gb25_status s;
    for (int id = 0; id < GB25_FIELD_COUNT; id++)
      if (is_catke_field(id) && (s = alloc_like(m, m->f[id], id))) return s;
    if ((s = alloc_like(m, m->catke_b, GB25_E))) return s;
    if ((s = alloc_like(m, m->catke_src, GB25_JB))) return s;
    if ((s = alloc_like(m, m->catke_scratch, GB25_E))) return s;
  }
  if (gb25_status s_ = materialize_prev_uv(m)) return s_;   // (while the closure still says where they are)
  m->catke = on != 0;
  m->valid.void_tracer_lookahead();
  m->valid.complete_fills_owed();
  return GB25_OK;
}
void gb25_default_catke_parameters(gb25_catke_parameters* p) {
  if (!p) return;
  const double hi[4] = {0.242, 0.098, 0.548, 0.579}, lo[4] = {0.361, 0.198, 7.863, 1.604}, un[4] = {0.370, 0.369, 1.447, 0.923};
  const double cc[4] = {3.705, 4.793, 3.642, 3.254}, ce[4] = {0.0, 0.112, 0.0, 0.0};
  p->Cs = 1.131; p->Cb = 0.28; p->Csp = 0.505; p->CRid = 1.02; p->CRi0 = 0.254;
  for (int q = 0; q < 4; q++) { p->Chi[q] = hi[q]; p->Clo[q] = lo[q]; p->Cun[q] = un[q]; p->Cc[q] = cc[q]; p->Ce[q] = ce[q]; }
  p->CWu = 3.179; p->CWw = 0.383;
  p->minimum_tke = 1e-9; p->minimum_convective_buoyancy_flux = 1e-11; p->negative_tke_damping_time_scale = 60.0;
  p->CWeps = 1.0;
}
gb25_status gb25_set_catke_parameters(gb25_model* m, const gb25_catke_parameters* p) {
  CHECK_MODEL(m);
  if (!p) return GB25_ERR_INVALID_ARGUMENT;
  if (!(p->CRid > 0) || !(p->negative_tke_damping_time_scale > 0) || !(p->minimum_convective_buoyancy_flux > 0) || !(p->minimum_tke > 0))
    return fail(m, GB25_ERR_INVALID_ARGUMENT, "CATKE parameters: CRid, the damping time scale, the minimum convective buoyancy flux and the minimum TKE must be positive");
  if (gb25_status s = collective_guard(m, 10, 0, p->Cb)) return s;
  m->catke_par = *p;
  m->valid.void_lookaheads();
  return GB25_OK;
}
gb25_status gb25_get_catke_parameters(const gb25_model* m, gb25_catke_parameters* p) {
  if (!m || !p) return GB25_ERR_INVALID_ARGUMENT;
  *p = m->catke_par;
  return GB25_OK;
}
gb25_status gb25_get_vertical_diffusivity(const gb25_model* m, double* nu, double* kappa) {
  if (!m || !nu || !kappa) return GB25_ERR_INVALID_ARGUMENT;
  *nu = m->nu;
  *kappa = m->kappa;
  return GB25_OK;
}

gb25_status gb25_initialize(gb25_model* m) { CHECK_MODEL(m); return initialize_impl(m); }
gb25_status gb25_mask_immersed_fields(gb25_model* m) {
  CHECK_MODEL(m);
  gb25_status s = mask_impl(m);
  if (s == GB25_OK && m->immersed) {   // the partner buffers of the look-aheads follow
    m->valid.void_lookaheads();
    if ((s = mirror_tracers(m))) return s;
    s = mirror_velocities(m);
  }
  return s;
}
// GridFittedBottom(bottom_height): bottom height (metres, negative down) at the centres of the interior columns,
// Nx x Ny doubles, i fastest.  Single-domain models only (a slab would need its neighbours' columns: decomposed
// models take an analytic grid_type).  Fields are masked at once.
gb25_status gb25_set_bottom_height(gb25_model* m, const double* zb) {
  CHECK_MODEL(m);
  if (!zb) return GB25_ERR_INVALID_ARGUMENT;
  if (gb25_status s = collective_guard(m, 7, 0, zb[0])) return s;   // (synchronises the exchange stream of a decomposed model)
  if (gb25_status s = quiesce_for_grid_change(m)) return s;
  if (m->group) HIPCHK(m->group->sync_side());
  m->host_bottom.assign(zb, zb + (size_t)m->cfg.Nx * m->cfg.Ny);   // GLOBAL cell centres (a slab picks its columns, its
  gb25_status s = rebuild_bottom(m);                                 // neighbours' and its fold partner's)
  if (s) return s;
  if (m->kernel_gen == 1 && m->immersed) m->kernel_gen = 2;
  return m->slab ? mask_impl(m) : gb25_mask_immersed_fields(m);
}
// ---- the host's horizontal grid
gb25_status gb25_set_curvilinear_grid(gb25_model* m, const double* const* metrics, int32_t nx, int32_t ny) {
  CHECK_MODEL(m);
  const gb25_config& c = m->cfg;
  const int H = c.halo, gsx = c.Nx + 2 * H, gsy = c.Ny + 2 * H + 1;
  if (!m->g.cv.on)
    return fail(m, GB25_ERR_STATE, "the model steps a LatitudeLongitudeGrid with row tables: create it with a curvilinear grid_type "
                                   "(lat_lon_as_curvilinear, tripolar, gaussian_islands) to hand it 2-D metrics");
  if (!metrics || nx != gsx || (ny != gsy && ny != gsy - 1))
    return fail(m, GB25_ERR_INVALID_ARGUMENT, "gb25_set_curvilinear_grid: %d arrays of (Nx_global + 2 halo) x (Ny + 2 halo [+ 1]) = "
                                              "%d x %d [%d] doubles, got %d x %d", (int)GB25_M2_COUNT, gsx, gsy - 1, gsy, (int)nx, (int)ny);
  for (int q = 0; q < GB25_M2_COUNT; q++)
    if (!metrics[q]) return fail(m, GB25_ERR_INVALID_ARGUMENT, "gb25_set_curvilinear_grid: metric %d is null", q);
  if (gb25_status s = collective_guard(m, 8, (unsigned)ny, metrics[0][(size_t)H + (size_t)gsx * H])) return s;
  if (gb25_status s = quiesce_for_grid_change(m)) return s;
  if (m->group) HIPCHK(m->group->sync_side());
  for (int q = 0; q < GB25_M2_COUNT; q++) {
    std::vector<double>& a = m->host_curv[q];
    a.assign((size_t)gsx * gsy, 0.0);
    std::memcpy(a.data(), metrics[q], (size_t)gsx * ny * sizeof(double));
    if (ny < gsy) std::memcpy(a.data() + (size_t)gsx * ny, a.data() + (size_t)gsx * (ny - 1), (size_t)gsx * sizeof(double));   // (never read)
    // lengths and areas must be positive on the rows the kernels divide by
    if (q != GB25_M2_FFF && q != GB25_M2_PHICC)
      for (int j = 0; j < c.Ny; j++)
        for (int i = 0; i < c.Nx; i++)
          if (!(a[(size_t)(i + H) + (size_t)gsx * (j + H)] > 0.0)) {
            for (auto& h : m->host_curv) h.clear();
            return fail(m, GB25_ERR_INVALID_ARGUMENT, "gb25_set_curvilinear_grid: metric %d is not positive at interior point (%d, %d)", q, i, j);
          }
  }
  gb25_status s;
  if ((s = build_curv_grid(m))) return s;
  if ((m->slab || m->g.cv.north_fold) && (s = build_curv_wide(m))) return s;
  return GB25_OK;
}
// ---- the host's vertical grid: grid.z faces, bottom to top (exponential_z_faces(Nz, depth, h) in the reference: src/model_utils.jl:56-62)
gb25_status gb25_set_vertical_faces(gb25_model* m, const double* zf, int32_t n) {
  CHECK_MODEL(m);
  if (!zf || n != m->cfg.Nz + 1) return fail(m, GB25_ERR_INVALID_ARGUMENT, "gb25_set_vertical_faces: Nz + 1 = %d faces, bottom to top", m->cfg.Nz + 1);
  for (int k = 0; k < m->cfg.Nz; k++)
    if (!(zf[k + 1] > zf[k])) return fail(m, GB25_ERR_INVALID_ARGUMENT, "gb25_set_vertical_faces: faces must increase (face %d)", k + 1);
  if (gb25_status s = collective_guard(m, 9, (unsigned)n, zf[0])) return s;
  if (gb25_status s = quiesce_for_grid_change(m)) return s;
  if (m->group) HIPCHK(m->group->sync_side());
  m->host_zf.assign(zf, zf + n);
  gb25_status s;
  if ((s = build_grid(m))) return s;          // (row tables again too: small)
  if ((s = build_eos_tables(m))) return s;
  if ((s = rebuild_bottom(m))) return s;
  return mask_impl(m);
}
// which: 0 = number of immersed cells of column (i, j) (0-based local indices), 1 = static depth at the U face,
// 2 = at the V face
gb25_status gb25_get_bottom_info(const gb25_model* m, int32_t which, int32_t i, int32_t j, double* value) {
  if (!m || !value || j < 0 || j >= m->Ny || i < 0 || i >= m->Nx || which < 0 || which > 2) return GB25_ERR_INVALID_ARGUMENT;
  if (m->kbot.empty()) { *value = which == 0 ? 0.0 : (double)m->g.Lz; return GB25_OK; }
  const int offk = m->metric_off_k, Nz = m->cfg.Nz;
  auto depth = [&](int ii, int jj) { return (double)(real)m->h_metric[GB25_M_ZF][offk + Nz] - (double)(real)m->h_metric[GB25_M_ZF][offk + first_wet_level(m, ii, jj)]; };
  *value = which == 0 ? (double)first_wet_level(m, i, j) : which == 1 ? std::min(depth(i - 1, j), depth(i, j)) : std::min(depth(i, j - 1), depth(i, j));
  return GB25_OK;
}
gb25_status gb25_fill_halo_regions(gb25_model* m) {
  CHECK_MODEL(m);
  if (m->slab) return fail(m, GB25_ERR_STATE, "phase-by-phase driving is for single-domain models: a slab's x halos come from the exchange inside gb25_first_time_step / gb25_time_step / gb25_loop");
  return fill_halos_impl(m, FillRequest::everything_periodic_x());
}
gb25_status gb25_compute_auxiliaries(gb25_model* m) {
  CHECK_MODEL(m);
  gb25_status s = compute_w_impl(m);
  if (!s) s = compute_p_impl(m, PressureBox::whole(launch_facts(m)));
  // (closure = CATKE: compute_diffusivities! is the third auxiliary -- it steps e and makes kappa_u, kappa_c, kappa_e, L^e, J^b)
  if (!s && m->catke && m->slab) return fail(m, GB25_ERR_STATE, "gb25_compute_auxiliaries with CATKE: phase-by-phase driving is for single-domain models");
  return s ? s : catke_diffusivities_impl(m);
}
gb25_status gb25_fill_diffusivity_halos(gb25_model* m) { CHECK_MODEL(m); return GB25_OK; }
gb25_status gb25_compute_momentum_tendencies(gb25_model* m) { CHECK_MODEL(m); return momentum_impl(m); }
gb25_status gb25_compute_tracer_tendencies(gb25_model* m) { CHECK_MODEL(m); return tracers_impl(m); }
// compute_hydrostatic_boundary_tendency_contributions! (src/precompile.jl:25,52-61): the flux boundary conditions are
// applied INSIDE the tendency kernels (the top cell's tendency gets -J/dz where it is computed, so that the AB2
// look-aheads see the complete tendency); as a phase of its own there is nothing left to do.
gb25_status gb25_compute_boundary_tendencies(gb25_model* m) { CHECK_MODEL(m); return GB25_OK; }
// FluxBoundaryCondition at the top of u, v, T or S (f = GB25_U, GB25_V, GB25_T, GB25_S): J at the interior points of the
// field's horizontal location (dims = gb25_field_dims(f, 0)[0..1], i fastest), positive upward (out of the ocean), in
// the units of the field times m/s.  NULL restores the default no-flux condition.  With ClimaOcean's ocean_simulation
// these are the arrays the coupled model fills every step (wind stress, heat and fresh-water flux).
gb25_status gb25_set_top_flux(gb25_model* m, gb25_field f, const void* host) {
  CHECK_MODEL(m);
  const int q = f == GB25_U ? 0 : f == GB25_V ? 1 : f == GB25_T ? 2 : f == GB25_S ? 3 : -1;
  if (q < 0) return fail(m, GB25_ERR_INVALID_ARGUMENT, "top flux boundary conditions exist for u, v, T, S");
  if (gb25_status s = collective_guard(m, 6, (unsigned)f, host ? 1.0 : 0.0)) return s;
  if (gb25_status s = wait_for_model(m)) return s;
  m->valid.void_lookaheads();
  const Field& F = m->f[f];
  const size_t n2 = (size_t)F.nx * F.ny;
  if (!host) {
    m->g.top_flux[q] = nullptr;   // (the array stays allocated for the next use)
    return GB25_OK;
  }
  if (!m->d_top_flux[q]) {
    HIPCHK(m->mem.alloc(&m->d_top_flux[q], n2 * sizeof(real), true));
    m->top_flux_elems[q] = n2;
  }
  int32_t di[3];
  gb25_field_dims(m, f, 0, di);   // (the interior of the field's horizontal location: Ny rows of y faces on a folded grid)
  const int H = m->cfg.halo, nxi = di[0], nyi = di[1];
  HIPCHK(hipMemcpy2D(m->d_top_flux[q] + (size_t)H * F.nx + H, (size_t)F.nx * sizeof(real), host, (size_t)nxi * sizeof(real),
                     (size_t)nxi * sizeof(real), nyi, hipMemcpyHostToDevice));
  m->g.top_flux[q] = m->d_top_flux[q];
  return GB25_OK;
}
gb25_status gb25_set_bottom_drag(gb25_model* m, double Cd) {
  CHECK_MODEL(m);
  if (!(Cd >= 0)) return fail(m, GB25_ERR_INVALID_ARGUMENT, "the bottom drag coefficient must be >= 0");
  if (gb25_status s = collective_guard(m, 11, 0, Cd)) return s;
  if (gb25_status s = wait_for_model(m)) return s;
  const size_t n2 = (size_t)m->g.sx * m->g.sy_v;
  for (int q = 0; q < 2; q++) {
    if (Cd != 0 && !m->d_bottom_flux[q]) HIPCHK(m->mem.alloc(&m->d_bottom_flux[q], n2 * sizeof(real), true));
    m->g.bottom_flux[q] = Cd != 0 ? m->d_bottom_flux[q] : nullptr;
  }
  m->bottom_drag = Cd;
  m->valid.void_lookaheads();
  return GB25_OK;
}
gb25_status gb25_set_tracer_advection_order(gb25_model* m, int32_t order) {
  CHECK_MODEL(m);
  if (order != 5 && order != 7) return fail(m, GB25_ERR_INVALID_ARGUMENT, "tracer_advection = WENO(order = 5) or WENO(order = 7), not %d", order);
  if (order == 7 && m->cfg.halo < 4) return fail(m, GB25_ERR_INVALID_ARGUMENT, "WENO(order = 7) needs a halo of at least 4");
  if (order == 7 && m->kernel_gen < 2) return fail(m, GB25_ERR_STATE, "the direct-stencil kernels (GB25_OPT_KERNELS = 1) know WENO(order = 5) only");
  if (gb25_status s = collective_guard(m, 12, (unsigned)order, 0.0)) return s;
  m->tracer_order = order;
  m->valid.void_lookaheads();
  m->valid.complete_fills_owed();
  return GB25_OK;
}
gb25_status gb25_get_tracer_advection_order(const gb25_model* m, int32_t* order) {
  if (!m || !order) return GB25_ERR_INVALID_ARGUMENT;
  *order = m->tracer_order;
  return GB25_OK;
}
gb25_status gb25_get_bottom_drag(const gb25_model* m, double* Cd) {
  if (!m || !Cd) return GB25_ERR_INVALID_ARGUMENT;
  *Cd = m->bottom_drag;
  return GB25_OK;
}
gb25_status gb25_get_top_flux(gb25_model* m, gb25_field f, void* host) {
  CHECK_MODEL(m);
  const int q = f == GB25_U ? 0 : f == GB25_V ? 1 : f == GB25_T ? 2 : f == GB25_S ? 3 : -1;
  if (q < 0 || !host) return fail(m, GB25_ERR_INVALID_ARGUMENT, "top flux boundary conditions exist for u, v, T, S");
  if (!m->g.top_flux[q]) return fail(m, GB25_ERR_STATE, "no top flux boundary condition is set for this field");
  HIPCHK(hipStreamSynchronize(m->stream));
  const Field& F = m->f[f];
  int32_t di[3];
  gb25_field_dims(m, f, 0, di);
  const int H = m->cfg.halo, nxi = di[0], nyi = di[1];
  HIPCHK(hipMemcpy2D(host, (size_t)nxi * sizeof(real), m->g.top_flux[q] + (size_t)H * F.nx + H, (size_t)F.nx * sizeof(real),
                     (size_t)nxi * sizeof(real), nyi, hipMemcpyDeviceToHost));
  return GB25_OK;
}
gb25_status gb25_set_prescribed_atmosphere(gb25_model* m, gb25_atmosphere_field f, const double* host) {
  CHECK_MODEL(m);
  if ((int)f < 0 || (int)f >= GB25_ATM_COUNT) return fail(m, GB25_ERR_INVALID_ARGUMENT, "atmosphere field %d", (int)f);
  if (gb25_status s = collective_guard(m, 9, (unsigned)f, host ? 1.0 : 0.0)) return s;
  if (gb25_status s = wait_for_model(m)) return s;
  const size_t n2 = (size_t)m->g.sx * m->g.sy_c;
  if (!host) {
    if (m->d_atm[f]) m->mem.release(m->d_atm[f]);
  } else {
    if (!m->d_atm[f]) HIPCHK(m->mem.alloc(&m->d_atm[f], n2 * sizeof(double)));
    HIPCHK(hipMemcpy(m->d_atm[f], host, n2 * sizeof(double), hipMemcpyHostToDevice));
  }
  m->coupled = true;
  for (auto p : m->d_atm) m->coupled = m->coupled && p != nullptr;
  m->valid.void_lookaheads();
  return GB25_OK;
}
gb25_status gb25_compute_atmosphere_ocean_fluxes(gb25_model* m) {
  CHECK_MODEL(m);
  if (!m->coupled) return fail(m, GB25_ERR_STATE, "no prescribed atmosphere: set all of its fields first (gb25_set_prescribed_atmosphere)");
  if (gb25_status s = materialize_uv(m)) return s;
  m->valid.void_lookaheads();   // (made from tendencies with the old fluxes)
  return atmosphere_ocean_fluxes_impl(m);
}
gb25_status gb25_compute_tendencies(gb25_model* m) {
  CHECK_MODEL(m);
  gb25_status s = momentum_impl(m);
  if (!s) s = tracers_impl(m);
  return s ? s : catke_tendency_impl(m);   // (closure = CATKE: the slow tendency of e)
}
gb25_status gb25_ab2_step(gb25_model* m, double dt, int euler) {
  CHECK_MODEL(m);
  if (m->slab) return fail(m, GB25_ERR_STATE, "gb25_ab2_step: phase-by-phase driving is for single-domain models");
  // ab2_step! leaves every halo as it is; look-ahead buffers written with their halos (fold_fills) are therefore not
  // adopted here: the stand-alone kernels give the same interior bits
  if (m->fold_fills) m->valid.void_tracer_lookahead();
  return ab2_step_impl(m, dt, euler);
}
gb25_status gb25_correct_velocities_and_cache_previous_tendencies(gb25_model* m, double) {
  CHECK_MODEL(m);
  return corrector_impl(m, CorrectorRequest::all(false));   // (a caller of the single phases may have touched u, v: no column integrals)
}
gb25_status gb25_update_state(gb25_model* m) {
  CHECK_MODEL(m);
  if (m->slab) return fail(m, GB25_ERR_STATE, "gb25_update_state: phase-by-phase driving is for single-domain models");
  return update_state_impl(m);
}
// ---- options: every switch of the library is a per-model option; nothing is read from the environment
// One row per option: the member it reads and writes; the values it accepts -- lo <= v <= hi in steps of `step`, or with step 0 a
// flag: any v, stored as v != 0 --; the message that refuses every other value; and, where setting it has a consequence, a hook
// that runs between that check and the store.  A hook may refuse, and it may change what is stored.
struct OptionRow {
  gb25_option id;
  int& (*at)(gb25_model*);
  int lo, hi, step;
  const char* refusal;
  gb25_status (*hook)(gb25_model*, int32_t*);
};
static gb25_status opt_kernels(gb25_model* m, int32_t* v) {
  if (*v == 1 && m->immersed) return fail(m, GB25_ERR_STATE, "the direct-stencil kernels know no immersed boundary");
  return GB25_OK;
}
static gb25_status opt_pressure_precision(gb25_model*, int32_t* v) {
  if (sizeof(real) == 8) *v = 64;   // (a Float64 model's own arithmetic IS fp64)
  return GB25_OK;
}
static gb25_status opt_fold_fills(gb25_model* m, int32_t*) {
  m->valid.complete_fills_owed();
  return GB25_OK;
}
static gb25_status opt_substep_order(gb25_model* m, int32_t* v) {
  if (*v == 1 && m->g.cv.on) return fail(m, GB25_ERR_STATE, "substep_order = 1 is built for the LatitudeLongitudeGrid kernels only (the oracle has it on every grid)");
  return GB25_OK;
}
static gb25_status opt_fold_pivot_slaved(gb25_model* m, int32_t* v) {
  if (*v != 0 && !m->g.cv.north_fold) return fail(m, GB25_ERR_STATE, "fold_pivot_slaved: this grid has no zipper fold");
  if (*v != 0 && m->slab) return fail(m, GB25_ERR_STATE, "fold_pivot_slaved is built for the single domain only (a slab's eastern half of the pivot row belongs to its partner rank)");
  return GB25_OK;
}
static gb25_status opt_catke_stale_e_halos(gb25_model* m, int32_t* v) {
  if (*v != 0 && m->slab) return fail(m, GB25_ERR_STATE, "catke_stale_e_halos: a decomposition cannot leave the halos of e stale at its internal boundaries");
  return GB25_OK;
}
static gb25_status opt_chunk_levels(gb25_model* m, int32_t* v) {
  // the tendency kernels reach one chunk of levels plus its stencil planes with 32-bit byte offsets (plan_layout checks the
  // default chunking by the same rule): the chosen one must stay within that reach too
  const TendencyReach r = tendency_reach_ok(m->layout, *v, (int)sizeof(real));
  if (!r.ok)
    return fail(m, GB25_ERR_INVALID_ARGUMENT, "chunks of %d levels (+ %d stencil planes of %.3g elements) exceed the 2 GB the tendency "
                "kernels address from one base: choose fewer levels per chunk", r.klen, r.planes - r.klen, r.plane);
  m->valid.void_colsums();
  return GB25_OK;
}
static gb25_status opt_immersed_kernels(gb25_model* m, int32_t* v) {
  // 1: run the immersed-boundary kernel variants even where nothing is immersed (they must then give the bits of
  // the plain ones: tests); 0: back to the choice the bottom makes
  if (*v != 0 && m->kernel_gen == 1) return fail(m, GB25_ERR_STATE, "the direct-stencil kernels know no immersed boundary");
  if (*v != 0 && !m->d_ord[0]) {
    if (m->cfg.Nz > 254) return fail(m, GB25_ERR_INVALID_ARGUMENT, "an immersed boundary needs Nz <= 254");
    if (gb25_status s = build_bottom(m, [](int, int) { return -1e30; })) return s;
  }
  for (int kb : m->kbot) *v = *v || (kb > 0 && kb < 255);
  return GB25_OK;
}
#define OPT_AT(member) [](gb25_model* m) -> int& { return m->member; }
#define OPT_FLAG 0, 0, 0, nullptr
static const OptionRow kOptions[GB25_OPT_COUNT] = {
    {GB25_OPT_KERNELS, OPT_AT(kernel_gen), 1, 2, 1, "GB25_OPT_KERNELS: 1 (direct stencil) or 2 (default)", opt_kernels},
    {GB25_OPT_AB2_LOOKAHEAD, OPT_AT(ab2_ahead), 0, 2, 1, "GB25_OPT_AB2_LOOKAHEAD: 0, 1 or 2 (tracers only)", nullptr},
    {GB25_OPT_SUBCYCLE_LOOKAHEAD, OPT_AT(baro_ahead), 0, 2, 1, "GB25_OPT_SUBCYCLE_LOOKAHEAD: 0, 1 (main stream) or 2 (own stream)", nullptr},
    {GB25_OPT_SUBCYCLE_BLOCK, OPT_AT(baro_block), 1, 7, 2, "GB25_OPT_SUBCYCLE_BLOCK: 1, 3, 5 or 7 substeps per launch", nullptr},
    {GB25_OPT_FILL_FUSED, OPT_AT(fill_fused), OPT_FLAG, nullptr},
    {GB25_OPT_TWO_STREAMS, OPT_AT(two_streams), OPT_FLAG, nullptr},
    {GB25_OPT_STORE_PRESSURE, OPT_AT(phy_pinned), OPT_FLAG, nullptr},
    {GB25_OPT_SPLIT_TENDENCIES, OPT_AT(split_tendencies), OPT_FLAG, nullptr},
    {GB25_OPT_PRESSURE_PRECISION, OPT_AT(pressure_bits), 32, 64, 32, "GB25_OPT_PRESSURE_PRECISION: 64 or 32", opt_pressure_precision},
    {GB25_OPT_IMMERSED_KERNELS, OPT_AT(immersed), OPT_FLAG, opt_immersed_kernels},
    {GB25_OPT_FOLD_FILLS, OPT_AT(fold_fills), OPT_FLAG, opt_fold_fills},
    {GB25_OPT_LAZY_CORRECTOR, OPT_AT(lazy_corrector), OPT_FLAG, nullptr},
    {GB25_OPT_MOMENTUM_CHUNK_LEVELS, OPT_AT(mom_chunk_levels), 6, 4096, 1, "chunk levels: 6 or more", opt_chunk_levels},
    {GB25_OPT_TRACER_CHUNK_LEVELS, OPT_AT(trc_chunk_levels), 6, 4096, 1, "chunk levels: 6 or more", opt_chunk_levels},
    {GB25_OPT_TRACERS_FIRST, OPT_AT(tracers_first), OPT_FLAG, nullptr},
    {GB25_OPT_W_ON_THE_FLY, OPT_AT(w_fly), OPT_FLAG, nullptr},
    {GB25_OPT_SUB_STREAM_PRIORITY, OPT_AT(sub_priority), OPT_FLAG, nullptr},
    {GB25_OPT_SUBCYCLE_WHOLE, OPT_AT(baro_whole), OPT_FLAG, nullptr},
    {GB25_OPT_EARLY_STRIPS, OPT_AT(early_strips), OPT_FLAG, nullptr},
    {GB25_OPT_CATKE_STALE_E_HALOS, OPT_AT(catke_stale_e_halos), OPT_FLAG, opt_catke_stale_e_halos},
    {GB25_OPT_COMM_TIMEOUT_SECONDS, OPT_AT(comm_timeout_s), 1, INT_MAX, 1, "comm_timeout_seconds: at least 1", nullptr},
    {GB25_OPT_ROCTX_RANGES, OPT_AT(roctx_ranges), OPT_FLAG, nullptr},
    {GB25_OPT_SUBSTEP_ORDER, OPT_AT(substep_order), 0, 1, 1, "substep_order: 0 (eta, then U, V) or 1 (U, V, then eta)", opt_substep_order},
    {GB25_OPT_FOLD_PIVOT_SLAVED, OPT_AT(g.cv.pivot_slaved), OPT_FLAG, opt_fold_pivot_slaved},
    {GB25_OPT_PRESSURE_FORM, OPT_AT(pressure_form), 0, 3, 1, "GB25_OPT_PRESSURE_FORM: 0 (the library's rule), 1 (tiles), 2 (one row per thread) or 3 (four rows per thread)", nullptr},
    {GB25_OPT_SPECTRUM_TABLE, OPT_AT(spectrum_table_where), 0, 1, 1, "GB25_OPT_SPECTRUM_TABLE: 0 (the library's rule) or 1 (global memory)", nullptr},
};
#undef OPT_FLAG
#undef OPT_AT
static const OptionRow* option_row(gb25_option opt) {
  for (const OptionRow& r : kOptions)
    if (r.id == opt) return &r;
  return nullptr;
}
gb25_status gb25_set_option(gb25_model* m, gb25_option opt, int32_t v) {
  CHECK_MODEL(m);
  if (gb25_status s = collective_guard(m, 5, (unsigned)opt, (double)v)) return s;
  // a switch may change which buffers carry the next time level: whatever is in flight finishes, every look-ahead is void
  if (gb25_status s = wait_for_model(m)) return s;
  m->valid.option_changes();
  const OptionRow* row = option_row(opt);
  if (!row) return fail(m, GB25_ERR_INVALID_ARGUMENT, "unknown option %d", (int)opt);
  if (row->step == 0) v = v != 0;
  else if (v < row->lo || v > row->hi || (v - row->lo) % row->step != 0) return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s", row->refusal);
  if (row->hook)
    if (gb25_status s = row->hook(m, &v)) return s;
  row->at(m) = v;
  return GB25_OK;
}
gb25_status gb25_get_option(const gb25_model* m, gb25_option opt, int32_t* v) {
  if (!m || !v) return GB25_ERR_INVALID_ARGUMENT;
  const OptionRow* row = option_row(opt);
  if (!row) return GB25_ERR_INVALID_ARGUMENT;
  *v = row->at(const_cast<gb25_model*>(m));   // (read only: the rows name their members through one accessor)
  return GB25_OK;
}

// ---- exchange context of a decomposed model ----------------------------------------------------------------------
gb25_status gb25_comm_unique_id(void* id_out) {
  if (!id_out) return GB25_ERR_INVALID_ARGUMENT;
  static_assert(sizeof(ncclUniqueId) == GB25_UNIQUE_ID_BYTES, "gb25.h: GB25_UNIQUE_ID_BYTES");
  if (!rccl().load()) return GB25_ERR_COMM;
  ncclUniqueId id;
  if (rccl().GetUniqueId(&id) != ncclSuccess) return GB25_ERR_COMM;
  memcpy(id_out, &id, sizeof id);
  return GB25_OK;
}
gb25_status gb25_comm_init_rccl(gb25_model* m, const void* unique_id) {
  CHECK_MODEL(m);
  if (!unique_id) return GB25_ERR_INVALID_ARGUMENT;
  if (!m->slab) return fail(m, GB25_ERR_STATE, "a single periodic domain (nranks = 1, slab_mode = 0) has nothing to exchange");
  if (!rccl().load()) return fail(m, GB25_ERR_COMM, "%s", rccl().error.c_str());
  HIPCHK(hipSetDevice(m->cfg.device));
  RcclTransport* tr = new RcclTransport();
  tr->rank = m->cfg.rank;
  tr->nranks = m->cfg.nranks;
  ncclUniqueId id;
  memcpy(&id, unique_id, sizeof id);
  (void)hipGetLastError();   // (RCCL reports a stale, already-handled HIP error of this process as "unhandled cuda error")
  // GB25_REHEARSE_ALONE=1: this rank of a decomposition runs alone, its neighbours are itself (a timing proxy, not a simulation)
  const char* solo = getenv("GB25_REHEARSE_ALONE");
  tr->alone = solo && solo[0] == '1' && tr->nranks > 1;
  // ncclCommInitRank blocks until every rank of the communicator has called it: a rank that never arrives (a crashed process, a
  // launcher that started fewer ranks than --gpus says) would leave the others waiting for ever.  It runs on a helper thread and
  // this one waits for it with a bound (option COMM_TIMEOUT_SECONDS); past it the call fails with the rank -- the helper thread
  // is abandoned, the process is expected to exit.
  ncclResult_t r = ncclInvalidArgument;
  if (!tr->alone) {
    struct InitState { std::mutex mu; std::condition_variable cv; bool done = false; ncclResult_t r = ncclSuccess; ncclComm_t comm = nullptr; };
    auto st = std::make_shared<InitState>();
    const int dev = m->cfg.device, nr = tr->nranks, rk = tr->rank;
    std::thread([st, id, dev, nr, rk]() {
      (void)hipSetDevice(dev);
      ncclComm_t c = nullptr;
      const ncclResult_t rr = rccl().CommInitRank(&c, nr, id, rk);
      std::lock_guard<std::mutex> lk(st->mu);
      st->r = rr; st->comm = c; st->done = true;
      st->cv.notify_all();
    }).detach();
    std::unique_lock<std::mutex> lk(st->mu);
    if (!st->cv.wait_for(lk, std::chrono::seconds(m->comm_timeout_s), [&] { return st->done; })) {
      delete tr;
      return fail(m, GB25_ERR_COMM, "rank %d of %d: ncclCommInitRank did not return within %d s -- not every rank of the communicator "
                  "called it (were all %d processes started, with the same unique id?)", rk, nr, m->comm_timeout_s, nr);
    }
    r = st->r;
    tr->comm = st->comm;
  }
  if (r != ncclSuccess && (tr->nranks == 1 || tr->alone)) {
    // a one-rank communicator (the self-ring) needs nobody's agreement: once more with a fresh id
    (void)hipGetLastError();
    if (rccl().GetUniqueId(&id) == ncclSuccess) r = rccl().CommInitRank(&tr->comm, 1, id, 0);
  }
  if (r != ncclSuccess) {
    tr->comm = nullptr;
    delete tr;
    return fail(m, GB25_ERR_COMM, "ncclCommInitRank(rank %d of %d) failed: %s", m->cfg.rank, m->cfg.nranks,
                rccl().GetErrorString(r));
  }
  gb25_model* one[1] = {m};
  if (gb25_status s = group_create(one, 1, tr)) return s;
  // The first exchange with every peer this rank will ever talk to -- the ring neighbours, the rows' neighbours of a 2-D
  // decomposition, the fold partner -- a few bytes each, bounded by the same timeout: a peer that built another decomposition (or
  // none) shows here, with the rank and the buffer set, instead of as a hang in the first time step.
  SlabGroup* G = m->group;
  for (BufferSet b : {SetBundle, SetBundleRows, SetFoldBundle}) {   // (one set per Peer)
    const Peer peer = set_info(b).peer;
    if ((peer == Peer::Rows && m->Ry < 2) || (peer == Peer::FoldPartner && !m->g.cv.north_fold)) continue;
    const size_t nbytes = std::min<size_t>(16, G->elems[b] * sizeof(real));
    if (gb25_status s = tr->exchange(*G, b, nbytes, G->main)) return s;
    const auto t0 = std::chrono::steady_clock::now();
    hipError_t q;
    while ((q = hipStreamQuery(G->main)) == hipErrorNotReady) {
      if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(m->comm_timeout_s))
        return fail(m, GB25_ERR_COMM, "rank %d of %d (%d x %d): the first exchange of buffer set %d (%s) did not complete within %d s",
                    m->cfg.rank, m->cfg.nranks, m->Rx, m->Ry, b, peer == Peer::Ring ? "west / east ring neighbours" : peer == Peer::Rows ? "southern / northern neighbours" : "fold partner",
                    m->comm_timeout_s);
      std::this_thread::sleep_for(std::chrono::milliseconds(1));
    }
    if (q != hipSuccess) return fail(m, GB25_ERR_HIP, "the first exchange of buffer set %d failed: %s", b, hipGetErrorString(q));
  }
  return GB25_OK;
}
// What the exchange context of this model is: transport 0 none, 1 RCCL, 2 local ring (all slabs in this process), 3 host callback;
// comm_ranks: the size of the communicator AS RCCL REPORTS IT (ncclCommCount; 0 without RCCL) -- bench.py prints it so that a
// scaling line says how many ranks really talked to each other
gb25_status gb25_comm_info(const gb25_model* m, int32_t* transport, int32_t* comm_ranks) {
  if (!m) return GB25_ERR_INVALID_ARGUMENT;
  int t = 0, n = 0;
  if (m->group && m->group->transport) {
    const std::string name = m->group->transport->name();
    t = name == "rccl" ? 1 : name == "local" ? 2 : 3;
    if (t == 1) {
      RcclTransport* R = static_cast<RcclTransport*>(m->group->transport);
      if (R->comm && rccl().CommCount(R->comm, &n) != ncclSuccess) n = -1;
    }
  }
  if (transport) *transport = t;
  if (comm_ranks) *comm_ranks = n;
  return GB25_OK;
}
// The sends and receives ONE rank of an Rx x Ry decomposition posts for exchange group `group`, in posting order, as text:
// "send <peer> <side>" / "recv <peer> <side>" per line ("copy" when the rank is its own fold partner).  No GPU is touched: this is
// RcclTransport::exchange's own plan (exchange_plan).  folded_grid: the GLOBAL grid has a zipper fold (only the top row of ranks folds).
// -1 for a `group` that is no row of the table of groups (slab_protocol.hpp).
int64_t gb25_debug_exchange_plan(int32_t Rx, int32_t Ry, int32_t rank, int32_t folded_grid, int32_t group, char* out, int64_t cap) {
  if (Rx < 1 || Ry < 1 || rank < 0 || rank >= Rx * Ry) return -1;
  const MeshPos q(Rx, Ry, rank);
  const bool fold = folded_grid != 0 && q.ry == Ry - 1;
  const GroupInfo* info = find_group(group);
  if (!info) return -1;
  const Peer peer = info->peer;
  std::string log;
  if (peer == Peer::FoldPartner && fold && q.partner() == rank) log = "copy\n";
  else if (!(peer == Peer::FoldPartner && !fold) && !(peer == Peer::Rows && Ry < 2))
    for (const PlanOp& op : exchange_plan(q, fold, peer)) {
      char line[48];
      snprintf(line, sizeof line, "%s %d %d\n", op.send ? "send" : "recv", op.peer, op.side);
      log += line;
    }
  const int64_t need = (int64_t)log.size() + 1;
  if (out && cap > 0) {
    const int64_t ncopy = std::min<int64_t>(cap - 1, (int64_t)log.size());
    memcpy(out, log.data(), (size_t)ncopy);
    out[ncopy] = 0;
  }
  return need;
}
gb25_status gb25_comm_init_callback(gb25_model* m, gb25_exchange_fn fn, void* user) {
  CHECK_MODEL(m);
  if (!fn) return GB25_ERR_INVALID_ARGUMENT;
  CallbackTransport* tr = new CallbackTransport();
  tr->fn = fn;
  tr->user = user;
  gb25_model* one[1] = {m};
  return group_create(one, 1, tr);
}
gb25_status gb25_comm_init_local(gb25_model* const* slabs, int32_t n) {
  if (!slabs || n < 1 || !slabs[0]) return GB25_ERR_INVALID_ARGUMENT;
  gb25_model* m = slabs[0];
  for (int s = 0; s < n; s++) {
    if (!slabs[s]) return GB25_ERR_INVALID_ARGUMENT;
    const gb25_config &a = slabs[s]->cfg, &b = m->cfg;
    if (a.nranks != n || a.rank != s || a.device != b.device || a.Nx != b.Nx || a.Ny != b.Ny || a.Nz != b.Nz || a.ranks_y != b.ranks_y ||
        a.halo != b.halo || a.substeps != b.substeps)
      return fail(m, GB25_ERR_INVALID_ARGUMENT,
                  "gb25_comm_init_local wants the %d slabs of ONE decomposition in rank order on one device (slab %d does "
                  "not fit)", n, s);
  }
  return group_create(slabs, n, new LocalRingTransport());
}
gb25_status gb25_comm_finalize(gb25_model* m) {
  CHECK_MODEL(m);
  if (m->group) group_destroy(m->group);
  return GB25_OK;
}

static gb25_status need_group(gb25_model* m, const char* what) {
  if (m->group) return group_refresh(m->group);   // (the bundles grow when a closure adds fields)
  return fail(m, GB25_ERR_STATE,
              "%s on a slab of a decomposition needs an exchange context first: gb25_comm_init_rccl (one process per GPU), "
              "gb25_comm_init_local (all slabs in this process) or gb25_comm_init_callback", what);
}

// ---- composites: GordonBell25.first_time_step!/time_step!/loop! (src/timestepping_utils.jl:21-45) ----------------------
// On a slab these step every slab of the exchange context in lock-step (one slab per process with RCCL).
gb25_status gb25_first_time_step(gb25_model* m) {
  CHECK_MODEL(m);
  Range r_first(m, "first_time_step");
  gb25_status s;
  if (m->slab) {
    if ((s = need_group(m, "gb25_first_time_step"))) return s;
    GroupOps ops(*m->group);
    return sequence_first_time_step(ops, m->group->lookahead_in_flight);
  }
  if ((s = initialize_impl(m))) return s;
  if ((s = update_state_impl(m))) return s;
  if ((s = first_fluxes_impl(m))) return s;
  return time_step_impl(m, 1);
}
static gb25_status loop_impl(gb25_model* m, int32_t n);
gb25_status gb25_time_step(gb25_model* m) {
  CHECK_MODEL(m);
  Range r_step(m, "time_step");
  return loop_impl(m, 1);
}
gb25_status gb25_loop(gb25_model* m, int32_t n) {
  CHECK_MODEL(m);
  Range r_loop(m, "loop");
  return loop_impl(m, n);
}
static gb25_status loop_impl(gb25_model* m, int32_t n) {
  if (m->slab) {
    if (gb25_status s = need_group(m, "gb25_loop")) return s;
    GroupOps ops(*m->group);
    for (int it = 0; it < n; it++)
      if (gb25_status s = sequence_time_step(ops, 0, m->group->lookahead_in_flight)) return s;
    // (steps that kept the corrector inside its consumers: memory holds the corrected velocities when the call returns)
    for (gb25_model* q : m->group->slabs)
      if (gb25_status s = materialize_uv(q)) return fail(m, s, "%s", q->err.c_str());
    return GB25_OK;
  }
  // (every step of the call may keep the corrector inside its consumers, the last one too: one sweep u += du, v += dv and one w
  // kernel when the call returns -- a last step with the stand-alone corrector would first materialise the step before it, then
  // run its own corrector and w: 0.75 ms more than a steady step at 1440x720x48, against 0.37)
  for (int it = 0; it < n; it++)
    if (gb25_status s = time_step_impl(m, 0, true)) return s;
  return materialize_uv(m);   // (no-op unless the last step kept the corrector inside its consumers)
}

gb25_status gb25_lookahead_state(const gb25_model* m, int32_t* velocities_ready, int32_t* subcycle_adopted) {
  if (!m) return GB25_ERR_INVALID_ARGUMENT;
  if (velocities_ready) *velocities_ready = m->valid.velocities_ready(m->baro_ahead) ? 1 : 0;
  if (subcycle_adopted) *subcycle_adopted = m->baro_adopted ? 1 : 0;
  return GB25_OK;
}

// The order of operations of one (first) time step of `nslabs` slabs as text, one operation per line, without touching
// a GPU: "stage <n> slab <s> euler <e> <stream>", "pack|unpack <group> slab <s> <stream>", "exchange <group> <stream>",
// "record|wait <event> <stream>".  adopted / ready: what the slabs would report (sub-cycle look-ahead adopted by stage 0;
// velocity look-ahead available after stage 3).  Returns the number of bytes needed (incl. the terminator).
int64_t gb25_debug_sequence(int32_t nslabs, int32_t first, int32_t adopted, int32_t ready, char* out, int64_t cap) {
  if (nslabs < 1) return -1;
  TraceOps ops(nslabs, adopted != 0, ready != 0);
  if (first & 2) ops.fold = true;   // (bit 1 of `first`: a folded grid)
  if (first & 4) ops.is_coupled = true;   // (bit 2: a coupled model -- data-free forcing)
  if (first & 64) ops.early = true;       // (bit 6: plain x slabs whose bundle is unpacked on the exchange stream)
  if (first & 32) ops.is_lazy = true;     // (bit 5: a step that keeps the corrector inside its consumers)
  if (first & 16) ops.mesh = true;        // (bit 4: a 2-D decomposition -- y halos from the southern / northern neighbour)
  if (first & 128) ops.is_catke = true;   // (bit 7: closure = CATKE -- the halos of e and J^b travel inside update_state!)
  bool in_flight = (first & 8) != 0;      // (bit 3: the previous step left the look-ahead chain in flight)
  first &= 1;
  if (first) sequence_first_time_step(ops, in_flight);
  else sequence_time_step(ops, 0, in_flight);
  ops.add("lookahead_in_flight %d", in_flight ? 1 : 0);
  const int64_t need = (int64_t)ops.log.size() + 1;
  if (out && cap > 0) {
    const int64_t ncopy = std::min<int64_t>(cap - 1, (int64_t)ops.log.size());
    memcpy(out, ops.log.data(), (size_t)ncopy);
    out[ncopy] = 0;
  }
  return need;
}

// ---- state dump: save_model_state(dir, model, arch; label) (src/sharded_io.jl:122-138) -- see state_io.hpp
gb25_status gb25_save_state(gb25_model* m, const char* directory, const char* label) {
  CHECK_MODEL(m);
  if (!directory || !*directory) return GB25_ERR_INVALID_ARGUMENT;
  const std::string dir = std::string(directory) + "/" + (label && *label ? label : "checkpoint");
  for (size_t q = 1; q <= dir.size(); q++)   // mkpath
    if (q == dir.size() || dir[q] == '/') mkdir(dir.substr(0, q).c_str(), 0777);
  const std::string path = dir + "/fields_rank" + std::to_string(m->cfg.rank) + ".npz";
  NpzWriter z;
  if (!z.open(path)) return fail(m, GB25_ERR_STATE, "cannot write %s", path.c_str());
  const int64_t meta[4] = {m->iteration, (int64_t)m->cfg.rank, (int64_t)m->cfg.nranks, (int64_t)sizeof(real)};
  z.add_array("iteration", "<i8", {}, &meta[0]);
  z.add_array("time", "<f8", {}, &m->time);
  z.add_array("rank", "<i8", {}, &meta[1]);
  z.add_array("nranks", "<i8", {}, &meta[2]);
  // Oceananigans.fields(model): velocities, free surface, tracers -- (T, S), and e with closure = CATKEVerticalDiffusivity()
  struct Member { const char* name; gb25_field id; };
  std::vector<Member> fs = {{"u", GB25_U}, {"v", GB25_V}, {"w", GB25_W}, {"eta", GB25_ETA}, {"T", GB25_T}, {"S", GB25_S}};
  if (m->catke) fs.push_back({"e", GB25_E});
  std::string names;
  std::vector<real> host;
  for (auto& fld : fs) {
    int32_t d[3];
    gb25_field_dims(m, fld.id, 0, d);
    host.resize((size_t)d[0] * d[1] * d[2]);
    if (gb25_status s = gb25_get_field(m, fld.id, host.data(), 0)) {
      z.close();
      return s;
    }
    const int64_t i0 = (int64_t)m->rx * m->Nx, j0 = m->j0;
    const int64_t slice[6] = {i0, i0 + d[0], j0, j0 + d[1], 0, d[2]};
    const int64_t gshape[3] = {m->cfg.Nx, m->Ry > 1 ? global_rows(m->layout, fld.id) : d[1], d[2]};
    z.add_array(std::string(fld.name) + ".data", sizeof(real) == 8 ? "<f8" : "<f4", {d[0], d[1], d[2]}, host.data());
    z.add_array(std::string(fld.name) + ".slice", "<i8", {6}, slice);
    z.add_array(std::string(fld.name) + ".global_shape", "<i8", {3}, gshape);
    names += std::string(fld.name) + "\n";
  }
  z.add("field_names", names, nullptr, 0);
  if (!z.close()) return fail(m, GB25_ERR_STATE, "writing %s failed (disk full, or a member beyond the 4 GB of zip32)", path.c_str());
  return GB25_OK;
}

// ---- profiling ------------------------------------------------------------------------------
gb25_status gb25_profile_enable(gb25_model* m, int on) {
  CHECK_MODEL(m);
  m->profile = on != 0;
  m->profile_only = on >= 2 ? on - 2 : -1;   // on = 2 + k: only kernel k
  if (m->profile_only >= GB25_K_COUNT) return fail(m, GB25_ERR_INVALID_ARGUMENT, "no such kernel id %d", on - 2);
  return GB25_OK;
}
gb25_status gb25_profile_reset(gb25_model* m) {
  CHECK_MODEL(m);
  resolve_profile(m);
  for (int k = 0; k < GB25_K_COUNT; k++) {
    m->prof_count[k] = 0;
    m->prof_ms[k] = 0;
  }
  return GB25_OK;
}
gb25_status gb25_profile_get(gb25_model* m, gb25_kernel k, int64_t* launches, double* total_ms) {
  if (!m || k < 0 || k >= GB25_K_COUNT) return GB25_ERR_INVALID_ARGUMENT;
  resolve_profile(m);
  if (launches) *launches = m->prof_count[k];
  if (total_ms) *total_ms = m->prof_ms[k];
  return GB25_OK;
}

}  // extern "C"

#include "restart_host.hpp"
#include "diagnostics_host.hpp"
#include "averages_host.hpp"
#include "classes_host.hpp"
#include "particles_host.hpp"
#include "passive_host.hpp"
#include "spectrum_host.hpp"
#include "surfaces_host.hpp"
#include "stability_host.hpp"
#include "kinematics_host.hpp"
#include "region_host.hpp"
#include "zonal_eddy_host.hpp"
#include "blocks_host.hpp"
#include "filters_host.hpp"
