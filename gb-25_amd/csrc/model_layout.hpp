// model_layout.hpp -- the shape of a model: its place in the decomposition, the chunking of the tendency kernels and whether they can
// address the arrays, the substepping, the extents of the sub-cycle's work arrays, the defaults of two options, and the extents of
// every field.  plan_layout() is the ONLY place any of this is decided, and it refuses a configuration before a device is touched;
// gb25_create (gb25_api.hip) adopts the layout and allocates from it.  Plain C++, no HIP, no gb25_model: a host compiler can include
// this file alone (tests/test_model_layout.py).  The rules in prose: DESIGN.md, "The layout of a model".
#pragma once
#include "../../include/gb25.h"
#include "tendency_plan.hpp"   // the reach of the tendency kernels

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace {

// ---- field shapes: one row per gb25_field, in the order of the enum
struct FieldShape {
  bool v_shaped;  // on the y faces: its parent keeps the row a northern wall needs
  bool flat;      // 2-D: one level, no z halo
  bool z_faces;   // on the z faces: Nz + 1 levels
  bool catke;     // exists with closure = CATKEVerticalDiffusivity() only (gb25_set_closure_catke allocates it)
};
constexpr FieldShape kFieldShapes[] = {
    /* U */ {0, 0, 0, 0}, /* V */ {1, 0, 0, 0}, /* W */ {0, 0, 1, 0}, /* T */ {0, 0, 0, 0}, /* S */ {0, 0, 0, 0}, /* PHY */ {0, 0, 0, 0},
    /* GN_U */ {0, 0, 0, 0}, /* GN_V */ {1, 0, 0, 0}, /* GN_T */ {0, 0, 0, 0}, /* GN_S */ {0, 0, 0, 0},
    /* GM_U */ {0, 0, 0, 0}, /* GM_V */ {1, 0, 0, 0}, /* GM_T */ {0, 0, 0, 0}, /* GM_S */ {0, 0, 0, 0},
    /* ETA */ {0, 1, 0, 0}, /* BT_U */ {0, 1, 0, 0}, /* BT_V */ {1, 1, 0, 0},
    /* ETA_BAR */ {0, 1, 0, 0}, /* U_BAR */ {0, 1, 0, 0}, /* V_BAR */ {1, 1, 0, 0},
    /* GN_BT_U */ {0, 1, 0, 0}, /* GN_BT_V */ {1, 1, 0, 0},
    /* E */ {0, 0, 0, 1}, /* GN_E */ {0, 0, 0, 1}, /* GM_E */ {0, 0, 0, 1},
    /* KAPPA_U */ {0, 0, 1, 1}, /* KAPPA_C */ {0, 0, 1, 1}, /* KAPPA_E */ {0, 0, 1, 1}, /* LE */ {0, 0, 0, 1}, /* JB */ {0, 1, 0, 1},
    /* PREV_U */ {0, 0, 0, 1}, /* PREV_V */ {1, 0, 0, 1},
};
static_assert(sizeof kFieldShapes / sizeof kFieldShapes[0] == GB25_FIELD_COUNT, "one row per field");
static_assert(kFieldShapes[GB25_W].z_faces && kFieldShapes[GB25_BT_V].v_shaped && kFieldShapes[GB25_GN_BT_V].flat &&
              kFieldShapes[GB25_JB].flat && kFieldShapes[GB25_KAPPA_E].z_faces && !kFieldShapes[GB25_LE].z_faces &&
              kFieldShapes[GB25_PREV_V].v_shaped && kFieldShapes[GB25_E].catke && !kFieldShapes[GB25_GN_BT_V].catke, "rows in the order of the enum");
inline bool is_v_shaped(int id) { return kFieldShapes[id].v_shaped; }
inline bool is_2d(int id) { return kFieldShapes[id].flat; }
inline bool is_catke_field(int id) { return kFieldShapes[id].catke; }

// Split-explicit averaging weights (Oceananigans FixedSubstepNumber, restated): shape function
// (p=2, q=4, r=0.18927) sampled at tau = 2m/Ns, truncated like searchsortedlast(w, 0, rev=true).
struct Substepping {
  int Ns = 0;             // effective substeps
  double dtau_frac = 0;
  std::vector<double> weights;
};
inline Substepping plan_substeps(int N) {
  std::vector<double> w(N + 1, 0.0);
  const double p = 2, q = 4, r = 0.18927, tau0 = (p + 2) * (p + q + 2) / (p + 1) / (p + q + 1);
  for (int k = 1; k <= N; k++) {
    double x = (2.0 * k / N) / tau0;
    w[k] = std::pow(x, p) * (1 - std::pow(x, q)) - r * x;
  }
  int lo = 0, hi = N + 1;
  while (lo < hi - 1) {
    int mid = lo + ((hi - lo) >> 1);
    if (w[mid] < 0.0) hi = mid; else lo = mid;
  }
  double s = 0;
  for (int k = 1; k <= lo; k++) s += w[k];
  Substepping out;
  out.Ns = lo;
  out.dtau_frac = 2.0 / N;
  out.weights.resize(lo);
  for (int k = 1; k <= lo; k++) out.weights[k - 1] = w[k] / s;
  return out;
}

struct ModelLayout {
  int Nx_global = 0, Ny_global = 0, Nz = 0, H = 0;
  // 2-D (x, y) decomposition, Partition(Rx, Ry, 1) of the reference (sharding/sharded_baroclinic_instability_simulation_run.jl:
  // 65-72): rank = ry Rx + rx owns the columns [rx Nx, (rx + 1) Nx) and the rows [j0, j0 + Ny) of the global grid.  Ry = 1: x slabs.
  int Nx = 0, Ny = 0;   // local columns and rows
  int Rx = 1, Ry = 1, rx = 0, ry = 0, j0 = 0;
  bool ys_open = false, yn_open = false;   // a southern / northern neighbour rank exists (no wall on that side)
  bool slab = false;                       // x halos come from a neighbour (nranks > 1, or the self-ring of slab_mode = 1)
  // The northern edge of this rank: the fold of a tripolar grid (the top row of ranks only), a wall (v has a row Ny), or -- neither
  // of the two -- a neighbour rank.
  bool tripolar = false, north_fold = false, north_wall = false;
  Substepping sub;
  // work arrays of the sub-cycle: widened by W columns either side on a slab, tall by Wy rows beyond row Ny - 1 (the images of a
  // fold, or a northern neighbour's) and by Wys rows below row 0 (a southern neighbour's); a single folded domain has W = 0
  int W = 0, Wy = 0, Wys = 0;
  // the defaults of options (gb25_set_option changes the model's copies, never these)
  int chunk_levels = 12;     // MOMENTUM_ / TRACER_CHUNK_LEVELS
  int baro_ahead = 0;        // SUBCYCLE_LOOKAHEAD
  int split_tendencies = 1;  // SPLIT_TENDENCIES
  int tracer_rows_forced = 0;   // 1, 2: GB25_TRACER_ROWS in the environment of gb25_create forced it; 0: the library's rule
  bool wide() const { return slab || north_fold; }   // the sub-cycle runs on work arrays of its own
};

struct Dims {
  int nx, ny, nz;
  size_t elems() const { return (size_t)nx * ny * nz; }
};
// what the host sees of a field without its halos: a y-face field has the row Ny only below a wall (beyond a fold or a neighbour
// rank those faces are halo cells), a z-face field has Nz + 1 levels, a 2-D field one
inline Dims interior_dims(const ModelLayout& L, int id) {
  const FieldShape s = kFieldShapes[id];
  return {L.Nx, L.Ny + (s.v_shaped && L.north_wall ? 1 : 0), s.flat ? 1 : L.Nz + (s.z_faces ? 1 : 0)};
}
inline Dims halo_depth(const ModelLayout& L, int id) { return {L.H, L.H, kFieldShapes[id].flat ? 0 : L.H}; }
// ... with them (gb25_field_dims) ...
inline Dims host_dims(const ModelLayout& L, int id, bool include_halos) {
  const Dims d = interior_dims(L, id), h = halo_depth(L, id);
  return include_halos ? Dims{d.nx + 2 * h.nx, d.ny + 2 * h.ny, d.nz + 2 * h.nz} : d;
}
// ... and the device array: every y-face field keeps the row a wall needs, whatever lies north of the rank
inline Dims parent_dims(const ModelLayout& L, int id) {
  const FieldShape s = kFieldShapes[id];
  return {L.Nx + 2 * L.H, L.Ny + 2 * L.H + (s.v_shaped ? 1 : 0), s.flat ? 1 : L.Nz + 2 * L.H + (s.z_faces ? 1 : 0)};
}
// rows of the GLOBAL interior (the state dump of a rank of a 2-D decomposition)
inline int global_rows(const ModelLayout& L, int id) { return L.Ny_global + (kFieldShapes[id].v_shaped && !L.tripolar ? 1 : 0); }
// the sub-cycle's work array that stands for the 2-D field id
inline Dims wide_dims(const ModelLayout& L, int id) { return {L.Nx + 2 * L.W, parent_dims(L, id).ny + L.Wy + L.Wys, 1}; }
// (chunk, column) pairs of the partial sums the momentum look-ahead leaves and of the chunk bases of w on the fly: room for chunks
// of 6 levels, the least the options accept
inline size_t chunk_columns(const ModelLayout& L) { return (size_t)std::max(1, L.Nz / 6) * parent_dims(L, GB25_BT_V).elems(); }
// single folded domain: the buffer the image rows of eta, U, V, G.U, G.V pass through (k_tall_rows)
inline size_t tall_buf_elems(const ModelLayout& L) { return (size_t)5 * (L.Wy + 1) * wide_dims(L, GB25_ETA).nx; }

// The kernels address a parent array with 32-bit ELEMENT indices; the tendency kernels with 32-bit BYTE offsets from the
// first plane their block touches (tendency_kernels.hpp): a chunk of levels plus its stencil planes must stay below 2 GB.  The planes
// are counted by the rule the launches follow (tendency_plan.hpp, "the reach of the tendency kernels").
struct TendencyReach {
  bool ok;
  int klen, planes;     // levels of the longest chunk; with its stencil planes
  double plane, bytes;  // elements of one plane of a y-face field; what `planes` of them weigh
};
inline TendencyReach tendency_reach_ok(const ModelLayout& L, int chunk_levels, int real_bytes) {
  const Dims v = parent_dims(L, GB25_V);
  const double plane = (double)v.nx * v.ny;
  const LevelChunks c = level_chunks(L.Nz, L.H, chunk_levels, plane * real_bytes, true);
  const int planes = chunk_planes_at_creation(c);
  return {within_reach(c, planes), c.klen, planes, plane, planes * c.plane_bytes};
}

struct LayoutPlan {
  gb25_status status = GB25_OK;
  std::string refusal;   // why not, when status is not GB25_OK
  ModelLayout layout;
};

// cfg: the caller's configuration.  real_bytes: sizeof(real) of the library.  tracer_rows: the value of GB25_TRACER_ROWS, or null.
// The refusals come in a fixed order, the first that applies wins; the layout is complete only when none does.
inline LayoutPlan plan_layout(const gb25_config& cfg, int real_bytes, const char* tracer_rows) {
  LayoutPlan p;
  ModelLayout& L = p.layout;
  auto refuse = [&p](const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    p.status = GB25_ERR_INVALID_ARGUMENT;
    p.refusal = buf;
    return p;
  };
  L.Ry = cfg.ranks_y > 1 ? cfg.ranks_y : 1;
  if (cfg.Nx < 8 || cfg.Ny < 8 || cfg.Nz < 4 || cfg.halo < 4 || cfg.substeps < 1 || cfg.substeps > 4096 ||
      cfg.nranks < 1 || cfg.rank < 0 || cfg.rank >= cfg.nranks || cfg.nranks % L.Ry != 0 ||
      cfg.Nx % (cfg.nranks / L.Ry) != 0 || cfg.Ny % L.Ry != 0)
    return refuse("invalid configuration: need Nx,Ny >= 8, Nz >= 4, halo >= 4, 1 <= substeps <= 4096, nranks = Rx ranks_y, "
                  "Nx %% Rx == 0, Ny %% ranks_y == 0");
  if (cfg.slab_mode < 0 || cfg.slab_mode > 1)
    return refuse("slab_mode must be 0 (x halos by exchange iff nranks > 1) or 1 (always)");
  L.Nx_global = cfg.Nx; L.Ny_global = cfg.Ny; L.Nz = cfg.Nz; L.H = cfg.halo;
  L.Rx = cfg.nranks / L.Ry;
  L.rx = cfg.rank % L.Rx;
  L.ry = cfg.rank / L.Rx;
  L.Nx = cfg.Nx / L.Rx;
  L.Ny = cfg.Ny / L.Ry;
  L.j0 = L.ry * L.Ny;
  L.ys_open = L.ry > 0;
  L.yn_open = L.ry < L.Ry - 1;
  L.slab = cfg.nranks > 1 || cfg.slab_mode == 1;
  L.tripolar = cfg.grid_type >= GB25_GRID_TRIPOLAR;
  L.north_fold = L.tripolar && !L.yn_open;
  L.north_wall = !L.tripolar && !L.yn_open;
  if (tracer_rows) {
    if (strcmp(tracer_rows, "1") != 0 && strcmp(tracer_rows, "2") != 0)
      return refuse("GB25_TRACER_ROWS must be 1 or 2 (unset: the library's rule)");
    L.tracer_rows_forced = tracer_rows[0] - '0';
  }
  if (L.Nx < L.H) return refuse("slab narrower than the halo");
  // a rank of a 2-D decomposition steps on the staged sequence without the interior / edge split of the tendencies and
  // without the early pressure of the own columns
  L.split_tendencies = L.Ry > 1 ? 0 : 1;
  if (L.Ry > 1 && L.Ny < L.H + 2) return refuse("a rank's band of rows is narrower than the halo");
  {
    // Levels per chunk of the two tendency kernels (options MOMENTUM_ / TRACER_CHUNK_LEVELS): 24 where that still leaves four
    // rounds of blocks on the chip's 1024 block slots -- 1440 x 720 x 48: two chunks per column instead of four, +1.3 % steps/s
    // (415.5 -> 420.9 on one box; 1440 x 720 x 60 with the islands 280 -> 285.5), the start-up of a chunk's march paid half as
    // often --, 12 on narrower models: a 180-column rank of an 8-way decomposition would drop to one round and 0.47 -> 0.53 ms
    // per step (tools/slab_selfring.py) -- and on models so large that chunks of 24 levels lie beyond the kernels' reach.  The
    // chunking is the association of the column integrals of u, v: results differ in the last bits between the two, so a
    // bit-for-bit comparison of a wide single domain with its narrow ranks pins the options.
    const int nbx = (L.Nx + 63) / 64, nby = (L.Ny + 3) / 4;
    const bool four_rounds = (long)nbx * nby * std::max(1, L.Nz / 24) >= 4096;
    L.chunk_levels = four_rounds && tendency_reach_ok(L, 24, real_bytes).ok ? 24 : 12;
    const TendencyReach r = tendency_reach_ok(L, L.chunk_levels, real_bytes);
    const double elems = r.plane * parent_dims(L, GB25_W).nz;
    if (elems >= 2147483648.0 || !r.ok)
      return refuse("a %dx%dx%d slab has %.2g elements per 3-D array (%.1f GB) and %.2g per plane; the kernels index at most 2^31 "
                    "elements per array and %d planes of 2 GB together: decompose in x (nranks) so that the local slab is narrower",
                    L.Nx, L.Ny, L.Nz, elems, elems * real_bytes / 1e9, r.plane, r.planes);
  }
  // On launch-latency-bound grids the extra cross-stream hops of the sub-cycle look-ahead cost more than the
  // sub-cycle they hide (0.252 vs 0.262 ms/step at 360x180x24, 0.173 vs 0.185 at 128x64x8; +3.5 % at 1440x720x48).
  // A slab of a decomposition always uses it: there it also takes two exchanges off the critical path.
  L.baro_ahead = (L.slab || (long)cfg.Nx * cfg.Ny * cfg.Nz >= 8000000L) ? 1 : 0;
  L.sub = plan_substeps(cfg.substeps);
  if (cfg.grid_type < 0 || cfg.grid_type >= GB25_GRID_COUNT)
    return refuse("grid_type %d: 0 lat-lon, 1 lat-lon with the Gaussian islands, 2 lat-lon "
                  "through the curvilinear kernels, 3 tripolar, 4 tripolar with the Gaussian islands", cfg.grid_type);
  if (L.tripolar && (cfg.Nx % 2 || L.Ny < 2 * L.H))
    return refuse("the tripolar grid needs an even Nx and Ny >= 2 halo (the fold maps columns onto columns)");
  const int Ns = L.sub.Ns;
  if (L.slab) {
    // wide enough that after the Ns substeps the valid region still covers the slab's x HALO columns of eta, U, V: they are
    // computed here like the neighbour computes them (same inputs, same arithmetic) and no exchange follows the sub-cycle
    L.W = Ns + 1 + L.H;
    if (L.Nx < L.W) return refuse("slab width %d is narrower than the barotropic halo %d", L.Nx, L.W);
  }
  // folded grid: image rows beyond the pivot row, enough that what the last row's missing neighbour spoils (one row per
  // substep) never reaches the pivot row
  // (Oceananigans errors when the extended halo of its free surface exceeds the grid; so does this: with fewer rows the spoiled
  // rows would reach the pivot row and eta, U, V next to the fold would be wrong without a word)
  if (L.north_fold) {
    if (L.Ny - 2 < Ns + 1)
      return refuse("a folded grid needs Ny >= %d rows per rank for its %d effective substeps (the sub-cycle's "
                    "image rows beyond the pivot row: Ns + 1 of them, made from the rows south of it); this rank has %d", Ns + 3, Ns, L.Ny);
    L.Wy = Ns + 1;
  }
  // 2-D decomposition: wide halos in y as in x on the sides where a neighbour rank exists
  if (L.yn_open) L.Wy = L.W;
  if (L.ys_open) L.Wys = L.W;
  if ((L.yn_open || L.ys_open) && L.Ny < L.W)
    return refuse("a rank's band of %d rows is narrower than the barotropic halo %d", L.Ny, L.W);
  return p;
}
}  // namespace
