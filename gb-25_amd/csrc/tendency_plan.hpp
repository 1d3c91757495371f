// tendency_plan.hpp -- what the launches at the centre of a step put on the device: the tile columns, chunks of levels and runs of
// chunks of the momentum kernel with its bottom-drag and finish launches, the blocks and the rows per lane of the tracer kernels, the
// columns and the form of the barotropic corrector, the columns, rows and block of the head of an unswept step.  plan_momentum(),
// plan_tracers(), plan_single(), plan_corrector() and the named HeadRequests are the ONLY place any of this is decided; momentum_impl,
// tracers_impl, catke_tendency_impl, corrector_impl and unswept_head (gb25_api.hip) bind the model's arrays and issue it.  The reach of
// the kernels' 32-bit byte offsets is stated here once, for gb25_create (model_layout.hpp), the chunk-level options and the launch loop.
// Plain C++, no HIP, no gb25_model: a host compiler can include this file alone (tests/test_tendency_plan.py).
// The vocabulary, the table of forms and the quirks in prose: DESIGN.md, "The launches of the tendency kernels and the corrector".
#pragma once
#include <algorithm>

#include "launch_plan.hpp"
#include "tile_sizes.hpp"
namespace {

// ---- the reach of the tendency kernels --------------------------------------------------------------------------------------------------
// The kernels' per-lane offsets are 32-bit BYTE offsets from the array pointers.  An array beyond that reach (4.4 GB per field for
// config 5 as one domain) takes several launches, each a run of chunks of levels whose planes -- stencil and halo layers included --
// lie within 2 GB of pointers rebased by `kofs` planes.  Normally: one launch, kofs = 0.
constexpr double TENDENCY_REACH = 2147483648.0;
struct LevelChunks {
  int Nz, H, kchunks, klen;   // chunks of levels and the levels of the longest one
  double plane_bytes;         // one plane of a y-face field, the larger of the two shapes
  bool rebased;               // a 3-D array is beyond the reach as a whole: every run rebases the pointers.  Otherwise kofs = 0
};
inline LevelChunks level_chunks(int Nz, int H, int chunk_levels, double plane_bytes, bool rebased) {
  const int kchunks = std::max(1, Nz / chunk_levels);
  return {Nz, H, kchunks, (Nz + kchunks - 1) / kchunks, plane_bytes, rebased};
}
// the lowest plane a run starting with chunk `first` touches: three levels below its first one, or a bottom halo layer
inline int run_base(const LevelChunks& c, int first) { return c.rebased ? std::max(0, first * c.klen + c.H - 4) : 0; }
// THE planes a run of the chunks first .. last touches, counted from its base: up to the highest plane of its last chunk -- window, w,
// top halo layer
inline int run_planes(const LevelChunks& c, int first, int last) { return std::min(c.Nz, (last + 1) * c.klen) + c.H + 5 - run_base(c, first); }
inline bool within_reach(const LevelChunks& c, int planes) { return planes * c.plane_bytes < TENDENCY_REACH; }
// the run that starts with chunk `first`: every following chunk whose highest plane is within reach.  Its first chunk is taken as it
// is: gb25_create and the chunk-level options have refused a chunking whose single chunk is out of reach (chunk_planes_at_creation)
struct ChunkRun {
  int first, count, kofs;
};
inline ChunkRun chunk_run(const LevelChunks& c, int first) {
  int end = first + 1;
  while (end < c.kchunks && within_reach(c, run_planes(c, first, end))) end++;
  return {first, end - first, run_base(c, first)};
}
// What gb25_create and the chunk-level options price a chunking at: a rebased run of the first chunk alone -- klen + 9 planes, the
// most a run of one chunk touches -- and one plane more.  The margin is older than the runs; it stays because it decides which grids
// fall back from chunks of 24 levels to 12 and which are refused, and the chunking is the association of the column integrals of
// u, v: without it a grid on the border would change its bits.  (klen + 9 holds because the halo is at least 4 planes deep -- the base
// of chunk 0 is plane H - 4 -- and a chunk is no longer than the column: plan_layout refuses halo < 4 before it asks.  A smaller
// minimum halo would change this count, and with it which grids fall back or are refused.)
constexpr int CREATION_MARGIN_PLANES = 1;
inline int chunk_planes_at_creation(LevelChunks c) {
  c.rebased = true;
  return run_planes(c, 0, 0) + CREATION_MARGIN_PLANES;
}

// ---- momentum -----------------------------------------------------------------------------------------------------------------------------
// Tile columns of the momentum kernel that read the slab's own columns only (u, v up to 3 columns, w up to 2 columns
// away): [1, end).  Empty (end = 1) when the slab is too narrow.
inline int interior_tile_columns_end(int Nx) {
  const int nbx = (Nx + V2_TX - 1) / V2_TX;
  return std::max(1, std::min(nbx - 1, (Nx - 3) / V2_TX));
}
// the geometry's half of the split of a slab's tendencies into the Interior and Edges passes (the options' half: tendencies_split,
// gb25_api.hip): an interior tile column exists, and no rows arrive last -- those beyond a fold, or of a neighbour in y
inline bool momentum_splittable(const LaunchFacts& f) {
  return f.slab && interior_tile_columns_end(f.Nx) > 1 && !f.north_fold && f.Ry == 1;
}
struct MomentumPlan {
  int nbx, nby, kchunks;        // tile columns of the grid, rows of tiles (zipper fold: the y faces on the fold line have a tendency too), chunks
  int n, nlead, bx0, bx1;       // the tile columns of the pass, as TileCols takes them (tendency_kernels.hpp)
  int interior_end;             // interior_tile_columns_end
  bool splittable;              // momentum_splittable
  int drag_i_first, drag_n;     // columns of the bottom-drag flux launch
  bool finish;                  // the look-ahead's finish kernel follows this pass
  LevelChunks chunks;           // for chunk_run
  int nb() const { return n * nby * kchunks; }
};
inline MomentumPlan plan_momentum(Pass pass, const LaunchFacts& f) {
  MomentumPlan p{};
  p.nbx = (f.Nx + V2_TX - 1) / V2_TX;
  p.nby = (f.v_rows + MOMENTUM_TY - 1) / MOMENTUM_TY;
  p.chunks = level_chunks(f.Nz, f.H, f.mom_chunk_levels, (double)f.pl_v * f.real_bytes, !((double)f.w_elems * f.real_bytes < TENDENCY_REACH));
  p.kchunks = p.chunks.kchunks;
  const int hi = p.interior_end = interior_tile_columns_end(f.Nx);
  p.splittable = momentum_splittable(f);
  p.n = p.nlead = p.nbx;   // Whole: every tile column
  if (pass == Pass::Interior) {   // 1 .. hi - 1
    p.n = p.nlead = hi - 1;
    p.bx0 = 1;
  }
  if (pass == Pass::Edges) {   // 0, then hi .. nbx - 1
    p.n = 1 + p.nbx - hi;
    p.nlead = 1;
    p.bx1 = hi;
  }
  // A slab's interior pass runs before the x halos arrive: face 0, the one that reads v of the west halo column, waits for the edge pass
  p.drag_i_first = pass == Pass::Interior ? 1 : 0;
  p.drag_n = pass == Pass::Edges ? 1 : f.Nx - p.drag_i_first;
  p.finish = pass != Pass::Interior;
  return p;
}

// ---- tracers ------------------------------------------------------------------------------------------------------------------------------
// Rows per lane of the tracer kernel (tracer_tile_rows2, tendency_kernels.hpp).  Two where the instance exists (flat grid, order 5),
// the launch covers a whole single domain -- a slab or a rank of a mesh keeps one, so that the bitwise comparisons of a decomposition
// with the single domain compare the two forms --, the model is Float32 (Float64: 252 VGPRs, two waves, the launch 5 % slower) and the
// blocks of 8 rows still number TRACER_ROWS2_MIN_BLOCKS: measured 1440 x 720 x 48 (4140 blocks) +1 % steps/s, 720 x 720 x 48 (2160)
// +-0, 720 x 360 x 48 (2160 of 12 levels) -1.7 %, 360 x 360 x 48 -4 %.  GB25_TRACER_ROWS = 1 | 2 in the
// environment of gb25_create forces the value wherever the instance exists.
constexpr long TRACER_ROWS2_MIN_BLOCKS = 4096;
struct TracerPlan {
  int rows;                    // per lane
  int nbx, nby, kchunks, nb;   // blocks of 64 x 4 threads: four waves of `rows` rows each
};
inline TracerPlan plan_tracers(const LaunchFacts& f) {
  const int nbx = (f.Nx + V3_OUT - 1) / V3_OUT, kchunks = std::max(1, f.Nz / f.trc_chunk_levels);
  const bool exists = !f.immersed && !f.curvilinear && f.tracer_order == 5;
  int rows = (!f.slab && f.real_bytes == 4 && (long)nbx * ((f.Ny + 7) / 8) * kchunks >= TRACER_ROWS2_MIN_BLOCKS) ? 2 : 1;
  if (f.tracer_rows_forced) rows = f.tracer_rows_forced;
  if (!exists) rows = 1;
  const int nby = (f.Ny + 4 * rows - 1) / (4 * rows);
  return {rows, nbx, nby, kchunks, nbx * nby * kchunks};
}
// the one-tracer kernel (CATKE's e): two columns per lane, one row
inline TracerPlan plan_single(const LaunchFacts& f) {
  const int nbx = (f.Nx + V3_PAIR - 1) / V3_PAIR, nby = (f.Ny + 3) / 4, kchunks = std::max(1, f.Nz / f.trc_chunk_levels);
  return {1, nbx, nby, kchunks, nbx * nby * kchunks};
}

// ---- the barotropic corrector -------------------------------------------------------------------------------------------------------------
enum class Part {
  All,           // every column this model corrects (a slab of a decomposition includes its x-halo columns)
  OwnColumns,    // the slab's own columns only (needs no halo data: runs while the last exchanges are in flight)
  HaloColumns,   // the x-halo columns only.  The G^n / G^- exchange happens once, with All or OwnColumns
};
struct CorrectorRequest {
  Part part;
  bool may_use_colsum;   // only inside a composite time step, where nothing can have touched u, v since the AB2 kernel
  static constexpr CorrectorRequest all(bool may_use_colsum) { return {Part::All, may_use_colsum}; }
  static constexpr CorrectorRequest own_columns() { return {Part::OwnColumns, true}; }
  static constexpr CorrectorRequest halo_columns() { return {Part::HaloColumns, true}; }
};
enum class CorrectorForm {
  Nothing,   // the halo columns of a single domain
  Cells,     // k_corrector_cells: one thread per cell, the column integrals at hand
  Sweep,     // k_corrector: one thread per column, marching up the levels
};
struct CorrectorPlan {
  CorrectorForm form;
  Cols cols;
  int j0, nj;          // rows: the own ones (the halo rows of a rank of a 2-D decomposition arrive corrected: group 10 travels after this)
  bool reads_colsum;   // Sweep: takes the column integrals instead of summing the column itself
  bool caches;         // G^- <- G^n follows, and the column integrals are used up
};
// colsum_valid, halo_colsum_valid: the model holds the column integrals of its own / of its x-halo columns (validity.hpp)
inline CorrectorPlan plan_corrector(const CorrectorRequest& rq, const LaunchFacts& f, bool colsum_valid, bool halo_colsum_valid) {
  const bool halo = rq.part == Part::HaloColumns;
  if (halo && !f.slab) return {CorrectorForm::Nothing, NO_COLS, 0, 0, false, false};
  Cols c{0, f.Nx, INT_MAX, 0};
  if (rq.part == Part::All && f.slab) c = Cols{-f.H, f.Nx + 2 * f.H, INT_MAX, 0};
  if (halo) c = Cols{-f.H, 2 * f.H, 0, f.Nx};
  // one thread per cell where the column integrals are at hand: the own columns of a slab, and its x-halo columns when
  // the integrals came with the 3-D bundle (group 0 carries the owner's; marching 16 columns x Ny threads up 48 levels
  // for them was 36 us of latency on the critical path of a 180-column rank)
  const bool at_hand = rq.may_use_colsum && (halo ? halo_colsum_valid : colsum_valid);
  const bool cells = f.slab && rq.part != Part::All && at_hand;
  return {cells ? CorrectorForm::Cells : CorrectorForm::Sweep, c, 0, f.Ny, at_hand && !halo, !halo};
}

// ---- the head of a step whose corrector is not the sweep -----------------------------------------------------------------------------------
// du, dv (k_corrector_2d) on `cols`, rows j0 + [0, nj); the chunk bases of w (k_w_bases) on `bases`; both in blocks of bx x by threads;
// G^- <- G^n where `cache` says so.  An empty range launches nothing.  carry_w: the step's tendency kernels carry w (StepRoute).
// the columns whose chunk bases a single domain's tendency kernels read: the w tiles reach two columns out
inline Cols wide_bases(const LaunchFacts& f) { return {-2, f.Nx + 4, INT_MAX, 0}; }
struct HeadRequest {
  Cols cols;
  int j0, nj;
  Cols bases;
  int bx, by;
  bool cache;
  static Cols own(const LaunchFacts& f) { return {0, f.Nx, INT_MAX, 0}; }
  // single domain, the corrector in its consumers: the own faces up to the wall face of v
  static HeadRequest in_consumers(const LaunchFacts& f, bool carry_w) {
    return {own(f), 0, f.Ny + 1, carry_w ? wide_bases(f) : NO_COLS, 64, 4, true};
  }
  // single domain, the corrector through the tracer kernel: du, dv on the own faces (rows of y faces: [0, Ny) on a folded grid,
  // [0, Ny] below a wall) ...
  static HeadRequest through_tracers_faces(const LaunchFacts& f) { return {own(f), 0, f.Ny + (f.north_fold ? 0 : 1), NO_COLS, 64, 4, false}; }
  // ... and, once their halo cells are filled, the chunk bases
  static HeadRequest through_tracers_bases(const LaunchFacts& f) { return {NO_COLS, 0, 0, wide_bases(f), 64, 4, false}; }
  // a slab's own columns (LazyHead / OwnColumns): chunk bases of w on the columns [0, Nx - 2] (their u faces are own columns), before
  // the interior momentum pass overwrites the chunk sums they are made from.  (A rank of a 2-D decomposition has no interior pass:
  // nothing here but the exchange of the tendency pairs, everything else in mesh_rank when every halo is in)
  static HeadRequest slab_own_columns(const LaunchFacts& f, bool carry_w) {
    const bool own_pass = f.Ry == 1;
    return {own_pass ? own(f) : NO_COLS, 0, f.Ny + 1, own_pass && carry_w ? Cols{0, f.Nx - 1, INT_MAX, 0} : NO_COLS, 64, 4, true};
  }
  // a slab's x-halo strips in blocks of 16 x 16, and the chunk bases of w on the columns -2, -1 and Nx - 1, Nx, Nx + 1
  static HeadRequest slab_halo_strips(const LaunchFacts& f, bool carry_w) {
    return {Cols{-f.H, 2 * f.H, 0, f.Nx}, 0, f.Ny + 1, carry_w ? Cols{-2, 5, 0, f.Nx - 1} : NO_COLS, 16, 16, false};
  }
  // a rank of a 2-D decomposition: everything at once -- own cells, halo columns, halo rows of the open sides (corners included);
  // rows: from the southern halo rows (or row 0) to the last northern halo row of the cell-shaped arrays (or the wall face)
  static HeadRequest mesh_rank(const LaunchFacts& f, bool carry_w) {
    const int hs = f.ys_open ? f.H : 0;
    return {Cols{-f.H, f.Nx + 2 * f.H, INT_MAX, 0}, -hs, hs + f.Ny + (f.yn_open ? f.H : 1), carry_w ? wide_bases(f) : NO_COLS, 64, 4, false};
  }
};

}  // namespace
