// launch_plan.hpp -- what the three launch helpers of a step put on the device: which halo-fill kernels over which cells, which columns
// and block shape the w kernel gets, which form of the pressure kernel over which box.  plan_fill(), w_columns() and plan_pressure()
// are the ONLY place any of this is decided; fill_halos_impl, compute_w_impl and compute_p_impl (gb25_api.hip) bind the model's arrays
// to the plan and issue it.  Plain C++, no HIP, no gb25_model: a host compiler can include this file alone (tests/test_launch_plan.py).
// The vocabulary, the table of forms and the quirks in prose: DESIGN.md, "The launches of a fill, of w and of the pressure".
// (The tendency kernels, the corrector and the head of an unswept step: tendency_plan.hpp, on the same LaunchFacts, Cols and Pass.)
#pragma once
#include <climits>
namespace {

// everything the plans depend on, filled from the model in one place (launch_facts, gb25_api.hip)
struct LaunchFacts {
  int Nx, Ny, Nz, H;   // the rank's columns, rows and levels, the halo
  int sy_c, sy_v;      // parent rows of a cell-shaped and of a y-face array
  bool x_periodic;     // the x halos are the model's own columns (single domain)
  bool north_fold;     // the northern edge is the zipper fold
  int pivot_slaved;    // option FOLD_PIVOT_SLAVED: the fold fill writes one more row (0 | 1)
  bool slab;           // x halos come from a neighbour
  bool ys_open, yn_open;   // a southern / northern neighbour rank exists
  bool fill_fused;     // option FILL_FUSED
  bool curvilinear;
  // ... and what the plans of the tendency kernels and the corrector read besides (tendency_plan.hpp)
  int pl_c, pl_v;      // elements of one plane of a cell-shaped and of a y-face array
  long w_elems;        // elements of w, the tallest 3-D array
  int real_bytes;      // sizeof(real)
  int mom_chunk_levels, trc_chunk_levels;   // options MOMENTUM_ / TRACER_CHUNK_LEVELS
  int v_rows;          // rows of y faces a launch covers
  int Ry;              // ranks in y of the decomposition
  bool immersed;
  int tracer_order;         // 5 | 7
  int tracer_rows_forced;   // 1, 2: GB25_TRACER_ROWS forced it; 0: the rule of plan_tracers
};

// columns i0 + [0, ni); from column skip_from on: + skip.  Two ranges in one launch: the first ends before skip_from, the second begins
// `skip` columns further on.  (The kernels of the unswept head take these four numbers; the w and pressure kernels take the ranges.)
struct Cols {
  int i0, ni, skip_from, skip;
  int na() const { return skip_from >= i0 + ni ? ni : skip_from > i0 ? skip_from - i0 : 0; }   // columns of the first range
  int nb() const { return ni - na(); }                                                        // ... of the second
  int b0() const { return nb() ? i0 + na() + skip : 0; }                                      // its first column (0 when there is none)
};
constexpr Cols NO_COLS{0, 0, INT_MAX, 0};

// ---- halo fills -----------------------------------------------------------------------------------------------------------------------
enum class Fields3 : unsigned { None = 0, UV = 1, TS = 2, E = 4 };   // a set: Fields3::UV | Fields3::TS.  (E: the TKE tracer of CATKE)
constexpr Fields3 operator|(Fields3 a, Fields3 b) { return Fields3((unsigned)a | (unsigned)b); }
constexpr bool has(Fields3 set, Fields3 f) { return ((unsigned)set & (unsigned)f) != 0; }
enum class Fields2 {
  None,
  Prognostic,   // eta, U, V
  Given,        // the caller's Halo2: G.U, G.V; du, dv with their fold signs; the look-ahead's eta, U, V
};
enum class Columns {
  Own,                // y / z layers on the own columns
  OwnWithPeriodicX,   // ... and the periodic x copy where the grid is periodic in x (a slab's x halos arrive by exchange: no copy)
  Extended,           // y / z layers on the x-halo columns too (a slab, after the neighbours' columns were unpacked)
};
struct FillRequest {
  Fields3 f3;
  Fields2 f2;
  Columns cols;
  int n_given = 0;   // Given: how many 2-D fields the caller's Halo2 holds (set by whoever binds it: fill_halos_impl)
  constexpr int n2() const { return f2 == Fields2::None ? 0 : f2 == Fields2::Prognostic ? 3 : n_given; }
  constexpr bool empty() const { return f3 == Fields3::None && f2 == Fields2::None; }
  // the requests that recur
  static constexpr FillRequest everything(Columns c) { return {Fields3::UV | Fields3::TS, Fields2::Prognostic, c}; }
  static constexpr FillRequest everything_periodic_x() { return everything(Columns::OwnWithPeriodicX); }
  static constexpr FillRequest uv(Columns c) { return {Fields3::UV, Fields2::None, c}; }
  static constexpr FillRequest ts(Columns c) { return {Fields3::TS, Fields2::None, c}; }
  static constexpr FillRequest e(Columns c) { return {Fields3::E, Fields2::None, c}; }
  static constexpr FillRequest uvts(Columns c) { return {Fields3::UV | Fields3::TS, Fields2::None, c}; }   // the 3-D bundle
  static constexpr FillRequest flat(Fields2 f, Columns c) { return {Fields3::None, f, c}; }                // 2-D fields only
  static constexpr FillRequest flat_extended(Fields2 f = Fields2::Prognostic) { return flat(f, Columns::Extended); }
};

enum class FillKernel { Y, YZ, Fold, X, Fused };   // k_fill_y, k_fill_yz, k_fill_fold, k_fill_x, k_fill_fused (kernels.hpp)
struct FillLaunch {
  FillKernel kernel;
  unsigned gx, gy, gz;   // the grid; blocks of 256 threads
  int i0, ni, jlo;       // Y, YZ: columns i0 + [0, ni); YZ: first row of the z layers
  int n2;                // 2-D fields it carries (the 3-D ones are the request's)
  bool flat;             // runs on the copy of the grid with Nz = 0: Y takes its 2-D branch, X sees no row of a 3-D field
  int rows_c, rows_v;    // X, Fused: rows of a cell-shaped / y-face 3-D array, all levels
  int nbx, nb_yz, nbr;   // Fused: blocks per row of the y / z part, blocks of that part, blocks of the x copy per field
};
enum class FillForm { Flat2D, FoldedSingle, FlatY, Fused, Layers };   // the rows of the table in DESIGN.md
struct FillPlan {
  FillForm form;
  int n;   // launches, issued in order
  FillLaunch l[3];
};

inline FillPlan plan_fill(const FillRequest& rq, const LaunchFacts& f) {
  FillPlan p{};
  const unsigned nbx = (unsigned)((f.Nx + 255) / 256);
  const int n2 = rq.n2();
  const bool only_2d = rq.f3 == Fields3::None, folded_single = f.north_fold && !f.slab;
  const bool x_copy = rq.cols == Columns::OwnWithPeriodicX && f.x_periodic;
  auto add = [&p](FillLaunch l) { p.l[p.n++] = l; };
  // the 2-D route: the y layer, the rows beyond the fold, the periodic x copy, each of the 2-D fields alone.
  //  * a 2-D-only request with the periodic x copy takes it (a slab has no copy to make: the y layer alone);
  //  * on a folded single domain a 2-D-only request takes it whatever columns it asked for, with the caller's Halo2 when one is given.
  if (only_2d && (rq.cols == Columns::OwnWithPeriodicX || folded_single)) {
    p.form = FillForm::Flat2D;
    add({FillKernel::Y, nbx, 1, 1, 0, f.Nx, 0, n2, true});
    if (folded_single)   // (a slab's rows beyond the fold come from its partner rank: slab_step.hpp)
      add({FillKernel::Fold, nbx, (unsigned)(f.H + f.pivot_slaved), 1, 0, f.Nx, 0, n2, false});
    // (k_fill_x is launched with 4 + n2 slices however many 3-D fields are present: here the first four see zero rows and fall through)
    if (f.x_periodic) add({FillKernel::X, (unsigned)(((long)f.sy_v * 2 * f.H + 255) / 256), (unsigned)(4 + n2), 1, 0, f.Nx, 0, n2, true});
    return p;
  }
  const int rows_c = f.sy_c * (f.Nz + 2 * f.H), rows_v = f.sy_v * (f.Nz + 2 * f.H);
  const unsigned x_blocks = (unsigned)(((long)rows_v * 2 * f.H + 255) / 256);
  // a folded single domain ALWAYS does y / z layers on its own columns, the rows beyond the fold (H + pivot_slaved of them, on Nz + 2
  // planes and one more for the 2-D fields), then the periodic x copy over all of them -- whatever columns were asked for
  if (folded_single) {
    p.form = FillForm::FoldedSingle;
    add({FillKernel::YZ, nbx, (unsigned)(f.Nz + 1 + f.Ny), 1, 0, f.Nx, 0, n2, false});
    add({FillKernel::Fold, nbx, (unsigned)(f.H + f.pivot_slaved), (unsigned)(f.Nz + 2 + (n2 ? 1 : 0)), 0, f.Nx, 0, n2, false});
    add({FillKernel::X, x_blocks, (unsigned)(4 + n2), 1, 0, f.Nx, 0, n2, false, rows_c, rows_v});
    return p;
  }
  const bool extended = rq.cols == Columns::Extended;
  const int i0 = extended ? -f.H : 0, ni = extended ? f.Nx + 2 * f.H : f.Nx;
  if (only_2d) {   // (Own or Extended: the y layer of the 2-D fields, no x copy)
    p.form = FillForm::FlatY;
    add({FillKernel::Y, (unsigned)((ni + 255) / 256), 1, 1, i0, ni, 0, n2, true});
    return p;
  }
  if (f.fill_fused && x_copy) {   // single domain: y, z and periodic x in one launch
    p.form = FillForm::Fused;
    const int nb_yz = (int)nbx * (f.Nz + 1 + f.Ny), nbr = (int)x_blocks;
    add({FillKernel::Fused, (unsigned)(nb_yz + nbr * (4 + n2)), 1, 1, 0, f.Nx, 0, n2, false, rows_c, rows_v, (int)nbx, nb_yz, nbr});
    return p;
  }
  // z layers: the own rows; an extended fill on a rank of a 2-D decomposition also the halo rows of its OPEN sides -- they arrived with
  // the neighbours' rows, interior levels only
  p.form = FillForm::Layers;
  const int jlo = (extended && f.ys_open) ? -f.H : 0, jhi = (extended && f.yn_open) ? f.Ny + f.H : f.Ny;
  add({FillKernel::YZ, (unsigned)((ni + 255) / 256), (unsigned)(f.Nz + 1 + (jhi - jlo)), 1, i0, ni, jlo, n2, false});
  if (x_copy) add({FillKernel::X, x_blocks, (unsigned)(4 + n2), 1, 0, f.Nx, 0, n2, false, rows_c, rows_v});
  return p;
}

// ---- w ----------------------------------------------------------------------------------------------------------------------------------
// The passes of compute_w_impl and momentum_impl over a slab whose tendencies are split around the arrival of the x-halo bundle.
enum class Pass {
  Whole,      // w: the whole extended range -H+1 .. Nx+H-2; momentum: every tile column
  Interior,   // w: the own columns 0 .. Nx-2 (they read own columns only); momentum: the interior tile columns -- while the bundle travels
  Edges,      // w: the two strips Interior left out; momentum: the edge tile columns, then whatever follows the complete evaluation
};
struct WColumns {
  Cols cols;
  int rows;     // -H+1 .. Ny+H-2
  int bx, by;   // the block: 64 x 4; narrow strips 16 x 16 (a 64-wide block would be three-quarters empty)
};
inline WColumns w_columns(Pass pass, const LaunchFacts& f) {
  Cols c{-f.H + 1, f.Nx + 2 * f.H - 2, INT_MAX, 0};
  if (pass == Pass::Interior) c = Cols{0, f.Nx - 1, INT_MAX, 0};
  if (pass == Pass::Edges) c = Cols{-f.H + 1, 2 * f.H - 1, 0, f.Nx - 1};
  const bool wide = c.ni >= 64;
  return {c, f.Ny + 2 * f.H - 2, wide ? 64 : 16, wide ? 4 : 16};
}

// ---- hydrostatic pressure ---------------------------------------------------------------------------------------------------------------
// the written columns (column i0 - 1 of each range is read as the west neighbour of its first x difference) and rows
struct PressureBox {
  Cols cols;
  int j_first, j_last;
  static PressureBox of(Cols c, const LaunchFacts& f) { return {c, -f.H + 1, f.Ny + f.H - 2}; }
  static PressureBox whole(const LaunchFacts& f) { return of(Cols{-f.H + 1, f.Nx + 2 * f.H - 2, INT_MAX, 0}, f); }   // -H+1 .. Nx+H-2
  static PressureBox own_columns(const LaunchFacts& f) { return of(Cols{0, f.Nx, INT_MAX, 0}, f); }                  // 0 .. Nx-1
  // the strips next to a slab's x halos: west -H+1 .. 0 (redoes column 0, whose x difference read a stale halo column), east Nx .. Nx+H-2
  static PressureBox strips(const LaunchFacts& f) { return of(Cols{-f.H + 1, 2 * f.H - 1, 1, f.Nx - 1}, f); }
};
constexpr int PRESSURE_ROWS = 4;   // rows per thread of form 3 (PR, kernels.hpp)
struct PressurePlan {
  int form;          // 1: tiles (a wave = 16 columns x 4 rows, 15 x 3 written), 2: one row per thread, 3: PRESSURE_ROWS rows per thread
  unsigned gx, gy;   // the grid; blocks of 64 x 4
  int tiles_a;       // blocks in x of the first column range
};
// strips and narrow slabs: with four rows per thread a 180-column slab is 138 blocks on 256 CUs and the fp64 chains run at their latency
// (0.14 ms, against 0.31 ms for 1440 columns): one row per thread (4x the waves, 2.03 evaluations per cell).  The narrowest of them on
// the lat-lon grid take the tile form: 5.6x the waves of the four-row form, 1.42 evaluations per cell, rows of 64 B.  Same box, one
// rank alone: 180 columns 0.497 -> 0.484 ms per step, 360: 0.808 -> 0.794, the 4 x 2 mesh rank 0.518 -> 0.510; but 720 columns 1.358 ->
// 1.401 and the folded grid's slabs 0.614 -> 0.617 (180) and 0.978 -> 1.018 (360) beside their heavier curvilinear neighbours: those
// keep the one-row form.  forced_form (option PRESSURE_FORM) forces one form, on any grid: the kernels read no horizontal metric.
inline PressurePlan plan_pressure(const PressureBox& box, const LaunchFacts& f, int forced_form) {
  const int na = box.cols.na(), nb = box.cols.nb();
  const int ncol = na + 1, ncol_b = nb ? nb + 1 : 0;   // written columns + the helper column
  const int nrow = box.j_last - box.j_first + 1;
  const int tiles_a = (ncol + 62) / 63, tiles_b = (ncol_b + 62) / 63, rows4 = (nrow + PRESSURE_ROWS * 4 - 1) / (PRESSURE_ROWS * 4);
  const bool narrow = (tiles_a + tiles_b) * rows4 < 1024;
  const int form = forced_form ? forced_form : (narrow && !f.curvilinear && ncol + ncol_b <= 400) ? 1 : narrow ? 2 : 3;
  if (form == 1) {
    const int ta = (na + 14) / 15, tb = (nb + 14) / 15;
    return {1, (unsigned)(ta + tb), (unsigned)((nrow + 11) / 12), ta};
  }
  if (form == 2) return {2, (unsigned)(tiles_a + tiles_b), (unsigned)((nrow + 3) / 4), tiles_a};
  return {3, (unsigned)(tiles_a + tiles_b), (unsigned)rows4, tiles_a};
}

}  // namespace
