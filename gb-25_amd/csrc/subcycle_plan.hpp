// subcycle_plan.hpp -- which kernel form advances the split-explicit sub-cycle, on which arrays, over which range, in which launches,
// and what has to happen around them.  plan_subcycle() is the ONLY place any of this is decided; barotropic_impl (gb25_api.hip) binds
// the model's buffers to the plan and carries it out.  Plain C++, no HIP, no gb25_model: a host compiler can include this file alone
// (tests/test_subcycle_plan.py).  The forms, when each is chosen and the rules below in prose: DESIGN.md, "The forms of the sub-cycle".
#pragma once
namespace {
// tiles of the temporally blocked kernels: BT_TX columns by TY rows, BT_NT threads; BT_SMAX: the most substeps one launch takes (the
// weights travel in the launch's arguments; 24: the whole sub-cycle in one launch, k_barotropic_whole, with its BW_NT threads)
constexpr int BT_TX = 64, BT_NT = 256, BT_SMAX = 24, BW_NT = 1024;
// the one substep count k_barotropic_whole is instantiated for: the 21 effective substeps of SplitExplicitFreeSurface(substeps = 30);
// other counts take the blocked launches
constexpr int BW_NS = 21;

enum class SubcycleForm {
  PerSubstep,      // k_barotropic_substep<IMM, ORDER>: one launch per substep, (64, 4) threads
  PerSubstepCurv,  // k_barotropic_substep_curv: the same with per-point metrics
  Blocked,         // k_barotropic_multi<S, TY, IMM>: S substeps per launch on 64 x TY tiles
  BlockedCurv,     // k_barotropic_multi_curv<5, 17>
  Whole,           // k_barotropic_whole<21, IMM, TY>: every substep in one launch
};
enum class SubcycleArrays {
  Canonical,  // eta, U, V where the model keeps them, two scratch sets beside them (single domain)
  Wide,       // the work arrays: widened in x on a slab, tall beyond the pivot row on a folded grid
};

// everything the decision depends on
struct SubcycleSetting {
  int Nx, Ny, H;     // the rank's columns and rows, the halo
  int W, Wy, Wys;    // the work arrays' extra columns either side, rows beyond row Ny - 1, rows below row 0
  bool slab, curv, north_fold, ys_open, yn_open, immersed;
  int Ns;            // effective substeps
  int subcycle_block, substep_order, subcycle_whole;   // the options
  int n_cu, real_bytes;
  bool ahead;        // the sub-cycle of the NEXT step, into the partner buffers
  bool own_given;    // (slab) the caller handed over the pieces of the own columns, which still sit in the canonical arrays ...
  bool own_five;     // ... all five of them: eta, U, V, G.U, G.V
  bool composite, producers_fold;   // inside a composite step; the single-domain producers write the halo cells of their output
};

struct SubcycleLaunch {   // the flags of BaroMulti (kernels.hpp); the kernels of one substep per launch have none
  int s0, ns;             // the first substep and how many
  bool first, last;       // first: the averages start from zero in the kernel; last: eta, U, V <- the results, the averages published
};

struct SubcyclePlan {
  SubcycleForm form;
  SubcycleArrays arrays;
  int S, TY, ORDER;       // template parameters: substeps per launch (1: PerSubstep*), rows per tile (0: no tiles), SUBSTEP_ORDER
  bool IMM;
  int ilo, ihi, jlo, jhi, yo, top_open, wrap, sx, xo;   // Baro's geometry (kernels.hpp)
  int grid_x, grid_y, block_x, block_y;
  unsigned lds_bytes;     // dynamic LDS (Whole only)
  int Ns, n_launches;
  // ---- the work around the kernels, in the order it is carried out
  bool copy_state_in;     // single folded domain: eta, U, V, G.U, G.V into the tall arrays, then their image rows (k_tall_rows)
  bool zero_averages;     // one memset over the three averages (the kernels of several substeps start them from zero themselves)
  bool copy_own_first;    // slab: the own columns from the canonical into the work arrays (k_copy_interior_columns)
  bool own_in_place;      // ... or Whole reads them where they are
  bool write_layers;      // Whole also writes the y layers next to the walls of the new eta, U, V: no fill after the sub-cycle
  bool halo_images_on_last;   // the last launch also writes every halo cell derived from the new eta, U, V (BaroMulti::fold)
  bool publish_through_eb_out;   // the last launch also writes the averages into the canonical filtered-state arrays
  bool finalize_after;    // k_barotropic_finalize: eta, U, V <- the averages' source, over fin_nx x fin_ny cells
  bool publish_after;     // ... and a copy of the averages from the work arrays into the filtered-state arrays
  int out_halo, out_js, out_jn;   // BaroMulti: x halo columns and rows [out_js, out_jn) of the new eta, U, V that are written
  int fin_nx, fin_ny, fin_yo;     // the finalize launch: cells, and the array row of j = 0

  // launch i of n_launches.  A launch is `last` when the sub-cycle ends in it -- unless a finalize launch follows (rule 3)
  SubcycleLaunch launch(int i) const {
    const bool flags = form != SubcycleForm::PerSubstep && form != SubcycleForm::PerSubstepCurv;
    const int s0 = i * S, left = Ns - s0;
    return {s0, left < S ? left : S, flags && i == 0, flags && s0 + S >= Ns && !finalize_after};
  }
  // index into the form's table of kernel instances (gb25_api.hip): [IMM][ORDER], [IMM][S = 3, 5, 7], [IMM][TY = 17, 24]; no choice: 0
  int instance() const {
    switch (form) {
      case SubcycleForm::PerSubstep: return 2 * IMM + ORDER;
      case SubcycleForm::Blocked: return 3 * IMM + (S - 3) / 2;
      case SubcycleForm::Whole: return 2 * IMM + (TY == 17 ? 0 : 1);
      default: return 0;
    }
  }
};

inline SubcyclePlan plan_subcycle(const SubcycleSetting& c) {
  auto cdiv = [](int a, int b) { return (a + b - 1) / b; };
  SubcyclePlan p{};
  // Rule 1: option SUBSTEP_ORDER = 1 exists in the one-substep-per-launch kernel only: the temporally blocked ones keep the default order
  const int block = c.substep_order ? 1 : c.subcycle_block;
  const bool blocked = block > 1;
  // work arrays: a slab's are widened in x (filled by the exchange of BaroWide / BaroWideAhead before the sub-cycle), a folded grid's
  // are tall (image rows beyond the pivot row: a slab's come from its partner before the sub-cycle, a single domain's are made here)
  const bool wide = c.slab || c.north_fold;
  p.arrays = wide ? SubcycleArrays::Wide : SubcycleArrays::Canonical;
  p.IMM = c.immersed;
  p.ORDER = c.substep_order ? 1 : 0;
  p.Ns = c.Ns;
  p.jlo = -c.Wys;
  p.jhi = c.Ny + c.Wy;
  p.yo = c.H + c.Wys;
  p.top_open = (c.north_fold || c.yn_open) ? 1 : 0;
  p.sx = wide ? c.Nx + 2 * c.W : c.Nx + 2 * c.H;
  p.xo = wide ? c.W : c.H;
  // (a slab computes on [-W + 1, Nx + W - 1): the invalid rim grows by a column per substep and never reaches the interior)
  p.ilo = c.slab ? -c.W + 1 : 0;
  p.ihi = c.slab ? c.Nx + c.W - 1 : c.Nx;
  p.wrap = c.slab ? 0 : 1;
  p.copy_state_in = wide && !c.slab;
  p.zero_averages = !blocked;
  p.out_halo = c.slab ? c.H : 0;   // (a widened slab also writes the x halo columns of the new eta, U, V: nothing is exchanged after)
  p.out_js = c.ys_open ? -c.H : 0;   // (... and a rank of a 2-D decomposition the halo rows of its open sides)
  p.out_jn = c.yn_open ? c.Ny + c.H : c.Ny;
  const int cols = p.ihi - p.ilo, rows = p.jhi - p.jlo;
  const int rows_open = rows + p.top_open;   // (no wall: the curvilinear kernels carry the face row behind the last advanced row along)

  // Whole: a narrow slab has fewer tiles than the chip has CUs.  Rows per tile: 17 (125 KB of LDS) or, when only that brings the tile
  // count under the number of CUs, 24 (140 KB).  Float32 only: the Float64 build would need twice the LDS
  const int wcols = cdiv(cols, BT_TX);
  const int wty = wcols * cdiv(rows, 17) <= c.n_cu ? 17 : 24;
  const bool whole = blocked && !c.curv && c.slab && c.subcycle_whole && c.Ns == BW_NS && wcols * cdiv(rows, wty) <= c.n_cu &&
                     c.real_bytes == 4;
  // Rule 4: Whole reads the own columns in place only when it writes elsewhere -- the look-ahead's partner buffers; inside its own
  // step the results go into the very arrays other blocks are still loading their rings from
  p.own_in_place = whole && c.own_given && c.own_five && c.ahead;
  p.copy_own_first = c.own_given && !p.own_in_place;

  if (whole) {
    p.form = SubcycleForm::Whole;
    p.S = BW_NS; p.TY = wty;
    p.grid_x = wcols; p.grid_y = cdiv(rows, wty); p.block_x = BW_NT; p.block_y = 1;
    p.lds_bytes = 5u * (BT_TX + 2 * BW_NS) * (wty + 2 * BW_NS) * c.real_bytes;
    p.write_layers = c.own_given;
  } else if (blocked && c.curv) {
    // Rule 2: on a curvilinear grid every SUBCYCLE_BLOCK > 1 means 5 substeps on 64 x 17 tiles: the one instance that is built
    p.form = SubcycleForm::BlockedCurv;
    p.S = 5; p.TY = 17;
    p.grid_x = cdiv(cols, BT_TX); p.grid_y = cdiv(rows_open, p.TY); p.block_x = BT_NT; p.block_y = 1;
  } else if (blocked) {
    p.form = SubcycleForm::Blocked;
    p.S = block <= 3 ? 3 : (block <= 5 ? 5 : 7);
    p.TY = p.S == 5 ? 17 : 16;   // (5 substeps per launch: 64 x 17 tiles keep LDS under 40 KB -- four blocks per CU)
    p.grid_x = cdiv(cols, BT_TX); p.grid_y = cdiv(rows, p.TY); p.block_x = BT_NT; p.block_y = 1;
  } else {
    p.form = c.curv ? SubcycleForm::PerSubstepCurv : SubcycleForm::PerSubstep;
    p.S = 1; p.TY = 0;
    p.block_x = 64; p.block_y = 4;
    p.grid_x = cdiv(cols, p.block_x); p.grid_y = cdiv(c.curv ? rows_open : rows, p.block_y);
  }
  p.n_launches = cdiv(c.Ns, p.S);
  // Rule 3: a sub-cycle that fits ONE launch on the canonical arrays inside its own step would read and write eta, U, V in the same
  // launch: it is not `last`, and the finalize launch writes them
  p.finalize_after = !blocked || (p.n_launches == 1 && !wide && !c.ahead);
  p.publish_after = !blocked && wide;
  p.publish_through_eb_out = blocked && wide;
  p.halo_images_on_last = p.form == SubcycleForm::Blocked && !wide && c.producers_fold && c.composite && !p.finalize_after;
  p.fin_nx = c.Nx + 2 * p.out_halo;   // (a slab: with the x halo columns)
  p.fin_ny = p.out_jn - p.out_js;
  p.fin_yo = wide ? p.yo : c.H;
  return p;
}
}  // namespace
