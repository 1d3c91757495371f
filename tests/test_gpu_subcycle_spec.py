"""The split-explicit sub-cycle on the device, cell by cell: tests/subcycle_spec.py (proved on the CPU oracle by
tests/test_subcycle_spec.py, whose inputs and drive are used here) applied to the fields a caller reads before and after ONE
gb25_ab2_step -- which always runs the sub-cycle in-step, on a single domain, outside a composite step.

Forms (csrc/subcycle_plan.hpp; form_of names the one a case takes and its kernel instance):
  PerSubstep      k_barotropic_substep<IMM, ORDER>: subcycle_block = 1, or substep_order = 1 (rule 1) -- flat and island lat-lon;
  Blocked         k_barotropic_multi<3 | 5 | 7, 16 | 17 | 16, IMM>: subcycle_block = 3, 5, 7 -- with the remainder launch, and with
                  Ns <= S the single launch that is not `last` and k_barotropic_finalize behind it (rule 3);
  PerSubstepCurv  k_barotropic_substep_curv, BlockedCurv  k_barotropic_multi_curv<5, 17> (rule 2: any block > 1) -- on the canonical
                  arrays (lat_lon_as_curvilinear) and on the tall arrays behind k_tall_rows (tripolar, gaussian_islands).
Not here: k_barotropic_whole and the widened arrays of a slab, the look-ahead sub-cycle of gb25_loop ("The sub-cycle,
cell by cell": both are tied bit for bit to forms judged here).

Every case asserts, after checking through get_option and substepping() that it got the configuration it asked for:
  * every interior cell of eta, U, V within the spec's bound (the two conditions on the inputs, growth < 2 and signal, included);
  * eta_bar, U_bar, V_bar equal eta, U, V bit for bit on the interior;
  * the interior outputs do not change by a bit when the halo cells of eta, U, V hold other noise: no form reads a halo cell
    (the lat-lon kernels wrap by index; the tall arrays' images are made from interior rows);
  * outside the interior, exactly what the form may write (read off barotropic_impl and the kernels):
      eta, U, V          nothing, in every form: k_barotropic_finalize and the `last` blocked launch write [0, Nx) x [0, Ny) --
                         the northern wall row of V and every halo cell keep their bits;
      eta_bar, U_bar, V_bar (handed to the call full of noise)
        PerSubstep, PerSubstepCurv on the canonical arrays: one memset over the three arrays, then the interior is accumulated:
                         every cell outside the interior is zero;
        Blocked, BlockedCurv on either array set: the averages start from zero in the kernel and only owned interior cells are
                         written (into the canonical arrays directly, or through eb_out): every cell outside keeps its bits;
        PerSubstepCurv on the tall arrays: the publish copy takes columns [0, Nx) of EVERY row of the filtered arrays from the
                         tall averages -- zero below row 0 and from row Ny + Ns + 1 on, the averages of the image rows in
                         between (finite; nothing reads them) -- and the x halo columns keep their bits.
Each case prints its worst residual / bound per field."""
import numpy as np
import pytest

import gb25_amd as gb
import subcycle_spec as sc
import test_subcycle_spec as tss
from helpers import counter_rng

pytestmark = pytest.mark.gpu

BUILDS = ["Float32", "Float64"]
NS = {30: 21, 14: 10, 6: 4, 3: 2}
LATLON_FORMS = [(1, 0), (3, 0), (5, 0), (7, 0), (5, 1)]            # (subcycle_block, substep_order)
# (70, 13): a ragged second column tile, Ny below one tile; (16, 9): Nx below the ring of 7 -- the ring wraps more than once;
# (129, 35): one column in the third tile, Ny = 2 * 17 + 1 = 2 * 16 + 3 -- one-row and three-row last tiles
FLAT_SHAPES = [(70, 13, 4), (16, 9, 4), (129, 35, 4)]
# dt (at substeps = 30; dtau is kept for other counts) per (grid, shape): growth of |A| below 2 at the narrowest cell
DT = {("simple_lat_lon", (70, 13, 4)): 100.0, ("simple_lat_lon", (16, 9, 4)): 300.0, ("simple_lat_lon", (129, 35, 4)): 40.0,
      ("gaussian_islands_lat_lon", (48, 24, 6)): 100.0, ("gaussian_islands_lat_lon", (70, 27, 6)): 60.0,
      ("lat_lon_as_curvilinear", (48, 24, 6)): 100.0, ("lat_lon_as_curvilinear", (80, 40, 6)): 50.0,
      ("tripolar", (48, 24, 6)): 20.0, ("tripolar", (80, 40, 6)): 8.0,
      ("gaussian_islands", (48, 24, 6)): 20.0, ("gaussian_islands", (80, 40, 6)): 8.0}
CASES = [("simple_lat_lon", s, 30, blk, o) for s in FLAT_SHAPES for blk, o in LATLON_FORMS]
CASES += [("gaussian_islands_lat_lon", (48, 24, 6), 30, blk, o) for blk, o in LATLON_FORMS]
CASES += [("gaussian_islands_lat_lon", (70, 27, 6), 30, blk, o) for blk, o in ((1, 0), (3, 0), (5, 0), (7, 0))]
# (48, 24): Ny = Ns + 3 exactly; (80, 40): Nx no multiple of 64, 40 and 40 + 22 (+ 1) rows no multiple of 17
CASES += [(g, s, 30, blk, 0) for g in ("lat_lon_as_curvilinear", "tripolar", "gaussian_islands") for s in ((48, 24, 6), (80, 40, 6)) for blk in (1, 5)]
# substep counts: for S = 3, 5, 7 an exact division (Ns = 21, 10, 21: above for 3 and 7), a remainder launch (10, 21: above, 10) and
# Ns < S (2, 4, 4: one launch that is not last, then the finalize launch)
CASES += [(g, (70, 13, 4) if g == "simple_lat_lon" else (48, 24, 6), sub, blk, 0)
          for g in ("simple_lat_lon", "gaussian_islands_lat_lon") for blk, sub in ((3, 14), (3, 3), (5, 14), (5, 6), (7, 14), (7, 6))]
CASES += [(g, (48, 24, 6), sub, blk, 0) for g in ("lat_lon_as_curvilinear", "gaussian_islands") for sub in (14, 6) for blk in (1, 5)]
CASES = [(ft,) + c for ft in BUILDS for c in CASES]
IDS = ["%s-%s-%dx%dx%d-substeps%d-block%d-order%d" % ((c[0], c[1]) + c[2] + c[3:]) for c in CASES]


def form_of(grid, substeps, block, order):
    """(form, kernel instance, launches, a finalize launch follows, the tall arrays) as plan_subcycle decides them."""
    Ns, imm, curv, tall = NS[substeps], "islands" in grid, grid in sc.CURVILINEAR, grid in sc.FOLDED
    blocked = block > 1 and not order
    if curv:
        S = 5 if blocked else 1
        name = "k_barotropic_multi_curv<5,17>" if blocked else "k_barotropic_substep_curv"
        form = "BlockedCurv" if blocked else "PerSubstepCurv"
    else:
        S = (3 if block <= 3 else 5 if block <= 5 else 7) if blocked else 1
        name = ("k_barotropic_multi<%d,%d,%s>" % (S, 17 if S == 5 else 16, str(imm).lower()) if blocked
                else "k_barotropic_substep<%s,%d>" % (str(imm).lower(), order))
        form = "Blocked" if blocked else "PerSubstep"
    launches = -(-Ns // S)
    return form, name, launches, (not blocked) or (launches == 1 and not tall), tall


def run(float_type, grid, shape, substeps, block, order, halo_seed=None):
    halo = 8 if grid in sc.FOLDED else 4
    dt = DT[(grid, shape)] * substeps / 30.0
    arch = gb.GPU(float_type=float_type)
    m = gb.baroclinic_instability_model(arch, *shape, dt=dt, halo=(halo,) * 3, grid_type=grid, substeps=substeps,
                                        options=dict(subcycle_block=block, substep_order=order))
    b = m.backend
    try:
        assert b.get_option("subcycle_block") == block and b.get_option("substep_order") == order
        assert b.dtype == (np.float32 if float_type == "Float32" else np.float64)
        sub = b.substepping()
        assert sub[0] == NS[substeps], f"substeps = {substeps} gives Ns = {sub[0]}"
        g = sc.read_geometry(b, grid, shape, halo)
        before = tss.set_inputs(b, 0, halo_seed)
        for q, n in enumerate(("eta_bar", "U_bar", "V_bar")):          # noise in the filtered state: what the call leaves of it is seen
            b.set_field(n, (3 * counter_rng(b.field_dims(n, True), 800, q) + 1).astype(b.dtype), True)
            before[n] = b.get_field(n, True)
        b.ab2_step(dt, False)
        after = {n: b.get_field(n, True) for n in tss.OUTPUTS}
        return g, before, after, dt, sub, b.dtype
    finally:
        b.close()


def outside(a, g):
    H = g["H"]
    mask = np.ones(a.shape, bool)
    mask[H:H + g["Nx"], H:H + g["Ny"]] = False
    return mask


@pytest.mark.parametrize("float_type,grid,shape,substeps,block,order", CASES, ids=IDS)
def test_the_subcycle_cell_by_cell(float_type, grid, shape, substeps, block, order):
    form, kernel, launches, finalize, tall = form_of(grid, substeps, block, order)
    label = f"{float_type} {grid} {shape} Ns {NS[substeps]} {form} {kernel} x {launches}{' + finalize' if finalize else ''}{' tall' if tall else ''}"
    g, before, after, dt, sub, dtype = run(float_type, grid, shape, substeps, block, order)
    H, Nx, Ny, Ns = g["H"], g["Nx"], g["Ny"], sub[0]
    if g["immersed"]:
        assert g["wet"].any() and (~g["wet"]).any(), "an island grid has wet and dry columns"
    assert all(np.isfinite(a).all() for a in after.values())
    spec, growth = sc.subcycle(before, after["Gn.U"], after["Gn.V"], g, sub, dt, dtype, order)
    tss.assert_input_conditions(label, g, before, after, spec, growth)
    out = sc.measure(after, spec, g)
    print(f"[subcycle] {label}: growth {growth:.3f}, max residual / bound = " + ", ".join(f"{n} {r:.4f} at {at}" for n, (r, at) in out.items()))
    sc.judge(label, after, spec, g)
    for n in sc.FIELDS:
        assert np.array_equal(tss.interior(after[n + "_bar"], g), tss.interior(after[n], g)), f"{label}: {n}_bar is not {n} on the interior"
        out_ = outside(after[n], g)
        assert np.array_equal(after[n][out_], before[n][out_]), f"{label}: a cell of {n} outside the interior changed"
        bar, bar0 = after[n + "_bar"], before[n + "_bar"]
        if form in ("Blocked", "BlockedCurv"):
            assert np.array_equal(bar[out_], bar0[out_]), f"{label}: a cell of {n}_bar outside the interior changed"
        elif not tall:
            assert not np.any(bar[out_]), f"{label}: {n}_bar is not zero outside the interior"
        else:
            cols = np.zeros(bar.shape, bool)
            cols[H:H + Nx] = True
            assert np.array_equal(bar[~cols], bar0[~cols]), f"{label}: an x halo column of {n}_bar changed"
            assert not np.any(bar[H:H + Nx, :H]), f"{label}: {n}_bar below row 0 is not zero"
            assert not np.any(bar[H:H + Nx, H + Ny + Ns + 1:]), f"{label}: {n}_bar beyond the image rows is not zero"
    # other noise in the halo cells of eta, U, V: the same bits on the interior
    _, before2, after2, _, _, _ = run(float_type, grid, shape, substeps, block, order, halo_seed=1)
    for n in sc.FIELDS:
        out_ = outside(before[n], g)
        assert not np.array_equal(before2[n][out_], before[n][out_]) and np.array_equal(tss.interior(before2[n], g), tss.interior(before[n], g))
        assert np.array_equal(tss.interior(after2[n], g), tss.interior(after[n], g)), f"{label}: {n} depends on a halo cell of eta, U or V"
