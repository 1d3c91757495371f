"""Zonal-mean and eddy statistics on the device (gb25_get_zonal_eddy) against their numpy restatement (gb-25_amd/eddies.py, pinned on
the CPU by tests/test_zonal_eddy_host.py) of the DOWNLOADED parents and of the potential density gb25_get_derived hands out: every
member of every record bit for bit in both float types, on lines of more than 256 cells (a lane takes a second chunk), of an odd
width below 64 (a partial chunk, misaligned rows), with islands, and on the folded grid (the pivot row's 1/2, the fold's halo row
of v); measure and points against gb25_integrate_field, windows, repeatability, the caller's means, planted NaNs, an all-land
line, x slabs, the refusals by name, and the proof that asking changes nothing a model computes.

Equality is tobytes() equality wherever the file says "same".  The slabs add the parts of a line in another order than the single
domain: there first and co are held to (Nx + 64) 2^-53 times the same sums over absolute values, the rounding bound of two
summation orders of at most Nx terms through a tree of 64 lanes -- not a measured tolerance.  Measured on an MI355X: at most
0.03 of that bound.  `measure` of the slabs is the single domain's bit for bit: the ensemble sums the cells' static measure over
the whole line in the single domain's order (test_the_measure_of_the_slabs_is_the_single_domain_s says why)."""
import functools

import numpy as np
import pytest

import gb25_amd as gb
from gb25_amd.binding import KERNEL_IDS, ZONAL_EDDY_DTYPE
from gb25_amd.distributed import LocalSlabEnsemble
from gb25_amd.eddies import PAIRS, centred_values, co_index, zonal_eddy_host
from gb25_amd.integrals import cell_measure
from helpers import BASE_FIELDS, GRID_NAMES, counter_rng, stepped_model

pytestmark = pytest.mark.gpu
# name: (grid type, size, dt)
GRIDS = {"wide": (0, (300, 12, 5), 600.0), "odd": (0, (37, 12, 5), 600.0), "islands": (1, (48, 24, 6), 600.0),
         "folded": (4, (72, 36, 8), 60.0)}
CASES = [(ft, g) for ft in ("Float32", "Float64") for g in GRIDS]
MEMBERS = ZONAL_EDDY_DTYPE.names


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def same_where_numbers(a, b):
    """The same bits wherever both hold a number, NaN where the other holds one."""
    if a.dtype.kind != "f":
        return same(a, b)
    nan = np.isnan(a)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(nan, np.isnan(b)) and same(np.where(nan, 0, a), np.where(nan, 0, b))


def same_records(a, b):
    return all(same_where_numbers(a[f], b[f]) for f in MEMBERS)


def model_of(float_type, grid, steps=3, **options):
    grid_type, size, dt = GRIDS[grid]
    return stepped_model(float_type, grid_type, steps=steps, size=size, dt=dt, **options)


def restated(b, levels=None, means=None):
    return zonal_eddy_host(b, levels, means, sigma=b.get_derived("potential_density"))


def report(label, got, want):
    for f in MEMBERS:
        print(f"  {label} {f}: differing {int((got[f] != want[f]).sum())} of {got[f].size}")


@pytest.mark.parametrize("float_type,grid", CASES)
def test_every_member_of_every_record_bit_for_bit(float_type, grid):
    m = model_of(float_type, grid)
    b = m.backend
    Nx, Ny, Nz = GRIDS[grid][1]
    assert b.zonal_eddy_dims() == (Ny, Nz)
    want = restated(b)
    got = b.zonal_eddy()
    report(f"{float_type} {grid}", got, want)
    assert got.shape == (Ny, Nz) and got.dtype == ZONAL_EDDY_DTYPE
    for f in MEMBERS:
        assert same_where_numbers(got[f], want[f]), f
    # not zeros against zeros: three steps of a noisy flow give every line with cells eddy kinetic energy and a w
    lines = got["points"] > 1
    assert lines.any() and (got["co"][..., co_index("U", "U")][lines] > 0).all() and (got["co"][..., co_index("V", "V")][lines] > 0).all()
    assert (got["co"][..., co_index("W", "W")][lines] > 0).any() and (got["co"][..., co_index("U", "SIGMA")][lines] != 0).any()
    assert got["nonfinite"].sum() == 0 and np.isfinite(got["co"]).all()
    if grid in ("islands", "folded"):
        assert (got["points"][got["points"] > 0] < Nx).any(), "the islands take cells out of some lines"
    # measure and points ARE the ROWS record of gb25_integrate_field(GB25_T)
    rows = b.integrate_field("T", "rows")
    assert same(got["measure"], rows["measure"]) and same(got["points"], rows["points"])
    # a window is that slice; two calls give the same bytes
    part = b.zonal_eddy((1, 2))
    assert part.shape == (Ny, 2) and same_records(part, got[:, 1:3])
    assert same_records(b.zonal_eddy(), got) and same_records(b.zonal_eddy((Nz - 1, 1)), got[:, Nz - 1:])
    # the call's own means give the call's bytes; shifted means change co as the restatement says
    assert same_records(b.zonal_eddy(None, got["mean"]), got)
    assert same_records(b.zonal_eddy((1, 2), part["mean"]), part)
    shifted = part["mean"] + np.array([1e-3, -2e-3, 1e-6, 0.25, -0.125, 0.5])
    about = b.zonal_eddy((1, 2), shifted)
    assert same_records(about, restated(b, (1, 2), shifted))
    assert same(about["mean"], shifted) and same(about["first"], part["first"]) and same(about["measure"], part["measure"])
    assert not same(about["co"], part["co"])
    # the public function
    ze = gb.zonal_eddy(m, levels=(1, 2))
    assert same_records(ze.records, part) and same(ze.mean("T"), part["mean"][..., 3])
    assert (ze.eddy_kinetic_energy()[part["points"] > 1] > 0).all()
    b.close()


@pytest.mark.parametrize("float_type,grid", [("Float32", "wide"), ("Float64", "folded")])
def test_planted_nans_are_skipped_and_counted(float_type, grid):
    m = model_of(float_type, grid)
    b = m.backend
    Nx, Ny, Nz = GRIDS[grid][1]
    before = b.zonal_eddy()
    kbot = np.array([[b.bottom_info("kbot", i, j) for j in range(1, Ny + 1)] for i in range(1, Nx + 1)]).astype(int)
    open_water = (kbot == 0) & (np.roll(kbot, 1, 0) == 0) & (np.roll(kbot, -1, 0) == 0)
    open_water[[0, 1, Nx - 2, Nx - 1]] = False
    open_water[:, [0, Ny - 1]] = False
    spots = np.argwhere(open_water)
    (iT, jT), (iu, ju) = (tuple(int(q) for q in spots[len(spots) // 3]), tuple(int(q) for q in spots[2 * len(spots) // 3]))
    kT, ku = 1, Nz - 2
    assert (jT, kT) != (ju, ku)
    T, u = b.get_field("T", False), b.get_field("u", False)
    T[iT, jT, kT] = np.nan
    u[iu, ju, ku] = np.nan
    b.set_field("T", T, False)
    b.set_field("u", u, False)
    got = b.zonal_eddy()
    want = restated(b)
    report(f"{float_type} {grid} NaN", got, want)
    assert same_records(got, want)
    skipped = np.zeros((Ny, Nz), np.int64)
    skipped[jT, kT] = 1                       # the cell
    skipped[ju, ku] = 2                       # the two cells the face touches
    assert np.array_equal(got["nonfinite"], skipped) and np.array_equal(got["points"], before["points"] - skipped)
    assert np.isfinite(got["first"]).all() and np.isfinite(got["co"]).all() and np.isfinite(got["mean"]).all()
    untouched = skipped == 0
    for f in MEMBERS:
        assert same(got[f][untouched], before[f][untouched]), f
    assert (got["measure"][~untouched] < before["measure"][~untouched]).all()
    rows = b.integrate_field("T", "rows")     # (T's own record skips the T cell alone)
    assert same(got["measure"][untouched], rows["measure"][untouched]) and rows["nonfinite"][jT, kT] == 1
    b.close()


@pytest.mark.parametrize("float_type", ["Float32", "Float64"])
def test_an_all_land_line(float_type):
    m = model_of(float_type, "islands", steps=1)
    b = m.backend
    Nx, Ny, Nz = GRIDS["islands"][1]
    zc = np.array([b.metric("zc", k) for k in range(1, Nz + 1)])
    zb = np.full((Nx, Ny), -1e30)
    zb[:, 5] = 10.0                                   # a row of land
    zb[:, 9] = 0.5 * (zc[2] + zc[3])                  # a row whose three deepest levels are rock
    zb[10:14, 15] = 10.0
    b.set_bottom_height(zb)
    got = b.zonal_eddy()
    want = restated(b)
    report(f"{float_type} land", got, want)
    assert same_records(got, want)
    zero = np.zeros(1).tobytes()
    for j, levels in ((5, range(Nz)), (9, range(3))):
        for k in levels:
            r = got[j, k]
            assert r["measure"] == 0 and r["points"] == 0 and r["nonfinite"] == 0, (j, k)
            assert r["mean"].tobytes() == zero * 6 and r["co"].tobytes() == zero * 21 and r["first"].tobytes() == zero * 6, (j, k)
    assert (got["points"][9, 3:] == Nx).all() and (got["points"][15] == Nx - 4).all()
    rows = b.integrate_field("T", "rows")
    assert same(got["measure"], rows["measure"]) and same(got["points"], rows["points"])
    b.close()


LOOKAHEADS = dict(subcycle_lookahead=1, ab2_lookahead=1)


@pytest.mark.parametrize("float_type,grid", [("Float32", "wide"), ("Float64", "folded")])
def test_the_run_is_untouched(float_type, grid):
    """Two identical models; one asks between its steps.  Same bytes in every parent array, the look-aheads the same before and
    after the calls and the same as the twin's, the same launches of every kernel but the diagnostics'."""
    watched = model_of(float_type, grid, steps=0, **LOOKAHEADS)
    alone = model_of(float_type, grid, steps=0, **LOOKAHEADS)
    for m in (watched, alone):
        m.backend.profile_enable(True)
        m.backend.profile_reset()
    wb = watched.backend
    Nz = GRIDS[grid][1][2]
    for step in range(5):               # after first_time_step, then after each of loop's 4 steps
        before = wb.lookahead_state()
        r = wb.zonal_eddy(None if step % 2 else (Nz // 2, 2))
        wb.zonal_eddy(None if step % 2 else (Nz // 2, 2), r["mean"])
        gb.zonal_eddy(watched, levels=(0, 1))
        assert wb.lookahead_state() == before == alone.backend.lookahead_state(), step
        if step < 4:
            for m in (watched, alone):
                gb.loop(m, 1)
    assert wb.clock() == alone.backend.clock() and wb.clock()[1] == 5, wb.clock()
    for k in KERNEL_IDS:
        if k != "diagnostics":
            assert wb.profile_get(k)[0] == alone.backend.profile_get(k)[0], k
    assert wb.profile_get("diagnostics")[0] > 0 and alone.backend.profile_get("diagnostics")[0] == 0
    for name in BASE_FIELDS:
        a, c = wb.get_field(name, True), alone.backend.get_field(name, True)
        assert a.tobytes() == c.tobytes(), name
    assert np.abs(wb.get_field("u", False)).max() > 0
    for m in (watched, alone):
        m.backend.close()


def absolute_sums(b, records):
    """sum mu |x_q| [j, k, 6] and sum mu |d_p d_q| [j, k, 21] of the counted cells of every line, d about the records' means."""
    x = centred_values(b, b.get_derived("potential_density"))
    mu = cell_measure(b, "T")
    ok = (mu > 0) & np.isfinite(x).all(axis=0)
    w = np.where(ok, mu, 0.0)
    d = np.abs(np.where(ok, x - np.moveaxis(records["mean"], -1, 0)[:, None], 0.0))
    first = np.stack([(w * np.abs(np.where(ok, x[q], 0.0))).sum(axis=0) for q in range(6)], axis=-1)
    co = np.stack([(w * d[p] * d[q]).sum(axis=0) for p, q in PAIRS], axis=-1)
    return first, co


SLABS = [(2, 0), (4, 0), (2, 4)]


@functools.lru_cache(maxsize=None)
def slabs_and_single(P, grid_type):
    """The records of P x slabs (two phases: LocalSlabEnsemble.zonal_eddy) and of the single domain after the same three steps
    from the same state, the sums over absolute values of the single domain, and a window through the ensemble; computed once.
    The state has noise on T and S as well as on u, v: on a line where a variable is exactly uniform -- T in the deep levels of
    the analytic state, S everywhere -- its deviations are the rounding of the mean alone, the comoment is rounding noise of the
    order of (the error of the mean) x (the residual of the first moment), and the two means (the ranks' combined one, the single
    domain's) differ in the last bit: measured on the folded grid without the noise, [T* S*] = -9.96e-14 against 4.98e-14 beside
    a measure of 1e13, 8.8e4 times a bound that is proportional to sum mu |d_T d_S| = 4e-14.  The bound below is about the ORDER of a
    sum of given terms; it says nothing about terms that are themselves rounding errors."""
    Nx, Ny, Nz = (72, 36, 8) if grid_type else (64, 32, 8)
    dt = 60.0 if grid_type else 600.0
    kw = {} if grid_type else dict(substeps=2)
    exact = dict(w_on_the_fly=0)        # (what the decomposition tests switch off for bit-exactness)
    single = gb.baroclinic_instability_model(gb.GPU(), Nx, Ny, Nz, dt=dt, grid_type=GRID_NAMES[grid_type], options=exact, **kw)
    gb.set_baroclinic_instability(single)
    sb = single.backend
    vrows = sb.field_dims("v", False)[1]
    single.set(u=(1e-2 * counter_rng((Nx, Ny, Nz), 42, 1)).astype(np.float32),
               v=(1e-2 * counter_rng((Nx, vrows, Nz), 42, 2)).astype(np.float32),
               eta=(1e-2 * counter_rng((Nx, Ny, 1), 42, 3)).astype(np.float32))
    for n, salt in (("T", 4), ("S", 5)):
        x = sb.get_field(n, False)
        sb.set_field(n, x + (0.05 * counter_rng(x.shape, 42, salt)).astype(sb.dtype), False)
    init = {n: sb.get_field(n, False) for n in ("u", "v", "T", "S", "eta")}
    ens = LocalSlabEnsemble(Nx, Ny, Nz, P, dt=dt, grid_type=grid_type, options=exact, **kw)
    for n, a in init.items():
        ens.scatter(n, a)
    gb.first_time_step(single)
    ens.first_time_step()
    gb.loop(single, 2)
    ens.loop(2)
    premise = {name: np.array_equal(ens.gather(name), sb.get_field(name, False)) for name in ("u", "v", "w", "T", "S")}
    want = sb.zonal_eddy()
    got = ens.zonal_eddy().records
    abs_first, abs_co = absolute_sums(sb, want)
    part = ens.zonal_eddy((Nz // 2, 2)).records
    ens.close()
    sb.close()
    return dict(size=(Nx, Ny, Nz), premise=premise, want=want, got=got, abs_first=abs_first, abs_co=abs_co, part=part)


@pytest.mark.parametrize("P,grid_type", SLABS)
def test_slabs_against_the_single_domain(P, grid_type):
    """x slabs, two phases: the ranks share the global mean.  points and nonfinite equal the single domain's; first and co agree
    within the rounding bound of the two summation orders."""
    r = slabs_and_single(P, grid_type)
    Nx, Ny, Nz = r["size"]
    assert all(r["premise"].values()), r["premise"]          # (the slabs hold the single domain's fields bit for bit)
    got, want = r["got"], r["want"]
    bound = (Nx + 64) * 2.0 ** -53
    err_first = np.abs(got["first"] - want["first"])
    err_co = np.abs(got["co"] - want["co"])
    with np.errstate(divide="ignore", invalid="ignore"):
        print(f"  {P} slabs grid {grid_type}: first: max error / (bound x absolute sum) {np.nanmax(err_first / (bound * r['abs_first'])):.3g}; "
              f"co: {np.nanmax(err_co / (bound * r['abs_co'])):.3g}; differing first {int((err_first != 0).sum())}, co {int((err_co != 0).sum())}")
    assert np.array_equal(got["points"], want["points"]) and np.array_equal(got["nonfinite"], want["nonfinite"])
    assert (want["points"] > 0).any() and got["nonfinite"].sum() == 0
    assert (err_first <= bound * r["abs_first"]).all() and (err_co <= bound * r["abs_co"]).all()
    lines = want["points"] > 1
    assert (want["co"][lines] != 0).all(), "noise on every variable: no comoment of a line with cells is 0"
    # a window of levels, through the ensemble
    part = r["part"]
    assert part.shape == (Ny, 2) and same(part["measure"], got["measure"][:, Nz // 2:Nz // 2 + 2])
    assert same(part["co"], got["co"][:, Nz // 2:Nz // 2 + 2])


@pytest.mark.parametrize("P,grid_type", SLABS)
def test_the_measure_of_the_slabs_is_the_single_domain_s(P, grid_type):
    """measure of the combined records equals the single domain's exactly.

    The ranks' partial sums added in rank order are another association of the same numbers than the single domain's one tree
    over the whole line.  On the LatitudeLongitudeGrid every cell of a line has the same mu and the lines of these sizes are cut
    into whole chunks, so both are exact; on the folded grid mu changes along the line and they differ in the last bit (measured
    with 2 slabs at 72 x 36 x 8: 4 of the 288 lines, max relative difference 1.97e-16).  LocalSlabEnsemble.zonal_eddy therefore
    sums the cells' static measure over the WHOLE line in the single domain's order (eddies.single_domain_measure) instead of
    adding the ranks' sums, and the mean is first / that measure."""
    r = slabs_and_single(P, grid_type)
    got, want = r["got"], r["want"]
    differing = got["measure"] != want["measure"]
    with np.errstate(divide="ignore", invalid="ignore"):
        print(f"  {P} slabs grid {grid_type}: measure differing {int(differing.sum())} of {differing.size}, "
              f"max relative {np.nanmax(np.abs(got['measure'] - want['measure']) / want['measure']):.3g}, at {np.argwhere(differing).tolist()}")
    assert same(got["measure"], want["measure"])
    lines = got["measure"] > 0
    assert same(got["mean"][lines], (got["first"] / np.where(lines, got["measure"], 1.0)[..., None])[lines])


def test_refusals_by_name_leave_the_model_alone():
    m = model_of("Float32", "odd")
    b = m.backend
    Nx, Ny, Nz = GRIDS["odd"][1]
    fields = {n: b.get_field(n, True) for n in BASE_FIELDS}
    clock, state, good = b.clock(), b.lookahead_state(), b.zonal_eddy()
    bad_means = np.zeros((Ny, Nz, 6))
    bad_means[3, 2, 1] = np.nan
    out = np.zeros((Nz, Ny), ZONAL_EDDY_DTYPE)
    for word, call in (("out is NULL", lambda: b._call("gb25_get_zonal_eddy", 0, -1, None, None)),
                       ("window", lambda: b.zonal_eddy((0, 0))),
                       ("window", lambda: b.zonal_eddy((Nz, 1))),
                       ("window", lambda: b.zonal_eddy((Nz - 1, 2))),
                       ("window", lambda: b.zonal_eddy((-1, 1))),
                       ("window", lambda: b._call("gb25_get_zonal_eddy", 2, Nz, None, out.ctypes.data)),
                       ("means must be finite", lambda: b.zonal_eddy(None, bad_means)),
                       ("variable 1 of row 3 of level 2", lambda: b.zonal_eddy(None, bad_means))):
        with pytest.raises(gb.GB25Error, match=word):
            call()
        assert b.clock() == clock and b.lookahead_state() == state
        for n, a in fields.items():
            assert b.get_field(n, True).tobytes() == a.tobytes(), (word, n)
    with pytest.raises(ValueError):
        b.zonal_eddy((1, 2), bad_means)              # (the binding: the shape of means is that of the window)
    assert not out["points"].any()
    assert same_records(b.zonal_eddy(), good)
    b.close()


def test_the_dims_need_no_stepped_model():
    for grid_type, size, dt in ((3, (72, 36, 8), 60.0), (0, (37, 12, 5), 600.0)):
        m = gb.baroclinic_instability_model(gb.GPU(), *size, dt=dt, grid_type=GRID_NAMES[grid_type])
        assert m.backend.zonal_eddy_dims() == size[1:]
        m.backend.close()
