"""Flow kinematics on the device (gb25_compute_kinematics, gb25_get_kinematics, gb25_get_kinematics_stats) against their numpy
restatement (gb-25_amd/kinematics.py, pinned on the CPU by tests/test_kinematics_host.py) of the DOWNLOADED parents and of the
potential density gb25_get_derived hands out: every quantity bit for bit on every grid type in both float types, windows of
levels, statistics, the device pointer, a planted NaN, decomposition invariance, the refusals by name, and the proof that asking
changes nothing a model computes.  Equality is tobytes() equality throughout: there is no tolerance in this file.

Shapes: those tests/test_gpu_passive.py steps -- 32 x 24 x 8 lat-lon, 48 x 24 x 6 lat-lon with islands, 72 x 36 x 8 tripolar and
tripolar with islands: a fold, bottom steps inside a block's ring, more than one block in x and in y.  Every case is compared
twice: two steps in, and with fresh noisy velocities and tracers over the interior and the halos filled from them, so that the
wall rows, the fold's rows and the seam hold what the noise put there.  A comparison of zeros with zeros cannot pass:
every quantity must be non-zero in at least a quarter of the wet cells (the noisy state also puts noise on T and S; two steps in,
S is still uniform along the rows in most cells, so its gradient is held to that only in the noisy state)."""
import numpy as np
import pytest

import gb25_amd as gb
from gb25_amd.binding import KINEMATICS_IDS
from gb25_amd.distributed import LocalSlabEnsemble
from gb25_amd.kinematics import CORNER_KINDS, TRACER_KINDS, gather_kinematics, kinematics_host
from helpers import BASE_FIELDS, GRID_NAMES, counter_rng, set_noisy_velocities, stepped_model

pytestmark = pytest.mark.gpu
SIZES = {0: (32, 24, 8), 1: (48, 24, 6), 3: (72, 36, 8), 4: (72, 36, 8)}
DT = {0: 600.0, 1: 600.0, 3: 60.0, 4: 60.0}
CASES = [(ft, gt) for ft in ("Float32", "Float64") for gt in SIZES]
REQUESTS = [(kind, p) for kind in KINEMATICS_IDS for p in ((0, 1, 2) if kind in TRACER_KINDS else (0,))]


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def same_where_numbers(a, b):
    """The same bits wherever both hold a number, NaN where the other holds one: the sign and the payload of a NaN that the
    arithmetic makes are the processor's, not the definition's."""
    nan = np.isnan(a)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(nan, np.isnan(b)) and same(np.where(nan, 0, a), np.where(nan, 0, b))


def model_of(float_type, grid_type, steps=2, **options):
    return stepped_model(float_type, grid_type, steps=steps, size=SIZES[grid_type], dt=DT[grid_type], **options)


def wet_cells(b):
    Nx, Ny, Nz = b.field_dims("T", False)
    kbot = np.array([[b.bottom_info("kbot", i, j) for j in range(1, Ny + 1)] for i in range(1, Nx + 1)]).astype(int)
    return np.arange(Nz)[None, None, :] >= kbot[:, :, None], kbot


@pytest.mark.parametrize("float_type,grid_type", CASES)
def test_every_quantity_bit_for_bit(float_type, grid_type):
    m = model_of(float_type, grid_type)
    b = m.backend
    Nx, Ny, Nz = SIZES[grid_type]
    wet, kbot = wet_cells(b)
    if grid_type in (1, 4):
        assert (kbot >= Nz).any() and ((kbot > 0) & (kbot < Nz)).any(), "the islands give dry and partial columns"
    for state in ("stepped", "noisy"):
        if state == "noisy":
            set_noisy_velocities(m, amplitude=0.05, seed=7)
            for n, salt in (("T", 3), ("S", 4)):            # (S is horizontally uniform at the start: give both tracers structure)
                a = b.get_field(n, False)
                b.set_field(n, a + (0.05 * counter_rng(a.shape, 7, salt)).astype(b.dtype), False)
            b.fill_halo_regions()                           # (the density of the ring is that of the periodic image)
        sigma = b.get_derived("potential_density")
        for kind, param in REQUESTS:
            want = kinematics_host(b, kind, param, sigma=sigma)
            got = b.get_kinematics(kind, param)
            rows = b.field_dims("v", False)[1] if kind in CORNER_KINDS else Ny
            assert got.shape == (Nx, rows, Nz) == b.kinematics_dims(kind) and got.dtype == b.dtype, kind
            cells = want[:, :Ny][wet]
            print(f"  {float_type} grid {grid_type} {state} {kind}({param}): non-zero {int((cells != 0).sum())} of {cells.size} wet, "
                  f"non-finite {int((~np.isfinite(want)).sum())}, differing {int((got != want).sum())}, max |x| {np.abs(want).max():.6g}")
            assert same(got, want), (state, kind, param)
            assert np.isfinite(want).all() and cells.size > 0, (state, kind, param)
            if state == "noisy" or param != 1:              # (two steps in, S is still uniform along most rows)
                assert 4 * int((cells != 0).sum()) >= cells.size, (state, kind, param)
            if kind not in CORNER_KINDS:
                assert (want[~wet] == 0).all(), kind
            for levels in ((Nz - 1, 1), (1, 3)):
                part = b.get_kinematics(kind, param, levels)
                assert same(part, want[:, :, levels[0]:levels[0] + levels[1]]), (state, kind, param, levels)
            assert same(b.get_kinematics(kind, param), got), kind            # repeatable
    b.close()


def test_the_device_pointer_and_the_public_functions():
    m = model_of("Float64", 1)
    other = model_of("Float32", 1, steps=0)
    b = m.backend
    Nx, Ny, Nz = SIZES[1]
    # the device pointer holds the packed result: consumed by gb25_compare_field of ANOTHER model, of the other float type
    for kind, param, levels in (("okubo_weiss", 0, (2, 3)), ("frontogenesis", 2, None), ("gradient", 1, (Nz - 1, 1))):
        x = np.asarray(b.get_kinematics(kind, param, levels), np.float64)
        ptr, dims = b.compute_kinematics(kind, param, levels)
        assert ptr and dims == x.shape
        for n in range(x.shape[2]):
            d = other.backend.compare_field("eta", ptr, real_bytes=8, dims=dims, origin=(0, 0, n))
            assert d.max_abs_b == np.abs(x[:, :, n]).max() and d.nonfinite == 0 and d.count == Nx * Ny, (kind, n)
    for got, want in ((gb.divergence(m), b.get_kinematics("divergence")),
                      (gb.normal_strain(m, levels=(1, 2)), b.get_kinematics("normal_strain", 0, (1, 2))),
                      (gb.shear_strain(m), b.get_kinematics("shear_strain")),
                      (gb.okubo_weiss(m), b.get_kinematics("okubo_weiss")),
                      (gb.rossby_number(m), b.get_kinematics("rossby_number")),
                      (gb.gradient_magnitude(m, "S"), b.get_kinematics("gradient", 1)),
                      (gb.gradient_magnitude(m, "potential_density", levels=(0, 1)), b.get_kinematics("gradient", 2, (0, 1))),
                      (m.tracers.T.gradient_magnitude(), b.get_kinematics("gradient", "T")),
                      (gb.frontogenesis(m), b.get_kinematics("frontogenesis", 2)),
                      (gb.frontogenesis(m, of="T"), b.get_kinematics("frontogenesis", 0))):
        assert same(got, want) and (want != 0).any()
    for mm in (m, other):
        mm.backend.close()


@pytest.mark.parametrize("float_type,grid_type", [("Float32", 0), ("Float64", 4)])
def test_stats_and_a_planted_nan(float_type, grid_type):
    m = model_of(float_type, grid_type)
    b = m.backend
    Nx, Ny, Nz = SIZES[grid_type]
    for kind, param in REQUESTS:
        x = np.asarray(b.get_kinematics(kind, param), np.float64)
        s = b.kinematics_stats(kind, param)
        assert (s.min, s.max, s.max_abs) == (x.min(), x.max(), np.abs(x).max()), kind
        assert (s.count, s.nonfinite) == (x.size, 0) and tuple(s.first_nonfinite) == (0, 0, 0), kind
        assert np.isfinite(s.sum) and np.isfinite(s.sum_sq), kind                    # (the mean is sum / count)
    # one NaN in u, in open water away from the seam and the edges
    _, kbot = wet_cells(b)
    open_water = kbot == 0
    for di in (-1, 0, 1):
        for dj in (-1, 0, 1):
            open_water &= np.roll(kbot, (di, dj), (0, 1)) == 0
    open_water[[0, 1, Nx - 2, Nx - 1]] = False
    open_water[:, [0, 1, Ny - 2, Ny - 1]] = False
    spots = np.argwhere(open_water)
    i0, j0 = (int(q) for q in spots[len(spots) // 2])
    k0 = Nz // 2
    before = {r: b.get_kinematics(*r) for r in REQUESTS}
    u = b.get_field("u", False)
    u[i0, j0, k0] = np.nan
    b.set_field("u", u, False)
    # u(i0, j0) is a face of the cells i0 - 1 and i0, and enters the corners (i0, j0) and (i0, j0 + 1), which the cells
    # i0 - 1, i0 of the rows j0 - 1, j0, j0 + 1 average
    reach = {"divergence": [(i0 - 1, j0), (i0, j0)], "normal_strain": [(i0 - 1, j0), (i0, j0)],
             "shear_strain": [(i0, j0), (i0, j0 + 1)], "rossby_number": [(i0, j0), (i0, j0 + 1)], "gradient": []}
    reach["okubo_weiss"] = reach["frontogenesis"] = [(i, j) for i in (i0 - 1, i0) for j in (j0 - 1, j0, j0 + 1)]
    sigma = b.get_derived("potential_density")
    for kind, param in REQUESTS:
        got = b.get_kinematics(kind, param)
        s = b.kinematics_stats(kind, param)
        nan = np.isnan(got)
        want = np.zeros(got.shape, bool)
        for i, j in reach[kind]:
            want[i, j, k0] = True
        print(f"  {float_type} grid {grid_type} {kind}({param}): NaN at {np.argwhere(nan).tolist()}")
        assert np.array_equal(nan, want) and s.nonfinite == int(want.sum()), (kind, param)
        assert (s.nonfinite > 0) == (kind != "gradient"), kind
        assert same_where_numbers(got, kinematics_host(b, kind, param, sigma=sigma)), (kind, param)
        assert same(got[~want], before[(kind, param)][~want]), (kind, param)
    b.close()


LOOKAHEADS = dict(subcycle_lookahead=1, ab2_lookahead=1)


@pytest.mark.parametrize("float_type,grid_type", [("Float32", 0), ("Float64", 4)])
def test_the_run_is_untouched(float_type, grid_type):
    """Two identical models; one makes every kinematics call between its steps.  Same bytes in every parent array, the
    look-aheads the same before and after the calls and the same as the twin's."""
    watched = model_of(float_type, grid_type, steps=0, **LOOKAHEADS)
    alone = model_of(float_type, grid_type, steps=0, **LOOKAHEADS)
    wb = watched.backend
    Nz = SIZES[grid_type][2]
    for step in range(5):               # after first_time_step, then after each of loop's 4 steps
        before = wb.lookahead_state()
        for kind, param in REQUESTS:
            wb.get_kinematics(kind, param, None if step % 2 else (Nz // 2, 2))
        wb.compute_kinematics("frontogenesis", 2, (1, 1 + step % 3))
        wb.kinematics_stats(("okubo_weiss", "rossby_number", "divergence")[step % 3])
        assert wb.lookahead_state() == before == alone.backend.lookahead_state(), step
        if step < 4:
            for m in (watched, alone):
                gb.loop(m, 1)
    assert wb.clock() == alone.backend.clock() and wb.clock()[1] == 5, wb.clock()
    for name in BASE_FIELDS:
        a, c = wb.get_field(name, True), alone.backend.get_field(name, True)
        assert a.tobytes() == c.tobytes(), name
    assert np.abs(wb.get_field("u", False)).max() > 0
    for m in (watched, alone):
        m.backend.close()


@pytest.mark.parametrize("P,grid_type", [(2, 0), (4, 0), (2, 4)])
def test_gathered_slabs_equal_the_single_domain(P, grid_type):
    """x slabs: a slab's result comes from the x halos the step left, and equals the single domain's bit for bit.  The narrow
    lat-lon slabs take few barotropic substeps (a slab is at least substeps + 1 + halo columns wide)."""
    Nx, Ny, Nz = (72, 36, 8) if grid_type else (64, 32, 8)
    dt = DT[grid_type]
    kw = {} if grid_type else dict(substeps=2)
    exact = dict(w_on_the_fly=0)        # (what the decomposition tests switch off for bit-exactness)
    single = gb.baroclinic_instability_model(gb.GPU(), Nx, Ny, Nz, dt=dt, grid_type=GRID_NAMES[grid_type], options=exact, **kw)
    gb.set_baroclinic_instability(single)
    vrows = single.backend.field_dims("v", False)[1]
    single.set(u=(1e-2 * counter_rng((Nx, Ny, Nz), 42, 1)).astype(np.float32),
               v=(1e-2 * counter_rng((Nx, vrows, Nz), 42, 2)).astype(np.float32),
               eta=(1e-2 * counter_rng((Nx, Ny, 1), 42, 3)).astype(np.float32))
    init = {n: single.backend.get_field(n, False) for n in ("u", "v", "T", "S", "eta")}
    ens = LocalSlabEnsemble(Nx, Ny, Nz, P, dt=dt, grid_type=grid_type, options=exact, **kw)
    for n, a in init.items():
        ens.scatter(n, a)
    gb.first_time_step(single)
    ens.first_time_step()
    gb.loop(single, 1)
    ens.loop(1)
    sb = single.backend
    for name in ("u", "v", "T", "S"):
        assert np.array_equal(ens.gather(name), sb.get_field(name, False)), name     # (the premise)
    for kind, param in (("okubo_weiss", 0), ("frontogenesis", 2)):
        want = sb.get_kinematics(kind, param)
        got = gather_kinematics(ens, kind, param)
        print(f"  {P} slabs grid {grid_type} {kind}: differing values {(got != want).sum()} of {want.size}, non-zero {(want != 0).sum()}")
        assert same(got, want) and (want != 0).any(), kind
        assert same(ens.kinematics(kind, param), got)
        assert same(gather_kinematics(ens, kind, param, (Nz // 2, 2)), want[:, :, Nz // 2:Nz // 2 + 2]), kind
    ens.close()
    sb.close()


def test_refusals_by_name_leave_the_model_alone():
    m = model_of("Float32", 0)
    b = m.backend
    Nz = SIZES[0][2]
    fields = {n: b.get_field(n, True) for n in BASE_FIELDS}
    clock, good = b.clock(), b.get_kinematics("frontogenesis", 2)
    import ctypes as C
    for word, call in (("no kinematics quantity", lambda: b.get_kinematics(len(KINEMATICS_IDS))),
                       ("no kinematics quantity", lambda: b.get_kinematics(-1)),
                       ("tracer", lambda: b.get_kinematics("gradient", 3)),
                       ("tracer", lambda: b.get_kinematics("frontogenesis", -1)),
                       ("takes 0", lambda: b.get_kinematics("okubo_weiss", 1)),
                       ("takes 0", lambda: b.kinematics_stats("rossby_number", 2)),
                       ("window", lambda: b.get_kinematics("divergence", 0, (0, 0))),
                       ("window", lambda: b.get_kinematics("divergence", 0, (Nz, 1))),
                       ("window", lambda: b.get_kinematics("shear_strain", 0, (Nz - 1, 2))),
                       ("window", lambda: b.get_kinematics("gradient", 0, (-1, 1))),
                       ("window", lambda: b.compute_kinematics("okubo_weiss", 0, (2, Nz))),
                       ("host is NULL", lambda: b._call("gb25_get_kinematics", 0, 0, 0, -1, None)),
                       ("dev is NULL", lambda: b._call("gb25_compute_kinematics", 0, 0, 0, -1, None, (C.c_int32 * 3)())),
                       ("out is NULL", lambda: b._call("gb25_get_kinematics_stats", 0, 0, None))):
        with pytest.raises(gb.GB25Error, match=word):
            call()
        assert b.clock() == clock
        for n, a in fields.items():
            assert b.get_field(n, True).tobytes() == a.tobytes(), (word, n)
    assert same(b.get_kinematics("frontogenesis", 2), good)
    b.close()


def test_the_dims_need_no_stepped_model():
    m = gb.baroclinic_instability_model(gb.GPU(), *SIZES[3], dt=60.0, grid_type=GRID_NAMES[3])
    b = m.backend
    Nx, Ny, Nz = SIZES[3]
    for kind in KINEMATICS_IDS:                       # (a folded grid: the corner quantities have the Ny rows of its v)
        assert b.kinematics_dims(kind) == (Nx, Ny, Nz), kind
    b.close()
    m = gb.baroclinic_instability_model(gb.GPU(), *SIZES[0], dt=600.0)
    b = m.backend
    Nx, Ny, Nz = SIZES[0]
    for kind in KINEMATICS_IDS:
        assert b.kinematics_dims(kind) == (Nx, Ny + (1 if kind in CORNER_KINDS else 0), Nz), kind
    b.close()
