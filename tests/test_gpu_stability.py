"""Stability diagnostics on the device (gb25_compute_stability, gb25_get_stability, gb25_get_stability_stats) against their numpy
restatement (gb-25_amd/stability.py, pinned on the CPU by tests/test_stability_host.py) of the DOWNLOADED parents and of the
potential density gb25_get_derived hands out: every quantity bit for bit on every grid type in both float types, windows of faces,
statistics, the device pointer, a planted NaN, decomposition invariance, the argument errors, and the proof that asking changes
nothing a model computes.

Shapes: the smallest each grid type accepts (helpers.size_of), a few steps in; they still have a wall row, the periodic seam, the
fold's pivot row, immersed columns and partially immersed ones.  A comparison of zeros with zeros cannot pass: N2, S2 and the
potential vorticity must be non-zero on at least a quarter of the wet interior faces of every case.  The test prints the counts.

Sums of the statistics: the integrals' bound, (n + 4) eps(Float64) sum|term| (tests/test_gpu_integrals.py)."""
import math

import numpy as np
import pytest

import gb25_amd as gb
from gb25_amd.binding import KERNEL_IDS, STABILITY_IDS
from gb25_amd.distributed import LocalSlabEnsemble
from gb25_amd.stability import gather_stability, stability_host, vorticity_corners_host
from helpers import BASE_FIELDS, CATKE_FIELDS, EPS, GRID_NAMES, counter_rng, size_of, stepped_model

pytestmark = pytest.mark.gpu
CASES = [(ft, gt) for ft in ("Float32", "Float64") for gt in (0, 1, 3, 4)]
FACE_KINDS = tuple(k for k in STABILITY_IDS if k != "wave_speed")
PARAMS = {"richardson": 1e-12, "eady_rate": 0.0}

_MODELS = {}
_WANT = {}


@pytest.fixture(scope="module", autouse=True)
def _close_models():
    yield
    for m in _MODELS.values():
        m.backend.close()
    _MODELS.clear()
    _WANT.clear()


def model_of(float_type, grid_type):
    """One stepped model per case for the whole module: the diagnostics are read-only, so the tests can share it."""
    key = (float_type, grid_type)
    if key not in _MODELS:
        _MODELS[key] = stepped_model(float_type, grid_type, dt=60.0 if grid_type == 3 else None)   # (the tripolar grid's short step, as grid 4's)
    return _MODELS[key]


def restated(float_type, grid_type):
    """The restatement of every quantity of a case, computed once: {kind: array}, and the wet interior faces."""
    key = (float_type, grid_type)
    if key not in _WANT:
        b = model_of(float_type, grid_type).backend
        Nx, Ny, Nz = b.field_dims("T", False)
        sigma, corners = b.get_derived("potential_density"), vorticity_corners_host(b)
        want = {k: stability_host(b, k, PARAMS.get(k), sigma=sigma, vorticity=corners) for k in STABILITY_IDS}
        kbot = np.array([[b.bottom_info("kbot", i, j) for j in range(1, Ny + 1)] for i in range(1, Nx + 1)]).astype(int)
        faces = np.arange(Nz + 1)[None, None, :]
        want["wet_faces"] = (faces > kbot[:, :, None]) & (faces < Nz)
        want["kbot"], want["corners"] = kbot, corners
        _WANT[key] = want
    return _WANT[key]


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def same_where_numbers(a, b):
    """The same bits wherever both hold a number, NaN where the other holds one: the sign and the payload of a NaN that the
    arithmetic makes are the processor's, not the definition's."""
    nan = np.isnan(a)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(nan, np.isnan(b)) and same(np.where(nan, 0, a), np.where(nan, 0, b))


@pytest.mark.parametrize("float_type,grid_type", CASES)
def test_every_quantity_bit_for_bit(float_type, grid_type):
    b = model_of(float_type, grid_type).backend
    want = restated(float_type, grid_type)
    Nx, Ny, Nz = size_of(grid_type)
    wet = want["wet_faces"]
    if grid_type in (1, 4):
        assert (want["kbot"] >= Nz).any() and ((want["kbot"] > 0) & (want["kbot"] < Nz)).any(), "the islands give dry and partial columns"
    # (the premise of the potential vorticity: the corners' vorticity is the derived field's where that has the corner)
    zeta = b.get_derived("vorticity")
    assert same(want["corners"][:Nx, :zeta.shape[1]], zeta)
    for kind in STABILITY_IDS:
        x = want[kind]
        got = b.get_stability(kind, PARAMS.get(kind))
        nf = 1 if kind == "wave_speed" else Nz + 1
        assert got.shape == (Nx, Ny, nf) and got.dtype == b.dtype, kind
        bad = (got != x) & ~(np.isnan(got) & np.isnan(x))
        nonzero = int((x[wet] != 0).sum()) if nf > 1 else int((x != 0).sum())
        print(f"  {float_type} grid {grid_type} {kind}: non-zero {nonzero} of {int(wet.sum()) if nf > 1 else x.size}, "
              f"non-finite {int((~np.isfinite(x)).sum())}, differing {int(bad.sum())}, max |x| {np.nanmax(np.abs(x)):.6g}")
        assert same(got, x), kind
        if kind in ("n2", "shear2", "ertel_pv"):
            assert 4 * nonzero >= int(wet.sum()) > 0, kind
        assert nonzero > 0 and np.isfinite(x).all(), kind
        if nf > 1:
            assert (x[~wet] == 0).all(), kind
            for k_first, k_count in ((0, 1), (Nz, 1), (Nz // 2, 2), (1, -1), (0, -1)):
                part = b.get_stability(kind, PARAMS.get(kind), (k_first, k_count))
                assert same(part, x[:, :, k_first:(None if k_count == -1 else k_first + k_count)]), (kind, k_first, k_count)
        else:
            assert same(b.get_stability(kind, None, (0, 1)), x) and same(gb.baroclinic_wave_speed(model_of(float_type, grid_type)), x[:, :, 0])
        assert same(b.get_stability(kind, PARAMS.get(kind)), got), kind        # repeatable
    # other floors than the defaults
    sigma = b.get_derived("potential_density")
    for kind, param in (("richardson", 1e-7), ("eady_rate", 1e-6)):
        assert same(b.get_stability(kind, param), stability_host(b, kind, param, sigma=sigma)), kind


@pytest.mark.parametrize("float_type,grid_type", [("Float32", 0), ("Float64", 1), ("Float32", 3), ("Float64", 4)])
def test_stats(float_type, grid_type):
    b = model_of(float_type, grid_type).backend
    for kind in STABILITY_IDS:
        x = np.asarray(b.get_stability(kind, PARAMS.get(kind)), np.float64)
        s = b.stability_stats(kind, PARAMS.get(kind))
        assert (s.min, s.max, s.max_abs) == (x.min(), x.max(), np.abs(x).max()), kind
        flat = np.abs(x).ravel(order="F")                    # (memory order: i fastest; the first of equal values)
        at = np.unravel_index(int(np.argmax(flat)), x.shape, order="F")
        assert tuple(s.at_max_abs) == tuple(int(q) + 1 for q in at), kind
        assert (s.count, s.nonfinite) == (x.size, 0) and tuple(s.first_nonfinite) == (0, 0, 0) and tuple(s.global_offset) == (0, 0, 0), kind
        n = x.size
        for got, terms in ((s.sum, x.ravel()), (s.sum_sq, (x * x).ravel())):
            exact, bound = math.fsum(terms), (n + 4) * EPS * math.fsum(np.abs(terms))
            assert abs(got - exact) <= bound, (kind, got, exact, bound)
        assert b.stability_stats(kind, PARAMS.get(kind)) == s, kind
    assert b.stability_stats("richardson") == b.stability_stats("richardson", 1e-12)


def test_the_device_pointer_and_the_public_functions():
    m = model_of("Float64", 0)
    b = m.backend
    Nx, Ny, Nz = size_of(0)
    other = model_of("Float32", 0).backend
    # the device pointer holds the packed result: consumed by gb25_compare_field of ANOTHER model, of the other float type
    for kind, levels in (("ertel_pv", (2, 3)), ("n2", None), ("wave_speed", None)):
        x = np.asarray(b.get_stability(kind, None, levels), np.float64)
        ptr, dims = b.compute_stability(kind, None, levels)
        assert ptr and dims == x.shape
        for n in range(x.shape[2]):
            d = other.compare_field("eta", ptr, real_bytes=8, dims=dims, origin=(0, 0, n))
            assert d.max_abs_b == np.abs(x[:, :, n]).max() and d.nonfinite == 0 and d.count == Nx * Ny, (kind, n)
            assert d.sum_sq_b > 0 or not x[:, :, n].any(), (kind, n)
    assert b.stability_dims("n2") == (Nx, Ny, Nz + 1) and b.stability_dims("wave_speed") == (Nx, Ny, 1)
    for got, want in ((gb.buoyancy_frequency(m), b.get_stability("n2")),
                      (gb.buoyancy_frequency(m, levels=(3, 2)), b.get_stability("n2", None, (3, 2))),
                      (gb.shear_squared(m), b.get_stability("shear2")),
                      (gb.richardson_number(m), b.get_stability("richardson", 1e-12)),
                      (gb.richardson_number(m, 1e-8), b.get_stability("richardson", 1e-8)),
                      (gb.eady_growth_rate(m), b.get_stability("eady_rate", 0.0)),
                      (gb.eady_growth_rate(m, 1e-6, levels=(1, 1)), b.get_stability("eady_rate", 1e-6, (1, 1))),
                      (gb.ertel_pv(m), b.get_stability("ertel_pv")),
                      (gb.baroclinic_wave_speed(m), b.get_stability("wave_speed")[:, :, 0])):
        assert same(got, want)
    Ld, res = gb.deformation_radius(m), gb.eddy_resolution(m)
    assert Ld.shape == res.shape == (Nx, Ny) and (Ld > 0).all() and (res > 0).all() and np.isfinite(Ld).all()


@pytest.mark.parametrize("float_type,grid_type", [("Float32", 0), ("Float64", 4)])
def test_a_planted_nan_stays_in_its_stencil(float_type, grid_type):
    m = stepped_model(float_type, grid_type)
    b = m.backend
    Nx, Ny, Nz = size_of(grid_type)
    before = {k: b.get_stability(k, PARAMS.get(k)) for k in STABILITY_IDS}
    kbot = restated(float_type, grid_type)["kbot"]
    open_water = (kbot == 0)
    for di, dj in ((1, 0), (-1, 0), (0, 1), (0, -1)):
        open_water &= np.roll(kbot, (di, dj), (0, 1)) == 0
    open_water[[0, 1, Nx - 2, Nx - 1]] = False          # (away from the seam and the edges: set_field fills no halo)
    open_water[:, [0, 1, Ny - 2, Ny - 1]] = False
    spots = np.argwhere(open_water)
    i0, j0 = (int(q) for q in spots[len(spots) // 2])
    T = b.get_field("T", False)
    T[i0, j0, Nz // 2] = np.nan
    b.set_field("T", T, False)
    own = np.zeros((Nx, Ny), bool)
    own[i0, j0] = True
    cross = own.copy()
    for di, dj in ((1, 0), (-1, 0), (0, 1), (0, -1)):
        cross[i0 + di, j0 + dj] = True
    sigma = b.get_derived("potential_density")
    assert np.isnan(sigma[i0, j0, Nz // 2]) and np.isnan(sigma).sum() == 1
    for kind in STABILITY_IDS:
        got = b.get_stability(kind, PARAMS.get(kind))
        changed = ((got != before[kind]) | (np.isnan(got) != np.isnan(before[kind]))).any(axis=2)
        touched = cross if kind == "ertel_pv" else own
        print(f"  {float_type} grid {grid_type} {kind}: columns changed {int(changed.sum())}, column ({i0}, {j0}) {got[i0, j0].tolist()}")
        assert same_where_numbers(got, stability_host(b, kind, PARAMS.get(kind), sigma=sigma)), kind
        assert np.isnan(got).any() == (kind in ("n2", "richardson", "ertel_pv")), kind
        assert same(got[~touched], before[kind][~touched]), kind
        if kind == "shear2":
            assert not changed.any()
        elif kind in ("n2", "wave_speed", "ertel_pv"):
            assert np.array_equal(changed, touched), kind
    b.close()


LOOKAHEADS = dict(subcycle_lookahead=1, ab2_lookahead=1)


@pytest.mark.parametrize("float_type,grid_type,catke", [("Float32", 0, False), ("Float64", 4, False), ("Float32", 4, True)])
def test_asking_changes_nothing(float_type, grid_type, catke):
    """Two identical models; one is asked for every quantity between every two steps.  Same bits, the look-aheads alive, the
    same launches of every phase of a step."""
    closure = gb.CATKEVerticalDiffusivity() if catke else None
    watched = stepped_model(float_type, grid_type, steps=0, closure=closure, **LOOKAHEADS)
    alone = stepped_model(float_type, grid_type, steps=0, closure=closure, **LOOKAHEADS)
    Nz = size_of(grid_type)[2]
    names = BASE_FIELDS + (CATKE_FIELDS if catke else [])
    for m in (watched, alone):
        m.backend.profile_enable(True)
        m.backend.profile_reset()
    wb = watched.backend
    for step in range(6):
        before = wb.lookahead_state()
        for kind in STABILITY_IDS:
            wb.get_stability(kind, PARAMS.get(kind), None if step % 2 or kind == "wave_speed" else (Nz // 2, 2))
        wb.compute_stability("ertel_pv", None, (1, 1 + step % 3))
        wb.stability_stats(("n2", "richardson", "wave_speed")[step % 3])
        gb.deformation_radius(watched)
        assert wb.lookahead_state() == before, step
        for m in (watched, alone):
            gb.time_step(m)
        assert wb.lookahead_state() == alone.backend.lookahead_state(), step
    assert alone.backend.lookahead_state()[0] and wb.lookahead_state()[0], "the velocity look-ahead is alive"
    for k in KERNEL_IDS:
        if k != "diagnostics":
            assert wb.profile_get(k)[0] == alone.backend.profile_get(k)[0], k
    assert wb.profile_get("diagnostics")[0] > 0 and alone.backend.profile_get("diagnostics")[0] == 0
    for name in names:
        a, b = wb.get_field(name, True), alone.backend.get_field(name, True)
        bad = np.argwhere(~((a == b) | (np.isnan(a) & np.isnan(b))))
        if len(bad):
            print(f"  {name}: {len(bad)} of {a.size} elements differ, first at {bad[0].tolist()}, last at {bad[-1].tolist()}, "
                  f"max |delta| {np.nanmax(np.abs(a - b)):.3g} of max {np.nanmax(np.abs(b)):.3g}")
        assert np.array_equal(a, b, equal_nan=True), name
    assert np.abs(wb.get_field("u", False)).max() > 0
    for m in (watched, alone):
        m.backend.close()


@pytest.mark.parametrize("P,Ry,grid_type", [(2, 1, 1), (4, 2, 4)])
def test_gathered_ranks_equal_the_single_domain(P, Ry, grid_type):
    if Ry == 1:
        Nx, Ny, Nz, dt, kw = 96, 40, 10, 600.0, {}
    else:
        Nx, Ny, Nz, dt, kw = 128, 48 * Ry, 8, 600.0, dict(slab_mode=1)
    exact = dict(w_on_the_fly=0)        # (what the decomposition tests switch off for bit-exactness)
    single = gb.baroclinic_instability_model(gb.GPU(), Nx, Ny, Nz, dt=dt, grid_type=GRID_NAMES[grid_type])
    gb.set_baroclinic_instability(single)
    vrows = Ny if grid_type == 4 else Ny + 1
    single.set(u=(1e-2 * counter_rng((Nx, Ny, Nz), 42, 1)).astype(np.float32),
               v=(1e-2 * counter_rng((Nx, vrows, Nz), 42, 2)).astype(np.float32),
               eta=(1e-2 * counter_rng((Nx, Ny, 1), 42, 3)).astype(np.float32))
    init = {n: single.backend.get_field(n, False) for n in ("u", "v", "T", "S", "eta")}
    ens = LocalSlabEnsemble(Nx, Ny, Nz, P, dt=dt, ranks_y=Ry, grid_type=grid_type, options=exact, **kw)
    for n, a in init.items():
        ens.scatter(n, a)
    gb.first_time_step(single)
    ens.first_time_step()
    gb.loop(single, 4)
    ens.loop(4)
    sb = single.backend
    for name in ("u", "v", "T", "S"):
        assert np.array_equal(ens.gather(name), sb.get_field(name, False)), name     # (the premise)
    for kind in STABILITY_IDS:
        want = sb.get_stability(kind, PARAMS.get(kind))
        got = gather_stability(ens, kind, PARAMS.get(kind))
        print(f"  {P} ranks ({Ry} in y) grid {grid_type} {kind}: differing values {(got != want).sum()} of {want.size}, "
              f"non-zero {(want != 0).sum()}")
        assert same(got, want), kind
        assert (want != 0).any()
        assert same(ens.stability(kind, PARAMS.get(kind)), got)
        if kind != "wave_speed":
            assert same(gather_stability(ens, kind, PARAMS.get(kind), (Nz // 2, 2)), want[:, :, Nz // 2:Nz // 2 + 2]), kind
    ens.close()
    sb.close()


def test_argument_errors_leave_the_model_usable():
    b = model_of("Float32", 0).backend
    Nz = size_of(0)[2]
    good = b.get_stability("ertel_pv")
    for word, call in (("no stability diagnostic", lambda: b.get_stability(len(STABILITY_IDS))),
                       ("no stability diagnostic", lambda: b.get_stability(-1)),
                       ("window", lambda: b.get_stability("n2", None, (0, 0))),
                       ("window", lambda: b.get_stability("n2", None, (Nz + 1, 1))),
                       ("window", lambda: b.get_stability("n2", None, (Nz, 2))),
                       ("window", lambda: b.get_stability("n2", None, (-1, 1))),
                       ("Richardson", lambda: b.get_stability("richardson", 0.0)),
                       ("Richardson", lambda: b.get_stability("richardson", -1e-12)),
                       ("Eady", lambda: b.get_stability("eady_rate", -1e-12)),
                       ("window", lambda: b.get_stability("wave_speed", None, (0, 2))),
                       ("window", lambda: b.get_stability("wave_speed", None, (1, 1))),
                       ("window", lambda: b.compute_stability("shear2", None, (2, Nz))),
                       ("Richardson", lambda: b.stability_stats("richardson", 0.0))):
        with pytest.raises(gb.GB25Error, match=word):
            call()
        assert same(b.get_stability("ertel_pv"), good)
