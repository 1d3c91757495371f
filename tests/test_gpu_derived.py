"""Derived fields on the device (gb25_compute_derived, gb25_get_derived, gb25_get_derived_stats, gb25_get_field_levels)
against their numpy restatements (gb-25_amd/derived.py, pinned on the CPU by tests/test_derived_host.py) of the DOWNLOADED
parents: vorticity, kinetic energy and mixed-layer depth bit for bit; the densities against the oracle's TEOS-10 polynomial;
level ranges, statistics, halo currency, decomposition invariance, and the proof that asking changes nothing a model computes.

Densities: |device - (teos10_rho(T, S, Z) - rho0)| <= eps(real) |ref| + 1e-9 kg/m^3.  The first term is the one rounding of the
result; the second bounds the difference between two Horner evaluations of the same 55-term polynomial: about 100 operations,
at most ~2e4 in the sum of the term magnitudes at S ~ 35, so ~4e-10.  Z is the level's centre as the model holds it, the mean of
its two faces (the faces are numbers of the model's float type; gb25_get_metric(ZC) would round their mean once more).  A wrong
level's table is off by >= 1e-3 kg/m^3 per metre.  The test prints the worst difference of every case.

Sums of the statistics: the integrals' bound, (n + 4) eps(Float64) sum|term| (tests/test_gpu_integrals.py)."""
import math

import numpy as np
import pytest

import gb25_amd as gb
from gb25_amd.binding import DERIVED_IDS, FIELD_IDS
from gb25_amd.derived import DERIVED_3D, gather_derived, kinetic_energy_host, mixed_layer_depth_host, vorticity_host
from gb25_amd.distributed import LocalSlabEnsemble
from helpers import BASE_FIELDS, CASES, EPS, GRID_NAMES, counter_rng, size_of, stepped_model

pytestmark = pytest.mark.gpu
THRESHOLDS = (0.03, 0.125)


_MODELS = {}


@pytest.fixture(scope="module", autouse=True)
def _close_models():
    yield
    for m in _MODELS.values():
        m.backend.close()
    _MODELS.clear()


def model_of(float_type, grid_type):
    """One stepped model per case for the whole module: the diagnostics are read-only, so the tests can share it."""
    key = (float_type, grid_type)
    if key not in _MODELS:
        _MODELS[key] = stepped_model(float_type, grid_type)
    return _MODELS[key]


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == np.ascontiguousarray(b).tobytes()


def kbot_of(b):
    Nx, Ny, _ = b.field_dims("T", False)
    return np.array([[b.bottom_info("kbot", i, j) for j in range(1, Ny + 1)] for i in range(1, Nx + 1)]).astype(int)


@pytest.mark.parametrize("float_type,grid_type", CASES)
def test_vorticity_kinetic_energy_and_mixed_layer_bit_for_bit(float_type, grid_type):
    b = model_of(float_type, grid_type).backend
    Nx, Ny, Nz = size_of(grid_type)
    zeta, ke = b.get_derived("vorticity"), b.get_derived("kinetic_energy")
    assert zeta.shape == b.field_dims("v", False) == b.derived_dims("vorticity") and ke.shape == (Nx, Ny, Nz)
    assert zeta.dtype == b.dtype and np.abs(zeta).max() > 0 and ke.max() > 0
    want = vorticity_host(b)
    print(f"  {float_type} grid {grid_type}: max|zeta| {np.abs(zeta).max():.3e}, differing elements {(zeta != want).sum()}, max KE {ke.max():.3e}")
    assert same(zeta, want)
    assert same(ke, kinetic_energy_host(b))
    sigma = b.get_derived("potential_density")
    kbot = kbot_of(b)
    if grid_type:
        assert (kbot == Nz).any() and ((kbot > 0) & (kbot < Nz)).any(), "the islands give dry columns and partial columns"
    for thr in THRESHOLDS:
        mld = b.get_derived("mixed_layer_depth", thr)
        want = mixed_layer_depth_host(b, sigma, thr)
        assert mld.shape == (Nx, Ny, 1) and same(mld, want), thr
        assert (mld[kbot == Nz] == 0).all() and (mld[kbot < Nz] > 0).all()
        print(f"    threshold {thr}: depth {mld[kbot < Nz].min():.2f} .. {mld.max():.2f} m, {int((kbot == Nz).sum())} dry columns")
    assert same(gb.mixed_layer_depth(model_of(float_type, grid_type)), b.get_derived("mixed_layer_depth", 0.03)[:, :, 0])
    assert (b.get_derived("mixed_layer_depth", 0.125) >= b.get_derived("mixed_layer_depth", 0.03)).all()
    with pytest.raises(gb.GB25Error, match="threshold"):
        b.get_derived("mixed_layer_depth", -1.0)
    with pytest.raises(gb.GB25Error, match="levels"):
        b.get_derived("vorticity", levels=(Nz, 1))


@pytest.mark.parametrize("float_type,grid_type", CASES)
def test_densities_against_the_oracle_polynomial(float_type, grid_type):
    from oracle_backend import OracleBackend
    b = model_of(float_type, grid_type).backend
    ob = OracleBackend(8, 8, 4, dt=1.0)
    rho = np.vectorize(ob.teos10_rho)
    Nx, Ny, Nz = size_of(grid_type)
    T, S = (np.asarray(b.get_field(n, False), np.float64) for n in ("T", "S"))
    zf = np.array([b.metric("zf", k) for k in range(1, Nz + 2)])
    zc = 0.5 * (zf[:-1] + zf[1:])
    wet = np.arange(Nz)[None, None, :] >= kbot_of(b)[:, :, None]
    eps_real = float(np.finfo(b.dtype).eps)
    rho0 = float(b.cfg.rho0)
    for name, Z in (("density_anomaly", np.broadcast_to(zc[None, None, :], T.shape)), ("potential_density", np.zeros(T.shape))):
        got = np.asarray(b.get_derived(name), np.float64)
        ref = rho(T, S, Z) - rho0
        err = np.abs(got - ref)
        tol = eps_real * np.abs(ref) + 1e-9
        worst = float((err / tol)[wet].max())
        print(f"  {float_type} grid {grid_type} {name}: worst |diff| {err[wet].max():.3e} kg/m3, worst |diff| / tolerance {worst:.3f}, "
              f"range {got[wet].min():.3f} .. {got[wet].max():.3f}")
        assert (err[wet] <= tol[wet]).all(), name
        assert (got[~wet] == 0).all() and (got[wet] != 0).all(), name
    if grid_type:
        assert (~wet).any()
    # in situ against potential: the compression of the column above, > 1e-3 kg/m^3 per metre
    d = np.asarray(b.get_derived("density_anomaly"), np.float64) - np.asarray(b.get_derived("potential_density"), np.float64)
    assert (d[wet] > 1e-3 * -np.broadcast_to(zc[None, None, :], T.shape)[wet]).all()
    ob.close()


@pytest.mark.parametrize("float_type,grid_type", CASES)
def test_level_ranges_of_the_derived_fields(float_type, grid_type):
    m = model_of(float_type, grid_type)
    b = m.backend
    Nz = size_of(grid_type)[2]
    for name in DERIVED_3D:
        whole = b.get_derived(name)
        for k0, kc in ((Nz - 1, 1), (2, 3), (0, -1), (1, -1)):
            part = b.get_derived(name, levels=(k0, kc))
            assert same(part, whole[:, :, k0:(None if kc == -1 else k0 + kc)]), (name, k0, kc)
        # repeatable: the same call twice
        assert b.get_derived(name, levels=(2, 3)).tobytes() == b.get_derived(name, levels=(2, 3)).tobytes(), name
        ptr, dims = b.compute_derived(name, levels=(2, 3))
        assert ptr and dims == whole.shape[:2] + (3,)
    assert same(gb.vorticity(m, levels=(Nz - 1, 1)), b.get_derived("vorticity")[:, :, Nz - 1:])
    assert same(gb.kinetic_energy(m), b.get_derived("kinetic_energy")) and same(gb.density_anomaly(m), b.get_derived("density_anomaly"))
    assert same(gb.potential_density(m, levels=(0, 2)), b.get_derived("potential_density")[:, :, :2])
    for levels in ((0, 1), (0, -1), None):
        assert same(b.get_derived("mixed_layer_depth", 0.03, levels), b.get_derived("mixed_layer_depth", 0.03))
    for levels in ((0, 2), (1, 1)):
        with pytest.raises(gb.GB25Error, match="levels"):
            b.get_derived("mixed_layer_depth", 0.03, levels)


def test_the_device_pointer_holds_the_packed_result():
    """gb25_compute_derived's pointer consumed by gb25_compare_field of ANOTHER model, of the other float type."""
    src, other = model_of("Float64", 0).backend, model_of("Float32", 0).backend
    x = np.asarray(src.get_derived("density_anomaly", levels=(5, 3)), np.float64)
    ptr, dims = src.compute_derived("density_anomaly", levels=(5, 3))
    assert dims == (64, 32, 3)
    # (the box of eta, 64 x 32 x 1, against each level of the packed array in turn)
    for kk in range(3):
        d = other.compare_field("eta", ptr, real_bytes=8, dims=dims, origin=(0, 0, kk))
        assert d.max_abs_b == np.abs(x[:, :, kk]).max() and d.nonfinite == 0 and d.count == 64 * 32
        terms = (x[:, :, kk] ** 2).ravel()
        assert abs(d.sum_sq_b - math.fsum(terms)) <= (len(terms) + 4) * EPS * math.fsum(terms)


@pytest.mark.parametrize("float_type,grid_type", CASES)
def test_get_field_levels_of_every_field(float_type, grid_type):
    m = stepped_model(float_type, grid_type)
    b = m.backend
    Nz = size_of(grid_type)[2]
    assert b.get_option("store_pressure") == 0
    # pHY while it is stale (the steps stored only its differences): the gather recomputes it, as get_field would
    stale = b.get_field_levels("pHY", 2, 3)
    stale_stats = b.field_stats("pHY")
    assert np.abs(stale).max() > 0
    for name in BASE_FIELDS:
        whole = b.get_field(name, False)
        if whole.shape[2] == 1:
            assert same(b.get_field_levels(name, 0, 1), whole) and same(b.get_field_levels(name), whole), name
            with pytest.raises(gb.GB25Error, match="levels"):
                b.get_field_levels(name, 1, 1)
            continue
        nz = whole.shape[2]                         # (w: Nz + 1)
        for k0, kc in ((nz - 1, 1), (2, 3), (0, -1)):
            assert same(b.get_field_levels(name, k0, kc), whole[:, :, k0:(None if kc == -1 else k0 + kc)]), (name, k0, kc)
        with pytest.raises(gb.GB25Error, match="levels"):
            b.get_field_levels(name, nz - 1, 2)
    assert same(stale, b.get_field("pHY", False)[:, :, 2:5]) and b.field_stats("pHY") == stale_stats
    assert same(m.tracers.T.surface(), b.get_field("T", False)[:, :, Nz - 1:]) and same(m.velocities.w.levels(Nz, 1), b.get_field("w", False)[:, :, Nz:])
    b.close()


@pytest.mark.parametrize("float_type,grid_type", [("Float32", 0), ("Float64", 4)])
def test_get_field_levels_of_the_previous_velocities(float_type, grid_type):
    """closure = CATKE: previous_u, previous_v are read where they live (the look-ahead's partner buffers after a step)."""
    m = stepped_model(float_type, grid_type, closure=gb.CATKEVerticalDiffusivity(), subcycle_lookahead=1, ab2_lookahead=1)
    b = m.backend
    before = b.lookahead_state()
    got = {n: b.get_field_levels(n, 2, 3) for n in ("previous_u", "previous_v", "e", "kappa_u")}
    top = b.get_field_levels("previous_u", size_of(grid_type)[2] - 1, 1)
    assert b.lookahead_state() == before
    for n, a in got.items():
        assert same(a, b.get_field(n, False)[:, :, 2:5]), n
    assert same(top, b.get_field("previous_u", False)[:, :, -1:]) and np.abs(top).max() > 0
    b.close()


@pytest.mark.parametrize("float_type,grid_type", CASES)
def test_derived_stats(float_type, grid_type):
    b = model_of(float_type, grid_type).backend
    for name in DERIVED_IDS:
        param = 0.125 if name == "mixed_layer_depth" else None
        x = np.asarray(b.get_derived(name, param), np.float64)
        s = b.derived_stats(name, param)
        assert (s.min, s.max, s.max_abs) == (x.min(), x.max(), np.abs(x).max()), name
        flat = np.abs(x).ravel(order="F")                    # (memory order: i fastest; the first of equal values)
        at = np.unravel_index(int(np.argmax(flat)), x.shape, order="F")
        assert tuple(s.at_max_abs) == tuple(int(q) + 1 for q in at), name
        assert (s.count, s.nonfinite) == (x.size, 0) and tuple(s.first_nonfinite) == (0, 0, 0) and tuple(s.global_offset) == (0, 0, 0), name
        n = x.size
        for got, terms in ((s.sum, x.ravel()), (s.sum_sq, (x * x).ravel())):
            exact, bound = math.fsum(terms), (n + 4) * EPS * math.fsum(np.abs(terms))
            assert abs(got - exact) <= bound, (name, got, exact, bound)
        assert b.derived_stats(name, param) == s, name
    assert b.derived_stats("mixed_layer_depth") == b.derived_stats("mixed_layer_depth", 0.03)


@pytest.mark.parametrize("float_type,grid_type", [("Float32", 0), ("Float64", 0), ("Float32", 4), ("Float64", 4)])
def test_the_halo_cells_the_stencils_read_are_current(float_type, grid_type):
    """zeta and KE read the first halo column and row of u, v: whenever a composite has returned they hold what an explicit
    fill_halo_regions would write ("Derived fields")."""
    for steps, lookaheads in ((3, {}), (4, dict(subcycle_lookahead=1, ab2_lookahead=1))):
        m = stepped_model(float_type, grid_type, steps=steps, **lookaheads)
        b = m.backend
        gb.time_step(m)
        before = {n: b.get_derived(n) for n in ("vorticity", "kinetic_energy")}
        b.fill_halo_regions()
        for n, a in before.items():
            after = b.get_derived(n)
            print(f"  {float_type} grid {grid_type} {n} lookaheads {bool(lookaheads)}: elements changed by the fill {(after != a).sum()}")
            assert same(after, a), n
        b.close()


@pytest.mark.parametrize("P,Ry,grid_type", [(2, 1, 1), (4, 1, 4), (4, 2, 4)])
def test_gathered_ranks_equal_the_single_domain(P, Ry, grid_type):
    if Ry == 1:
        Nx, Ny, Nz, dt, kw = 96 * P // 2, 40, 10, 600.0, {}
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
    for name in DERIVED_3D:
        got, want = gather_derived(ens, name), sb.get_derived(name)
        print(f"  {P} ranks ({Ry} in y) grid {grid_type} {name}: differing elements {(got != want).sum()} of {want.size}")
        assert same(got, want), name
        assert same(gather_derived(ens, name, levels=(Nz - 1, 1)), want[:, :, Nz - 1:]), name
    for thr in THRESHOLDS:
        assert same(gather_derived(ens, "mixed_layer_depth", thr), sb.get_derived("mixed_layer_depth", thr)), thr
    # a rank's statistics carry its offsets
    for b in ens.backends:
        assert tuple(b.derived_stats("kinetic_energy").global_offset) == (b.rx * ens.Nx_loc, b.ry * ens.Ny_loc, 0)
    ens.close()
    sb.close()


LOOKAHEADS = dict(subcycle_lookahead=1, ab2_lookahead=1)


@pytest.mark.parametrize("float_type,grid_type,catke", [("Float32", 0, False), ("Float64", 4, False), ("Float32", 1, False),
                                                        ("Float32", 4, True)])
def test_derived_fields_are_read_only(float_type, grid_type, catke):
    """Two identical models; one is asked for every derived field, its statistics and level slices of the fields between
    every two steps.  Same bits, the look-aheads alive, the same launches of every phase of a step."""
    closure = gb.CATKEVerticalDiffusivity() if catke else None
    watched = stepped_model(float_type, grid_type, steps=0, closure=closure, **LOOKAHEADS)
    alone = stepped_model(float_type, grid_type, steps=0, closure=closure, **LOOKAHEADS)
    Nz = size_of(grid_type)[2]
    names = BASE_FIELDS + ([n for n, i in FIELD_IDS.items() if i >= FIELD_IDS["e"]] if catke else [])
    for m in (watched, alone):
        m.backend.profile_enable(True)
        m.backend.profile_reset()
    wb = watched.backend
    for step in range(6):
        before = wb.lookahead_state()
        for name in DERIVED_3D:
            wb.get_derived(name, levels=None if step % 2 else (Nz - 1, 1))
            wb.compute_derived(name, levels=(1, 2))
        wb.get_derived("mixed_layer_depth", THRESHOLDS[step % 2])
        wb.derived_stats(("vorticity", "potential_density", "mixed_layer_depth")[step % 3])
        for name in names:
            nz = wb.field_dims(name, False)[2]
            wb.get_field_levels(name, nz - 1, 1)
        assert wb.lookahead_state() == before, step
        for m in (watched, alone):
            gb.time_step(m)
        assert wb.lookahead_state() == alone.backend.lookahead_state(), step
    assert alone.backend.lookahead_state()[0] and wb.lookahead_state()[0], "the velocity look-ahead is alive"
    from gb25_amd.binding import KERNEL_IDS
    for k in KERNEL_IDS:
        if k != "diagnostics":
            assert wb.profile_get(k)[0] == alone.backend.profile_get(k)[0], k
    assert wb.profile_get("diagnostics")[0] > 0 and alone.backend.profile_get("diagnostics")[0] == 0
    for name in names:
        a, b = wb.get_field(name, True), alone.backend.get_field(name, True)
        assert np.array_equal(a, b, equal_nan=True), name
    assert np.abs(wb.get_field("u", False)).max() > 0
    for m in (watched, alone):
        m.backend.close()
