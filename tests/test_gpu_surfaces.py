"""Fields on surfaces on the device (gb25_compute_on_surfaces, gb25_get_on_surfaces) against their numpy restatement
(gb-25_amd/surfaces.py, pinned on the CPU by tests/test_surfaces_host.py) of the DOWNLOADED parents and of the arrays
gb25_get_derived hands out: values and status bytes bit for bit, for every search variable; target counts on both sides of a
group of targets, independence of the list's order, depth slices against the levels themselves, a planted NaN, decomposition
invariance, the argument errors, and the proof that asking changes nothing a model computes.

Targets: quantiles of the restatement's q over the wet cells, one value below its minimum and one above its maximum.  A comparison
of nothing with nothing cannot pass: on the islands the restatement must yield all four statuses, and FOUND in at least a quarter
of the wet (column, value) pairs of a case, counted over its search variables together (of the seven targets two can never be
found; isotherms of the whole domain cross few columns of this state, whose temperature varies more with latitude than with
depth, while isohalines, isopycnals and depths cross most) -- and in some pair for every search variable by itself.  The test
prints the counts."""
import numpy as np
import pytest

import gb25_amd as gb
from gb25_amd.binding import SURFACE_CARRIED, SURFACE_STATUS, SURFACE_VARIABLES
from gb25_amd.distributed import LocalSlabEnsemble
from gb25_amd.surfaces import DRY, FOUND, GROUNDED, OUTCROP, gather_surfaces, layer_thickness, on_surfaces_host
from helpers import BASE_FIELDS, CASES, CATKE_FIELDS, GRID_NAMES, counter_rng, size_of, stepped_model

pytestmark = pytest.mark.gpu
CARRIED = ("depth", "T", "kinetic_energy", "potential_density")
QUANTILES = (0.1, 0.3, 0.5, 0.7, 0.9)

_MODELS = {}
_PARENTS = {}


@pytest.fixture(scope="module", autouse=True)
def _close_models():
    yield
    for m in _MODELS.values():
        m.backend.close()
    _MODELS.clear()
    _PARENTS.clear()


def model_of(float_type, grid_type):
    """One stepped model per case for the whole module: the diagnostics are read-only, so the tests can share it."""
    key = (float_type, grid_type)
    if key not in _MODELS:
        _MODELS[key] = stepped_model(float_type, grid_type)
    return _MODELS[key]


def parents_of(b):
    """What the restatement is fed with, downloaded once per backend: the derived arrays, q of every search variable, kbot."""
    Nx, Ny, Nz = b.field_dims("T", False)
    sigma, ke = b.get_derived("potential_density"), b.get_derived("kinetic_energy")
    zc = np.array([b.metric("zc", k) for k in range(1, Nz + 1)], np.float64)
    kbot = np.array([[b.bottom_info("kbot", i, j) for j in range(1, Ny + 1)] for i in range(1, Nx + 1)]).astype(int)
    q = {"T": np.asarray(b.get_field("T", False), np.float64), "S": np.asarray(b.get_field("S", False), np.float64),
         "potential_density": np.asarray(sigma, np.float64), "depth": np.broadcast_to(-zc, (Nx, Ny, Nz))}
    return dict(sigma=sigma, ke=ke, zc=zc, kbot=kbot, q=q, wet=np.arange(Nz)[None, None, :] >= kbot[:, :, None])


def shared_parents(float_type, grid_type):
    key = (float_type, grid_type)
    if key not in _PARENTS:
        _PARENTS[key] = parents_of(model_of(float_type, grid_type).backend)
    return _PARENTS[key]


def targets_of(p, variable, quantiles=QUANTILES):
    x = p["q"][variable][p["wet"]]
    x = x[np.isfinite(x)]
    return np.concatenate([np.quantile(x, quantiles), [x.min() - 1.0, x.max() + 1.0]])


def restate(b, p, variable, carried, values):
    return on_surfaces_host(b, variable, carried, values, sigma=p["sigma"], ke=p["ke"])


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


@pytest.mark.parametrize("float_type,grid_type", CASES)
def test_values_and_status_bit_for_bit(float_type, grid_type):
    b = model_of(float_type, grid_type).backend
    p = shared_parents(float_type, grid_type)
    Nx, Ny, Nz = size_of(grid_type)
    wet_column = p["kbot"] < Nz
    if grid_type:
        assert (~wet_column).any() and ((p["kbot"] > 0) & wet_column).any(), "the islands give dry columns and partial columns"
    pooled_found = pooled_pairs = 0
    for variable in SURFACE_VARIABLES:
        values = targets_of(p, variable)
        for carried in CARRIED:
            want, want_status = restate(b, p, variable, carried, values)
            counts = np.bincount(want_status.ravel(), minlength=4)
            found = int((want_status[wet_column] == FOUND).sum())
            print(f"  {float_type} grid {grid_type} {variable} -> {carried}: found {counts[0]} outcrop {counts[1]} grounded {counts[2]} "
                  f"dry {counts[3]}; found in {found} of {want_status[wet_column].size} wet pairs")
            # (the premise: the comparison is not of nothing with nothing)
            assert found > 0 and counts[OUTCROP] > 0 and counts[GROUNDED] > 0, (variable, carried)
            if grid_type:
                assert counts[DRY] > 0, (variable, carried)
            if carried == "depth":
                pooled_found, pooled_pairs = pooled_found + found, pooled_pairs + want_status[wet_column].size
            got, status = b.get_on_surfaces(variable, carried, values)
            assert got.shape == status.shape == (Nx, Ny, len(values)) and got.dtype == b.dtype and status.dtype == np.uint8
            bad = (got != want) & ~(np.isnan(got) & np.isnan(want))
            print(f"      differing values {int(bad.sum())}, differing status bytes {int((status != want_status).sum())}")
            assert same(status, want_status), (variable, carried)
            assert same(got, want), (variable, carried)
            # repeatable: the same call twice
            again, status_again = b.get_on_surfaces(variable, carried, values)
            assert same(again, got) and same(status_again, status), (variable, carried)
    print(f"  {float_type} grid {grid_type}: found in {pooled_found} of {pooled_pairs} wet pairs of the four search variables")
    assert 4 * pooled_found >= pooled_pairs


@pytest.mark.parametrize("float_type,grid_type", CASES)
def test_target_counts_on_both_sides_of_a_group(float_type, grid_type):
    """1, a group of targets, one more than a group, and the most: the kernel marches once per 16 targets (SURF_TG); 8 is the
    other group size it was measured with."""
    b = model_of(float_type, grid_type).backend
    p = shared_parents(float_type, grid_type)
    for variable, carried in (("potential_density", "T"), ("T", "depth"), ("depth", "kinetic_energy")):
        values64 = targets_of(p, variable, np.linspace(0.01, 0.99, 62))
        order = np.argsort(counter_rng((64,), 7, 3))           # (in no order at all)
        values64 = values64[order]
        want64, status64 = restate(b, p, variable, carried, values64)
        for n in (1, 8, 9, 16, 17, 64):
            got, status = b.get_on_surfaces(variable, carried, values64[:n])
            assert same(got, want64[:, :, :n]) and same(status, status64[:, :, :n]), (variable, carried, n)
        # the order of the list does not matter on the device either
        perm = np.argsort(counter_rng((17,), 11, 5))
        got, status = b.get_on_surfaces(variable, carried, values64[:17][perm])
        assert same(got, want64[:, :, :17][:, :, perm]) and same(status, status64[:, :, :17][:, :, perm]), (variable, carried)
        sub = [16, 3, 40]
        got, status = b.get_on_surfaces(variable, carried, values64[sub])
        assert same(got, want64[:, :, sub]) and same(status, status64[:, :, sub]), (variable, carried)


@pytest.mark.parametrize("float_type,grid_type", CASES)
def test_depth_slices_at_the_level_centres_are_the_levels(float_type, grid_type):
    m = model_of(float_type, grid_type)
    b = m.backend
    p = shared_parents(float_type, grid_type)
    Nz = size_of(grid_type)[2]
    for name in ("T", "S"):
        got, status = gb.at_depths(m, name, -p["zc"])
        assert same(got, b.get_on_surfaces("depth", name, -p["zc"])[0])
        for k in range(Nz):
            ok = p["kbot"] <= k
            level = b.get_field_levels(name, k, 1)[:, :, 0]
            assert same(got[:, :, k][ok], level[ok]), (name, k)
            # (a column of one wet level has no pair to cross: its only level is handed out as an outcrop)
            assert (status[:, :, k][ok] == np.where(p["kbot"][ok] == Nz - 1, OUTCROP, FOUND)).all(), (name, k)
        assert same(getattr(m.tracers, name).at_depths(-p["zc"])[0], got)


@pytest.mark.parametrize("float_type,grid_type", [("Float32", 0), ("Float64", 4)])
def test_a_planted_nan_stays_in_its_column(float_type, grid_type):
    m = stepped_model(float_type, grid_type)
    b = m.backend
    Nz = size_of(grid_type)[2]
    combos = (("T", "depth"), ("potential_density", "T"), ("depth", "T"), ("potential_density", "depth"), ("S", "T"))
    p = parents_of(b)
    values = {v: targets_of(p, v) for v in SURFACE_VARIABLES}
    before = {c: b.get_on_surfaces(c[0], c[1], values[c[0]]) for c in combos}
    T = b.get_field("T", False)
    wet = np.argwhere(p["kbot"] == 0)
    (i0, j0), (i1, j1) = wet[len(wet) // 3], wet[2 * len(wet) // 3]
    T[i0, j0, :] = np.nan            # a whole column
    T[i1, j1, Nz // 2] = np.nan      # one level of another
    b.set_field("T", T, False)
    p = parents_of(b)
    assert np.isnan(p["sigma"][i0, j0]).all() and np.isnan(p["sigma"][i1, j1, Nz // 2])
    touched = np.zeros(T.shape[:2], bool)
    touched[i0, j0] = touched[i1, j1] = True
    for c in combos:
        got, status = b.get_on_surfaces(c[0], c[1], values[c[0]])
        want, want_status = restate(b, p, c[0], c[1], values[c[0]])
        print(f"  {float_type} grid {grid_type} {c[0]} -> {c[1]}: column ({i0}, {j0}) {got[i0, j0].tolist()} {status[i0, j0].tolist()}; "
              f"column ({i1}, {j1}) {got[i1, j1].tolist()} {status[i1, j1].tolist()}")
        assert same(status, want_status) and same(got, want), c
        assert same(got[~touched], before[c][0][~touched]) and same(status[~touched], before[c][1][~touched]), c
    # the NaN is skipped by the search for T and handed out where T is carried
    assert (b.get_on_surfaces("T", "depth", values["T"])[1][i0, j0] != FOUND).all()
    assert np.isnan(b.get_on_surfaces("depth", "T", values["depth"])[0][i0, j0]).any()
    b.close()


LOOKAHEADS = dict(subcycle_lookahead=1, ab2_lookahead=1)


@pytest.mark.parametrize("float_type,grid_type,catke", [("Float32", 0, False), ("Float64", 4, False), ("Float32", 4, True)])
def test_asking_changes_nothing(float_type, grid_type, catke):
    """Two identical models; one is asked for surfaces between every two steps.  Same bits, the look-aheads alive, the same
    launches of every phase of a step."""
    closure = gb.CATKEVerticalDiffusivity() if catke else None
    watched = stepped_model(float_type, grid_type, steps=0, closure=closure, **LOOKAHEADS)
    alone = stepped_model(float_type, grid_type, steps=0, closure=closure, **LOOKAHEADS)
    names = BASE_FIELDS + (CATKE_FIELDS if catke else [])
    for m in (watched, alone):
        m.backend.profile_enable(True)
        m.backend.profile_reset()
    wb = watched.backend
    sigmas = np.linspace(-23.0, -5.0, 17)
    for step in range(6):
        before = wb.lookahead_state()
        gb.isosurface_depth(watched, "potential_density", sigmas)
        gb.on_isosurface(watched, "T", of="potential_density", values=sigmas[:3])
        gb.on_isosurface(watched, "kinetic_energy", of="S", values=[5.0, 10.0])
        gb.at_depths(watched, "density_anomaly", [300.0, 1000.0])
        gb.layer_thickness(watched, "T", [5.0, 10.0, 20.0])
        wb.compute_on_surfaces("depth", "potential_density", [50.0] * (1 + step))
        if catke:
            gb.at_depths(watched, "e", [100.0])
            watched.tracers.T.at_depths([300.0])
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
    p = parents_of(sb)
    for variable, carried in (("potential_density", "depth"), ("potential_density", "T"), ("depth", "kinetic_energy")):
        values = targets_of(p, variable)
        want, want_status = sb.get_on_surfaces(variable, carried, values)
        got, status = gather_surfaces(ens, variable, carried, values)
        print(f"  {P} ranks ({Ry} in y) grid {grid_type} {variable} -> {carried}: differing values {(got != want).sum()} of {want.size}, "
              f"statuses {np.bincount(want_status.ravel(), minlength=4).tolist()}")
        assert same(got, want) and same(status, want_status), (variable, carried)
        assert (want_status == FOUND).any()
        again, status_again = ens.on_surfaces(variable, carried, values)
        assert same(again, got) and same(status_again, status)
    ens.close()
    sb.close()


def test_argument_errors_leave_the_model_usable():
    b = model_of("Float32", 0).backend
    good = b.get_on_surfaces("T", "depth", [10.0])
    for word, call in (("values", lambda: b.get_on_surfaces("T", "depth", [])),
                       ("values", lambda: b.get_on_surfaces("T", "depth", np.linspace(1.0, 20.0, 65))),
                       ("values", lambda: b.get_on_surfaces("T", "depth", [10.0, np.inf])),
                       ("values", lambda: b.get_on_surfaces("T", "depth", [np.nan])),
                       ("carried", lambda: b.get_on_surfaces("T", "e", [10.0])),           # (no CATKE on this model)
                       ("variable", lambda: b.get_on_surfaces(len(SURFACE_VARIABLES), "depth", [10.0])),
                       ("variable", lambda: b.get_on_surfaces(-1, "depth", [10.0])),
                       ("carried", lambda: b.get_on_surfaces("T", len(SURFACE_CARRIED), [10.0])),
                       ("values", lambda: b.compute_on_surfaces("T", "depth", []))):
        with pytest.raises(gb.GB25Error, match=word):
            call()
        again = b.get_on_surfaces("T", "depth", [10.0])
        assert same(again[0], good[0]) and same(again[1], good[1])


def test_public_functions_and_the_device_pointers():
    m = model_of("Float64", 0)
    b = m.backend
    p = shared_parents("Float64", 0)
    sig, deep = targets_of(p, "potential_density"), np.array([300.0, 1000.0, 2500.0])
    for got, want in ((gb.isosurface_depth(m, "potential_density", sig), b.get_on_surfaces("potential_density", "depth", sig)),
                      (gb.isosurface_depth(m, "T", [5.0, 12.0]), b.get_on_surfaces("T", "depth", [5.0, 12.0])),
                      (gb.on_isosurface(m, "T", of="potential_density", values=sig), b.get_on_surfaces("potential_density", "T", sig)),
                      (gb.on_isosurface(m, "kinetic_energy", of="S", values=[8.0]), b.get_on_surfaces("S", "kinetic_energy", [8.0])),
                      (gb.at_depths(m, "T", deep), b.get_on_surfaces("depth", "T", deep)),
                      (gb.at_depths(m, "density_anomaly", deep), b.get_on_surfaces("depth", "density_anomaly", deep)),
                      (m.tracers.S.at_depths(deep), b.get_on_surfaces("depth", "S", deep))):
        assert same(got[0], want[0]) and same(got[1], want[1])
    # in-situ density carried: the array gb25_get_derived hands out, interpolated by the restatement
    want, want_status = on_surfaces_host(b, "depth", "density_anomaly", deep)
    got, status = b.get_on_surfaces("depth", "density_anomaly", deep)
    assert same(got, want) and same(status, want_status)
    edges = np.sort(sig)
    depth = b.get_on_surfaces("potential_density", "depth", edges)[0]
    h = gb.layer_thickness(m, "potential_density", edges)
    assert same(h, layer_thickness(depth)) and h.shape == depth.shape[:2] + (len(edges) - 1,)
    assert set(SURFACE_STATUS.values()) == {FOUND, OUTCROP, GROUNDED, DRY}
    # the device pointers hold the packed results: consumed by gb25_compare_field of ANOTHER model, of the other float type
    other = model_of("Float32", 0).backend
    x = np.asarray(depth, np.float64)
    ptr, status_ptr, dims = b.compute_on_surfaces("potential_density", "depth", edges)
    assert ptr and status_ptr and dims == (64, 32, len(edges))
    for n in range(len(edges)):
        d = other.compare_field("eta", ptr, real_bytes=8, dims=dims, origin=(0, 0, n))
        assert d.max_abs_b == np.abs(x[:, :, n]).max() and d.nonfinite == 0 and d.count == 64 * 32
