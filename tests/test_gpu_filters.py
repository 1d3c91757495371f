"""The moving-window filter on the device (gb25_get_filter_sums, gb25_compute_filter_sums, gb25_get_derived_filter_sums) against its
numpy restatement (gb-25_amd/filters.py, pinned on the CPU by tests/test_filters_host.py) of the DOWNLOADED parents: every plane and
the info record bit for bit on every grid type in both float types, strides, weights, a radius per row, windows of levels, the tiles
of the x pass and the seam, a planted NaN, the device pointer, the argument errors, the refusal on a rank, the ensemble's host
path, and the proof that asking changes nothing a model computes.

Shapes: the smallest each grid type accepts (helpers.size_of), a few steps in; they still have a wall row, the periodic seam, the
fold's pivot row, immersed columns and partially immersed ones.  A comparison of zeros with zeros cannot pass: `first` must be
non-zero in at least a quarter of the non-empty outputs of T and of u in every case.  The test prints the counts."""
import numpy as np
import pytest

import gb25_amd as gb
from gb25_amd.binding import KERNEL_IDS, OPTION_IDS
from gb25_amd.distributed import LocalSlabEnsemble, SlabModel
from gb25_amd.filters import PLANES, filter_sums_host, kernel_weights, rows_for_length
from helpers import BASE_FIELDS, CATKE_FIELDS, GRID_NAMES, counter_rng, size_of, stepped_model

pytestmark = pytest.mark.gpu
CASES = [(ft, gt) for ft in ("Float32", "Float64") for gt in (0, 1, 3, 4)]
FIELDS = ("T", "S", "u", "v", "w", "eta", "U")
DERIVED = ("kinetic_energy", "potential_density", "mixed_layer_depth")
X_TILE = 256          # FLT_TILE of csrc/filter_kernels.hpp: the columns a workgroup of the x pass takes

_MODELS = {}


@pytest.fixture(scope="module", autouse=True)
def _close_models():
    yield
    for m in _MODELS.values():
        m.backend.close()
    _MODELS.clear()


def model_of(float_type, grid_type):
    """One stepped model per case for the whole module: the diagnostic is read-only, so the tests can share it."""
    key = (float_type, grid_type)
    if key not in _MODELS:
        _MODELS[key] = stepped_model(float_type, grid_type, dt=60.0 if grid_type == 3 else None)
    return _MODELS[key]


def levels_of(b, source):
    return b.derived_dims(source)[2] if source in DERIVED else b.field_dims(source, False)[2]


def specs_of(grid_type, nlev):
    """[dict(radius, stride, levels, wx, wy, rx_of_row)] of a source with nlev levels: the issue's windows."""
    Nx, Ny, Nz = size_of(grid_type)
    widest = (Nx - 1) // 2                      # 23 on 48, 31 on 64
    ladder = np.array([min(widest, (5 * j) % 13) for j in range(Ny)], np.int32)
    g4 = kernel_weights("gaussian", 4)
    specs = [dict(radius=(0, 0)), dict(radius=(1, 0)), dict(radius=(0, 1)), dict(radius=(2, 3)), dict(radius=(widest, 32)),
             dict(radius=(2, 3), stride=(4, 2)), dict(radius=(4, 4), wx=g4, wy=g4), dict(radius=(0, 2), rx_of_row=ladder),
             dict(radius=(3, 1), stride=(2, 4), rx_of_row=ladder, wy=kernel_weights("triangle", 1))]
    if nlev > 1:
        specs += [dict(radius=(2, 3), levels=(Nz - 1, 1)), dict(radius=(1, 2), stride=(4, 2), levels=(1, -1))]
    else:
        specs += [dict(radius=(2, 3), levels=(0, 1)), dict(radius=(1, 2), levels=(0, -1))]
    return specs


def call(fn, source, spec, **kw):
    return fn(source, spec["radius"], spec.get("stride", (1, 1)), spec.get("levels"), spec.get("wx"), spec.get("wy"), spec.get("rx_of_row"), **kw)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_same_sums(got, want, what):
    for plane in PLANES:
        g, w = getattr(got, plane), getattr(want, plane)
        bad = int((g != w).sum())
        if bad:
            print(f"    {what} {plane}: {bad} of {w.size} outputs differ, max |delta| {np.abs(g - w).max():.3e} of max {np.abs(w).max():.3e}")
        assert same(g, w), (what, plane)
    assert got.info == want.info, (what, got.info, want.info)


def describe(spec):
    return ", ".join(f"{k}={'...' if isinstance(v, np.ndarray) else v}" for k, v in spec.items())


@pytest.mark.parametrize("float_type,grid_type", CASES)
def test_every_plane_bit_for_bit(float_type, grid_type):
    b = model_of(float_type, grid_type).backend
    Nx, Ny, Nz = size_of(grid_type)
    for source in FIELDS + DERIVED:
        nlev = levels_of(b, source)
        param = 0.03 if source == "mixed_layer_depth" else None
        values = b.get_derived(source, param) if source in DERIVED else b.get_field(source, False)
        for spec in specs_of(grid_type, nlev):
            want = filter_sums_host(b, source, spec["radius"], spec.get("stride", (1, 1)), spec.get("levels"), spec.get("wx"), spec.get("wy"),
                                    spec.get("rx_of_row"), values=values)
            got = call(b.filter_sums, source, spec, param=param)
            assert got.dims == want.dims == b.filter_dims(source, spec["radius"], spec.get("stride", (1, 1)), spec.get("levels")), (source, spec)
            assert_same_sums(got, want, f"{source} {describe(spec)}")
            assert got.nonfinite == 0
            if source in ("T", "u"):
                full = want.measure > 0
                nonzero = int((want.first[full] != 0).sum())
                print(f"  {float_type} grid {grid_type} {source} {describe(spec)}: first != 0 in {nonzero} of {int(full.sum())} non-empty outputs, "
                      f"empty {want.empty}, clipped {want.clipped}")
                assert 4 * nonzero >= int(full.sum()) > 0, (source, spec)
        assert_same_sums(call(b.filter_sums, source, spec, param=param), got, f"{source} again")   # repeatable
    tall = b.filter_sums("T", ((Nx - 1) // 2, 32))
    assert tall.clipped == Nx * Ny * Nz, "ry >= Ny: every window is cut"
    points = b.filter_sums("T", (0, 0))
    if grid_type in (1, 4):
        # the islands: dry outputs, and windows that are part wet, part dry -- their measure lies strictly between 0 and that of
        # the same window with every point counted (the sum of the areas is what a flat bottom would give: compare with the count)
        wet = (points.measure > 0).astype(np.float64)
        counted = b.filter_sums("T", (2, 3)).measure
        from gb25_amd.filters import filter_of_planes
        n_wet = filter_of_planes(np.ones_like(wet), wet, (2, 3))[0]
        n_all = filter_of_planes(np.ones_like(wet), np.ones_like(wet), (2, 3))[0]
        partial = int(((n_wet > 0) & (n_wet < n_all)).sum())
        print(f"  {float_type} grid {grid_type}: empty outputs at radius (0, 0) {points.empty}, part wet part dry windows at (2, 3) {partial} of {n_all.size}")
        assert points.empty > 0 and partial > 0, "the islands give dry points and partly dry windows"
        assert np.array_equal(counted > 0, n_wet > 0)
    if grid_type in (3, 4):
        # the pivot row carries the 1/2: the measure with and without it, on the host
        one = points.measure
        dz = np.array([b.metric("dzc", k) for k in range(1, Nz + 1)], np.float64)
        H = int(b.cfg.halo)
        az = np.asarray(b.metric2("azcc"), np.float64)[H:H + Nx, H:H + Ny]
        for j, fold in ((Ny - 1, 0.5), (Ny - 2, 1.0)):
            whole = az[:, j, None] * dz[None, :]
            wet = one[:, j] > 0
            print(f"  {float_type} grid {grid_type}: row {j} wet points {int(wet.sum())}, factor {fold}")
            assert wet.any() and np.array_equal(one[:, j][wet], (whole * fold)[wet]), j
            assert fold == 1.0 or not np.array_equal(one[:, j][wet], whole[wet])


def test_tiles_of_the_x_pass_and_the_seam():
    """Two tiles of X_TILE columns and a remainder of 64, two levels of the model's smallest tested height; rx = 32: windows
    straddle the tiles and wrap around the seam."""
    Nx, Ny, Nz = 2 * X_TILE + 64, 32, 8
    m = stepped_model("Float32", 0, steps=1, size=(Nx, Ny, Nz))
    b = m.backend
    g = kernel_weights("gaussian", 32)
    ladder = np.array([32, 0, 31, 1, 32, 5, 17, 32] * (Ny // 8), np.int32)
    for name in ("T", "u", "eta"):
        levels = None if name == "eta" else (3, 2)
        for spec in (dict(radius=(32, 1)), dict(radius=(32, 0), stride=(3, 1)), dict(radius=(32, 2), wx=g), dict(radius=(7, 1), stride=(64, 2)),
                     dict(radius=(0, 0), rx_of_row=ladder)):
            spec = dict(spec, levels=levels)
            got, want = call(b.filter_sums, name, spec), call(lambda *a: filter_sums_host(b, *a), name, spec)
            assert got.dims == (Nx // spec.get("stride", (1, 1))[0], Ny // spec.get("stride", (1, 1))[1], 1 if name == "eta" else 2)
            assert_same_sums(got, want, f"{name} {describe(spec)}")
            assert (want.first != 0).any()
    b.close()


@pytest.mark.parametrize("float_type,grid_type", [("Float32", 0), ("Float64", 4)])
def test_a_planted_nan(float_type, grid_type):
    m = stepped_model(float_type, grid_type)
    b = m.backend
    Nx, Ny, Nz = size_of(grid_type)
    radius = (2, 3)
    before = b.filter_sums("T", radius)
    wet = np.argwhere(b.filter_sums("T", (0, 0)).measure[:, :, Nz - 1] > 0)
    i0, j0 = (int(q) for q in wet[len(wet) // 2])
    T = b.get_field("T", False)
    T[i0, j0, Nz - 1] = np.nan
    b.set_field("T", T, False)
    got, want = b.filter_sums("T", radius), filter_sums_host(b, "T", radius)
    assert got.nonfinite == 1 and before.nonfinite == 0
    assert_same_sums(got, want, "planted NaN")
    assert_same_sums(b.filter_sums("T", radius, (4, 2)), filter_sums_host(b, "T", radius, (4, 2)), "planted NaN, strided")   # (counted once, in a row or not)
    inside = np.zeros(got.dims, bool)
    for d in range(-radius[0], radius[0] + 1):
        for e in range(-radius[1], radius[1] + 1):
            if 0 <= j0 + e < Ny:
                inside[(i0 + d) % Nx, j0 + e, Nz - 1] = True
    for plane in PLANES:
        assert np.isfinite(getattr(got, plane)).all(), plane
        assert same(getattr(got, plane)[~inside], getattr(before, plane)[~inside]), plane
    assert (got.measure[inside] < before.measure[inside]).all()
    b.close()


def test_the_device_pointer():
    b = model_of("Float64", 1).backend
    other = model_of("Float32", 1).backend
    Nx, Ny, Nz = size_of(1)
    for name, spec in (("T", dict(radius=(2, 3))), ("u", dict(radius=(4, 4), wx=kernel_weights("gaussian", 4))), ("eta", dict(radius=(1, 1))),
                       ("w", dict(radius=(2, 1), levels=(Nz, 1))), ("T", dict(radius=(2, 3), stride=(4, 2)))):
        want = call(b.filter_sums, name, spec)
        ptr, dims, info = call(b.compute_filter_sums, name, spec)
        assert ptr and dims == want.dims and tuple(info.dims) == dims
        assert (info.nonfinite, info.empty, info.clipped, tuple(info.global_offset)) == (want.nonfinite, want.empty, want.clipped, want.global_offset)
        if dims[:2] == (Nx, Ny):
            # the three planes one after another, read through gb25_compare_field of ANOTHER model as one array of 3 dims[2] levels
            d3 = (Nx, Ny, 3 * dims[2])
            for q, plane in enumerate(PLANES):
                x = getattr(want, plane)
                for n in range(dims[2]):
                    d = other.compare_field("eta", ptr, real_bytes=8, dims=d3, origin=(0, 0, q * dims[2] + n))
                    assert d.max_abs_b == np.abs(x[:, :, n]).max() and d.sum_sq_b > 0 and d.nonfinite == 0, (name, plane, n)
        again = call(b.compute_filter_sums, name, spec)
        assert again[1] == dims and again[2] == info                 # repeatable call to call
        assert_same_sums(call(b.filter_sums, name, spec), want, name)
    # only the planes asked for
    only = b.filter_sums("T", (2, 3), planes=("first",))
    assert only.measure is None and only.second is None and same(only.first, b.filter_sums("T", (2, 3)).first)
    only = b.filter_sums("kinetic_energy", (2, 3), planes=("measure", "second"))
    whole = b.filter_sums("kinetic_energy", (2, 3))
    assert only.first is None and same(only.second, whole.second) and same(only.measure, whole.measure) and only.empty == whole.empty


def test_argument_errors_leave_the_model_usable():
    b = model_of("Float32", 0).backend
    Nx, Ny, Nz = size_of(0)
    good = b.filter_sums("T", (2, 3), (4, 2))
    ones3 = np.ones(3)
    for word, fn in (("rx", lambda: b.filter_sums("T", (-1, 0))), ("rx", lambda: b.filter_sums("T", (33, 0))),
                     ("ry", lambda: b.filter_sums("T", (0, -1))), ("ry", lambda: b.filter_sums("T", (0, 33))),
                     ("2 rx", lambda: b.filter_sums("T", (32, 0))),                     # (2 rx + 1 = 65 > Nx = 64)
                     ("sx", lambda: b.filter_sums("T", (1, 1), (5, 1))), ("sx", lambda: b.filter_sums("T", (1, 1), (0, 1))),
                     ("sy", lambda: b.filter_sums("T", (1, 1), (1, 5))), ("sy", lambda: b.filter_sums("v", (1, 1), (1, Ny + 1))),
                     ("window", lambda: b.filter_sums("T", (1, 1), levels=(Nz, 1))), ("window", lambda: b.filter_sums("T", (1, 1), levels=(0, 0))),
                     ("window", lambda: b.filter_sums("eta", (1, 1), levels=(0, 2))),
                     ("window", lambda: b.compute_filter_sums("w", (1, 1), levels=(Nz + 1, 1))),
                     ("wx", lambda: b.filter_sums("T", (1, 1), wx=-ones3)), ("wx", lambda: b.filter_sums("T", (1, 1), wx=np.r_[1.0, np.nan, 1.0])),
                     ("wy", lambda: b.filter_sums("T", (1, 1), wy=np.r_[1.0, np.inf, 1.0])), ("wy", lambda: b.filter_sums("T", (1, 1), wy=0 * ones3)),
                     ("wx", lambda: b.filter_sums("T", (1, 1), wx=np.ones(5))), ("wx", lambda: b.filter_sums("kinetic_energy", (1, 1), wx=0 * ones3)),
                     ("rx_of_row", lambda: b.filter_sums("T", (1, 1), wx=ones3, rx_of_row=np.ones(Ny, np.int32))),
                     ("rx_of_row", lambda: b.filter_sums("T", (1, 1), rx_of_row=np.full(Ny, 32, np.int32))),
                     ("rx_of_row", lambda: b.filter_sums("T", (1, 1), rx_of_row=np.r_[np.ones(Ny - 1, np.int32), -1])),
                     ("rx_of_row", lambda: b.filter_sums("T", (1, 1), rx_of_row=np.ones(Ny - 1, np.int32))),
                     ("no output", lambda: b.filter_sums("T", (1, 1), planes=())),
                     ("no output", lambda: b.filter_sums("kinetic_energy", (1, 1), planes=())),
                     ("GB25_D_VORTICITY", lambda: b.filter_sums("vorticity", (1, 1))),
                     ("no field", lambda: b.filter_sums("no_such_field", (1, 1)))):
        with pytest.raises(gb.GB25Error, match=word):
            fn()
        assert_same_sums(b.filter_sums("T", (2, 3), (4, 2)), good, word)


def test_a_rank_refuses():
    m = SlabModel(96, 40, 10, dt=600.0, rank=0, nranks=1, slab_mode=1, transport="rccl")
    b = m.backend
    assert b.filter_dims("T", (2, 3)) == (96, 40, 10)
    for fn in (lambda: b.filter_sums("T", (2, 3)), lambda: b.compute_filter_sums("T", (2, 3)), lambda: b.filter_sums("kinetic_energy", (1, 1))):
        with pytest.raises(gb.GB25Error, match="rank of a decomposition"):
            fn()
    assert b.filter_dims("u", (2, 3), (4, 2)) == (24, 20, 10)      # (the model still answers)
    b.close()


@pytest.mark.parametrize("P,Ry,grid_type", [(2, 1, 1), (4, 1, 1), (4, 2, 4)])
def test_the_ensemble_equals_the_single_domain(P, Ry, grid_type):
    if Ry == 1:
        Nx, Ny, Nz, dt, kw = (96 if P == 2 else 128), 40, 10, 600.0, {}      # (a slab is at least 30 columns wide)
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
    for name in ("u", "v", "T"):
        assert np.array_equal(ens.gather(name), sb.get_field(name, False)), name     # (the premise)
    g = kernel_weights("gaussian", 4)
    for name in ("T", "u", "v"):
        for spec in (dict(radius=(2, 3)), dict(radius=(4, 4), stride=(4, 2), wx=g, wy=g), dict(radius=(32, 32), levels=(Nz - 1, 1)),
                     dict(radius=(0, 2), rx_of_row=rows_for_length(sb, name, 3.0e6), levels=(1, -1))):
            want = call(sb.filter_sums, name, spec)
            got = call(ens.filter_sums, name, spec)
            print(f"  {P} ranks ({Ry} in y) grid {grid_type} {name} {describe(spec)}: differing outputs {(got.first != want.first).sum()} of "
                  f"{want.first.size}, non-zero {(want.first != 0).sum()}, empty {want.empty}")
            assert_same_sums(got, want, f"{name} {describe(spec)}")
            assert (want.first != 0).any()
    with pytest.raises(gb.GB25Error, match="rank of a decomposition"):
        ens.backends[0].filter_sums("T", (1, 1))
    ens.close()
    sb.close()


LOOKAHEADS = dict(subcycle_lookahead=1, ab2_lookahead=1)


def _burst(b, Nz, step):
    """Filter calls of every kind."""
    g = kernel_weights("gaussian", 2)
    b.filter_sums("T", (2, 2), wx=g, wy=g)
    b.filter_sums("u", (4, 1), (4, 2), (Nz // 2, 2))
    b.filter_sums("v", (1, 3))
    b.filter_sums("w", (0, 0))
    b.filter_sums("eta", (3, 3), (2, 2))
    b.filter_sums("pHY", (2, 2), (4, 4))                      # (a stale pHY is recomputed under the diagnostics timer)
    b.filter_sums("kinetic_energy", (2, 2), levels=(1 + step % 3, 1))
    b.filter_sums("mixed_layer_depth", (2, 2))
    b.filter_sums("S", (0, 1), rx_of_row=np.arange(b.field_dims("T", False)[1], dtype=np.int32) % 5)
    b.compute_filter_sums("S", (1, 1))


@pytest.mark.parametrize("float_type,grid_type,catke", [("Float32", 0, False), ("Float64", 4, False), ("Float32", 4, True)])
def test_asking_changes_nothing(float_type, grid_type, catke):
    """Three identical models; one is asked between every two steps.  Same bits, the look-aheads alive, every option unchanged,
    the same launches of every phase of a step (tests/test_gpu_blocks.py, test_asking_changes_nothing)."""
    closure = gb.CATKEVerticalDiffusivity() if catke else None
    watched, alone, control = (stepped_model(float_type, grid_type, steps=0, closure=closure, **LOOKAHEADS) for _ in range(3))
    Nz = size_of(grid_type)[2]
    names = BASE_FIELDS + (CATKE_FIELDS if catke else [])
    for m in (watched, alone):
        m.backend.profile_enable(True)
        m.backend.profile_reset()
    wb = watched.backend
    # asking with no step between: the fields, the look-ahead state and every option stay what they were
    before = {n: wb.get_field(n, True) for n in names}
    state, options = wb.lookahead_state(), {o: wb.get_option(o) for o in OPTION_IDS}
    _burst(wb, Nz, 0)
    assert wb.lookahead_state() == state and {o: wb.get_option(o) for o in OPTION_IDS} == options
    for n in names:
        assert np.array_equal(wb.get_field(n, True), before[n], equal_nan=True), n
    for step in range(6):
        state = wb.lookahead_state()
        _burst(wb, Nz, step)
        assert wb.lookahead_state() == state, step
        for m in (watched, alone, control):
            gb.time_step(m)
        assert wb.lookahead_state() == alone.backend.lookahead_state(), step
    assert {o: wb.get_option(o) for o in OPTION_IDS} == options
    for n in names:
        assert np.array_equal(alone.backend.get_field(n, True), control.backend.get_field(n, True), equal_nan=True), \
            f"two models that were never asked differ in {n}"
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
    for m in (watched, alone, control):
        m.backend.close()
