"""Block sums on the device (gb25_get_block_sums, gb25_compute_block_sums, gb25_get_derived_block_sums) against their numpy
restatement (gb-25_amd/blocks.py, pinned on the CPU by tests/test_blocks_host.py) of the DOWNLOADED parents: every plane and the info
record bit for bit on every grid type in both float types, windows of levels, level weights, tiles in x, a planted NaN, the
totals against gb25_integrate_field, decomposition invariance, the device pointer, the argument errors, and the proof that asking
changes nothing a model computes.

Shapes: the smallest each grid type accepts (helpers.size_of), a few steps in; they still have a wall row, the periodic seam, the
fold's pivot row, immersed columns and partially immersed ones.  A comparison of zeros with zeros cannot pass: `first` must be
non-zero in at least a quarter of the non-empty blocks of T and of u in every case.  The test prints the counts.

Totals: the integrals' bound, (n + 4) eps(Float64) sum|term| (tests/test_gpu_integrals.py)."""
import math

import numpy as np
import pytest

import gb25_amd as gb
from gb25_amd.binding import KERNEL_IDS, OPTION_IDS
from gb25_amd.blocks import PLANES, block_sums_host, column_area, depth_weights
from gb25_amd.distributed import LocalSlabEnsemble
from gb25_amd.integrals import cell_measure
from helpers import BASE_FIELDS, CATKE_FIELDS, EPS, GRID_NAMES, counter_rng, size_of, stepped_model

pytestmark = pytest.mark.gpu
CASES = [(ft, gt) for ft in ("Float32", "Float64") for gt in (0, 1, 3, 4)]
FIELDS = ("T", "S", "u", "v", "w", "eta", "U")
DERIVED = ("kinetic_energy", "potential_density", "mixed_layer_depth")

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
    """[(block, levels)] of a source with nlev levels: the issue's blocks and windows."""
    Nx, Ny, Nz = size_of(grid_type)
    bx, by = (3, 2) if (Nx, Ny, Nz) == (48, 24, 6) else (4, 2)
    if nlev == 1:
        return [((1, 1, 1), None), ((4, 4, 1), (0, 1)), ((bx, by, 1), (0, -1)), ((Nx, 1, 1), None), ((16, 8, 1), None)]
    even = (nlev % 2, nlev - nlev % 2)
    return [((1, 1, nlev), None), ((4, 4, 1), None), ((bx, by, 2), even), ((Nx, 1, 1), None), ((1, 1, 1), None), ((16, 8, nlev), None),
            ((4, 4, 1), (0, 1)), ((bx, by, 1), (Nz - 1, 1)), ((bx, by, 2), (Nz // 2, 2)), ((1, 1, nlev - 1), (1, -1))]


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_same_sums(got, want, what):
    for plane in PLANES:
        g, w = getattr(got, plane), getattr(want, plane)
        bad = int((g != w).sum())
        if bad:
            print(f"    {what} {plane}: {bad} of {w.size} blocks differ, max |delta| {np.abs(g - w).max():.3e} of max {np.abs(w).max():.3e}")
        assert same(g, w), (what, plane)
    assert got.info == want.info, (what, got.info, want.info)


@pytest.mark.parametrize("float_type,grid_type", CASES)
def test_every_plane_bit_for_bit(float_type, grid_type):
    b = model_of(float_type, grid_type).backend
    Nx, Ny, Nz = size_of(grid_type)
    for source in FIELDS + DERIVED:
        nlev = levels_of(b, source)
        values = b.get_derived(source, 0.03 if source == "mixed_layer_depth" else None) if source in DERIVED else None
        for block, levels in specs_of(grid_type, nlev):
            want = block_sums_host(b, source, block, levels, values=values)
            got = b.block_sums(source, block, levels)
            assert got.dims == want.dims == b.block_dims(source, block, levels), (source, block, levels)
            assert_same_sums(got, want, f"{source} {block} {levels}")
            assert got.nonfinite == 0 and got.points == want.points_of_blocks.sum()
            if source in ("T", "u"):
                full = want.measure > 0
                nonzero = int((want.first[full] != 0).sum())
                print(f"  {float_type} grid {grid_type} {source} {block} {levels}: first != 0 in {nonzero} of {int(full.sum())} non-empty blocks, "
                      f"empty {want.empty_blocks}, points {want.points}")
                assert 4 * nonzero >= int(full.sum()) > 0, (source, block, levels)
        assert_same_sums(b.block_sums(source, block, levels), got, f"{source} again")   # repeatable
    cols = block_sums_host(b, "T", (1, 1, Nz))
    if grid_type in (1, 4):
        partial = int(((cols.points_of_blocks > 0) & (cols.points_of_blocks < Nz)).sum())
        print(f"  {float_type} grid {grid_type}: columns empty {cols.empty_blocks}, partial {partial} of {Nx * Ny}")
        assert cols.empty_blocks > 0 and partial > 0, "the islands give dry and partial columns"
        assert b.block_sums("T", (1, 1, Nz)).empty_blocks == cols.empty_blocks
    if grid_type in (3, 4):
        # the pivot row's blocks carry the 1/2: the measure with and without it, on the host
        one = b.block_sums("T", (1, 1, 1)).measure
        dz = np.array([b.metric("dzc", k) for k in range(1, Nz + 1)], np.float64)
        H = int(b.cfg.halo)
        az = np.asarray(b.metric2("azcc"), np.float64)[H:H + Nx, H:H + Ny]
        for j, fold in ((Ny - 1, 0.5), (Ny - 2, 1.0)):
            whole = az[:, j, None] * dz[None, :]
            wet = one[:, j] > 0
            assert wet.any() and np.array_equal(one[:, j][wet], (whole * fold)[wet]), j
            assert fold == 1.0 or not np.array_equal(one[:, j][wet], whole[wet])


@pytest.mark.parametrize("float_type,grid_type", CASES)
def test_unit_blocks_are_the_measure_and_the_totals_are_the_integrals(float_type, grid_type):
    b = model_of(float_type, grid_type).backend
    Ny = size_of(grid_type)[1]
    for name in FIELDS:
        mu = cell_measure(b, name)[:, :Ny]
        x = np.asarray(b.get_field(name, False), np.float64)[:, :Ny]
        one = b.block_sums(name, (1, 1, 1))
        wet = mu > 0
        assert same(one.measure, np.where(wet, mu, 0.0)) and same(one.first, np.where(wet, mu * np.where(wet, x, 0.0), 0.0)), name
        total = b.integrate_field(name, "total")
        terms = {"measure": mu[wet], "first": (mu * x)[wet], "second": (mu * x * x)[wet]}
        n = int(wet.sum())
        nlev = x.shape[2]
        for block in ((1, 1, nlev), (4, 4, 1), (1, 1, 1)):
            s = b.block_sums(name, block)
            assert (s.points, s.nonfinite) == (int(total["points"]), int(total["nonfinite"])) and s.points == n, (name, block)
            for plane in PLANES:
                host_sum = float(np.add.accumulate(getattr(s, plane).ravel(order="F"))[-1])      # left to right, I fastest
                bound = (n + 4) * EPS * math.fsum(np.abs(terms[plane]))
                print(f"    {float_type} grid {grid_type} {name} {block} {plane}: blocks {host_sum!r} integral {float(total[plane])!r} "
                      f"|diff| {abs(host_sum - float(total[plane])):.3e} bound {bound:.3e}")
                assert abs(host_sum - float(total[plane])) <= bound, (name, block, plane)


@pytest.mark.parametrize("float_type,grid_type", [("Float32", 0), ("Float64", 1), ("Float32", 3), ("Float64", 4)])
def test_level_weights(float_type, grid_type):
    m = model_of(float_type, grid_type)
    b = m.backend
    Nx, Ny, Nz = size_of(grid_type)
    for name, block in (("T", (3 if Nx == 48 else 4, 2, 2)), ("u", (1, 1, Nz)), ("w", (4, 4, 1)), ("kinetic_energy", (4, 4, 2))):
        nlev = levels_of(b, name)
        plain, ones = b.block_sums(name, block), b.block_sums(name, block, None, np.ones(nlev))
        for plane in PLANES:
            assert same(getattr(plain, plane), getattr(ones, plane)), (name, plane)
        assert plain.info == ones.info
        lw = 0.125 + counter_rng((nlev,), 9, 1)
        lw[nlev // 2] = 0.0
        values = b.get_derived(name) if name in DERIVED else None
        assert_same_sums(b.block_sums(name, block, None, lw), block_sums_host(b, name, block, None, lw, values=values), f"{name} weighted")
    # zeros below k0, whole columns = the window from k0 on
    for k0 in (1, Nz // 2):
        lw = (np.arange(Nz) >= k0).astype(np.float64)
        a, w = b.block_sums("T", (1, 1, Nz), None, lw), b.block_sums("T", (1, 1, Nz - k0), (k0, Nz - k0))
        for plane in PLANES:
            assert same(getattr(a, plane), getattr(w, plane)), (k0, plane)
        assert a.info == w.info and a.points > 0
    # the heat content down to a depth inside a level: the host formula from the restated planes
    zf = np.array([b.metric("zf", k) for k in range(1, Nz + 2)], np.float64)
    d = -0.5 * (zf[Nz - 2] + zf[Nz - 1])
    lw = depth_weights(b, 0.0, d)
    assert 0 < lw[Nz - 2] < 1 and lw[Nz - 1] == 1
    top = block_sums_host(b, "T", (1, 1, Nz), None, lw)
    area = block_sums_host(b, "eta", (1, 1, 1)).measure[:, :, 0]
    assert same(column_area(b, "T"), area)
    ocean = area > 0
    want = np.where(ocean, (b.cfg.rho0 * 3991.86795711963) * top.first[:, :, 0] / np.where(ocean, area, 1.0), 0.0)
    hc = gb.heat_content(m, depth_range=(0.0, d))
    assert same(hc, want) and (hc[ocean] != 0).all()
    assert np.array_equal(gb.depth_mean(m, "T", (0.0, d)), top.mean()[:, :, 0], equal_nan=True)
    assert np.array_equal(gb.coarsen(m, "T", (4, 4, 2)), block_sums_host(b, "T", (4, 4, 2)).mean(), equal_nan=True)
    assert np.array_equal(gb.subgrid_variance(m, "u", (4, 4, 1)), block_sums_host(b, "u", (4, 4, 1)).variance(), equal_nan=True)
    assert np.array_equal(m.tracers.T.coarsen((4, 4, 2)), gb.coarsen(m, "T", (4, 4, 2)), equal_nan=True)
    assert gb.column_integral(m, "T").shape == (Nx, Ny)


@pytest.mark.parametrize("float_type,grid_type", [("Float32", 0), ("Float64", 4)])
def test_a_planted_nan(float_type, grid_type):
    m = stepped_model(float_type, grid_type)
    b = m.backend
    Nx, Ny, Nz = size_of(grid_type)
    block = (3 if Nx == 48 else 4, 2, 2)
    mu = cell_measure(b, "T")
    before = b.block_sums("T", block)
    wet = np.argwhere(mu[:, :, Nz - 1] > 0)
    i0, j0 = (int(q) for q in wet[len(wet) // 2])
    T = b.get_field("T", False)
    T[i0, j0, Nz - 1] = np.nan
    b.set_field("T", T, False)
    got, want = b.block_sums("T", block), block_sums_host(b, "T", block)
    at = (i0 // block[0], j0 // block[1], (Nz - 1) // block[2])
    was = block_sums_host(b, "T", block, values=np.where(np.isnan(T), 0.0, T))
    print(f"  {float_type} grid {grid_type}: NaN at ({i0}, {j0}, {Nz - 1}), block {at}: points {was.points_of_blocks[at]} -> {want.points_of_blocks[at]}")
    assert got.nonfinite == 1 and got.points == before.points - 1 and want.points_of_blocks[at] == was.points_of_blocks[at] - 1
    assert_same_sums(got, want, "planted NaN")
    assert np.isfinite(got.first).all() and np.isfinite(got.second).all() and got.measure[at] < before.measure[at]
    others = np.ones(got.dims, bool)
    others[at] = False
    for plane in PLANES:
        assert same(getattr(got, plane)[others], getattr(before, plane)[others]), plane
    # one in an immersed cell changes nothing
    if grid_type == 4:
        dry = np.argwhere(mu[:, :, 0] == 0)
        i1, j1 = (int(q) for q in dry[len(dry) // 2])
        T[i1, j1, 0] = np.inf
        b.set_field("T", T, False)
        again = b.block_sums("T", block)
        for plane in PLANES:
            assert same(getattr(again, plane), getattr(got, plane)), plane
        assert again.info == got.info
    b.close()


def test_tiles_in_x():
    """Wider than one tile of 256 columns: bx = 5 gives tiles of 255 columns and a short last one, bx = 64 two tiles of 256 and 64."""
    Nx, Ny, Nz = 320, 32, 8
    m = stepped_model("Float32", 0, steps=1, size=(Nx, Ny, Nz))
    b = m.backend
    for name in ("T", "u", "w", "eta"):
        nlev = levels_of(b, name)
        for block in ((5, 2, 1), (64, 4, nlev), (1, 1, nlev), (160, 1, 1), (2, 32, 1)):
            got, want = b.block_sums(name, block), block_sums_host(b, name, block)
            assert got.dims == (Nx // block[0], Ny // block[1], nlev // block[2])
            assert_same_sums(got, want, f"{name} {block}")
            assert (want.first != 0).any()
    b.close()


@pytest.mark.parametrize("P,Ry,grid_type", [(2, 1, 1), (4, 1, 1), (4, 2, 4)])
def test_gathered_ranks_equal_the_single_domain(P, Ry, grid_type):
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
    for name in ("u", "v", "T", "S"):
        assert np.array_equal(ens.gather(name), sb.get_field(name, False)), name     # (the premise)
    lw = 0.25 + counter_rng((Nz,), 3, 1)
    for name in ("T", "u"):
        for block, levels, w in (((4, 2, 2), None, None), ((1, 1, Nz), None, lw), ((Nx // (P // Ry), 4, 1), (Nz - 1, 1), None), ((2, 2, 1), (1, -1), None)):
            want = sb.block_sums(name, block, levels, w)
            got = ens.block_sums(name, block, levels, w)
            print(f"  {P} ranks ({Ry} in y) grid {grid_type} {name} {block}: differing blocks {(got.first != want.first).sum()} of {want.first.size}, "
                  f"non-zero {(want.first != 0).sum()}, empty {want.empty_blocks}")
            assert got.dims == want.dims and got.global_offset == (0, 0, 0)
            assert_same_sums(got, want, f"{name} {block}")
            assert (want.first != 0).any()
    with pytest.raises(gb.GB25Error, match="bx"):
        ens.block_sums("T", (2 * (Nx // (P // Ry)), 1, 1))      # (divides the grid's Nx, not a rank's)
    ens.close()
    sb.close()


def test_the_device_pointer():
    b = model_of("Float64", 1).backend
    other = model_of("Float32", 1).backend
    Nx, Ny, Nz = size_of(1)
    for name, block, levels, lw in (("T", (3, 2, 2), None, None), ("u", (1, 1, Nz), None, 0.5 + counter_rng((Nz,), 5, 1)), ("eta", (4, 4, 1), None, None),
                                    ("w", (4, 4, 1), (Nz, 1), None), ("T", (1, 1, 2), None, None)):
        want = b.block_sums(name, block, levels, lw)
        ptr, dims, info = b.compute_block_sums(name, block, levels, lw)
        assert ptr and dims == want.dims and tuple(info.dims) == dims
        assert (info.points, info.nonfinite, info.empty_blocks, tuple(info.global_offset)) == (want.points, want.nonfinite, want.empty_blocks, want.global_offset)
        if block[:2] == (1, 1):
            # a full-resolution map: the three planes one after another, read through gb25_compare_field of ANOTHER model as one
            # array of 3 dims[2] levels
            d3 = (Nx, Ny, 3 * dims[2])
            for q, plane in enumerate(PLANES):
                x = getattr(want, plane)
                for n in range(dims[2]):
                    d = other.compare_field("eta", ptr, real_bytes=8, dims=d3, origin=(0, 0, q * dims[2] + n))
                    assert d.max_abs_b == np.abs(x[:, :, n]).max() and d.sum_sq_b > 0 and d.nonfinite == 0, (name, plane, n)
        again = b.compute_block_sums(name, block, levels, lw)
        assert again[1] == dims and again[2] == info                 # repeatable call to call
        assert_same_sums(b.block_sums(name, block, levels, lw), want, name)
    # only the planes asked for
    only = b.block_sums("T", (4, 4, 1), None, None, None, planes=("first",))
    assert only.measure is None and only.second is None and same(only.first, b.block_sums("T", (4, 4, 1)).first)


def test_argument_errors_leave_the_model_usable():
    b = model_of("Float32", 0).backend
    Nx, Ny, Nz = size_of(0)
    good = b.block_sums("T", (4, 4, 2))
    for word, call in (("bx", lambda: b.block_sums("T", (0, 1, 1))), ("bx", lambda: b.block_sums("T", (5, 1, 1))),
                       ("bx", lambda: b.block_sums("T", (8 * Nx, 1, 1))), ("by", lambda: b.block_sums("T", (1, 5, 1))),
                       ("by", lambda: b.block_sums("v", (1, Ny + 1, 1))), ("by", lambda: b.block_sums("T", (1, -1, 1))),
                       ("bz", lambda: b.block_sums("T", (1, 1, 3))), ("bz", lambda: b.block_sums("eta", (1, 1, 2))),
                       ("bz", lambda: b.block_sums("w", (1, 1, 2))),
                       ("window", lambda: b.block_sums("T", (1, 1, 1), (Nz, 1))), ("window", lambda: b.block_sums("T", (1, 1, 1), (0, 0))),
                       ("window", lambda: b.block_sums("T", (1, 1, 1), (2, Nz))), ("window", lambda: b.block_sums("eta", (1, 1, 1), (0, 2))),
                       ("window", lambda: b.compute_block_sums("w", (1, 1, 1), (Nz + 1, 1))),
                       ("level_weight", lambda: b.block_sums("T", (1, 1, 1), None, -np.ones(Nz))),
                       ("level_weight", lambda: b.block_sums("T", (1, 1, 1), None, np.r_[np.ones(Nz - 1), np.nan])),
                       ("level_weight", lambda: b.block_sums("T", (1, 1, 1), None, np.r_[np.ones(Nz - 1), np.inf])),
                       ("level_weight", lambda: b.block_sums("T", (1, 1, 1), None, np.ones(Nz + 1))),
                       ("level_weight", lambda: b.block_sums("eta", (1, 1, 1), None, np.ones(1))),
                       ("level_weight", lambda: b.block_sums("mixed_layer_depth", (1, 1, 1), None, np.ones(1))),
                       ("no output", lambda: b.block_sums("T", (1, 1, 1), planes=())),
                       ("no output", lambda: b.block_sums("kinetic_energy", (1, 1, 1), planes=())),
                       ("GB25_D_VORTICITY", lambda: b.block_sums("vorticity", (1, 1, 1))),
                       ("no field", lambda: b.block_sums("no_such_field", (1, 1, 1)))):
        with pytest.raises(gb.GB25Error, match=word):
            call()
        assert_same_sums(b.block_sums("T", (4, 4, 2)), good, word)


LOOKAHEADS = dict(subcycle_lookahead=1, ab2_lookahead=1)


def _burst(b, Nz, step):
    """Block-sum calls of every kind."""
    lw = 0.5 + counter_rng((Nz,), 1, step)
    b.block_sums("T", (1, 1, Nz), None, lw)
    b.block_sums("u", (4, 4, 1), (Nz // 2, 2))
    b.block_sums("v", (2, 2, 2))
    b.block_sums("w", (1, 1, 1))
    b.block_sums("eta", (4, 2, 1))
    b.block_sums("pHY", (4, 4, Nz))                        # (a stale pHY is recomputed under the diagnostics timer)
    b.block_sums("kinetic_energy", (4, 4, 1), (1 + step % 3, 1))
    b.block_sums("mixed_layer_depth", (2, 2, 1))
    b.compute_block_sums("S", (1, 1, Nz))


@pytest.mark.parametrize("float_type,grid_type,catke", [("Float32", 0, False), ("Float64", 4, False), ("Float32", 4, True)])
def test_asking_changes_nothing(float_type, grid_type, catke):
    """Three identical models; one is asked between every two steps.  Same bits, the look-aheads alive, every option unchanged,
    the same launches of every phase of a step.  The two models that are never asked must agree with each other too: a step is
    reproducible (tests/test_gpu_reproducible.py; the Float64 grid-4 case used to differ between two such models because a block
    allocated in mid-run was zeroed behind its first kernels -- DESIGN.md, "Reproducibility of a step")."""
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
