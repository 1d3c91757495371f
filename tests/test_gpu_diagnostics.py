"""Device diagnostics (gb25_get_field_stats, gb25_compare_field, gb25_get_state_monitor) against numpy on the downloaded
fields, and the proof that asking for them changes nothing a model computes.

Sums: the kernels add fp64 terms in a fixed but not sequential order; any order of n terms is within (n - 1) eps(Float64)
sum|term| of the exact sum (Higham, Accuracy and Stability of Numerical Algorithms, eq. 4.4 to first order), and math.fsum
gives the exact sum correctly rounded, so the bound asserted is n eps sum|term|.  Everything else is exact."""
import math

import numpy as np
import pytest

import gb25_amd as gb
from gb25_amd.binding import FIELD_IDS
from gb25_amd.distributed import LocalSlabEnsemble
from helpers import BASE_FIELDS, CASES, CATKE_FIELDS, EPS, GRID_NAMES, counter_rng, set_noisy_velocities, size_of, stepped_model

pytestmark = pytest.mark.gpu


def memory_order(a):
    """The values of an [i, j, k] array in memory order (i fastest)."""
    return np.asarray(a, np.float64).transpose(2, 1, 0).ravel()


def position(offset, shape):
    """1-based (i, j, k) of a linear offset in memory order."""
    return (offset % shape[0] + 1, offset // shape[0] % shape[1] + 1, offset // (shape[0] * shape[1]) + 1)


def assert_sum(got, terms, what):
    exact, bound = math.fsum(terms), len(terms) * EPS * math.fsum(np.abs(terms))
    print(f"    {what}: device {got!r} fsum {exact!r} |diff| {abs(got - exact):.3e} bound {bound:.3e}")
    assert abs(got - exact) <= bound, (what, got, exact, bound)


def check_stats(s, a, what):
    """s: FieldStats of the [i, j, k] array a."""
    x = memory_order(a)
    fin = np.isfinite(x)
    xf = x[fin]
    print(f"  {what}: n {x.size} min {s.min!r} max {s.max!r} max_abs {s.max_abs!r} at {tuple(s.at_max_abs)} nonfinite {s.nonfinite}")
    assert s.count == x.size and s.nonfinite == int((~fin).sum()), what
    assert s.min == xf.min() and s.max == xf.max() and s.max_abs == np.abs(xf).max(), what
    first_max = int(np.argmax(np.where(fin, np.abs(x), -1.0)))         # (argmax: the first of equal values)
    assert tuple(s.at_max_abs) == position(first_max, a.shape), what
    want_first = position(int(np.argmax(~fin)), a.shape) if s.nonfinite else (0, 0, 0)
    assert tuple(s.first_nonfinite) == want_first, what
    assert_sum(s.sum, xf, what + " sum")
    assert_sum(s.sum_sq, xf * xf, what + " sum_sq")


@pytest.mark.parametrize("float_type,grid_type", CASES)
def test_field_stats_of_every_field(float_type, grid_type):
    m = stepped_model(float_type, grid_type)
    b = m.backend
    for name in BASE_FIELDS:
        for halos in (False, True):
            check_stats(b.field_stats(name, halos), b.get_field(name, halos), f"{name} halos={halos}")
    assert m.tracers.T.stats().as_dict() == b.field_stats("T").as_dict()
    assert tuple(b.field_stats("T", True).global_offset) == (-8, -8, -8) and tuple(b.field_stats("eta").global_offset) == (0, 0, 0)
    with pytest.raises(gb.GB25Error, match="no such field"):
        b.field_stats("e")
    b.close()


@pytest.mark.parametrize("float_type", ["Float32", "Float64"])
def test_field_stats_of_the_catke_fields(float_type):
    m = stepped_model(float_type, 0, closure=gb.CATKEVerticalDiffusivity())
    b = m.backend
    for name in CATKE_FIELDS + ["u", "T"]:
        for halos in (False, True):
            check_stats(b.field_stats(name, halos), b.get_field(name, halos), f"{name} halos={halos}")
    b.close()


@pytest.mark.parametrize("float_type", ["Float32", "Float64"])
def test_ties_and_nonfinite_values(float_type):
    m = stepped_model(float_type, 0, steps=0)
    b = m.backend
    T = b.get_field("T", False).copy()
    big = float(np.abs(T).max()) * 2
    # two equal maxima of |x|: (40, 3, 5) lies BEHIND (7, 20, 2) in memory although its i, j are ahead in C order
    T[39, 2, 4] = -big
    T[6, 19, 1] = big
    b.set_field("T", T, False)
    s = b.field_stats("T")
    assert s.max_abs == np.float64(T.dtype.type(big)) and tuple(s.at_max_abs) == (7, 20, 2)
    check_stats(s, T, "T with a tie")
    # the same in one row, both inside one 16-byte chunk and in chunks of different lanes
    for i1, i2 in ((9, 10), (3, 60)):
        T2 = T.copy()
        T2[i1, 5, 0] = T2[i2, 5, 0] = 3 * big
        b.set_field("T", T2, False)
        assert tuple(b.field_stats("T").at_max_abs) == (i1 + 1, 6, 1)
    # a NaN and an Inf: counted, the earlier one reported, everything else over the remaining values
    T[50, 10, 3] = np.nan
    T[2, 30, 1] = np.inf
    b.set_field("T", T, False)
    s = b.field_stats("T")
    assert s.nonfinite == 2 and tuple(s.first_nonfinite) == (3, 31, 2)
    check_stats(s, T, "T with NaN and Inf")
    check_stats(b.field_stats("T", True), b.get_field("T", True), "parent of T with NaN and Inf")
    mon = b.state_monitor()
    assert mon.nonfinite_total == 2 and mon.T.as_dict() == s.as_dict()
    b.close()


def host_record(name, a, b, rtol):
    """One record of compare_states' numpy path (gb-25_amd/correctness.py, _compare)."""
    from gb25_amd.correctness import _compare
    out = []
    _compare(name, a, b, rtol, 0.0, out)
    return out[0]


BACKEND_NAME = {"filtered.U": "U_bar", "filtered.V": "V_bar", "filtered.eta": "eta_bar"}


def assert_reports_agree(dev, host, m1, m2, include_halos, what, unique=False):
    """Every record of the device path against the host path's.  The position: where |delta| attains its maximum once, both
    paths must name that place (unique=True asserts that precondition: pairs whose differences are not a few ulps); where it
    attains it several times -- two schedules differ by one or two ulps in many places, and the periodic halo columns repeat
    interior values -- the host path's argmax walks k fastest and the device reports Julia's findmax, the smallest offset in
    memory order, which is recomputed here."""
    assert [r["name"] for r in dev] == [r["name"] for r in host]
    for d, h in zip(dev, host):
        print(f"  {what} {d['name']}: rel {d['rel']:.6e} / {h['rel']:.6e} maxdelta {d['maxdelta']:.6e} at {d['index']} ok {d['ok']}")
        assert (d["max1"], d["max2"], d["maxdelta"], d["ok"]) == (h["max1"], h["max2"], h["maxdelta"], h["ok"]), (what, d, h)
        name = BACKEND_NAME.get(d["name"], d["name"])
        a = m1.backend.get_field(name, include_halos).astype(np.float64)
        b = m2.backend.get_field(name, include_halos).astype(np.float64)[:a.shape[0], :a.shape[1], :a.shape[2]]
        delta = np.abs(a - b)
        once = delta.max() == 0 or int((delta == delta.max()).sum()) == 1
        if unique:
            assert once, f"precondition: |delta| of {name} attains its maximum twice"
        if once:
            assert d["index"] == h["index"], (what, d, h)
        assert d["index"] == position(int(np.argmax(memory_order(delta))), a.shape), (what, d)
        # rel = sqrt(S_d) / sqrt(max(S_a, S_b)): each sum of n squares within n eps of its exact value relatively (all terms
        # are non-negative, on the device and in numpy alike), so the quotient of the roots within 2 n eps, plus the roundings
        assert abs(d["rel"] - h["rel"]) <= (2 * a.size + 8) * EPS * h["rel"], (what, d, h)


def report_pair(m1, m2, rtol, include_halos=False):
    _, dev = gb.compare_states(m1, m2, rtol=rtol, include_halos=include_halos, verbose=False, on_device=True)
    _, host = gb.compare_states(m1, m2, rtol=rtol, include_halos=include_halos, verbose=False, on_device=False)
    return dev, host


@pytest.mark.parametrize("float_type,grid_type", CASES)
def test_compare_states_on_the_device_equals_the_host_path(float_type, grid_type):
    rtol = math.sqrt(np.finfo(np.float32 if float_type == "Float32" else np.float64).eps)
    # another schedule, last bits differ: the direct-stencil kernels on the flat grid; where there is a bottom (they know
    # none) another chunking of the momentum kernel's levels, i.e. another association of the column integrals of u, v
    size = None if grid_type == 0 else (48, 24, 14)
    other = dict(kernels=1) if grid_type == 0 else dict(momentum_chunk_levels=6)
    m1 = stepped_model(float_type, grid_type, steps=4, size=size)
    m2 = stepped_model(float_type, grid_type, steps=4, size=size, **other)
    for halos in (False, True):
        dev, host = report_pair(m1, m2, rtol, halos)
        assert_reports_agree(dev, host, m1, m2, halos, f"{other} halos={halos}")
    assert any(r["maxdelta"] > 0 for r in dev)
    # a model against itself: all zeros, ok
    ok, rep = gb.compare_states(m1, m1, verbose=False, on_device=True)
    assert ok and all(r["maxdelta"] == 0 and r["rel"] == 0 and r["index"] == (1, 1, 1) for r in rep)
    # another noise: not ok on either path
    m3 = stepped_model(float_type, grid_type, steps=4, size=size, seed=7)
    dev, host = report_pair(m1, m3, rtol)
    assert_reports_agree(dev, host, m1, m3, False, "other noise", unique=True)
    assert not all(r["ok"] for r in dev)
    for m in (m1, m2, m3):
        m.backend.close()


@pytest.mark.parametrize("grid_type", [0, 1, 4])
def test_compare_a_float32_with_a_float64_model(grid_type):
    m64 = stepped_model("Float64", grid_type, steps=0)
    Nx, Ny, Nz = size_of(grid_type)
    m32 = gb.baroclinic_instability_model(gb.GPU(float_type="Float32"), Nx, Ny, Nz, dt=m64.clock.last_dt, grid_type=GRID_NAMES[grid_type])
    gb.sync_states(m32, m64)
    gb.first_time_step(m32)
    for m in (m32, m64):
        gb.loop(m, 3)
    rtol = math.sqrt(np.finfo(np.float32).eps)
    for a, b in ((m32, m64), (m64, m32)):
        for halos in (False, True):
            dev, host = report_pair(a, b, rtol, halos)
            assert_reports_agree(dev, host, a, b, halos, f"{a.backend.float_type} against {b.backend.float_type} halos={halos}",
                                 unique=not halos)
    assert all(r["ok"] for r in dev if r["name"] in ("T", "S"))
    m32.backend.close()
    m64.backend.close()


@pytest.mark.parametrize("float_type", ["Float32", "Float64"])
def test_compare_with_a_larger_array_and_bad_arguments(float_type):
    """compare_parent's view(psi2, 1:Nx, 1:Ny, 1:Nz): the other model is larger in every direction."""
    small = stepped_model(float_type, 0, steps=2, size=(64, 32, 8))
    large = stepped_model("Float64" if float_type == "Float32" else "Float32", 0, steps=2, size=(80, 40, 10))
    b = small.backend
    for name in ("T", "u", "v", "w", "eta"):
        for halos in (False, True):
            a, o = b.get_field(name, halos), large.backend.get_field(name, halos)
            want = host_record(name, a, o, 1e-3)
            d = b.compare_field(name, large.backend, halos)
            from gb25_amd.correctness import diff_record
            got = diff_record(name, d, 1e-3, 0.0)
            assert (got["max1"], got["max2"], got["maxdelta"], got["ok"]) == \
                   (want["max1"], want["max2"], want["maxdelta"], want["ok"]), (name, halos, got, want)
            delta = np.abs(a.astype(np.float64) - o.astype(np.float64)[:a.shape[0], :a.shape[1], :a.shape[2]])
            assert got["index"] == position(int(np.argmax(memory_order(delta))), a.shape), (name, halos, got)
            if int((delta == delta.max()).sum()) == 1:
                assert got["index"] == want["index"], (name, halos, got, want)
            assert abs(got["rel"] - want["rel"]) <= (2 * a.size + 8) * EPS * want["rel"]
            assert d.count == a.size and d.nonfinite == 0
    before = large.backend.lookahead_state()
    ptr, dims = large.backend.field_device_ptr_readonly("T")
    assert dims == (96, 56, 26) and large.backend.lookahead_state() == before
    with pytest.raises(gb.GB25Error, match="status 1"):
        b.compare_field("T", ptr, real_bytes=2, dims=dims)
    with pytest.raises(gb.GB25Error, match="status 1"):
        b.compare_field("T", ptr, real_bytes=4, dims=(64, 32, 8), origin=(1, 0, 0))     # the box does not fit
    with pytest.raises(gb.GB25Error, match="status 1"):
        large.backend.compare_field("T", b, False)                                      # the other array is the smaller one
    small.backend.close()
    large.backend.close()


LOOKAHEADS = dict(subcycle_lookahead=1, ab2_lookahead=1)


@pytest.mark.parametrize("float_type,grid_type,catke", [("Float32", 0, False), ("Float64", 0, False), ("Float32", 1, False),
                                                        ("Float32", 4, False), ("Float64", 4, False), ("Float32", 0, True),
                                                        ("Float32", 4, True)])
def test_diagnostics_are_read_only(float_type, grid_type, catke):
    """Two identical models; one is asked for everything between every two steps.  Same bits, same look-ahead state, same
    launches of every phase of a step."""
    closure = gb.CATKEVerticalDiffusivity() if catke else None
    watched = stepped_model(float_type, grid_type, steps=0, closure=closure, **LOOKAHEADS)
    alone = stepped_model(float_type, grid_type, steps=0, closure=closure, **LOOKAHEADS)
    names = BASE_FIELDS + (CATKE_FIELDS if catke else [])
    for m in (watched, alone):
        m.backend.profile_enable(True)
        m.backend.profile_reset()
    for step in range(6):
        mon = watched.backend.state_monitor()
        assert mon.iteration == step + 1 and mon.nonfinite_total == 0 and mon.cfl > 0
        for name in names:
            watched.backend.field_stats(name, step % 2 == 0)
        watched.backend.compare_field("T", alone.backend)
        for m in (watched, alone):
            gb.time_step(m)
        assert watched.backend.lookahead_state() == alone.backend.lookahead_state(), step
    assert alone.backend.lookahead_state()[0], "the velocity look-ahead is on in this configuration"
    from gb25_amd.binding import KERNEL_IDS
    for k in KERNEL_IDS:
        if k != "diagnostics":
            assert watched.backend.profile_get(k)[0] == alone.backend.profile_get(k)[0], k
    assert watched.backend.profile_get("diagnostics")[0] > 0 and alone.backend.profile_get("diagnostics")[0] == 0
    for name in names:
        a, b = watched.backend.get_field(name, True), alone.backend.get_field(name, True)
        assert np.array_equal(a, b, equal_nan=True), name
    assert np.abs(watched.backend.get_field("u", False)).max() > 0
    for m in (watched, alone):
        m.backend.close()


@pytest.mark.parametrize("float_type,grid_type", [("Float32", 0), ("Float64", 4)])
def test_repeatable_to_the_last_bit(float_type, grid_type):
    m1, m2 = stepped_model(float_type, grid_type), stepped_model(float_type, grid_type)
    for name in ("u", "T", "eta", "Gn.v", "pHY"):
        for halos in (False, True):
            s = [bytes(m.backend.field_stats(name, halos)) for m in (m1, m1, m2)]
            assert s[0] == s[1] == s[2], (name, halos)
    mons = [bytes(m.backend.state_monitor()) for m in (m1, m1, m2)]
    assert mons[0] == mons[1] == mons[2]
    d = [bytes(a.backend.compare_field("u", b.backend, True)) for a, b in ((m1, m2), (m1, m2), (m2, m1))]
    assert d[0] == d[1] == d[2]
    m1.backend.close()
    m2.backend.close()


def blob(result):
    """Every array and number of a result, as bytes."""
    if isinstance(result, (tuple, list)):
        return b"|".join(blob(r) for r in result)
    if result is None or isinstance(result, (int, float)):
        return repr(result).encode()
    if isinstance(result, np.ndarray):
        return np.ascontiguousarray(result).tobytes()
    return blob([result.measure, result.first, result.second] + list(result.info.values()))      # (BlockSums, FilterSums)


@pytest.mark.parametrize("float_type,grid_type", [("Float32", 0), ("Float64", 4)])
def test_a_buffer_that_grows_and_is_reused(float_type, grid_type):
    """The families whose results grow with the request keep ONE allocation each, made anew when a call needs more bytes: a small
    request, one that needs more, the small one again.  The small results are the same bytes before and after the growth (a call
    finds its parts at offsets of its own, whatever the buffer has room for), and the large one is what a fresh model gives,
    whose buffer was made for exactly that request."""
    m, fresh = stepped_model(float_type, grid_type), stepped_model(float_type, grid_type)
    b, f = m.backend, fresh.backend
    Nx, Ny, Nz = size_of(grid_type)
    T = b.get_field("T", False)
    targets = np.linspace(float(T.min()), float(T.max()), 10)[1:9]
    edges = lambda n: np.linspace(float(T.min()), float(T.max()), n + 2)[1:-1]
    families = {
        "block sums": (lambda k: k.block_sums("T", (8, 8, Nz)), lambda k: k.block_sums("T", (1, 1, 1))),
        "filter sums": (lambda k: k.filter_sums("T", (1, 1), (8, 8), (0, 1), planes=("first",)), lambda k: k.filter_sums("T", (2, 3))),
        "zonal spectrum": (lambda k: k.zonal_spectrum("T", (0, 2), (0, 1)), lambda k: k.zonal_spectrum("T")),
        "on surfaces": (lambda k: k.get_on_surfaces("T", "depth", targets[:1]), lambda k: k.get_on_surfaces("T", "depth", targets)),
        "class sums": (lambda k: k.class_sums("cells", "T", edges(3), "cumulative"), lambda k: k.class_sums("cells", "T", edges(63), "cumulative")),
    }
    for name, (small, large) in families.items():
        first, second, third = blob(small(b)), blob(large(b)), blob(small(b))
        assert len(second) > len(first) > 0, name
        assert first == third, name
        assert second == blob(large(f)), name
        assert any(first) and any(second), name
    b.close()
    f.close()


@pytest.mark.parametrize("float_type,grid_type", [("Float32", 0), ("Float64", 0), ("Float32", 4), ("Float64", 4)])
def test_advective_cfl(float_type, grid_type):
    """max over the interior cells of |u|/dx + |v|/dy + |w|/dz, restated from the fields and the metric getters."""
    m = stepped_model(float_type, grid_type, steps=4)
    b = m.backend
    Nx, Ny, Nz = size_of(grid_type)
    H = 8
    u, v, w = (np.abs(b.get_field(n, False).astype(np.float64))[:Nx, :Ny, :Nz] for n in ("u", "v", "w"))
    dz = np.array([b.metric("dzf", k) for k in range(1, Nz + 1)])
    if grid_type == 0:
        dx = np.array([b.metric("dxc", j) for j in range(1, Ny + 1)])[None, :, None]
        dy = b.metric("dy")
    else:
        dx = b.metric2("dxfc")[H:H + Nx, H:H + Ny, None]
        dy = b.metric2("dycf")[H:H + Nx, H:H + Ny, None]
    cfl = (u / dx + v / dy) + w / dz[None, None, :]
    want = memory_order(cfl)
    mon = b.state_monitor()
    print(f"  cfl device {mon.cfl!r} numpy {want.max()!r} at {tuple(mon.at_cfl)}")
    assert want.max() > 0 and abs(mon.cfl - want.max()) <= 8 * EPS * want.max()
    assert tuple(mon.at_cfl) == position(int(np.argmax(want)), cfl.shape)
    for name in ("u", "v", "w", "eta", "T", "S"):
        assert getattr(mon, name).as_dict() == b.field_stats(name).as_dict(), name
    t, it, _ = b.clock()
    assert (mon.time, mon.iteration) == (t, it) and str(gb.state_monitor(m)) == str(mon)
    b.close()


@pytest.mark.parametrize("P,Ry", [(2, 1), (4, 1), (4, 2)])
def test_combined_ranks_equal_the_single_domain(P, Ry):
    Nx, Ny, Nz, dt = 128, 48 * Ry, 8, 600.0
    exact = dict(w_on_the_fly=0)
    single = gb.baroclinic_instability_model(gb.GPU(), Nx, Ny, Nz, dt=dt)
    gb.set_baroclinic_instability(single)
    u0 = (1e-2 * counter_rng((Nx, Ny, Nz), 42, 1)).astype(np.float32)
    v0 = (1e-2 * counter_rng((Nx, Ny + 1, Nz), 42, 2)).astype(np.float32)
    e0 = (1e-2 * counter_rng((Nx, Ny, 1), 42, 3)).astype(np.float32)
    single.set(u=u0, v=v0, eta=e0)
    init = {n: single.backend.get_field(n, False) for n in ("u", "v", "T", "S", "eta")}
    ens = LocalSlabEnsemble(Nx, Ny, Nz, P, dt=dt, ranks_y=Ry, slab_mode=1, options=exact)
    for n, a in init.items():
        ens.scatter(n, a)
    gb.first_time_step(single)
    ens.first_time_step()
    gb.loop(single, 4)
    ens.loop(4)
    for name in ("u", "T", "eta", "v"):
        assert np.array_equal(ens.gather(name), single.backend.get_field(name, False)), name     # (the premise)
        c, s = ens.field_stats(name), single.backend.field_stats(name)
        print(f"  {name}: combined max_abs {c.max_abs!r} at {tuple(c.at_max_abs)}; single at {tuple(s.at_max_abs)}")
        assert (c.min, c.max, c.max_abs, c.count, c.nonfinite) == (s.min, s.max, s.max_abs, s.count, s.nonfinite), name
        assert tuple(c.at_max_abs) == tuple(s.at_max_abs) and tuple(c.first_nonfinite) == (0, 0, 0), name
        x = memory_order(single.backend.get_field(name, False))
        assert_sum(c.sum, x, name + " combined sum")
        assert_sum(c.sum_sq, x * x, name + " combined sum_sq")
    cm, sm = ens.state_monitor(), single.backend.state_monitor()
    assert cm.cfl == sm.cfl and tuple(cm.at_cfl) == tuple(sm.at_cfl) and cm.iteration == sm.iteration
    # a value planted in one rank shows up at its global place, and a tie across ranks goes to the smaller global offset
    T = single.backend.get_field("T", False).copy()
    T[5, 3, 2] = T[Nx - 2, 3, 2] = 99.0
    T[Nx // 2 + 1, Ny - 1, 0] = np.nan
    single.backend.set_field("T", T, False)
    ens.scatter("T", T)
    c, s = ens.field_stats("T"), single.backend.field_stats("T")
    assert tuple(c.at_max_abs) == tuple(s.at_max_abs) == (6, 4, 3) and c.max_abs == 99.0
    assert c.nonfinite == 1 and tuple(c.first_nonfinite) == tuple(s.first_nonfinite) == (Nx // 2 + 2, Ny, 1)
    ens.close()
    single.backend.close()


def test_state_monitor_at_full_size():
    """1440 x 720 x 48 Float32: rows of 1440 + 16 elements, 34560 rows per field."""
    Nx, Ny, Nz = 1440, 720, 48
    m = gb.baroclinic_instability_model(gb.GPU(), Nx, Ny, Nz, dt=120.0)
    gb.set_baroclinic_instability(m)
    set_noisy_velocities(m, amplitude=1e-2)
    gb.first_time_step(m)
    gb.loop(m, 3)
    b = m.backend
    mon = b.state_monitor()
    fields = {}
    for name in ("u", "v", "w", "eta", "T", "S"):
        fields[name] = b.get_field(name, False)
        check_stats(getattr(mon, name), fields[name], name)
    check_stats(b.field_stats("T", True), b.get_field("T", True), "parent of T")
    dx = np.array([b.metric("dxc", j) for j in range(1, Ny + 1)])[None, :, None]
    dz = np.array([b.metric("dzf", k) for k in range(1, Nz + 1)])[None, None, :]
    u, v, w = (np.abs(fields[n].astype(np.float64))[:Nx, :Ny, :Nz] for n in ("u", "v", "w"))
    want = memory_order((u / dx + v / b.metric("dy")) + w / dz)
    assert abs(mon.cfl - want.max()) <= 8 * EPS * want.max() and tuple(mon.at_cfl) == position(int(np.argmax(want)), (Nx, Ny, Nz))
    assert mon.nonfinite_total == 0 and mon.iteration == 4
    b.close()
