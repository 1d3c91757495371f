"""Zonal-mean and eddy statistics, the parts that need no GPU: the numpy restatement of gb-25_amd/eddies.py (it is what the device
records are compared with bit for bit in tests/test_gpu_zonal_eddy.py, so it is pinned here independently of the HIP kernel)
against a plain triple-loop statement of include/gb25.h on Python floats -- the six centred variables, the measure, the counting
rule, the two passes and the ORDER of every sum: chunks of four aligned in the parent array of T, 64 lanes, the pairwise tree --,
a zonally uniform state, a planted wave with a known covariance, the Lorenz cycle on synthetic records, the combination of the
ranks' records, and the new ABI entries on a handle without a device.

The zonally uniform state.  co is exactly +0.0 when the mean of a constant line IS the constant.  In fp64 that holds when the
constant is a power of two: mu c is then exact, every partial sum of the mu c is c times the same partial sum of the mu, and the one
division returns c.  For another constant first / measure may differ from c in the last bit and co is of the order of that bit
squared, not 0: the test therefore plants powers of two (a different one per line and variable)."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest

import gb25_amd as gb
from gb25_amd import binding
from gb25_amd.binding import ZONAL_EDDY_DTYPE
from gb25_amd.eddies import (PAIRS, VARIABLES, ZonalEddy, co_index, combine_zonal_eddy, line_misalignment, line_sums,
                             lorenz_cycle_of_records, single_domain_measure, zonal_eddy_host)
from helpers import GRID_NAMES, make_oracle, set_noisy_state_with_halos

SIZES = {0: (18, 10, 4), 1: (48, 24, 6), 3: (48, 24, 6)}
FOLDED = (3, 4)
LAT_LON = (0, 1)
MEMBERS = ZONAL_EDDY_DTYPE.names


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


@functools.lru_cache(maxsize=None)
def noisy_oracle(grid_type, size=None):
    """The baroclinic-instability state with noisy velocities and noise on every cell of the parents, halos included; w = noise too."""
    Nx, Ny, Nz = size or SIZES[grid_type]
    m = make_oracle(Nx, Ny, Nz, 600.0, grid_type=GRID_NAMES[grid_type])
    set_noisy_state_with_halos(m, amplitude=0.05)
    b = m.backend
    w = b.get_field("w", True)
    from helpers import counter_rng
    b.set_field("w", (1e-4 * (counter_rng(w.shape, 11, 1) - 0.5)).astype(b.dtype), True)
    return m


def stand_in_density(b):
    """An oracle backend has no get_derived: a potential density that is linear in T and S, rounded to the backend's dtype."""
    T, S = (np.asarray(b.get_field(n, False), np.float64) for n in ("T", "S"))
    return (28.0 - 0.2 * T + 0.8 * (S - 35.0)).astype(b.dtype)


def lane_sum(terms, a):
    """The sum of the floats `terms` (one per cell of a line, ascending i; None: the cell adds nothing) in the header's order."""
    lanes = [0.0] * 64
    for x, t in enumerate(terms):
        if t is not None:
            lane = ((x + a) // 4) % 64
            lanes[lane] = lanes[lane] + t
    while len(lanes) > 1:
        lanes = [lanes[n] + lanes[n + 1] for n in range(0, len(lanes), 2)]
    return lanes[0]


def records_by_loops(b, sigma, levels=None, means=None):
    """include/gb25.h, one cell at a time on Python floats."""
    Nx, Ny, Nz = b.field_dims("T", False)
    sx, sy, _ = b.field_dims("T", True)
    H = (sx - Nx) // 2
    k0, kc = (0, Nz) if levels is None else levels
    f = {n: np.asarray(b.get_field(n, True), np.float64) for n in ("u", "v", "w", "T", "S")}
    at = lambda n, i, j, k: float(f[n][H + i, H + j, H + k])
    latlon = b.cfg.grid_type in LAT_LON
    out = np.zeros((Ny, kc), ZONAL_EDDY_DTYPE)
    for kk in range(kc):
        k = k0 + kk
        dz = float(b.metric("dzc", k + 1))
        for j in range(Ny):
            a = (H + sx * ((j + H) + sy * (k + H))) % 4
            fold = 0.5 if (b.cfg.grid_type in FOLDED and j == Ny - 1) else 1.0
            cells, points, skipped = [], 0, 0
            for i in range(Nx):
                area = float(b.metric("azc", j + 1)) if latlon else float(b.metric2("azcc", i + 1, j + 1))
                mu = (area * dz) * fold if k >= int(b.bottom_info("kbot", i + 1, j + 1)) else 0.0
                x = (0.5 * (at("u", i, j, k) + at("u", i + 1, j, k)), 0.5 * (at("v", i, j, k) + at("v", i, j + 1, k)),
                     0.5 * (at("w", i, j, k) + at("w", i, j, k + 1)), at("T", i, j, k), at("S", i, j, k), float(sigma[i, j, k]))
                if not mu > 0.0:
                    cells.append(None)
                elif all(math.isfinite(q) for q in x):
                    cells.append((mu, x))
                    points += 1
                else:
                    cells.append(None)
                    skipped += 1
            measure = lane_sum([None if c is None else c[0] for c in cells], a)
            first = [lane_sum([None if c is None else c[0] * c[1][q] for c in cells], a) for q in range(6)]
            if means is not None:
                mean = [float(means[j, kk, q]) for q in range(6)]
            else:
                mean = [0.0 if measure == 0.0 else first[q] / measure for q in range(6)]
            co = []
            for p, q in PAIRS:
                co.append(lane_sum([None if c is None else (c[0] * (c[1][p] - mean[p])) * (c[1][q] - mean[q]) for c in cells], a))
            out[j, kk] = (measure, first, mean, co, points, skipped)
    return out


@pytest.mark.parametrize("grid_type", [0, 1, 3])
def test_the_restatement_equals_the_triple_loop(grid_type):
    b = noisy_oracle(grid_type).backend
    Nx, Ny, Nz = SIZES[grid_type]
    sigma = stand_in_density(b)
    got = zonal_eddy_host(b, sigma=sigma)
    want = records_by_loops(b, sigma)
    assert got.shape == (Ny, Nz) and got.dtype == ZONAL_EDDY_DTYPE
    for f in MEMBERS:
        assert same(got[f], want[f]), f
    assert (got["co"] != 0).all(axis=(0, 1)).all() or grid_type != 0, "noise on every variable: no comoment is 0"
    assert (got["points"] > 0).any() and got["nonfinite"].sum() == 0
    if grid_type == 0:
        assert len(set(line_misalignment(b).ravel().tolist())) > 1, "rows of 18 + 16 elements: more than one alignment"
        assert (got["points"] == Nx).all()
    if grid_type == 1:
        assert (got["points"] < Nx).any(), "the islands take cells out of some lines"
    if grid_type == 3:       # the pivot row weighs 1/2
        k = Nz - 1
        full = sum(float(b.metric2("azcc", i + 1, Ny)) * float(b.metric("dzc", k + 1)) for i in range(Nx)
                   if k >= int(b.bottom_info("kbot", i + 1, Ny)))
        assert got["measure"][Ny - 1, k] == pytest.approx(0.5 * full, rel=1e-13)
    # a window of levels is that slice; means given: echoed, and the comoments are those about them
    part = zonal_eddy_host(b, levels=(1, 2), sigma=sigma)
    for f in MEMBERS:
        assert same(part[f], got[f][:, 1:3]), f
    shifted = got["mean"][:, 1:3] + np.array([1e-3, -2e-3, 1e-5, 0.25, -0.125, 0.5])
    about = zonal_eddy_host(b, levels=(1, 2), means=shifted, sigma=sigma)
    loops = records_by_loops(b, sigma, (1, 2), shifted)
    for f in MEMBERS:
        assert same(about[f], loops[f]), f
    assert same(about["mean"], shifted) and same(about["first"], part["first"]) and not same(about["co"], part["co"])
    own = zonal_eddy_host(b, levels=(1, 2), means=part["mean"], sigma=sigma)
    for f in MEMBERS:
        assert same(own[f], part[f]), f


def test_a_line_longer_than_256_cells_and_a_planted_nan():
    """More than 64 chunks: a lane takes a second one.  A NaN in T skips its cell; one in a face of u the two cells it touches."""
    Nx, Ny, Nz = 302, 8, 4
    m = noisy_oracle(0, (Nx, Ny, Nz))
    b = m.backend
    sigma = stand_in_density(b)
    got = zonal_eddy_host(b, sigma=sigma)
    want = records_by_loops(b, sigma)
    for f in MEMBERS:
        assert same(got[f], want[f]), f
    # line_sums against the scalar statement, every alignment, lengths around the chunk and the round
    rng = np.random.default_rng(5)
    for n in (1, 3, 4, 5, 37, 255, 256, 257, 300, 513):
        for a in range(4):
            t = rng.standard_normal((n, 2))
            assert line_sums(t, a)[0] == lane_sum(list(t[:, 0]), a) and line_sums(t, a)[1] == lane_sum(list(t[:, 1]), a), (n, a)
    T, u = b.get_field("T", True), b.get_field("u", True)
    H = (T.shape[0] - Nx) // 2
    T[H + 7, H + 2, H + 1] = np.nan
    u[H + 280, H + 4, H + 2] = np.nan
    try:
        b.set_field("T", T, True)
        b.set_field("u", u, True)
        sigma2 = stand_in_density(b)
        nan = zonal_eddy_host(b, sigma=sigma2)
        loops = records_by_loops(b, sigma2)
        for f in MEMBERS:
            assert same(nan[f], loops[f]), f
        skipped = np.zeros((Ny, Nz), np.int64)
        skipped[2, 1], skipped[4, 2] = 1, 2
        assert np.array_equal(nan["nonfinite"], skipped) and np.array_equal(nan["points"], Nx - skipped)
        untouched = skipped == 0
        for f in MEMBERS:
            assert same(nan[f][untouched], got[f][untouched]), f
        assert np.isfinite(nan["co"]).all() and np.isfinite(nan["first"]).all()
    finally:
        noisy_oracle.cache_clear()


def test_a_zonally_uniform_state_has_no_eddies():
    Nx, Ny, Nz = SIZES[0]
    m = make_oracle(Nx, Ny, Nz, 600.0, grid_type=GRID_NAMES[0])
    b = m.backend
    shape = b.field_dims("T", True)
    j, k = np.meshgrid(np.arange(shape[1] + 1), np.arange(shape[2] + 1), indexing="ij")
    for n, (name, sign, e) in enumerate((("u", -1.0, -6), ("v", 1.0, -7), ("w", -1.0, -12), ("T", 1.0, 2), ("S", 1.0, 4))):
        d = b.field_dims(name, True)
        # a power of two per line; v the same in every row and w at every level, so that their centred means are powers of two too
        vary = 2 * k if name == "v" else j if name == "w" else j + 2 * k
        line = sign * np.exp2(e + (vary + n) % 3)[: d[1], : d[2]]
        b.set_field(name, np.broadcast_to(line[None], d).astype(b.dtype), True)
    jj, kk = np.meshgrid(np.arange(Ny), np.arange(Nz), indexing="ij")
    sigma = np.broadcast_to(np.exp2(4 + (jj + kk) % 2)[None], (Nx, Ny, Nz)).astype(b.dtype)
    r = zonal_eddy_host(b, sigma=sigma)
    assert same(r["co"], np.zeros((Ny, Nz, 21))), "every comoment is +0.0, sign included"
    assert (r["points"] == Nx).all() and (r["mean"][..., 3] >= 4).all() and (r["mean"][..., 0] < 0).all()
    assert np.array_equal(r["mean"][..., 5], np.exp2(4 + (jj + kk) % 2))
    ze = ZonalEddy(r)
    assert not ze.eddy_kinetic_energy().any() and not ze.eddy_flux("VT").any()


@pytest.mark.parametrize("Nx,wave,phase", [(18, 2, 0.0), (18, 3, 1.0), (48, 5, 2.5), (302, 7, math.pi / 2)])
def test_a_planted_wave_has_the_covariance_of_its_amplitudes(Nx, wave, phase):
    """U* = a cos(m lambda), V* = b cos(m lambda + phi) on flat lines: [U*V*] = a b cos(phi) / 2, within the rounding of the sum --
    (Nx + 64) 2^-53 times the same sum over absolute values."""
    Ny, Nz = 8, 4
    a, c = 0.3, 0.2
    m = make_oracle(Nx, Ny, Nz, 600.0, grid_type=GRID_NAMES[0])
    b = m.backend
    d = b.field_dims("T", True)
    H = (d[0] - Nx) // 2
    lam = 2.0 * math.pi * (np.arange(d[0]) - H) / Nx                       # cell centres of the parent's columns, periodic
    half = math.pi * wave / Nx                                            # m dlambda / 2
    u = 1.5 + a * np.cos(wave * (lam - math.pi / Nx)) / math.cos(half)    # faces: 0.5 (u(i) + u(i+1)) = 1.5 + a cos(m lambda_i)
    v = -0.5 + c * np.cos(wave * lam + phase)
    for name, line in (("u", u), ("v", v)):
        dd = b.field_dims(name, True)
        b.set_field(name, np.broadcast_to(line[:, None, None], dd).astype(b.dtype), True)
    r = zonal_eddy_host(b, sigma=np.zeros((Nx, Ny, Nz), b.dtype))
    ze = ZonalEddy(r)
    got = ze.covariance("U", "V")
    mu = np.array([[b.metric("azc", j + 1) * b.metric("dzc", k + 1) for k in range(Nz)] for j in range(Ny)])
    dU, dV = a * np.cos(wave * lam[H:H + Nx]), c * np.cos(wave * lam[H:H + Nx] + phase)
    absolute = mu * np.abs(dU * dV).sum()                                   # sum mu |d_p d_q| of a line
    bound = (Nx + 64) * 2.0 ** -53 * absolute / r["measure"]
    want = 0.5 * a * c * math.cos(phase)
    print(f"  Nx {Nx} m {wave} phi {phase:.3g}: [U*V*] {got[0, 0]:.17g} want {want:.17g}, max error {np.abs(got - want).max():.3g}, bound {bound.min():.3g}")
    assert (np.abs(got - want) <= bound).all()
    assert np.abs(ze.mean("U") - 1.5).max() < 1e-14 and np.abs(ze.mean("V") + 0.5).max() < 1e-14
    assert np.abs(ze.eddy_kinetic_energy() - 0.25 * (a * a + c * c)).max() <= 2 * (Nx + 64) * 2.0 ** -53
    assert same(ze.eddy_flux("UV"), got) and same(ze.covariance("V", "U"), got)


def synthetic_records(Ny, Nz, co=None):
    r = np.zeros((Ny, Nz), ZONAL_EDDY_DTYPE)
    y = np.linspace(-1.0, 1.0, Ny)[:, None]
    z = np.linspace(-1.0, 0.0, Nz)[None, :]
    r["measure"] = 2.0e9 * (1.0 + 0.1 * y * y) * np.ones((1, Nz))
    mean = np.zeros((Ny, Nz, 6))
    mean[..., 0] = 0.1 * (1.0 - y * y) * (1.0 + z)            # a jet
    mean[..., 5] = 27.0 - 2.0 * z + 0.5 * y                    # light above heavy, heavier to the north
    r["mean"] = mean
    r["first"] = mean * r["measure"][..., None]
    r["points"] = 10
    for pair, value in (co or {}).items():
        r["co"][..., co_index(*pair)] = value * r["measure"]
    return r


def test_the_lorenz_cycle_on_synthetic_records():
    Ny, Nz = 9, 5
    zc, y = np.linspace(-900.0, -100.0, Nz), np.linspace(-2.0e6, 2.0e6, Ny)
    gr = 9.80665 / 1020.0
    quiet = lorenz_cycle_of_records(synthetic_records(Ny, Nz), zc, y, gr)
    for n in ("K_E", "P_E", "C_PM_PE", "C_PE_KE", "C_KE_KM"):
        assert quiet["total"][n] == 0.0 and not quiet[n].any(), n
    assert quiet["total"]["K_M"] > 0 and quiet["total"]["P_M"] > 0 and (quiet["N2"] > 0).all()
    assert quiet["K_M"].shape == (Ny, Nz)
    # a known [W* sigma*]: C(P_E -> K_E) = sum mu [W* b*] = -(g / rho0) sum mu [W* sigma*]
    wb = -3.0e-9
    r = synthetic_records(Ny, Nz, {("W", "SIGMA"): wb})
    c = lorenz_cycle_of_records(r, zc, y, gr)
    assert c["total"]["C_PE_KE"] == pytest.approx(-gr * wb * r["measure"].sum(), rel=1e-14)
    assert np.allclose(c["C_PE_KE"], -gr * wb * r["measure"], rtol=1e-14) and c["total"]["C_KE_KM"] == 0.0
    # the others, from their formulas
    r = synthetic_records(Ny, Nz, {("U", "U"): 4e-4, ("V", "V"): 2e-4, ("U", "V"): 1e-4, ("V", "SIGMA"): -2e-5, ("SIGMA", "SIGMA"): 1e-4})
    c = lorenz_cycle_of_records(ZonalEddy(r), zc, y, gr)
    assert c["total"]["K_E"] == pytest.approx(0.5 * 6e-4 * r["measure"].sum(), rel=1e-14)
    N2 = np.gradient(-gr * (27.0 - 2.0 * np.linspace(-1.0, 0.0, Nz) + 0.0), zc)
    assert np.allclose(c["N2"], N2, rtol=1e-9)
    assert np.allclose(c["P_E"], 0.5 * r["measure"] * gr * gr * 1e-4 / c["N2"][None, :], rtol=1e-13)
    # d[b]/dy = -(g / rho0) 0.5 per unit of the scaled y, which is 2e6 m
    assert np.allclose(c["C_PM_PE"], -r["measure"] * (-gr * -2e-5) * (-gr * 0.5 / 2.0e6) / c["N2"][None, :], rtol=1e-9)
    assert c["total"]["C_KE_KM"] != 0.0
    with pytest.raises(ValueError):
        lorenz_cycle_of_records(synthetic_records(Ny, 1), zc[:1], y, gr)


def test_lorenz_cycle_of_a_model_and_its_refusal():
    m = noisy_oracle(0)
    sigma = stand_in_density(m.backend)
    c = gb.lorenz_cycle(m, sigma=sigma)
    Nx, Ny, Nz = SIZES[0]
    assert c["K_E"].shape == (Ny, Nz) and all(math.isfinite(v) for v in c["total"].values()) and c["total"]["K_E"] > 0
    ze = gb.zonal_eddy(m, sigma=sigma)
    assert c["total"]["K_E"] == pytest.approx(0.5 * (ze.records["co"][..., 0] + ze.records["co"][..., co_index("V", "V")]).sum(), rel=1e-13)
    with pytest.raises(ValueError, match="2-D metrics"):
        gb.lorenz_cycle(noisy_oracle(3), sigma=stand_in_density(noisy_oracle(3).backend))


def test_the_public_function_falls_back_to_the_restatement_and_the_ranks_combine():
    m = noisy_oracle(1)
    b = m.backend
    sigma = stand_in_density(b)
    want = zonal_eddy_host(b, sigma=sigma)
    ze = gb.zonal_eddy(m, sigma=sigma)
    assert isinstance(ze, ZonalEddy) and all(same(ze.records[f], want[f]) for f in MEMBERS)
    assert same(ze.mean("T"), want["mean"][..., 3]) and same(gb.zonal_eddy(m, levels=(2, 1), sigma=sigma).records["co"], want["co"][:, 2:3])
    cov = ze.covariance("V", "T")
    wet = want["measure"] > 0
    assert same(cov[wet], (want["co"][..., co_index("T", "V")] / want["measure"])[wet]) and not cov[~wet].any()
    for bad in (lambda: ze.mean("Q"), lambda: ze.eddy_flux("VQ"), lambda: zonal_eddy_host(b, levels=(0, 0), sigma=sigma),
                lambda: zonal_eddy_host(b, means=np.full(want["mean"].shape, np.nan), sigma=sigma),
                lambda: zonal_eddy_host(b, means=np.zeros((2, 2, 6)), sigma=sigma)):
        with pytest.raises(ValueError):
            bad()
    # two ranks with the same rows add member by member and divide once; other rows are stacked
    half = want.copy()
    for f in ("measure", "first", "co"):
        half[f] = 0.5 * want[f]
    both = combine_zonal_eddy([half, half], [0, 0])
    for f in ("measure", "first", "co"):
        assert same(both[f], want[f]), f
    assert np.array_equal(both["points"], 2 * want["points"])
    assert same(both["mean"][wet], (want["first"] / np.where(wet, want["measure"], 1.0)[..., None])[wet]) and not both["mean"][~wet].any()
    # the measure of the whole line in the order of one domain, from the cells' static measure: the restatement's own, bit for bit,
    # on every grid type; handed to the combination it replaces the ranks' sum on the lines without a skipped cell
    from gb25_amd.integrals import cell_measure
    for gt in (0, 1, 3):
        bb = noisy_oracle(gt).backend
        whole = single_domain_measure(cell_measure(bb, "T"), bb.H)
        assert same(whole, zonal_eddy_host(bb, sigma=stand_in_density(bb))["measure"]), gt
        assert same(single_domain_measure(cell_measure(bb, "T"), bb.H, (1, 2)), whole[:, 1:3]), gt
    whole = single_domain_measure(cell_measure(b, "T"), b.H)
    off = half.copy()
    off["measure"] = half["measure"] * (1.0 + 2.0 ** -52)
    off["nonfinite"][3, 2] = 1
    fixed = combine_zonal_eddy([off, half], [0, 0], whole)
    kept = np.zeros(want.shape, bool)
    kept[3, 2] = True
    assert same(fixed["measure"][~kept], want["measure"][~kept]) and fixed["measure"][3, 2] == off["measure"][3, 2] + half["measure"][3, 2]
    assert same(fixed["mean"][wet], (fixed["first"] / np.where(wet, fixed["measure"], 1.0)[..., None])[wet])
    stacked = combine_zonal_eddy([want[:10], want[10:]], [0, 10])
    assert all(same(stacked[f], want[f]) for f in ("measure", "first", "co", "points", "nonfinite"))


def test_the_abi_on_a_handle_without_a_device():
    import torch
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "gb25.h")).read()
    lib = binding.load_library("Float32")
    for symbol in ("gb25_get_zonal_eddy", "gb25_zonal_eddy_dims", "gb25_zonal_eddy_bytes"):
        assert symbol in text and hasattr(lib, symbol) and symbol in binding.ABI_SYMBOLS, symbol
    assert "zonal-mean and eddy statistics on the device" in text
    assert lib.gb25_zonal_eddy_bytes() == C.sizeof(binding.ZonalEddyRow) == ZONAL_EDDY_DTYPE.itemsize == 8 * 36
    assert tuple(binding.ZONAL_EDDY_VARIABLES) == VARIABLES and len(PAIRS) == 21
    assert [co_index(p, q) for p, q in PAIRS] == list(range(21)) and co_index("SIGMA", "U") == 5
    INVALID, NO_DEVICE = 1, 4
    Nx, Ny, Nz = 48, 24, 6
    cfg = binding.Config()
    lib.gb25_default_config(C.byref(cfg), Nx, Ny, Nz)
    h = C.c_void_p()
    st = lib.gb25_create(C.byref(cfg), C.byref(h))
    assert h and st == (0 if torch.cuda.is_available() else NO_DEVICE)
    d = (C.c_int32 * 2)()
    assert lib.gb25_zonal_eddy_dims(h, d) == 0 and tuple(d) == (Ny, Nz)
    assert lib.gb25_zonal_eddy_dims(h, None) == INVALID and lib.gb25_zonal_eddy_dims(None, d) == INVALID
    out = np.zeros((Nz, Ny), ZONAL_EDDY_DTYPE)
    po = out.ctypes.data_as(C.c_void_p)
    means = np.zeros((Nz, Ny, 6))
    means[2, 3, 4] = np.inf
    bad = [(lambda: lib.gb25_get_zonal_eddy(h, 0, -1, None, None), b"out is NULL"),
           (lambda: lib.gb25_get_zonal_eddy(h, 0, 0, None, po), b"window"),
           (lambda: lib.gb25_get_zonal_eddy(h, Nz, 1, None, po), b"window"),
           (lambda: lib.gb25_get_zonal_eddy(h, Nz - 1, 2, None, po), b"window"),
           (lambda: lib.gb25_get_zonal_eddy(h, -1, 1, None, po), b"window"),
           (lambda: lib.gb25_get_zonal_eddy(h, 0, -1, means.ctypes.data_as(C.c_void_p), po), b"means must be finite")]
    for n, (call, word) in enumerate(bad):
        assert call() == INVALID, n
        assert word in lib.gb25_last_error_string(h), (n, lib.gb25_last_error_string(h))
    assert b"variable 4 of row 3 of level 2" in lib.gb25_last_error_string(h)
    assert lib.gb25_get_zonal_eddy(None, 0, -1, None, po) == INVALID
    if not torch.cuda.is_available():
        means[2, 3, 4] = 0.0
        for call in (lambda: lib.gb25_get_zonal_eddy(h, 0, -1, None, po), lambda: lib.gb25_get_zonal_eddy(h, 1, 2, means.ctypes.data_as(C.c_void_p), po)):
            assert call() == NO_DEVICE and b"no device" in lib.gb25_last_error_string(h)
    assert not out["points"].any()
    lib.gb25_destroy(h)
    for name in ("zonal_eddy", "zonal_eddy_host", "combine_zonal_eddy", "lorenz_cycle", "lorenz_cycle_of_records"):
        assert callable(getattr(gb, name)), name
    from gb25_amd.distributed import LocalSlabEnsemble
    assert callable(LocalSlabEnsemble.zonal_eddy) and callable(binding.HipBackend.zonal_eddy) and callable(binding.HipBackend.zonal_eddy_dims)
