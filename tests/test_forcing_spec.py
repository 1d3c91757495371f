"""tests/forcing_spec.py proved on the CPU oracle before tests/test_gpu_forcing_spec.py judges the device by it, and the inputs both
use: the "regime atlas", an atmosphere made so that every branch of the flux solve is taken where kernels go wrong.

The atlas (atlas(); a deterministic function of the parent cell through helpers.counter_rng, so a halo cell carries values of its
own, not a periodic image): patches of 2 x 2 cells of four kinds, kind = ((i + 1) // 2 + (j + 1) // 2) mod 4 of the logical
cell (i, j) --
    0  calm, cold air    |du|, |dv| <= 0.03 m/s about the ocean's own velocity, T_a - T_s in [-12, -2] K, q_a in [0, 0.01]
    1  calm, warm air    the same winds, T_a - T_s in [+2, +12] K, q_a in [0.01, 0.02]
    2  driven, cold air  3 .. 20 m/s from any direction, T_a - T_s in [-12, -2] K, q_a in [0, 0.02]
    3  driven, warm air  the same winds, T_a - T_s in [+2, +12] K
with p_a in [98 000, 103 000] Pa, Q_lw in [0, 450], Q_sw in [0, 900] W/m2 everywhere.  With a period of 8 cells along i and along j
every kind falls on the west halo column, the south halo row, columns 63 and 64, the last block of every shape and beside the land
of the immersed grids (test_the_atlas_covers_every_regime asserts it).  The ocean is set_baroclinic_instability +
set_noisy_velocities(0.2) with the surface T shifted by +-3 K in blocks of 4 x 4 cells: calm patches over warm and over cold water.

Folded grids are refused below Ny = 2 halo rows and below the image rows of their sub-cycle: the shapes' Ny is raised to 24 there,
the smallest this suite is known to create (tests/test_catke_spec.py)."""
import functools

import numpy as np
import pytest

import gb25_amd as gb
import forcing_spec as fs
import step_spec as ss
from helpers import counter_rng, set_noisy_velocities
from oracle_backend import CPU

DT = 300.0
CD = 0.003
GRIDS = ("simple_lat_lon", "gaussian_islands_lat_lon", "lat_lon_as_curvilinear", "gaussian_islands")
SHAPES = ((64, 8, 6), (70, 13, 6), (130, 9, 6))
CASES = [(grid, shape) for grid in GRIDS for shape in SHAPES]
FLUXES = ("u", "v", "T", "S")
FLUX_SCALE = dict(T=1e-4, S=2e-5, u=1e-4, v=2e-5)       # the magnitudes of tests/test_gpu_fluxes.py::fluxes


def shape_on(grid, shape):
    Nx, Ny, Nz = shape
    return (Nx, max(Ny, 24), Nz) if grid in ss.FOLDED else shape


def made_levels(kbot, Nz):
    """The islands' own dry levels with land made on top (the islands of grids this small hardly reach the surface): a block of
    4 x 3 columns across columns 62 .. 65 with half-raised columns west and south of it, two land cells in the last column (their
    periodic images lie in the west halo column) and a 2 x 2 block next to the southern wall."""
    Nx, Ny = kbot.shape
    level = kbot.copy()
    i0 = min(62, Nx - 6)
    level[i0 - 2:i0, 2:5] = np.maximum(level[i0 - 2:i0, 2:5], Nz // 3)
    level[i0:i0 + 4, 1] = np.maximum(level[i0:i0 + 4, 1], (2 * Nz) // 3)
    level[i0:i0 + 4, 2:5] = Nz
    level[Nx - 1, 5:7] = Nz
    level[10:12, 0:2] = Nz
    return level


def raise_land(b, shape):
    Nx, Ny, Nz = shape
    kbot = np.array([[b.bottom_info("kbot", i + 1, j + 1) for j in range(Ny)] for i in range(Nx)]).astype(int)
    zf = np.array([b.metric("zf", k) for k in range(1, Nz + 2)])
    zc = np.array([b.metric("zc", k) for k in range(1, Nz + 1)])
    level = made_levels(kbot, Nz)
    # the bottom between the centre of the highest dry cell and its top face
    b.set_bottom_height(np.where(level > 0, 0.5 * (zc[np.maximum(level, 1) - 1] + zf[level]), -1e4))
    got = np.array([[b.bottom_info("kbot", i + 1, j + 1) for j in range(Ny)] for i in range(Nx)]).astype(int)
    assert np.array_equal(got, level), "the bottom is not the one this test made"


def build(arch, grid, shape, **options):
    """(model, geometry): geometry is step_spec.read_geometry's with the build's g and rho0."""
    shape = shape_on(grid, shape)
    m = gb.baroclinic_instability_model(arch, *shape, dt=DT, grid_type=grid, **(dict(options=options) if options else {}))
    b = m.backend
    if "islands" in grid:
        raise_land(b, shape)
    g = ss.read_geometry(b, grid, shape, b.H if hasattr(b, "H") else b.cfg.halo)
    g["grav"], g["rho0"] = float(b.dtype(b.cfg.g)), float(b.dtype(b.cfg.rho0))
    return m, g


def logical(g):
    H = g["H"]
    return np.meshgrid(np.arange(g["Nx"] + 2 * H) - H, np.arange(g["Ny"] + 2 * H) - H, indexing="ij")


def kinds(g):
    i, j = logical(g)
    return ((i + 1) // 2 + (j + 1) // 2) % 4


def set_ocean(m, g, amplitude=0.2):
    """The ocean of the module docstring, then update_state (masks, halos); returns the parent arrays of u, v, T, S."""
    b, H, Nz = m.backend, g["H"], g["Nz"]
    gb.set_baroclinic_instability(m)
    set_noisy_velocities(m, amplitude)
    i, j = logical(g)
    T = b.get_field("T", True)
    T[:, :, H + Nz - 1] += np.where(((i + 1) // 4 + (j + 1) // 4) % 2 == 0, 3.0, -3.0).astype(b.dtype)
    b.set_field("T", T, True)
    gb.update_state(m)
    return {n: b.get_field(n, True) for n in ("u", "v", "T", "S")}


def other_halos(m, g, ocean, seed):
    """Other values in the halo cells of u, v, T, S west of column 0 and south of row 0 (noise of the fields' own size): the ones
    the extra column and row of the flux solve read.  (The east halo column of u and the row of v beyond the last row of cells belong
    to the centre averages of the interior's last column and row.)"""
    b, H = m.backend, g["H"]
    for q, (n, amp) in enumerate((("u", 0.2), ("v", 0.2), ("T", 2.0), ("S", 0.5))):
        a = ocean[n]
        inner = np.zeros(a.shape, bool)
        inner[H:, H:] = True
        a = np.where(inner, a, a + (amp * (2 * counter_rng(a.shape, 950 + seed, q) - 1)).astype(a.dtype))
        b.set_field(n, a, True)
        ocean[n] = b.get_field(n, True)
    return ocean


def atlas(g, ocean, seed=0, halo_seed=None):
    """{name: parent (Nx + 2H, Ny + 2H) float64} for forcing_spec.ATMOSPHERE (module docstring), about the ocean as the model holds
    it.  halo_seed: other random numbers in the halo cells west of column 0 and south of row 0, every other cell as before."""
    H, Nx, Ny, Nz = g["H"], g["Nx"], g["Ny"], g["Nz"]
    shape = (Nx + 2 * H, Ny + 2 * H)
    inner = np.zeros(shape, bool)
    inner[H:, H:] = True

    def r(salt):
        a = counter_rng(shape, 900 + seed, salt)
        return a if halo_seed is None else np.where(inner, a, counter_rng(shape, 970 + halo_seed, salt))

    top = H + Nz - 1
    u, v = (np.asarray(ocean[n], np.float64)[:, :, top] for n in ("u", "v"))
    uo = (u + np.concatenate([u[1:], u[-1:]], axis=0)) / 2
    vo = ((v[:, :-1] + v[:, 1:]) / 2)[:, :shape[1]] if v.shape[1] > shape[1] else (v + np.concatenate([v[:, 1:], v[:, -1:]], axis=1)) / 2
    Ts = np.asarray(ocean["T"], np.float64)[:, :, top] + 273.15
    kind = kinds(g)
    calm, warm_air = kind < 2, kind % 2 == 1
    speed, angle = 3 + 17 * r(1), 2 * np.pi * r(2)
    out = dict(u=np.where(calm, uo + 0.03 * (2 * r(3) - 1), speed * np.cos(angle)),
               v=np.where(calm, vo + 0.03 * (2 * r(4) - 1), speed * np.sin(angle)),
               T=Ts + (2 + 10 * r(5)) * np.where(warm_air, 1.0, -1.0),
               q=np.where(calm, np.where(warm_air, 0.01 + 0.01 * r(6), 0.01 * r(6)), 0.02 * r(6)),
               p=98000 + 5000 * r(7), shortwave=900 * r(8), longwave=450 * r(9))
    return out


def set_atmosphere(m, atm):
    for n in fs.ATMOSPHERE:
        m.backend.set_prescribed_atmosphere(n, atm[n])


def solved(arch, grid, shape, halo_seed=None, **options):
    """(model, case): the atlas set about the updated ocean, compute_atmosphere_ocean_fluxes, the four top fluxes read in full.
    case: g, ocean, atm, got {name: top_flux(name)}."""
    m, g = build(arch, grid, shape, **options)
    ocean = set_ocean(m, g)
    if halo_seed is not None:
        ocean = other_halos(m, g, ocean, halo_seed)
    atm = atlas(g, ocean, halo_seed=halo_seed)
    set_atmosphere(m, atm)
    m.backend.compute_atmosphere_ocean_fluxes()
    return m, dict(g=g, ocean=ocean, atm=atm, got={n: np.array(m.backend.top_flux(n)) for n in FLUXES})


def statement(case, **kw):
    o = case["ocean"]
    return fs.top_fluxes(case["atm"], o["u"], o["v"], o["T"], o["S"], case["g"], **kw)


@functools.lru_cache(maxsize=None)
def oracle_case(precision, grid, shape):
    m, case = solved(CPU(precision), grid, shape)
    m.backend.close()
    case["want"], case["regimes"] = statement(case, south_row_is_land=True)
    return case


def yardstick(case):
    """{(field, regime): largest |loop float32 - loop float64| / max |float64|} of the statement on the inputs of `case`, the south
    row computed as the device has it: a property of the statement, not of any kernel."""
    want, regimes = statement(case)
    single, _ = statement(case, loop_dtype=np.float32)
    return {(n, r): d for n in FLUXES for r, d in fs.deviation_by_regime(single[n], want[n], fs.regimes_at(regimes, n, want[n].shape[1])).items()}


def exact_facts(label, case, got, want, regimes):
    """Both builds: land is exactly zero, faces between two land cells too, the unwritten row of J^v keeps its zero, all finite.
    That J^u next to land is the half-sum with a zero cannot be asked exactly: the stress at the centres has no getter.  It is
    asked through the statement (tau = 0 on land) at the tolerance of the field."""
    g = case["g"]
    land = regimes["land"]
    for n in FLUXES:
        assert np.isfinite(got[n]).all(), f"{label}: J^{n} is not finite"
    for n in ("T", "S"):
        ss.check_zero(f"{label}: J^{n} on land", got[n], land[1:, 1:])
    ss.check_zero(f"{label}: J^u between two land cells", got["u"], land[:-1, 1:] & land[1:, 1:])
    if not g["folded"]:
        assert got["v"].shape[1] == g["Ny"] + 1
        ss.check_zero(f"{label}: the row of J^v that is never written", got["v"][:, -1:], np.ones((g["Nx"], 1), bool))


# ---- the atlas reaches what it is made for ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid,shape", CASES)
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_the_atlas_covers_every_regime(precision, grid, shape):
    case = oracle_case(precision, grid, shape)
    g = case["g"]
    _, regimes = statement(case)                                     # (the south row computed: the device's view)
    halo = np.zeros(regimes["land"].shape, bool)
    halo[0, :] = halo[:, 0] = True
    for r in ("unstable", "stable", "clamped", "gust_floor", "lq_cap"):
        assert regimes[r].sum() >= 16, f"{grid} {shape} {precision}: {regimes[r].sum()} cells are {r}"
        assert (regimes[r] & halo).any(), f"{grid} {shape} {precision}: no cell of the halo column or row is {r}"
    if g["immersed"]:
        assert regimes["land"].sum() >= 16
    # every kind of patch on the west column, the south row, columns 63 | 64, the last block of 64 columns, and beside land
    H = g["H"]
    kind = kinds(g)[H - 1:H + g["Nx"], H - 1:H + g["Ny"]]
    i = np.arange(-1, g["Nx"])[:, None] + 0 * kind
    places = {"west halo column": i == -1, "south halo row": halo & (i >= 0), "columns 63 and 64": (i == 63) | (i == 64) if g["Nx"] > 64 else i == 63,
              "the last block": i >= 64 * ((g["Nx"]) // 64) if g["Nx"] % 64 else i >= g["Nx"] - 64}
    if g["immersed"]:
        land = regimes["land"]
        beside = np.zeros(land.shape, bool)
        beside[1:] |= land[:-1]; beside[:-1] |= land[1:]; beside[:, 1:] |= land[:, :-1]; beside[:, :-1] |= land[:, 1:]
        places["beside land"] = beside & ~land
    for name, where in places.items():
        found = set(kind[where].tolist())
        assert found == {0, 1, 2, 3}, f"{grid} {shape}: only the kinds {sorted(found)} on {name}"
    atm = case["atm"]
    for n, lo, hi in (("q", 0, 0.02), ("p", 98000, 103000), ("longwave", 0, 450), ("shortwave", 0, 900), ("u", -20.1, 20.1), ("v", -20.1, 20.1)):
        assert lo <= atm[n].min() and atm[n].max() <= hi and np.ptp(atm[n]) > 0.5 * (hi - lo), n
    # the halo cells are no periodic images
    assert not np.array_equal(atm["q"][H - 1, H:H + g["Ny"]], atm["q"][H + g["Nx"] - 1, H:H + g["Ny"]])


# ---- the oracle against the statement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid,shape", CASES)
def test_the_oracle_is_the_statement(grid, shape):
    case = oracle_case("f64", grid, shape)
    label = f"oracle f64 {grid} {shape}"
    for n in FLUXES:
        fs.judge_flux(label, n, case["got"][n], case["want"][n], fs.regimes_at(case["regimes"], n, case["want"][n].shape[1]))
    exact_facts(label, case, case["got"], case["want"], case["regimes"])


@pytest.mark.parametrize("grid,shape", CASES)
def test_the_float32_oracle_only_rounds_the_result(grid, shape):
    """Its loop is fp64: one u32 of the cell's own value for the store (and the statement's own 1e-10 of the scale, which is what
    the fp64 oracle is within)."""
    case = oracle_case("f32", grid, shape)
    label = f"oracle f32 {grid} {shape}"
    for n in FLUXES:
        want = case["want"][n]
        fs.judge_flux(label, n, case["got"][n], want, fs.regimes_at(case["regimes"], n, case["want"][n].shape[1]),
                      tol=ss.U32 * np.abs(want) + fs.RTOL_F64 * np.abs(want).max())
    exact_facts(label, case, case["got"], case["want"], case["regimes"])


@pytest.mark.parametrize("grid", GRIDS)
def test_the_yardstick_of_a_float32_iteration(grid):
    """loop_dtype = float32 against float64, per case, field and regime, in units of the field's scale: printed, finite, and the
    classes `clamped` and `gust_floor` really are exercised in single precision."""
    for shape in SHAPES:
        y = yardstick(oracle_case("f32", grid, shape))
        print(f"\nyardstick {grid} {shape_on(grid, shape)}:  " + "  ".join(f"{r:>10s}" for r in fs.REGIMES[1:]))
        for n in FLUXES:
            print(f"    J^{n}  " + "  ".join(f"{y[n, r]:10.3e}" for r in fs.REGIMES[1:]))
        assert all(np.isfinite(v) for v in y.values()), y
        for r in ("clamped", "gust_floor"):
            assert any(y[n, r] > 0 for n in FLUXES), f"{grid} {shape}: the float32 iteration equals the float64 one on every {r} cell"


# ---- where the tendencies receive the fluxes ----------------------------------------------------------------------------------------------------
def random_top_fluxes(m, seed=0):
    b = m.backend
    return {n: (FLUX_SCALE[n] * (2 * counter_rng(b.field_dims(n, False)[:2], 800 + seed, q) - 1)).astype(b.dtype) for q, n in enumerate(FLUXES)}


def tendencies(m, g):
    return {n: ss.interior(m.backend.get_field("Gn." + n, True), g) for n in FLUXES}


def three_ways(m, g, evaluate):
    """{"none", "top", "drag": {name: interior Gn.name}} of the state the model holds, the top fluxes set and the velocities the
    drag reads; the model is left without boundary fluxes."""
    b = m.backend
    out = {}
    b.set_bottom_drag(0.0)
    gb.set_top_flux(m, u=None, v=None, T=None, S=None)
    evaluate(m)
    out["none"] = tendencies(m, g)
    J = random_top_fluxes(m)
    gb.set_top_flux(m, **J)
    evaluate(m)
    out["top"] = tendencies(m, g)
    gb.set_top_flux(m, u=None, v=None, T=None, S=None)
    b.set_bottom_drag(CD)
    evaluate(m)
    out["drag"] = tendencies(m, g)
    vel = {n: b.get_field(n, True) for n in ("u", "v")}
    b.set_bottom_drag(0.0)
    return out, J, vel


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(f"u{a.dtype.itemsize}")


def judge_application(label, name, G_without, G_with, inc, touched, u_, extra=0):
    """Off the touched cells the same bits; on them G with - G without = inc within forcing_spec.application_bound.  Returns the
    worst ratio."""
    same = bits(G_with) == bits(G_without)
    bad = np.argwhere(~touched & ~same)
    assert bad.size == 0, f"{label}: Gn.{name} changes at {tuple(int(q) for q in bad[0])} (and {len(bad) - 1} more cells), which no boundary flux touches"
    d = G_with.astype(ss.LD) - G_without.astype(ss.LD)
    bound = fs.application_bound(G_without, inc, u_, extra) + ss.SPEC * ss.EPS_LD * np.abs(inc)
    return ss.check(f"{label}: the boundary flux in Gn.{name}", d - inc, bound, where=touched)


def judge_three_ways(label, g, out, J, vel, dtype, mutate_top=None, mutate_drag=None):
    u_ = ss.unit_roundoff(dtype)
    res = {}
    inc, touched = fs.boundary_contribution(J, None, g)
    if mutate_top:
        inc, touched = mutate_top(inc, touched)
    for n in FLUXES:
        assert touched[n].any() and (np.abs(inc[n][touched[n]]) > 0).all()
        res["top " + n] = judge_application(label + " top", n, out["none"][n], out["top"][n], inc[n], touched[n], u_)
    Cd = dtype(CD)
    exact = (mutate_drag or fs.bottom_drag)(vel["u"], vel["v"], g, Cd)
    bound = fs.bottom_drag(vel["u"], vel["v"], g, Cd, dtype)
    inc, touched = fs.boundary_contribution(None, dict(u=exact["u"], v=exact["v"]), g)
    extra, _ = fs.boundary_contribution(None, dict(u=bound["bound_u"], v=bound["bound_v"]), g)
    for n in ("u", "v"):
        assert touched[n].any() and np.abs(inc[n][touched[n]]).max() > 0
        res["drag " + n] = judge_application(label + " drag", n, out["none"][n], out["drag"][n], inc[n], touched[n], u_, extra[n])
        # the same as a statement about the flux itself: J = (G with - G without) dz against bottom_drag
        k = np.minimum(exact["k" + n][:, :g["Ny"]], g["Nz"] - 1)
        dz = np.asarray(g["dz"]).astype(ss.LD)[k]
        take = lambda a: np.take_along_axis(a[:, :g["Ny"]], k[:, :, None], axis=2)[:, :, 0]
        Jdev = take(out["drag"][n].astype(ss.LD) - out["none"][n].astype(ss.LD)) * dz
        Jbound = take(fs.application_bound(out["none"][n], inc[n], u_, extra[n])) * dz
        free = exact["k" + n][:, :g["Ny"]] < g["Nz"]
        Jx = np.asarray(exact[n])[:, :g["Ny"]]
        rel = np.where(free & (Jx != 0), Jbound / np.where(Jx != 0, np.abs(Jx), 1), 0).astype(float)
        print(f"{label}: the drag flux of {n} is read off the tendencies to within {np.median(rel[free]):.2e} of itself (median; worst {rel.max():.2e})")
        ss.check(f"{label}: the drag flux of {n}", Jdev - Jx, Jbound + ss.SPEC * ss.EPS_LD * np.abs(Jx), where=free)
    for n in ("T", "S"):
        assert np.array_equal(bits(out["drag"][n]), bits(out["none"][n])), f"{label}: the drag changes Gn.{n}"
    print(f"{label}: " + "  ".join(f"{k} {v:.3f}" for k, v in res.items()))
    return res


@functools.lru_cache(maxsize=None)
def oracle_three_ways(precision, grid, Nz=6):
    m, g = build(CPU(precision), grid, (70, 13, Nz))
    set_ocean(m, g)
    out, J, vel = three_ways(m, g, lambda m: m.backend.compute_tendencies())
    dtype = m.backend.dtype
    m.backend.close()
    return g, out, J, vel, dtype


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_the_oracle_applies_the_fluxes_where_the_statement_says(precision, grid):
    g, out, J, vel, dtype = oracle_three_ways(precision, grid)
    if g["immersed"]:
        ku, _ = fs.first_free_levels(g)
        assert (ku == 0).any() and ((ku > 0) & (ku < g["Nz"])).any() and (ku == g["Nz"]).any()
    judge_three_ways(f"oracle {precision} {grid}", g, out, J, vel, dtype)


# ---- the judges are sharp: a mutated statement fails on the same oracle output ----------------------------------------------------------------
def test_swapped_humidity_and_longwave_fail():
    case = oracle_case("f64", "gaussian_islands_lat_lon", (70, 13, 6))
    atm = dict(case["atm"], q=case["atm"]["longwave"], longwave=case["atm"]["q"])
    want, regimes = statement(dict(case, atm=atm), south_row_is_land=True)
    for n in FLUXES:
        with pytest.raises(AssertionError, match=f"J\\^{n}"):
            fs.judge_flux("swapped", n, case["got"][n], want[n])
    # (and one of them alone)
    want, _ = statement(dict(case, atm=dict(case["atm"], longwave=0 * case["atm"]["longwave"])), south_row_is_land=True)
    with pytest.raises(AssertionError, match="J\\^T"):
        fs.judge_flux("no longwave", "T", case["got"]["T"], want["T"])
    fs.judge_flux("no longwave", "S", case["got"]["S"], want["S"])


@pytest.mark.parametrize("grid", ["simple_lat_lon", "gaussian_islands"])
def test_a_shifted_west_halo_column_fails(grid):
    """The statement reading column -2 (or the periodic image) where the kernel reads column -1: J^u of column 0 fails, and only it."""
    case = oracle_case("f64", grid, (70, 13, 6))
    H, Nx = case["g"]["H"], case["g"]["Nx"]
    for source in (H - 2, H + Nx - 1):
        atm = {n: a.copy() for n, a in case["atm"].items()}
        for a in atm.values():
            a[H - 1] = a[source]
        want, _ = statement(dict(case, atm=atm), south_row_is_land=True)
        with pytest.raises(AssertionError, match=r"J\^u at \(0, "):
            fs.judge_flux("shifted", "u", case["got"]["u"], want["u"])
        for n in ("v", "T", "S"):
            fs.judge_flux("shifted", n, case["got"][n], want[n])


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_a_top_flux_one_level_down_fails(precision):
    g, out, J, vel, dtype = oracle_three_ways(precision, "gaussian_islands_lat_lon")

    def down(inc, touched):
        return ({n: np.roll(a, -1, axis=2) for n, a in inc.items()}, {n: np.roll(a, -1, axis=2) for n, a in touched.items()})

    with pytest.raises(AssertionError, match="which no boundary flux touches"):
        judge_three_ways("one level down", g, out, J, vel, dtype, mutate_top=down)


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("grid", ["simple_lat_lon", "gaussian_islands"])
def test_a_two_point_average_in_the_drag_fails(precision, grid):
    g, out, J, vel, dtype = oracle_three_ways(precision, grid)

    def two_points(u, v, g, Cd, dtype=None):
        return fs.bottom_drag(u, v, g, Cd, dtype, points=2)

    with pytest.raises(AssertionError, match="drag"):
        judge_three_ways("two points", g, out, J, vel, dtype, mutate_drag=two_points)


def test_a_first_free_level_one_too_high_fails():
    g, out, J, vel, dtype = oracle_three_ways("f64", "gaussian_islands_lat_lon")

    def higher(u, v, g2, Cd, dtype=None):
        return fs.bottom_drag(u, v, dict(g2, kbot=np.where(g2["kbot"] > 0, g2["kbot"] + 1, 0)), Cd, dtype)

    with pytest.raises(AssertionError):
        judge_three_ways("one level up", g, out, J, vel, dtype, mutate_drag=higher)
