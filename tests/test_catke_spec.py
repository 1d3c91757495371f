"""tests/catke_spec.py proved on the CPU oracle before tests/test_gpu_catke_spec.py judges the device by it: the oracle in Float64
AND in Float32 is judged cell by cell for every grid at Nz 6, 33, 65 -- the bounds C_<field> of catke_spec are 4 x the largest r
measured HERE (test_the_oracle_measures_the_bounds prints them) --, no cell of these inputs sits near a switch, and the spec
notices every wrong kernel the issue of this work lists: handed a mutated input, formula or output, the same oracle output fails.

Inputs (set_inputs; through set / set_field(..., True) with counter_rng): u, v of order 0.05; T a column profile with level
differences of 1.1e-3 .. 5e-3 K, a third of them unstable; S with differences at least four times weaker in buoyancy; e
log-uniform 1e-7 .. 1e-3 with a few per cent negative and a few per cent under e_min / 2; J^b per column 0 or 1e-9 .. 1e-6; the
old kappa_u, kappa_c log-uniform with 5 % zeros and INDEPENDENT noise in every halo cell; G^n.e, G^-.e of order 1e-8; kappa_e,
L^e noise everywhere; top fluxes of u, v, T, S per column, T of both signs.

Drive: update_state on the fresh model (u- = u); the inputs, with new u, v; previous_u, previous_v read back and asserted to
differ from u, v; the judged update_state (dt_since = 0: J^b keeps its bits); one time_step (dt_since = dt: the J^b filter)."""
import functools

import numpy as np
import pytest

import gb25_amd as gb
import catke_spec as cs
import step_spec as ss
import test_implicit_spec as tis
from helpers import counter_rng
from oracle_backend import CPU

DT = 600.0
GRIDS = list(tis.GRID_TYPES)
READ = ("u", "v", "T", "S", "e", "kappa_u", "kappa_c", "kappa_e", "Le", "Jb", "previous_u", "previous_v", "Gn.e", "Gm.e")
JUDGED = ("Gm.e", "Le", "e", "kappa_u", "kappa_c", "kappa_e")


def shape_of(grid, Nz, device=False):
    return ((70, 13, Nz) if device else (20, 9, Nz)) if grid in ("flat", "made") else (48, 24, Nz)


def level_chunks(columns, Nz):
    """The rule of catke_level_chunks (gb25_api.hip), written out a second time."""
    kch = 1
    while kch < 8 and columns * kch < 600000 and Nz // (kch + 1) >= 8:
        kch += 1
    return kch


def form_of(float_type, Nz, columns):
    """(chunks of levels of the column kernels, the form of the e solve)"""
    limit = 64 if float_type == "Float32" else 32
    return level_chunks(columns, Nz), "stream" if Nz > limit else "var<%d>" % next(n for n in (32, 48, 64) if Nz <= n)


def _loguniform(shape, lo, hi, seed, salt):
    return 10.0 ** (np.log10(lo) + (np.log10(hi) - np.log10(lo)) * counter_rng(shape, seed, salt))


def set_inputs(m, g, seed=0, still=False, halo_seed=None):
    """The inputs of the module docstring; returns the top fluxes as the build holds them.  halo_seed: other noise in the halo
    cells of the old kappa_u (first halo column / row included), the interior as before."""
    b, H, Nx, Ny, Nz = m.backend, g["H"], g["Nx"], g["Ny"], g["Nz"]
    dtype = b.dtype
    r = lambda shape, salt: counter_rng(shape, 700 + seed, salt)
    c3 = (Nx, Ny, Nz)
    vals = {}
    for q, n in enumerate(("u", "v")):
        a = 0.05 * (2 * r(b.field_dims(n, False), q) - 1) * (0.0 if still else 1.0)
        if n == "v":
            a[:, 0] = 0
            if not g["folded"]:
                a[:, -1] = 0
        vals[n] = a.astype(dtype)
    step = np.where(r(c3, 2) < 1 / 3, -1.0, 1.0) * (1.1e-3 + 3.9e-3 * r(c3, 3))
    vals["T"] = (12.0 + 2 * (r((Nx, Ny, 1), 4) - 0.5) + np.cumsum(step, axis=2)).astype(dtype)
    vals["S"] = (35.0 + 0.2 * (r((Nx, Ny, 1), 5) - 0.5) + 1.5e-5 * (2 * r(c3, 6) - 1)).astype(dtype)
    m.set(**vals)

    def parent(n, make):
        shape = b.field_dims(n, True)
        b.set_field(n, make(shape).astype(dtype), True)

    def tke(shape):
        kind = r(shape, 8)
        return np.where(kind < 0.04, -_loguniform(shape, 1e-8, 1e-6, 700 + seed, 9),
                        np.where(kind < 0.08, _loguniform(shape, 1e-12, 5e-10, 700 + seed, 10), _loguniform(shape, 1e-7, 1e-3, 700 + seed, 11)))

    parent("e", tke)
    parent("Jb", lambda s: np.where(r(s, 12) < 0.05, 0.0, _loguniform(s, 1e-9, 1e-6, 700 + seed, 13)))
    for q, n in enumerate(("kappa_u", "kappa_c")):
        def kappa(s, q=q, n=n):
            a = np.where(r(s, 14 + q) < 0.05, 0.0, _loguniform(s, 1e-6, 1e-1, 700 + seed, 16 + q))
            if n == "kappa_u" and halo_seed is not None:
                other = _loguniform(s, 1e-6, 1e-1, 900 + halo_seed, 16)
                inner = np.zeros(s, bool)
                inner[H:H + Nx, H:H + Ny] = True
                a = np.where(inner, a, other)
            return a
        parent(n, kappa)
    for q, n in enumerate(("Gn.e", "Gm.e")):
        parent(n, lambda s, q=q: 1e-8 * (2 * r(s, 18 + q) - 1))
    parent("kappa_e", lambda s: _loguniform(s, 1e-6, 1e-1, 700 + seed, 20))
    parent("Le", lambda s: -_loguniform(s, 1e-6, 1e-2, 700 + seed, 21))
    flux = {}
    for q, (n, amp) in enumerate((("u", 1e-4), ("v", 1e-4), ("T", 2e-5), ("S", 1e-6))):
        flux[n] = (amp * (2 * r(b.field_dims(n, False)[:2], 22 + q) - 1)).astype(dtype)
    gb.set_top_flux(m, **flux)
    return flux


def drive(arch, grid, shape, still=False, halo_seed=None, step=True, **options):
    """(model, case): the drive of the module docstring.  case: g, x (the spec's inputs of the judged call), before / got (parent
    arrays around it), and around the time_step: x2 (inputs read after it), Jb_old, Jb_new, e_new."""
    m, g, _, _ = tis.build(arch, grid, shape, "catke", dt=DT, **options)
    b = m.backend
    gb.update_state(m)
    flux = set_inputs(m, g, still=still, halo_seed=halo_seed)
    before = {n: b.get_field(n, True) for n in READ}
    if not still:
        for n in ("u", "v"):
            assert not np.array_equal(before["previous_" + n], before[n]), f"previous_{n} was dragged along by the setter of {n}"
    gb.update_state(m)
    got = {n: b.get_field(n, True) for n in READ + ("Gn.e",)}
    fields = {n: (got[n] if n in ("u", "v", "T", "S") else before[n]) for n in cs.FIELDS_IN}    # (u, v, T, S: masked, halos filled)
    case = dict(g=g, before=before, got=got, x=cs.Inputs(b, g, DT, fields=fields, top_flux=flux), flux=flux)
    if step:
        gb.time_step(m)
        after = {n: b.get_field(n, True) for n in READ}
        case.update(x2=cs.Inputs(b, g, DT, fields={n: after[n] for n in cs.FIELDS_IN}, top_flux=flux), Jb_old=got["Jb"], Jb_new=after["Jb"],
                    e_new=ss.interior(after["e"], g))
    return m, case


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    t = np.dtype(f"u{a.dtype.itemsize}")
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(t), b.view(t))


def check_case(label, case, strict=True, keep=True):
    """Everything the spec says about one driven case; returns {field: worst r} (the update's fields, then Jb after the step)."""
    g, x, before, got = case["g"], case["x"], case["before"], case["got"]
    out = cs.judge_update(label, x, got, strict=strict)
    for n in ("u", "v"):
        assert bits_equal(got["previous_" + n], got[n]), f"{label}: previous_{n} is not {n} bit for bit after the call"
    Jin, land = ss.interior(before["Jb"], g), g["kbot"] >= g["Nz"]
    assert bits_equal(ss.interior(got["Jb"], g), np.where(land, 0, Jin).astype(Jin.dtype)), f"{label}: Jb changed in a call with dt_since = 0"
    cs.exact_zeros(label, x, got)
    for n in cs.OUTSIDE_FIELDS:
        cs.check_outside(label, g, n, before[n], got[n], keep=keep)
    res = {n: v[0] for n, v in out.items()}
    left = max(v[2] for v in out.values())
    if "x2" in case:
        r, at, l2 = cs.judge_flux(label, case["x2"], case["e_new"], case["Jb_old"], case["Jb_new"], DT, strict=strict)
        res["Jb"] = r
        assert np.abs(ss.interior(case["Jb_new"], g) - ss.interior(case["Jb_old"], g)).max() > 0, f"{label}: the filter did nothing"
    return res, left


def report(label, res):
    print(f"[catke] {label}: worst r / C = " + ", ".join(f"{n} {r / cs.C[n]:.3f} (r {r:.3g})" for n, r in res.items()))


@functools.lru_cache(maxsize=None)
def oracle_case(precision, grid, Nz, still=False):
    m, case = drive(CPU(precision), grid, shape_of(grid, Nz), still=still)
    m.backend.close()
    return case


# ---- the spec's own pieces --------------------------------------------------------------------------------------------------
def test_alpha_and_beta_are_the_oracles():
    m, _ = drive(CPU("f64"), "flat", shape_of("flat", 6), step=False)
    try:
        for (T, S, Z) in ((10.0, 35.0, -1000.0), (25.0, 33.0, -5.0), (2.0, 36.5, -3500.0)):
            a, b = m.backend.teos10_sensitivities(T, S, Z)
            sa, sb, _, _ = cs.teos10_sensitivities(T, S, Z)
            assert float(sa) == pytest.approx(a, rel=1e-13) and float(sb) == pytest.approx(b, rel=1e-13)
    finally:
        m.backend.close()


def test_the_chunk_rule_gives_the_forms_of_the_issue():
    want = {6: (1, "var<32>", "var<32>"), 15: (1, "var<32>", "var<32>"), 17: (2, "var<32>", "var<32>"), 33: (4, "var<48>", "stream"),
            64: (8, "var<64>", "stream"), 65: (8, "stream", "stream")}
    for Nz, (kch, f32, f64) in want.items():
        for columns in (70 * 13, 48 * 24):
            assert form_of("Float32", Nz, columns) == (kch, f32) and form_of("Float64", Nz, columns) == (kch, f64)
    assert level_chunks(70 * 13, 16) == 2 and level_chunks(600000, 65) == 1


def test_the_thomas_sweep_is_a_dense_solve():
    case = oracle_case("f64", "made", 6)
    x = case["x"]
    w = cs.tke_step(x)
    i, j = 2, 2
    Nz, dt = x.Nz, float(x.dt)
    A = np.zeros((Nz, Nz))
    dzc, dzf, ke, L = (np.asarray(a, np.float64) for a in (x.dzc, x.dzf, w["ke"][i, j], w["Le"][i, j]))
    for k in range(Nz):
        lo = -dt * ke[k] / (dzc[k] * dzf[k]) if k > 0 else 0.0
        up = -dt * ke[k + 1] / (dzc[k] * dzf[k + 1]) if k < Nz - 1 else 0.0
        A[k, k] = 1 - lo - up - dt * L[k]
        if k > 0:
            A[k, k - 1] = lo
        if k < Nz - 1:
            A[k, k + 1] = up
    assert np.allclose(np.linalg.solve(A, np.asarray(w["es"][i, j], np.float64)), np.asarray(w["e"][i, j], np.float64), rtol=1e-12, atol=0)


# ---- the oracle is judged, and measures the bounds ------------------------------------------------------------------------------
@pytest.mark.parametrize("Nz", [6, 33, 65])
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_the_oracle_stays_within_the_bounds(precision, grid, Nz):
    case = oracle_case(precision, grid, Nz)
    g, x = case["g"], case["x"]
    label = f"oracle {precision} {grid} Nz {Nz}"
    kb = g["kbot"]
    if grid != "flat":
        assert (kb > 0).any() and (kb == 0).any() and (kb != np.roll(kb, 1, axis=0)).any()
    # the inputs are what they are meant to be
    F = cs.face_state(x)
    T, S = x.cells("T"), x.cells("S")
    al, be, _, _ = cs.teos10_sensitivities((T[:, :, 1:] + T[:, :, :-1]) / 2, (S[:, :, 1:] + S[:, :, :-1]) / 2, x.zf[1:Nz][None, None, :])
    op = F["open"][:, :, 1:Nz]
    assert (np.abs(al * np.diff(T, axis=2))[op] >= 4 * np.abs(be * np.diff(S, axis=2))[op]).all(), "S weighs more than a quarter of T in N^2"
    unstable = (F["N2"] < 0)[F["open"]].mean()
    assert 0.2 < unstable < 0.45, unstable
    above = np.concatenate([F["N2"][:, :, 1:], np.zeros_like(F["N2"][:, :, :1])], axis=2)
    assert ((F["N2"] > 0) & (above < 0) & (x.column("Jb") > 1e-11)[:, :, None]).any(), "no entraining face"
    e = x.cells("e")
    assert (e < 0).any() and ((e > 0) & (e < 5e-10)).any()
    res, left = check_case(label, case, keep=False)     # (the oracle's fills write more halo cells than the device's images)
    assert left == 0.0, f"{label}: cells near a switch with these inputs"
    report(label, res)
    assert all(np.isfinite(r) for r in res.values())


def test_the_oracle_measures_the_bounds():
    """The largest r per field over every case above, both precisions: C_<field> = 4 x these (catke_spec)."""
    worst = {}
    for precision in ("f64", "f32"):
        for grid in GRIDS:
            for Nz in (6, 33, 65):
                res, _ = check_case("measure", oracle_case(precision, grid, Nz), strict=False, keep=False)
                for n, r in res.items():
                    worst[n] = max(worst.get(n, 0.0), r)
            src, s = cs.surface_source(oracle_case(precision, grid, 17, True)["x"])
            got = ss.interior(oracle_case(precision, grid, 17, True)["got"]["Gn.e"], oracle_case(precision, grid, 17, True)["g"])[:, :, -1]
            r = cs.measure(got, src, s, ss.unit_roundoff(got.dtype), np.ones(src.shape, bool), np.zeros(src.shape, bool))[0]
            worst["source"] = max(worst.get("source", 0.0), r)
    print("[catke] the oracle's largest r per field: " + ", ".join(f"{n} {r:.3g}" for n, r in worst.items()))
    # (the constants were written down from this print; another compiler or libm moves the oracle's r a little, so the check is
    # that each constant still is about 4 x what the oracle reaches: between 2 x and 8 x)
    for n, r in worst.items():
        assert cs.C[n] / 8 <= r <= cs.C[n] / 2, f"{n}: the oracle reaches r = {r:.4g}; C_{n} = {cs.C[n]:.4g} is no longer about 4 x that"


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_the_still_case_on_the_oracle(precision, grid):
    check_still(f"oracle {precision} {grid} still", oracle_case(precision, grid, 17, True))


def check_still(label, case):
    """u = v = 0 with fluxes set: G^n.e is exactly 0 below the top cell and the surface source in it."""
    g, x = case["g"], case["x"]
    Gn = ss.interior(case["got"]["Gn.e"], g)
    ss.check_zero(f"{label}: Gn.e below the top cell", Gn[:, :, :-1], np.ones(Gn[:, :, :-1].shape, bool))
    src, s = cs.surface_source(x)
    r, at, _ = cs.measure(Gn[:, :, -1], src, s, x.u_, np.ones(src.shape, bool), np.zeros(src.shape, bool))
    print(f"[catke] {label}: surface source r / C = {r / cs.C_SRC:.3f} at {at}")
    assert r <= cs.C_SRC, f"{label}: the surface source is {r:.4g} u away at column {at}; the bound is {cs.C_SRC:.4g}"
    ss.check_zero(f"{label}: the source on land", Gn[:, :, -1], g["kbot"] >= g["Nz"])
    assert np.abs(Gn[:, :, -1]).max() > 0
    return r


# ---- the spec must notice a wrong kernel --------------------------------------------------------------------------------------
def mutated_inputs(case):
    """{name: (fields that must fail, the spec's inputs mutated)}"""
    x, g = case["x"], case["g"]
    H, Nx, Nz, kb = g["H"], g["Nx"], g["Nz"], g["kbot"]
    ku, kc = x.f["kappa_u"], x.f["kappa_c"]
    image = ku.copy()
    image[H - 1] = ku[H + Nx - 1]
    every = JUDGED
    return {"kappa_u of the west face averaged with i+1": (("Gm.e",), x.but(mut=["kappa_u west with i+1"])),
            "kappa_u of the south face averaged with j+1": (("Gm.e",), x.but(mut=["kappa_u south with j+1"])),
            "the periodic image at i = -1": (("Gm.e",), x.but(kappa_u=image)),
            "previous velocities replaced by the current ones": (("Gm.e",), x.but(previous_u=x.f["u"], previous_v=x.f["v"])),
            "first active level one too high": (every, x.but(kbot=np.minimum(kb + 1, Nz))),
            "first active level one too low": (every, x.but(kbot=np.maximum(kb - 1, 0))),
            "shear not masked at an inactive node": (("Gm.e",), x.but(mut=["shear not masked"])),
            "kappa one face too high": (("Gm.e",), x.but(kappa_u=tis.shifted(ku, 2), kappa_c=tis.shifted(kc, 2))),
            "N2 of the face above taken from the face itself": (("kappa_c",), x.but(mut=["N2 above is N2"])),
            "e_min floor dropped in Le": (("Le",), x.but(mut=["no e_min floor in Le"])),
            "bottom flux on level 0 of a raised column": (("Le",), x.but(mut=["bottom flux on level 0"]))}


MUTATIONS = ["kappa_u of the west face averaged with i+1", "kappa_u of the south face averaged with j+1", "the periodic image at i = -1",
             "previous velocities replaced by the current ones", "first active level one too high", "first active level one too low",
             "shear not masked at an inactive node", "kappa one face too high", "N2 of the face above taken from the face itself",
             "e_min floor dropped in Le", "bottom flux on level 0 of a raised column"]


@pytest.mark.parametrize("mutation", MUTATIONS)
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_a_mutated_input_fails_the_spec(precision, mutation):
    case = oracle_case(precision, "made", 33)
    cs.judge_update("unmutated", case["x"], case["got"])
    fields, x = mutated_inputs(case)[mutation]
    for n in fields:
        with pytest.raises(AssertionError):
            cs.judge_update(mutation, x, case["got"], fields=(n,))


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_the_old_flux_replaced_by_the_new_one_fails_the_filter(precision):
    case = oracle_case(precision, "made", 33)
    cs.judge_flux("unmutated", case["x2"], case["e_new"], case["Jb_old"], case["Jb_new"], DT)
    with pytest.raises(AssertionError):
        cs.judge_flux("old = new", case["x2"], case["e_new"], case["Jb_new"], case["Jb_new"], DT)


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_a_moved_level_fails_the_spec(precision):
    """One level of one output column moved by 4 x its bound: a flat column, one beside the step, the column at i = 0; the first
    wet level, a middle one, the top one."""
    case = oracle_case(precision, "made", 33)
    x, g, got = case["x"], case["g"], case["got"]
    H, Nz = g["H"], g["Nz"]
    want = cs.tke_step(x, Gm_got=ss.interior(got["Gm.e"], g))
    F = cs.face_state(x, e=ss.interior(got["e"], g), Jb=ss.interior(got["Jb"], g))
    scales = {"Gm.e": want["s_Gm"], "Le": want["s_Le"], "e": want["s_e"], "kappa_u": F["s_ku"], "kappa_c": F["s_kc"], "kappa_e": F["s_ke"]}
    for n in JUDGED:
        for (i, j) in ((2, 2), (12, 3), (0, 5)):
            kf = int(g["kbot"][i, j]) + (1 if n.startswith("kappa") else 0)
            for k in sorted({kf, (kf + Nz) // 2, Nz - 1}):
                moved = dict(got)
                a = got[n].astype(np.longdouble)
                a[H + i, H + j, H + k] += 4 * cs.C[n] * x.u_ * scales[n][i, j, k]
                moved[n] = a
                assert scales[n][i, j, k] > 0
                with pytest.raises(AssertionError):
                    cs.judge_update(f"{n} moved at {(i, j, k)}", x, moved, fields=(n,))


@pytest.mark.parametrize("grid", ["made", "folded"])
def test_a_wrong_halo_image_fails_the_table(grid):
    case = oracle_case("f32", grid, 6)
    g, got = case["g"], case["got"]
    H, Nx, Ny, Nz = g["H"], g["Nx"], g["Ny"], g["Nz"]
    for n in cs.OUTSIDE_FIELDS:
        cs.check_outside("unmutated", g, n, case["before"][n], got[n], keep=False)
        k = 0 if n == "Jb" else H + 2
        for cell in ((H - 1, H - 1, k), (H + Nx, H + Ny, k), (0, H + 3, k)) + (((H + 5, H + Ny + H - 1, k),) if grid == "folded" else ()):
            a = got[n].copy()
            a[cell] = np.nextafter(a[cell], np.inf)
            with pytest.raises(AssertionError):
                cs.check_outside("one image wrong", g, n, case["before"][n], a, keep=False)
        a = got[n].copy()
        a[0, 0, 0] += 1          # a corner the call does not write: it must keep its bits
        with pytest.raises(AssertionError):
            cs.check_outside("a cell nobody writes", g, n, got[n], a, keep=True)
