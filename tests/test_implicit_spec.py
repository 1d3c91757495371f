"""tests/implicit_spec.py proved on the CPU oracle before tests/test_gpu_implicit.py judges the device by it: the oracle in Float64
AND in Float32 stays within the derived bound of the residual, and the spec notices every wrong kernel the issue of this work
lists -- handed a mutated input, the same oracle output fails.

The solve is driven alone (drive): u, v, T, S through set, noise in every halo cell of theirs, zero tendencies, with CATKE the
diffusivity fields set with their halos (independent noise there, NOT the periodic image), then ab2_step(dt, euler) -- no
update_state in between, so no closure overwrites the kappa the test set.  The e slice of the CATKE solve is not covered here:
tests/test_catke_spec.py and tests/test_gpu_catke_spec.py judge it (its right-hand side is rebuilt from G^-.e).

set_bottom_height on simple_lat_lon does switch both implementations to their immersed paths (the oracle's is_immersed; the
library's immersed kernel instances follow the same flag), so the made bottom (made_levels) is an immersed case of its own
beside the built-in island grids."""
import functools

import numpy as np
import pytest

import gb25_amd as gb
import implicit_spec as isp
import step_spec as ss
from helpers import counter_rng
from oracle_backend import CPU

DT = 1800.0
K_CONST = 10.0
GRID_TYPES = {"flat": "simple_lat_lon", "made": "simple_lat_lon", "islands": "gaussian_islands_lat_lon", "folded": "gaussian_islands"}
MEANS = {"u": 0.0, "v": 0.0, "T": 10.0, "S": 35.0}


def made_levels(Nx, Ny, Nz):
    """Number of dry levels per column of the made bottom: a fully dry column, one whose only wet level is the top one, a raised
    block with a step in it (neighbours of different depth in x and in y), raised columns at i = 0 and i = Nx-1 (the periodic
    neighbours) and on both wall rows, flat columns everywhere else."""
    assert Nx >= 16 and Ny >= 8 and Nz >= 6
    level = np.zeros((Nx, Ny), int)
    level[5, 4] = Nz
    level[9, 6] = Nz - 1
    level[12:15, 2:5] = Nz // 2
    level[13, 3] = Nz // 2 + 1
    level[0, 7], level[Nx - 1, 2], level[Nx - 1, 7] = 2, 3, 1
    level[3, 0], level[7, Ny - 1] = 1, 2
    return level


def build(arch, grid, shape, closure, dt=DT, K=K_CONST, **options):
    """A model of `grid` (GRID_TYPES) with the closure "const" (VerticalScalarDiffusivity(K, K)) or "catke", its geometry and spacings."""
    Nx, Ny, Nz = shape
    cl = gb.CATKEVerticalDiffusivity() if closure == "catke" else gb.VerticalScalarDiffusivity(nu=K, kappa=K)
    m = gb.baroclinic_instability_model(arch, Nx, Ny, Nz, dt=dt, grid_type=GRID_TYPES[grid], closure=cl, **(dict(options=options) if options else {}))
    b = m.backend
    if grid == "made":
        zf = np.array([b.metric("zf", k) for k in range(1, Nz + 2)])
        zc = np.array([b.metric("zc", k) for k in range(1, Nz + 1)])
        level = made_levels(Nx, Ny, Nz)
        # the bottom between the centre of the highest dry cell and its top face
        b.set_bottom_height(np.where(level > 0, 0.5 * (zc[np.maximum(level, 1) - 1] + zf[level]), -5000.0))
    g = ss.read_geometry(b, GRID_TYPES[grid], shape, b.H if hasattr(b, "H") else b.cfg.halo)
    if grid == "made":
        assert np.array_equal(g["kbot"], made_levels(Nx, Ny, Nz)), "the bottom is not the one this test made"
    dzc, dzf = isp.spacings(b, Nz)
    return m, g, dzc, dzf


def set_inputs(m, g, dzf, dt, closure, seed=0):
    """x* of order 1 around MEANS (S not uniform) through set, noise in every halo cell, zero tendencies, and with CATKE kappa_u,
    kappa_c log-uniform per cell and face so that dt kappa / dz^2 spans 1e-6 .. 1e4, about 5 % of the faces exactly 0, halos
    included and independent.  Returns the parent arrays the model holds: {name: array}."""
    b, H, Nz = m.backend, g["H"], g["Nz"]
    dtype = b.dtype
    vals = {}
    for q, n in enumerate(isp.FIELDS):
        a = MEANS[n] + 2 * counter_rng(b.field_dims(n, False), 100 + seed, q) - 1
        if n == "v":
            a[:, 0] = 0
            if not g["folded"]:
                a[:, -1] = 0
        vals[n] = a.astype(dtype)
    m.set(**vals)
    for q, n in enumerate(isp.FIELDS):
        a = b.get_field(n, True)
        halo = np.ones(a.shape, bool)
        halo[H:H + g["Nx"], H:H + isp.rows_of(n, g), H:H + Nz] = False
        a[halo] = (MEANS[n] + 2 * counter_rng(a.shape, 200 + seed, q) - 1).astype(dtype)[halo]
        b.set_field(n, a, True)
    for n in ("Gn.u", "Gn.v", "Gn.T", "Gn.S", "Gm.u", "Gm.v", "Gm.T", "Gm.S"):
        b.set_field(n, np.zeros(b.field_dims(n, True), dtype), True)
    held = {}
    if closure == "catke":
        for q, n in enumerate(("kappa_u", "kappa_c")):
            shape = b.field_dims(n, True)
            ratio = 10.0 ** (-6 + 10 * counter_rng(shape, 300 + seed, q))
            zero = counter_rng(shape, 400 + seed, q) < 0.05
            dz = dzf[np.clip(np.arange(shape[2]) - H, 0, Nz)]
            b.set_field(n, np.where(zero, 0.0, ratio * (dz * dz / dt)[None, None, :]).astype(dtype), True)
            held[n] = b.get_field(n, True)
    for n in isp.FIELDS:
        held[n] = b.get_field(n, True)
    return held


def judge(label, before, after, g, dt, dzc, dzf, u_, closure, K=K_CONST, fields=isp.FIELDS, **mutated):
    """{field: largest residual / bound}, printed, then asserted to be within 1; `mutated`: kappa_u, kappa_c or kfirst
    ({field: table}) in place of the inputs'."""
    out = {}
    for n in fields:
        kw = dict(K=K) if closure == "const" else dict(kappa_u=mutated.get("kappa_u", before.get("kappa_u")),
                                                       kappa_c=mutated.get("kappa_c", before.get("kappa_c")))
        kf = mutated["kfirst"][n] if "kfirst" in mutated else None
        out[n] = isp.check_solve(label, n, before[n], after[n], g, dt, dzc, dzf, u_, kfirst=kf, measure=True, **kw)
    print(f"[implicit solve] {label}: max residual / bound = " + ", ".join(f"{k} {v:.4f}" for k, v in out.items()))
    worst = max(out, key=out.get)
    assert out[worst] <= 1.0, f"{label}: the residual of the implicit solve of {worst} is {out[worst]:.4g} x the bound"
    return out


def drive(arch, grid, shape, closure, dt=DT, K=K_CONST, **options):
    """The solve alone on a fresh model: (model, geometry, dzc, dzf, parents before, parents after)."""
    m, g, dzc, dzf = build(arch, grid, shape, closure, dt, K, **options)
    before = set_inputs(m, g, dzf, dt, closure)
    m.backend.ab2_step(dt, True)
    after = {n: m.backend.get_field(n, True) for n in isp.FIELDS}
    return m, g, dzc, dzf, before, after


def shape_of(grid, Nz):
    return (20, 9, Nz) if grid in ("flat", "made") else (48, 24, Nz)


@functools.lru_cache(maxsize=None)
def oracle_solve(precision, grid, closure, Nz):
    m, g, dzc, dzf, before, after = drive(CPU(precision), grid, shape_of(grid, Nz), closure)
    u_ = ss.unit_roundoff(m.backend.dtype)
    m.backend.close()
    return g, dzc, dzf, before, after, u_


@pytest.mark.parametrize("Nz", [6, 33, 65])
@pytest.mark.parametrize("grid", list(GRID_TYPES))
@pytest.mark.parametrize("closure", ["const", "catke"])
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_the_oracle_stays_within_the_bound(precision, closure, grid, Nz):
    g, dzc, dzf, before, after, u_ = oracle_solve(precision, grid, closure, Nz)
    label = f"oracle {precision} {closure} {grid} Nz {Nz}"
    kb = g["kbot"]
    if grid != "flat":     # the inputs are what they are meant to be: wet and dry cells, faces between columns of different depth
        assert (kb > 0).any() and (kb == 0).any() and (kb != np.roll(kb, 1, axis=0)).any() and (kb[:, 1:] != kb[:, :-1]).any()
    if grid == "made":     # ... a fully dry column and a 1x1 system
        assert (kb == Nz).any() and (kb == Nz - 1).any()
    for n in isp.FIELDS:
        assert not np.array_equal(before[n], after[n]), f"{label}: the solve did nothing to {n}"
    judge(label, before, after, g, DT, dzc, dzf, u_, closure)


# ---- the spec must notice a wrong kernel --------------------------------------------------------------------------------------
def shifted(a, axis):
    """a[p + 1] at p along `axis` (the last one repeated): handed to the spec, its i-1 / j-1 / k become i / j / k+1 ... + 1."""
    return np.concatenate([np.take(a, range(1, a.shape[axis]), axis=axis), np.take(a, [a.shape[axis] - 1], axis=axis)], axis=axis)


def wrong_first_levels(g):
    kf, Nz = isp.first_free_levels(g), g["Nz"]
    return {"first free level one too high": (isp.FIELDS, dict(kfirst={n: np.minimum(k + 1, Nz) for n, k in kf.items()})),
            "first free level one too low": (isp.FIELDS, dict(kfirst={n: np.where(k < Nz, np.maximum(k - 1, 0), k) for n, k in kf.items()}))}


def mutations(g, before):
    """{name: (fields the mutation must fail on, the mutated inputs of the spec)}"""
    H, Nx = g["H"], g["Nx"]
    ku = before["kappa_u"]
    image = ku.copy()
    image[H - 1] = ku[H + Nx - 1]
    return {"kappa_u averaged with i+1": (("u",), dict(kappa_u=shifted(ku, 0))),
            "kappa_u averaged with j+1": (("v",), dict(kappa_u=shifted(ku, 1))),
            "kappa one face too high": (isp.FIELDS, dict(kappa_u=shifted(ku, 2), kappa_c=shifted(before["kappa_c"], 2))),
            "periodic image at i = 0": (("u",), dict(kappa_u=image)), **wrong_first_levels(g)}


MUTATIONS = ["kappa_u averaged with i+1", "kappa_u averaged with j+1", "kappa one face too high", "first free level one too high",
             "first free level one too low", "periodic image at i = 0"]


@pytest.mark.parametrize("mutation", MUTATIONS)
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_a_mutated_input_fails_the_spec(precision, mutation):
    g, dzc, dzf, before, after, u_ = oracle_solve(precision, "made", "catke", 33)
    judge("unmutated", before, after, g, DT, dzc, dzf, u_, "catke")
    fields, mutated = mutations(g, before)[mutation]
    for n in fields:
        with pytest.raises(AssertionError):
            judge(mutation, before, after, g, DT, dzc, dzf, u_, "catke", fields=(n,), **mutated)


@pytest.mark.parametrize("way", ["high", "low"])
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_a_wrong_first_level_fails_the_spec_with_a_constant_diffusivity(precision, way):
    g, dzc, dzf, before, after, u_ = oracle_solve(precision, "made", "const", 33)
    fields, mutated = wrong_first_levels(g)[f"first free level one too {way}"]
    for n in fields:
        with pytest.raises(AssertionError):
            judge(way, before, after, g, DT, dzc, dzf, u_, "const", fields=(n,), kfirst=mutated["kfirst"])


@pytest.mark.parametrize("closure", ["const", "catke"])
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_a_moved_level_fails_the_spec(precision, closure):
    """One level of one column of the output moved by 4 x bound_k / |diag_k|: a flat column, a column next to the step, the 1x1
    system, the column at i = 0; the bottom level, a middle one, the top one."""
    g, dzc, dzf, before, after, u_ = oracle_solve(precision, "made", closure, 33)
    Nz, H = g["Nz"], g["H"]
    kfs = isp.first_free_levels(g)
    for n in isp.FIELDS:
        kw = dict(K=K_CONST) if closure == "const" else dict(kappa_u=before["kappa_u"], kappa_c=before["kappa_c"])
        Kf = isp.face_diffusivity(n, g, **kw)
        _, bound, dg = isp.solve_residual(ss.interior(before[n], g), ss.interior(after[n], g), Kf, DT, dzc, dzf, kfs[n], u_)
        for (i, j) in ((2, 2), (12, 3), (9, 6), (0, 5)):
            kf = int(kfs[n][i, j])
            for k in sorted({kf, (kf + Nz) // 2, Nz - 1}):
                moved = after[n].astype(np.longdouble)
                moved[H + i, H + j, H + k] += 4 * bound[i, j, k] / abs(dg[i, j, k])
                r, b2, _ = isp.solve_residual(ss.interior(before[n], g), ss.interior(moved, g), Kf, DT, dzc, dzf, kfs[n], u_)
                with pytest.raises(AssertionError):
                    ss.check(f"{n} moved at {(i, j, k)}", r, b2)
