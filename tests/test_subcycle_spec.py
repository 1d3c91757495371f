"""tests/subcycle_spec.py proved on the CPU oracle before tests/test_gpu_subcycle_spec.py judges the kernels by it.

The oracle (oracle/gb25_oracle.c, step_free_surface and step_free_surface_fold) runs the sub-cycle with true divisions and
separate products, half by half over whole arrays -- another order of operations than the fused kernels': a bound that holds
there in Float64 AND in Float32 is not tuned to the kernels.  And the spec must notice a wrong kernel: handed ONE mutation
(subcycle_spec.MUTATIONS), the same oracle output fails, and the message names the cell.

The sub-cycle is driven through ab2_step alone (drive): counter-rng noise on every cell of the parent arrays of eta (0.1 .. 1 m),
U, V (+-400 m2/s) and of Gn.u, Gn.v, Gm.u, Gm.v (+-1e-3 m/s2, which puts a signal on Gn.U, Gn.V) -- the halo cells hold
independent noise, the wall rows of V included (a kernel that reads one is seen).  Two conditions on these inputs are asserted
with every case: the propagated bound stays within 2 x the sum of the local bounds (dt is chosen for that: DT), and the change
of each field over the sub-cycle is at least 1e3 x its bound on at least 90 % of the wet cells."""
import functools

import numpy as np
import pytest

import gb25_amd as gb
import subcycle_spec as sc
from helpers import counter_rng
from oracle_backend import CPU

PRECISIONS = ["f64", "f32"]
# (grid, shape, halo); the folded grids need Ns + 3 = 24 rows
GRIDS = {"simple_lat_lon": ((20, 11, 4), 4), "gaussian_islands_lat_lon": ((48, 24, 6), 4), "lat_lon_as_curvilinear": ((20, 11, 4), 4),
         "tripolar": ((48, 24, 6), 8), "gaussian_islands": ((48, 24, 6), 8)}
SUBSTEPS = [30, 6, 14]                       # Ns = 21, 4, 10
# dt per (grid, substeps): the gravity-wave Courant number of a substep at the narrowest cell of the grid decides the growth of |A|
DT = {"simple_lat_lon": 300.0, "gaussian_islands_lat_lon": 100.0, "lat_lon_as_curvilinear": 300.0, "tripolar": 20.0, "gaussian_islands": 20.0}
AMPLITUDE = {"eta": None, "U": 400.0, "V": 400.0, "Gn.u": 1e-3, "Gn.v": 1e-3, "Gm.u": 1e-3, "Gm.v": 1e-3}
OUTPUTS = ("eta", "U", "V", "eta_bar", "U_bar", "V_bar", "Gn.U", "Gn.V")


def dt_of(grid, substeps):
    return DT[grid] * substeps / 30.0       # (dtau = 2 dt / substeps: the same dtau for every count)


def set_inputs(b, seed=0, halo_seed=None):
    """Noise on every cell of the parent arrays (AMPLITUDE); halo_seed: other noise in the halo cells of eta, U, V, the interior
    kept.  Returns the parents of eta, U, V as the model holds them."""
    dtype = b.dtype
    for q, (n, amp) in enumerate(AMPLITUDE.items()):
        shape = b.field_dims(n, True)
        r = counter_rng(shape, 700 + seed, q)
        a = 0.1 + 0.9 * r if amp is None else amp * (2 * r - 1)
        if halo_seed is not None and n in sc.FIELDS:
            H = (shape[0] - b.field_dims(n, False)[0]) // 2
            r2 = counter_rng(shape, 900 + halo_seed, q)
            other = 0.1 + 0.9 * r2 if amp is None else amp * (2 * r2 - 1)
            other[H:-H, H:-H] = a[H:-H, H:-H]
            a = other
        b.set_field(n, a.astype(dtype), True)
    return {n: b.get_field(n, True) for n in sc.FIELDS}


def drive(arch, grid, substeps, order, shape=None, halo=None, dt=None, seed=0, halo_seed=None, **options):
    """One ab2_step on a fresh model: (backend, geometry, parents before, parents after (OUTPUTS), dt)."""
    shape = shape or GRIDS[grid][0]
    halo = halo or GRIDS[grid][1]
    dt = dt or dt_of(grid, substeps)
    m = gb.baroclinic_instability_model(arch, *shape, dt=dt, halo=(halo,) * 3, grid_type=grid, substeps=substeps,
                                        **(dict(options=options) if options else {}))
    b = m.backend
    if order:
        b.set_option("substep_order", 1)
    g = sc.read_geometry(b, grid, shape, halo)
    before = set_inputs(b, seed, halo_seed)
    b.ab2_step(dt, False)
    after = {n: b.get_field(n, True) for n in OUTPUTS}
    return b, g, before, after, dt


def wet_faces(g):
    """{field: the cells / faces of the interior that are wet and stepped} (V: not the wall row 0, whose slope is zero)."""
    v = g["Hcf"] > 0
    v[:, 0] = False
    return {"eta": g["wet"], "U": g["Hfc"] > 0, "V": v}


def interior(a, g):
    H = g["H"]
    return np.asarray(a)[H:H + g["Nx"], H:H + g["Ny"], 0]


def assert_input_conditions(label, g, before, after, spec, growth):
    assert growth < 2.0, f"{label}: the propagated bound is {growth:.3f} x the sum of the local bounds: dt is too long for this grid"
    for n, wet in wet_faces(g).items():
        change = np.abs(interior(after[n], g).astype(np.longdouble) - interior(before[n], g).astype(np.longdouble))
        strong = (change >= 1e3 * spec[n][1]) & wet
        share = strong.sum() / max(int(wet.sum()), 1)
        assert share >= 0.9, f"{label}: {n} changes by 1e3 bounds on {100 * share:.1f} % of the wet cells only"


@functools.lru_cache(maxsize=None)
def oracle_case(precision, grid, substeps, order):
    b, g, before, after, dt = drive(CPU(precision), grid, substeps, order)
    sub, dtype = b.substepping(), b.dtype
    b.close()
    return g, before, after, dt, sub, dtype


@pytest.mark.parametrize("substeps", SUBSTEPS)
@pytest.mark.parametrize("grid", list(GRIDS))
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_the_oracle_stays_within_the_bound(precision, order, grid, substeps):
    g, before, after, dt, sub, dtype = oracle_case(precision, grid, substeps, order)
    label = f"oracle {precision} {grid} substeps {substeps} (Ns {sub[0]}) order {order}"
    assert sub[0] == {30: 21, 6: 4, 14: 10}[substeps]
    if g["immersed"]:
        assert g["wet"].any() and (~g["wet"]).any() and (g["Hfc"] != g["Hcf"]).any(), "an island grid has wet and dry columns"
    spec, growth = sc.subcycle(before, after["Gn.U"], after["Gn.V"], g, sub, dt, dtype, order)
    assert np.abs(interior(after["Gn.U"], g)).max() > 0 and np.abs(interior(after["Gn.V"], g)).max() > 0, "no forcing"
    assert_input_conditions(label, g, before, after, spec, growth)
    out = sc.measure(after, spec, g)
    print(f"[subcycle spec] {label}: growth {growth:.3f}, max residual / bound = " + ", ".join(f"{n} {r:.4f}" for n, (r, _) in out.items()))
    sc.judge(label, after, spec, g)
    H, Nx, Ny = g["H"], g["Nx"], g["Ny"]
    for n in sc.FIELDS:          # the filtered state holds the same averages, and nothing outside the interior moved
        assert np.array_equal(interior(after[n + "_bar"], g), interior(after[n], g)), n
        halo = np.ones(after[n].shape, bool)
        halo[H:H + Nx, H:H + Ny] = False
        assert np.array_equal(after[n][halo], before[n][halo]), f"{n}: a cell outside the interior changed"
    # V on the wall faces is exactly what the spec gives: the face row Ny of an unfolded grid is not stepped and keeps its bits
    # (checked above); on row 0 the slope is zero and so is G.V, every substep returns V, and the residual is that of the average
    assert not np.any(interior(after["Gn.V"], g)[:, 0]), "G.V on the southern wall faces"
    r, bound = sc.residuals(after, spec, g)["V"]
    sc.check(f"{label}: V on the southern wall faces", r[:, :1], bound[:, :1])


# ---- the spec must notice a wrong kernel --------------------------------------------------------------------------------------
# mutation -> the grid it is shown on
MUTATION_GRID = {"weights shifted by one substep": "simple_lat_lon", "one substep fewer": "simple_lat_lon", "the other half order": "simple_lat_lon",
                 "dxf[j] for dxf[j+1] in the V flux": "simple_lat_lon", "azc of the row above": "simple_lat_lon",
                 "northern wall open": "simple_lat_lon", "southern wall open": "simple_lat_lon", "dye not zero on row 0": "simple_lat_lon",
                 "east neighbour of column Nx-1 clamped": "simple_lat_lon", "G.U dropped": "simple_lat_lon",
                 "Hfc and Hcf exchanged": "gaussian_islands_lat_lon", "the cell's own depth": "gaussian_islands_lat_lon",
                 "image column of U as Nx-i+1": "gaussian_islands", "sign of the U images not flipped": "tripolar",
                 "V image row off by one": "gaussian_islands"}
assert set(MUTATION_GRID) == set(sc.MUTATIONS)


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("mutation", sc.MUTATIONS)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_mutated_spec_fails_on_the_same_output(precision, mutation, order):
    grid = MUTATION_GRID[mutation]
    g, before, after, dt, sub, dtype = oracle_case(precision, grid, 30, order)
    spec, _ = sc.subcycle(before, after["Gn.U"], after["Gn.V"], g, sub, dt, dtype, order)
    sc.judge("unmutated", after, spec, g)
    wrong, _ = sc.subcycle(before, after["Gn.U"], after["Gn.V"], g, sub, dt, dtype, order, mutation=mutation)
    with pytest.raises(AssertionError, match=r"behind the sub-cycle.*at cell \(\d+, \d+\)"):
        sc.judge(mutation, after, wrong, g)


@pytest.mark.parametrize("grid", ["simple_lat_lon", "gaussian_islands"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_moved_output_cell_fails_the_spec(precision, grid):
    """One cell of the output moved by four bounds, away from zero: a middle cell, the corners, the cell beside each wall and the
    pivot row -- for each field."""
    g, before, after, dt, sub, dtype = oracle_case(precision, grid, 30, 0)
    spec, _ = sc.subcycle(before, after["Gn.U"], after["Gn.V"], g, sub, dt, dtype, 0)
    H, Nx, Ny = g["H"], g["Nx"], g["Ny"]
    res = sc.residuals(after, spec, g)
    for n in sc.FIELDS:
        r, bound = res[n]
        for (i, j) in ((Nx // 2, Ny // 2), (0, 0), (Nx - 1, Ny - 1), (0, Ny - 1), (Nx - 1, 0), (3, 1)):
            if not bound[i, j] > 0:
                continue
            moved = {k: v for k, v in after.items()}
            a = after[n].astype(np.longdouble)
            a[H + i, H + j, 0] += 4 * bound[i, j] * (1 if r[i, j] >= 0 else -1)
            moved[n] = a
            with pytest.raises(AssertionError, match=r"%s behind the sub-cycle.*at cell \(%d, %d\)" % (n, i, j)):
                sc.judge("moved", moved, spec, g)
