"""Surface forcing and bottom drag on the device, cell by cell: tests/forcing_spec.py (proved on the CPU oracle by
tests/test_forcing_spec.py, whose atlas, ocean and judges are used here) applied to what a caller reads, in both builds.

(a) k_similarity_fluxes + k_stress_to_faces: the atlas about the updated ocean, compute_atmosphere_ocean_fluxes, top_flux of u, v,
    T, S in full, at (64, 8, 6) (the Nx + 1 columns of threads spill one column into a second block), (70, 13, 6) (a ragged block,
    odd Ny), (130, 9, 6) (three blocks, a one-row last block), on the four grids (folded ones at Ny = 24: test_forcing_spec).
    Float64: every cell within 1e-10 of the field's scale of the fp64 statement.  Float32: per field and regime, the worst
    deviation (less one u32 of the value for the store) within 4 x the yardstick -- the statement's own float32 iteration
    against its float64 one on the same inputs.  Land, faces between land, the unwritten row of J^v: exact zeros.
    The halo cells west and south are read: other values there change J^u in column 0 and J^v in row 0 and no other bit.
(b) where the tendency kernels put the fluxes: Gn.u, v, T, S of one state three ways (no boundary flux, host-set top fluxes, the
    bottom drag alone); untouched cells keep their bits, touched ones carry forcing_spec.boundary_contribution within
    forcing_spec.application_bound; the drag flux is read off the difference.  Instances: INSTANCES below.  What tells the
    instance: the advection order and the chunk-level options read back from the model (options, not the plan: the library
    reports neither the chunks of a launch nor the rows per lane; tests/test_gpu_tracer_rows.py says how the latter is known),
    and one timed scope of each tendency kernel per evaluation.
    NOT judged: the tails of the instances that carry w on the fly.  Only a composite step selects them (the route of a
    time step inside a loop); update_state, the one call after which the tendencies of a known state can be read three ways,
    always runs the stand-alone w and the instances without it, whatever w_on_the_fly says.
(c) the coupled order: update_state after the stand-alone flux solve puts its fluxes into the tendencies per (b) (that top_flux
    keeps its bits there only says that update_state does not solve again: it never calls the flux solve).  Then first_time_step,
    whose last act IS the flux solve: the top_flux it leaves is judged as in (a) from the state it leaves, and a stand-alone
    solve from that state returns the same bits.

Measured on the MI355X, Float32: the largest (deviation - u32 |value|) / yardstick over the twelve cases of (a) and the halo and
coupled cases (printed per case by judge_case; the yardsticks themselves are 0.5e-7 .. 4e-7 of a field's scale, test_forcing_spec
prints them); the assertion is forcing_spec.FACTOR_F32 = 4:
              unstable   stable   clamped   gust_floor   lq_cap
    J^u         1.90      1.37     1.14       1.37        1.14
    J^v         1.76      1.38     1.60       1.38        1.60
    J^T         1.59      1.41     1.53       1.41        1.53
    J^S         1.93      1.55     1.52       1.55        1.52
No regime needs more than 2: the device's single-precision log / pow / atan / cbrt / exp cost no more than numpy's, and neither the
clamps at zeta = +-50 nor the 0.11 nu / u* term of weakly driven cells lose the answer.  In (b) the worst |difference| / bound was
0.33 (Float32) and 0.51 (Float64) over every instance run, and in Float32 the drag flux is read off the tendencies to within 4e-5
(u) / 8e-5 (v) of itself in the median cell, 0.5 where the drag is lost under the tendency; in Float64 to within 1e-13 (worst 7e-10).

Not judged: the w-on-the-fly instances (above), slabs and mesh ranks (tied to the single domain bit for bit by tests/test_gpu_data_free.py, test_gpu_bottom_drag.py,
test_gpu_fluxes.py), more than five iterations, kernels = 1 (refuses flux boundary conditions: tests/test_gpu_fluxes.py)."""
import os

import numpy as np
import pytest

import gb25_amd as gb
import forcing_spec as fs
import step_spec as ss
import test_forcing_spec as tfs

pytestmark = pytest.mark.gpu

BUILDS = ["Float32", "Float64"]


def dtype_of(float_type):
    return np.float32 if float_type == "Float32" else np.float64


def judge_case(label, case, float_type, every_regime=True):
    """(a) for one solved case; returns {(field, regime): deviation / yardstick} in Float32, {field: worst ratio} in Float64.
    every_regime = False: a regime the case does not reach is passed over (coverage is asserted on the cases of (a))."""
    want, regimes = tfs.statement(case)
    got = case["got"]
    tfs.exact_facts(label, case, got, want, regimes)
    out = {}
    if float_type == "Float64":
        for n in tfs.FLUXES:
            out[n] = fs.judge_flux(label, n, got[n], want[n], fs.regimes_at(regimes, n, want[n].shape[1]))
        return out
    y = tfs.yardstick(case)
    bad = []
    for n in tfs.FLUXES:
        assert got[n].dtype == np.float32 and got[n].shape == want[n].shape
        scale = np.abs(want[n]).max()
        excess = np.maximum(np.abs(got[n].astype(np.float64) - want[n]) - ss.U32 * np.abs(want[n]), 0) / scale
        for r, mask in fs.regimes_at(regimes, n, want[n].shape[1]).items():
            if r == "land":
                continue
            if not every_regime and not mask.any():
                continue
            assert mask.any() and y[n, r] > 0, (label, n, r)
            at = np.unravel_index(int(np.argmax(np.where(mask, excess, -1))), excess.shape)
            out[n, r] = float(excess[at] / y[n, r])
            if out[n, r] > fs.FACTOR_F32:
                bad.append(f"J^{n} {r} at {tuple(int(q) for q in at)}: {out[n, r]:.3g} x the yardstick {y[n, r]:.3g}")
    print(f"{label}: deviation / yardstick  " + "  ".join(f"{n}:{r} {v:.2f}" for (n, r), v in out.items()))
    assert not bad, f"{label}: " + "; ".join(bad)
    return out


@pytest.mark.parametrize("grid,shape", tfs.CASES)
@pytest.mark.parametrize("float_type", BUILDS)
def test_the_flux_solve_cell_by_cell(float_type, grid, shape):
    m, case = tfs.solved(gb.GPU(float_type=float_type), grid, shape)
    try:
        assert m.backend.dtype == dtype_of(float_type)
        if case["g"]["immersed"]:
            assert (case["g"]["kbot"] >= case["g"]["Nz"]).sum() >= 16
        judge_case(f"{float_type} {grid} {tfs.shape_on(grid, shape)}", case, float_type)
    finally:
        m.backend.close()


@pytest.mark.parametrize("grid", ["simple_lat_lon", "gaussian_islands"])
@pytest.mark.parametrize("float_type", BUILDS)
def test_the_halo_cells_west_and_south_are_read(float_type, grid):
    """(70, 13, 6) a second time with other values in the halo cells west of column 0 and south of row 0 (atmosphere and u, v, T,
    S): the statement still holds, J^u changes in column 0, J^v in row 0, and every other cell of the four fluxes keeps its bits.
    (The folded grid needs no extra row: j_hi = Ny stops the kernel below the fold.)"""
    runs = []
    for halo_seed in (None, 1):
        m, case = tfs.solved(gb.GPU(float_type=float_type), grid, (70, 13, 6), halo_seed=halo_seed)
        try:
            judge_case(f"{float_type} {grid} halo cells {halo_seed}", case, float_type)
            runs.append(case)
        finally:
            m.backend.close()
    a, b = (c["got"] for c in runs)
    label = f"{float_type} {grid}"
    assert not np.array_equal(a["u"][0, :], b["u"][0, :]), f"{label}: J^u in column 0 does not read the halo column west of it"
    assert not np.array_equal(a["v"][:, 0], b["v"][:, 0]), f"{label}: J^v in row 0 does not read the halo row south of it"
    # (a calm halo cell beside a driven one can change the half-sum by less than a rounding: most faces change, not all)
    land = fs.surface_land(runs[0]["g"])
    between_land = land[0, 1:] & land[1, 1:]
    changed = a["u"][0, :] != b["u"][0, :]
    assert not changed[between_land].any() and changed[~between_land].sum() > 0.5 * (~between_land).sum(), f"{label}: J^u in column 0"
    assert (a["v"][:, 0] != b["v"][:, 0]).sum() > 0.5 * a["v"].shape[0], f"{label}: J^v in row 0"
    assert np.array_equal(tfs.bits(a["u"][1:]), tfs.bits(b["u"][1:])), f"{label}: J^u changes away from column 0"
    assert np.array_equal(tfs.bits(a["v"][:, 1:]), tfs.bits(b["v"][:, 1:])), f"{label}: J^v changes away from row 0"
    for n in ("T", "S"):
        assert np.array_equal(tfs.bits(a[n]), tfs.bits(b[n])), f"{label}: J^{n} depends on a halo cell"


# ---- (b) ------------------------------------------------------------------------------------------------------------------------------
CHUNKS = dict(momentum_chunk_levels=12, tracer_chunk_levels=12)        # Nz = 25: two chunks, 13 + 12 levels
INSTANCES = {
    "flat": dict(grid="simple_lat_lon"),
    "flat, two rows per lane": dict(grid="simple_lat_lon", rows=2),
    "WENO7 tracers": dict(grid="simple_lat_lon", order=7),
    "islands lat-lon": dict(grid="gaussian_islands_lat_lon"),
    "curvilinear": dict(grid="lat_lon_as_curvilinear"),
    "folded with islands": dict(grid="gaussian_islands"),
    "islands lat-lon, two chunks": dict(grid="gaussian_islands_lat_lon", Nz=25, options=CHUNKS),
    "folded with islands, two chunks": dict(grid="gaussian_islands", Nz=25, options=CHUNKS),
    "flat, two chunks": dict(grid="simple_lat_lon", Nz=25, options=CHUNKS),
}


def instance_model(float_type, grid, Nz=6, rows=None, order=None, options=None):
    before = os.environ.get("GB25_TRACER_ROWS")
    if rows:
        os.environ["GB25_TRACER_ROWS"] = str(rows)
    try:
        m, g = tfs.build(gb.GPU(float_type=float_type), grid, (70, 13, Nz), **(options or {}))
    finally:
        if rows:
            if before is None:
                del os.environ["GB25_TRACER_ROWS"]
            else:
                os.environ["GB25_TRACER_ROWS"] = before
    b = m.backend
    if order:
        b.set_tracer_advection_order(order)
    assert b.dtype == dtype_of(float_type) and b.tracer_advection_order() == (order or 5)
    for n, v in (options or {}).items():
        assert b.get_option(n) == v, (n, b.get_option(n), v)
    return m, g


@pytest.mark.parametrize("name", list(INSTANCES))
@pytest.mark.parametrize("float_type", BUILDS)
def test_where_the_tendency_kernels_put_the_fluxes(float_type, name):
    spec = INSTANCES[name]
    m, g = instance_model(float_type, **spec)
    b = m.backend
    try:
        Nz = g["Nz"]
        if Nz == 25:
            if g["immersed"]:
                ku, kv = fs.first_free_levels(g)
                for k in (ku, kv):
                    assert (k < 13).any() and ((k >= 13) & (k < Nz)).any(), "first free levels must fall in both chunks"
        tfs.set_ocean(m, g)
        b.profile_enable(True)
        scopes = []

        def evaluate(model):
            b.profile_reset()
            gb.update_state(model)
            scopes.append((b.profile_get("gu")[0], b.profile_get("tracers")[0]))

        out, J, vel = tfs.three_ways(m, g, evaluate)
        assert scopes == [(1, 1)] * 3, scopes
        tfs.judge_three_ways(f"{float_type} {name}", g, out, J, vel, dtype_of(float_type))
    finally:
        b.close()


# ---- (c) ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("float_type", BUILDS)
def test_the_coupled_call_order(float_type):
    """Folded grid with islands (module docstring, (c))."""
    grid, shape = "gaussian_islands", (70, 13, 6)
    m, g = tfs.build(gb.GPU(float_type=float_type), grid, shape)
    b = m.backend
    try:
        ocean = tfs.set_ocean(m, g)
        without = tfs.tendencies(m, g)
        atm = tfs.atlas(g, ocean)
        tfs.set_atmosphere(m, atm)
        b.compute_atmosphere_ocean_fluxes()
        case = dict(g=g, ocean=ocean, atm=atm, got={n: np.array(b.top_flux(n)) for n in tfs.FLUXES})
        label = f"{float_type} coupled"
        judge_case(label, case, float_type)
        gb.update_state(m)
        for n in ("u", "v", "T", "S"):
            assert np.array_equal(tfs.bits(ocean[n]), tfs.bits(b.get_field(n, True))), f"{label}: update_state moved {n}"
            assert np.array_equal(tfs.bits(b.top_flux(n)), tfs.bits(case["got"][n])), f"{label}: update_state changed the top flux of {n}"
        with_ = tfs.tendencies(m, g)
        inc, touched = fs.boundary_contribution(case["got"], None, g)
        u_ = ss.unit_roundoff(b.dtype)
        for n in tfs.FLUXES:
            assert touched[n].any()
            tfs.judge_application(label, n, without[n], with_[n], inc[n], touched[n], u_)
        # the flux solve as a step runs it
        b.set_dt(30.0)
        gb.first_time_step(m)
        after = {n: b.get_field(n, True) for n in ("u", "v", "T", "S")}
        assert not np.array_equal(after["T"], ocean["T"]) and np.isfinite(after["u"]).all()
        in_step = {n: np.array(b.top_flux(n)) for n in tfs.FLUXES}
        assert not np.array_equal(in_step["T"], case["got"]["T"]), f"{label}: the step did not solve the fluxes again"
        judge_case(label + " in the step", dict(g=g, ocean=after, atm=atm, got=in_step), float_type, every_regime=False)
        b.compute_atmosphere_ocean_fluxes()
        for n in tfs.FLUXES:
            assert np.array_equal(tfs.bits(b.top_flux(n)), tfs.bits(in_step[n])), f"{label}: J^{n} of the step is not the stand-alone solve of the state it left"
    finally:
        b.close()
