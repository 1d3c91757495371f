"""The implicit vertical solves on the device, cell by cell: tests/implicit_spec.py (proved on the CPU oracle by
tests/test_implicit_spec.py, whose inputs and drive are used here) applied to the fields a caller reads before and after ONE
gb25_ab2_step with zero tendencies -- the step is then the solve alone, and with CATKE the diffusivities are the ones this
test set, halos included (no update_state runs in between).

Kernel forms (form_of names the one a case takes):
  constant K    k_implicit_vertical_reg<32|48|64|128> (Nz <= 128, factors from the host's table), k_implicit_vertical (deeper:
                the column in LDS; at (70, 13) every such launch needs more than 64 KB and takes the raised attribute);
  kappa fields  k_implicit_vertical_var<32|48|64> MODE 0 (u, v) and MODE 1 (T with S, one elimination), and
                k_implicit_vertical_var_stream above 64 levels in Float32, above 32 in Float64;
each flat and immersed (the made bottom of tests/test_implicit_spec.py: a dry column, a 1x1 system, steps in x and y, raised
columns at i = 0 and Nx-1 and on the wall rows; the built-in island grids; the folded grid).  (70, 13, Nz): one ragged 64-wide
tile, odd Ny, every row next to a wall.

Not covered here: the e slice of MODE 1 (kappa_e, -dt L^e on the diagonal, src_e).  tests/test_gpu_catke_spec.py judges it cell by
cell (tests/test_catke_spec.py on the oracle): e* is rebuilt from the total tendency k_catke_tke_step leaves in G^-.e, and
L^e <= 0 by construction keeps the system diagonally dominant.

Also here: the cache key (dt, K) of the host's factor table; T and S through one elimination (S does not change by a bit when
T's input does); and the column integrals the solve kernels rewrite for the corrector -- phase by phase (the corrected column
carries U, V) and over whole steps (continuity and masks after every call), with both chunkings of the sums.  The AB2 update
identities of step_spec.check_step do not hold with a closure (the solve sits between them) and are not asserted.
Every test prints its largest residual / bound; the bound is the derived one (implicit_spec's docstring)."""
import numpy as np
import pytest

import gb25_amd as gb
import implicit_spec as isp
import step_spec as ss
import test_implicit_spec as tis
from helpers import counter_rng, set_noisy_state_with_halos

pytestmark = pytest.mark.gpu

BUILDS = ["Float32", "Float64"]
CONST_NZ = [6, 32, 33, 48, 49, 64, 65, 128, 129, 160]
CATKE_NZ = [6, 32, 33, 48, 49, 64, 65, 100]
SOLVES = [(ft, "const", grid, Nz) for ft in BUILDS for grid in ("flat", "made") for Nz in CONST_NZ]
SOLVES += [(ft, "const", grid, Nz) for ft in BUILDS for grid in ("islands", "folded") for Nz in (6, 129)]
SOLVES += [(ft, "catke", grid, Nz) for ft in BUILDS for grid in ("flat", "made", "folded") for Nz in CATKE_NZ]
SOLVES += [(ft, "catke", "islands", Nz) for ft in BUILDS for Nz in (6, 65, 100)]


def shape_of(grid, Nz):
    return (70, 13, Nz) if grid in ("flat", "made") else (48, 24, Nz)


def form_of(float_type, closure, Nz):
    if closure == "const":
        return "LDS" if Nz > 128 else "reg<%d>" % next(n for n in (32, 48, 64, 128) if Nz <= n)
    limit = 64 if float_type == "Float32" else 32
    return "stream" if Nz > limit else "var<%d>" % next(n for n in (32, 48, 64) if Nz <= n)


def report(label, out):
    print(f"[implicit solve] {label}: max residual / bound = " + ", ".join(f"{k} {v:.4f}" for k, v in out.items()))


@pytest.mark.parametrize("float_type,closure,grid,Nz", SOLVES)
def test_the_solve_cell_by_cell(float_type, closure, grid, Nz):
    m, g, dzc, dzf, before, after = tis.drive(gb.GPU(float_type=float_type), grid, shape_of(grid, Nz), closure)
    b = m.backend
    label = f"{float_type} {closure} {form_of(float_type, closure, Nz)} {grid} Nz {Nz}"
    try:
        assert b.dtype == (np.float32 if float_type == "Float32" else np.float64)
        if grid != "flat":
            assert (g["kbot"] > 0).any() and (g["kbot"] == 0).any(), "an immersed grid must have wet and dry cells"
        for n in isp.FIELDS:
            assert not np.array_equal(before[n], after[n]), f"{label}: the solve did nothing to {n}"
        tis.judge(label, before, after, g, tis.DT, dzc, dzf, ss.unit_roundoff(b.dtype), closure)
    finally:
        b.close()


@pytest.mark.parametrize("Nz", [33, 129])
@pytest.mark.parametrize("float_type", BUILDS)
def test_the_factor_table_follows_dt_and_K(float_type, Nz):
    """One model, four solves: (dt, K), (dt / 3, K), then other values through set_vertical_diffusivity with dt / 3 and with dt
    again -- each judged with ITS dt and K (Nz = 33: the table the host caches under (dt, K); 129: the LDS kernel, which has none)."""
    m, g, dzc, dzf = tis.build(gb.GPU(float_type=float_type), "made", shape_of("made", Nz), "const")
    b = m.backend
    u_, t = ss.unit_roundoff(b.dtype), np.dtype(b.dtype).type
    nu, kappa = tis.K_CONST, tis.K_CONST
    try:
        for call, (dt, change) in enumerate(((tis.DT, None), (tis.DT / 3, None), (tis.DT / 3, (0.3, 7.5)), (tis.DT, None))):
            if change:
                b.set_vertical_diffusivity(*change)
                nu, kappa = (float(t(x)) for x in change)          # (the numbers of the build)
            before = tis.set_inputs(m, g, dzf, dt, "const", seed=call)
            b.ab2_step(dt, True)
            after = {n: b.get_field(n, True) for n in isp.FIELDS}
            label = f"{float_type} {form_of(float_type, 'const', Nz)} call {call}: dt {dt:g}, nu {nu:g}, kappa {kappa:g}"
            tis.judge(label, before, after, g, dt, dzc, dzf, u_, "const", K=nu, fields=("u", "v"))
            tis.judge(label, before, after, g, dt, dzc, dzf, u_, "const", K=kappa, fields=("T", "S"))
    finally:
        b.close()


@pytest.mark.parametrize("Nz", [33, 100])
@pytest.mark.parametrize("float_type", BUILDS)
def test_T_and_S_share_one_elimination(float_type, Nz):
    """MODE 1: one elimination, two right-hand sides.  Both are judged, and S's result does not change by a bit when T's input
    is replaced (Nz = 33: the register kernel in Float32, the streamed one in Float64; 100: streamed in both)."""
    results = []
    for other_T in (False, True):
        m, g, dzc, dzf = tis.build(gb.GPU(float_type=float_type), "made", shape_of("made", Nz), "catke")
        b = m.backend
        try:
            before = tis.set_inputs(m, g, dzf, tis.DT, "catke")
            if other_T:
                m.set(T=(3.0 + 5 * counter_rng(b.field_dims("T", False), 7, 7)).astype(b.dtype))
                before["T"] = b.get_field("T", True)
            b.ab2_step(tis.DT, True)
            after = {n: b.get_field(n, True) for n in isp.FIELDS}
            label = f"{float_type} catke {form_of(float_type, 'catke', Nz)} Nz {Nz}, {'another' if other_T else 'the'} T"
            tis.judge(label, before, after, g, tis.DT, dzc, dzf, ss.unit_roundoff(b.dtype), "catke", fields=("T", "S"))
            results.append((before, after))
        finally:
            b.close()
    (b0, a0), (b1, a1) = results
    assert np.array_equal(b0["S"], b1["S"]) and not np.array_equal(b0["T"], b1["T"]) and not np.array_equal(a0["T"], a1["T"])
    assert np.array_equal(a0["S"], a1["S"]), "S depends on T's right-hand side"


# ---- the column integrals the solve rewrites ----------------------------------------------------------------------------------
# one register form and one LDS / streamed form per closure, in both builds
SUM_FORMS = [("const", 20), ("const", 130), ("catke", 20), ("catke", 70)]
PHASES = [(ft, c, Nz, grid, chunk) for ft in BUILDS for c, Nz in SUM_FORMS for grid in ("flat", "made") for chunk in (0, 7)]


@pytest.mark.parametrize("float_type,closure,Nz,grid,chunk", PHASES)
def test_the_corrected_column_carries_the_transport(float_type, closure, Nz, grid, chunk):
    """ab2_step (the solve rewrites colsum and, where they exist, the chunk partials), fill_halo_regions, the corrector: the
    corrected columns carry U and V (step_spec.transport with its own bound), whichever way the sums are chunked."""
    shape = shape_of(grid, Nz)
    m, g, dzc, dzf = tis.build(gb.GPU(float_type=float_type), grid, shape, closure, **(dict(momentum_chunk_levels=chunk) if chunk else {}))
    b = m.backend
    try:
        if chunk:
            assert b.get_option("momentum_chunk_levels") == chunk
        u_ = ss.unit_roundoff(b.dtype)
        tis.set_inputs(m, g, dzf, tis.DT, closure)
        for q, n in enumerate(("U", "V")):            # transports of order the columns' own: depth x velocity
            a = 4000 * (2 * counter_rng(b.field_dims(n, False), 500, q) - 1)
            if n == "V":
                a[:, 0] = a[:, -1] = 0
            b.set_field(n, a.astype(b.dtype), False)
        b.ab2_step(tis.DT, True)
        b.fill_halo_regions()
        star = {n: ss.interior(b.get_field(n, True), g) for n in ("u", "v")}
        b.correct_velocities_and_cache_previous_tendencies(tis.DT)
        wet, wu, wv = ss.wet_levels(g)
        rc, rv = ss.compared_rows(g)
        out = {}
        label = f"{float_type} {closure} {form_of(float_type, closure, Nz)} {grid} Nz {Nz} chunk {chunk}"
        for n, N, wetf, rows in (("u", "U", wu, rc), ("v", "V", wv, rv)):
            after = ss.interior(b.get_field(n, True), g)
            d = ss._ld(after) - ss._ld(star[n])
            r, bound, dcol = ss.column_spread(d, u_ * np.abs(ss._ld(after)), wetf)
            out[n + " spread"] = ss.check(f"{label}: correction of {n} within its column", r[:, rows], bound[:, rows], origin=(0, rows.start, 0))
            assert np.abs(dcol[:, rows]).max() > 0, f"{label}: the corrector did nothing to {n}"
            r, bound = ss.transport(after, ss.interior(b.get_field(N, True), g), g["dz"], u_, dcol, wetf)
            out[n + " transport"] = ss.check(f"{label}: transport of the corrected {n}", r[:, rows], bound[:, rows], origin=(0, rows.start))
        report(label, out)
    finally:
        b.close()


ROUTES = {"sweep": dict(subcycle_lookahead=1, lazy_corrector=0, w_on_the_fly=0),
          "lazy+wfly": dict(subcycle_lookahead=1, lazy_corrector=1, w_on_the_fly=1)}
STEPS = [(ft, c, Nz, grid, chunk, route) for ft in BUILDS for c, Nz in SUM_FORMS for route in ROUTES
         for grid, chunk in (("simple_lat_lon", 0), ("simple_lat_lon", 7), ("gaussian_islands_lat_lon", 0))]


@pytest.mark.parametrize("float_type,closure,Nz,grid,chunk,route", STEPS)
def test_continuity_and_masks_over_whole_steps_with_a_closure(float_type, closure, Nz, grid, chunk, route):
    """first_time_step, time_step, loop(3) with the closure on: after each call w is the one of the velocities the step left
    behind (continuity over the written range of w) and the masks hold -- the corrector and w on the fly take the column
    integrals and the chunk partials from the solve kernels."""
    shape, halo, dt = (70, 13, Nz), 8, 300.0
    cl = gb.CATKEVerticalDiffusivity() if closure == "catke" else gb.VerticalScalarDiffusivity(nu=5.0, kappa=0.5)
    m = gb.baroclinic_instability_model(gb.GPU(float_type=float_type), *shape, dt=dt, halo=(halo,) * 3, grid_type=grid, closure=cl,
                                        options=dict(ROUTES[route], **(dict(momentum_chunk_levels=chunk) if chunk else {})))
    b = m.backend
    try:
        set_noisy_state_with_halos(m)
        g = ss.read_geometry(b, grid, shape, halo)
        u_ = ss.unit_roundoff(b.dtype)
        label = f"{float_type} {closure} {form_of(float_type, closure, Nz)} {grid} Nz {Nz} chunk {chunk} {route}"
        out = {}
        for call, run in (("first_time_step", lambda: gb.first_time_step(m)), ("time_step", lambda: gb.time_step(m)), ("loop(3)", lambda: gb.loop(m, 3))):
            run()
            s = ss.read_state(b)
            assert all(np.isfinite(a).all() for a in s.values()) and np.abs(s["w"]).max() > 0, f"{label} after {call}: no flow to speak about"
            out[call] = ss.check_state(s, g, u_, f"{label} after {call}")["continuity"]
        report(label + ", continuity", out)
    finally:
        b.close()
