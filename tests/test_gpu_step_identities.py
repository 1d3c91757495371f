"""What a step does around the tendencies, cell by cell, on the device: tests/step_spec.py (proved on the CPU oracle by
tests/test_step_spec.py) applied to the fields a caller reads before and after one ABI call.

  continuity      w[k+1] - w[k] + D_k / Az at every column and row w is written on (-H+1 .. N+H-2, halo cells included), w[0] = 0;
  masks           u, v, w, T, S exactly zero where the bottom or a wall says so, V zero on the wall faces;
  AB2 update      T, S at every wet cell; u, v: the correction d is one number per column, zero on dry levels;
  corrector       the corrected column carries the new transport U, V;
  column sums     Gn.U, Gn.V and U_bar, V_bar of the phase-by-phase drive, with both chunkings.

Every route of a step is driven: the sweeping corrector, the corrector inside its consumers or through the tracer kernel
(lazy_corrector), w carried by the tendency kernels (w_on_the_fly), the step without the AB2 look-ahead, one and two rows
per lane of the tracer kernel.  The bounds are operation counts (step_spec's docstring); every test prints the largest
residual / bound per identity.

Stale w.  DESIGN.md ("Which kernel corrects u, v") lets the field w go stale only INSIDE gb25_loop: its return, and every step
that sweeps, recomputes it.  So no call returns with a stale w, and continuity is asserted after every call of every route;
test_update_state_changes_nothing_after_a_step adds that a following update_state changes no field at all.
"""
import functools
import os

import numpy as np
import pytest

import gb25_amd as gb
import step_spec as ss
from helpers import set_noisy_state_with_halos

pytestmark = pytest.mark.gpu

BUILDS = ["Float32", "Float64"]
# (70, 13, 7): two ragged tiles of 63, odd Ny, every row next to a wall; (40, 21, 6): narrow halo, Nx below a tile; (16, 9, 4): the
# minimum size; (150, 70, 25) with chunks of 12 levels in both tendency kernels: the column sums and w are carried across chunks
SHAPES = {"ragged": ((70, 13, 7), 8, {}), "narrow": ((40, 21, 6), 4, {}), "tiny": ((16, 9, 4), 4, {}),
          "chunks": ((150, 70, 25), 8, dict(tracer_chunk_levels=12, momentum_chunk_levels=12))}
LATLON = ("simple_lat_lon", "gaussian_islands_lat_lon", "lat_lon_as_curvilinear")
GRID_SHAPES = [(g, s) for g in LATLON for s in SHAPES] + [("gaussian_islands", "folded")]
ROUTES = {"sweep": dict(subcycle_lookahead=1, lazy_corrector=0, w_on_the_fly=0),
          "lazy": dict(subcycle_lookahead=1, lazy_corrector=1, w_on_the_fly=0),
          "wfly": dict(subcycle_lookahead=1, lazy_corrector=0, w_on_the_fly=1),
          "lazy+wfly": dict(subcycle_lookahead=1, lazy_corrector=1, w_on_the_fly=1),
          "no look-ahead": dict(ab2_lookahead=0)}
# (the corrector inside its consumers exists for the flat lat-lon grid only: on the other grids "lazy" without w on the fly is the
# sweep again -- DESIGN.md, "Which kernel corrects u, v" -- and is not run twice; "lazy+wfly" there is the corrector through the tracer kernel)
CONFIGS = [(ft, g, s, r, 0) for ft in BUILDS for g, s in GRID_SHAPES for r in ("sweep", "lazy", "wfly", "lazy+wfly")
           if r != "lazy" or g == "simple_lat_lon"]
CONFIGS += [(ft, g, "ragged", "no look-ahead", 0) for ft in BUILDS for g in LATLON]
CONFIGS += [(ft, "simple_lat_lon", "ragged", r, rows) for ft in BUILDS for r in ("sweep", "lazy+wfly") for rows in (1, 2)]
IDS = ["%s-%s-%s-%s-rows%d" % c for c in CONFIGS]
CALLS = ("update_state", "first_time_step", "time_step", "last step of loop(4)", "time_step after the loop", "update_state again")


def shape_of(grid, shape_name):
    if grid == "gaussian_islands":
        return (144, 64, 6), 8, {}, 60.0
    return SHAPES[shape_name] + (300.0,)


def make_model(float_type, grid, shape_name, route, rows):
    shape, halo, extra, dt = shape_of(grid, shape_name)
    before = os.environ.get("GB25_TRACER_ROWS")
    if rows:
        os.environ["GB25_TRACER_ROWS"] = str(rows)
    try:
        m = gb.baroclinic_instability_model(gb.GPU(float_type=float_type), *shape, dt=dt, halo=(halo,) * 3, grid_type=grid,
                                            options=dict(extra, **ROUTES[route]))
    finally:
        if rows and before is None:
            del os.environ["GB25_TRACER_ROWS"]
        elif rows:
            os.environ["GB25_TRACER_ROWS"] = before
    set_noisy_state_with_halos(m)
    return m


def same_bits(a, b):
    return [n for n in a if not np.array_equal(a[n], b[n])]


@functools.lru_cache(maxsize=None)
def driven(config):
    """One model per configuration (and its twin, which stops one step short of the loop), driven through CALLS.  Nothing is
    asserted here: {call: {identity: worst ratio}}, {call: largest |d|} and the list of failures, for the tests to judge."""
    float_type, grid, shape_name, route, rows = config
    shape, halo, _, dt = shape_of(grid, shape_name)
    a, t = (make_model(*config) for _ in range(2))
    b = a.backend
    g = ss.read_geometry(b, grid, shape, halo)
    u_ = ss.unit_roundoff(b.dtype)
    ratios, signal, failures, w_max = {}, {}, [], {}
    b.profile_enable(True)

    def judge(call, before, after, euler=False):
        label = f"{'-'.join(str(c) for c in config)} after {call}"
        w_max[call] = float(np.abs(after["w"]).max())
        try:
            ratios[call] = ss.check_state(after, g, u_, label)
        except AssertionError as e:
            failures.append(("state", str(e)))
        if before is not None:
            try:
                out, signal[call] = ss.check_step(before, after, g, dt, *ss.ab2_coefficients(b.cfg.chi, euler, b.dtype), u_, label)
                ratios.setdefault(call, {}).update(out)
            except AssertionError as e:
                failures.append(("step", str(e)))

    for m in (a, t):
        gb.update_state(m)
    s0 = ss.read_state(b)
    judge(CALLS[0], None, s0)
    for m in (a, t):
        gb.first_time_step(m)
    s1 = ss.read_state(b)
    judge(CALLS[1], s0, s1, euler=True)
    for m in (a, t):
        gb.time_step(m)
    s2 = ss.read_state(b)
    judge(CALLS[2], s1, s2)
    twin_differs = same_bits(s2, ss.read_state(t.backend))
    gb.loop(t, 3)
    s3m = ss.read_state(t.backend)
    t.backend.close()
    launches = b.profile_get("compute_w")[0]
    gb.loop(a, 4)
    launches = b.profile_get("compute_w")[0] - launches
    lookahead = b.lookahead_state()[0]
    s3 = ss.read_state(b)
    judge(CALLS[3], s3m, s3)
    gb.time_step(a)
    s4 = ss.read_state(b)
    judge(CALLS[4], s3, s4)
    gb.update_state(a)
    s5 = ss.read_state(b)
    judge(CALLS[5], None, s5)
    wet = ss.wet_levels(g)[0]
    facts = dict(twin_differs=twin_differs, update_state_changed=same_bits(s4, s5), w_max=w_max, w_launches_in_loop=launches,
                 wet=bool(wet.any()), dry=bool((~wet).any()), immersed=g["immersed"], finite=all(np.isfinite(x).all() for x in s4.values()),
                 options={k: b.get_option(k) for k in ROUTES[route]}, lookahead=lookahead)
    b.close()
    return ratios, signal, failures, facts


def report(config, ratios, calls):
    for call in calls:
        if call in ratios:
            print(f"[step identities] {'-'.join(str(c) for c in config)} {call}: max residual / bound = "
                  + ", ".join(f"{k} {v:.4f}" for k, v in ratios[call].items()))


@pytest.mark.parametrize("config", CONFIGS, ids=IDS)
def test_continuity_and_masks_after_every_call(config):
    ratios, signal, failures, facts = driven(config)
    report(config, {c: {k: v for k, v in r.items() if k == "continuity"} for c, r in ratios.items()}, CALLS)
    assert facts["options"] == ROUTES[config[3]], "the model did not keep the options of its route"
    if config[1] == "simple_lat_lon" and config[3].startswith("lazy"):
        # (what the library tells about the route: the lazy corrector needs both look-aheads, tests/test_gpu_tracer_rows.py)
        assert facts["lookahead"], "the loop ended without the look-aheads the lazy corrector rides on"
    assert facts["finite"] and all(facts["w_max"][c] > 0 for c in CALLS), f"no flow to speak about: max |w| = {facts['w_max']}"
    # what the library tells about the route (its launch counters, as tests/test_gpu_step_routes.py reads them): a loop of four steps
    # launches the stand-alone w kernel once per step, unless its tendency kernels carry w -- then at least one step goes without
    if "wfly" in config[3]:
        assert facts["w_launches_in_loop"] < 4, f"w on the fly was asked for and never taken: {facts['w_launches_in_loop']} launches of compute_w"
    else:
        assert facts["w_launches_in_loop"] == 4, f"{facts['w_launches_in_loop']} launches of compute_w in loop(4)"
    assert facts["wet"] and (facts["dry"] or not facts["immersed"]), "an island grid must have wet and dry cells"
    bad = [msg for kind, msg in failures if kind == "state"]
    assert not bad, "\n".join(bad)
    assert all("continuity" in ratios[c] for c in CALLS)


@pytest.mark.parametrize("config", CONFIGS, ids=IDS)
def test_update_identities_across_every_stepping_call(config):
    ratios, signal, failures, facts = driven(config)
    report(config, {c: {k: v for k, v in r.items() if k != "continuity"} for c, r in ratios.items()}, CALLS[1:5])
    assert not facts["twin_differs"], f"the twin model differs before the loop in {facts['twin_differs']}"
    bad = [msg for kind, msg in failures if kind == "step"]
    assert not bad, "\n".join(bad)
    for call in CALLS[1:5]:
        assert signal[call] > 0, f"{call}: the corrector did nothing (max |d| = 0)"
        assert set(ratios[call]) >= {"T", "S", "u spread", "v spread", "u transport", "v transport"}


@pytest.mark.parametrize("config", CONFIGS, ids=IDS)
def test_update_state_changes_nothing_after_a_step(config):
    """No route leaves a stale w behind when a call returns: update_state after a time_step rewrites every field with the
    bits it held (w included), and continuity holds before and after."""
    ratios, signal, failures, facts = driven(config)
    assert not facts["update_state_changed"], f"update_state changed {facts['update_state_changed']}"


# ---- phase by phase -------------------------------------------------------------------------------------------------------
PHASE_SHAPE = ((40, 21, 14), 4)      # 14 levels: one chunk by default, two of 7 with momentum_chunk_levels = 7
PHASES = [(ft, g, ch, e) for ft in BUILDS for g in LATLON for ch in (0, 7) for e in (True, False)]
PHASES += [(ft, "gaussian_islands", ch, False) for ft in BUILDS for ch in (0, 7)]


@pytest.mark.parametrize("float_type,grid,chunk,euler", PHASES)
def test_column_integrals_phase_by_phase(float_type, grid, chunk, euler):
    """ab2_step(dt, euler), the halo fill and the corrector one by one, from a state set through set_field (no closure): Gn.U, Gn.V,
    the update of u, v, U_bar, V_bar and the corrected transports; momentum_chunk_levels unset and set -- the association of the
    column sums differs, the bound does not."""
    (shape, halo), dt = (((144, 64, 14), 8), 60.0) if grid == "gaussian_islands" else (PHASE_SHAPE, 300.0)
    m = gb.baroclinic_instability_model(gb.GPU(float_type=float_type), *shape, dt=dt, halo=(halo,) * 3, grid_type=grid,
                                        options=dict(momentum_chunk_levels=chunk) if chunk else None)
    b = m.backend
    set_noisy_state_with_halos(m)
    gb.first_time_step(m)
    gb.time_step(m)                      # Gn and Gm differ and are not zero
    for n in ("u", "v", "T", "S"):         # ... and the state the phases start from comes through set_field
        b.set_field(n, b.get_field(n, True), True)
    g = ss.read_geometry(b, grid, shape, halo)
    label = f"{float_type} {grid} chunk {chunk} euler {euler}"
    out = ss.check_phases(b, g, dt, b.cfg.chi, euler, ss.unit_roundoff(b.dtype), label)
    if chunk:
        assert b.get_option("momentum_chunk_levels") == chunk
    print(f"[step identities] phases {label}: max residual / bound = " + ", ".join(f"{k} {v:.4f}" for k, v in out.items()))
    b.close()


@pytest.mark.parametrize("route", ["sweep", "lazy+wfly", "no look-ahead"])
@pytest.mark.parametrize("grid", ["simple_lat_lon", "gaussian_islands_lat_lon"])
@pytest.mark.parametrize("float_type", BUILDS)
def test_an_euler_step_does_not_read_the_previous_tendencies(float_type, grid, route):
    """1e30 planted in Gm.T, Gm.S, Gm.u, Gm.v (finite: 0 x 1e30 = 0): first_time_step gives the bits it gives with zeros there."""
    runs = []
    for plant in (0.0, 1e30):
        m = make_model(float_type, grid, "ragged", route, 0)
        b = m.backend
        for n in ("Gm.T", "Gm.S", "Gm.u", "Gm.v"):
            b.set_field(n, np.full(b.field_dims(n, True), plant, b.dtype), True)
        gb.first_time_step(m)
        runs.append({n: b.get_field(n, True) for n in ("T", "S", "u", "v", "w")})
        b.close()
    for n, a in runs[0].items():
        assert np.isfinite(a).all() and np.abs(a).max() > 0 and np.array_equal(a, runs[1][n]), n
