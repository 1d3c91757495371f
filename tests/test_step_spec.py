"""tests/step_spec.py proved on the CPU oracle before it judges a kernel.

The oracle (oracle/gb25_oracle.c) evaluates the same step with separate products, true divisions and one chain per column
sum -- another order of operations than the kernels' -- in Float64 and in Float32.  Every identity of step_spec must hold
within its counted bound after update_state, first_time_step, time_step and loop(3) on each of the four grids, and each
check must FAIL, naming the cell, when one cell of the oracle's state is moved by four times its bound (away from zero: in
the direction of the residual the cell already has).
"""
import functools

import numpy as np
import pytest

import gb25_amd as gb
import step_spec as ss
from helpers import set_noisy_state_with_halos
from oracle_backend import CPU

# (grid, shape, halo, dt): Nx below and above a power of two, odd Ny; the folded grid needs Ns + 3 = 33 rows
GRIDS = [("simple_lat_lon", (20, 11, 6), 4, 600.0), ("gaussian_islands_lat_lon", (40, 21, 6), 4, 600.0),
         ("lat_lon_as_curvilinear", (20, 11, 6), 4, 600.0), ("gaussian_islands", (48, 34, 6), 8, 60.0)]
IDS = [g[0] for g in GRIDS]
PRECISIONS = ["f64", "f32"]


def make(precision, case):
    grid, shape, halo, dt = case
    m = gb.baroclinic_instability_model(CPU(precision), *shape, dt=dt, halo=halo, grid_type=grid)
    set_noisy_state_with_halos(m)
    return m


@functools.lru_cache(maxsize=None)
def trajectory(precision, case):
    """(geometry, [(call, state before the call's last step or None, state after, euler)], chi, dtype, dt) of one oracle model.
    The state before the last step of loop(3) is that of a twin model after loop(2), shown bit-equal before the loops."""
    grid, shape, halo, dt = case
    m, twin = make(precision, case), make(precision, case)
    b = m.backend
    g = ss.read_geometry(b, grid, shape, halo)
    steps, last = [], None
    for call, advance, euler in (("update_state", gb.update_state, None), ("first_time_step", gb.first_time_step, True),
                                 ("time_step", gb.time_step, False)):
        for q in (m, twin):
            advance(q)
        s = ss.read_state(b)
        steps.append((call, last if euler is not None else None, s, bool(euler)))
        last = s
    t = ss.read_state(twin.backend)
    assert all(np.array_equal(last[n], t[n]) for n in last), "the twin differs before the loops"
    gb.loop(twin, 2)
    gb.loop(m, 3)
    steps.append(("loop(3)", ss.read_state(twin.backend), ss.read_state(b), False))
    chi, dtype = b.cfg.chi, b.dtype
    b.close()
    twin.backend.close()
    return g, steps, chi, dtype, dt


def step_checks(precision, case):
    """(geometry, steps as trajectory returns them, unit round-off, euler -> (C1, C2), dt)."""
    g, steps, chi, dtype, dt = trajectory(precision, case)
    return g, steps, ss.unit_roundoff(dtype), lambda euler: ss.ab2_coefficients(chi, euler, dtype), dt


@pytest.mark.parametrize("case", GRIDS, ids=IDS)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_the_oracle_keeps_every_identity(precision, case):
    """update_state, first_time_step (Euler), time_step and loop(3): continuity and the masks after each, the update
    identities across first_time_step, time_step and the last step of loop(3)."""
    g, steps, u_, coeff, dt = step_checks(precision, case)
    worst = {}
    for call, before, s, euler in steps:
        label = f"{precision} {case[0]} after {call}"
        out = ss.check_state(s, g, u_, label)
        assert np.abs(s["w"]).max() > 0
        if before is not None:
            res, signal = ss.check_step(before, s, g, dt, *coeff(euler), u_, label)
            assert signal > 0, f"{label}: the corrector did nothing"
            out.update(res)
        for k, v in out.items():
            worst[k] = max(worst.get(k, 0.0), v)
    if g["immersed"]:
        wet = ss.wet_levels(g)[0]
        assert wet.any() and (~wet).any(), "the islands must leave wet and dry cells"
    print(f"[step_spec] oracle {precision} {case[0]}: max residual / bound = " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))


@pytest.mark.parametrize("euler", [True, False])
@pytest.mark.parametrize("case", GRIDS, ids=IDS)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_the_oracle_keeps_the_column_integrals_phase_by_phase(precision, case, euler):
    grid, shape, halo, dt = case
    m = make(precision, case)
    b = m.backend
    g = ss.read_geometry(b, grid, shape, halo)
    gb.first_time_step(m)
    gb.time_step(m)              # Gn and Gm differ, the velocities are in balance with U, V
    out = ss.check_phases(b, g, dt, b.cfg.chi, euler, ss.unit_roundoff(b.dtype), f"{precision} {grid} euler={euler}")
    print(f"[step_spec] oracle phases {precision} {grid} euler={euler}: " + ", ".join(f"{k} {v:.4f}" for k, v in out.items()))
    b.close()


@pytest.mark.parametrize("case", [GRIDS[0], GRIDS[1]], ids=IDS[:2])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_an_euler_step_does_not_read_the_previous_tendencies(precision, case):
    """1e30 planted in Gm.T, Gm.S, Gm.u, Gm.v: first_time_step gives the bits it gives with zeros there."""
    runs = []
    for plant in (0.0, 1e30):
        m = make(precision, case)
        b = m.backend
        for n in ("Gm.T", "Gm.S", "Gm.u", "Gm.v"):
            b.set_field(n, np.full(b.field_dims(n, True), plant, b.dtype), True)
        gb.first_time_step(m)
        runs.append({n: b.get_field(n, True) for n in ("T", "S", "u", "v", "w")})
        b.close()
    for n, a in runs[0].items():
        assert np.isfinite(a).all() and np.array_equal(a, runs[1][n]), n


@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_correction_that_dwarfs_the_velocity_needs_its_own_scale(precision):
    """Why two scales of step_spec are not the ones first proposed for them (2 u |u'| for the spread of the correction,
    sum dz |u'| + |U| for the transport).  A column made for it: u = 1 m/s + noise on every level while the barotropic transport U
    says the column is at rest, so one time_step corrects u by d = -1 m/s and leaves u' = O(noise).  What was rounded is the
    uncorrected u' - d = O(1): the oracle -- which is right by definition here -- misses both bounds stated on |u'| alone, and
    keeps the ones that carry |u' - d| and |d|."""
    case = GRIDS[0]
    grid, shape, halo, dt = case
    m = make(precision, case)
    b = m.backend
    g = ss.read_geometry(b, grid, shape, halo)
    gb.first_time_step(m)
    u = b.get_field("u", False)
    m.set(u=(u + 1.0).astype(b.dtype))                     # (U, V keep the transport of the state before)
    gb.update_state(m)
    before = ss.read_state(b)
    gb.time_step(m)
    after = ss.read_state(b)
    C1, C2 = ss.ab2_coefficients(b.cfg.chi, False, b.dtype)
    u_ = ss.unit_roundoff(b.dtype)
    out, signal = ss.check_step(before, after, g, dt, C1, C2, u_, "made column")
    assert signal > 0.9 and np.abs(ss.interior(after["u"], g)).max() < 0.2, (signal, out)
    with pytest.raises(AssertionError, match="correction of u within its column"):
        ss.check_step(before, after, g, dt, C1, C2, u_, "made column, scales on |u'| alone", issue_scales=True)
    ua = ss.interior(after["u"], g)
    r, bound = ss.transport(ua, ss.interior(after["U"], g), g["dz"], u_)
    ratio, at = ss.worst(r, bound)
    print(f"[step_spec] made column {precision}: with the restated scales {out}; transport against sum dz |u'| + |U|: {ratio:.3f} x at {at}")
    assert ratio > 1.0, "the transport of the made column keeps the bound stated on |u'| alone"
    b.close()


# ---- sensitivity: each check fails, and says where, when one cell is moved by four times its bound ------------------------------
def four_bounds(bound, r, sign=1.0):
    """4 x bound, with the sign that moves the residual r away from zero (sign = -1: the field enters the residual negatively)."""
    return sign * (4.0 * float(bound)) * (1.0 if float(r) >= 0 else -1.0)


def moved(state, name, index, by):
    s = dict(state)
    a = s[name].copy()
    a[index] = a.dtype.type(float(a[index]) + float(by))
    assert a[index] != state[name][index]
    s[name] = a
    return s


def nonzero_bound(bound, start):
    """The first cell at or after `start` (in C order over the last axis) of a column whose bound is positive."""
    i, j, k = start
    ks = np.nonzero(np.asarray(bound[i, j]) > 0)[0]
    assert ks.size, "no level of that column has a positive bound"
    return (i, j, int(ks[min(len(ks) - 1, k)]))


SENSITIVITY = [(p, c) for p in PRECISIONS for c in (GRIDS[0], GRIDS[3])]


@pytest.mark.parametrize("precision,case", SENSITIVITY, ids=[f"{p}-{c[0]}" for p, c in SENSITIVITY])
def test_each_check_fails_where_a_cell_is_moved(precision, case):
    g, steps, u_, coeff, dt = step_checks(precision, case)
    H, Nx, Ny, Nz = g["H"], g["Nx"], g["Ny"], g["Nz"]
    _, before, after, _ = steps[2]                        # the time_step behind first_time_step
    C1, C2 = coeff(False)
    ss.check_state(after, g, u_, "unmoved")
    ss.check_step(before, after, g, dt, C1, C2, u_, "unmoved")
    wet, wu, wv = ss.wet_levels(g)
    full = np.argwhere(wu[:, 1:Ny - 2].all(axis=2) & wv[:, 1:Ny - 2].all(axis=2))      # a column whose faces are wet on every level
    ci, cj = int(full[len(full) // 2][0]), int(full[len(full) // 2][1]) + 1

    # one w level of the interior, and one of a halo column: the top face, so that only the level below it sees the change
    r, bound = ss.continuity(after["u"], after["v"], after["w"], g, u_)
    for (i, j) in ((ci, cj), (-H + 1, cj), (Nx + H - 2, cj)):
        at = (i + H - 1, j + H - 1, Nz - 1)
        s = moved(after, "w", (i + H, j + H, H + Nz), four_bounds(bound[at], r[at]))
        with pytest.raises(AssertionError, match=r"continuity.*at cell \(%d, %d, %d\)" % (i, j, Nz - 1)):
            ss.check_state(s, g, u_, "moved")
    # ... and w at the bottom face is exactly zero
    s = moved(after, "w", (ci + H, cj + H, H), 1e-30)
    with pytest.raises(AssertionError, match="w at the bottom face"):
        ss.check_state(s, g, u_, "moved")

    # one T cell
    d, bound = ss.ab2_update(ss.interior(before["T"], g), ss.interior(after["T"], g), ss.interior(before["Gm.T"], g),
                             ss.interior(after["Gm.T"], g), dt, C1, C2, u_)
    k = Nz // 2
    s = moved(after, "T", (ci + H, cj + H, k + H), four_bounds(bound[ci, cj, k], d[ci, cj, k]))
    with pytest.raises(AssertionError, match=r"update of T.*at cell \(%d, %d, %d\)" % (ci, cj, k)):
        ss.check_step(before, s, g, dt, C1, C2, u_, "moved")

    # one u level of one column: the spread of the correction
    d, b = ss.ab2_update(ss.interior(before["u"], g), ss.interior(after["u"], g), ss.interior(before["Gm.u"], g),
                         ss.interior(after["Gm.u"], g), dt, C1, C2, u_, extra="correction")
    r, bound, dcol = ss.column_spread(d, b, wu)
    at = nonzero_bound(bound, (ci, cj, k))
    s = moved(after, "u", (ci + H, cj + H, at[2] + H), four_bounds(bound[at], r[at]))
    with pytest.raises(AssertionError, match=r"correction of u within its column.*at cell \(%d, %d, %d\)" % at):
        ss.check_step(before, s, g, dt, C1, C2, u_, "moved")

    # the transport of one column: U moved (every level of u moved by one number would pass the spread and fail here alike)
    r, bound = ss.transport(ss.interior(after["u"], g), ss.interior(after["U"], g), g["dz"], u_, dcol, wu)
    s = moved(after, "U", (ci + H, cj + H, 0), four_bounds(bound[ci, cj], r[ci, cj], -1.0))
    with pytest.raises(AssertionError, match=r"transport of the corrected u.*at cell \(%d, %d\)" % (ci, cj)):
        ss.check_step(before, s, g, dt, C1, C2, u_, "moved")
    # the same for a v column
    vj = max(cj, 1)
    d, b = ss.ab2_update(ss.interior(before["v"], g), ss.interior(after["v"], g), ss.interior(before["Gm.v"], g),
                         ss.interior(after["Gm.v"], g), dt, C1, C2, u_, extra="correction")
    _, _, dcol = ss.column_spread(d, b, wv)
    r, bound = ss.transport(ss.interior(after["v"], g), ss.interior(after["V"], g), g["dz"], u_, dcol, wv)
    s = moved(after, "V", (ci + H, vj + H, 0), four_bounds(bound[ci, vj], r[ci, vj], -1.0))
    with pytest.raises(AssertionError, match=r"transport of the corrected v.*at cell \(%d, %d\)" % (ci, vj)):
        ss.check_step(before, s, g, dt, C1, C2, u_, "moved")

    if g["immersed"]:
        # a dry level of a face that has wet ones above it: not exactly zero any more
        faces = np.argwhere(~wu[:, :, 0] & wu[:, :, -1])
        i, j = [int(q) for q in faces[len(faces) // 2]]
        s = moved(after, "u", (i + H, j + H, H), 1e-30)
        with pytest.raises(AssertionError, match=r"u on a face that touches the solid.*\(%d, %d, 0\)" % (i, j)):
            ss.check_state(s, g, u_, "moved")
