"""Lagrangian particles, the parts that need no GPU: the numpy restatement of gb-25_amd/particles.py on the CPU oracle's fields
against answers known in closed form and against a per-particle loop written out here (it is what the device's particles are
compared with bit for bit in tests/test_gpu_particles.py, so it is pinned here independently of the HIP kernel), the properties
the ranks of a decomposition rest on, the hand-over on the host, and the handle on a backend without the kernel."""
import math

import numpy as np
import pytest

import gb25_amd as gb
from gb25_amd.binding import PARTICLE_COUNTERS, PARTICLE_STATUS
from gb25_amd.particles import (BELOW_ONE, STATE_KEYS, ParticlesHost, TooFar, advance_host, copy_state, exchange_particles, make_state,
                                particle_fields, particle_rates, particle_tables, sample_host, seed_positions)
from helpers import counter_rng, make_oracle, set_noisy_velocities

H = 8
EPS64 = float(np.finfo(np.float64).eps)
ACTIVE, AT_FOLD, OUTSIDE, NONFINITE = (PARTICLE_STATUS[n] for n in ("active", "at_fold", "outside", "nonfinite"))


def quiet_oracle(size=(16, 12, 4), precision="f64", grid_type="simple_lat_lon"):
    return make_oracle(*size, 600.0, precision=precision, grid_type=grid_type)


def exact(state, q, r):
    """cell + fraction as a long double: exact."""
    return np.asarray(state[q], np.longdouble) + np.asarray(state[r], np.longdouble)


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_known_answer_in_x(precision):
    """u = omega dxu(j) per row, v = w = 0: every call moves every particle dt omega cells along x, the wrap included.  u is
    stored in `real` and divided in fp64, so the relative error of a substep's rate is at most 2 eps(real); the sum of a
    fraction and a displacement rounds once more: after n calls the error is at most 2 eps(real) n dt omega + n eps(double) cells."""
    Nx, Ny, Nz = 16, 12, 4
    m = quiet_oracle((Nx, Ny, Nz), precision)
    b = m.backend
    eps_real = float(np.finfo(b.dtype).eps)
    dt, omega, n = 1024.0, 1.25 * 2.0 ** -12, 40          # dt omega = 0.3125 exactly
    u = np.zeros(b.field_dims("u", True))
    for j in range(-H, Ny + H):
        u[:, j + H, :] = omega * b.metric("dxc", j + 1)
    b.set_field("u", u.astype(b.dtype), True)
    state = seed_positions(b, 200, seed=1)
    start = copy_state(state)
    tables = particle_tables(b)
    for _ in range(n):
        state, cnt = advance_host(b, state, dt, 1, tables=tables)
        assert not any(cnt.values())
    moved = exact(state, "i", "a") - exact(start, "i", "a") - np.longdouble(n * dt * omega)
    moved = moved - Nx * np.round(moved / Nx)            # (the wrap: whole turns are exact)
    bound = 2 * eps_real * n * dt * omega + n * EPS64
    print(f"{precision}: largest error {float(np.abs(moved).max()):.3e} cells, bound {bound:.3e}")
    assert np.abs(moved).max() <= bound
    assert n * dt * omega > Nx / 2 and ((state["i"] >= 0) & (state["i"] < Nx)).all()
    for q in ("j", "k", "b", "c", "status"):
        assert state[q].tobytes() == start[q].tobytes(), q


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_known_answer_in_z(precision):
    """Uniform w = omega_z dzc on evenly spaced levels: every call lifts every particle dt omega_z levels, with the bound of the
    x case; at the surface the particles stop just below the top face and clamped_z counts them."""
    Nx, Ny, Nz = 16, 12, 8
    m = quiet_oracle((Nx, Ny, Nz), precision)
    b = m.backend
    b.set_vertical_faces(np.linspace(-4096.0, 0.0, Nz + 1))
    eps_real = float(np.finfo(b.dtype).eps)
    dz = b.metric("dzc", 1)
    assert dz == 512.0 and b.metric("dzc", Nz) == 512.0
    dt, omega, n = 1024.0, 1.25 * 2.0 ** -12, 8
    b.set_field("w", np.full(b.field_dims("w", True), omega * dz, b.dtype), True)
    state = seed_positions(b, 200, seed=2, levels=(0, 3))
    start = copy_state(state)
    tables = particle_tables(b)
    for _ in range(n):
        state, cnt = advance_host(b, state, dt, 1, tables=tables)
        assert not any(cnt.values())
    rise = exact(state, "k", "c") - exact(start, "k", "c") - np.longdouble(n * dt * omega)
    bound = 2 * eps_real * n * dt * omega + n * EPS64
    print(f"{precision}: largest error {float(np.abs(rise).max()):.3e} levels, bound {bound:.3e}")
    assert np.abs(rise).max() <= bound
    clamped = 0
    for _ in range(20):
        state, cnt = advance_host(b, state, dt, 1, tables=tables)
        clamped += cnt["clamped_z"]
    assert (state["k"] == Nz - 1).all() and (state["c"] == BELOW_ONE).all() and clamped >= 200
    assert cnt["clamped_z"] == 200 and (state["status"] == ACTIVE).all()      # (they keep arriving at the face: every call clamps)
    for q in ("i", "j", "a", "b"):
        assert state[q].tobytes() == start[q].tobytes(), q


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_linear_u_within_one_cell(precision):
    """u = 0 on the western face of a cell and gamma dxu on the eastern: the rate is a gamma and one midpoint step of length h
    gives a (1 + h gamma + (h gamma)^2 / 2).  gamma carries the relative error eps(real) of its stored u and of its division;
    it enters h gamma once and (h gamma)^2 twice; five more fp64 roundings of numbers below 2: the error is at most
    a (h gamma + (h gamma)^2) eps(real) + 5 eps(double)."""
    Nx, Ny, Nz = 16, 12, 4
    m = quiet_oracle((Nx, Ny, Nz), precision)
    b = m.backend
    eps_real = float(np.finfo(b.dtype).eps)
    i0, j0, k0 = 5, 6, 2
    h, gamma = 1024.0, 0.4 / 1024.0
    u = np.zeros(b.field_dims("u", True))
    u[i0 + 1 + H, j0 + H, k0 + H] = gamma * b.metric("dxc", j0 + 1)
    b.set_field("u", u.astype(b.dtype), True)
    a = np.linspace(0.01, 0.65, 60)          # (a (1 + 0.4 + 0.08) stays inside the cell)
    state = make_state(np.full(60, i0), j0, k0, a, 0.5, 0.5)
    rx, ry, rz = particle_rates(b, state)
    assert np.abs(rx - a * gamma).max() <= eps_real * gamma and not ry.any() and not rz.any()
    new, cnt = advance_host(b, state, h, 1)
    hg = np.longdouble(h * gamma)
    want = np.asarray(a, np.longdouble) * (1 + hg + hg * hg / 2)
    err = np.abs(exact(new, "i", "a") - i0 - want)
    bound = a * float(hg + hg * hg) * eps_real + 5 * EPS64
    print(f"{precision}: largest error {float(err.max()):.3e} cells, bound {float(bound.max()):.3e}")
    assert (err <= bound).all() and (new["i"] == i0).all() and not any(cnt.values())


# ---- the per-particle loop: include/gb25.h read line by line, one particle at a time, numpy scalars for IEEE semantics
def loop_advance(t, f, state, dt, substeps):
    F = np.float64
    Hh, Nx, Ny, Nz = t["H"], t["Nx"], t["Ny"], t["Nz"]
    out = copy_state(state)
    cnt = {n: 0 for n in PARTICLE_COUNTERS}
    h = F(dt) / F(substeps)

    def clamp(x, lo, hi):
        return min(max(int(x), lo), hi)

    def rate(p):
        i, j, k, a, b, c = p
        ic, jc, kc = clamp(i, -Hh, Nx + Hh - 2) + Hh, clamp(j, -Hh, Ny + Hh - 2) + Hh, clamp(k, -Hh, Nz + Hh - 2) + Hh
        if t["curv"]:
            dx0, dx1, dy0, dy1 = t["dxu"][ic, jc], t["dxu"][ic + 1, jc], t["dyv"][ic, jc], t["dyv"][ic, jc + 1]
        else:
            dx0 = dx1 = t["dxu"][jc]
            dy0 = dy1 = F(t["dy"])
        x = (F(1) - a) * (f["u"][ic, jc, kc] / dx0) + a * (f["u"][ic + 1, jc, kc] / dx1)
        y = (F(1) - b) * (f["v"][ic, jc, kc] / dy0) + b * (f["v"][ic, jc + 1, kc] / dy1)
        z = ((F(1) - c) * f["w"][ic, jc, kc] + c * f["w"][ic, jc, kc + 1]) / t["dzc"][kc]
        return x, y, z

    def recell(i, a, d):
        x = a + d
        n = math.floor(x)
        i, x = i + n, x - F(n)
        if x >= 1:
            i, x = i + 1, F(0)
        return i, x

    def kbot(i, j):
        return int(t["kbot"][clamp(i, -Hh, Nx + Hh - 1) + Hh, clamp(j, -Hh, Ny + Hh) + Hh])

    def move(p, d):
        ev = set()
        (i, a), (j, b), (k, c) = recell(p[0], p[3], d[0]), recell(p[1], p[4], d[1]), recell(p[2], p[5], d[2])
        if t["x_periodic"]:
            i %= Nx
        if j < t["j_south"]:
            j, b = t["j_south"], F(0)
            ev.add("clamped_y")
        elif j >= t["j_north"]:
            j, b = t["j_north"] - 1, F(BELOW_ONE)
            ev.add("clamped_y")
        if k < kbot(p[0], p[1]):
            k, c = kbot(p[0], p[1]), F(0)
            ev.add("clamped_z")
        if k >= Nz:
            k, c = Nz - 1, F(BELOW_ONE)
            ev.add("clamped_z")
        if kbot(i, j) > k:
            i, j, a, b = p[0], p[1], p[3], p[4]
            ev.add("blocked")
        if i < -1 or i > Nx or j < -1 or j > Ny:
            ev.add("too_far")
        return (i, j, k, a, b, c), ev

    def small(d):
        return all(abs(x) < 2.0 ** 30 for x in d)

    with np.errstate(all="ignore"):
        for n in range(out["i"].size):
            p = (int(out["i"][n]), int(out["j"][n]), int(out["k"][n]), F(out["a"][n]), F(out["b"][n]), F(out["c"][n]))
            status = int(out["status"][n])
            for _ in range(substeps):
                if status != ACTIVE:
                    break
                if t["fold"] and (p[1] > Ny - 1 or (p[1] == Ny - 1 and p[4] >= 0.5)):
                    status = AT_FOLD
                    cnt["at_fold"] += 1
                    break
                d0 = tuple((F(0.5) * h) * r for r in rate(p))
                if not small(d0):
                    status = NONFINITE
                    cnt["nonfinite"] += 1
                    break
                pm, evm = move(p, d0)
                d1 = tuple(h * r for r in rate(pm))
                if not small(d1):
                    status = NONFINITE
                    cnt["nonfinite"] += 1
                    break
                q, ev = move(p, d1)
                if "too_far" in ev | evm:
                    cnt["too_far"] += 1
                    break
                p = q
                for name in ("blocked", "clamped_y", "clamped_z"):
                    cnt[name] += name in ev
                if t["fold"] and p[1] == Ny - 1 and p[4] >= 0.5:
                    status = AT_FOLD
                    cnt["at_fold"] += 1
                elif p[0] < 0 or p[0] >= Nx or p[1] < 0 or p[1] >= Ny:
                    status = OUTSIDE
                    cnt["outside"] += 1
            for q_, x in zip(("i", "j", "k", "a", "b", "c"), p):
                out[q_][n] = x
            out["status"][n] = status
    return out, cnt


@pytest.mark.parametrize("grid_type", ["gaussian_islands_lat_lon", "gaussian_islands"])
def test_walls_and_bathymetry(grid_type):
    """50 advances through a stepped, noisy state with mountains: no particle in a dry cell, none beyond a wall, every fraction in
    [0, 1); the events are those the per-particle loop counts and the vectorised restatement equals the loop bit for bit."""
    Nx, Ny, Nz = 48, 24, 6
    m = make_oracle(Nx, Ny, Nz, 60.0 if grid_type == "gaussian_islands" else 600.0, grid_type=grid_type)
    gb.set_baroclinic_instability(m)
    set_noisy_velocities(m, amplitude=0.3)
    gb.first_time_step(m)
    b = m.backend
    tables, fields = particle_tables(b), particle_fields(b)
    # particles around the mountains and along both walls
    kb = tables["kbot"][H:H + Nx, H:H + Ny]
    near = np.argwhere((kb == 0) & ((np.roll(kb, 1, 0) > 0) | (np.roll(kb, -1, 0) > 0) | (np.roll(kb, 1, 1) > 0) | (np.roll(kb, -1, 1) > 0)))
    near = near[near[:, 1] < Ny - 1][:40]
    walls = np.array([(i, j) for i in range(0, Nx, 4) for j in (0, 1, Ny - 2)])
    cells = np.concatenate([near, walls])
    n = len(cells)
    state = make_state(cells[:, 0], cells[:, 1], np.arange(n) % Nz, counter_rng((n,), 3, 1), counter_rng((n,), 3, 2), counter_rng((n,), 3, 3))
    state["k"] = np.maximum(state["k"], kb[state["i"], state["j"]]).astype(np.int32)
    one = copy_state(state)
    total = {q: 0 for q in PARTICLE_COUNTERS}
    # 0.3 m/s over cells of 800 km: half a cell per call; three times that on the lat-lon grid, where only a midpoint that
    # overshoots the vanishing normal rate at an immersed face ever meets a dry cell
    span = 1.5e6 if grid_type == "gaussian_islands" else 5.0e6
    for r in range(50):
        state, cnt = advance_host(b, state, span, 1 + r % 2, fields, tables)
        one, cnt_loop = loop_advance(tables, fields, one, span, 1 + r % 2)
        assert cnt == cnt_loop, (r, cnt, cnt_loop)
        for q in STATE_KEYS:
            assert state[q].tobytes() == one[q].tobytes(), (r, q)
        for q, v in cnt.items():
            total[q] += v
    print(grid_type, total)
    assert total["blocked"] > 0 and total["clamped_y"] > 0 and total["clamped_z"] > 0 and total["too_far"] == 0 == total["outside"]
    assert (state["k"] >= kb[state["i"], state["j"]]).all() and (state["k"] < Nz).all(), "no particle in a dry cell"
    assert ((state["i"] >= 0) & (state["i"] < Nx) & (state["j"] >= 0) & (state["j"] < Ny)).all(), "none beyond a wall"
    for q in ("a", "b", "c"):
        assert ((state[q] >= 0) & (state[q] < 1)).all(), q
    if grid_type == "gaussian_islands":
        frozen = state["status"] == AT_FOLD
        assert ((state["j"][frozen] == Ny - 1) & (state["b"][frozen] >= 0.5)).all() and frozen.sum() == total["at_fold"]
    assert sample_host(b, state, "T").tobytes() == np.asarray(b.get_field("T", False), np.float64)[state["i"], state["j"], state["k"]].tobytes()


def periodic_parent(parent, Nx, shift):
    """The parent array with its interior columns rolled by `shift` and the x halos made the periodic images."""
    inner = np.roll(parent[H:H + Nx], shift, axis=0)
    return np.concatenate([inner[-H:], inner, inner[:H]], axis=0)


def test_translation_invariance_and_substeps():
    """Rolling every field by 5 columns and adding 5 to every i gives the same j, k, a, b, c and status byte for byte -- the
    property the slabs of a decomposition rest on --, and advance(dt, 3) equals three advance(dt / 3, 1)."""
    Nx, Ny, Nz = 16, 12, 4
    m = quiet_oracle((Nx, Ny, Nz))
    gb.set_baroclinic_instability(m)
    set_noisy_velocities(m, amplitude=0.3)
    gb.first_time_step(m)
    gb.loop(m, 2)
    b = m.backend
    tables = particle_tables(b)
    here = {q: periodic_parent(a, Nx, 0) for q, a in particle_fields(b).items()}
    there = {q: periodic_parent(a, Nx, 5) for q, a in particle_fields(b).items()}
    s0 = seed_positions(b, 300, seed=4)
    s1 = copy_state(s0)
    s1["i"] = ((s0["i"] + 5) % Nx).astype(np.int32)
    for r in range(6):
        s0, c0 = advance_host(b, s0, 2.0e6, 1 + r % 3, here, tables)
        s1, c1 = advance_host(b, s1, 2.0e6, 1 + r % 3, there, tables)
        assert c0 == c1
        for q in ("j", "k", "a", "b", "c", "status"):
            assert s0[q].tobytes() == s1[q].tobytes(), (r, q)
        assert np.array_equal((s0["i"] + 5) % Nx, s1["i"])
    start = seed_positions(b, 300, seed=4)
    assert (s0["i"] != start["i"]).any() and (s0["j"] != start["j"]).any() and c0["clamped_z"] > 0
    # substeps
    whole, cw = advance_host(b, start, 3.0e6, 3, here, tables)
    parts, cp = start, {q: 0 for q in PARTICLE_COUNTERS}
    for _ in range(3):
        parts, c = advance_host(b, parts, 3.0e6 / 3, 1, here, tables)
        cp = {q: cp[q] + c[q] for q in cp}
    assert cw == cp
    for q in STATE_KEYS:
        assert whole[q].tobytes() == parts[q].tobytes(), q
    other, _ = advance_host(b, start, 3.0e6, 1, here, tables)
    assert other["a"].tobytes() != whole["a"].tobytes()


def test_a_nan_and_the_refusals_of_the_restatement():
    m = quiet_oracle()
    b = m.backend
    u = np.zeros(b.field_dims("u", True))
    u[5 + H, 6 + H, 2 + H] = np.nan
    b.set_field("u", u, True)
    state = make_state(np.arange(2, 10), 6, 2, 0.25)
    new, cnt = advance_host(b, state, 100.0, 2)
    assert np.array_equal(new["status"] == NONFINITE, (state["i"] == 4) | (state["i"] == 5)) and cnt["nonfinite"] == 2
    for q in ("i", "j", "k", "a", "b", "c"):
        assert new[q].tobytes() == state[q].tobytes(), q
    for dt, substeps in ((0.0, 1), (float("nan"), 1), (-1.0, 1), (1.0, 0), (1.0, 1.5)):
        with pytest.raises(ValueError):
            advance_host(b, state, dt, substeps)
    with pytest.raises(ValueError, match="c,c,c"):
        sample_host(b, state, "u")


def test_the_hand_over_on_the_host():
    """Synthetic parts of four x slabs of 8 columns: the OUTSIDE particles go to the owner of their cell, only integers change,
    the set of particles is conserved and no OUTSIDE is left."""
    nx, P = 8, 4
    offsets = [(r * nx, 0) for r in range(P)]
    parts = []
    for r in range(P):
        n = 12
        i = (np.arange(n) % nx).astype(np.int32)
        s = make_state(i, np.arange(n) % 5, np.arange(n) % 3, counter_rng((n,), r, 1), counter_rng((n,), r, 2), counter_rng((n,), r, 3))
        s["i"][0], s["status"][0] = -1, OUTSIDE          # leaves to the west (rank 0: wraps to the last rank)
        s["i"][5], s["status"][5] = nx, OUTSIDE          # leaves to the east
        s["status"][7] = AT_FOLD                         # stays, frozen
        s["id"] = 100 * r + np.arange(n)
        parts.append(s)
    new, moved = exchange_particles(parts, offsets, (nx, 5))
    assert moved == 2 * P and sum(p["i"].size for p in new) == 12 * P
    old = {int(q): (r, n) for r, p in enumerate(parts) for n, q in enumerate(p["id"])}
    seen = set()
    for r, p in enumerate(new):
        assert p["i"].dtype == np.int32 and ((p["i"] >= 0) & (p["i"] < nx)).all() and not (p["status"] == OUTSIDE).any()
        for n, q in enumerate(p["id"]):
            r0, n0 = old[int(q)]
            seen.add(int(q))
            src = parts[r0]
            assert (src["i"][n0] + offsets[r0][0]) % (nx * P) == p["i"][n] + offsets[r][0]
            for key in ("j", "k", "a", "b", "c"):
                assert src[key][n0] == p[key][n]
            assert p["status"][n] == (ACTIVE if src["status"][n0] == OUTSIDE else src["status"][n0])
            assert (r != r0) == (src["status"][n0] == OUTSIDE)
    assert seen == set(old)
    again, moved = exchange_particles(new, offsets, (nx, 5))
    assert moved == 0 and all(a[q].tobytes() == n_[q].tobytes() for a, n_ in zip(again, new) for q in STATE_KEYS)


def test_the_handle_on_a_backend_without_the_kernel():
    m = quiet_oracle()
    gb.set_baroclinic_instability(m)
    set_noisy_velocities(m, amplitude=0.3)
    gb.first_time_step(m)
    state = np.random.get_state()[1].copy()
    p = gb.seed_particles(m, 50, seed=9)
    again = seed_positions(m.backend, 50, seed=9)
    assert np.array_equal(np.random.get_state()[1], state), "the global generator is not touched"
    assert isinstance(p._p, ParticlesHost) and all(p.state()[q].tobytes() == again[q].tobytes() for q in STATE_KEYS)
    traj = gb.run_with_particles(m, p, 5, every=2)
    assert traj["xi"].shape == traj["T"].shape == traj["status"].shape == (3, 50) and traj["time"].shape == (3,)
    info = p.info()
    assert info.calls == 3 and info.count == 50 and info.time_advanced == 5 * 600.0
    assert (p.depth() < 0).all() and (p.depth() > -4000).all()
    assert np.array_equal(p.positions()["zeta"], traj["zeta"][-1]) and np.array_equal(p.sample("S"), traj["S"][-1])
    with pytest.raises(ValueError, match="dry|interior|fraction"):
        gb.particles(m, 3, 3, 2, a=1.0)
    with pytest.raises(ValueError):
        p.advance(-1.0)
    assert p.info().calls == 3
    p.close()
    # more than one cell beyond a rank's interior: the restatement refuses and leaves the state alone
    b = m.backend
    tables = dict(particle_tables(b), x_periodic=False)
    s = make_state(np.array([15, 3]), 6, 3, 0.9)
    fields = particle_fields(b)
    fields["u"] = np.full(fields["u"].shape, 50.0)
    gone, cnt = advance_host(b, s, 0.1 * tables["dxu"][H + 6] / 50.0, 1, fields, tables)
    assert gone["status"].tolist() == [OUTSIDE, ACTIVE] and gone["i"].tolist() == [16, 4] and cnt["outside"] == 1
    with pytest.raises(TooFar, match="substeps") as e:
        advance_host(b, s, 3.0 * tables["dxu"][H + 6] / 50.0, 1, fields, tables)
    assert e.value.count == 1
