"""Lagrangian particles advected and sampled on the device (gb25_particles_*) against the numpy restatement of the scheme
(gb-25_amd/particles.py, pinned on the CPU by tests/test_particles_host.py), bit for bit: cells, fractions, statuses, counters and
samples; the folded grid, the ranks of a decomposition against the single domain, the refusals, a NaN, and the proof that
advancing particles changes nothing a model computes."""
import ctypes as C

import numpy as np
import pytest

import gb25_amd as gb
from gb25_amd.binding import FIELD_IDS, KERNEL_IDS, PARTICLE_STATUS
from gb25_amd.distributed import LocalSlabEnsemble
from gb25_amd.particles import (STATE_KEYS, advance_host, make_state, particle_fields, particle_tables, sample_host, seed_positions)
from helpers import BASE_FIELDS, CASES, GRID_NAMES, counter_rng, size_of, stepped_model

pytestmark = pytest.mark.gpu
INVALID, OUT_OF_MEMORY, STATE = 1, 3, 5
N_MANY = 1000 + 193          # not a multiple of 64: the last wave is partly filled


def same(got, want, what):
    for q in STATE_KEYS:
        assert got[q].dtype == want[q].dtype and got[q].tobytes() == want[q].tobytes(), (what, q)


def advance_both(b, state, dt, substeps, tables, what):
    """One advance on the device and in numpy on the same fields; returns the state (the device's, proven equal) and the counters."""
    want, cnt = advance_host(b, state, dt, substeps, particle_fields(b), tables)
    b.particles_advance(dt, substeps)
    got = b.particles_get()
    same(got, want, what)
    assert b.particles_info().counters() == cnt, (what, b.particles_info().counters(), cnt)
    return got, cnt


def check_against_the_restatement(m, n, what, samples=("T", "S")):
    b = m.backend
    tables = particle_tables(b)
    state = seed_positions(b, n, seed=7)
    b.particles_begin(n)
    b.particles_set(*(state[q] for q in STATE_KEYS[:6]))
    same(b.particles_get(), state, what + " as set")
    total = {}
    last = b.clock()[0]
    calls = substeps = 0
    # five rounds of two steps, the particles advanced over the time the model covered, substeps 1 and 3 alternating; then four
    # rounds over a span long enough for whole cells to be crossed, walls to be met and dry cells to block (displacements of
    # 1e-3 m/s over 1200 s are 1e-6 cells)
    Nx = tables["Nx"]
    spans = [None] * 5 + [3.0e8 * 64 / Nx] * 4
    for r, span in enumerate(spans):
        gb.loop(m, 2)
        now = b.clock()[0]
        dt, last = (now - last if span is None else span), now
        state, cnt = advance_both(b, state, dt, 1 + 2 * (r % 2), tables, f"{what} round {r}")
        calls, substeps = calls + 1, substeps + 1 + 2 * (r % 2)
        for k, v in cnt.items():
            total[k] = total.get(k, 0) + v
        for name in samples:
            got = b.particles_sample(name)
            assert got.dtype == np.float64 and got.tobytes() == sample_host(b, state, name).tobytes(), (what, r, name)
    info = b.particles_info()
    assert (info.count, info.capacity, info.calls, info.substeps) == (n, n, calls, substeps)
    assert info.counters("total") == total and total["too_far"] == 0 and total["nonfinite"] == 0
    assert ((state["a"] >= 0) & (state["a"] < 1) & (state["b"] >= 0) & (state["b"] < 1) & (state["c"] >= 0) & (state["c"] < 1)).all()
    H = tables["H"]
    assert (state["k"] >= tables["kbot"][state["i"] + H, state["j"] + H]).all(), "no particle in a dry cell"
    b.particles_end()
    return state, total


@pytest.mark.parametrize("float_type,grid_type", CASES)
@pytest.mark.parametrize("n", [1, N_MANY])
def test_bit_for_bit_against_the_restatement(float_type, grid_type, n):
    m = stepped_model(float_type, grid_type, steps=0)
    state, total = check_against_the_restatement(m, n, f"{float_type} grid {grid_type} n {n}")
    if n == N_MANY:
        start = seed_positions(m.backend, n, seed=7)
        assert (state["i"] != start["i"]).any() and (state["k"] != start["k"]).any(), "cells were crossed"
        assert total["clamped_z"] > 0
        if grid_type == 4:
            assert total["at_fold"] > 0 or (state["status"] == PARTICLE_STATUS["active"]).all()
    m.backend.close()


def test_against_the_restatement_with_catke():
    m = stepped_model("Float32", 4, steps=0, closure=gb.CATKEVerticalDiffusivity())
    check_against_the_restatement(m, N_MANY, "CATKE", samples=("T", "S", "e"))
    m.backend.close()


def test_an_odd_width():
    m = stepped_model("Float32", 0, steps=0, size=(9, 8, 4))
    check_against_the_restatement(m, 200, "9 columns")
    m.backend.close()


@pytest.mark.parametrize("float_type,grid_type", [("Float32", 3), ("Float64", 4)])
def test_the_folded_grid(float_type, grid_type):
    """Particles in the two rows below the pivot row and a northward v planted everywhere: they reach the centres of the pivot
    row, get AT_FOLD, and stay where they are in both implementations."""
    m = stepped_model(float_type, grid_type, steps=0, dt=60.0)
    b = m.backend
    Nx, Ny, Nz = size_of(grid_type)
    b.set_field("v", np.full(b.field_dims("v", True), 1.0), True)
    tables = particle_tables(b)
    i = np.tile(np.arange(Nx), 2)
    j = np.repeat([Ny - 3, Ny - 2], Nx)
    state = make_state(i, j, Nz - 1, counter_rng((2 * Nx,), 5, 1), counter_rng((2 * Nx,), 5, 2), 0.5)
    wet = state["k"] >= tables["kbot"][state["i"] + tables["H"], state["j"] + tables["H"]]
    state = {q: state[q][wet] for q in STATE_KEYS}
    assert wet.sum() > Nx // 2
    b.particles_begin(2 * Nx)
    b.particles_set(*(state[q] for q in STATE_KEYS[:6]))
    at_fold = 0
    for r in range(8):
        state, cnt = advance_both(b, state, 6.0e5, 1 + r % 2, tables, f"fold round {r}")
        at_fold += cnt["at_fold"]
    frozen = state["status"] == PARTICLE_STATUS["at_fold"]
    assert frozen.sum() == at_fold > 0
    assert ((state["j"][frozen] == Ny - 1) & (state["b"][frozen] >= 0.5)).all()
    if grid_type == 3:      # (no island in the way)
        assert frozen.all()
    later, cnt = advance_both(b, state, 6.0e5, 2, tables, "after the fold")
    for q in STATE_KEYS:
        assert later[q][frozen].tobytes() == state[q][frozen].tobytes(), q
    if grid_type == 3:
        assert cnt["at_fold"] == 0
    assert b.particles_sample("T").tobytes() == sample_host(b, later, "T").tobytes()
    b.close()


@pytest.mark.parametrize("float_type,grid_type", [("Float32", 1), ("Float64", 0)])
def test_the_tables_follow_the_host_grid_setters(float_type, grid_type):
    """The device's kbot table is made by the first advance; set_bottom_height must drop it.  The particles that are there are set
    anew into wet cells around the raised columns WITHOUT a new particles_begin (which would make the table anew by itself) and
    advanced: bit for bit the restatement with the tables read afterwards, and not what the tables read before give."""
    Nx, Ny, Nz = size = (48, 24, 6)
    m = stepped_model(float_type, grid_type, steps=0, size=size)
    b = m.backend
    n, span = 300, 3.0e8 * 64 / Nx
    state = seed_positions(b, n, seed=3)
    b.particles_begin(n)
    b.particles_set(*(state[q] for q in STATE_KEYS[:6]))
    old = particle_tables(b)
    advance_both(b, state, span, 1, old, "before set_bottom_height")       # (the device has made its table)
    zc = np.array([b.metric("zc", k) for k in range(1, Nz + 1)])
    zb = np.full((Nx, Ny), -1e30)
    zb[5:9, 4:7] = 0.5 * (zc[1] + zc[2])          # two immersed cells
    zb[20:22, 10] = 0.5 * (zc[3] + zc[4])         # four
    zb[30, 12:15] = 10.0                          # land
    b.set_bottom_height(zb)
    assert b.bottom_info("kbot", 6, 5) == 2 and b.bottom_info("kbot", 31, 13) == Nz
    new = particle_tables(b)
    H = new["H"]
    state = seed_positions(b, n, seed=9, rows=(3, 5))                      # (wet cells of the new bottom, rows 3 .. 7)
    changed = old["kbot"][state["i"] + H, state["j"] + H] != new["kbot"][state["i"] + H, state["j"] + H]
    print(f"  {int((old['kbot'] != new['kbot']).sum())} columns changed their first wet level, {int(changed.sum())} particles stand on one")
    assert changed.any()
    b.particles_set(*(state[q] for q in STATE_KEYS[:6]))
    stale, _ = advance_host(b, state, span, 3, particle_fields(b), old)
    got, cnt = advance_both(b, state, span, 3, new, "after set_bottom_height")
    assert any(got[q].tobytes() != stale[q].tobytes() for q in STATE_KEYS), "a stale table would have passed"
    assert cnt["nonfinite"] == 0 and cnt["too_far"] == 0
    b.particles_end()
    check_against_the_restatement(m, n, f"{float_type} grid {grid_type} on the new bottom")
    b.close()


LOOKAHEADS = dict(subcycle_lookahead=1, ab2_lookahead=1)


@pytest.mark.parametrize("float_type,grid_type", [("Float32", 0), ("Float64", 4)])
def test_advancing_is_read_only(float_type, grid_type):
    """Two identical models; one advances particles after every step.  Same bits, same look-ahead state, same launches of every
    phase of a step."""
    watched = stepped_model(float_type, grid_type, steps=0, **LOOKAHEADS)
    alone = stepped_model(float_type, grid_type, steps=0, **LOOKAHEADS)
    for m in (watched, alone):
        m.backend.profile_enable(True)
        m.backend.profile_reset()
    p = gb.seed_particles(watched, 300, seed=1)
    for step in range(6):
        for m in (watched, alone):
            gb.time_step(m)
        before = watched.backend.lookahead_state()
        p.advance(substeps=2)
        p.sample("T")
        assert watched.backend.lookahead_state() == before == alone.backend.lookahead_state(), step
    assert alone.backend.lookahead_state()[0], "the velocity look-ahead is on in this configuration"
    for k in KERNEL_IDS:
        if k != "diagnostics":
            assert watched.backend.profile_get(k)[0] == alone.backend.profile_get(k)[0], k
    assert watched.backend.profile_get("diagnostics")[0] == 12 and alone.backend.profile_get("diagnostics")[0] == 0
    for name in BASE_FIELDS:
        assert np.array_equal(watched.backend.get_field(name, True), alone.backend.get_field(name, True), equal_nan=True), name
    info = p.info()
    assert info.calls == 6 and info.substeps == 12 and info.time_advanced == 6 * watched.backend.clock()[2]
    p.close()
    for m in (watched, alone):
        m.backend.close()


@pytest.mark.parametrize("P,grid_type", [(2, 0), (4, 0), (2, 1)])
def test_slabs_against_the_single_domain(P, grid_type):
    """x slabs with the hand-over on the host against the single domain: global cells, fractions, statuses and samples byte for
    byte after 8 steps with an advance each.  A planted zonal flow of 0.5 m/s carries the particles, seeded within 20 degrees
    of the equator, 0.4 cells per call (the span below): after 8 calls every particle has crossed three cell faces and those
    near a seam have changed rank (the CPU restatement of tests/test_particles_host.py moves them the same distance)."""
    Nx, Ny, Nz, dt = 96 * P // 2, 40, 10, 600.0
    opts = dict(w_on_the_fly=0)
    single = gb.baroclinic_instability_model(gb.GPU(), Nx, Ny, Nz, dt=dt, grid_type=GRID_NAMES[grid_type], options=opts)
    gb.set_baroclinic_instability(single)
    single.set(u=(0.5 + 1e-2 * counter_rng((Nx, Ny, Nz), 42, 1)).astype(np.float32),
               v=(1e-2 * counter_rng((Nx, Ny + 1, Nz), 42, 2)).astype(np.float32))
    init = {n: single.backend.get_field(n, False) for n in ("u", "v", "T", "S", "eta")}
    ens = LocalSlabEnsemble(Nx, Ny, Nz, P, dt=dt, grid_type=grid_type, options=opts)
    for n, a in init.items():
        ens.scatter(n, a)
    gb.first_time_step(single)
    ens.first_time_step()
    sb = single.backend
    seeds = seed_positions(sb, 600, seed=11, rows=(Ny // 2 - 5, 10), levels=(Nz - 3, 3))
    sb.particles_begin(600)
    sb.particles_set(*(seeds[q] for q in STATE_KEYS[:6]))
    ens.particles_begin(*(seeds[q] for q in STATE_KEYS[:6]))
    span = 0.4 * sb.metric("dxc", Ny // 2) / 0.5
    for step in range(8):
        gb.time_step(single)
        ens.time_step()
        sb.particles_advance(span, 2)
        ens.particles_advance(span, 2)
    assert np.array_equal(ens.gather("u"), sb.get_field("u", False)) and np.array_equal(ens.gather("w"), sb.get_field("w", False))   # (the premise)
    one, many = sb.particles_get(), ens.particles_positions()
    what = f"{P} slabs grid {grid_type}"
    for q in STATE_KEYS:
        assert one[q].tobytes() == many[q].tobytes(), (what, q)
    for name in ("T", "S"):
        assert ens.particles_sample(name).tobytes() == sb.particles_sample(name).tobytes(), (what, name)
    assert ens.particles_moved > 0 and (one["i"] != seeds["i"]).all(), what
    assert (many["rank"] != seeds["i"] // (Nx // P)).any()
    # too far: several cells per call is refused, names substeps, and leaves every particle where it was
    with pytest.raises(gb.GB25Error, match="substeps") as e:
        ens.particles_advance(40 * span, 1)
    assert "status 5" in str(e.value)
    again = ens.particles_positions()
    for q in ("i", "j", "k", "a", "b", "c"):
        assert again[q].tobytes() == many[q].tobytes(), (what, q, "after the refusal")
    assert any(b.particles_info().counters()["too_far"] > 0 for b in ens.backends)
    for b, part in zip(ens.backends, ens._parts):      # (the device holds what the ensemble reports)
        held = b.particles_get()
        for q in ("i", "j", "k", "a", "b", "c"):
            assert held[q].tobytes() == np.ascontiguousarray(part[q]).tobytes(), (what, q)
    ens.close()
    sb.close()


def test_refusals():
    m = stepped_model("Float32", 1, steps=0)
    b = m.backend
    lib, h = b.lib, b.h
    Nx, Ny, Nz = size_of(1)
    err = lambda: lib.gb25_last_error_string(h)
    one_i, one_d = (C.c_int32 * 4)(), (C.c_double * 4)()
    # before begin
    assert lib.gb25_particles_advance(h, 1.0, 1) == STATE and b"gb25_particles_begin" in err()
    assert lib.gb25_particles_set(h, 0, 1, one_i, one_i, one_i, one_d, one_d, one_d) == STATE
    assert lib.gb25_particles_get(h, 0, 0, None, None, None, None, None, None, None) == STATE
    assert lib.gb25_particles_sample(h, FIELD_IDS["T"], one_d, 0) == STATE
    assert b.particles_info().capacity == 0
    # a capacity the device cannot hold: refused by the size check, nothing is allocated
    assert lib.gb25_particles_begin(h, 1 << 50) == OUT_OF_MEMORY and b"capacity" in err() and b"free" in err()
    assert lib.gb25_particles_begin(h, 0) == INVALID and b"capacity" in err()
    assert b.particles_info().capacity == 0 and lib.gb25_particles_advance(h, 1.0, 1) == STATE
    state = seed_positions(b, 100, seed=2)
    b.particles_begin(128)
    b.particles_set(*(state[q] for q in STATE_KEYS[:6]))
    b.particles_advance(1000.0, 2)
    before, info = b.particles_get(), b.particles_info()
    for dt in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.gb25_particles_advance(h, dt, 1) == INVALID and b"dt" in err(), dt
    for substeps in (0, -3):
        assert lib.gb25_particles_advance(h, 1.0, substeps) == INVALID and b"substeps" in err(), substeps
    for first, count in ((-1, 1), (101, 1), (0, 129), (100, 29), (0, -1)):
        assert lib.gb25_particles_set(h, first, count, one_i, one_i, one_i, one_d, one_d, one_d) == INVALID and b"first" in err(), (first, count)
    for first, count in ((-1, 1), (0, 101), (100, 1), (0, -1)):
        assert lib.gb25_particles_get(h, first, count, None, None, None, None, None, None, None) == INVALID and b"count" in err(), (first, count)
    big = (C.c_double * 128)()
    for count in (99, 101, 0):
        assert lib.gb25_particles_sample(h, FIELD_IDS["T"], big, count) == INVALID and b"count" in err(), count
    for name in ("u", "v", "w", "eta", "U"):
        assert lib.gb25_particles_sample(h, FIELD_IDS[name], big, 100) == INVALID and b"field" in err(), name
    assert lib.gb25_particles_sample(h, 99, big, 100) == INVALID and lib.gb25_particles_sample(h, FIELD_IDS["e"], big, 100) == INVALID
    # a dry cell, a fraction of 1.0, a cell outside the interior
    H = 8
    kb = particle_tables(b)["kbot"][H:H + Nx, H:H + Ny]
    i_dry, j_dry = (int(x[0]) for x in np.nonzero(kb > 0))
    ok = dict(i=3, j=3, k=Nz - 1, a=0.5, b=0.5, c=0.5)
    for change, word in ((dict(i=i_dry, j=j_dry, k=int(kb[i_dry, j_dry]) - 1), b"dry"), (dict(a=1.0), b"fraction"), (dict(c=-0.1), b"fraction"),
                         (dict(b=float("nan")), b"fraction"), (dict(i=Nx), b"interior"), (dict(j=-1), b"interior"), (dict(k=Nz), b"interior")):
        s = make_state(**{**ok, **change})
        with pytest.raises(gb.GB25Error, match=word.decode()):
            b.particles_set(*(s[q] for q in STATE_KEYS[:6]), first=100)
    # nothing of that touched the particles or the info
    same(b.particles_get(), before, "after the refusals")
    assert b.particles_info() == info and info.count == 100 and info.calls == 1
    # append, truncate; begin twice starts over; end, then advance
    s = make_state(**ok)
    b.particles_set(*(s[q] for q in STATE_KEYS[:6]), first=100)
    assert b.particles_info().count == 101 and b.particles_get(100, 1)["k"][0] == Nz - 1
    b.particles_set(*(s[q][:0] for q in STATE_KEYS[:6]), first=40)
    assert b.particles_info().count == 40
    same(b.particles_get(), {q: before[q][:40] for q in STATE_KEYS}, "truncated")
    b.particles_begin(16)
    fresh = b.particles_info()
    assert (fresh.count, fresh.capacity, fresh.calls, fresh.time_advanced) == (0, 16, 0, 0.0) and not any(fresh.total)
    b.particles_advance(1.0, 1)          # (no particle: nothing to launch)
    b.particles_end()
    assert lib.gb25_particles_advance(h, 1.0, 1) == STATE and b.particles_info().capacity == 0
    b.close()


@pytest.mark.parametrize("float_type,grid_type", [("Float32", 0), ("Float64", 4)])
def test_a_nan_stays_where_it_is(float_type, grid_type):
    """A NaN in one u face freezes exactly the particles of the two cells it bounds; every other particle equals the run without."""
    m, twin = stepped_model(float_type, grid_type, steps=2), stepped_model(float_type, grid_type, steps=2)
    Nx, Ny, Nz = size_of(grid_type)
    i0, j0, k0 = 20, 9, Nz - 1
    u = m.backend.get_field("u", False).copy()
    u[i0, j0, k0] = np.nan
    m.backend.set_field("u", u, False)
    ii, jj = np.meshgrid(np.arange(i0 - 4, i0 + 4), np.arange(j0 - 2, j0 + 3), indexing="ij")
    state = make_state(ii.ravel(), jj.ravel(), k0, 0.5, 0.5, 0.5)
    results = []
    for mm in (m, twin):
        b = mm.backend
        b.particles_begin(state["i"].size)
        b.particles_set(*(state[q] for q in STATE_KEYS[:6]))
        got, cnt = advance_both(b, state, 1200.0, 2, particle_tables(b), "nan")
        results.append((got, cnt))
    (got, cnt), (clean, clean_cnt) = results
    hit = (state["j"] == j0) & ((state["i"] == i0 - 1) | (state["i"] == i0))
    assert hit.sum() == 2 == cnt["nonfinite"] and clean_cnt["nonfinite"] == 0
    assert np.array_equal(got["status"] == PARTICLE_STATUS["nonfinite"], hit)
    for q in STATE_KEYS[:6]:
        assert got[q][hit].tobytes() == state[q][hit].tobytes(), q            # (frozen where they were)
        assert got[q][~hit].tobytes() == clean[q][~hit].tobytes(), q
    assert (clean["a"] != 0.5).any()
    m.backend.close()
    twin.backend.close()
