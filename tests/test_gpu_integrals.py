"""Volume-weighted integrals on the device (gb25_integrate_field, gb25_get_budget) against math.fsum over the downloaded
fields weighted with the numpy restatement of the cell measure (gb-25_amd/integrals.py, pinned on the CPU by
tests/test_integrals_host.py), and the proof that asking for them changes nothing a model computes.

Sums: a row record adds n fp64 terms in a fixed but not sequential order; any order of n terms is within (n - 1) eps(Float64)
sum|term| of the exact sum (Higham, Accuracy and Stability of Numerical Algorithms, eq. 4.4 to first order), math.fsum gives
the exact sum of the terms correctly rounded, and forming mu and a term costs up to four more roundings: the bound asserted is
(n + 4) eps sum|term|.  Levels and totals are DEFINED as left-to-right sums of the rows and levels and are compared bit for bit."""
import math

import numpy as np
import pytest

import gb25_amd as gb
from gb25_amd.binding import FIELD_IDS
from gb25_amd.distributed import LocalSlabEnsemble
from gb25_amd.integrals import cell_measure, combine_budgets, fold_records
from helpers import BASE_FIELDS, CASES, CATKE_FIELDS, EPS, GRID_NAMES, counter_rng, size_of, stepped_model

pytestmark = pytest.mark.gpu
MEMBERS = ("measure", "first", "second", "points", "nonfinite")


def assert_sum(got, terms, what, quiet=False):
    n = len(terms)
    exact, bound = math.fsum(terms), (n + 4) * EPS * math.fsum(np.abs(terms))
    if not quiet:
        print(f"    {what}: device {got!r} fsum {exact!r} |diff| {abs(got - exact):.3e} bound {bound:.3e}")
    assert abs(got - exact) <= bound, (what, got, exact, bound)


def check_field(b, name, mu=None):
    """ROWS against fsum, LEVELS and TOTAL against the left-to-right sums of what was downloaded."""
    x = np.asarray(b.get_field(name, False), np.float64)
    mu = cell_measure(b, name) if mu is None else mu
    rows, levels, total = (b.integrate_field(name, s) for s in ("rows", "levels", "total"))
    bx, by, bz = x.shape
    assert rows.shape == (by, bz) and levels.shape == (bz,) and total.shape == () and mu.shape == x.shape
    wet = mu > 0
    fin = np.isfinite(x)
    worst = 0.0
    for k in range(bz):
        for j in range(by):
            ok = wet[:, j, k] & fin[:, j, k]
            r = rows[j, k]
            assert r["points"] == int(ok.sum()) and r["nonfinite"] == int((wet[:, j, k] & ~fin[:, j, k]).sum()), (name, j, k)
            m_, x_ = mu[ok, j, k], x[ok, j, k]
            for member, terms in (("measure", m_), ("first", m_ * x_), ("second", (m_ * x_) * x_)):
                # (n = the terms of the row: a row with dry points has fewer, and the smaller bound is the one asserted)
                exact, bound = math.fsum(terms), (len(terms) + 4) * EPS * math.fsum(np.abs(terms))
                assert abs(float(r[member]) - exact) <= bound, (name, member, j, k, float(r[member]), exact, bound)
                if bound > 0:
                    worst = max(worst, abs(float(r[member]) - exact) / bound)
    print(f"  {name}: {by} x {bz} rows of {bx}, wet points {int(total['points'])}, measure {float(total['measure'])!r}, "
          f"first {float(total['first'])!r}, worst |diff| / bound {worst:.3f}")
    want_levels = fold_records(rows)
    want_total = fold_records(levels)
    for f in MEMBERS:
        # (fold_records is np.add.accumulate: sequential; restated with Python floats for the doubles)
        if f in ("measure", "first", "second"):
            for k in range(bz):
                acc = 0.0
                for j in range(by):
                    acc += float(rows[j, k][f])
                assert acc == float(levels[k][f]) or (math.isnan(acc) and math.isnan(float(levels[k][f]))), (name, f, k)
            acc = 0.0
            for k in range(bz):
                acc += float(levels[k][f])
            assert acc == float(total[f]), (name, f)
        assert np.array_equal(want_levels[f], levels[f]) and want_total[f] == total[f], (name, f)
    assert int(total["points"]) == int((wet & fin).sum())
    return total


@pytest.mark.parametrize("float_type,grid_type", CASES)
def test_rows_levels_and_totals_of_every_field(float_type, grid_type):
    m = stepped_model(float_type, grid_type)
    b = m.backend
    for name in BASE_FIELDS:
        check_field(b, name)
    assert m.tracers.T.integral() == b.integrate_field("T", "total")
    lv = b.integrate_field("T", "levels")
    assert np.array_equal(m.tracers.T.horizontal_mean(), lv["first"] / lv["measure"], equal_nan=True)
    rw = b.integrate_field("u", "rows")
    with np.errstate(invalid="ignore", divide="ignore"):
        assert np.array_equal(m.velocities.u.zonal_mean(), rw["first"] / rw["measure"], equal_nan=True)
    with pytest.raises(gb.GB25Error, match="no such field"):
        b.integrate_field("e")
    from gb25_amd.binding import Moments
    out = (Moments * 4)()
    assert b.lib.gb25_integrate_field(b.h, FIELD_IDS["T"], 2, out, 2) == 1          # TOTAL is one record
    assert b"count" in b.lib.gb25_last_error_string(b.h)
    assert b.lib.gb25_integrate_field(b.h, FIELD_IDS["T"], 1, out, 3) == 1          # LEVELS are bz
    assert b.lib.gb25_integrate_field(b.h, FIELD_IDS["T"], 7, out, 1) == 1
    b.close()


@pytest.mark.parametrize("float_type,grid_type", [("Float32", 0), ("Float64", 0), ("Float32", 4)])
def test_rows_levels_and_totals_of_the_catke_fields(float_type, grid_type):
    m = stepped_model(float_type, grid_type, closure=gb.CATKEVerticalDiffusivity())
    b = m.backend
    for name in CATKE_FIELDS + ["u", "T", "w"]:
        check_field(b, name)
    b.close()


@pytest.mark.parametrize("float_type,grid_type", [("Float32", 1), ("Float64", 4)])
def test_nonfinite_values_in_wet_and_immersed_cells(float_type, grid_type):
    m = stepped_model(float_type, grid_type, steps=0)
    b = m.backend
    mu = cell_measure(b, "T")
    dry = np.argwhere(mu == 0)
    wet = np.argwhere(mu > 0)
    assert len(dry) > 0, "the islands immerse cells"
    clean = b.integrate_field("T", "total")
    T = b.get_field("T", False).copy()
    (i0, j0, k0), (i1, j1, k1), (i2, j2, k2) = wet[7], wet[len(wet) // 2], dry[len(dry) // 2]
    T[i0, j0, k0] = np.nan
    T[i1, j1, k1] = np.inf
    T[i2, j2, k2] = np.nan
    b.set_field("T", T, False)
    # (set_field masks the immersed cells of T: the value that stays in an immersed cell is planted below, in fields it leaves alone)
    total = check_field(b, "T", mu)
    assert total["nonfinite"] == 2 and total["points"] == clean["points"] - 2
    rows = b.integrate_field("T", "rows")
    assert rows[j0, k0]["nonfinite"] == 1 and rows[j1, k1]["nonfinite"] >= 1 and rows["nonfinite"].sum() == 2
    bud = b.budget()
    assert bud.T.nonfinite == 2 and math.isfinite(bud.T.first) and bud.S.nonfinite == 0
    # a NaN and an Inf in immersed cells (a tendency of a tracer, a field on the z faces, a tendency on the x faces): they stay in memory and are invisible --
    # every record of every shape keeps its bytes
    for name in ("Gn.T", "w", "Gn.u"):
        mu_n = cell_measure(b, name)
        dry_n = np.argwhere(mu_n == 0)
        assert len(dry_n) >= 2, name
        before = [b.integrate_field(name, s).tobytes() for s in ("rows", "levels", "total")]
        clean_total = b.integrate_field(name, "total")
        a = b.get_field(name, False).copy()
        (ia, ja, ka), (ib, jb, kb) = dry_n[len(dry_n) // 3], dry_n[2 * len(dry_n) // 3]
        a[ia, ja, ka] = np.nan
        a[ib, jb, kb] = -np.inf
        b.set_field(name, a, False)
        back = b.get_field(name, False)
        assert np.isnan(back[ia, ja, ka]) and np.isinf(back[ib, jb, kb]), f"{name}: the immersed cells hold the planted values"
        after = [b.integrate_field(name, s).tobytes() for s in ("rows", "levels", "total")]
        assert after == before, name
        total_n = check_field(b, name, mu_n)
        assert total_n["nonfinite"] == 0 and total_n["points"] == clean_total["points"] == int((mu_n > 0).sum()), name
        assert math.isfinite(total_n["first"]) and math.isfinite(total_n["second"]), name
    b.close()


@pytest.mark.parametrize("float_type,grid_type", CASES)
def test_budget(float_type, grid_type):
    m = stepped_model(float_type, grid_type, steps=0)
    b = m.backend
    first = b.budget()
    gb.loop(m, 3)
    bud = gb.budget(m)
    print(" ", bud)
    for name in ("T", "S", "u", "v", "eta"):
        t = b.integrate_field(name, "total")
        r = getattr(bud, name)
        assert tuple(getattr(r, f) for f in MEMBERS) == tuple(t[f] for f in MEMBERS), name
    assert bud.volume == bud.T.measure and bud.surface_area == bud.eta.measure
    assert bud.kinetic_energy == 0.5 * (bud.u.second + bud.v.second) and bud.kinetic_energy > 0
    assert bud.eta_potential_energy == 0.5 * b.cfg.g * bud.eta.second and bud.eta_potential_energy > 0
    t, it, _ = b.clock()
    assert (bud.time, bud.iteration) == (t, it) and tuple(bud.global_offset) == (0, 0, 0)
    # the measure does not move with the state
    assert (bud.volume, bud.surface_area, bud.T.points, bud.u.measure) == (first.volume, first.surface_area, first.T.points, first.u.measure)
    assert bud.T.first != first.T.first or bud.u.second != first.u.second
    b.close()


LOOKAHEADS = dict(subcycle_lookahead=1, ab2_lookahead=1)


@pytest.mark.parametrize("float_type,grid_type,catke", [("Float32", 0, False), ("Float64", 0, False), ("Float32", 1, False),
                                                        ("Float32", 4, False), ("Float64", 4, False), ("Float32", 0, True),
                                                        ("Float32", 4, True)])
def test_integrals_are_read_only(float_type, grid_type, catke):
    """Two identical models; one is asked for every integral between every two steps.  Same bits, same look-ahead state, same
    launches of every phase of a step."""
    closure = gb.CATKEVerticalDiffusivity() if catke else None
    watched = stepped_model(float_type, grid_type, steps=0, closure=closure, **LOOKAHEADS)
    alone = stepped_model(float_type, grid_type, steps=0, closure=closure, **LOOKAHEADS)
    names = BASE_FIELDS + (CATKE_FIELDS if catke else [])
    for m in (watched, alone):
        m.backend.profile_enable(True)
        m.backend.profile_reset()
    for step in range(6):
        if step % 2 == 0:
            before = watched.backend.lookahead_state()
            bud = watched.backend.budget()
            assert watched.backend.lookahead_state() == before
            assert bud.iteration == step + 1 and bud.T.nonfinite == 0 and bud.volume > 0
            for name in names:
                watched.backend.integrate_field(name, ("rows", "levels", "total")[(step // 2) % 3])
            assert watched.backend.lookahead_state() == before
        for m in (watched, alone):
            gb.time_step(m)
        assert watched.backend.lookahead_state() == alone.backend.lookahead_state(), step
    assert alone.backend.lookahead_state()[0], "the velocity look-ahead is on in this configuration"
    from gb25_amd.binding import KERNEL_IDS
    for k in KERNEL_IDS:
        if k != "diagnostics":
            assert watched.backend.profile_get(k)[0] == alone.backend.profile_get(k)[0], k
    assert watched.backend.profile_get("diagnostics")[0] > 0 and alone.backend.profile_get("diagnostics")[0] == 0
    for name in names:
        a, b = watched.backend.get_field(name, True), alone.backend.get_field(name, True)
        assert np.array_equal(a, b, equal_nan=True), name
    assert np.abs(watched.backend.get_field("u", False)).max() > 0
    for m in (watched, alone):
        m.backend.close()


@pytest.mark.parametrize("float_type,grid_type", [("Float32", 0), ("Float64", 4), ("Float32", 1)])
def test_repeatable_to_the_last_bit(float_type, grid_type):
    m1, m2 = stepped_model(float_type, grid_type), stepped_model(float_type, grid_type)
    for name in ("u", "v", "T", "eta", "w", "Gn.v", "pHY"):
        for shape in ("rows", "levels", "total"):
            s = [m.backend.integrate_field(name, shape).tobytes() for m in (m1, m1, m2)]
            assert s[0] == s[1] == s[2], (name, shape)
    buds = [bytes(m.backend.budget()) for m in (m1, m1, m2)]
    assert buds[0] == buds[1] == buds[2]
    m1.backend.close()
    m2.backend.close()


@pytest.mark.parametrize("float_type,grid_type", [("Float32", 0), ("Float64", 1), ("Float32", 4)])
def test_the_tables_follow_the_host_grid_setters(float_type, grid_type):
    m = stepped_model(float_type, grid_type, steps=1)
    b = m.backend
    Nx, Ny, Nz = size_of(grid_type)
    before = b.integrate_field("T", "total")
    zc = np.array([b.metric("zc", k) for k in range(1, Nz + 1)])
    zb = np.full((Nx, Ny), -1e30)
    zb[5:9, 4:7] = 0.5 * (zc[1] + zc[2])          # two immersed cells
    zb[20:22, 10] = 0.5 * (zc[3] + zc[4])         # four
    zb[30, 12:15] = 10.0                          # land
    b.set_bottom_height(zb)
    assert b.bottom_info("kbot", 6, 5) == 2 and b.bottom_info("kbot", 31, 13) == Nz
    for name in ("T", "u", "v", "w", "eta", "U", "V"):
        check_field(b, name)
    after = b.integrate_field("T", "total")
    assert after["measure"] != before["measure"] and after["points"] == Nx * Ny * Nz - 12 * 2 - 2 * 4 - 3 * Nz
    if grid_type == 0:
        # other vertical faces: the spacings of the measure follow
        zf = -4000.0 * (1.0 - np.linspace(0.0, 1.0, Nz + 1)) ** 1.5
        b.set_vertical_faces(zf)
        for name in ("T", "w", "v"):
            check_field(b, name)
    b.close()


DECOMPOSITIONS = [(2, 1), (4, 1), (4, 2)]


@pytest.mark.parametrize("grid_type", [1, 4])
@pytest.mark.parametrize("P,Ry", DECOMPOSITIONS)
def test_combined_budgets_of_the_ranks(P, Ry, grid_type):
    if Ry == 1:
        Nx, Ny, Nz, dt, kw = 96 * P // 2, 40, 10, 600.0, {}
    else:
        Nx, Ny, Nz, dt, kw = 128, 48 * Ry, 8, 600.0, dict(slab_mode=1)
    exact = dict(w_on_the_fly=0)
    single = gb.baroclinic_instability_model(gb.GPU(), Nx, Ny, Nz, dt=dt, grid_type=GRID_NAMES[grid_type])
    gb.set_baroclinic_instability(single)
    vrows = Ny if grid_type == 4 else Ny + 1
    single.set(u=(1e-2 * counter_rng((Nx, Ny, Nz), 42, 1)).astype(np.float32),
               v=(1e-2 * counter_rng((Nx, vrows, Nz), 42, 2)).astype(np.float32),
               eta=(1e-2 * counter_rng((Nx, Ny, 1), 42, 3)).astype(np.float32))
    init = {n: single.backend.get_field(n, False) for n in ("u", "v", "T", "S", "eta")}
    ens = LocalSlabEnsemble(Nx, Ny, Nz, P, dt=dt, ranks_y=Ry, grid_type=grid_type, options=exact, **kw)
    for n, a in init.items():
        ens.scatter(n, a)
    gb.first_time_step(single)
    ens.first_time_step()
    gb.loop(single, 4)
    ens.loop(4)
    sb = single.backend
    parts = [b.budget() for b in ens.backends]
    comb, one = combine_budgets(parts), sb.budget()
    assert comb.as_dict()["iteration"] == one.iteration and bytes(ens.budget()) == bytes(comb)
    for name in ("T", "S", "u", "v", "eta"):
        assert np.array_equal(ens.gather(name), sb.get_field(name, False)), name     # (the premise)
        # every rank's measure is the single domain's on its window -- the 1/2 of the pivot row on the top row of ranks only
        mu = cell_measure(sb, name)
        for b in ens.backends:
            d = b.field_dims(name, False)
            i0, j0 = b.rx * ens.Nx_loc, b.ry * ens.Ny_loc
            assert np.array_equal(cell_measure(b, name), mu[i0:i0 + d[0], j0:j0 + d[1]]), (name, b.cfg.rank)
        x = np.asarray(sb.get_field(name, False), np.float64)
        c, s = getattr(comb, name), getattr(one, name)
        assert (c.points, c.nonfinite) == (s.points, s.nonfinite) == (int((mu > 0).sum()), 0), name
        for member, terms in (("measure", mu), ("first", mu * x), ("second", (mu * x) * x)):
            terms = terms[mu > 0].ravel()
            assert_sum(getattr(c, member), terms, f"{name} {member} combined")
            assert_sum(getattr(s, member), terms, f"{name} {member} single", quiet=True)
        rows = ens.integrate_field(name, "rows")
        srows = sb.integrate_field(name, "rows")
        assert rows.shape == srows.shape and np.array_equal(rows["points"], srows["points"]), name
        # row by row: the ranks' rows added (x slabs) and stacked (mesh) are the single domain's rows within the row's bound
        for k in range(rows.shape[1]):
            for j in range(rows.shape[0]):
                ok = mu[:, j, k] > 0
                m_, x_ = mu[ok, j, k], x[ok, j, k]
                for member, terms in (("measure", m_), ("first", m_ * x_), ("second", (m_ * x_) * x_)):
                    exact, bound = math.fsum(terms), (len(terms) + 4) * EPS * math.fsum(np.abs(terms))
                    assert abs(float(rows[j, k][member]) - exact) <= bound, (name, member, j, k, "combined")
                    assert abs(float(srows[j, k][member]) - exact) <= bound, (name, member, j, k, "single")
    if grid_type == 4:
        for b in ens.backends:
            H = b.cfg.halo
            az = b.metric2("azcc")[H:H + ens.Nx_loc, H:H + ens.Ny_loc]
            mu = cell_measure(b, "eta")[:, :, 0]
            half = np.where(mu > 0, 0.5 * az, 0.0)
            full = np.where(mu > 0, az, 0.0)
            assert np.array_equal(mu[:, :-1], full[:, :-1]) and (mu[:, -1] > 0).any(), b.cfg.rank
            assert np.array_equal(mu[:, -1], half[:, -1] if b.ry == Ry - 1 else full[:, -1]), b.cfg.rank
            r = b.integrate_field("eta", "rows")[:, 0]["measure"]
            assert_sum(float(r[-1]), mu[:, -1][mu[:, -1] > 0], f"rank {b.cfg.rank} measure of its last row", quiet=True)
    assert comb.volume == comb.T.measure and comb.kinetic_energy == 0.5 * (comb.u.second + comb.v.second)
    ens.close()
    sb.close()


def eta_drift(model):
    """d = |sum mu eta| / sum mu |eta| and the number of terms."""
    b = model.backend
    mu = cell_measure(b, "eta")
    eta = np.asarray(b.get_field("eta", False), np.float64)
    den = math.fsum((mu * np.abs(eta)).ravel())
    num = b.budget().eta.first if hasattr(b, "budget") else math.fsum((mu * eta).ravel())
    return abs(num) / den, int((mu > 0).sum())


@pytest.mark.parametrize("float_type,grid_type", [(ft, gt) for ft in ("Float32", "Float64") for gt in (0, 4)])
def test_the_volume_of_eta_is_conserved(float_type, grid_type):
    """sum mu eta starts at zero and stays there to round-off: d = |sum mu eta| / sum mu |eta| of the device against the same
    quantity of the CPU oracle of the same float type stepped the same way, d_device <= 10 max(d_oracle, n eps(real)).  Two
    correct implementations differ in operation order, so their round-off sums differ by a small factor; a non-conservative
    defect shows at truncation size, orders of magnitude above (tools/budget_probe.py --eta-drift records both values:
    profiles/integrals_eta_drift.json)."""
    from oracle_backend import CPU
    real = np.float32 if float_type == "Float32" else np.float64
    m = stepped_model(float_type, grid_type, steps=20)
    o = stepped_model(float_type, grid_type, steps=20, arch=CPU("f32" if float_type == "Float32" else "f64"))
    d_dev, n = eta_drift(m)
    d_ora, n_o = eta_drift(o)
    floor = n * float(np.finfo(real).eps)
    print(f"  {float_type} grid {grid_type}: d_device {d_dev:.3e} d_oracle {d_ora:.3e} n eps {floor:.3e}")
    assert n == n_o and np.abs(m.backend.get_field("eta", False)).max() > 0
    assert d_dev <= 10 * max(d_ora, floor)
    m.backend.close()
