"""The cell measure and the host side of the integrals (gb-25_amd/integrals.py) on the CPU oracle's backend: the numpy
definition of mu = A dz fold wet (include/gb25.h) pinned independently of the HIP kernels.

Sums of n fp64 terms in any order lie within (n - 1) eps sum|term| of the exact sum (Higham, Accuracy and Stability of
Numerical Algorithms, eq. 4.4 to first order); forming mu (two roundings) and a term mu x, mu x x (two more) adds four, so the
bound asserted is (n + 4) eps sum|term|."""
import math

import numpy as np
import pytest

import gb25_amd as gb
from gb25_amd.integrals import cell_measure, combine_moments, fold_records, integrate_host
from helpers import make_oracle

R = 6371e3
EPS = float(np.finfo(np.float64).eps)


def test_the_measure_tiles_the_sphere_on_the_tripolar_grid():
    Nx, Ny = 72, 36
    m = make_oracle(Nx, Ny, 6, 600.0, grid_type="tripolar")
    mu = cell_measure(m.backend, "eta")
    assert mu.shape == (Nx, Ny, 1) and (mu > 0).all()
    dphi = 170.0 / (Ny - 1)
    want = 2 * math.pi * R * R * (1 + math.sin(math.radians(80 + dphi / 2)))
    print(f"  tripolar: sum mu {mu.sum()!r} sphere north of 80 S - dphi/2 {want!r}")
    assert mu.sum() == pytest.approx(want, rel=2e-5)
    # the 1/2 of the pivot row, on the rows of cell centres only
    az = np.array([[m.backend.metric2("azcc", i, j) for j in range(1, Ny + 1)] for i in range(1, Nx + 1)])
    assert np.array_equal(mu[:, Ny - 1, 0], 0.5 * az[:, Ny - 1]) and np.array_equal(mu[:, :Ny - 1, 0], az[:, :Ny - 1])
    azcf = np.array([[m.backend.metric2("azcf", i, j) for j in range(1, Ny + 1)] for i in range(1, Nx + 1)])
    muV = cell_measure(m.backend, "V")
    assert muV.shape == (Nx, Ny, 1) and np.array_equal(muV[:, 1:, 0], azcf[:, 1:]) and (muV[:, 0] == 0).all()
    assert integrate_host(m.backend, "eta")["measure"] == pytest.approx(want, rel=2e-5)


def test_the_measure_tiles_the_zone_on_the_lat_lon_grid():
    Nx, Ny = 72, 36
    m = make_oracle(Nx, Ny, 6, 600.0)
    mu = cell_measure(m.backend, "eta")
    want = R * R * 2 * math.pi * (math.sin(math.radians(80)) - math.sin(math.radians(-80)))
    print(f"  lat-lon: sum mu {mu.sum()!r} zone {want!r}")
    assert mu.shape == (Nx, Ny, 1) and mu.sum() == pytest.approx(want, rel=2e-5)


NX, NY, NZ = 8, 8, 4      # (the smallest model the oracle builds; the hand-built bottom occupies its 6 x 4 x 3 corner)


def hand_built(Nx=NX, Ny=NY, Nz=NZ):
    """A lat-lon model with three columns of different kbot put through set_bottom_height."""
    m = make_oracle(Nx, Ny, Nz, 600.0)
    b = m.backend
    zc = np.array([b.metric("zc", k) for k in range(1, Nz + 1)])
    zb = np.full((Nx, Ny), -1e30)
    zb[1, 1] = 0.5 * (zc[0] + zc[1])      # one immersed cell
    zb[2, 1] = 0.5 * (zc[1] + zc[2])      # two
    zb[4, 2] = 1.0                        # the whole column
    b.set_bottom_height(zb)
    kbot = np.zeros((Nx, Ny), int)
    kbot[1, 1], kbot[2, 1], kbot[4, 2] = 1, 2, Nz
    return m, kbot


def test_the_measure_of_a_hand_built_bottom():
    Nx, Ny, Nz = NX, NY, NZ
    m, kbot = hand_built(Nx, Ny, Nz)
    b = m.backend
    assert np.array_equal([[b.bottom_info("kbot", i, j) for j in range(1, Ny + 1)] for i in range(1, Nx + 1)], kbot)
    azc = np.array([b.metric("azc", j) for j in range(1, Ny + 1)])
    azf = np.array([b.metric("azf", j) for j in range(1, Ny + 2)])
    dzc = np.array([b.metric("dzc", k) for k in range(1, Nz + 1)])
    dzf = np.array([b.metric("dzf", k) for k in range(1, Nz + 2)])
    # T: cell k of column (i, j) is wet from level kbot on
    want = np.zeros((Nx, Ny, Nz))
    for i in range(Nx):
        for j in range(Ny):
            for k in range(Nz):
                want[i, j, k] = azc[j] * dzc[k] * (k >= kbot[i, j])
    assert np.array_equal(cell_measure(b, "T"), want)
    assert want[1, 1, 0] == 0 and want[1, 1, 1] > 0 and want[2, 1, 1] == 0 and want[2, 1, 2] > 0 and (want[4, 2] == 0).all()
    # u: the face between columns i - 1 (periodic) and i is wet where both are
    want = np.zeros((Nx, Ny, Nz))
    for i in range(Nx):
        for j in range(Ny):
            for k in range(Nz):
                want[i, j, k] = azc[j] * dzc[k] * (k >= max(kbot[i - 1, j], kbot[i, j]))
    assert np.array_equal(cell_measure(b, "u"), want)
    assert want[3, 1, 1] == 0 and want[3, 1, 2] > 0 and (want[5, 2] == 0).all() and (want[4, 2] == 0).all()
    # v: Ny + 1 rows of faces, both walls dry, the face between rows j - 1 and j wet where both are
    want = np.zeros((Nx, Ny + 1, Nz))
    for i in range(Nx):
        for j in range(1, Ny):
            for k in range(Nz):
                want[i, j, k] = azf[j] * dzc[k] * (k >= max(kbot[i, j - 1], kbot[i, j]))
    assert np.array_equal(cell_measure(b, "v"), want)
    assert want[1, 2, 0] == 0 and want[1, 2, 1] > 0 and (want[4, 3] == 0).all() and (want[:, 0] == 0).all() and (want[:, Ny] == 0).all()
    # w: Nz + 1 faces, wet where the cell above or the cell below is
    want = np.zeros((Nx, Ny, Nz + 1))
    for i in range(Nx):
        for j in range(Ny):
            for k in range(Nz + 1):
                above, below = k < Nz and k >= kbot[i, j], k >= 1 and k - 1 >= kbot[i, j]
                want[i, j, k] = azc[j] * dzf[k] * (above or below)
    assert np.array_equal(cell_measure(b, "w"), want)
    assert want[2, 1, 1] == 0 and want[2, 1, 2] > 0 and want[2, 1, 3] > 0 and (want[4, 2] == 0).all() and want[0, 0, 0] > 0
    # eta: the column has a wet cell
    want = np.zeros((Nx, Ny, 1))
    for i in range(Nx):
        for j in range(Ny):
            want[i, j, 0] = azc[j] * (kbot[i, j] < Nz)
    assert np.array_equal(cell_measure(b, "eta"), want)
    assert want[4, 2, 0] == 0 and want.sum() > 0


def check(got, terms, n, what):
    terms = np.asarray(terms, np.float64).ravel()
    exact, bound = math.fsum(terms), (n + 4) * EPS * math.fsum(np.abs(terms))
    print(f"    {what}: {got!r} fsum {exact!r} |diff| {abs(got - exact):.3e} bound {bound:.3e}")
    assert abs(got - exact) <= bound, (what, got, exact, bound)


def test_a_uniform_tracer():
    m, kbot = hand_built()
    b = m.backend
    mu = cell_measure(b, "T")
    b.set_field("T", np.where(mu > 0, 7.0, 0.0), False)
    rows, levels, total = (integrate_host(b, "T", s) for s in ("rows", "levels", "total"))
    n_row, n_level, n_all = NX, NX * NY, NX * NY * NZ
    assert rows.shape == (NY, NZ) and levels.shape == (NZ,) and total.shape == ()
    for j in range(NY):
        for k in range(NZ):
            check(rows[j, k]["measure"], mu[:, j, k], n_row, f"measure of row {j} {k}")
            check(rows[j, k]["first"], 7 * mu[:, j, k], n_row, f"first of row {j} {k}")
            check(rows[j, k]["second"], 49 * mu[:, j, k], n_row, f"second of row {j} {k}")
    for k in range(NZ):
        check(levels[k]["first"], 7 * mu[:, :, k], n_level, f"first of level {k}")
        check(levels[k]["second"], 49 * mu[:, :, k], n_level, f"second of level {k}")
        check(levels[k]["measure"], mu[:, :, k], n_level, f"measure of level {k}")
    check(total["measure"], mu, n_all, "measure")
    check(total["first"], 7 * mu, n_all, "first")
    check(total["second"], 49 * mu, n_all, "second")
    assert total["points"] == int((mu > 0).sum()) == n_all - 1 - 2 - NZ and total["nonfinite"] == 0
    # levels and the total are the left-to-right sums of the rows and of the levels, bit for bit
    for f in ("measure", "first", "second"):
        for k in range(NZ):
            acc = 0.0
            for j in range(NY):
                acc += float(rows[j, k][f])
            assert acc == levels[k][f]
        acc = 0.0
        for k in range(NZ):
            acc += float(levels[k][f])
        assert acc == total[f]
    # a value in an immersed cell is invisible, one in a wet cell is counted and skipped
    T = b.get_field("T", False).copy()
    T[4, 2, 1] = np.nan
    T[0, 0, 0] = np.inf
    b.set_field("T", T, False)
    t2 = integrate_host(b, "T")
    assert t2["nonfinite"] == 1 and t2["points"] == total["points"] - 1
    check(t2["measure"], np.where(np.isfinite(T), mu, 0.0), n_all, "measure without the skipped point")


class Half:
    """Half of the columns of a backend's field, measure included: a rank of an x decomposition as the host functions see
    one."""

    def __init__(self, backend, lo, hi):
        self.b, self.lo, self.hi = backend, lo, hi

    def records(self, name, shape):
        from gb25_amd.binding import MOMENTS_DTYPE
        x = np.asarray(self.b.get_field(name, False), np.float64)[self.lo:self.hi]
        mu = cell_measure(self.b, name)[self.lo:self.hi]
        rows = np.zeros(x.shape[1:], MOMENTS_DTYPE)
        rows["measure"], rows["first"], rows["second"] = mu.sum(axis=0), (mu * x).sum(axis=0), (mu * x * x).sum(axis=0)
        rows["points"] = (mu > 0).sum(axis=0)
        return rows if shape == "rows" else fold_records(rows) if shape == "levels" else fold_records(fold_records(rows))


def test_combining_the_halves_of_a_field():
    m, _ = hand_built()
    b = m.backend
    gb.set_baroclinic_instability(m)
    mu = cell_measure(b, "T")
    x = np.asarray(b.get_field("T", False), np.float64)
    n_all = NX * NY * NZ
    west, east = Half(b, 0, NX // 2), Half(b, NX // 2, NX)
    total = combine_moments([west.records("T", "total"), east.records("T", "total")])
    check(total["first"], mu * x, n_all, "combined first")
    check(total["second"], mu * x * x, n_all, "combined second")
    check(total["measure"], mu, n_all, "combined measure")
    assert total["points"] == n_all - 1 - 2 - NZ
    single = integrate_host(b, "T")
    assert abs(total["first"] - single["first"]) <= 2 * (n_all + 4) * EPS * math.fsum(np.abs(mu * x).ravel())
    rows = combine_moments([west.records("T", "rows"), east.records("T", "rows")])
    for f in ("measure", "first", "second", "points"):
        assert np.array_equal(rows[f], west.records("T", "rows")[f] + east.records("T", "rows")[f])
    # a mesh: the southern and the northern two rows, each in two halves of columns
    parts = [h.records("T", "rows")[j0:j0 + NY // 2] for j0 in (0, NY // 2) for h in (west, east)]
    stacked = combine_moments(parts, [0, 0, NY // 2, NY // 2])
    for f in ("measure", "first", "second", "points"):
        assert np.array_equal(stacked[f], rows[f])
