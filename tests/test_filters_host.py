"""The moving-window filter, the parts that need no GPU: the numpy restatement of gb-25_amd/filters.py (it is what the device's
planes are compared with bit for bit in tests/test_gpu_filters.py, so it is pinned here independently of the HIP kernels) against
a loop-by-loop statement of the definition of include/gb25.h, radius (0, 0) against the block sums of single points, the seam
under a cyclic shift, a constant field, a planted NaN, windows taller than the grid, the weights, the radius per row, and the
fallback of the public functions on the oracle backend."""
import numpy as np
import pytest

import gb25_amd as gb
from gb25_amd.blocks import block_sums_host
from gb25_amd.filters import (MAX_RADIUS, FilterSums, check_window, filter_of_planes, filter_sums_host, kernel_weights,
                              rows_for_length)
from gb25_amd.integrals import cell_measure
from helpers import counter_rng, size_of, stepped_model
from oracle_backend import CPU

EPS = float(np.finfo(np.float64).eps)
_MODELS = {}


@pytest.fixture(scope="module", autouse=True)
def _close_models():
    yield
    for m in _MODELS.values():
        m.backend.close()
    _MODELS.clear()


def oracle_of(grid_type):
    """One oracle model per grid type for the whole module, one step in."""
    if grid_type not in _MODELS:
        _MODELS[grid_type] = stepped_model("Float64", grid_type, steps=0, arch=CPU("f64"), dt=60.0 if grid_type == 3 else None)
    return _MODELS[grid_type]


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def loop_reference(x, mu, radius, stride, wx=None, wy=None, rows=None):
    """The definition, point by point, in Python floats: the terms, the x sums of every row (ascending d, the seam by index), the
    y sums (ascending e, rows outside skipped); every sum from +0.0."""
    Nx, Ny, n = x.shape
    (rx, ry), (sx, sy) = radius, stride
    nI, nJ = Nx // sx, Ny // sy
    out = np.zeros((3, nI, nJ, n))
    nonfinite = 0
    for k in range(n):
        terms = [[None] * Ny for _ in range(Nx)]
        for i in range(Nx):
            for j in range(Ny):
                m, v = float(mu[i, j, k]), float(x[i, j, k])
                if m > 0.0 and np.isfinite(v):
                    t = m * v
                    terms[i][j] = (m, t, t * v)
                else:
                    terms[i][j] = (0.0, 0.0, 0.0)
                    nonfinite += 1 if m > 0.0 else 0
        for I in range(nI):
            s = [None] * Ny
            for j in range(Ny):
                r = rx if rows is None else int(rows[j])
                acc = [0.0, 0.0, 0.0]
                for d in range(-r, r + 1):
                    term = terms[(I * sx + d) % Nx][j]
                    for p in range(3):
                        acc[p] = acc[p] + (term[p] if wx is None else float(wx[d + rx]) * term[p])
                s[j] = acc
            for J in range(nJ):
                acc = [0.0, 0.0, 0.0]
                for e in range(-ry, ry + 1):
                    jj = J * sy + e
                    if jj < 0 or jj >= Ny:
                        continue
                    for p in range(3):
                        acc[p] = acc[p] + (s[jj][p] if wy is None else float(wy[e + ry]) * s[jj][p])
                out[:, I, J, k] = acc
    return out[0], out[1], out[2], nonfinite


def test_the_restatement_equals_the_loop():
    """48 x 24 x 6 islands, fp64: radii (2, 3), stride (4, 2), Gaussian weights, one rx_of_row vector with differing entries."""
    b = oracle_of(1).backend
    Nx, Ny, Nz = size_of(1)
    ladder = np.array([(3 * j) % 7 for j in range(Ny)], np.int32)
    assert len(set(ladder.tolist())) > 3
    gauss = (kernel_weights("gaussian", 2), kernel_weights("gaussian", 3))
    for name in ("T", "u", "v", "eta"):
        x = np.asarray(b.get_field(name, False), np.float64)[:, :Ny]
        mu = cell_measure(b, name)[:, :Ny]
        for stride, wx, wy, rows in (((1, 1), None, None, None), ((4, 2), None, None, None), ((1, 1), gauss[0], gauss[1], None),
                                     ((4, 2), gauss[0], None, None), ((1, 1), None, None, ladder), ((4, 2), None, gauss[1], ladder)):
            got = filter_of_planes(x, mu, (2, 3), stride, wx, wy, rows)
            want = loop_reference(x, mu, (2, 3), stride, wx, wy, rows)
            for q in range(3):
                assert same(got[q], want[q]), (name, stride, wx is not None, wy is not None, rows is not None, q)
            assert got[3] == want[3] == 0
            assert (want[1] != 0).any()
        host = filter_sums_host(b, name, (2, 3), (4, 2), None, gauss[0], gauss[1])
        want = loop_reference(x, mu, (2, 3), (4, 2), gauss[0], gauss[1])
        assert same(host.measure, want[0]) and same(host.first, want[1]) and same(host.second, want[2]), name
        assert host.dims == (Nx // 4, Ny // 2, x.shape[2]) and host.empty == int((want[0] == 0).sum())
    # a window of levels
    x = np.asarray(b.get_field("T", False), np.float64)
    mu = cell_measure(b, "T")
    host = filter_sums_host(b, "T", (2, 3), (4, 2), (1, -1))
    want = loop_reference(x[:, :, 1:], mu[:, :, 1:], (2, 3), (4, 2))
    assert host.dims[2] == Nz - 1 and same(host.first, want[1]) and same(host.measure, want[0])


@pytest.mark.parametrize("grid_type", [0, 4])
def test_radius_zero_is_the_block_sums_of_single_points(grid_type):
    b = oracle_of(grid_type).backend
    for name in ("T", "u", "v", "w", "eta"):
        f, s = filter_sums_host(b, name, (0, 0)), block_sums_host(b, name, (1, 1, 1))
        assert same(f.measure, s.measure) and same(f.first, s.first) and same(f.second, s.second), name
        assert f.dims == s.dims and f.empty == s.empty_blocks and f.nonfinite == s.nonfinite == 0 and f.clipped == 0
        assert (f.first != 0).any()


def test_a_cyclic_shift_shifts_every_plane():
    """The seam: on the lat-lon grid mu does not depend on i, so a field rolled in i gives rolled planes, bit for bit."""
    b = oracle_of(0).backend
    Nx, Ny, Nz = size_of(0)
    x = np.asarray(b.get_field("T", False), np.float64) + counter_rng((Nx, Ny, Nz), 11, 1)
    mu = cell_measure(b, "T")
    assert same(mu, np.roll(mu, 5, axis=0))
    gauss = kernel_weights("gaussian", 7)
    for radius, wx in (((7, 2), None), ((7, 2), gauss), ((31, 0), None)):
        base = filter_of_planes(x, mu, radius, (1, 1), wx)
        for shift in (1, 5, Nx - 3):
            moved = filter_of_planes(np.roll(x, shift, axis=0), mu, radius, (1, 1), wx)
            for q in range(3):
                assert same(moved[q], np.roll(base[q], shift, axis=0)), (radius, shift, q)
        assert not same(base[1], np.roll(base[1], 1, axis=0))


@pytest.mark.parametrize("grid_type", [1, 4])
def test_a_constant_field(grid_type):
    """|xbar - c| <= (2 n + 4) eps |c| with n the points of the largest window: each of the two sums of n non-negative terms
    carries at most n roundings per term, the quotient adds one; the variance within the same bound times c^2."""
    b = oracle_of(grid_type).backend
    Nx, Ny, Nz = size_of(grid_type)
    mu = cell_measure(b, "T")
    c = 3.7
    for radius, w in (((2, 3), None), ((5, 4), kernel_weights("gaussian", 5))):
        wy = None if w is None else kernel_weights("gaussian", radius[1])
        m, t, q, _ = filter_of_planes(np.full(mu.shape, c), mu, radius, (1, 1), w, wy)
        sums = FilterSums(m, t, q, radius=radius, stride=(1, 1), dims=m.shape, nonfinite=0, empty=int((m == 0).sum()), clipped=0)
        n = (2 * radius[0] + 1) * (2 * radius[1] + 1)
        full = m > 0
        bound = (2 * n + 4) * EPS * abs(c)
        err = np.abs(sums.mean()[full] - c).max()
        var = sums.variance()[full].max()
        print(f"  grid {grid_type} radius {radius}: max |xbar - c| {err:.3e} bound {bound:.3e}, max variance {var:.3e} bound {bound * abs(c):.3e}, "
              f"empty {sums.empty}")
        assert full.any() and err <= bound and var <= bound * abs(c)
        assert np.isnan(sums.mean()[~full]).all()


def test_a_planted_nan():
    b = oracle_of(1).backend
    Nx, Ny, Nz = size_of(1)
    x = np.array(b.get_field("T", False), np.float64)
    mu = cell_measure(b, "T")
    radius = (2, 3)
    before = filter_of_planes(x, mu, radius)
    wet = np.argwhere(mu[:, :, Nz - 1] > 0)
    i0, j0 = (int(q) for q in wet[len(wet) // 2])
    x[i0, j0, Nz - 1] = np.nan
    after = filter_of_planes(x, mu, radius)
    assert after[3] == 1 and before[3] == 0
    inside = np.zeros(mu.shape, bool)
    for d in range(-radius[0], radius[0] + 1):
        for e in range(-radius[1], radius[1] + 1):
            if 0 <= j0 + e < Ny:
                inside[(i0 + d) % Nx, j0 + e, Nz - 1] = True
    for q in range(3):
        assert np.isfinite(after[q]).all()
        changed = after[q] != before[q]
        assert np.array_equal(changed, inside) if q == 0 else not changed[~inside].any(), q
    assert (after[1] != before[1])[inside].sum() >= inside.sum() - 1      # (T is nowhere 0 there)
    # one in an immersed cell is invisible
    dry = np.argwhere(mu[:, :, 0] == 0)
    i1, j1 = (int(q) for q in dry[len(dry) // 2])
    x[i1, j1, 0] = np.inf
    again = filter_of_planes(x, mu, radius)
    assert again[3] == 1 and all(same(again[q], after[q]) for q in range(3))


def test_a_window_taller_than_the_grid():
    b = oracle_of(1).backend
    Nx, Ny, Nz = size_of(1)
    assert MAX_RADIUS >= Ny
    tall = filter_sums_host(b, "T", (1, Ny), (1, 2))
    assert tall.clipped == tall.dims[0] * tall.dims[1] * tall.dims[2] == Nx * (Ny // 2) * Nz
    assert same(tall.first, filter_sums_host(b, "T", (1, MAX_RADIUS), (1, 2)).first)      # (every row is in every window)
    assert same(tall.first[:, 0], tall.first[:, 1])
    part = filter_sums_host(b, "T", (1, 3))
    assert part.clipped == Nx * 6 * Nz
    assert filter_sums_host(b, "T", (1, 0)).clipped == 0


def test_the_weights_and_the_checks():
    for kind in ("box", "gaussian", "triangle"):
        for r in (0, 1, 4, MAX_RADIUS):
            w = kernel_weights(kind, r)
            assert w.shape == (2 * r + 1,) and w.dtype == np.float64 and (w > 0).all() and same(w, w[::-1].copy()) and w[r] == w.max()
    with pytest.raises(ValueError, match="kernel"):
        kernel_weights("cosine", 2)
    for word, kw in (("rx", dict(radius=(-1, 0))), ("rx", dict(radius=(MAX_RADIUS + 1, 0))), ("ry", dict(radius=(0, MAX_RADIUS + 1))),
                     ("ry", dict(radius=(0, -2))), ("rx", dict(radius=(24, 0))), ("sx", dict(radius=(1, 1), stride=(5, 1))),
                     ("sy", dict(radius=(1, 1), stride=(1, 0))), ("wx", dict(radius=(1, 1), wx=[1.0, -1.0, 1.0])),
                     ("wx", dict(radius=(1, 1), wx=[1.0, np.nan, 1.0])), ("wy", dict(radius=(1, 1), wy=[0.0, 0.0, 0.0])),
                     ("wy", dict(radius=(1, 1), wy=[1.0, 1.0])), ("rx_of_row", dict(radius=(1, 1), wx=[1.0, 1.0, 1.0], rx_of_row=[1] * 24)),
                     ("rx_of_row", dict(radius=(1, 1), rx_of_row=[1] * 23)), ("rx_of_row", dict(radius=(1, 1), rx_of_row=[24] * 24))):
        with pytest.raises(ValueError, match=word):
            check_window(48, 24, **kw)
    b = oracle_of(1).backend
    for word, call in (("window", lambda: filter_sums_host(b, "T", (1, 1), levels=(6, 1))), ("window", lambda: filter_sums_host(b, "eta", (1, 1), levels=(0, 2))),
                       ("vorticity", lambda: filter_sums_host(b, "vorticity", (1, 1)))):
        with pytest.raises(ValueError, match=word):
            call()


def test_rows_for_length_is_monotone_in_latitude():
    b = oracle_of(0).backend
    Nx, Ny, Nz = size_of(0)
    lat = np.array([b.metric("phic", j) for j in range(1, Ny + 1)])
    rows = rows_for_length(b, "T", 2.0e6)
    assert rows.dtype == np.int32 and rows.shape == (Ny,) and (rows >= 0).all() and (rows <= min(MAX_RADIUS, (Nx - 1) // 2)).all()
    order = np.argsort(np.abs(lat), kind="stable")
    assert (np.diff(rows[order]) >= 0).all() and rows[order][-1] > rows[order][0], rows
    dx = np.array([b.metric("dxc", j) for j in range(1, Ny + 1)])
    free = rows < min(MAX_RADIUS, (Nx - 1) // 2)
    assert free.any() and (np.abs((2 * rows[free]) * dx[free] - 2.0e6) <= dx[free]).all()      # (the width that was asked for, to a point)
    assert same(rows_for_length(b, "u", 2.0e6), rows)
    curv = rows_for_length(oracle_of(4).backend, "T", 1.0e6)
    assert curv.shape == (size_of(4)[1],) and (curv >= 0).all() and curv.max() > curv.min()
    # a radius per row is what the filter takes
    sums = filter_sums_host(b, "T", (0, 2), rx_of_row=rows)
    assert sums.dims == (Nx, Ny, Nz) and sums.empty == 0 and np.isfinite(sums.mean()).all()


def test_the_public_functions_fall_back_on_the_oracle_backend():
    m = oracle_of(1)
    b = m.backend
    Nx, Ny, Nz = size_of(1)
    host = filter_sums_host(b, "T", (2, 3))
    assert np.array_equal(gb.filtered(m, "T", (2, 3)), host.mean(), equal_nan=True)
    assert np.array_equal(m.tracers.T.filtered((2, 3)), host.mean(), equal_nan=True)
    assert np.array_equal(gb.subfilter_variance(m, "T", (2, 3)), host.variance(), equal_nan=True)
    g = filter_sums_host(b, "u", (4, 2), (4, 2), (Nz - 1, 1), kernel_weights("gaussian", 4), kernel_weights("gaussian", 2))
    assert np.array_equal(gb.filtered(m, "u", (4, 2), kernel="gaussian", stride=(4, 2), levels=(Nz - 1, 1)), g.mean(), equal_nan=True)
    rows = rows_for_length(b, "T", 1.5e6)
    by_length = filter_sums_host(b, "T", (0, 1), rx_of_row=rows)
    assert np.array_equal(gb.filtered(m, "T", (0, 1), length=1.5e6), by_length.mean(), equal_nan=True)
    ke = gb.filtered(m, "kinetic_energy", (2, 2))
    assert ke.shape == (Nx, Ny, Nz) and np.nanmax(ke) > 0
    eddy = gb.eddy_part(m, "T", (2, 3))
    mu = cell_measure(b, "T")
    x = np.asarray(b.get_field("T", False), np.float64)
    assert eddy.shape == (Nx, Ny, Nz) and np.array_equal(np.isnan(eddy), ~(mu > 0))
    wet = mu > 0
    assert np.array_equal(eddy[wet], (x - host.mean())[wet]) and (eddy[wet] != 0).any()
    # the eddy part of a filtered constant is 0 to rounding, and the variance of the parts adds up: mean(x'^2) is about the variance
    assert np.nanmax(np.abs(eddy)) < np.nanmax(np.abs(x))
