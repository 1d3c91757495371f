"""The bin rule, the terms and the host side of the sums in classes (gb-25_amd/classes.py) on synthetic arrays and on the CPU
oracle's backend: the numpy definitions of include/gb25.h ("sums in classes on the device") pinned independently of the HIP
kernel."""
import numpy as np
import pytest

import gb25_amd as gb
from gb25_amd.binding import CLASS_MAX_BINS, CLASS_SUM_DTYPE
from gb25_amd.classes import (SUMS, check_edges, class_bins, class_edges, class_sums_host, class_terms, class_values,
                              combine_class_sums, fold_classes, total_classes)
from gb25_amd.integrals import cell_measure
from gb25_amd.transports import transport_host, transport_terms
from helpers import make_oracle, set_noisy_velocities


def test_the_bin_rule():
    edges = np.array([-1.0, 0.0, 0.5, 2.0])
    below, above = np.nextafter(-1.0, -np.inf), np.nextafter(2.0, np.inf)
    values = np.array([-5.0, below, -1.0, -0.5, -0.0, 0.0, 0.25, 0.5, np.nextafter(0.5, 1.0), 2.0, above, 1e300])
    want = np.array([0, 0, 1, 1, 2, 2, 2, 3, 3, 4, 4, 4])
    assert np.array_equal(class_bins(edges, values), want)
    # a value equal to an edge belongs to the bin ABOVE the edge: the number of edges <= the value
    assert np.array_equal(class_bins(edges, values), [(edges <= v).sum() for v in values])
    assert class_bins([3.0], [2.0, 3.0, 4.0]).tolist() == [0, 1, 1]
    e = class_edges(20.0, 30.0, 11)
    assert e.size == 11 and e[0] == 20.0 and e[-1] == 30.0 and (np.diff(e) > 0).all()


def test_edges_that_are_refused():
    for bad in ([], [1.0, 1.0], [2.0, 1.0], [0.0, np.nan], [0.0, np.inf], np.arange(CLASS_MAX_BINS)):
        with pytest.raises(ValueError):
            check_edges(bad)
    assert check_edges(np.arange(CLASS_MAX_BINS - 1)).size == CLASS_MAX_BINS - 1
    with pytest.raises(ValueError):
        class_edges(1.0, 1.0, 4)


def synthetic_rows(n, B, seed):
    rng = np.random.default_rng(seed)
    r = np.zeros((n, B), CLASS_SUM_DTYPE)
    for f in SUMS:
        r[f] = rng.standard_normal((n, B)) * 10.0 ** rng.integers(-3, 9, (n, B))
    r["count"] = rng.integers(0, 50, (n, B))
    r["nonfinite"][:, 0] = rng.integers(0, 3, n)
    return r


def test_folding_rows():
    rows = synthetic_rows(7, 5, 1)
    psi = fold_classes(rows)
    assert psi.shape == (7, 6) and psi.dtype == CLASS_SUM_DTYPE
    total = total_classes(rows)
    assert total.shape == (5,) and total.dtype == CLASS_SUM_DTYPE
    for f in CLASS_SUM_DTYPE.names:
        for n in range(7):
            acc = type(rows[f][n, 0].item())(0)
            assert psi[f][n, 0] == 0
            for b in range(5):
                acc = acc + rows[f][n, b].item()
                assert psi[f][n, b + 1] == acc, (f, n, b)
        for b in range(5):
            acc = type(rows[f][0, b].item())(0)
            for n in range(7):
                acc = acc + rows[f][n, b].item()
            assert total[f][b] == acc, (f, b)


def test_combining_the_rows_of_two_slabs_and_of_a_mesh():
    B = 4
    w, e = synthetic_rows(5, B, 2), synthetic_rows(5, B, 3)
    got = combine_class_sums([w, e], "faces_y", [(0, 0), (6, 0)])
    for f in CLASS_SUM_DTYPE.names:
        assert np.array_equal(got[f], w[f] + e[f])
    # a 2 x 2 mesh: the southern ranks hold 4 rows of y faces (the seam row belongs to the northern ones), the northern ones 5
    sw, se, nw, ne = synthetic_rows(4, B, 6), synthetic_rows(4, B, 7), synthetic_rows(5, B, 8), synthetic_rows(5, B, 9)
    offsets = [(0, 0), (6, 0), (0, 4), (6, 4)]
    got = combine_class_sums([sw, se, nw, ne], "faces_y", offsets)
    assert got.shape == (9, B)
    for f in CLASS_SUM_DTYPE.names:
        assert np.array_equal(got[f][:4], sw[f] + se[f]) and np.array_equal(got[f][4:], nw[f] + ne[f])
    # rows of cells: 4 and 4
    parts = [synthetic_rows(4, B, s) for s in (10, 11, 12, 13)]
    got = combine_class_sums(parts, "cells", offsets)
    assert got.shape == (8, B)
    for f in CLASS_SUM_DTYPE.names:
        assert np.array_equal(got[f][:4], parts[0][f] + parts[1][f]) and np.array_equal(got[f][4:], parts[2][f] + parts[3][f])
    # CUMULATIVE and TOTAL are folded again from the combined rows
    assert combine_class_sums(parts, "cells", offsets, "cumulative").tobytes() == fold_classes(got).tobytes()
    assert combine_class_sums(parts, "cells", offsets, "total").tobytes() == total_classes(got).tobytes()
    with pytest.raises(ValueError):
        combine_class_sums(parts, "faces_x", offsets)
    with pytest.raises(ValueError):
        combine_class_sums(parts, "cells", offsets, "levels")


@pytest.fixture(scope="module")
def oracle():
    m = make_oracle(48, 24, 6, 600.0, "f64", grid_type="gaussian_islands_lat_lon")
    gb.set_baroclinic_instability(m)
    set_noisy_velocities(m)
    gb.first_time_step(m)
    gb.loop(m, 1)
    return m.backend


@pytest.mark.parametrize("variable", ["T", "S"])
def test_the_host_records(oracle, variable):
    b = oracle
    Nx, Ny, Nz = b.field_dims("T", False)
    x = np.asarray(b.get_field(variable, False), np.float64)
    edges = class_edges(x.min(), x.max(), 6)
    B = edges.size + 1
    # cells: every wet cell lands in the bin of its own value; the sums are the integrals'
    t = class_terms(b, "cells", variable, edges)
    mu = cell_measure(b, "T")
    assert np.array_equal(t["counted"], mu > 0) and not t["skipped"].any() and 0 < t["counted"].sum() < mu.size
    assert np.array_equal(t["bin"][t["counted"]], np.searchsorted(edges, x[t["counted"]], side="right"))
    assert (t["bin"][~t["counted"]] == -1).all() and (t["flow"] == 0).all()
    rows = class_sums_host(b, "cells", variable, edges)
    assert rows.shape == (Ny, B) and rows["count"].sum() == t["counted"].sum() and (rows["nonfinite"] == 0).all()
    assert (rows["flow"] == 0).all() and len(np.flatnonzero(rows["count"].sum(axis=0))) > 2
    assert np.allclose(rows["measure"].sum(), mu.sum(), rtol=1e-12, atol=0)
    # the order: p(n, k, b) sequentially over i, then left to right in k
    for f in ("measure", "heat"):
        for n in (3, 11):
            for bin_ in range(B):
                acc = 0.0
                for k in range(Nz):
                    p = 0.0
                    for i in range(Nx):
                        if t["bin"][i, n, k] == bin_:
                            p = p + t[f][i, n, k]
                    acc = acc + p
                assert acc == rows[f][n, bin_], (f, n, bin_)
    # faces: the class of a face is the mean of its two cells; the last cumulative column is the depth-integrated transport
    tf = class_terms(b, "faces_y", variable, edges)
    tt = transport_terms(b, "across_y")
    cv = class_values(b, variable)
    assert cv.shape == (Nx, Ny + 2, Nz) and np.array_equal(cv[:, 1:Ny + 1], x)
    assert np.array_equal(tf["counted"], tt["counted"]) and np.array_equal(tf["flow"], tt["volume"])
    mean = 0.5 * (cv[:, :-1] + cv[:, 1:])
    assert np.array_equal(tf["bin"][tf["counted"]], np.searchsorted(edges, mean[tf["counted"]], side="right"))
    psi = class_sums_host(b, "faces_y", variable, edges, "cumulative")
    rows = class_sums_host(b, "faces_y", variable, edges)
    assert psi.shape == (Ny + 1, B + 1) and psi.tobytes() == fold_classes(rows).tobytes()
    profile = transport_host(b, "across_y", "profile")
    assert np.array_equal(psi["count"][:, -1], profile["faces"])
    assert np.allclose(psi["flow"][:, -1], profile["volume"], rtol=1e-9, atol=1e-9 * np.abs(tt["volume"]).sum(axis=(0, 2)).max())
    assert class_sums_host(b, "faces_y", variable, edges, "total").tobytes() == total_classes(rows).tobytes()
    # all edges above every value: everything in bin 0
    high = class_sums_host(b, "cells", variable, [1e6, 2e6])
    assert (high["count"][:, 1:] == 0).all() and high["count"][:, 0].sum() == t["counted"].sum()
    # a window of i
    w = class_sums_host(b, "cells", variable, edges, window=(5, 9))
    assert w["count"].sum() == t["counted"][5:14].sum()


def test_a_nan_and_the_argument_errors(oracle):
    b = oracle
    edges = class_edges(5.0, 25.0, 5)
    T = b.get_field("T", False).copy()
    mu = cell_measure(b, "T")
    i, j, k = next((i, j, k) for k in range(6) for j in range(3, 20) for i in range(3, 40) if mu[i, j, k] > 0)
    before = class_sums_host(b, "cells", "T", edges)
    keep = T[i, j, k]
    T[i, j, k] = np.nan
    b.set_field("T", T, False)
    try:
        after = class_sums_host(b, "cells", "T", edges)
    finally:
        T[i, j, k] = keep
        b.set_field("T", T, False)
    want = np.zeros(after.shape, np.int64)
    want[j, 0] = 1
    assert np.array_equal(after["nonfinite"], want) and after["count"].sum() == before["count"].sum() - 1
    assert np.isfinite(after["heat"]).all()
    other = np.arange(after.shape[0]) != j
    assert after[other].tobytes() == before[other].tobytes()
    for bad in (dict(what="faces_x"), dict(variable="rho"), dict(shape="levels"), dict(edges=[2.0, 1.0]), dict(window=(48, 1)),
                dict(window=(0, 0))):
        kw = dict(what="cells", variable="T", edges=edges, shape="rows", window=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            class_sums_host(b, **kw)
    # the model-level entry points fall back to the host on a backend without the kernel
    m = type("M", (), {"backend": b})()
    psi = gb.overturning_in_classes(m, edges, "T")
    assert np.array_equal(psi, class_sums_host(b, "faces_y", "T", edges, "cumulative")["flow"])
    assert gb.water_mass_census(m, edges, "S").tobytes() == class_sums_host(b, "cells", "S", edges, "total").tobytes()
    assert gb.water_mass_census(m, edges, "S", by_row=True).shape == (24, 6)
