"""Sums in classes on the device (gb25_get_class_sums) against the numpy restatement (gb-25_amd/classes.py, pinned on the CPU by
tests/test_classes_host.py) BIT FOR BIT -- the order of every sum is part of the ABI --, against the transports and the integrals
that exist, and the proof that asking for them changes nothing a model computes.

Where two different orders of the same n terms are compared (the depth-integrated transport of a row, the volume of the ocean, the
ranks of a decomposition) the bound is the one of tests/test_gpu_transports.py: any order of n fp64 terms is within (n - 1) eps
sum|term| of the exact sum, forming a term costs at most four roundings: (n + 4) eps fsum(|terms|)."""
import ctypes
import math

import numpy as np
import pytest

import gb25_amd as gb
from gb25_amd.binding import CLASS_SUM_DTYPE, FIELD_IDS, KERNEL_IDS, ClassSum
from gb25_amd.classes import (class_edges, class_sums_host, class_terms, class_values, fold_classes, total_classes)
from gb25_amd.distributed import LocalSlabEnsemble
from gb25_amd.integrals import cell_measure
from gb25_amd.transports import transport_terms
from helpers import BASE_FIELDS, CASES, CATKE_FIELDS, EPS, GRID_NAMES, counter_rng, size_of, stepped_model

pytestmark = pytest.mark.gpu
WHAT = ("faces_y", "cells")
VARIABLES = ("T", "S", "potential_density")
SHAPES = ("rows", "cumulative", "total")
SUMS = ("measure", "flow", "heat", "salt")
BINS = (2, 7, 64, 65, 256)     # 64 -> 65: a lane gets a second bin; 256 fills LDS


def edges_for(b, variable, B):
    """B - 1 evenly spaced edges over the range the variable takes in the interior (B = 2: the middle of it)."""
    Ny = b.field_dims("T", False)[1]
    x = class_values(b, variable)[:, 1:Ny + 1]
    lo, hi = float(np.nanmin(x)), float(np.nanmax(x))
    if not hi > lo:
        hi = lo + 1.0
    return np.array([0.5 * (lo + hi)]) if B == 2 else class_edges(lo, hi, B - 1)


def all_edges(b, B):
    return {v: edges_for(b, v, B) for v in VARIABLES}


def check_bit_for_bit(b, B, window=None, what_text=""):
    for variable, edges in all_edges(b, B).items():
        for what in WHAT:
            tag = (what_text, what, variable, B, window)
            rows = b.class_sums(what, variable, edges, "rows", window)
            want = class_sums_host(b, what, variable, edges, "rows", window)
            assert rows.shape == want.shape and rows.dtype == CLASS_SUM_DTYPE, tag
            assert np.array_equal(rows["count"], want["count"]) and np.array_equal(rows["nonfinite"], want["nonfinite"]), tag
            for f in SUMS:
                assert np.ascontiguousarray(rows[f]).tobytes() == np.ascontiguousarray(want[f]).tobytes(), tag + (f,)
            assert rows.tobytes() == want.tobytes(), tag
            assert rows["count"].sum() > 0 and np.abs(rows["heat"]).max() > 0, tag
            assert b.class_sums(what, variable, edges, "cumulative", window).tobytes() == fold_classes(rows).tobytes(), tag
            assert b.class_sums(what, variable, edges, "total", window).tobytes() == total_classes(rows).tobytes(), tag
            assert b.class_sums(what, variable, edges, "rows", window).tobytes() == rows.tobytes(), tag     # (repeatable)


@pytest.mark.parametrize("float_type,grid_type", CASES)
def test_bit_for_bit(float_type, grid_type):
    m = stepped_model(float_type, grid_type)
    b = m.backend
    for B in BINS:
        check_bit_for_bit(b, B, None, f"{float_type} grid {grid_type}")
    edges = edges_for(b, "potential_density", 21)
    psi = gb.overturning_in_classes(m, edges)
    assert psi.shape == (b.field_dims("v", False)[1], 22) and (psi[:, 0] == 0).all()
    assert np.array_equal(psi, b.class_sums("faces_y", "potential_density", edges, "cumulative")["flow"])
    assert gb.water_mass_census(m, edges).tobytes() == b.class_sums("cells", "potential_density", edges, "total").tobytes()
    assert gb.water_mass_census(m, edges, "T", by_row=True).tobytes() == b.class_sums("cells", "T", edges, "rows").tobytes()
    b.close()


def test_bit_for_bit_on_a_width_that_fills_no_chunk():
    m = stepped_model("Float32", 1, size=(50, 24, 6))
    b = m.backend
    for B in (7, 65):
        check_bit_for_bit(b, B, None, "50 columns")
    b.close()


@pytest.mark.parametrize("float_type,grid_type", CASES)
def test_edges_on_stored_values(float_type, grid_type):
    """Edges that ARE class values of the cells (the face averages): a one-ulp disagreement between the kernel's class value and
    the host's moves a cell across an edge and shows in the counts."""
    m = stepped_model(float_type, grid_type)
    b = m.backend
    Ny = b.field_dims("T", False)[1]
    by = b.field_dims("v", False)[1]
    for variable in VARIABLES:
        cv = class_values(b, variable)
        wet = cell_measure(b, "T") > 0
        faces = transport_terms(b, "across_y")["counted"]
        values = {"cells": cv[:, 1:Ny + 1][wet], "faces_y": (0.5 * (cv[:, 0:by] + cv[:, 1:by + 1]))[faces]}
        for what in WHAT:
            distinct = np.unique(values[what])
            edges = distinct[np.linspace(0, distinct.size - 1, min(255, distinct.size)).astype(int)]
            edges = np.unique(edges)
            assert edges.size > 100 or variable == "S", (what, variable, edges.size)     # (S is nearly uniform in this flow)
            rows = b.class_sums(what, variable, edges)
            want = class_sums_host(b, what, variable, edges)
            assert np.array_equal(rows["count"], want["count"]), (what, variable)
            assert rows.tobytes() == want.tobytes(), (what, variable)
            # every edge is the value of a face (cell): the bin above it is not empty
            assert (rows["count"].sum(axis=0)[1:] > 0).all(), (what, variable)
    b.close()


def within(value, x):
    exact, bound = math.fsum(x), (len(x) + 4) * EPS * math.fsum(np.abs(x))
    return abs(float(value) - exact) <= bound, (float(value), exact, bound)


@pytest.mark.parametrize("float_type,grid_type", CASES)
def test_consistent_with_the_transports_and_the_integrals(float_type, grid_type):
    m = stepped_model(float_type, grid_type)
    b = m.backend
    B = 33
    t = transport_terms(b, "across_y")
    profile = b.transport("across_y", "profile")
    for variable, edges in all_edges(b, B).items():
        psi = b.class_sums("faces_y", variable, edges, "cumulative")
        assert np.array_equal(psi["count"][:, B], profile["faces"]) and np.array_equal(psi["nonfinite"][:, B], profile["nonfinite"])
        for f, g in zip(SUMS, ("area", "volume", "heat", "salt")):
            for n in range(psi.shape[0]):
                x = t[g][:, n, :][t["counted"][:, n, :]]
                ok, info = within(psi[f][n, B], x)
                assert ok, (variable, f, n, info)
                bound = (len(x) + 4) * EPS * math.fsum(np.abs(x))
                assert abs(float(psi[f][n, B]) - float(profile[g][n])) <= bound, (variable, f, n)
        total = b.class_sums("cells", variable, edges, "total")
        whole = b.integrate_field("T", "total")
        mu = cell_measure(b, "T")
        Tv = np.asarray(b.get_field("T", False), np.float64)
        assert total["count"].sum() == whole["points"] and total["nonfinite"].sum() == whole["nonfinite"] == 0
        ok, info = within(math.fsum(total["measure"]), mu[mu > 0])
        assert ok, (variable, info)
        bound = (int((mu > 0).sum()) + 4) * EPS * math.fsum(mu[mu > 0])
        assert abs(math.fsum(total["measure"]) - float(whole["measure"])) <= bound, variable
        ok, info = within(math.fsum(total["heat"]), (mu * Tv)[mu > 0])
        assert ok, (variable, "heat", info)
        assert (total["flow"] == 0).all() and not np.signbit(total["flow"]).any()
        # all edges above every value: everything in bin 0
        for what in WHAT:
            high = b.class_sums(what, variable, [1e6, 2e6, 3e6])
            assert (high["count"][:, 1:] == 0).all() and (high["measure"][:, 1:] == 0).all(), (what, variable)
            assert high["count"][:, 0].sum() == (profile["faces"].sum() if what == "faces_y" else whole["points"])
            low = b.class_sums(what, variable, [-3e6, -2e6])
            assert (low["count"][:, :2] == 0).all() and low["count"][:, 2].sum() == high["count"][:, 0].sum()
    b.close()


@pytest.mark.parametrize("float_type,grid_type,size", [("Float32", 1, None), ("Float64", 4, None), ("Float32", 1, (50, 24, 6))])
def test_windows(float_type, grid_type, size):
    m = stepped_model(float_type, grid_type, size=size)
    b = m.backend
    Nx, Ny, Nz = size or size_of(grid_type)
    by = b.field_dims("v", False)[1]
    for w in ((3, 41), (1, 1), (Nx - 3, -1)):
        check_bit_for_bit(b, 70, w, f"{float_type} grid {grid_type} {Nx} columns")
    edges = edges_for(b, "T", 70)
    whole = b.class_sums("cells", "T", edges)
    parts = [b.class_sums("cells", "T", edges, "rows", w) for w in ((0, 20), (20, -1))]
    assert np.array_equal(parts[0]["count"] + parts[1]["count"], whole["count"])
    # empty and out-of-range windows through the ABI
    E = (ctypes.c_double * edges.size)(*edges)
    B = edges.size + 1
    out = (ClassSum * ((by + 1) * (B + 1)))()
    call = b.lib.gb25_get_class_sums
    for what, n in ((0, by), (1, Ny)):
        assert call(b.h, what, 0, E, edges.size, 0, 0, -1, out, n * B) == 0
        for first, count in ((0, 0), (Nx, 1), (-1, 2), (Nx - 2, 3), (0, Nx + 1), (3, -2)):
            assert call(b.h, what, 0, E, edges.size, 0, first, count, out, n * B) == 1, (what, first, count)
            assert b"window" in b.lib.gb25_last_error_string(b.h)
    with pytest.raises(gb.GB25Error, match="window"):
        b.class_sums("cells", "T", edges, "rows", (Nx, 1))
    b.close()


@pytest.mark.parametrize("float_type,grid_type", [("Float32", 1), ("Float64", 4)])
def test_a_nan_in_a_wet_cell(float_type, grid_type):
    m = stepped_model(float_type, grid_type, steps=0)
    b = m.backend
    Nx, Ny, Nz = size_of(grid_type)
    ay = transport_terms(b, "across_y")["area"]
    i, j, k = next((i, j, k) for k in range(Nz) for j in range(3, Ny - 3) for i in range(3, Nx - 3)
                   if ay[i, j, k] > 0 and ay[i, j + 1, k] > 0)
    every = all_edges(b, 12)
    before = {(w, v): b.class_sums(w, v, every[v]) for w in WHAT for v in VARIABLES}
    T = b.get_field("T", False).copy()
    T[i, j, k] = np.nan
    b.set_field("T", T, False)
    for (what, variable), old in before.items():
        edges = every[variable]
        new = b.class_sums(what, variable, edges)
        want = np.zeros(new.shape, np.int64)
        hit = [j, j + 1] if what == "faces_y" else [j]
        want[hit, 0] = 1
        assert np.array_equal(new["nonfinite"], want), (what, variable)
        for f in SUMS:
            assert np.isfinite(new[f]).all(), (what, variable, f)
        other = np.ones(new.shape[0], bool)
        other[hit] = False
        assert new[other].tobytes() == old[other].tobytes(), (what, variable)
        assert np.array_equal(new["count"][hit].sum(axis=1), old["count"][hit].sum(axis=1) - 1), (what, variable)
        assert new.tobytes() == class_sums_host(b, what, variable, edges).tobytes(), (what, variable)
        total = b.class_sums(what, variable, edges, "total")
        assert total["nonfinite"][0] == len(hit) and total["nonfinite"][1:].sum() == 0
    b.close()


LOOKAHEADS = dict(subcycle_lookahead=1, ab2_lookahead=1)


@pytest.mark.parametrize("float_type,grid_type,catke", [("Float32", 0, False), ("Float64", 4, False), ("Float32", 4, False),
                                                        ("Float32", 0, True)])
def test_class_sums_are_read_only(float_type, grid_type, catke):
    """Two identical models; one is asked for every shape, variable and kind between every two steps.  Same bits, same look-ahead
    state, same launches of every phase of a step."""
    closure = gb.CATKEVerticalDiffusivity() if catke else None
    watched = stepped_model(float_type, grid_type, steps=0, closure=closure, **LOOKAHEADS)
    alone = stepped_model(float_type, grid_type, steps=0, closure=closure, **LOOKAHEADS)
    names = BASE_FIELDS + (CATKE_FIELDS if catke else [])
    edges = class_edges(0.0, 40.0, 80)
    for m in (watched, alone):
        m.backend.profile_enable(True)
        m.backend.profile_reset()
    for step in range(6):
        if step % 2 == 0:
            before = watched.backend.lookahead_state()
            for what in WHAT:
                for variable in VARIABLES:
                    for shape in SHAPES:
                        r = watched.backend.class_sums(what, variable, edges, shape, None if step else (1, 7))
                        assert r["nonfinite"].sum() == 0 and r["count"].sum() > 0
            assert watched.backend.lookahead_state() == before
        for m in (watched, alone):
            gb.time_step(m)
        assert watched.backend.lookahead_state() == alone.backend.lookahead_state(), step
    assert alone.backend.lookahead_state()[0], "the velocity look-ahead is on in this configuration"
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


def test_repeatable_on_two_models():
    m1, m2 = stepped_model("Float32", 4), stepped_model("Float32", 4)
    every = all_edges(m1.backend, 100)
    for what in WHAT:
        for variable, edges in every.items():
            for shape in SHAPES:
                s = [m.backend.class_sums(what, variable, edges, shape).tobytes() for m in (m1, m1, m2)]
                assert s[0] == s[1] == s[2], (what, variable, shape)
    m1.backend.close()
    m2.backend.close()


DECOMPOSITIONS = [(2, 1), (4, 1), (4, 2)]


@pytest.mark.parametrize("grid_type", [1, 4])
@pytest.mark.parametrize("P,Ry", DECOMPOSITIONS)
def test_combined_class_sums_of_the_ranks(P, Ry, grid_type):
    if Ry == 1:
        Nx, Ny, Nz, dt, kw = 96 * P // 2, 40, 10, 600.0, {}
    else:
        Nx, Ny, Nz, dt, kw = 128, 48 * Ry, 8, 600.0, dict(slab_mode=1)
    single = gb.baroclinic_instability_model(gb.GPU(), Nx, Ny, Nz, dt=dt, grid_type=GRID_NAMES[grid_type])
    gb.set_baroclinic_instability(single)
    vrows = Ny if grid_type == 4 else Ny + 1
    single.set(u=(1e-2 * counter_rng((Nx, Ny, Nz), 42, 1)).astype(np.float32),
               v=(1e-2 * counter_rng((Nx, vrows, Nz), 42, 2)).astype(np.float32),
               eta=(1e-2 * counter_rng((Nx, Ny, 1), 42, 3)).astype(np.float32))
    init = {n: single.backend.get_field(n, False) for n in ("u", "v", "T", "S", "eta")}
    ens = LocalSlabEnsemble(Nx, Ny, Nz, P, dt=dt, ranks_y=Ry, grid_type=grid_type, options=dict(w_on_the_fly=0), **kw)
    for n, a in init.items():
        ens.scatter(n, a)
    gb.first_time_step(single)
    ens.first_time_step()
    gb.loop(single, 4)
    ens.loop(4)
    sb = single.backend
    for name in ("v", "T", "S"):
        assert np.array_equal(ens.gather(name), sb.get_field(name, False)), name     # (the premise)
    B = 9
    every = all_edges(sb, B)
    for what in WHAT:
        for variable in ("potential_density", "T"):
            edges = every[variable]
            for window in (None, (Nx // (P // Ry) - 5, 11)):     # (the window straddles a seam between two ranks)
                tag = f"{P} ranks ({Ry} in y) grid {grid_type} {what} {variable} window {window}"
                rows, one = ens.class_sums(what, variable, edges, "rows", window), sb.class_sums(what, variable, edges, "rows", window)
                # the counts of every bin are the single domain's: the first row of faces of a northern rank bins the class of the
                # tracer halo row exactly as the single domain bins the interior row
                assert rows.shape == one.shape and np.array_equal(rows["count"], one["count"]), tag
                assert rows["nonfinite"].sum() == 0 and rows["count"].sum() > 0, tag
                t = class_terms(sb, what, variable, edges, window)
                for f in SUMS:
                    for n in range(rows.shape[0]):
                        for bin_ in range(B):
                            x = t[f][:, n, :][t["bin"][:, n, :] == bin_]
                            ok, info = within(rows[f][n, bin_], x)
                            assert ok, (tag, f, n, bin_, "combined", info)
                            ok, info = within(one[f][n, bin_], x)
                            assert ok, (tag, f, n, bin_, "single", info)
                assert ens.class_sums(what, variable, edges, "cumulative", window).tobytes() == fold_classes(rows).tobytes(), tag
                assert ens.class_sums(what, variable, edges, "total", window).tobytes() == total_classes(rows).tobytes(), tag
    with pytest.raises(ValueError):
        ens.class_sums("cells", "T", every["T"], "rows", (Nx, 1))
    ens.close()
    sb.close()


def test_argument_errors_through_the_abi():
    m = stepped_model("Float32", 0, steps=0)
    b = m.backend
    Nx, Ny, Nz = size_of(0)
    by = b.field_dims("v", False)[1]
    call = b.lib.gb25_get_class_sums
    out = (ClassSum * ((by + 1) * 257))()

    def edges_of(values):
        return (ctypes.c_double * len(values))(*values)

    good = edges_of([10.0, 20.0, 30.0])
    assert call(b.h, 0, 2, good, 3, 0, 0, -1, out, by * 4) == 0 and call(b.h, 1, 2, good, 3, 0, 0, -1, out, Ny * 4) == 0
    assert call(b.h, 0, 2, good, 3, 1, 0, -1, out, by * 5) == 0 and call(b.h, 0, 2, good, 3, 2, 0, -1, out, 4) == 0
    for bad in ([20.0, 10.0, 30.0], [10.0, 10.0, 30.0], [10.0, float("nan"), 30.0], [10.0, 20.0, float("inf")],
                [float("-inf"), 20.0, 30.0]):
        assert call(b.h, 0, 2, edges_of(bad), 3, 0, 0, -1, out, by * 4) == 1, bad
        assert b"edges" in b.lib.gb25_last_error_string(b.h)
    many = edges_of(list(np.arange(256.0)))
    assert call(b.h, 0, 2, many, 0, 0, 0, -1, out, by) == 1 and b"n_edges" in b.lib.gb25_last_error_string(b.h)
    assert call(b.h, 0, 2, many, 256, 0, 0, -1, out, by * 257) == 1 and b"n_edges" in b.lib.gb25_last_error_string(b.h)
    assert call(b.h, 0, 2, many, 255, 0, 0, -1, out, by * 256) == 0
    for what, n in ((0, by), (1, Ny)):
        for shape, count in ((0, n), (0, n * 4 + 1), (1, n * 4), (1, n * 5 - 1), (2, n * 4), (2, 0), (2, 5)):
            assert call(b.h, what, 2, good, 3, shape, 0, -1, out, count) == 1, (what, shape, count)
            assert b"count" in b.lib.gb25_last_error_string(b.h)
    assert call(b.h, 2, 2, good, 3, 0, 0, -1, out, by * 4) == 1 and call(b.h, 0, 3, good, 3, 0, 0, -1, out, by * 4) == 1
    assert call(b.h, 0, 2, good, 3, 3, 0, -1, out, by * 4) == 1 and call(b.h, 0, 2, None, 3, 0, 0, -1, out, by * 4) == 1
    assert b.lib.gb25_class_sum_bytes() == ctypes.sizeof(ClassSum) == CLASS_SUM_DTYPE.itemsize == 48
    with pytest.raises(ValueError):
        class_sums_host(b, "cells", "T", [2.0, 1.0])
    b.close()
