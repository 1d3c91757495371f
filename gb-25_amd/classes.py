"""Sums in classes on the host: the definitions of include/gb25.h ("sums in classes on the device") restated with numpy from a
backend's public getters alone, in fp64, with the order of every sum of the kernel (csrc/class_kernels.hpp, k_class_rows /
k_class_fold), so that the device's records equal these bit for bit; the host fallback of gb25_get_class_sums; and the arithmetic
that combines the records of the ranks of a decomposition.  Works on binding.HipBackend and, for the classes of T and S, on the
test suite's oracle backend.

    bin of a class value c       the number of edges e <= c: np.searchsorted(edges, c, side="right"); B = len(edges) + 1 bins
    class of a cell              T, S as stored, or the potential density as get_derived("potential_density") returns it
    class of a y face            0.5 (c(i,j-1,k) + c(i,j,k))
    "faces_y"                    the terms of transports.transport_terms("across_y"): measure = a, flow = q, heat = qT, salt = qS
    "cells"                      V = integrals.cell_measure("T"): measure = V, flow = 0, heat = V T, salt = V S

A wet face (cell) whose values and class are finite adds its terms to its bin and 1 to count; one with a value that is not finite
adds 1 to nonfinite of bin 0 of its row.  The level partial p(n, k, b) is the SEQUENTIAL sum over i ascending from +0.0;
ROWS[n, b] adds the partials left to right in k; CUMULATIVE[n, e] are the running sums over the bins from 0; TOTAL[b] adds the
rows south to north."""
import numpy as np

from .binding import CLASS_MAX_BINS, CLASS_SUM_DTYPE
from .integrals import _halo, cell_measure
from .transports import _window, transport_terms

SUMS = ("measure", "flow", "heat", "salt")
WHAT = ("faces_y", "cells")
VARIABLES = ("T", "S", "potential_density")
SHAPES = ("rows", "cumulative", "total")


def class_edges(lo, hi, n):
    """n evenly spaced edges from lo to hi inclusive: n + 1 classes, the first below lo, the last from hi on."""
    return check_edges(np.linspace(float(lo), float(hi), int(n)))


def check_edges(edges):
    """The edges as a float64 vector; ValueError unless they are 1 .. CLASS_MAX_BINS - 1 finite, strictly increasing numbers."""
    edges = np.array(edges, np.float64).reshape(-1)
    if not 1 <= edges.size <= CLASS_MAX_BINS - 1:
        raise ValueError(f"{edges.size} edges: must be 1 .. {CLASS_MAX_BINS - 1}")
    if not np.isfinite(edges).all() or not (np.diff(edges) > 0).all():
        raise ValueError("the edges must be finite and strictly increasing")
    return edges


def class_bins(edges, values):
    """The bin of every class value: the number of edges <= the value."""
    return np.searchsorted(check_edges(edges), values, side="right")


def _check(what, variable, shape="rows"):
    if what not in WHAT:
        raise ValueError(f"what must be one of {WHAT}, got {what!r}")
    if variable not in VARIABLES:
        raise ValueError(f"variable must be one of {VARIABLES}, got {variable!r}")
    if shape not in SHAPES:
        raise ValueError(f"shape must be one of {SHAPES}, got {shape!r}")


def class_values(backend, variable):
    """The class value of the cells of the local rows -1 .. Ny (the interior and one row of tracer cells either side), float64
    [i, Ny + 2, k].  T and S come from the parent array; the potential density from get_derived, which covers the interior: its
    two outer rows are NaN here (the southern one is read only by the first row of faces of a rank with a southern neighbour)."""
    _check("cells", variable)
    Nx, Ny, Nz = backend.field_dims("T", False)
    if variable == "potential_density":
        out = np.full((Nx, Ny + 2, Nz), np.nan)
        out[:, 1:Ny + 1] = np.asarray(backend.get_derived("potential_density"), np.float64)
        return out
    H = _halo(backend)
    x = np.asarray(backend.get_field(variable, True), np.float64)
    return np.array(x[H:H + Nx, H - 1:H + Ny + 1, H:H + Nz])


def class_terms(backend, what, variable, edges, window=None):
    """The terms of every face (cell) of the window, [i, n, k] float64: {"measure", "flow", "heat", "salt"} (0 where it does not
    contribute), "counted", "skipped" and "bin" (-1 where it does not contribute)."""
    _check(what, variable)
    edges = check_edges(edges)
    cv = class_values(backend, variable)
    Nx, Ny, Nz = backend.field_dims("T", False)
    if what == "faces_y":
        if variable == "potential_density" and getattr(backend, "ry", 0) > 0:
            raise NotImplementedError("the potential density of the southern neighbour's row is not available on the host")
        t = transport_terms(backend, "across_y", window)
        by = t["area"].shape[1]
        w = _window(window, Nx)
        cls = 0.5 * (cv[w, 0:by] + cv[w, 1:by + 1])
        out = {"measure": t["area"], "flow": t["volume"], "heat": t["heat"], "salt": t["salt"]}
        wet, counted = t["counted"] | t["skipped"], t["counted"]
    else:
        w = _window(window, Nx)
        mu = cell_measure(backend, "T")[w]
        T = np.asarray(backend.get_field("T", False), np.float64)[w]
        S = np.asarray(backend.get_field("S", False), np.float64)[w]
        cls = cv[w, 1:Ny + 1]
        wet = mu > 0
        counted = wet & np.isfinite(T) & np.isfinite(S)
        with np.errstate(invalid="ignore", over="ignore"):
            out = {"measure": mu, "flow": np.zeros_like(mu), "heat": mu * T, "salt": mu * S}
    counted = counted & np.isfinite(cls)
    out = {f: np.where(counted, x, 0.0) for f, x in out.items()}
    out["counted"], out["skipped"] = counted, wet & ~counted
    out["bin"] = np.where(counted, np.searchsorted(edges, np.where(counted, cls, 0.0), side="right"), -1)
    return out


def fold_classes(rows):
    """CUMULATIVE [n, e], e = 0 .. B, of ROWS [n, b]: 0 at e = 0, then the left-to-right running sums over the bins, member by
    member -- the order of k_class_fold, bit for bit."""
    rows = np.asarray(rows)
    out = np.zeros((rows.shape[0], rows.shape[1] + 1), CLASS_SUM_DTYPE)
    for f in CLASS_SUM_DTYPE.names:
        out[f][:, 1:] = rows[f]
        out[f] = np.add.accumulate(out[f], axis=1)
    return out


def total_classes(rows):
    """TOTAL [b] of ROWS [n, b]: the rows added south to north, member by member, starting from 0."""
    rows = np.asarray(rows)
    out = np.zeros(rows.shape[1], CLASS_SUM_DTYPE)
    for f in CLASS_SUM_DTYPE.names:
        out[f] = np.add.accumulate(np.concatenate([np.zeros((1, rows.shape[1]), rows[f].dtype), rows[f]], axis=0), axis=0)[-1]
    return out


def _shaped(rows, shape):
    return rows if shape == "rows" else fold_classes(rows) if shape == "cumulative" else total_classes(rows)


def class_sums_host(backend, what, variable, edges, shape="rows", window=None):
    """What HipBackend.class_sums returns, computed with numpy from the downloaded fields, bit for bit: the fallback for a
    backend without the device reduction.  np.add.at applies its additions in the order of the index array, which is flattened
    with i slowest: for a fixed (n, k, b) the terms are added over i ascending."""
    _check(what, variable, shape)
    edges = check_edges(edges)
    t = class_terms(backend, what, variable, edges, window)
    _, N, Nz = t["bin"].shape
    B = edges.size + 1
    use = t["counted"].ravel()
    n, k = np.meshgrid(np.arange(N), np.arange(Nz), indexing="ij")
    index = ((n * Nz + k)[None, :, :] * B + t["bin"]).ravel()[use]
    rows = np.zeros((N, B), CLASS_SUM_DTYPE)
    for f in SUMS:
        p = np.zeros(N * Nz * B)
        np.add.at(p, index, t[f].ravel()[use])
        p = p.reshape(N, Nz, B)
        acc = np.zeros((N, B))
        for level in range(Nz):
            acc = acc + p[:, level, :]
        rows[f] = acc
    rows["count"] = np.bincount(index, minlength=N * Nz * B).reshape(N, Nz, B).sum(axis=1)
    rows["nonfinite"][:, 0] = t["skipped"].sum(axis=(0, 2))
    return _shaped(rows, shape)


def combine_class_sums(parts, what, offsets, shape="rows"):
    """The ROWS of the ranks of a decomposition (HipBackend.class_sums(what, variable, edges, "rows", ...) of every rank, in
    rank order) as the rows of the whole; offsets: (i0, j0) of every rank's interior in the global one.  Ranks with the same j0
    hold the same rows and add in rank order -- x slabs; others are stacked by j0 -- a mesh; a row of y faces on the seam between
    two ranks belongs to the northern one alone.  CUMULATIVE and TOTAL are folded again from the combined rows."""
    if what not in WHAT:
        raise ValueError(f"what must be one of {WHAT}, got {what!r}")
    if shape not in SHAPES:
        raise ValueError(f"shape must be one of {SHAPES}, got {shape!r}")
    bands = {}
    for p, o in zip(parts, offsets):
        p = np.asarray(p)
        if o[1] in bands:
            acc = bands[o[1]]
            for f in CLASS_SUM_DTYPE.names:
                acc[f] = acc[f] + p[f]
        else:
            bands[o[1]] = p.astype(CLASS_SUM_DTYPE, copy=True)
    rows = np.concatenate([bands[o] for o in sorted(bands)], axis=0)
    return _shaped(rows, shape)
