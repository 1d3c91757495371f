"""Transports on the host: the terms of include/gb25.h ("transports on the device") restated with numpy from a backend's public
getters alone -- get_field, metric, metric2, bottom_info, field_dims -- in fp64 with the operation order of the kernels
(csrc/diagnostics_kernels.hpp, k_transport_*), the host fallback of gb25_get_transport, and the arithmetic that combines the
records of the ranks of a decomposition.  Works on binding.HipBackend and on the test suite's oracle backend.

    "across_y"  the faces of v, (c,f,c):  a = (dx dzc(k)) wet,         q = a v,  qT = q (0.5 (T(i,j-1) + T(i,j))),  qS likewise
                dx = dxcf(i,j) (lat-lon: dxf(j)); wet = k >= max(kbot(i,j-1), kbot(i,j)), 0 on a global wall row
    "across_x"  the faces of u, (f,c,c):  a = ((dy dzc(k)) fold(j)) wet,  q = a u,  tracers averaged over i-1, i
                dy = dyfc(i,j) (lat-lon: metric("dy")); wet = k >= max(kbot(i-1,j), kbot(i,j)); fold = 1/2 on the global pivot row

A face with a > 0 whose five values are finite adds a, q, qT, qS to area, volume, heat, salt and 1 to faces; one with a value that
is not finite adds 1 to nonfinite.  LINES [n, k]: "across_y" one record per row j, summed along i (a fixed but not sequential
order on the device: compare with math.fsum); "across_x" one per column i, summed along j south to north IN THAT ORDER (the
device's record bit for bit).  The streamfunction [n, kf] holds the running sums in k from 0; its last column is the PROFILE."""
import numpy as np

from .binding import TRANSPORT_DTYPE
from .derived import _dy, _metric2_parent
from .integrals import LAT_LON_GRID_TYPES, _area, _halo, fold_and_wet

SUMS = ("area", "volume", "heat", "salt")
FACES = ("across_y", "across_x")


def _velocity(faces):
    if faces not in FACES:
        raise ValueError(f"faces must be one of {FACES}, got {faces!r}")
    return "v" if faces == "across_y" else "u"


def _window(window, extent):
    """(first, count) of the summed index as a slice of [0, extent); count = -1: to the end."""
    if window is None:
        return slice(0, extent)
    first, count = window
    last = extent if count == -1 else first + count
    if first < 0 or first >= extent or count < -1 or count == 0 or last > extent:
        raise ValueError(f"window {window!r} of {extent}: empty or out of range")
    return slice(first, last)


def face_area(backend, faces):
    """a of every interior face of the direction, float64, shaped like get_field("v" | "u", include_halos=False)."""
    name = _velocity(faces)
    Nx, by, Nz = backend.field_dims(name, False)
    if backend.cfg.grid_type in LAT_LON_GRID_TYPES:
        if faces == "across_y":
            length = np.array([backend.metric("dxf", j) for j in range(1, by + 1)], np.float64)[None, :]
        else:
            length = np.full((1, by), _dy(backend))
        length = np.broadcast_to(length, (Nx, by))
    else:
        H = _halo(backend)
        length = _metric2_parent(backend, "dxcf" if faces == "across_y" else "dyfc")[H:H + Nx, H:H + by]
    dz = np.array([backend.metric("dzc", k) for k in range(1, Nz + 1)], np.float64)
    fold, wet = fold_and_wet(backend, name)
    return ((length[:, :, None] * dz[None, None, :]) * fold[None, :, None]) * wet


def transport_terms(backend, faces, window=None):
    """The terms of every face of the window, [i, j, k] float64: {"area", "volume", "heat", "salt"} (0 where the face does
    not contribute), "counted" (a > 0, every value finite) and "skipped" (a > 0, a value not finite)."""
    name = _velocity(faces)
    H = _halo(backend)
    Nx, by, Nz = backend.field_dims(name, False)
    a = face_area(backend, faces)
    vel = np.asarray(backend.get_field(name, False), np.float64)
    di, dj = (0, -1) if faces == "across_y" else (-1, 0)

    def pair(tracer):
        x = np.asarray(backend.get_field(tracer, True), np.float64)
        return x[H + di:H + di + Nx, H + dj:H + dj + by, H:H + Nz], x[H:H + Nx, H:H + by, H:H + Nz]

    (t0, t1), (s0, s1) = pair("T"), pair("S")
    wet = a > 0
    finite = np.isfinite(vel) & np.isfinite(t0) & np.isfinite(t1) & np.isfinite(s0) & np.isfinite(s1)
    counted = wet & finite
    with np.errstate(invalid="ignore", over="ignore"):
        q = a * vel
        qT = q * (0.5 * (t0 + t1))
        qS = q * (0.5 * (s0 + s1))
    out = {"area": a, "volume": q, "heat": qT, "salt": qS}
    out = {f: np.where(counted, x, 0.0) for f, x in out.items()}
    out["counted"], out["skipped"] = counted, wet & ~finite
    w = _window(window, Nx if faces == "across_y" else by)
    return {f: (x[w] if faces == "across_y" else x[:, w]) for f, x in out.items()}


def fold_transports(lines):
    """The streamfunction records [n, kf], kf = 0 .. Nz, of LINES [n, k]: 0 at kf = 0, then the left-to-right running sums in k,
    member by member -- the order of k_transport_fold, bit for bit.  The PROFILE is the last column, [:, -1]."""
    lines = np.asarray(lines)
    out = np.zeros((lines.shape[0], lines.shape[1] + 1), TRANSPORT_DTYPE)
    for f in TRANSPORT_DTYPE.names:
        out[f][:, 1:] = lines[f]
        out[f] = np.add.accumulate(out[f], axis=1)
    return out


def _shaped(lines, shape):
    if shape == "lines":
        return lines
    psi = fold_transports(lines)
    return psi[:, -1] if shape == "profile" else psi


def transport_host(backend, faces, shape="lines", window=None):
    """What HipBackend.transport returns, computed with numpy from the downloaded fields: the fallback for a backend without
    the device reduction.  "across_y" lines are summed by numpy, "across_x" lines south to north in that order."""
    t = transport_terms(backend, faces, window)
    axis = 0 if faces == "across_y" else 1
    n = t["area"].shape[1 - axis]
    lines = np.zeros((n, t["area"].shape[2]), TRANSPORT_DTYPE)
    for f in SUMS:
        lines[f] = t[f].sum(axis=0) if faces == "across_y" else np.add.accumulate(t[f], axis=1)[:, -1]
    lines["faces"] = t["counted"].sum(axis=axis)
    lines["nonfinite"] = t["skipped"].sum(axis=axis)
    return _shaped(lines, shape)


def combine_transports(parts, faces, offsets, shape="lines"):
    """The LINES of the ranks of a decomposition (HipBackend.transport(faces, "lines", ...) of every rank, in rank order) as
    the lines of the whole; offsets: (i0, j0) of every rank's interior in the global one.  "across_y" lines [j, k]: ranks with the
    same j0 hold the same rows and add -- x slabs; others are stacked by j0 -- a mesh; a row of y faces on the seam between two
    ranks belongs to the northern one alone.  "across_x" lines [i, k]: ranks with the same i0 add south to north -- mesh bands;
    others are concatenated in i -- x slabs.  PROFILE and STREAMFUNCTION are folded again from the combined lines."""
    _velocity(faces)
    key = 1 if faces == "across_y" else 0
    bands = {}
    for p, o in zip(parts, offsets):
        p = np.asarray(p)
        if o[key] in bands:
            acc = bands[o[key]]
            for f in TRANSPORT_DTYPE.names:
                acc[f] = acc[f] + p[f]
        else:
            bands[o[key]] = p.astype(TRANSPORT_DTYPE, copy=True)
    lines = np.concatenate([bands[o] for o in sorted(bands)], axis=0)
    return _shaped(lines, shape)


def continuity_closure(backend, lines=None):
    """How well the "across_y" LINES `lines` (default: transport_host's) close the model's own continuity equation on a single
    domain: over the rows of cells (j, k) that have a row of y faces on either side -- every row of a grid between two walls,
    where V = 0 on the wall rows; every row but the last row of cell centres of a folded grid, which holds no row of faces
    beyond it --, the largest |sum_i Az (w(k+1) - w(k)) + (V[j+1, k] - V[j, k])| / (sum_i |q_south| + sum_i |q_north| +
    sum_i |q_u|), V = the lines' volume.  The model's w comes from these very face transports and the zonal terms cancel over a
    periodic row, so the value is round-off of the model's float type when the definitions of the terms are the model's."""
    if lines is None:
        lines = transport_host(backend, "across_y")
    V = np.asarray(lines["volume"], np.float64)
    Nx, Ny, Nz = backend.field_dims("T", False)
    w = np.asarray(backend.get_field("w", False), np.float64)
    Az = np.asarray(_area(backend, "cc", Nx, Ny), np.float64)
    lhs = (Az[:, :, None] * (w[:, :, 1:] - w[:, :, :-1])).sum(axis=0)
    qy = np.abs(transport_terms(backend, "across_y")["volume"]).sum(axis=0)
    qx = np.abs(transport_terms(backend, "across_x")["volume"]).sum(axis=0)
    rows, north = slice(0, V.shape[0] - 1), slice(1, V.shape[0])
    residual = np.abs(lhs[rows] + (V[north] - V[rows]))
    scale = qy[rows] + qy[north] + qx[rows]
    return float((residual[scale > 0] / scale[scale > 0]).max())
