"""The moving-window filter on the host: the definition of include/gb25.h ("moving-window filter on the device") restated with
numpy from a backend's public getters alone -- get_field, get_derived, metric / metric2, bottom_info, field_dims -- in fp64 with the
operation order of the kernels (csrc/filter_kernels.hpp, k_filter_x and k_filter_y), so that the device's planes equal these bit
for bit.  It is also what the public functions fall back to on a backend without the kernels (the test suite's oracle backend).

    horizontal, level by level; mu = integrals.cell_measure (THE MEASURE of gb25_integrate_field); a source point counts iff
    mu > 0 and x is finite: m = mu, t = mu * x, q = t * x (no fused multiply-add); otherwise m = t = q = +0.0
    output (I, J, K) is centred on the fine point (I sx, J sy, k_first + K); x wraps modulo Nx, y is clipped to 0 .. Ny - 1
    s(i, j) = sum over d = -rx .. rx, ascending, of [wx[d + rx] *] a(wrap(i + d), j)          (every sum starts from +0.0)
    b(i, j) = sum over e = -ry .. ry, ascending, rows outside skipped, of [wy[e + ry] *] s(i, j + e)
    measure = b of m, first = b of t, second = b of q;  xbar = first / measure,  variance = second / measure - xbar^2

rx_of_row gives row j of s its own rx (the box in x): a fixed physical width on a grid whose dx shrinks towards the poles."""
import numpy as np

from .binding import DERIVED_IDS
from .integrals import LAT_LON_GRID_TYPES, _halo, cell_measure, location

PLANES = ("measure", "first", "second")
MAX_RADIUS = 32                                     # GB25_FILTER_MAX_RADIUS


class FilterSums:
    """The planes of one call, [I, J, K] float64 each (None: not asked for), and its info: dims, nonfinite (source points with
    mu > 0 whose value is not finite, each once), empty (outputs with measure 0), clipped (outputs whose y window was cut),
    global_offset of the fine interior; radius = (rx, ry), stride = (sx, sy)."""

    def __init__(self, measure, first, second, *, radius, stride, dims, nonfinite, empty, clipped, global_offset=(0, 0, 0)):
        self.measure, self.first, self.second = measure, first, second
        self.radius = tuple(int(q) for q in radius)
        self.stride = tuple(int(q) for q in stride)
        self.dims = tuple(int(q) for q in dims)
        self.nonfinite, self.empty, self.clipped = int(nonfinite), int(empty), int(clipped)
        self.global_offset = tuple(int(q) for q in global_offset)

    @property
    def info(self):
        return dict(dims=self.dims, nonfinite=self.nonfinite, empty=self.empty, clipped=self.clipped, global_offset=self.global_offset)

    def mean(self):
        """The filtered field xbar = first / measure; NaN where the window has no counted point (measure 0)."""
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(self.measure > 0, self.first / self.measure, np.nan)

    def variance(self):
        """second / measure - xbar^2, clipped at 0: the variance below the filter scale; NaN where measure is 0."""
        mean = self.mean()
        with np.errstate(invalid="ignore", divide="ignore"):
            v = self.second / self.measure - mean * mean
        return np.where(self.measure > 0, np.maximum(v, 0.0), np.nan)

    def __repr__(self):
        return f"FilterSums(radius={self.radius}, stride={self.stride}, {', '.join(f'{k}={v}' for k, v in self.info.items())})"


def kernel_weights(kind, r):
    """The 2 r + 1 weights of a window of radius r, float64, symmetric and positive; not normalised (the measure plane carries the
    same weights, so a mean needs no normalisation).  "box": ones (pass None to the filter instead: no multiply is made);
    "gaussian": exp(-d^2 / (2 sigma^2)) with sigma = r / 2, the window ends at two standard deviations; "triangle": r + 1 - |d|."""
    r = int(r)
    if r < 0:
        raise ValueError(f"radius r = {r} must be >= 0")
    d = np.arange(-r, r + 1, dtype=np.float64)
    if kind == "box":
        return np.ones(2 * r + 1)
    if kind == "gaussian":
        return np.exp(-0.5 * (d / (0.5 * r)) ** 2) if r else np.ones(1)
    if kind == "triangle":
        return (r + 1) - np.abs(d)
    raise ValueError(f"kernel {kind!r}: 'box', 'gaussian' or 'triangle'")


def _weights(name, w, r):
    if w is None:
        return None
    w = np.ascontiguousarray(w, np.float64).reshape(-1)
    if w.size != 2 * r + 1 or not (np.isfinite(w) & (w >= 0)).all():
        raise ValueError(f"{name}: {2 * r + 1} finite values >= 0")
    if not w.sum() > 0:
        raise ValueError(f"{name}: the weights sum to zero")
    return w


def check_window(Nx, Ny, radius, stride=(1, 1), wx=None, wy=None, rx_of_row=None):
    """The checks of gb25_get_filter_sums that concern the window, on the host: (rx, ry, sx, sy, wx, wy, rx_of_row) as ints and
    arrays.  ValueError names the argument, as the library's message does."""
    rx, ry = (int(q) for q in radius)
    sx, sy = (int(q) for q in stride)
    if not 0 <= rx <= MAX_RADIUS:
        raise ValueError(f"rx = {rx} must be 0 .. {MAX_RADIUS}")
    if not 0 <= ry <= MAX_RADIUS:
        raise ValueError(f"ry = {ry} must be 0 .. {MAX_RADIUS}")
    if 2 * rx + 1 > Nx:
        raise ValueError(f"rx = {rx}: a window of 2 rx + 1 columns exceeds Nx = {Nx}")
    if sx <= 0 or Nx % sx:
        raise ValueError(f"sx = {sx} must be > 0 and divide Nx = {Nx}")
    if sy <= 0 or Ny % sy:
        raise ValueError(f"sy = {sy} must be > 0 and divide Ny = {Ny}")
    if wx is not None and rx_of_row is not None:
        raise ValueError("wx and rx_of_row exclude each other: with a radius per row x is the box")
    wx, wy = _weights("wx", wx, rx), _weights("wy", wy, ry)
    if rx_of_row is not None:
        rows = np.ascontiguousarray(rx_of_row).reshape(-1)
        if rows.size != Ny or not np.issubdtype(rows.dtype, np.integer) or (rows < 0).any() or (rows > MAX_RADIUS).any() or (2 * rows + 1 > Nx).any():
            raise ValueError(f"rx_of_row: {Ny} integers 0 .. {MAX_RADIUS} with 2 rx + 1 <= Nx = {Nx}")
        rx_of_row = rows.astype(np.int32)
    return rx, ry, sx, sy, wx, wy, rx_of_row


def like_of(source):
    """The field whose measure a source takes: itself, or T / eta for the derived fields at (c,c)."""
    if source == "vorticity":
        raise ValueError("source: the vorticity lives at (f,f,c), for which the measure is not defined")
    return ("eta" if source == "mixed_layer_depth" else "T") if source in DERIVED_IDS else source


def resolve(backend, source, radius, stride=(1, 1), levels=None, wx=None, wy=None, rx_of_row=None):
    """All checks of gb25_get_filter_sums on the host: (measure name, (Nx, Ny, levels), k_first, k_count, dims, window)."""
    like = like_of(source)
    Nx, Ny, _ = backend.field_dims("T", False)
    nlev = backend.field_dims(like, False)[2]
    window = check_window(Nx, Ny, radius, stride, wx, wy, rx_of_row)
    k_first, k_count = (0, -1) if levels is None else (int(levels[0]), int(levels[1]))
    kc = nlev - k_first if k_count == -1 else k_count
    if k_first < 0 or k_first >= nlev or k_count < -1 or k_count == 0 or k_first + kc > nlev:
        raise ValueError(f"window k_first = {k_first}, k_count = {k_count} of {nlev} levels")
    return like, (Nx, Ny, nlev), k_first, kc, (Nx // window[2], Ny // window[3], kc), window


def filter_of_planes(x, mu, radius, stride=(1, 1), wx=None, wy=None, rx_of_row=None):
    """The definition on plain arrays: x [Nx, Ny, n] the values, mu [Nx, Ny, n] the measure, of the rows of cell centres and the
    window of levels alone.  (measure, first, second, nonfinite): three planes [Nx / sx, Ny / sy, n] and the number of points
    with mu > 0 whose value is not finite."""
    x = np.asarray(x, np.float64)
    mu = np.asarray(mu, np.float64)
    Nx, Ny, n = x.shape
    rx, ry, sx, sy, wx, wy, rows = check_window(Nx, Ny, radius, stride, wx, wy, rx_of_row)
    nI, nJ = Nx // sx, Ny // sy
    wet = mu > 0
    ok = wet & np.isfinite(x)
    x0 = np.where(ok, x, 0.0)
    with np.errstate(over="ignore", invalid="ignore"):
        t = np.where(ok, mu * x0, 0.0)
        q = np.where(ok, t * x0, 0.0)
    m = np.where(ok, mu, 0.0)
    cols = np.arange(nI) * sx
    centres = np.arange(nJ) * sy
    out = []
    with np.errstate(over="ignore", invalid="ignore"):
        for a in (m, t, q):
            s = np.zeros((nI, Ny, n))
            if rows is None:
                for d in range(-rx, rx + 1):                  # the x sums, ascending d, the seam by index
                    term = a[(cols + d) % Nx]
                    s = s + (term if wx is None else wx[d + rx] * term)
            else:
                for r in np.unique(rows):                     # ... with the radius of the row
                    these = np.flatnonzero(rows == r)
                    for d in range(-int(r), int(r) + 1):
                        s[:, these] = s[:, these] + a[(cols + d) % Nx][:, these]
            b = np.zeros((nI, nJ, n))
            for e in range(-ry, ry + 1):                      # the y sums, ascending e, rows outside 0 .. Ny - 1 skipped
                jj = centres + e
                inside = np.flatnonzero((jj >= 0) & (jj < Ny))
                term = s[:, jj[inside]]
                b[:, inside] = b[:, inside] + (term if wy is None else wy[e + ry] * term)
            out.append(b)
    return out[0], out[1], out[2], int((wet & ~ok).sum())


def clipped_outputs(Ny, ry, sy, nI, nK):
    """The outputs whose y window leaves the rows 0 .. Ny - 1."""
    centres = np.arange(Ny // sy) * sy
    return int(((centres - ry < 0) | (centres + ry > Ny - 1)).sum()) * nI * nK


def _global_offset(backend):
    return (int(getattr(backend, "rx", 0)) * int(getattr(backend, "Nx_local", 0)),
            int(getattr(backend, "ry", 0)) * int(getattr(backend, "Ny_local", 0)), 0)


def source_values(backend, source, param=None):
    """The interior of a source, all its levels: get_field, or get_derived (the kinetic energy from its host restatement on a
    backend without the derived fields)."""
    if source not in DERIVED_IDS:
        return backend.get_field(source, False)
    if hasattr(backend, "get_derived"):
        return backend.get_derived(source, param)
    if source == "kinetic_energy":
        from .derived import kinetic_energy_host
        return kinetic_energy_host(backend)
    raise NotImplementedError(f"{source} needs a backend with get_derived, or values=")


def sums_of_arrays(x, mu, radius, stride, wx, wy, rx_of_row, global_offset=(0, 0, 0)):
    """FilterSums of plain arrays (filter_of_planes and the counts)."""
    m, t, q, nonfinite = filter_of_planes(x, mu, radius, stride, wx, wy, rx_of_row)
    return FilterSums(m, t, q, radius=radius, stride=stride, dims=m.shape, nonfinite=nonfinite, empty=int((m == 0).sum()),
                      clipped=clipped_outputs(x.shape[1], int(radius[1]), int(stride[1]), m.shape[0], m.shape[2]), global_offset=global_offset)


def filter_sums_host(backend, source, radius, stride=(1, 1), levels=None, wx=None, wy=None, rx_of_row=None, *, param=None, values=None):
    """What HipBackend.filter_sums returns, computed with numpy from the downloaded field (or derived field) and cell_measure: the
    restatement, bit for bit, and the fallback of a backend without the kernels.  source: a field name or a derived name at
    (c,c): "kinetic_energy", "density_anomaly", "potential_density", "mixed_layer_depth" (param: its threshold).  radius = (rx,
    ry) in grid points; stride = (sx, sy); levels = (k_first, k_count) of the field's own levels, None: all; wx, wy: 2 rx + 1 and
    2 ry + 1 weights or None (the box); rx_of_row: one rx per row or None.  values: the interior of the source, all its levels,
    where the backend cannot hand it out."""
    like, (Nx, Ny, nlev), k0, kc, dims, window = resolve(backend, source, radius, stride, levels, wx, wy, rx_of_row)
    x = np.asarray(source_values(backend, source, param) if values is None else values, np.float64)[:, :Ny, k0:k0 + kc]
    mu = cell_measure(backend, like)[:, :Ny, k0:k0 + kc]
    return sums_of_arrays(x, mu, window[:2], window[2:4], window[4], window[5], window[6], _global_offset(backend))


def filter_sums(backend, source, radius, stride=(1, 1), levels=None, wx=None, wy=None, rx_of_row=None, param=None):
    """From the device where the backend has the kernels, from the restatement where it has not."""
    if hasattr(backend, "filter_sums"):
        return backend.filter_sums(source, radius, stride, levels, wx, wy, rx_of_row, param)
    return filter_sums_host(backend, source, radius, stride, levels, wx, wy, rx_of_row, param=param)


def _row_mean_dx(backend, hloc, Nx, Ny):
    """The mean over i of dx at the horizontal location, by row of cell centres [m]."""
    if backend.cfg.grid_type in LAT_LON_GRID_TYPES:
        return np.array([backend.metric("dxf" if hloc == "cf" else "dxc", j) for j in range(1, Ny + 1)], np.float64)
    name = "dx" + hloc
    try:
        H = _halo(backend)
        dx = np.asarray(backend.metric2(name), np.float64)[H:H + Nx, H:H + Ny]
    except TypeError:          # (a backend whose metric2 answers point by point)
        dx = np.array([[backend.metric2(name, i, j) for j in range(1, Ny + 1)] for i in range(1, Nx + 1)], np.float64)
    return dx.mean(axis=0)


def rows_for_length(backend, source, length_m):
    """rx_of_row for a window about length_m metres wide in x: rx(j) = round(length_m / (2 dx(j))) with dx(j) the ROW MEAN of dx at
    the source's horizontal location, capped at GB25_FILTER_MAX_RADIUS and at the largest rx with 2 rx + 1 <= Nx; int32 [Ny].
    On the LatitudeLongitudeGrid dx is a function of the row and the width is what was asked for (up to the rounding and the
    cap); on the curvilinear grids dx varies along a row and the width is right for the row's mean only."""
    if not float(length_m) > 0:
        raise ValueError(f"length_m = {length_m} must be > 0")
    Nx, Ny, _ = backend.field_dims("T", False)
    dx = _row_mean_dx(backend, location(like_of(source))[0], Nx, Ny)
    rx = np.floor(0.5 * float(length_m) / dx + 0.5)
    return np.minimum(rx, min(MAX_RADIUS, (Nx - 1) // 2)).astype(np.int32)


def ensemble_filter_sums(ensemble, source, radius, stride=(1, 1), levels=None, wx=None, wy=None, rx_of_row=None):
    """The filter over the ranks of a LocalSlabEnsemble on the host (a window reaches beyond a rank, so the device entry refuses
    there): the source gathered with `gather`, the measure with the ranks' block sums of single points -- mu of every counted
    point, from the device's own tables --, then the definition.  Equals the single domain's planes bit for bit.  source: a field."""
    from .blocks import block_sums, gather_blocks
    if source in DERIVED_IDS:
        raise NotImplementedError("the ensemble filters fields; a derived field is gathered by the caller (filter_of_planes)")
    b0 = ensemble.backends[0]
    nlev = b0.field_dims(source, False)[2]
    k_first, k_count = (0, -1) if levels is None else (int(levels[0]), int(levels[1]))
    kc = nlev - k_first if k_count == -1 else k_count
    if k_first < 0 or k_first >= nlev or k_count < -1 or k_count == 0 or k_first + kc > nlev:
        raise ValueError(f"window k_first = {k_first}, k_count = {k_count} of {nlev} levels")
    ones = gather_blocks([block_sums(b, source, (1, 1, 1), (k_first, kc)) for b in ensemble.backends])
    Ny = ones.dims[1]
    x = np.asarray(ensemble.gather(source), np.float64)[:, :Ny, k_first:k_first + kc]
    out = sums_of_arrays(x, ones.measure, radius, stride, wx, wy, rx_of_row)
    out.nonfinite += ones.nonfinite          # (the block sums have skipped and counted them: their measure there is 0)
    return out
