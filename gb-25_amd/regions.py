"""Coherent regions on the host: the definition of include/gb25.h ("coherent regions on the device") restated with plain numpy, so
that the device's label planes, records and infos equal these bit for bit.  It is also what the public functions fall back to on a
backend without the kernels (the test suite's oracle backend).

    foreground: x < threshold (or >) compared in the backend's float type, x finite, mu > 0 (mu = integrals.cell_measure of T: THE
    MEASURE of gb25_integrate_field at (c,c,c))
    4-connectivity within a level; column Nx - 1 is the neighbour of column 0 on a grid periodic in x; nothing across a wall or the
    fold; levels are independent
    key = the smallest linear index i + Nx j of a region; the regions of a level are numbered in ascending key; label -1: background
    every sum of a record: fp64, from +0.0, acc = acc + term over the region's cells in ascending linear index, the terms mu,
    t = mu * x, t * x, mu * y, mu * di, mu * dj each rounded by itself (no fused multiply-add)

Arrays are [i, j] or [i, j, k] like every array of this package."""
import numpy as np

from .binding import (DERIVED_IDS, FIELD_IDS, KINEMATICS_IDS, REGION_DERIVED, REGION_DTYPE, REGION_FIELDS, REGION_KINEMATICS,
                      REGIONS_INFO_DTYPE)


def label_host(mask, periodic_x=True):
    """(labels int32 [Nx, Ny], n): the regions of the boolean plane mask [Nx, Ny] numbered 0 .. n - 1 in ascending order of their
    smallest linear index i + Nx j, -1 in the background.  Runs of foreground cells along i are found row by row and joined by a
    union-find whose root is always the smaller run: runs are numbered in ascending (j, i), which is ascending linear index."""
    m = np.asarray(mask, bool)
    Nx, Ny = m.shape
    rows = np.ascontiguousarray(m.T)                       # [j, i]: C order is the linear index
    edge = np.diff(np.concatenate([np.zeros((Ny, 1), np.int8), rows.astype(np.int8), np.zeros((Ny, 1), np.int8)], axis=1), axis=1)
    start_j, start_i = np.nonzero(edge == 1)               # ascending (j, i)
    end_i = np.nonzero(edge == -1)[1]                      # exclusive
    nruns = start_i.size
    parent = list(range(nruns))

    def find(a):
        r = a
        while parent[r] != r:
            r = parent[r]
        while parent[a] != r:
            parent[a], a = r, parent[a]
        return r

    def union(a, b):
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)

    first_of_row = np.searchsorted(start_j, np.arange(Ny + 1))
    s, e = start_i.tolist(), end_i.tolist()
    for j in range(Ny):
        lo, hi = int(first_of_row[j]), int(first_of_row[j + 1])
        if periodic_x and Nx > 1 and hi > lo and s[lo] == 0 and e[hi - 1] == Nx:
            union(lo, hi - 1)
        if j == 0:
            continue
        a, a_end = int(first_of_row[j - 1]), lo             # the runs of the row below, two pointers
        b = lo
        while a < a_end and b < hi:
            if s[a] < e[b] and s[b] < e[a]:
                union(a, b)
            if e[a] < e[b]:
                a += 1
            else:
                b += 1
    roots = np.array([find(r) for r in range(nruns)], np.int64)
    is_root = roots == np.arange(nruns)
    number = np.cumsum(is_root) - 1                        # of a root: its rank among the roots
    labels = np.full(Nx * Ny, -1, np.int32)
    labels[np.flatnonzero(rows.ravel())] = np.repeat(number[roots], end_i - start_i).astype(np.int32)
    return np.ascontiguousarray(labels.reshape(Ny, Nx).T), int(is_root.sum())


def _sequential(terms):
    """((+0.0 + t0) + t1) + ...: np.cumsum adds left to right, one rounding per term."""
    return np.cumsum(np.concatenate([[0.0], terms]))[-1]


def region_records_host(x, mu, labels, carried=None, cmp="below", periodic_x=True, max_regions=None):
    """The records (REGION_DTYPE) of the regions 0 .. min(n, max_regions) - 1 of one level: x, mu [Nx, Ny] the criterion (its float64
    value) and the measure, labels [Nx, Ny] from label_host, carried [Nx, Ny] or None."""
    lab = np.ascontiguousarray(np.asarray(labels).T).ravel()              # linear index order
    Nx, Ny = np.asarray(labels).shape
    flat = lambda a: np.ascontiguousarray(np.asarray(a, np.float64).T).ravel()
    xs, ms = flat(x), flat(mu)
    ys = None if carried is None else flat(carried)
    cells = np.flatnonzero(lab >= 0)
    order = cells[np.argsort(lab[cells], kind="stable")]                    # by region, ascending linear index inside
    n = int(lab.max()) + 1 if cells.size else 0
    counts = np.bincount(lab[cells], minlength=n)
    ends = np.cumsum(counts)
    stored = n if max_regions is None else min(n, int(max_regions))
    out = np.zeros(stored, REGION_DTYPE)
    for r in range(stored):
        c = order[ends[r] - counts[r]:ends[r]]
        i, j = c % Nx, c // Nx
        rec = out[r]
        rec["cells"] = c.size
        ki, kj = int(i[0]), int(j[0])
        rec["key_i"], rec["key_j"] = ki, kj
        rec["i_min"], rec["i_max"], rec["j_min"], rec["j_max"] = i.min(), i.max(), j.min(), j.max()
        at0, at1 = lab[j * Nx] == r, lab[j * Nx + Nx - 1] == r
        rec["wraps"] = int(bool(periodic_x) and Nx > 1 and bool((at0 & at1).any()))
        di = i - ki
        if periodic_x:
            di = np.where(2 * di >= Nx, di - Nx, np.where(2 * di < -Nx, di + Nx, di))
        m, v = ms[c], xs[c]
        with np.errstate(over="ignore", invalid="ignore"):
            t = m * v
            rec["measure"] = _sequential(m)
            rec["first"] = _sequential(t)
            rec["second"] = _sequential(t * v)
            rec["carried"] = 0.0 if ys is None else _sequential(m * ys[c])
            rec["sum_di"] = _sequential(m * di.astype(np.float64))
            rec["sum_dj"] = _sequential(m * (j - kj).astype(np.float64))
        at = int(np.argmax(v) if cmp == "above" else np.argmin(v))          # (the first of equal values: the smallest index)
        rec["extreme"], rec["extreme_i"], rec["extreme_j"] = v[at], i[at], j[at]
    return out


def foreground(x, mu, cmp, threshold):
    """(mask, nonfinite): the foreground of planes or volumes x (in the float type it is compared in) and mu."""
    x = np.asarray(x)
    wet = np.asarray(mu) > 0
    finite = np.isfinite(x)
    thr = x.dtype.type(threshold)
    with np.errstate(invalid="ignore"):
        hit = (x > thr) if cmp == "above" else (x < thr)
    return wet & finite & hit, int((wet & ~finite).sum())


def regions_of_arrays(x, mu, cmp, threshold, carried=None, periodic_x=True, max_regions=4096):
    """(labels int32 [i, j, kk], records [kk, min(max_regions, ceil(Nx Ny / 2))], infos [kk]) of the volumes x, mu (and carried) [i, j, kk]: what
    HipBackend.get_regions returns, level by level."""
    x, mu = np.asarray(x), np.asarray(mu, np.float64)
    Nx, Ny, nk = x.shape
    max_regions = min(int(max_regions), (Nx * Ny + 1) // 2)       # (the most a level can hold: HipBackend.get_regions clamps alike)
    labels = np.empty((Nx, Ny, nk), np.int32)
    records = np.zeros((nk, int(max_regions)), REGION_DTYPE)
    infos = np.zeros(nk, REGIONS_INFO_DTYPE)
    for k in range(nk):
        mask, bad = foreground(x[:, :, k], mu[:, :, k], cmp, threshold)
        labels[:, :, k], n = label_host(mask, periodic_x)
        rec = region_records_host(x[:, :, k].astype(np.float64), mu[:, :, k], labels[:, :, k], None if carried is None else carried[:, :, k],
                                  cmp, periodic_x, max_regions)
        records[k, :rec.size] = rec
        infos[k] = (n, rec.size, int(mask.sum()), bad)
    return labels, records, infos


def check_source(source):
    """The checks of gb25_get_regions that concern the criterion, on the host."""
    if source in REGION_FIELDS or source in REGION_DERIVED or source in REGION_KINEMATICS:
        return
    if source in ("vorticity", "shear_strain", "rossby_number"):
        raise ValueError(f"source: {source} is a corner quantity, at (f,f,c): it has no cell to label")
    if source in FIELD_IDS or source in DERIVED_IDS or source in KINEMATICS_IDS:
        raise ValueError(f"source: {source} is not a 3-D quantity at (c,c,c): T, S, e, {', '.join(REGION_DERIVED + REGION_KINEMATICS)}")
    raise ValueError(f"source: no field, derived field or kinematics quantity {source!r}")


def source_values(backend, source, param=None, levels=None):
    """The criterion [i, j, kk] in the backend's float type: get_field, get_derived or the kinematics."""
    k0, kc = (0, -1) if levels is None else (int(levels[0]), int(levels[1]))
    if source in REGION_FIELDS:
        a = backend.get_field(source, False)
        return a[:, :, k0:(None if kc == -1 else k0 + kc)]
    if source in REGION_DERIVED:
        return backend.get_derived(source, None, levels)
    from .kinematics import kinematics
    return kinematics(backend, source, param, levels)


def regions_host(backend, source, cmp, threshold, levels=None, carry=None, max_regions=4096, param=None, values=None):
    """What HipBackend.get_regions returns, computed with numpy from the downloaded criterion and cell_measure: the restatement,
    bit for bit, and the fallback of a backend without the kernels.  values: the criterion of the window where the backend cannot
    hand it out."""
    from .integrals import cell_measure
    check_source(source)
    if carry is not None and carry not in REGION_FIELDS:
        raise ValueError(f"carry: T, S, e or None, not {carry!r}")
    if int(max_regions) < 1:
        raise ValueError(f"max_regions = {max_regions} must be >= 1")
    Nz = backend.field_dims("T", False)[2]
    k0, kc = (0, -1) if levels is None else (int(levels[0]), int(levels[1]))
    n = Nz - k0 if kc == -1 else kc
    if k0 < 0 or k0 >= Nz or kc < -1 or kc == 0 or k0 + n > Nz:
        raise ValueError(f"window k_first = {k0}, k_count = {kc} of {Nz} levels")
    x = np.asarray(source_values(backend, source, param, (k0, n)) if values is None else values)
    mu = cell_measure(backend, "T")[:, :, k0:k0 + n]
    y = None if carry is None else backend.get_field(carry, False)[:, :, k0:k0 + n]
    periodic = getattr(backend, "Rx", 1) == 1
    return regions_of_arrays(x, mu, cmp, threshold, y, periodic, max_regions)


class Regions:
    """The regions of a window of levels: `.labels()` int32 [i, j, kk] (-1: background); `.records` -- a list with one structured
    array (binding.REGION_DTYPE) per level, or that array itself when the window has ONE level --; `.count` likewise; `.infos`
    (binding.REGIONS_INFO_DTYPE [kk]).  volume / area / mean / centroid take level = the level's position in the window (default 0).
    From the device the label planes are not copied with the records: labels() asks the device for them when it is first called,
    by the same call on the same state -- the same bits --, and refuses once the model's clock has moved on since the records were
    taken (pass labels=True to regions() to take them at once)."""

    def __init__(self, backend, labels, records, infos, levels, fetch=None):
        self._b, self._labels, self._fetch = backend, labels, fetch
        self.infos = infos
        self.levels = levels
        self._records = [records[k, :int(infos["stored"][k])] for k in range(infos.size)]
        self._clock = tuple(backend.clock()[:2]) if hasattr(backend, "clock") else None

    @property
    def records(self):
        return self._records[0] if len(self._records) == 1 else self._records

    @property
    def count(self):
        n = [int(q) for q in self.infos["regions"]]
        return n[0] if len(n) == 1 else n

    def labels(self):
        if self._labels is None:
            if self._clock is not None and tuple(self._b.clock()[:2]) != self._clock:
                raise RuntimeError("Regions.labels(): the model has been stepped since these records were taken; ask for the labels "
                                   "before stepping, or call regions(..., labels=True)")
            self._labels = self._fetch()
        return self._labels

    def volume(self, level=0):
        """sum mu of every stored region [m^3]: the measure of a cell is its volume."""
        return self._records[level]["measure"].copy()

    def area(self, level=0):
        """The horizontal area [m^2] of every stored region: its volume over the thickness dzc of its level (on a folded grid the
        cells of the pivot row count half, as in the measure)."""
        k = (0 if self.levels is None else int(self.levels[0])) + level
        return self._records[level]["measure"] / float(self._b.metric("dzc", k + 1))

    def mean(self, level=0, of="criterion"):
        """first / measure: the measure-weighted mean of the criterion (of="carried": of the carried field)."""
        r = self._records[level]
        return (r["carried"] if of == "carried" else r["first"]) / r["measure"]

    def centroid(self, level=0):
        """(i, j) float64 of every stored region, fractional 0-based interior indices; i wrapped into [0, Nx)."""
        r = self._records[level]
        Nx = self._b.field_dims("T", False)[0]
        return (r["key_i"] + r["sum_di"] / r["measure"]) % Nx, r["key_j"] + r["sum_dj"] / r["measure"]

    def centroid_lonlat(self, level=0):
        """(longitude, latitude) in degrees of the centroids, interpolated linearly in the index from the grid's metric getters.
        On the LatitudeLongitudeGrid only: a curvilinear grid has no longitude among its metrics."""
        from .integrals import LAT_LON_GRID_TYPES
        b = self._b
        if b.cfg.grid_type not in LAT_LON_GRID_TYPES:
            raise NotImplementedError("centroid_lonlat: the LatitudeLongitudeGrid only")
        Nx, Ny, _ = b.field_dims("T", False)
        ci, cj = self.centroid(level)
        phic = np.array([b.metric("phic", j) for j in range(1, Ny + 1)], np.float64)
        lon = b.cfg.lon_west + (ci + 0.5) * (b.cfg.lon_east - b.cfg.lon_west) / Nx
        return lon, np.interp(cj, np.arange(Ny), phic)

    def __repr__(self):
        return f"Regions(levels={self.levels}, count={self.count}, stored={[int(q) for q in self.infos['stored']]})"


def regions(backend, source, *, below=None, above=None, levels=None, carry=None, max_regions=4096, param=None, labels=False):
    """Regions of `source` below (or above) a threshold: from the device where the backend has the kernels (the label planes are
    copied with the records only with labels=True, else when .labels() is first asked for), from the restatement where it has not."""
    if (below is None) == (above is None):
        raise ValueError("regions: exactly one of below= and above=")
    cmp, threshold = ("below", below) if above is None else ("above", above)
    if hasattr(backend, "get_regions"):
        lab, rec, info = backend.get_regions(source, cmp, threshold, levels, carry, max_regions, param, labels=bool(labels))
        fetch = lambda: backend.get_regions(source, cmp, threshold, levels, carry, max_regions, param, labels=True)[0]
        return Regions(backend, lab, rec, info, levels, fetch)
    lab, rec, info = regions_host(backend, source, cmp, threshold, levels, carry, max_regions, param)
    return Regions(backend, lab, rec, info, levels)


def okubo_weiss_sigma(backend, level):
    """sigma_W of ONE level: the standard deviation (numpy's, float64) of the Okubo-Weiss parameter over the level's wet cells
    whose W is finite.  The level's plane alone is computed on the device and copied (gb25_get_kinematics, one level); the wet
    cells are those with mu > 0 (integrals.cell_measure) on a grid with a bottom table, every cell on the others."""
    from .integrals import ISLAND_GRID_TYPES, cell_measure
    from .kinematics import kinematics
    w = np.asarray(kinematics(backend, "okubo_weiss", None, (int(level), 1)), np.float64)[:, :, 0]
    keep = np.isfinite(w)
    if backend.cfg.grid_type in ISLAND_GRID_TYPES:      # (elsewhere the measure is positive in every cell: nothing to ask for)
        keep &= cell_measure(backend, "T")[:, :, int(level)] > 0
    return float(np.std(w[keep])) if keep.any() else 0.0


def okubo_weiss_threshold(backend, level, factor=0.2):
    """-factor * sigma_W of that level (okubo_weiss_sigma): the usual Okubo-Weiss criterion of a vortex core."""
    return -float(factor) * okubo_weiss_sigma(backend, level)


def eddy_census(backend, level=None, factor=0.2, carry=None, max_regions=4096, labels=False):
    """The regions of the level where W < -factor * sigma_W of that level (okubo_weiss_threshold); level: default the surface."""
    Nz = backend.field_dims("T", False)[2]
    level = Nz - 1 if level is None else int(level)
    return regions(backend, "okubo_weiss", below=okubo_weiss_threshold(backend, level, factor), levels=(level, 1), carry=carry,
                   max_regions=max_regions, labels=labels)
