"""Zonal-mean and eddy statistics on the host: the line records of include/gb25.h ("zonal-mean and eddy statistics on the device")
restated with numpy from a backend's public getters alone, in fp64, with the order of every sum of the kernel
(csrc/zonal_eddy_kernels.hpp, k_zonal_eddy), so that the device's records equal these bit for bit; the host fallback of
gb25_get_zonal_eddy; the object the public function returns; the arithmetic that combines the records of the ranks of a
decomposition; and the Lorenz energy cycle from the records.

    a line          interior row j, level k, along i
    x_q             U = 0.5 (u(i) + u(i+1)), V = 0.5 (v(j) + v(j+1)), W = 0.5 (w(k) + w(k+1)), T, S, SIGMA = the potential density as
                    get_derived("potential_density") returns it
    mu              integrals.cell_measure("T"); a cell counts iff mu > 0 and the six values are finite
    measure, first  sum mu, sum mu x_q;  mean[q] = first[q] / measure (+0.0 for an empty line), or the caller's
    co[p, q]        sum (mu d_p) d_q, d_q = x_q - mean[q], for p <= q, row-major: index p (11 - p) / 2 + q

The order of a sum over a line: the cells are cut into chunks of four aligned to four elements in the parent array of T -- the
first chunk holds the 4 - a first cells, a = (element offset of the line's first cell) mod 4 --, lane l of 64 adds the cells of the
chunks l, l + 64, ... in ascending i starting from +0.0, and the lanes are added pairwise: (l0 + l1) + (l2 + l3), ... six times.

The Lorenz cycle is plain float64 host arithmetic on the records and not part of the bit-for-bit contract."""
import numpy as np

from .binding import ZONAL_EDDY_DTYPE, ZONAL_EDDY_VARIABLES
from .integrals import LAT_LON_GRID_TYPES, cell_measure

VARIABLES = tuple(ZONAL_EDDY_VARIABLES)
PAIRS = tuple((p, q) for p in range(6) for q in range(p, 6))


def variable_index(name):
    if isinstance(name, str) and name.upper() in ZONAL_EDDY_VARIABLES:
        return ZONAL_EDDY_VARIABLES[name.upper()]
    if isinstance(name, (int, np.integer)) and 0 <= int(name) < 6:
        return int(name)
    raise ValueError(f"variable: {name!r} is none of {VARIABLES}")


def co_index(a, b):
    """Where co holds the comoment of the variables a and b (names or indices, either order)."""
    p, q = sorted((variable_index(a), variable_index(b)))
    return p * (11 - p) // 2 + q


def _levels(levels, Nz):
    k0, kc = (0, -1) if levels is None else (int(levels[0]), int(levels[1]))
    kc = Nz - k0 if kc == -1 else kc
    if k0 < 0 or k0 >= Nz or kc <= 0 or k0 + kc > Nz:
        raise ValueError(f"window first = {k0}, count = {kc} of {Nz} levels (k_first, k_count)")
    return k0, kc


def centred_values(backend, sigma=None):
    """x[q] of every interior cell, float64 [6, i, j, k], from the parents (u's halo column, v's next row, w's next level)."""
    Nx, Ny, Nz = backend.field_dims("T", False)
    H = (backend.field_dims("T", True)[0] - Nx) // 2
    box = lambda n, di, dj, dk: np.asarray(backend.get_field(n, True), np.float64)[H:H + Nx + di, H:H + Ny + dj, H:H + Nz + dk]
    u, v, w = box("u", 1, 0, 0), box("v", 0, 1, 0), box("w", 0, 0, 1)
    if sigma is None:
        sigma = backend.get_derived("potential_density")
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([0.5 * (u[:-1] + u[1:]), 0.5 * (v[:, :-1] + v[:, 1:]), 0.5 * (w[:, :, :-1] + w[:, :, 1:]),
                         box("T", 0, 0, 0), box("S", 0, 0, 0), np.asarray(sigma, np.float64)])


def line_misalignment(backend):
    """a[j, k] of every interior line: the element offset of its first cell in the parent array of T, mod 4."""
    Nx, Ny, Nz = backend.field_dims("T", False)
    sx, sy, _ = backend.field_dims("T", True)
    H = (sx - Nx) // 2
    j, k = np.meshgrid(np.arange(Ny), np.arange(Nz), indexing="ij")
    return (H + sx * ((j + H) + sy * (k + H))) % 4


def line_sums(terms, a):
    """The sums of `terms` [i, line] over i in the kernel's order, for lines that share the misalignment a: [line]."""
    terms = np.asarray(terms, np.float64)
    n, L = terms.shape
    rounds = ((a + n + 3) // 4 + 63) // 64
    padded = np.zeros((rounds * 256, L))
    padded[a:a + n] = terms
    padded = padded.reshape(rounds, 64, 4, L)
    acc = np.zeros((64, L))
    for r in range(rounds):
        for s in range(4):
            acc = acc + padded[r, :, s]
    while acc.shape[0] > 1:
        acc = acc[0::2] + acc[1::2]
    return acc[0]


def zonal_eddy_host(backend, levels=None, means=None, sigma=None):
    """What HipBackend.zonal_eddy returns, computed with numpy from the downloaded parents, bit for bit: records of
    ZONAL_EDDY_DTYPE [j, kk].  means: None or float64 [j, kk, 6]; sigma: the potential density as stored, [i, j, k] (default: the
    backend's get_derived).  Also the fallback of a backend without the kernel."""
    Nx, Ny, Nz = backend.field_dims("T", False)
    k0, kc = _levels(levels, Nz)
    if means is not None:
        means = np.asarray(means, np.float64)
        if means.shape != (Ny, kc, 6):
            raise ValueError(f"means: expected shape {(Ny, kc, 6)}, got {means.shape}")
        if not np.isfinite(means).all():
            raise ValueError("every entry of means must be finite")
    ks = slice(k0, k0 + kc)
    x = centred_values(backend, sigma)[:, :, :, ks]
    mu = cell_measure(backend, "T")[:, :, ks]
    wet = mu > 0
    counted = wet & np.isfinite(x).all(axis=0)
    mis = line_misalignment(backend)[:, ks]
    out = np.zeros((Ny, kc), ZONAL_EDDY_DTYPE)
    out["points"] = counted.sum(axis=0)
    out["nonfinite"] = (wet & ~counted).sum(axis=0)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for a in range(4):
            at = mis == a
            if not at.any():
                continue
            c, m = counted[:, at], mu[:, at]                       # [i, line]
            xs = x[:, :, at]
            measure = line_sums(np.where(c, m, 0.0), a)
            first = np.stack([line_sums(np.where(c, m * xs[q], 0.0), a) for q in range(6)], axis=-1)
            if means is None:
                mean = np.where(measure[:, None] == 0.0, 0.0, first / np.where(measure == 0.0, 1.0, measure)[:, None])
            else:
                mean = means[at]
            d = [xs[q] - mean[None, :, q] for q in range(6)]
            co = np.stack([line_sums(np.where(c, (m * d[p]) * d[q], 0.0), a) for p, q in PAIRS], axis=-1)
            rec = out[at]
            rec["measure"], rec["first"], rec["mean"], rec["co"] = measure, first, mean, co
            out[at] = rec
    return out


class ZonalEddy:
    """The line records of one call, [j, kk], and what one reads from them.  Names: "U", "V", "W", "T", "S", "SIGMA"."""

    def __init__(self, records, levels=None):
        self.records = np.asarray(records)
        self.levels = levels

    @property
    def measure(self):
        return self.records["measure"]

    def mean(self, name):
        """[x] of the lines, [j, kk]."""
        return self.records["mean"][..., variable_index(name)]

    def covariance(self, a, b):
        """[a* b*] = co / measure of the lines, [j, kk]; 0 on a line without a counted cell."""
        m = self.measure
        return np.divide(self.records["co"][..., co_index(a, b)], m, out=np.zeros(m.shape), where=m > 0)

    def eddy_kinetic_energy(self):
        """1/2 ([U* U*] + [V* V*]) [m^2 s^-2], [j, kk]."""
        return 0.5 * (self.covariance("U", "U") + self.covariance("V", "V"))

    def eddy_flux(self, pair):
        """The covariance of two variables written together: "VT" = [V* T*], "UV" = [U* V*], "WSIGMA" = [W* SIGMA*]."""
        pair = pair.upper()
        for n in VARIABLES:
            if pair.startswith(n) and pair[len(n):] in ZONAL_EDDY_VARIABLES:
                return self.covariance(n, pair[len(n):])
        raise ValueError(f"eddy_flux: {pair!r} is not two of {VARIABLES} written together")


def _backend_of(model):
    return getattr(model, "backend", model)


def zonal_eddy(model, levels=None, means=None, **host):
    """The zonal-mean and eddy statistics of every interior line of a model (or a backend) as a ZonalEddy: from the device where the
    backend has the kernel, from the restatement where it has not.  levels = (k_first, k_count), 0-based (k_count = -1: all from
    k_first on); means: float64 [j, kk, 6], the means the deviations are taken about (default: the lines' own).  host: sigma = ...
    for a backend without get_derived."""
    b = _backend_of(model)
    if hasattr(b, "zonal_eddy"):
        return ZonalEddy(b.zonal_eddy(levels, means), levels)
    return ZonalEddy(zonal_eddy_host(b, levels, means, **host), levels)


def combine_zonal_eddy(parts, row_offsets=None, measure=None):
    """The records of the ranks of a decomposition, in rank order, as the records of the whole.  Ranks with the same row_offsets
    entry (the global index of their first row) hold parts of the same lines: measure, first, co, points and nonfinite add in rank
    order -- x slabs; ranks with different entries are stacked in y -- a mesh.  mean = first / measure of the combined sums, one
    division.  Two phases make the eddies those about the GLOBAL mean: combine the ranks' records of means = None, hand every
    rank the combined mean of its rows, combine what they return (LocalSlabEnsemble.zonal_eddy).
    measure: None, or [j, kk] from single_domain_measure -- the sum of the cells' mu over the whole line in the order of ONE
    domain.  The ranks' partial sums added in rank order are another association of the same numbers and may differ from it in
    the last bit where mu varies along a line (curvilinear grids); with it given, `measure` of every line without a skipped
    cell IS the single domain's, bit for bit, whatever the decomposition.  A line with a skipped cell keeps the ranks' sum:
    which of its cells were skipped is not in the records."""
    parts = [np.asarray(getattr(p, "records", p)) for p in parts]
    if row_offsets is None:
        row_offsets = [0] * len(parts)
    bands = {}
    for p, o in zip(parts, row_offsets):
        if o in bands:
            acc = bands[o]
            for f in ("measure", "first", "co", "points", "nonfinite"):
                acc[f] = acc[f] + p[f]
        else:
            bands[o] = p.astype(ZONAL_EDDY_DTYPE, copy=True)
    out = np.concatenate([bands[o] for o in sorted(bands)], axis=0)
    if measure is not None:
        out["measure"] = np.where(out["nonfinite"] == 0, np.asarray(measure, np.float64), out["measure"])
    m = out["measure"][..., None]
    out["mean"] = np.divide(out["first"], m, out=np.zeros(out["first"].shape), where=m != 0)
    return out


def gathered_measure(backends):
    """mu of every cell of the GLOBAL interior, float64 [i, j, k], from the ranks' integrals.cell_measure("T") placed by their
    offsets.  Static: it changes only with the grid or the bottom."""
    first = backends[0]
    Nx, Ny, Nz = int(first.cfg.Nx), int(first.cfg.Ny), int(first.cfg.Nz)
    mu = np.zeros((Nx, Ny, Nz))
    for b in backends:
        part = cell_measure(b, "T")
        i0, j0 = b.rx * b.Nx_local, b.ry * b.Ny_local
        mu[i0:i0 + part.shape[0], j0:j0 + part.shape[1]] = part
    return mu


def single_domain_measure(mu, halo, levels=None):
    """`measure` of every line of the global interior as ONE domain sums it -- the chunks, lanes and tree of the whole line, cut
    by the alignment of the single domain's parent array of T -- from the cells' mu [i, j, k] (gathered_measure), with every wet
    cell counted: [j, kk].  A sum of given numbers in a fixed order, so it does not depend on how the ranks cut the lines."""
    Nx, Ny, Nz = mu.shape
    k0, kc = _levels(levels, Nz)
    H, sx, sy = int(halo), Nx + 2 * int(halo), Ny + 2 * int(halo)
    j, k = np.meshgrid(np.arange(Ny), np.arange(k0, k0 + kc), indexing="ij")
    mis = (H + sx * ((j + H) + sy * (k + H))) % 4
    part = mu[:, :, k0:k0 + kc]
    out = np.zeros((Ny, kc))
    for a in range(4):
        at = mis == a
        if at.any():
            out[at] = line_sums(np.where(part[:, at] > 0, part[:, at], 0.0), a)
    return out


def lorenz_cycle_of_records(records, zc, y, g_over_rho0):
    """The Lorenz energy cycle from line records [j, kk] (ZonalEddy or ZONAL_EDDY_DTYPE): zc [kk] the depths of the levels [m], y [j]
    the meridional coordinate of the rows [m], g_over_rho0 = g / rho0.  Quasi-geostrophic form, b = -(g / rho0) sigma:

        [x]       the line's mean, x* the deviation from it; mu the line's measure (its volume)
        b_r(k)    = sum_j first_b / sum_j measure, the measure-weighted horizontal mean; N2(k) = d b_r / dz (centred, one-sided at the ends)
        K_M       = 1/2 sum mu ([U]^2 + [V]^2)                K_E = 1/2 sum mu ([U*U*] + [V*V*])
        P_M       = 1/2 sum mu ([b] - b_r)^2 / N2             P_E = 1/2 sum mu [b*b*] / N2
        C(P_M -> P_E) = -sum mu [V*b*] d[b]/dy / N2
        C(P_E -> K_E) =  sum mu [W*b*]
        C(K_E -> K_M) =  sum mu ([U*V*] d[U]/dy + [U*W*] d[U]/dz)

    d/dy and d/dz are np.gradient along the rows and the levels.  A level whose N2 is not positive contributes 0 to P_M, P_E and
    C(P_M -> P_E).  Returns a dict: every quantity [j, kk] under its name, the totals under "total" (a dict of floats), "N2" [kk]."""
    ze = records if isinstance(records, ZonalEddy) else ZonalEddy(records)
    zc, y = np.asarray(zc, np.float64), np.asarray(y, np.float64)
    mu = ze.measure
    Ny, kc = mu.shape
    if kc < 2 or Ny < 2 or zc.shape != (kc,) or y.shape != (Ny,):
        raise ValueError("lorenz_cycle: at least two rows and two levels, zc [levels] and y [rows]")
    gr = float(g_over_rho0)
    first_sigma = ze.records["first"][..., variable_index("SIGMA")]
    tot_mu = mu.sum(axis=0)
    b_r = -gr * np.divide(first_sigma.sum(axis=0), tot_mu, out=np.zeros(kc), where=tot_mu > 0)
    N2 = np.gradient(b_r, zc)
    inv = np.divide(1.0, N2, out=np.zeros(kc), where=N2 > 0)[None, :]
    U, V, b = ze.mean("U"), ze.mean("V"), -gr * ze.mean("SIGMA")
    bb, Vb, Wb = gr * gr * ze.covariance("SIGMA", "SIGMA"), -gr * ze.covariance("V", "SIGMA"), -gr * ze.covariance("W", "SIGMA")
    dUdy, dUdz, dbdy = np.gradient(U, y, axis=0), np.gradient(U, zc, axis=1), np.gradient(b, y, axis=0)
    out = {"K_M": 0.5 * mu * (U * U + V * V),
           "K_E": mu * ze.eddy_kinetic_energy(),
           "P_M": 0.5 * mu * (b - b_r[None, :]) ** 2 * inv,
           "P_E": 0.5 * mu * bb * inv,
           "C_PM_PE": -mu * Vb * dbdy * inv,
           "C_PE_KE": mu * Wb,
           "C_KE_KM": mu * (ze.covariance("U", "V") * dUdy + ze.covariance("U", "W") * dUdz)}
    out["total"] = {n: float(a.sum()) for n, a in out.items()}
    out["N2"] = N2
    return out


def lorenz_cycle(model, levels=None, **host):
    """The four reservoirs and three conversions of the Lorenz energy cycle of a model (or a backend, or anything with .backends
    and .zonal_eddy: a LocalSlabEnsemble), from gb.zonal_eddy's records: lorenz_cycle_of_records with the grid's zc, y = radius x
    latitude of the rows and g / rho0.  Refuses a grid with 2-D metrics: there a line is not a latitude circle."""
    b = _backend_of(model)
    first = b.backends[0] if hasattr(b, "backends") else b
    if first.cfg.grid_type not in LAT_LON_GRID_TYPES:
        raise ValueError("lorenz_cycle: this grid has 2-D metrics (a curvilinear grid): a line along i is not a latitude circle; "
                         "the zonal-mean energy cycle is defined on the LatitudeLongitudeGrid only")
    if hasattr(b, "backends"):
        ze = b.zonal_eddy(levels)
        Ny, Nz = int(first.cfg.Ny), int(first.cfg.Nz)
        rows = [(r, j) for r in sorted({q.ry for q in b.backends}) for j in range(1, first.Ny_local + 1)]
        phi = [next(q for q in b.backends if q.ry == r).metric("phic", j) for r, j in rows]
    else:
        ze = zonal_eddy(b, levels, **host)
        Ny, Nz = b.field_dims("T", False)[1:]
        phi = [b.metric("phic", j) for j in range(1, Ny + 1)]
    k0, kc = _levels(levels, Nz)
    zc = np.array([first.metric("zc", k) for k in range(k0 + 1, k0 + kc + 1)], np.float64)
    y = float(first.cfg.radius) * np.deg2rad(np.asarray(phi, np.float64))
    return lorenz_cycle_of_records(ze, zc, y, first.cfg.g / first.cfg.rho0)
