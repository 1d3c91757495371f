"""Stability diagnostics on the host: the definitions of include/gb25.h ("stability diagnostics on the device") restated with
numpy from a backend's public getters alone -- get_field, get_derived, metric / metric2, bottom_info, field_dims -- in fp64, with
the operation order of the kernels (csrc/stability_kernels.hpp, k_stability_faces, k_stability_wave_speed), so that the device's
values equal these bit for bit.  Works on binding.HipBackend and, with the potential density passed in, on the test suite's
oracle backend; it is also what the public functions fall back to on a backend without the kernel.

    face k lies between the cells k-1 and k (k = 0 the deepest level), dz = zc(k) - zc(k-1); sigma = the potential density as
    stored; b = -(g / rho0) sigma
    N2   = (-(g / rho0) (sigma(k) - sigma(k-1))) / dz
    S2   = du du + dv dv,  du = (ub(k) - ub(k-1)) / dz,  ub = 0.5 (u(i) + u(i+1)),  dv, vb likewise with v(j), v(j+1)
    Ri   = N2 / (S2 > floor ? S2 : floor)
    Eady = N2 > floor ? ((0.31 |fc|) sqrt(S2)) / sqrt(N2) : 0,  fc = 0.25 ((f(i,j) + f(i+1,j)) + (f(i,j+1) + f(i+1,j+1)))
    PV   = (fc + zb) N2 + (du by - dv bx),  zb = 0.125 (Z(k-1) + Z(k)),  Z = (z(i,j) + z(i+1,j)) + (z(i,j+1) + z(i+1,j+1)) of the
           vorticity as stored;  bx = 0.25 ((gx(i,k-1) + gx(i+1,k-1)) + (gx(i,k) + gx(i+1,k))),  gx(i) = (b(i) - b(i-1)) / dx(i),
           0 when either cell is immersed;  by likewise with y faces, 0 as well across the edges of the global grid
    c1   = (sum over the wet interior faces, bottom to top, of sqrt(N2 > 0 ? N2 : 0) dz) / pi
    faces 0 and Nz, and every face k <= kbot of the column, are 0

The potential density of the halo column is taken from the periodic image in x, which is what the halo of a single domain
holds; the restatement is therefore one of a whole domain in x.  Results are local fields of a rank: there is nothing to
combine, gather_stability places the ranks' results by their global offsets."""
import numpy as np

from .derived import _dy, _levels, _metric2_parent
from .integrals import LAT_LON_GRID_TYPES, _halo

STABILITY_NAMES = ("n2", "shear2", "richardson", "eady_rate", "ertel_pv", "wave_speed")
DEFAULT_PARAM = {"richardson": 1e-12}        # (a convention: the floor on S2 in s^-2; every other default is 0)
PI = 3.141592653589793


def check_param(kind, param):
    """The floor of a diagnostic as a float: > 0 for the Richardson number (default 1e-12), >= 0 for the Eady rate (default 0)."""
    if kind not in STABILITY_NAMES:
        raise ValueError(f"kind: {kind!r} is none of {STABILITY_NAMES}")
    param = float(DEFAULT_PARAM.get(kind, 0.0) if param is None else param)
    if kind == "richardson" and not param > 0.0:
        raise ValueError("the Richardson number needs a floor > 0 s^-2 on the squared shear")
    if kind == "eady_rate" and not param >= 0.0:
        raise ValueError("the Eady growth rate needs a floor >= 0 s^-2 on N^2")
    return param


def pad_ring(a, x_periodic=True):
    """An array [i, j, ...] with one ring of columns around it: the periodic image in x (or the edge column), the edge row in y
    (no result depends on a row beyond an edge of the global grid)."""
    a = np.asarray(a)
    west, east = (a[-1:], a[:1]) if x_periodic else (a[:1], a[-1:])
    a = np.concatenate([west, a, east], axis=0)
    return np.concatenate([a[:, :1], a, a[:, -1:]], axis=1)


def stability_of_columns(kind, zc, kbot, sigma=None, u=None, v=None, *, g_over_rho0, param=None, fc=None, zeta=None, dx=None,
                         dy=None, wall_y=None, levels=None):
    """The definitions of include/gb25.h on plain arrays, float64 [i, j, face] (the wave speed: [i, j, 1]), not yet rounded.
    For Nx x Ny columns of Nz levels, k = 0 the deepest:
        zc[k] the cell centres; kbot[Nx + 2, Ny + 2] the immersed cells per column WITH the ring of columns around the interior
        (pad_ring); sigma[Nx + 2, Ny + 2, Nz] the potential density with the same ring; u[Nx + 1, Ny, Nz] the x faces i and i + 1
        of every cell, v[Nx, Ny + 1, Nz] its y faces; fc[Nx, Ny] the Coriolis parameter at the cells; zeta[Nx + 1, Ny + 1, Nz] the
        vorticity at the cells' corners; dx[Nx + 1, Ny], dy[Nx, Ny + 1] the spacings across the x and the y faces; wall_y[Ny + 1]
        the y faces across which a gradient is 0.  Only what `kind` reads needs to be given.
    levels = (k_first, k_count) of the faces, 0-based, k_count = -1: all from k_first on."""
    param = check_param(kind, param)
    zc = np.asarray(zc, np.float64)
    Nz = zc.size
    kbot = np.asarray(kbot).astype(int)
    kb = kbot[1:-1, 1:-1]
    ngr = -float(g_over_rho0)
    if sigma is not None:
        sigma = np.asarray(sigma, np.float64)
        sc = sigma[1:-1, 1:-1]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if kind == "wave_speed":
            total = np.zeros(kb.shape)
            for k in range(1, Nz):
                dz = zc[k] - zc[k - 1]
                n2 = (ngr * (sc[:, :, k] - sc[:, :, k - 1])) / dz
                term = np.sqrt(np.where(n2 > 0.0, n2, 0.0)) * dz
                total = np.where(k > kb, total + term, total)
            return (total / PI)[:, :, None]
        k0, kc = _levels(levels, Nz + 1)
        out = np.zeros(kb.shape + (kc,))
        if kind != "n2":
            u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
            ub, vb = 0.5 * (u[:-1] + u[1:]), 0.5 * (v[:, :-1] + v[:, 1:])
        if kind == "ertel_pv":
            b = ngr * sigma
            zeta = np.asarray(zeta, np.float64)
            dx, dy = np.asarray(dx, np.float64), np.asarray(dy, np.float64)
            closed = np.asarray(wall_y, bool)[None, :]
            kc_, kw, ke, ks, kn = kbot[1:-1, 1:-1], kbot[:-2, 1:-1], kbot[2:, 1:-1], kbot[1:-1, :-2], kbot[1:-1, 2:]

            def gradients(l):
                bc, bw, be, bs, bn = b[1:-1, 1:-1, l], b[:-2, 1:-1, l], b[2:, 1:-1, l], b[1:-1, :-2, l], b[1:-1, 2:, l]
                wet = l >= kc_
                gxw = np.where(wet & (l >= kw), (bc - bw) / dx[:-1], 0.0)
                gxe = np.where(wet & (l >= ke), (be - bc) / dx[1:], 0.0)
                gys = np.where(~closed[:, :-1] & wet & (l >= ks), (bc - bs) / dy[:, :-1], 0.0)
                gyn = np.where(~closed[:, 1:] & wet & (l >= kn), (bn - bc) / dy[:, 1:], 0.0)
                return gxw, gxe, gys, gyn

            def corners(l):
                return (zeta[:-1, :-1, l] + zeta[1:, :-1, l]) + (zeta[:-1, 1:, l] + zeta[1:, 1:, l])

        for k in range(max(k0, 1), min(k0 + kc, Nz)):
            dz = zc[k] - zc[k - 1]
            if kind != "shear2":
                n2 = (ngr * (sc[:, :, k] - sc[:, :, k - 1])) / dz
            if kind != "n2":
                du, dv = (ub[:, :, k] - ub[:, :, k - 1]) / dz, (vb[:, :, k] - vb[:, :, k - 1]) / dz
                s2 = du * du + dv * dv
            if kind == "n2":
                x = n2
            elif kind == "shear2":
                x = s2
            elif kind == "richardson":
                x = n2 / np.where(s2 > param, s2, param)
            elif kind == "eady_rate":
                x = np.where(n2 > param, ((0.31 * np.abs(fc)) * np.sqrt(s2)) / np.sqrt(n2), 0.0)
            else:
                lo, hi = gradients(k - 1), gradients(k)
                bx = 0.25 * ((lo[0] + lo[1]) + (hi[0] + hi[1]))
                by = 0.25 * ((lo[2] + lo[3]) + (hi[2] + hi[3]))
                zb = 0.125 * (corners(k - 1) + corners(k))
                x = (fc + zb) * n2 + (du * by - dv * bx)
            out[:, :, k - k0] = np.where(k > kb, x, 0.0)
    return out


def vorticity_corners_host(backend):
    """The vorticity of include/gb25.h (GB25_D_VORTICITY) at the corners of every cell, [Nx + 1, Ny + 1, Nz]: the expression of
    derived.vorticity_host one column and one row further, rounded to the backend's dtype -- what gb25_get_derived hands out
    where it has the corner."""
    H = _halo(backend)
    Nx, Ny, Nz = backend.field_dims("T", False)
    bx, by = Nx + 1, Ny + 1
    u = np.asarray(backend.get_field("u", True), np.float64)
    v = np.asarray(backend.get_field("v", True), np.float64)
    ks = slice(H, H + Nz)

    def box(a, di, dj):
        return a[H + di:H + di + bx, H + dj:H + dj + by, ks]

    if backend.cfg.grid_type in LAT_LON_GRID_TYPES:
        dy = dyw = _dy(backend)
        dx = np.array([backend.metric("dxc", j) for j in range(1, by + 1)], np.float64)[None, :, None]
        dxs = np.array([backend.metric("dxc", j - 1) for j in range(1, by + 1)], np.float64)[None, :, None]
        az = np.array([backend.metric("azf", j) for j in range(1, by + 1)], np.float64)[None, :, None]
    else:
        dycf, dxfc, azff = (_metric2_parent(backend, n) for n in ("dycf", "dxfc", "azff"))

        def box2(a, di, dj):
            return a[H + di:H + di + bx, H + dj:H + dj + by, None]

        dy, dyw, dx, dxs, az = box2(dycf, 0, 0), box2(dycf, -1, 0), box2(dxfc, 0, 0), box2(dxfc, 0, -1), box2(azff, 0, 0)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        z = ((dy * box(v, 0, 0) - dyw * box(v, -1, 0)) - (dx * box(u, 0, 0) - dxs * box(u, 0, -1))) / az
    z = np.where(np.broadcast_to(az, z.shape) == 0.0, 0.0, z)
    return z.astype(backend.dtype)


def coriolis_at_cells(backend):
    """fc[i, j] of include/gb25.h: the mean of the Coriolis parameter at the four corners of a cell, in the written order."""
    H = _halo(backend)
    Nx, Ny, _ = backend.field_dims("T", False)
    if backend.cfg.grid_type in LAT_LON_GRID_TYPES:
        f = np.array([backend.metric("fcor", j) for j in range(1, Ny + 2)], np.float64)
        row = 0.25 * ((f[:-1] + f[:-1]) + (f[1:] + f[1:]))
        return np.broadcast_to(row[None, :], (Nx, Ny))
    f = _metric2_parent(backend, "fff")[H:H + Nx + 1, H:H + Ny + 1]
    return 0.25 * ((f[:-1, :-1] + f[1:, :-1]) + (f[:-1, 1:] + f[1:, 1:]))


def _face_spacings(backend, Nx, Ny):
    """(dx [Nx + 1, Ny] across the x faces, dy [Nx, Ny + 1] across the y faces)."""
    H = _halo(backend)
    if backend.cfg.grid_type in LAT_LON_GRID_TYPES:
        dxc = np.array([backend.metric("dxc", j) for j in range(1, Ny + 1)], np.float64)
        return np.broadcast_to(dxc[None, :], (Nx + 1, Ny)), np.full((Nx, Ny + 1), _dy(backend))
    return (_metric2_parent(backend, "dxfc")[H:H + Nx + 1, H:H + Ny], _metric2_parent(backend, "dycf")[H:H + Nx, H:H + Ny + 1])


def stability_host(backend, kind, param=None, levels=None, sigma=None, vorticity=None):
    """One stability diagnostic of include/gb25.h from the backend's public getters, in the backend's dtype: [i, j, face] for
    "n2", "shear2", "richardson", "eady_rate", "ertel_pv" (levels = (k_first, k_count) of the Nz + 1 faces), [i, j, 1] for
    "wave_speed".  sigma: the potential density as stored, [i, j, k] (default: the backend's get_derived); vorticity: the
    vorticity as stored at the corners of the cells, [Nx + 1, Ny + 1, Nz] (default: vorticity_corners_host)."""
    param = check_param(kind, param)
    H = _halo(backend)
    Nx, Ny, Nz = backend.field_dims("T", False)
    zc = np.array([backend.metric("zc", k) for k in range(1, Nz + 1)], np.float64)
    kbot = np.array([[backend.bottom_info("kbot", i, j) for j in range(1, Ny + 1)] for i in range(1, Nx + 1)]).astype(int)
    args = dict(g_over_rho0=backend.cfg.g / backend.cfg.rho0, param=param, levels=levels)
    if kind != "shear2":
        if sigma is None:
            sigma = backend.get_derived("potential_density")
        sigma = pad_ring(np.asarray(sigma, np.float64))
    u = v = None
    if kind not in ("n2", "wave_speed"):
        ks = slice(H, H + Nz)
        u = np.asarray(backend.get_field("u", True), np.float64)[H:H + Nx + 1, H:H + Ny, ks]
        v = np.asarray(backend.get_field("v", True), np.float64)[H:H + Nx, H:H + Ny + 1, ks]
    if kind in ("eady_rate", "ertel_pv"):
        args["fc"] = coriolis_at_cells(backend)
    if kind == "ertel_pv":
        args["zeta"] = vorticity_corners_host(backend) if vorticity is None else vorticity
        args["dx"], args["dy"] = _face_spacings(backend, Nx, Ny)
        j0 = int(getattr(backend, "ry", 0)) * Ny           # (the rank's first row in the global grid)
        rows = j0 + np.arange(Ny + 1)
        args["wall_y"] = (rows == 0) | (rows == int(backend.cfg.Ny))
    return stability_of_columns(kind, zc, pad_ring(kbot), sigma, u, v, **args).astype(backend.dtype)


def stability(backend, kind, param=None, levels=None, sigma=None, vorticity=None):
    """From the device where the backend has the kernel, from the restatement where it has not."""
    if hasattr(backend, "get_stability"):
        return backend.get_stability(kind, param, levels)
    return stability_host(backend, kind, param, levels, sigma=sigma, vorticity=vorticity)


def deformation_radius_of(c1, latitude, Omega, radius, equatorial_band=5.0):
    """The first baroclinic deformation radius [m] from the wave speed c1 [m/s] and the latitude [degrees] of the same points:
    c1 / |f| poleward of `equatorial_band` degrees, sqrt(c1 / (2 beta)) within it, f = 2 Omega sin(phi), beta = 2 Omega cos(phi)
    / radius.  Plain float64 host arithmetic."""
    c1 = np.asarray(c1, np.float64)
    phi = np.deg2rad(np.asarray(latitude, np.float64))
    f = 2.0 * Omega * np.sin(phi)
    beta = 2.0 * Omega * np.cos(phi) / radius
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(np.abs(np.asarray(latitude)) >= equatorial_band, c1 / np.abs(f), np.sqrt(c1 / (2.0 * beta)))


def cell_latitudes(backend):
    """The latitude of the cell centres [degrees], [i, j]."""
    H = _halo(backend)
    Nx, Ny, _ = backend.field_dims("T", False)
    if backend.cfg.grid_type in LAT_LON_GRID_TYPES:
        row = np.array([backend.metric("phic", j) for j in range(1, Ny + 1)], np.float64)
        return np.broadcast_to(row[None, :], (Nx, Ny))
    return _metric2_parent(backend, "phicc")[H:H + Nx, H:H + Ny]


def cell_spacings(backend):
    """max(dx, dy) of every cell [m], [i, j]: the spacings across its western and its southern face."""
    Nx, Ny, _ = backend.field_dims("T", False)
    dx, dy = _face_spacings(backend, Nx, Ny)
    return np.maximum(dx[:-1], dy[:, :-1])


def gather_stability(ensemble, kind, param=None, levels=None):
    """A stability diagnostic of a LocalSlabEnsemble (or anything with .backends): every rank computes its own columns on the
    device, the results are placed by global offset -- offset of a rank's interior = (rx Nx_local, ry Ny_local)."""
    parts = [(b, stability(b, kind, param, levels)) for b in ensemble.backends]
    nx = max(b.rx * b.Nx_local + a.shape[0] for b, a in parts)
    ny = max(b.ry * b.Ny_local + a.shape[1] for b, a in parts)
    out = np.zeros((nx, ny, parts[0][1].shape[2]), parts[0][1].dtype)
    for b, a in parts:
        i0, j0 = b.rx * b.Nx_local, b.ry * b.Ny_local
        out[i0:i0 + a.shape[0], j0:j0 + a.shape[1]] = a
    return out
