"""Derived fields on the host: the definitions of include/gb25.h ("derived fields on the device") restated with numpy from a
backend's public getters alone -- get_field, metric, metric2, bottom_info, field_dims -- in fp64, with the operation order of
the kernels (csrc/diagnostics_kernels.hpp, k_derived_*), so that vorticity, kinetic energy and mixed-layer depth of the device
equal these bit for bit.  Works on binding.HipBackend and on the test suite's oracle backend.

    zeta(i,j,k) = ((dy v(i,j,k) - dy' v(i-1,j,k)) - (dx u(i,j,k) - dx' u(i,j-1,k))) / Az       at (f,f,c), dims of v
        curvilinear grids:      dy = dycf(i,j), dy' = dycf(i-1,j), dx = dxfc(i,j), dx' = dxfc(i,j-1), Az = azff(i,j)
        LatitudeLongitudeGrid:  dy = dy' = metric("dy"), dx = dxc(j), dx' = dxc(j-1), Az = azf(j);   Az == 0 gives 0
    KE(i,j,k)   = 0.25 ((u(i)^2 + u(i+1)^2) + (v(j)^2 + v(j+1)^2))                              at (c,c,c)
    mixed-layer depth: sigma = the potential density as stored; d(k) = sigma(k) - sigma(top); marching down from the level
        below the top, at the first wet k with d(k) >= threshold:
        -(zc(k+1) + (zc(k) - zc(k+1)) ((threshold - d(k+1)) / (d(k) - d(k+1)))); never reached: -zf(first wet level); dry: 0

Values are read from the parent arrays (halo cells included) as get_field(name, True) returns them.  Results are local fields
of a rank: there is nothing to combine, gather_derived places the ranks' results by their global offsets."""
import math

import numpy as np

from .integrals import LAT_LON_GRID_TYPES, _halo

DERIVED_3D = ("vorticity", "kinetic_energy", "density_anomaly", "potential_density")
DERIVED_NAMES = DERIVED_3D + ("mixed_layer_depth",)


def _levels(levels, Nz):
    if levels is None:
        return 0, Nz
    k_first, k_count = levels
    return k_first, (Nz - k_first if k_count == -1 else k_count)


def _metric2_parent(backend, name):
    """One 2-D metric in the parent layout (Nx + 2H, Ny + 2H + 1), [i, j], float64."""
    try:
        return np.asarray(backend.metric2(name), np.float64)
    except TypeError:          # (a backend whose metric2 answers point by point)
        return np.asarray(backend.metric2_array(name), np.float64)


def _dy(backend):
    """The LatitudeLongitudeGrid's constant meridional spacing."""
    try:
        return float(backend.metric("dy", 1))
    except KeyError:           # (a backend without that metric id: the spacing from its configuration)
        c = backend.cfg
        return c.radius * ((c.lat_north - c.lat_south) / c.Ny) * (math.pi / 180.0)


def vorticity_host(backend, levels=None):
    """zeta at (f,f,c) for the interior levels `levels` = (k_first, k_count), shaped like get_field("v", False)."""
    H = _halo(backend)
    Nx, by, Nz = backend.field_dims("v", False)
    k0, kc = _levels(levels, Nz)
    u = np.asarray(backend.get_field("u", True), np.float64)
    v = np.asarray(backend.get_field("v", True), np.float64)
    ks = slice(H + k0, H + k0 + kc)

    def box(a, di, dj):
        return a[H + di:H + di + Nx, H + dj:H + dj + by, ks]

    if backend.cfg.grid_type in LAT_LON_GRID_TYPES:
        dy = dyw = _dy(backend)
        dx = np.array([backend.metric("dxc", j) for j in range(1, by + 1)], np.float64)[None, :, None]
        dxs = np.array([backend.metric("dxc", j - 1) for j in range(1, by + 1)], np.float64)[None, :, None]
        az = np.array([backend.metric("azf", j) for j in range(1, by + 1)], np.float64)[None, :, None]
    else:
        dycf, dxfc, azff = (_metric2_parent(backend, n) for n in ("dycf", "dxfc", "azff"))

        def box2(a, di, dj):
            return a[H + di:H + di + Nx, H + dj:H + dj + by, None]

        dy, dyw, dx, dxs, az = box2(dycf, 0, 0), box2(dycf, -1, 0), box2(dxfc, 0, 0), box2(dxfc, 0, -1), box2(azff, 0, 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        z = ((dy * box(v, 0, 0) - dyw * box(v, -1, 0)) - (dx * box(u, 0, 0) - dxs * box(u, 0, -1))) / az
    z = np.where(np.broadcast_to(az, z.shape) == 0.0, 0.0, z)
    return z.astype(backend.dtype)


def kinetic_energy_host(backend, levels=None):
    """KE at (c,c,c) for the interior levels `levels`, shaped like get_field("T", False)."""
    H = _halo(backend)
    Nx, Ny, Nz = backend.field_dims("T", False)
    k0, kc = _levels(levels, Nz)
    u = np.asarray(backend.get_field("u", True), np.float64)
    v = np.asarray(backend.get_field("v", True), np.float64)
    ks = slice(H + k0, H + k0 + kc)
    u0, u1 = u[H:H + Nx, H:H + Ny, ks], u[H + 1:H + 1 + Nx, H:H + Ny, ks]
    v0, v1 = v[H:H + Nx, H:H + Ny, ks], v[H:H + Nx, H + 1:H + 1 + Ny, ks]
    ke = 0.25 * ((u0 * u0 + u1 * u1) + (v0 * v0 + v1 * v1))
    return ke.astype(backend.dtype)


def mixed_layer_depth_of_profiles(sigma, zc, zf, kbot, threshold):
    """The mixed-layer depth of include/gb25.h for columns sigma[i, j, k] (k = 0 the deepest level), centres zc[k], faces
    zf[k] (Nz + 1 of them), kbot[i, j] immersed cells per column.  float64 [i, j]."""
    sigma = np.asarray(sigma, np.float64)
    zc, zf = np.asarray(zc, np.float64), np.asarray(zf, np.float64)
    kbot = np.asarray(kbot).astype(int)
    Nz = sigma.shape[2]
    if not threshold > 0:
        raise ValueError("the density threshold must be > 0 kg/m^3")
    wet_column = kbot < Nz
    depth = np.where(wet_column, -zf[np.minimum(kbot, Nz)], 0.0)
    found = ~wet_column
    s0 = sigma[:, :, Nz - 1]
    dprev = np.zeros(s0.shape)
    for k in range(Nz - 2, -1, -1):
        wet = k >= kbot
        dk = sigma[:, :, k] - s0
        hit = ~found & wet & (dk >= threshold)
        with np.errstate(divide="ignore", invalid="ignore"):
            value = -(zc[k + 1] + (zc[k] - zc[k + 1]) * ((threshold - dprev) / (dk - dprev)))
        depth = np.where(hit, value, depth)
        found |= hit
        dprev = np.where(wet, dk, dprev)
    return depth


def mixed_layer_depth_host(backend, sigma=None, threshold=0.03):
    """The mixed-layer depth [i, j, 1] from the potential density `sigma` [i, j, k] as stored (default: the backend's
    get_derived("potential_density")), the backend's zc, zf and bottom."""
    if sigma is None:
        sigma = backend.get_derived("potential_density")
    Nx, Ny, Nz = np.shape(sigma)
    zc = np.array([backend.metric("zc", k) for k in range(1, Nz + 1)], np.float64)
    zf = np.array([backend.metric("zf", k) for k in range(1, Nz + 2)], np.float64)
    kbot = np.array([[backend.bottom_info("kbot", i, j) for j in range(1, Ny + 1)] for i in range(1, Nx + 1)]).astype(int)
    depth = mixed_layer_depth_of_profiles(np.asarray(sigma, np.float64), zc, zf, kbot, threshold)
    return depth.astype(backend.dtype)[:, :, None]


def gather_derived(ensemble, name, param=None, levels=None):
    """A derived field of a LocalSlabEnsemble (or anything with .backends): every rank computes its own interior on the
    device, the results are placed by global offset -- offset of a rank's interior = (rx Nx_local, ry Ny_local)."""
    parts = [(b, b.get_derived(name, param, levels)) for b in ensemble.backends]
    nx = max(b.rx * b.Nx_local + a.shape[0] for b, a in parts)
    ny = max(b.ry * b.Ny_local + a.shape[1] for b, a in parts)
    out = np.zeros((nx, ny, parts[0][1].shape[2]), parts[0][1].dtype)
    for b, a in parts:
        i0, j0 = b.rx * b.Nx_local, b.ry * b.Ny_local
        out[i0:i0 + a.shape[0], j0:j0 + a.shape[1]] = a
    return out
