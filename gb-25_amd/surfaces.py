"""Fields on surfaces on the host: the definition of include/gb25.h ("fields on surfaces on the device") restated with numpy
from a backend's public getters alone -- get_field, get_derived, metric, bottom_info, field_dims -- in fp64, with the operation
order of the kernel (csrc/surface_kernels.hpp, k_on_surfaces), so that the values and status bytes of the device equal these bit
for bit.  Works on binding.HipBackend and, for the search variables and carried quantities that need no density, on the test
suite's oracle backend; it is also what the public functions fall back to on a backend without the kernel.

    per column, k increasing upward, kb = the first wet level, ks = Nz - 1; for a target c, marching k = Nz - 2 down to kb with
    qa = q(k+1), qb = q(k): the pair crosses when both are finite and (qa <= c <= qb) or (qb <= c <= qa); at the FIRST crossing
        frac = 0 if qa == qb else (c - qa) / (qb - qa);  g = 1 - frac
        depth = -(zc(k+1) g + zc(k) frac);  value = f(k+1) g + f(k) frac                              status FOUND
    no crossing, down = (q(kb) >= q(ks)):  (c > q(ks)) == down: depth = -zf(kb), value = f(kb)        status GROUNDED
                                           otherwise:           depth = -zf(Nz), value = f(ks)        status OUTCROP
    a dry column: 0, 0                                                                                status DRY

Results are local fields of a rank: there is nothing to combine, gather_surfaces places the ranks' results by their global
offsets."""
import numpy as np

from .derived import kinetic_energy_host

SURFACE_VARIABLES = ("T", "S", "potential_density", "depth")
SURFACE_CARRIED = ("depth", "T", "S", "e", "kinetic_energy", "density_anomaly", "potential_density")
FOUND, OUTCROP, GROUNDED, DRY = 0, 1, 2, 3
STATUS_NAMES = ("found", "outcrop", "grounded", "dry")
MAX_VALUES = 64


def check_values(values):
    """The targets as a float64 vector: 1 .. 64 finite values, in any order."""
    values = np.atleast_1d(np.asarray(values, np.float64)).reshape(-1)
    if not 1 <= values.size <= MAX_VALUES:
        raise ValueError(f"values: {values.size} of them, must be 1 .. {MAX_VALUES}")
    if not np.isfinite(values).all():
        raise ValueError("values: every value must be finite")
    return values


def surfaces_of_profiles(q, f, zc, zf, kbot, values):
    """The definition of include/gb25.h for columns q[i, j, k] of the search variable (k = 0 the deepest level) and f[i, j, k]
    of the carried quantity (None: the result is the depth), centres zc[k], faces zf[k] (Nz + 1 of them), kbot[i, j] immersed
    cells per column, targets values[n].  Returns (result float64 [i, j, n], status uint8 [i, j, n])."""
    q = np.asarray(q, np.float64)
    zc, zf = np.asarray(zc, np.float64), np.asarray(zf, np.float64)
    kbot = np.asarray(kbot).astype(int)
    c = check_values(values)[None, None, :]
    Nz = q.shape[2]
    q = np.broadcast_to(q, kbot.shape + (Nz,))
    f = None if f is None else np.broadcast_to(np.asarray(f, np.float64), q.shape)
    shape = kbot.shape + (c.shape[2],)
    wet_column = kbot < Nz
    kb = np.minimum(kbot, Nz - 1)
    ii, jj = np.indices(kbot.shape)
    q_kb, q_ks = q[ii, jj, kb], q[:, :, Nz - 1]
    result = np.zeros(shape)
    found = np.zeros(shape, bool)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for k in range(Nz - 2, -1, -1):
            wet = (k >= kbot)[:, :, None]
            qa, qb = q[:, :, k + 1, None], q[:, :, k, None]
            cross = np.isfinite(qa) & np.isfinite(qb) & (((qa <= c) & (c <= qb)) | ((qb <= c) & (c <= qa)))
            hit = ~found & wet & cross
            frac = np.where(qa == qb, 0.0, (c - qa) / (qb - qa))
            g = 1.0 - frac
            if f is None:
                value = -(zc[k + 1] * g + zc[k] * frac)
            else:
                value = f[:, :, k + 1, None] * g + f[:, :, k, None] * frac
            result = np.where(hit, value, result)
            found |= hit
        down = (q_kb >= q_ks)[:, :, None]
        grounded = (c > q_ks[:, :, None]) == down
    if f is None:
        at_bottom, at_top = -zf[np.minimum(kbot, Nz)][:, :, None], np.full(kbot.shape, -zf[Nz])[:, :, None]
    else:
        at_bottom, at_top = f[ii, jj, kb][:, :, None], f[:, :, Nz - 1, None]
    result = np.where(found, result, np.where(grounded, at_bottom, at_top))
    status = np.where(found, FOUND, np.where(grounded, GROUNDED, OUTCROP))
    wet3 = np.broadcast_to(wet_column[:, :, None], shape)
    return np.where(wet3, result, 0.0), np.where(wet3, status, DRY).astype(np.uint8)


def _column_tables(backend, Nx, Ny, Nz):
    zc = np.array([backend.metric("zc", k) for k in range(1, Nz + 1)], np.float64)
    zf = np.array([backend.metric("zf", k) for k in range(1, Nz + 2)], np.float64)
    kbot = np.array([[backend.bottom_info("kbot", i, j) for j in range(1, Ny + 1)] for i in range(1, Nx + 1)]).astype(int)
    return zc, zf, kbot


def on_surfaces_host(backend, variable, carried, values, sigma=None, ke=None):
    """(result [i, j, n] of the backend's dtype, status uint8 [i, j, n]) of include/gb25.h from the backend's public getters:
    the search variable `variable` ("T", "S", "potential_density", "depth"), the carried quantity `carried` ("depth", "T", "S",
    "e", "kinetic_energy", "density_anomaly", "potential_density").  sigma, ke: the potential density and the kinetic energy as
    stored, [i, j, k] (default: the backend's get_derived; the kinetic energy of a backend without it: kinetic_energy_host)."""
    if variable not in SURFACE_VARIABLES:
        raise ValueError(f"variable: {variable!r} is none of {SURFACE_VARIABLES}")
    if carried not in SURFACE_CARRIED:
        raise ValueError(f"carried: {carried!r} is none of {SURFACE_CARRIED}")
    values = check_values(values)
    Nx, Ny, Nz = backend.field_dims("T", False)
    zc, zf, kbot = _column_tables(backend, Nx, Ny, Nz)

    def stored(name):
        return np.asarray(backend.get_field(name, False), np.float64)

    def derived(name, given=None):
        return np.asarray(backend.get_derived(name) if given is None else given, np.float64)

    if variable == "depth":
        q = np.broadcast_to(-zc[None, None, :], (Nx, Ny, Nz))
    elif variable == "potential_density":
        q = derived("potential_density", sigma)
    else:
        q = stored(variable)
    if carried == "depth":
        f = None
    elif carried in ("T", "S", "e"):
        f = stored(carried)
    elif carried == "kinetic_energy":
        f = np.asarray(ke if ke is not None else
                       backend.get_derived("kinetic_energy") if hasattr(backend, "get_derived") else kinetic_energy_host(backend), np.float64)
    elif carried == "potential_density":
        f = q if variable == "potential_density" else derived("potential_density", sigma)
    else:
        f = derived(carried)
    result, status = surfaces_of_profiles(q, f, zc, zf, kbot, values)
    return result.astype(backend.dtype), status


def layer_thickness(depths):
    """The thickness of the layers between consecutive surfaces: depths[..., e + 1] - depths[..., e] along the last axis, in
    the precision of `depths` (positive where the surfaces are ordered downward, as isopycnals of increasing density are in a
    stable column).  A surface that outcrops sits at the top face, a grounded one at the column's bottom face, so that the
    layers between edges that bracket the whole column add up to its depth."""
    depths = np.asarray(depths)
    return depths[..., 1:] - depths[..., :-1]


def on_surfaces(backend, variable, carried, values):
    """(result, status) from the device where the backend has the kernel, from the restatement where it has not."""
    if hasattr(backend, "get_on_surfaces"):
        return backend.get_on_surfaces(variable, carried, values)
    return on_surfaces_host(backend, variable, carried, values)


def gather_surfaces(ensemble, variable, carried, values):
    """(result, status) of a LocalSlabEnsemble (or anything with .backends): every rank searches its own columns on the device,
    the results are placed by global offset -- offset of a rank's interior = (rx Nx_local, ry Ny_local)."""
    parts = [(b, on_surfaces(b, variable, carried, values)) for b in ensemble.backends]
    nx = max(b.rx * b.Nx_local + a.shape[0] for b, (a, _) in parts)
    ny = max(b.ry * b.Ny_local + a.shape[1] for b, (a, _) in parts)
    n = parts[0][1][0].shape[2]
    out, status = np.zeros((nx, ny, n), parts[0][1][0].dtype), np.zeros((nx, ny, n), np.uint8)
    for b, (a, s) in parts:
        i0, j0 = b.rx * b.Nx_local, b.ry * b.Ny_local
        out[i0:i0 + a.shape[0], j0:j0 + a.shape[1]] = a
        status[i0:i0 + a.shape[0], j0:j0 + a.shape[1]] = s
    return out, status
