"""Flow kinematics on the host: the definitions of include/gb25.h ("flow kinematics on the device") restated with numpy from a
backend's public getters alone -- get_field, metric / metric2, bottom_info, field_dims, and get_derived for the potential density
-- in fp64, with the operation order of the kernels (csrc/kinematics_kernels.hpp), so that the device's values equal these bit
for bit.  Works on binding.HipBackend and, with the potential density passed in, on the test suite's oracle backend; it is also
what the public functions fall back to on a backend without the kernel.

    at a cell (c,c,c), i and j 0-based interior:
        ax = DYFC(i+1,j) u(i+1,j) - DYFC(i,j) u(i,j)        ay = DXCF(i,j+1) v(i,j+1) - DXCF(i,j) v(i,j)
        divergence    delta = (ax + ay) / AZCC              normal_strain  s_n = (ax - ay) / AZCC              AZCC == 0 gives 0
    at a corner (f,f,c), the metrics, operands and order of derived.vorticity_host:
        dv = dy v(i,j) - dy' v(i-1,j)                        du = dx u(i,j) - dx' u(i,j-1)
        shear_strain  s_s = (dv + du) / Az      zeta = (dv - du) / Az      rossby_number  zeta / f      Az == 0, f == 0 give 0
    <a> = 0.25 ((a(i,j) + a(i+1,j)) + (a(i,j+1) + a(i+1,j+1))) over the four corners of a cell, of the fp64 values
        okubo_weiss   W = (s_n s_n + <s_s s_s>) - <zeta zeta>
    the gradient of x = T, S or the potential density as stored:
        dx(i) = (x(i,j) - x(i-1,j)) / DXFC(i,j), dy(j) = (x(i,j) - x(i,j-1)) / DYCF(i,j); 0 across a face with an immersed side
        and, dy, across the southern and the northern edge of the global grid
        gx = 0.5 (dx(i) + dx(i+1)), gy = 0.5 (dy(j) + dy(j+1))
        gradient      sqrt(gx gx + gy gy)
        frontogenesis F = -(((gx gx) (0.5 (delta + s_n)) + (gx gy) <s_s>) + (gy gy) (0.5 (delta - s_n)))
    the quantities at cells are 0 in an immersed cell
    LatitudeLongitudeGrid: DYFC = DYCF = dy, DXCF(j) = dxf(j), AZCC = azc(j), DXFC(j) = dxc(j), Az = azf(j), f = fcor(j)

u, v, T and S are read from the parent arrays (halo cells included) as get_field(name, True) returns them.  The potential density
and the immersed cells of the ring of columns around the interior are taken from the periodic image in x and the edge row in y
(stability.pad_ring), which is what the halo of a single domain holds: with them the restatement is one of a whole domain.
Results are local fields of a rank: there is nothing to combine, gather_kinematics places the ranks' results by their global
offsets."""
import numpy as np

from .derived import _dy, _levels, _metric2_parent
from .integrals import LAT_LON_GRID_TYPES, _halo
from .stability import pad_ring

KINEMATICS_NAMES = ("divergence", "normal_strain", "shear_strain", "okubo_weiss", "rossby_number", "gradient", "frontogenesis")
CORNER_KINDS = ("shear_strain", "rossby_number")
TRACER_KINDS = ("gradient", "frontogenesis")
TRACERS = ("T", "S", "potential_density")


def check_param(kind, param):
    """The tracer of a quantity as its id: 0 .. 2 (or the names of TRACERS) for the gradient and the frontogenesis function
    (default: the potential density), 0 for the others."""
    if kind not in KINEMATICS_NAMES:
        raise ValueError(f"kind: {kind!r} is none of {KINEMATICS_NAMES}")
    if kind in TRACER_KINDS:
        param = 2 if param is None else (TRACERS.index(param) if param in TRACERS else param)
        if param not in (0, 1, 2):
            raise ValueError(f"{kind}: the tracer is one of {TRACERS} or 0 .. 2, got {param!r}")
        return int(param)
    if param not in (None, 0):
        raise ValueError(f"{kind} takes no tracer, got {param!r}")
    return 0


def _rows(backend, name, first, count):
    """A row table of the LatitudeLongitudeGrid for the 0-based rows first .. first + count - 1, [1, count, 1]."""
    return np.array([backend.metric(name, j + 1) for j in range(first, first + count)], np.float64)[None, :, None]


def corner_values(backend, bx, by, levels=None):
    """(s_s, zeta, f) in fp64, not rounded, at the corners (i, j), i < bx, j < by, of the levels: [bx, by, k] twice and f
    broadcastable to them."""
    H = _halo(backend)
    Nz = backend.field_dims("T", False)[2]
    k0, kc = _levels(levels, Nz)
    u = np.asarray(backend.get_field("u", True), np.float64)
    v = np.asarray(backend.get_field("v", True), np.float64)
    ks = slice(H + k0, H + k0 + kc)

    def box(a, di, dj):
        return a[H + di:H + di + bx, H + dj:H + dj + by, ks]

    if backend.cfg.grid_type in LAT_LON_GRID_TYPES:
        dy = dyw = _dy(backend)
        dx, dxs, az, f = _rows(backend, "dxc", 0, by), _rows(backend, "dxc", -1, by), _rows(backend, "azf", 0, by), _rows(backend, "fcor", 0, by)
    else:
        dycf, dxfc, azff, fff = (_metric2_parent(backend, n) for n in ("dycf", "dxfc", "azff", "fff"))

        def box2(a, di, dj):
            return a[H + di:H + di + bx, H + dj:H + dj + by, None]

        dy, dyw, dx, dxs, az, f = box2(dycf, 0, 0), box2(dycf, -1, 0), box2(dxfc, 0, 0), box2(dxfc, 0, -1), box2(azff, 0, 0), box2(fff, 0, 0)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        dv = dy * box(v, 0, 0) - dyw * box(v, -1, 0)
        du = dx * box(u, 0, 0) - dxs * box(u, 0, -1)
        ss, zeta = (dv + du) / az, (dv - du) / az
    flat = np.broadcast_to(az, ss.shape) == 0.0
    return np.where(flat, 0.0, ss), np.where(flat, 0.0, zeta), f


def cell_strain(backend, levels=None):
    """(ax, ay, AZCC, delta, s_n) in fp64, not rounded, at the cells of the levels: [Nx, Ny, k] (AZCC broadcastable)."""
    H = _halo(backend)
    Nx, Ny, Nz = backend.field_dims("T", False)
    k0, kc = _levels(levels, Nz)
    u = np.asarray(backend.get_field("u", True), np.float64)
    v = np.asarray(backend.get_field("v", True), np.float64)
    ks = slice(H + k0, H + k0 + kc)

    def box(a, di, dj):
        return a[H + di:H + di + Nx, H + dj:H + dj + Ny, ks]

    if backend.cfg.grid_type in LAT_LON_GRID_TYPES:
        dyw = dye = _dy(backend)
        dxs, dxn, az = _rows(backend, "dxf", 0, Ny), _rows(backend, "dxf", 1, Ny), _rows(backend, "azc", 0, Ny)
    else:
        dyfc, dxcf, azcc = (_metric2_parent(backend, n) for n in ("dyfc", "dxcf", "azcc"))

        def box2(a, di, dj):
            return a[H + di:H + di + Nx, H + dj:H + dj + Ny, None]

        dyw, dye, dxs, dxn, az = box2(dyfc, 0, 0), box2(dyfc, 1, 0), box2(dxcf, 0, 0), box2(dxcf, 0, 1), box2(azcc, 0, 0)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ax = dye * box(u, 1, 0) - dyw * box(u, 0, 0)
        ay = dxn * box(v, 0, 1) - dxs * box(v, 0, 0)
        delta, sn = (ax + ay) / az, (ax - ay) / az
    flat = np.broadcast_to(az, delta.shape) == 0.0
    return ax, ay, az, np.where(flat, 0.0, delta), np.where(flat, 0.0, sn)


def corner_mean(a):
    """<a> of include/gb25.h: [Nx + 1, Ny + 1, k] at the corners -> [Nx, Ny, k] at the cells, in the written order."""
    return 0.25 * ((a[:-1, :-1] + a[1:, :-1]) + (a[:-1, 1:] + a[1:, 1:]))


def bottom_levels(backend):
    """kbot[i, j], the immersed cells of every column of the interior."""
    Nx, Ny, _ = backend.field_dims("T", False)
    return np.array([[backend.bottom_info("kbot", i, j) for j in range(1, Ny + 1)] for i in range(1, Nx + 1)]).astype(int)


def tracer_ring(backend, param, levels=None, sigma=None):
    """x of include/gb25.h with the ring of columns around the interior, float64 [Nx + 2, Ny + 2, k]: T or S from the parent
    array, the potential density as stored (sigma [i, j, k] of ALL levels; default: the backend's get_derived) with the periodic
    image in x and the edge row in y."""
    H = _halo(backend)
    Nx, Ny, Nz = backend.field_dims("T", False)
    k0, kc = _levels(levels, Nz)
    if param == 2:
        if sigma is None:
            sigma = backend.get_derived("potential_density")
        return pad_ring(np.asarray(sigma, np.float64)[:, :, k0:k0 + kc])
    a = np.asarray(backend.get_field(TRACERS[param], True), np.float64)
    return a[H - 1:H + Nx + 1, H - 1:H + Ny + 1, H + k0:H + k0 + kc]


def cell_gradient(backend, param, levels=None, sigma=None, kbot=None):
    """(gx, gy) in fp64, not rounded, at the cells of the levels: [Nx, Ny, k]."""
    H = _halo(backend)
    Nx, Ny, Nz = backend.field_dims("T", False)
    k0, kc = _levels(levels, Nz)
    x = tracer_ring(backend, param, levels, sigma)
    kb = pad_ring(bottom_levels(backend) if kbot is None else kbot)[:, :, None]
    wet = (k0 + np.arange(kc))[None, None, :] >= kb                  # [Nx + 2, Ny + 2, k]
    if backend.cfg.grid_type in LAT_LON_GRID_TYPES:
        gxw = gxe = _rows(backend, "dxc", 0, Ny)
        gys = gyn = _dy(backend)
    else:
        dxfc, dycf = (_metric2_parent(backend, n) for n in ("dxfc", "dycf"))
        gxw, gxe = dxfc[H:H + Nx, H:H + Ny, None], dxfc[H + 1:H + Nx + 1, H:H + Ny, None]
        gys, gyn = dycf[H:H + Nx, H:H + Ny, None], dycf[H:H + Nx, H + 1:H + Ny + 1, None]
    j0 = int(getattr(backend, "ry", 0)) * Ny                         # (the rank's first row in the global grid)
    rows = j0 + np.arange(Ny + 1)
    closed = ((rows == 0) | (rows == int(backend.cfg.Ny)))[None, :, None]
    xc, wc = x[1:-1, 1:-1], wet[1:-1, 1:-1]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        dw = np.where(wc & wet[:-2, 1:-1], (xc - x[:-2, 1:-1]) / gxw, 0.0)
        de = np.where(wc & wet[2:, 1:-1], (x[2:, 1:-1] - xc) / gxe, 0.0)
        ds = np.where(~closed[:, :-1] & wc & wet[1:-1, :-2], (xc - x[1:-1, :-2]) / gys, 0.0)
        dn = np.where(~closed[:, 1:] & wc & wet[1:-1, 2:], (x[1:-1, 2:] - xc) / gyn, 0.0)
        return 0.5 * (dw + de), 0.5 * (ds + dn)


def kinematics_pieces(backend, kind, param=None, levels=None, sigma=None):
    """Every fp64 piece `kind` is made of, not rounded, and the result "value" (float64, the zeros of include/gb25.h applied, not
    yet rounded to the backend's dtype): a dict with ax, ay, az, delta, s_n at the cells; s_s, zeta at the corners of the cells
    ([Nx + 1, Ny + 1, k]; the corner quantities: at their own box) and f; gx, gy -- those `kind` reads."""
    param = check_param(kind, param)
    Nx, Ny, Nz = backend.field_dims("T", False)
    k0, kc = _levels(levels, Nz)
    P = {}
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if kind in CORNER_KINDS:
            bx, by, _ = backend.field_dims("v", False)
            P["s_s"], P["zeta"], P["f"] = corner_values(backend, bx, by, levels)
            if kind == "shear_strain":
                P["value"] = P["s_s"]
            else:
                P["value"] = np.where(np.broadcast_to(P["f"], P["zeta"].shape) == 0.0, 0.0, P["zeta"] / P["f"])
            return P
        if kind != "gradient":
            P["ax"], P["ay"], P["az"], P["delta"], P["s_n"] = cell_strain(backend, levels)
        if kind in ("okubo_weiss", "frontogenesis"):
            P["s_s"], P["zeta"], _ = corner_values(backend, Nx + 1, Ny + 1, levels)
        kbot = bottom_levels(backend)
        if kind in TRACER_KINDS:
            P["gx"], P["gy"] = cell_gradient(backend, param, levels, sigma, kbot)
        if kind == "divergence":
            x = P["delta"]
        elif kind == "normal_strain":
            x = P["s_n"]
        elif kind == "okubo_weiss":
            x = (P["s_n"] * P["s_n"] + corner_mean(P["s_s"] * P["s_s"])) - corner_mean(P["zeta"] * P["zeta"])
        elif kind == "gradient":
            x = np.sqrt(P["gx"] * P["gx"] + P["gy"] * P["gy"])
        else:
            gx, gy, delta, sn = P["gx"], P["gy"], P["delta"], P["s_n"]
            x = -(((gx * gx) * (0.5 * (delta + sn)) + (gx * gy) * corner_mean(P["s_s"])) + (gy * gy) * (0.5 * (delta - sn)))
        if kind in ("okubo_weiss", "frontogenesis"):
            x = np.where(np.broadcast_to(P["az"], x.shape) == 0.0, 0.0, x)
        immersed = (k0 + np.arange(kc))[None, None, :] < kbot[:, :, None]
        P["value"] = np.where(immersed, 0.0, x)
    return P


def kinematics_host(backend, kind, param=None, levels=None, sigma=None):
    """One quantity of include/gb25.h from the backend's public getters, in the backend's dtype: [i, j, k] of the levels
    `levels` = (k_first, k_count), shaped like get_field("T", False) (the shear strain and the Rossby number: like
    get_field("v", False)).  param: the tracer of "gradient" and "frontogenesis" ("T", "S", "potential_density" or 0 .. 2);
    sigma: the potential density as stored, [i, j, k] of all levels (default: the backend's get_derived)."""
    with np.errstate(over="ignore", invalid="ignore"):
        return kinematics_pieces(backend, kind, param, levels, sigma)["value"].astype(backend.dtype)


def kinematics(backend, kind, param=None, levels=None, sigma=None):
    """From the device where the backend has the kernel, from the restatement where it has not."""
    if hasattr(backend, "get_kinematics"):
        return backend.get_kinematics(kind, check_param(kind, param), levels)
    return kinematics_host(backend, kind, param, levels, sigma=sigma)


def gather_kinematics(ensemble, kind, param=None, levels=None):
    """A quantity of a LocalSlabEnsemble (or anything with .backends): every rank computes its own interior on the device, the
    results are placed by global offset -- offset of a rank's interior = (rx Nx_local, ry Ny_local)."""
    parts = [(b, kinematics(b, kind, param, levels)) for b in ensemble.backends]
    nx = max(b.rx * b.Nx_local + a.shape[0] for b, a in parts)
    ny = max(b.ry * b.Ny_local + a.shape[1] for b, a in parts)
    out = np.zeros((nx, ny, parts[0][1].shape[2]), parts[0][1].dtype)
    for b, a in parts:
        i0, j0 = b.rx * b.Nx_local, b.ry * b.Ny_local
        out[i0:i0 + a.shape[0], j0:j0 + a.shape[1]] = a
    return out
