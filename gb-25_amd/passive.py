"""Passive tracers carried beside a run: dyes and ideal age on the device (gb25_tracers_*, include/gb25.h), and the numpy
restatement of the one kernel that is new for them (k_passive_update, csrc/passive_kernels.hpp).

    tr = gb.passive_tracers(model, dye=2, age=True)
    tr.set(0, lambda lam, phi, z: np.exp(-((phi - 30) / 5) ** 2))
    gb.run_with_tracers(model, tr, 100)                  # advance(), then time_step, per step
    tr.get(0), tr.integral(0), tr.stats(2).max

A set is advanced by calls of its own BETWEEN the model's steps, with u, v, w as they stand: nothing inside a model step changes and
the model's bits are those of a run without tracers.  The tendency G = -div(U c) is the model's one-tracer kernel (the scheme T and
S are advected with); the update is

    c <- (c + dt ((1.5 + chi) G^n - (0.5 + chi) G^-)) + dt source        (Euler: the factors are 1 and 0)

in the model's float type without fused multiply-adds, then the surface reset, the clip, zero in immersed cells and the halo cells
(passive_update_host below, bit for bit).  Single domains with closure = nothing; a set is NOT part of a checkpoint: save it with
get, restore it with set -- set restarts with an Euler step, so the tracers of a restarted run are not those of the run that went on
to the last bit.

run_with_tracers cannot use the steady-state schedule of gb25_loop: every step is a gb25_time_step of its own, which ends with u, v
and w materialised in memory (one sweep and one w kernel that a step inside gb25_loop(n) leaves out), and every advance waits for
its launches before it returns."""
import numpy as np

from .binding import TRACERS_MAX, TracerSpec
from .integrals import FOLDED_GRID_TYPES, LAT_LON_GRID_TYPES, _halo, cell_measure


def ab2_factors(dtype, chi, euler):
    """(C1, C2) = (1.5 + chi, 0.5 + chi) as the device forms them: in the float type, chi = -0.5 for an Euler step."""
    dtype = np.dtype(dtype).type
    chi = dtype(-0.5) if euler else dtype(chi)
    return dtype(1.5) + chi, dtype(0.5) + chi


def passive_update_host(c, Gn, Gm, dt, chi, H, *, euler=False, source=0.0, surface_value=0.0, surface_reset=False,
                        clip_negative=False, kbot=None, fold=False, update=True):
    """k_passive_update restated: the new PARENT array [Nx + 2H, Ny + 2H, Nz + 2H] of one tracer from the parents of c, G^n, G^-.
    kbot: the first wet level of every interior column [Nx, Ny] (None: no immersed cell).  fold: the rows beyond the last row of
    cells are images across a zipper fold, else row Ny is the layer beyond a wall.  update = False: the mask and the halo cells
    alone (what gb25_tracers_set does to what it has copied).  Every cell the kernel does not write keeps its value."""
    c = np.array(c)
    dtype = c.dtype.type
    Nx, Ny, Nz = (n - 2 * H for n in c.shape)
    I = (slice(H, H + Nx), slice(H, H + Ny), slice(H, H + Nz))
    x = c[I].copy()
    if update:
        C1, C2 = ab2_factors(dtype, chi, euler)
        t = C1 * np.asarray(Gn, dtype)[I] - C2 * np.asarray(Gm, dtype)[I]
        x = (x + dtype(dt) * t) + dtype(float(dt) * float(source))
        if surface_reset:
            x[:, :, Nz - 1] = dtype(surface_value)
        if clip_negative:
            x = np.where(x < 0, dtype(0), x)
    if kbot is not None:
        x[np.arange(Nz)[None, None, :] < np.asarray(kbot)[:, :, None]] = 0
    out = c
    out[I] = x

    def x_images(rows, levels):
        """the periodic x images of the interior columns, over the given parent rows and levels"""
        out[:H, rows, levels] = out[Nx:Nx + H, rows, levels]
        out[H + Nx:, rows, levels] = out[H:2 * H, rows, levels]

    # the layer below the bottom and above the top of the interior rows
    out[I[0], I[1], H - 1] = x[:, :, 0]
    out[I[0], I[1], H + Nz] = x[:, :, Nz - 1]
    x_images(I[1], slice(H - 1, H + Nz + 1))
    # the layer beyond the southern wall: interior levels only
    out[I[0], H - 1, I[2]] = x[:, 0, :]
    x_images(H - 1, I[2])
    if fold:
        for q in range(1, H + 1):
            if Ny - 1 - q < 0:
                break
            src = out[I[0], H + Ny - 1 - q, H - 1:H + Nz + 1]          # (with its bottom / top layer)
            out[I[0], H + Ny - 1 + q, H - 1:H + Nz + 1] = src[::-1]    # cell (Nx-1-i, Ny-1+q) <- cell (i, Ny-1-q)
            x_images(H + Ny - 1 + q, slice(H - 1, H + Nz + 1))
    else:
        out[I[0], H + Ny, I[2]] = x[:, Ny - 1, :]
        x_images(H + Ny, I[2])
    return out


def kbot_interior(backend):
    """The first wet level of every interior column [Nx, Ny], or None on a model without a bottom table."""
    Nx, Ny, Nz = backend.field_dims("T", False)
    kb = np.array([[backend.bottom_info("kbot", i, j) for j in range(1, Ny + 1)] for i in range(1, Nx + 1)]).astype(np.int64)
    return np.minimum(kb, Nz) if kb.any() else None


def cell_centres(backend):
    """(lam [Nx, 1, 1], phi [Nx, Ny, 1], z [1, 1, Nz]) of the interior cell centres, float64.  phi is the latitude of the cell
    centre on every grid; lam is the longitude of the grid's column, lon_west + (i + 1/2) dlam -- on the tripolar grid the
    longitude the column has south of the cap."""
    Nx, Ny, Nz = backend.field_dims("T", False)
    cfg = backend.cfg
    lam = cfg.lon_west + (np.arange(Nx) + 0.5) * (cfg.lon_east - cfg.lon_west) / Nx
    if cfg.grid_type in LAT_LON_GRID_TYPES:
        phi = np.broadcast_to(np.array([backend.metric("phic", j) for j in range(1, Ny + 1)], np.float64)[None, :], (Nx, Ny))
    else:
        H = _halo(backend)
        phi = np.asarray(backend.metric2("phicc"), np.float64)[H:H + Nx, H:H + Ny]
    z = np.array([backend.metric("zc", k) for k in range(1, Nz + 1)], np.float64)
    return lam[:, None, None], np.array(phi)[:, :, None], z[None, None, :]


class PassiveTracers:
    """A set of passive tracers on the device, beside `model`.  names[n] is "dye0", "dye1", ... and "age"."""

    def __init__(self, model, specs, names=None):
        self.model = model
        self.backend = b = model.backend
        self.specs = [s if isinstance(s, TracerSpec) else TracerSpec(**s) for s in specs]
        self.names = list(names or [f"c{n}" for n in range(len(self.specs))])
        self.handle = b.tracers_begin(self.specs)
        self.count = len(self.specs)

    def _index(self, n):
        return self.names.index(n) if isinstance(n, str) else int(n)

    def set(self, n, value, include_halos=False):
        """Tracer n (index or name) from an array shaped like T's interior (parent with include_halos), or from
        callable(lam, phi, z) of the cell centres in degrees, degrees and metres.  The next advance is an Euler step."""
        b = self.backend
        if callable(value):
            lam, phi, z = cell_centres(b)
            value = np.broadcast_to(np.asarray(value(lam, phi, z), np.float64), b.field_dims("T", False))
            include_halos = False
        b.tracers_set(self.handle, self._index(n), value, include_halos)

    def get(self, n, include_halos=False):
        return self.backend.tracers_get(self.handle, self._index(n), "c", include_halos)

    def tendency(self, n, which="Gn", include_halos=False):
        """G^n of the last advance ("Gm": of the one before), -div(U c)."""
        return self.backend.tracers_get(self.handle, self._index(n), which, include_halos)

    def advance(self):
        """One dt with the model's u, v, w as they stand; call it before the model's step (run_with_tracers does)."""
        self.backend.tracers_advance(self.handle)

    def stats(self, n):
        return self.backend.tracers_stats(self.handle, self._index(n))

    def integral(self, n):
        """sum mu c over the interior, fp64 on the host with the cell measure of gb-25_amd/integrals.py."""
        return float((cell_measure(self.backend, "T") * np.asarray(self.get(n), np.float64)).sum())

    def clock(self):
        return self.backend.tracers_clock(self.handle)

    def close(self):
        if self.handle is not None and getattr(self.backend, "h", None):
            self.backend.tracers_end(self.handle)
        self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def passive_tracers(model, dye=1, age=False, clip_negative=False):
    """`dye` dyes (source 0) and, with age = True, an ideal age in seconds behind them (source 1, the top level reset to 0 after
    every update).  At most 8 tracers in a set."""
    specs = [TracerSpec(0.0, 0.0, 0, int(bool(clip_negative))) for _ in range(int(dye))]
    names = [f"dye{n}" for n in range(int(dye))]
    if age:
        specs.append(TracerSpec(1.0, 0.0, 1, 0))
        names.append("age")
    if not 1 <= len(specs) <= TRACERS_MAX:
        raise ValueError(f"a set holds 1 .. {TRACERS_MAX} tracers, got {len(specs)}")
    return PassiveTracers(model, specs, names)


def run_with_tracers(model, tracers, steps):
    """`steps` times: tracers.advance(), then one step of the model (the order the set's clock asks for).  At model iteration 0
    the step is first_time_step, and the advance before it needs w and the halo cells of u, v, which do not exist yet: initialize
    and update_state make them first (first_time_step makes them again, to the same bits)."""
    b = model.backend
    for _ in range(int(steps)):
        if b.clock()[1] == 0:
            b.initialize()
            b.update_state()
            tracers.advance()
            b.first_time_step()
        else:
            tracers.advance()
            b.time_step()
    return tracers
