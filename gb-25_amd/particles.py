"""Lagrangian particles on the host: the section "Lagrangian particles advected and sampled on the device" of include/gb25.h
restated with numpy from a backend's public getters alone -- get_field, metric, metric2, bottom_info --, in fp64 with the
operation order of the kernel (csrc/particle_kernels.hpp, k_particles_advance), so that the device's particles equal these bit
for bit; the same advance for a backend without the device kernel (ParticlesHost); the handle gb.particles returns; seeding; and
the hand-over of particles between the ranks of a decomposition, which runs on the host.  Works on binding.HipBackend and on the
test suite's oracle backend.

A particle is a cell (i, j, k), int32, 0-based in the rank's interior, fractions (a, b, c) in [0, 1) from the cell's western,
southern and lower face, and a status (binding.PARTICLE_STATUS).  A state is a dict of seven arrays: i j k a b c status.

    rate      dxi   = (1 - a) * (u(i,j,k) / dxu(i,j)) + a * (u(i+1,j,k) / dxu(i+1,j))        dxu: dxfc(i,j)  (lat-lon: dxc(j))
              deta  = (1 - b) * (v(i,j,k) / dyv(i,j)) + b * (v(i,j+1,k) / dyv(i,j+1))        dyv: dycf(i,j)  (lat-lon: dy)
              dzeta = ((1 - c) * w(i,j,k) + c * w(i,j,k+1)) / dzc(k)
    substep   r0 = rate(p); pm = move(p, (0.5 h) r0); r1 = rate(pm); p <- move(p, h r1)           h = dt / substeps
    move      re-cell every component, then x wrap, y walls, z clamp, dry-cell block (include/gb25.h has the rules)
"""
import numpy as np

from .binding import PARTICLE_COUNTERS, PARTICLE_STATUS, ParticlesInfo
from .derived import _dy, _metric2_parent
from .integrals import FOLDED_GRID_TYPES, LAT_LON_GRID_TYPES, _halo

ACTIVE, AT_FOLD, OUTSIDE, NONFINITE = (PARTICLE_STATUS[n] for n in ("active", "at_fold", "outside", "nonfinite"))
BELOW_ONE = float(np.nextafter(1.0, 0.0))      # the largest double below 1
FAR = float(2 ** 30)                            # a displacement not below it (in cells) counts as not finite
STATE_KEYS = ("i", "j", "k", "a", "b", "c", "status")
CCC_FIELDS = ("T", "S", "pHY", "Gn.T", "Gn.S", "Gm.T", "Gm.S", "e", "Gn.e", "Gm.e", "Le")


class TooFar(ValueError):
    """An advance that would move a particle more than one cell beyond the rank's interior: nothing was moved."""

    def __init__(self, count):
        super().__init__(f"{count} particle(s) would leave the rank by more than one cell per call: more substeps or a shorter dt")
        self.count = count


def make_state(i, j, k, a=0.5, b=0.5, c=0.5, status=None):
    """A state from cells and fractions (scalars broadcast), every particle ACTIVE unless status is given."""
    i = np.atleast_1d(np.asarray(i))
    n = i.size
    out = {q: np.array(np.broadcast_to(np.asarray(x), (n,)), np.int32) for q, x in (("i", i), ("j", j), ("k", k))}
    out.update({q: np.array(np.broadcast_to(np.asarray(x, np.float64), (n,))) for q, x in (("a", a), ("b", b), ("c", c))})
    out["status"] = np.zeros(n, np.int32) if status is None else np.array(status, np.int32)
    return out


def copy_state(state):
    return {q: np.array(state[q]) for q in STATE_KEYS}


def particle_fields(backend):
    """The three parent arrays an advance reads, as float64: {"u", "v", "w"}."""
    return {n: np.asarray(backend.get_field(n, True), np.float64) for n in ("u", "v", "w")}


def kbot_table(backend):
    """The first wet level of every column the parent arrays hold, int [Nx + 2H, Ny + 2H + 1] (the parent layout of a (c,f) 2-D
    field): the interior from bottom_info; rows beyond the interior repeat the nearest row (what gb25_get_bottom_info does at the
    walls); x halo columns are the periodic images on a single domain.  On a rank with neighbours they repeat the edge column
    here -- the device holds the neighbours' values: pass the true table as tables["kbot"] where that matters."""
    H = _halo(backend)
    Nx, Ny, Nz = backend.field_dims("T", False)
    kb = np.array([[backend.bottom_info("kbot", i, j) for j in range(1, Ny + 1)] for i in range(1, Nx + 1)]).astype(np.int64)
    kb = np.minimum(kb, Nz)
    ii = np.arange(-H, Nx + H)
    ii = ii % Nx if _x_periodic(backend) else np.clip(ii, 0, Nx - 1)
    jj = np.clip(np.arange(-H, Ny + H + 1), 0, Ny - 1)
    return kb[ii][:, jj]


def _x_periodic(backend):
    return getattr(backend, "Rx", 1) == 1 and not getattr(backend.cfg, "slab_mode", 0)


def particle_tables(backend):
    """Everything an advance needs besides the velocities: sizes, the metrics gb25_get_metric / gb25_get_metric2 return, kbot, the
    walls.  Arrays are indexed by (index + H) like the parent arrays."""
    H = _halo(backend)
    Nx, Ny, Nz = backend.field_dims("T", False)
    cfg = backend.cfg
    t = dict(H=H, Nx=Nx, Ny=Ny, Nz=Nz, curv=cfg.grid_type not in LAT_LON_GRID_TYPES, x_periodic=_x_periodic(backend))
    if t["curv"]:
        t["dxu"], t["dyv"] = _metric2_parent(backend, "dxfc"), _metric2_parent(backend, "dycf")
    else:
        t["dxu"] = np.array([backend.metric("dxc", j + 1) for j in range(-H, Ny + H - 1)], np.float64)
        t["dy"] = _dy(backend)
    t["dzc"] = np.array([backend.metric("dzc", k + 1) for k in range(-H, Nz + H - 1)], np.float64)
    t["kbot"] = kbot_table(backend)
    ry, Ry = getattr(backend, "ry", 0), getattr(backend, "Ry", 1)
    j0 = ry * Ny
    folded = cfg.grid_type in FOLDED_GRID_TYPES
    t["fold"] = folded and ry == Ry - 1
    t["j_south"] = -j0
    t["j_north"] = Ny if t["fold"] else (1 << 20) if folded else cfg.Ny - j0
    return t


def _rates(t, f, i, j, k, a, b, c):
    H = t["H"]
    ic = np.clip(i, -H, t["Nx"] + H - 2) + H
    jc = np.clip(j, -H, t["Ny"] + H - 2) + H
    kc = np.clip(k, -H, t["Nz"] + H - 2) + H
    u, v, w = f["u"], f["v"], f["w"]
    u0, u1 = u[ic, jc, kc], u[ic + 1, jc, kc]
    v0, v1 = v[ic, jc, kc], v[ic, jc + 1, kc]
    w0, w1 = w[ic, jc, kc], w[ic, jc, kc + 1]
    if t["curv"]:
        dx0, dx1 = t["dxu"][ic, jc], t["dxu"][ic + 1, jc]
        dy0, dy1 = t["dyv"][ic, jc], t["dyv"][ic, jc + 1]
    else:
        dx0 = dx1 = t["dxu"][jc]
        dy0 = dy1 = t["dy"]
    dz = t["dzc"][kc]
    with np.errstate(all="ignore"):
        rx = (1.0 - a) * (u0 / dx0) + a * (u1 / dx1)
        ry = (1.0 - b) * (v0 / dy0) + b * (v1 / dy1)
        rz = ((1.0 - c) * w0 + c * w1) / dz
    return rx, ry, rz


def particle_rates(backend, state, fields=None, tables=None):
    """(dxi, deta, dzeta) of every particle of the state, cells per second, float64."""
    t = tables if tables is not None else particle_tables(backend)
    f = fields if fields is not None else particle_fields(backend)
    return _rates(t, f, *(np.asarray(state[q]) for q in ("i", "j", "k", "a", "b", "c")))


def _recell(i, a, d):
    x = a + d
    n = np.floor(x)
    i = i + n.astype(np.int32)
    x = x - n
    over = x >= 1.0
    return (i + over).astype(np.int32), np.where(over, 0.0, x)


def _kbot(t, i, j):
    H = t["H"]
    return t["kbot"][np.clip(i, -H, t["Nx"] + H - 1) + H, np.clip(j, -H, t["Ny"] + H) + H]


def _move(t, p, dx, dy, dz):
    """move(p, d): the new position and the events (blocked, clamped_y, clamped_z, too_far) as boolean arrays."""
    i0, j0, k0, a0, b0, c0 = p
    i, a = _recell(i0, a0, dx)
    j, b = _recell(j0, b0, dy)
    k, c = _recell(k0, c0, dz)
    if t["x_periodic"]:
        i = (i % t["Nx"]).astype(np.int32)
    south, north = j < t["j_south"], j >= t["j_north"]
    j = np.where(south, t["j_south"], np.where(north, t["j_north"] - 1, j)).astype(np.int32)
    b = np.where(south, 0.0, np.where(north, BELOW_ONE, b))
    kb0, kb1 = _kbot(t, i0, j0), _kbot(t, i, j)
    low = k < kb0
    k = np.where(low, kb0, k)
    c = np.where(low, 0.0, c)
    high = k >= t["Nz"]
    k = np.where(high, t["Nz"] - 1, k).astype(np.int32)
    c = np.where(high, BELOW_ONE, c)
    blocked = kb1 > k
    i, j = np.where(blocked, i0, i).astype(np.int32), np.where(blocked, j0, j).astype(np.int32)
    a, b = np.where(blocked, a0, a), np.where(blocked, b0, b)
    far = (i < -1) | (i > t["Nx"]) | (j < -1) | (j > t["Ny"])
    return (i, j, k, a, b, c), dict(blocked=blocked, clamped_y=south | north, clamped_z=low | high, too_far=far)


def _small(dx, dy, dz):
    with np.errstate(invalid="ignore"):
        return (np.abs(dx) < FAR) & (np.abs(dy) < FAR) & (np.abs(dz) < FAR)


def advance_host(backend, state, dt, substeps=1, fields=None, tables=None):
    """`substeps` midpoint substeps of dt / substeps on the backend's fields as they are now (or on `fields` / `tables` taken
    earlier).  Returns (new state, counters {name: count} of PARTICLE_COUNTERS); the state passed in is not changed.  TooFar if a
    particle would leave the rank by more than one cell (x slabs, 2-D mesh)."""
    dt = float(dt)
    if not (np.isfinite(dt) and dt > 0):
        raise ValueError(f"dt must be finite and > 0, got {dt!r}")
    if int(substeps) != substeps or substeps <= 0:
        raise ValueError(f"substeps must be an integer > 0, got {substeps!r}")
    t = tables if tables is not None else particle_tables(backend)
    f = fields if fields is not None else particle_fields(backend)
    s = copy_state(state)
    p = tuple(s[q] for q in ("i", "j", "k", "a", "b", "c"))
    status = s["status"]
    cnt = {n: 0 for n in PARTICLE_COUNTERS}
    h = dt / float(substeps)
    hh = 0.5 * h
    dead = np.zeros(status.shape, bool)
    Nx, Ny = t["Nx"], t["Ny"]

    def at_fold(p):
        return (p[1] > Ny - 1) | ((p[1] == Ny - 1) & (p[4] >= 0.5))

    for _ in range(int(substeps)):
        act = (status == ACTIVE) & ~dead
        if t["fold"]:
            hit = act & at_fold(p)
            status[hit] = AT_FOLD
            cnt["at_fold"] += int(hit.sum())
            act &= ~hit
        with np.errstate(all="ignore"):
            d0 = tuple(hh * r for r in _rates(t, f, *p))
        bad = act & ~_small(*d0)
        act &= ~bad
        pm, evm = _move(t, p, *(np.where(act, d, 0.0) for d in d0))
        with np.errstate(all="ignore"):
            d1 = tuple(h * r for r in _rates(t, f, *pm))
        bad |= act & ~_small(*d1)
        status[bad] = NONFINITE
        cnt["nonfinite"] += int(bad.sum())
        act &= ~bad
        q, ev = _move(t, p, *(np.where(act, d, 0.0) for d in d1))
        far = act & (ev["too_far"] | evm["too_far"])
        cnt["too_far"] += int(far.sum())
        dead |= far
        act &= ~far
        p = tuple(np.where(act, new, old) for new, old in zip(q, p))
        for n in ("blocked", "clamped_y", "clamped_z"):
            cnt[n] += int((act & ev[n]).sum())
        hit = act & at_fold(p) if t["fold"] else np.zeros(act.shape, bool)
        out = act & ~hit & ((p[0] < 0) | (p[0] >= Nx) | (p[1] < 0) | (p[1] >= Ny))
        status[hit] = AT_FOLD
        status[out] = OUTSIDE
        cnt["at_fold"] += int(hit.sum())
        cnt["outside"] += int(out.sum())
    if cnt["too_far"]:
        raise TooFar(cnt["too_far"])
    for q, x in zip(("i", "j", "k"), p[:3]):
        s[q] = np.ascontiguousarray(x, np.int32)
    for q, x in zip(("a", "b", "c"), p[3:]):
        s[q] = np.ascontiguousarray(x, np.float64)
    return s, cnt


def sample_host(backend, state, name, field=None):
    """The value of the (c,c,c) field `name` in every particle's cell, float64 (halo cells for OUTSIDE particles)."""
    if name not in CCC_FIELDS:
        raise ValueError(f"sample: {name!r} is not a (c,c,c) field (one of {CCC_FIELDS})")
    H = _halo(backend)
    Nx, Ny, Nz = backend.field_dims("T", False)
    a = np.asarray(field if field is not None else backend.get_field(name, True))
    return np.asarray(a[np.clip(state["i"], -H, Nx + H - 1) + H, np.clip(state["j"], -H, Ny + H - 1) + H,
                        np.clip(state["k"], -H, Nz + H - 1) + H], np.float64)


def check_settable(backend, state, kbot=None):
    """What gb25_particles_set refuses: a cell outside the interior, a fraction outside [0, 1), a dry cell."""
    Nx, Ny, Nz = backend.field_dims("T", False)
    i, j, k = state["i"], state["j"], state["k"]
    if ((i < 0) | (i >= Nx) | (j < 0) | (j >= Ny) | (k < 0) | (k >= Nz)).any():
        raise ValueError(f"a particle's cell i, j, k is outside the interior {Nx} x {Ny} x {Nz}")
    for q in ("a", "b", "c"):
        if not ((state[q] >= 0.0) & (state[q] < 1.0)).all():
            raise ValueError(f"a particle's fraction {q} must lie in [0, 1)")
    H = _halo(backend)
    kb = kbot_table(backend) if kbot is None else kbot
    if (k < kb[i + H, j + H]).any():
        raise ValueError("a particle's cell i, j, k is dry")


class ParticlesHost:
    """gb25_particles_* in numpy for any backend: the fallback of a backend without the device kernel.  The methods are those
    HipBackend has under the names particles_set / particles_get / particles_advance / particles_sample / particles_info."""

    def __init__(self, backend, capacity):
        if capacity <= 0:
            raise ValueError(f"capacity = {capacity} must be > 0")
        self.backend, self.capacity = backend, int(capacity)
        self.state = make_state(np.zeros(0, np.int32), 0, 0)
        self.tables = None
        self._info = dict(calls=0, substeps=0, time_advanced=0.0, last=[0] * 8, total=[0] * 8)

    def set(self, i, j, k, a, b, c, first=0):
        new = make_state(i, j, k, a, b, c)
        n = new["i"].size
        if first < 0 or first > self.state["i"].size or first + n > self.capacity:
            raise ValueError(f"window first = {first}, count = {n} of {self.state['i'].size} particles so far, capacity {self.capacity}")
        if self.tables is None:
            self.tables = particle_tables(self.backend)
        check_settable(self.backend, new, self.tables["kbot"])
        self.state = {q: np.concatenate([self.state[q][:first], new[q]]) for q in STATE_KEYS}

    def get(self):
        return copy_state(self.state)

    def advance(self, dt, substeps=1):
        if self.tables is None:
            self.tables = particle_tables(self.backend)
        I = self._info
        try:
            self.state, cnt = advance_host(self.backend, self.state, dt, substeps, tables=self.tables)
        except TooFar as e:
            I["last"] = [0] * 8
            I["last"][PARTICLE_COUNTERS.index("too_far")] = e.count
            I["total"][PARTICLE_COUNTERS.index("too_far")] += e.count
            raise
        I["last"] = [cnt[n] for n in PARTICLE_COUNTERS] + [0]
        I["total"] = [x + y for x, y in zip(I["total"], I["last"])]
        I["calls"] += 1
        I["substeps"] += int(substeps)
        I["time_advanced"] = I["time_advanced"] + float(dt)

    def sample(self, name):
        return sample_host(self.backend, self.state, name)

    def info(self):
        out = ParticlesInfo()
        out.count, out.capacity = self.state["i"].size, self.capacity
        out.calls, out.substeps, out.time_advanced = self._info["calls"], self._info["substeps"], self._info["time_advanced"]
        out.last[:], out.total[:] = self._info["last"], self._info["total"]
        return out

    def end(self):
        self.state = make_state(np.zeros(0, np.int32), 0, 0)


class _DeviceParticles:
    """The same methods on a backend that has the kernel."""

    def __init__(self, backend, capacity):
        self.backend = backend
        backend.particles_begin(capacity)

    def set(self, i, j, k, a, b, c, first=0): self.backend.particles_set(i, j, k, a, b, c, first)
    def get(self): return self.backend.particles_get()
    def advance(self, dt, substeps=1): self.backend.particles_advance(dt, substeps)
    def sample(self, name): return self.backend.particles_sample(name)
    def info(self): return self.backend.particles_info()

    def end(self):
        if getattr(self.backend, "h", None):
            self.backend.particles_end()


class Particles:
    """The handle `particles(model, i, j, k, ...)` returns: Lagrangian particles advected where the velocities live
    (include/gb25.h, "Lagrangian particles advected and sampled on the device").  advance() between two composite calls moves
    them through the fields as they are now -- one launch, nothing downloaded --; positions / sample copy to the host."""

    def __init__(self, model, i, j, k, a=0.5, b=0.5, c=0.5, capacity=None):
        self.model = model
        b_ = model.backend
        s = make_state(i, j, k, a, b, c)
        capacity = max(1, s["i"].size) if capacity is None else int(capacity)
        self._p = _DeviceParticles(b_, capacity) if hasattr(b_, "particles_begin") else ParticlesHost(b_, capacity)
        self._p.set(*(s[q] for q in ("i", "j", "k", "a", "b", "c")))
        self._time = b_.clock()[0]

    def advance(self, dt=None, substeps=1):
        """Move the particles over dt (default: the model time elapsed since the last advance, or since the handle was made)
        in `substeps` midpoint substeps through the velocities as they are now."""
        now = self.model.backend.clock()[0]
        if dt is None:
            dt = now - self._time
        self._p.advance(dt, substeps)
        self._time = now
        return self

    def state(self):
        """{"i", "j", "k", "a", "b", "c", "status"} as the library holds them."""
        return self._p.get()

    def positions(self):
        """{"xi", "eta", "zeta" (index coordinates i + a, j + b, k + c, float64), "status"}."""
        s = self._p.get()
        return dict(xi=s["i"] + s["a"], eta=s["j"] + s["b"], zeta=s["k"] + s["c"], status=s["status"])

    def depth(self):
        """z of every particle [m, negative down]: zf(k) + c * dzc(k)."""
        b = self.model.backend
        Nz = b.field_dims("T", False)[2]
        zf = np.array([b.metric("zf", k + 1) for k in range(Nz)], np.float64)
        dz = np.array([b.metric("dzc", k + 1) for k in range(Nz)], np.float64)
        s = self._p.get()
        k = np.clip(s["k"], 0, Nz - 1)
        return zf[k] + s["c"] * dz[k]

    def sample(self, name):
        """The value of a (c,c,c) field ("T", "S", "e", "pHY", ...) in every particle's cell, float64: a copy, hence exact."""
        return self._p.sample(name)

    def info(self):
        return self._p.info()

    def close(self):
        self._p.end()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def particles(model, i, j, k, a=0.5, b=0.5, c=0.5, capacity=None):
    """Start particles in the cells (i, j, k) (0-based interior) at the fractions (a, b, c); returns the Particles handle:
    `p = particles(model, i, j, k); loop(model, 10); p.advance(); p.positions(); p.sample("T"); p.close()`."""
    return Particles(model, i, j, k, a, b, c, capacity)


def run_with_particles(model, p, steps, every=1, substeps=1, fields=("T", "S")):
    """loop(model, every) then p.advance(), repeated until `steps` steps are done (a remainder shorter than `every` is stepped
    and advanced last); returns the trajectory {"xi", "eta", "zeta", "status", "time", and one entry per sampled field}, arrays
    [samples, N] (time: [samples])."""
    out = {n: [] for n in ("xi", "eta", "zeta", "status", "time") + tuple(fields)}
    done = 0
    while done < steps:
        n = min(int(every), steps - done)
        model.backend.loop(n)
        p.advance(substeps=substeps)
        pos = p.positions()
        for q in ("xi", "eta", "zeta", "status"):
            out[q].append(pos[q])
        for q in fields:
            out[q].append(p.sample(q))
        out["time"].append(model.backend.clock()[0])
        done += n
    return {q: np.array(v) for q, v in out.items()}


def counter_uniform(n, seed, salt):
    """n numbers of U[0, 1) from SplitMix64 of the index: platform-independent, no global generator state."""
    with np.errstate(over="ignore"):
        x = (np.arange(n, dtype=np.uint64) + np.uint64(seed) * np.uint64(0x9E3779B97F4A7C15)
             + np.uint64(salt) * np.uint64(0xD1B54A32D192ED03))
        x ^= x >> np.uint64(30); x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(27); x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    return (x >> np.uint64(11)).astype(np.float64) / float(1 << 53)


def seed_positions(backend, n, levels=None, seed=0, rows=None):
    """A state of n particles uniform over the wet cells of the levels levels = (k_first, k_count) (None: all) and the rows
    rows = (j_first, j_count) (None: all; on a folded grid the pivot row, where a particle is frozen at once, is left out)."""
    H = _halo(backend)
    Nx, Ny, Nz = backend.field_dims("T", False)
    kb = kbot_table(backend)[H:H + Nx, H:H + Ny]
    k0, kc = (0, Nz) if levels is None else (levels[0], Nz - levels[0] if levels[1] == -1 else levels[1])
    j0, jc = (0, Ny - 1 if backend.cfg.grid_type in FOLDED_GRID_TYPES else Ny) if rows is None else rows
    wet = np.zeros((Nx, Ny, Nz), bool)
    wet[:, j0:j0 + jc, k0:k0 + kc] = True
    wet &= np.arange(Nz)[None, None, :] >= kb[:, :, None]
    cells = np.flatnonzero(wet.reshape(-1, order="F"))      # (i fastest, like the fields)
    if cells.size == 0:
        raise ValueError("no wet cell to seed")
    pick = cells[np.minimum((counter_uniform(n, seed, 1) * cells.size).astype(np.int64), cells.size - 1)]
    i, j, k = pick % Nx, (pick // Nx) % Ny, pick // (Nx * Ny)
    return make_state(i, j, k, *(counter_uniform(n, seed, salt) for salt in (2, 3, 4)))


def seed_particles(model, n, levels=None, seed=0, rows=None):
    """n particles seeded uniformly over the wet cells (seed_positions); returns the Particles handle."""
    s = seed_positions(model.backend, n, levels, seed, rows)
    return Particles(model, *(s[q] for q in ("i", "j", "k", "a", "b", "c")))


def exchange_particles(parts, offsets, shape=None):
    """The hand-over between the ranks of a decomposition, on the host.  parts[r]: the state of rank r (a dict of the seven
    arrays; further arrays of the same length, e.g. "id", travel with the particles); offsets[r] = (i0, j0), the rank's place in
    the global interior; shape = (Nx_local, Ny_local) (default: from the offsets).  Every OUTSIDE particle goes to the rank that
    owns its cell: the integer cell is shifted by the offsets (x periodic), the fractions are untouched, the status becomes
    ACTIVE.  Returns (new parts, moved) -- survivors in their order, then the arrivals ordered by source rank; moved: how many
    changed rank."""
    offsets = [tuple(int(x) for x in o) for o in offsets]
    if shape is None:
        xs, ys = sorted({o[0] for o in offsets}), sorted({o[1] for o in offsets})
        if len(xs) < 2:
            raise ValueError("exchange_particles: shape = (Nx_local, Ny_local) is needed with one rank along x")
        shape = (xs[1] - xs[0], ys[1] - ys[0] if len(ys) > 1 else None)
    nx, ny = shape
    Nx_global = max(o[0] for o in offsets) + nx
    owner = {(o[0] // nx, 0 if ny is None else o[1] // ny): r for r, o in enumerate(offsets)}
    keep, arrive = [], [[] for _ in parts]
    moved = 0
    for r, (part, (i0, j0)) in enumerate(zip(parts, offsets)):
        keys = list(part)
        out = np.asarray(part["status"]) == OUTSIDE
        keep.append({q: np.asarray(part[q])[~out] for q in keys})
        if not out.any():
            continue
        gi = (np.asarray(part["i"])[out].astype(np.int64) + i0) % Nx_global
        gj = np.asarray(part["j"])[out].astype(np.int64) + j0
        for n, (x, y) in enumerate(zip(gi, gj)):
            dest = owner.get((int(x) // nx, 0 if ny is None else int(y) // ny))
            if dest is None:
                raise ValueError(f"exchange_particles: no rank owns the global cell ({x}, {y}) of a particle of rank {r}")
            one = {q: np.asarray(part[q])[out][n:n + 1] for q in keys}
            one["i"] = np.array([x - offsets[dest][0]], np.int32)
            one["j"] = np.array([y - offsets[dest][1]], np.int32)
            one["status"] = np.array([ACTIVE], np.int32)
            arrive[dest].append(one)
            moved += 1
    new = []
    for r, k in enumerate(keep):
        new.append({q: np.concatenate([k[q]] + [one[q] for one in arrive[r]]) for q in k})
    return new, moved
