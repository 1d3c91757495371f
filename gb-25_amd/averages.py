"""Time averages on the host: the terms of include/gb25.h ("time averages and eddy fluxes accumulated on the device") restated with
numpy from a backend's public getters alone -- get_field, field_dims --, in fp64 with the operation order of the kernel
(csrc/averages_kernels.hpp, k_averages_accumulate), so that the device's accumulators equal these bit for bit; the same
accumulation for a backend without the device kernel (AveragesHost); what follows from the means -- eddy fluxes, eddy kinetic
energy, tracer variance --; and the placement of the ranks' results in the global interior.  Works on binding.HipBackend and on
the test suite's oracle backend.

    MEANS    u v w T S eta       x, at the field's own location, interior dims of the field
    SQUARES  uu vv TT SS etaeta  x * x
    FLUXES   uT uS at (f,c,c)    u(i,j,k) * (0.5 * (T(i-1,j,k) + T(i,j,k)))
             vT vS at (c,f,c)    v(i,j,k) * (0.5 * (T(i,j-1,k) + T(i,j,k)))
             wT wS at (c,c,f)    w(i,j,k) * (0.5 * (T(i,j,k-1) + T(i,j,k))) at the faces 1 .. Nz-1, exactly 0 at the faces 0 and Nz

Values are read from the parent arrays (halo cells included) as get_field(name, True) returns them.  One sample adds
acc = acc + weight * term; the mean is acc / weight_sum.  window = (k_first, k_count) selects cell levels, 0-based, k_count = -1
or window = None: all; a (c,c,f) quantity covers the k_count + 1 faces that bound them, eta and etaeta ignore it."""
import numpy as np

from .binding import AVERAGE_GROUPS, AVERAGE_IDS, AveragesInfo, average_group_of, average_groups_mask
from .integrals import _halo

MEANS = ("u", "v", "w", "T", "S", "eta")
SQUARES = ("uu", "vv", "TT", "SS", "etaeta")
FLUXES = ("uT", "uS", "vT", "vS", "wT", "wS")
QUANTITIES = MEANS + SQUARES + FLUXES
SOURCES = ("u", "v", "w", "T", "S", "eta")
assert QUANTITIES == tuple(AVERAGE_IDS)


def _levels(window, Nz):
    """(k_first, k_count) resolved against Nz cell levels; an empty or out-of-range window is a ValueError."""
    k_first, k_count = (0, -1) if window is None else window
    kc = Nz - k_first if k_count == -1 else k_count
    if k_first < 0 or k_first >= Nz or k_count < -1 or k_count == 0 or k_first + kc > Nz:
        raise ValueError(f"levels {window!r} of {Nz}: empty or out of range")
    return int(k_first), int(kc)


def quantities_of(groups):
    """The names of the quantities of the groups (names or a mask), in the order of gb25_average."""
    mask = average_groups_mask(groups)
    return tuple(n for n in QUANTITIES if mask & AVERAGE_GROUPS[average_group_of(n)])


def sample_fields(backend):
    """The six parent arrays one sample reads, as float64: {"u", "v", "w", "T", "S", "eta"}."""
    return {n: np.asarray(backend.get_field(n, True), np.float64) for n in SOURCES}


def average_terms(backend, quantity, window=None, fields=None):
    """The term of `quantity` at every point of its packed box for the window, float64 [i, j, k]: what one sample of weight 1
    adds to a zero accumulator.  fields: sample_fields(backend) taken earlier (default: downloaded now)."""
    if quantity not in AVERAGE_IDS:
        raise ValueError(f"no average {quantity!r}: one of {QUANTITIES}")
    f = fields if fields is not None else sample_fields(backend)
    H = _halo(backend)
    Nx, Ny, Nz = backend.field_dims("T", False)
    byv = backend.field_dims("v", False)[1]
    k0, kc = _levels(window, Nz)
    ks = slice(H + k0, H + k0 + kc)

    def box(a, rows, di=0, dj=0, k=ks):
        return a[H + di:H + di + Nx, H + dj:H + dj + rows, k]

    if quantity in ("eta", "etaeta"):
        x = f["eta"][H:H + Nx, H:H + Ny, 0:1]
        return x.copy() if quantity == "eta" else x * x
    if quantity in MEANS or quantity in SQUARES:
        name = quantity[0]
        if name == "w":
            x = box(f["w"], Ny, k=slice(H + k0, H + k0 + kc + 1))
        else:
            x = box(f[name], byv if name == "v" else Ny)
        return x.copy() if quantity in MEANS else x * x
    vel, c = f[quantity[0]], f[quantity[1]]
    with np.errstate(invalid="ignore", over="ignore"):
        if quantity[0] == "u":
            return box(vel, Ny) * (0.5 * (box(c, Ny, di=-1) + box(c, Ny)))
        if quantity[0] == "v":
            return box(vel, byv) * (0.5 * (box(c, byv, dj=-1) + box(c, byv)))
        out = np.zeros((Nx, Ny, kc + 1))
        for q in range(kc + 1):
            kf = k0 + q
            if 1 <= kf <= Nz - 1:      # (the bottom and the top face carry exactly 0: no halo level is read)
                w = vel[H:H + Nx, H:H + Ny, H + kf]
                out[:, :, q] = w * (0.5 * (c[H:H + Nx, H:H + Ny, H + kf - 1] + c[H:H + Nx, H:H + Ny, H + kf]))
        return out


class AveragesHost:
    """The accumulation of gb25_averages_* in numpy for any backend: acc = acc + weight * term in that order, weight_sum on
    the side.  The methods are those of the handle gb.averages returns for a device model."""

    def __init__(self, backend, groups=("means", "squares", "fluxes"), levels=None):
        self.backend = backend
        self.groups = average_groups_mask(groups)
        if not self.groups & AVERAGE_GROUPS["means"] or self.groups & ~7:
            raise ValueError('groups must contain "means" (the eddy parts need the means)')
        self.k_first, self.k_count = _levels(levels, backend.field_dims("T", False)[2])
        self.window = (self.k_first, self.k_count)
        self.names = quantities_of(self.groups)
        self.acc = {}
        self.samples, self.weight_sum = 0, 0.0
        self.first, self.last = (0, 0.0), (0, 0.0)

    def sample(self, weight=1.0):
        weight = float(weight)
        if not (np.isfinite(weight) and weight > 0):
            raise ValueError(f"weight must be finite and > 0, got {weight!r}")
        fields = sample_fields(self.backend)
        with np.errstate(invalid="ignore", over="ignore"):
            for n in self.names:
                t = average_terms(self.backend, n, self.window, fields)
                self.acc[n] = (self.acc[n] if n in self.acc else np.zeros(t.shape)) + weight * t
        time, iteration = self.backend.clock()[:2]
        if self.samples == 0:
            self.first = (iteration, time)
        self.last = (iteration, time)
        self.samples += 1
        self.weight_sum = self.weight_sum + weight

    def info(self):
        out = AveragesInfo()
        out.groups, out.k_first, out.k_count, out.samples, out.weight_sum = self.groups, self.k_first, self.k_count, self.samples, self.weight_sum
        (out.first_iteration, out.first_time), (out.last_iteration, out.last_time) = self.first, self.last
        return out

    def raw(self, name):
        if name not in self.names:
            raise ValueError(f"average {name!r} belongs to a group that was not asked for")
        if name not in self.acc:
            return np.zeros(average_terms(self.backend, name, self.window).shape)
        return self.acc[name].copy()

    def mean(self, name):
        if self.samples == 0:
            raise ValueError("no sample yet")
        with np.errstate(invalid="ignore", over="ignore"):
            return self.raw(name) / self.weight_sum

    def close(self):
        self.acc = {}


def eddy_flux(means, name):
    """<v'T'> = <vT> - <v> (0.5 (<T>(j-1) + <T>(j))) and its siblings "uT", "uS", "vS", "wT", "wS" from GLOBAL interior means
    (a dict name -> [i, j, k], e.g. {n: handle.mean(n) for n in ("v", "T", "vT")}), at the location and with the dims of the
    velocity.  x wraps periodically; the rows of y faces without a row of cells on both sides -- the southern wall row, and the
    northern wall row -- are 0; so are the lowest and the highest z face of the window (the faces 0 and Nz of the whole column)."""
    if name not in FLUXES:
        raise ValueError(f"eddy_flux of one of {FLUXES}, got {name!r}")
    vel, c, flux = (np.asarray(means[n], np.float64) for n in (name[0], name[1], name))
    out = np.zeros(flux.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        if name[0] == "u":
            out = flux - vel * (0.5 * (np.roll(c, 1, axis=0) + c))
        elif name[0] == "v":
            j = slice(1, min(vel.shape[1], c.shape[1]))      # the rows of faces with a row of cells on both sides
            out[:, j] = flux[:, j] - vel[:, j] * (0.5 * (c[:, j.start - 1:j.stop - 1] + c[:, j]))
        else:
            k = slice(1, c.shape[2])
            out[:, :, k] = flux[:, :, k] - vel[:, :, k] * (0.5 * (c[:, :, :-1] + c[:, :, 1:]))
    return out


def tracer_variance(means, name):
    """<x'x'> = <xx> - <x> <x> for x = "T", "S" (or "u", "v", "eta"), at the field's own points."""
    x = np.asarray(means[name], np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.asarray(means[name + name], np.float64) - x * x


def eddy_kinetic_energy(means):
    """0.25 ((u'u'(i) + u'u'(i+1)) + (v'v'(j) + v'v'(j+1))) at (c,c,c) from GLOBAL interior means of u, v, uu, vv: the kinetic
    energy per cell of include/gb25.h with the variances in place of the squares.  i + 1 wraps periodically; a row of y faces
    the interior does not hold (beyond the last row of cells of a folded grid) counts as 0."""
    uu, vv = tracer_variance(means, "u"), tracer_variance(means, "v")
    Ny = uu.shape[1]
    north = np.zeros(uu.shape)
    rows = min(Ny, vv.shape[1] - 1)
    north[:, :rows] = vv[:, 1:rows + 1]
    with np.errstate(invalid="ignore", over="ignore"):
        return 0.25 * ((uu + np.roll(uu, -1, axis=0)) + (vv[:, :Ny] + north))


def gather_averages(parts, offsets):
    """The results of the ranks of a decomposition (get_average of every rank, [i, j, k]) as the array of the whole: each is
    placed at its offset (i0, j0) in the global interior (a rank below a northern neighbour holds no wall row of v: nothing
    overlaps)."""
    parts = [np.asarray(p) for p in parts]
    nx = max(o[0] + p.shape[0] for p, o in zip(parts, offsets))
    ny = max(o[1] + p.shape[1] for p, o in zip(parts, offsets))
    out = np.zeros((nx, ny, parts[0].shape[2]), parts[0].dtype)
    for p, (i0, j0) in zip(parts, offsets):
        out[i0:i0 + p.shape[0], j0:j0 + p.shape[1]] = p
    return out
