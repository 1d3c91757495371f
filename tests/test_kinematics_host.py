"""Flow kinematics, the parts that need no GPU: the numpy restatement of gb-25_amd/kinematics.py (it is what the device results
are compared with bit for bit in tests/test_gpu_kinematics.py, so it is pinned here independently of the HIP kernels) against a
plain triple-loop statement of the table of include/gb25.h on Python floats, identities between its fp64 pieces, answers known by
hand, the header's enum against the binding and the exported names, and the new ABI entries on a handle without a device.

The triple loop reads the parents and the metrics point by point (metric, metric2(name, i, j), bottom_info) and does one IEEE
operation per Python operator, in the order the header writes; a division by a zero area is never formed (the header selects 0).

The additive identity.  delta + s_n = 2 ax / Az holds in real numbers; in fp64 the two quotients and their sum round three times, so
it is exact only where no rounding can part the sides: with v = 0 both quotients ARE ax / Az and their sum is its exact double,
with u = 0 they are ay / Az and -(ay / Az) and the sum is exactly 0.  Those two are asserted bit for bit on noisy velocities.  With
both components noisy the sides differ by at most the three roundings, |delta| eps / 2 + |s_n| eps / 2 + |delta + s_n| eps / 2 plus
the two roundings of ax +- ay carried through the division, (|ax + ay| + |ax - ay|) eps / (2 |Az|) (1 + eps): the test asserts
that bound, doubled for the second-order terms -- it comes from the format, not from the code."""
import ctypes as C
import functools
import math
import os
import re

import numpy as np
import pytest

import gb25_amd as gb
from gb25_amd import binding
from gb25_amd.derived import vorticity_host
from gb25_amd.kinematics import (CORNER_KINDS, KINEMATICS_NAMES, TRACER_KINDS, cell_gradient, cell_strain, corner_mean, corner_values,
                                 kinematics_host, kinematics_pieces)
from helpers import GRID_NAMES, make_oracle, set_noisy_state_with_halos, set_noisy_velocities

EPS = float(np.finfo(np.float64).eps)
SIZES = {0: (16, 10, 4), 1: (48, 24, 6), 3: (48, 24, 6)}
LAT_LON = (0, 1)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


@functools.lru_cache(maxsize=None)
def noisy_oracle(grid_type, precision="f64"):
    """The baroclinic-instability state with noisy velocities and noise on EVERY cell of the parents, halos included, so that the
    wall rows, the fold's rows and the halo columns hold non-trivial values."""
    Nx, Ny, Nz = SIZES[grid_type]
    m = make_oracle(Nx, Ny, Nz, 600.0, precision=precision, grid_type=GRID_NAMES[grid_type])
    set_noisy_state_with_halos(m, amplitude=0.05)
    return m


def stand_in_density(b):
    """An oracle backend has no get_derived: a potential density that is linear in T and S, rounded to the backend's dtype."""
    T, S = (np.asarray(b.get_field(n, False), np.float64) for n in ("T", "S"))
    return (28.0 - 0.2 * T + 0.8 * (S - 35.0)).astype(b.dtype)


class Loop:
    """The table of include/gb25.h, one point at a time on Python floats."""

    def __init__(self, b, sigma=None):
        self.b, self.H = b, b.H
        self.Nx, self.Ny, self.Nz = b.field_dims("T", False)
        self.latlon = b.cfg.grid_type in LAT_LON
        self.f = {n: np.asarray(b.get_field(n, True), np.float64) for n in ("u", "v", "T", "S")}
        self.sigma = None if sigma is None else np.asarray(sigma, np.float64)
        self.dy = float(b.metric("dy", 1))
        self.rows0 = 0                      # (a single domain: the first row is the global grid's)

    def at(self, name, i, j, k):
        H = self.H
        return float(self.f[name][H + i, H + j, H + k])

    @functools.lru_cache(maxsize=None)
    def m1(self, name, j):
        return float(self.b.metric(name, j + 1))

    @functools.lru_cache(maxsize=None)
    def m2(self, name, i, j):
        return float(self.b.metric2(name, i + 1, j + 1))

    @functools.lru_cache(maxsize=None)
    def kbot(self, i, j):
        i = i % self.Nx                                  # the periodic image
        j = min(max(j, 0), self.Ny - 1)                  # the edge row
        return int(self.b.bottom_info("kbot", i + 1, j + 1))

    def corner(self, i, j, k):
        """(s_s, zeta, f) at corner (i, j)."""
        if self.latlon:
            dy = dyw = self.dy
            dx, dxs, az, f = self.m1("dxc", j), self.m1("dxc", j - 1), self.m1("azf", j), self.m1("fcor", j)
        else:
            dy, dyw, dx, dxs = self.m2("dycf", i, j), self.m2("dycf", i - 1, j), self.m2("dxfc", i, j), self.m2("dxfc", i, j - 1)
            az, f = self.m2("azff", i, j), self.m2("fff", i, j)
        dv = dy * self.at("v", i, j, k) - dyw * self.at("v", i - 1, j, k)
        du = dx * self.at("u", i, j, k) - dxs * self.at("u", i, j - 1, k)
        if az == 0.0:
            return 0.0, 0.0, f
        return (dv + du) / az, (dv - du) / az, f

    def strain(self, i, j, k):
        """(delta, s_n, Az) at cell (i, j)."""
        if self.latlon:
            dyw = dye = self.dy
            dxs, dxn, az = self.m1("dxf", j), self.m1("dxf", j + 1), self.m1("azc", j)
        else:
            dyw, dye, dxs, dxn = self.m2("dyfc", i, j), self.m2("dyfc", i + 1, j), self.m2("dxcf", i, j), self.m2("dxcf", i, j + 1)
            az = self.m2("azcc", i, j)
        ax = dye * self.at("u", i + 1, j, k) - dyw * self.at("u", i, j, k)
        ay = dxn * self.at("v", i, j + 1, k) - dxs * self.at("v", i, j, k)
        if az == 0.0:
            return 0.0, 0.0, az
        return (ax + ay) / az, (ax - ay) / az, az

    def x(self, param, i, j, k):
        if param == 2:
            return float(self.sigma[i % self.Nx, min(max(j, 0), self.Ny - 1), k])
        return self.at("TS"[param], i, j, k)

    def gradient(self, param, i, j, k):
        if self.latlon:
            gxw = gxe = self.m1("dxc", j)
            gys = gyn = self.dy
        else:
            gxw, gxe, gys, gyn = self.m2("dxfc", i, j), self.m2("dxfc", i + 1, j), self.m2("dycf", i, j), self.m2("dycf", i, j + 1)
        wet = lambda a, b: k >= self.kbot(a, b)
        xc = self.x(param, i, j, k)
        dw = (xc - self.x(param, i - 1, j, k)) / gxw if wet(i, j) and wet(i - 1, j) else 0.0
        de = (self.x(param, i + 1, j, k) - xc) / gxe if wet(i, j) and wet(i + 1, j) else 0.0
        ds = (xc - self.x(param, i, j - 1, k)) / gys if j + self.rows0 != 0 and wet(i, j) and wet(i, j - 1) else 0.0
        dn = (self.x(param, i, j + 1, k) - xc) / gyn if j + 1 + self.rows0 != self.b.cfg.Ny and wet(i, j) and wet(i, j + 1) else 0.0
        return 0.5 * (dw + de), 0.5 * (ds + dn)

    def value(self, kind, param, i, j, k):
        if kind in CORNER_KINDS:
            ss, zeta, f = self.corner(i, j, k)
            if kind == "shear_strain":
                return ss
            return 0.0 if f == 0.0 else zeta / f
        if k < self.kbot(i, j):
            return 0.0
        if kind == "gradient":
            gx, gy = self.gradient(param, i, j, k)
            return math.sqrt(gx * gx + gy * gy)
        delta, sn, az = self.strain(i, j, k)
        if kind == "divergence":
            return delta
        if kind == "normal_strain":
            return sn
        if az == 0.0:
            return 0.0
        c = [self.corner(i + a, j + b, k) for b in (0, 1) for a in (0, 1)]          # (i,j), (i+1,j), (i,j+1), (i+1,j+1)
        if kind == "okubo_weiss":
            ms = 0.25 * ((c[0][0] * c[0][0] + c[1][0] * c[1][0]) + (c[2][0] * c[2][0] + c[3][0] * c[3][0]))
            mz = 0.25 * ((c[0][1] * c[0][1] + c[1][1] * c[1][1]) + (c[2][1] * c[2][1] + c[3][1] * c[3][1]))
            return (sn * sn + ms) - mz
        gx, gy = self.gradient(param, i, j, k)
        ms = 0.25 * ((c[0][0] + c[1][0]) + (c[2][0] + c[3][0]))
        return -(((gx * gx) * (0.5 * (delta + sn)) + (gx * gy) * ms) + (gy * gy) * (0.5 * (delta - sn)))

    def field(self, kind, param=0, levels=None):
        bx, by, _ = self.b.field_dims("v" if kind in CORNER_KINDS else "T", False)
        k0, kc = (0, self.Nz) if levels is None else levels
        out = np.zeros((bx, by, kc))
        for k in range(kc):
            for j in range(by):
                for i in range(bx):
                    out[i, j, k] = self.value(kind, param, i, j, k0 + k)
        return out.astype(self.b.dtype)


def requests():
    return [(kind, p) for kind in KINEMATICS_NAMES for p in ((0, 1, 2) if kind in TRACER_KINDS else (0,))]


@pytest.mark.parametrize("grid_type,precision", [(0, "f64"), (0, "f32"), (1, "f64"), (3, "f64")])
def test_the_vectorised_restatement_equals_the_triple_loop(grid_type, precision):
    b = noisy_oracle(grid_type, precision).backend
    Nx, Ny, Nz = SIZES[grid_type]
    sigma = stand_in_density(b)
    loop = Loop(b, sigma)
    if grid_type == 1:
        kbot = np.array([[loop.kbot(i, j) for j in range(Ny)] for i in range(Nx)])
        assert (kbot >= Nz).any() and ((kbot > 0) & (kbot < Nz)).any(), "the islands give dry and partial columns"
    for kind, param in requests():
        want = loop.field(kind, param)
        got = kinematics_host(b, kind, param, sigma=sigma)
        rows = b.field_dims("v" if kind in CORNER_KINDS else "T", False)[1]
        assert got.shape == (Nx, rows, Nz) and got.dtype == b.dtype, kind
        print(f"  grid {grid_type} {precision} {kind}({param}): non-zero {int((want != 0).sum())} of {want.size}, differing "
              f"{int((got != want).sum())}, max |x| {np.abs(want).max():.6g}")
        assert same(got, want), (kind, param)
        assert (want != 0).sum() * 2 > want.size and np.isfinite(want).all(), (kind, param)
        for levels in ((Nz - 1, 1), (1, 2), (1, -1)):
            part = kinematics_host(b, kind, param, levels, sigma=sigma)
            assert same(part, want[:, :, levels[0]:(None if levels[1] == -1 else levels[0] + levels[1])]), (kind, param, levels)


def test_identities_between_the_fp64_pieces():
    m = make_oracle(*SIZES[0], 600.0)
    gb.set_baroclinic_instability(m)
    set_noisy_velocities(m, amplitude=0.05)
    b = m.backend
    b.fill_halo_regions()
    ax, ay, az, delta, sn = cell_strain(b)
    assert same(delta, (ax + ay) / az) and same(sn, (ax - ay) / az) and (ax != 0).all() and (ay != 0).all()
    # both components noisy: the three roundings of the module's docstring
    two = 2.0 * (ax / az)
    bound = EPS * (np.abs(delta) + np.abs(sn) + np.abs(delta + sn) + (np.abs(ax + ay) + np.abs(ax - ay)) / np.abs(az))
    print(f"  delta + s_n against 2 ax / Az: max difference {np.abs((delta + sn) - two).max():.3g}, bound >= {bound.min():.3g}, "
          f"equal bits in {int(((delta + sn) == two).sum())} of {two.size}")
    assert (np.abs((delta + sn) - two) <= bound).all()
    # W from the pieces returned separately
    P = kinematics_pieces(b, "okubo_weiss")
    ss, zeta, _ = corner_values(b, SIZES[0][0] + 1, SIZES[0][1] + 1)
    assert same(P["s_s"], ss) and same(P["zeta"], zeta) and same(P["s_n"], sn)
    W = (sn * sn + corner_mean(ss * ss)) - corner_mean(zeta * zeta)
    assert same(P["value"], W) and same(kinematics_host(b, "okubo_weiss"), W.astype(b.dtype)) and (W > 0).any() and (W < 0).any()
    # v = 0: delta and s_n are the same double, their sum is exactly twice the x-difference term
    v = b.get_field("v", True)
    b.set_field("v", np.zeros_like(v), True)
    ax, ay, az, delta, sn = cell_strain(b)
    assert (ay == 0).all() and same(delta, sn) and same(delta + sn, 2.0 * (ax / az)) and (delta != 0).all()
    # u = 0: s_n = -delta, the sum is exactly 0
    b.set_field("v", v, True)
    b.set_field("u", np.zeros_like(b.get_field("u", True)), True)
    ax, ay, az, delta, sn = cell_strain(b)
    assert (ax == 0).all() and same(sn, -delta) and ((delta + sn) == 0).all() and (delta != 0).all()
    b.close()


@pytest.mark.parametrize("grid_type", [0, 1, 3])
def test_known_answers(grid_type):
    Nx, Ny, Nz = SIZES[grid_type]
    m = make_oracle(Nx, Ny, Nz, 600.0, grid_type=GRID_NAMES[grid_type])
    gb.set_baroclinic_instability(m)
    b = m.backend
    H = b.H
    sigma = stand_in_density(b)
    # u = v = 0: zeros everywhere, whatever the tracers hold
    for name in ("u", "v"):
        b.set_field(name, np.zeros_like(b.get_field(name, True)), True)
    for kind, param in requests():
        assert (kinematics_host(b, kind, param, sigma=sigma) == 0).all() or kind == "gradient", (kind, param)
    assert (kinematics_host(b, "gradient", 0) != 0).any()
    # a uniform T under noisy velocities: |grad T| = 0 and F = 0 exactly
    set_noisy_velocities(m, amplitude=0.05)
    b.fill_halo_regions()
    b.set_field("T", np.full_like(b.get_field("T", True), 7.25), True)
    assert (kinematics_host(b, "gradient", "T") == 0).all() and (kinematics_host(b, "frontogenesis", "T") == 0).all()
    assert (kinematics_host(b, "okubo_weiss") != 0).any()
    # immersed cells are 0 in every quantity at cells
    kbot = np.array([[b.bottom_info("kbot", i, j) for j in range(1, Ny + 1)] for i in range(1, Nx + 1)]).astype(int)
    immersed = np.arange(Nz)[None, None, :] < kbot[:, :, None]
    S = b.get_field("S", True)
    S += 0.01 * np.arange(S.shape[0])[:, None, None] * np.arange(S.shape[1])[None, :, None]
    b.set_field("S", S, True)
    for kind, param in requests():
        if kind not in CORNER_KINDS:
            x = kinematics_host(b, kind, 1 if kind in TRACER_KINDS else 0)
            assert (x[immersed] == 0).all() and (x[~immersed] != 0).any(), kind
    if grid_type != 1:
        assert not immersed.any()
        b.close()
        return
    assert immersed.any() and (~immersed).any()
    # a face next to an island contributes 0: a huge S inside the island changes nothing, and the wet cell east of it has
    # gx = 0.5 (0 + dx(i+1))
    i0, j0, k0 = (int(q) for q in np.argwhere(immersed[:-1] & ~immersed[1:])[0])     # (i0 immersed, i0 + 1 wet at level k0)
    before = {p: kinematics_host(b, "gradient", p, sigma=sigma) for p in (1, 2)}
    gx_before, _ = cell_gradient(b, 1)
    planted = b.get_field("S", True)
    planted[H + i0, H + j0, H + k0] = 1e30
    b.set_field("S", planted, True)
    huge = sigma.copy()
    huge[i0, j0, k0] = 1e30
    assert same(kinematics_host(b, "gradient", 1), before[1]) and same(kinematics_host(b, "gradient", 2, sigma=huge), before[2])
    Sd = np.asarray(planted, np.float64)
    east = (Sd[H + i0 + 2, H + j0, H + k0] - Sd[H + i0 + 1, H + j0, H + k0]) / b.metric("dxc", j0 + 1)
    wet_east = k0 >= kbot[(i0 + 2) % Nx, j0]
    assert gx_before[i0 + 1, j0, k0] == 0.5 * (0.0 + (east if wet_east else 0.0)) and (not wet_east or east != 0)
    b.close()


def test_a_tracer_linear_in_i():
    Nx, Ny, Nz = SIZES[0]
    m = make_oracle(Nx, Ny, Nz, 600.0)
    gb.set_baroclinic_instability(m)
    b = m.backend
    T = b.get_field("T", True)
    slope = 0.375
    T[...] = slope * np.arange(T.shape[0])[:, None, None]
    b.set_field("T", T, True)
    gx, gy = cell_gradient(b, 0)
    dxc = np.array([b.metric("dxc", j) for j in range(1, Ny + 1)])
    assert (gy == 0).all()
    assert same(gx, np.broadcast_to((slope / dxc)[None, :, None], gx.shape).copy())
    assert same(kinematics_host(b, "gradient", "T"), np.broadcast_to(np.abs(slope / dxc)[None, :, None], gx.shape).astype(b.dtype))
    b.close()


@pytest.mark.parametrize("grid_type", [0, 3])
def test_the_rossby_number_is_the_vorticity_over_f(grid_type):
    b = noisy_oracle(grid_type).backend
    bx, by, Nz = b.field_dims("v", False)
    ss, zeta, f = corner_values(b, bx, by)
    assert same(zeta.astype(b.dtype), vorticity_host(b))                   # (the bits of the vorticity before its rounding)
    f = np.broadcast_to(f, zeta.shape)
    ro = kinematics_host(b, "rossby_number")
    with np.errstate(divide="ignore", invalid="ignore"):
        assert same(ro, np.where(f == 0, 0.0, zeta / f).astype(b.dtype)) and (ro != 0).any()

    # where f is 0 the Rossby number is 0: a backend whose Coriolis parameter vanishes on one row of corners
    class NoCoriolisRow:
        def __init__(self, inner):
            self.inner = inner

        def __getattr__(self, name):
            return getattr(self.inner, name)

        def metric(self, name, index=1):
            return 0.0 if name == "fcor" and index == 3 else self.inner.metric(name, index)

        def metric2_array(self, name):
            a = self.inner.metric2_array(name)
            if name == "fff":
                a[:, self.inner.H + 2] = 0.0
            return a

    z = kinematics_host(NoCoriolisRow(b), "rossby_number")
    assert (z[:, 2] == 0).all() and same(np.delete(z, 2, axis=1), np.delete(ro, 2, axis=1)) and (ro[:, 2] != 0).any()


def test_the_enum_the_binding_and_the_public_names():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "gb25.h")).read(), flags=re.S)
    body = re.search(r"typedef enum \{([^}]*)\}\s*gb25_kinematics;", text).group(1)
    names = [s.strip().split()[0] for s in body.split(",") if s.strip()]
    assert names == ["GB25_KIN_DIVERGENCE", "GB25_KIN_NORMAL_STRAIN", "GB25_KIN_SHEAR_STRAIN", "GB25_KIN_OKUBO_WEISS",
                     "GB25_KIN_ROSSBY_NUMBER", "GB25_KIN_GRADIENT", "GB25_KIN_FRONTOGENESIS", "GB25_KIN_COUNT"]
    assert [n.lower() for n in names[:-1]] == ["gb25_kin_" + k for k in binding.KINEMATICS_IDS]
    assert list(binding.KINEMATICS_IDS.values()) == list(range(len(names) - 1)) and tuple(binding.KINEMATICS_IDS) == KINEMATICS_NAMES
    lib = binding.load_library("Float32")
    for symbol in ("gb25_kinematics_dims", "gb25_compute_kinematics", "gb25_get_kinematics", "gb25_get_kinematics_stats"):
        assert symbol in text and hasattr(lib, symbol) and symbol in binding.ABI_SYMBOLS, symbol
    julia = open(os.path.join(root, "julia", "GB25HIP.jl")).read()
    for word in ("KINEMATICS", "kinematics_dims", "compute_kinematics", "get_kinematics", "kinematics_stats", ":gb25_get_kinematics_stats"):
        assert word in julia, word
    for name in ("divergence", "normal_strain", "shear_strain", "okubo_weiss", "rossby_number", "gradient_magnitude", "frontogenesis",
                 "kinematics_host", "kinematics_pieces", "gather_kinematics"):
        assert callable(getattr(gb, name)), name
    for name in ("get_kinematics", "compute_kinematics", "kinematics_stats", "kinematics_dims"):
        assert callable(getattr(binding.HipBackend, name)), name
    from gb25_amd.distributed import LocalSlabEnsemble
    assert callable(LocalSlabEnsemble.kinematics) and callable(gb.Field.gradient_magnitude)


def test_the_public_functions_fall_back_to_the_restatement():
    m = noisy_oracle(0)
    b = m.backend
    sigma = stand_in_density(b)
    for got, want in ((gb.divergence(m), kinematics_host(b, "divergence")),
                      (gb.normal_strain(m, levels=(1, 2)), kinematics_host(b, "normal_strain", None, (1, 2))),
                      (gb.shear_strain(m), kinematics_host(b, "shear_strain")),
                      (gb.okubo_weiss(m), kinematics_host(b, "okubo_weiss")),
                      (gb.rossby_number(m), kinematics_host(b, "rossby_number")),
                      (gb.gradient_magnitude(m, "S"), kinematics_host(b, "gradient", 1)),
                      (m.tracers.T.gradient_magnitude(), kinematics_host(b, "gradient", 0)),
                      (gb.gradient_magnitude(m, "potential_density", sigma=sigma), kinematics_host(b, "gradient", 2, sigma=sigma)),
                      (gb.frontogenesis(m, sigma=sigma), kinematics_host(b, "frontogenesis", 2, sigma=sigma)),
                      (gb.frontogenesis(m, of="T", levels=(0, 1)), kinematics_host(b, "frontogenesis", 0, (0, 1)))):
        assert same(got, want) and (want != 0).any()
    for bad in (lambda: kinematics_host(b, "gradient", 3), lambda: kinematics_host(b, "divergence", 1), lambda: kinematics_host(b, "curl"),
                lambda: m.velocities.u.gradient_magnitude()):
        with pytest.raises(ValueError):
            bad()


def test_the_abi_on_a_handle_without_a_device():
    import torch
    lib = binding.load_library("Float32")
    INVALID, NO_DEVICE = 1, 4
    Nx, Ny, Nz = 48, 24, 6
    cfg = binding.Config()
    lib.gb25_default_config(C.byref(cfg), Nx, Ny, Nz)
    h = C.c_void_p()
    st = lib.gb25_create(C.byref(cfg), C.byref(h))
    assert h and st == (0 if torch.cuda.is_available() else NO_DEVICE)
    d = (C.c_int32 * 3)()
    for q in range(7):
        assert lib.gb25_kinematics_dims(h, q, d) == 0 and tuple(d) == (Nx, Ny + (1 if q in (2, 4) else 0), Nz), q
    assert lib.gb25_kinematics_dims(h, 7, d) == INVALID and lib.gb25_kinematics_dims(h, -1, d) == INVALID
    assert lib.gb25_kinematics_dims(h, 0, None) == INVALID
    host, stats, p = (C.c_float * (Nx * (Ny + 1) * Nz))(), binding.FieldStats(), C.c_void_p()
    bad = [(lambda: lib.gb25_get_kinematics(h, 7, 0, 0, -1, host), b"no kinematics quantity"),
           (lambda: lib.gb25_get_kinematics(h, -1, 0, 0, -1, host), b"no kinematics quantity"),
           (lambda: lib.gb25_get_kinematics(h, 5, 3, 0, -1, host), b"tracer"),
           (lambda: lib.gb25_get_kinematics(h, 6, -1, 0, -1, host), b"tracer"),
           (lambda: lib.gb25_get_kinematics(h, 0, 1, 0, -1, host), b"takes 0"),
           (lambda: lib.gb25_get_kinematics(h, 3, 2, 0, -1, host), b"takes 0"),
           (lambda: lib.gb25_get_kinematics(h, 0, 0, 0, 0, host), b"window"),
           (lambda: lib.gb25_get_kinematics(h, 0, 0, Nz, 1, host), b"window"),
           (lambda: lib.gb25_get_kinematics(h, 2, 0, Nz - 1, 2, host), b"window"),
           (lambda: lib.gb25_get_kinematics(h, 6, 2, -1, 1, host), b"window"),
           (lambda: lib.gb25_get_kinematics(h, 0, 0, 0, -1, None), b"host"),
           (lambda: lib.gb25_compute_kinematics(h, 0, 0, 0, -1, None, d), b"dev"),
           (lambda: lib.gb25_compute_kinematics(h, 3, 0, 3, 9, C.byref(p), d), b"window"),
           (lambda: lib.gb25_get_kinematics_stats(h, 5, 4, C.byref(stats)), b"tracer"),
           (lambda: lib.gb25_get_kinematics_stats(h, 9, 0, C.byref(stats)), b"no kinematics quantity"),
           (lambda: lib.gb25_get_kinematics_stats(h, 0, 0, None), b"out")]
    for n, (call, word) in enumerate(bad):
        assert call() == INVALID, n
        assert word in lib.gb25_last_error_string(h), (n, lib.gb25_last_error_string(h))
    assert lib.gb25_get_kinematics(None, 0, 0, 0, -1, host) == INVALID
    if not torch.cuda.is_available():
        good = [lambda: lib.gb25_get_kinematics(h, 0, 0, 0, -1, host),
                lambda: lib.gb25_get_kinematics(h, 6, 2, 1, 2, host),
                lambda: lib.gb25_get_kinematics(h, 4, 0, Nz - 1, 1, host),
                lambda: lib.gb25_compute_kinematics(h, 3, 0, 0, -1, C.byref(p), d),
                lambda: lib.gb25_compute_kinematics(h, 5, 1, 2, 1, C.byref(p), None),
                lambda: lib.gb25_get_kinematics_stats(h, 3, 0, C.byref(stats)),
                lambda: lib.gb25_get_kinematics_stats(h, 6, 2, C.byref(stats))]
        for n, call in enumerate(good):
            assert call() == NO_DEVICE, n
            assert b"no device" in lib.gb25_last_error_string(h), n
    lib.gb25_destroy(h)
