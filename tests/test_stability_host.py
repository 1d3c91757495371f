"""Stability diagnostics, the parts that need no GPU: the numpy restatement of gb-25_amd/stability.py (it is what the device
results are compared with bit for bit in tests/test_gpu_stability.py, so it is pinned here independently of the HIP kernels)
against answers worked out by hand on columns of dyadic numbers, the rest state, a uniform density, the masking at the bottom and
across immersed neighbours, the header's enum against the binding and the exported names, the fallback of the public functions on
the oracle backend, and the new ABI entries on a handle without a device.

The hand-built columns: centres zc = -40, -24, -16, -4 (dz = 16, 8, 12), g / rho0 = 2^-7, sigma = -z / 8, u = z / 64, v = 0.  Every
difference, product and quotient below is then exact in binary floating point:
    N2 = (-2^-7 (sigma(k) - sigma(k-1))) / dz = (2^-7 dz / 8) / dz = 2^-10         S2 = ((dz / 64) / dz)^2 = 2^-12
    Ri = 2^-10 / 2^-12 = 4         Eady = ((0.31 2^-13) 2^-6) / 2^-5 = 0.31 2^-14 with fc = 2^-13
    c1 = (2^-5 16 + 2^-5 8 + 2^-5 12) / pi = 1.125 / pi, one division"""
import ctypes as C
import os
import re

import numpy as np

import gb25_amd as gb
from gb25_amd import binding
from gb25_amd.derived import vorticity_host
from gb25_amd.stability import (PI, STABILITY_NAMES, coriolis_at_cells, deformation_radius_of, pad_ring, stability_host,
                                stability_of_columns, vorticity_corners_host)
from helpers import counter_rng, make_oracle, set_noisy_velocities

ZC = np.array([-40.0, -24.0, -16.0, -4.0])
GR = 2.0 ** -7
FACE_KINDS = STABILITY_NAMES[:-1]


def columns(Nx, Ny, kbot=None):
    """The hand-built columns of the module's docstring as the arguments of stability_of_columns."""
    Nz = ZC.size
    sigma = np.broadcast_to(-ZC / 8.0, (Nx, Ny, Nz)).copy()
    u = np.broadcast_to(ZC / 64.0, (Nx + 1, Ny, Nz)).copy()
    v = np.zeros((Nx, Ny + 1, Nz))
    kbot = np.zeros((Nx, Ny), int) if kbot is None else kbot
    wall = np.zeros(Ny + 1, bool)
    wall[0] = wall[Ny] = True
    extra = dict(g_over_rho0=GR, fc=np.full((Nx, Ny), 2.0 ** -13), zeta=np.zeros((Nx + 1, Ny + 1, Nz)), dx=np.full((Nx + 1, Ny), 8.0),
                 dy=np.full((Nx, Ny + 1), 4.0), wall_y=wall)
    return sigma, u, v, kbot, extra


def run(kind, sigma, u, v, kbot, extra, param=None, levels=None):
    return stability_of_columns(kind, ZC, pad_ring(kbot), pad_ring(sigma), u, v, param=param, levels=levels, **extra)


def test_known_answers_on_dyadic_columns():
    Nx, Ny, Nz = 5, 4, ZC.size
    sigma, u, v, kbot, extra = columns(Nx, Ny)
    inner = slice(1, Nz)          # the interior faces
    for kind, want in (("n2", 2.0 ** -10), ("shear2", 2.0 ** -12), ("richardson", 4.0), ("eady_rate", 0.31 * 2.0 ** -14)):
        got = run(kind, sigma, u, v, kbot, extra)
        assert got.shape == (Nx, Ny, Nz + 1) and got.dtype == np.float64
        assert (got[:, :, inner] == want).all(), kind
        assert (got[:, :, 0] == 0).all() and (got[:, :, Nz] == 0).all(), kind
    c1 = run("wave_speed", sigma, u, v, kbot, extra)
    assert c1.shape == (Nx, Ny, 1) and (c1 == (2.0 ** -5 * 16.0 + 2.0 ** -5 * 8.0 + 2.0 ** -5 * 12.0) / PI).all()
    assert 1.125 / PI == float(c1[0, 0, 0])
    # the floors: a shear floor above S2 replaces it, an N2 floor at N2 switches the Eady rate off (the comparison is strict)
    assert (run("richardson", sigma, u, v, kbot, extra, param=2.0 ** -11)[:, :, inner] == 2.0).all()
    assert (run("eady_rate", sigma, u, v, kbot, extra, param=2.0 ** -10)[:, :, inner] == 0).all()
    assert (run("eady_rate", sigma, u, v, kbot, extra, param=2.0 ** -11)[:, :, inner] == 0.31 * 2.0 ** -14).all()
    # the potential vorticity with a density that also rises northward, sigma += j / 2: b = -2^-7 sigma, gy = -2^-8 / 4 = -2^-10
    # across every open y face, 0 across the two walls; no vorticity: q = fc N2 + du by, du = 2^-6
    tilted = sigma + 0.5 * np.arange(Ny)[None, :, None]
    got = run("ertel_pv", tilted, u, v, kbot, extra)
    by = np.full(Ny, -2.0 ** -10)
    by[0] = by[Ny - 1] = 0.25 * ((0.0 + -2.0 ** -10) + (0.0 + -2.0 ** -10))
    want = 2.0 ** -13 * 2.0 ** -10 + 2.0 ** -6 * by
    assert (got[:, :, inner] == want[None, :, None]).all()
    # ... with a uniform vorticity z at the corners: zb = z, q = (fc + z) N2 + du by
    extra["zeta"][...] = 2.0 ** -14
    assert (run("ertel_pv", tilted, u, v, kbot, extra)[:, :, inner] == ((2.0 ** -13 + 2.0 ** -14) * 2.0 ** -10 + 2.0 ** -6 * by)[None, :, None]).all()
    # ... and a density that rises eastward instead, with v = z / 32: gx = -2^-8 / 8 except across the seam of the periodic image
    east = sigma + 0.5 * np.arange(Nx)[:, None, None]
    v2 = np.broadcast_to(ZC / 32.0, v.shape)
    extra["zeta"][...] = 0.0
    got = run("ertel_pv", east, u, v2, kbot, extra)
    assert (got[1:Nx - 1, :, inner] == 2.0 ** -13 * 2.0 ** -10 + (2.0 ** -6 * 0.0 - 2.0 ** -5 * -2.0 ** -11)).all()
    # windows of faces are the same numbers
    whole = run("ertel_pv", tilted, u, v, kbot, extra)
    for k_first, k_count in ((0, 1), (Nz, 1), (1, 2), (2, -1)):
        part = run("ertel_pv", tilted, u, v, kbot, extra, levels=(k_first, k_count))
        assert np.array_equal(part, whole[:, :, k_first:(None if k_count == -1 else k_first + k_count)])


def test_the_rest_state():
    Nx, Ny, Nz = 6, 5, ZC.size
    _, u, v, kbot, extra = columns(Nx, Ny)
    sigma = 20.0 + 8.0 * counter_rng((Nx, Ny, Nz), 3, 1)
    extra["fc"] = 1e-4 * (counter_rng((Nx, Ny), 3, 2) - 0.5)
    u[...] = 0.0
    n2 = run("n2", sigma, u, v, kbot, extra)
    assert (n2 != 0).any() and (n2 < 0).any() and (n2 > 0).any()
    assert (run("shear2", sigma, u, v, kbot, extra) == 0).all()
    assert (run("eady_rate", sigma, u, v, kbot, extra) == 0).all()
    assert np.array_equal(run("richardson", sigma, u, v, kbot, extra, param=2.5e-7), n2 / 2.5e-7)
    assert np.array_equal(run("ertel_pv", sigma, u, v, kbot, extra), extra["fc"][:, :, None] * n2)


def test_a_uniform_density():
    Nx, Ny, Nz = 6, 5, ZC.size
    sigma, u, v, kbot, extra = columns(Nx, Ny)
    sigma[...] = 27.25
    u += 0.01 * counter_rng(u.shape, 5, 1)
    v += 0.01 * counter_rng(v.shape, 5, 2)
    extra["zeta"] = 1e-5 * counter_rng(extra["zeta"].shape, 5, 3)
    assert (run("n2", sigma, u, v, kbot, extra) == 0).all()
    assert (run("ertel_pv", sigma, u, v, kbot, extra) == 0).all()
    assert (run("wave_speed", sigma, u, v, kbot, extra) == 0).all()
    assert (run("shear2", sigma, u, v, kbot, extra)[:, :, 1:Nz] > 0).all()


def test_masking_at_the_bottom_and_across_immersed_neighbours():
    Nx, Ny, Nz = 7, 6, ZC.size
    kbot = np.zeros((Nx, Ny), int)
    kbot[2, 2], kbot[3, 2], kbot[4, 3], kbot[0, 1] = 1, 2, 3, 2
    kbot[5, 4] = Nz                     # a dry column
    sigma, u, v, _, extra = columns(Nx, Ny, kbot)
    sigma += 0.5 * counter_rng(sigma.shape, 9, 1)
    u += 0.01 * counter_rng(u.shape, 9, 2)
    v += 0.01 * counter_rng(v.shape, 9, 3)
    extra["zeta"] = 1e-5 * counter_rng(extra["zeta"].shape, 9, 4)
    immersed = np.arange(Nz)[None, None, :] < kbot[:, :, None]
    planted = np.where(immersed, 1e30, sigma)       # a huge density in every immersed cell
    faces = np.arange(Nz + 1)[None, None, :]
    zero = (faces <= kbot[:, :, None]) | (faces == 0) | (faces == Nz)
    for kind in FACE_KINDS:
        got = run(kind, sigma, u, v, kbot, extra)
        assert (got[zero] == 0).all() and (got[5, 4] == 0).all(), kind
        assert (got[~zero] != 0).all() and np.isfinite(got).all(), kind
        assert np.array_equal(run(kind, planted, u, v, kbot, extra), got), kind
    c1 = run("wave_speed", sigma, u, v, kbot, extra)
    assert c1[5, 4, 0] == 0 and c1[4, 3, 0] == 0 and c1[3, 2, 0] > 0      # dry; one wet level: no interior face; two wet levels
    assert np.array_equal(run("wave_speed", planted, u, v, kbot, extra), c1)
    # the gradient across an OPEN face does see its neighbour: the same plant in a wet cell changes the columns beside it
    wet_plant = sigma.copy()
    wet_plant[3, 4, 2] = 1e30
    changed = (run("ertel_pv", wet_plant, u, v, kbot, extra) != run("ertel_pv", sigma, u, v, kbot, extra)).any(axis=2)
    want = np.zeros((Nx, Ny), bool)
    for i, j in ((3, 4), (2, 4), (4, 4), (3, 3), (3, 5)):
        want[i, j] = True
    assert np.array_equal(changed, want)


def test_the_enum_the_binding_and_the_public_names():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "gb25.h")).read(), flags=re.S)
    body = re.search(r"typedef enum \{([^}]*)\}\s*gb25_stability;", text).group(1)
    names = [s.strip().split()[0] for s in body.split(",") if s.strip()]
    assert names == ["GB25_ST_N2", "GB25_ST_SHEAR2", "GB25_ST_RICHARDSON", "GB25_ST_EADY_RATE", "GB25_ST_ERTEL_PV", "GB25_ST_WAVE_SPEED",
                     "GB25_ST_COUNT"]
    assert [n.lower() for n in names[:-1]] == ["gb25_st_" + k for k in binding.STABILITY_IDS]
    assert list(binding.STABILITY_IDS.values()) == list(range(len(names) - 1)) and tuple(binding.STABILITY_IDS) == STABILITY_NAMES
    lib = binding.load_library("Float32")
    for symbol in ("gb25_stability_dims", "gb25_compute_stability", "gb25_get_stability", "gb25_get_stability_stats"):
        assert symbol in text and hasattr(lib, symbol), symbol
    for name in ("buoyancy_frequency", "shear_squared", "richardson_number", "eady_growth_rate", "ertel_pv", "baroclinic_wave_speed",
                 "deformation_radius", "eddy_resolution", "stability_host", "stability_of_columns", "gather_stability"):
        assert callable(getattr(gb, name)), name
    for name in ("get_stability", "compute_stability", "stability_stats", "stability_dims"):
        assert callable(getattr(binding.HipBackend, name)), name
    from gb25_amd.distributed import LocalSlabEnsemble
    assert callable(LocalSlabEnsemble.stability)


def test_the_public_functions_fall_back_to_the_restatement():
    m = make_oracle(16, 8, 4, 600.0)
    gb.set_baroclinic_instability(m)
    set_noisy_velocities(m, amplitude=0.05)
    b = m.backend
    Nx, Ny, Nz = b.field_dims("T", False)
    # the corners' vorticity is the derived field's where that has the corner
    corners = vorticity_corners_host(b)
    assert corners.shape == (Nx + 1, Ny + 1, Nz) and np.array_equal(corners[:Nx], vorticity_host(b))
    # the potential density handed in (an oracle backend has no get_derived): a stand-in that is linear in T
    sigma = (28.0 - 0.2 * np.asarray(b.get_field("T", False), np.float64)).astype(b.dtype)
    given = dict(sigma=sigma)
    n2 = gb.buoyancy_frequency(m, **given)
    assert n2.shape == (Nx, Ny, Nz + 1) and n2.dtype == b.dtype and (n2[:, :, 1:Nz] > 0).all()
    assert np.array_equal(n2, stability_host(b, "n2", sigma=sigma))
    assert np.array_equal(gb.buoyancy_frequency(m, levels=(2, 2), **given), n2[:, :, 2:4])
    s2 = gb.shear_squared(m)
    assert np.array_equal(s2, stability_host(b, "shear2")) and (s2[:, :, 1:Nz] > 0).all()
    assert np.array_equal(gb.richardson_number(m, **given), stability_host(b, "richardson", 1e-12, sigma=sigma))
    assert np.array_equal(gb.richardson_number(m, 1.0, **given), n2)           # (a floor above every S2: Ri = N2 / 1)
    eady = gb.eady_growth_rate(m, **given)
    assert np.array_equal(eady, stability_host(b, "eady_rate", 0.0, sigma=sigma)) and (eady[:, :, 1:Nz] > 0).all()
    pv = gb.ertel_pv(m, **given)
    assert np.array_equal(pv, stability_host(b, "ertel_pv", sigma=sigma, vorticity=corners)) and (pv[:, :, 1:Nz] != 0).all()
    assert np.array_equal(gb.ertel_pv(m, vorticity=np.zeros_like(corners), **given),
                          stability_host(b, "ertel_pv", sigma=sigma, vorticity=np.zeros_like(corners)))
    fc = coriolis_at_cells(b)
    assert fc.shape == (Nx, Ny) and (fc[:, :Ny // 2] < 0).all() and (fc[:, Ny // 2:] > 0).all()
    c1 = gb.baroclinic_wave_speed(m, **given)
    assert c1.shape == (Nx, Ny) and np.array_equal(c1, stability_host(b, "wave_speed", sigma=sigma)[:, :, 0]) and (c1 > 0).all()
    # the deformation radius and the resolution: host arithmetic on c1
    Ld = gb.deformation_radius(m, **given)
    lat = np.array([b.metric("phic", j) for j in range(1, Ny + 1)])
    f = 2.0 * b.cfg.Omega * np.sin(np.deg2rad(lat))
    assert np.abs(lat).min() >= 5.0 and np.allclose(Ld, np.asarray(c1, np.float64) / np.abs(f)[None, :], rtol=1e-14)
    band = deformation_radius_of([2.0, 2.0], [0.0, 60.0], 7.292115e-5, 6371e3)
    assert np.isclose(band[0], np.sqrt(2.0 / (2.0 * 2.0 * 7.292115e-5 / 6371e3))) and np.isclose(band[1], 2.0 / (2.0 * 7.292115e-5 * np.sin(np.pi / 3)))
    res = gb.eddy_resolution(m, **given)
    assert res.shape == (Nx, Ny) and (res > 0).all() and (res < Ld).all()
    b.close()


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
    for q in range(6):
        assert lib.gb25_stability_dims(h, q, d) == 0 and tuple(d) == (Nx, Ny, 1 if q == 5 else Nz + 1), q
    assert lib.gb25_stability_dims(h, 6, d) == INVALID and lib.gb25_stability_dims(h, -1, d) == INVALID
    host, stats, p = (C.c_float * (Nx * Ny * (Nz + 1)))(), binding.FieldStats(), C.c_void_p()
    bad = [(lambda: lib.gb25_get_stability(h, 6, 0.0, 0, -1, host), b"no stability diagnostic"),
           (lambda: lib.gb25_get_stability(h, -1, 0.0, 0, -1, host), b"no stability diagnostic"),
           (lambda: lib.gb25_get_stability(h, 0, 0.0, 0, 0, host), b"window"),
           (lambda: lib.gb25_get_stability(h, 0, 0.0, Nz + 1, 1, host), b"window"),
           (lambda: lib.gb25_get_stability(h, 0, 0.0, Nz, 2, host), b"window"),
           (lambda: lib.gb25_get_stability(h, 0, 0.0, -1, 1, host), b"window"),
           (lambda: lib.gb25_get_stability(h, 5, 0.0, 0, 2, host), b"window"),
           (lambda: lib.gb25_get_stability(h, 5, 0.0, 1, 1, host), b"window"),
           (lambda: lib.gb25_get_stability(h, 2, 0.0, 0, -1, host), b"Richardson"),
           (lambda: lib.gb25_get_stability(h, 2, -1.0, 0, -1, host), b"Richardson"),
           (lambda: lib.gb25_get_stability(h, 2, float("nan"), 0, -1, host), b"Richardson"),
           (lambda: lib.gb25_get_stability(h, 3, -1e-9, 0, -1, host), b"Eady"),
           (lambda: lib.gb25_get_stability(h, 0, 0.0, 0, -1, None), b"host"),
           (lambda: lib.gb25_compute_stability(h, 0, 0.0, 0, -1, None, d), b"dev"),
           (lambda: lib.gb25_compute_stability(h, 4, 0.0, 3, 9, C.byref(p), d), b"window"),
           (lambda: lib.gb25_get_stability_stats(h, 2, 0.0, C.byref(stats)), b"Richardson"),
           (lambda: lib.gb25_get_stability_stats(h, 7, 0.0, C.byref(stats)), b"no stability diagnostic"),
           (lambda: lib.gb25_get_stability_stats(h, 0, 0.0, None), b"out")]
    for n, (call, word) in enumerate(bad):
        assert call() == INVALID, n
        assert word in lib.gb25_last_error_string(h), (n, lib.gb25_last_error_string(h))
    assert lib.gb25_get_stability(None, 0, 0.0, 0, -1, host) == INVALID
    if not torch.cuda.is_available():
        good = [lambda: lib.gb25_get_stability(h, 0, 0.0, 0, -1, host),
                lambda: lib.gb25_get_stability(h, 2, 1e-12, 1, 2, host),
                lambda: lib.gb25_get_stability(h, 3, 0.0, Nz, 1, host),
                lambda: lib.gb25_get_stability(h, 5, 0.0, 0, 1, host),
                lambda: lib.gb25_compute_stability(h, 4, 0.0, 0, -1, C.byref(p), d),
                lambda: lib.gb25_compute_stability(h, 1, 0.0, 2, 1, C.byref(p), None),
                lambda: lib.gb25_get_stability_stats(h, 4, 0.0, C.byref(stats)),
                lambda: lib.gb25_get_stability_stats(h, 5, 0.0, C.byref(stats))]
        for n, call in enumerate(good):
            assert call() == NO_DEVICE, n
            assert b"no device" in lib.gb25_last_error_string(h), n
    lib.gb25_destroy(h)
