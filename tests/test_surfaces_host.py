"""Fields on surfaces, the parts that need no GPU: the numpy restatement of gb-25_amd/surfaces.py (it is what the device results
are compared with bit for bit in tests/test_gpu_surfaces.py, so it is pinned here independently of the HIP kernel) against a
column-by-column loop written out below, known answers, independence of the targets, the layers' sum, a stepped oracle model,
and the new ABI entries' argument checks on a handle without a device.

Layers: with edges that bracket the whole profile the first surface outcrops (depth = -zf(Nz)) and the last is grounded (depth =
-zf(kb)), so the n - 1 differences telescope to the column's depth D = -zf(kb) + zf(Nz); each difference is one rounding of
numbers no larger than D and the sum of n - 1 of them adds n - 2 more: within (n + 2) eps(Float64) D."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

import gb25_amd as gb
from gb25_amd import binding
from gb25_amd.surfaces import (DRY, FOUND, GROUNDED, OUTCROP, layer_thickness, on_surfaces_host, surfaces_of_profiles)
from helpers import counter_rng, make_oracle, set_noisy_velocities

EPS = float(np.finfo(np.float64).eps)


def column_loop(q, f, zc, zf, kb, c):
    """The definition of include/gb25.h for ONE column and ONE value, in plain Python floats: (result, status)."""
    Nz = len(q)
    if kb >= Nz:
        return 0.0, DRY
    for k in range(Nz - 2, kb - 1, -1):
        qa, qb = float(q[k + 1]), float(q[k])
        if not (math.isfinite(qa) and math.isfinite(qb)):
            continue
        if (qa <= c <= qb) or (qb <= c <= qa):
            frac = 0.0 if qa == qb else (c - qa) / (qb - qa)
            g = 1.0 - frac
            if f is None:
                return -(float(zc[k + 1]) * g + float(zc[k]) * frac), FOUND
            return float(f[k + 1]) * g + float(f[k]) * frac, FOUND
    down = float(q[kb]) >= float(q[Nz - 1])
    if (c > float(q[Nz - 1])) == down:
        return (-float(zf[kb]) if f is None else float(f[kb])), GROUNDED
    return (-float(zf[Nz]) if f is None else float(f[Nz - 1])), OUTCROP


def grid_of(Nz, seed):
    """Faces zf[0 .. Nz] from -depth up to 0 with uneven spacing, centres zc."""
    dz = 10.0 + 90.0 * counter_rng((Nz,), seed, 11)
    zf = np.concatenate([[0.0], np.cumsum(dz)])
    zf = zf - zf[-1]
    return 0.5 * (zf[:-1] + zf[1:]), zf


def same_bits(a, b):
    return a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


@pytest.mark.parametrize("Nz", [5, 6, 7, 8])
def test_profiles_against_a_column_by_column_loop(Nz):
    Nx, Ny = 9, Nz + 1
    zc, zf = grid_of(Nz, Nz)
    u = counter_rng((Nx, Ny, Nz), Nz, 1)
    q = np.empty((Nx, Ny, Nz))
    q[0:3] = np.cumsum(u[0:3], axis=2)[:, :, ::-1]            # monotone, decreasing upward (a stable density)
    q[3:5] = np.cumsum(u[3:5], axis=2)                        # monotone, increasing upward (a temperature)
    q[5:7] = 4.0 * u[5:7]                                     # not monotone
    q[7] = np.round(3.0 * u[7])                               # equal neighbours
    q[8] = 4.0 * u[8]
    q[8, :, 2] = np.nan                                       # a NaN level
    q[8, 0, :] = np.nan
    q[6, 1, 1] = np.inf
    f = 10.0 * counter_rng((Nx, Ny, Nz), Nz, 2) - 5.0
    kbot = np.broadcast_to(np.arange(Ny)[None, :], (Nx, Ny)).copy()   # 0 .. Nz: row Nz is dry
    finite = q[np.isfinite(q)]
    values = np.concatenate([np.quantile(finite, [0.1, 0.35, 0.5, 0.8]), [finite.min() - 1.0, finite.max() + 1.0, q[7, 0, 1], 1.0]])
    seen = set()
    for carried in (None, f):
        got, status = surfaces_of_profiles(q, carried, zc, zf, kbot, values)
        assert got.shape == status.shape == (Nx, Ny, len(values)) and got.dtype == np.float64 and status.dtype == np.uint8
        for i, j, n in itertools.product(range(Nx), range(Ny), range(len(values))):
            want, st = column_loop(q[i, j], None if carried is None else carried[i, j], zc, zf, kbot[i, j], float(values[n]))
            assert status[i, j, n] == st, (i, j, n)
            assert np.array([got[i, j, n]]).tobytes() == np.array([want]).tobytes(), (i, j, n, got[i, j, n], want)
            seen.add(st)
    assert seen == {FOUND, OUTCROP, GROUNDED, DRY}


def test_a_profile_linear_in_zc_gives_the_exact_depth():
    Nz = 8
    zf = -np.array([2048.0, 1024.0, 512.0, 256.0, 128.0, 64.0, 32.0, 16.0, 0.0])
    zc = 0.5 * (zf[:-1] + zf[1:])
    q = (1.0 - zc / 64.0)[None, None, :]                       # exact in fp64: powers of two
    depths = np.array([10.0, 24.0, 30.0, 36.0, 72.0, 120.0, 672.0, 1536.0])   # (fractions of a pair that fp64 holds exactly)
    got, status = surfaces_of_profiles(q, None, zc, zf, np.zeros((1, 1), int), 1.0 + depths / 64.0)
    assert (status == FOUND).all() and np.array_equal(got[0, 0], depths)
    # the carried quantity linear in z as well: its value at that depth
    got, _ = surfaces_of_profiles(q, (3.0 * zc)[None, None, :], zc, zf, np.zeros((1, 1), int), 1.0 + depths / 64.0)
    assert np.array_equal(got[0, 0], -3.0 * depths)


def test_a_slice_at_a_level_centre_returns_that_level_bit_for_bit():
    Nz = 7
    zc, zf = grid_of(Nz, 3)
    f = (counter_rng((4, 3, Nz), 5, 1) * 30.0 - 2.0).astype(np.float32).astype(np.float64)
    kbot = np.array([[0, 1, 2], [3, 4, 5], [6, 7, 0], [0, 0, 3]])
    got, status = surfaces_of_profiles(np.broadcast_to(-zc, f.shape), f, zc, zf, kbot, -zc)
    for k in range(Nz):
        wet = kbot <= k
        assert same_bits(got[:, :, k][wet], f[:, :, k][wet]), k
        # (a column of ONE wet level has no pair to cross: its only level is handed out as an outcrop)
        assert (status[:, :, k][wet] == np.where(kbot[wet] == Nz - 1, OUTCROP, FOUND)).all(), k
        # a level below the column's bottom: grounded, the value of the first wet level; dry columns give DRY and 0
        below = (kbot > k) & (kbot < Nz)
        ii, jj = np.nonzero(below)
        assert (status[:, :, k][below] == GROUNDED).all() and np.array_equal(got[ii, jj, k], f[ii, jj, kbot[ii, jj]])
    assert (status[kbot >= Nz] == DRY).all() and (got[kbot >= Nz] == 0).all() and (kbot >= Nz).any()


def test_the_extreme_targets_outcrop_above_and_ground_below():
    Nz = 6
    zc, zf = grid_of(Nz, 9)
    sigma = np.array([27.5, 27.0, 26.0, 25.5, 25.0, 24.0])     # denser downward
    theta = sigma[::-1].copy()                                  # warmer upward
    f = np.arange(Nz) + 100.0
    kbot = np.array([[0, 2, Nz]])
    for q, light, heavy in ((sigma, 20.0, 30.0), (theta, 30.0, 20.0)):
        cols = np.broadcast_to(q, (1, 3, Nz))
        for carried in (None, np.broadcast_to(f, (1, 3, Nz))):
            got, status = surfaces_of_profiles(cols, carried, zc, zf, kbot, [light, heavy])
            assert status[0, :2, 0].tolist() == [OUTCROP, OUTCROP] and status[0, :2, 1].tolist() == [GROUNDED, GROUNDED]
            assert status[0, 2].tolist() == [DRY, DRY] and got[0, 2].tolist() == [0.0, 0.0]
            if carried is None:
                assert got[0, :2, 0].tolist() == [-zf[Nz], -zf[Nz]] and got[0, :2, 1].tolist() == [-zf[0], -zf[2]]
            else:
                assert got[0, :2, 0].tolist() == [f[Nz - 1], f[Nz - 1]] and got[0, :2, 1].tolist() == [f[0], f[2]]
    # a column of one wet level has no pair: everything outcrops or is grounded
    got, status = surfaces_of_profiles(sigma[None, None, :], None, zc, zf, np.array([[Nz - 1]]), [20.0, 24.0, 30.0])
    assert status[0, 0].tolist() == [OUTCROP, OUTCROP, GROUNDED] and got[0, 0].tolist() == [-zf[Nz], -zf[Nz], -zf[Nz - 1]]


def test_a_value_does_not_depend_on_the_other_values():
    Nz = 8
    zc, zf = grid_of(Nz, 2)
    q = 4.0 * counter_rng((6, 5, Nz), 21, 1)
    f = counter_rng((6, 5, Nz), 21, 2)
    kbot = (counter_rng((6, 5), 21, 3) * (Nz + 1)).astype(int)
    values = np.concatenate([np.quantile(q, np.linspace(0.02, 0.98, 11)), [-1.0, 5.0]])
    whole, wstatus = surfaces_of_profiles(q, f, zc, zf, kbot, values)
    for trial in range(4):
        order = np.argsort(counter_rng((len(values),), trial, 7))
        sub = order[:len(values) - 3 * trial]
        got, status = surfaces_of_profiles(q, f, zc, zf, kbot, values[sub])
        assert same_bits(got, whole[:, :, sub]) and same_bits(status, wstatus[:, :, sub]), trial
    for n in range(len(values)):
        got, status = surfaces_of_profiles(q, f, zc, zf, kbot, values[n:n + 1])
        assert same_bits(got, whole[:, :, n:n + 1]) and same_bits(status, wstatus[:, :, n:n + 1]), n


def test_layers_that_bracket_the_profile_sum_to_the_column_depth():
    Nz = 8
    zc, zf = grid_of(Nz, 4)
    q = np.cumsum(counter_rng((7, 6, Nz), 31, 1), axis=2)[:, :, ::-1] + 20.0
    kbot = (counter_rng((7, 6), 31, 3) * Nz).astype(int)       # every column wet
    for n in (2, 3, 9, 33):
        edges = np.linspace(q.min() - 1.0, q.max() + 1.0, n)
        depth, status = surfaces_of_profiles(q, None, zc, zf, kbot, edges)
        assert (status[:, :, 0] == OUTCROP).all() and (status[:, :, -1] == GROUNDED).all()
        h = layer_thickness(depth)
        assert h.shape == (7, 6, n - 1) and (h >= 0).all()
        D = -zf[kbot] + zf[Nz]
        err = np.abs(h.sum(axis=2) - D)
        print(f"  {n} edges: worst |sum h - D| / (eps D) = {(err / (EPS * D)).max():.2f}, bound {n + 2}")
        assert (err <= (n + 2) * EPS * D).all(), n


def test_the_values_are_checked():
    zc, zf = grid_of(5, 1)
    q = np.zeros((1, 1, 5))
    for bad in ([], np.zeros(65), [1.0, np.inf], [np.nan]):
        with pytest.raises(ValueError, match="values"):
            surfaces_of_profiles(q, None, zc, zf, np.zeros((1, 1), int), bad)
    m = make_oracle(16, 8, 4, 600.0)
    with pytest.raises(ValueError, match="variable"):
        on_surfaces_host(m.backend, "w", "T", [1.0])
    with pytest.raises(ValueError, match="carried"):
        on_surfaces_host(m.backend, "T", "w", [1.0])


@pytest.mark.parametrize("grid_type", ["simple_lat_lon", "gaussian_islands_lat_lon"])
def test_on_surfaces_host_on_a_stepped_oracle_model(grid_type):
    Nx, Ny, Nz = (24, 12, 6) if grid_type == "simple_lat_lon" else (48, 24, 6)   # (the islands need 48 columns for a dry one)
    m = make_oracle(Nx, Ny, Nz, 600.0, grid_type=grid_type)
    gb.set_baroclinic_instability(m)
    set_noisy_velocities(m)
    gb.first_time_step(m)
    gb.loop(m, 2)
    b = m.backend
    T, S = (np.asarray(b.get_field(n, False), np.float64) for n in ("T", "S"))
    zc = np.array([b.metric("zc", k) for k in range(1, Nz + 1)])
    zf = np.array([b.metric("zf", k) for k in range(1, Nz + 2)])
    kbot = np.array([[b.bottom_info("kbot", i, j) for j in range(1, Ny + 1)] for i in range(1, Nx + 1)]).astype(int)
    wet = kbot < Nz
    if grid_type != "simple_lat_lon":
        assert (~wet).any() and ((kbot > 0) & wet).any()
    # isotherms and isohalines: the depth lies between the faces of the column, T on its own isotherm is the isotherm
    for name, x in (("T", T), ("S", S)):
        values = np.quantile(x[wet], [0.2, 0.5, 0.8])
        depth, status = on_surfaces_host(b, name, "depth", values)
        assert depth.shape == status.shape == (Nx, Ny, 3) and depth.dtype == b.dtype and status.dtype == np.uint8
        assert (status[~wet] == DRY).all() and (status[wet] != DRY).all() and (status == FOUND).any()
        assert (depth[wet] >= 0).all() and (depth[wet] <= -zf[kbot[wet]][:, None]).all()
        on_itself, st2 = on_surfaces_host(b, name, name, values)
        assert np.array_equal(st2, status)
        hit = status == FOUND
        want = np.broadcast_to(values, hit.shape)[hit]
        assert np.abs(on_itself[hit] - want).max() <= 4 * EPS * np.abs(x).max()
        other, _ = on_surfaces_host(b, name, "S" if name == "T" else "T", values)
        assert np.isfinite(other).all()
    # depth slices: every level's centre returns the level, 300 m lies between its neighbours
    for name, x in (("T", T), ("S", S)):
        got, status = on_surfaces_host(b, "depth", name, -zc)
        for k in range(Nz):
            ok = kbot <= k
            assert same_bits(got[:, :, k][ok], x[:, :, k][ok].astype(b.dtype)), (name, k)
            assert (status[:, :, k][ok] == np.where(kbot[ok] == Nz - 1, OUTCROP, FOUND)).all(), (name, k)
        between = -0.5 * (zc[2] + zc[3])                        # a depth that is no model level
        got, status = gb.at_depths(m, name, [between])         # (the public function falls back to the restatement)
        k = 3
        lo, hi = np.minimum(x[:, :, k - 1], x[:, :, k]), np.maximum(x[:, :, k - 1], x[:, :, k])
        ok = status[:, :, 0] == FOUND
        assert ok.any() and ((got[:, :, 0] >= lo) & (got[:, :, 0] <= hi))[ok].all()
        assert same_bits(getattr(m.tracers, name).at_depths([between])[0], got)
    mid = 0.5 * (T[Nx // 2, Ny // 2, 2] + T[Nx // 2, Ny // 2, 3])        # crossed by that column at the least
    assert kbot[Nx // 2, Ny // 2] <= 2
    ke, status = on_surfaces_host(b, "T", "kinetic_energy", [mid])
    assert (ke[status == FOUND] > 0).all() and (status == FOUND).any()
    # the potential density handed in (an oracle backend has no get_derived): here a stand-in that is linear in T
    sigma = 28.0 - 0.2 * T
    d1, s1 = on_surfaces_host(b, "potential_density", "depth", [28.0 - 0.2 * float(np.median(T[wet]))], sigma=sigma)
    d2, s2 = surfaces_of_profiles(sigma, None, zc, zf, kbot, [28.0 - 0.2 * float(np.median(T[wet]))])
    assert same_bits(d1, d2.astype(b.dtype)) and same_bits(s1, s2)
    # the public functions on a backend without the kernel
    depth, status = gb.isosurface_depth(m, "T", np.quantile(T[wet], [0.2, 0.8]))
    assert same_bits(depth, on_surfaces_host(b, "T", "depth", np.quantile(T[wet], [0.2, 0.8]))[0])
    assert same_bits(gb.on_isosurface(m, "S", of="T", values=[float(np.median(T[wet]))])[0],
                     on_surfaces_host(b, "T", "S", [float(np.median(T[wet]))])[0])
    assert same_bits(gb.layer_thickness(m, "T", np.quantile(T[wet], [0.2, 0.8])), depth[:, :, 1:] - depth[:, :, :1])


def test_new_abi_entries_check_their_arguments_without_a_device():
    import torch
    lib = binding.load_library("Float32")
    INVALID, NO_DEVICE = 1, 4
    cfg = binding.Config()
    lib.gb25_default_config(C.byref(cfg), 48, 24, 6)
    h = C.c_void_p()
    st = lib.gb25_create(C.byref(cfg), C.byref(h))
    assert h and st == (0 if torch.cuda.is_available() else NO_DEVICE)
    n64 = (C.c_double * 65)(*([1.0] * 65))
    inf = (C.c_double * 2)(1.0, float("inf"))
    nan = (C.c_double * 1)(float("nan"))
    host, status = (C.c_float * (48 * 24 * 64))(), (C.c_uint8 * (48 * 24 * 64))()
    p, ps, d = C.c_void_p(), C.c_void_p(), (C.c_int32 * 3)()
    bad = [(lambda: lib.gb25_get_on_surfaces(h, 2, 0, n64, 0, host, status), b"values"),
           (lambda: lib.gb25_get_on_surfaces(h, 2, 0, n64, 65, host, status), b"values"),
           (lambda: lib.gb25_get_on_surfaces(h, 2, 0, n64, -1, host, status), b"values"),
           (lambda: lib.gb25_get_on_surfaces(h, 2, 0, inf, 2, host, status), b"values"),
           (lambda: lib.gb25_get_on_surfaces(h, 2, 0, nan, 1, host, status), b"values"),
           (lambda: lib.gb25_get_on_surfaces(h, 2, 0, None, 1, host, status), b"values"),
           (lambda: lib.gb25_get_on_surfaces(h, 4, 0, n64, 1, host, status), b"variable"),
           (lambda: lib.gb25_get_on_surfaces(h, -1, 0, n64, 1, host, status), b"variable"),
           (lambda: lib.gb25_get_on_surfaces(h, 0, 7, n64, 1, host, status), b"carried"),
           (lambda: lib.gb25_get_on_surfaces(h, 0, -1, n64, 1, host, status), b"carried"),
           (lambda: lib.gb25_get_on_surfaces(h, 0, binding.SURFACE_CARRIED["e"], n64, 1, host, status), b"carried"),   # no CATKE
           (lambda: lib.gb25_get_on_surfaces(h, 0, 0, n64, 1, None, status), b"host"),
           (lambda: lib.gb25_compute_on_surfaces(h, 0, 0, n64, 1, None, C.byref(ps), d), b"dev"),
           (lambda: lib.gb25_compute_on_surfaces(h, 3, 1, n64, 0, C.byref(p), C.byref(ps), d), b"values")]
    for n, (call, word) in enumerate(bad):
        assert call() == INVALID, n
        assert word in lib.gb25_last_error_string(h), (n, lib.gb25_last_error_string(h))
    assert lib.gb25_get_on_surfaces(None, 0, 0, n64, 1, host, status) == INVALID
    if not torch.cuda.is_available():
        for call in (lambda: lib.gb25_get_on_surfaces(h, 2, 0, n64, 64, host, None),
                     lambda: lib.gb25_compute_on_surfaces(h, 3, 1, n64, 1, C.byref(p), None, None)):
            assert call() == NO_DEVICE and b"no device" in lib.gb25_last_error_string(h)
    lib.gb25_destroy(h)


def test_the_enums_and_the_public_names():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "gb25.h")).read(), flags=re.S)
    for enum, prefix, ids in (("gb25_surface_variable", "gb25_sv_", binding.SURFACE_VARIABLES),
                              ("gb25_surface_carried", "gb25_sc_", binding.SURFACE_CARRIED),
                              ("gb25_surface_status", "gb25_surf_", binding.SURFACE_STATUS)):
        body = re.search(r"typedef enum \{([^}]*)\}\s*" + enum + ";", text).group(1)
        names = [s.strip().split()[0].lower() for s in body.split(",") if s.strip()]
        names = [n for n in names if not n.endswith("_count")]
        assert names == [prefix + k.lower() for k in ids] and list(ids.values()) == list(range(len(ids))), enum
    assert int(re.search(r"#define GB25_SURFACE_MAX_VALUES (\d+)", text).group(1)) == binding.SURFACE_MAX_VALUES == 64
    assert (FOUND, OUTCROP, GROUNDED, DRY) == tuple(binding.SURFACE_STATUS.values())
    for name in ("isosurface_depth", "on_isosurface", "at_depths", "layer_thickness", "gather_surfaces", "on_surfaces_host",
                 "surfaces_of_profiles"):
        assert callable(getattr(gb, name)), name
    assert callable(gb.Field.at_depths) and callable(binding.HipBackend.get_on_surfaces)
    from gb25_amd.distributed import LocalSlabEnsemble
    assert callable(LocalSlabEnsemble.on_surfaces)
