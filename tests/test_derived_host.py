"""Derived fields, the parts that need no GPU: the numpy restatements of gb-25_amd/derived.py on the CPU oracle's metrics and
fields (they are what the device results are compared with bit for bit in tests/test_gpu_derived.py, so they are pinned here
independently of the HIP kernels), and the new ABI entries -- dims and argument checks -- on a handle without a device.

Stokes: zeta Az summed over a box of (f,f) points telescopes to the circulation of dx u, dy v round its edge.  Every zeta Az
is the four products dy v, dy' v', dx u, dx' u' combined by three subtractions, one division and one multiplication (at most
seven roundings on top of the sum), so with the 4 n products of the box's n points as the terms, both sides lie within
(4 n + 4) eps(Float64) sum|terms| of each other -- the integrals tests' (n + 4) eps sum|term| with n = the number of terms."""
import ctypes as C
import math

import numpy as np
import pytest

import gb25_amd as gb
from gb25_amd import binding
from gb25_amd.derived import (kinetic_energy_host, mixed_layer_depth_host, mixed_layer_depth_of_profiles, vorticity_host,
                              _metric2_parent)
from helpers import make_oracle, set_noisy_velocities

EPS = float(np.finfo(np.float64).eps)


def stepped_oracle(grid_type, Nx=48, Ny=24, Nz=6):
    m = make_oracle(Nx, Ny, Nz, 60.0 if grid_type == "tripolar" else 600.0, grid_type=grid_type)
    gb.set_baroclinic_instability(m)
    set_noisy_velocities(m)
    gb.first_time_step(m)
    gb.loop(m, 2)
    return m


@pytest.mark.parametrize("grid_type", ["simple_lat_lon", "tripolar"])
def test_stokes(grid_type):
    m = stepped_oracle(grid_type)
    b = m.backend
    H = b.H
    zeta = np.asarray(vorticity_host(b), np.float64)
    Nx, by, Nz = zeta.shape
    assert zeta.shape == b.field_dims("v", False) and np.abs(zeta).max() > 0
    u = np.asarray(b.get_field("u", True), np.float64)
    v = np.asarray(b.get_field("v", True), np.float64)
    if grid_type == "simple_lat_lon":
        dy = np.full((Nx + 2 * H, by + 2 * H), gb.derived._dy(b))
        dx = np.broadcast_to(np.array([b.metric("dxc", j) for j in range(1 - H, by + H + 1)])[None, :], dy.shape)
        az = np.broadcast_to(np.array([b.metric("azf", j) for j in range(1 - H, by + H + 1)])[None, :], dy.shape)
    else:
        dy, dx, az = (_metric2_parent(b, n) for n in ("dycf", "dxfc", "azff"))
    # the box of (f,f) points [i0, i1) x [j0, j1), 0-based interior indices; k = every level
    i0, i1, j0, j1 = 3, Nx - 5, 2, by - 3
    for k in range(Nz):
        P = lambda a, i, j: a[i + H, j + H, k + H]      # parent value at the 0-based interior index
        lhs = [zeta[i, j, k] * az[i + H, j + H] for i in range(i0, i1) for j in range(j0, j1)]
        edge = [dy[i1 - 1 + H, j + H] * P(v, i1 - 1, j) for j in range(j0, j1)]            # east
        edge += [-dy[i0 - 1 + H, j + H] * P(v, i0 - 1, j) for j in range(j0, j1)]          # west
        edge += [-dx[i + H, j1 - 1 + H] * P(u, i, j1 - 1) for i in range(i0, i1)]          # north
        edge += [dx[i + H, j0 - 1 + H] * P(u, i, j0 - 1) for i in range(i0, i1)]           # south
        terms = [t for i in range(i0, i1) for j in range(j0, j1)
                 for t in (dy[i + H, j + H] * P(v, i, j), dy[i - 1 + H, j + H] * P(v, i - 1, j),
                           dx[i + H, j + H] * P(u, i, j), dx[i + H, j - 1 + H] * P(u, i, j - 1))]
        got, want = math.fsum(lhs), math.fsum(edge)
        bound = (len(terms) + 4) * EPS * math.fsum(np.abs(terms))
        print(f"  {grid_type} level {k}: sum zeta Az {got!r} circulation {want!r} |diff| {abs(got - want):.3e} bound {bound:.3e}")
        assert want != 0.0 and abs(got - want) <= bound, (k, got, want, bound)


def test_kinetic_energy_of_a_unit_zonal_flow_is_one_half():
    m = make_oracle(16, 8, 4, 600.0)
    b = m.backend
    b.set_field("u", np.ones(b.field_dims("u", True)), True)
    b.set_field("v", np.zeros(b.field_dims("v", True)), True)
    ke = kinetic_energy_host(b)
    assert ke.shape == (16, 8, 4) and (ke == 0.5).all()
    assert np.array_equal(kinetic_energy_host(b, levels=(3, 1)), ke[:, :, 3:4])
    assert np.array_equal(vorticity_host(b, levels=(1, 2)), vorticity_host(b)[:, :, 1:3])


def column(values):
    return np.asarray(values, np.float64)[None, None, :]


def test_mixed_layer_depth_of_a_linear_profile():
    """sigma = a (-z): d(k) = a (zc(top) - zc(k)), the threshold is reached a distance param / a below the centre of the top
    cell, where d = 0 by definition: the depth is param / a - zc(top).  With centres whose top one lies at z = 0 that is
    param / a itself; on the oracle's own levels the top centre lies half a cell down."""
    a, param = 2.0 ** -10, 0.03
    # (a power of two: a z is exact, so the profile is linear to the last bit)
    zc = -np.array([500.0, 300.0, 180.0, 100.0, 50.0, 20.0, 0.0])
    zf = np.concatenate([[-600.0], 0.5 * (zc[1:] + zc[:-1]), [10.0]])
    got = mixed_layer_depth_of_profiles(column(a * -zc), zc, zf, np.zeros((1, 1), int), param)[0, 0]
    print(f"  synthetic levels: {got!r} against param / a = {param / a!r}, relative {abs(got - param / a) / (param / a):.2e}")
    assert abs(got - param / a) <= 4 * EPS * (param / a)
    m = make_oracle(8, 8, 16, 600.0)
    b = m.backend
    Nz = 16
    zc = np.array([b.metric("zc", k) for k in range(1, Nz + 1)])
    sigma = np.broadcast_to((a * -zc)[None, None, :], (8, 8, Nz))
    got = mixed_layer_depth_host(b, sigma, param)
    want = param / a - zc[Nz - 1]
    assert got.shape == (8, 8, 1) and -zc[Nz - 2] > want > -zc[Nz - 1]      # (the crossing lies in the second layer)
    print(f"  the oracle's levels: {got[0, 0, 0]!r} against param / a - zc(top) = {want!r}")
    assert (np.abs(got - want) <= 4 * EPS * want).all()


def test_mixed_layer_depth_edge_cases():
    zc = -np.array([450.0, 350.0, 250.0, 150.0, 50.0])
    zf = -np.array([500.0, 400.0, 300.0, 200.0, 100.0, 0.0])
    kb0 = np.zeros((1, 1), int)
    mld = lambda s, kb=kb0, p=0.03: mixed_layer_depth_of_profiles(column(s), zc, zf, kb, p)[0, 0]
    # never crosses: the bottom face of the column -- the sea floor, or the first wet level's bottom face
    assert mld([1.02, 1.02, 1.01, 1.0, 1.0]) == 500.0
    assert mld([9.0, 9.0, 1.01, 1.0, 1.0], np.full((1, 1), 2)) == 300.0          # (the immersed values are not looked at)
    # a dry column
    assert mld([0.0] * 5, np.full((1, 1), 5)) == 0.0
    # not monotone: the first crossing from the top, although the profile comes back below the threshold further down
    got = mld([1.0, 1.5, 1.0, 1.06, 1.0])
    assert got == -(zc[4] + (zc[3] - zc[4]) * ((0.03 - 0.0) / (1.06 - 1.0 - 0.0))) and 50.0 < got < 150.0
    # the crossing uses the last level ABOVE it that is below the threshold, whatever that level's own d
    got = mld([2.0, 2.0, 2.0, 1.02, 1.0])
    d1, d0 = 1.02 - 1.0, 2.0 - 1.0
    assert got == -(zc[3] + (zc[2] - zc[3]) * ((0.03 - d1) / (d0 - d1))) and 150.0 < got < 250.0
    # exactly the threshold counts as reached
    assert mld([1.0, 1.0, 1.0, 1.0 + 0.5, 1.0], p=0.5) == 150.0
    with pytest.raises(ValueError):
        mld([1.0] * 5, p=0.0)
    # several columns at once, each by its own rule
    s = np.stack([column([1.02, 1.02, 1.01, 1.0, 1.0])[0, 0], column([0.0] * 5)[0, 0]])[None, :, :]
    out = mixed_layer_depth_of_profiles(s, zc, zf, np.array([[0, 5]]), 0.03)
    assert out.tolist() == [[500.0, 0.0]]


@pytest.fixture(scope="module", params=["Float32", "Float64"])
def lib(request):
    gb.build_library()
    return binding.load_library(request.param)


def test_derived_dims_and_argument_checks_through_the_abi(lib):
    """gb25_create without a device hands out a handle that knows its configuration: the dims need no more; every call that
    would launch returns GB25_ERR_NO_DEVICE -- after its arguments were checked."""
    import torch
    INVALID, NO_DEVICE = 1, 4
    for name in ("gb25_derived_dims", "gb25_compute_derived", "gb25_get_derived", "gb25_get_derived_stats", "gb25_get_field_levels"):
        assert hasattr(lib, name) and name in binding.ABI_SYMBOLS, name
    assert list(binding.DERIVED_IDS.values()) == list(range(5))
    d = (C.c_int32 * 3)()
    for grid_type, rows_of_v in ((0, 25), (1, 25), (4, 24)):
        cfg = binding.Config()
        lib.gb25_default_config(C.byref(cfg), 48, 24, 6)
        cfg.grid_type = grid_type
        h = C.c_void_p()
        st = lib.gb25_create(C.byref(cfg), C.byref(h))
        assert h and st == (0 if torch.cuda.is_available() else NO_DEVICE)
        want = {"vorticity": (48, rows_of_v, 6), "kinetic_energy": (48, 24, 6), "density_anomaly": (48, 24, 6),
                "potential_density": (48, 24, 6), "mixed_layer_depth": (48, 24, 1)}
        for name, q in binding.DERIVED_IDS.items():
            assert lib.gb25_derived_dims(h, q, d) == 0 and tuple(d) == want[name], (grid_type, name)
        assert lib.gb25_derived_dims(h, 5, d) == INVALID and lib.gb25_derived_dims(h, -1, d) == INVALID
        assert lib.gb25_derived_dims(h, 0, None) == INVALID and lib.gb25_derived_dims(None, 0, d) == INVALID
        p, host = C.c_void_p(), (C.c_double * (48 * 25 * 7))()
        stats = binding.FieldStats()
        bad = [lambda: lib.gb25_compute_derived(h, 5, 0.0, 0, -1, C.byref(p), d),          # no such derived field
               lambda: lib.gb25_compute_derived(h, 0, 0.0, 0, -1, None, d),                # NULL output
               lambda: lib.gb25_compute_derived(h, 0, 0.0, 6, 1, C.byref(p), d),           # first level beyond the top
               lambda: lib.gb25_compute_derived(h, 0, 0.0, 4, 3, C.byref(p), d),           # range beyond the top
               lambda: lib.gb25_compute_derived(h, 0, 0.0, -1, 1, C.byref(p), d),
               lambda: lib.gb25_compute_derived(h, 0, 0.0, 0, 0, C.byref(p), d),           # no levels
               lambda: lib.gb25_compute_derived(h, 0, 0.0, 0, -2, C.byref(p), d),
               lambda: lib.gb25_get_derived(h, 4, 0.03, 0, 2, host),                       # a 2-D result: 0, 1 or 0, -1 only
               lambda: lib.gb25_get_derived(h, 4, 0.03, 1, 1, host),
               lambda: lib.gb25_get_derived(h, 4, 0.0, 0, 1, host),                        # the threshold must be > 0
               lambda: lib.gb25_get_derived(h, 4, -0.1, 0, -1, host),
               lambda: lib.gb25_get_derived(h, 4, float("nan"), 0, -1, host),
               lambda: lib.gb25_get_derived(h, 1, 0.0, 0, -1, None),
               lambda: lib.gb25_get_derived_stats(h, 7, 0.0, C.byref(stats)),
               lambda: lib.gb25_get_derived_stats(h, 0, 0.0, None),
               lambda: lib.gb25_get_derived_stats(h, 4, 0.0, C.byref(stats)),
               lambda: lib.gb25_get_field_levels(h, 99, 0, 1, host),
               lambda: lib.gb25_get_field_levels(h, -1, 0, 1, host),
               lambda: lib.gb25_get_field_levels(h, binding.FIELD_IDS["T"], 0, 1, None),
               lambda: lib.gb25_get_field_levels(h, binding.FIELD_IDS["T"], -1, 1, host),
               lambda: lib.gb25_get_field_levels(h, binding.FIELD_IDS["T"], 0, 0, host)]
        for n, call in enumerate(bad):
            assert call() == INVALID, n
            assert len(lib.gb25_last_error_string(h)) > 10, n       # (a message, naming the call)
        if not torch.cuda.is_available():
            good = [lambda: lib.gb25_compute_derived(h, 0, 0.0, 5, 1, C.byref(p), d),
                    lambda: lib.gb25_get_derived(h, 3, 0.0, 0, -1, host),
                    lambda: lib.gb25_get_derived(h, 4, 0.03, 0, 1, host),
                    lambda: lib.gb25_get_derived_stats(h, 1, 0.0, C.byref(stats)),
                    lambda: lib.gb25_get_field_levels(h, binding.FIELD_IDS["T"], 5, 1, host)]
            for n, call in enumerate(good):
                assert call() == NO_DEVICE, n
                assert b"no device" in lib.gb25_last_error_string(h), n
        lib.gb25_destroy(h)


def test_the_enum_and_the_public_names():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "gb25.h")).read(), flags=re.S)
    body = re.search(r"typedef enum \{([^}]*)\}\s*gb25_derived;", text).group(1)
    names = [s.strip().split()[0] for s in body.split(",") if s.strip()]
    assert names == ["GB25_D_VORTICITY", "GB25_D_KINETIC_ENERGY", "GB25_D_DENSITY_ANOMALY", "GB25_D_POTENTIAL_DENSITY",
                     "GB25_D_MIXED_LAYER_DEPTH", "GB25_D_COUNT"]
    assert [n.lower() for n in names[:-1]] == ["gb25_d_" + k for k in binding.DERIVED_IDS]
    for name in ("vorticity", "kinetic_energy", "density_anomaly", "potential_density", "mixed_layer_depth", "gather_derived",
                 "vorticity_host", "kinetic_energy_host", "mixed_layer_depth_host"):
        assert callable(getattr(gb, name)), name
    assert callable(gb.Field.levels) and callable(gb.Field.surface)
    # a backend without the device kernels: the public functions fall back to the numpy restatement
    m = make_oracle(16, 8, 4, 600.0)
    gb.set_baroclinic_instability(m)
    set_noisy_velocities(m)
    assert np.array_equal(gb.vorticity(m, levels=(3, 1)), vorticity_host(m.backend, (3, 1)))
    assert np.array_equal(gb.kinetic_energy(m), kinetic_energy_host(m.backend))
    T = m.tracers.T
    assert np.array_equal(T.surface(), T.interior[:, :, 3:4]) and np.array_equal(T.levels(1, 2), T.interior[:, :, 1:3])
    assert np.array_equal(T.levels(2, -1), T.interior[:, :, 2:])
