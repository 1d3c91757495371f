"""passive_update_host (gb-25_amd/passive.py), the numpy restatement of k_passive_update, against a scalar loop written out here cell
by cell; and the C ABI of the passive tracers: declared in include/gb25.h, mirrored in binding.py, exported by both libraries."""
import ctypes
import os
import re

import numpy as np
import pytest

import gb25_amd as gb
from gb25_amd import binding
from gb25_amd.passive import ab2_factors, passive_update_host
from helpers import counter_rng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Nx, Ny, Nz, H = 8, 6, 4, 3
SHAPE = (Nx + 2 * H, Ny + 2 * H, Nz + 2 * H)


def parents(dtype, seed):
    """c, G^n, G^- with noise in EVERY cell of the parents, halos included (a cell the update must not touch shows if it does)."""
    return [(counter_rng(SHAPE, seed, q) - 0.4).astype(dtype) for q in (1, 2, 3)]


def kbot_with_a_column():
    kb = np.zeros((Nx, Ny), int)
    kb[2, 3] = 2          # an immersed column: two dry cells
    kb[7, 0] = Nz         # land next to the x seam and the southern wall
    kb[0, Ny - 2] = 1     # a source cell of the fold's images
    return kb


def scalar_update(c, Gn, Gm, dt, chi, euler, source, surface_value, surface_reset, clip, kbot, fold, update=True):
    """The definition, one cell at a time, in the order of the kernel; every product and sum rounded to the array's type."""
    f = c.dtype.type
    out = c.copy()
    C1 = f(1.5) + (f(-0.5) if euler else f(chi))
    C2 = f(0.5) + (f(-0.5) if euler else f(chi))
    src = f(float(dt) * float(source))

    def put(x, a, jj, kk):
        """cell (a, jj, kk) of the interior numbering and its periodic x images"""
        out[a + H, jj + H, kk + H] = x
        if a < H:
            out[a + Nx + H, jj + H, kk + H] = x
        if a >= Nx - H:
            out[a - Nx + H, jj + H, kk + H] = x

    for i in range(Nx):
        for j in range(Ny):
            for k in range(Nz):
                x = c[i + H, j + H, k + H]
                if update:
                    t = f(f(C1 * Gn[i + H, j + H, k + H]) - f(C2 * Gm[i + H, j + H, k + H]))
                    x = f(f(x + f(f(dt) * t)) + src)
                    if surface_reset and k == Nz - 1:
                        x = f(surface_value)
                    if clip and x < 0:
                        x = f(0)
                if kbot is not None and k < kbot[i, j]:
                    x = f(0)
                levels = [k] + ([-1] if k == 0 else []) + ([Nz] if k == Nz - 1 else [])
                for kk in levels:
                    put(x, i, j, kk)
                if j == 0:
                    put(x, i, -1, k)
                if fold:
                    q = Ny - 1 - j
                    if 1 <= q <= H:
                        for kk in levels:
                            put(x, Nx - 1 - i, Ny - 1 + q, kk)
                elif j == Ny - 1:
                    put(x, i, Ny, k)
    return out


CASES = [
    dict(euler=True),
    dict(euler=False),
    dict(euler=False, source=1.0),
    dict(euler=False, source=1.0, surface_value=0.0, surface_reset=True),
    dict(euler=True, source=-0.25, surface_value=2.5, surface_reset=True, clip_negative=True),
    dict(euler=False, clip_negative=True),
]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("immersed", [False, True])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_update_against_the_scalar_loop(dtype, fold, immersed, case):
    kw = dict(source=0.0, surface_value=0.0, surface_reset=False, clip_negative=False)
    kw.update(CASES[case])
    c, Gn, Gm = parents(dtype, 11 + case)
    kbot = kbot_with_a_column() if immersed else None
    dt, chi = 600.0, 0.1
    got = passive_update_host(c, Gn, Gm, dt, chi, H, kbot=kbot, fold=fold, **kw)
    want = scalar_update(c, Gn, Gm, dt, chi, kw["euler"], kw["source"], kw["surface_value"], kw["surface_reset"], kw["clip_negative"],
                         kbot, fold)
    assert got.dtype == want.dtype == np.dtype(dtype) and got.tobytes() == want.tobytes()
    # the pieces, each by its own property
    I = (slice(H, H + Nx), slice(H, H + Ny), slice(H, H + Nz))
    x = got[I]
    assert (x != c[I]).any()
    assert np.array_equal(got[:H, H:H + Ny, H:H + Nz], x[Nx - H:]) and np.array_equal(got[H + Nx:, H:H + Ny, H:H + Nz], x[:H]), "x images"
    assert np.array_equal(got[H:H + Nx, H - 1, H:H + Nz], x[:, 0]) and np.array_equal(got[H:H + Nx, H:H + Ny, H - 1], x[:, :, 0]), "walls"
    assert np.array_equal(got[H:H + Nx, H:H + Ny, H + Nz], x[:, :, Nz - 1])
    if fold:
        for q in range(1, H + 1):
            assert np.array_equal(got[H:H + Nx, H + Ny - 1 + q, H:H + Nz], x[::-1, Ny - 1 - q]), ("fold row", q)
            assert np.array_equal(got[:H, H + Ny - 1 + q, H:H + Nz], x[::-1, Ny - 1 - q][Nx - H:]), ("x image of a fold row", q)
    else:
        assert np.array_equal(got[H:H + Nx, H + Ny, H:H + Nz], x[:, Ny - 1])
        assert np.array_equal(got[:, H + Ny + 1:], c[:, H + Ny + 1:]), "rows beyond the layer of the wall are not written"
    assert np.array_equal(got[:, :H - 1], c[:, :H - 1]) and np.array_equal(got[:, :, :H - 1], c[:, :, :H - 1]), "deeper layers are not written"
    assert np.array_equal(got[H:H + Nx, H - 1, H - 1], c[H:H + Nx, H - 1, H - 1]), "no corner of the wall layers"
    if kw["surface_reset"]:
        wet = np.ones((Nx, Ny), bool) if kbot is None else kbot < Nz
        assert (x[:, :, Nz - 1][wet] == dtype(kw["surface_value"])).all()
    if kw["clip_negative"]:
        assert (x >= 0).all()
    if immersed:
        assert (x[2, 3, :2] == 0).all() and (x[7, 0] == 0).all()
        assert x[2, 3, 2] != 0 or kw["clip_negative"], "the first wet cell of the column is not masked (a clip may still zero it)"


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_factors_and_the_arithmetic(dtype):
    """Euler: the factors are exactly 1 and 0, so c + dt G^n whatever G^- holds; AB2: (1.5 + chi, 0.5 + chi) in the array's type;
    the source is ONE rounded product dt * source added last."""
    f = dtype
    assert ab2_factors(dtype, 0.1, True) == (f(1.0), f(0.0))
    assert ab2_factors(dtype, 0.1, False) == (f(1.5) + f(0.1), f(0.5) + f(0.1))
    c, Gn, Gm = parents(dtype, 3)
    I = (slice(H, H + Nx), slice(H, H + Ny), slice(H, H + Nz))
    e = passive_update_host(c, Gn, Gm, 600.0, 0.1, H, euler=True)[I]
    assert np.array_equal(e, c[I] + f(600.0) * Gn[I])
    a = passive_update_host(c, Gn, Gm, 600.0, 0.1, H, source=1.0 / 3.0)[I]
    C1, C2 = ab2_factors(dtype, 0.1, False)
    assert np.array_equal(a, (c[I] + f(600.0) * (C1 * Gn[I] - C2 * Gm[I])) + f(600.0 * (1.0 / 3.0)))
    # an ideal age without flow: n dt after n updates, the top level 0
    age = np.zeros(SHAPE, dtype)
    zero = np.zeros(SHAPE, dtype)
    for n in range(1, 6):
        age = passive_update_host(age, zero, zero, 600.0, 0.1, H, euler=n == 1, source=1.0, surface_reset=True)
        assert (age[I][:, :, :Nz - 1] == f(600.0 * n)).all() and (age[I][:, :, Nz - 1] == 0).all()


def test_the_mask_and_halos_alone():
    """update = False (what gb25_tracers_set does to what it has copied): the interior is kept, immersed cells are zeroed, the halo
    cells are made."""
    c, Gn, Gm = parents(np.float32, 5)
    kbot = kbot_with_a_column()
    for fold in (False, True):
        got = passive_update_host(c, None, None, 600.0, 0.1, H, kbot=kbot, fold=fold, update=False)
        want = scalar_update(c, Gn, Gm, 600.0, 0.1, False, 0.0, 0.0, False, False, kbot, fold, update=False)
        assert got.tobytes() == want.tobytes()
        wet = np.arange(Nz)[None, None, :] >= kbot[:, :, None]
        assert np.array_equal(got[H:H + Nx, H:H + Ny, H:H + Nz][wet], c[H:H + Nx, H:H + Ny, H:H + Nz][wet])


# ---- the ABI
TRACER_SYMBOLS = ["gb25_tracer_spec_bytes", "gb25_tracers_advance", "gb25_tracers_begin", "gb25_tracers_clock", "gb25_tracers_end",
                  "gb25_tracers_get", "gb25_tracers_set", "gb25_tracers_stats"]


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gb25.h")).read(), flags=re.S)


def test_the_header_declares_and_the_binding_mirrors():
    text = header_text()
    declared = sorted(n for n in set(re.findall(r"\b(gb25_[a-z_0-9]+)\s*\(", text)) if n.startswith("gb25_tracer"))
    assert declared == TRACER_SYMBOLS
    assert all(n in binding.ABI_SYMBOLS for n in TRACER_SYMBOLS)
    assert re.search(r"#define\s+GB25_TRACERS_MAX\s+8\b", text) and binding.TRACERS_MAX == 8
    # the struct, field by field, in the header's order
    body = re.search(r"typedef struct \{([^}]*)\}\s*gb25_tracer_spec;", text).group(1)
    fields = re.findall(r"\b(double|int32_t)\s+(\w+);", body)
    ctypes_of = {"double": ctypes.c_double, "int32_t": ctypes.c_int32}
    assert [(n, ctypes_of[t]) for t, n in fields] == list(binding.TracerSpec._fields_)
    assert binding.TRACER_ARRAYS == {"c": 0, "Gn": 1, "Gm": 2}


@pytest.mark.parametrize("float_type", ["Float32", "Float64"])
def test_the_libraries_export_them(float_type):
    gb.build_library()
    lib = binding.load_library(float_type)
    for name in TRACER_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.gb25_tracer_spec_bytes() == ctypes.sizeof(binding.TracerSpec) == 24
    blob = open(binding.LIB_PATHS[float_type], "rb").read()
    assert b"k_passive_update" in blob


def test_the_python_names():
    for name in ("passive_tracers", "run_with_tracers", "passive_update_host", "PassiveTracers"):
        assert hasattr(gb, name), name
    for name in ("tracers_begin", "tracers_set", "tracers_get", "tracers_advance", "tracers_stats", "tracers_clock", "tracers_end"):
        assert hasattr(binding.HipBackend, name), name
