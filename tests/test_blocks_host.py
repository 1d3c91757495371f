"""Block sums, the parts that need no GPU: the numpy restatement of gb-25_amd/blocks.py (it is what the device's planes are compared
with bit for bit in tests/test_gpu_blocks.py, so it is pinned here independently of the HIP kernel) against a plain triple-nested
Python loop per block written in the order include/gb25.h defines, the level weights, BlockSums' arithmetic with an empty block,
gather_blocks of hand-made parts, the fallback of the public functions on the oracle backend, the header against the binding, and
the new ABI entries on a handle without a device."""
import ctypes as C
import os

import numpy as np
import pytest

import gb25_amd as gb
from gb25_amd import binding
from gb25_amd.blocks import (BlockSums, block_sums_host, column_area, depth_weights, gather_blocks, resolve, sums_of_blocks)
from gb25_amd.integrals import cell_measure
from helpers import counter_rng, size_of, stepped_model
from oracle_backend import CPU

FIELDS = ("T", "u", "v", "w", "eta")
EPS = float(np.finfo(np.float64).eps)
_MODELS = {}


@pytest.fixture(scope="module", autouse=True)
def _close_models():
    yield
    for m in _MODELS.values():
        m.backend.close()
    _MODELS.clear()


def oracle_of(grid_type):
    """One oracle model per grid type for the whole module, one step in (w is not zero), with noise on eta."""
    if grid_type not in _MODELS:
        m = stepped_model("Float64", grid_type, steps=0, arch=CPU("f64"), dt=60.0 if grid_type == 3 else None)
        b = m.backend
        eta = b.get_field("eta", False)
        b.set_field("eta", eta + 1e-2 * counter_rng(eta.shape, 7, 1), False)
        _MODELS[grid_type] = m
    return _MODELS[grid_type]


def blocks_of(grid_type, nlev):
    """[(block, levels)]: whole columns, 4 x 4 in the horizontal, the grid's own odd block (two levels deep over an even window),
    whole rows; a 2-D field has one level."""
    Nx, Ny, Nz = size_of(grid_type)
    bx, by = (3, 2) if (Nx, Ny, Nz) == (48, 24, 6) else (4, 2)
    if nlev == 1:
        return [((1, 1, 1), None), ((4, 4, 1), (0, 1)), ((bx, by, 1), (0, -1)), ((Nx, 1, 1), None)]
    return [((1, 1, nlev), None), ((4, 4, 1), None), ((bx, by, 2), (nlev % 2, nlev - nlev % 2)), ((Nx, 1, 1), None)]


def loop_reference(x, mu, block, lw=None):
    """The definition, point by point: per block the column partials (ascending k), the segments (ascending i), the block
    (ascending j); every sum from +0.0, what does not count adds nothing."""
    bx, by, bz = block
    nI, nJ, nK = x.shape[0] // bx, x.shape[1] // by, x.shape[2] // bz
    out = np.zeros((3, nI, nJ, nK))
    points = np.zeros((nI, nJ, nK), int)
    nonfinite = np.zeros((nI, nJ, nK), int)
    for I in range(nI):
        for J in range(nJ):
            for K in range(nK):
                block_sum = [0.0, 0.0, 0.0]
                for j in range(J * by, (J + 1) * by):
                    segment = [0.0, 0.0, 0.0]
                    for i in range(I * bx, (I + 1) * bx):
                        column = [0.0, 0.0, 0.0]
                        for k in range(K * bz, (K + 1) * bz):
                            m = float(mu[i, j, k])
                            if lw is not None:
                                m = m * float(lw[k])
                            if not m > 0.0:
                                continue
                            v = float(x[i, j, k])
                            if not np.isfinite(v):
                                nonfinite[I, J, K] += 1
                                continue
                            t = m * v
                            q = t * v
                            column = [column[0] + m, column[1] + t, column[2] + q]
                            points[I, J, K] += 1
                        segment = [a + c for a, c in zip(segment, column)]
                    block_sum = [a + s for a, s in zip(block_sum, segment)]
                out[:, I, J, K] = block_sum
    return out[0], out[1], out[2], points, nonfinite


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("grid_type", [0, 1, 3, 4])
def test_the_restatement_equals_the_loop(grid_type):
    b = oracle_of(grid_type).backend
    Nx, Ny, Nz = size_of(grid_type)
    for name in FIELDS:
        full = np.asarray(b.get_field(name, False), np.float64)
        nlev = full.shape[2]
        mu_full = cell_measure(b, name)
        for block, levels in blocks_of(grid_type, nlev):
            k0, kc = (0, nlev) if levels is None else (levels[0], nlev - levels[0] if levels[1] == -1 else levels[1])
            got = block_sums_host(b, name, block, levels)
            x, mu = full[:, :Ny, k0:k0 + kc], mu_full[:, :Ny, k0:k0 + kc]
            m, t, q, points, nonfinite = loop_reference(x, mu, block)
            assert got.dims == m.shape == (Nx // block[0], Ny // block[1], kc // block[2]), (name, block)
            assert same(got.measure, m) and same(got.first, t) and same(got.second, q), (name, block)
            assert np.array_equal(got.points_of_blocks, points) and got.points == points.sum() and got.nonfinite == 0, (name, block)
            assert got.empty_blocks == int((m == 0).sum()) and got.global_offset == (0, 0, 0), (name, block)
            assert (t != 0).any(), (name, block)
        # block (1, 1, 1) is the measure itself and mu x
        one = block_sums_host(b, name, (1, 1, 1))
        counted = mu_full[:, :Ny] > 0
        assert same(one.measure, np.where(counted, mu_full[:, :Ny], 0.0)) and same(one.first, np.where(counted, mu_full[:, :Ny] * full[:, :Ny], 0.0)), name
    if grid_type in (1, 4):
        cols = block_sums_host(b, "T", (1, 1, Nz))
        assert cols.empty_blocks > 0 and ((cols.points_of_blocks > 0) & (cols.points_of_blocks < Nz)).any(), "dry and partial columns"
    if grid_type in (3, 4):
        # the pivot row carries the 1/2, the row below it does not: the measure with and without it
        dz = np.array([b.metric("dzc", k) for k in range(1, Nz + 1)])
        one = block_sums_host(b, "T", (1, 1, 1)).measure
        for j, fold in ((Ny, 0.5), (Ny - 1, 1.0)):
            whole = np.array([b.metric2("azcc", i, j) for i in range(1, Nx + 1)])[:, None] * dz[None, :]
            wet = one[:, j - 1] > 0
            assert wet.any() and np.array_equal(one[:, j - 1][wet], (whole * fold)[wet]), j
            assert fold == 1.0 or not np.array_equal(one[:, j - 1][wet], whole[wet])


def test_a_planted_nan_and_weights_in_the_loop_order():
    b = oracle_of(1).backend
    Nx, Ny, Nz = size_of(1)
    x = np.asarray(b.get_field("T", False), np.float64).copy()
    mu = cell_measure(b, "T")
    i0, j0 = (int(q) for q in np.argwhere(mu[:, :, Nz - 1] > 0)[5])
    x[i0, j0, Nz - 1] = np.nan
    dry = np.argwhere(mu[:, :, 0] == 0)[0]
    x[dry[0], dry[1], 0] = np.inf                          # (in an immersed cell: invisible)
    lw = np.array([0.0, 0.25, 1.0, 1.0, 0.5, 1.0])
    for block in ((3, 2, 2), (1, 1, Nz), (4, 4, 1)):
        for w in (None, lw):
            got = block_sums_host(b, "T", block, None, w, values=x)
            m, t, q, points, nonfinite = loop_reference(x, mu, block, w)
            assert same(got.measure, m) and same(got.first, t) and same(got.second, q), (block, w is None)
            assert got.nonfinite == nonfinite.sum() == 1 and np.array_equal(got.points_of_blocks, points), (block, w is None)
            assert np.isfinite(got.first).all() and np.isfinite(got.second).all()


def test_depth_weights():
    b = oracle_of(0).backend
    Nz = size_of(0)[2]
    zf = np.array([b.metric("zf", k) for k in range(1, Nz + 2)], np.float64)
    depth, dz = -zf[0], np.diff(zf)
    assert depth > 0 and zf[Nz] == 0
    assert (depth_weights(b, 0.0, depth) == 1).all() and (depth_weights(b, 0.0, 2 * depth) == 1).all()
    assert (depth_weights(b, 0.0, depth, faces=True) == 1).all() and depth_weights(b, 0.0, depth, faces=True).shape == (Nz + 1,)
    assert (depth_weights(b, 1.5 * depth, 2 * depth) == 0).all() and (depth_weights(b, 0.0, 0.0) == 0).all()
    zc = 0.5 * (zf[:-1] + zf[1:])
    dzf = np.diff(np.concatenate([zf[:1], zc, zf[-1:]]))
    for top, bottom in ((0.0, 700.0), (0.0, -zf[Nz - 1] * 0.5), (-zf[3], -zf[1]), (33.0, 0.77 * depth), (10.0, 2 * depth)):
        w = depth_weights(b, top, bottom)
        assert w.shape == (Nz,) and (w >= 0).all() and (w <= 1).all()
        assert abs(float((w * dz).sum()) - (min(bottom, depth) - min(top, depth))) <= 4 * EPS * depth, (top, bottom)
        inside = (-zf[1:] >= top) & (-zf[:-1] <= bottom)
        assert (w[inside] == 1).all() and (w[(-zf[:-1] <= top) | (-zf[1:] >= bottom)] == 0).all(), (top, bottom)
        wf = depth_weights(b, top, bottom, faces=True)
        assert abs(float((wf * dzf).sum()) - (min(bottom, depth) - min(top, depth))) <= 4 * EPS * depth, (top, bottom)
    with pytest.raises(ValueError, match="depth range"):
        depth_weights(b, 10.0, 5.0)


def test_weights_of_ones_and_zeros():
    b = oracle_of(4).backend
    Nx, Ny, Nz = size_of(4)
    for name, block in (("T", (3, 2, 2)), ("u", (1, 1, Nz)), ("w", (4, 4, 1))):
        nlev = b.field_dims(name, False)[2]
        plain = block_sums_host(b, name, block)
        ones = block_sums_host(b, name, block, None, np.ones(nlev))
        for plane in ("measure", "first", "second"):
            assert same(getattr(plain, plane), getattr(ones, plane)), (name, plane)
        assert plain.points == ones.points
    # zeros below k0 with whole columns = the window from k0 on
    k0 = 2
    lw = (np.arange(Nz) >= k0).astype(float)
    a = block_sums_host(b, "T", (1, 1, Nz), None, lw)
    w = block_sums_host(b, "T", (1, 1, Nz - k0), (k0, Nz - k0))
    assert same(a.measure, w.measure) and same(a.first, w.first) and same(a.second, w.second) and a.points == w.points


def test_mean_variance_and_integral_with_an_empty_block():
    m = np.array([[[2.0], [0.0]], [[4.0], [1.0]]])
    t = np.array([[[6.0], [0.0]], [[-4.0], [3.0]]])
    q = np.array([[[20.0], [0.0]], [[4.0], [9.0]]])
    s = BlockSums(m, t, q, block=(2, 2, 1), dims=(2, 2, 1), points=7, nonfinite=0, empty_blocks=1)
    mean, var = s.mean(), s.variance()
    assert np.isnan(mean[0, 1, 0]) and np.isnan(var[0, 1, 0])
    assert mean[0, 0, 0] == 3.0 and mean[1, 0, 0] == -1.0 and mean[1, 1, 0] == 3.0
    assert var[0, 0, 0] == 1.0 and var[1, 0, 0] == 0.0 and var[1, 1, 0] == 0.0
    assert s.integral() is t and s.info["empty_blocks"] == 1 and s.info["dims"] == (2, 2, 1)
    # rounding may leave second / measure a hair below mean^2: clipped at 0
    tiny = BlockSums(np.array([[[3.0]]]), np.array([[[0.3]]]), np.array([[[0.03 * (1 - 4 * EPS)]]]), block=(1, 1, 1), dims=(1, 1, 1),
                     points=1, nonfinite=0, empty_blocks=0)
    assert tiny.variance()[0, 0, 0] == 0.0


def test_gather_blocks_of_hand_made_parts():
    rng = lambda shape, salt: counter_rng(shape, 11, salt)
    parts, whole = [], {n: np.zeros((6, 4, 2)) for n in ("measure", "first", "second")}
    for rank, (rx, ry) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
        planes = {n: rng((3, 2, 2), 10 * rank + q) for q, n in enumerate(whole)}
        for n in whole:
            whole[n][3 * rx:3 * rx + 3, 2 * ry:2 * ry + 2] = planes[n]
        parts.append(BlockSums(planes["measure"], planes["first"], planes["second"], block=(4, 3, 2), dims=(3, 2, 2), points=10 + rank,
                               nonfinite=rank, empty_blocks=1, global_offset=(12 * rx, 6 * ry, 0)))
    got = gather_blocks(parts)
    assert got.dims == (6, 4, 2) and got.block == (4, 3, 2) and got.global_offset == (0, 0, 0)
    assert (got.points, got.nonfinite, got.empty_blocks) == (46, 6, 4) and got.points_of_blocks is None
    for n in whole:
        assert same(getattr(got, n), whole[n]), n
    only_first = [BlockSums(None, p.first, None, block=p.block, dims=p.dims, points=0, nonfinite=0, empty_blocks=0, global_offset=p.global_offset)
                  for p in parts]
    got = gather_blocks(only_first)
    assert got.measure is None and got.second is None and same(got.first, whole["first"])
    parts[1].global_offset = (10, 0, 0)
    with pytest.raises(ValueError, match="offset"):
        gather_blocks(parts)


def test_the_argument_checks_of_the_restatement():
    b = oracle_of(0).backend
    Nx, Ny, Nz = size_of(0)
    assert resolve(b, "w", (4, 4, 2), (1, Nz))[4] == (Nx // 4, Ny // 4, Nz // 2)
    assert resolve(b, "w", (1, 1, Nz + 1))[4] == (Nx, Ny, 1) and resolve(b, "eta", (2, 2, 1), (0, -1))[4] == (Nx // 2, Ny // 2, 1)
    for word, call in (("bx", lambda: resolve(b, "T", (0, 1, 1))), ("bx", lambda: resolve(b, "T", (5, 1, 1))),
                       ("by", lambda: resolve(b, "T", (1, 5, 1))), ("by", lambda: resolve(b, "v", (1, Ny + 1, 1))),
                       ("bz", lambda: resolve(b, "T", (1, 1, 3))), ("bz", lambda: resolve(b, "T", (1, 1, 0))),
                       ("bz", lambda: resolve(b, "eta", (1, 1, 2))),
                       ("window", lambda: resolve(b, "T", (1, 1, 1), (Nz, 1))), ("window", lambda: resolve(b, "T", (1, 1, 1), (1, Nz))),
                       ("window", lambda: resolve(b, "eta", (1, 1, 1), (0, 2))),
                       ("level_weights", lambda: resolve(b, "T", (1, 1, 1), None, -np.ones(Nz))),
                       ("level_weights", lambda: resolve(b, "T", (1, 1, 1), None, np.full(Nz, np.nan))),
                       ("level_weights", lambda: resolve(b, "T", (1, 1, 1), None, np.ones(Nz + 1))),
                       ("level_weights", lambda: resolve(b, "eta", (1, 1, 1), None, np.ones(1))),
                       ("vorticity", lambda: resolve(b, "vorticity", (1, 1, 1)))):
        with pytest.raises(ValueError, match=word):
            call()
    with pytest.raises(ValueError, match="bx = 512 must be 1 .. 256"):
        resolve(b, "T", (8 * Nx, 1, 1))


def test_the_public_functions_fall_back_to_the_restatement():
    m = oracle_of(1)
    b = m.backend
    Nx, Ny, Nz = size_of(1)
    T = np.asarray(b.get_field("T", False), np.float64)
    mu = cell_measure(b, "T")
    coarse = gb.coarsen(m, "T", (4, 4, 2))
    ref = block_sums_host(b, "T", (4, 4, 2))
    assert coarse.shape == (Nx // 4, Ny // 4, Nz // 2) and np.array_equal(coarse, ref.mean(), equal_nan=True)
    assert np.array_equal(m.tracers.T.coarsen((4, 4, 2)), coarse, equal_nan=True)
    assert np.array_equal(gb.coarsen(m, "T", (4, 4, 1), levels=(Nz - 1, 1)), block_sums_host(b, "T", (4, 4, 1), (Nz - 1, 1)).mean(), equal_nan=True)
    wet = ref.measure > 0
    assert wet.any() and (coarse[wet] >= T[mu > 0].min()).all() and (coarse[wet] <= T[mu > 0].max()).all()
    var = gb.subgrid_variance(m, "T", (4, 4, 2))
    assert np.array_equal(var, ref.variance(), equal_nan=True) and (var[wet] >= 0).all() and (var[wet] > 0).any()
    ke = gb.coarsen(m, "kinetic_energy", (2, 2, 1))
    assert ke.shape == (Nx // 2, Ny // 2, Nz) and np.nanmax(ke) > 0
    # columns: the integral over depth, the depth mean, the heat content
    area = column_area(b, "T")
    assert same(area, block_sums_host(b, "eta", (1, 1, 1)).measure[:, :, 0]) and (area >= 0).all() and (area == 0).any()
    cols = block_sums_host(b, "T", (1, 1, Nz))
    ocean = area > 0
    want = np.where(ocean, cols.first[:, :, 0] / np.where(ocean, area, 1.0), 0.0)
    assert np.array_equal(gb.column_integral(m, "T"), want)
    dz = np.array([b.metric("dzc", k) for k in range(1, Nz + 1)])
    plain = (np.where(mu > 0, T, 0.0) * dz[None, None, :]).sum(axis=2)
    assert np.allclose(gb.column_integral(m, "T")[ocean], plain[ocean], rtol=1e-12)
    assert np.array_equal(gb.depth_mean(m, "T"), cols.mean()[:, :, 0], equal_nan=True)
    zf = np.array([b.metric("zf", k) for k in range(1, Nz + 2)])
    d = -0.5 * (zf[Nz - 2] + zf[Nz - 1])                    # (inside a level)
    lw = depth_weights(b, 0.0, d)
    assert 0 < lw[Nz - 2] < 1 and lw[Nz - 1] == 1 and (lw[:Nz - 2] == 0).all()
    top = block_sums_host(b, "T", (1, 1, Nz), None, lw)
    rho0, cp = b.cfg.rho0, 3991.86795711963
    want = np.where(ocean, (rho0 * cp) * top.first[:, :, 0] / np.where(ocean, area, 1.0), 0.0)
    hc = gb.heat_content(m, depth_range=(0.0, d))
    assert np.array_equal(hc, want) and (hc[ocean & (top.measure[:, :, 0] > 0)] > 0).all()
    shifted = gb.heat_content(m, depth_range=(0.0, d), reference_temperature=1.0)
    assert np.allclose((hc - shifted)[ocean], (rho0 * cp) * (top.measure[:, :, 0] / np.where(ocean, area, 1.0))[ocean], rtol=1e-9)
    assert np.array_equal(gb.column_integral(m, "w", depth_range=(0.0, d)).shape, (Nx, Ny))


def test_the_header_the_binding_and_the_exports():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "gb25.h")).read()
    lib = binding.load_library("Float32")
    for symbol in ("gb25_block_info_bytes", "gb25_block_dims", "gb25_derived_block_dims", "gb25_get_block_sums", "gb25_compute_block_sums",
                   "gb25_get_derived_block_sums"):
        assert symbol in text and hasattr(lib, symbol) and symbol in binding.ABI_SYMBOLS, symbol
    assert lib.gb25_block_info_bytes() == C.sizeof(binding.BlockInfo) == 56 and C.sizeof(binding.Blocks) == 24
    assert "#define GB25_BLOCK_MAX_BX 256" in text
    for name in ("coarsen", "column_integral", "depth_mean", "heat_content", "subgrid_variance", "block_sums_host", "depth_weights",
                 "gather_blocks", "sums_of_blocks"):
        assert callable(getattr(gb, name)), name
    for name in ("block_sums", "compute_block_sums", "block_dims"):
        assert callable(getattr(binding.HipBackend, name)), name
    from gb25_amd.distributed import LocalSlabEnsemble
    assert callable(LocalSlabEnsemble.block_sums) and callable(gb.Field.coarsen)


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
    F = binding.FIELD_IDS
    d = (C.c_int32 * 3)()
    B = lambda bx, by, bz, k0=0, kc=-1: C.byref(binding.Blocks(bx, by, bz, k0, kc, 0))
    for f, blk, want in (("T", B(4, 4, 2), (12, 6, 3)), ("w", B(1, 1, Nz + 1), (Nx, Ny, 1)), ("v", B(3, 2, 2, 1, 4), (16, 12, 2)),
                         ("eta", B(Nx, 1, 1, 0, 1), (1, Ny, 1)), ("U", B(2, 2, 1), (24, 12, 1))):
        assert lib.gb25_block_dims(h, F[f], blk, d) == 0 and tuple(d) == want, f
    assert lib.gb25_derived_block_dims(h, 1, B(4, 4, 2), d) == 0 and tuple(d) == (12, 6, 3)
    assert lib.gb25_derived_block_dims(h, 4, B(4, 4, 1), d) == 0 and tuple(d) == (12, 6, 1)
    n = Nx * Ny * (Nz + 1)
    a, info, p = (C.c_double * n)(), binding.BlockInfo(), C.c_void_p()
    vector = lambda values: (C.c_double * (Nz + 1))(*values)
    ones, neg, last, nan = vector([1.0] * (Nz + 1)), vector([1.0, -1.0] + [1.0] * (Nz - 1)), vector([1.0] * Nz + [-0.5]), vector([float("nan")] * (Nz + 1))
    get = lambda f, blk, lw=None, outs=(a, a, a): lib.gb25_get_block_sums(h, F[f], blk, lw, *outs, C.byref(info))
    bad = [(lambda: get("T", B(0, 1, 1)), b"bx"), (lambda: get("T", B(-2, 1, 1)), b"bx"), (lambda: get("T", B(5, 1, 1)), b"bx"), (lambda: get("T", B(8 * Nx, 1, 1)), b"bx"),
           (lambda: get("T", B(1, 0, 1)), b"by"), (lambda: get("T", B(1, 5, 1)), b"by"), (lambda: get("v", B(1, Ny + 1, 1)), b"by"),
           (lambda: get("T", B(1, 1, 0)), b"bz"), (lambda: get("T", B(1, 1, 4)), b"bz"), (lambda: get("T", B(1, 1, 2, 1, 3)), b"bz"),
           (lambda: get("eta", B(1, 1, 2)), b"bz"),
           (lambda: get("T", B(1, 1, 1, Nz, 1)), b"window"), (lambda: get("T", B(1, 1, 1, 0, 0)), b"window"),
           (lambda: get("T", B(1, 1, 1, 2, Nz)), b"window"), (lambda: get("T", B(1, 1, 1, -1, 1)), b"window"),
           (lambda: get("eta", B(1, 1, 1, 0, 2)), b"window"), (lambda: get("eta", B(1, 1, 1, 1, 1)), b"window"),
           (lambda: get("T", B(1, 1, 1), neg), b"level_weight[1]"), (lambda: get("w", B(1, 1, 1), last), b"level_weight[6]"),
           (lambda: get("T", B(1, 1, 1), nan), b"level_weight[0]"), (lambda: get("eta", B(1, 1, 1), ones), b"level_weight"),
           (lambda: get("T", B(1, 1, 1), None, (None, None, None)), b"no output"),
           (lambda: lib.gb25_get_block_sums(h, F["T"], None, None, a, a, a, None), b"blocks"),
           (lambda: lib.gb25_get_block_sums(h, 999, B(1, 1, 1), None, a, a, a, None), b"no field"),
           (lambda: lib.gb25_compute_block_sums(h, F["T"], B(1, 1, 1), None, None, None, d), b"dev"),
           (lambda: lib.gb25_compute_block_sums(h, F["T"], B(7, 1, 1), None, None, C.byref(p), d), b"bx"),
           (lambda: lib.gb25_get_derived_block_sums(h, 0, 0.0, B(1, 1, 1), None, a, a, a, None), b"GB25_D_VORTICITY"),
           (lambda: lib.gb25_get_derived_block_sums(h, 9, 0.0, B(1, 1, 1), None, a, a, a, None), b"no derived field"),
           (lambda: lib.gb25_get_derived_block_sums(h, 4, 0.0, B(1, 1, 1), None, a, a, a, None), b"mixed-layer"),
           (lambda: lib.gb25_get_derived_block_sums(h, 4, 0.03, B(1, 1, 1), ones, a, a, a, None), b"level_weight"),
           (lambda: lib.gb25_get_derived_block_sums(h, 1, 0.0, B(1, 1, 4), None, a, a, a, None), b"bz"),
           (lambda: lib.gb25_get_derived_block_sums(h, 1, 0.0, B(1, 1, 1), None, None, None, None, None), b"no output"),
           (lambda: lib.gb25_block_dims(h, F["T"], B(5, 1, 1), d), b"bx"),
           (lambda: lib.gb25_derived_block_dims(h, 0, B(1, 1, 1), d), b"GB25_D_VORTICITY")]
    for n_, (call, word) in enumerate(bad):
        assert call() == INVALID, n_
        assert word in lib.gb25_last_error_string(h), (n_, lib.gb25_last_error_string(h))
    assert lib.gb25_get_block_sums(None, F["T"], B(1, 1, 1), None, a, a, a, None) == INVALID
    if not torch.cuda.is_available():
        good = [lambda: get("T", B(4, 4, 2)), lambda: get("w", B(1, 1, Nz + 1), ones), lambda: get("eta", B(1, 1, 1), None, (a, None, None)),
                lambda: lib.gb25_compute_block_sums(h, F["u"], B(3, 2, 2), None, C.byref(info), C.byref(p), d),
                lambda: lib.gb25_get_derived_block_sums(h, 1, 0.0, B(4, 4, 1), None, None, a, None, C.byref(info)),
                lambda: lib.gb25_get_derived_block_sums(h, 4, 0.03, B(1, 1, 1), None, a, a, a, None)]
        for n_, call in enumerate(good):
            assert call() == NO_DEVICE, n_
            assert b"no device" in lib.gb25_last_error_string(h), n_
    lib.gb25_destroy(h)
