"""The face areas, the terms and the host side of the transports (gb-25_amd/transports.py) on the CPU oracle's backend: the
numpy definitions of include/gb25.h pinned independently of the HIP kernels, and the proof that they are the model's own --
the rows of y-face transports close the continuity equation the model's w was computed from, to round-off."""
import numpy as np
import pytest

import gb25_amd as gb
from gb25_amd.binding import TRANSPORT_DTYPE
from gb25_amd.transports import (combine_transports, continuity_closure, face_area, fold_transports, transport_host,
                                 transport_terms)
from helpers import make_oracle, set_noisy_velocities

NX, NY, NZ = 8, 8, 4      # (the smallest model the oracle builds)
SUMS = ("area", "volume", "heat", "salt")


def hand_built():
    """A lat-lon model with three columns of different kbot put through set_bottom_height."""
    m = make_oracle(NX, NY, NZ, 600.0)
    b = m.backend
    zc = np.array([b.metric("zc", k) for k in range(1, NZ + 1)])
    zb = np.full((NX, NY), -1e30)
    zb[1, 1] = 0.5 * (zc[0] + zc[1])      # one immersed cell
    zb[2, 1] = 0.5 * (zc[1] + zc[2])      # two
    zb[4, 2] = 1.0                        # the whole column
    b.set_bottom_height(zb)
    kbot = np.zeros((NX, NY), int)
    kbot[1, 1], kbot[2, 1], kbot[4, 2] = 1, 2, NZ
    return m, kbot


def test_the_face_areas_of_a_hand_built_bottom():
    m, kbot = hand_built()
    b = m.backend
    c = b.cfg
    dxf = np.array([b.metric("dxf", j) for j in range(1, NY + 2)])
    dzc = np.array([b.metric("dzc", k) for k in range(1, NZ + 1)])
    dy = c.radius * ((c.lat_north - c.lat_south) / c.Ny) * (np.pi / 180.0)
    # y faces: Ny + 1 rows, both walls dry, the face between rows j - 1 and j wet where both cells are
    want = np.zeros((NX, NY + 1, NZ))
    for i in range(NX):
        for j in range(1, NY):
            for k in range(NZ):
                want[i, j, k] = dxf[j] * dzc[k] * (k >= max(kbot[i, j - 1], kbot[i, j]))
    got = face_area(b, "across_y")
    assert np.array_equal(got, want)
    assert want[1, 2, 0] == 0 and want[1, 2, 1] > 0 and want[2, 1, 1] == 0 and want[2, 1, 2] > 0
    assert (want[4, 2] == 0).all() and (want[4, 3] == 0).all() and (want[:, 0] == 0).all() and (want[:, NY] == 0).all()
    # x faces: the face between columns i - 1 (periodic) and i wet where both cells are
    want = np.zeros((NX, NY, NZ))
    for i in range(NX):
        for j in range(NY):
            for k in range(NZ):
                want[i, j, k] = dy * dzc[k] * (k >= max(kbot[i - 1, j], kbot[i, j]))
    got = face_area(b, "across_x")
    assert np.array_equal(got, want)
    assert want[3, 1, 1] == 0 and want[3, 1, 2] > 0 and (want[4, 2] == 0).all() and (want[5, 2] == 0).all() and want[0, 0, 0] > 0
    with pytest.raises(ValueError):
        face_area(b, "across_z")


def test_the_face_areas_of_the_tripolar_grid():
    Nx, Ny, Nz = 48, 24, 6      # (a folded grid needs more rows than its sub-cycle has substeps to spare)
    m = make_oracle(Nx, Ny, Nz, 600.0, grid_type="tripolar")
    b = m.backend
    dzc = np.array([b.metric("dzc", k) for k in range(1, Nz + 1)])
    dyfc = np.array([[b.metric2("dyfc", i, j) for j in range(1, Ny + 1)] for i in range(1, Nx + 1)])
    dxcf = np.array([[b.metric2("dxcf", i, j) for j in range(1, Ny + 1)] for i in range(1, Nx + 1)])
    ax = face_area(b, "across_x")
    assert ax.shape == (Nx, Ny, Nz) and (ax > 0).all()
    # the 1/2 of the pivot row on the rows of cell centres ...
    assert np.array_equal(ax[:, :Ny - 1], dyfc[:, :Ny - 1, None] * dzc[None, None, :])
    assert np.array_equal(ax[:, Ny - 1], 0.5 * (dyfc[:, Ny - 1, None] * dzc[None, :]))
    # ... and none on the rows of y faces, which a folded grid holds once: Ny of them, the southern wall dry
    ay = face_area(b, "across_y")
    assert ay.shape == (Nx, Ny, Nz) and (ay[:, 0] == 0).all()
    assert np.array_equal(ay[:, 1:], dxcf[:, 1:, None] * dzc[None, None, :])


def synthetic_lines(n, nz, seed):
    rng = np.random.default_rng(seed)
    r = np.zeros((n, nz), TRANSPORT_DTYPE)
    for f in SUMS:
        r[f] = rng.standard_normal((n, nz)) * 10.0 ** rng.integers(-3, 9, (n, nz))
    r["faces"] = rng.integers(0, 50, (n, nz))
    r["nonfinite"] = rng.integers(0, 3, (n, nz))
    return r


def test_folding_lines():
    lines = synthetic_lines(7, 5, 1)
    psi = fold_transports(lines)
    assert psi.shape == (7, 6) and psi.dtype == TRANSPORT_DTYPE
    for f in TRANSPORT_DTYPE.names:
        for n in range(7):
            acc = type(lines[f][n, 0].item())(0)
            assert psi[f][n, 0] == 0
            for k in range(5):
                acc = acc + lines[f][n, k].item()
                assert psi[f][n, k + 1] == acc, (f, n, k)


def test_combining_the_lines_of_two_slabs_and_of_a_mesh():
    nz = 3
    # two x slabs of 6 columns, 5 rows of y faces
    w, e = synthetic_lines(5, nz, 2), synthetic_lines(5, nz, 3)
    got = combine_transports([w, e], "across_y", [(0, 0), (6, 0)])
    for f in TRANSPORT_DTYPE.names:
        assert np.array_equal(got[f], w[f] + e[f])
    wx, ex = synthetic_lines(6, nz, 4), synthetic_lines(6, nz, 5)
    got = combine_transports([wx, ex], "across_x", [(0, 0), (6, 0)])
    assert got.shape == (12, nz) and got[:6].tobytes() == wx.tobytes() and got[6:].tobytes() == ex.tobytes()
    # a 2 x 2 mesh: the southern ranks hold 4 rows of y faces (the seam row belongs to the northern ones), the northern ones 5
    sw, se, nw, ne = synthetic_lines(4, nz, 6), synthetic_lines(4, nz, 7), synthetic_lines(5, nz, 8), synthetic_lines(5, nz, 9)
    offsets = [(0, 0), (6, 0), (0, 4), (6, 4)]
    got = combine_transports([sw, se, nw, ne], "across_y", offsets)
    assert got.shape == (9, nz)
    for f in TRANSPORT_DTYPE.names:
        assert np.array_equal(got[f][:4], sw[f] + se[f]) and np.array_equal(got[f][4:], nw[f] + ne[f])
    parts = [synthetic_lines(6, nz, s) for s in (10, 11, 12, 13)]
    got = combine_transports(parts, "across_x", offsets)
    assert got.shape == (12, nz)
    for f in TRANSPORT_DTYPE.names:
        assert np.array_equal(got[f][:6], parts[0][f] + parts[2][f]) and np.array_equal(got[f][6:], parts[1][f] + parts[3][f])
    # PROFILE and STREAMFUNCTION are folded again from the combined lines
    psi = combine_transports(parts, "across_x", offsets, "streamfunction")
    assert psi.tobytes() == fold_transports(got).tobytes()
    assert combine_transports(parts, "across_x", offsets, "profile").tobytes() == psi[:, -1].tobytes()


def stepped_oracle(grid, precision, steps=3, size=(48, 24, 6)):
    m = make_oracle(*size, 60.0 if grid == "gaussian_islands" else 600.0, precision, grid_type=grid)
    gb.set_baroclinic_instability(m)
    set_noisy_velocities(m)
    gb.first_time_step(m)
    gb.loop(m, steps)
    return m


def test_the_host_records():
    b = stepped_oracle("gaussian_islands_lat_lon", "f64", steps=1).backend
    for faces in ("across_y", "across_x"):
        t = transport_terms(b, faces)
        lines = transport_host(b, faces)
        axis = 0 if faces == "across_y" else 1
        assert np.array_equal(lines["faces"], t["counted"].sum(axis=axis)) and lines["nonfinite"].sum() == 0
        assert 0 < lines["faces"].sum() < t["counted"].size, "the islands dry some faces"
        assert np.allclose(lines["volume"], t["volume"].sum(axis=axis), rtol=1e-12, atol=0)
        psi = transport_host(b, faces, "streamfunction")
        assert psi.tobytes() == fold_transports(lines).tobytes()
        assert transport_host(b, faces, "profile").tobytes() == psi[:, -1].tobytes()
    # the sequential sum of the x faces, and a window of it
    t = transport_terms(b, "across_x", (2, 9))
    lines = transport_host(b, "across_x", "lines", (2, 9))
    acc = np.zeros(lines.shape)
    for j in range(9):
        acc = acc + t["heat"][:, j]
    assert t["heat"].shape[1] == 9 and np.array_equal(acc, lines["heat"])
    for bad in ((0, 0), (24, 1), (-1, 2), (20, 5)):
        with pytest.raises(ValueError):
            transport_terms(b, "across_x", bad)


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("grid", ["simple_lat_lon", "gaussian_islands_lat_lon", "gaussian_islands"])
def test_the_y_face_transports_close_the_continuity_equation(grid, precision):
    """|sum_i Az (w(k+1) - w(k)) + (V[j+1, k] - V[j, k])| over the sum of the |q| of the row's faces, at 48 x 24 x 6 after three
    steps: 3.4e-16 .. 3.8e-16 (f64) and 8.1e-8 .. 8.6e-8 (f32) when the definitions are the model's; asserted <= 16 eps(real)."""
    m = stepped_oracle(grid, precision)
    eps = float(np.finfo(m.backend.dtype).eps)
    r = continuity_closure(m.backend)
    print(f"  {grid} {precision}: residual {r:.3e}, 16 eps {16 * eps:.3e}")
    assert np.abs(m.backend.get_field("w", False)).max() > 0
    assert r <= 16 * eps
