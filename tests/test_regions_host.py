"""The numpy restatement of the coherent regions (gb-25_amd/regions.py: label_host, region_records_host, foreground) against answers
written out here: the definition of include/gb25.h pinned on the CPU, before tests/test_gpu_regions.py holds the device to it."""
import functools

import numpy as np

from gb25_amd.binding import REGION_DTYPE, Region, RegionsInfo, REGIONS_INFO_DTYPE
from gb25_amd.regions import foreground, label_host, region_records_host, regions_of_arrays


def plane(rows):
    """[i, j] bool from strings, one per row j, written with row 0 FIRST; '#' is foreground."""
    return np.array([[ch == "#" for ch in row] for row in rows]).T


def spiral(Nx, Ny):
    """A one-cell-wide path winding inwards from (0, 0), one background cell between its turns: it steps ahead while the cell
    ahead is free and the cell behind that one is not already on the path, else it turns left; it ends when it cannot."""
    m = np.zeros((Nx, Ny), bool)
    inside = lambda i, j: 0 <= i < Nx and 0 <= j < Ny
    i, j, di, dj = 0, 0, 1, 0
    m[0, 0] = True
    moved = True
    while moved:
        moved = False
        for _ in range(2):
            ni, nj = i + di, j + dj
            if inside(ni, nj) and not m[ni, nj] and not (inside(ni + di, nj + dj) and m[ni + di, nj + dj]):
                i, j, moved = ni, nj, True
                m[i, j] = True
                break
            di, dj = -dj, di
    return m


def test_the_struct_mirrors():
    assert REGION_DTYPE.itemsize == 96 and REGIONS_INFO_DTYPE.itemsize == 24
    import ctypes
    assert ctypes.sizeof(Region) == 96 and ctypes.sizeof(RegionsInfo) == 24
    assert [n for n, _ in Region._fields_] == list(REGION_DTYPE.names)


def test_a_spiral_is_one_region():
    for shape in ((9, 7), (48, 24), (200, 72)):
        m = spiral(*shape)
        assert m.sum() > shape[0] * shape[1] // 3
        lab, n = label_host(m, periodic_x=False)
        assert n == 1 and np.array_equal(lab, np.where(m, 0, -1))
    # the hand-drawn one
    m = plane(["#####",
               "....#",
               "###.#",
               "#...#",
               "#####"])
    lab, n = label_host(m, False)
    assert n == 1 and np.array_equal(lab >= 0, m)


def test_a_comb():
    m = plane(["#.#.#.#",
               "#.#.#.#",
               "#######",
               ".......",
               "#.#.#.#"])
    lab, n = label_host(m, False)
    assert n == 5
    assert np.array_equal(lab.T, [[0, -1, 0, -1, 0, -1, 0], [0, -1, 0, -1, 0, -1, 0], [0] * 7, [-1] * 7, [1, -1, 2, -1, 3, -1, 4]])
    lab, n = label_host(m, True)            # the seam joins the two outer teeth of the last row
    assert n == 4 and np.array_equal(lab.T[4], [1, -1, 2, -1, 3, -1, 1])


def test_diagonal_neighbours_are_two_regions():
    m = plane(["##..",
               "##..",
               "..##",
               "..##"])
    lab, n = label_host(m, False)
    assert n == 2 and np.array_equal(lab.T, [[0, 0, -1, -1], [0, 0, -1, -1], [-1, -1, 1, 1], [-1, -1, 1, 1]])


def test_a_blob_across_the_seam():
    m = plane(["......",
               "##..##",
               "#....#",
               "......"])
    lab, n = label_host(m, True)
    assert n == 1 and np.array_equal(lab.T[1], [0, 0, -1, -1, 0, 0])
    lab, n = label_host(m, False)
    assert n == 2 and np.array_equal(lab.T[1], [0, 0, -1, -1, 1, 1]) and np.array_equal(lab.T[2], [0, -1, -1, -1, -1, 1])


def test_a_checkerboard_is_numbered_in_index_order():
    Nx, Ny = 6, 4
    ii, jj = np.meshgrid(np.arange(Nx), np.arange(Ny), indexing="ij")
    m = (ii + jj) % 2 == 0
    for periodic in (False, True):          # (Nx even: column 0 and column Nx - 1 are never both foreground in a row)
        lab, n = label_host(m, periodic)
        assert n == 12
        assert np.array_equal(lab.T.ravel()[m.T.ravel()], np.arange(12))
    odd = (np.add.outer(np.arange(5), np.arange(2)) % 2 == 0)
    assert label_host(odd, True)[1] == 4 and label_host(odd, False)[1] == 5   # row 0: # . # . # joins across the seam


def test_all_and_none():
    lab, n = label_host(np.ones((5, 3), bool), True)
    assert n == 1 and (lab == 0).all()
    lab, n = label_host(np.zeros((5, 3), bool), True)
    assert n == 0 and (lab == -1).all()
    rec = region_records_host(np.zeros((5, 3)), np.ones((5, 3)), lab)
    assert rec.size == 0 and rec.dtype == REGION_DTYPE


def test_land_splits_a_blob_and_a_nan_is_counted():
    x = np.full((6, 3), -1.0, np.float32)
    mu = np.ones((6, 3))
    mu[2, :] = 0.0                                      # a strip of land
    x[4, 1] = np.nan
    x[2, 0] = np.nan                                    # (on land: invisible)
    x[5, 2] = 0.5                                       # above the threshold
    mask, bad = foreground(x, mu, "below", 0.0)
    assert bad == 1 and mask.sum() == 18 - 3 - 1 - 1
    lab, n = label_host(mask, periodic_x=False)
    assert n == 2 and (lab[:2] == 0).all() and (lab[2] == -1).all() and lab[4, 1] == -1 and lab[5, 2] == -1
    assert (lab[3:][mask[3:]] == 1).all()
    lab, n = label_host(mask, periodic_x=True)          # columns 0 and 5 meet in rows 0 and 1
    assert n == 1
    labels, records, infos = regions_of_arrays(x[:, :, None], mu[:, :, None], "below", 0.0, periodic_x=False, max_regions=1)
    assert tuple(infos[0]) == (2, 1, 13, 1) and records.shape == (1, 1) and records[0, 0]["cells"] == 6
    assert np.array_equal(labels[:, :, 0], label_host(mask, False)[0])
    above = foreground(x, mu, "above", 0.0)
    assert above[0].sum() == 1 and above[1] == 1


def test_the_record_of_a_five_cell_region():
    """Nx = 8, periodic; the region: (7, 1), (0, 1), (1, 1), (0, 2), (7, 2) -- across the seam.  Its key is (0, 1), index 8."""
    Nx, Ny = 8, 4
    m = np.zeros((Nx, Ny), bool)
    for i, j in ((7, 1), (0, 1), (1, 1), (0, 2), (7, 2)):
        m[i, j] = True
    m[4, 3] = True                                       # another region, numbered 1
    lab, n = label_host(m, True)
    assert n == 2 and lab[0, 1] == 0 and lab[7, 2] == 0 and lab[4, 3] == 1
    x = np.zeros((Nx, Ny))
    mu = np.zeros((Nx, Ny))
    y = np.zeros((Nx, Ny))
    # in ascending linear index: (0,1)=8, (1,1)=9, (7,1)=15, (0,2)=16, (7,2)=23
    cells = [(0, 1), (1, 1), (7, 1), (0, 2), (7, 2)]
    xv = [-3.0, -7.5, 0.1, -7.5, -1.0]                   # the extreme -7.5 twice: the first in index order is (1, 1)
    mv = [0.7, 0.6, 0.8, 1e16, 0.7]
    yv = [10.0, 20.0, 30.0, 40.0, 50.0]
    for (i, j), a, b, c in zip(cells, xv, mv, yv):
        x[i, j], mu[i, j], y[i, j] = a, b, c
    x[4, 3], mu[4, 3] = -2.0, 5.0
    rec = region_records_host(x, mu, lab, y, "below", True)
    r = rec[0]
    assert (r["cells"], r["key_i"], r["key_j"], r["i_min"], r["i_max"], r["j_min"], r["j_max"], r["wraps"]) == (5, 0, 1, 0, 7, 1, 2, 1)
    seq = lambda terms: functools.reduce(lambda a, t: a + t, terms, 0.0)
    assert r["measure"] == seq(mv)
    assert r["first"] == seq([b * a for a, b in zip(xv, mv)])
    assert r["second"] == seq([(b * a) * a for a, b in zip(xv, mv)])
    assert r["carried"] == seq([b * c for b, c in zip(mv, yv)])
    di = [0, 1, -1, 0, -1]                               # column 7 is one to the WEST of the key's column
    dj = [0, 0, 0, 1, 1]
    assert r["sum_di"] == seq([b * d for b, d in zip(mv, di)]) and r["sum_dj"] == seq([b * d for b, d in zip(mv, dj)])
    assert (r["extreme"], r["extreme_i"], r["extreme_j"]) == (-7.5, 1, 1)
    # the order is part of the answer: with these magnitudes another order of the same terms rounds differently
    assert seq(mv) != seq(mv[::-1]) and r["measure"] == ((((0.0 + 0.7) + 0.6) + 0.8) + 1e16) + 0.7
    # behind walls the same cells are two regions and nothing wraps
    lab_w, n_w = label_host(m, False)
    rec_w = region_records_host(x, mu, lab_w, y, "below", False)
    assert n_w == 3 and [int(q) for q in rec_w["cells"]] == [3, 2, 1] and not rec_w["wraps"].any()
    assert rec_w[1]["key_i"] == 7 and rec_w[1]["key_j"] == 1 and rec_w[1]["sum_di"] == 0.0
    # above: the largest, and a cap
    top = region_records_host(x, mu, lab, y, "above", True, max_regions=1)
    assert top.size == 1 and (top[0]["extreme"], top[0]["extreme_i"], top[0]["extreme_j"]) == (0.1, 7, 1)
    # a single cell whose term is -0.0 sums to +0.0 (every sum starts from +0.0)
    one = region_records_host(np.array([[-0.0]]), np.array([[1.0]]), np.array([[0]], np.int32))
    assert not np.signbit(one[0]["first"])
