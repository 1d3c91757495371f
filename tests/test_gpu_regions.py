"""Coherent regions on the device (gb25_get_regions, gb25_label_regions) against their numpy restatement (gb-25_amd/regions.py,
pinned on the CPU by tests/test_regions_host.py): the label planes, the records as bytes and the infos, exactly.  Patterns are
planted in T with Field.set on small models -- 48 x 24 x 6, the size of the other diagnostics' tests, and 200 x 72 x 4, whose Nx is
no multiple of 64 and whose 14400 cells of a level span 57 blocks of 256 cells, rows cut by blocks and waves anywhere --: the
spiral (the longest union-find chains), the comb, blobs across the seam and below the fold, the checkerboard beyond the cap,
random masks, regions that meet only across a block edge or the seam.  Then the sources a run has (Okubo-Weiss, the potential
density) on a stepped model with islands, windows of levels, the carried field, every refusal by name, and the proof that asking
changes nothing a model computes."""
import numpy as np
import pytest

import gb25_amd as gb
from gb25_amd.binding import REGION_DTYPE
from gb25_amd.distributed import SlabModel
from gb25_amd.integrals import cell_measure
from gb25_amd.regions import regions_host
from helpers import GRID_NAMES, counter_rng, size_of, stepped_model
from test_regions_host import spiral

pytestmark = pytest.mark.gpu
SMALL, WIDE = (48, 24, 6), (200, 72, 4)
BLOCK = 256            # REG_THREADS of csrc/region_kernels.hpp: the cells a workgroup takes

_MODELS = {}


@pytest.fixture(scope="module", autouse=True)
def _close_models():
    yield
    for m in _MODELS.values():
        m.backend.close()
    _MODELS.clear()


def model_of(float_type, grid_type, size):
    """One model per case for the whole module; the tests plant what they need in T."""
    key = (float_type, grid_type, size)
    if key not in _MODELS:
        m = gb.baroclinic_instability_model(gb.GPU(float_type=float_type), *size, dt=60.0, grid_type=GRID_NAMES[grid_type])
        gb.set_baroclinic_instability(m)
        _MODELS[key] = m
    return _MODELS[key]


def plant(m, masks):
    """T = +1 + noise everywhere, -1 - noise where masks[k] (a plane [i, j] per level, None: no foreground) holds: the regions
    of T < 0.  The noise makes every sum a sum of different numbers."""
    Nx, Ny, Nz = m.tracers.T.shape
    noise = counter_rng((Nx, Ny, Nz), 7, 3)
    T = 1.0 + noise
    for k, mask in masks.items():
        T[:, :, k] = np.where(mask, -1.0 - noise[:, :, k], T[:, :, k])
    m.tracers.T.set(T.astype(m.backend.dtype))


def assert_same(b, source, cmp, threshold, levels=None, carry=None, max_regions=4096, param=None, what=""):
    labels, records, infos = b.get_regions(source, cmp, threshold, levels, carry, max_regions, param)
    want = regions_host(b, source, cmp, threshold, levels, carry, max_regions, param)
    bad = int((labels != want[0]).sum())
    print(f"  {what or source}: regions {infos['regions'].tolist()}, stored {infos['stored'].tolist()}, foreground "
          f"{infos['foreground_cells'].tolist()}, label cells that differ {bad}")
    assert labels.dtype == np.int32 and np.array_equal(labels, want[0]), what
    assert infos.tobytes() == want[2].tobytes(), (what, infos, want[2])
    if records.tobytes() != want[1].tobytes():
        for k in range(infos.size):
            for r in range(int(infos["stored"][k])):
                assert records[k, r] == want[1][k, r], (what, k, r, records[k, r], want[1][k, r])
    assert records.tobytes() == want[1].tobytes(), what
    return labels, records, infos


def patterns(Nx, Ny):
    """{name: mask [i, j]} of the planted planes."""
    ii, jj = np.meshgrid(np.arange(Nx), np.arange(Ny), indexing="ij")
    out = {"spiral": spiral(Nx, Ny)}
    out["comb"] = (jj == 2) | ((ii % 2 == 0) & (jj > 2) & (jj < Ny - 1))
    seam = np.zeros((Nx, Ny), bool)
    seam[:3, 4:8] = seam[Nx - 4:, 5:7] = True                          # one blob across the seam ...
    seam[Nx // 2 - 2:Nx // 2 + 2, 1:4] = True                          # ... and one in the middle
    out["seam"] = seam
    out["checkerboard"] = (ii + jj) % 2 == 0
    out["all"] = np.ones((Nx, Ny), bool)
    for density in (0.3, 0.59, 0.9):
        out[f"random {density}"] = counter_rng((Nx, Ny), 11, int(100 * density)) < density
    # regions that meet only across a block edge: cell c = BLOCK q - 1 and its eastern neighbour (where both lie in one row), a
    # pair across a row that a block boundary cuts, and two that meet across the seam alone
    edges = np.zeros(Nx * Ny, bool)
    for q in range(1, (Nx * Ny) // BLOCK + 1):
        c = BLOCK * q - 1
        if c + 1 < Nx * Ny and (c + 1) % Nx:
            edges[c] = edges[c + 1] = True
        elif c + Nx < Nx * Ny:
            edges[c] = edges[c + Nx] = True
    edges = edges.reshape(Ny, Nx).T.copy()
    edges[0, Ny - 1] = edges[Nx - 1, Ny - 1] = True
    out["block edges"] = edges
    return out


@pytest.mark.parametrize("float_type", ["Float32", "Float64"])
@pytest.mark.parametrize("size", [SMALL, WIDE])
def test_planted_patterns(float_type, size):
    m = model_of(float_type, 0, size)
    b = m.backend
    Nx, Ny, Nz = size
    for name, mask in patterns(Nx, Ny).items():
        plant(m, {Nz - 1: mask, 0: ~mask})
        cap = 7 if name == "checkerboard" else 4096
        labels, records, infos = assert_same(b, "T", "below", 0.0, (Nz - 1, 1), "S", cap, what=f"{float_type} {size} {name}")
        assert np.array_equal(labels[:, :, 0] >= 0, mask) and infos["foreground_cells"][0] == mask.sum()
        if name in ("spiral", "all"):
            assert infos["regions"][0] == 1 and records[0, 0]["cells"] == mask.sum()
        if name == "all":
            assert records[0, 0]["wraps"] == 1 and (records[0, 0]["i_min"], records[0, 0]["i_max"]) == (0, Nx - 1)
        if name == "seam":
            assert infos["regions"][0] == 2 and records[0]["wraps"][:2].tolist() == [0, 1]
        if name == "checkerboard":
            assert infos["regions"][0] == Nx * Ny // 2 and infos["stored"][0] == 7 and labels.max() == Nx * Ny // 2 - 1
        if name == "block edges":
            assert (records[0]["cells"][:infos["stored"][0]] == 2).all() and records[0]["wraps"].sum() == 1
        # the complement, above the threshold, on the bottom level
        assert_same(b, "T", "above", 0.0, (0, 1), None, 4096, what=f"{float_type} {size} not {name}, above")
    plant(m, {})
    labels, records, infos = assert_same(b, "T", "below", 0.0, (Nz - 1, 1), what="no foreground")
    assert (labels == -1).all() and infos["regions"][0] == 0 and not records.tobytes().strip(b"\0")


@pytest.mark.parametrize("grid_type", [3, 1])
def test_the_fold_the_walls_and_the_land(grid_type):
    """Two blobs in the last row at mirrored columns: across the tripolar fold they would meet, here they are two regions, and so
    they are below a wall.  On the grids with islands land is background whatever T holds."""
    m = model_of("Float32", grid_type, SMALL)
    b = m.backend
    Nx, Ny, Nz = SMALL
    mask = np.zeros((Nx, Ny), bool)
    mask[5:8, Ny - 2:] = mask[Nx - 8:Nx - 5, Ny - 2:] = True
    mask[:2, 0] = mask[Nx - 2:, 0] = True                               # ... and one across the seam in the first row
    wet = cell_measure(b, "T")[:, :, Nz - 1] > 0
    plant(m, {Nz - 1: mask, 1: np.ones((Nx, Ny), bool)})
    labels, records, infos = assert_same(b, "T", "below", 0.0, (Nz - 1, 1), what=f"grid {grid_type} fold")
    assert np.array_equal(labels[:, :, 0] >= 0, mask & wet)
    if wet[mask].all():
        assert infos["regions"][0] == 3 and records[0]["wraps"][:3].tolist() == [1, 0, 0]
    labels, records, infos = assert_same(b, "T", "below", 0.0, (1, 1), what=f"grid {grid_type} all foreground")
    wet1 = cell_measure(b, "T")[:, :, 1] > 0
    assert np.array_equal(labels[:, :, 0] >= 0, wet1)
    if grid_type == 1:
        assert 0 < wet1.sum() < wet1.size, "the islands give land on this level"


@pytest.mark.parametrize("float_type", ["Float32", "Float64"])
def test_sources_of_a_run_windows_and_carry(float_type):
    m = stepped_model(float_type, 4)
    b = m.backend
    Nx, Ny, Nz = size_of(4)
    # the criterion's bits are those the getters hand out (regions_host reads them), land is background
    ow = b.get_kinematics("okubo_weiss")
    wet = cell_measure(b, "T")[:, :, Nz - 1] > 0
    threshold = float(np.percentile(np.asarray(ow[:, :, Nz - 1], np.float64)[wet], 25))      # the lowest quarter of the wet surface
    labels, records, infos = assert_same(b, "okubo_weiss", "below", threshold, (Nz - 1, 1), "T", what=f"{float_type} okubo_weiss")
    assert infos["regions"][0] > 1 and not (labels[:, :, 0] >= 0)[~wet].any() and (~wet).any()
    assert np.array_equal(labels[:, :, 0] >= 0, wet & (ow[:, :, Nz - 1] < b.dtype(threshold)))
    found = gb.regions(m, "okubo_weiss", below=threshold, levels=(Nz - 1, 1), carry="T")
    assert found.count == infos["regions"][0] and found.records.tobytes() == records[0, :infos["stored"][0]].tobytes()
    assert np.array_equal(found.labels(), labels)
    assert np.allclose(found.mean(of="carried"), found.records["carried"] / found.volume()) and (found.mean() < threshold).all()
    assert np.array_equal(found.area(), found.volume() / b.metric("dzc", Nz)) and (found.area() > 0).all()
    ci, cj = found.centroid()
    assert ((ci >= 0) & (ci < Nx) & (cj >= 0) & (cj <= Ny - 1)).all()
    sigma = b.get_derived("potential_density")
    mid = float(np.median(np.asarray(sigma[:, :, Nz - 2], np.float64)[cell_measure(b, "T")[:, :, Nz - 2] > 0]))
    # a window of several levels equals the levels one by one; carry = S
    whole = assert_same(b, "potential_density", "above", mid, (1, Nz - 1), "S", 64, what=f"{float_type} potential_density, window")
    assert (whole[1]["carried"][whole[1]["cells"] > 0] != 0).all() and whole[2]["regions"].sum() > 0
    for kk in range(Nz - 1):
        one = b.get_regions("potential_density", "above", mid, (1 + kk, 1), "S", 64)
        assert np.array_equal(one[0][:, :, 0], whole[0][:, :, kk]) and one[1].tobytes() == whole[1][kk].tobytes(), kk
        assert one[2].tobytes() == whole[2][kk:kk + 1].tobytes(), kk
    for source, param in (("kinetic_energy", None), ("divergence", None), ("gradient", "T"), ("frontogenesis", "potential_density")):
        x = b.get_derived(source) if source == "kinetic_energy" else b.get_kinematics(source, param)
        thr = float(np.median(np.asarray(x[:, :, Nz - 1], np.float64)[wet]))
        assert_same(b, source, "above", thr, (Nz - 1, 1), param=param, what=f"{float_type} {source}")
    # the device-pointer form: both pointers and the same infos
    pl, pr, info = b.label_regions("okubo_weiss", "below", threshold, (Nz - 1, 1), "T")
    assert pl and pr and info.tobytes() == infos.tobytes()
    r = gb.regions(m, "T", above=float(np.median(b.get_field("T", False)[:, :, Nz - 1])), levels=(Nz - 1, 1))
    f = m.tracers.T.regions(above=float(np.median(b.get_field("T", False)[:, :, Nz - 1])), levels=(Nz - 1, 1))
    assert r.count == f.count and r.records.tobytes() == f.records.tobytes() and r.records.dtype == REGION_DTYPE
    b.close()


@pytest.mark.parametrize("float_type", ["Float32", "Float64"])
def test_the_census_takes_sigma_of_its_own_level(float_type):
    """gb.eddy_census: W < -factor sigma_W with sigma_W the standard deviation of W over the wet cells of THAT level.  On the
    stepped model with islands it finds regions at the surface and at depth, each level at its own threshold (a level whose sigma is
    made by a few large positive values of W, as near the bottom between the islands, may hold none)."""
    from gb25_amd.regions import okubo_weiss_threshold
    m = stepped_model(float_type, 4)
    b = m.backend
    Nx, Ny, Nz = size_of(4)
    ow = np.asarray(b.get_kinematics("okubo_weiss"), np.float64)
    mu = cell_measure(b, "T")
    thresholds = []
    for level, factor in ((Nz - 1, 0.2), (2, 0.2), (Nz - 1, 1.0)):
        wet = mu[:, :, level] > 0
        want = -factor * float(np.std(ow[:, :, level][wet]))
        got = okubo_weiss_threshold(b, level, factor)
        thresholds.append(got)
        census = gb.eddy_census(m, level=level, factor=factor, carry="T", labels=True)
        direct = b.get_regions("okubo_weiss", "below", want, (level, 1), "T")
        print(f"  {float_type} level {level} factor {factor}: threshold {got:.6e}, regions {census.count}, foreground {int(census.infos['foreground_cells'][0])}")
        assert got == want and want < 0
        assert census.infos.tobytes() == direct[2].tobytes() and np.array_equal(census.labels(), direct[0])
        if (level, factor) == (Nz - 1, 0.2):
            assert census.count > 0, "the surface of the stepped model holds vortex cores"
        assert np.array_equal(census.labels()[:, :, 0] >= 0, wet & (ow[:, :, level].astype(b.dtype) < b.dtype(want)))
    assert thresholds[0] != thresholds[1], "the levels have their own sigma"
    assert gb.eddy_census(m).count == gb.eddy_census(m, level=Nz - 1).count
    # labels() asked for after the model has moved on refuses; taken with the records they stay those of the records' state
    lazy, eager = gb.eddy_census(m), gb.eddy_census(m, labels=True)
    kept = eager.labels().copy()
    gb.time_step(m)
    with pytest.raises(RuntimeError, match="stepped"):
        lazy.labels()
    assert np.array_equal(eager.labels(), kept)
    b.close()


def test_a_planted_nan_is_background_and_counted():
    m = model_of("Float32", 0, SMALL)
    b = m.backend
    Nx, Ny, Nz = SMALL
    plant(m, {Nz - 1: np.ones((Nx, Ny), bool)})
    T = b.get_field("T", False)
    T[10, 12, Nz - 1] = np.nan
    T[11, 12, Nz - 1] = -np.inf
    b.set_field("T", T, False)
    labels, records, infos = assert_same(b, "T", "below", 0.0, (Nz - 1, 1), what="planted NaN")
    assert infos["nonfinite_cells"][0] == 2 and labels[10, 12, 0] == -1 and labels[11, 12, 0] == -1 and infos["regions"][0] == 1


def test_refusals_by_name_leave_the_model_and_an_earlier_result():
    m = model_of("Float32", 0, SMALL)
    b = m.backend
    Nx, Ny, Nz = SMALL
    plant(m, {Nz - 1: patterns(Nx, Ny)["seam"]})
    before = {n: b.get_field(n, True) for n in ("T", "S", "u", "v", "eta")}
    pl, pr, info = b.label_regions("T", "below", 0.0, (Nz - 1, 1), "S")
    good = b.get_regions("T", "below", 0.0, (Nz - 1, 1), "S")
    for word, fn in (("corner quantity", lambda: b.get_regions("shear_strain", "below", 0.0)),
                     ("corner quantity", lambda: b.get_regions("rossby_number", "below", 0.0)),
                     ("corner quantity", lambda: b.get_regions("vorticity", "below", 0.0)),
                     ("2-D", lambda: b.get_regions("mixed_layer_depth", "below", 0.0)),
                     ("face field", lambda: b.get_regions("u", "below", 0.0)), ("face field", lambda: b.get_regions("w", "below", 0.0)),
                     ("face field", lambda: b.get_regions("eta", "below", 0.0)),
                     ("no such field", lambda: b.get_regions("e", "below", 0.0)),
                     ("carried_field", lambda: b.get_regions("T", "below", 0.0, carry="u")),
                     ("window", lambda: b.get_regions("T", "below", 0.0, (Nz, 1))), ("window", lambda: b.get_regions("T", "below", 0.0, (0, 0))),
                     ("window", lambda: b.get_regions("okubo_weiss", "below", 0.0, (2, Nz))),
                     ("max_regions", lambda: b.get_regions("T", "below", 0.0, max_regions=0)),
                     ("max_regions", lambda: b.label_regions("T", "below", 0.0, max_regions=-3)),
                     ("param", lambda: b.get_regions("gradient", "above", 0.0, param=3)),
                     ("param", lambda: b.get_regions("okubo_weiss", "below", 0.0, param=1)),
                     ("cmp", lambda: b.get_regions("T", 2, 0.0)), ("source_kind", lambda: b.get_regions((3, 0), "below", 0.0)),
                     ("threshold", lambda: b.get_regions("T", "below", float("nan")))):
        with pytest.raises(gb.GB25Error, match=word):
            fn()
    # nothing was made anew by a refused call: the device form hands out the same pointers and the same infos, and the host form
    # the same planes, records and infos
    again = b.label_regions("T", "below", 0.0, (Nz - 1, 1), "S")
    assert again[:2] == (pl, pr) and again[2].tobytes() == info.tobytes()
    now = b.get_regions("T", "below", 0.0, (Nz - 1, 1), "S")
    assert all(x.tobytes() == y.tobytes() for x, y in zip(now, good)) and good[2]["regions"][0] == 2
    for n, a in before.items():
        assert np.array_equal(b.get_field(n, True), a, equal_nan=True), n


def test_a_rank_refuses():
    m = SlabModel(96, 40, 10, dt=600.0, rank=0, nranks=1, slab_mode=1, transport="rccl")
    b = m.backend
    assert b.region_dims() == (96, 40, 10)
    for fn in (lambda: b.get_regions("T", "below", 0.0), lambda: b.label_regions("okubo_weiss", "below", 0.0)):
        with pytest.raises(gb.GB25Error, match="rank of a decomposition"):
            fn()
    b.close()


def test_a_census_between_the_steps_changes_nothing():
    watched, alone = (stepped_model("Float32", 4, steps=0) for _ in range(2))
    Nz = size_of(4)[2]
    for step in range(4):
        c = gb.eddy_census(watched, carry="T")
        gb.regions(watched, "potential_density", above=25.0, levels=(1, 2), carry="S").labels()
        watched.tracers.T.regions(below=10.0, levels=(Nz - 1, 1))
        assert c.count > 0, step
        for m in (watched, alone):
            gb.loop(m, 2)
    for name in ("u", "v", "w", "T", "S", "eta", "pHY", "Gn.u", "Gn.T", "U", "V"):
        assert np.array_equal(watched.backend.get_field(name, True), alone.backend.get_field(name, True), equal_nan=True), name
    assert np.abs(watched.backend.get_field("u", False)).max() > 0
    for m in (watched, alone):
        m.backend.close()
