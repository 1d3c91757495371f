"""Time averages accumulated on the device (gb25_averages_*) against the numpy restatement of their terms (gb-25_amd/averages.py,
pinned on the CPU by tests/test_averages_host.py), bit for bit, and the proof that sampling changes nothing a model computes.

gb25_create accepts an odd Nx on the LatitudeLongitudeGrid (Nx >= 8): the case 9 x 8 x 4, the smallest, runs the one-element
path of the kernel (a lane owns one i; with an even Nx it owns two and every accumulator access is 16 bytes wide)."""
import ctypes as C

import numpy as np
import pytest

import gb25_amd as gb
from gb25_amd.averages import FLUXES, MEANS, QUANTITIES, SQUARES, average_terms, eddy_flux, eddy_kinetic_energy, quantities_of, sample_fields
from gb25_amd.binding import FIELD_IDS, KERNEL_IDS, AVERAGE_IDS
from gb25_amd.distributed import LocalSlabEnsemble
from helpers import BASE_FIELDS, CASES, CATKE_FIELDS, GRID_NAMES, counter_rng, size_of, stepped_model

pytestmark = pytest.mark.gpu
WEIGHTS = (1.0, 0.3, 2.5, 0.7, 1.9)
INVALID, STATE = 1, 5


def sampled(m, groups=("means", "squares", "fluxes"), levels=None, weights=WEIGHTS, every=2, restate=True):
    """Take len(weights) samples, one every `every` steps; returns the numpy accumulators of the restatement and weight_sum."""
    b = m.backend
    b.averages_begin(groups, levels)
    acc, total = {}, 0.0
    for w in weights:
        if every:
            gb.loop(m, every)
        b.averages_accumulate(w)
        total = total + w
        if restate:
            fields = sample_fields(b)
            for q in quantities_of(groups):
                t = average_terms(b, q, levels, fields)
                acc[q] = acc.get(q, np.zeros(t.shape)) + w * t
    return acc, total


def check_against_the_restatement(m, what):
    b = m.backend
    acc, total = sampled(m)
    info = b.averages_info()
    assert (info.samples, info.weight_sum, info.groups) == (len(WEIGHTS), total, 7), what
    assert info.last_iteration - info.first_iteration == 2 * (len(WEIGHTS) - 1)
    for q in QUANTITIES:
        raw, mean = b.get_average(q, False), b.get_average(q, True)
        assert raw.shape == acc[q].shape == b.average_dims(q), (what, q)
        assert raw.tobytes() == acc[q].tobytes(), (what, q, "raw")
        assert mean.tobytes() == (acc[q] / total).tobytes(), (what, q, "normalized")
        assert np.isfinite(raw).all()
    for q in ("u", "v", "w", "T", "eta", "uT", "vS", "wT"):
        assert np.abs(b.get_average(q, False)).max() > 0, (what, q)
    b.averages_end()


@pytest.mark.parametrize("float_type,grid_type", CASES)
def test_every_quantity_against_the_restatement(float_type, grid_type):
    m = stepped_model(float_type, grid_type, steps=1)
    check_against_the_restatement(m, f"{float_type} grid {grid_type}")
    m.backend.close()


def test_against_the_restatement_with_catke():
    m = stepped_model("Float32", 4, steps=1, closure=gb.CATKEVerticalDiffusivity())
    check_against_the_restatement(m, "CATKE")
    m.backend.close()


def test_the_one_element_path_of_an_odd_width():
    m = stepped_model("Float32", 0, steps=1, size=(9, 8, 4))
    check_against_the_restatement(m, "9 columns")
    m.backend.close()


@pytest.mark.parametrize("float_type,grid_type", [("Float32", 1), ("Float64", 4)])
def test_masks_and_windows(float_type, grid_type):
    m = stepped_model(float_type, grid_type, steps=0)
    b = m.backend
    Nx, Ny, Nz = size_of(grid_type)
    lib, h = b.lib, b.h
    host = (C.c_double * (Nx * (Ny + 1) * (Nz + 1) + 1))()
    assert lib.gb25_averages_accumulate(h, 1.0) == STATE and b"gb25_averages_begin" in lib.gb25_last_error_string(h)
    assert lib.gb25_get_average(h, 0, 0, host, Nx * Ny * Nz) == STATE
    results = {}
    for groups in (("means",), ("means", "squares"), ("means", "squares", "fluxes")):
        for levels in ((Nz - 1, 1), (2, 3), None):
            sampled(m, groups, levels, WEIGHTS[:2], every=0, restate=False)
            results[groups, levels] = {q: b.get_average(q, False) for q in quantities_of(groups)}
            for q in QUANTITIES:
                if q not in quantities_of(groups):
                    assert lib.gb25_get_average(h, AVERAGE_IDS[q], 0, host, 1) == INVALID, (groups, q)
                    assert b"group" in lib.gb25_last_error_string(h)
    full = results[("means", "squares", "fluxes"), None]
    acc, _ = sampled(m, weights=WEIGHTS[:2], every=0)
    for q in QUANTITIES:
        assert full[q].tobytes() == acc[q].tobytes(), q
    for (groups, levels), r in results.items():
        k0, kc = (0, Nz) if levels is None else levels
        for q, a in r.items():
            faces = 1 if q[0] == "w" else 0
            want = full[q] if q.startswith("eta") else full[q][:, :, k0:k0 + kc + faces]
            assert a.shape == want.shape and a.tobytes() == np.ascontiguousarray(want).tobytes(), (groups, levels, q)
    # refusals: groups without MEANS, bad windows, counts and weights, each naming its argument
    b.averages_begin(("means", "squares"), (1, 2))
    before = b.get_average("TT", False)
    for groups in (0, 2, 4, 6, 8, 15):
        assert lib.gb25_averages_begin(h, groups, 0, -1) == INVALID and b"groups" in lib.gb25_last_error_string(h), groups
    for first, count in ((Nz, 1), (-1, 1), (0, 0), (Nz - 2, 3), (0, -2)):
        assert lib.gb25_averages_begin(h, 7, first, count) == INVALID and b"k_first" in lib.gb25_last_error_string(h), (first, count)
    for w in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.gb25_averages_accumulate(h, w) == INVALID and b"weight" in lib.gb25_last_error_string(h), w
    n = Nx * Ny * 2
    for q, count in ((AVERAGE_IDS["T"], n + 1), (AVERAGE_IDS["T"], 0), (AVERAGE_IDS["w"], n), (AVERAGE_IDS["eta"], n)):
        assert lib.gb25_get_average(h, q, 0, host, count) == INVALID and b"count" in lib.gb25_last_error_string(h), (q, count)
    assert lib.gb25_get_average(h, 17, 0, host, n) == INVALID and lib.gb25_get_average(h, AVERAGE_IDS["uT"], 0, host, n) == INVALID
    with pytest.raises(gb.GB25Error, match="weight"):
        b.averages_accumulate(-2.0)
    # nothing of that touched the accumulators or the info; begin twice starts from zero
    assert b.get_average("TT", False).tobytes() == before.tobytes() and b.averages_info().samples == 0
    b.averages_accumulate(1.0)
    assert np.abs(b.get_average("TT", False)).max() > 0
    b.averages_begin(("means", "squares"), (1, 2))
    assert not b.get_average("TT", False).any() and b.averages_info().samples == 0 and b.averages_info().weight_sum == 0
    ptr, dims = b.average_device_ptr("w")
    assert ptr and dims == (Nx, Ny, 3) == b.average_dims("w")
    b.averages_end()
    assert lib.gb25_averages_accumulate(h, 1.0) == STATE
    b.close()


@pytest.mark.parametrize("float_type,grid_type", CASES)
def test_a_steady_state(float_type, grid_type):
    """Four samples of weight 1 of the same state: every sum is exact (4 is a power of two)."""
    m = stepped_model(float_type, grid_type)
    h = gb.averages(m)
    for _ in range(4):
        h.sample(1.0)
    b = m.backend
    fields = sample_fields(b)
    for q in MEANS + SQUARES:
        assert h.mean(q).tobytes() == average_terms(b, q, None, fields).tobytes(), q
    assert np.array_equal(h.mean("T"), np.asarray(b.get_field("T", False), np.float64))
    assert np.array_equal(h.mean("uu"), np.asarray(b.get_field("u", False), np.float64) ** 2)
    assert not h.eddy_kinetic_energy().any() and not h.tracer_variance("T").any()
    for q in FLUXES:
        assert np.abs(h.mean(q)).max() > 0 and not h.eddy_flux(q).any(), q
    assert h.info().weight_sum == 4.0
    h.close()
    b.close()


LOOKAHEADS = dict(subcycle_lookahead=1, ab2_lookahead=1)


@pytest.mark.parametrize("float_type,grid_type,catke", [("Float32", 0, False), ("Float64", 0, False), ("Float32", 4, False),
                                                        ("Float64", 4, False), ("Float32", 0, True), ("Float32", 4, True)])
def test_sampling_is_read_only(float_type, grid_type, catke):
    """Two identical models; one is sampled, all groups, between every two steps.  Same bits, same look-ahead state, same
    launches of every phase of a step."""
    closure = gb.CATKEVerticalDiffusivity() if catke else None
    watched = stepped_model(float_type, grid_type, steps=0, closure=closure, **LOOKAHEADS)
    alone = stepped_model(float_type, grid_type, steps=0, closure=closure, **LOOKAHEADS)
    names = BASE_FIELDS + (CATKE_FIELDS if catke else [])
    for m in (watched, alone):
        m.backend.profile_enable(True)
        m.backend.profile_reset()
    watched.backend.averages_begin()
    for step in range(6):
        if step % 2 == 0:
            before = watched.backend.lookahead_state()
            watched.backend.averages_accumulate(1.0 + step)
            assert watched.backend.lookahead_state() == before
        for m in (watched, alone):
            gb.time_step(m)
        assert watched.backend.lookahead_state() == alone.backend.lookahead_state(), step
    assert alone.backend.lookahead_state()[0], "the velocity look-ahead is on in this configuration"
    for k in KERNEL_IDS:
        if k != "diagnostics":
            assert watched.backend.profile_get(k)[0] == alone.backend.profile_get(k)[0], k
    assert watched.backend.profile_get("diagnostics")[0] == 3 and alone.backend.profile_get("diagnostics")[0] == 0    # one launch a sample
    for name in names:
        a, b = watched.backend.get_field(name, True), alone.backend.get_field(name, True)
        assert np.array_equal(a, b, equal_nan=True), name
    assert np.abs(watched.backend.get_field("u", False)).max() > 0 and watched.backend.averages_info().samples == 3
    for m in (watched, alone):
        m.backend.close()


def test_run_averaged_leaves_the_bits_of_a_twin():
    a, b = (stepped_model("Float32", 4, steps=0, **LOOKAHEADS) for _ in range(2))
    h = gb.run_averaged(a, 6, every=3)
    gb.loop(b, 3)
    gb.loop(b, 3)
    info = h.info()
    dt = a.backend.clock()[2]
    assert info.samples == 2 and info.weight_sum == dt + 3 * dt and info.last_iteration - info.first_iteration == 3
    for name in BASE_FIELDS:
        assert np.array_equal(a.backend.get_field(name, True), b.backend.get_field(name, True), equal_nan=True), name
    assert np.abs(h.eddy_flux("vT")).max() > 0 and h.eddy_kinetic_energy().shape == (48, 24, 6)
    h.close()
    a.backend.close()
    b.backend.close()


@pytest.mark.parametrize("float_type,grid_type", [("Float32", 0), ("Float64", 4), ("Float32", 1)])
def test_repeatable_to_the_last_bit(float_type, grid_type):
    m1, m2 = stepped_model(float_type, grid_type), stepped_model(float_type, grid_type)
    for m in (m1, m2):
        sampled(m, weights=WEIGHTS[:3], restate=False)
    for q in QUANTITIES:
        for normalized in (False, True):
            s = [m.backend.get_average(q, normalized).tobytes() for m in (m1, m1, m2)]
            assert s[0] == s[1] == s[2], (q, normalized)
    m1.backend.close()
    m2.backend.close()


@pytest.mark.parametrize("float_type,grid_type", [("Float32", 1), ("Float64", 4)])
def test_a_nan_stays_where_it_is(float_type, grid_type):
    m, twin = stepped_model(float_type, grid_type, steps=0), stepped_model(float_type, grid_type, steps=0)
    Nx, Ny, Nz = size_of(grid_type)
    kbot = lambda b, i, j: int(b.bottom_info("kbot", i + 1, j + 1))
    for k in (3, Nz - 1):                                              # an interior cell; a cell under the top face
        i, j = next((i, j) for j in range(3, Ny - 3) for i in range(3 + k, Nx - 3) if kbot(m.backend, i, j) <= k)      # (a wet cell)
        for mm, poison in ((m, True), (twin, False)):
            b = mm.backend
            if poison:
                T = b.get_field("T", False).copy()
                T[i, j, k] = np.nan
                b.set_field("T", T, False)
                assert np.isnan(b.get_field("T", False)[i, j, k])
            b.averages_begin()
            b.averages_accumulate(1.5)
        hit = {"T": [(i, j, k)], "TT": [(i, j, k)], "uT": [(i, j, k), (i + 1, j, k)], "vT": [(i, j, k), (i, j + 1, k)],
               "wT": [(i, j, kf) for kf in (k, k + 1) if 1 <= kf <= Nz - 1]}
        assert len(hit["wT"]) == (2 if k < Nz - 1 else 1)
        for q in QUANTITIES:
            a, c = m.backend.get_average(q, False), twin.backend.get_average(q, False)
            want = np.zeros(a.shape, bool)
            for p in hit.get(q, []):
                want[p] = True
            assert np.array_equal(~np.isfinite(a), want), (q, np.argwhere(~np.isfinite(a)).tolist())
            assert a[~want].tobytes() == c[~want].tobytes(), q
        T = m.backend.get_field("T", False).copy()                      # (put the value back for the next cell)
        T[i, j, k] = twin.backend.get_field("T", False)[i, j, k]
        m.backend.set_field("T", T, False)
    m.backend.close()
    twin.backend.close()


@pytest.mark.parametrize("grid_type", [1, 4])
@pytest.mark.parametrize("P,Ry", [(2, 1), (4, 2)])
def test_gathered_averages_of_the_ranks(P, Ry, grid_type):
    if Ry == 1:
        Nx, Ny, Nz, dt, kw = 96 * P // 2, 40, 10, 600.0, {}
    else:
        Nx, Ny, Nz, dt, kw = 128, 48 * Ry, 8, 600.0, dict(slab_mode=1)
    single = gb.baroclinic_instability_model(gb.GPU(), Nx, Ny, Nz, dt=dt, grid_type=GRID_NAMES[grid_type], options=dict(w_on_the_fly=0))
    gb.set_baroclinic_instability(single)
    vrows = Ny if grid_type == 4 else Ny + 1
    single.set(u=(1e-2 * counter_rng((Nx, Ny, Nz), 42, 1)).astype(np.float32),
               v=(1e-2 * counter_rng((Nx, vrows, Nz), 42, 2)).astype(np.float32),
               eta=(1e-2 * counter_rng((Nx, Ny, 1), 42, 3)).astype(np.float32))
    init = {n: single.backend.get_field(n, False) for n in ("u", "v", "T", "S", "eta")}
    ens = LocalSlabEnsemble(Nx, Ny, Nz, P, dt=dt, ranks_y=Ry, grid_type=grid_type, options=dict(w_on_the_fly=0), **kw)
    for n, a in init.items():
        ens.scatter(n, a)
    gb.first_time_step(single)
    ens.first_time_step()
    sb = single.backend
    sb.averages_begin()
    ens.averages_begin()
    for w in WEIGHTS[:3]:
        gb.loop(single, 2)
        ens.loop(2)
        sb.averages_accumulate(w)
        ens.averages_sample(w)
    for name in ("u", "v", "w", "T", "S", "eta"):
        assert np.array_equal(ens.gather(name), sb.get_field(name, False)), name     # (the premise)
    what = f"{P} ranks ({Ry} in y) grid {grid_type}"
    means = {}
    for q in QUANTITIES:
        for normalized in (False, True):
            a, one = ens.average(q, normalized), sb.get_average(q, normalized)
            assert a.shape == one.shape and a.tobytes() == one.tobytes(), (what, q, normalized)
        means[q] = a
    for q in FLUXES:
        f = eddy_flux(means, q)
        assert f.tobytes() == eddy_flux({n: sb.get_average(n) for n in (q[0], q[1], q)}, q).tobytes() and np.abs(f).max() > 0, (what, q)
    assert np.array_equal(eddy_kinetic_energy(means), eddy_kinetic_energy({n: sb.get_average(n) for n in ("u", "v", "uu", "vv")}))
    ens.close()
    sb.close()


def test_out_of_memory_is_clean():
    """A window that needs more than the device has free is refused by the size check BEFORE anything is allocated.  The small
    test model cannot express such a window on a device of this size: skipped there -- nothing here allocates toward exhaustion."""
    import torch
    m = stepped_model("Float32", 0, steps=0)
    Nx, Ny, Nz = size_of(0)
    need = 8 * 18 * Nx * (Ny + 1) * (Nz + 1)                    # (an upper bound of what begin asks for)
    free = torch.cuda.mem_get_info()[0]
    if need <= free:
        m.backend.close()
        pytest.skip(f"the accumulators of the {Nx}x{Ny}x{Nz} model need {need} bytes, the device has {free} free")
    with pytest.raises(gb.GB25Error, match="free"):
        m.backend.averages_begin()
    assert m.backend.averages_info().groups == 0
    m.backend.close()
