"""Checkpoint and bit-for-bit restart on the device (include/gb25.h, "checkpoint and bit-for-bit restart").

Model A: first_time_step, loop(3), checkpoint, loop(4).  A fresh model B of the same configuration: restore, loop(4).  Every parent
array, halos included, and the clock are equal to the bit; a twin that never checkpoints equals A too.  The comparison is between
runs with the same call boundaries (the last bits of w's association belong to a gb25_loop call: W_ON_THE_FLY).

The members whose element count is no multiple of the vector width: test_checksums_heads_and_tails runs 67 x 30 x 8, whose planes
have 83 columns; it says there which members are odd and which start off a 16-byte boundary.  Decompositions: test_decompositions."""
import os

import numpy as np
import pytest

import gb25_amd as gb
from gb25_amd import restart
from gb25_amd.binding import FIELD_IDS, GB25Error
from helpers import CASES, GRID_NAMES, set_noisy_velocities, size_of

pytestmark = pytest.mark.gpu

CATKE_CASES = [("Float32", 0), ("Float64", 4)]


def build(float_type, grid_type, size=None, closure=None, coupled=False, bottom=None, **options):
    Nx, Ny, Nz = size or size_of(grid_type)
    dt = 60.0 if grid_type == 4 else 600.0
    if coupled:
        return gb.data_free_ocean_climate_model_init(gb.GPU(float_type=float_type), Nz=Nz, size=(Nx, Ny), dt=30.0)
    m = gb.baroclinic_instability_model(gb.GPU(float_type=float_type), Nx, Ny, Nz, dt=dt, grid_type=GRID_NAMES[grid_type],
                                        closure=closure, options=options or None)
    if bottom is not None:
        m.backend.set_bottom_height(bottom)
    gb.set_baroclinic_instability(m)
    set_noisy_velocities(m)
    return m


def existing_fields(m):
    out = []
    for n in FIELD_IDS:
        try:
            m.backend.field_dims(n, True)
            m.backend.get_field(n, True)
            out.append(n)
        except GB25Error:
            pass
    return out


def state_of(m):
    return {n: m.backend.get_field(n, True) for n in existing_fields(m)}


def bits(a):
    a = np.asarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def assert_same_bits(a, b, label):
    sa, sb = state_of(a), state_of(b)
    assert list(sa) == list(sb), label
    bad = [n for n in sa if not np.array_equal(bits(sa[n]), bits(sb[n]))]
    assert not bad, f"{label}: fields differ in their bits: {bad}"
    assert a.backend.clock() == b.backend.clock(), label


def restart_roundtrip(tmp_path, make, steps_before, label):
    """A: steps_before, checkpoint, then on; B: restore, then on; A2: a twin of A that never checkpoints."""
    a, a2, b = make(), make(), make()
    for m in (a, a2):
        if steps_before >= 1:
            gb.first_time_step(m)
        if steps_before > 1:
            gb.loop(m, steps_before - 1)
    before = a.backend.lookahead_state()
    path = a.checkpoint(str(tmp_path), label)
    assert a.backend.lookahead_state() == before, "a snapshot voids no look-ahead"
    assert os.path.exists(path) and not os.path.exists(path + ".tmp")
    info = gb.restore(b, str(tmp_path), label)
    assert info.members == len(restart.read_checkpoint(path).names())
    assert b.backend.clock() == a.backend.clock()
    for m in (a, a2, b):
        if steps_before == 0:
            gb.first_time_step(m)
        gb.loop(m, 4)
    assert_same_bits(a, a2, f"{label}: the run that checkpointed against its twin that never did")
    assert_same_bits(a, b, f"{label}: the restored run against the run that went on")
    assert restart.verify(path) == []
    return path


@pytest.mark.parametrize("float_type, grid_type", CASES)
def test_bit_for_bit(tmp_path, float_type, grid_type):
    restart_roundtrip(tmp_path, lambda: build(float_type, grid_type), 4, f"{float_type}-{grid_type}")


@pytest.mark.parametrize("steps_before", [0, 1])
@pytest.mark.parametrize("float_type, grid_type", [("Float32", 0), ("Float64", 4)])
def test_bit_for_bit_at_the_start(tmp_path, float_type, grid_type, steps_before):
    restart_roundtrip(tmp_path, lambda: build(float_type, grid_type), steps_before, f"start{steps_before}")


@pytest.mark.parametrize("float_type, grid_type", CATKE_CASES)
def test_bit_for_bit_catke(tmp_path, float_type, grid_type):
    path = restart_roundtrip(tmp_path, lambda: build(float_type, grid_type, closure=gb.CATKEVerticalDiffusivity()), 4, "catke")
    assert len(restart.read_checkpoint(path).names()) >= 31


def test_bit_for_bit_coupled(tmp_path):
    path = restart_roundtrip(tmp_path, lambda: build("Float32", 4, size=(48, 24, 6), coupled=True), 4, "coupled")
    assert "top_flux.T" in restart.read_checkpoint(path).names()


def test_bit_for_bit_direct_stencil_kernels(tmp_path):
    restart_roundtrip(tmp_path, lambda: build("Float32", 0, kernels=1), 4, "kernels1")


@pytest.mark.parametrize("float_type", ["Float32", "Float64"])
def test_checksums_heads_and_tails(tmp_path, float_type):
    """67 x 30 x 8: planes of 83 columns.  V, V_bar, Gn.V have 83 x 47 = 3901 elements, an odd count: a tail behind the last whole
    vector in both float types.  eta_bar, U_bar, V_bar are ONE allocation: U_bar starts 83 x 46 = 3818 elements behind eta_bar, in
    Float32 15272 bytes, 8 past a 16-byte boundary, while its place in the arena is on one: that member goes element by element,
    in the snapshot and in the restore.  Every member's s1, s2 in the file equal the numpy restatement."""
    m = build(float_type, 0, size=(67, 30, 8))
    gb.first_time_step(m)
    gb.loop(m, 2)
    want = state_of(m)
    path = m.checkpoint(str(tmp_path), "odd")
    c = restart.read_checkpoint(path)
    assert c["V"].size == 3901 and c["V"].size % 4 and c["V"].size % 2 and (c["eta_bar"].size * 4) % 16 == 8
    for n in c.names():
        assert restart.checksums(c[n]) == (c.table[n]["s1"], c.table[n]["s2"]), n
    for n in want:
        assert np.array_equal(bits(c[n]), bits(want[n])), n
    b = build(float_type, 0, size=(67, 30, 8))
    gb.restore(b, str(tmp_path), "odd")
    gb.loop(m, 2)
    gb.loop(b, 2)
    assert_same_bits(m, b, "odd shape")


def test_isolation_and_overlap(tmp_path):
    m = build("Float32", 1)
    gb.first_time_step(m)
    gb.loop(m, 3)
    want = state_of(m)
    clock = m.backend.clock()
    handle = m.checkpoint(str(tmp_path), "overlap", wait=False)
    gb.loop(m, 2)
    path = handle.write()
    assert m.backend.clock()[1] == clock[1] + 2
    c = restart.read_checkpoint(path)
    assert (c.time, c.iteration, c.last_dt) == (clock[0], clock[1], clock[2])
    for n in want:
        assert np.array_equal(bits(c[n]), bits(want[n])), n
    after = state_of(m)
    assert not np.array_equal(after["T"], want["T"])


@pytest.mark.parametrize("closure", [None, "catke"])
def test_one_launch(tmp_path, closure):
    m = build("Float32", 0, closure=gb.CATKEVerticalDiffusivity() if closure else None)
    gb.first_time_step(m)
    gb.loop(m, 2)
    b = m.backend
    b.checkpoint_snapshot()        # (the first snapshot allocates)
    b.checkpoint_write(str(tmp_path), "warm")
    b.synchronize()
    b.profile_enable(True)
    b.profile_reset()
    before = b.profile_get("diagnostics")[0]
    b.checkpoint_snapshot()
    info = b.checkpoint_info()
    path = b.checkpoint_write(str(tmp_path), "one")
    b.synchronize()
    assert b.profile_get("diagnostics")[0] - before == 1
    b.profile_enable(False)
    names = restart.read_checkpoint(path).names()
    # (21 fields -- pHY' is stale inside a loop --, CATKE's 10, and whatever look-aheads were valid)
    assert info.pieces == 1 and info.members == len(names) >= (31 if closure else 21) and len(names) > 21


def test_bounded_arena(tmp_path):
    m = build("Float32", 4)
    gb.first_time_step(m)
    gb.loop(m, 2)
    whole = open(m.checkpoint(str(tmp_path), "whole"), "rb").read()
    largest = max(a.nbytes for a in restart.read_checkpoint(os.path.join(str(tmp_path), "whole", "restart_rank0.gb25")).members.values())
    for label, cap in (("small", largest // 3), ("ragged", 100000)):
        m.backend.checkpoint_snapshot(cap)
        info = m.backend.checkpoint_info()
        assert info.pieces > 1 and info.arena_bytes <= cap
        assert open(m.backend.checkpoint_write(str(tmp_path), label), "rb").read() == whole, label
    b = build("Float32", 4)
    gb.restore(b, str(tmp_path), "ragged")
    gb.loop(m, 2)
    gb.loop(b, 2)
    assert_same_bits(m, b, "bounded arena")


def test_refusals(tmp_path):
    a = build("Float32", 1)
    gb.first_time_step(a)
    gb.loop(a, 2)
    with pytest.raises(GB25Error, match="no snapshot"):
        a.backend.checkpoint_write(str(tmp_path), "none")
    path = a.checkpoint(str(tmp_path), "good")
    a.backend.checkpoint_snapshot()
    with pytest.raises(GB25Error, match="waits to be written"):
        a.backend.checkpoint_snapshot()
    a.backend.checkpoint_release()
    # one byte of a member flipped
    c = restart.read_checkpoint(path)
    raw = bytearray(open(path, "rb").read())
    raw[c.table["S"]["offset"] + 1001] ^= 0x10
    os.makedirs(os.path.join(str(tmp_path), "flipped"))
    open(os.path.join(str(tmp_path), "flipped", "restart_rank0.gb25"), "wb").write(bytes(raw))
    b = build("Float32", 1)
    before = state_of(b)
    clock = b.backend.clock()
    with pytest.raises(GB25Error, match="status 5.*checksum mismatch in member S "):
        gb.restore(b, str(tmp_path), "flipped")
    after = state_of(b)
    assert all(np.array_equal(bits(before[n]), bits(after[n])) for n in before) and b.backend.clock() == clock
    # another Nz, another float type, CATKE on against off, another bottom
    Nx, Ny, Nz = size_of(1)
    with pytest.raises(GB25Error, match="status 5.*Nz 6 .file. / 7 .model."):
        gb.restore(build("Float32", 1, size=(Nx, Ny, Nz + 1)), str(tmp_path), "good")
    with pytest.raises(GB25Error, match="status 5.*Float32 numbers, this library steps Float64"):
        gb.restore(build("Float64", 1), str(tmp_path), "good")
    with pytest.raises(GB25Error, match="status 5.*CATKEVerticalDiffusivity.. is off in the file and on in the model"):
        gb.restore(build("Float32", 1, closure=gb.CATKEVerticalDiffusivity()), str(tmp_path), "good")
    zb = np.full((Nx, Ny), -3000.0)
    zb[10:14, 8:12] = -500.0
    with pytest.raises(GB25Error, match="status 5.*another grid"):
        gb.restore(build("Float32", 1, bottom=zb), str(tmp_path), "good")
    with pytest.raises(GB25Error, match="cannot read"):
        gb.restore(build("Float32", 1), str(tmp_path), "missing")
    # and the good file still restores
    gb.restore(b, str(tmp_path), "good")
    gb.loop(a, 2)
    gb.loop(b, 2)
    assert_same_bits(a, b, "after the refusals")


# 64 x 32 x 8 as two slabs; 48 x 24 x 6 tripolar with the islands as two slabs (each the other's fold partner); 64 x 32 x 8 as a
# 2 x 2 mesh.  Few substeps where the sub-cycle's wide halos (Ns + 1 + halo columns / rows) would not fit a rank otherwise.
DECOMPOSITIONS = {"two_slabs": dict(size=(64, 32, 8), P=2, ranks_y=1, grid_type=0, kw=dict()),
                  "tripolar_islands_two_slabs": dict(size=(48, 24, 6), P=2, ranks_y=1, grid_type=4, kw=dict(substeps=2)),
                  "mesh_2x2": dict(size=(64, 32, 8), P=4, ranks_y=2, grid_type=0, kw=dict(substeps=2))}


@pytest.mark.parametrize("case", sorted(DECOMPOSITIONS))
def test_decompositions(tmp_path, case):
    from gb25_amd.distributed import LocalSlabEnsemble
    c = DECOMPOSITIONS[case]
    (Nx, Ny, Nz), dt = c["size"], 60.0 if c["grid_type"] == 4 else 600.0
    single = build("Float32", c["grid_type"], size=c["size"])
    init = {n: single.backend.get_field(n, False) for n in ("u", "v", "T", "S", "eta")}

    def make():
        return LocalSlabEnsemble(Nx, Ny, Nz, c["P"], dt=dt, ranks_y=c["ranks_y"], grid_type=c["grid_type"], **c["kw"])
    a, b = make(), make()
    for n, x in init.items():
        a.scatter(n, x)
    a.first_time_step()
    a.loop(2)
    paths = a.checkpoint(str(tmp_path), case)
    assert [os.path.basename(p) for p in paths] == [f"restart_rank{r}.gb25" for r in range(c["P"])]
    b.restore(str(tmp_path), case)
    a.loop(3)
    b.loop(3)
    for r, (ba, bb) in enumerate(zip(a.backends, b.backends)):
        assert ba.clock() == bb.clock()
        for n in FIELD_IDS:
            if FIELD_IDS[n] < FIELD_IDS["e"]:
                assert np.array_equal(bits(ba.get_field(n, True)), bits(bb.get_field(n, True))), (case, r, n)
    # another decomposition than the one that wrote the files is refused, and named
    other = LocalSlabEnsemble(2 * Nx, Ny, Nz, 2 * c["P"], dt=dt, ranks_y=c["ranks_y"], grid_type=c["grid_type"], **c["kw"])
    with pytest.raises(GB25Error, match="status 5.*another decomposition"):
        other.backends[0].restore(str(tmp_path), case)


def test_a_dropped_snapshot_is_released(tmp_path):
    m = build("Float32", 0)
    handle = m.checkpoint(str(tmp_path), "dropped", wait=False)
    handle.release()
    assert m.backend.checkpoint_info().taken == 0
    assert os.path.exists(m.checkpoint(str(tmp_path), "kept"))


def test_the_oracle_backend_says_so(tmp_path):
    from helpers import make_oracle
    with pytest.raises(NotImplementedError, match="HIP backend"):
        make_oracle(64, 32, 8, dt=600.0).checkpoint(str(tmp_path))
