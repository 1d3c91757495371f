"""Passive tracers carried beside a run (gb25_tracers_*): the fused update against its numpy restatement bit for bit
(gb-25_amd/passive.py, pinned on the CPU by tests/test_passive_host.py), the tendency against the oracle's G.T for T := c, a dye that
starts as T against T, constants, conservation, ideal age, the proof that the run beside them is untouched, the refusals and the
memory."""
import ctypes as C
import functools

import numpy as np
import pytest

import gb25_amd as gb
from gb25_amd.binding import HipBackend, TracerSpec
from gb25_amd.integrals import cell_measure
from gb25_amd.passive import PassiveTracers, kbot_interior, passive_update_host
from helpers import BASE_FIELDS, GRID_NAMES, SQRT_EPS64, counter_rng, make_oracle, set_noisy_velocities, stepped_model

pytestmark = pytest.mark.gpu
INVALID, STATE = 1, 5
H = 8
# lat-lon, lat-lon with islands, tripolar, tripolar with islands (the smallest size tests/test_gpu_tripolar.py steps)
SIZES = {0: (32, 24, 8), 1: (48, 24, 6), 3: (72, 36, 8), 4: (72, 36, 8)}
DT = {0: 600.0, 1: 600.0, 3: 60.0, 4: 60.0}
FOLDED = (3, 4)
CASES = [(ft, gt) for ft in ("Float32", "Float64") for gt in SIZES]


def fresh_model(float_type, grid_type, order=5, **options):
    """The baroclinic-instability state with noisy velocities at iteration 0."""
    Nx, Ny, Nz = SIZES[grid_type]
    m = gb.baroclinic_instability_model(gb.GPU(float_type=float_type), Nx, Ny, Nz, dt=DT[grid_type], grid_type=GRID_NAMES[grid_type],
                                        options=options or None)
    if order != 5:
        m.backend.set_tracer_advection_order(order)
    gb.set_baroclinic_instability(m)
    set_noisy_velocities(m, 1e-2)
    return m


def smooth_plus_noise(shape, seed):
    i, j, k = np.meshgrid(*(np.arange(n) for n in shape), indexing="ij")
    return (1.0 + 0.5 * np.sin(2 * np.pi * i / shape[0]) * np.cos(np.pi * j / shape[1]) + 0.1 * k / shape[2]
            + 0.05 * (counter_rng(shape, seed, 1) - 0.5))


# ---- 1. the update, bit for bit
@pytest.mark.parametrize("float_type,grid_type", CASES)
def test_the_update_bit_for_bit(float_type, grid_type):
    m = stepped_model(float_type, grid_type, steps=1, size=SIZES[grid_type], dt=DT[grid_type])
    b = m.backend
    shape = b.field_dims("T", False)
    specs = [TracerSpec(0.0, 0.0, 0, 0), TracerSpec(-1e-4, 0.0, 0, 1), TracerSpec(1.0, 0.0, 1, 0), TracerSpec(0.25, 3.5, 1, 0)]
    tr = PassiveTracers(m, specs)
    kbot, fold = kbot_interior(b), grid_type in FOLDED
    assert (kbot is not None) == (grid_type in (1, 4))
    dt, chi = b.clock()[2], b.cfg.chi
    for n in range(4):
        before = tr.get(n, True)
        assert not before.any()
        field = (smooth_plus_noise(shape, 3 + n) - (1.0 if n == 1 else 0.0)).astype(b.dtype)   # (tracer 1: negative values to clip)
        tr.set(n, field)
        full = before.copy()
        full[H:-H, H:-H, H:-H] = field
        want = passive_update_host(full, None, None, dt, chi, H, kbot=kbot, fold=fold, update=False)
        assert tr.get(n, True).tobytes() == want.tobytes(), ("as set", n)
    for step, euler in enumerate((True, False, False)):
        c0 = [tr.get(n, True) for n in range(4)]
        tr.advance()
        for n, sp in enumerate(specs):
            Gn, Gm = tr.tendency(n, "Gn", True), tr.tendency(n, "Gm", True)
            assert Gn[H:-H, H:-H, H:-H].any() and (step == 0) == (not Gm.any())
            want = passive_update_host(c0[n], Gn, Gm, dt, chi, H, euler=euler, source=sp.source, surface_value=sp.surface_value,
                                       surface_reset=bool(sp.surface_reset), clip_negative=bool(sp.clip_negative), kbot=kbot, fold=fold)
            got = tr.get(n, True)
            assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (float_type, grid_type, step, n, np.argwhere(got != want)[:4])
            assert np.array_equal(Gn[:H], np.zeros_like(Gn[:H])), "the tendency has no halo cells"
        assert (tr.get(1) >= 0).all() and (tr.get(3)[:, :, -1][(kbot if kbot is not None else np.zeros(shape[:2])) < shape[2]] == 3.5).all()
        assert tr.clock()[1] == b.clock()[1] + 1 and tr.clock()[0] > b.clock()[0]
        b.time_step()
    tr.close()
    b.close()


# ---- 2. the tendency against the oracle
@pytest.mark.parametrize("grid_type,order", [(0, 5), (1, 5), (3, 5), (4, 5), (0, 7), (4, 7)])
def test_the_tendency_against_the_oracle(grid_type, order):
    """Float64.  The oracle gets T := c (the parent the device holds, halo cells as the device made them) and the device's u, v, w;
    its fill must leave that parent as it is (the halo rule is the oracle's), its G.T is the reference.  Element-wise: every
    |difference| within sqrt(eps) of the largest |G| -- a tendency is a difference of fluxes, so the error of a cell scales with
    the fluxes, not with what is left of them."""
    Nx, Ny, Nz = SIZES[grid_type]
    m = fresh_model("Float64", grid_type, order)
    gb.first_time_step(m)
    gb.loop(m, 2)
    b = m.backend
    tr = gb.passive_tracers(m, dye=1)
    tr.set(0, smooth_plus_noise((Nx, Ny, Nz), 9))
    c = tr.get(0, True)
    v = make_oracle(Nx, Ny, Nz, DT[grid_type], grid_type=GRID_NAMES[grid_type])
    if order != 5:
        v.backend.set_tracer_advection_order(order)
    for n in ("u", "v", "w", "S"):
        v.backend.set_field(n, b.get_field(n, True), True)
    v.backend.set_field("T", c, True)
    v.backend.fill_halo_regions()
    filled = v.backend.get_field("T", True)
    assert np.array_equal(filled, c), ("the halo cells are the oracle's", np.argwhere(filled != c)[:4])
    v.backend.compute_tendencies()
    want = v.backend.get_field("Gn.T", False)
    tr.advance()
    got = tr.tendency(0)
    scale = np.abs(want).max()
    worst = np.abs(got - want).max()
    print(f"  grid {grid_type} order {order}: max |G| = {scale:.3e}, worst difference {worst:.3e} = {worst / scale:.2e} of it")
    assert scale > 0 and worst <= SQRT_EPS64 * scale
    tr.close()
    b.close()


# ---- 3. a dye that starts as T stays T to the last bits
@functools.lru_cache(maxsize=None)
def last_bits_of_T(float_type):
    """The project's own last bits: T after 6 steps with GB25_OPT_KERNELS = 1 against = 2, largest difference."""
    out = []
    for kernels in (1, 2):
        m = fresh_model(float_type, 0, kernels=kernels)
        gb.first_time_step(m)
        gb.loop(m, 5)
        out.append(np.asarray(m.backend.get_field("T", False), np.float64))
        m.backend.close()
    return float(np.abs(out[0] - out[1]).max())


@pytest.mark.parametrize("float_type", ["Float32", "Float64"])
def test_a_twin_of_T(float_type):
    m = fresh_model(float_type, 0)
    tr = gb.passive_tracers(m, dye=1)
    tr.set(0, m.backend.get_field("T", False))
    gb.run_with_tracers(m, tr, 6)
    assert m.backend.clock()[1] == 6 == tr.clock()[1]
    T = np.asarray(m.backend.get_field("T", False), np.float64)
    diff = float(np.abs(np.asarray(tr.get(0), np.float64) - T).max())
    yard = last_bits_of_T(float_type)
    print(f"  {float_type}: dye against T after 6 steps: {diff:.3e}; T with kernels = 1 against 2: {yard:.3e} (allowed: 4 x)")
    assert diff <= 4 * yard
    tr.close()
    m.backend.close()


# ---- 4., 5., 6.: ten steps with a constant, a patch and two ages beside a model whose S is uniform (the yardstick of the constant and
# of the ages) or the model's own (the yardstick of the conservation).  Not on the bare tripolar grid: its two northern poles are wet
# cells, and the model itself is non-finite there after six steps of this state (with the islands they are land).
S0 = 35.0
STEPS = 10
STEPPED = [(ft, gt) for ft in ("Float32", "Float64") for gt in (0, 1, 4)]


@functools.lru_cache(maxsize=None)
def ten_steps(float_type, grid_type, uniform_S=True):
    m = fresh_model(float_type, grid_type)
    b = m.backend
    Nx, Ny, Nz = shape = SIZES[grid_type]
    if uniform_S:
        b.set_field("S", np.full(shape, S0), False)
    specs = [TracerSpec(0.0, 0.0, 0, 0), TracerSpec(0.0, 0.0, 0, 0), TracerSpec(1.0, 0.0, 0, 0), TracerSpec(1.0, 0.0, 1, 0)]
    tr = PassiveTracers(m, specs, ["one", "patch", "age_free", "age"])
    tr.set("one", np.ones(shape))
    i, j, k = np.meshgrid(*(np.arange(n) for n in shape), indexing="ij")
    # compact: nothing of it within three rows of the walls in y, nor in the two top levels (the free surface moves through the upper
    # face of the top one, for T and S as for a dye)
    patch = np.exp(-(((i - Nx // 2) / 3.0) ** 2 + ((j - Ny // 2) / 1.5) ** 2 + ((k - (Nz // 2 - 1)) / 0.5) ** 2))
    patch[patch < 1e-6] = 0.0
    assert not patch[:, :3].any() and not patch[:, -3:].any() and not patch[:, :, -2:].any() and patch.any()
    tr.set("patch", patch)
    mu = cell_measure(b, "T")
    wet = mu > 0
    sums0 = (float((mu * np.asarray(b.get_field("S", False), np.float64)).sum()), tr.integral("patch"))
    dry_always_zero = True
    for _ in range(STEPS):
        gb.run_with_tracers(m, tr, 1)
        dry_always_zero &= all(not tr.get(n)[~wet].any() for n in range(4))
    S = np.asarray(b.get_field("S", False), np.float64)
    out = dict(wet=wet, dt=b.clock()[2], S_dev=float(np.abs(S[wet] / S0 - 1.0).max()),
               S_sum=(sums0[0], float((mu * S).sum())), patch_sum=(sums0[1], tr.integral("patch")), dry_always_zero=dry_always_zero,
               **{n: np.asarray(tr.get(n), np.float64) for n in tr.names})
    tr.close()
    b.close()
    return out


@pytest.mark.parametrize("float_type,grid_type", STEPPED)
def test_constants_stay_constant(float_type, grid_type):
    r = ten_steps(float_type, grid_type)
    dev = float(np.abs(r["one"][r["wet"]] - 1.0).max())
    print(f"  {float_type} grid {grid_type}: |c - 1| <= {dev:.3e}; the model's uniform S: |S / S0 - 1| <= {r['S_dev']:.3e} (allowed: 4 x)")
    assert dev <= 4 * r["S_dev"]
    assert r["dry_always_zero"]


@pytest.mark.parametrize("grid_type", [0, 1])
def test_conservation(grid_type):
    r = ten_steps("Float64", grid_type, uniform_S=False)
    rel = lambda ab: abs(ab[1] - ab[0]) / abs(ab[0])
    print(f"  grid {grid_type}: relative change of sum mu c: {rel(r['patch_sum']):.3e}; of sum mu S: {rel(r['S_sum']):.3e} (allowed: 4 x)")
    assert r["patch_sum"][0] > 0 and rel(r["patch_sum"]) <= 4 * rel(r["S_sum"])
    assert r["dry_always_zero"], "dry cells hold exactly 0 throughout"


@pytest.mark.parametrize("float_type,grid_type", STEPPED)
def test_ideal_age(float_type, grid_type):
    r = ten_steps(float_type, grid_type)
    wet, t = r["wet"], STEPS * r["dt"]
    free = r["age_free"]
    dev = float(np.abs(free[wet] - t).max())
    print(f"  {float_type} grid {grid_type}: |age - n dt| <= {dev:.3e} of n dt = {t}; allowed {4 * r['S_dev'] * t:.3e}")
    assert dev <= 4 * r["S_dev"] * t
    age = r["age"]
    assert not age[:, :, -1].any(), "the top level is exactly 0"
    below = age[:, :, :-1][wet[:, :, :-1]]
    assert (below > 0).all() and (below <= t * (1 + 1e-6)).all(), (below.min(), below.max(), t)


# ---- 7. the run is untouched
LOOKAHEADS = dict(subcycle_lookahead=1, ab2_lookahead=1)


@pytest.mark.parametrize("float_type,grid_type", [("Float32", 0), ("Float64", 4), ("Float32", 1)])
def test_the_run_is_untouched(float_type, grid_type):
    watched = stepped_model(float_type, grid_type, steps=0, **LOOKAHEADS)
    alone = stepped_model(float_type, grid_type, steps=0, **LOOKAHEADS)
    tr = gb.passive_tracers(watched, dye=2, age=True)
    tr.set(0, watched.backend.get_field("T", False))
    tr.set(1, lambda lam, phi, z: np.exp(-(phi / 20.0) ** 2) + 0 * lam + 0 * z)
    for step in range(6):
        before = watched.backend.lookahead_state()
        tr.advance()
        tr.stats(0)
        assert watched.backend.lookahead_state() == before == alone.backend.lookahead_state(), step
        for m in (watched, alone):
            gb.time_step(m)
    assert alone.backend.lookahead_state()[0], "the velocity look-ahead is on in this configuration"
    for name in BASE_FIELDS:
        assert np.array_equal(watched.backend.get_field(name, True), alone.backend.get_field(name, True), equal_nan=True), name
    assert tr.stats(2).max > 0 and tr.stats("age").nonfinite == 0
    tr.close()
    for m in (watched, alone):
        m.backend.close()


@pytest.mark.parametrize("float_type,grid_type", [("Float32", 0), ("Float64", 4)])
def test_run_with_tracers_from_the_start_leaves_the_run_alone(float_type, grid_type):
    """At iteration 0 run_with_tracers runs initialize and update_state ahead of the first advance; first_time_step runs them again."""
    watched, alone = fresh_model(float_type, grid_type), fresh_model(float_type, grid_type)
    tr = gb.passive_tracers(watched, dye=1, age=True)
    tr.set(0, np.ones(SIZES[grid_type]))
    gb.run_with_tracers(watched, tr, 4)
    gb.first_time_step(alone)
    for _ in range(3):
        gb.time_step(alone)
    assert watched.backend.lookahead_state() == alone.backend.lookahead_state()
    for name in BASE_FIELDS:
        assert np.array_equal(watched.backend.get_field(name, True), alone.backend.get_field(name, True), equal_nan=True), name
    tr.close()
    for m in (watched, alone):
        m.backend.close()


# ---- 8. refusals, the clock, the memory
def test_refusals_and_clock():
    m = stepped_model("Float32", 1, steps=1, size=SIZES[1])
    other = stepped_model("Float32", 0, steps=0, size=SIZES[0])
    b, lib, h = m.backend, m.backend.lib, m.backend.h
    err = lambda: lib.gb25_last_error_string(h).decode()
    spec = (TracerSpec * 9)()
    out = C.c_void_p()
    for count in (0, -1, 9):
        assert lib.gb25_tracers_begin(h, count, spec, C.byref(out)) == INVALID and "count" in err() and not out.value, count
    bad = (TracerSpec * 1)(TracerSpec(float("nan"), 0.0, 0, 0))
    assert lib.gb25_tracers_begin(h, 1, bad, C.byref(out)) == INVALID and "source" in err()
    tr = gb.passive_tracers(m, dye=1, age=True)
    tr.set(0, smooth_plus_noise(SIZES[1], 1))
    tr.advance()
    state = lambda: (tr.get(0, True).tobytes(), tr.get(1, True).tobytes(), tr.tendency(0, "Gn", True).tobytes(), tr.clock())
    fields = lambda: [b.get_field(n, True).tobytes() for n in ("u", "v", "w", "T", "S", "eta")]
    held, model_held, clock = state(), fields(), b.clock()
    # a second advance without a model step
    assert lib.gb25_tracers_advance(h, tr.handle) == STATE
    assert f"iteration {clock[1] + 1}" in err() and f"iteration {clock[1]}" in err()
    # a set of another model, tracer indices, which
    foreign = gb.passive_tracers(other, dye=1)
    buf = np.zeros(b.field_dims("T", True)[::-1], b.dtype)
    p = buf.ctypes.data_as(C.c_void_p)
    assert lib.gb25_tracers_advance(h, foreign.handle) == INVALID and "another model" in err()
    assert lib.gb25_tracers_get(h, foreign.handle, 0, 0, p, 1) == INVALID and lib.gb25_tracers_end(h, foreign.handle) == INVALID
    assert lib.gb25_tracers_get(h, tr.handle, 2, 0, p, 1) == INVALID and "tracer n" in err()
    assert lib.gb25_tracers_get(h, tr.handle, 0, 3, p, 1) == INVALID and "which" in err()
    assert lib.gb25_tracers_set(h, tr.handle, -1, p, 1) == INVALID
    # turning a closure on while a set exists
    assert lib.gb25_set_vertical_diffusivity(h, 1e-4, 1e-5) == STATE and "passive tracers" in err() and b.vertical_diffusivity() == (0.0, 0.0)
    assert lib.gb25_set_closure_catke(h, 1) == STATE and "passive tracers" in err()
    assert lib.gb25_set_vertical_diffusivity(h, 0.0, 0.0) == 0          # (closure = nothing stays allowed)
    assert state() == held and fields() == model_held and b.clock() == clock
    # the step makes the advance valid again
    b.time_step()
    tr.advance()
    assert tr.clock()[1] == b.clock()[1] + 1
    foreign.close()
    tr.close()
    assert lib.gb25_tracers_advance(h, tr.handle or C.c_void_p(1)) == INVALID
    # models that cannot carry tracers: a closure, a rank of a decomposition
    b.set_vertical_diffusivity(1e-4, 1e-5)
    assert lib.gb25_tracers_begin(h, 1, spec, C.byref(out)) == STATE and "closure = nothing" in err() and not out.value
    b.set_vertical_diffusivity(0.0, 0.0)
    b.set_catke(True)
    assert lib.gb25_tracers_begin(h, 1, spec, C.byref(out)) == STATE and "CATKE" in err() and not out.value
    ring = HipBackend(64, 32, 8, dt=600.0, slab_mode=1)
    assert ring.lib.gb25_tracers_begin(ring.h, 1, spec, C.byref(out)) == STATE and not out.value
    assert "decomposition" in ring.lib.gb25_last_error_string(ring.h).decode()
    for x in (ring, b, other.backend):
        x.close()


def test_nothing_leaks():
    import torch
    big = (256, 128, 16)     # (eight tracers: 24 arrays of 5 MB, more than the runtime keeps in hand)
    m = stepped_model("Float32", 0, steps=0, size=big)
    torch.cuda.synchronize()
    free = torch.cuda.mem_get_info()[0]
    need = 24 * (big[0] + 2 * H) * (big[1] + 2 * H) * (big[2] + 2 * H) * 4
    for life in range(2):
        tr = gb.passive_tracers(m, dye=8)
        tr.advance()
        assert free - torch.cuda.mem_get_info()[0] >= need // 2
        tr.close()
        assert torch.cuda.mem_get_info()[0] == free, life
    # sets the user forgot: destroy frees them.  A second life of the same model finds the memory the first one found
    m.backend.close()
    left = []
    for life in range(2):
        m = stepped_model("Float32", 0, steps=0, size=SIZES[0])
        for count in (3, 5):
            gb.passive_tracers(m, dye=count).advance()
        m.backend.close()
        torch.cuda.synchronize()
        left.append(torch.cuda.mem_get_info()[0])
    one_array = (SIZES[0][0] + 2 * H) * (SIZES[0][1] + 2 * H) * (SIZES[0][2] + 2 * H) * 4
    assert abs(left[0] - left[1]) < one_array, left
