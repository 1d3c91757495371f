"""Which kernel corrects u, v in a step -- the route of DESIGN.md, "Which kernel corrects u, v: the route of a step" -- and what the
calls that interrupt a route do, pinned through the library's launch counters.  Every case runs the same sequence of calls; after
each call the cumulative launch counts of the kernels a route adds or removes equal a table of literals.  The table was measured
with this very test on the libraries of commit 90c3ca2 (the parent of the change that gave the routes one owner, StepRoute), not on
the code that change left: a launch that moved, doubled or went missing on any route shows here as a changed count.

A wrong route crashes nothing: it gives plausible velocities or a stale w.  So beside the counts, wherever the routes promise the
same bits -- the corrector inside its consumers with w from the stand-alone kernel against the sweep, the corrector through the
tracer kernel against the sweep with w on the fly -- every parent array equals the sweeping model's, halos included; elsewhere (w
carried inside the tendency kernels: another association of the vertical sum) the criterion of
tests/test_gpu_parity.py::test_w_on_the_fly_agrees_to_round_off holds, with its tolerance."""
import functools

import numpy as np
import pytest

import gb25_amd as gb
from gb25_amd.binding import KERNEL_IDS
from gb25_amd.distributed import LocalSlabEnsemble
from helpers import ALL_FIELDS, counter_rng, set_noisy_velocities

pytestmark = pytest.mark.gpu

COUNTED = ("compute_w", "corrector", "fill_halos", "tracers", "gu", "ab2_velocities", "barotropic")
SLAB_FIELDS = ["u", "v", "w", "T", "S", "eta", "U", "V", "eta_bar", "U_bar", "V_bar", "Gn.u", "Gn.v", "Gn.T", "Gn.S", "Gm.u", "Gm.v", "pHY"]
EPS32 = float(np.finfo(np.float32).eps)
FLAT = dict(shape=(150, 70, 24), dt=300.0, noise=0.05)     # 24 levels: two chunks of 12, a chunk boundary for k_w_bases to get wrong
ISLANDS = dict(FLAT, grid_type="gaussian_islands_lat_lon")
FOLDED = dict(shape=(72, 36, 12), dt=600.0, noise=1e-2, grid_type="gaussian_islands")   # (tests/test_gpu_tripolar.py runs the look-aheads there)

# id -> how the model is made.  fly: the value of w_on_the_fly the model starts with (the sequence switches to the other one).
RUNS = {
    # the smallest shape at which the parity tests run the look-aheads
    "sweep": dict(shape=(40, 21, 6), halo=4, dt=300.0, noise=0.05, fly=0, options=dict(lazy_corrector=0)),
    "sweep_wfly": dict(FLAT, fly=1, options=dict(lazy_corrector=0)),
    "in_consumers_w_kernel": dict(FLAT, fly=0, options={}),
    "in_consumers_wfly": dict(FLAT, fly=1, options={}),
    "through_tracers_islands": dict(ISLANDS, fly=1, options={}),
    "through_tracers_folded": dict(FOLDED, fly=1, options={}),
    "slabs_w_kernel": dict(slabs=(384, 48, 36, 2, 1), fly=0),      # (as test_w_on_the_fly_on_slabs)
    "slabs_wfly": dict(slabs=(384, 48, 36, 2, 1), fly=1),
    "mesh_w_kernel": dict(slabs=(256, 96, 36, 4, 2), fly=0),       # (as test_w_on_the_fly_on_a_mesh)
    "mesh_wfly": dict(slabs=(256, 96, 36, 4, 2), fly=1),
    # the sweeping models the cases above are compared with (no row in the table)
    "ref_flat_sweep": dict(FLAT, fly=0, options=dict(lazy_corrector=0)),
    "ref_islands_sweep_wfly": dict(ISLANDS, fly=1, options=dict(lazy_corrector=0)),
    "ref_folded_sweep_wfly": dict(FOLDED, fly=1, options=dict(lazy_corrector=0)),
}
# case -> (the run it is compared with, the same bits?)
COMPARED = {
    "sweep_wfly": ("ref_flat_sweep", False),
    "in_consumers_w_kernel": ("ref_flat_sweep", True),
    "in_consumers_wfly": ("ref_flat_sweep", False),
    "through_tracers_islands": ("ref_islands_sweep_wfly", True),
    "through_tracers_folded": ("ref_folded_sweep_wfly", True),
    "slabs_wfly": ("slabs_w_kernel", False),
    "mesh_wfly": ("mesh_w_kernel", False),
}
CALLS = ("first_time_step", "loop(3)", "time_step", "get_field(u)", "loop(2)", "set_option(w_on_the_fly)", "loop(2)",
         "field_device_ptr(T)", "loop(2)")
# Cumulative launch counts (COUNTED, in that order; summed over the ranks of a decomposition) after each of CALLS.
TABLE = {
    "sweep": [
        (2, 1, 3, 2, 2, 1, 2),
        (5, 4, 5, 5, 5, 1, 5),
        (6, 5, 5, 6, 6, 1, 6),
        (6, 5, 5, 6, 6, 1, 6),
        (8, 7, 5, 8, 8, 1, 8),
        (8, 7, 5, 8, 8, 1, 8),
        (10, 9, 6, 10, 10, 2, 11),
        (10, 9, 6, 10, 10, 2, 11),
        (12, 11, 8, 12, 12, 4, 13)],
    "sweep_wfly": [
        (2, 1, 3, 2, 2, 1, 2),
        (4, 4, 5, 5, 5, 1, 5),
        (5, 5, 5, 6, 6, 1, 6),
        (5, 5, 5, 6, 6, 1, 6),
        (6, 7, 5, 8, 8, 1, 8),
        (6, 7, 5, 8, 8, 1, 8),
        (8, 9, 6, 10, 10, 2, 11),
        (8, 9, 6, 10, 10, 2, 11),
        (10, 11, 8, 12, 12, 4, 13)],
    "in_consumers_w_kernel": [
        (2, 1, 3, 2, 2, 1, 2),
        (5, 4, 5, 5, 5, 1, 5),
        (6, 5, 5, 6, 6, 1, 6),
        (6, 5, 5, 6, 6, 1, 6),
        (8, 7, 5, 8, 8, 1, 8),
        (8, 7, 5, 8, 8, 1, 8),
        (10, 9, 6, 10, 10, 2, 11),
        (10, 9, 6, 10, 10, 2, 11),
        (12, 11, 8, 12, 12, 4, 13)],
    "in_consumers_wfly": [
        (2, 1, 3, 2, 2, 1, 2),
        (4, 4, 5, 5, 5, 1, 5),
        (5, 5, 5, 6, 6, 1, 6),
        (5, 5, 5, 6, 6, 1, 6),
        (6, 7, 5, 8, 8, 1, 8),
        (6, 7, 5, 8, 8, 1, 8),
        (8, 9, 6, 10, 10, 2, 11),
        (8, 9, 6, 10, 10, 2, 11),
        (10, 11, 8, 12, 12, 4, 13)],
    "through_tracers_islands": [
        (2, 1, 3, 2, 2, 1, 2),
        (4, 4, 8, 5, 5, 1, 5),
        (5, 5, 10, 6, 6, 1, 6),
        (5, 5, 10, 6, 6, 1, 6),
        (6, 7, 14, 8, 8, 1, 8),
        (6, 7, 14, 8, 8, 1, 8),
        (8, 9, 15, 10, 10, 2, 11),
        (8, 9, 15, 10, 10, 2, 11),
        (10, 11, 17, 12, 12, 4, 13)],
    "through_tracers_folded": [
        (2, 1, 3, 2, 2, 1, 2),
        (4, 4, 11, 5, 5, 1, 5),
        (5, 5, 14, 6, 6, 1, 6),
        (5, 5, 14, 6, 6, 1, 6),
        (6, 7, 20, 8, 8, 1, 8),
        (6, 7, 20, 8, 8, 1, 8),
        (8, 9, 24, 10, 10, 2, 11),
        (8, 9, 24, 10, 10, 2, 11),
        (10, 11, 28, 12, 12, 4, 13)],
    "slabs_w_kernel": [
        (6, 4, 10, 4, 6, 2, 4),
        (18, 10, 16, 10, 18, 2, 10),
        (22, 12, 18, 12, 22, 2, 12),
        (22, 12, 18, 12, 22, 2, 12),
        (30, 16, 22, 16, 30, 2, 16),
        (30, 16, 22, 16, 30, 2, 16),
        (36, 22, 30, 20, 38, 4, 22),
        (36, 22, 30, 20, 38, 4, 22),
        (44, 30, 42, 24, 46, 8, 26)],
    "slabs_wfly": [
        (6, 4, 10, 4, 6, 2, 4),
        (8, 10, 16, 10, 18, 2, 10),
        (10, 12, 18, 12, 22, 2, 12),
        (10, 12, 18, 12, 22, 2, 12),
        (12, 16, 22, 16, 30, 2, 16),
        (12, 16, 22, 16, 30, 2, 16),
        (20, 22, 30, 20, 38, 4, 22),
        (20, 22, 30, 20, 38, 4, 22),
        (28, 30, 42, 24, 46, 8, 26)],
    "mesh_w_kernel": [
        (8, 8, 24, 8, 8, 4, 8),
        (20, 20, 60, 20, 20, 4, 20),
        (24, 24, 72, 24, 24, 4, 24),
        (24, 24, 72, 24, 24, 4, 24),
        (32, 32, 96, 32, 32, 4, 32),
        (32, 32, 96, 32, 32, 4, 32),
        (40, 44, 124, 40, 40, 8, 44),
        (40, 44, 124, 40, 40, 8, 44),
        (48, 60, 148, 48, 48, 16, 52)],
    "mesh_wfly": [
        (8, 8, 24, 8, 8, 4, 8),
        (12, 20, 60, 20, 20, 4, 20),
        (16, 24, 72, 24, 24, 4, 24),
        (16, 24, 72, 24, 24, 4, 24),
        (20, 32, 96, 32, 32, 4, 32),
        (20, 32, 96, 32, 32, 4, 32),
        (28, 44, 124, 40, 40, 8, 44),
        (28, 44, 124, 40, 40, 8, 44),
        (36, 60, 148, 48, 48, 16, 52)],
}


class Single:
    def __init__(self, shape, dt, noise, fly, options, halo=8, grid_type="simple_lat_lon"):
        self.m = gb.baroclinic_instability_model(gb.GPU(), *shape, dt=dt, halo=(halo,) * 3, grid_type=grid_type,
                                                 options=dict(options, subcycle_lookahead=1, w_on_the_fly=fly))
        gb.set_baroclinic_instability(self.m)
        set_noisy_velocities(self.m, noise)
        self.backends = [self.m.backend]
        self.first_time_step = lambda: gb.first_time_step(self.m)
        self.time_step = lambda: gb.time_step(self.m)
        self.loop = lambda n: gb.loop(self.m, n)

    def fields(self):
        return {n: self.m.backend.get_field(n, True) for n in ALL_FIELDS}

    def close(self):
        self.m.backend.close()


class Slabs(LocalSlabEnsemble):
    def __init__(self, Nx, Ny, Nz, P, Ry, fly):
        super().__init__(Nx, Ny, Nz, P, dt=600.0, ranks_y=Ry, options=dict(subcycle_lookahead=1, w_on_the_fly=fly))
        single = gb.baroclinic_instability_model(gb.GPU(), Nx, Ny, Nz, dt=600.0)
        gb.set_baroclinic_instability(single)
        single.set(u=(1e-2 * counter_rng((Nx, Ny, Nz), 42, 1)).astype(np.float32),
                   v=(1e-2 * counter_rng((Nx, Ny + 1, Nz), 42, 2)).astype(np.float32),
                   eta=(1e-2 * counter_rng((Nx, Ny, 1), 42, 3)).astype(np.float32))
        for n in ("u", "v", "T", "S", "eta"):
            self.scatter(n, single.backend.get_field(n, False))
        single.backend.close()

    def fields(self):
        return {n: self.gather(n) for n in SLAB_FIELDS}


@functools.lru_cache(maxsize=None)
def run(name):
    """The sequence on one model: (the counts after every call, the fields before the option changes, the fields at the end)."""
    kw = dict(RUNS[name])
    fly = kw["fly"]
    x = Slabs(*kw["slabs"], fly) if "slabs" in kw else Single(**kw)
    for b in x.backends:
        b.profile_enable(True)
    counts, before = [], None

    def ready():
        return all(b.lookahead_state()[0] for b in x.backends)

    def count():
        counts.append(tuple(sum(b.profile_get(k)[0] for b in x.backends) for k in KERNEL_IDS))

    x.first_time_step(); count()
    x.loop(3); count()
    x.time_step(); count()
    for b in x.backends:
        b.get_field("u", True)
    count()
    x.loop(2); count()
    assert ready(), name
    before = x.fields()
    x.set_option("w_on_the_fly", 1 - fly) if "slabs" in kw else x.m.backend.set_option("w_on_the_fly", 1 - fly)
    count()
    x.loop(2); count()
    assert ready(), name
    for b in x.backends:
        b.field_device_ptr("T")
    count()
    assert not any(b.lookahead_state()[0] for b in x.backends), name       # no look-ahead ever again
    x.loop(2); count()
    assert not any(b.lookahead_state()[0] for b in x.backends), name
    end = x.fields()
    x.close()
    return counts, before, end


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    n = max(np.linalg.norm(a.ravel()), np.linalg.norm(b.ravel()))
    return 0.0 if n == 0 else float(np.linalg.norm((a - b).ravel()) / n)


@pytest.mark.parametrize("name", [n for n in RUNS if not n.startswith("ref_")])
def test_route_launches_and_state(name):
    counts, before, end = run(name)
    ids = [list(KERNEL_IDS).index(k) for k in COUNTED]
    got = [tuple(c[i] for i in ids) for c in counts]
    print(f'\n    "{name}": [' + ", ".join(str(g) for g in got) + "],")
    other, same_bits = COMPARED.get(name, (None, False))
    worst = {}
    if other:
        _, obefore, oend = run(other)
        if same_bits:
            print("   ", name, "bits before:", [n for n in before if not np.array_equal(before[n], obefore[n])],
                  "at the end:", [n for n in end if not np.array_equal(end[n], oend[n])])
        worst = {n: rel(end[n], oend[n]) for n in end}
        print("   ", name, "rel at the end:", {n: f"{v:.2e}" for n, v in worst.items()})
    assert len(got) == len(CALLS)
    for call, g, want in zip(CALLS, got, TABLE[name]):
        assert g == want, (name, call, dict(zip(COUNTED, g)), dict(zip(COUNTED, want)))
    # once a pointer is out the model sweeps and computes w in every step, whatever its route was
    last = dict(zip(COUNTED, (a - b for a, b in zip(got[8], got[7]))))
    n_ranks = RUNS[name]["slabs"][3] if "slabs" in RUNS[name] else 1
    assert last["tracers"] == 2 * n_ranks and last["gu"] >= 2 * n_ranks and last["compute_w"] >= 2 * n_ranks, last
    if other and same_bits:
        for n in before:     # u, v and w as memory holds them when the call returns: corrected, and the w of the last step
            assert np.array_equal(before[n], obefore[n]), (name, "before the option changes", n)
    if name.startswith("through_tracers"):
        for n in end:        # (without w on the fly both models sweep: the same kernels on the same bits)
            assert np.array_equal(end[n], oend[n]), (name, "at the end", n)
    elif other:
        for n, v in worst.items():
            assert v < (200 if n == "w" else 2000) * EPS32, (name, n, v)
    u = end["u"]
    assert np.isfinite(u).all() and np.abs(u).max() > 0
