"""The forms of the split-explicit sub-cycle (csrc/subcycle_plan.hpp, DESIGN.md "The forms of the sub-cycle") against each other:
the blocked launches of 3, 5 and 7 substeps, one launch per substep, the one-launch path of a short sub-cycle with its finalize,
and the whole sub-cycle of a narrow slab in one launch.  Only options that every build has: the same file checks the host code
before and after it is rearranged."""
import numpy as np
import pytest

import gb25_amd as gb
from gb25_amd.distributed import LocalSlabEnsemble
from helpers import ALL_FIELDS, counter_rng, set_noisy_velocities

pytestmark = pytest.mark.gpu


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    n = max(np.linalg.norm(a.ravel()), np.linalg.norm(b.ravel()))
    return 0.0 if n == 0 else float(np.linalg.norm((a - b).ravel()) / n)


def stepped(size, steps=3, grid_type="simple_lat_lon", substeps=30, dt=600.0, amplitude=0.05, **options):
    """Noisy velocities and a non-zero eta, first_time_step, then a loop of `steps`; every parent array, halos included."""
    Nx, Ny, Nz = size
    m = gb.baroclinic_instability_model(gb.GPU(), Nx, Ny, Nz, dt=dt, grid_type=grid_type, substeps=substeps,
                                        options=dict(options, w_on_the_fly=0))
    for k, v in options.items():
        assert m.backend.get_option(k) == v
    gb.set_baroclinic_instability(m)
    set_noisy_velocities(m, amplitude)
    m.set(eta=(1e-2 * counter_rng((Nx, Ny, 1), 42, 3)).astype(np.float32))
    gb.first_time_step(m)
    gb.loop(m, steps)
    assert m.clock.iteration == steps + 1
    out = {n: m.backend.get_field(n, True) for n in ALL_FIELDS}
    assert all(np.isfinite(a).all() for a in out.values())
    assert np.abs(out["eta"]).max() > 0 and np.abs(out["U"]).max() > 0
    return out, m.backend.substepping()[0]


@pytest.mark.parametrize("lookahead", [{}, dict(subcycle_lookahead=0)], ids=["default", "in_step"])
def test_blocked_launches_of_3_5_and_7_substeps_give_equal_bits(lookahead):
    """150 x 70: ragged tiles in both directions (150 = 2 * 64 + 22, 70 = 4 * 17 + 2 = 4 * 16 + 6)."""
    runs = {blk: stepped((150, 70, 6), subcycle_block=blk, **lookahead)[0] for blk in (5, 3, 7)}
    for blk in (3, 7):
        for n in ALL_FIELDS:
            assert np.array_equal(runs[5][n], runs[blk][n]), (blk, n, rel(runs[5][n], runs[blk][n]))


@pytest.mark.parametrize("grid_type,dt,amplitude", [("lat_lon_as_curvilinear", 600.0, 0.05), ("gaussian_islands", 60.0, 1e-2)])
def test_curvilinear_blocked_equals_one_launch_per_substep(grid_type, dt, amplitude):
    """k_barotropic_substep_curv and k_barotropic_multi_curv are compiled without contraction so that they are interchangeable bit
    for bit (the comment above the former): canonical arrays without the fold, the tall arrays with it (the tripolar grid with
    islands: without land the poles do not survive four steps).  Every parent array, halos included -- but for the halo cells of
    the filtered state on the folded grid, which nothing reads: one launch per substep publishes the averages with a copy of
    whole columns, image rows beyond the fold included, the last blocked launch writes the rows [0, Ny) only (measured before
    the host code was rearranged: the three arrays differ there by 0.41 .. 0.50 norm-wise, their interiors and every other
    array are equal)."""
    one, _ = stepped((48, 24, 6), grid_type=grid_type, dt=dt, amplitude=amplitude, subcycle_block=1)
    five, _ = stepped((48, 24, 6), grid_type=grid_type, dt=dt, amplitude=amplitude, subcycle_block=5)
    H = 8
    for n in ALL_FIELDS:
        a, b = one[n], five[n]
        if grid_type == "gaussian_islands" and n in ("eta_bar", "U_bar", "V_bar"):
            a, b = a[H:-H, H:-H], b[H:-H, H:-H]
        assert np.array_equal(a, b), (grid_type, n, rel(a, b))


@pytest.mark.parametrize("lookahead", [{}, dict(subcycle_lookahead=0)], ids=["default", "in_step"])
def test_a_subcycle_of_one_launch_with_its_finalize(lookahead):
    """substeps = 6 leaves 4 effective substeps: one blocked launch that is first and, into the partner buffers of the look-ahead,
    also last; inside its own step it is not last and k_barotropic_finalize follows.  Against one launch per substep, to the
    round-off of test_schedule_options_are_bitwise_neutral (that kernel divides where the blocked one multiplies by reciprocals)."""
    five, Ns = stepped((150, 70, 6), substeps=6, subcycle_block=5, **lookahead)
    one, _ = stepped((150, 70, 6), substeps=6, subcycle_block=1, **lookahead)
    assert 1 <= Ns <= 5
    for n in ALL_FIELDS:
        print(f"  Ns {Ns} {n}: rel {rel(five[n], one[n]):.3e}")
    for n in ALL_FIELDS:
        assert rel(five[n], one[n]) < 2e-5, (n, rel(five[n], one[n]))


def test_the_whole_subcycle_of_a_narrow_slab_in_one_launch():
    """Two slabs of 64 columns: 2 x 3 tiles of the widened range, far fewer than the chip has CUs -- k_barotropic_whole (option
    subcycle_whole, the default) against the blocked launches on the same wide arrays; every parent array of every slab."""
    Nx, Ny, Nz, P = 128, 48, 6, 2
    single = gb.baroclinic_instability_model(gb.GPU(), Nx, Ny, Nz, dt=600.0)
    gb.set_baroclinic_instability(single)
    init = {n: single.backend.get_field(n, False) for n in ("T", "S")}
    init["u"] = (1e-2 * counter_rng((Nx, Ny, Nz), 42, 1)).astype(np.float32)
    init["v"] = (1e-2 * counter_rng((Nx, Ny + 1, Nz), 42, 2)).astype(np.float32)
    init["eta"] = (1e-2 * counter_rng((Nx, Ny, 1), 42, 3)).astype(np.float32)
    runs = []
    for whole in (1, 0):
        ens = LocalSlabEnsemble(Nx, Ny, Nz, P, dt=600.0, slab_mode=1, options=dict(subcycle_whole=whole, w_on_the_fly=0))
        assert all(b.get_option("subcycle_whole") == whole and b.substepping()[0] == 21 for b in ens.backends)
        for n, a in init.items():
            ens.scatter(n, a)
        ens.first_time_step()
        ens.loop(3)
        runs.append([{n: b.get_field(n, True) for n in ALL_FIELDS} for b in ens.backends])
        ens.close()
    assert np.abs(runs[0][0]["U"]).max() > 0
    for r in range(P):
        for n in ALL_FIELDS:
            assert np.array_equal(runs[0][r][n], runs[1][r][n]), (r, n, rel(runs[0][r][n], runs[1][r][n]))
