"""How many timed scopes a short run opens for the halo fills, w and the hydrostatic pressure (csrc/launch_plan.hpp and the three
helpers that issue its plans): first_time_step + loop(4) of a small model with the profile on, counted by gb25_profile_get.  A request
that silently became two scopes, or none, changes a count."""
import pytest

from gb25_amd.binding import HipBackend
from gb25_amd.distributed import LocalSlabEnsemble

pytestmark = pytest.mark.gpu

SIZE, DT = (64, 32, 8), 600.0
MODELS = {
    "walled": lambda: [HipBackend(*SIZE, dt=DT)],
    "folded": lambda: [HipBackend(*SIZE, dt=DT, grid_type=4)],                     # the tripolar grid with its islands: a zipper fold
    "self_ring": lambda: LocalSlabEnsemble(*SIZE, 1, dt=DT, slab_mode=1).backends,  # a slab that is its own neighbour
}
# (fill_halos, compute_w, compute_p) scopes: measured ONCE with this very function on the library of the commit before
# launch_plan.hpp (positional fill_halos_impl / compute_w_impl / compute_p_impl); exact, no margin
EXPECTED = {
    "walled": (5, 6, 6),
    "folded": (11, 6, 6),
    "self_ring": (8, 3, 11),
}


def scopes(name):
    backends = MODELS[name]()
    b = backends[0]
    try:
        b.set_baroclinic_instability()
        b.profile_enable(True)
        b.first_time_step()
        b.loop(4)
        return tuple(b.profile_get(k)[0] for k in ("fill_halos", "compute_w", "compute_p"))
    finally:
        for x in backends:
            x.close()


@pytest.mark.parametrize("name", list(MODELS))
def test_the_scopes_of_five_steps_on(name):
    assert scopes(name) == EXPECTED[name]
