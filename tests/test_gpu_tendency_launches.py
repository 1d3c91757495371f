"""How many timed scopes a short run opens for the tendency kernels, the barotropic corrector and the closure (csrc/tendency_plan.hpp
and the helpers that issue its plans): first_time_step + loop(4) of a small model with the profile on, counted by gb25_profile_get.  A
pass that silently ran twice, a corrector part that was dropped or a head that moved under another timer changes a count."""
import pytest

from gb25_amd.binding import HipBackend
from gb25_amd.distributed import LocalSlabEnsemble

pytestmark = pytest.mark.gpu

SIZE, DT = (64, 32, 8), 600.0


def catke_model():
    b = HipBackend(*SIZE, dt=DT)
    b.set_catke(True)
    return [b]


MODELS = {
    "walled": lambda: [HipBackend(*SIZE, dt=DT)],
    "folded": lambda: [HipBackend(*SIZE, dt=DT, grid_type=4)],                     # the tripolar grid with its islands: a zipper fold
    "self_ring": lambda: LocalSlabEnsemble(*SIZE, 1, dt=DT, slab_mode=1).backends,  # a slab that is its own neighbour
    "catke": catke_model,
    "slab_192": lambda: LocalSlabEnsemble(192, 32, 8, 1, dt=DT, slab_mode=1).backends,   # three tile columns: the Interior and Edges passes
    "slab_130": lambda: LocalSlabEnsemble(130, 32, 8, 1, dt=DT, slab_mode=1).backends,   # no interior tile column yet: one pass
}
SCOPES = ("gu", "tracers", "corrector", "closure")
# measured ONCE with this very function on the library of the commit before tendency_plan.hpp (momentum_impl, tracers_impl,
# corrector_impl(m, use_colsum, part) and unswept_head with their inline geometry); exact, no margin
EXPECTED = {
    "walled": (6, 6, 5, 0),
    "folded": (6, 6, 5, 0),
    "self_ring": (6, 6, 6, 0),
    "catke": (6, 6, 5, 18),
    "slab_192": (11, 6, 6, 0),   # (five split steps: two passes each; the first evaluation is whole)
    "slab_130": (6, 6, 6, 0),
}


def scopes(name):
    backends = MODELS[name]()
    b = backends[0]
    try:
        b.set_baroclinic_instability()
        b.profile_enable(True)
        b.first_time_step()
        b.loop(4)
        return tuple(b.profile_get(k)[0] for k in SCOPES)
    finally:
        for x in backends:
            x.close()


@pytest.mark.parametrize("name", list(MODELS))
def test_the_scopes_of_five_steps_on(name):
    assert scopes(name) == EXPECTED[name]
