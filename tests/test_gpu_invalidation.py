"""Every call that may invalidate state made ahead of time (the AB2 look-aheads of T, S and of u, v, the sub-cycle run one step
early, the cached column integrals, the halo cells producers write themselves) leaves a model that steps bit for bit like one
that never looks ahead -- and voids, or keeps, the velocity look-ahead as the table "Validity of look-aheads and caches" of
DESIGN.md says.  A changed dt, host writes into S and Gn.T, an Euler restart, phase-by-phase driving and a handed-out pointer
are in tests/test_gpu_parity.py (test_ab2_lookahead_is_bitwise_neutral, test_fills_folded_into_their_producers_are_bitwise_neutral);
here: one case per remaining invalidator.  A forgotten reset crashes nothing: it gives plausible wrong numbers, so the check is
bitwise and covers every parent array."""
import numpy as np
import pytest

import gb25_amd as gb
from gb25_amd.data_free import ATMOSPHERE_FIELDS, Tatm, sunlight, zonal_wind
from helpers import ALL_FIELDS, counter_rng, set_noisy_velocities

pytestmark = pytest.mark.gpu

SHAPE, HALO = (40, 21, 6), 4     # the smallest shape the parity tests run with the look-aheads on
OFF = dict(ab2_lookahead=0, w_on_the_fly=0)
ON = dict(ab2_lookahead=1, subcycle_lookahead=1, w_on_the_fly=0)


def scaled_field(name):
    def call(m):
        m.backend.set_field(name, m.backend.get_field(name, True) * np.float32(1.5), True)
    return call


def top_flux_of_T(m):
    m.backend.set_top_flux("T", (1e-4 * (counter_rng(SHAPE[:2], 3, 1) - 0.5)).astype(np.float32))


def flat_bottom(m):
    m.backend.set_bottom_height(np.full(SHAPE[:2], m.backend.metric("zf", 1)))     # at the grid's depth: nothing is immersed


def constant_atmosphere(m):
    """The analytic atmosphere of the data-free model (tests/test_gpu_data_free.py) as it is at 30 N, everywhere."""
    value = dict.fromkeys(ATMOSPHERE_FIELDS, 0.0)
    value.update(T=Tatm(0.0, 30.0) + 273.15, u=zonal_wind(0.0, 30.0), shortwave=sunlight(0.0, 30.0), p=101325.0)
    for n in ATMOSPHERE_FIELDS:
        m.backend.set_prescribed_atmosphere(n, np.full((SHAPE[0] + 2 * HALO, SHAPE[1] + 2 * HALO), value[n]))
    m.backend.compute_atmosphere_ocean_fluxes()


CATKE = dict(closure="catke")
ISLANDS = dict(grid_type="gaussian_islands_lat_lon")
# (id, model keywords, [(call, velocity look-ahead right after it)], velocity look-ahead once the model steps again)
CASES = [
    ("set_field-u", {}, [(scaled_field("u"), False)], True),
    ("set_field-T", {}, [(scaled_field("T"), False)], True),
    ("set_field-eta", {}, [(scaled_field("eta"), False)], True),
    ("set_field-Gn.u", {}, [(scaled_field("Gn.u"), False)], True),
    ("set_top_flux", {}, [(top_flux_of_T, False), (lambda m: m.backend.set_top_flux("T", None), False)], True),
    ("set_bottom_drag", {}, [(lambda m: m.backend.set_bottom_drag(0.003), False)], True),
    ("set_tracer_advection_order", {}, [(lambda m: m.backend.set_tracer_advection_order(7), False)], True),
    ("set_catke_parameters", CATKE, [(lambda m: m.backend.set_catke_parameters(Cb=0.3), False)], True),
    ("set_option-tracers_first", {}, [(lambda m: m.backend.set_option("tracers_first", 0), False)], True),
    ("set_option-momentum_chunk_levels", {}, [(lambda m: m.backend.set_option("momentum_chunk_levels", 6), False)], True),
    ("mask_immersed_fields", ISLANDS, [(lambda m: m.backend.mask_immersed_fields(), False)], True),
    ("set_bottom_height", {}, [(flat_bottom, False)], True),
    ("field_device_ptr", {}, [(lambda m: m.backend.field_device_ptr("u"), False)], False),   # no look-ahead ever again
    ("prescribed_atmosphere", {}, [(constant_atmosphere, False)], True),
    # narrower resets: the velocity look-ahead stays
    ("set_vertical_diffusivity", {}, [(lambda m: m.backend.set_vertical_diffusivity(1e-4, 1e-5), True)], True),
    ("set_closure_catke-off", CATKE, [(lambda m: m.backend.set_catke(False), True)], True),
    ("set_dt", {}, [(lambda m: m.backend.set_dt(240.0), True)], True),     # (the keys fail the adoption, not a flag)
]


@pytest.mark.parametrize("kw,calls,ready_again", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_invalidating_call_keeps_the_lookahead_model_bitwise(kw, calls, ready_again, request):
    kw = dict(kw)
    if kw.pop("closure", None):
        kw["closure"] = gb.CATKEVerticalDiffusivity()
    a, b = (gb.baroclinic_instability_model(gb.GPU(), *SHAPE, dt=300.0, halo=(HALO,) * 3, options=o, **kw) for o in (OFF, ON))
    for m in (a, b):
        gb.set_baroclinic_instability(m)
        set_noisy_velocities(m, 0.05)
        gb.first_time_step(m)
        gb.loop(m, 3)
    for call, ready_after in calls:
        assert b.backend.lookahead_state()[0]          # there is a look-ahead to void
        for m in (a, b):
            call(m)
        assert b.backend.lookahead_state()[0] == ready_after
        for m in (a, b):
            gb.loop(m, 1)
        if request.node.callspec.id == "set_dt":
            assert not b.backend.lookahead_state()[1]  # the step after set_dt adopted nothing
        for m in (a, b):
            gb.loop(m, 3)      # through the two complete-fill steps, back into the adopting route
        assert b.backend.lookahead_state()[0] == ready_again
        for n in ALL_FIELDS:
            assert np.array_equal(a.backend.get_field(n, True), b.backend.get_field(n, True)), n
    assert np.isfinite(b.backend.get_field("u", True)).all() and np.abs(b.backend.get_field("u", False)).max() > 0
    for m in (a, b):
        m.backend.close()
