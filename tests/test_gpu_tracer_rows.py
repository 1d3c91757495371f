"""The tracer tendency kernel with two rows per lane (ROWS = 2: the y face between the rows reconstructed once) against the
one-row form: the same operands in the same order, so every cell of every parent array must agree bit for bit.  The form is
chosen when a model is created (GB25_TRACER_ROWS in the environment: 1 or 2), so two models in one process compare them.

What these tests cannot see: the library exports nothing that tells which instance was launched, so if the variable were read and
then ignored every bitwise case would still pass.  That the variable is read is shown by the last test (a bad value is refused);
that two rows per lane really run where asked for is shown by the kernel's name in a trace (profiles/tracer_rows_kernel_stats_after.csv)
and by tools/tracer_rows_ab.py, whose two settings time differently."""
import os

import numpy as np
import pytest

import gb25_amd as gb
from gb25_amd.binding import GB25Error
from helpers import ALL_FIELDS, counter_rng, set_noisy_velocities

pytestmark = pytest.mark.gpu

# (70, 13, 7): two ragged tiles of 63, Ny odd (the last lane's upper row is a masked duplicate), every row next to a wall;
# (40, 21, 6): Nx below a tile, Ny odd; (16, 9, 4): fewer rows than two blocks; (150, 70, 24) in two chunks of 12 levels: the
# carried top flux and the start of w on the fly are taken per row and per chunk
SHAPES = {"ragged": ((70, 13, 7), 8, {}), "narrow": ((40, 21, 6), 4, {}), "tiny": ((16, 9, 4), 4, {}),
          "chunks": ((150, 70, 24), 8, dict(tracer_chunk_levels=12, momentum_chunk_levels=12))}
ROUTES = [(0, 0), (1, 0), (1, 1)]   # (lazy_corrector, w_on_the_fly)


def model_with_rows(rows, shape, halo, float_type, options):
    before = os.environ.get("GB25_TRACER_ROWS")
    os.environ["GB25_TRACER_ROWS"] = str(rows)
    try:
        m = gb.baroclinic_instability_model(gb.GPU(float_type=float_type), *shape, dt=300.0, halo=(halo,) * 3, options=options)
    finally:
        if before is None:
            del os.environ["GB25_TRACER_ROWS"]
        else:
            os.environ["GB25_TRACER_ROWS"] = before
    dtype = np.float32 if float_type == "Float32" else np.float64
    gb.set_baroclinic_instability(m)
    set_noisy_velocities(m, 0.05)
    for n, seed in (("T", 5), ("S", 4), ("u", 6), ("v", 7), ("eta", 8), ("V", 9)):
        a = m.backend.get_field(n, True)
        a += (1e-3 * counter_rng(a.shape, seed, 1)).astype(dtype)          # noise in EVERY halo layer
        m.backend.set_field(n, a, True)
    return m


def compare_forms(shape, halo, float_type, options, lazy=None):
    a, b = (model_with_rows(rows, shape, halo, float_type, options) for rows in (1, 2))

    def same(label):
        for n in ALL_FIELDS:
            x, y = a.backend.get_field(n, True), b.backend.get_field(n, True)
            assert np.array_equal(x, y), (label, n, float(np.abs(x - y).max()))

    for label, advance in (("first_time_step", lambda m: gb.first_time_step(m)), ("loop of 7", lambda m: gb.loop(m, 7)),
                           ("a single time_step", lambda m: gb.time_step(m)), ("loop of 2", lambda m: gb.loop(m, 2))):
        for m in (a, b):
            advance(m)
        same(label)
        if lazy and label.startswith("loop"):
            # the lazy route needs both look-aheads.  The first flag says that the velocity look-ahead exists and that the sub-cycle
            # look-ahead is switched on; the second flag is kept by the staged step of a slab only -- on a single domain it
            # is always False, so `== (True, True)` as the slab tests have it cannot be asked here.
            for m in (a, b):
                assert m.backend.get_option("lazy_corrector") == 1 and m.backend.get_option("subcycle_lookahead") == 1
                assert m.backend.lookahead_state()[0], label
    assert np.abs(a.velocities.u.interior).max() > 0.01
    assert np.isfinite(a.tracers.T.interior).all()


CASES = [(s, "Float32", r) for s in SHAPES for r in ROUTES] + [(s, "Float64", r) for s in ("ragged", "chunks") for r in ROUTES]


@pytest.mark.parametrize("shape_name,float_type,route", CASES)
def test_two_rows_per_lane_give_the_bits_of_one(shape_name, float_type, route):
    """first_time_step, loop(7), a single time_step and loop(2): every parent array of the model stepped with two rows per lane
    equals, bit for bit, that of the model stepped with one -- with the corrector's sweep, with the corrector inside its
    consumers, and with w carried on the fly as well."""
    shape, halo, extra = SHAPES[shape_name]
    lazy, fly = route
    options = dict(extra, subcycle_lookahead=1, lazy_corrector=lazy, w_on_the_fly=fly)
    compare_forms(shape, halo, float_type, options, lazy=lazy)


def test_two_rows_per_lane_without_the_lookahead():
    """The instance that does not write the next time level (ab2_lookahead = 0) on the ragged shape."""
    shape, halo, _ = SHAPES["ragged"]
    compare_forms(shape, halo, "Float32", dict(ab2_lookahead=0))


def test_the_variable_takes_only_1_or_2():
    before = os.environ.get("GB25_TRACER_ROWS")
    os.environ["GB25_TRACER_ROWS"] = "3"
    try:
        with pytest.raises(GB25Error, match="GB25_TRACER_ROWS must be 1 or 2"):
            gb.baroclinic_instability_model(gb.GPU(), 16, 9, 4, dt=300.0)
    finally:
        if before is None:
            del os.environ["GB25_TRACER_ROWS"]
        else:
            os.environ["GB25_TRACER_ROWS"] = before
