"""The loads of the two-rows tracer kernel (tracer_tile_rows2): the lane's own cell comes from the vertical window instead of being
loaded again with the x and the y window, and the y window is loaded one level ahead.  Neither changes an operand, so the model
stepped with two rows per lane must equal the model stepped with one, bit for bit, as in test_gpu_tracer_rows.py (two models in one
process, GB25_TRACER_ROWS set around their creation).  The shapes aim at what these two changes can break:

(70, 13, 12), halo 4: Ny odd -- the last wave's upper row is a clamped duplicate of row Ny - 1, so the y window's row j + 1 is the
  halo row and must still come from memory; in chunks of 6 levels and as one chunk, so that the window loaded ahead at a chunk's last
  level and at the top level is covered;
(126, 17, 12), halo 8: exactly two full tiles of 63, Ny = 1 mod 8, chunks of 6 levels;
(16, 9, 4), halo 4: fewer levels than the vertical window.

Each with the look-ahead on and off (ab2_lookahead) and with the corrector as a sweep and inside its consumers (lazy_corrector; with
it w is carried on the fly, the headline route)."""
import numpy as np
import pytest

import gb25_amd as gb
from test_gpu_tracer_rows import model_with_rows

pytestmark = pytest.mark.gpu

CHUNKS_OF_6 = dict(tracer_chunk_levels=6, momentum_chunk_levels=6)
ONE_CHUNK = dict(tracer_chunk_levels=12, momentum_chunk_levels=12)
SHAPES = {"odd_rows_chunks": ((70, 13, 12), 4, CHUNKS_OF_6), "odd_rows_one_chunk": ((70, 13, 12), 4, ONE_CHUNK),
          "two_tiles": ((126, 17, 12), 8, CHUNKS_OF_6), "few_levels": ((16, 9, 4), 4, {})}
FIELDS = ["T", "S", "Gn.T", "Gn.S"]


@pytest.mark.parametrize("lazy", [0, 1])
@pytest.mark.parametrize("ahead", [1, 0])
@pytest.mark.parametrize("shape_name", list(SHAPES))
def test_own_cell_and_window_ahead_give_the_bits_of_one_row(shape_name, ahead, lazy):
    """first_time_step and loop(3): T, S and their tendencies (parent arrays, halos included) of the two forms are equal."""
    shape, halo, extra = SHAPES[shape_name]
    options = dict(extra, ab2_lookahead=ahead, subcycle_lookahead=1, lazy_corrector=lazy, w_on_the_fly=lazy)
    a, b = (model_with_rows(rows, shape, halo, "Float32", options) for rows in (1, 2))
    for m in (a, b):
        gb.first_time_step(m)
        gb.loop(m, 3)
    for n in FIELDS:
        x, y = a.backend.get_field(n, True), b.backend.get_field(n, True)
        assert np.array_equal(x, y), (n, float(np.abs(x - y).max()))
    assert np.isfinite(a.tracers.T.interior).all()
    assert np.abs(a.backend.get_field("Gn.T", False)).max() > 0
