"""gb25_set_option / gb25_get_option, option by option: the default, every accepted value and what the getter returns after it,
every refused value with its status and the text of its message, and that a refusal leaves the option as it was.  The expected
values are read off the library's source, not off a run.  No time step is made."""
import pytest

from gb25_amd.binding import OPTION_IDS, GB25Error, HipBackend
from gb25_amd.distributed import LocalSlabEnsemble

pytestmark = pytest.mark.gpu
SIZE = (48, 24, 6)
INVALID, STATE = 1, 5   # GB25_ERR_INVALID_ARGUMENT, GB25_ERR_STATE (include/gb25.h)

NO_IMMERSED = "the direct-stencil kernels know no immersed boundary"
NO_FOLD = "fold_pivot_slaved: this grid has no zipper fold"
PIVOT_SLAB = ("fold_pivot_slaved is built for the single domain only (a slab's eastern half of the pivot row belongs to its "
              "partner rank)")
STALE_SLAB = "catke_stale_e_halos: a decomposition cannot leave the halos of e stale at its internal boundaries"
ORDER_CURV = "substep_order = 1 is built for the LatitudeLongitudeGrid kernels only (the oracle has it on every grid)"


def flag(default):
    """an option stored as v != 0"""
    return dict(default=default, accept=[(0, 0), (1, 1), (2, 1), (-1, 1), (1 - default, 1 - default)], refuse=[])


def ranged(default, values, message, outside):
    return dict(default=default, accept=[(v, v) for v in values], refuse=[(v, INVALID, message) for v in outside])


# a single Float32 domain on the LatitudeLongitudeGrid, 48 x 24 x 6, nothing immersed: name -> default, (value, what get returns
# after it), (refused value, status, message)
EXPECTED = {
    "kernels": ranged(2, [1, 2], "GB25_OPT_KERNELS: 1 (direct stencil) or 2 (default)", [0, 3, -1]),
    "ab2_lookahead": ranged(1, [0, 2, 1], "GB25_OPT_AB2_LOOKAHEAD: 0, 1 or 2 (tracers only)", [-1, 3]),
    "subcycle_lookahead": ranged(0, [1, 2, 0], "GB25_OPT_SUBCYCLE_LOOKAHEAD: 0, 1 (main stream) or 2 (own stream)", [-1, 3]),
    "subcycle_block": ranged(5, [1, 3, 7, 5], "GB25_OPT_SUBCYCLE_BLOCK: 1, 3, 5 or 7 substeps per launch", [0, 2, 4, 6, 8, 9, -1]),
    "fill_fused": flag(1),
    "two_streams": flag(1),
    "store_pressure": flag(0),
    "split_tendencies": flag(1),
    "pressure_precision": ranged(64, [32, 64], "GB25_OPT_PRESSURE_PRECISION: 64 or 32", [0, 16, 33, 48, 96, -32]),
    "immersed_kernels": dict(default=0, accept=[(1, 1), (0, 0), (5, 1), (0, 0)], refuse=[]),
    "fold_fills": flag(1),
    "lazy_corrector": flag(1),
    "momentum_chunk_levels": ranged(12, [6, 24, 4096, 12], "chunk levels: 6 or more", [5, 0, -1, 4097]),
    "tracer_chunk_levels": ranged(12, [6, 24, 4096, 12], "chunk levels: 6 or more", [5, 0, -1, 4097]),
    "tracers_first": flag(1),
    "w_on_the_fly": flag(1),
    "sub_stream_priority": flag(0),
    "subcycle_whole": flag(1),
    "early_strips": flag(1),
    "catke_stale_e_halos": flag(0),
    "comm_timeout_seconds": ranged(180, [1, 2**31 - 1, 180], "comm_timeout_seconds: at least 1", [0, -5]),
    "roctx_ranges": flag(1),
    "substep_order": ranged(0, [1, 0], "substep_order: 0 (eta, then U, V) or 1 (U, V, then eta)", [2, -1]),
    "fold_pivot_slaved": dict(default=0, accept=[(0, 0)], refuse=[(1, STATE, NO_FOLD), (-3, STATE, NO_FOLD)]),
    "pressure_form": ranged(0, [1, 2, 3, 0], "GB25_OPT_PRESSURE_FORM: 0 (the library's rule), 1 (tiles), 2 (one row per thread) or "
                            "3 (four rows per thread)", [-1, 4]),
    "spectrum_table": ranged(0, [1, 0], "GB25_OPT_SPECTRUM_TABLE: 0 (the library's rule) or 1 (global memory)", [-1, 2]),
}


def accepted(b, name, value, reads_back):
    b.set_option(name, value)
    assert b.get_option(name) == reads_back, (name, value)


def refused(b, name, value, status, message):
    before = b.get_option(name)
    with pytest.raises(GB25Error) as e:
        b.set_option(name, value)
    assert str(e.value) == f"gb25_set_option: status {status}: {message}", (name, value)
    assert b.get_option(name) == before, (name, value)


@pytest.fixture(scope="module")
def model():
    b = HipBackend(*SIZE, dt=600.0)
    yield b
    b.close()


def test_the_table_names_every_option():
    assert set(EXPECTED) == set(OPTION_IDS) and sorted(OPTION_IDS.values()) == list(range(len(OPTION_IDS)))


@pytest.mark.parametrize("name", list(OPTION_IDS))
def test_default_accepted_and_refused_values(model, name):
    want = EXPECTED[name]
    assert model.get_option(name) == want["default"]
    for value, reads_back in want["accept"]:
        accepted(model, name, value, reads_back)
    for value, status, message in want["refuse"]:
        refused(model, name, value, status, message)
    accepted(model, name, want["default"], want["default"])   # (as found: the next option starts from the defaults)


def test_an_id_outside_the_enum_is_refused_by_both_calls(model):
    import ctypes as C
    for bad in (len(OPTION_IDS), -1, 1000):
        st = model.lib.gb25_set_option(model.h, bad, 1)
        assert st == INVALID and model.lib.gb25_last_error_string(model.h).decode() == f"unknown option {bad}"
        v = C.c_int32(-77)
        assert model.lib.gb25_get_option(model.h, bad, C.byref(v)) == INVALID and v.value == -77
    assert model.lib.gb25_get_option(model.h, 0, None) == INVALID
    for name, want in EXPECTED.items():   # ... and none of it touched an option
        assert model.get_option(name) == want["default"], name


def test_the_direct_stencil_kernels_and_the_immersed_variants_exclude_each_other(model):
    accepted(model, "immersed_kernels", 1, 1)
    refused(model, "kernels", 1, STATE, NO_IMMERSED)
    accepted(model, "immersed_kernels", 0, 0)   # (the flat bottom the option built immerses nothing)
    accepted(model, "kernels", 1, 1)
    refused(model, "immersed_kernels", 1, STATE, NO_IMMERSED)
    accepted(model, "immersed_kernels", 0, 0)
    accepted(model, "kernels", 2, 2)


def test_a_float64_model_keeps_its_pressure_in_fp64():
    b = HipBackend(*SIZE, dt=600.0, float_type="Float64")
    try:
        assert b.get_option("pressure_precision") == 64
        accepted(b, "pressure_precision", 32, 64)
        accepted(b, "pressure_precision", 64, 64)
        refused(b, "pressure_precision", 16, INVALID, "GB25_OPT_PRESSURE_PRECISION: 64 or 32")
    finally:
        b.close()


def test_immersed_kernels_reads_back_the_models_state_where_cells_are_immersed():
    b = HipBackend(*SIZE, dt=600.0, grid_type=1)   # the Gaussian islands on the LatitudeLongitudeGrid
    try:
        assert b.get_option("immersed_kernels") == 1
        accepted(b, "immersed_kernels", 0, 1)
        accepted(b, "immersed_kernels", 1, 1)
        refused(b, "kernels", 1, STATE, NO_IMMERSED)
    finally:
        b.close()


def test_the_options_of_a_folded_grid():
    b = HipBackend(*SIZE, dt=600.0, grid_type=3)   # TripolarGrid
    try:
        assert b.get_option("fold_pivot_slaved") == 0 and b.get_option("immersed_kernels") == 0
        for value, reads_back in ((1, 1), (0, 0), (7, 1), (-1, 1), (0, 0)):
            accepted(b, "fold_pivot_slaved", value, reads_back)
        refused(b, "substep_order", 1, STATE, ORDER_CURV)
        refused(b, "substep_order", 2, INVALID, "substep_order: 0 (eta, then U, V) or 1 (U, V, then eta)")
        accepted(b, "substep_order", 0, 0)
    finally:
        b.close()


def test_what_a_slab_refuses():
    ens = LocalSlabEnsemble(*SIZE, 2, dt=600.0, grid_type=3, substeps=2)   # (few substeps: the wide halos fit 24 columns)
    try:
        for b in ens.backends:
            assert b.get_option("subcycle_lookahead") == 1 and b.get_option("split_tendencies") == 1
            refused(b, "catke_stale_e_halos", 1, STATE, STALE_SLAB)
            accepted(b, "catke_stale_e_halos", 0, 0)
            refused(b, "fold_pivot_slaved", 1, STATE, PIVOT_SLAB)
            accepted(b, "fold_pivot_slaved", 0, 0)
        ens.set_option("two_streams", 0)
        assert [b.get_option("two_streams") for b in ens.backends] == [0, 0]
    finally:
        ens.close()
