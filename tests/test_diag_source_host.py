"""The argument checks of the block sums, the moving-window filter and the zonal spectra, every entry point of a field and its
derived twin, on a handle without a device: the exact status and the exact text of bad calls, in the order the library makes its
checks -- several arguments are bad at once in some rows, so that the order shows.  The texts are literals: what a call reads (a
field, or a derived field with its parameter) is resolved in one place of the host layer, and this table is what that place has to
keep saying."""
import ctypes as C

import pytest

from gb25_amd import binding

INVALID, NO_DEVICE = 1, 4
Nx, Ny, Nz = 48, 24, 6
SILENT = None      # the status alone: the call writes no text, the last one stays
NO_DEV = "this model has no device (gb25_create failed); libgb25hip has no CPU fallback"
VORTICITY = "derived GB25_D_VORTICITY lives at (f,f,c), for which the measure is not defined"
MLD = "the mixed-layer depth needs a density threshold > 0 kg/m^3 as param, got 0"
NO_OUTPUT = "measure, first and second are all NULL: no output requested"
WINDOW = "0-based local interior indices, count = -1: to the end"


@pytest.fixture(scope="module")
def handle():
    """(library, model, has the model a device): 48 x 24 x 6, lat-lon, every default."""
    import torch
    lib = binding.load_library("Float32")
    cfg, h = binding.Config(), C.c_void_p()
    lib.gb25_default_config(C.byref(cfg), Nx, Ny, Nz)
    st = lib.gb25_create(C.byref(cfg), C.byref(h))
    device = torch.cuda.is_available()
    assert h and st == (0 if device else NO_DEVICE)
    yield lib, h, device
    lib.gb25_destroy(h)


def run(lib, h, device, rows):
    """rows: (call, status, text, on a handle without a device only)."""
    for n, (call, status, text, deviceless) in enumerate(rows):
        if deviceless and device:
            continue
        before = lib.gb25_last_error_string(h)
        assert call() == status, (n, lib.gb25_last_error_string(h))
        assert lib.gb25_last_error_string(h) == (before if text is SILENT else text.encode()), (n, lib.gb25_last_error_string(h))


F = binding.FIELD_IDS
VORT, KE, MIXED = 0, 1, 4                       # gb25_derived: GB25_D_VORTICITY, GB25_D_KINETIC_ENERGY, GB25_D_MIXED_LAYER_DEPTH
a = (C.c_double * (Nx * Ny * (Nz + 1)))()
d = (C.c_int32 * 3)()


def test_block_sums(handle):
    lib, h, device = handle
    B = lambda bx, by, bz, k0=0, kc=-1: C.byref(binding.Blocks(bx, by, bz, k0, kc, 0))
    p = C.c_void_p()
    lw = lambda *v: (C.c_double * (Nz + 1))(*(list(v) + [1.0] * (Nz + 1 - len(v))))
    outs = (a, a, a)
    dims = lambda f, blk: lib.gb25_block_dims(h, f, blk, d)
    ddims = lambda q, blk: lib.gb25_derived_block_dims(h, q, blk, d)
    get = lambda f, blk, w=None, o=outs: lib.gb25_get_block_sums(h, f, blk, w, *o, None)
    compute = lambda f, blk, w=None, dev=C.byref(p): lib.gb25_compute_block_sums(h, f, blk, w, None, dev, d)
    dget = lambda q, param, blk, w=None, o=outs: lib.gb25_get_derived_block_sums(h, q, param, blk, w, *o, None)

    def of_a_field(what, field):
        e = lambda text: f"{what}: {text}"
        return [(lambda: field(999, None), INVALID, e("no field 999"), False),                                  # the id before the struct
                (lambda: field(-1, B(5, 5, 4, 9, 9)), INVALID, e("no field -1"), False),
                (lambda: field(F["T"], None), INVALID, e("blocks is NULL"), False),
                (lambda: field(F["T"], B(5, 5, 4, 9, 9)), INVALID, e("bx = 5 must be 1 .. 256 and divide the rank's Nx = 48"), False),   # bx, by, window, bz
                (lambda: field(F["T"], B(8 * Nx, 1, 1)), INVALID, e("bx = 384 must be 1 .. 256 and divide the rank's Nx = 48"), False),
                (lambda: field(F["v"], B(4, Ny + 1, 4, 9, 9)), INVALID, e("by = 25 must be > 0 and divide the rank's Ny = 24 (rows of cell centres)"), False),
                (lambda: field(F["T"], B(4, 4, 4, 2, Nz)), INVALID, e(f"window first = 2, count = 6 of 6 levels (k_first, k_count); {WINDOW}"), False),
                (lambda: field(F["w"], B(4, 4, 4, Nz + 1, 1)), INVALID, e(f"window first = 7, count = 1 of 7 levels (k_first, k_count); {WINDOW}"), False),
                (lambda: field(F["eta"], B(4, 4, 2, 0, 2)), INVALID, e(f"window first = 0, count = 2 of 1 levels (k_first, k_count); {WINDOW}"), False),
                (lambda: field(F["T"], B(4, 4, 4)), INVALID, e("bz = 4 must be > 0 and divide the 6 levels of the window"), False)]

    def of_a_derived_field(what, derived, has_param=True):
        e = lambda text: f"{what}: {text}"
        return [(lambda: derived(9, 0.0, None), INVALID, e("no derived field 9 (0 .. 4)"), False),
                (lambda: derived(VORT, 0.0, None), INVALID, e(VORTICITY), False),                                # the source before the struct
                (lambda: derived(MIXED, 0.0, None), INVALID, e(MLD if has_param else "blocks is NULL"), False),
                (lambda: derived(MIXED, 0.03, None), INVALID, e("blocks is NULL"), False),
                (lambda: derived(KE, 0.0, B(5, 5, 4, 9, 9)), INVALID, e("bx = 5 must be 1 .. 256 and divide the rank's Nx = 48"), False),
                (lambda: derived(MIXED, 0.03, B(4, 4, 1, 1, 1)), INVALID, e(f"window first = 1, count = 1 of 1 levels (k_first, k_count); {WINDOW}"), False),
                (lambda: derived(KE, 0.0, B(4, 4, 4)), INVALID, e("bz = 4 must be > 0 and divide the 6 levels of the window"), False)]

    rows = (of_a_field("gb25_block_dims", dims) + of_a_field("gb25_get_block_sums", get) + of_a_field("gb25_compute_block_sums", compute) +
            of_a_derived_field("gb25_derived_block_dims", lambda q, param, blk: ddims(q, blk), False) +
            of_a_derived_field("gb25_get_derived_block_sums", dget))
    g = lambda text: f"gb25_get_block_sums: {text}"
    rows += [(lambda: get(999, None, None, (None, None, None)), INVALID, g(NO_OUTPUT), False),                       # no output before the id
             (lambda: dget(9, 0.0, None, None, (None, None, None)), INVALID, f"gb25_get_derived_block_sums: {NO_OUTPUT}", False),
             (lambda: compute(999, None, None, None), INVALID, "gb25_compute_block_sums: dev is NULL: no output requested", False),
             (lambda: get(F["T"], B(4, 4, 4), lw(1.0, -1.0)), INVALID, g("bz = 4 must be > 0 and divide the 6 levels of the window"), False),   # bz before the weights
             (lambda: get(F["T"], B(4, 4, 2), lw(1.0, -1.0, float("nan"))), INVALID, g("level_weight[1] = -1 must be finite and >= 0"), False),
             (lambda: get(F["w"], B(4, 4, 1), lw(*([1.0] * Nz + [float("nan")]))), INVALID, g("level_weight[6] = nan must be finite and >= 0"), False),
             (lambda: get(F["eta"], B(4, 4, 1), lw(-1.0)), INVALID, g("level_weight must be NULL for a 2-D field"), False),
             (lambda: dget(MIXED, 0.03, B(4, 4, 1), lw()), INVALID, "gb25_get_derived_block_sums: level_weight must be NULL for a 2-D field", False),
             (lambda: dget(MIXED, -1.0, B(5, 4, 1), lw()), INVALID, "gb25_get_derived_block_sums: the mixed-layer depth needs a density threshold > 0 kg/m^3 as param, got -1", False),
             (lambda: dget(VORT, 0.0, B(5, 4, 1), lw(-1.0)), INVALID, f"gb25_get_derived_block_sums: {VORTICITY}", False),
             # every check passed: the device is asked for last
             (lambda: get(F["u"], B(3, 2, 2, 2, 4), lw()), NO_DEVICE, g(NO_DEV), True),
             (lambda: compute(F["eta"], B(1, 1, 1)), NO_DEVICE, f"gb25_compute_block_sums: {NO_DEV}", True),
             (lambda: dget(MIXED, 0.03, B(4, 4, 1)), NO_DEVICE, f"gb25_get_derived_block_sums: {NO_DEV}", True)]
    run(lib, h, device, rows)
    assert dims(F["v"], B(3, 2, 2, 1, 4)) == 0 and tuple(d) == (16, 12, 2)
    assert ddims(MIXED, B(4, 4, 1)) == 0 and tuple(d) == (12, 6, 1)


def test_filter_sums(handle):
    lib, h, device = handle
    Flt = lambda rx, ry, sx=1, sy=1, k0=0, kc=-1: C.byref(binding.Filter(rx, ry, sx, sy, k0, kc, 0))
    p = C.c_void_p()
    w3 = lambda *v: (C.c_double * 3)(*v)
    rows_of = lambda r: (C.c_int32 * Ny)(*([r] * Ny))
    outs = (a, a, a)
    dims = lambda f, flt: lib.gb25_filter_dims(h, f, flt, d)
    ddims = lambda q, flt: lib.gb25_derived_filter_dims(h, q, flt, d)
    get = lambda f, flt, wx=None, wy=None, rr=None, o=outs: lib.gb25_get_filter_sums(h, f, flt, wx, wy, rr, *o, None)
    compute = lambda f, flt, wx=None, wy=None, rr=None, dev=C.byref(p): lib.gb25_compute_filter_sums(h, f, flt, wx, wy, rr, None, dev, d)
    dget = lambda q, param, flt, wx=None, wy=None, rr=None, o=outs: lib.gb25_get_derived_filter_sums(h, q, param, flt, wx, wy, rr, *o, None)

    def of_a_field(what, field):
        e = lambda text: f"{what}: {text}"
        return [(lambda: field(999, None), INVALID, e("no field 999"), False),                                  # the id before the struct
                (lambda: field(F["T"], None), INVALID, e("filter is NULL"), False),
                (lambda: field(F["T"], Flt(65, 65, 5, 5, 9, 9)), INVALID, e("rx = 65 must be 0 .. 32"), False),         # rx, ry, the width, sx, sy, window
                (lambda: field(F["T"], Flt(1, -1, 5, 5, 9, 9)), INVALID, e("ry = -1 must be 0 .. 32"), False),
                (lambda: field(F["T"], Flt(24, 1, 5, 5, 9, 9)), INVALID, e("rx = 24: a window of 2 rx + 1 = 49 columns exceeds Nx = 48 (a point would enter it twice)"), False),
                (lambda: field(F["T"], Flt(1, 1, 5, 5, 9, 9)), INVALID, e("sx = 5 must be > 0 and divide Nx = 48"), False),
                (lambda: field(F["v"], Flt(1, 1, 4, 25, 9, 9)), INVALID, e("sy = 25 must be > 0 and divide Ny = 24 (rows of cell centres)"), False),
                (lambda: field(F["T"], Flt(1, 1, 4, 2, 2, Nz)), INVALID, e(f"window first = 2, count = 6 of 6 levels (k_first, k_count); {WINDOW}"), False),
                (lambda: field(F["eta"], Flt(1, 1, 4, 2, 1, 1)), INVALID, e(f"window first = 1, count = 1 of 1 levels (k_first, k_count); {WINDOW}"), False)]

    def of_a_derived_field(what, derived, has_param=True):
        e = lambda text: f"{what}: {text}"
        return [(lambda: derived(9, 0.0, None), INVALID, e("no derived field 9 (0 .. 4)"), False),
                (lambda: derived(VORT, 0.0, None), INVALID, e(VORTICITY), False),                                # the source before the struct
                (lambda: derived(MIXED, 0.0, None), INVALID, e(MLD if has_param else "filter is NULL"), False),
                (lambda: derived(MIXED, 0.03, None), INVALID, e("filter is NULL"), False),
                (lambda: derived(KE, 0.0, Flt(1, 1, 5, 5, 9, 9)), INVALID, e("sx = 5 must be > 0 and divide Nx = 48"), False),
                (lambda: derived(MIXED, 0.03, Flt(1, 1, 4, 2, 0, 2)), INVALID, e(f"window first = 0, count = 2 of 1 levels (k_first, k_count); {WINDOW}"), False)]

    rows = (of_a_field("gb25_filter_dims", dims) + of_a_field("gb25_get_filter_sums", get) + of_a_field("gb25_compute_filter_sums", compute) +
            of_a_derived_field("gb25_derived_filter_dims", lambda q, param, flt: ddims(q, flt), False) +
            of_a_derived_field("gb25_get_derived_filter_sums", dget))
    g = lambda text: f"gb25_get_filter_sums: {text}"
    dg = lambda text: f"gb25_get_derived_filter_sums: {text}"
    both = "wx and rx_of_row exclude each other: with a radius per row x is the box"
    rows += [(lambda: get(999, None, None, None, None, (None, None, None)), INVALID, g(NO_OUTPUT), False),           # no output before the id
             (lambda: dget(9, 0.0, None, None, None, None, (None, None, None)), INVALID, dg(NO_OUTPUT), False),
             (lambda: compute(999, None, None, None, None, None), INVALID, "gb25_compute_filter_sums: dev is NULL: no output requested", False),
             (lambda: get(F["T"], Flt(1, 1, 4, 2, 2, Nz), w3(1, 1, 1), None, rows_of(1)), INVALID, g(f"window first = 2, count = 6 of 6 levels (k_first, k_count); {WINDOW}"), False),
             (lambda: get(F["T"], Flt(1, 1), w3(1, -1, 1), None, rows_of(99)), INVALID, g(both), False),             # the pair before the weights and the rows
             (lambda: compute(F["T"], Flt(1, 1), w3(1, -1, 1), None, rows_of(99)), INVALID, f"gb25_compute_filter_sums: {both}", False),
             (lambda: dget(KE, 0.0, Flt(1, 1), w3(1, -1, 1), None, rows_of(99)), INVALID, dg(both), False),
             (lambda: get(F["T"], Flt(1, 1), w3(1, -1, 1), w3(0, 0, 0)), INVALID, g("wx[1] = -1 must be finite and >= 0"), False),
             (lambda: get(F["T"], Flt(1, 1), None, w3(0, 0, 0), rows_of(99)), INVALID, g("wy: the 3 weights sum to 0, not to a positive number"), False),
             (lambda: get(F["T"], Flt(1, 1), None, None, rows_of(24)), INVALID, g("rx_of_row[0] = 24 must be 0 .. 32 with 2 rx + 1 <= Nx = 48"), False),
             (lambda: dget(KE, 0.0, Flt(1, 1), None, w3(1, float("nan"), 1)), INVALID, dg("wy[1] = nan must be finite and >= 0"), False),
             (lambda: dget(MIXED, -1.0, Flt(65, 1), w3(1, 1, 1), None, rows_of(1)), INVALID, dg("the mixed-layer depth needs a density threshold > 0 kg/m^3 as param, got -1"), False),
             (lambda: dget(VORT, 0.0, Flt(65, 1), w3(1, 1, 1), None, rows_of(1)), INVALID, dg(VORTICITY), False),
             # every check passed: the device is asked for last
             (lambda: get(F["u"], Flt(2, 3, 4, 2, 1, 4), None, w3(1, 2, 1), rows_of(3)), NO_DEVICE, g(NO_DEV), True),
             (lambda: compute(F["eta"], Flt(0, 0)), NO_DEVICE, f"gb25_compute_filter_sums: {NO_DEV}", True),
             (lambda: dget(MIXED, 0.03, Flt(1, 1), w3(1, 2, 1), w3(1, 2, 1)), NO_DEVICE, dg(NO_DEV), True)]
    run(lib, h, device, rows)
    assert dims(F["v"], Flt(2, 3, 4, 2, 1, 4)) == 0 and tuple(d) == (12, 12, 4)
    assert ddims(MIXED, Flt(1, 1, 4, 4)) == 0 and tuple(d) == (12, 6, 1)


def test_zonal_spectra(handle):
    lib, h, device = handle
    rec = (binding.SpectralCoefficient * (Nz * (Ny + 1) * (Nx // 2 + 1)))()
    bad = C.c_int64()
    get = lambda f, mw, kw, count, out=rec: lib.gb25_get_zonal_spectrum(h, f, *mw, *kw, out, count, C.byref(bad))
    dget = lambda q, param, mw, kw, count, out=rec: lib.gb25_get_derived_zonal_spectrum(h, q, param, *mw, *kw, out, count, C.byref(bad))
    g = lambda text: f"gb25_get_zonal_spectrum: {text}"
    dg = lambda text: f"gb25_get_derived_zonal_spectrum: {text}"
    M = Nx // 2 + 1
    rows = [(lambda: get(999, (99, 1), (9, 9), 0, None), INVALID, g("no field 999"), False),                          # the id before `out`
            (lambda: get(F["T"], (99, 1), (9, 9), 0, None), INVALID, g("out is NULL"), False),
            # a handle without a device has no fields: the library refuses a field there without a text, whatever else is asked
            (lambda: get(F["T"], (99, 1), (9, 9), 0), INVALID, SILENT, True),
            (lambda: get(F["T"], (0, -1), (0, -1), Nz * Ny * M), INVALID, SILENT, True),
            (lambda: dget(9, 0.0, (99, 1), (9, 9), 0, None), INVALID, dg("out is NULL"), False),                      # `out` before the id
            (lambda: dget(9, 0.0, (99, 1), (9, 9), 0), INVALID, dg("no derived field 9 (0 .. 4)"), False),
            (lambda: dget(MIXED, 0.0, (99, 1), (9, 9), 0), INVALID, dg(MLD), False),                                  # the source before the windows
            (lambda: dget(KE, 0.0, (99, 1), (9, 9), 0), INVALID, dg(f"window first = 99, count = 1 of 25 wavenumbers (m_first, m_count); {WINDOW}"), False),
            (lambda: dget(KE, 0.0, (3, 7), (2, Nz), 0), INVALID, dg(f"window first = 2, count = 6 of 6 levels (k_first, k_count); {WINDOW}"), False),
            (lambda: dget(MIXED, 0.03, (3, 7), (1, 1), 0), INVALID, dg(f"window first = 1, count = 1 of 1 levels (k_first, k_count); {WINDOW}"), False),
            (lambda: dget(KE, 0.0, (3, 7), (1, 2), 5), INVALID, dg("these windows have 336 records (levels 2, rows 24, wavenumbers 7), count is 5"), False),
            # vorticity has no measure, and a spectrum needs none: its rows are those of v below the wall
            (lambda: dget(VORT, 0.0, (3, 7), (2, Nz), 0), INVALID, dg(f"window first = 2, count = 6 of 6 levels (k_first, k_count); {WINDOW}"), False),
            (lambda: dget(VORT, 0.0, (3, 7), (1, 2), 336), INVALID, dg("these windows have 350 records (levels 2, rows 25, wavenumbers 7), count is 336"), False),
            (lambda: dget(VORT, 0.0, (3, 7), (1, 2), 350), NO_DEVICE, dg(NO_DEV), True),
            (lambda: dget(MIXED, 0.03, (0, -1), (0, -1), Ny * M), NO_DEVICE, dg(NO_DEV), True)]
    run(lib, h, device, rows)
