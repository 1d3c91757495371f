"""Zonal wavenumber spectra on the device (include/gb25.h, gb25_get_zonal_spectrum / gb25_get_derived_zonal_spectrum;
csrc/spectrum_kernels.hpp) against their numpy restatement (gb-25_amd/spectra.py), bit for bit: every source, windows of
wavenumbers and levels, the shapes at which the kernel cuts its blocks differently, the table in global memory, a line that is not
finite, the ranks of a decomposition, and that a call changes nothing a step reads."""
import ctypes

import numpy as np
import pytest

import gb25_amd as gb
from gb25_amd.binding import DERIVED_IDS, FIELD_IDS, KERNEL_IDS
from gb25_amd.distributed import LocalSlabEnsemble
from gb25_amd.spectra import combine_spectra, power_spectrum, spectrum_host, spectrum_table_of
from helpers import BASE_FIELDS, CASES, EPS, size_of, stepped_model

pytestmark = pytest.mark.gpu

SOURCES = ("u", "v", "w", "T", "S", "eta", "pHY", "vorticity", "kinetic_energy", "mixed_layer_depth")
FLAT = ("eta", "mixed_layer_depth")


def levels_of(b, src):
    return b.derived_dims(src)[2] if src in ("vorticity", "kinetic_energy", "mixed_layer_depth") else b.field_dims(src, False)[2]


def check_bit_for_bit(b, src, wavenumbers, levels, tag=""):
    X, bad = b.zonal_spectrum(src, wavenumbers, levels)
    H, hbad = spectrum_host(b, src, wavenumbers, levels)
    assert X.shape == H.shape and X.dtype == H.dtype == np.complex128, (tag, src, wavenumbers, levels)
    assert X.tobytes() == H.tobytes() and bad == hbad, (tag, src, wavenumbers, levels)
    return X, bad


@pytest.mark.parametrize("float_type,grid_type", CASES)
def test_bit_for_bit(float_type, grid_type):
    m = stepped_model(float_type, grid_type)
    b = m.backend
    N = size_of(grid_type)[0]
    c, s = b.spectrum_table()
    assert c.shape == s.shape == (N,) and c[0] == 1.0 and s[0] == 0.0
    for src in SOURCES:
        nz = levels_of(b, src)
        level_windows = (None, (0, 1), (0, -1)) if src in FLAT else (None, (nz - 1, 1), (1, 2))
        for wavenumbers in (None, (0, 1), (N // 2, 1), (3, 7)):
            for levels in level_windows:
                X, bad = check_bit_for_bit(b, src, wavenumbers, levels, f"{float_type} grid {grid_type}")
                assert bad == 0
                again, _ = b.zonal_spectrum(src, wavenumbers, levels)
                assert again.tobytes() == X.tobytes(), (src, wavenumbers, levels)
                if wavenumbers is None and levels is None:
                    assert power_spectrum(X, N).max() > 0, src        # (all zeros cannot pass)
                    rows = b.derived_dims(src)[1] if src in ("vorticity", "kinetic_energy", "mixed_layer_depth") else b.field_dims(src, False)[1]
                    assert X.shape == (nz, rows, N // 2 + 1)
    # the public functions go through the kernel
    X, _ = gb.zonal_spectrum(m, "v", levels=(size_of(grid_type)[2] - 1, 1))
    assert X.tobytes() == b.zonal_spectrum("v", None, (size_of(grid_type)[2] - 1, 1))[0].tobytes()
    assert np.array_equal(gb.zonal_power_spectrum(m, "v", (2, 5)), power_spectrum(m.velocities.v.zonal_spectrum((2, 5))[0], N, 2))
    b.close()


# (136, 12, 4): the model needs four levels at the least
@pytest.mark.parametrize("size,wavenumbers", [((50, 24, 6), None), ((50, 24, 6), (5, 3)), ((136, 12, 4), None), ((136, 12, 4), (60, 9)),
                                              ((64, 32, 8), (0, 1)), ((64, 32, 8), (7, 1)), ((50, 24, 6), (25, 1))])
def test_shapes_where_the_kernel_can_go_wrong(size, wavenumbers):
    """50 columns fill no chunk and are no multiple of 4 or 64; 136 columns have 69 wavenumbers, more than one wave of lanes; one
    wavenumber fills the lanes of a wave with 64 lines; 25 rows of v and windows of levels leave the last block partly empty."""
    m = stepped_model("Float32", 1, size=size)
    b = m.backend
    some_power = False
    for src in ("u", "v", "eta", "vorticity"):
        nz = levels_of(b, src)
        for levels in ((None,) if src == "eta" else (None, (1, 1), (0, nz - 1))):
            X, bad = check_bit_for_bit(b, src, wavenumbers, levels, f"{size}")
            assert bad == 0
            some_power = some_power or np.abs(X).max() > 0
    assert some_power
    b.close()


def test_a_table_past_64_kb_of_lds():
    """3200 columns: 51,200 bytes of table and 16,432 of staged lines are more dynamic LDS than a launch gets without the
    function attribute the host side raises; wide and shallow, so that the restatement stays quick."""
    m = stepped_model("Float32", 0, steps=0, size=(3200, 12, 4), dt=60.0)
    b = m.backend
    X, bad = check_bit_for_bit(b, "v", None, (3, 1), "3200 columns")
    assert bad == 0 and X.shape == (1, 13, 1601) and np.abs(X[..., 1:]).max() > 0
    X, bad = check_bit_for_bit(b, "u", (1500, 70), None, "3200 columns")
    assert bad == 0 and np.abs(X).max() > 0
    check_bit_for_bit(b, "eta", (0, 1), None, "3200 columns")          # (one wavenumber: 256 lines a block, 8 columns a chunk)
    b.set_option("spectrum_table", 1)
    assert b.zonal_spectrum("u", (1500, 70))[0].tobytes() == X.tobytes()
    b.close()


@pytest.mark.parametrize("float_type,grid_type", [("Float32", 1), ("Float64", 4)])
def test_the_table_in_global_memory(float_type, grid_type):
    m = stepped_model(float_type, grid_type)
    b = m.backend
    for src in ("v", "eta", "kinetic_energy"):
        for wavenumbers in (None, (0, 1), (3, 7)):
            b.set_option("spectrum_table", 0)
            lds, _ = b.zonal_spectrum(src, wavenumbers)
            b.set_option("spectrum_table", 1)
            assert b.get_option("spectrum_table") == 1
            X, _ = check_bit_for_bit(b, src, wavenumbers, None, "global table")
            assert X.tobytes() == lds.tobytes() and np.abs(X).max() > 0
    with pytest.raises(gb.GB25Error):
        b.set_option("spectrum_table", 2)
    b.close()


@pytest.mark.parametrize("float_type,grid_type", [("Float32", 1), ("Float64", 4)])
def test_a_nan_in_a_line(float_type, grid_type):
    m = stepped_model(float_type, grid_type, steps=1)
    b = m.backend
    before, bad = b.zonal_spectrum("T")
    assert bad == 0 and np.count_nonzero(before[2, 3]) > 0
    T = b.get_field("T", False).copy()
    T[7, 3, 2] = np.nan
    m.tracers.T.set(T)
    for wavenumbers in (None, (0, 1), (3, 7)):
        X, bad = check_bit_for_bit(b, "T", wavenumbers, None, "NaN")
        assert bad == 1
        assert X[2, 3].tobytes() == np.zeros(X.shape[2], np.complex128).tobytes()
    X, _ = b.zonal_spectrum("T")
    keep = np.ones(X.shape[:2], bool)
    keep[2, 3] = False
    assert X[keep].tobytes() == before[keep].tobytes()
    assert b.zonal_spectrum("T", None, (3, 1))[1] == 0 and b.zonal_spectrum("S")[1] == 0
    b.close()


def sum_of_term_magnitudes(b, x):
    c, s = spectrum_table_of(b)
    N = c.size
    r = np.outer(np.arange(x.shape[0]), np.arange(N // 2 + 1)) % N
    ax = np.abs(np.asarray(x, np.float64)).transpose(2, 1, 0)
    return ax @ np.abs(c[r]), ax @ np.abs(s[r])


@pytest.mark.parametrize("P,Ry", [(2, 1), (4, 1), (4, 2)])
def test_the_ranks_of_a_decomposition(P, Ry):
    """The 48 x 24 x 6 state on 2 and 4 slabs and on a 2 x 2 mesh: every rank's part is its restatement bit for bit, the combined
    coefficients are combine_spectra of the host's parts bit for bit and the single domain's to (n + 4) eps sum |terms|."""
    Nx, Ny, Nz = size_of(1)
    single = stepped_model("Float32", 1)
    sb = single.backend
    kw = dict(slab_mode=1) if Ry > 1 else {}
    # (the ensemble holds the scattered state and is never stepped: two substeps keep the wide halo of the sub-cycle, which
    # a rank must be wider than, within the 12 columns and rows of the narrowest rank)
    ens = LocalSlabEnsemble(Nx, Ny, Nz, P, dt=600.0, ranks_y=Ry, grid_type=1, substeps=2, **kw)
    for n in ("u", "v", "T", "S", "eta"):
        ens.scatter(n, sb.get_field(n, False))
    offsets = [(r.rx * ens.Nx_loc, r.ry * ens.Ny_loc) for r in ens.backends]
    for src in ("u", "v", "T", "eta"):
        assert np.array_equal(ens.gather(src), sb.get_field(src, False)), src            # (the premise)
        for wavenumbers in (None, (3, 7)):
            host_parts = []
            for r in ens.backends:
                X, bad = check_bit_for_bit(r, src, wavenumbers, None, f"rank {r.rx}, {r.ry} of {P} ({Ry} in y)")
                assert bad == 0
                host_parts.append(spectrum_host(r, src, wavenumbers)[0])
            got, bad = ens.zonal_spectrum(src, wavenumbers)
            assert bad == 0 and got.tobytes() == combine_spectra(host_parts, offsets).tobytes(), (src, wavenumbers)
            one, _ = sb.zonal_spectrum(src, wavenumbers)
            tA, tB = sum_of_term_magnitudes(sb, sb.get_field(src, False))
            if wavenumbers is not None:
                tA, tB = tA[..., 3:10], tB[..., 3:10]
            assert got.shape == one.shape and np.abs(got).max() > 0
            assert (np.abs(got.real - one.real) <= (Nx + 4) * EPS * tA).all(), (src, wavenumbers)
            assert (np.abs(got.imag - one.imag) <= (Nx + 4) * EPS * tB).all(), (src, wavenumbers)
    ens.close()
    sb.close()


LOOKAHEADS = dict(subcycle_lookahead=1, ab2_lookahead=1)


@pytest.mark.parametrize("float_type,grid_type", [("Float32", 0), ("Float64", 4)])
def test_spectra_are_read_only(float_type, grid_type):
    """Two identical models; one is asked for spectra of fields and of derived fields between every two steps.  Same bits, same
    look-ahead state, same launches of every phase of a step."""
    watched = stepped_model(float_type, grid_type, steps=0, **LOOKAHEADS)
    alone = stepped_model(float_type, grid_type, steps=0, **LOOKAHEADS)
    for m in (watched, alone):
        m.backend.profile_enable(True)
        m.backend.profile_reset()
    for step in range(6):
        if step % 2 == 0:
            before = watched.backend.lookahead_state()
            for src in ("v", "T", "eta", "pHY", "vorticity", "kinetic_energy", "mixed_layer_depth"):
                X, bad = watched.backend.zonal_spectrum(src, None if step else (1, 9))
                assert bad == 0 and (step > 0 or np.abs(X).max() > 0), src
            assert watched.backend.lookahead_state() == before
        for m in (watched, alone):
            gb.time_step(m)
        assert watched.backend.lookahead_state() == alone.backend.lookahead_state(), step
    for k in KERNEL_IDS:
        if k != "diagnostics":
            assert watched.backend.profile_get(k)[0] == alone.backend.profile_get(k)[0], k
    assert watched.backend.profile_get("diagnostics")[0] > 0 and alone.backend.profile_get("diagnostics")[0] == 0
    for name in BASE_FIELDS:
        a, b = watched.backend.get_field(name, True), alone.backend.get_field(name, True)
        assert a.tobytes() == b.tobytes(), name
    assert np.abs(watched.backend.get_field("u", False)).max() > 0
    for m in (watched, alone):
        m.backend.close()


def test_argument_errors_through_the_abi():
    m = stepped_model("Float32", 0, steps=0)
    b = m.backend
    Nx, Ny, Nz = size_of(0)
    M = Nx // 2 + 1
    out = np.zeros((Nz + 1) * (Ny + 1) * M, np.complex128)
    p, bad = out.ctypes.data_as(ctypes.c_void_p), ctypes.c_int64(0)
    field, derived = b.lib.gb25_get_zonal_spectrum, b.lib.gb25_get_derived_zonal_spectrum
    T, ETA, KE, MLD = FIELD_IDS["T"], FIELD_IDS["eta"], DERIVED_IDS["kinetic_energy"], DERIVED_IDS["mixed_layer_depth"]
    assert field(b.h, T, 0, -1, 0, -1, p, Nz * Ny * M, ctypes.byref(bad)) == 0
    assert field(b.h, T, 0, -1, 0, -1, p, Nz * Ny * M, None) == 0                       # (the count may be left out)
    assert derived(b.h, KE, 0.0, 0, -1, 0, -1, p, Nz * Ny * M, ctypes.byref(bad)) == 0
    assert field(b.h, ETA, 0, -1, 0, 1, p, Ny * M, ctypes.byref(bad)) == 0 and field(b.h, ETA, 0, -1, 0, -1, p, Ny * M, ctypes.byref(bad)) == 0
    cases = [("m_first > N/2", (M, 1, 0, -1, Nz * Ny), b"window"), ("m_count = 0", (0, 0, 0, -1, 0), b"window"),
             ("m_count too long", (3, M - 2, 0, -1, Nz * Ny * (M - 2)), b"window"),
             ("a wrong count", (0, -1, 0, -1, Nz * Ny * M - 1), b"count"), ("a wrong count", (0, 4, 0, 2, 2 * Ny * 4 + 1), b"count"),
             ("levels out of range", (0, -1, Nz, 1, Ny * M), b"window"), ("levels out of range", (0, -1, 2, Nz - 1, (Nz - 1) * Ny * M), b"window"),
             ("k_count = 0", (0, -1, 0, 0, 0), b"window")]
    for what, (m_first, m_count, k_first, k_count, count), word in cases:
        assert field(b.h, T, m_first, m_count, k_first, k_count, p, count, ctypes.byref(bad)) == 1, what
        assert word in b.lib.gb25_last_error_string(b.h), what
        assert derived(b.h, KE, 0.0, m_first, m_count, k_first, k_count, p, count, ctypes.byref(bad)) == 1, what
        assert word in b.lib.gb25_last_error_string(b.h), what
    # a 2-D source has one level
    assert field(b.h, ETA, 0, -1, 1, 1, p, Ny * M, ctypes.byref(bad)) == 1 and b"window" in b.lib.gb25_last_error_string(b.h)
    assert derived(b.h, MLD, 0.03, 0, -1, 1, 1, p, Ny * M, ctypes.byref(bad)) == 1 and b"window" in b.lib.gb25_last_error_string(b.h)
    assert derived(b.h, MLD, 0.03, 0, -1, 0, 1, p, Ny * M, ctypes.byref(bad)) == 0
    assert derived(b.h, MLD, 0.0, 0, -1, 0, 1, p, Ny * M, ctypes.byref(bad)) == 1      # (no threshold)
    assert field(b.h, 999, 0, -1, 0, -1, p, Nz * Ny * M, ctypes.byref(bad)) == 1 and derived(b.h, 99, 0.0, 0, -1, 0, -1, p, Nz * Ny * M, ctypes.byref(bad)) == 1
    assert field(b.h, T, 0, -1, 0, -1, None, Nz * Ny * M, ctypes.byref(bad)) == 1
    c = np.zeros(Nx)
    assert b.lib.gb25_get_spectrum_table(b.h, c.ctypes.data_as(ctypes.c_void_p), c.ctypes.data_as(ctypes.c_void_p), Nx - 1) == 1
    assert b.lib.gb25_spectral_coefficient_bytes() == 16
    with pytest.raises(gb.GB25Error, match="window"):
        b.zonal_spectrum("T", (M, 1))
    # the model still steps, and answers
    gb.time_step(m)
    X, bad = check_bit_for_bit(b, "T", None, None, "after the errors")
    assert bad == 0 and np.abs(X).max() > 0
    b.close()
