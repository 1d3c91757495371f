"""The zonal wavenumber spectra on the host (gb-25_amd/spectra.py) on the CPU oracle's backend: the numpy restatement of
include/gb25.h pinned independently of the HIP kernel -- against np.fft.rfft, by Parseval's identity, by a single harmonic --,
the arithmetic over the ranks of a decomposition, the line that is skipped, and the table."""
import ctypes
import functools

import numpy as np
import pytest

import gb25_amd as gb
from gb25_amd import binding
from gb25_amd.spectra import (combine_spectra, cospectrum, dominant_wavenumber, global_columns, host_table, power_spectrum,
                              spectrum_host, spectrum_table_of, zonal_coefficients)
from helpers import EPS, make_oracle, stepped_model
from oracle_backend import CPU

SOURCES = ("u", "v", "T", "eta")


@functools.lru_cache(maxsize=None)
def stepped(grid_type):
    """The 48 x 24 x 6 (lat-lon: 64 x 32 x 8) oracle state after three steps; shared, never changed."""
    return stepped_model(grid_type=grid_type, arch=CPU("f64"))


def interior(b, src):
    return np.asarray(b.get_field(src, False), np.float64)


@pytest.mark.parametrize("grid_type", [0, 1, 4])
def test_against_the_fft(grid_type):
    """|dA|, |dB| <= (n + 16) eps sum_i |x(i)| per line: n products and sums of about half an ulp each, table entries within a
    few ulp of exact from the rounded angle."""
    b = stepped(grid_type).backend
    some_power = False
    for src in SOURCES:
        x = interior(b, src)
        n = x.shape[0]
        X, bad = spectrum_host(b, src)
        assert bad == 0 and X.dtype == np.complex128 and X.shape == (x.shape[2], x.shape[1], n // 2 + 1)
        ref = np.fft.rfft(x, axis=0).transpose(2, 1, 0)
        bound = (n + 16) * EPS * np.abs(x).sum(axis=0).T[:, :, None]
        dA, dB = np.abs(X.real - ref.real), np.abs(X.imag - ref.imag)
        print(f"  grid {grid_type} {src}: max dA / bound {np.max(dA / np.maximum(bound, 1e-300)):.3f}, dB {np.max(dB / np.maximum(bound, 1e-300)):.3f}")
        assert (dA <= bound).all() and (dB <= bound).all(), src
        some_power = some_power or power_spectrum(X, n)[..., 1:].max() > 0
    assert some_power
    # a window of wavenumbers and of levels is that part of the whole, bit for bit
    X, _ = spectrum_host(b, "v")
    W, _ = spectrum_host(b, "v", (3, 7), (1, 2))
    assert W.tobytes() == np.ascontiguousarray(X[1:3, :, 3:10]).tobytes()
    for bad_window in ((0, 0), (X.shape[2], 1), (-1, 2), (3, X.shape[2])):
        with pytest.raises(ValueError):
            spectrum_host(b, "v", bad_window)
    with pytest.raises(ValueError):
        spectrum_host(b, "eta", None, (1, 1))


@pytest.mark.parametrize("n", [48, 49])
def test_parseval(n):
    """sum_m P(m) = mean_i x^2: an even width has a Nyquist term of weight 1, an odd width has none."""
    rng = np.random.default_rng(n)
    x = rng.standard_normal((n, 5, 3)) * 10.0 ** rng.integers(-2, 3, (1, 5, 3))
    X, bad = zonal_coefficients(x, host_table(n))
    assert bad == 0 and X.shape == (3, 5, n // 2 + 1)
    P = power_spectrum(X, n)
    want = (x * x).mean(axis=0).T
    bound = 2 * np.abs(x).max(axis=0).T * (n + 16) * EPS * np.abs(x).sum(axis=0).T
    err = np.abs(P.sum(axis=-1) - want)
    print(f"  n = {n}: max error / bound {np.max(err / bound):.3e}")
    assert (err <= bound).all()
    # the weights follow the width: the last wavenumber of an even width counts once, of an odd width twice
    X1 = np.ones((1, 1, n // 2 + 1), np.complex128)
    w = power_spectrum(X1, n)[0, 0] * n * n
    assert w[0] == 1 and (w[1:-1] == 2).all() and w[-1] == (1 if n % 2 == 0 else 2)
    # ... and a window of wavenumbers carries the weights of its own wavenumbers
    assert np.array_equal(power_spectrum(X[..., 3:9], n, 3), P[..., 3:9])
    # the cospectrum of a field with itself is its power spectrum; summed, the cospectrum is the mean of the product
    assert np.array_equal(cospectrum(X, X, n), P)
    y = rng.standard_normal(x.shape)
    Y, _ = zonal_coefficients(y, host_table(n))
    assert np.allclose(cospectrum(X, Y, n).sum(axis=-1), (x * y).mean(axis=0).T, rtol=0, atol=1e-10 * np.abs(x).max())
    with pytest.raises(ValueError):
        cospectrum(X, Y[..., 1:], n)


def test_a_single_harmonic():
    m = make_oracle(48, 24, 6, 600.0)
    N = 48
    T = np.zeros((48, 24, 6))
    T[:, 7, 2] = np.cos(2 * np.pi * 5 * np.arange(N) / N + 0.3)
    m.tracers.T.set(T)
    X, bad = gb.zonal_spectrum(m, "T")              # (a backend without the kernel: the fallback)
    P = gb.zonal_power_spectrum(m, "T")
    assert bad == 0 and X.shape == (6, 24, 25) and np.array_equal(P, power_spectrum(X, N))
    assert dominant_wavenumber(P[2, 7]) == 5 and dominant_wavenumber(P)[2, 7] == 5
    assert abs(np.angle(X[2, 7, 5]) - 0.3) <= 1e-12 and abs(P[2, 7, 5] - 0.5) <= 1e-14
    others = np.delete(P[2, 7], 5)
    assert others.max() <= 1e-28
    assert np.count_nonzero(np.delete(P, 7, axis=1)) == 0
    # a window that starts at a wavenumber m_first names its wavenumbers from there
    Xw, _ = m.tracers.T.zonal_spectrum((4, 3), (2, 1))
    assert Xw.shape == (1, 24, 3) and dominant_wavenumber(power_spectrum(Xw, N, 4), 4)[0, 7] == 5


def rank_order_sum(parts):
    """"Add in rank order, +0.0 first", stated on its own: member by member."""
    re, im = np.zeros(parts[0].shape), np.zeros(parts[0].shape)
    for p in parts:
        re, im = re + p.real, im + p.imag
    return re, im


def sum_of_term_magnitudes(b, x):
    """sum_i |x(i) c[r(i)]| and the same with s, [level, row, m]."""
    c, s = spectrum_table_of(b)
    N = c.size
    r = np.outer(np.arange(x.shape[0]), np.arange(N // 2 + 1)) % N                 # [i, m]
    ax = np.abs(x).transpose(2, 1, 0)                                              # [level, row, i]
    return ax @ np.abs(c[r]), ax @ np.abs(s[r])


@pytest.mark.parametrize("src", ["v", "T"])
def test_the_ranks_of_a_decomposition(src):
    b = stepped(1).backend
    x = interior(b, src)
    nx, rows = x.shape[0], x.shape[1]
    assert nx == 48
    whole, _ = spectrum_host(b, src)
    tA, tB = sum_of_term_magnitudes(b, x)
    for P in (2, 3):
        w = nx // P
        parts = [spectrum_host(b, src, part=(r * w, w, 0, rows))[0] for r in range(P)]
        got = combine_spectra(parts, [(r * w, 0) for r in range(P)])
        re, im = rank_order_sum(parts)
        assert got.shape == whole.shape and got.real.tobytes() == re.tobytes() and got.imag.tobytes() == im.tobytes()
        # another order of the same terms than the single domain's
        assert (np.abs(got.real - whole.real) <= (nx + 4) * EPS * tA).all() and (np.abs(got.imag - whole.imag) <= (nx + 4) * EPS * tB).all()
        assert np.abs(got).max() > 0
    # a 2 x 2 mesh: the northern ranks of a y-face field hold the row of the wall as well
    w, h = nx // 2, 12
    blocks = [(0, w, 0, h), (w, w, 0, h), (0, w, h, rows - h), (w, w, h, rows - h)]
    parts = [spectrum_host(b, src, part=p)[0] for p in blocks]
    got = combine_spectra(parts, [(p[0], p[2]) for p in blocks])
    south, north = rank_order_sum(parts[:2]), rank_order_sum(parts[2:])
    assert got.shape == whole.shape
    assert got.real.tobytes() == np.concatenate([south[0], north[0]], axis=1).tobytes()
    assert got.imag.tobytes() == np.concatenate([south[1], north[1]], axis=1).tobytes()
    assert (np.abs(got.real - whole.real) <= (nx + 4) * EPS * tA).all() and (np.abs(got.imag - whole.imag) <= (nx + 4) * EPS * tB).all()
    # every rank uses the global column: a part is NOT the transform of the block taken from column 0
    c, s = spectrum_table_of(b)
    assert parts[1].tobytes() != zonal_coefficients(x[w:, :h], (c, s))[0].tobytes()
    with pytest.raises(ValueError):
        combine_spectra([parts[0], parts[2][:, :1]], [(0, 0), (w, 0)])


def test_a_line_that_is_not_finite():
    m = stepped_model(grid_type=1, steps=1, arch=CPU("f64"))
    b = m.backend
    before, bad = spectrum_host(b, "T")
    assert bad == 0 and np.count_nonzero(before[2, 3]) > 0
    T = np.array(b.get_field("T", False))
    T[7, 3, 2] = np.nan
    m.tracers.T.set(T)
    X, bad = spectrum_host(b, "T")
    assert bad == 1
    assert X[2, 3].tobytes() == np.zeros(X.shape[2], np.complex128).tobytes()      # (+0.0, +0.0): not -0.0, not NaN
    keep = np.ones(X.shape[:2], bool)
    keep[2, 3] = False
    assert X[keep].tobytes() == before[keep].tobytes()
    T[9, 3, 2] = np.inf                                                          # (a second value of the same line: one line)
    T[0, 5, 0] = -np.inf
    m.tracers.T.set(T)
    assert spectrum_host(b, "T")[1] == 2


def test_the_table():
    for N in (48, 49, 64):
        c, s = host_table(N)
        assert c.shape == s.shape == (N,) and c.dtype == s.dtype == np.float64
        assert c[0] == 1.0 and s[0] == 0.0 and not np.signbit(s[0])
        assert np.abs(c * c + s * s - 1).max() <= 4 * EPS
    b = stepped(1).backend
    assert global_columns(b) == (48, 0)
    c, s = spectrum_table_of(b)                     # (a backend without a table of its own: the library's formula)
    assert np.array_equal(c, host_table(48)[0]) and np.array_equal(s, host_table(48)[1])
    # gb25_get_spectrum_table needs no device: a model whose creation found none still hands its table out
    lib = binding.load_library("Float32")
    cfg, h = binding.Config(), ctypes.c_void_p()
    lib.gb25_default_config(ctypes.byref(cfg), 48, 24, 6)
    lib.gb25_create(ctypes.byref(cfg), ctypes.byref(h))
    assert h
    try:
        c, s = np.full(49, np.nan), np.full(49, np.nan)
        args = (c.ctypes.data_as(ctypes.c_void_p), s.ctypes.data_as(ctypes.c_void_p))
        assert lib.gb25_get_spectrum_table(h, *args, 48) == 0
        assert c[0] == 1.0 and s[0] == 0.0 and np.isfinite(c[:48]).all() and np.isnan(c[48]) and np.isnan(s[48])
        assert np.abs(c[:48] - host_table(48)[0]).max() <= 2 * EPS and np.abs(s[:48] - host_table(48)[1]).max() <= 2 * EPS
        for count in (47, 49, 25, 0, -1):
            assert lib.gb25_get_spectrum_table(h, *args, count) == 1, count          # (GB25_ERR_INVALID_ARGUMENT)
    finally:
        lib.gb25_destroy(h)
