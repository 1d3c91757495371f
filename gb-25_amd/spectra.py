"""Zonal wavenumber spectra on the host: the definition of include/gb25.h ("zonal wavenumber spectra on the device") restated
with numpy from a backend's public getters alone, in fp64, with the order of every sum of the kernel (csrc/spectrum_kernels.hpp,
k_zonal_spectrum), so that the device's coefficients equal these bit for bit; the host fallback of gb25_get_zonal_spectrum; the
helpers that turn coefficients into power spectra; and the arithmetic that combines the parts of the ranks of a decomposition.
Works on binding.HipBackend and on the test suite's oracle backend.

    line                 interior row j and level k of the source, local columns i = 0 .. nx-1, global column g = i + offset
    table                c[r] = cos((2 pi r) / N), s[r] = sin((2 pi r) / N): the backend's (HipBackend.spectrum_table, the table
                         of the definition), host_table(N) for a backend without one
    A(m), B(m)           (((+0.0 + x(0) c[r(0)]) + x(1) c[r(1)]) + ...) and the same with s, r(i) = (m g) mod N, SEQUENTIAL over i
    X(m) = A(m) - i B(m) np.fft.rfft's sign, and its value when the rank holds the whole row
    a line with a value that is not finite: every coefficient +0.0, counted once

Coefficients are complex128 arrays [level, row, m].  The transform is taken along the grid's index i: on the curvilinear and
folded grids that is the grid line, not a latitude circle."""
import numpy as np

from .binding import DERIVED_IDS

TWO_PI = 6.283185307179586


def host_table(N):
    """(c, s), the table of the definition for a grid of N columns, by the library's formula."""
    a = (TWO_PI * np.arange(int(N), dtype=np.float64)) / float(int(N))
    return np.cos(a), np.sin(a)


def global_columns(backend):
    """(N, offset): the columns of the global grid and the global 0-based column of this backend's local column 0."""
    nx = backend.field_dims("T", False)[0]
    return nx * getattr(backend, "Rx", 1), nx * getattr(backend, "rx", 0)


def spectrum_table_of(backend):
    if hasattr(backend, "spectrum_table"):
        return backend.spectrum_table()
    return host_table(global_columns(backend)[0])


def _span(window, extent, noun):
    """(first, count) of a window = (first, count) of 0 .. extent-1, count = -1: to the end; None: all."""
    first, count = (0, -1) if window is None else (int(window[0]), int(window[1]))
    n = extent - first if count == -1 else count
    if first < 0 or first >= extent or count < -1 or count == 0 or first + n > extent:
        raise ValueError(f"window first = {first}, count = {count} of {extent} {noun}")
    return first, n


def zonal_coefficients(x, table, offset=0, wavenumbers=None):
    """(X [level, row, m] complex128, the number of skipped lines) of x [i, row, level] (or [i, row]): the loop over i of the
    kernel, vectorised over (m, row, level).  numpy rounds the product and the sum separately: no fused multiply-add."""
    c, s = (np.asarray(t, np.float64) for t in table)
    N = c.size
    x = np.asarray(x, np.float64)
    if x.ndim == 2:
        x = x[:, :, None]
    m_first, mc = _span(wavenumbers, N // 2 + 1, "wavenumbers")
    m = np.arange(m_first, m_first + mc, dtype=np.int64)
    lines = np.ascontiguousarray(x.transpose(2, 1, 0))           # [level, row, i]
    A = np.zeros(lines.shape[:2] + (mc,))
    B = np.zeros(lines.shape[:2] + (mc,))
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(lines.shape[2]):
            r = (m * (i + int(offset))) % N
            xi = lines[:, :, i, None]
            A = A + xi * c[r]
            B = B + xi * s[r]
    bad = ~np.isfinite(lines).all(axis=2)
    X = np.empty(A.shape, np.complex128)
    X.real, X.imag = A, -B
    X[bad] = 0.0
    return X, int(bad.sum())


def source_values(backend, source, levels=None, param=None):
    """The interior of a source -- a field name or a derived name -- as the device reads it, [i, row, level] of the levels
    (k_first, k_count) (None: all; a 2-D source has one)."""
    if source in DERIVED_IDS:
        if hasattr(backend, "get_derived"):
            return np.asarray(backend.get_derived(source, param, levels))
        from . import derived as host                     # (a backend without the device kernels: the numpy restatement)
        if source == "vorticity":
            return np.asarray(host.vorticity_host(backend, levels))
        if source == "kinetic_energy":
            return np.asarray(host.kinetic_energy_host(backend, levels))
        raise NotImplementedError(f"{source} needs a backend with get_derived")
    a = np.asarray(backend.get_field(source, False))
    k_first, kc = _span(levels, a.shape[2], "levels")
    return a[:, :, k_first:k_first + kc]


def spectrum_host(backend, source, wavenumbers=None, levels=None, param=None, part=None):
    """What HipBackend.zonal_spectrum returns, (X [level, row, m], nonfinite_lines), computed with numpy from the downloaded
    source and the backend's table, bit for bit: the fallback for a backend without the kernel.  part = (i0, nx, j0, ny): only
    that block of the backend's interior, as the rank of a decomposition that owns it would see it (its lines start at the
    global column offset + i0)."""
    x = source_values(backend, source, levels, param)
    _, offset = global_columns(backend)
    if part is not None:
        i0, nx, j0, ny = part
        x, offset = x[i0:i0 + nx, j0:j0 + ny], offset + i0
    return zonal_coefficients(x, spectrum_table_of(backend), offset, wavenumbers)


def _weights(n, N, m_first):
    m = np.arange(m_first, m_first + n)
    return np.where((m == 0) | ((N % 2 == 0) & (m == N // 2)), 1.0, 2.0)


def power_spectrum(X, N, m_first=0):
    """The one-sided power spectrum P(m) = w_m |X(m)|^2 / N^2 of coefficients X [..., m] of lines of N columns, w = 1 for m = 0
    and for m = N/2 when N is even, else 2: the sum over all m = 0 .. N/2 is the zonal mean of x^2.  m_first: the wavenumber of
    X[..., 0]."""
    X = np.asarray(X)
    return _weights(X.shape[-1], N, m_first) * (X.real * X.real + X.imag * X.imag) / (float(N) * float(N))


def cospectrum(Xa, Xb, N, m_first=0):
    """The one-sided cospectrum w_m Re(Xa(m) conj(Xb(m))) / N^2, normalised like power_spectrum: the sum over all m is the zonal
    mean of a b (v and T: which scales carry the eddy heat flux).  The shapes must be equal."""
    Xa, Xb = np.asarray(Xa), np.asarray(Xb)
    if Xa.shape != Xb.shape:
        raise ValueError(f"cospectrum of coefficients shaped {Xa.shape} and {Xb.shape}")
    return _weights(Xa.shape[-1], N, m_first) * (Xa.real * Xb.real + Xa.imag * Xb.imag) / (float(N) * float(N))


def dominant_wavenumber(P, m_first=0):
    """The wavenumber of the largest power along the last axis of P [..., m] (the first of equals)."""
    return np.argmax(np.asarray(P), axis=-1) + m_first


def combine_spectra(parts, offsets):
    """The coefficients of the ranks of a decomposition (zonal_spectrum of every rank, in rank order) as those of the whole;
    offsets: (i0, j0) of every rank's interior in the global one.  The transform is linear and every rank has used the global
    column and N, so ranks with the same j0 hold parts of the same lines and ADD, in rank order, starting from +0.0; others are
    stacked by j0.  The sum is another order of the same terms than the single domain's: equal to round-off, not to the bit."""
    bands = {}
    for p, o in zip(parts, offsets):
        p = np.asarray(p, np.complex128)
        if o[1] not in bands:
            bands[o[1]] = np.zeros(p.shape, np.complex128)
        acc = bands[o[1]]
        if acc.shape != p.shape:
            raise ValueError(f"ranks of one band of rows hold coefficients shaped {acc.shape} and {p.shape}")
        acc.real, acc.imag = acc.real + p.real, acc.imag + p.imag
    return np.concatenate([bands[o] for o in sorted(bands)], axis=1)
