"""The numpy statement of the hydrostatic pressure (tests/pressure_spec.py) against the oracle and against itself in
np.longdouble: what keeps the reference of tests/test_gpu_pressure.py honest.  No GPU."""
import numpy as np
import pytest

import gb25_amd as gb
import pressure_spec as ps
from helpers import counter_rng, make_oracle
from oracle_backend import OracleBackend

G, RHO0 = 9.80665, 1020.0
# (shape, halo) of tests/test_gpu_pressure.py
GPU_CASES = [((150, 37, 6), 8), ((70, 21, 5), 4), ((450, 13, 4), 8), ((144, 64, 6), 8)]


def z_metrics(Nz, dtype=np.float64):
    """The model's vertical grid: Nz + 2 faces as numbers of the model's float type, centres and spacings from them in fp64."""
    ob = OracleBackend(16, 16, Nz, dt=1.0)
    zf = np.array([ob.metric("zf", k) for k in range(1, Nz + 3)])
    zc, dzf = ps.vertical_metrics(zf.astype(dtype).astype(np.float64))
    if dtype == np.float64:   # the oracle derives its own the same way
        assert np.array_equal(zc, [ob.metric("zc", k) for k in range(1, Nz + 1)])
        assert np.array_equal(dzf[1:], [ob.metric("dzf", k) for k in range(2, Nz + 2)])
    return zc, dzf


def test_density_matches_the_oracle():
    """Two statements of the polynomial -- the sum of monomials here, nested Horner there -- at 4096 points.  Each carries
    about 60 roundings of size <= u64 A / 2 (A = the sum of the absolute terms, 13 rho here) that add like a random walk,
    sqrt(60) u64 A / 2 = 4 u64 A together: 8 u64 A = 2^-50 A for the two, about 50 ulps of rho in the worst column."""
    ob = OracleBackend(16, 16, 6, dt=1.0)
    zc, dzf = z_metrics(6)
    n = 4096
    T = -2.0 + 34.0 * counter_rng((n,), 11, 1)
    S = 0.5 + 41.5 * counter_rng((n,), 11, 2)
    Z = -6000.0 * counter_rng((n,), 11, 3)
    Z[:8] = [zc[-1] - dzf[-2], zc[0], zc[-1], 0.0, -1000.0, -4000.0, -5999.0, -10.0]   # the mirrored level, the deepest centre, ...
    T[4], S[4] = 10.0, 30.0
    rho, A = ps.teos10_rho(T, S, Z)
    assert abs(rho[4] - 1027.45140) < 6e-6                                 # the published check value
    ref = np.array([ob.teos10_rho(t, s, z) for t, s, z in zip(T, S, Z)])
    err = np.abs(rho - ref)
    print("max |rho - oracle| = %.2e kg/m3 = %.1f ulps of rho, %.3f of the bound" % (err.max(), (err / np.spacing(ref)).max(), (err / (8 * ps.U64 * A)).max()))
    assert (err <= 8 * ps.U64 * A).all()
    assert (A > np.abs(rho)).all() and (A < 2e5).all()


def test_pressure_matches_the_fp64_oracle():
    Nx, Ny, Nz, H = 24, 13, 6, 8
    m = make_oracle(Nx, Ny, Nz, 600.0)
    T, S = ps.rest_state((Nx, Ny, Nz), "random")
    m.set(T=T, S=S)
    gb.update_state(m)
    Tp, Sp, got = m.tracers.T.parent, m.tracers.S.parent, m.pressure.pHY.parent
    zc, dzf = z_metrics(Nz)
    p, E = ps.pressure(Tp, Sp, zc, dzf, H, G, RHO0)
    # every cell compute_p writes: columns and rows -H+1 .. N+H-2, levels 0 .. Nz-1
    w = (slice(1, -1), slice(1, -1))
    err = np.abs(got[:, :, H:H + Nz] - p)[w]
    print("max |pHY - spec| / E_p = %.3f" % (err / E[w]).max())
    assert (err <= E[w]).all()
    inner = (slice(H, -H), slice(H, -H))
    assert (E[inner] < 2e-11 * np.abs(p[inner])).all()   # (what the bound is worth: 1e-11 of the pressure)


def masked(a, H, Nz, seed):
    """Like the immersed grids: zeros below a bottom that varies from column to column."""
    a = a.copy()
    kbot = (counter_rng(a.shape[:2], seed, 5) * (Nz + 1)).astype(int)
    k = np.arange(a.shape[2])[None, None, :] - H
    a[(k >= 0) & (k < kbot[:, :, None])] = 0.0
    return a


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["Float32", "Float64"])
@pytest.mark.parametrize("kind", ["random", "smooth"])
@pytest.mark.parametrize("shape,H", GPU_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"h{v}")
def test_float64_spec_is_within_a_quarter_of_its_bound(shape, H, kind, dtype):
    """The reference the GPU tests use is itself within E_p / 4 of the same expression evaluated in np.longdouble, on every
    state they use (here with the halos filled as the model fills them, and once more with immersed cells zeroed)."""
    if np.finfo(np.longdouble).eps >= 2.0 ** -60:
        pytest.fail("np.longdouble is no wider than 64 bits here: the reference cannot be checked")
    Nz = shape[2]
    zc, dzf = z_metrics(Nz, dtype)
    g, rho0 = float(dtype(G)), float(dtype(RHO0))
    T, S = ps.rest_state(shape, kind, dtype)
    Tp, Sp = ps.parent_from_interior(T, H), ps.parent_from_interior(S, H)
    for Tq, Sq in ((Tp, Sp), (masked(Tp, H, Nz, 3), masked(Sp, H, Nz, 3))):
        p, E = ps.pressure(Tq, Sq, zc, dzf, H, g, rho0)
        pl, El = ps.pressure(Tq, Sq, zc, dzf, H, g, rho0, longdouble=True)
        ratio = float((np.abs(p - pl) / El).max())
        print("max |p64 - p80| / E_p = %.4f" % ratio)
        assert ratio <= 0.25
        assert float((np.abs(E - El) / El).max()) < 1e-12
