"""The boundary forcing as statements between arrays a caller can read: numpy only.

TEST INFRASTRUCTURE ONLY.  Nothing under gb-25_amd/ imports this module, and it imports nothing from the library.  Written from the
formulas of the oracle's header comment ("data-free forcing", oracle/gb25_oracle.c) and the scalar fluxes_numpy of
tests/test_oracle_data_free.py, vectorised over PARENT arrays (halo cells included): the similarity-theory flux solve, its
interpolation onto the velocity faces, the quadratic bottom drag, and what compute_boundary_tendencies adds to the tendencies.

Index conventions.  A "centre array" has shape (Nx + 1, Ny + 1) and holds the logical cells i = -1 .. Nx-1, j = -1 .. Ny-1 at
[i + 1, j + 1]: the interior, one halo column to the west and one halo row to the south -- the centres the device computes
(k_similarity_fluxes: thread (0, 0) is cell (-1, -1); j_hi = Ny on every grid, so no row beyond a fold).  The oracle counts the
south row as land (inactive_cell: j < 1), the device computes it from the halo cells; the only value that reads it is J^v in row 0,
the face on the southern wall, which no tendency kernel applies.  `south_row_is_land` says which of the two is stated.

How every tolerance of tests/test_forcing_spec.py and tests/test_gpu_forcing_spec.py is formed:

    field                        against                       tolerance
    ---------------------------  ----------------------------  -----------------------------------------------------------------------
    J^u, J^v, J^T, J^S  fp64     similarity_fluxes (fp64)      RTOL_F64 = 1e-10 of the field's largest magnitude in the case: the tolerance
                                                               of test_the_c_restatement_is_the_formulas for this algorithm
    the same, oracle f32 build   the same                      1 u32 of the cell's own value: its loop is fp64, only the store rounds;
                                                               + RTOL_F64 of the scale, the row above: what is rounded is the oracle's
                                                               fp64 value, not the statement's (it matters below 2e-3 of the scale)
    the same, Float32 device     the same                      per regime FACTOR_F32 = 4 x the yardstick (loop_dtype = float32 against
                                                               float64 of THIS module, same case, field, regime) + 1 u32 of the value
    land, the unwritten J^v row  --                            exactly zero
    drag flux J                  bottom_drag (longdouble)      gamma(C_DRAG, u) Cd |u| sqrt(u^2 + A^2), A = sum |v_i| / 4.  C_DRAG = 8: the
                                                               three additions of the average (relative to A, and the root is 1-Lipschitz
                                                               in the average) (3), two squares and their sum (3, halved by the root: 1.5),
                                                               the root (1), two products with Cd and u (2): 7.5, rounded up.  Cd is the
                                                               number the build holds.
    G with - G without           boundary_contribution         gamma(c_apply(u), u) (|G without| + |J / dz|) (+ the drag flux's own bound
                                                               / dz).  c_apply = 3 in Float64: the reciprocal thickness of the table
                                                               (gb25_api.hip, recip(dzc)), its product with J and the sum
                                                               (tendency_kernels.hpp, `gu = gu - g.top_flux[0][o2] * rdz` and its siblings;
                                                               a contracted product lowers the count; the oracle divides and adds: 2).
                                                               c_apply = 4 in Float32: the table rounds 1 / dz of the fp64 thickness while
                                                               the accessor hands out the thickness rounded to the build, one more u.
    every other cell of G        --                            the same bits
"""
import numpy as np

from step_spec import LD, U32, gamma, unit_roundoff

RTOL_F64 = 1e-10
FACTOR_F32 = 4.0
C_DRAG = 8
REGIMES = ("land", "unstable", "stable", "clamped", "gust_floor", "lq_cap")
ATMOSPHERE = ("u", "v", "T", "q", "p", "shortwave", "longwave")

# the constants of the oracle's header comment
KAPPA, RD, RV, CPD, CPV, CPL, LV0, T0, PTR = 0.4, 287.0, 461.5, 1005.0, 1859.0, 4181.0, 2.5008e6, 273.16, 611.657
HEIGHT, ZI, BETA, CHARNOCK, NU, EMISSIVITY, ALBEDO = 10.0, 600.0, 1.2, 0.011, 1.5e-5, 0.97, 0.05
SIGMA, CP_OCEAN, RHO_FRESH = 5.670374419e-8, 3991.86795711963, 1000.0
GUST_FLOOR, LQ_CAP, ZETA_MAX = 0.2, 1.6e-4, 50.0


def c_apply(u_):
    return 4 if u_ == U32 else 3


# ---- where the solid is --------------------------------------------------------------------------------------------------------------
def surface_land(g, south_row_is_land=False):
    """Centre array: the column is solid up to the surface (kbot = Nz).  The west halo column is the periodic image of column
    Nx-1; the south halo row lies beyond the wall."""
    land = g["kbot"] >= g["Nz"]
    out = np.zeros((g["Nx"] + 1, g["Ny"] + 1), bool)
    out[1:, 1:] = land
    out[0, 1:] = land[-1]
    out[:, 0] = south_row_is_land
    return out


def first_free_levels(g):
    """(ku, kv) [i, j]: first level at which the x face (i, j) / the y face (i, j) touches no solid cell; Nz where none does.
    x is periodic; the y faces on a wall (row 0, and row Ny of a grid without a fold) never move: Nz."""
    kb, Nz, Ny = g["kbot"], g["Nz"], g["Ny"]
    ku = np.minimum(np.maximum(kb, np.roll(kb, 1, axis=0)), Nz)
    kv = np.full((g["Nx"], Ny if g["folded"] else Ny + 1), Nz)
    kv[:, 1:Ny] = np.minimum(np.maximum(kb[:, 1:], kb[:, :-1]), Nz)
    return ku, kv


# ---- the flux solve ---------------------------------------------------------------------------------------------------------------------
def _psi_blend(z, pk, y, t):
    r3 = t(np.sqrt(3.0))
    pc = t(1.5) * np.log((1 + y + y * y) / 3) - r3 * np.arctan((1 + 2 * y) / r3) + t(np.pi) / r3
    f = z * z / (1 + z * z)
    return (1 - f) * pk + f * pc


def psi_u(z, t):
    """COARE 3.5 stability function of momentum: Kansas / convective blend for zeta < 0, Beljaars-Holtslag for zeta >= 0."""
    zn, zp = np.minimum(z, 0), np.maximum(z, 0)
    x = np.sqrt(np.sqrt(1 - 15 * zn))
    pk = 2 * np.log((1 + x) / 2) + np.log((1 + x * x) / 2) - 2 * np.arctan(x) + t(np.pi / 2)
    neg = _psi_blend(zn, pk, np.cbrt(1 - t(10.15) * zn), t)
    pos = -(t(0.7) * zp + t(0.75) * (zp - t(5 / 0.35)) * np.exp(-np.minimum(t(0.35) * zp, 50)) + t(0.75 * 5 / 0.35))
    return np.where(z < 0, neg, pos)


def psi_q(z, t):
    zn, zp = np.minimum(z, 0), np.maximum(z, 0)
    pk = 2 * np.log((1 + np.sqrt(1 - 15 * zn)) / 2)
    neg = _psi_blend(zn, pk, np.cbrt(1 - t(34.15) * zn), t)
    s = 1 + t(2 / 3) * zp
    pos = -(s * np.sqrt(s) + t(2 / 3) * (zp - t(14.28)) * np.exp(-np.minimum(t(0.35) * zp, 50)) + t(8.525))
    return np.where(z < 0, neg, pos)


def _centres(a, H, Nx, Ny):
    return np.asarray(a, np.float64)[H - 1:H + Nx, H - 1:H + Ny]


def similarity_fluxes(atm, u, v, T, S, g, loop_dtype=np.float64, iterations=5, south_row_is_land=False):
    """(tau_x, tau_y, J^T, J^S, regimes): centre arrays (module docstring).  atm: {name: parent (Nx + 2H, Ny + 2H) array} for
    ATMOSPHERE; u, v, T, S: parent arrays as the model holds them; g: read_geometry's, with g["grav"], g["rho0"] the numbers
    of the build.  The ocean velocity at a centre is the average of its two faces at the top level.  On land everything is zero.
    loop_dtype = float32: the characteristic scales are iterated in numpy float32 from inputs rounded to it -- the place where the
    Float32 build leaves fp64; the thermodynamics before and the fluxes after stay fp64.
    regimes: {name: bool centre array} for REGIMES, to be taken from the fp64 run: `clamped` |zeta| = 50 in any iteration;
    `unstable` / `stable` the sign of zeta in the last iteration, never clamped; `gust_floor` U_g = 0.2 and `lq_cap`
    l_q = 1.6e-4 in the last iteration.  A cell may carry several."""
    H, Nx, Ny, Nz = g["H"], g["Nx"], g["Ny"], g["Nz"]
    top = H + Nz - 1
    c = lambda a: _centres(a, H, Nx, Ny)
    ua, va, Ta, qa, pa, Qsw, Qlw = (c(atm[n]) for n in ATMOSPHERE)
    u, v = np.asarray(u, np.float64)[:, :, top], np.asarray(v, np.float64)[:, :, top]
    uo = (u[H - 1:H + Nx, H - 1:H + Ny] + u[H:H + Nx + 1, H - 1:H + Ny]) / 2
    vo = (v[H - 1:H + Nx, H - 1:H + Ny] + v[H - 1:H + Nx, H:H + Ny + 1]) / 2
    To, So = c(np.asarray(T)[:, :, top]), c(np.asarray(S)[:, :, top])
    grav, rho0 = float(g["grav"]), float(g["rho0"])
    land = surface_land(g, south_row_is_land)
    with np.errstate(all="ignore"):
        Ts = To + 273.15
        psat = PTR * (Ts / T0) ** ((CPV - CPL) / RV) * np.exp((LV0 - (CPV - CPL) * T0) / RV * (1 / T0 - 1 / Ts))
        qs = 0.98 * (RD / RV) * psat / (pa - (1 - RD / RV) * psat)
        rho_a = pa / ((RD * (1 - qa) + RV * qa) * Ta)
        cpm = CPD * (1 - qa) + CPV * qa
        Lv = LV0 + (CPV - CPL) * (Ts - T0)
        du, dv = ua - uo, va - vo
        dth, dq = Ta + grav / cpm * HEIGHT - Ts, qa - qs
        Tv = Ta * (1 + 0.608 * qa)
        U = np.sqrt(du * du + dv * dv + GUST_FLOOR ** 2)
        chi0 = np.log(HEIGHT / 1e-4)
        us, ths, qst = KAPPA * U / chi0, KAPPA * dth / chi0, KAPPA * dq / chi0
        # ---- the iteration, in loop_dtype
        t = np.dtype(loop_dtype).type
        f = lambda a: np.asarray(a).astype(t)
        kap, h, gr, nu = t(KAPPA), t(HEIGHT), t(grav), t(NU)
        rTv, qaF, TaF, duF, dvF, dthF, dqF = f(1 / Tv), f(qa), f(Ta), f(du), f(dv), f(dth), f(dq)
        us, ths, qst, U = f(us), f(ths), f(qst), f(U)
        clamped = np.zeros(U.shape, bool)
        zeta = np.zeros(U.shape, t)
        Ug, lq = np.full(U.shape, t(GUST_FLOOR)), np.full(U.shape, t(LQ_CAP))
        for _ in range(iterations):
            bs = gr * rTv * (ths * (1 + t(0.608) * qaF) + t(0.608) * TaF * qst)
            Ug = np.maximum(t(GUST_FLOOR), t(BETA) * np.cbrt(np.maximum(-us * bs, t(0)) * t(ZI)))
            U = np.sqrt(duF * duF + dvF * dvF + Ug * Ug)
            lu = t(CHARNOCK) * us * us / gr + t(0.11) * nu / us
            lq = np.minimum(t(LQ_CAP), t(5.8e-5) / (lu * us / nu) ** t(0.72))
            zeta = np.clip(kap * h * bs / (us * us), t(-ZETA_MAX), t(ZETA_MAX))
            clamped |= np.abs(zeta) == t(ZETA_MAX)
            chiu = np.log(h / lu) - psi_u(zeta, t) + psi_u(zeta * lu / h, t)
            chiq = np.log(h / lq) - psi_q(zeta, t) + psi_q(zeta * lq / h, t)
            us, ths, qst = kap * U / chiu, kap * dthF / chiq, kap * dqF / chiq
        regimes = dict(land=land, clamped=clamped & ~land, unstable=(zeta < 0) & ~clamped & ~land, stable=(zeta > 0) & ~clamped & ~land,
                       gust_floor=(Ug == t(GUST_FLOOR)) & ~land, lq_cap=(lq == t(LQ_CAP)) & ~land)
        us, ths, qst, U = (np.asarray(a, np.float64) for a in (us, ths, qst, U))
        # ---- the fluxes, positive upward
        taux, tauy = rho_a * us * us * du / U, rho_a * us * us * dv / U
        Q = -rho_a * cpm * us * ths - rho_a * Lv * us * qst + EMISSIVITY * (SIGMA * Ts ** 4 - Qlw) - (1 - ALBEDO) * Qsw
        JT = Q / (rho0 * CP_OCEAN)
        JS = -So * (-rho_a * us * qst) / RHO_FRESH
    zero = lambda a: np.where(land, 0.0, a)
    return zero(taux), zero(tauy), zero(JT), zero(JS), regimes


def stress_to_faces(tau_x, tau_y, g):
    """(J^u, J^v) at the interior faces from the centre arrays of the stress: J^u = -Ix(tau_x) / rho0 on rows 0 .. Ny-1,
    J^v = -Iy(tau_y) / rho0 on rows 0 .. Ny-1 -- the rows atmosphere_ocean_fluxes_impl launches k_stress_to_faces for (j_hi = Ny).
    J^v has Ny + 1 rows on a grid without a fold: row Ny, the face on the northern wall, is NEVER written and keeps the zero it was
    allocated with.  (A folded grid has Ny rows of y faces: all written.)"""
    rho0 = float(g["rho0"])
    Ju = -(tau_x[:-1, 1:] + tau_x[1:, 1:]) / 2 / rho0
    Jv = np.zeros((g["Nx"], g["Ny"] if g["folded"] else g["Ny"] + 1))
    Jv[:, :g["Ny"]] = -(tau_y[1:, :-1] + tau_y[1:, 1:]) / 2 / rho0
    return Ju, Jv


def top_fluxes(atm, u, v, T, S, g, **kw):
    """({u, v, T, S: interior-shaped flux}, regimes): the two statements above chained, shaped like top_flux(name)."""
    tx, ty, JT, JS, regimes = similarity_fluxes(atm, u, v, T, S, g, **kw)
    Ju, Jv = stress_to_faces(tx, ty, g)
    return dict(u=Ju, v=Jv, T=JT[1:, 1:], S=JS[1:, 1:]), regimes


def regimes_at(regimes, name, rows=None):
    """The regime masks carried to the points of flux `name`: a face belongs to every regime of the two centres it averages
    (rows: the rows of the flux array; the unwritten row of J^v belongs to none)."""
    out = {}
    for r, m in regimes.items():
        if name == "u":
            a = m[:-1, 1:] | m[1:, 1:]
        elif name == "v":
            a = m[1:, :-1] | m[1:, 1:]
        else:
            a = m[1:, 1:]
        if rows is not None and rows > a.shape[1]:
            a = np.concatenate([a, np.zeros((a.shape[0], rows - a.shape[1]), bool)], axis=1)
        out[r] = a
    return out


# ---- the quadratic bottom drag --------------------------------------------------------------------------------------------------------
def bottom_drag(u, v, g, Cd, dtype=None, points=4):
    """{u, v: J, bound_u, bound_v, ku, kv}: J = -Cd u sqrt(u^2 + Ixy(v)^2) at the first free level of every x face (i, j), the
    other component averaged over the four y faces around it (i-1 and i, j and j+1), and likewise for the y faces (x faces i and
    i+1, j-1 and j); zero where the face's column is solid, and for v on the southern wall (and the northern one).  From the parent
    arrays.  dtype: evaluated in that type in the order the formula is written (the build's); None: np.longdouble.  bound: the
    module docstring's, for any evaluation in arithmetic of unit round-off u(dtype) (zero with dtype None).  points = 2: the WRONG
    average over the first two faces only (tests/test_forcing_spec.py shows that the judges notice it)."""
    H, Nx, Ny, Nz = g["H"], g["Nx"], g["Ny"], g["Nz"]
    t = LD if dtype is None else np.dtype(dtype).type
    u, v = np.asarray(u).astype(t), np.asarray(v).astype(t)
    Cd = t(Cd)
    ku, kv = first_free_levels(g)
    ii, jj = np.meshgrid(np.arange(Nx) + H, np.arange(Ny) + H, indexing="ij")
    out = {}
    for name, kf, vel, other, corners in (("u", ku, u, v, ((-1, 0), (0, 0), (-1, 1), (0, 1))),
                                          ("v", kv[:, :Ny], v, u, ((0, -1), (1, -1), (0, 0), (1, 0)))):
        k = np.minimum(kf, Nz - 1) + H
        own = vel[ii, jj, k]
        parts = [other[ii + di, jj + dj, k] for di, dj in corners]
        avg = (((parts[0] + parts[1]) + parts[2]) + parts[3]) / t(4) if points == 4 else (parts[0] + parts[1]) / t(2)
        A = sum(np.abs(p).astype(LD) for p in parts) / 4
        J = np.where(kf < Nz, -Cd * own * np.sqrt(own * own + avg * avg), t(0))
        bound = np.where(kf < Nz, LD(Cd) * np.abs(own).astype(LD) * np.sqrt(own.astype(LD) ** 2 + A ** 2), LD(0))
        bound = bound * (0.0 if dtype is None else gamma(C_DRAG, unit_roundoff(dtype)))
        if name == "v" and not g["folded"]:
            J, bound = (np.concatenate([a, np.zeros((Nx, 1), a.dtype)], axis=1) for a in (J, bound))
        out[name], out["bound_" + name] = J, bound
    out["ku"], out["kv"] = ku, kv
    return out


# ---- what the tendencies receive ----------------------------------------------------------------------------------------------------------
def boundary_contribution(J_top, J_bottom, g):
    """({name: increment [i, j, k] in longdouble}, {name: touched [i, j, k]}) for the names of J_top (u, v, T, S) and J_bottom
    (u, v): -J_top / dz(Nz) at the top level where the face or cell is active, +J_bottom / dz(k_first) at the first free level of
    the face, zero elsewhere -- compute_boundary_tendencies of the oracle: a face that touches a solid cell at that level and an
    inactive cell are skipped, and so is every v face of row 0 (and of the northern wall)."""
    Nx, Ny, Nz = g["Nx"], g["Ny"], g["Nz"]
    dz = np.asarray(g["dz"]).astype(LD)
    ku, kv = first_free_levels(g)
    first = dict(u=ku, v=kv, T=np.minimum(g["kbot"], Nz), S=np.minimum(g["kbot"], Nz))
    inc, touched = {}, {}
    for n in set(J_top or {}) | set(J_bottom or {}):
        kf = first[n]
        a = np.zeros(kf.shape + (Nz,), LD)
        m = np.zeros(a.shape, bool)
        free = kf < Nz
        if J_top and J_top.get(n) is not None:
            a[:, :, Nz - 1] += np.where(free, -np.asarray(J_top[n]).astype(LD) / dz[Nz - 1], 0)
            m[:, :, Nz - 1] |= free
        if J_bottom and J_bottom.get(n) is not None:
            k = np.minimum(kf, Nz - 1)
            at = np.arange(Nz)[None, None, :] == k[:, :, None]
            at &= free[:, :, None]
            a += np.where(at, (np.asarray(J_bottom[n]).astype(LD) / dz[k])[:, :, None], 0)
            m |= at
        inc[n], touched[n] = a, m
    return inc, touched


def application_bound(G_without, inc, u_, extra=0):
    """gamma(c_apply, u) (|G without| + |J / dz|) + extra (the module docstring)."""
    return gamma(c_apply(u_), u_) * (np.abs(np.asarray(G_without).astype(LD)) + np.abs(inc)) + extra


# ---- judges ----------------------------------------------------------------------------------------------------------------------------
def judge_flux(label, name, got, want, regimes=None, tol=None):
    """One flux field cell by cell.  tol: array of absolute tolerances, or None for RTOL_F64 of the field's largest magnitude.
    Returns the worst |got - want| / tolerance."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, f"{label}: J^{name} has shape {got.shape}, the statement {want.shape}"
    assert np.isfinite(got).all(), f"{label}: J^{name} is not finite at {tuple(np.argwhere(~np.isfinite(got))[0])}"
    assert np.isfinite(want).all(), f"{label}: the statement of J^{name} is not finite"
    scale = np.abs(want).max()
    assert scale > 0, f"{label}: J^{name} carries no signal"
    tol = np.full(want.shape, RTOL_F64 * scale) if tol is None else np.asarray(tol, np.float64)
    d = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(tol > 0, d / np.where(tol > 0, tol, 1), np.where(d == 0, 0.0, np.inf))
    at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    names = [r for r, m in (regimes or {}).items() if m[at]]
    assert ratio[at] <= 1.0, (f"{label}: J^{name} at {tuple(int(q) for q in at)} {names} is {got[at]:.12g}, the statement {want[at]:.12g}: "
                              f"{ratio[at]:.4g} x the tolerance")
    return float(ratio[at])


def deviation_by_regime(got, want, regimes):
    """{regime: largest |got - want| / max |want|} over the cells of each regime (nan where a regime is empty)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = np.abs(want).max()
    d = np.abs(got - want) / scale
    return {r: (float(d[m].max()) if m.any() else float("nan")) for r, m in regimes.items() if r != "land"}
