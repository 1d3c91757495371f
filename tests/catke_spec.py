"""An independent numpy statement of the CATKE restatement, cell by cell: what ONE compute_diffusivities! does to a model
state -- the e step (substep_turbulent_kinetic_energy! + the implicit solve), the filtered surface buoyancy flux, the
diffusivities, and the cells outside the interior the call writes.  Written from the formulas in the header comment of the
CATKE section of oracle/gb25_oracle.c, array-wise in np.longdouble, sharing no code with the C loops or the kernels.
TEST INFRASTRUCTURE ONLY: nothing under gb-25_amd/ imports this module; a backend is only asked through its accessors.
[UPSTREAM-UNVERIFIED like the oracle itself: it pins the implementations to the stated formulas, not the formulas to Oceananigans.]

Indices are 0-based: cell k = 0 .. Nz-1, face f = 0 .. Nz between the cells f-1 and f, kbot = number of dry levels of a column
(step_spec.read_geometry).  The rules of an immersed bottom, from the same header:
    a face is OPEN when 1 <= f <= Nz-1 and both its cells are wet (f > kbot); N^2, the lengths and the kappas are zero elsewhere;
    dz u at the x face i vanishes where a node is inactive -- both cells beside it dry: f <= min(kbot[i-1], kbot[i]) -- and on the
    faces 0 and Nz; dz v likewise with the rows j-1, j; beyond a wall every cell is dry, beyond the fold it is the image's;
    the bottom flux -CWeps sqrt(max(e, 0)) / dz belongs to the first wet cell k = kbot; zbot = zf[kbot], Hcol = zf[Nz] - zbot;
    on land (kbot = Nz) J^b = 0 and the surface source is 0; dry cells keep e, G^-.e, and have L^e = 0.

The measure of a judged quantity X is r = |X_got - X_spec| / (u s): u the unit round-off of the build, s a per-cell scale --
the sum of the absolute values of the terms that are added to make X; for products and quotients the magnitude of the spec's
value; for the solved e the largest |e*| of the column.  judge() asserts r <= C_<field>, the constants below.

The cells whose value rests on a DISCONTINUOUS switch with an argument within 64 u of its threshold (relative to the argument's
scale) are left out: the sign of N^2 at a face and at the face above (convecting / entraining, Cun against Clo), the sign of the
centred N^2 (the same choice in the dissipation length), J^b > J^b_min, e > e_min in L^e, e < 0 in omega.  max(e, e_min), min /
max of lengths, the clip of Ri and min / max(wb, 0) are continuous and are not flagged.  At most 0.1 % of a field may be left out.

What the call writes outside the interior (outside_table; read off the header comments of k_catke_tke_step, k_catke_surface_flux,
k_catke_diffusivities, k_catke_fold and the host path catke_tke_step_impl / catke_diffusivities_finish_impl):
    kappa_u, kappa_c, kappa_e   face levels 0 .. Nz of every interior column; their periodic x images in all H halo columns;
    L^e                         levels 0 .. Nz-1 likewise, and the bottom / top layer (levels -1, Nz <- 0, Nz-1) on interior rows;
    J^b                         the interior and its x images;
    beside a wall               ONE y layer (row -1 <- row 0, row Ny <- row Ny-1), with its x images; not L^e's bottom / top layer;
    on a folded grid            the H rows beyond the pivot row over EVERY parent column, (i, Ny-1+q) <- (Nx-1-i mod Nx, Ny-1-q):
                                face levels 0 .. Nz of the three kappa, levels -1 .. Nz of L^e (source level clamped), J^b.
Every other parent cell keeps its bits."""
import numpy as np

import pressure_spec
import step_spec as ss
from step_spec import LD

DEFAULTS = dict(Cs=1.131, Cb=0.28, Csp=0.505, CRid=1.02, CRi0=0.254,
                Chi=(0.242, 0.098, 0.548, 0.579), Clo=(0.361, 0.198, 7.863, 1.604), Cun=(0.370, 0.369, 1.447, 0.923),
                Cc=(3.705, 4.793, 3.642, 3.254), Ce=(0.0, 0.112, 0.0, 0.0), CWu=3.179, CWw=0.383,
                emin=1e-9, Jbmin=1e-11, tau_neg=60.0, CWeps=1.0)
G, RHO0 = 9.80665, 1020.0
NEAR = 64            # a switch's argument within NEAR u of its threshold: the cell is left out
MAX_LEFT_OUT = 1e-3

# C_<field>: 4 x the largest r the ORACLE reaches (Float64 and Float32, every grid, Nz 6, 33, 65: tests/test_catke_spec.py);
# the measured value stands beside each.  The factor 4 covers another association of the sums, FMA contraction, the one
# reciprocal per column rjb where the oracle divides, and the 1-ulp reciprocal of the pivot in the register solve.
C_GM = 4 * 5.57      # G^-.e, the total tendency                    measured 5.57
C_LE = 4 * 3.58      # L^e                                          measured 3.58
C_E = 4 * 13.5       # e after the solve                            measured 13.5
C_KU = 4 * 5.61      # kappa_u                                      measured 5.61
C_KC = 4 * 5.24      # kappa_c                                      measured 5.24
C_KE = 4 * 5.98      # kappa_e                                      measured 5.98
C_JB = 4 * 1.58      # J^b after the filter                         measured 1.58
C_SRC = 4 * 4.73     # the surface source in G^n.e (still case)     measured 4.73
C = {"Gm.e": C_GM, "Le": C_LE, "e": C_E, "kappa_u": C_KU, "kappa_c": C_KC, "kappa_e": C_KE, "Jb": C_JB, "source": C_SRC}


def parameters(dtype=np.float64, P=DEFAULTS):
    """The closure's parameters as numbers of the build (each rounded once, as every implementation holds them)."""
    t = np.dtype(dtype).type
    return {k: tuple(float(t(x)) for x in v) if isinstance(v, tuple) else float(t(v)) for k, v in P.items()}


# ---- alpha and beta: the polynomial of pressure_spec (its table R) differentiated term by term -------------------------------
def teos10_sensitivities(Theta, Sa, Z):
    """(-d rho / d Theta, d rho / d S_A) [kg/m3/K, kg/m3/(g/kg)] and the sums of the absolute values of their terms; longdouble."""
    Theta, Sa, Z = np.broadcast_arrays(*(ss._ld(a) for a in (Theta, Sa, Z)))
    tau, zeta = Theta * LD(0.025), -Z * LD(1e-4)
    s = np.sqrt((Sa + LD(32.0)) * LD(0.875 / 35.16504))
    sp, tp, zp = (pressure_spec._powers(a, 6) for a in (s, tau, zeta))
    dT, dS, aT, aS = (np.zeros(s.shape, LD) for _ in range(4))
    for (i, j, k), c in pressure_spec.R.items():
        if j > 0:
            term = LD(c) * j * sp[i] * tp[j - 1] * zp[k]
            dT, aT = dT + term, aT + np.abs(term)
        if i > 0:
            term = LD(c) * i * sp[i - 1] * tp[j] * zp[k]
            dS, aS = dS + term, aS + np.abs(term)
    ds = LD(0.875 / 35.16504) / (2 * s)          # d s / d S_A
    return -dT * LD(0.025), dS * ds, aT * LD(0.025), aS * ds


# ---- the inputs of one call ---------------------------------------------------------------------------------------------------
FIELDS_IN = ("u", "v", "T", "S", "e", "kappa_u", "kappa_c", "Jb", "previous_u", "previous_v", "Gn.e", "Gm.e")


class Inputs:
    """Everything one compute_diffusivities! reads: parent arrays `f` (as the model holds them), geometry `g`
    (step_spec.read_geometry: Nx, Ny, Nz, H, kbot, folded), the vertical grid, the parameters and constants of the build."""

    def __init__(self, b, g, dt, chi=0.1, fields=None, top_flux=None):
        self.g, self.dtype = g, np.dtype(b.dtype)
        self.Nx, self.Ny, self.Nz, self.H = g["Nx"], g["Ny"], g["Nz"], g["H"]
        Nz = self.Nz
        self.f = dict(fields) if fields is not None else {n: b.get_field(n, True) for n in FIELDS_IN}
        self.zf = ss._ld([b.metric("zf", k) for k in range(1, Nz + 2)])
        self.zc = ss._ld([b.metric("zc", k) for k in range(1, Nz + 1)])
        self.dzc = ss._ld([b.metric("dzc", k) for k in range(1, Nz + 1)])
        self.dzf = ss._ld([b.metric("dzf", k) for k in range(1, Nz + 2)])    # dzf[f]: between the centres f-1 and f
        self.kb = np.asarray(g["kbot"], int)
        self.P = parameters(self.dtype)
        t = self.dtype.type
        self.grav, self.rho0, self.dt = LD(float(t(G))), LD(RHO0), LD(float(t(dt)))
        self.C1, self.C2 = (LD(c) for c in ss.ab2_coefficients(chi, False, self.dtype))
        self.top_flux = {n: (None if a is None else np.asarray(a, self.dtype)) for n, a in (top_flux or {}).items()}
        self.u_ = ss.unit_roundoff(self.dtype)
        self.mut = frozenset()          # wrong formulas, by name: the mutation tests of tests/test_catke_spec.py

    def but(self, mut=(), **fields):
        """A copy with some parent arrays replaced (`kbot=`: the geometry's) and / or wrong formulas switched on."""
        import copy
        x = copy.copy(self)
        x.f = dict(self.f)
        if "kbot" in fields:
            x.kb = np.asarray(fields.pop("kbot"), int)
        x.f.update(fields)
        x.mut = frozenset(mut) | self.mut
        return x

    def cells(self, name, di=0, dj=0):
        H, a = self.H, self.f[name] if isinstance(name, str) else name
        return ss._ld(a[H + di:H + di + self.Nx, H + dj:H + dj + self.Ny, H:H + self.Nz])

    def faces(self, name, di=0, dj=0):
        H, a = self.H, self.f[name] if isinstance(name, str) else name
        return ss._ld(a[H + di:H + di + self.Nx, H + dj:H + dj + self.Ny, H:H + self.Nz + 1])

    def column(self, name):
        H = self.H
        return ss._ld(self.f[name][H:H + self.Nx, H:H + self.Ny, 0])

    # the first level from which the nodes of the x faces i (di = 0), i+1 (di = 1) / the y faces j, j+1 are active
    def node_levels(self, axis, d):
        kb, Nz = self.kb, self.Nz
        if axis == 0:
            lo = np.roll(kb, 1 - d, axis=0)         # d = 0: column i-1; d = 1: column i
            hi = np.roll(kb, -d, axis=0)            # d = 0: column i;   d = 1: column i+1
            return np.minimum(lo, hi)
        south = np.concatenate([np.full((self.Nx, 1), Nz), kb[:, :-1]], axis=1)
        beyond = kb[::-1, self.Ny - 2:self.Ny - 1] if self.g["folded"] else np.full((self.Nx, 1), Nz)
        north = np.concatenate([kb[:, 1:], beyond], axis=1)
        return np.minimum(south, kb) if d == 0 else np.minimum(kb, north)

    def dz_velocity(self, name, axis, d):
        """dz of u (axis 0) / v (axis 1) at the face i + d / j + d of every interior column, on the faces 0 .. Nz"""
        c = self.cells(name, d, 0) if axis == 0 else self.cells(name, 0, d)
        out = np.zeros((self.Nx, self.Ny, self.Nz + 1), LD)
        out[:, :, 1:self.Nz] = (c[:, :, 1:] - c[:, :, :-1]) / self.dzf[1:self.Nz]
        if "shear not masked" in self.mut:
            return out
        return np.where(np.arange(self.Nz + 1)[None, None, :] > self.node_levels(axis, d)[:, :, None], out, LD(0))


def _sigma(P, p, Ri, amp=1):
    """(sigma_psi(Ri), the sum of the absolute values of its terms); amp: the scale of Ri's numerator over its magnitude"""
    t = (Ri - P["CRi0"]) / P["CRid"]
    st = np.clip(t, 0.0, 1.0)
    ramp = (t > 0) & (t < 1)
    mid = P["Clo"][p] + (P["Chi"][p] - P["Clo"][p]) * st
    smid = np.where(ramp, abs(P["Clo"][p]) + abs(P["Chi"][p] - P["Clo"][p]) * (np.abs(Ri) * amp + P["CRi0"]) / P["CRid"], np.abs(mid))
    return np.where(Ri < 0, LD(P["Cun"][p]), mid), np.where(Ri < 0, LD(P["Cun"][p]), smid)


def face_state(x, e=None, Jb=None):
    """N^2, S^2, the three kappa and the convective dissipation length at the faces 0 .. Nz of every interior column, each
    with its scale (s_*), and the faces near a switch (near)."""
    P, Nz, u_ = x.P, x.Nz, x.u_
    e = x.cells("e") if e is None else ss._ld(e)
    Jb = x.column("Jb") if Jb is None else ss._ld(Jb)
    T, S = x.cells("T"), x.cells("S")
    f_ = np.arange(Nz + 1)[None, None, :]
    is_open = (f_ >= 1) & (f_ <= Nz - 1) & (f_ > x.kb[:, :, None])
    zero = lambda: np.zeros((x.Nx, x.Ny, Nz + 1), LD)
    N2, sN2, fN2 = zero(), zero(), zero()
    if Nz > 1:
        dT, dS = T[:, :, 1:] - T[:, :, :-1], S[:, :, 1:] - S[:, :, :-1]
        al, be, aT, aS = teos10_sensitivities((T[:, :, 1:] + T[:, :, :-1]) / 2, (S[:, :, 1:] + S[:, :, :-1]) / 2, x.zf[1:Nz][None, None, :])
        N2[:, :, 1:Nz] = x.grav * (al * dT - be * dS) / x.dzf[1:Nz] / x.rho0
        # (alpha and beta are sums themselves: their scales are the sums of the absolute values of the polynomial's terms)
        sN2[:, :, 1:Nz] = x.grav * (aT * np.abs(dT) + aS * np.abs(dS)) / x.dzf[1:Nz] / x.rho0
        fN2[:, :, 1:Nz] = x.grav * (np.abs(al * dT) + np.abs(be * dS)) / x.dzf[1:Nz] / x.rho0      # the scale of the switch's argument
    N2, sN2, fN2 = np.where(is_open, N2, LD(0)), np.where(is_open, sN2, LD(0)), np.where(is_open, fN2, LD(0))
    S2 = (x.dz_velocity("u", 0, 0) ** 2 + x.dz_velocity("u", 0, 1) ** 2) / 2 + (x.dz_velocity("v", 1, 0) ** 2 + x.dz_velocity("v", 1, 1) ** 2) / 2
    w = np.sqrt(np.maximum(e, P["emin"]))
    mean = lambda a: np.concatenate([np.zeros_like(a[:, :, :1]), (a[:, :, 1:] + a[:, :, :-1]) / 2, np.zeros_like(a[:, :, :1])], axis=2)
    ws, ws2, ws3 = mean(w), mean(w * w), mean(w * w * w)
    zbot = x.zf[x.kb][:, :, None]
    Hcol = x.zf[Nz] - zbot
    Jb3, Jbe = Jb[:, :, None], LD(P["Jbmin"])
    with np.errstate(divide="ignore", invalid="ignore"):
        Ri = np.where(N2 == 0, LD(0), N2 / S2)
        d = np.minimum(np.maximum(P["Cs"] * (x.zf[Nz] - x.zf[None, None, :]), 0), np.maximum(P["Cb"] * (x.zf[None, None, :] - zbot), 0))
        lN = ws / np.sqrt(np.where(N2 > 0, N2, LD(1)))
        ls = np.where(N2 > 0, np.minimum(d, lN), d)
        ampN = np.where(N2 != 0, sN2 / np.where(N2 != 0, np.abs(N2), LD(1)), LD(1))      # the scale of N^2 over its magnitude
        m_ls = np.where((N2 > 0) & (lN < d), (1 + ampN) / 2, LD(1))                       # ... of which N^-1 carries half
        N2above = np.concatenate([N2[:, :, 1:], np.zeros_like(N2[:, :, :1])], axis=2)
        if "N2 above is N2" in x.mut:
            N2above = N2
        conv = (Jb3 > Jbe) & (N2 < 0)
        entr = (Jb3 > Jbe) & (N2 > 0) & (N2above < 0)
        Sp = P["Csp"] * np.sqrt(S2) * ws2 / (Jb3 + Jbe)
        esp = 1 - Sp
        lconv, slconv = [], []
        for p in range(4):
            raw = np.where(conv, P["Cc"][p] * ws3 / (Jb3 + Jbe), P["Ce"][p] * Jb3 / (ws * N2 + Jbe))
            on = conv | entr
            lconv.append(np.where(on, np.maximum(esp * raw, 0), LD(0)))
            slconv.append(np.where(on, (1 + Sp) * np.abs(raw) * np.where(conv, LD(1), ampN), LD(0)))
        out = dict(N2=N2, S2=S2, sN2=sN2, fN2=fN2, open=is_open, ws=ws)
        for p, n in enumerate(("ku", "kc", "ke")):
            sg, ssg = _sigma(P, p, Ri, ampN)
            l = np.minimum(Hcol, np.maximum(sg * ls, lconv[p]))
            out[n] = np.where(is_open, l * ws, LD(0))
            # (the cap at H cuts the scale only where it cuts the length)
            out["s_" + n] = np.where(is_open, np.where(l >= Hcol, Hcol, np.maximum(ssg * ls * m_ls, slconv[p])) * ws, LD(0))
        out["convD"], out["s_convD"] = np.where(is_open, lconv[3], LD(0)), np.where(is_open, slconv[3], LD(0))
    # faces near a switch: the sign of N^2 here or on the face above, J^b against J^b_min
    nearN = is_open & (np.abs(N2) <= NEAR * u_ * fN2)
    nearJ = np.abs(Jb3 - Jbe) <= NEAR * u_ * (np.abs(Jb3) + Jbe)
    out["near"] = nearN | np.concatenate([nearN[:, :, 1:], np.zeros_like(nearN[:, :, :1])], axis=2) | (nearJ & is_open)
    return out


def centre_length(x, F, e):
    """the dissipation length at the centres (c,c,c) of the wet cells, its scale, and the cells near the switch of its own Ri"""
    P, Nz = x.P, x.Nz
    c = lambda a: (a[:, :, :-1] + a[:, :, 1:]) / 2
    N2, S2, lh, slh, sN2 = c(F["N2"]), c(F["S2"]), c(F["convD"]), c(F["s_convD"]), c(F["sN2"])
    zbot = x.zf[x.kb][:, :, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        Ri = np.where(N2 == 0, LD(0), N2 / S2)
        d = np.minimum(np.maximum(P["Cs"] * (x.zf[Nz] - x.zc[None, None, :]), 0), np.maximum(P["Cb"] * (x.zc[None, None, :] - zbot), 0))
        wc = np.sqrt(np.maximum(e, P["emin"]))
        lN = wc / np.sqrt(np.where(N2 > 0, N2, LD(1)))
        ls = np.where(N2 > 0, np.minimum(d, lN), d)
        ampN = np.where(N2 != 0, sN2 / np.where(N2 != 0, np.abs(N2), LD(1)), LD(1))
        m_ls = np.where((N2 > 0) & (lN < d), (1 + ampN) / 2, LD(1))
        sg, ssg = _sigma(P, 3, Ri, ampN)
        Hcol = x.zf[Nz] - zbot
        l = np.minimum(Hcol, np.maximum(ls / sg, lh))
        # (a quotient by sigma: its relative error is that of sigma, ssg / sg)
        sl = np.where(l >= Hcol, Hcol, np.maximum(ls / sg * (ssg / sg) * m_ls, slh))
    near = (N2 != 0) & (np.abs(N2) <= NEAR * x.u_ * c(F["fN2"]))
    return l, np.maximum(sl, l), near


def shear_production(x):
    """(P, the sum of the absolute values of its terms): Ix [Iz(nu dz u- dzf dz u+) + Iz(nu dz u+ dzf dz u+)] / (2 dzc) + the
    same in y, nu = the OLD kappa_u averaged to the face's column from the PARENT array as it is (halo columns included)"""
    ku = x.f["kappa_u"]

    def half(axis, d):
        lo = (d - 1, 0) if axis == 0 else (0, d - 1)
        hi = (d, 0) if axis == 0 else (0, d)
        if axis == 0 and d == 0 and "kappa_u west with i+1" in x.mut:
            lo = (1, 0)
        if axis == 1 and d == 0 and "kappa_u south with j+1" in x.mut:
            lo = (0, 1)
        nu = (x.faces(ku, *lo) + x.faces(ku, *hi)) / 2
        prev, cur = ("previous_u", "u") if axis == 0 else ("previous_v", "v")
        dm, dp = x.dz_velocity(prev, axis, d), x.dz_velocity(cur, axis, d)
        a, b = nu * dm * x.dzf * dp, nu * dp * x.dzf * dp
        iz = lambda q: (q[:, :, :-1] + q[:, :, 1:]) / 2
        return (iz(a) + iz(b)) / (2 * x.dzc), (iz(np.abs(a)) + iz(np.abs(b))) / (2 * x.dzc)

    parts = [half(0, 0), half(0, 1), half(1, 0), half(1, 1)]
    return ((parts[0][0] + parts[1][0]) / 2 + (parts[2][0] + parts[3][0]) / 2, (parts[0][1] + parts[1][1]) / 2 + (parts[2][1] + parts[3][1]) / 2)


def solve_columns(x, rhs, ke, L):
    """(1 - dt dz kappa_e dz - dt L^e) e = rhs per column from its first wet level on, dry cells unchanged: one Thomas sweep
    over the levels, vectorised over the columns, in longdouble."""
    Nz, dt = x.Nz, x.dt
    k_ = np.arange(Nz)[None, None, :]
    wet = k_ >= x.kb[:, :, None]
    lo = np.where(wet & (k_ > x.kb[:, :, None]), -dt * ke[:, :, :Nz] / (x.dzc * x.dzf[:Nz]), LD(0))
    up = np.where(wet & (k_ < Nz - 1), -dt * ke[:, :, 1:] / (x.dzc * x.dzf[1:]), LD(0))
    dg = np.where(wet, 1 - lo - up - dt * L, LD(1))
    out, gam = np.array(rhs, LD), np.zeros(rhs.shape, LD)
    bet = dg[:, :, 0].copy()
    out[:, :, 0] = out[:, :, 0] / bet
    for k in range(1, Nz):
        gam[:, :, k] = up[:, :, k - 1] / bet
        bet = dg[:, :, k] - lo[:, :, k] * gam[:, :, k]
        out[:, :, k] = (out[:, :, k] - lo[:, :, k] * out[:, :, k - 1]) / bet
    for k in range(Nz - 2, -1, -1):
        out[:, :, k] = out[:, :, k] - gam[:, :, k + 1] * out[:, :, k + 1]
    return out


def tke_step(x, Gm_got=None, Le_got=None):
    """time_step_catke_equation!: G^-.e (the total tendency), L^e, the kappa_e it solves with, e* and e, with their scales and the
    cells near a switch.  Gm_got: e* is rebuilt from THIS total tendency (the implementation's own) instead of the spec's.
    Le_got: in a cell whose L^e sits near a switch (and is left out for that) the solve takes the implementation's own L^e, so
    that the rest of its column is still judged; a face near a switch (kappa_e) leaves the whole column of e out."""
    P, Nz = x.P, x.Nz
    e, k_ = x.cells("e"), np.arange(Nz)[None, None, :]
    wet = k_ >= x.kb[:, :, None]
    F = face_state(x)
    kc = x.faces("kappa_c")
    wbf = -(kc * F["N2"])
    swbf = np.abs(kc) * F["sN2"]
    wb, swb = (wbf[:, :, :-1] + wbf[:, :, 1:]) / 2, (swbf[:, :, :-1] + swbf[:, :, 1:]) / 2
    lD, slD, nearD = centre_length(x, F, e)
    floor = e > P["emin"] if "no e_min floor in Le" not in x.mut else np.ones(e.shape, bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        omega = np.where(e < 0, LD(1) / P["tau_neg"], np.sqrt(np.abs(e)) / lD)
        somega = np.where(e < 0, omega, omega * slD / lD)
        first = np.where(floor, np.minimum(wb, 0) / e, LD(0))
        sfirst = np.where(floor & (wb < 0), swb / np.abs(e), LD(0))
    bottom = k_ == (0 if "bottom flux on level 0" in x.mut else x.kb[:, :, None])
    divJ = np.where(bottom, -(P["CWeps"] * np.sqrt(np.maximum(e, 0)) / x.dzc), LD(0))
    L, sL = np.where(wet, first - omega + divJ, LD(0)), np.where(wet, sfirst + np.abs(somega) + np.abs(divJ), LD(0))
    Pr, sPr = shear_production(x)
    Gn, Gm_old = x.cells("Gn.e"), x.cells("Gm.e")
    total = np.where(wet, Gn + (Pr + np.maximum(wb, 0)), Gm_old)
    stotal = np.where(wet, np.abs(Gn) + sPr + swb, LD(0))
    used = total if Gm_got is None else ss._ld(Gm_got)
    es = np.where(wet, e + x.dt * (x.C1 * used - x.C2 * Gm_old), e)
    u_ = x.u_
    near_e = (np.abs(e - P["emin"]) <= NEAR * u_ * (np.abs(e) + P["emin"])) | (e == 0)
    near_face = wet & (F["near"][:, :, :-1] | F["near"][:, :, 1:])
    near_cell = near_face | (wet & (nearD | near_e))
    enew = solve_columns(x, es, F["ke"], L if Le_got is None else np.where(near_cell, ss._ld(Le_got), L))
    se = np.where(wet, np.abs(np.where(wet, es, LD(0))).max(axis=2, keepdims=True), LD(0)) * np.ones(e.shape, LD)
    col = lambda m: m.any(axis=2, keepdims=True) & np.ones(e.shape, bool)
    return dict(Gm=total, s_Gm=stotal, near_Gm=np.zeros(e.shape, bool), Le=L, s_Le=sL, near_Le=near_cell, ke=F["ke"], es=es,
                e=enew, s_e=se, near_e=col(near_face) | (near_cell & (Le_got is None)), wet=wet, F=F)


def top_buoyancy_flux(x):
    """(J^b*, its scale) = g (alpha J^T - beta J^S) / rho0 of the top flux boundary conditions, alpha and beta at the surface cell"""
    H, Nz = x.H, x.Nz
    T, S = x.cells("T")[:, :, -1], x.cells("S")[:, :, -1]
    a, b, aT, aS = teos10_sensitivities(T, S, x.zc[Nz - 1])
    z = np.zeros((x.Nx, x.Ny), LD)
    JT = z if x.top_flux.get("T") is None else ss._ld(x.top_flux["T"])
    JS = z if x.top_flux.get("S") is None else ss._ld(x.top_flux["S"])
    land = x.kb >= Nz
    return (np.where(land, LD(0), x.grav * (a * JT - b * JS) / x.rho0),
            np.where(land, LD(0), x.grav * (aT * np.abs(JT) + aS * np.abs(JS)) / x.rho0))


def filtered_flux(x, e_new, Jb_old, dt_since):
    """(J^b, scale, near) after compute_average_surface_buoyancy_flux!: the dissipation length of the top cell from the NEW e
    and the OLD J^b; 0 on land"""
    P, Nz = x.P, x.Nz
    J = ss._ld(Jb_old)
    F = face_state(x, e=e_new, Jb=J)
    lD, slD, nearD = centre_length(x, F, ss._ld(e_new))
    lD, slD = lD[:, :, -1], slD[:, :, -1]
    Jstar, sJstar = top_buoyancy_flux(x)
    Jp = np.maximum(np.maximum(LD(P["Jbmin"]), J), Jstar)
    with np.errstate(divide="ignore", invalid="ignore"):
        eps = LD(float(x.dtype.type(dt_since))) / np.cbrt(lD * lD / Jp)
        new = (J + eps * Jstar) / (1 + eps)
        # eps carries two thirds of l_D's relative error and a third of J+'s (J* at worst): a factor on the term it multiplies
        amp = 1 + (slD / lD - 1) + np.where(Jp == Jstar, sJstar / np.maximum(np.abs(Jstar), LD(1e-300)) - 1, LD(0))
        s = (np.abs(J) + eps * sJstar * amp) / (1 + eps) + np.abs(new) * eps / (1 + eps) * (amp - 1)
    land = x.kb >= Nz
    near = (F["near"][:, :, Nz - 1] | nearD[:, :, -1]) & ~land
    return np.where(land, LD(0), new), np.where(land, LD(0), s), near


def surface_source(x):
    """(the surface TKE source in G^n.e of the top cell, its scale): (CWu u*^3 + CWw max(J^b*, 0) dz) / dz, u* from the flux
    values at (i, j); 0 on land"""
    P, Nz = x.P, x.Nz
    z = np.zeros((x.Nx, x.Ny), LD)
    Ju = z if x.top_flux.get("u") is None else ss._ld(x.top_flux["u"])[:, :x.Ny]
    Jv = z if x.top_flux.get("v") is None else ss._ld(x.top_flux["v"])[:, :x.Ny]
    us2 = np.sqrt(Ju * Ju + Jv * Jv)
    us3 = us2 * np.sqrt(us2)
    Jstar, sJstar = top_buoyancy_flux(x)
    dz = x.dzc[Nz - 1]
    land = x.kb >= Nz
    src = (P["CWu"] * us3 + P["CWw"] * np.maximum(Jstar, 0) * dz) / dz
    s = (P["CWu"] * us3 + P["CWw"] * np.where(Jstar > 0, sJstar, LD(0)) * dz) / dz
    return np.where(land, LD(0), src), np.where(land, LD(0), s)


# ---- the measure and the judge --------------------------------------------------------------------------------------------
def measure(got, want, scale, u_, where, near):
    """(largest r over the cells `where` that are not `near`, its index, the fraction left out); a cell whose scale is zero must
    agree exactly (r = inf otherwise)"""
    d = np.abs(ss._ld(got) - want)
    assert np.isfinite(ss._ld(got)).all() and np.isfinite(want[where]).all(), "a value is not finite"
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(scale > 0, d / (u_ * np.where(scale > 0, scale, 1)), np.where(d == 0, 0.0, np.inf)).astype(np.float64)
    r = np.where(where & ~near, r, 0.0)
    at = np.unravel_index(int(np.argmax(r)), r.shape)
    n = int(where.sum())
    return float(r[at]), tuple(int(q) for q in at), (float((where & near).sum()) / n if n else 0.0)


def judge_update(label, x, got, fields=("Gm.e", "Le", "e", "kappa_u", "kappa_c", "kappa_e"), bounds=C, strict=True):
    """The interior of what ONE compute_diffusivities! with dt_since = 0 left (`got`: parent arrays by name, read after the call)
    against the spec of the inputs `x` (read before it; u, v, T, S as the call saw them: masked, halos filled).
    Returns {field: (worst r, its cell, fraction left out)}; asserts r <= bounds[field] when `strict`."""
    H, Nx, Ny, Nz = x.H, x.Nx, x.Ny, x.Nz
    inner = lambda a, faces=False: a[H:H + Nx, H:H + Ny, H:H + Nz + (1 if faces else 0)]
    out = {}
    want = tke_step(x, Gm_got=inner(got["Gm.e"]), Le_got=inner(got["Le"]))
    wet = want["wet"]
    every = np.ones(wet.shape, bool)
    if "Gm.e" in fields:
        out["Gm.e"] = measure(inner(got["Gm.e"]), want["Gm"], want["s_Gm"], x.u_, every, want["near_Gm"])
    if "Le" in fields:
        out["Le"] = measure(inner(got["Le"]), want["Le"], want["s_Le"], x.u_, every, want["near_Le"])
    if "e" in fields:
        out["e"] = measure(inner(got["e"]), want["e"], want["s_e"], x.u_, every, want["near_e"])
    if any(n.startswith("kappa") for n in fields):
        F = face_state(x, e=inner(got["e"]), Jb=got["Jb"][H:H + Nx, H:H + Ny, 0])
        for n, key in (("kappa_u", "ku"), ("kappa_c", "kc"), ("kappa_e", "ke")):
            if n in fields:
                out[n] = measure(inner(got[n], True), F[key], F["s_" + key], x.u_, np.ones(F[key].shape, bool), F["near"])
    for n, (r, at, left) in out.items():
        assert left <= MAX_LEFT_OUT, f"{label}: {left:.2%} of the cells of {n} sit near a switch and were left out"
        if strict:
            assert r <= bounds[n], f"{label}: {n} is {r:.4g} u of its scale away from the spec at cell {at}; the bound is {bounds[n]:.4g}"
    return out


def judge_flux(label, x, e_new, Jb_old, Jb_got, dt_since, bound=C_JB, strict=True):
    """J^b after a compute with dt_since != 0 (x: the fields read AFTER the step; Jb_old: read before it)"""
    H, Nx, Ny = x.H, x.Nx, x.Ny
    sl = lambda a: a[H:H + Nx, H:H + Ny, 0]
    want, s, near = filtered_flux(x, e_new, sl(Jb_old), dt_since)
    r, at, left = measure(sl(Jb_got), want, s, x.u_, np.ones(want.shape, bool), near)
    assert left <= MAX_LEFT_OUT, f"{label}: {left:.2%} of the columns of Jb sit near a switch and were left out"
    if strict:
        assert r <= bound, f"{label}: Jb is {r:.4g} u of its scale away from the spec at column {at}; the bound is {bound:.4g}"
    return r, at, left


def exact_zeros(label, x, got):
    """The zeros the formulas state: bottom and top faces of the three kappa, faces touching the solid; L^e in dry cells, J^b on land"""
    H, Nx, Ny, Nz = x.H, x.Nx, x.Ny, x.Nz
    f_, k_ = np.arange(Nz + 1)[None, None, :], np.arange(Nz)[None, None, :]
    shut = ~((f_ >= 1) & (f_ <= Nz - 1) & (f_ > x.kb[:, :, None]))
    for n in ("kappa_u", "kappa_c", "kappa_e"):
        ss.check_zero(f"{label}: {n} on a bottom / top face or a face touching the solid", got[n][H:H + Nx, H:H + Ny, H:H + Nz + 1], shut)
    ss.check_zero(f"{label}: Le in a dry cell", got["Le"][H:H + Nx, H:H + Ny, H:H + Nz], k_ < x.kb[:, :, None])
    ss.check_zero(f"{label}: Jb on land", got["Jb"][H:H + Nx, H:H + Ny, 0], x.kb >= Nz)


# ---- what the call writes outside the interior ------------------------------------------------------------------------------
OUTSIDE_FIELDS = ("kappa_u", "kappa_c", "kappa_e", "Le", "Jb")


def outside_table(g, field, shape):
    """src [parent shape + (3,)]: the parent index of the INTERIOR cell a parent cell is a copy of after the call, -1 where the
    call does not write it (the module docstring's table); an interior cell the call writes maps to itself."""
    Nx, Ny, Nz, H = g["Nx"], g["Ny"], g["Nz"], g["H"]
    assert H <= Nx and H < Ny
    I, J, K = np.meshgrid(np.arange(shape[0]) - H, np.arange(shape[1]) - H, (np.arange(shape[2]) - H) if shape[2] > 1 else np.zeros(1, int), indexing="ij")
    si, sj, sk = np.mod(I, Nx), J.copy(), K.copy()
    rows_in = (J >= 0) & (J < Ny)
    layer = (J == -1) | ((J == Ny) & (not g["folded"]))
    sj = np.where(J == -1, 0, np.where(J == Ny, Ny - 1, sj))
    fold = np.zeros(I.shape, bool)
    if g["folded"]:
        fold = (J >= Ny) & (J < Ny + H)
        si = np.where(fold, Nx - 1 - np.mod(I, Nx), si)
        sj = np.where(fold, 2 * (Ny - 1) - J, sj)
    if field == "Jb":
        lev = np.ones(I.shape, bool)
    elif field == "Le":
        ends = (K == -1) | (K == Nz)
        lev = ((K >= 0) & (K < Nz)) | (ends & (rows_in | fold))
        sk = np.clip(K, 0, Nz - 1)
    else:
        lev = (K >= 0) & (K <= Nz)
    written = lev & (rows_in | layer | fold)
    src = np.stack([si + H, sj + H, (sk + H) if shape[2] > 1 else sk], axis=-1)
    return np.where(written[..., None], src, -1)


def check_outside(label, g, field, before, after, keep=True):
    """Images equal their interior source bit for bit; with `keep`, every cell the table does not name keeps the bits it had."""
    before, after = np.ascontiguousarray(before), np.ascontiguousarray(after)
    bits = np.dtype(f"u{after.dtype.itemsize}")
    src = outside_table(g, field, after.shape)
    written = src[..., 0] >= 0
    image = after[np.where(written, src[..., 0], 0), np.where(written, src[..., 1], 0), np.where(written, src[..., 2], 0)]
    bad = np.argwhere(written & (after.view(bits) != image.view(bits)))
    assert bad.size == 0, (f"{label}: {field} at parent cell {tuple(int(q) for q in bad[0])} is not the image of "
                           f"{tuple(int(q) for q in src[tuple(bad[0])])} (and {len(bad) - 1} more)")
    if keep:
        bad = np.argwhere(~written & (after.view(bits) != before.view(bits)))
        assert bad.size == 0, f"{label}: {field} changed at parent cell {tuple(int(q) for q in bad[0])} (and {len(bad) - 1} more), which the call does not write"


# ---- the flat-bottom interface tests/test_oracle_catke.py was written against ------------------------------------------------
class State(Inputs):
    """The inputs of the next compute_diffusivities! of the oracle model `m` (flat bottom), read now."""

    def __init__(self, m):
        b = m.backend
        Nx, Ny, Nz = m.grid.size
        g = dict(Nx=Nx, Ny=Ny, Nz=Nz, H=b.H, folded=False, kbot=np.zeros((Nx, Ny), int))
        super().__init__(b, g, 0.0)
        self.backend = b
        for short, name in (("u", "u"), ("v", "v"), ("T", "T"), ("S", "S"), ("e", "e"), ("ku", "kappa_u"), ("kc", "kappa_c"),
                            ("um", "previous_u"), ("vm", "previous_v"), ("Gn", "Gn.e"), ("Gm", "Gm.e")):
            setattr(self, short, self.f[name])

    @property
    def Jb(self):
        return self.f["Jb"]

    @Jb.setter
    def Jb(self, a):
        self.f["Jb"] = np.asarray(a)


def sensitivities(st, T, S, Z):
    """(alpha, beta) / rho0, analytically"""
    a, b, _, _ = teos10_sensitivities(T, S, Z)
    return (a / RHO0).astype(np.float64), (b / RHO0).astype(np.float64)


def face_quantities(st, P=DEFAULTS, e=None, Jb=None):
    F = face_state(st, e=e, Jb=Jb)
    return {k: np.asarray(F[k], np.float64) for k in ("N2", "S2", "ku", "kc", "ke", "convD")}


def flat_tke_step(st, dt):
    x = st.but()
    x.dt = LD(dt)
    w = tke_step(x)
    return {k: np.asarray(w[k], np.float64) for k in ("e", "Gm", "Le", "ke")}


def filtered_surface_flux(st, e_new, Jstar, dt_since, P=DEFAULTS):
    """J^b after compute_average_surface_buoyancy_flux! with the instantaneous J^b* handed in"""
    F = face_state(st, e=e_new)
    lD = centre_length(st, F, ss._ld(e_new))[0][:, :, -1]
    J = st.column("Jb")
    Jp = np.maximum(np.maximum(LD(P["Jbmin"]), J), ss._ld(Jstar))
    eps = LD(dt_since) / np.cbrt(lD * lD / Jp)
    return np.asarray((J + eps * ss._ld(Jstar)) / (1 + eps), np.float64)
