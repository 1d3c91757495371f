"""The fp64 hydrostatic pressure kernels, cell by cell.

Every launch form of compute_p (option pressure_form: 1 = 16 x 4 tiles, 2 = one row per thread, 3 = four rows per thread,
0 = the library's own choice) against tests/pressure_spec.py, an independent fp64 statement of the same operation:

  pHY'      at every cell the kernel writes, within the spec's own error bound E_p (+ one rounding of the store in Float32);
            every other cell of the parent array still holds a planted sentinel;
  dpx, dpy  the two differences the momentum kernel consumes, through a model at rest, where G.u = -(dpx rdxc) and
            G.v = -(dpy rdy) exactly: |G + dp_ref / dx| <= 8 u |dp_ref / dx| + (E_p[i] + E_p[i-1]) / dx, u the unit round-off
            of the build (one rounding of the stored difference, a reciprocal of at most 2 ulps, one product: 6 u);
  the forms the same bits from each, pHY' and tendencies;
  WRITE_P   the instances that store only the differences (the steady-state schedule of gb25_loop) likewise.

The bounds are those of pressure_spec.pressure: derived from operation counts.  Every test prints the largest observed
error / bound.
"""
import functools

import numpy as np
import pytest

import gb25_amd as gb
import pressure_spec as ps

pytestmark = pytest.mark.gpu

FORMS = (1, 2, 3, 0)
KINDS = ("random", "smooth")
SENTINEL = -12345.6789
# smallest shapes that leave a ragged tile in every form: 150 + 2 x 8 - 2 + 1 = 165 columns with the helper = 2 x 63 + 39
# = 11 x 15, 51 rows (no multiple of 3, 4 or 16); a narrow halo; more than 400 columns (the rule leaves the tile form)
LATLON_SHAPES = [((150, 37, 6), 8), ((70, 21, 5), 4), ((450, 13, 4), 8)]
CASES = [(g, s, h) for g in ("simple_lat_lon", "lat_lon_as_curvilinear", "gaussian_islands_lat_lon") for s, h in LATLON_SHAPES]
CASES.append(("gaussian_islands", (144, 64, 6), 8))
CASE_IDS = ["%s-%dx%dx%d-h%d" % ((g,) + s + (h,)) for g, s, h in CASES]
BUILDS = ["Float32", "Float64"]
FOLDED = ("gaussian_islands", "tripolar")
CURVILINEAR = ("lat_lon_as_curvilinear",) + FOLDED


def unit_roundoff(b):
    return ps.U32 if b.dtype == np.float32 else ps.U64


def make_model(float_type, grid, shape, halo, dt=600.0, **options):
    return gb.baroclinic_instability_model(gb.GPU(float_type=float_type), *shape, dt=dt, halo=halo, grid_type=grid,
                                           options=options or None)


def reference(b, shape, halo):
    """(p_ref, E_p) [parent i, parent j, k] from the T and S the device holds (halo cells as the fills left them, immersed
    cells masked), the vertical grid from the model's own faces, g and rho0 as numbers of the model's float type."""
    Nz = shape[2]
    zf = np.array([b.metric("zf", k) for k in range(1, Nz + 3)])       # faces ARE numbers of the model's float type
    zc, dzf = ps.vertical_metrics(zf)
    g, rho0 = float(b.dtype(b.cfg.g)), float(b.dtype(b.cfg.rho0))
    T, S = b.get_field("T", True).astype(np.float64), b.get_field("S", True).astype(np.float64)
    p, E = ps.pressure(T, S, zc, dzf, halo, g, rho0)
    # the reference is honest: within E_p / 4 of the same expression in extended precision, on this very state
    pl, El = ps.pressure(T, S, zc, dzf, halo, g, rho0, longdouble=True)
    assert float((np.abs(p - pl) / El)[1:-1, 1:-1].max()) <= 0.25
    return p, E


def face_metrics(b, grid, shape, halo):
    """(dx [i, j] of G.u's faces, dy [i, j] of G.v's faces) over the interior, the numbers the momentum kernel divides by."""
    Nx, Ny, _ = shape
    nyv = b.field_dims("Gn.v", False)[1]
    if grid in CURVILINEAR:
        dx = b.metric2("dxfc")[halo:halo + Nx, halo:halo + Ny]
        dy = b.metric2("dycf")[halo:halo + Nx, halo:halo + nyv]
    else:
        dx = np.broadcast_to(np.array([b.metric("dxc", j + 1) for j in range(Ny)])[None, :], (Nx, Ny))
        dy = np.full((Nx, nyv), b.metric("dy"))
    return dx, dy


def wet_faces(b, grid, shape):
    """(u faces, v faces) [i, j, k] over the interior that lie between two wet cells (everything on a flat bottom)."""
    Nx, Ny, Nz = shape
    nyv = b.field_dims("Gn.v", False)[1]
    if "islands" not in grid:
        return np.ones((Nx, Ny, Nz), bool), np.ones((Nx, nyv, Nz), bool)
    kbot = np.array([[b.bottom_info("kbot", i + 1, j + 1) for j in range(Ny)] for i in range(Nx)])
    wet = np.arange(Nz)[None, None, :] >= kbot[:, :, None]
    wu = wet & np.roll(wet, 1, axis=0)                                  # periodic in x
    wv = np.zeros((Nx, nyv, Nz), bool)
    wv[:, 1:Ny] = wet[:, 1:] & wet[:, :-1]
    return wu, wv


def compared_rows(grid, Ny):
    """Rows of G.u and of G.v that are compared: the v faces on the southern wall and on the northern wall (or fold) are
    never used; on the folded grid both stop one row below the pivot row (the last row of cells, held twice)."""
    top = Ny - 1 if grid in FOLDED else Ny
    return slice(0, top), slice(1, top)


def set_state(m, shape, kind):
    T, S = ps.rest_state(shape, kind, m.backend.dtype)
    m.set(T=T.astype(m.backend.dtype), S=S.astype(m.backend.dtype))


def read(b):
    return dict(pHY=b.get_field("pHY", True), Gu=b.get_field("Gn.u", False), Gv=b.get_field("Gn.v", False),
                w=b.get_field("w", False), GT=b.get_field("Gn.T", False), u=b.get_field("u", False), v=b.get_field("v", False))


@functools.lru_cache(maxsize=None)
def at_rest(float_type, grid, shape, halo):
    """update_state of both states at rest with every launch form, on one model; the sentinel is planted before each."""
    m = make_model(float_type, grid, shape, halo)
    b = m.backend
    out = {"dx_dy": face_metrics(b, grid, shape, halo), "wet": wet_faces(b, grid, shape), "u": unit_roundoff(b)}
    sentinel = np.full(b.field_dims("pHY", True), SENTINEL, b.dtype)
    for kind in KINDS:
        set_state(m, shape, kind)
        for form in FORMS:
            b.set_option("pressure_form", form)
            assert b.get_option("pressure_form") == form and b.get_option("pressure_precision") == 64
            b.set_field("pHY", sentinel, True)
            gb.update_state(m)
            out[kind, form] = read(b)
        out[kind, "ref"] = reference(b, shape, halo)
    b.close()
    return out


def check_phy(got, ref, halo, Nz, u, label):
    """|pHY' - p_ref| <= E_p (+ u32 |p_ref| for the one rounded store of a Float32 build) wherever the kernel writes, the
    sentinel bit for bit everywhere else.  Returns the largest error / bound."""
    p, E = ref
    H = halo
    written = np.zeros(got.shape, bool)
    written[1:-1, 1:-1, H:H + Nz] = True                     # columns, rows -H+1 .. N+H-2, levels 0 .. Nz-1
    assert np.array_equal(got[~written], np.full((~written).sum(), SENTINEL, got.dtype)), f"{label}: wrote outside its range"
    g = got[1:-1, 1:-1, H:H + Nz].astype(np.float64)
    pr, Er = p[1:-1, 1:-1], E[1:-1, 1:-1]
    bound = Er + (ps.U32 * np.abs(pr) if got.dtype == np.float32 else 0.0)
    ratio = np.abs(g - pr) / bound
    assert np.isfinite(g).all() and not (g == np.float64(got.dtype.type(SENTINEL))).any(), f"{label}: a cell was not written"
    worst = np.unravel_index(np.argmax(ratio), ratio.shape)
    assert ratio.max() <= 1.0, f"{label}: pHY' off by {ratio.max():.3g} x the bound at written cell {worst}"
    return float(ratio.max())


def check_differences(r, ref, cal, grid, shape, halo, label):
    """G.u and G.v of a model at rest against -(p_ref(i) - p_ref(i-1)) / dx, -(p_ref(j) - p_ref(j-1)) / dy."""
    Nx, Ny, Nz = shape
    H, u = halo, cal["u"]
    p, E = ref
    dx, dy = cal["dx_dy"]
    wu, wv = cal["wet"]
    ru, rv = compared_rows(grid, Ny)
    worst = {}
    for name, G, d, wetf, rows, sh in (("G.u", r["Gu"], dx, wu, ru, (1, 0)), ("G.v", r["Gv"], dy, wv, rv, (0, 1))):
        ny = G.shape[1]
        here = (slice(H, H + Nx), slice(H, H + ny))
        there = (slice(H - sh[0], H + Nx - sh[0]), slice(H - sh[1], H + ny - sh[1]))
        Gref = -(p[here] - p[there]) / d[:, :, None]
        bound = 8 * u * np.abs(Gref) + (E[here] + E[there]) / d[:, :, None]
        G = G.astype(np.float64)[:, rows]
        Gref, bound, wetf = Gref[:, rows], bound[:, rows], wetf[:, rows]
        assert np.isfinite(G).all(), f"{label}: {name} not finite"
        assert (G[~wetf] == 0.0).all(), f"{label}: {name} not zero on a face that touches a solid cell"
        assert wetf.any() and np.abs(Gref[wetf]).max() > 0.0
        ratio = np.where(wetf, np.abs(G - Gref) / bound, 0.0)
        at = np.unravel_index(np.argmax(ratio), ratio.shape)
        assert ratio.max() <= 1.0, f"{label}: {name} off by {ratio.max():.3g} x the bound at {at} of the compared rows"
        worst[name] = float(ratio.max())
    return worst


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("float_type", BUILDS)
def test_phy_at_every_written_cell(float_type, case, form):
    grid, shape, halo = case
    res = at_rest(float_type, *case)
    for kind in KINDS:
        label = f"{float_type} {grid} {shape} form {form} {kind}"
        worst = check_phy(res[kind, form]["pHY"], res[kind, "ref"], halo, shape[2], res["u"], label)
        print(f"[pressure] pHY {label}: max error / bound = {worst:.4f}")


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("float_type", BUILDS)
def test_the_forms_give_the_same_bits(float_type, case):
    res = at_rest(float_type, *case)
    for kind in KINDS:
        for form in FORMS[1:]:
            for name in ("pHY", "Gu", "Gv"):
                assert np.array_equal(res[kind, form][name], res[kind, FORMS[0]][name]), (kind, name, "form", form, "against form", FORMS[0])


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("float_type", BUILDS)
def test_differences_through_the_state_of_rest(float_type, case, form):
    grid, shape, halo = case
    res = at_rest(float_type, *case)
    for kind in KINDS:
        r = res[kind, form]
        label = f"{float_type} {grid} {shape} form {form} {kind}"
        for name in ("w", "GT", "u", "v"):      # a pure pressure force: no flow, no tracer tendency
            assert not r[name].any(), f"{label}: {name} is not exactly zero"
        worst = check_differences(r, res[kind, "ref"], res, grid, shape, halo, label)
        print(f"[pressure] differences {label}: max error / bound = G.u {worst['G.u']:.4f}, G.v {worst['G.v']:.4f}")


@pytest.mark.parametrize("float_type", BUILDS)
def test_differences_with_the_direct_stencil_kernels(float_type):
    """options = dict(kernels = 1): k_gu / k_gv read the same two arrays."""
    grid, (shape, halo) = "simple_lat_lon", LATLON_SHAPES[0]
    m = make_model(float_type, grid, shape, halo, kernels=1)
    b = m.backend
    cal = {"dx_dy": face_metrics(b, grid, shape, halo), "wet": wet_faces(b, grid, shape), "u": unit_roundoff(b)}
    for kind in KINDS:
        set_state(m, shape, kind)
        gb.update_state(m)
        r = read(b)
        for name in ("w", "GT"):
            assert not r[name].any(), name
        label = f"{float_type} kernels=1 {kind}"
        worst = check_differences(r, reference(b, shape, halo), cal, grid, shape, halo, label)
        print(f"[pressure] differences {label}: max error / bound = G.u {worst['G.u']:.4f}, G.v {worst['G.v']:.4f}")
        # and the two kernel generations agree on a pure pressure force bit for bit
        ref = at_rest(float_type, grid, shape, halo)[kind, 0]
        ru, rv = compared_rows(grid, shape[1])
        assert np.array_equal(r["Gu"][:, ru], ref["Gu"][:, ru]) and np.array_equal(r["Gv"][:, rv], ref["Gv"][:, rv])
    b.close()


STEADY = [CASES[0], CASES[3], CASES[6], CASES[9]]      # every grid, at its first shape


@pytest.mark.parametrize("case", STEADY, ids=[CASE_IDS[q] for q in (0, 3, 6, 9)])
@pytest.mark.parametrize("float_type", BUILDS)
def test_steady_state_schedule_stores_only_the_differences(float_type, case):
    """first_time_step + loop(3) at the reference protocol's dt = 1e-9: the last pressure of the call comes from a
    WRITE_P = false instance.  The velocities are then ~1e-13 m/s and what they add to G.u, G.v (Coriolis: 1e-17) is far
    below the bound, so the bounds are those of the state of rest, from the T and S the model holds afterwards."""
    grid, shape, halo = case
    runs = {}
    for form in FORMS:
        for store in (0, 1):
            m = make_model(float_type, grid, shape, halo, dt=1e-9, pressure_form=form, store_pressure=store)
            b = m.backend
            set_state(m, shape, "random")
            gb.first_time_step(m)
            gb.loop(m, 3)
            assert b.get_option("store_pressure") == store
            r = read(b)                                       # (pHY' of store = 0 is stale: recomputed on demand)
            assert b.get_option("store_pressure") == store
            r["T"], r["S"] = b.get_field("T", True), b.get_field("S", True)
            runs[form, store] = r
            label = f"{float_type} {grid} {shape} form {form} store_pressure {store} after 4 steps"
            if store == 0:
                cal = {"dx_dy": face_metrics(b, grid, shape, halo), "wet": wet_faces(b, grid, shape), "u": unit_roundoff(b)}
                ref = reference(b, shape, halo)
                assert np.abs(r["u"]).max() < 1e-10 and np.abs(r["v"]).max() < 1e-10
                worst = check_differences(r, ref, cal, grid, shape, halo, label)
                p, E = ref
                g = r["pHY"][1:-1, 1:-1, halo:halo + shape[2]].astype(np.float64)
                bound = E[1:-1, 1:-1] + (ps.U32 * np.abs(p[1:-1, 1:-1]) if b.dtype == np.float32 else 0.0)
                ratio = float((np.abs(g - p[1:-1, 1:-1]) / bound).max())
                assert ratio <= 1.0, f"{label}: pHY' on demand off by {ratio:.3g} x the bound"
                print(f"[pressure] {label}: max error / bound = pHY {ratio:.4f}, G.u {worst['G.u']:.4f}, G.v {worst['G.v']:.4f}")
            b.close()
    for form in FORMS:
        for name, a in runs[form, 0].items():
            assert np.array_equal(a, runs[form, 1][name]), (name, "form", form, "store_pressure 0 against 1")
            assert np.array_equal(a, runs[FORMS[0], 0][name]), (name, "form", form, "against form", FORMS[0])


def test_pressure_precision_32_differences_come_from_the_stored_pressure():
    """pressure_precision = 32 (Float32, lat-lon): k_pressure_differences takes p(i) - p(i-1) and p(j) - p(j-1) from the
    stored pHY' in fp32, so G.u, G.v at rest are -((p(i) - p(i-1)) rdxc) formed in numpy float32 from pHY' as read back,
    within 8 x 2^-24 |value| (the product's rounding and the reciprocal of the metric, rounded twice here)."""
    grid, (shape, halo) = "simple_lat_lon", LATLON_SHAPES[0]
    Nx, Ny, Nz = shape
    H = halo
    m = make_model("Float32", grid, shape, halo, pressure_precision=32, pressure_form=3)
    b = m.backend
    assert b.get_option("pressure_precision") == 32
    dx, dy = face_metrics(b, grid, shape, halo)
    ru, rv = compared_rows(grid, Ny)
    for kind in KINDS:
        set_state(m, shape, kind)
        gb.update_state(m)
        r = read(b)
        p = r["pHY"][:, :, H:H + Nz]
        assert p.dtype == np.float32
        for name, G, d, rows, sh in (("G.u", r["Gu"], dx, ru, (1, 0)), ("G.v", r["Gv"], dy, rv, (0, 1))):
            ny = G.shape[1]
            dp = p[H:H + Nx, H:H + ny] - p[H - sh[0]:H + Nx - sh[0], H - sh[1]:H + ny - sh[1]]          # fp32, as the kernel
            want = -(dp * (np.float32(1.0) / d.astype(np.float32))[:, :, None])
            assert want.dtype == np.float32
            err = np.abs(G.astype(np.float64) - want.astype(np.float64))[:, rows]
            bound = 8 * ps.U32 * np.abs(want.astype(np.float64))[:, rows]
            assert np.abs(want[:, rows]).max() > 0 and (err <= bound).all(), (kind, name, float((err / np.maximum(bound, 1e-300)).max()))
            print(f"[pressure] pressure_precision=32 {kind} {name}: max error / (2^-24 |value|) = {float((err[bound > 0] / bound[bound > 0]).max() * 8):.3f}")
    b.close()
