"""Transports on the device (gb25_get_transport) against the numpy restatement of their terms (gb-25_amd/transports.py, pinned on
the CPU by tests/test_transports_host.py), and the proof that asking for them changes nothing a model computes.

Sums: an "across_y" line adds n fp64 terms in a fixed but not sequential order; any order of n terms is within (n - 1)
eps(Float64) sum|term| of the exact sum (Higham, Accuracy and Stability of Numerical Algorithms, eq. 4.4 to first order),
math.fsum gives the exact sum of the terms correctly rounded, and forming a term costs at most four roundings (a: two, q, q T):
the bound asserted is (n + 4) eps sum|term|, the integrals'.  An "across_x" line is DEFINED as the sequential sum south to north
and is compared bit for bit; PROFILE and STREAMFUNCTION are defined as left-to-right sums of the lines and are compared bit for
bit."""
import math

import numpy as np
import pytest

import gb25_amd as gb
from gb25_amd.binding import FIELD_IDS, KERNEL_IDS, Transport
from gb25_amd.distributed import LocalSlabEnsemble
from gb25_amd.transports import continuity_closure, face_area, fold_transports, transport_terms
from helpers import BASE_FIELDS, CASES, CATKE_FIELDS, EPS, GRID_NAMES, counter_rng, size_of, stepped_model

pytestmark = pytest.mark.gpu
FACES = ("across_y", "across_x")
SHAPES = ("lines", "profile", "streamfunction")
SUMS = ("area", "volume", "heat", "salt")


def check_lines(lines, terms, faces, what):
    """LINES against the terms: "across_y" within the fsum bound, "across_x" the sequential sum bit for bit; counts exact."""
    axis = 0 if faces == "across_y" else 1
    assert lines.shape == tuple(np.delete(terms["area"].shape, axis)), what
    assert np.array_equal(lines["faces"], terms["counted"].sum(axis=axis)), what
    assert np.array_equal(lines["nonfinite"], terms["skipped"].sum(axis=axis)), what
    worst = 0.0
    for f in SUMS:
        t = terms[f]
        if faces == "across_x":
            acc = np.zeros(lines.shape)
            for j in range(t.shape[1]):
                acc = acc + t[:, j]
            assert acc.tobytes() == np.ascontiguousarray(lines[f]).tobytes(), (what, f)
            continue
        for j in range(t.shape[1]):
            for k in range(t.shape[2]):
                x = t[:, j, k][terms["counted"][:, j, k]]
                exact, bound = math.fsum(x), (len(x) + 4) * EPS * math.fsum(np.abs(x))
                assert abs(float(lines[f][j, k]) - exact) <= bound, (what, f, j, k, float(lines[f][j, k]), exact, bound)
                if bound > 0:
                    worst = max(worst, abs(float(lines[f][j, k]) - exact) / bound)
    print(f"  {what} {faces}: {lines.shape[0]} lines, wet faces {int(lines['faces'].sum())}, skipped {int(lines['nonfinite'].sum())}, "
          f"worst |diff| / bound {worst:.3f}")


def check_backend(b, window=None, what=""):
    for faces in FACES:
        lines, profile, psi = (b.transport(faces, s, window) for s in SHAPES)
        check_lines(lines, transport_terms(b, faces, window), faces, what)
        assert lines["faces"].sum() > 0 and np.abs(lines["volume"]).max() > 0 and np.abs(lines["heat"]).max() > 0, what
        want = fold_transports(lines)
        assert psi.shape == (lines.shape[0], lines.shape[1] + 1) and psi.tobytes() == want.tobytes(), (what, faces)
        assert profile.tobytes() == np.ascontiguousarray(psi[:, -1]).tobytes(), (what, faces)
        assert (psi["volume"][:, 0] == 0).all() and (psi["faces"][:, 0] == 0).all()


@pytest.mark.parametrize("float_type,grid_type", CASES)
def test_lines_profiles_and_streamfunctions(float_type, grid_type):
    m = stepped_model(float_type, grid_type)
    b = m.backend
    check_backend(b, None, f"{float_type} grid {grid_type}")
    psi = gb.overturning(m)
    assert np.array_equal(psi, b.transport("across_y", "streamfunction")["volume"]) and psi.shape == (b.field_dims("v", False)[1], size_of(grid_type)[2] + 1)
    assert np.array_equal(gb.meridional_transport(m)["heat"], b.transport("across_y", "profile")["heat"])
    assert np.array_equal(gb.heat_transport(m, rho0_cp=2.0), 2.0 * gb.meridional_transport(m)["heat"])
    assert gb.section_transport(m, 5, (2, 9)) == b.transport("across_x", "profile", (2, 9))[5]
    b.close()


@pytest.mark.parametrize("float_type,grid_type,size", [("Float32", 1, None), ("Float64", 4, None), ("Float32", 1, (50, 24, 6))])
def test_windows(float_type, grid_type, size):
    m = stepped_model(float_type, grid_type, size=size)
    b = m.backend
    Nx, Ny, Nz = size or size_of(grid_type)
    by = b.field_dims("v", False)[1]
    for faces, windows in (("across_y", [(3, 41), (1, 1), (Nx - 3, -1)]), ("across_x", [(2, 9), (Ny - 1, 1), (5, -1)])):
        for w in windows:
            lines = b.transport(faces, "lines", w)
            check_lines(lines, transport_terms(b, faces, w), faces, f"{float_type} grid {grid_type} {Nx} columns window {w}")
            assert b.transport(faces, "streamfunction", w).tobytes() == fold_transports(lines).tobytes()
    if size:
        check_backend(b, None, f"{Nx} columns")
    # empty and out-of-range windows, wrong counts
    out = (Transport * (max(Nx, by) * (Nz + 1) + 1))()
    call = b.lib.gb25_get_transport
    for faces, n, along in ((0, by, Nx), (1, Nx, Ny)):
        assert call(b.h, faces, 0, 0, -1, out, n * Nz) == 0 and call(b.h, faces, 1, 0, -1, out, n) == 0
        assert call(b.h, faces, 2, 0, -1, out, n * (Nz + 1)) == 0
        for first, count in ((0, 0), (along, 1), (-1, 2), (along - 2, 3), (0, along + 1), (3, -2)):
            assert call(b.h, faces, 0, first, count, out, n * Nz) == 1, (faces, first, count)
            assert b"window" in b.lib.gb25_last_error_string(b.h)
        for shape, count in ((0, n), (0, n * Nz + 1), (1, n * Nz), (1, n - 1), (2, n * Nz), (2, 0)):
            assert call(b.h, faces, shape, 0, -1, out, count) == 1, (faces, shape, count)
            assert b"count" in b.lib.gb25_last_error_string(b.h)
    assert call(b.h, 2, 0, 0, -1, out, by * Nz) == 1 and call(b.h, 0, 3, 0, -1, out, by * Nz) == 1
    with pytest.raises(gb.GB25Error, match="window"):
        b.transport("across_y", "lines", (Nx, 1))
    b.close()


@pytest.mark.parametrize("float_type,grid_type", [("Float32", 1), ("Float64", 4)])
def test_a_nan_in_a_wet_cell(float_type, grid_type):
    m = stepped_model(float_type, grid_type, steps=0)
    b = m.backend
    Nx, Ny, Nz = size_of(grid_type)
    ay, ax = face_area(b, "across_y"), face_area(b, "across_x")
    # a wet interior cell away from the edges whose four faces are wet
    i, j, k = next((i, j, k) for k in range(Nz) for j in range(3, Ny - 3) for i in range(3, Nx - 3)
                   if ay[i, j, k] > 0 and ay[i, j + 1, k] > 0 and ax[i, j, k] > 0 and ax[i + 1, j, k] > 0)
    before = {(f, s): b.transport(f, s) for f in FACES for s in SHAPES}
    T = b.get_field("T", False).copy()
    T[i, j, k] = np.nan
    b.set_field("T", T, False)
    assert np.isnan(b.get_field("T", False)[i, j, k])
    after = {(f, s): b.transport(f, s) for f in FACES for s in SHAPES}
    ly, lx = after["across_y", "lines"], after["across_x", "lines"]
    # exactly the wet faces that touch the cell: its southern and northern y faces, its western and eastern x faces
    want_y = np.zeros(ly.shape, np.int64)
    want_y[j, k], want_y[j + 1, k] = 1, 1
    want_x = np.zeros(lx.shape, np.int64)
    want_x[i, k], want_x[i + 1, k] = 1, 1
    assert np.array_equal(ly["nonfinite"], want_y) and np.array_equal(lx["nonfinite"], want_x)
    for key, r in after.items():
        for f in SUMS:
            assert np.isfinite(r[f]).all(), (key, f)
    assert after["across_y", "profile"]["nonfinite"].sum() == 2 and after["across_x", "streamfunction"]["nonfinite"][i, -1] == 1
    # every other record keeps its bytes
    for f, want in (("across_y", want_y), ("across_x", want_x)):
        a, c = after[f, "lines"], before[f, "lines"]
        same = want == 0
        assert a[same].tobytes() == c[same].tobytes(), f
        hit = ~same
        assert np.array_equal(a["faces"][hit], c["faces"][hit] - 1), f
        untouched = want.sum(axis=1) == 0
        assert after[f, "profile"][untouched].tobytes() == before[f, "profile"][untouched].tobytes(), f
    check_backend(b, None, "with a NaN")
    b.close()


@pytest.mark.parametrize("float_type,grid_type", [(ft, gt) for ft in ("Float32", "Float64") for gt in (0, 4)])
def test_the_y_face_transports_close_the_continuity_equation(float_type, grid_type):
    """The residual of continuity_closure with the device's V and the downloaded w against the same quantity of the CPU oracle of
    the same float type stepped the same way: r_device <= 10 max(r_oracle, eps(real)).  Two correct implementations differ in
    operation order, so their round-off differs by a small factor; a wrong metric or mask shows orders of magnitude above
    (tools/transport_probe.py --closure records both values: profiles/transports_closure.json)."""
    from oracle_backend import CPU
    real = np.float32 if float_type == "Float32" else np.float64
    m = stepped_model(float_type, grid_type)
    o = stepped_model(float_type, grid_type, arch=CPU("f32" if float_type == "Float32" else "f64"))
    r_dev = continuity_closure(m.backend, m.backend.transport("across_y", "lines"))
    r_ora = continuity_closure(o.backend)
    eps = float(np.finfo(real).eps)
    print(f"  {float_type} grid {grid_type}: r_device {r_dev:.3e} r_oracle {r_ora:.3e} eps {eps:.3e}")
    assert np.abs(m.backend.get_field("w", False)).max() > 0
    assert r_dev <= 10 * max(r_ora, eps)
    m.backend.close()


LOOKAHEADS = dict(subcycle_lookahead=1, ab2_lookahead=1)


@pytest.mark.parametrize("float_type,grid_type,catke", [("Float32", 0, False), ("Float64", 0, False), ("Float32", 4, False),
                                                        ("Float64", 4, False), ("Float32", 0, True), ("Float32", 4, True)])
def test_transports_are_read_only(float_type, grid_type, catke):
    """Two identical models; one is asked for every shape and direction between every two steps.  Same bits, same look-ahead
    state, same launches of every phase of a step."""
    closure = gb.CATKEVerticalDiffusivity() if catke else None
    watched = stepped_model(float_type, grid_type, steps=0, closure=closure, **LOOKAHEADS)
    alone = stepped_model(float_type, grid_type, steps=0, closure=closure, **LOOKAHEADS)
    names = BASE_FIELDS + (CATKE_FIELDS if catke else [])
    for m in (watched, alone):
        m.backend.profile_enable(True)
        m.backend.profile_reset()
    for step in range(6):
        if step % 2 == 0:
            before = watched.backend.lookahead_state()
            for faces in FACES:
                for shape in SHAPES:
                    r = watched.backend.transport(faces, shape, None if step else (1, 7))
                    assert r["nonfinite"].sum() == 0 and r["faces"].sum() > 0
            assert watched.backend.lookahead_state() == before
        for m in (watched, alone):
            gb.time_step(m)
        assert watched.backend.lookahead_state() == alone.backend.lookahead_state(), step
    assert alone.backend.lookahead_state()[0], "the velocity look-ahead is on in this configuration"
    for k in KERNEL_IDS:
        if k != "diagnostics":
            assert watched.backend.profile_get(k)[0] == alone.backend.profile_get(k)[0], k
    assert watched.backend.profile_get("diagnostics")[0] > 0 and alone.backend.profile_get("diagnostics")[0] == 0
    for name in names:
        a, b = watched.backend.get_field(name, True), alone.backend.get_field(name, True)
        assert np.array_equal(a, b, equal_nan=True), name
    assert np.abs(watched.backend.get_field("u", False)).max() > 0
    for m in (watched, alone):
        m.backend.close()


@pytest.mark.parametrize("float_type,grid_type", [("Float32", 0), ("Float64", 4), ("Float32", 1)])
def test_repeatable_to_the_last_bit(float_type, grid_type):
    m1, m2 = stepped_model(float_type, grid_type), stepped_model(float_type, grid_type)
    for faces in FACES:
        for shape in SHAPES:
            for window in (None, (3, 11)):
                s = [m.backend.transport(faces, shape, window).tobytes() for m in (m1, m1, m2)]
                assert s[0] == s[1] == s[2], (faces, shape, window)
    m1.backend.close()
    m2.backend.close()


@pytest.mark.parametrize("float_type,grid_type", [("Float32", 0), ("Float64", 1), ("Float32", 4)])
def test_the_tables_follow_the_host_grid_setters(float_type, grid_type):
    m = stepped_model(float_type, grid_type, steps=1)
    b = m.backend
    Nx, Ny, Nz = size_of(grid_type)
    before = b.transport("across_y", "profile")
    zc = np.array([b.metric("zc", k) for k in range(1, Nz + 1)])
    zb = np.full((Nx, Ny), -1e30)
    zb[5:9, 4:7] = 0.5 * (zc[1] + zc[2])          # two immersed cells
    zb[20:22, 10] = 0.5 * (zc[3] + zc[4])         # four
    zb[30, 12:15] = 10.0                          # land
    b.set_bottom_height(zb)
    assert b.bottom_info("kbot", 6, 5) == 2 and b.bottom_info("kbot", 31, 13) == Nz
    check_backend(b, None, "after set_bottom_height")
    after = b.transport("across_y", "profile")
    assert after["faces"].sum() != before["faces"].sum() and after["area"][5] != before["area"][5]     # (the new bottom replaces the grid's own)
    if grid_type == 0:
        # other vertical faces: the spacings of the face areas follow
        zf = -4000.0 * (1.0 - np.linspace(0.0, 1.0, Nz + 1)) ** 1.5
        b.set_vertical_faces(zf)
        check_backend(b, None, "after set_vertical_faces")
        assert b.transport("across_y", "profile")["area"][5] != after["area"][5]
    b.close()


DECOMPOSITIONS = [(2, 1), (4, 1), (4, 2)]


@pytest.mark.parametrize("grid_type", [1, 4])
@pytest.mark.parametrize("P,Ry", DECOMPOSITIONS)
def test_combined_transports_of_the_ranks(P, Ry, grid_type):
    if Ry == 1:
        Nx, Ny, Nz, dt, kw = 96 * P // 2, 40, 10, 600.0, {}
    else:
        Nx, Ny, Nz, dt, kw = 128, 48 * Ry, 8, 600.0, dict(slab_mode=1)
    single = gb.baroclinic_instability_model(gb.GPU(), Nx, Ny, Nz, dt=dt, grid_type=GRID_NAMES[grid_type])
    gb.set_baroclinic_instability(single)
    vrows = Ny if grid_type == 4 else Ny + 1
    single.set(u=(1e-2 * counter_rng((Nx, Ny, Nz), 42, 1)).astype(np.float32),
               v=(1e-2 * counter_rng((Nx, vrows, Nz), 42, 2)).astype(np.float32),
               eta=(1e-2 * counter_rng((Nx, Ny, 1), 42, 3)).astype(np.float32))
    init = {n: single.backend.get_field(n, False) for n in ("u", "v", "T", "S", "eta")}
    ens = LocalSlabEnsemble(Nx, Ny, Nz, P, dt=dt, ranks_y=Ry, grid_type=grid_type, options=dict(w_on_the_fly=0), **kw)
    for n, a in init.items():
        ens.scatter(n, a)
    gb.first_time_step(single)
    ens.first_time_step()
    gb.loop(single, 4)
    ens.loop(4)
    sb = single.backend
    for name in ("u", "v", "T", "S"):
        assert np.array_equal(ens.gather(name), sb.get_field(name, False)), name     # (the premise)
    # windows of the global summed index that straddle a seam between two ranks (and, along j, between two bands)
    windows = {"across_y": [None, (Nx // (P // Ry) - 5, 11)], "across_x": [None, (Ny // Ry - 5, 11) if Ry > 1 else (7, 20)]}
    for faces in FACES:
        for window in windows[faces]:
            what = f"{P} ranks ({Ry} in y) grid {grid_type} window {window}"
            terms = transport_terms(sb, faces, window)
            lines, one = ens.transport(faces, "lines", window), sb.transport(faces, "lines", window)
            assert lines.shape == one.shape and np.array_equal(lines["faces"], one["faces"]), what
            assert lines["nonfinite"].sum() == 0 and lines["faces"].sum() > 0
            if faces == "across_x" and Ry == 1:
                assert lines.tobytes() == one.tobytes(), what          # x slabs: every column is summed on one rank
            else:
                # within the fsum bound of the line (for the x faces of a mesh: n terms in another association)
                axis = 0 if faces == "across_y" else 1
                for f in SUMS:
                    t = np.moveaxis(terms[f], axis, 0)
                    for n in range(lines.shape[0]):
                        for k in range(lines.shape[1]):
                            x = t[:, n, k]
                            x = x[np.moveaxis(terms["counted"], axis, 0)[:, n, k]]
                            exact, bound = math.fsum(x), (len(x) + 4) * EPS * math.fsum(np.abs(x))
                            assert abs(float(lines[f][n, k]) - exact) <= bound, (what, f, n, k, "combined")
                            assert abs(float(one[f][n, k]) - exact) <= bound, (what, f, n, k, "single")
            psi = ens.transport(faces, "streamfunction", window)
            assert psi.tobytes() == fold_transports(lines).tobytes(), what
            assert ens.transport(faces, "profile", window).tobytes() == np.ascontiguousarray(psi[:, -1]).tobytes(), what
    with pytest.raises(ValueError):
        ens.transport("across_y", "lines", (Nx, 1))
    ens.close()
    sb.close()
