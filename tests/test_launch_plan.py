"""The launches of a halo fill, of w and of the hydrostatic pressure (csrc/launch_plan.hpp) as a host-only harness: a small main includes
the header alone and prints the plan of every request below on every grid below; they are compared with expectations written out here --
the fill_halos_impl, fill_halos_2d, compute_w_impl and compute_p_impl this header replaced, restated line by line with their positional
parameters and bit masks, and a few numbers worked out by hand -- not read off the header.  No GPU, no library."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_MAX = 2**31 - 1

# ---- grids: what launch_facts reads from a model.  sy_c, sy_v: parent rows of a cell-shaped / y-face array, Ny + 2H and one more
BASE = dict(Nx=40, Ny=21, Nz=6, H=4, x_periodic=1, north_fold=0, pivot_slaved=0, slab=0, ys_open=0, yn_open=0, fill_fused=0, curvilinear=0)
FOLDED = dict(BASE, Ny=24, north_fold=1, curvilinear=1)
GRIDS = {
    "walled": BASE,                                                   # single domain 40 x 21 x 6, halo 4, option FILL_FUSED = 0
    "walled_fused": dict(BASE, fill_fused=1),                         # ... and 1, the default
    "folded": FOLDED,                                                 # single domain 40 x 24 x 6 below the zipper fold
    "folded_pivot_slaved": dict(FOLDED, pivot_slaved=1),              # ... with option FOLD_PIVOT_SLAVED
    "self_ring": dict(BASE, slab=1, x_periodic=0, fill_fused=1),      # the walled grid as a slab that is its own neighbour
    "north_open": dict(BASE, slab=1, x_periodic=0, yn_open=1, fill_fused=1),   # a mesh rank below a neighbour (test_model_layout.py)
    "south_open": dict(BASE, slab=1, x_periodic=0, ys_open=1, fill_fused=1),   # ... and above one
    "row_1440": dict(BASE, Nx=1440, Ny=720, Nz=48, H=8, fill_fused=1),         # the headline grid: the x copy counts in long
    "row_1440_two_launches": dict(BASE, Nx=1440, Ny=720, Nz=48, H=8),
}

# ---- requests: every distinct one a call site makes, with the arguments the same call site passed to the old functions:
# (with_x, extended, which, sel3) of fill_halos_impl, n_other = the fields of its h2_other; or fill_halos_2d with a Halo2 of n fields
PX, OWN, EXT = "Columns::OwnWithPeriodicX", "Columns::Own", "Columns::Extended"
REQUESTS = {
    # name: (the request in C++, n_given, the old call)
    "everything_periodic_x": ("FillRequest::everything_periodic_x()", 0, ("impl", True, False, 3, 3, None)),   # gb25_api.hip update_state_impl, time_step_impl, gb25_fill_halo_regions
    "e_periodic_x": ("FillRequest::e(%s)" % PX, 0, ("impl", True, False, 1, 4, None)),        # gb25_api.hip catke_diffusivities_impl, update_state_impl, time_step_impl
    "uv_periodic_x": ("FillRequest::uv(%s)" % PX, 0, ("impl", True, False, 1, 1, None)),      # gb25_api.hip tracers_impl; time_step_impl (`stale`: only u, v)
    "ts_periodic_x": ("FillRequest::ts(%s)" % PX, 0, ("impl", True, False, 1, 2, None)),      # gb25_api.hip time_step_impl
    "stale_eta_periodic_x": ("FillRequest{Fields3::None, Fields2::Prognostic, %s}" % PX, 0, ("impl", True, False, 2, 1, None)),   # gb25_api.hip time_step_impl (`stale`)
    "stale_uv_eta_periodic_x": ("FillRequest{Fields3::UV, Fields2::Prognostic, %s}" % PX, 0, ("impl", True, False, 3, 1, None)),  # gb25_api.hip time_step_impl (`stale`)
    "given_two": ("FillRequest::flat(Fields2::Given, %s)" % PX, 2, ("2d", 2)),                # gb25_api.hip fill_halos_2d: ab2_step_impl, time_step_impl (G.U, G.V; du, dv)
    "given_three": ("FillRequest::flat(Fields2::Given, %s)" % PX, 3, ("2d", 3)),              # gb25_api.hip fill_halos_2d: initialize_impl
    "e_own": ("FillRequest::e(%s)" % OWN, 0, ("impl", False, False, 1, 4, None)),             # slab_step.hpp catke_step_local
    "e_extended": ("FillRequest::e(%s)" % EXT, 0, ("impl", False, True, 1, 4, None)),         # slab_step.hpp catke_finish_local
    "uvts_own": ("FillRequest::uvts(%s)" % OWN, 0, ("impl", False, False, 1, 3, None)),       # slab_step.hpp stage_update
    "ahead_eta_extended": ("FillRequest::flat_extended(Fields2::Given)", 3, ("impl", False, True, 2, 3, 3)),   # slab_step.hpp stage_subcycle (ahead)
    "eta_extended": ("FillRequest::flat_extended()", 0, ("impl", False, True, 2, 3, None)),   # slab_step.hpp stage_subcycle
    "uv_own": ("FillRequest::uv(%s)" % OWN, 0, ("impl", False, False, 1, 1, None)),           # slab_step.hpp stage_own_columns
    "arrived_uv_eta": ("FillRequest{Fields3::UV, Fields2::Prognostic, %s}" % EXT, 0, ("impl", False, True, 3, 1, None)),   # slab_step.hpp stage_halo_columns (`arrived`, strips first)
    "everything_extended": ("FillRequest::everything(%s)" % EXT, 0, ("impl", False, True, 3, 3, None)),   # slab_step.hpp stage_halo_columns, update_state_local_impl, MaskFillLocal
    "everything_own": ("FillRequest::everything(%s)" % OWN, 0, ("impl", False, False, 3, 3, None)),       # slab_step.hpp update_state_local_impl, FillLocal
}
ONLY_2D = {"stale_eta_periodic_x", "given_two", "given_three", "ahead_eta_extended", "eta_extended"}
PERIODIC_X = {"everything_periodic_x", "e_periodic_x", "uv_periodic_x", "ts_periodic_x", "stale_eta_periodic_x", "stale_uv_eta_periodic_x",
              "given_two", "given_three"}

# what each kernel takes from the host besides the fields (kernels.hpp): only these are compared
TAKES = {"y": ("grid", "i0", "ni", "n2", "flat"), "yz": ("grid", "i0", "ni", "jlo", "n2", "flat"), "fold": ("grid", "n2", "flat"),
         "x": ("grid", "n2", "flat", "rows_c", "rows_v"), "fused": ("grid", "n2", "flat", "nbx", "nb_yz", "nbr", "rows_c", "rows_v")}


def old_fill_halos_2d(g, n):
    """fill_halos_2d(m, h2) of the old gb25_api.hip with a Halo2 of n fields"""
    Nx, H = g["Nx"], g["H"]
    out = [dict(kernel="y", grid=((Nx + 255) // 256, 1, 1), i0=0, ni=Nx, n2=n, flat=1)]
    if g["north_fold"] and not g["slab"]:
        out.append(dict(kernel="fold", grid=((Nx + 255) // 256, H + g["pivot_slaved"], 1), n2=n, flat=0))
    if g["x_periodic"]:
        threads = g["sy_v"] * 2 * H
        out.append(dict(kernel="x", grid=((threads + 255) // 256, 4 + n, 1), n2=n, flat=1, rows_c=0, rows_v=0))
    return out


def old_fill_halos_impl(g, with_x, extended, which, sel3, n_other):
    """fill_halos_impl(m, with_x, extended, which, sel3, nullptr, true, h2_other) of the old gb25_api.hip, its ladder in its order"""
    Nx, Ny, Nz, H = g["Nx"], g["Ny"], g["Nz"], g["H"]
    n2 = 3 if n_other is None else n_other
    i0, ni = (-H, Nx + 2 * H) if extended else (0, Nx)
    if which == 2 and with_x and g["x_periodic"] and not extended and n_other is None:
        return old_fill_halos_2d(g, 3)
    rows_c, rows_v = g["sy_c"] * (Nz + 2 * H), g["sy_v"] * (Nz + 2 * H)
    if g["north_fold"] and not g["slab"]:
        if which == 2:
            return old_fill_halos_2d(g, n2)
        if which == 1:
            n2 = 0
        return [dict(kernel="yz", grid=((Nx + 255) // 256, Nz + 1 + Ny, 1), i0=0, ni=Nx, jlo=0, n2=n2, flat=0),
                dict(kernel="fold", grid=((Nx + 255) // 256, H + g["pivot_slaved"], Nz + 2 + (1 if n2 else 0)), n2=n2, flat=0),
                dict(kernel="x", grid=((rows_v * 2 * H + 255) // 256, 4 + n2, 1), n2=n2, flat=0, rows_c=rows_c, rows_v=rows_v)]
    if which == 2:
        return [dict(kernel="y", grid=((ni + 255) // 256, 1, 1), i0=i0, ni=ni, n2=n2, flat=1)]
    if which == 1:
        n2 = 0
    if g["fill_fused"] and with_x and g["x_periodic"] and not extended:
        nbx = (Nx + 255) // 256
        nb_yz = nbx * (Nz + 1 + Ny)
        nbr = (rows_v * 2 * H + 255) // 256
        return [dict(kernel="fused", grid=(nb_yz + nbr * (4 + n2), 1, 1), n2=n2, flat=0, nbx=nbx, nb_yz=nb_yz, nbr=nbr, rows_c=rows_c, rows_v=rows_v)]
    jlo = -H if (extended and g["ys_open"]) else 0
    jhi = Ny + H if (extended and g["yn_open"]) else Ny
    out = [dict(kernel="yz", grid=((ni + 255) // 256, Nz + 1 + (jhi - jlo), 1), i0=i0, ni=ni, jlo=jlo, n2=n2, flat=0)]
    if with_x and g["x_periodic"]:
        out.append(dict(kernel="x", grid=((rows_v * 2 * H + 255) // 256, 4 + n2, 1), n2=n2, flat=0, rows_c=rows_c, rows_v=rows_v))
    return out


def old_fill(g, call):
    return old_fill_halos_2d(g, call[1]) if call[0] == "2d" else old_fill_halos_impl(g, *call[1:])


def table_form(g, name):
    """the table of launch forms in DESIGN.md, "The launches of a fill, of w and of the pressure", first row that applies"""
    folded_single = g["north_fold"] and not g["slab"]
    if name in ONLY_2D and (name in PERIODIC_X or folded_single):
        return "flat2d"
    if folded_single:
        return "folded_single"
    if name in ONLY_2D:
        return "flat_y"
    if name in PERIODIC_X and g["x_periodic"] and g["fill_fused"]:
        return "fused"
    return "layers"


def old_compute_w_impl(g, part):
    """compute_w_impl(m, part) of the old gb25_api.hip: the kernel's four column arguments, the rows, the block"""
    Nx, Ny, H = g["Nx"], g["Ny"], g["H"]
    ia, na, ib, nb = -H + 1, Nx + 2 * H - 2, 0, 0
    if part == 1:
        ia, na = 0, Nx - 1
    elif part == 2:
        ia, na, ib, nb = -H + 1, H - 1, Nx - 1, H
    return dict(ia=ia, na=na, ib=ib, nb=nb, rows=Ny + 2 * H - 2, block=(64, 4) if na + nb >= 64 else (16, 16))


def old_compute_p_impl(g, cols, forced):
    """compute_p_impl(m, i_first, i_last, i_first_b, i_last_b) of the old gb25_api.hip (None: its INT_MIN default), option PRESSURE_FORM
    = forced: the kernel's column and row arguments, the form, the grid, tiles_a"""
    Nx, Ny, H, PR = g["Nx"], g["Ny"], g["H"], 4
    i_first, i_last, i_first_b, i_last_b = (-H + 1, Nx + H - 2, 0, -1) if cols is None else cols
    ncol = i_last - i_first + 2
    ncol_b = i_last_b - i_first_b + 2 if i_last_b >= i_first_b else 0
    j_first, j_last = -H + 1, Ny + H - 2
    nrow = j_last - j_first + 1
    tiles_a, tiles_b = (ncol + 62) // 63, (ncol_b + 62) // 63
    narrow = (tiles_a + tiles_b) * ((nrow + PR * 4 - 1) // (PR * 4)) < 1024
    form = forced if forced else 1 if (narrow and not g["curvilinear"] and ncol + ncol_b <= 400) else 2 if narrow else 3
    if form == 1:
        ta = (i_last - i_first + 1 + 14) // 15
        tb = (i_last_b - i_first_b + 1 + 14) // 15 if ncol_b else 0
        grid, tiles = (ta + tb, (nrow + 11) // 12), ta
    elif form == 2:
        grid, tiles = (tiles_a + tiles_b, (nrow + 3) // 4), tiles_a
    else:
        grid, tiles = (tiles_a + tiles_b, (nrow + PR * 4 - 1) // (PR * 4)), tiles_a
    return dict(args=(i_first, i_last, i_first_b, i_last_b, j_first, j_last), form=form, grid=grid, tiles_a=tiles)


# pressure: the boxes the call sites name, as the old call sites passed them
BOXES = {
    "whole": ("PressureBox::whole(f)", lambda g: None),
    "own_columns": ("PressureBox::own_columns(f)", lambda g: (0, g["Nx"] - 1, 0, -1)),                           # slab_step.hpp stage_update
    "strips": ("PressureBox::strips(f)", lambda g: (-g["H"] + 1, 0, g["Nx"], g["Nx"] + g["H"] - 2)),             # slab_step.hpp stage_strips, stage_halo_columns
}
P_GRIDS = {"%s_%d" % (kind, nx): dict(BASE, Nx=nx, Ny=720, Nz=48, H=8, slab=1, x_periodic=0, curvilinear=int(kind == "curvilinear"))
           for kind in ("latlon", "curvilinear") for nx in (180, 360, 400, 401, 720)}
P_GRIDS["latlon_1440"] = GRIDS["row_1440"]
P_CASES = [(gname, box, 0) for gname in P_GRIDS for box in BOXES if gname != "latlon_1440" or box == "whole"] + \
          [(gname, "whole", forced) for gname in ("latlon_180", "curvilinear_720", "latlon_1440") for forced in (1, 2, 3)]
# w: a 180-column slab and one narrower than 64 columns (the walled grid's self-ring)
W_GRIDS = {"latlon_180": P_GRIDS["latlon_180"], "self_ring": GRIDS["self_ring"]}
PASSES = {"Whole": 0, "Interior": 1, "Edges": 2}

MAIN = r'''
#include <cstdio>
static const char* kernel_name(FillKernel k) {
  switch (k) {
    case FillKernel::Y: return "y";
    case FillKernel::YZ: return "yz";
    case FillKernel::Fold: return "fold";
    case FillKernel::X: return "x";
    case FillKernel::Fused: return "fused";
  }
  return "?";
}
static const char* form_name(FillForm f) {
  switch (f) {
    case FillForm::Flat2D: return "flat2d";
    case FillForm::FoldedSingle: return "folded_single";
    case FillForm::FlatY: return "flat_y";
    case FillForm::Fused: return "fused";
    case FillForm::Layers: return "layers";
  }
  return "?";
}
static void show_fill(const char* grid, const char* name, FillRequest rq, int n_given, const LaunchFacts& f) {
  rq.n_given = n_given;
  const FillPlan p = plan_fill(rq, f);
  std::printf("fill\t%s\t%s\tform=%s\tn=%d", grid, name, form_name(p.form), p.n);
  for (int q = 0; q < p.n; q++) {
    const FillLaunch& l = p.l[q];
    std::printf("\t%s,%u,%u,%u,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d", kernel_name(l.kernel), l.gx, l.gy, l.gz, l.i0, l.ni, l.jlo, l.n2, (int)l.flat,
                l.rows_c, l.rows_v, l.nbx, l.nb_yz, l.nbr);
  }
  std::printf("\n");
}
static void show_w(const char* grid, const char* name, Pass pass, const LaunchFacts& f) {
  const WColumns w = w_columns(pass, f);
  std::printf("w\t%s\t%s\tia=%d\tna=%d\tib=%d\tnb=%d\trows=%d\tbx=%d\tby=%d\tni=%d\n", grid, name, w.cols.i0, w.cols.na(), w.cols.b0(), w.cols.nb(),
              w.rows, w.bx, w.by, w.cols.ni);
}
static void show_p(const char* grid, const char* name, int forced, const PressureBox& box, const LaunchFacts& f) {
  const PressurePlan p = plan_pressure(box, f, forced);
  const Cols& c = box.cols;   // (the kernel's column arguments as compute_p_impl passes them)
  std::printf("p\t%s\t%s\t%d\targs=%d,%d,%d,%d,%d,%d\tform=%d\tgrid=%u,%u\ttiles_a=%d\n", grid, name, forced, c.i0, c.i0 + c.na() - 1, c.b0(),
              c.b0() + c.nb() - 1, box.j_first, box.j_last, p.form, p.gx, p.gy, p.tiles_a);
}
int main() {
'''


def facts(g):
    return "LaunchFacts{%d, %d, %d, %d, %d, %d, %s, %s, %d, %s, %s, %s, %s, %s}" % (
        g["Nx"], g["Ny"], g["Nz"], g["H"], g["Ny"] + 2 * g["H"], g["Ny"] + 2 * g["H"] + 1, *(
            ("true" if g[k] else "false") if k != "pivot_slaved" else g[k]
            for k in ("x_periodic", "north_fold", "pivot_slaved", "slab", "ys_open", "yn_open", "fill_fused", "curvilinear")))


def with_rows(g):
    return dict(g, sy_c=g["Ny"] + 2 * g["H"], sy_v=g["Ny"] + 2 * g["H"] + 1)


def source():
    """the program: the header alone, then one call per case"""
    body = []
    for gname, g in {**GRIDS, **P_GRIDS}.items():
        body.append("  {\n    const LaunchFacts f = %s;\n" % facts(g))
        if gname in GRIDS:
            for name, (cxx, n_given, _) in REQUESTS.items():
                body.append('    show_fill("%s", "%s", %s, %d, f);\n' % (gname, name, cxx, n_given))
        if gname in W_GRIDS:
            for name in PASSES:
                body.append('    show_w("%s", "%s", Pass::%s, f);\n' % (gname, name, name))
        for pg, box, forced in P_CASES:
            if pg == gname:
                body.append('    show_p("%s", "%s", %d, %s, f);\n' % (gname, box, forced, BOXES[box][0]))
        body.append("  }\n")
    return '#include "%s"\n' % os.path.join(ROOT, "gb-25_amd", "csrc", "launch_plan.hpp") + MAIN + "".join(body) + "  return 0;\n}\n"


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("launch_plan")
    src, exe = tmp / "plan.cpp", tmp / "plan"
    src.write_text(source())
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    got = dict(fill={}, w={}, p={})
    keys = ("i0", "ni", "jlo", "n2", "flat", "rows_c", "rows_v", "nbx", "nb_yz", "nbr")
    for line in out.splitlines():
        kind, gname, name, *rest = line.split("\t")
        if kind == "fill":
            launches = []
            for item in rest[2:]:
                k, gx, gy, gz, *v = item.split(",")
                launches.append(dict(zip(keys, (int(x) for x in v)), kernel=k, grid=(int(gx), int(gy), int(gz))))
            got["fill"][(gname, name)] = dict(form=rest[0].split("=")[1], n=int(rest[1].split("=")[1]), launches=launches)
        elif kind == "w":
            got["w"][(gname, name)] = {k: int(v) for k, v in (kv.split("=") for kv in rest)}
        else:
            got["p"][(gname, name, int(rest[0]))] = dict(kv.split("=") for kv in rest[1:])
    return got


@pytest.mark.parametrize("gname", list(GRIDS))
@pytest.mark.parametrize("name", list(REQUESTS))
def test_the_fill_of(printed, name, gname):
    g, got = with_rows(GRIDS[gname]), printed["fill"][(gname, name)]
    want = old_fill(g, REQUESTS[name][2])
    assert got["n"] == len(got["launches"]) == len(want) <= 3, (got, want)
    for a, b in zip(got["launches"], want):
        assert {k: a[k] for k in ("kernel",) + TAKES[a["kernel"]]} == b, (gname, name, got["launches"], want)
    assert got["form"] == table_form(g, name), (gname, name)


def test_a_few_fills_by_hand(printed):
    launches = lambda g, r: [(l["kernel"],) + l["grid"] for l in printed["fill"][(g, r)]["launches"]]
    # walled 40 x 21 x 6, halo 4: one block of 256 threads per row of columns; 6 + 1 planes of the y layer and 21 rows of the z layers;
    # the x copy: 30 rows x 14 levels = 420 rows of v, x 8 halo columns = 3360 threads = 14 blocks, 4 + 3 slices
    assert launches("walled", "everything_periodic_x") == [("yz", 1, 28, 1), ("x", 14, 7, 1)]
    assert launches("walled_fused", "everything_periodic_x") == [("fused", 28 + 14 * 7, 1, 1)]
    assert launches("walled_fused", "e_periodic_x") == [("fused", 28 + 14 * 4, 1, 1)]          # (no 2-D field: 4 slices all the same)
    assert launches("walled", "stale_eta_periodic_x") == [("y", 1, 1, 1), ("x", 1, 7, 1)]       # 30 rows x 8 = 240 threads: one block
    assert launches("walled", "given_two") == [("y", 1, 1, 1), ("x", 1, 6, 1)]
    # folded 40 x 24 x 6: 7 + 24 rows of blocks; the fold: 4 rows (5 with the pivot row) on 6 + 2 planes and one for the 2-D fields;
    # the x copy: 33 x 14 = 462 rows x 8 = 3696 threads = 15 blocks
    assert launches("folded", "everything_periodic_x") == [("yz", 1, 31, 1), ("fold", 1, 4, 9), ("x", 15, 7, 1)]
    assert launches("folded_pivot_slaved", "uv_periodic_x") == [("yz", 1, 31, 1), ("fold", 1, 5, 8), ("x", 15, 4, 1)]
    assert launches("folded", "everything_extended") == launches("folded", "everything_periodic_x")   # (whatever the columns)
    assert launches("folded", "given_two") == [("y", 1, 1, 1), ("fold", 1, 4, 1), ("x", 2, 6, 1)]      # 33 x 8 = 264 threads
    assert launches("folded", "ahead_eta_extended") == [("y", 1, 1, 1), ("fold", 1, 4, 1), ("x", 2, 7, 1)]
    # a slab: 48 columns with the x halos; the z layers of an extended fill reach the 4 halo rows of an open side only
    assert launches("self_ring", "everything_extended") == [("yz", 1, 28, 1)]
    assert launches("north_open", "everything_extended") == launches("south_open", "everything_extended") == [("yz", 1, 32, 1)]
    assert launches("north_open", "everything_own") == [("yz", 1, 28, 1)]
    jlo = lambda g: printed["fill"][(g, "everything_extended")]["launches"][0]["jlo"]
    assert (jlo("self_ring"), jlo("north_open"), jlo("south_open")) == (0, 0, -4)
    assert launches("self_ring", "given_three") == launches("self_ring", "eta_extended") == [("y", 1, 1, 1)]
    # 1440 x 720 x 48, halo 8: 6 blocks per row; 737 x 64 = 47168 rows of v, x 16 = 754688 threads = 2948 blocks
    assert launches("row_1440_two_launches", "everything_periodic_x") == [("yz", 6, 49 + 720, 1), ("x", 2948, 7, 1)]
    assert launches("row_1440", "everything_periodic_x") == [("fused", 6 * 769 + 2948 * 7, 1, 1)]
    x = printed["fill"][("row_1440_two_launches", "ts_periodic_x")]["launches"][1]
    assert (x["rows_c"], x["rows_v"], x["grid"]) == (736 * 64, 737 * 64, (2948, 4, 1))


@pytest.mark.parametrize("gname", list(W_GRIDS))
@pytest.mark.parametrize("name", list(PASSES))
def test_the_w_columns_of(printed, name, gname):
    got, want = printed["w"][(gname, name)], old_compute_w_impl(W_GRIDS[gname], PASSES[name])
    assert {k: got[k] for k in ("ia", "na", "ib", "nb", "rows")} == {k: want[k] for k in ("ia", "na", "ib", "nb", "rows")}
    assert (got["bx"], got["by"]) == want["block"] and got["ni"] == want["na"] + want["nb"]


def test_the_block_of_w_switches_below_64_columns(printed):
    block = lambda g, p: (printed["w"][(g, p)]["bx"], printed["w"][(g, p)]["by"])
    assert [block("latlon_180", p) for p in PASSES] == [(64, 4), (64, 4), (16, 16)]   # 194 and 179 columns; strips of 7 + 8
    assert [block("self_ring", p) for p in PASSES] == [(16, 16)] * 3                   # 46, 39 and 3 + 4 columns
    assert printed["w"][("latlon_180", "Edges")] == dict(ia=-7, na=7, ib=179, nb=8, rows=734, bx=16, by=16, ni=15)


@pytest.mark.parametrize("gname,box,forced", P_CASES)
def test_the_pressure_plan_of(printed, gname, box, forced):
    g = P_GRIDS[gname]
    got, want = printed["p"][(gname, box, forced)], old_compute_p_impl(g, BOXES[box][1](g), forced)
    assert tuple(int(x) for x in got["args"].split(",")) == want["args"], (gname, box)
    assert (int(got["form"]), tuple(int(x) for x in got["grid"].split(",")), int(got["tiles_a"])) == (want["form"], want["grid"], want["tiles_a"])


def test_a_few_pressure_plans_by_hand(printed):
    form = lambda g, b: int(printed["p"][(g, b, 0)]["form"])
    # whole range of a slab: Nx + 14 written columns and the helper column; 734 rows = 46 blocks of 16 rows; the tile form up to 400
    # columns on the lat-lon grid only: 360 + 15 = 375, 400 + 15 = 415
    assert [form("latlon_%d" % n, "whole") for n in (180, 360, 400, 401, 720)] == [1, 1, 2, 2, 2]
    assert [form("curvilinear_%d" % n, "whole") for n in (180, 360, 400, 401, 720)] == [2] * 5
    # own columns: Nx + 1; the two strips: 9 + 8 columns whatever the width
    assert [form("latlon_%d" % n, "own_columns") for n in (180, 360, 400, 401, 720)] == [1, 1, 2, 2, 2]
    assert [form("latlon_%d" % n, "strips") for n in (180, 720)] == [1, 1] and form("curvilinear_720", "strips") == 2
    # 1440 x 720: 1455 columns = 24 tiles of 63, x 46 = 1104 blocks: not narrow
    assert printed["p"][("latlon_1440", "whole", 0)] == dict(args="-7,1446,0,-1,-7,726", form="3", grid="24,46", tiles_a="24")
    # 180 columns: -7 .. 186 = 194 written columns in 13 tiles of 15, 734 rows in 62 blocks of 12
    assert printed["p"][("latlon_180", "whole", 0)] == dict(args="-7,186,0,-1,-7,726", form="1", grid="13,62", tiles_a="13")
    assert printed["p"][("latlon_180", "strips", 0)] == dict(args="-7,0,180,186,-7,726", form="1", grid="2,62", tiles_a="1")
    assert printed["p"][("curvilinear_720", "strips", 0)] == dict(args="-7,0,720,726,-7,726", form="2", grid="2,184", tiles_a="1")
    assert [int(printed["p"][("latlon_1440", "whole", k)]["form"]) for k in (1, 2, 3)] == [1, 2, 3]
