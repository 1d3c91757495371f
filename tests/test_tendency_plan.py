"""The launches of the tendency kernels, of the barotropic corrector and of the head of an unswept step (csrc/tendency_plan.hpp) as a
host-only harness: a small main includes the header alone and prints the plan of every request below on every grid below; they are
compared with expectations written out here -- the momentum_impl, tracer_rows, tracers_impl, catke_tendency_impl, corrector_impl and
the call sites of unswept_head this header replaced, restated line by line with their positional arguments, and a few numbers worked
out by hand -- not read off the header.  A second main includes csrc/model_layout.hpp and prints the runs of chunks of every layout
gb25_create accepts: what creation admits is what the launches can reach.  No GPU, no library."""
import os
import subprocess

import pytest

from test_launch_plan import GRIDS as FILL_GRIDS                       # the nine grids of the fills
from test_model_layout import BASE as CONFIG, LAYOUTS                  # every configuration whose layout is accepted there

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gb-25_amd", "csrc")
INT_MAX = 2**31 - 1
V2_TX, TYM, V3_OUT = 64, 4, 63   # tile width and rows of the momentum kernel, outputs per wave of the tracer kernel (as the old helpers had them)

# ---- grids: what launch_facts reads from a model.  Defaults: a Float32 single domain, 12-level chunks, flat bottom, WENO 5, rows by the rule
MORE = dict(real_bytes=4, mom_levels=12, trc_levels=12, Ry=1, immersed=0, order=5, forced=0)
GRIDS = {k: dict(MORE, **g, Ry=2 if g["ys_open"] or g["yn_open"] else 1) for k, g in FILL_GRIDS.items()}
BASE = GRIDS["walled"]
SLAB = dict(BASE, Ny=32, Nz=8, slab=1, x_periodic=0, fill_fused=1)
GRIDS.update({"slab_%d" % nx: dict(SLAB, Nx=nx) for nx in (128, 129, 130, 131, 192, 193)})   # interior_tile_columns_end first exceeds 1 at 131
GRIDS["rows_30"] = dict(BASE, Nx=200, Ny=30, Nz=24)                                          # Ny no multiple of 4 or 8
ROW_1440 = dict(GRIDS["row_1440"], mom_levels=24, trc_levels=24)
GRIDS.update({
    "t_1440": ROW_1440,                                            # 23 * 90 * 2 = 4140 blocks of 8 rows: two rows per lane
    "t_720": dict(ROW_1440, Nx=720),                               # 12 * 90 * 2 = 2160: one
    "t_1440_forced_1": dict(ROW_1440, forced=1),
    "t_720_forced_2": dict(ROW_1440, Nx=720, forced=2),
    "t_1440_f64": dict(ROW_1440, real_bytes=8),
    "t_1440_slab": dict(ROW_1440, slab=1, x_periodic=0),
    "t_1440_immersed": dict(ROW_1440, immersed=1, forced=2),       # no such instance: one row whatever is forced
    "t_1440_order_7": dict(ROW_1440, order=7, forced=2),
    "t_1440_curvilinear": dict(ROW_1440, curvilinear=1, north_fold=1),
    # the reach: tests/test_gpu_config5.py as one domain (4.4 GB per field), and the two grids of tests/test_model_layout.py
    "config5": dict(BASE, Nx=4320, Ny=2160, Nz=100, H=8, north_fold=1, curvilinear=1, immersed=1, mom_levels=24, trc_levels=24),
    "float32_5760": dict(BASE, Nx=5760, Ny=2880, Nz=48, H=8),
    "float64_4320": dict(BASE, Nx=4320, Ny=2160, Nz=100, H=8, real_bytes=8),
})
PASSES = {"Whole": 0, "Interior": 1, "Edges": 2}
HEAD_GRIDS = ("walled", "folded", "self_ring", "north_open", "south_open")


def derived(g):
    sx, sy_c = g["Nx"] + 2 * g["H"], g["Ny"] + 2 * g["H"]
    return dict(g, sx=sx, sy_c=sy_c, sy_v=sy_c + 1, pl_c=sx * sy_c, pl_v=sx * (sy_c + 1), w_elems=sx * sy_c * (g["Nz"] + 2 * g["H"] + 1), v_rows=g["Ny"])


# ---- the old helpers (gb25_api.hip of the parent commit)
def old_interior_tile_columns_end(g):
    nbx = (g["Nx"] + V2_TX - 1) // V2_TX
    return max(1, min(nbx - 1, (g["Nx"] - 3) // V2_TX))


def old_chunk_runs(g, kchunks):
    """the loop of momentum_impl over runs of chunks: (c0, c1 - c0, kofs) of every launch"""
    klen = (g["Nz"] + kchunks - 1) // kchunks
    plane_bytes, reach = g["pl_v"] * g["real_bytes"], 2147483648
    small = g["w_elems"] * g["real_bytes"] < reach
    runs, c0 = [], 0
    while c0 < kchunks:
        kofs = 0 if small else max(0, c0 * klen + g["H"] - 4)
        c1 = c0 + 1
        while c1 < kchunks and (min(g["Nz"], (c1 + 1) * klen) + g["H"] + 5 - kofs) * plane_bytes < reach:
            c1 += 1
        runs.append((c0, c1 - c0, kofs))
        c0 = c1
    return runs


def old_momentum_impl(g, part):
    nbx = (g["Nx"] + V2_TX - 1) // V2_TX
    nby = (g["v_rows"] + TYM - 1) // TYM
    kchunks = max(1, g["Nz"] // g["mom_levels"])
    tc = (nbx, nbx, 0, 0)
    if part != 0:
        hi = old_interior_tile_columns_end(g)
        tc = (hi - 1, hi - 1, 1, 0) if part == 1 else (1 + nbx - hi, 1, 0, hi)
    i_first = 1 if part == 1 else 0
    n = 1 if part == 2 else g["Nx"] - i_first
    return dict(nbx=nbx, nby=nby, kchunks=kchunks, tc=tc, nb=tc[0] * nby * kchunks, drag=(i_first, n), finish=int(part != 1),
                end=old_interior_tile_columns_end(g),
                split=int(bool(g["slab"] and old_interior_tile_columns_end(g) > 1 and not g["north_fold"] and g["Ry"] == 1)),
                runs=old_chunk_runs(g, kchunks))


def old_tracers_impl(g):
    nbx = (g["Nx"] + V3_OUT - 1) // V3_OUT
    kchunks = max(1, g["Nz"] // g["trc_levels"])
    exists = not g["immersed"] and not g["curvilinear"] and g["order"] == 5    # tracer_rows(m, nbx, kchunks)
    if not exists or g["forced"] == 1:
        rows = 1
    elif g["forced"] == 2:
        rows = 2
    else:
        rows = 2 if (not g["slab"] and g["real_bytes"] == 4 and nbx * ((g["Ny"] + 7) // 8) * kchunks >= 4096) else 1
    nby = (g["Ny"] + 4 * rows - 1) // (4 * rows)
    return dict(rows=rows, nbx=nbx, nby=nby, kchunks=kchunks, nb=nbx * nby * kchunks)


def old_catke_tendency_impl(g):
    nbx, nby, kchunks = (g["Nx"] + 2 * V3_OUT - 1) // (2 * V3_OUT), (g["Ny"] + 3) // 4, max(1, g["Nz"] // g["trc_levels"])
    return dict(rows=1, nbx=nbx, nby=nby, kchunks=kchunks, nb=nbx * nby * kchunks)


def old_corrector_impl(g, use_colsum, part, colsum_valid, halo_colsum_valid):
    """corrector_impl(m, use_colsum, part): None where it returned at once; else the kernel, the eight ints of its lambda, whether the
    sweep got the column integrals, and whether the exchange of the tendency pairs followed"""
    Nx, Ny, H, ext = g["Nx"], g["Ny"], g["H"], bool(g["slab"])
    i0, ni, skip_from, skip = (-H, Nx + 2 * H, INT_MAX, 0) if ext else (0, Nx, INT_MAX, 0)
    if part == 1:
        i0, ni = 0, Nx
    elif part == 2:
        if not ext:
            return None
        i0, ni, skip_from, skip = -H, 2 * H, 0, Nx
    cs = use_colsum and colsum_valid and part != 2
    cells_halo = ext and part == 2 and use_colsum and halo_colsum_valid
    cells = (ext and part == 1 and cs) or cells_halo
    return dict(form="cells" if cells else "sweep", cols=(i0, ni, skip_from, skip), rows=(0, Ny), reads=int(bool(cs)) if not cells else None,
                caches=int(part != 2))


# every CorrectorRequest a call site makes: (the request in C++, use_colsum, part of the old call)
CORRECTORS = {
    "all_with_colsum": ("CorrectorRequest::all(true)", True, 0),     # gb25_api.hip time_step_impl (both schedules)
    "all_without": ("CorrectorRequest::all(false)", False, 0),       # gb25_correct_velocities_and_cache_previous_tendencies
    "own_columns": ("CorrectorRequest::own_columns()", True, 1),     # slab_step.hpp stage_own_columns
    "halo_columns": ("CorrectorRequest::halo_columns()", True, 2),   # slab_step.hpp stage_halo_rows_corrector, stage_halo_columns
}
NO = (0, 0, INT_MAX, 0)   # NO_COLS


def old_heads(g, wfly):
    """the arguments (b, c, jr0, nj, bases, cache) of every call of unswept_head in the parent commit, and `wide` of SweepWFly"""
    Nx, Ny, H = g["Nx"], g["Ny"], g["H"]
    own, wide = (0, Nx, INT_MAX, 0), (-2, Nx + 4, INT_MAX, 0)
    own_pass = g["Ry"] == 1
    hs = H if g["ys_open"] else 0
    return {
        "in_consumers": ((64, 4), own, 0, Ny + 1, wide if wfly else NO, 1),                                   # time_step_impl
        "through_tracers_faces": ((64, 4), own, 0, Ny + (0 if g["north_fold"] else 1), NO, 0),
        "through_tracers_bases": ((64, 4), NO, 0, 0, wide, 0),
        "slab_own_columns": ((64, 4), own if own_pass else NO, 0, Ny + 1, (0, Nx - 1, INT_MAX, 0) if own_pass and wfly else NO, 1),   # stage_own_columns
        "slab_halo_strips": ((16, 16), (-H, 2 * H, 0, Nx), 0, Ny + 1, (-2, 5, 0, Nx - 1) if wfly else NO, 0),   # stage_halo_columns
        "mesh_rank": ((64, 4), (-H, Nx + 2 * H, INT_MAX, 0), -hs, hs + Ny + (H if g["yn_open"] else 1), wide if wfly else NO, 0),
    }


HEADS = {"in_consumers": "in_consumers(f, %s)", "through_tracers_faces": "through_tracers_faces(f)", "through_tracers_bases": "through_tracers_bases(f)",
         "slab_own_columns": "slab_own_columns(f, %s)", "slab_halo_strips": "slab_halo_strips(f, %s)", "mesh_rank": "mesh_rank(f, %s)"}

SHOW = r'''
#include <cstdio>
static void show_runs(const MomentumPlan& p) {
  std::printf("\truns=");
  for (int c0 = 0; c0 < p.kchunks;) {
    const ChunkRun r = chunk_run(p.chunks, c0);
    std::printf("%s%d,%d,%d", c0 ? ";" : "", r.first, r.count, r.kofs);
    c0 = r.first + r.count;
  }
}
static void show_momentum(const char* grid, const char* name, Pass pass, const LaunchFacts& f) {
  const MomentumPlan p = plan_momentum(pass, f);
  std::printf("mom\t%s\t%s\tnbx=%d\tnby=%d\tkchunks=%d\ttc=%d,%d,%d,%d\tnb=%d\tdrag=%d,%d\tfinish=%d\tend=%d\tsplit=%d", grid, name, p.nbx, p.nby,
              p.kchunks, p.n, p.nlead, p.bx0, p.bx1, p.nb(), p.drag_i_first, p.drag_n, (int)p.finish, p.interior_end, (int)p.splittable);
  show_runs(p);
  std::printf("\n");
}
'''
MAIN = SHOW + r'''
static void show_tracers(const char* kind, const char* grid, const TracerPlan& p) {
  std::printf("%s\t%s\t-\trows=%d\tnbx=%d\tnby=%d\tkchunks=%d\tnb=%d\n", kind, grid, p.rows, p.nbx, p.nby, p.kchunks, p.nb);
}
static void show_cols(const char* key, const Cols& c) { std::printf("\t%s=%d,%d,%d,%d", key, c.i0, c.ni, c.skip_from, c.skip); }
static void show_corrector(const char* grid, const char* name, CorrectorRequest rq, const LaunchFacts& f) {
  for (int v = 0; v < 4; v++) {
    const CorrectorPlan p = plan_corrector(rq, f, v & 1, v & 2);
    std::printf("corr\t%s\t%s,%d\tform=%s", grid, name, v, p.form == CorrectorForm::Nothing ? "nothing" : p.form == CorrectorForm::Cells ? "cells" : "sweep");
    show_cols("cols", p.cols);
    std::printf("\trows=%d,%d\treads=%d\tcaches=%d\n", p.j0, p.nj, (int)p.reads_colsum, (int)p.caches);
  }
}
static void show_head(const char* grid, const char* name, int carry_w, const HeadRequest& h) {
  std::printf("head\t%s\t%s,%d\tblock=%d,%d", grid, name, carry_w, h.bx, h.by);
  show_cols("cols", h.cols);
  std::printf("\trows=%d,%d", h.j0, h.nj);
  show_cols("bases", h.bases);
  std::printf("\tcache=%d\n", (int)h.cache);
}
int main() {
'''
# ... and the second program: csrc/model_layout.hpp, the facts as launch_facts fills them from an adopted layout
LAYOUT_MAIN = SHOW + r'''
static void show_layout(const char* name, gb25_config c, int real_bytes) {
  const LayoutPlan p = plan_layout(c, real_bytes, nullptr);
  if (p.status) return;
  const ModelLayout& L = p.layout;
  const Dims v = parent_dims(L, GB25_V), w = parent_dims(L, GB25_W);
  LaunchFacts f{};
  f.Nx = L.Nx; f.Ny = L.Ny; f.Nz = L.Nz; f.H = L.H; f.slab = L.slab; f.north_fold = L.north_fold; f.Ry = L.Ry;
  f.pl_v = v.nx * v.ny; f.w_elems = (long)w.elems(); f.real_bytes = real_bytes; f.mom_chunk_levels = f.trc_chunk_levels = L.chunk_levels;
  f.v_rows = L.Ny;
  show_momentum(name, "Whole", Pass::Whole, f);
  std::printf("layout\t%s\t-\tNx=%d\tNy=%d\tNz=%d\tH=%d\tlevels=%d\n", name, L.Nx, L.Ny, L.Nz, L.H, L.chunk_levels);
}
int main() {
'''


def facts(g):
    g, b = derived(g), lambda k: "true" if g[k] else "false"
    return "LaunchFacts{%d, %d, %d, %d, %d, %d, %s, %s, %d, %s, %s, %s, %s, %s, %d, %d, %dL, %d, %d, %d, %d, %d, %s, %d, %d}" % (
        g["Nx"], g["Ny"], g["Nz"], g["H"], g["sy_c"], g["sy_v"], b("x_periodic"), b("north_fold"), g["pivot_slaved"], b("slab"), b("ys_open"),
        b("yn_open"), b("fill_fused"), b("curvilinear"), g["pl_c"], g["pl_v"], g["w_elems"], g["real_bytes"], g["mom_levels"], g["trc_levels"],
        g["v_rows"], g["Ry"], b("immersed"), g["order"], g["forced"])


def source():
    body = []
    for gname, g in GRIDS.items():
        body.append("  {\n    const LaunchFacts f = %s;\n" % facts(g))
        for name in PASSES:
            body.append('    show_momentum("%s", "%s", Pass::%s, f);\n' % (gname, name, name))
        body.append('    show_tracers("trc", "%s", plan_tracers(f));\n    show_tracers("single", "%s", plan_single(f));\n' % (gname, gname))
        if gname in HEAD_GRIDS:
            for name, (cxx, _, _) in CORRECTORS.items():
                body.append('    show_corrector("%s", "%s", %s, f);\n' % (gname, name, cxx))
            for name, cxx in HEADS.items():
                for carry in ((0, 1) if "%s" in cxx else (0,)):
                    body.append('    show_head("%s", "%s", %d, HeadRequest::%s);\n' % (gname, name, carry, cxx % ("true" if carry else "false") if "%s" in cxx else cxx))
            body.append('    std::printf("wide\\t%s\\t-");\n    show_cols("cols", wide_bases(f));\n    std::printf("\\n");\n' % gname)
        body.append("  }\n")
    return '#include "%s"\n' % os.path.join(CSRC, "tendency_plan.hpp") + MAIN + "".join(body) + "  return 0;\n}\n"


def layout_source():
    body = []
    for name, (change, _) in LAYOUTS.items():
        c = dict(CONFIG, **change)
        body.append("  {\n    gb25_config c{};\n    c.Nx = %d; c.Ny = %d; c.Nz = %d; c.halo = %d; c.substeps = %d; c.rank = %d; c.nranks = %d; c.slab_mode = %d; "
                    "c.grid_type = %d; c.ranks_y = %d;\n" % tuple(c[k] for k in ("Nx", "Ny", "Nz", "halo", "substeps", "rank", "nranks", "slab_mode", "grid_type", "ranks_y")))
        body.append('    show_layout("%s", c, %d);\n  }\n' % (name, c["real_bytes"]))
    return '#include "%s"\n' % os.path.join(CSRC, "model_layout.hpp") + LAYOUT_MAIN + "".join(body) + "  return 0;\n}\n"


def parse(out):
    got = {}
    for line in out.splitlines():
        kind, gname, name, *rest = line.split("\t")
        d = {}
        for kv in rest:
            k, v = kv.split("=", 1)
            if k == "runs":
                d[k] = [tuple(int(x) for x in r.split(",")) for r in v.split(";")]
            elif k == "form":
                d[k] = v
            else:
                d[k] = tuple(int(x) for x in v.split(",")) if "," in v else int(v)
        got[(kind, gname, name)] = d
    return got


def build_and_run(tmp, stem, text, flags):
    src, exe = tmp / (stem + ".cpp"), tmp / stem
    src.write_text(text)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-o", str(exe), str(src)], check=True)
    return subprocess.run([str(exe)], check=True, capture_output=True, text=True)


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("tendency_plan")


@pytest.fixture(scope="module")
def printed(tmp):
    return parse(build_and_run(tmp, "plan", source(), []).stdout)


@pytest.fixture(scope="module")
def layouts(tmp):
    return parse(build_and_run(tmp, "layouts", layout_source(), []).stdout)


def test_the_program_runs_clean_under_the_sanitizers(tmp, printed):
    """the same stand-alone program with -fsanitize=address,undefined: no report, the same output"""
    run = build_and_run(tmp, "plan_san", source(), ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert run.stderr == "" and parse(run.stdout) == printed


@pytest.mark.parametrize("gname", list(GRIDS))
@pytest.mark.parametrize("name", list(PASSES))
def test_the_momentum_plan_of(printed, name, gname):
    want = old_momentum_impl(derived(GRIDS[gname]), PASSES[name])
    assert printed[("mom", gname, name)] == want, (gname, name)


def test_the_split_begins_at_131_columns(printed):
    """(Nx - 3) / 64 reaches 2 at 131 columns: tile column 1 then reads own columns only (up to column 127 + 3)"""
    end = {nx: printed[("mom", "slab_%d" % nx, "Whole")]["end"] for nx in (128, 129, 130, 131, 192, 193)}
    assert end == {128: 1, 129: 1, 130: 1, 131: 2, 192: 2, 193: 2}
    assert [printed[("mom", "slab_%d" % nx, "Whole")]["split"] for nx in (130, 131, 192, 193)] == [0, 1, 1, 1]
    assert printed[("mom", "self_ring", "Whole")]["split"] == 0 and printed[("mom", "walled", "Whole")]["split"] == 0
    # 131 and 192 columns: three tile columns, the interior pass takes column 1, the edges 0 and 2; 193: four, the edges 0, 2, 3
    assert [printed[("mom", "slab_131", p)]["tc"] for p in PASSES] == [(3, 3, 0, 0), (1, 1, 1, 0), (2, 1, 0, 2)]
    assert [printed[("mom", "slab_193", p)]["tc"] for p in PASSES] == [(4, 4, 0, 0), (1, 1, 1, 0), (3, 1, 0, 2)]
    assert printed[("mom", "slab_192", "Interior")]["drag"] == (1, 191) and printed[("mom", "slab_192", "Edges")]["drag"] == (0, 1)


@pytest.mark.parametrize("gname", ["slab_131", "slab_192", "slab_193", "t_1440_slab", "rows_30"])
def test_the_passes_partition_the_tile_columns_of(printed, gname):
    def columns(p):
        n, nlead, bx0, bx1 = printed[("mom", gname, p)]["tc"]
        return [bx0 + q if q < nlead else bx1 + (q - nlead) for q in range(n)]   # tile_column (tendency_kernels.hpp)
    nbx = printed[("mom", gname, "Whole")]["nbx"]
    assert columns("Whole") == list(range(nbx))
    assert sorted(columns("Interior") + columns("Edges")) == list(range(nbx))
    assert all(printed[("mom", gname, p)]["nb"] == len(columns(p)) * printed[("mom", gname, p)]["nby"] * printed[("mom", gname, p)]["kchunks"] for p in PASSES)


def test_a_few_momentum_plans_by_hand(printed):
    # 200 x 30 x 24: 4 tile columns, 30 rows = 8 rows of tiles (the last half empty), 2 chunks of 12 levels
    got = printed[("mom", "rows_30", "Whole")]
    assert (got["nbx"], got["nby"], got["kchunks"], got["nb"], got["runs"]) == (4, 8, 2, 64, [(0, 2, 0)])
    # the headline grid: 23 x 180 x 2 blocks in one launch
    got = printed[("mom", "t_1440", "Whole")]
    assert (got["nbx"], got["nby"], got["kchunks"], got["nb"], got["runs"], got["finish"]) == (23, 180, 2, 8280, [(0, 2, 0)], 1)
    assert printed[("mom", "t_1440", "Interior")]["finish"] == 0 and printed[("mom", "t_1440", "Edges")]["finish"] == 1


@pytest.mark.parametrize("gname", list(GRIDS))
def test_the_tracer_plans_of(printed, gname):
    g = derived(GRIDS[gname])
    assert printed[("trc", gname, "-")] == old_tracers_impl(g), gname
    assert printed[("single", gname, "-")] == old_catke_tendency_impl(g), gname


def test_the_rows_per_lane_by_hand(printed):
    rows = lambda g: printed[("trc", g, "-")]["rows"]
    assert printed[("trc", "t_1440", "-")] == dict(rows=2, nbx=23, nby=90, kchunks=2, nb=4140)      # 23 * 90 * 2 >= 4096
    assert printed[("trc", "t_720", "-")] == dict(rows=1, nbx=12, nby=180, kchunks=2, nb=4320)      # 12 * 90 * 2 = 2160 blocks of 8 rows
    assert (rows("t_1440_forced_1"), rows("t_720_forced_2")) == (1, 2)
    assert (rows("t_1440_f64"), rows("t_1440_slab"), rows("t_1440_immersed"), rows("t_1440_order_7"), rows("t_1440_curvilinear")) == (1,) * 5
    assert printed[("trc", "rows_30", "-")] == dict(rows=1, nbx=4, nby=8, kchunks=2, nb=64)
    assert printed[("single", "t_1440", "-")] == dict(rows=1, nbx=12, nby=180, kchunks=2, nb=4320)   # 1440 / 126 = 11.4


def check_reach(runs, kchunks, Nz, H, plane_bytes):
    """computed here, not by the old loop: the runs tile [0, kchunks) without gap or overlap; the run's base is no higher than the
    lowest plane its first level's stencil reads (three levels down); and the highest plane of the run -- plane min(Nz, (c + 1) klen)
    + H + 4 of the parent: above the last level its window, w and a top halo layer -- ends within 2^31 bytes of the base.  The run's
    first chunk included, which the launch loop takes unchecked."""
    assert [r[0] for r in runs] == [sum(r[1] for r in runs[:q]) for q in range(len(runs))] and sum(r[1] for r in runs) == kchunks
    klen = -(-Nz // kchunks)
    for first, count, kofs in runs:
        assert 0 <= kofs <= first * klen + H - 3                       # the base is at or below the lowest stencil plane of the first level
        highest = min(Nz, (first + count) * klen) + H + 4
        assert (highest - kofs + 1) * plane_bytes < 2**31, (first, count, kofs)


@pytest.mark.parametrize("gname,runs", [("config5", 4), ("float32_5760", 4), ("float64_4320", 8)])
def test_the_runs_of_chunks_of(printed, gname, runs):
    g = derived(GRIDS[gname])
    got = printed[("mom", gname, "Whole")]
    assert got["runs"] == old_chunk_runs(g, got["kchunks"]) and len(got["runs"]) == runs
    check_reach(got["runs"], got["kchunks"], g["Nz"], g["H"], g["pl_v"] * g["real_bytes"])


def test_the_runs_of_config_5_by_hand(printed):
    # 4336 x 2177 x 4 B = 37.8 MB per plane: 56 planes within reach.  4 chunks of 25 levels; a run of one chunk touches 25 + 9 planes
    # from its base, three levels below its first (plane 25 c + 8 - 4); with the next chunk 59: every chunk is a run of its own
    assert printed[("mom", "config5", "Whole")]["runs"] == [(0, 1, 4), (1, 1, 29), (2, 1, 54), (3, 1, 79)]
    # 5776 x 2897 x 4 B = 66.9 MB: 32 planes.  4 chunks of 12 levels: 21 planes alone, 33 with the next
    assert printed[("mom", "float32_5760", "Whole")]["runs"] == [(0, 1, 4), (1, 1, 16), (2, 1, 28), (3, 1, 40)]
    # 4336 x 2177 x 8 B = 75.5 MB: 28 planes.  8 chunks of 13 levels (the last of 9): 22 planes alone, 35 with the next
    assert printed[("mom", "float64_4320", "Whole")]["runs"] == [(c, 1, 13 * c + 4) for c in range(8)]


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_what_creation_admits_the_launches_reach(layouts, name):
    """every layout tests/test_model_layout.py sees accepted, with the chunking creation chose: the old loop's runs, and within reach"""
    c = dict(CONFIG, **LAYOUTS[name][0])
    L, got = layouts[("layout", name, "-")], layouts[("mom", name, "Whole")]
    g = derived(dict(BASE, Nx=L["Nx"], Ny=L["Ny"], Nz=L["Nz"], H=L["H"], real_bytes=c["real_bytes"], mom_levels=L["levels"]))
    assert got["runs"] == old_chunk_runs(g, got["kchunks"])
    check_reach(got["runs"], got["kchunks"], g["Nz"], g["H"], g["pl_v"] * c["real_bytes"])


@pytest.mark.parametrize("gname", HEAD_GRIDS)
@pytest.mark.parametrize("name", list(CORRECTORS))
def test_the_corrector_plan_of(printed, name, gname):
    g = derived(GRIDS[gname])
    _, use_colsum, part = CORRECTORS[name]
    for v in range(4):
        got, want = printed[("corr", gname, "%s,%d" % (name, v))], old_corrector_impl(g, use_colsum, part, bool(v & 1), bool(v & 2))
        if want is None:
            assert got["form"] == "nothing" and not g["slab"], (gname, name)
            continue
        if want["reads"] is None:   # (k_corrector_cells takes the column integrals always)
            want["reads"] = got["reads"]
        assert got == want, (gname, name, v)


def test_a_few_corrector_plans_by_hand(printed):
    plan = lambda g, n, v: printed[("corr", g, "%s,%d" % (n, v))]
    assert plan("walled", "all_with_colsum", 1) == dict(form="sweep", cols=(0, 40, INT_MAX, 0), rows=(0, 21), reads=1, caches=1)
    assert plan("walled", "all_with_colsum", 0)["reads"] == 0 and plan("walled", "all_without", 3)["reads"] == 0
    assert plan("self_ring", "all_with_colsum", 3) == dict(form="sweep", cols=(-4, 48, INT_MAX, 0), rows=(0, 21), reads=1, caches=1)
    assert plan("self_ring", "own_columns", 1)["form"] == "cells" and plan("self_ring", "own_columns", 2)["form"] == "sweep"
    assert plan("self_ring", "halo_columns", 2) == dict(form="cells", cols=(-4, 8, 0, 40), rows=(0, 21), reads=0, caches=0)
    assert plan("self_ring", "halo_columns", 1) == dict(form="sweep", cols=(-4, 8, 0, 40), rows=(0, 21), reads=0, caches=0)
    assert plan("walled", "halo_columns", 3)["form"] == plan("folded", "halo_columns", 3)["form"] == "nothing"


@pytest.mark.parametrize("gname", HEAD_GRIDS)
def test_the_head_requests_of(printed, gname):
    g = derived(GRIDS[gname])
    for wfly in (0, 1):
        for name, (block, cols, jr0, nj, bases, cache) in old_heads(g, wfly).items():
            if wfly and "%s" not in HEADS[name]:
                continue
            assert printed[("head", gname, "%s,%d" % (name, wfly))] == dict(block=block, cols=cols, rows=(jr0, nj), bases=bases, cache=cache), (gname, name, wfly)
    assert printed[("wide", gname, "-")]["cols"] == (-2, g["Nx"] + 4, INT_MAX, 0)


def test_a_few_heads_by_hand(printed):
    head = lambda g, n, w: printed[("head", g, "%s,%d" % (n, w))]
    assert head("walled", "in_consumers", 1) == dict(block=(64, 4), cols=(0, 40, INT_MAX, 0), rows=(0, 22), bases=(-2, 44, INT_MAX, 0), cache=1)
    assert head("folded", "through_tracers_faces", 0)["rows"] == (0, 24) and head("walled", "through_tracers_faces", 0)["rows"] == (0, 22)
    assert head("self_ring", "slab_halo_strips", 1) == dict(block=(16, 16), cols=(-4, 8, 0, 40), rows=(0, 22), bases=(-2, 5, 0, 39), cache=0)
    assert head("self_ring", "slab_own_columns", 1)["bases"] == (0, 39, INT_MAX, 0)
    assert head("north_open", "slab_own_columns", 1) == dict(block=(64, 4), cols=NO, rows=(0, 22), bases=NO, cache=1)
    assert head("north_open", "mesh_rank", 0)["rows"] == (0, 25) and head("south_open", "mesh_rank", 0)["rows"] == (-4, 26)
    assert head("south_open", "mesh_rank", 1)["cols"] == (-4, 48, INT_MAX, 0) and head("south_open", "mesh_rank", 1)["bases"] == (-2, 44, INT_MAX, 0)
