"""The layout of a model (csrc/model_layout.hpp) as a host-only harness: a small main includes the header alone, prints the layout or
the refusal of each configuration below, and they are compared with expectations written out here -- read off the gb25_create this
header replaced (its rules are restated in the helpers below where a table would be long), not off the header.  No GPU, no library.

Not here: "no HIP device visible" and "device ordinal out of range".  They are the device's refusals, issued by gb25_create after the
layout has accepted the configuration."""
import math
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1   # GB25_ERR_INVALID_ARGUMENT (include/gb25.h)

# the fields in the order of gb25_field (include/gb25.h), and what the old gb25_create, gb25_set_closure_catke and gb25_field_dims
# said of each: is_v_shaped's list, is_2d's range (eta .. Gn.V, and Jb), "+ 1" for w and for the three kappa, CATKE's fields from e on
FIELDS = ["u", "v", "w", "T", "S", "pHY", "Gn.u", "Gn.v", "Gn.T", "Gn.S", "Gm.u", "Gm.v", "Gm.T", "Gm.S", "eta", "U", "V", "eta_bar",
          "U_bar", "V_bar", "Gn.U", "Gn.V", "e", "Gn.e", "Gm.e", "kappa_u", "kappa_c", "kappa_e", "Le", "Jb", "previous_u", "previous_v"]
V_SHAPED = {"v", "Gn.v", "Gm.v", "V", "V_bar", "Gn.V", "previous_v"}
FLAT = {"eta", "U", "V", "eta_bar", "U_bar", "V_bar", "Gn.U", "Gn.V", "Jb"}
Z_FACES = {"w", "kappa_u", "kappa_c", "kappa_e"}
CATKE = set(FIELDS[FIELDS.index("e"):])

# every configuration starts from gb25_default_config(1440, 720, 48) in a Float32 library, GB25_TRACER_ROWS unset
BASE = dict(Nx=1440, Ny=720, Nz=48, halo=8, substeps=30, rank=0, nranks=1, slab_mode=0, grid_type=0, ranks_y=1, real_bytes=4, rows=None)
TRIPOLAR = 3
SINGLE = dict(Rx=1, Ry=1, rx=0, ry=0, Nx=1440, Ny=720, j0=0, ys_open=0, yn_open=0, slab=0, north_fold=0, north_wall=1, W=0, Wy=0, Wys=0,
              Ns=21, chunk_levels=24, baro_ahead=1, split_tendencies=1, tracer_rows_forced=0)
MESH = dict(nranks=8, ranks_y=2)   # 4 x 2 ranks of 360 columns and 360 rows

LAYOUTS = {
    # ---- decomposition
    "single": (dict(), SINGLE),
    "x8_rank3": (dict(nranks=8, rank=3), dict(Rx=8, Ry=1, rx=3, ry=0, Nx=180, Ny=720, j0=0, ys_open=0, yn_open=0, slab=1, W=30, Wy=0,
                                              Wys=0, chunk_levels=12, baro_ahead=1, split_tendencies=1)),
    "mesh_bottom_row": (dict(MESH, rank=1), dict(Rx=4, Ry=2, rx=1, ry=0, Nx=360, Ny=360, j0=0, ys_open=0, yn_open=1, slab=1, north_fold=0,
                                                 north_wall=0, W=30, Wy=30, Wys=0, split_tendencies=0, chunk_levels=12)),
    "mesh_top_row": (dict(MESH, rank=6), dict(Rx=4, Ry=2, rx=2, ry=1, Nx=360, Ny=360, j0=360, ys_open=1, yn_open=0, slab=1, north_fold=0,
                                              north_wall=1, W=30, Wy=0, Wys=30, split_tendencies=0)),
    "self_ring": (dict(slab_mode=1), dict(SINGLE, slab=1, W=30, chunk_levels=24)),
    "tracer_rows_2": (dict(rows="2"), dict(SINGLE, tracer_rows_forced=2)),
    # ---- chunk levels: 24 where (Nx / 64)(Ny / 4)(Nz / 24) >= 4096 blocks, else 12 ("single", "x8_rank3" above) ...
    "chunks_just_four_rounds": (dict(Nx=1024, Ny=512, Nz=48), dict(chunk_levels=24, klen=24, planes=34)),    # 16 * 128 * 2 = 4096
    "chunks_below_four_rounds": (dict(Nx=1024, Ny=508, Nz=48), dict(chunk_levels=12, klen=12, planes=22)),   # 16 * 127 * 2 = 4064
    # ... and 12 where 24 lie beyond the 2 GB reach of the tendency kernels (the wanted change: the old check priced Nz / 12 chunks
    # whatever had been chosen, accepted both grids, and ran them with 24).  bytes = (Nx + 2H)(Ny + 2H + 1)(klen + 10) sizeof(real)
    "float32_5760": (dict(Nx=5760, Ny=2880, Nz=48), dict(chunk_levels=12, klen=12, planes=22, bytes=5776 * 2897 * 22 * 4)),
    "float64_4320": (dict(Nx=4320, Ny=2160, Nz=100, real_bytes=8), dict(chunk_levels=12, klen=13, planes=23, bytes=4336 * 2177 * 23 * 8)),
    # ---- W, Wy, Wys: W = Ns + 1 + H on a slab; Wy = Ns + 1 below a fold, W below a neighbour; Wys = W above a neighbour
    "folded_single": (dict(grid_type=TRIPOLAR), dict(SINGLE, north_fold=1, north_wall=0, W=0, Wy=22, Wys=0)),
    "folded_mesh_top_row": (dict(MESH, rank=6, grid_type=TRIPOLAR), dict(north_fold=1, north_wall=0, ys_open=1, yn_open=0, W=30, Wy=22, Wys=30)),
    "folded_mesh_bottom_row": (dict(MESH, rank=1, grid_type=TRIPOLAR), dict(north_fold=0, north_wall=0, ys_open=0, yn_open=1, W=30, Wy=30, Wys=0)),
    "substeps_12_slab": (dict(slab_mode=1, substeps=12), dict(Ns=8, W=17)),
    # ---- the default of SUBCYCLE_LOOKAHEAD: from 8 M cells of the GLOBAL grid, and on every slab
    "small": (dict(Nx=128, Ny=64, Nz=8), dict(baro_ahead=0, chunk_levels=12, slab=0, Nx=128, Ny=64)),
    "small_slab": (dict(Nx=64, Ny=16, Nz=8, slab_mode=1), dict(baro_ahead=1, slab=1, W=30)),
    # ---- the three layouts of the field shapes below
    "walled": (dict(Nx=40, Ny=21, Nz=6, halo=4), dict(north_wall=1, north_fold=0, Nx=40, Ny=21)),
    "folded": (dict(Nx=40, Ny=24, Nz=6, halo=4, grid_type=TRIPOLAR, substeps=12), dict(north_wall=0, north_fold=1, Wy=9, W=0)),
    "below_a_neighbour": (dict(Nx=40, Ny=42, Nz=6, halo=4, substeps=12, nranks=2, ranks_y=2, rank=0),
                          dict(north_wall=0, north_fold=0, yn_open=1, Nx=40, Ny=21, W=13, Wy=13, Wys=0)),
}
SHAPED = ("walled", "folded", "below_a_neighbour")

# every refusal of the old gb25_create once, in its order there, by a distinctive piece of its text ...
REFUSALS = {
    "too_small": (dict(Nx=4), "invalid configuration: need Nx,Ny >= 8, Nz >= 4, halo >= 4, 1 <= substeps <= 4096, nranks = Rx ranks_y, "
                              "Nx % Rx == 0, Ny % ranks_y == 0"),
    "rows_do_not_divide": (dict(Ny=721, nranks=2, ranks_y=2), "invalid configuration"),
    "slab_mode_2": (dict(slab_mode=2), "slab_mode must be 0 (x halos by exchange iff nranks > 1) or 1 (always)"),
    "tracer_rows_3": (dict(rows="3"), "GB25_TRACER_ROWS must be 1 or 2 (unset: the library's rule)"),
    "narrower_than_the_halo": (dict(Nx=64, Ny=16, Nz=8, nranks=16), "slab narrower than the halo"),
    "band_narrower_than_the_halo": (dict(Nx=64, Ny=16, Nz=8, nranks=2, ranks_y=2), "a rank's band of rows is narrower than the halo"),
    "beyond_reach": (dict(Nx=8640, Ny=2160, Nz=100), "and 23 planes of 2 GB together: decompose in x (nranks) so that the local slab is narrower"),
    "grid_type_7": (dict(grid_type=7), "grid_type 7: 0 lat-lon, 1 lat-lon with the Gaussian islands"),
    "grid_type_negative": (dict(grid_type=-1), "grid_type -1: 0 lat-lon"),
    "odd_Nx_on_a_fold": (dict(Nx=33, Ny=16, Nz=8, grid_type=4), "the tripolar grid needs an even Nx and Ny >= 2 halo"),
    "few_rows_on_a_fold": (dict(Nx=32, Ny=12, Nz=8, grid_type=TRIPOLAR), "the tripolar grid needs an even Nx and Ny >= 2 halo"),
    "slab_narrower_than_W": (dict(Nx=16, Ny=16, Nz=8, grid_type=TRIPOLAR, slab_mode=1), "slab width 16 is narrower than the barotropic halo 30"),
    "fold_needs_rows": (dict(Nx=48, Ny=20, Nz=6, grid_type=TRIPOLAR),
                        "a folded grid needs Ny >= 24 rows per rank for its 21 effective substeps (the sub-cycle's image rows beyond the "
                        "pivot row: Ns + 1 of them, made from the rows south of it); this rank has 20"),
    "band_narrower_than_W": (dict(Nx=64, Ny=40, Nz=8, nranks=2, ranks_y=2), "a rank's band of 20 rows is narrower than the barotropic halo 30"),
    # ... and configurations that break two rules at once: the earlier one in that order wins
    "too_small_and_slab_mode": (dict(Nx=4, slab_mode=2), "invalid configuration"),
    "tracer_rows_and_grid_type": (dict(rows="3", grid_type=7), "GB25_TRACER_ROWS must be 1 or 2"),
    "reach_and_grid_type": (dict(Nx=8640, Ny=2160, Nz=100, grid_type=7), "decompose in x"),
    "odd_Nx_and_slab_narrower_than_W": (dict(Nx=33, Ny=16, Nz=8, grid_type=4, slab_mode=1), "even Nx"),
    "slab_narrower_than_W_and_fold_needs_rows": (dict(Nx=16, Ny=20, Nz=8, grid_type=TRIPOLAR, slab_mode=1), "barotropic halo"),
}

# the grid whose reach is asked for once as creation asks and once as the option hook does
REACH_GRID, REACH_LEVELS = "float32_5760", (12, 24, 6, 48)

MAIN = r'''
#include <cstdio>
static gb25_config config(int Nx, int Ny, int Nz, int halo, int substeps, int rank, int nranks, int slab_mode, int grid_type, int ranks_y) {
  gb25_config c{};
  c.Nx = Nx; c.Ny = Ny; c.Nz = Nz; c.halo = halo; c.substeps = substeps; c.rank = rank; c.nranks = nranks;
  c.slab_mode = slab_mode; c.grid_type = grid_type; c.ranks_y = ranks_y;
  return c;
}
static void show_reach(const char* name, const ModelLayout& L, int levels, int real_bytes) {
  const TendencyReach r = tendency_reach_ok(L, levels, real_bytes);
  std::printf("reach\t%s\t%d\tok=%d\tklen=%d\tplanes=%d\tbytes=%.0f\n", name, levels, (int)r.ok, r.klen, r.planes, r.bytes);
}
static void show(const char* name, const gb25_config& c, int real_bytes, const char* rows, bool shapes, bool reach) {
  const LayoutPlan p = plan_layout(c, real_bytes, rows);
  if (p.status) {
    std::printf("refused\t%s\tstatus=%d\ttext=%s\n", name, (int)p.status, p.refusal.c_str());
    return;
  }
  const ModelLayout& L = p.layout;
  const TendencyReach r = tendency_reach_ok(L, L.chunk_levels, real_bytes);
  std::printf("layout\t%s\tRx=%d\tRy=%d\trx=%d\try=%d\tNx=%d\tNy=%d\tj0=%d\tys_open=%d\tyn_open=%d\tslab=%d\tnorth_fold=%d\tnorth_wall=%d",
              name, L.Rx, L.Ry, L.rx, L.ry, L.Nx, L.Ny, L.j0, (int)L.ys_open, (int)L.yn_open, (int)L.slab, (int)L.north_fold, (int)L.north_wall);
  std::printf("\tW=%d\tWy=%d\tWys=%d\tNs=%d\tchunk_levels=%d\tok=%d\tklen=%d\tplanes=%d\tbytes=%.0f\tbaro_ahead=%d\tsplit_tendencies=%d"
              "\ttracer_rows_forced=%d\n", L.W, L.Wy, L.Wys, L.sub.Ns, L.chunk_levels, (int)r.ok, r.klen, r.planes, r.bytes, L.baro_ahead,
              L.split_tendencies, L.tracer_rows_forced);
  if (shapes)
    for (int id = 0; id < GB25_FIELD_COUNT; id++) {
      const Dims a = parent_dims(L, id), b = interior_dims(L, id), h = host_dims(L, id, true), i = host_dims(L, id, false);
      std::printf("shape\t%s\t%d\tparent=%d,%d,%d\tinterior=%d,%d,%d\twith_halos=%d,%d,%d\twithout=%d,%d,%d\tflags=%d%d%d\tglobal_rows=%d\n", name,
                  id, a.nx, a.ny, a.nz, b.nx, b.ny, b.nz, h.nx, h.ny, h.nz, i.nx, i.ny, i.nz, (int)is_v_shaped(id), (int)is_2d(id),
                  (int)is_catke_field(id), global_rows(L, id));
    }
  if (reach)
    for (int levels : {REACH_LEVELS}) show_reach(name, L, levels, real_bytes);
}
static void show_substeps(int N) {
  const Substepping s = plan_substeps(N);
  std::printf("substeps\t%d\tNs=%d\tdtau_frac=%a\tweights=", N, s.Ns, s.dtau_frac);
  for (int k = 0; k < s.Ns; k++) std::printf("%s%a", k ? "," : "", s.weights[k]);
  std::printf("\n");
}
int main() {
  std::printf("fields\t%d\n", (int)GB25_FIELD_COUNT);
'''


def substepping(N):
    """build_substeps of the old gb25_api.hip, line by line"""
    p, q, r = 2.0, 4.0, 0.18927
    tau0 = (p + 2) * (p + q + 2) / (p + 1) / (p + q + 1)
    w = [0.0] * (N + 1)
    for k in range(1, N + 1):
        x = (2.0 * k / N) / tau0
        w[k] = math.pow(x, p) * (1 - math.pow(x, q)) - r * x
    lo, hi = 0, N + 1
    while lo < hi - 1:
        mid = lo + ((hi - lo) >> 1)
        if w[mid] < 0.0:
            hi = mid
        else:
            lo = mid
    s = 0.0
    for k in range(1, lo + 1):
        s += w[k]
    return lo, 2.0 / N, [w[k] / s for k in range(1, lo + 1)]


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("model_layout")
    src, exe = tmp / "layout.cpp", tmp / "layout"
    body = []
    for name, (change, _) in list(LAYOUTS.items()) + list(REFUSALS.items()):
        c = dict(BASE, **change)
        assert set(c) == set(BASE), name
        rows = "nullptr" if c["rows"] is None else '"%s"' % c["rows"]
        body.append('  show("%s", config(%d, %d, %d, %d, %d, %d, %d, %d, %d, %d), %d, %s, %s, %s);\n' % (
            name, c["Nx"], c["Ny"], c["Nz"], c["halo"], c["substeps"], c["rank"], c["nranks"], c["slab_mode"], c["grid_type"], c["ranks_y"],
            c["real_bytes"], rows, "true" if name in SHAPED else "false", "true" if name == REACH_GRID else "false"))
    body += ["  show_substeps(%d);\n" % N for N in (30, 12, 4)]
    main = MAIN.replace("REACH_LEVELS", ", ".join(str(v) for v in REACH_LEVELS))
    src.write_text('#include "%s"\n' % os.path.join(ROOT, "gb-25_amd", "csrc", "model_layout.hpp") + main + "".join(body) + "  return 0;\n}\n")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    got = dict(layout={}, refused={}, shape={}, reach={}, substeps={}, fields=None)
    for line in out.splitlines():
        kind, name, *rest = line.split("\t")
        if kind == "fields":
            got["fields"] = int(name)
        elif kind in ("shape", "reach"):
            got[kind][(name, int(rest[0]))] = dict(kv.split("=", 1) for kv in rest[1:])
        else:
            got[kind][name] = dict(kv.split("=", 1) for kv in rest)
    return got


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_the_layout_of(printed, name):
    assert name in printed["layout"], printed["refused"].get(name)
    got, want = printed["layout"][name], LAYOUTS[name][1]
    wrong = {k: (got[k], v) for k, v in want.items() if got[k] != str(v)}
    assert not wrong, f"{name}: (planned, expected) {wrong}"
    # whatever was chosen lies within the reach: fewer than 2^31 bytes from the first plane a block touches
    assert got["ok"] == "1" and int(got["bytes"]) < 2**31, (name, got["bytes"])


@pytest.mark.parametrize("name", list(REFUSALS))
def test_the_refusal_of(printed, name):
    assert name in printed["refused"], f"{name} was accepted: {printed['layout'].get(name)}"
    got = printed["refused"][name]
    assert got["status"] == str(INVALID) and REFUSALS[name][1] in got["text"], (name, got)
    assert "%" not in got["text"].replace("Nx % Rx", "").replace("Ny % ranks_y", ""), got["text"]   # (every format was filled in)


def test_the_text_of_the_reach_refusal(printed):
    """8640 x 2160 x 100: 8656 * 2177 * 117 = 2.2e9 elements per 3-D array, as the old message printed them"""
    plane = 8656 * 2177
    elems = plane * 117
    assert elems >= 2**31
    assert printed["refused"]["beyond_reach"]["text"] == (
        "a 8640x2160x100 slab has %.2g elements per 3-D array (%.1f GB) and %.2g per plane; the kernels index at most 2^31 elements per "
        "array and 23 planes of 2 GB together: decompose in x (nranks) so that the local slab is narrower" % (elems, elems * 4 / 1e9, plane))


@pytest.mark.parametrize("N", [30, 12, 4])
def test_the_substepping_of(printed, N):
    Ns, frac, weights = substepping(N)
    got = printed["substeps"][str(N)]
    assert int(got["Ns"]) == Ns and float.fromhex(got["dtau_frac"]) == frac
    w = [float.fromhex(x) for x in got["weights"].split(",")]
    assert len(w) == Ns
    for a, b in zip(w, weights):
        assert abs(a - b) <= math.ulp(b), (N, a, b)
    assert abs(sum(w) - 1.0) <= Ns * math.ulp(1.0), sum(w)


def test_the_known_substep_counts(printed):
    assert {N: int(printed["substeps"][N]["Ns"]) for N in ("30", "12", "4")} == {"30": 21, "12": 8, "4": 2}


@pytest.mark.parametrize("name", SHAPED)
def test_the_shape_of_every_field_on(printed, name):
    assert printed["fields"] == len(FIELDS)
    c = dict(BASE, **LAYOUTS[name][0])
    Ry = max(1, c["ranks_y"])
    Nx, Ny, Nz, H = c["Nx"] // (c["nranks"] // Ry), c["Ny"] // Ry, c["Nz"], c["halo"]
    # gb25_field_dims dropped the row of a y-face field where the grid folds or a neighbour rank lies to the north
    drops = c["grid_type"] >= TRIPOLAR or c["rank"] // (c["nranks"] // Ry) < Ry - 1
    assert drops == (name != "walled")
    for id, f in enumerate(FIELDS):
        got = printed["shape"][(name, id)]
        v, flat, faces = f in V_SHAPED, f in FLAT, f in Z_FACES
        parent = (Nx + 2 * H, Ny + 2 * H + (1 if v else 0), 1 if flat else Nz + 2 * H + (1 if faces else 0))
        with_halos = (parent[0], parent[1] - (1 if v and drops else 0), parent[2])
        without = (with_halos[0] - 2 * H, with_halos[1] - 2 * H, 1 if flat else with_halos[2] - 2 * H)
        want = dict(parent=parent, interior=without, with_halos=with_halos, without=without)
        assert {k: tuple(int(x) for x in got[k].split(",")) for k in want} == want, (name, f)
        assert got["flags"] == "%d%d%d" % (v, flat, f in CATKE), (name, f)
        # (the state dump: global rows Ny, + 1 for a y-face field of a grid with a northern wall)
        assert int(got["global_rows"]) == c["Ny"] + (1 if v and c["grid_type"] < TRIPOLAR else 0), (name, f)


def test_a_few_shapes_by_hand(printed):
    shape = lambda name, f, k: tuple(int(x) for x in printed["shape"][(name, FIELDS.index(f))][k].split(","))
    assert shape("walled", "w", "parent") == (48, 29, 15) and shape("walled", "w", "interior") == (40, 21, 7)
    assert shape("walled", "v", "parent") == (48, 30, 14) and shape("walled", "v", "interior") == (40, 22, 6)
    assert shape("walled", "kappa_c", "parent") == (48, 29, 15) and shape("walled", "Jb", "parent") == (48, 29, 1)
    assert shape("walled", "Gn.V", "parent") == (48, 30, 1) and shape("walled", "Gn.V", "interior") == (40, 22, 1)
    assert shape("folded", "v", "parent") == (48, 33, 14) and shape("folded", "v", "with_halos") == (48, 32, 14)
    assert shape("folded", "v", "interior") == (40, 24, 6) and shape("below_a_neighbour", "V", "interior") == (40, 21, 1)
    assert shape("below_a_neighbour", "previous_v", "with_halos") == (48, 29, 14)


def test_creation_and_the_option_price_a_chunking_alike(printed):
    """Float32 5760 x 2880 x 48: creation chose 12 levels per chunk; the option hook's formula (the old opt_chunk_levels: plane *
    (klen + 10) * sizeof(real) against 2^31) gives the same figures for 12, and refuses the 24 that creation turned down"""
    created = printed["layout"][REACH_GRID]
    plane, Nz = (5760 + 16) * (2880 + 16 + 1), 48
    for levels in REACH_LEVELS:
        kchunks = max(1, Nz // levels)
        klen = (Nz + kchunks - 1) // kchunks
        nbytes = plane * (klen + 10) * 4
        got = printed["reach"][(REACH_GRID, levels)]
        assert (int(got["klen"]), int(got["planes"]), int(got["bytes"]), got["ok"]) == (klen, klen + 10, nbytes, str(int(nbytes < 2**31))), levels
    as_option = printed["reach"][(REACH_GRID, int(created["chunk_levels"]))]
    assert {k: as_option[k] for k in ("ok", "klen", "planes", "bytes")} == {k: created[k] for k in ("ok", "klen", "planes", "bytes")}
    assert printed["reach"][(REACH_GRID, 24)]["ok"] == "0" and printed["reach"][(REACH_GRID, 12)]["ok"] == "1"
