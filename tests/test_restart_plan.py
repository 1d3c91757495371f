"""The restart set (csrc/restart_plan.hpp) as a host-only harness: a small main includes the header alone and prints, for each
configuration below, the member table and the pieces under a cap; the expectations are written out here.  No GPU, no library.

A rank of a decomposition has the members of a single domain with its own parent dims: the sub-cycle's widened arrays are work
arrays, filled anew every step, and what the sub-cycle made ahead of time lies in the partners of eta, U, V (ahead.*)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE = 5   # GB25_ERR_STATE

MAIN = r"""
#include "gb-25_amd/csrc/restart_plan.hpp"
#include <cstdlib>
int main(int argc, char** argv) {
  // Nx Ny Nz halo substeps rank nranks slab_mode grid_type ranks_y real_bytes catke phy top_flux_mask cap lookaheads
  gb25_config c{};
  int a = 1;
  c.Nx = atoi(argv[a++]); c.Ny = atoi(argv[a++]); c.Nz = atoi(argv[a++]); c.halo = atoi(argv[a++]); c.substeps = atoi(argv[a++]);
  c.rank = atoi(argv[a++]); c.nranks = atoi(argv[a++]); c.slab_mode = atoi(argv[a++]); c.grid_type = atoi(argv[a++]); c.ranks_y = atoi(argv[a++]);
  const int real_bytes = atoi(argv[a++]);
  RestartSwitches sw;
  sw.catke = atoi(argv[a++]); sw.phy_stored = atoi(argv[a++]);
  const int mask = atoi(argv[a++]);
  for (int q = 0; q < 4; q++) sw.top_flux[q] = (mask >> q) & 1;
  const unsigned long long cap = strtoull(argv[a++], nullptr, 10);
  sw.ahead_ts = sw.ahead_uv = sw.ahead_baro = sw.colsums = atoi(argv[a++]) != 0;
  const LayoutPlan lp = plan_layout(c, real_bytes, nullptr);
  if (lp.status) { printf("layout refused %d\n", (int)lp.status); return 0; }
  const RestartPlan p = plan_restart(lp.layout, sw, real_bytes);
  if (p.status) { printf("refused %d %s\n", (int)p.status, p.refusal.c_str()); return 0; }
  printf("arena %llu\n", (unsigned long long)p.arena_bytes);
  for (const RestartMember& m : p.members) {
    const Dims d = m.field >= 0 ? parent_dims(lp.layout, m.field) : m.dims;
    printf("member %s %d %d %d %d %d %d %llu %llu %d %d\n", m.name.c_str(), m.field, m.extra, m.dims.nx, m.dims.ny, m.dims.nz, m.elem_bytes,
           (unsigned long long)m.offset, (unsigned long long)m.bytes, d.nx * d.ny, m.field >= 0 ? d.nz : m.dims.nz);
  }
  const auto pieces = restart_pieces(p, cap);
  for (size_t q = 0; q < pieces.size(); q++)
    for (const RestartSpan& s : pieces[q])
      printf("span %zu %d %llu %llu %llu\n", q, s.member, (unsigned long long)s.begin, (unsigned long long)s.bytes, (unsigned long long)s.arena_offset);
  return 0;
}
"""

BASE_NAMES = ["u", "v", "w", "T", "S", "pHY", "Gn.u", "Gn.v", "Gn.T", "Gn.S", "Gm.u", "Gm.v", "Gm.T", "Gm.S", "eta", "U", "V", "eta_bar",
              "U_bar", "V_bar", "Gn.U", "Gn.V"]
CATKE_NAMES = ["e", "Gn.e", "Gm.e", "kappa_u", "kappa_c", "kappa_e", "Le", "Jb", "previous_u", "previous_v"]
NO_PHY = [n for n in BASE_NAMES if n != "pHY"]
# what was made ahead of time and is valid: the partners of T, S; of u, v, G.U, G.V, the column integrals and the partial sums; of
# eta, U, V and the filtered state; and the column integrals of the u, v in memory
AHEAD_NAMES = ["ahead.T", "ahead.S", "ahead.u", "ahead.v", "ahead.Gn.U", "ahead.Gn.V", "ahead.colsum.U", "ahead.colsum.V", "ahead.partials",
               "ahead.eta", "ahead.U", "ahead.V", "ahead.eta_bar", "ahead.U_bar", "ahead.V_bar", "colsum.U", "colsum.V"]
V_SHAPED = {"v", "Gn.v", "Gm.v", "V", "V_bar", "Gn.V", "previous_v", "top_flux.v", "ahead.v", "ahead.Gn.V", "ahead.colsum.V", "ahead.V",
            "ahead.V_bar", "colsum.V"}
FLAT = {"eta", "U", "V", "eta_bar", "U_bar", "V_bar", "Gn.U", "Gn.V", "Jb", "top_flux.u", "top_flux.v", "top_flux.T", "top_flux.S",
        "ahead.Gn.U", "ahead.Gn.V", "ahead.colsum.U", "ahead.colsum.V", "ahead.eta", "ahead.U", "ahead.V", "ahead.eta_bar", "ahead.U_bar",
        "ahead.V_bar", "colsum.U", "colsum.V"}
Z_FACES = {"w", "kappa_u", "kappa_c", "kappa_e"}

# name: (config, switches, the member list written out)
BASE = dict(Nx=64, Ny=32, Nz=8, halo=8, substeps=30, rank=0, nranks=1, slab_mode=0, grid_type=0, ranks_y=1, real_bytes=4)
CASES = {
    "flat": (dict(), dict(catke=0, phy=1, mask=0), BASE_NAMES),
    "flat_stale_pressure": (dict(), dict(catke=0, phy=0, mask=0), NO_PHY),
    "flat_float64": (dict(real_bytes=8), dict(catke=0, phy=1, mask=0), BASE_NAMES),
    "immersed": (dict(Nx=48, Ny=24, Nz=6, grid_type=1), dict(catke=0, phy=0, mask=0), NO_PHY),
    "tripolar": (dict(Nx=48, Ny=24, Nz=6, grid_type=4, substeps=10), dict(catke=0, phy=0, mask=0), NO_PHY),
    "catke": (dict(), dict(catke=1, phy=0, mask=0), NO_PHY + CATKE_NAMES),
    "coupled": (dict(Nx=48, Ny=24, Nz=6), dict(catke=0, phy=0, mask=15),
                NO_PHY + ["top_flux.u", "top_flux.v", "top_flux.T", "top_flux.S"]),
    "heat_flux_only": (dict(), dict(catke=0, phy=1, mask=4), BASE_NAMES + ["top_flux.T"]),
    "flat_with_lookaheads": (dict(), dict(catke=0, phy=0, mask=0, ahead=1), NO_PHY + AHEAD_NAMES),
    # ranks of a decomposition (local: 64 x 32 columns and rows of the two slabs, 64 x 32 of the 2 x 2 mesh)
    "two_slabs_rank1": (dict(Nx=128, nranks=2, rank=1, substeps=10), dict(catke=0, phy=0, mask=0, ahead=1), NO_PHY + AHEAD_NAMES),
    "mesh_2x2_rank3": (dict(Nx=128, Ny=64, nranks=4, ranks_y=2, rank=3, substeps=10), dict(catke=0, phy=0, mask=0, ahead=1),
                       NO_PHY + AHEAD_NAMES),
    "mesh_2x2_rank0_catke": (dict(Nx=128, Ny=64, nranks=4, ranks_y=2, rank=0, substeps=10), dict(catke=1, phy=1, mask=0),
                             BASE_NAMES + CATKE_NAMES),
    "self_ring": (dict(Nx=128, slab_mode=1, substeps=10), dict(catke=0, phy=0, mask=0), NO_PHY),
}


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("restart_plan")
    src = d / "main.cpp"
    src.write_text(MAIN)
    exe = d / "plan"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", "-I", ROOT, str(src), "-o", str(exe)], check=True)

    def run(cfg, sw, cap=0):
        c = dict(BASE, **cfg)
        args = [c[k] for k in ("Nx", "Ny", "Nz", "halo", "substeps", "rank", "nranks", "slab_mode", "grid_type", "ranks_y", "real_bytes")]
        args += [sw["catke"], sw["phy"], sw["mask"], cap, sw.get("ahead", 0)]
        out = subprocess.run([str(exe)] + [str(x) for x in args], check=True, capture_output=True, text=True).stdout.splitlines()
        return out
    return run


def parse(lines):
    members, spans = [], []
    for ln in lines:
        w = ln.split()
        if w[0] == "member":
            members.append(dict(name=w[1], field=int(w[2]), extra=int(w[3]), dims=tuple(map(int, w[4:7])), eb=int(w[7]), offset=int(w[8]),
                                bytes=int(w[9]), plane=int(w[10]), levels=int(w[11])))
        elif w[0] == "span":
            spans.append(dict(piece=int(w[1]), member=int(w[2]), begin=int(w[3]), bytes=int(w[4]), at=int(w[5])))
    return members, spans


def expected_dims(name, c):
    """Parent dims of the LOCAL slab: Nx / Rx columns, Ny / ranks_y rows, the halos, the row of a y-face field, the level of a z-face one."""
    H = c["halo"]
    nx = c["Nx"] // (c["nranks"] // c["ranks_y"]) + 2 * H
    ny = c["Ny"] // c["ranks_y"] + 2 * H + (1 if name in V_SHAPED else 0)
    if name == "ahead.partials":   # four partial sums per (chunk of 6 levels, column of a y-face plane)
        return (4 * max(1, c["Nz"] // 6) * nx * (c["Ny"] // c["ranks_y"] + 2 * H + 1), 1, 1)
    nz = 1 if name in FLAT else c["Nz"] + 2 * H + (1 if name in Z_FACES else 0)
    return (nx, ny, nz)


@pytest.mark.parametrize("case", sorted(CASES))
def test_member_table(harness, case):
    cfg, sw, names = CASES[case]
    c = dict(BASE, **cfg)
    lines = harness(cfg, sw)
    members, spans = parse(lines)
    assert [m["name"] for m in members] == names
    end = 0
    for m in members:
        # parent dims as the layout states them (restated here: x and y with halos, the row of a y-face field, the level of a z-face one)
        assert m["dims"] == expected_dims(m["name"], c), m
        assert m["plane"] * m["levels"] == m["dims"][0] * m["dims"][1] * m["dims"][2]
        assert m["eb"] == c["real_bytes"] and m["bytes"] == m["dims"][0] * m["dims"][1] * m["dims"][2] * c["real_bytes"]
        assert m["offset"] % 16 == 0 and m["offset"] >= end, m   # aligned, behind the member before it: no overlap
        end = m["offset"] + m["bytes"]
        assert (m["field"] >= 0) != (m["extra"] >= 0)
    assert int(lines[0].split()[1]) == (end + 15) // 16 * 16
    # without a cap: one piece, every member whole at its own offset
    assert [(s["piece"], s["member"], s["begin"], s["bytes"], s["at"]) for s in spans] == \
           [(0, q, 0, m["bytes"], m["offset"]) for q, m in enumerate(members)]


@pytest.mark.parametrize("case, cap", [(c, k) for c in ("flat", "catke", "coupled", "flat_float64", "two_slabs_rank1", "mesh_2x2_rank3")
                                       for k in ("below_largest_member", "no_multiple_of_a_member")] + [("flat", "sixteen")])
def test_pieces_cover_every_byte_once(harness, case, cap):
    cfg, sw, _ = CASES[case]
    members, _ = parse(harness(cfg, sw))
    largest = max(m["bytes"] for m in members)
    # (the flat 2-D members are 80 x 48 x 4 = 15360 bytes: 100000 is a multiple of none of the members)
    cap_bytes = {"below_largest_member": largest // 3 // 16 * 16, "no_multiple_of_a_member": 100000, "sixteen": 16}[cap]
    _, spans = parse(harness(cfg, sw, cap_bytes))
    cap16 = max(16, cap_bytes // 16 * 16)
    assert max(s["piece"] for s in spans) >= 1
    covered = {q: 0 for q in range(len(members))}
    last_piece, used = 0, 0
    for s in spans:
        assert s["begin"] == covered[s["member"]], "in order, no gap, no overlap"
        covered[s["member"]] += s["bytes"]
        assert s["begin"] % 16 == 0 and s["at"] % 16 == 0 and s["bytes"] > 0
        if s["piece"] != last_piece:
            assert s["piece"] == last_piece + 1
            last_piece, used = s["piece"], 0
        assert s["at"] >= used and s["at"] + s["bytes"] <= cap16, "spans of a piece do not overlap and stay inside the arena"
        used = s["at"] + s["bytes"]
    assert covered == {q: m["bytes"] for q, m in enumerate(members)}
