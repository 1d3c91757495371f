"""The plan of the split-explicit sub-cycle (csrc/subcycle_plan.hpp) as a host-only harness: a small main includes the header alone,
prints the plan of each setting below, and the plans are compared with expectations written out here -- read off the branches of the
barotropic_impl this header replaced.  No GPU, no library."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# every setting starts from a single lat-lon domain of 1440 x 720, halo 8, 21 effective substeps, Float32, 256 CUs, default options,
# inside a composite step whose producers write their halo cells
BASE = dict(Nx=1440, Ny=720, H=8, W=0, Wy=0, Wys=0, slab=0, curv=0, north_fold=0, ys_open=0, yn_open=0, immersed=0, Ns=21,
            subcycle_block=5, substep_order=0, subcycle_whole=1, n_cu=256, real_bytes=4, ahead=0, own_given=0, own_five=0,
            composite=1, producers_fold=1)
# a slab of 180 columns with wide halos of 30, its own columns handed over as five pieces
SLAB = dict(Nx=180, W=30, slab=1, own_given=1, own_five=1, producers_fold=0)
CURV = dict(curv=1, immersed=1)
FOLDED = dict(CURV, north_fold=1, Wy=22, producers_fold=0)
MESH = dict(SLAB, Ny=360, Wy=22, Wys=22, ys_open=1, yn_open=1, own_given=0, own_five=0)

NOTHING_AROUND = dict(copy_state_in=0, zero_averages=0, copy_own_first=0, own_in_place=0, write_layers=0, finalize_after=0,
                      publish_after=0)
L5 = "0:5:first 5:5 10:5 15:5 20:1:last"
PER_SUBSTEP = " ".join(f"{s}:1" for s in range(21))
WIDE_BLOCKED = dict(form="Blocked", arrays="Wide", S=5, TY=17, launches=L5, copy_own_first=1, own_in_place=0, out_halo=8,
                    publish_through_eb_out=1, write_layers=0, finalize_after=0, publish_after=0, lds_bytes=0)

CASES = {
    # ---- single lat-lon domain, canonical arrays
    "latlon_block5": (dict(), dict(NOTHING_AROUND, form="Blocked", arrays="Canonical", S=5, TY=17, IMM=0, ilo=0, ihi=1440, jlo=0,
                                   jhi=720, yo=8, sx=1456, xo=8, wrap=1, top_open=0, grid="23x43", block="256x1", lds_bytes=0,
                                   launches=L5, halo_images_on_last=1, publish_through_eb_out=0, out_halo=0, out_js=0, out_jn=720)),
    "latlon_block5_outside_a_composite": (dict(composite=0), dict(form="Blocked", launches=L5, halo_images_on_last=0)),
    "latlon_block5_producers_do_not_fold": (dict(producers_fold=0), dict(form="Blocked", launches=L5, halo_images_on_last=0)),
    "latlon_block5_immersed": (dict(immersed=1), dict(form="Blocked", IMM=1, instance=4)),
    "latlon_block7": (dict(subcycle_block=7), dict(NOTHING_AROUND, form="Blocked", arrays="Canonical", S=7, TY=16, grid="23x45",
                                                   block="256x1", launches="0:7:first 7:7 14:7:last", halo_images_on_last=1,
                                                   instance=2)),
    "latlon_block3": (dict(subcycle_block=3), dict(NOTHING_AROUND, form="Blocked", arrays="Canonical", S=3, TY=16, grid="23x45",
                                                   launches="0:3:first 3:3 6:3 9:3 12:3 15:3 18:3:last", halo_images_on_last=1,
                                                   instance=0)),
    "latlon_block1": (dict(subcycle_block=1), dict(form="PerSubstep", arrays="Canonical", S=1, ORDER=0, zero_averages=1,
                                                   launches=PER_SUBSTEP, grid="23x180", block="64x4", finalize_after=1,
                                                   fin="1440x720", fin_yo=8, publish_after=0, halo_images_on_last=0,
                                                   copy_state_in=0, copy_own_first=0, instance=0)),
    # rule 1: substep_order = 1 forces one substep per launch
    "latlon_block5_order1": (dict(substep_order=1), dict(form="PerSubstep", arrays="Canonical", S=1, ORDER=1, zero_averages=1,
                                                         launches=PER_SUBSTEP, grid="23x180", block="64x4", finalize_after=1,
                                                         fin="1440x720", publish_after=0, halo_images_on_last=0, instance=1)),
    # rule 3: a sub-cycle of one launch inside its own step is not `last`
    "latlon_4_substeps": (dict(Ns=4), dict(form="Blocked", S=5, launches="0:4:first", finalize_after=1, fin="1440x720",
                                           halo_images_on_last=0, zero_averages=0, publish_after=0)),
    "latlon_4_substeps_ahead": (dict(Ns=4, ahead=1), dict(form="Blocked", S=5, launches="0:4:first:last", finalize_after=0,
                                                          halo_images_on_last=1)),
    # ---- a slab of a decomposition, wide arrays
    "slab_whole_ahead": (dict(SLAB, ahead=1), dict(form="Whole", arrays="Wide", S=21, TY=17, ilo=-29, ihi=209, jlo=0, jhi=720,
                                                   sx=240, xo=30, yo=8, wrap=0, top_open=0, grid="4x43", block="1024x1",
                                                   lds_bytes=125080, launches="0:21:first:last", write_layers=1, own_in_place=1,
                                                   copy_own_first=0, zero_averages=0, finalize_after=0, publish_after=0,
                                                   publish_through_eb_out=1, halo_images_on_last=0, out_halo=8, instance=0)),
    # rule 4: in place only for the look-ahead
    "slab_whole_in_step": (dict(SLAB), dict(form="Whole", TY=17, grid="4x43", lds_bytes=125080, launches="0:21:first:last",
                                            write_layers=1, own_in_place=0, copy_own_first=1)),
    "slab_whole_without_pieces": (dict(SLAB, own_given=0, own_five=0), dict(form="Whole", write_layers=0, own_in_place=0,
                                                                            copy_own_first=0)),
    "slab_whole_160_cus": (dict(SLAB, n_cu=160, immersed=1), dict(form="Whole", TY=24, grid="4x30", lds_bytes=139920, instance=3)),
    "slab_whole_switched_off": (dict(SLAB, subcycle_whole=0), WIDE_BLOCKED),
    "slab_20_substeps": (dict(SLAB, Ns=20), dict(WIDE_BLOCKED, launches="0:5:first 5:5 10:5 15:5:last")),
    "slab_float64": (dict(SLAB, real_bytes=8), WIDE_BLOCKED),
    "slab_too_wide": (dict(SLAB, Nx=1440), dict(WIDE_BLOCKED, ilo=-29, ihi=1469, grid="24x43")),
    "slab_block1": (dict(SLAB, subcycle_block=1), dict(form="PerSubstep", arrays="Wide", zero_averages=1, copy_own_first=1,
                                                       launches=PER_SUBSTEP, grid="4x180", finalize_after=1, fin="196x720",
                                                       fin_yo=8, publish_after=1, publish_through_eb_out=0, write_layers=0)),
    # ---- curvilinear.  Rule 2: every block > 1 means 5 substeps on 64 x 17 tiles
    "curv_block3": (dict(CURV, subcycle_block=3), dict(NOTHING_AROUND, form="BlockedCurv", arrays="Canonical", S=5, TY=17,
                                                       grid="23x43", launches=L5, halo_images_on_last=0, instance=0)),
    "curv_block5": (dict(CURV), dict(NOTHING_AROUND, form="BlockedCurv", arrays="Canonical", S=5, TY=17, grid="23x43", launches=L5,
                                     halo_images_on_last=0)),
    "curv_block7": (dict(CURV, subcycle_block=7), dict(NOTHING_AROUND, form="BlockedCurv", arrays="Canonical", S=5, TY=17,
                                                       grid="23x43", launches=L5, halo_images_on_last=0)),
    "curv_block1": (dict(CURV, subcycle_block=1), dict(form="PerSubstepCurv", arrays="Canonical", zero_averages=1, grid="23x180",
                                                       launches=PER_SUBSTEP, finalize_after=1, publish_after=0)),
    # ---- a single folded domain: tall arrays, the rows of the grid count the open top
    "folded_block5": (dict(FOLDED), dict(form="BlockedCurv", arrays="Wide", copy_state_in=1, wrap=1, top_open=1, ilo=0, ihi=1440,
                                         jlo=0, jhi=742, sx=1440, xo=0, yo=8, grid="23x44", launches=L5, publish_through_eb_out=1,
                                         copy_own_first=0, zero_averages=0, finalize_after=0, publish_after=0,
                                         halo_images_on_last=0, out_halo=0, out_js=0, out_jn=720)),
    "folded_block1": (dict(FOLDED, subcycle_block=1), dict(form="PerSubstepCurv", arrays="Wide", copy_state_in=1, zero_averages=1,
                                                          jhi=742, grid="23x186", finalize_after=1, fin="1440x720", fin_yo=8,
                                                          publish_after=1, publish_through_eb_out=0)),
    # ---- a rank of a 2-D decomposition with a neighbour on both sides
    "mesh_rank_open_on_both_sides": (dict(MESH), dict(arrays="Wide", jlo=-22, jhi=382, yo=30, top_open=1, out_js=-8, out_jn=368,
                                                      out_halo=8, copy_own_first=0, write_layers=0)),
    "mesh_rank_block1": (dict(MESH, subcycle_block=1), dict(form="PerSubstep", grid="4x101", finalize_after=1, fin="196x376",
                                                            fin_yo=30, publish_after=1)),
}

MAIN = r'''
#include <cstdio>
static const char* form_name(SubcycleForm f) {
  switch (f) {
    case SubcycleForm::PerSubstep: return "PerSubstep";
    case SubcycleForm::PerSubstepCurv: return "PerSubstepCurv";
    case SubcycleForm::Blocked: return "Blocked";
    case SubcycleForm::BlockedCurv: return "BlockedCurv";
    case SubcycleForm::Whole: return "Whole";
  }
  return "?";
}
static void show(const char* name, const SubcycleSetting& c) {
  const SubcyclePlan p = plan_subcycle(c);
  std::printf("%s form=%s arrays=%s S=%d TY=%d ORDER=%d IMM=%d instance=%d", name, form_name(p.form),
              p.arrays == SubcycleArrays::Wide ? "Wide" : "Canonical", p.S, p.TY, p.ORDER, (int)p.IMM, p.instance());
  std::printf(" ilo=%d ihi=%d jlo=%d jhi=%d yo=%d top_open=%d wrap=%d sx=%d xo=%d", p.ilo, p.ihi, p.jlo, p.jhi, p.yo, p.top_open, p.wrap,
              p.sx, p.xo);
  std::printf(" grid=%dx%d block=%dx%d lds_bytes=%u", p.grid_x, p.grid_y, p.block_x, p.block_y, p.lds_bytes);
  std::printf(" copy_state_in=%d zero_averages=%d copy_own_first=%d own_in_place=%d write_layers=%d halo_images_on_last=%d"
              " publish_through_eb_out=%d finalize_after=%d publish_after=%d", (int)p.copy_state_in, (int)p.zero_averages,
              (int)p.copy_own_first, (int)p.own_in_place, (int)p.write_layers, (int)p.halo_images_on_last,
              (int)p.publish_through_eb_out, (int)p.finalize_after, (int)p.publish_after);
  std::printf(" out_halo=%d out_js=%d out_jn=%d fin=%dx%d fin_yo=%d launches=", p.out_halo, p.out_js, p.out_jn, p.fin_nx, p.fin_ny,
              p.fin_yo);
  for (int i = 0; i < p.n_launches; i++) {
    const SubcycleLaunch L = p.launch(i);
    std::printf("%s%d:%d%s%s", i ? "," : "", L.s0, L.ns, L.first ? ":first" : "", L.last ? ":last" : "");
  }
  std::printf("\n");
}
int main() {
  static_assert(BT_TX == 64 && BT_NT == 256 && BT_SMAX == 24 && BW_NT == 1024 && BW_NS == 21, "the tile constants");
'''


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("subcycle_plan")
    src, exe = tmp / "plan.cpp", tmp / "plan"
    body = []
    for name, (setting, _) in CASES.items():
        c = dict(BASE, **setting)
        assert set(c) == set(BASE), name
        body.append("  {\n    SubcycleSetting c{};\n" + "".join(f"    c.{k} = {v};\n" for k, v in c.items()) + f'    show("{name}", c);\n  }}\n')
    src.write_text('#include "%s"\n' % os.path.join(ROOT, "gb-25_amd", "csrc", "subcycle_plan.hpp") + MAIN + "".join(body) + "  return 0;\n}\n")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    got = {}
    for line in out.splitlines():
        name, *pairs = line.split(" ")
        got[name] = dict(kv.split("=", 1) for kv in pairs)
    return got


@pytest.mark.parametrize("name", list(CASES))
def test_the_plan_of(plans, name):
    want = CASES[name][1]
    got = plans[name]
    assert set(want) <= set(got)
    wrong = {k: (got[k], str(v).replace(" ", ",")) for k, v in want.items() if got[k] != str(v).replace(" ", ",")}
    assert not wrong, f"{name}: (planned, expected) {wrong}"


def test_the_launches_cover_every_substep_once(plans):
    for name, p in plans.items():
        s = 0
        for launch in p["launches"].split(","):
            s0, ns = (int(x) for x in launch.split(":")[:2])
            assert s0 == s and ns >= 1, name
            s += ns
        assert s == dict(BASE, **CASES[name][0])["Ns"], name
