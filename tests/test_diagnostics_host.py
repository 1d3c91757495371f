"""Device diagnostics, the parts that need no GPU: the new ABI entries in header, binding and both libraries, the ctypes
mirrors of the three result structs, the host arithmetic that combines the ranks of a decomposition, and the numpy path of
compare_states (which the device path must not have changed)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import gb25_amd as gb
from gb25_amd import binding
from gb25_amd.binding import FieldDiff, FieldStats, StateMonitor
from helpers import make_oracle, set_noisy_velocities

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["gb25_field_stats_bytes", "gb25_field_diff_bytes", "gb25_state_monitor_bytes", "gb25_get_field_stats",
               "gb25_compare_field", "gb25_get_state_monitor", "gb25_field_device_ptr_readonly"]


@pytest.fixture(scope="module", params=["Float32", "Float64"])
def lib(request):
    gb.build_library()
    return binding.load_library(request.param)


def header():
    text = open(os.path.join(ROOT, "include", "gb25.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_new_entries_in_header_binding_and_library(lib):
    declared = set(re.findall(r"\b(gb25_[a-z_0-9]+)\s*\(", header()))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in binding.ABI_SYMBOLS, name
        assert hasattr(lib, name), name


def test_struct_mirrors_have_the_library_sizes(lib):
    assert lib.gb25_field_stats_bytes() == ctypes.sizeof(FieldStats)
    assert lib.gb25_field_diff_bytes() == ctypes.sizeof(FieldDiff)
    assert lib.gb25_state_monitor_bytes() == ctypes.sizeof(StateMonitor)
    assert ctypes.sizeof(StateMonitor) >= 6 * ctypes.sizeof(FieldStats)


def test_struct_members_follow_the_header():
    """Member names of the three typedefs, in order, against the ctypes mirrors."""
    text = header()
    for cname, mirror in (("gb25_field_stats", FieldStats), ("gb25_field_diff", FieldDiff), ("gb25_state_monitor", StateMonitor)):
        body = re.search(r"typedef struct \{([^}]*)\}\s*" + cname + r"\s*;", text).group(1)
        names = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                names += [re.sub(r"\[\d+\]", "", n).strip() for n in decl.split(None, 1)[1].split(",")]
        assert names == [n for n, _ in mirror._fields_], cname


def test_enums_grew_at_their_ends():
    text = header()
    metric = re.search(r"typedef enum \{([^}]*)\}\s*gb25_metric;", text).group(1)
    assert [s.strip().split()[0] for s in metric.split(",") if s.strip()][-2:] == ["GB25_M_DZF", "GB25_M_DY"]
    assert binding.METRIC_IDS["dy"] == binding.METRIC_IDS["dzf"] + 1
    kernel = re.search(r"typedef enum \{([^}]*)\}\s*gb25_kernel;", text).group(1)
    assert [s.strip().split()[0] for s in kernel.split(",") if s.strip()][-3:] == ["GB25_K_FLUXES", "GB25_K_DIAGNOSTICS", "GB25_K_COUNT"]
    assert binding.KERNEL_IDS["diagnostics"] == binding.KERNEL_IDS["fluxes"] + 1


def stats(mn, mx, amax, at, s, ss, count, offset, nonfinite=0, first=(0, 0, 0)):
    r = FieldStats()
    r.min, r.max, r.max_abs, r.sum, r.sum_sq, r.count, r.nonfinite = mn, mx, amax, s, ss, count, nonfinite
    r.at_max_abs[:], r.first_nonfinite[:], r.global_offset[:] = at, first, offset
    return r


def test_combine_stats_of_two_slabs():
    # two x slabs of 4 columns each, 3 rows, 2 levels
    a = stats(-1.0, 2.0, 2.0, (3, 2, 1), 1.5, 6.0, 24, (0, 0, 0))
    b = stats(-3.0, 0.5, 3.0, (1, 1, 2), -2.0, 10.0, 24, (4, 0, 0), nonfinite=1, first=(2, 3, 1))
    c = gb.combine_stats([a, b])
    assert (c.min, c.max, c.max_abs, c.sum, c.sum_sq, c.count, c.nonfinite) == (-3.0, 2.0, 3.0, -0.5, 16.0, 48, 1)
    assert tuple(c.at_max_abs) == (5, 1, 2) and tuple(c.first_nonfinite) == (6, 3, 1) and tuple(c.global_offset) == (0, 0, 0)
    assert gb.combine_stats([a]).as_dict() == a.as_dict()


def test_combine_stats_tie_goes_to_the_smallest_global_offset():
    # the same maximum on both slabs.  Memory order is i fastest, so the eastern slab's (1, 1, 1) = global (5, 1, 1) comes
    # BEFORE the western slab's (2, 2, 1) ...
    west = stats(0.0, 7.0, 7.0, (2, 2, 1), 0.0, 0.0, 24, (0, 0, 0))
    east = stats(0.0, 7.0, 7.0, (1, 1, 1), 0.0, 0.0, 24, (4, 0, 0))
    for order in ([west, east], [east, west]):
        assert tuple(gb.combine_stats(order).at_max_abs) == (5, 1, 1)
    # ... and after the western slab's (4, 1, 1)
    west.at_max_abs[:] = (4, 1, 1)
    for order in ([west, east], [east, west]):
        assert tuple(gb.combine_stats(order).at_max_abs) == (4, 1, 1)
    # a rank with nothing finite has no position and never wins
    empty = stats(math.inf, -math.inf, 0.0, (0, 0, 0), 0.0, 0.0, 24, (8, 0, 0), nonfinite=24, first=(1, 1, 1))
    c = gb.combine_stats([west, east, empty])
    assert tuple(c.at_max_abs) == (4, 1, 1) and c.nonfinite == 24 and tuple(c.first_nonfinite) == (9, 1, 1)
    # rows of a mesh: the southern rank's last row comes before the northern rank's first
    south, north = stats(0, 1, 1.0, (4, 3, 1), 0, 0, 12, (0, 0, 0)), stats(0, 1, 1.0, (1, 1, 1), 0, 0, 12, (0, 3, 0))
    assert tuple(gb.combine_stats([north, south]).at_max_abs) == (4, 3, 1)


def test_combine_diffs():
    def diff(ma, mb, md, at, sa, sb, sd, off, nonfinite=0):
        r = FieldDiff()
        r.max_abs_a, r.max_abs_b, r.max_abs_delta, r.sum_sq_a, r.sum_sq_b, r.sum_sq_delta = ma, mb, md, sa, sb, sd
        r.count, r.nonfinite = 10, nonfinite
        r.at_max_abs_delta[:], r.global_offset[:] = at, off
        return r
    a, b = diff(1.0, 1.5, 0.5, (2, 1, 1), 4.0, 5.0, 0.25, (0, 0, 0)), diff(2.0, 1.0, 0.5, (1, 1, 1), 1.0, 2.0, 0.5, (2, 0, 0), 3)
    c = gb.combine_diffs([b, a])
    assert (c.max_abs_a, c.max_abs_b, c.max_abs_delta, c.sum_sq_a, c.sum_sq_b, c.sum_sq_delta) == (2.0, 1.5, 0.5, 5.0, 7.0, 0.75)
    assert tuple(c.at_max_abs_delta) == (2, 1, 1) and (c.count, c.nonfinite) == (20, 3)
    from gb25_amd.correctness import diff_record
    rec = diff_record("T", c, rtol=1.0, atol=0.0)
    assert rec["ok"] is False and math.isnan(rec["rel"])          # something was not finite
    rec = diff_record("T", a, rtol=0.3, atol=0.0)
    assert rec == dict(name="T", ok=True, rel=0.5 / math.sqrt(5.0), max1=1.0, max2=1.5, maxdelta=0.5, index=(2, 1, 1))
    assert diff_record("T", a, rtol=0.2, atol=0.0)["ok"] is False and diff_record("T", a, rtol=0.0, atol=0.5)["ok"] is True


def test_state_monitor_line():
    mon = StateMonitor()
    mon.iteration, mon.time, mon.cfl, mon.nonfinite_total = 40, 4800.0, 2.5e-4, 3
    mon.u.max_abs, mon.T.min, mon.T.max = 0.125, 1.5, 29.25
    line = str(mon)
    assert "\n" not in line and line.startswith("iter: 40, time: 4800 s")
    for piece in ("1.25e-01", "extrema(T): (1.500, 29.250)", "extrema(S)", "max|eta|", "2.500e-04", "non-finite: 3"):
        assert piece in line, (piece, line)


def test_host_path_of_compare_states_is_the_definition():
    """compare_states(on_device=False) on two oracle models: every record recomputed here from the definitions in
    correctness.py's docstring (isapprox's norm test, max|psi|, max|delta| and its 1-based index)."""
    m1, m2 = make_oracle(32, 16, 6, dt=600.0), make_oracle(32, 16, 6, dt=600.0)
    for m, seed in ((m1, 42), (m2, 43)):
        gb.set_baroclinic_instability(m)
        set_noisy_velocities(m, seed=seed)
        gb.first_time_step(m)
        gb.loop(m, 2)
    rtol = 1e-3
    ok, report = gb.compare_states(m1, m2, rtol=rtol, verbose=False, on_device=False)
    ok_default, report_default = gb.compare_states(m1, m2, rtol=rtol, verbose=False)
    assert (ok_default, report_default) == (ok, report)            # (no HIP model: the default is the host path)
    by_name = {r["name"]: r for r in report}
    assert list(by_name) == ["u", "Gn.u", "Gm.u", "v", "Gn.v", "Gm.v", "w", "eta", "T", "Gn.T", "Gm.T", "S", "Gn.S", "Gm.S",
                             "filtered.U", "filtered.V", "filtered.eta"]
    pairs = {"u": (m1.velocities.u, m2.velocities.u), "w": (m1.velocities.w, m2.velocities.w),
             "T": (m1.tracers.T, m2.tracers.T), "Gn.v": (m1.timestepper.Gn.v, m2.timestepper.Gn.v),
             "filtered.eta": (m1.free_surface.filtered_state.eta, m2.free_surface.filtered_state.eta)}
    all_ok = True
    for name, (f1, f2) in pairs.items():
        a, b = f1.interior.astype(np.float64), f2.interior.astype(np.float64)
        d = np.abs(a - b)
        dn, nn = math.sqrt(float((d * d).sum())), max(math.sqrt(float((a * a).sum())), math.sqrt(float((b * b).sum())))
        r = by_name[name]
        assert r["max1"] == np.abs(a).max() and r["max2"] == np.abs(b).max() and r["maxdelta"] == d.max(), name
        assert d[tuple(i - 1 for i in r["index"])] == d.max(), name
        assert r["ok"] == (dn <= rtol * nn), name
        assert r["rel"] == pytest.approx(dn / nn if nn > 0 else 0.0, rel=1e-12), name
        all_ok &= r["ok"]
    assert ok == all(r["ok"] for r in report) and (not all_ok) <= (not ok)
    assert by_name["u"]["ok"] is False and by_name["T"]["ok"] is True      # different noise in u; T barely moved in 3 steps
    with pytest.raises(TypeError):
        gb.compare_states(m1, m2, on_device=True)
