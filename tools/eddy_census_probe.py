#!/usr/bin/env python3
"""The eddy census of a stepped model, labelled and measured where the fields live (gb25_get_regions): the vortex cores of one
level by the Okubo-Weiss criterion W < -factor sigma_W (sigma_W of that level) -- their count, their total area, the share of the level they cover and
the distribution of their sizes in cells.  With --time, medians of --reps: the census as a call (records and infos alone cross
PCIe) and as kernels (the built-in GB25_K_DIAGNOSTICS timer), beside the two routes the library had before -- gb25_get_kinematics
of that plane alone, and that call plus regions.label_host / region_records_host on the host --, and the all-foreground plane
(one region whose record wave marches the whole level: the worst case); one JSON object (profiles/regions_1440x720x48.json).
usage: eddy_census_probe.py [--size 1440 720 48] [--dt 120] [--steps 200] [--level K] [--factor 0.2] [--time] [--reps 5] [--json PATH]"""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, nargs=3, default=[1440, 720, 48])
ap.add_argument("--dt", type=float, default=120.0)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--level", type=int, default=None)
ap.add_argument("--factor", type=float, default=0.2)
ap.add_argument("--float-type", default="Float32")
ap.add_argument("--time", action="store_true")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--json", default=None)
a = ap.parse_args()
import gb25_amd as gb
import bench
from gb25_amd.integrals import cell_measure
from gb25_amd.regions import label_host, okubo_weiss_threshold, region_records_host, foreground
Nx, Ny, Nz = a.size
m = gb.baroclinic_instability_model(gb.GPU(float_type=a.float_type), Nx, Ny, Nz, dt=a.dt)
b = m.backend
gb.set_baroclinic_instability(m)
m.set(u=(1e-3 * bench.counter_rng((Nx, Ny, Nz), 42, 1)).astype(b.dtype), v=(1e-3 * bench.counter_rng((Nx, Ny + 1, Nz), 42, 2)).astype(b.dtype))
gb.first_time_step(m)
if a.steps > 1:
    gb.loop(m, a.steps - 1)
level = Nz - 1 if a.level is None else a.level
cap = min(65536, (Nx * Ny + 1) // 2)
threshold = okubo_weiss_threshold(b, level, a.factor)
census = gb.eddy_census(m, level=level, factor=a.factor, carry="T", max_regions=cap)
rec, info = census.records, census.infos[0]
cells = np.sort(rec["cells"])[::-1]
res = {"size": [Nx, Ny, Nz], "float_type": a.float_type, "steps": a.steps, "level": level, "factor": a.factor, "threshold": threshold,
       "regions": int(info["regions"]), "foreground_cells": int(info["foreground_cells"]), "foreground_share": float(info["foreground_cells"]) / (Nx * Ny),
       "nonfinite_cells": int(info["nonfinite_cells"]), "total_measure": float(rec["measure"].sum()),
       "cells_largest": cells[:5].tolist(), "cells_median": float(np.median(cells)) if cells.size else 0.0,
       "cells_histogram": {f"<= {e}": int((cells <= e).sum()) for e in (1, 4, 16, 64, 256, 1024)}}
print(f"level {level}: W < {threshold:.3e} s^-2 in {res['foreground_cells']} cells ({100 * res['foreground_share']:.2f} % of the level), "
      f"{res['regions']} regions, total measure {res['total_measure']:.4e} m^3")
print(f"  sizes in cells: largest {res['cells_largest']}, median {res['cells_median']}, cumulative {res['cells_histogram']}")


def kernel_ms(call):
    """median and min of the GB25_K_DIAGNOSTICS timer over the launches of `call`"""
    call()
    out = []
    b.profile_enable(True)
    for _ in range(a.reps):
        b.profile_reset()
        call()
        out.append(b.profile_get("diagnostics")[1])
    b.profile_enable(False)
    return {"ms_median": statistics.median(out), "ms_min": min(out), "reps": a.reps}


def wall_ms(call, reps=None):
    reps = reps or a.reps
    call()
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        call()
        out.append(1e3 * (time.perf_counter() - t))
    return {"ms_median": statistics.median(out), "ms_min": min(out), "reps": reps}


if a.time:
    window = (level, 1)
    device = lambda: b.get_regions("okubo_weiss", "below", threshold, window, "T", cap, labels=False)
    plane = lambda: b.get_kinematics("okubo_weiss", None, window)
    mu = cell_measure(b, "T")[:, :, level]
    T = b.get_field("T", False)[:, :, level]

    def host():
        x = plane()[:, :, 0]
        mask, _ = foreground(x, mu, "below", threshold)
        lab, _ = label_host(mask, True)
        return region_records_host(x.astype(np.float64), mu, lab, T, "below", True)

    timing = {"census_call": wall_ms(device), "census_kernels": kernel_ms(device), "kinematics_kernels": kernel_ms(lambda: b.compute_kinematics("okubo_weiss", None, window)),
              "get_kinematics_call": wall_ms(plane), "host_route_call": wall_ms(host, 1 if Nx * Ny > 200000 else a.reps)}
    everything = lambda: b.get_regions("T", "above", -1.0e30, window, None, 1, labels=False)
    worst = everything()
    timing["all_foreground"] = {"regions": int(worst[2]["regions"][0]), "cells": int(worst[1][0, 0]["cells"]), "call": wall_ms(everything), "kernels": kernel_ms(everything)}
    for k, v in timing.items():
        print(f"{k}:", json.dumps(v), flush=True)
    res["timing"] = timing
if a.json:
    with open(a.json, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
