#!/usr/bin/env python3
"""What the flow is about to do: steps the baroclinic-instability model a few steps and prints, per band of rows, the zonal mean
of the Eady growth rate at the face where its global mean is largest, the first baroclinic wave speed c1, the deformation radius
L_d and the share of wet columns the grid resolves (L_d / max(dx, dy) >= 2), from the device-side stability diagnostics
(gb.eady_growth_rate, gb.baroclinic_wave_speed: csrc/stability_kernels.hpp), and the time of each call.  With --time: medians of
--reps calls of every quantity -- the wall time of the call and the library's `diagnostics` timer around the launch -- as one JSON
object (--json profiles/stability_<size>.json).  Not to be confused with stability_probe.py, which is about the TIME STEP's
stability (how large dt may be).
usage: stability_map_probe.py [--size 1440 720 48] [--steps 20] [--rows 12] [--time] [--reps 20] [--json PATH]"""
import argparse, json, os, statistics, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, nargs=3, default=[1440, 720, 48])
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--rows", type=int, default=12)
ap.add_argument("--dt", type=float, default=120.0)
ap.add_argument("--time", action="store_true")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--json", default=None)
a = ap.parse_args()
import gb25_amd as gb
import bench
from gb25_amd.binding import STABILITY_IDS
Nx, Ny, Nz = a.size

m = gb.baroclinic_instability_model(gb.GPU(), Nx, Ny, Nz, dt=a.dt)
gb.set_baroclinic_instability(m)
m.set(u=(1e-3 * bench.counter_rng((Nx, Ny, Nz), 42, 1)).astype(np.float32),
      v=(1e-3 * bench.counter_rng((Nx, Ny + 1, Nz), 42, 2)).astype(np.float32))
gb.first_time_step(m)
gb.loop(m, a.steps)
b = m.backend


def timed(call):
    b.synchronize()
    t = time.perf_counter()
    out = call()
    return out, 1e3 * (time.perf_counter() - t)


eady, t_eady = timed(lambda: gb.eady_growth_rate(m))
c1, t_c1 = timed(lambda: gb.baroclinic_wave_speed(m))
Ld, t_ld = timed(lambda: gb.deformation_radius(m))
res, t_res = timed(lambda: gb.eddy_resolution(m))
wet = c1 > 0
k_max = int(np.argmax(eady.astype(np.float64).mean(axis=(0, 1))))
print(f"{Nx}x{Ny}x{Nz} after {a.steps + 1} steps; Eady rate largest on face {k_max} (0-based, of {Nz + 1}); "
      f"calls: eady {t_eady:.2f} ms, c1 {t_c1:.2f} ms, L_d {t_ld:.2f} ms, resolution {t_res:.2f} ms")
print("  rows          Eady rate [1/day]   c1 [m/s]   L_d [km]   resolved (L_d / max(dx, dy) >= 2)")
bands = np.array_split(np.arange(Ny), min(a.rows, Ny))
for rows in bands:
    w = wet[:, rows]
    if not w.any():
        print(f"  {rows[0]:5d}-{rows[-1]:<5d}  dry")
        continue
    e = eady[:, rows, k_max].astype(np.float64)[w].mean() * 86400.0
    print(f"  {rows[0]:5d}-{rows[-1]:<5d}  {e:17.4f}   {c1[:, rows][w].mean():8.3f}   {1e-3 * Ld[:, rows][w].mean():8.1f}   "
          f"{100.0 * (res[:, rows][w] >= 2.0).mean():6.1f} %")
print(f"  all rows: c1 {c1[wet].mean():.3f} m/s, L_d {1e-3 * Ld[wet].mean():.1f} km, resolved in {100.0 * (res[wet] >= 2.0).mean():.1f} % "
      f"of {int(wet.sum())} wet columns")

if a.time:
    out = {"size": [Nx, Ny, Nz], "float_type": "Float32", "steps": a.steps + 1, "reps": a.reps, "calls": {}}
    b.profile_enable(True)
    for kind in STABILITY_IDS:
        b.get_stability(kind)
        wall, kernel = [], []
        for _ in range(a.reps):
            b.profile_reset()
            _, t = timed(lambda: b.get_stability(kind))
            wall.append(t)
            kernel.append(b.profile_get("diagnostics")[1])
        out["calls"][kind] = {"call_ms_median": statistics.median(wall), "kernel_ms_median": statistics.median(kernel),
                              "call_ms": wall, "kernel_ms": kernel}
        print(f"  {kind:12s} call {statistics.median(wall):8.3f} ms   kernel {statistics.median(kernel):8.3f} ms (medians of {a.reps})")
    b.profile_enable(False)
    text = json.dumps(out, indent=1)
    if a.json:
        with open(a.json, "w") as f:
            f.write(text + "\n")
    else:
        print(text)
b.close()
