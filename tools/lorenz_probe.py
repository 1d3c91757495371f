#!/usr/bin/env python3
"""The Lorenz energy cycle of a stepped baroclinic-instability model from the device-side zonal-mean and eddy statistics
(gb25_get_zonal_eddy, gb.lorenz_cycle): every --every steps the four reservoirs K_M, K_E, P_M, P_E [m^5 s^-2] and the three
conversions C(P_M -> P_E), C(P_E -> K_E), C(K_E -> K_M) [m^5 s^-3].  With --time: the kernel time (the built-in
GB25_K_DIAGNOSTICS timer) and the call time of one gb25_get_zonal_eddy over all levels, medians of --reps calls after --warmup,
beside, in the same process, gb25_get_budget and the five single-field gb25_integrate_field(..., ROWS) calls a user would
otherwise combine (first moments only), and the bytes the call must read; one JSON object (profiles/zonal_eddy_1440x720x48.json).
usage: lorenz_probe.py [--size 1440 720 48] [--dt 120] [--steps 100] [--every 20] [--time] [--reps 30] [--warmup 5] [--json PATH]"""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, nargs=3, default=[1440, 720, 48])
ap.add_argument("--dt", type=float, default=120.0)
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--every", type=int, default=20)
ap.add_argument("--float-type", default="Float32")
ap.add_argument("--time", action="store_true")
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--json", default=None)
a = ap.parse_args()
import gb25_amd as gb
import bench
Nx, Ny, Nz = a.size
m = gb.baroclinic_instability_model(gb.GPU(float_type=a.float_type), Nx, Ny, Nz, dt=a.dt)
b = m.backend
gb.set_baroclinic_instability(m)
m.set(u=(1e-3 * bench.counter_rng((Nx, Ny, Nz), 42, 1)).astype(b.dtype), v=(1e-3 * bench.counter_rng((Nx, Ny + 1, Nz), 42, 2)).astype(b.dtype))
gb.first_time_step(m)
NAMES = ("K_M", "K_E", "P_M", "P_E", "C_PM_PE", "C_PE_KE", "C_KE_KM")
res = {"size": [Nx, Ny, Nz], "float_type": a.float_type, "dt": a.dt, "cycle": []}
done = 1
while True:
    c = gb.lorenz_cycle(m)["total"]
    res["cycle"].append(dict(c, step=done))
    print(f"step {done:5d}: " + "  ".join(f"{n} {c[n]:.6e}" for n in NAMES), flush=True)
    if done >= a.steps:
        break
    n = min(a.every, a.steps - done)
    gb.loop(m, n)
    done += n


def timed(call):
    """medians of the GB25_K_DIAGNOSTICS timer and of the wall clock over --reps calls after --warmup"""
    for _ in range(a.warmup):
        call()
    kernel, wall = [], []
    b.profile_enable(True)
    for _ in range(a.reps):
        b.profile_reset()
        t = time.perf_counter()
        call()
        wall.append(1e3 * (time.perf_counter() - t))
        kernel.append(b.profile_get("diagnostics")[1])
    b.profile_enable(False)
    return {"kernel_ms_median": statistics.median(kernel), "kernel_ms_min": min(kernel), "call_ms_median": statistics.median(wall),
            "reps": a.reps, "warmup": a.warmup}


if a.time:
    rb = np.dtype(b.dtype).itemsize
    cells = Nx * Ny * Nz
    # what a call must read once: u, v, w, T, S over the lines, plus v's extra row and w's extra level
    nbytes = rb * (5 * cells + Nx * Nz + Nx * Ny)
    ze = timed(lambda: b.zonal_eddy())
    ze.update(bytes=nbytes, GB_per_s=nbytes / (1e6 * ze["kernel_ms_median"]))
    budget = timed(lambda: b.budget())
    rows = timed(lambda: [b.integrate_field(n, "rows") for n in ("u", "v", "w", "T", "S")])
    step = []
    for _ in range(5):
        b.synchronize()
        t = time.perf_counter()
        gb.loop(m, 10)
        b.synchronize()
        step.append(1e2 * (time.perf_counter() - t))
    res["timing"] = {"zonal_eddy_all_levels": ze, "budget": budget, "five_integrate_field_rows": rows,
                     "model_step_ms_median": statistics.median(step),
                     "zonal_eddy_over_budget": ze["kernel_ms_median"] / budget["kernel_ms_median"],
                     "zonal_eddy_over_five_rows": ze["kernel_ms_median"] / rows["kernel_ms_median"],
                     "zonal_eddy_over_model_step": ze["kernel_ms_median"] / statistics.median(step)}
    for k, v in res["timing"].items():
        print(f"{k}:", json.dumps(v), flush=True)
if a.json:
    with open(a.json, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
