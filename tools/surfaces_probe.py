#!/usr/bin/env python3
"""Where the isopycnals lie: steps the baroclinic-instability model a few steps and prints, per row, the zonal-mean depth of a
handful of isopycnals (gb.isosurface_depth: searched on the device, one 2-D array per surface crosses PCIe), the counts of the
status bytes, and the time per call.  With --time: the time per call for 1, 8 and 64 isopycnals, for their depth and for T on
them, the bytes the kernel must read and the bandwidth that implies, against the host route for the same answer (gb25_get_field
of the parents, the potential density array and the numpy restatement on_surfaces_host), one JSON object
(profiles/surfaces_1440x720x48.json).
usage: surfaces_probe.py [--size 1440 720 48] [--steps 20] [--surfaces 5] [--rows 12] [--time] [--reps 20] [--group 16]"""
import argparse, json, os, statistics, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, nargs=3, default=[1440, 720, 48])
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--surfaces", type=int, default=5)
ap.add_argument("--rows", type=int, default=12)
ap.add_argument("--dt", type=float, default=120.0)
ap.add_argument("--time", action="store_true")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--group", type=int, default=16, help="targets per march of the library (SURF_TG of csrc/surface_kernels.hpp)")
a = ap.parse_args()
import gb25_amd as gb
import bench
from gb25_amd.surfaces import STATUS_NAMES, on_surfaces_host
Nx, Ny, Nz = a.size

m = gb.baroclinic_instability_model(gb.GPU(), Nx, Ny, Nz, dt=a.dt)
gb.set_baroclinic_instability(m)
m.set(u=(1e-3 * bench.counter_rng((Nx, Ny, Nz), 42, 1)).astype(np.float32),
      v=(1e-3 * bench.counter_rng((Nx, Ny + 1, Nz), 42, 2)).astype(np.float32))
gb.first_time_step(m)
gb.loop(m, a.steps)
b = m.backend
sigma_stats = b.derived_stats("potential_density")


def isopycnals(n):
    """n potential densities inside the range the model holds"""
    return np.linspace(sigma_stats.min, sigma_stats.max, n + 2)[1:-1]


def wall_ms(call, reps, warm=True):
    if warm:
        call()
    out = []
    for _ in range(reps):
        b.synchronize()
        t = time.perf_counter()
        call()
        out.append(1e3 * (time.perf_counter() - t))
    return {"ms_median": statistics.median(out), "ms_min": min(out), "reps": reps}


def device_ms(call, reps):
    """the library's event pair around the launch of one call"""
    b.profile_enable(True)
    for _ in range(3):
        call()
    out = []
    for _ in range(reps):
        b.profile_reset()
        call()
        out.append(b.profile_get("diagnostics")[1])
    b.profile_enable(False)
    return {"ms_median": statistics.median(out), "ms_min": min(out)}


if a.time:
    real = np.dtype(b.dtype).itemsize
    res = {"size": [Nx, Ny, Nz], "float_type": b.float_type, "targets_per_march": a.group, "calls": {}}
    for carried in ("depth", "T"):
        for n in (1, 8, 64):
            values = isopycnals(n)
            groups = -(-n // a.group)
            # every march of a group reads T and S of every interior cell once; the results go out once
            read = groups * 2 * Nx * Ny * Nz * real
            written = Nx * Ny * n * (real + 1)
            w = {"values": n, "marches": groups, "bytes_read_at_least": read, "bytes_written": written, "bytes_to_host": written}
            w["device_call_wall"] = wall_ms(lambda: b.get_on_surfaces("potential_density", carried, values), a.reps)
            w["device_kernel"] = device_ms(lambda: b.compute_on_surfaces("potential_density", carried, values), a.reps)
            w["kernel_GB_per_s_of_those_bytes"] = (read + written) / (1e6 * w["device_kernel"]["ms_median"])
            if n == 8:
                def host_route():
                    T, S = b.get_field("T", True), b.get_field("S", True)       # (the parents a user without the kernel downloads)
                    return on_surfaces_host(b, "potential_density", carried, values)
                w["get_field_plus_on_surfaces_host_wall"] = wall_ms(host_route, 1, warm=False)
            res["calls"][f"potential_density_to_{carried}_n{n}"] = w
            print(f"potential_density -> {carried}, n = {n}:", json.dumps(w), flush=True)
    print(json.dumps(res, indent=1))
    sys.exit(0)

values = isopycnals(a.surfaces)
t = time.perf_counter()
depth, status = gb.isosurface_depth(m, "potential_density", values)
ms = 1e3 * (time.perf_counter() - t)
print(f"# zonal-mean depth [m] of {a.surfaces} isopycnals of {Nx} x {Ny} x {Nz} after {m.clock.iteration} steps; first call {ms:.2f} ms")
print("# (mean over the columns where the surface was found; '-': nowhere in the row)")
print("#   row  " + " ".join(f"{v:10.3f}" for v in values))
for j in np.linspace(0, Ny - 1, a.rows).astype(int):
    cells = []
    for n in range(len(values)):
        hit = status[:, j, n] == 0
        cells.append(f"{depth[:, j, n][hit].astype(np.float64).mean():10.2f}" if hit.any() else f"{'-':>10}")
    print(f"{j:7d}  " + " ".join(cells))
counts = np.bincount(status.ravel(), minlength=4)
print("# status: " + ", ".join(f"{name} {int(c)}" for name, c in zip(STATUS_NAMES, counts)))
w = wall_ms(lambda: gb.isosurface_depth(m, "potential_density", values), a.reps)
print(f"# time per call: median {w['ms_median']:.3f} ms, min {w['ms_min']:.3f} ms over {w['reps']} calls")
