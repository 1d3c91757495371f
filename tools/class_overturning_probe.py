#!/usr/bin/env python3
"""The overturning in density classes and the water-mass census of a run, binned and reduced on the device (gb25_get_class_sums):
the extrema of psi(y, sigma) in Sv and the volume, mean temperature and mean salinity of every class.
usage: class_overturning_probe.py [--size 1440 720 48] [--dt 120] [--steps 20] [--grid simple_lat_lon] [--float-type Float32]
                                  [--variable potential_density] [--bins 64]
       class_overturning_probe.py --time   milliseconds per call for B = 64, 128, 256 and both kinds (slot "diagnostics" of the
                                           library's HIP-event timers, host wall time of the call besides), against the only way to
                                           the same numbers without the kernel -- get_field of v, T, S, the potential density, then
                                           classes.class_sums_host -- in the same process: profiles/classes_1440x720x48.json
A GPU job built on this runs each invocation under its own `timeout` and stops at the first failure."""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, nargs=3, default=[1440, 720, 48])
ap.add_argument("--dt", type=float, default=120.0)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--grid", default="simple_lat_lon")
ap.add_argument("--float-type", default="Float32")
ap.add_argument("--noise", type=float, default=1e-3)
ap.add_argument("--variable", default="potential_density")
ap.add_argument("--bins", type=int, default=64)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--host-reps", type=int, default=1)
ap.add_argument("--time", action="store_true")
a = ap.parse_args()
import gb25_amd as gb
import bench
from gb25_amd.classes import class_sums_host, class_values


def model(arch, grid, size, dt, noise=1e-3):
    nx, ny, nz = size
    m = gb.baroclinic_instability_model(arch, nx, ny, nz, dt=dt, grid_type=grid)
    gb.set_baroclinic_instability(m)
    dtype = m.backend.dtype
    m.set(u=(noise * bench.counter_rng(m.velocities.u.shape, 42, 1)).astype(dtype),
          v=(noise * bench.counter_rng(m.velocities.v.shape, 42, 2)).astype(dtype))
    gb.first_time_step(m)
    return m


def edges_of(b, variable, B):
    x = class_values(b, variable)[:, 1:-1]
    return gb.class_edges(float(np.nanmin(x)), float(np.nanmax(x)), B - 1)


m = model(gb.GPU(float_type=a.float_type), a.grid, a.size, a.dt, a.noise)
b = m.backend
if a.time:
    gb.loop(m, 5)

    def cost(call):
        b.profile_enable(True)
        for _ in range(3):
            call()
        dev, host = [], []
        for _ in range(a.reps):
            b.profile_reset()
            t0 = time.perf_counter()
            call()
            host.append(1e3 * (time.perf_counter() - t0))
            dev.append(b.profile_get("diagnostics")[1])
        b.profile_enable(False)
        return {"device_ms_median": statistics.median(dev), "device_ms_min": min(dev), "host_ms_median": statistics.median(host)}

    res = {"size": a.size, "float_type": a.float_type, "grid": a.grid, "variable": a.variable, "reps": a.reps,
           "note": "device_ms: the launches of the call (HIP events); host_ms: the whole call, its device-to-host copy included; "
                   "host_path_ms: get_field of v, T, S, the potential density, then classes.class_sums_host, wall time"}
    for B in (64, 128, 256):
        edges = edges_of(b, a.variable, B)
        for what in ("faces_y", "cells"):
            r = cost(lambda: b.class_sums(what, a.variable, edges, "cumulative"))
            wall = []
            for _ in range(a.host_reps):
                t0 = time.perf_counter()
                want = class_sums_host(b, what, a.variable, edges, "cumulative")
                wall.append(1e3 * (time.perf_counter() - t0))
            r["host_path_ms"] = min(wall)
            r["host_path_over_device_call"] = r["host_path_ms"] / r["host_ms_median"]
            r["bit_for_bit"] = bool(b.class_sums(what, a.variable, edges, "cumulative").tobytes() == want.tobytes())
            res[f"{what}_B{B}"] = r
    print(json.dumps(res, indent=1))
else:
    gb.loop(m, a.steps)
    edges = edges_of(b, a.variable, a.bins)
    psi = gb.overturning_in_classes(m, edges, a.variable) / 1e6
    j, e = np.unravel_index(np.argmax(psi), psi.shape)
    jm, em = np.unravel_index(np.argmin(psi), psi.shape)
    census = gb.water_mass_census(m, edges, a.variable)
    full = census["measure"] > 0
    print(json.dumps({"iteration": m.clock.iteration, "variable": a.variable, "edges": [float(x) for x in edges],
                      "overturning_max_Sv": float(psi[j, e]), "at_max": [int(j), int(e)],
                      "overturning_min_Sv": float(psi[jm, em]), "at_min": [int(jm), int(em)],
                      "census_volume_m3": [float(x) for x in census["measure"]],
                      "census_mean_T": [float(h / v) if v > 0 else None for h, v in zip(census["heat"], census["measure"])],
                      "census_mean_S": [float(s / v) if v > 0 else None for s, v in zip(census["salt"], census["measure"])],
                      "classes_with_water": int(full.sum()), "cells": int(census["count"].sum())}))
