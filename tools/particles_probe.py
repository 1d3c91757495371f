"""Lagrangian particles on the device at a given size, Float32, one process: seeds --particles particles uniformly over the wet
cells, steps the model, advances the particles after every --every steps and prints their dispersion (the spread of the
displacements in cells) and the counters.  With --time: the cost of one gb25_particles_advance -- wall time per call and the
kernels' share of it from the library's HIP-event timer (slot "diagnostics": the advance launch and the fold of its counters) --
next to gb.loop alone in the same process and next to the route it replaces: get_field of u, v, w (halos included) and
advance_host, measured in the same run.  Medians over --reps calls after a warm-up, the spread reported.  The timing record is
written to profiles/particles_<Nx>x<Ny>x<Nz>.json (--out).
usage: particles_probe.py [--size 1440 720 48] [--particles 1000000] [--steps 20] [--every 2] [--substeps 1] [--time] [--reps 30]"""
import argparse, json, os, socket, statistics, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, nargs=3, default=[1440, 720, 48])
ap.add_argument("--particles", type=int, default=1000000)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--every", type=int, default=2)
ap.add_argument("--substeps", type=int, default=1)
ap.add_argument("--time", action="store_true")
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--host-reps", type=int, default=3)
ap.add_argument("--out", default=None)
a = ap.parse_args()
import gb25_amd as gb
import bench
from gb25_amd.particles import advance_host, particle_fields, particle_tables
Nx, Ny, Nz = a.size

m = gb.baroclinic_instability_model(gb.GPU(), Nx, Ny, Nz, dt=120.0)
gb.set_baroclinic_instability(m)
m.set(u=(1e-1 * bench.counter_rng((Nx, Ny, Nz), 42, 1)).astype(np.float32),
      v=(1e-1 * bench.counter_rng((Nx, Ny + 1, Nz), 42, 2)).astype(np.float32))
gb.first_time_step(m)
gb.loop(m, 5)
b = m.backend
p = gb.seed_particles(m, a.particles, seed=0)
start = p.positions()
traj = gb.run_with_particles(m, p, a.steps, every=a.every, substeps=a.substeps, fields=("T",))
end = p.positions()
dx = (end["xi"] - start["xi"] + Nx / 2) % Nx - Nx / 2
info = p.info()
res = {"size": [Nx, Ny, Nz], "float_type": "Float32", "particles": a.particles, "steps": a.steps, "every": a.every,
       "substeps": a.substeps, "host": socket.gethostname(),
       "dispersion_cells": {"x_rms": float(np.sqrt(np.mean(dx ** 2))), "y_rms": float(np.sqrt(np.mean((end["eta"] - start["eta"]) ** 2))),
                            "z_rms": float(np.sqrt(np.mean((end["zeta"] - start["zeta"]) ** 2)))},
       "T_carried": {"first_mean": float(traj["T"][0].mean()), "last_mean": float(traj["T"][-1].mean())},
       "calls": info.calls, "time_advanced_s": info.time_advanced, "counters_total": info.counters("total")}
if a.time:
    dt = b.clock()[2] * a.every

    def spread(x):
        return {"median": statistics.median(x), "min": min(x), "max": max(x)}

    for _ in range(5):
        b.particles_advance(dt, a.substeps)
    wall, kern = [], []
    b.profile_enable(True)
    for _ in range(a.reps):
        b.profile_reset()
        t = time.perf_counter()
        b.particles_advance(dt, a.substeps)
        wall.append(1e3 * (time.perf_counter() - t))
        n, ms = b.profile_get("diagnostics")
        assert n == 1
        kern.append(ms)
    b.profile_enable(False)
    loops = []
    for _ in range(5):
        b.synchronize()
        t = time.perf_counter()
        gb.loop(m, 20)
        b.synchronize()
        loops.append(1e3 * (time.perf_counter() - t) / 20)
    # the route without the kernel: three parent arrays to the host, then the numpy restatement
    tables = particle_tables(b)
    state = b.particles_get()
    down, host = [], []
    for _ in range(a.host_reps):
        t = time.perf_counter()
        fields = particle_fields(b)
        down.append(1e3 * (time.perf_counter() - t))
        t = time.perf_counter()
        advance_host(b, state, dt, a.substeps, fields, tables)
        host.append(1e3 * (time.perf_counter() - t))
    res["timing"] = {"reps": a.reps, "advance_wall_ms": spread(wall), "advance_kernels_ms": spread(kern),
                     "kernels_share_of_wall": statistics.median(kern) / statistics.median(wall),
                     "time_step_ms": spread(loops), "advance_over_time_step": statistics.median(wall) / statistics.median(loops),
                     "host_route": {"reps": a.host_reps, "download_uvw_ms": spread(down), "advance_host_ms": spread(host),
                                    "bytes": int(sum(f.size for f in fields.values()) * 4)},
                     "host_route_over_advance": (statistics.median(down) + statistics.median(host)) / statistics.median(wall)}
p.close()
text = json.dumps(res, indent=1)
print(text)
if a.time:
    out = a.out or os.path.join(ROOT, "profiles", f"particles_{Nx}x{Ny}x{Nz}.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    open(out, "w").write(text + "\n")
