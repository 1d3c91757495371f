#!/usr/bin/env python3
"""How the bench workload evolves: max |u|, |v|, |w|, |eta| and where, every `every` steps, until a field stops being finite.
usage: stability_probe.py [--size 1440 720 48] [--dt 120] [--steps 300] [--every 10] [--noise 1e-2]"""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, nargs=3, default=[1440, 720, 48])
ap.add_argument("--dt", type=float, default=120.0)
ap.add_argument("--steps", type=int, default=300)
ap.add_argument("--every", type=int, default=10)
ap.add_argument("--noise", type=float, default=None, help="replace the bench's velocity noise amplitude")
ap.add_argument("--opt", action="append", default=[])
a = ap.parse_args()
import gb25_amd as gb
import bench
Nx, Ny, Nz = a.size
m = gb.baroclinic_instability_model(gb.GPU(), Nx, Ny, Nz, dt=a.dt)
for kv in a.opt:
    k, v = kv.split("=")
    m.backend.set_option(k, int(v))
gb.set_baroclinic_instability(m)
amp = 1e-3 if a.noise is None else a.noise
m.set(u=(amp * bench.counter_rng((Nx, Ny, Nz), 42, 1)).astype(np.float32), v=(amp * bench.counter_rng((Nx, Ny + 1, Nz), 42, 2)).astype(np.float32))
gb.first_time_step(m)
done = 1
while done < a.steps:
    gb.loop(m, a.every)
    done += a.every
    line = [f"step {done:4d}"]
    bad = False
    mon = m.backend.state_monitor()      # reduced on the device: no field is downloaded, the schedule is not disturbed
    for n in ("u", "v", "w", "eta", "T"):
        s = getattr(mon, n)
        if s.nonfinite:                  # (positions 0-based [i, j, k], as the downloaded arrays were indexed)
            line.append(f"{n}: {s.nonfinite} non-finite, first at {[q - 1 for q in s.first_nonfinite]}")
            bad = True
        else:
            line.append(f"{n} max {s.max_abs:.3e} at {tuple(q - 1 for q in s.at_max_abs)}")
    print("  ".join(line), flush=True)
    if bad:
        break
