"""What passive tracers cost beside a run: python tools/passive_probe.py [--size 1440 720 48] [--dyes 4] [--out profiles/passive_1440x720x48.json]

Medians of 5, HIP events of the library's own timers (gb25_profile_*: the launches of an advance are filed under "diagnostics", the
model's tracer kernel under "tracers"):
  - one advance of a set of `dyes` dyes: the one-tracer tendency kernel once per dye, then ONE k_passive_update for the set;
  - the model's own tracer tendency kernel (T and S in one launch), per tracer, for orientation;
  - wall-clock per step of gb25_loop against run_with_tracers with an empty-handed set (advance + gb25_time_step), i.e. what leaving
    the steady-state schedule costs, and the same with the advances."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

import numpy as np

import gb25_amd as gb


def median_ms(b, kernel, work, repeats=5):
    out = []
    for _ in range(repeats):
        b.profile_reset()
        work()
        b.synchronize()
        n, ms = b.profile_get(kernel)
        out.append(ms)
    return statistics.median(out), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=3, default=(1440, 720, 48))
    ap.add_argument("--dyes", type=int, default=4)
    ap.add_argument("--float-type", default="Float32")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    Nx, Ny, Nz = a.size
    from helpers import set_noisy_velocities
    m = gb.baroclinic_instability_model(gb.GPU(float_type=a.float_type), Nx, Ny, Nz, dt=60.0)
    gb.set_baroclinic_instability(m)
    set_noisy_velocities(m)
    b = m.backend
    gb.first_time_step(m)
    gb.loop(m, 4)
    tr = gb.passive_tracers(m, dye=a.dyes)
    for n in range(a.dyes):
        tr.set(n, lambda lam, phi, z, n=n: np.exp(-((phi - 10.0 * n) / 15.0) ** 2) + 0 * lam + 0 * z)
    result = dict(size=[Nx, Ny, Nz], float_type=a.float_type, dyes=a.dyes)

    def step_with_advance():
        tr.advance()
        b.time_step()

    for _ in range(3):
        step_with_advance()
    b.profile_enable(True)
    adv, all_adv = median_ms(b, "diagnostics", step_with_advance)
    result["advance_ms"] = adv
    result["advance_ms_runs"] = all_adv
    result["advance_ms_per_tracer"] = adv / a.dyes
    trc, all_trc = median_ms(b, "tracers", lambda: b.time_step())
    result["model_tracer_kernel_ms"] = trc
    result["model_tracer_kernel_ms_per_tracer"] = trc / 2
    b.profile_enable(False)
    tr.close()

    # wall clock per step: the steady-state loop, single steps, single steps with the advances
    def wall(work, steps=20, repeats=5):
        out = []
        for _ in range(repeats):
            b.synchronize()
            t0 = time.perf_counter()
            work(steps)
            b.synchronize()
            out.append((time.perf_counter() - t0) / steps * 1e3)
        return statistics.median(out)

    result["loop_ms_per_step"] = wall(lambda n: b.loop(n))
    result["time_step_ms_per_step"] = wall(lambda n: [b.time_step() for _ in range(n)])
    tr = gb.passive_tracers(m, dye=a.dyes)
    result["run_with_tracers_ms_per_step"] = wall(lambda n: gb.run_with_tracers(m, tr, n))
    tr.close()
    b.close()
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
