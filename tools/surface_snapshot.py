#!/usr/bin/env python3
"""Step a model and every N steps write surface vorticity, surface T and the mixed-layer depth as .npy -- the surface writer of
the reference's simulations/ocean_climate_simulation.jl (`indices = (:, :, Nz)`, every three days) without a parent array
crossing PCIe -- and print what each snapshot cost next to the time of a step.

usage: surface_snapshot.py [--size 1440 720 48] [--float-type Float32] [--grid-type simple_lat_lon] [--steps 40] [--every 10]
                           [--dt 60] [--threshold 0.03] [--out DIR] [--measure FILE.json]
--measure: also time every derived field over all levels and over the surface level alone (kernel time from the library's
GB25_K_DIAGNOSTICS timer, bytes the kernels read and write, achieved bytes/s) and write the record to FILE.json."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gb25_amd as gb  # noqa: E402

# bytes per cell and level, in elements of the float type: (read, written)
TRAFFIC = {"vorticity": (4, 1), "kinetic_energy": (4, 1), "density_anomaly": (2, 1), "potential_density": (2, 1)}


def timed(backend, call, repeats=5):
    """(best wall seconds, best kernel seconds from the diagnostics timer) of `call` over `repeats` runs."""
    wall, kern = [], []
    for _ in range(repeats):
        backend.synchronize()
        backend.profile_reset()
        t0 = time.perf_counter()
        call()
        wall.append(time.perf_counter() - t0)
        kern.append(backend.profile_get("diagnostics")[1] * 1e-3)
    return min(wall), min(kern)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, nargs=3, default=(1440, 720, 48))
    ap.add_argument("--float-type", default="Float32")
    ap.add_argument("--grid-type", default="simple_lat_lon")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--every", type=int, default=10)
    ap.add_argument("--dt", type=float, default=60.0)
    ap.add_argument("--threshold", type=float, default=0.03)
    ap.add_argument("--out", default="surface_snapshots")
    ap.add_argument("--measure", default=None)
    a = ap.parse_args()
    Nx, Ny, Nz = a.size
    model = gb.baroclinic_instability_model(gb.GPU(float_type=a.float_type), Nx, Ny, Nz, dt=a.dt, grid_type=a.grid_type)
    b = model.backend
    gb.set_baroclinic_instability(model)
    rng = np.random.default_rng(42)
    model.set(u=(1e-3 * rng.random(model.velocities.u.shape)).astype(b.dtype), v=(1e-3 * rng.random(model.velocities.v.shape)).astype(b.dtype))
    os.makedirs(a.out, exist_ok=True)
    gb.first_time_step(model)
    gb.loop(model, a.every)          # (warm-up: the look-aheads are in their steady state)
    b.synchronize()
    done, step_s, snaps = 0, [], []
    while done < a.steps:
        n = min(a.every, a.steps - done)
        t0 = time.perf_counter()
        gb.loop(model, n)
        b.synchronize()
        step_s.append((time.perf_counter() - t0) / n)
        done += n
        t0 = time.perf_counter()
        zeta = gb.vorticity(model, levels=(Nz - 1, 1))[:, :, 0]
        T = model.tracers.T.surface()[:, :, 0]
        mld = gb.mixed_layer_depth(model, a.threshold)
        t1 = time.perf_counter()
        it = model.clock.iteration
        for name, x in (("zeta", zeta), ("T", T), ("mld", mld)):
            np.save(os.path.join(a.out, f"{name}_{it:06d}.npy"), x)
        t2 = time.perf_counter()
        snaps.append(t1 - t0)
        print(f"iteration {it}: snapshot {1e3 * (t1 - t0):.2f} ms on the device + copies, {1e3 * (t2 - t1):.2f} ms writing .npy; "
              f"a step {1e3 * step_s[-1]:.3f} ms; max|zeta| {np.abs(zeta).max():.3e} 1/s, T {T.min():.2f} .. {T.max():.2f}, "
              f"mixed layer {mld.min():.1f} .. {mld.max():.1f} m", flush=True)
    if not a.measure:
        return
    itemsize = np.dtype(b.dtype).itemsize
    rec = {"size": [Nx, Ny, Nz], "float_type": a.float_type, "grid_type": a.grid_type, "step_ms": 1e3 * min(step_s),
           "snapshot_ms": 1e3 * min(snaps), "fields": {}}
    b.profile_enable(True)
    for name, (rd, wr) in TRAFFIC.items():
        d = b.derived_dims(name)
        for what, levels, nk in (("all_levels", None, d[2]), ("surface", (d[2] - 1, 1), 1)):
            wall_k, kern = timed(b, lambda: b.compute_derived(name, levels=levels))
            wall_g, _ = timed(b, lambda: b.get_derived(name, levels=levels))
            nbytes = d[0] * d[1] * nk * (rd + wr) * itemsize
            rec["fields"].setdefault(name, {})[what] = {"kernel_ms": 1e3 * kern, "compute_wall_ms": 1e3 * wall_k, "get_wall_ms": 1e3 * wall_g,
                                                         "bytes": nbytes, "TB_per_s": nbytes / kern / 1e12 if kern > 0 else None}
    d = b.derived_dims("mixed_layer_depth")
    wall_k, kern = timed(b, lambda: b.compute_derived("mixed_layer_depth", a.threshold))
    wall_g, _ = timed(b, lambda: b.get_derived("mixed_layer_depth", a.threshold))
    nbytes = d[0] * d[1] * (Nz * 4 + 1) * itemsize            # (T, S read and sigma written, sigma read again: at most every level)
    rec["fields"]["mixed_layer_depth"] = {"all_levels": {"kernel_ms": 1e3 * kern, "compute_wall_ms": 1e3 * wall_k, "get_wall_ms": 1e3 * wall_g,
                                                          "bytes": nbytes, "TB_per_s": nbytes / kern / 1e12 if kern > 0 else None}}
    wall_l, kern_l = timed(b, lambda: b.get_field_levels("T", Nz - 1, 1))
    wall_f, _ = timed(b, lambda: b.get_field("T", False), repeats=2)
    rec["surface_T"] = {"get_field_levels_wall_ms": 1e3 * wall_l, "gather_kernel_ms": 1e3 * kern_l, "get_field_whole_interior_wall_ms": 1e3 * wall_f}
    b.profile_enable(False)
    with open(a.measure, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
