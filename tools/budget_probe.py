#!/usr/bin/env python3
"""The budget of a run -- volume, heat, salt, kinetic energy, the free surface's volume and potential energy, integrated on
the device (gb25_get_budget) -- and its drift relative to step 0, one JSON line every `every` steps.
usage: budget_probe.py [--size 1440 720 48] [--dt 120] [--steps 100] [--every 10] [--grid simple_lat_lon] [--float-type Float32]
       budget_probe.py --measure          cost of one gb25_get_budget against one gb25_get_state_monitor (slot "diagnostics" of the
                                          library's HIP-event timers, one process): profiles/integrals_1440x720x48.json
       budget_probe.py --eta-drift        d = |sum mu eta| / sum mu |eta| after first_time_step + loop(20), device against the CPU
                                          oracle of the same float type (tests/oracle_backend.py): profiles/integrals_eta_drift.json
A GPU job built on this runs each invocation under its own `timeout` and stops at the first failure."""
import argparse, json, math, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, nargs=3, default=[1440, 720, 48])
ap.add_argument("--dt", type=float, default=120.0)
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--every", type=int, default=10)
ap.add_argument("--grid", default="simple_lat_lon")
ap.add_argument("--float-type", default="Float32")
ap.add_argument("--noise", type=float, default=1e-3)
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--measure", action="store_true")
ap.add_argument("--eta-drift", action="store_true")
a = ap.parse_args()
import gb25_amd as gb
import bench
Nx, Ny, Nz = a.size


def model(arch, grid, size, dt, noise=1e-3):
    nx, ny, nz = size
    m = gb.baroclinic_instability_model(arch, nx, ny, nz, dt=dt, grid_type=grid)
    gb.set_baroclinic_instability(m)
    dtype = m.backend.dtype
    m.set(u=(noise * bench.counter_rng(m.velocities.u.shape, 42, 1)).astype(dtype),
          v=(noise * bench.counter_rng(m.velocities.v.shape, 42, 2)).astype(dtype))
    gb.first_time_step(m)
    return m


def drift(now, then):
    return (now - then) / abs(then) if then else now - then


if a.measure:
    m = model(gb.GPU(float_type=a.float_type), a.grid, a.size, a.dt, a.noise)
    gb.loop(m, 5)
    b = m.backend

    def device_ms(call):
        b.profile_enable(True)
        for _ in range(5):
            call()
        out = []
        for _ in range(a.reps):
            b.profile_reset()
            call()
            out.append(b.profile_get("diagnostics")[1])
        b.profile_enable(False)
        return {"device_ms_median": statistics.median(out), "device_ms_min": min(out)}

    cells = Nx * Ny * Nz
    item = np.dtype(b.dtype).itemsize
    res = {"size": a.size, "float_type": a.float_type, "grid": a.grid, "reps": a.reps,
           "budget": device_ms(b.budget), "state_monitor": device_ms(b.state_monitor),
           "integrate_field_T_total": device_ms(lambda: b.integrate_field("T", "total")),
           "integrate_field_T_rows": device_ms(lambda: b.integrate_field("T", "rows"))}
    res["budget"]["field_bytes"] = item * (4 * cells + Nx * (Ny + 1) * Nz - Nx * Ny * Nz + Nx * Ny)
    res["budget"]["TBps_median"] = res["budget"]["field_bytes"] / res["budget"]["device_ms_median"] / 1e9
    res["budget_over_state_monitor"] = res["budget"]["device_ms_median"] / res["state_monitor"]["device_ms_median"]
    print(json.dumps(res, indent=1))
elif a.eta_drift:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from oracle_backend import CPU
    from gb25_amd.integrals import cell_measure
    out = []
    for ft in ("Float32", "Float64"):
        for grid, size, dt in (("simple_lat_lon", (64, 32, 8), 600.0), ("gaussian_islands", (48, 24, 6), 60.0)):
            rec = {"float_type": ft, "grid": grid, "size": list(size), "dt": dt, "steps": "first_time_step + loop(20)"}
            for who, arch in (("device", gb.GPU(float_type=ft)), ("oracle", CPU("f32" if ft == "Float32" else "f64"))):
                m = model(arch, grid, size, dt)
                gb.loop(m, 20)
                mu = cell_measure(m.backend, "eta")
                eta = np.asarray(m.backend.get_field("eta", False), np.float64)
                num = m.backend.budget().eta.first if who == "device" else math.fsum((mu * eta).ravel())
                rec["d_" + who] = abs(num) / math.fsum((mu * np.abs(eta)).ravel())
                rec["n"] = int((mu > 0).sum())
            rec["n_eps_real"] = rec["n"] * float(np.finfo(np.float32 if ft == "Float32" else np.float64).eps)
            out.append(rec)
    print(json.dumps({"quantity": "d = |sum mu eta| / sum mu |eta| after first_time_step + loop(20) from noisy velocities; "
                                  "asserted: d_device <= 10 max(d_oracle, n eps(real))", "cases": out}, indent=1))
else:
    m = model(gb.GPU(float_type=a.float_type), a.grid, a.size, a.dt, a.noise)
    first = m.backend.budget()
    done = 1
    while True:
        bud = m.backend.budget()
        print(json.dumps({"iteration": bud.iteration, "time": bud.time, "volume": bud.volume, "heat": bud.T.first, "salt": bud.S.first,
                          "kinetic_energy": bud.kinetic_energy, "eta_volume": bud.eta.first,
                          "eta_potential_energy": bud.eta_potential_energy,
                          "nonfinite": bud.T.nonfinite + bud.S.nonfinite + bud.u.nonfinite + bud.v.nonfinite + bud.eta.nonfinite,
                          "drift": {"volume": drift(bud.volume, first.volume), "heat": drift(bud.T.first, first.T.first),
                                    "salt": drift(bud.S.first, first.S.first),
                                    "kinetic_energy": drift(bud.kinetic_energy, first.kinetic_energy),
                                    "eta_volume_over_area": bud.eta.first / bud.surface_area}}), flush=True)
        if done >= a.steps:
            break
        n = min(a.every, a.steps - done)
        gb.loop(m, n)
        done += n
