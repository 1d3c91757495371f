#!/usr/bin/env python3
"""The transports of a run, reduced on the device (gb25_get_transport): the extrema of the meridional overturning streamfunction
in Sv and the meridional heat transport by row.
usage: transport_probe.py [--size 1440 720 48] [--dt 120] [--steps 20] [--grid simple_lat_lon] [--float-type Float32]
       transport_probe.py --time          cost of every direction and shape against one gb25_get_budget (slot "diagnostics" of the
                                          library's HIP-event timers, host wall time of the call besides) and against downloading
                                          v, T, S, one process: profiles/transports_1440x720x48.json
       transport_probe.py --closure       the residual of the continuity equation closed with the device's y-face transports against
                                          the CPU oracle's of the same float type (tests/oracle_backend.py):
                                          profiles/transports_closure.json
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
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--time", action="store_true")
ap.add_argument("--closure", action="store_true")
a = ap.parse_args()
import gb25_amd as gb
import bench


def model(arch, grid, size, dt, noise=1e-3):
    nx, ny, nz = size
    m = gb.baroclinic_instability_model(arch, nx, ny, nz, dt=dt, grid_type=grid)
    gb.set_baroclinic_instability(m)
    dtype = m.backend.dtype
    m.set(u=(noise * bench.counter_rng(m.velocities.u.shape, 42, 1)).astype(dtype),
          v=(noise * bench.counter_rng(m.velocities.v.shape, 42, 2)).astype(dtype))
    gb.first_time_step(m)
    return m


if a.time:
    m = model(gb.GPU(float_type=a.float_type), a.grid, a.size, a.dt, a.noise)
    gb.loop(m, 5)
    b = m.backend

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

    Nx, Ny, Nz = a.size
    item = np.dtype(b.dtype).itemsize
    res = {"size": a.size, "float_type": a.float_type, "grid": a.grid, "reps": a.reps,
           "note": "device_ms: the launches of the call (HIP events); host_ms: the whole call, its device-to-host copy included",
           "budget": cost(b.budget)}
    for faces in ("across_y", "across_x"):
        for shape in ("lines", "profile", "streamfunction"):
            res[f"{faces}_{shape}"] = cost(lambda: b.transport(faces, shape))
    # an ESTIMATE of the bytes a kernel reads: the interior of its velocity once and of T and S twice (y faces: rows j - 1 and j;
    # x faces: columns i - 1 and i), halo cells, tables and whatever the caches save not counted
    for faces, name in (("across_y", "v"), ("across_x", "u")):
        r = res[f"{faces}_lines"]
        r["bytes_read_estimate"] = item * (int(np.prod(b.field_dims(name, False))) + 4 * Nx * Ny * Nz)
        r["TBps_median_estimate"] = r["bytes_read_estimate"] / r["device_ms_median"] / 1e9

    def download():
        for name in ("v", "T", "S"):
            b.get_field(name, True)

    host = []
    for _ in range(5):
        t0 = time.perf_counter()
        download()
        host.append(1e3 * (time.perf_counter() - t0))
    res["download_v_T_S"] = {"host_ms_median": statistics.median(host), "host_ms_min": min(host)}
    for faces in ("across_y", "across_x"):
        res[f"{faces}_lines_over_budget"] = res[f"{faces}_lines"]["device_ms_median"] / res["budget"]["device_ms_median"]
        res[f"{faces}_lines_host_over_download"] = res[f"{faces}_lines"]["host_ms_median"] / res["download_v_T_S"]["host_ms_median"]
    print(json.dumps(res, indent=1))
elif a.closure:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from oracle_backend import CPU
    from gb25_amd.transports import continuity_closure
    out = []
    for ft in ("Float32", "Float64"):
        for grid, size, dt in (("simple_lat_lon", (64, 32, 8), 600.0), ("gaussian_islands", (48, 24, 6), 60.0)):
            rec = {"float_type": ft, "grid": grid, "size": list(size), "dt": dt, "steps": "first_time_step + loop(3)"}
            for who, arch in (("device", gb.GPU(float_type=ft)), ("oracle", CPU("f32" if ft == "Float32" else "f64"))):
                m = model(arch, grid, size, dt)
                gb.loop(m, 3)
                lines = m.backend.transport("across_y", "lines") if who == "device" else None
                rec["r_" + who] = continuity_closure(m.backend, lines)
            rec["eps_real"] = float(np.finfo(np.float32 if ft == "Float32" else np.float64).eps)
            out.append(rec)
    print(json.dumps({"quantity": "r = max over the rows of cells of |sum_i Az (w(k+1) - w(k)) + (V[j+1,k] - V[j,k])| / (sum|q_south| + "
                                  "sum|q_north| + sum|q_u|), V = the y-face LINES' volume; asserted: r_device <= 10 max(r_oracle, eps(real))",
                      "cases": out}, indent=1))
else:
    m = model(gb.GPU(float_type=a.float_type), a.grid, a.size, a.dt, a.noise)
    gb.loop(m, a.steps)
    psi = gb.overturning(m) / 1e6
    heat = gb.heat_transport(m)
    j, k = np.unravel_index(np.argmax(psi), psi.shape)
    jm, km = np.unravel_index(np.argmin(psi), psi.shape)
    print(json.dumps({"iteration": m.clock.iteration, "overturning_max_Sv": float(psi[j, k]), "at_max": [int(j), int(k)],
                      "overturning_min_Sv": float(psi[jm, km]), "at_min": [int(jm), int(km)],
                      "heat_transport_W_by_row": [float(x) for x in heat]}))
