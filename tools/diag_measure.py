"""Cost of the device diagnostics at 1440x720x48 Float32, one process: the three kernels (HIP-event timers of the library,
slot "diagnostics": both launches of a call), compare_states on the device against the numpy path, state_monitor against one
time_step.  Prints one JSON object (profiles/diag_1440x720x48.json).
usage: diag_measure.py [--size 1440 720 48] [--reps 50]"""
import argparse, json, os, statistics, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, nargs=3, default=[1440, 720, 48])
ap.add_argument("--reps", type=int, default=50)
a = ap.parse_args()
import gb25_amd as gb
import bench
Nx, Ny, Nz = a.size


def model(seed):
    m = gb.baroclinic_instability_model(gb.GPU(), Nx, Ny, Nz, dt=120.0)
    gb.set_baroclinic_instability(m)
    m.set(u=(1e-3 * bench.counter_rng((Nx, Ny, Nz), seed, 1)).astype(np.float32),
          v=(1e-3 * bench.counter_rng((Nx, Ny + 1, Nz), seed, 2)).astype(np.float32))
    gb.first_time_step(m)
    gb.loop(m, 5)
    return m


def device_ms(b, call, reps):
    """median over `reps` of the library's event pair around the launches of one call"""
    b.profile_enable(True)
    for _ in range(5):
        call()
    out = []
    for _ in range(reps):
        b.profile_reset()
        call()
        out.append(b.profile_get("diagnostics")[1])
    b.profile_enable(False)
    return statistics.median(out), min(out)


def wall_ms(call, reps):
    call()
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        call()
        out.append(1e3 * (time.perf_counter() - t))
    return statistics.median(out)


m1, m2 = model(42), model(43)
b1, b2 = m1.backend, m2.backend
res = {"size": [Nx, Ny, Nz], "float_type": "Float32", "reps": a.reps, "hbm_streaming_reference_TBps": 6.3}
for label, halos in (("k_field_stats_T_interior", False), ("k_field_stats_T_parent", True)):
    n = int(np.prod(b1.field_dims("T", halos)))
    med, best = device_ms(b1, lambda: b1.field_stats("T", halos), a.reps)
    res[label] = {"elements": n, "bytes": 4 * n, "ms_median": med, "ms_min": best, "TBps_median": 4 * n / med / 1e9}
n = int(np.prod(b1.field_dims("T", False)))
med, best = device_ms(b1, lambda: b1.compare_field("T", b2), a.reps)
res["k_field_diff_T_interior"] = {"elements": n, "bytes": 8 * n, "ms_median": med, "ms_min": best, "TBps_median": 8 * n / med / 1e9}
med, best = device_ms(b1, b1.state_monitor, a.reps)
res["state_monitor"] = {"device_ms_median": med, "device_ms_min": best, "wall_ms_median": wall_ms(b1.state_monitor, a.reps)}
b1.synchronize()
t = time.perf_counter()
gb.loop(m1, 100)
b1.synchronize()
res["time_step_ms"] = 1e3 * (time.perf_counter() - t) / 100
res["state_monitor"]["in_time_steps"] = res["state_monitor"]["wall_ms_median"] / res["time_step_ms"]
cmp_dev = wall_ms(lambda: gb.compare_states(m1, m2, verbose=False, on_device=True), 5)
cmp_host = wall_ms(lambda: gb.compare_states(m1, m2, verbose=False, on_device=False), 1)
res["compare_states"] = {"device_ms": cmp_dev, "host_ms": cmp_host, "speedup": cmp_host / cmp_dev, "fields": 17}
print(json.dumps(res, indent=1))
