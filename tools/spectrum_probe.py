#!/usr/bin/env python3
"""Which zonal wavenumber grows, and how fast: steps the baroclinic-instability model and every few steps prints the dominant
wavenumber and the power of v along one row and level (gb.zonal_power_spectrum: transformed on the device, a few kilobytes
cross PCIe), with the exponential growth rate of that power between consecutive samples, sigma = ln(P2 / P1) / (2 (t2 - t1)).
With --time: the time per call of three windows against the host paths for the same answer (gb25_get_field + np.fft.rfft, and the
numpy restatement spectrum_host), one JSON object (profiles/spectrum_1440x720x48.json).
usage: spectrum_probe.py [--size 1440 720 48] [--steps 200] [--every 20] [--row J] [--level K] [--source v] [--time] [--reps 20]"""
import argparse, json, math, os, statistics, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, nargs=3, default=[1440, 720, 48])
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--every", type=int, default=20)
ap.add_argument("--row", type=int, default=None)
ap.add_argument("--level", type=int, default=None)
ap.add_argument("--source", default="v")
ap.add_argument("--dt", type=float, default=120.0)
ap.add_argument("--time", action="store_true")
ap.add_argument("--reps", type=int, default=20)
a = ap.parse_args()
import gb25_amd as gb
import bench
from gb25_amd.spectra import dominant_wavenumber, spectrum_host
Nx, Ny, Nz = a.size
row = Ny // 4 if a.row is None else a.row          # (the flank of the jet of the southern hemisphere)
level = Nz - 1 if a.level is None else a.level

m = gb.baroclinic_instability_model(gb.GPU(), Nx, Ny, Nz, dt=a.dt)
gb.set_baroclinic_instability(m)
m.set(u=(1e-3 * bench.counter_rng((Nx, Ny, Nz), 42, 1)).astype(np.float32),
      v=(1e-3 * bench.counter_rng((Nx, Ny + 1, Nz), 42, 2)).astype(np.float32))
gb.first_time_step(m)
b = m.backend


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
    """the library's event pair around the launches of one call"""
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
    gb.loop(m, 5)
    M = Nx // 2 + 1
    res = {"size": [Nx, Ny, Nz], "float_type": "Float32", "source": a.source, "windows": {}}
    windows = (("surface_all_wavenumbers", None, (Nz - 1, 1)), ("all_levels_wavenumbers_0_31", (0, 32), None),
               ("all_levels_all_wavenumbers", None, None))
    for name, wn, lv in windows:
        mc, kc = (M if wn is None else wn[1]), (Nz if lv is None else lv[1])
        w = {"records": mc * kc * b.field_dims(a.source, False)[1], "bytes_to_host": 16 * mc * kc * b.field_dims(a.source, False)[1]}
        w["device_call_wall"] = wall_ms(lambda: b.zonal_spectrum(a.source, wn, lv), a.reps)
        w["device_kernel"] = device_ms(lambda: b.zonal_spectrum(a.source, wn, lv), a.reps)

        def fft_path():
            x = b.get_field(a.source, True)            # (gb25_get_field: the parent array, as a user without the kernel would)
            H = b.cfg.halo
            k0 = 0 if lv is None else lv[0]
            x = x[H:H + Nx, H:H + b.field_dims(a.source, False)[1], H + k0:H + k0 + kc]
            X = np.fft.rfft(x.astype(np.float64), axis=0)
            return X if wn is None else X[wn[0]:wn[0] + wn[1]]
        w["get_field_plus_rfft_wall"] = wall_ms(fft_path, 3)
        if name == "all_levels_all_wavenumbers":
            # (the restatement loops over i in numpy over [level, row, m] arrays: one level is timed, not all of them)
            w["spectrum_host_wall_ONE_LEVEL_of_the_window"] = wall_ms(lambda: spectrum_host(b, a.source, wn, (Nz - 1, 1)), 1, warm=False)
        else:
            w["spectrum_host_wall"] = wall_ms(lambda: spectrum_host(b, a.source, wn, lv), 1, warm=False)
        res["windows"][name] = w
        print(name, json.dumps(w), flush=True)
    print(json.dumps(res, indent=1))
    sys.exit(0)

print(f"# {a.source} at row {row}, level {level} of {Nx} x {Ny} x {Nz}, dt = {a.dt} s")
print("# iteration   time [d]   dominant m   P(m) [unit^2]   growth rate [1/d]")
last = None
for it in range(0, a.steps + 1, a.every):
    if it:
        gb.loop(m, a.every)
    P = gb.zonal_power_spectrum(m, a.source, (1, -1), (level, 1))[0, row]      # (without the zonal mean)
    k = int(dominant_wavenumber(P, 1))
    t = m.clock.time
    rate = ""
    if last is not None and last[1][k - 1] > 0 and P[k - 1] > 0 and t > last[0]:      # (of the same wavenumber)
        rate = f"{math.log(P[k - 1] / last[1][k - 1]) / (2 * (t - last[0])) * 86400.0:12.4f}"
    print(f"{m.clock.iteration:9d} {t / 86400.0:10.4f} {k:12d} {P[k - 1]:15.6e} {rate}")
    last = (t, P)
