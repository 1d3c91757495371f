#!/usr/bin/env python3
"""Flow kinematics of a stepped model, computed where the fields live (gb25_get_kinematics): the area fraction of vortex cores
(W < -0.2 sigma_W) and of strain-dominated water (W > 0.2 sigma_W, sigma_W the standard deviation of the Okubo-Weiss parameter W
over the wet surface cells), max |Ro|, the 99th percentile of |grad rho|.  With --time, for W and for F(potential density), over
all levels and over the surface level alone: the launch time from the built-in GB25_K_DIAGNOSTICS timer (medians of --reps), the
bytes the request must read and write, the implied bandwidth -- beside gb25_compute_derived(GB25_D_VORTICITY) over the same window
in the same process (the project's existing stencil diagnostic over the same inputs: the yardstick) and gb25_get_field of u and v
(what a user pays without the kernels); one JSON object (profiles/kinematics_1440x720x48.json).
usage: kinematics_probe.py [--size 1440 720 48] [--dt 120] [--steps 20] [--time] [--reps 5] [--json PATH]"""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, nargs=3, default=[1440, 720, 48])
ap.add_argument("--dt", type=float, default=120.0)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--float-type", default="Float32")
ap.add_argument("--time", action="store_true")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--json", default=None)
a = ap.parse_args()
import gb25_amd as gb
import bench
Nx, Ny, Nz = a.size
m = gb.baroclinic_instability_model(gb.GPU(float_type=a.float_type), Nx, Ny, Nz, dt=a.dt)
b = m.backend
gb.set_baroclinic_instability(m)
m.set(u=(1e-3 * bench.counter_rng((Nx, Ny, Nz), 42, 1)).astype(b.dtype), v=(1e-3 * bench.counter_rng((Nx, Ny + 1, Nz), 42, 2)).astype(b.dtype))
gb.first_time_step(m)
if a.steps > 1:
    gb.loop(m, a.steps - 1)
top = (Nz - 1, 1)
W = np.asarray(gb.okubo_weiss(m, levels=top), np.float64)[:, :, 0]
wet = np.asarray(gb.potential_density(m, levels=top))[:, :, 0] != 0
sw = W[wet].std()
ro = b.kinematics_stats("rossby_number")
grad = np.asarray(gb.gradient_magnitude(m, "potential_density", levels=top), np.float64)[:, :, 0]
res = {"size": [Nx, Ny, Nz], "float_type": a.float_type, "steps": a.steps,
       "surface": {"sigma_W": sw, "area_fraction_cores": float((W[wet] < -0.2 * sw).mean()), "area_fraction_strain": float((W[wet] > 0.2 * sw).mean()),
                   "grad_rho_p99": float(np.percentile(grad[wet], 99))},
       "max_abs_Ro": ro.max_abs, "Ro_at": list(ro.at_max_abs)}
print(f"surface: sigma_W {sw:.3e} s^-2, cores (W < -0.2 sigma_W) {100 * res['surface']['area_fraction_cores']:.1f} % of the wet area, "
      f"strain (W > 0.2 sigma_W) {100 * res['surface']['area_fraction_strain']:.1f} %")
print(f"max |Ro| {ro.max_abs:.3e} at {tuple(ro.at_max_abs)}; 99th percentile of |grad rho| at the surface {res['surface']['grad_rho_p99']:.3e} kg/m^4")


def kernel_ms(call):
    """median and min of the GB25_K_DIAGNOSTICS timer over the launches of `call`"""
    call()
    out = []
    b.profile_enable(True)
    for _ in range(a.reps):
        b.profile_reset()
        call()
        out.append(b.profile_get("diagnostics")[1])
    b.profile_enable(False)
    return {"ms_median": statistics.median(out), "ms_min": min(out), "reps": a.reps}


def wall_ms(call):
    call()
    out = []
    for _ in range(a.reps):
        t = time.perf_counter()
        call()
        out.append(1e3 * (time.perf_counter() - t))
    return {"ms_median": statistics.median(out), "ms_min": min(out), "reps": a.reps}


if a.time:
    rb = np.dtype(b.dtype).itemsize
    timing = {}
    for label, levels in (("all_levels", (0, Nz)), ("surface", top)):
        nk = levels[1]
        plane = Nx * Ny * nk * rb
        zeta = kernel_ms(lambda: b.compute_derived("vorticity", None, levels))
        w = {"vorticity": dict(zeta, bytes=3 * plane, GB_per_s=3 * plane / (1e6 * zeta["ms_median"]))}
        # bytes a request must move: u, v (and T, S for the density) once, the result once
        for name, kind, param, fields in (("okubo_weiss", "okubo_weiss", 0, 2), ("frontogenesis_rho", "frontogenesis", 2, 4)):
            k = kernel_ms(lambda: b.compute_kinematics(kind, param, levels))
            nbytes = (fields + 1) * plane
            w[name] = dict(k, bytes=nbytes, GB_per_s=nbytes / (1e6 * k["ms_median"]), over_vorticity=k["ms_median"] / zeta["ms_median"])
        timing[label] = w
        print(f"{label}:", json.dumps(w), flush=True)
    pcie = wall_ms(lambda: (b.get_field("u", True), b.get_field("v", True)))
    timing["get_field_u_v"] = dict(pcie, bytes=int(sum(np.prod(b.field_dims(n, True)) for n in ("u", "v")) * rb))
    timing["get_field_u_v_over_okubo_weiss_all_levels"] = pcie["ms_median"] / timing["all_levels"]["okubo_weiss"]["ms_median"]
    print("get_field(u) + get_field(v):", json.dumps(timing["get_field_u_v"]), flush=True)
    res["timing"] = timing
if a.json:
    with open(a.json, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
