#!/usr/bin/env python3
"""A coarse map and the heat content: steps the baroclinic-instability model a few steps and prints the surface temperature on a
coarser grid (gb.coarsen: block means reduced on the device, one small array crosses PCIe), the sub-grid variance next to it, and a
summary of the heat content of the upper `--depth` metres per band of rows (gb.heat_content), with the time per call.  With --time:
the kernel and call times of the block sums of T for the blocks (1, 1, Nz), (4, 4, 1), (8, 8, Nz) and of the kinetic energy for
(4, 4, 1), next to gb25_integrate_field(TOTAL) of the same field -- it reads the same bytes -- and to the host route for the same
answer (get_field and blocks.block_sums_host), one JSON object (profiles/blocks_1440x720x48.json).
usage: coarsen_probe.py [--size 1440 720 48] [--steps 20] [--block 8 8] [--depth 700] [--rows 12] [--time] [--reps 20] [--json PATH]"""
import argparse, json, os, statistics, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, nargs=3, default=[1440, 720, 48])
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--block", type=int, nargs=2, default=[8, 8])
ap.add_argument("--depth", type=float, default=700.0)
ap.add_argument("--rows", type=int, default=12)
ap.add_argument("--dt", type=float, default=120.0)
ap.add_argument("--time", action="store_true")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--json", default=None)
a = ap.parse_args()
import gb25_amd as gb
import bench
from gb25_amd.blocks import block_sums_host
Nx, Ny, Nz = a.size

m = gb.baroclinic_instability_model(gb.GPU(), Nx, Ny, Nz, dt=a.dt)
gb.set_baroclinic_instability(m)
m.set(u=(1e-3 * bench.counter_rng((Nx, Ny, Nz), 42, 1)).astype(np.float32),
      v=(1e-3 * bench.counter_rng((Nx, Ny + 1, Nz), 42, 2)).astype(np.float32))
gb.first_time_step(m)
gb.loop(m, a.steps)
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
    """the library's event pairs around the launches of one call"""
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
    real = np.dtype(b.dtype).itemsize
    res = {"size": [Nx, Ny, Nz], "float_type": b.float_type, "calls": {}}
    read = Nx * Ny * Nz * real
    total = {"bytes_read_at_least": read}
    total["device_call_wall"] = wall_ms(lambda: b.integrate_field("T", "total"), a.reps)
    total["device_kernel"] = device_ms(lambda: b.integrate_field("T", "total"), a.reps)
    total["kernel_GB_per_s_of_those_bytes"] = read / (1e6 * total["device_kernel"]["ms_median"])
    res["integrate_field_T_total"] = total
    print("integrate_field(T, total):", json.dumps(total), flush=True)
    for source, block in (("T", (1, 1, Nz)), ("T", (4, 4, 1)), ("T", (8, 8, Nz)), ("kinetic_energy", (4, 4, 1))):
        blocks = (Nx // block[0]) * (Ny // block[1]) * (Nz // block[2])
        # T: every interior value once; the kinetic energy: u and v read and the packed array written and read again
        bytes_read = read if source == "T" else 3 * read
        w = {"source": source, "block": list(block), "blocks": blocks, "bytes_read_at_least": bytes_read,
             "bytes_written": 3 * 8 * blocks + (read if source != "T" else 0), "bytes_to_host": 3 * 8 * blocks}
        w["device_call_wall"] = wall_ms(lambda: b.block_sums(source, block), a.reps)
        if source == "T":
            w["device_kernel"] = device_ms(lambda: b.compute_block_sums(source, block), a.reps)
        else:       # (two launches under the timer: the derived field, then the block sums over it)
            w["device_kernel"] = device_ms(lambda: b.block_sums(source, block, planes=("first",)), a.reps)
        w["kernel_GB_per_s_of_those_bytes"] = (w["bytes_read_at_least"] + w["bytes_written"]) / (1e6 * w["device_kernel"]["ms_median"])
        w["kernel_over_integrate_field_total"] = w["device_kernel"]["ms_median"] / total["device_kernel"]["ms_median"]
        if (source, block) == ("T", (4, 4, 1)):
            def host_route():
                b.get_field(source, True)                   # (the parent a user without the kernel downloads)
                return block_sums_host(b, source, block)
            w["get_field_plus_block_sums_host_wall"] = wall_ms(host_route, 1, warm=False)
        res["calls"][f"{source}_{block[0]}x{block[1]}x{block[2]}"] = w
        print(f"{source} {block}:", json.dumps(w), flush=True)
    text = json.dumps(res, indent=1)
    print(text)
    if a.json:
        with open(a.json, "w") as f:
            f.write(text + "\n")
    sys.exit(0)

bx, by = a.block
t = time.perf_counter()
sst = gb.coarsen(m, "T", (bx, by, 1), levels=(Nz - 1, 1))[:, :, 0]
ms = 1e3 * (time.perf_counter() - t)
var = gb.subgrid_variance(m, "T", (bx, by, Nz))[:, :, 0]
print(f"# surface T of {Nx} x {Ny} x {Nz} after {m.clock.iteration} steps as means of {bx} x {by} cells: {sst.shape[0]} x {sst.shape[1]}; "
      f"first call {ms:.2f} ms")
print("# per coarse row: zonal mean and extrema of the block means, the largest variance inside a block of the whole column")
print("#   row       mean        min        max   max variance")
with np.errstate(invalid="ignore"):
    for J in np.linspace(0, sst.shape[1] - 1, a.rows).astype(int):
        row = sst[:, J]
        if np.isnan(row).all():
            print(f"{J:7d}  {'(land)':>9}")
            continue
        print(f"{J:7d}  {np.nanmean(row):9.4f}  {np.nanmin(row):9.4f}  {np.nanmax(row):9.4f}  {np.nanmax(var[:, J]):12.4e}")
hc = gb.heat_content(m, depth_range=(0.0, a.depth))
ocean = hc != 0
print(f"# heat content of the upper {a.depth:g} m [J m^-2], relative to 0 degrees: mean over the ocean {hc[ocean].mean():.6e}, "
      f"min {hc[ocean].min():.6e}, max {hc[ocean].max():.6e}; land columns {int((~ocean).sum())} of {hc.size}")
for j in np.linspace(0, Ny - 1, a.rows).astype(int):
    row = hc[:, j][ocean[:, j]]
    print(f"{j:7d}  {row.mean():.6e}" if row.size else f"{j:7d}  (land)")
w = wall_ms(lambda: gb.heat_content(m, depth_range=(0.0, a.depth)), a.reps)
print(f"# time per heat_content call (two block-sum calls): median {w['ms_median']:.3f} ms, min {w['ms_min']:.3f} ms over {w['reps']} calls")
