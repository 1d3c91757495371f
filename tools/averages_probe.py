"""Cost of one sample of the device averages (gb25_averages_accumulate) at a given size, Float32, one process: ms per sample from
the library's HIP-event timer (slot "diagnostics": the one launch of a sample) for the masks means / means+squares / all, the
algorithmic bytes of a sample -- every input element once, every active accumulator element read and written once -- and the
resulting GB/s, next to the only route without the accumulators: get_field of the five parents, halos included.  Medians over
--reps samples after a warm-up.  Prints one JSON object and writes it to profiles/averages_<Nx>x<Ny>x<Nz>.json (--out).
GB25_LIB selects another build of the library (the non-temporal A/B): --label names it in the output.
usage: averages_probe.py [--size 1440 720 48] [--reps 30] [--label default] [--out PATH] [--no-download]"""
import argparse, json, os, socket, statistics, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, nargs=3, default=[1440, 720, 48])
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--label", default="default")
ap.add_argument("--out", default=None)
ap.add_argument("--no-download", action="store_true")
a = ap.parse_args()
import gb25_amd as gb
import bench
from gb25_amd.averages import quantities_of
Nx, Ny, Nz = a.size

m = gb.baroclinic_instability_model(gb.GPU(), Nx, Ny, Nz, dt=120.0)
gb.set_baroclinic_instability(m)
m.set(u=(1e-3 * bench.counter_rng((Nx, Ny, Nz), 42, 1)).astype(np.float32),
      v=(1e-3 * bench.counter_rng((Nx, Ny + 1, Nz), 42, 2)).astype(np.float32))
gb.first_time_step(m)
gb.loop(m, 5)
b = m.backend


def algorithmic_bytes(groups):
    """fp32 inputs read once (u, v, w, T, S over their interiors, eta) + 16 B per element of every active accumulator"""
    inputs = 4 * (sum(int(np.prod(b.field_dims(n, False))) for n in ("u", "v", "w", "T", "S")) + Nx * Ny)
    acc = 16 * sum(int(np.prod(b.average_dims(q))) for q in quantities_of(groups))
    return inputs, acc


res = {"size": [Nx, Ny, Nz], "float_type": "Float32", "reps": a.reps, "host": socket.gethostname(), "label": a.label,
       "library": os.path.basename(os.environ.get("GB25_LIB") or "libgb25hip.so"), "masks": {}}
for name, groups in (("means", ("means",)), ("means+squares", ("means", "squares")), ("all", ("means", "squares", "fluxes"))):
    b.averages_begin(groups)
    b.profile_enable(True)
    for _ in range(5):
        b.averages_accumulate(1.0)
    ms = []
    for _ in range(a.reps):
        b.profile_reset()
        b.averages_accumulate(1.0)
        n, t = b.profile_get("diagnostics")
        assert n == 1
        ms.append(t)
    b.profile_enable(False)
    inputs, acc = algorithmic_bytes(groups)
    med = statistics.median(ms)
    res["masks"][name] = {"quantities": len(quantities_of(groups)), "ms_median": med, "ms_min": min(ms), "ms_max": max(ms),
                          "input_bytes": inputs, "accumulator_bytes": acc, "GBps_median": (inputs + acc) / med / 1e6}
    b.averages_end()
b.synchronize()
t = time.perf_counter()
gb.loop(m, 50)
b.synchronize()
res["time_step_ms"] = 1e3 * (time.perf_counter() - t) / 50
if not a.no_download:
    # the route of a model without the accumulators: the five parent arrays to the host, per sample
    wall = []
    for _ in range(3):
        t = time.perf_counter()
        parents = [b.get_field(n, True) for n in ("u", "v", "w", "T", "S")]
        wall.append(1e3 * (time.perf_counter() - t))
    nbytes = sum(p.nbytes for p in parents)
    res["download_route"] = {"fields": 5, "bytes": nbytes, "ms_median": statistics.median(wall), "ms_all": wall}
    res["download_over_all_groups"] = res["download_route"]["ms_median"] / res["masks"]["all"]["ms_median"]
text = json.dumps(res, indent=1)
print(text)
out = a.out or os.path.join(ROOT, "profiles", f"averages_{Nx}x{Ny}x{Nz}.json")
os.makedirs(os.path.dirname(out), exist_ok=True)
open(out, "w").write(text + "\n")
