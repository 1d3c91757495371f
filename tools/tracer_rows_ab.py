"""One row per lane of the tracer tendency kernel against two (GB25_TRACER_ROWS = 1 | 2, read by gb25_create), in ONE process on one
GPU with one library: a fresh model per timed loop, alternating 1, 2, 2, 1, ...  Per size: steps/s of the loops and, from a second
loop with the library's event timer on the tracer kernel alone, the mean time of its launch.  The first round warms the clocks.
python tools/tracer_rows_ab.py [--float-type Float32] [--steps 100] [--rounds 5] Nx,Ny,Nz [Nx,Ny,Nz ...]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gb25_amd as gb

ap = argparse.ArgumentParser()
ap.add_argument("sizes", nargs="+")
ap.add_argument("--float-type", default="Float32")
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--rounds", type=int, default=5)
args = ap.parse_args()


def timed(rows, shape):
    os.environ["GB25_TRACER_ROWS"] = str(rows)
    try:
        m = gb.baroclinic_instability_model(gb.GPU(float_type=args.float_type), *shape, dt=120.0)
    finally:
        del os.environ["GB25_TRACER_ROWS"]
    gb.set_baroclinic_instability(m)
    gb.first_time_step(m)
    gb.loop(m, 20)
    m.backend.synchronize()
    t = time.perf_counter()
    gb.loop(m, args.steps)
    m.backend.synchronize()
    rate = args.steps / (time.perf_counter() - t)
    m.backend.profile_enable(only="tracers")
    m.backend.profile_reset()
    gb.loop(m, 30)
    m.backend.synchronize()
    n, ms = m.backend.profile_get("tracers")
    m.backend.profile_enable(False)
    m.backend.close()
    return rate, ms / max(n, 1)


for size in args.sizes:
    shape = tuple(int(x) for x in size.split(","))
    out = {1: [], 2: []}
    for r in range(args.rounds):
        for rows in ((1, 2) if r % 2 == 0 else (2, 1)):
            out[rows].append(timed(rows, shape))
    mean = lambda v: sum(v[1:]) / (len(v) - 1)
    res = {"size": shape, "float_type": args.float_type}
    for rows in (1, 2):
        res[f"rows{rows}_steps_per_s"] = [round(a, 1) for a, _ in out[rows]]
        res[f"rows{rows}_tracer_launch_ms"] = [round(b, 4) for _, b in out[rows]]
    res["steps_2_over_1"] = round(mean([a for a, _ in out[2]]) / mean([a for a, _ in out[1]]), 4)
    res["tracer_launch_2_over_1"] = round(mean([b for _, b in out[2]]) / mean([b for _, b in out[1]]), 4)
    print(json.dumps(res), flush=True)
