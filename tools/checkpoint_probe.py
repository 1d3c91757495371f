"""What a checkpoint costs at a given size, Float32, one process, one run on one box:
 (a) how long gb25_checkpoint_snapshot keeps the model's stream busy: the one pack launch (the library's HIP-event timer, slot
     "diagnostics"), and the host time of the call;
 (b) the pack kernel's bytes moved per second (every byte of the set read once and written once);
 (c) the same gb25_field members copied with hipMemcpyDtoDAsync, member by member, between HIP events: the yardstick for (b);
 (d) loop(20) while the drain of a snapshot runs beside it, against loop(20) alone;
 (e) the members read with gb25_get_field one after the other, halos included: the only route without the snapshot, the yardstick
     for (a) + (d).
Warm-up first, then --reps repetitions; medians with minimum and maximum.  Prints one JSON object and writes it to
profiles/checkpoint_<Nx>x<Ny>x<Nz>.json (--out).
usage: checkpoint_probe.py [--size 1440 720 48] [--reps 7] [--out PATH]"""
import argparse, ctypes as C, json, os, socket, statistics, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, nargs=3, default=[1440, 720, 48])
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--out", default=None)
a = ap.parse_args()
import gb25_amd as gb
import bench
from gb25_amd import restart
Nx, Ny, Nz = a.size
STEPS = 20

m = gb.baroclinic_instability_model(gb.GPU(), Nx, Ny, Nz, dt=120.0)
gb.set_baroclinic_instability(m)
m.set(u=(1e-3 * bench.counter_rng((Nx, Ny, Nz), 42, 1)).astype(np.float32),
      v=(1e-3 * bench.counter_rng((Nx, Ny + 1, Nz), 42, 2)).astype(np.float32))
gb.first_time_step(m)
gb.loop(m, 5)
b = m.backend


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def timed(fn):
    b.synchronize()
    t0 = time.perf_counter()
    fn()
    b.synchronize()
    return (time.perf_counter() - t0) * 1e3


# ---- warm-up: the first snapshot allocates the arena and the pinned buffers
scratch = tempfile.mkdtemp(prefix="checkpoint_probe_")
b.checkpoint_snapshot()
info = b.checkpoint_info()
path = b.checkpoint_write(scratch, "warm")
members = restart.read_checkpoint(path).table
set_bytes = int(info.bytes)
field_names = [n for n, row in members.items() if row["field"] >= 0]
field_bytes = sum(members[n]["bytes"] for n in field_names)
gb.loop(m, STEPS)
b.synchronize()

res = {"size": [Nx, Ny, Nz], "float_type": "Float32", "reps": a.reps, "host": socket.gethostname(), "members": int(info.members),
       "set_bytes": set_bytes, "field_members": len(field_names), "field_bytes": field_bytes, "steps_per_loop": STEPS}

# ---- (a), (b): the pack launch and the call; each snapshot is released by writing nothing: wait for the drain, then drop it
pack_ms, call_ms, drain_ms = [], [], []
b.profile_enable(True)
for _ in range(a.reps):
    gb.loop(m, 2)
    b.synchronize()
    b.profile_reset()
    t0 = time.perf_counter()
    b.checkpoint_snapshot()
    call_ms.append((time.perf_counter() - t0) * 1e3)
    while not b.checkpoint_info().drained:
        time.sleep(0.0005)
    drain_ms.append((time.perf_counter() - t0) * 1e3)
    n, t = b.profile_get("diagnostics")
    assert n == 1, n
    pack_ms.append(t)
    b.checkpoint_write(scratch, "probe")
b.profile_enable(False)
res["a_pack_launch_ms"] = spread(pack_ms)
res["a_snapshot_call_host_ms"] = spread(call_ms)
res["drain_complete_after_ms"] = spread(drain_ms)
res["b_pack_GBps"] = spread([2 * set_bytes / t / 1e6 for t in pack_ms])

# ---- (c): hipMemcpyDtoDAsync of the field members, one call each, into a buffer of the arena's size
hip = C.CDLL("libamdhip64.so")
hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
hip.hipMemcpyDtoDAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
hip.hipEventSynchronize.argtypes = [C.c_void_p]
hip.hipFree.argtypes = [C.c_void_p]
buf, e0, e1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
assert hip.hipMalloc(C.byref(buf), field_bytes + 16 * len(field_names)) == 0
assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
b.synchronize()
ptrs = [(b.field_device_ptr_readonly(n)[0], members[n]["bytes"]) for n in field_names]


def copies():
    at = buf.value
    for p, nbytes in ptrs:
        assert hip.hipMemcpyDtoDAsync(at, p, nbytes, None) == 0
        at += (nbytes + 15) // 16 * 16


d2d_ms = []
for rep in range(a.reps + 2):
    hip.hipEventRecord(e0, None)
    copies()
    hip.hipEventRecord(e1, None)
    hip.hipEventSynchronize(e1)
    ms = C.c_float()
    hip.hipEventElapsedTime(C.byref(ms), e0, e1)
    if rep >= 2:
        d2d_ms.append(ms.value)
hip.hipFree(buf)
res["c_d2d_copies_ms"] = spread(d2d_ms)
res["c_d2d_GBps"] = spread([2 * field_bytes / t / 1e6 for t in d2d_ms])
res["c_pack_ms_scaled_to_field_bytes"] = res["a_pack_launch_ms"]["median"] * field_bytes / set_bytes

# ---- (d): loop(STEPS) alone, and beside the drain of a snapshot taken just before it
alone, beside = [], []
for _ in range(a.reps):
    alone.append(timed(lambda: gb.loop(m, STEPS)))
    b.synchronize()
    b.checkpoint_snapshot()
    t0 = time.perf_counter()
    gb.loop(m, STEPS)
    b.synchronize()
    beside.append((time.perf_counter() - t0) * 1e3)
    b.checkpoint_write(scratch, "probe")
res["d_loop_alone_ms"] = spread(alone)
res["d_loop_beside_drain_ms"] = spread(beside)
res["d_slowdown_ms"] = statistics.median(beside) - statistics.median(alone)

# ---- (e): gb25_get_field of every field member, halos included
res["e_get_field_ms"] = spread([timed(lambda: [b.get_field(n, True) for n in field_names]) for _ in range(max(3, a.reps // 2))])
res["a_plus_d_ms"] = res["a_pack_launch_ms"]["median"] + max(0.0, res["d_slowdown_ms"])
res["one_launch_faster_than_d2d"] = res["c_pack_ms_scaled_to_field_bytes"] < res["c_d2d_copies_ms"]["median"]
res["a_plus_d_beats_e"] = res["a_plus_d_ms"] < res["e_get_field_ms"]["median"]

for f in os.listdir(os.path.join(scratch, "probe")) + os.listdir(os.path.join(scratch, "warm")):
    for lab in ("probe", "warm"):
        if os.path.exists(os.path.join(scratch, lab, f)):
            os.remove(os.path.join(scratch, lab, f))
print(json.dumps(res))
out = a.out or os.path.join(ROOT, "profiles", f"checkpoint_{Nx}x{Ny}x{Nz}.json")
with open(out, "w") as fh:
    json.dump(res, fh, indent=1)
    fh.write("\n")
