"""Shared helpers for the test-suite: deterministic initial conditions and model factories."""
import numpy as np

import gb25_amd as gb
from gb25_amd.binding import FIELD_IDS
from oracle_backend import CPU


def counter_rng(shape, seed, salt):
    """Build-owned, platform-independent U(0,1) numbers (SplitMix64 on the linear index):
    the Julia RNG stream of the reference (Random.seed!(42)) cannot be reproduced outside Julia."""
    n = int(np.prod(shape))
    with np.errstate(over="ignore"):
        x = (np.arange(n, dtype=np.uint64) + np.uint64(seed) * np.uint64(0x9E3779B97F4A7C15)
             + np.uint64(salt) * np.uint64(0xD1B54A32D192ED03))
        x ^= x >> np.uint64(30); x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(27); x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    u = (x >> np.uint64(11)).astype(np.float64) / float(1 << 53)
    return u.reshape(shape, order="F")


def set_noisy_velocities(model, amplitude=1e-3, seed=42):
    """u, v = 1e-3 * rand (correctness/correctness_baroclinic_instability_simulation_run.jl:40-42)."""
    ui = amplitude * counter_rng(model.velocities.u.shape, seed, 1)
    vi = amplitude * counter_rng(model.velocities.v.shape, seed, 2)
    dt = model.backend.dtype
    model.set(u=ui.astype(dt), v=vi.astype(dt))
    return ui, vi


def set_noisy_state_with_halos(model, amplitude=0.05):
    """The baroclinic-instability state, noisy velocities of `amplitude`, and 1e-3 of counter-rng noise on every cell of the parent
    arrays of T, S, u, v, eta, V -- EVERY halo layer included (tests/test_step_spec.py, tests/test_gpu_step_identities.py)."""
    dtype = model.backend.dtype
    gb.set_baroclinic_instability(model)
    set_noisy_velocities(model, amplitude)
    for n, seed in (("T", 5), ("S", 4), ("u", 6), ("v", 7), ("eta", 8), ("V", 9)):
        a = model.backend.get_field(n, True)
        a += (1e-3 * counter_rng(a.shape, seed, 1)).astype(dtype)
        model.backend.set_field(n, a, True)


# What the GPU tests of the diagnostics (tests/test_gpu_{diagnostics,integrals,derived,transports,averages,classes,particles}.py) share
EPS = float(np.finfo(np.float64).eps)
GRID_NAMES = {0: "simple_lat_lon", 1: "gaussian_islands_lat_lon", 3: "tripolar", 4: "gaussian_islands"}
CASES = [(ft, gt) for ft in ("Float32", "Float64") for gt in (0, 1, 4)]
BASE_FIELDS = [n for n, i in FIELD_IDS.items() if i < FIELD_IDS["e"]]
CATKE_FIELDS = [n for n, i in FIELD_IDS.items() if i >= FIELD_IDS["e"]]


def size_of(grid_type):
    return (48, 24, 6) if grid_type else (64, 32, 8)


def stepped_model(float_type="Float32", grid_type=0, steps=3, size=None, seed=42, closure=None, dt=None, arch=None, **options):
    """The baroclinic-instability state with noisy velocities after first_time_step and `steps` more; arch: another backend
    factory (the CPU oracle) in place of GPU(float_type)."""
    Nx, Ny, Nz = size or size_of(grid_type)
    dt = dt or (60.0 if grid_type == 4 else 600.0)
    m = gb.baroclinic_instability_model(arch or gb.GPU(float_type=float_type), Nx, Ny, Nz, dt=dt, grid_type=GRID_NAMES[grid_type],
                                        closure=closure, options=options or None)
    gb.set_baroclinic_instability(m)
    set_noisy_velocities(m, seed=seed)
    gb.first_time_step(m)
    if steps:
        gb.loop(m, steps)
    return m


def make_pair(Nx, Ny, Nz, dt, precision="f64", float_type="Float32", **kw):
    """(HIP model, oracle model) with the same configuration, like rmodel / vmodel of the reference."""
    rmodel = gb.baroclinic_instability_model(gb.GPU(float_type=float_type), Nx, Ny, Nz, dt=dt, **kw)
    vmodel = gb.baroclinic_instability_model(CPU(precision), Nx, Ny, Nz, dt=dt, **kw)
    return rmodel, vmodel


def make_oracle(Nx, Ny, Nz, dt, precision="f64", **kw):
    return gb.baroclinic_instability_model(CPU(precision), Nx, Ny, Nz, dt=dt, **kw)


SQRT_EPS64 = float(np.sqrt(np.finfo(np.float64).eps))   # 1.4901e-8: the reference's rtol for Float64
SQRT_EPS32 = float(np.sqrt(np.finfo(np.float32).eps))   # 3.4527e-4: the reference's rtol for Float32
# One tolerance for every compared field (state AND tendencies), as in the reference.  It is attainable in fp32
# because the hydrostatic pressure (equation of state + vertical integral) is evaluated in fp64 inside the GPU
# kernel; with an fp32 equation of state G.u, G.S and w sit ~1e-3 away from an fp64 run.
TENDENCY_RTOL = SQRT_EPS32
STATE_FIELDS = ("u", "v", "w", "eta", "T", "S", "filtered.U", "filtered.V", "filtered.eta")
# every parent array of a model without a closure, by the names of binding.FIELD_IDS (the bitwise tests compare them all)
ALL_FIELDS = ["u", "v", "w", "T", "S", "pHY", "Gn.u", "Gn.v", "Gn.T", "Gn.S", "Gm.u", "Gm.v", "Gm.T", "Gm.S",
              "eta", "U", "V", "eta_bar", "U_bar", "V_bar", "Gn.U", "Gn.V"]


def assert_states_close(m1, m2, *, state_rtol=SQRT_EPS32, tendency_rtol=TENDENCY_RTOL, include_halos=True, label=""):
    """compare_states (norm-wise, atol = 0, halos included) at rtol = sqrt(eps(Float32)) for every field of the
    reference's compared set (src/correctness.jl:28-90)."""
    _, report = gb.compare_states(m1, m2, rtol=state_rtol, include_halos=include_halos, verbose=False)
    bad = []
    for r in report:
        tol = state_rtol if r["name"] in STATE_FIELDS else tendency_rtol
        if not (r["rel"] <= tol):
            bad.append((r["name"], r["rel"], tol, r["maxdelta"], r["index"]))
    assert not bad, f"{label}: fields out of tolerance: {bad}"
    return report
