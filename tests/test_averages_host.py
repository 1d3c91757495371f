"""Time averages, the parts that need no GPU: the numpy restatement of gb-25_amd/averages.py on the CPU oracle's fields against
triple loops written out here (it is what the device's accumulators are compared with bit for bit in tests/test_gpu_averages.py,
so it is pinned here independently of the HIP kernel), the host accumulation, what follows from the means on series whose answer
is known in closed form, the placement of the ranks' parts, and the new ABI entries on a handle without a device."""
import ctypes as C

import numpy as np
import pytest

import gb25_amd as gb
from gb25_amd import binding
from gb25_amd.averages import (FLUXES, MEANS, QUANTITIES, SQUARES, AveragesHost, average_terms, eddy_flux, eddy_kinetic_energy,
                               gather_averages, quantities_of, sample_fields, tracer_variance)
from helpers import make_oracle, set_noisy_velocities

H = 8


def stepped_oracle(grid_type="simple_lat_lon", size=(8, 8, 4), steps=2):
    m = make_oracle(*size, 60.0 if grid_type == "tripolar" else 600.0, grid_type=grid_type)
    gb.set_baroclinic_instability(m)
    set_noisy_velocities(m)
    gb.first_time_step(m)
    if steps:
        gb.loop(m, steps)
    return m


def loops(b, quantity, k0, kc):
    """The term of include/gb25.h at every point, by triple loops over 0-based interior indices into the parent arrays."""
    p = {n: np.asarray(b.get_field(n, True), np.float64) for n in ("u", "v", "w", "T", "S", "eta")}
    Nx, Ny, Nz = b.field_dims("T", False)
    byv = b.field_dims("v", False)[1]

    def at(n, i, j, k):
        return p[n][i + H, j + H, k + H]

    if quantity in ("eta", "etaeta"):
        out = np.zeros((Nx, Ny, 1))
        for i in range(Nx):
            for j in range(Ny):
                e = p["eta"][i + H, j + H, 0]
                out[i, j, 0] = e if quantity == "eta" else e * e
        return out
    vel = quantity[0]
    rows = byv if vel == "v" else Ny
    levels = kc + 1 if vel == "w" else kc
    out = np.zeros((Nx, rows, levels))
    for i in range(Nx):
        for j in range(rows):
            for q in range(levels):
                k = k0 + q
                if quantity in MEANS:
                    out[i, j, q] = at(quantity, i, j, k)
                elif quantity in SQUARES:
                    out[i, j, q] = at(vel, i, j, k) * at(vel, i, j, k)
                elif vel == "u":
                    out[i, j, q] = at("u", i, j, k) * (0.5 * (at(quantity[1], i - 1, j, k) + at(quantity[1], i, j, k)))
                elif vel == "v":
                    out[i, j, q] = at("v", i, j, k) * (0.5 * (at(quantity[1], i, j - 1, k) + at(quantity[1], i, j, k)))
                elif 1 <= k <= Nz - 1:
                    out[i, j, q] = at("w", i, j, k) * (0.5 * (at(quantity[1], i, j, k - 1) + at(quantity[1], i, j, k)))
    return out


@pytest.mark.parametrize("grid_type,size", [("simple_lat_lon", (8, 8, 4)), ("tripolar", (48, 24, 6))])
def test_average_terms_against_triple_loops(grid_type, size):
    m = stepped_oracle(grid_type, size)
    b = m.backend
    Nx, Ny, Nz = size
    byv = Ny if grid_type == "tripolar" else Ny + 1
    assert b.field_dims("v", False)[1] == byv
    fields = sample_fields(b)
    assert np.abs(b.get_field("w", False)).max() > 0 and np.abs(b.get_field("u", False)).max() > 0
    for window in (None, (Nz - 1, 1), (1, 3) if Nz > 4 else (1, 2)):
        k0, kc = (0, Nz) if window is None else window
        for q in QUANTITIES:
            got, want = average_terms(b, q, window, fields), loops(b, q, k0, kc)
            assert got.shape == want.shape and got.dtype == np.float64, (q, window)
            assert got.tobytes() == want.tobytes(), (q, window)
        # the face counts of the (c,c,f) quantities, the rows of the (c,f,c) ones, the 2-D ones ignore the window
        assert average_terms(b, "w", window, fields).shape == (Nx, Ny, kc + 1) == average_terms(b, "wT", window, fields).shape
        assert average_terms(b, "vS", window, fields).shape == (Nx, byv, kc) and average_terms(b, "uT", window, fields).shape == (Nx, Ny, kc)
        assert average_terms(b, "etaeta", window, fields).shape == (Nx, Ny, 1)
    # the z fluxes vanish exactly at the bottom and at the top face and nowhere else by construction
    wT = average_terms(b, "wT", None, fields)
    assert (wT[:, :, 0] == 0).all() and (wT[:, :, Nz] == 0).all() and np.abs(wT[:, :, 1:Nz]).max() > 0
    assert (average_terms(b, "wS", (Nz - 1, 1), fields)[:, :, 1] == 0).all()
    # the halo column i - 1 of column 0 is the periodic image
    T = fields["T"]
    assert np.array_equal(T[H - 1, H:H + Ny, H:H + Nz], T[H + Nx - 1, H:H + Ny, H:H + Nz])
    u0 = fields["u"][H, H:H + Ny, H:H + Nz]
    assert np.array_equal(average_terms(b, "uT", None, fields)[0], u0 * (0.5 * (T[H + Nx - 1, H:H + Ny, H:H + Nz] + T[H, H:H + Ny, H:H + Nz])))
    for bad in ((Nz, 1), (0, 0), (-1, 1), (1, Nz), (0, -2)):
        with pytest.raises(ValueError):
            average_terms(b, "T", bad, fields)
    with pytest.raises(ValueError):
        average_terms(b, "Tu", None, fields)
    assert quantities_of(("means",)) == MEANS and quantities_of(("means", "fluxes")) == MEANS + FLUXES and quantities_of(7) == QUANTITIES


@pytest.mark.parametrize("grid_type,size", [("simple_lat_lon", (8, 8, 4)), ("tripolar", (48, 24, 6))])
def test_averages_host_over_four_steps(grid_type, size):
    m = stepped_oracle(grid_type, size, steps=0)
    b = m.backend
    weights = (1.0, 0.3, 2.5, 0.7)
    a = AveragesHost(b)
    raw = {}
    total = 0.0
    for w in weights:
        gb.time_step(m)
        a.sample(w)
        for q in QUANTITIES:
            t = loops(b, q, 0, size[2])
            raw[q] = raw.get(q, np.zeros(t.shape)) + w * t
        total = total + w
    info = a.info()
    assert (info.samples, info.weight_sum, info.groups, info.k_first, info.k_count) == (4, total, 7, 0, size[2])
    assert info.last_iteration == info.first_iteration + 3
    for q in QUANTITIES:
        assert a.raw(q).tobytes() == raw[q].tobytes(), q
        assert a.mean(q).tobytes() == (raw[q] / total).tobytes(), q
    # the public handle on a backend without the device kernel is this accumulation; the default weight is last_dt per step
    h = gb.averages(m, groups=("means", "squares"), levels=(1, 2))
    h.sample()
    gb.loop(m, 3)
    h.sample()
    dt = b.clock()[2]
    assert h.info().weight_sum == dt + 3 * dt and h.info().samples == 2
    assert h.mean("T").shape == (size[0], size[1], 2) and h.raw("w").shape == (size[0], size[1], 3)
    with pytest.raises(ValueError):
        h.raw("vT")
    with pytest.raises(ValueError):
        gb.averages(m, groups=("squares",))
    with pytest.raises(ValueError):
        h.sample(0.0)
    assert h.eddy_kinetic_energy().shape == (size[0], size[1], 2)
    h.close()


def test_eddy_fluxes_and_energies_in_closed_form():
    """Two samples of equal weight of fields uniform in space, x1 and x2, all small integers (every operation exact):
    <x'y'> = (x1 - x2)(y1 - y2) / 4.  A steady series gives exactly 0."""
    Nx, Ny, Nz = 6, 5, 4
    for byv in (Ny + 1, Ny):
        shapes = {"u": (Nx, Ny, Nz), "v": (Nx, byv, Nz), "w": (Nx, Ny, Nz + 1), "T": (Nx, Ny, Nz), "S": (Nx, Ny, Nz)}
        series = [{"u": 3.0, "v": -2.0, "w": 1.0, "T": 10.0, "S": 34.0}, {"u": 7.0, "v": 4.0, "w": -3.0, "T": 6.0, "S": 36.0}]
        for samples, steady in ((series, False), ([series[0]] * 2, True)):
            acc = {}
            for s in samples:
                x = {n: np.full(shapes[n], s[n]) for n in shapes}
                terms = {**x, "uu": x["u"] * x["u"], "vv": x["v"] * x["v"], "TT": x["T"] * x["T"], "SS": x["S"] * x["S"]}
                for vel in "uvw":
                    for c in "TS":
                        terms[vel + c] = np.full(shapes[vel], s[vel] * s[c])
                for n, t in terms.items():
                    acc[n] = acc.get(n, 0.0) + 1.0 * t
            means = {n: a / 2.0 for n, a in acc.items()}
            a, b = samples
            for vel in "uvw":
                for c in "TS":
                    want = np.full(shapes[vel], (a[vel] - b[vel]) * (a[c] - b[c]) / 4.0)
                    if vel == "v":
                        want[:, 0] = 0.0                 # the southern wall row
                        want[:, Ny:] = 0.0               # the northern wall row (a folded grid holds none)
                    if vel == "w":
                        want[:, :, 0] = want[:, :, Nz] = 0.0
                    got = eddy_flux(means, vel + c)
                    assert got.shape == shapes[vel] and np.array_equal(got, want), (vel + c, byv, steady)
                    assert steady == (not got.any())
            uu, vv = (a["u"] - b["u"]) ** 2 / 4.0, (a["v"] - b["v"]) ** 2 / 4.0
            eke = eddy_kinetic_energy(means)
            want = np.full((Nx, Ny, Nz), 0.25 * ((uu + uu) + (vv + vv)))
            if byv == Ny:
                want[:, Ny - 1] = 0.25 * ((uu + uu) + (vv + 0.0))     # (no row of faces beyond the last row of cells)
            assert np.array_equal(eke, want) and steady == (not eke.any())
            assert np.array_equal(tracer_variance(means, "T"), np.full(shapes["T"], (a["T"] - b["T"]) ** 2 / 4.0))
    # x wraps periodically: a tracer that differs in column Nx - 1 enters the flux of column 0
    T = np.zeros((Nx, Ny, Nz))
    T[Nx - 1] = 8.0
    means = {"u": np.ones((Nx, Ny, Nz)), "T": T, "uT": np.zeros((Nx, Ny, Nz))}
    f = eddy_flux(means, "uT")
    assert (f[0] == -4.0).all() and (f[Nx - 1] == -4.0).all() and (f[1:Nx - 1] == 0).all()
    with pytest.raises(ValueError):
        eddy_flux(means, "Tu")


def test_gather_averages_of_hand_cut_parts():
    rng = np.random.default_rng(7)
    Nx, Ny, Nz = 12, 8, 3
    for rows in (Ny, Ny + 1):                   # a cell-centred quantity; the rows of v below a wall
        whole = rng.standard_normal((Nx, rows, Nz))
        parts, offsets = [], []
        for ry, (j0, j1) in enumerate(((0, 4), (4, rows))):      # (only the northern band holds the wall row)
            for i0 in (0, 4, 8):
                parts.append(whole[i0:i0 + 4, j0:j1].copy())
                offsets.append((i0, j0))
        order = rng.permutation(len(parts))
        got = gather_averages([parts[q] for q in order], [offsets[q] for q in order])
        assert got.shape == whole.shape and got.tobytes() == whole.tobytes()


@pytest.fixture(scope="module", params=["Float32", "Float64"])
def lib(request):
    gb.build_library()
    return binding.load_library(request.param)


def test_the_abi_on_a_handle_without_a_device(lib):
    """gb25_create without a device hands out a handle that knows its configuration: the dims need no more; gb25_averages_begin
    checks its arguments and then fails with GB25_ERR_NO_DEVICE like the other device diagnostics -- there is no CPU fallback
    behind the ABI; everything else is GB25_ERR_STATE before a successful begin."""
    import torch
    INVALID, STATE, NO_DEVICE = 1, 5, 4
    assert C.sizeof(binding.AveragesInfo) == lib.gb25_averages_info_bytes() == 64
    assert list(binding.AVERAGE_IDS.values()) == list(range(17)) and tuple(binding.AVERAGE_IDS) == QUANTITIES
    d = (C.c_int32 * 3)()
    for grid_type, rows_of_v in ((0, 25), (1, 25), (4, 24)):
        cfg = binding.Config()
        lib.gb25_default_config(C.byref(cfg), 48, 24, 6)
        cfg.grid_type = grid_type
        h = C.c_void_p()
        st = lib.gb25_create(C.byref(cfg), C.byref(h))
        assert h and st == (0 if torch.cuda.is_available() else NO_DEVICE)
        for name, q in binding.AVERAGE_IDS.items():
            want = (48, rows_of_v if name[0] == "v" else 24, 1 if name.startswith("eta") else 7 if name[0] == "w" else 6)
            assert lib.gb25_average_dims(h, q, d) == 0 and tuple(d) == want, (grid_type, name)
        assert lib.gb25_average_dims(h, 17, d) == INVALID and lib.gb25_average_dims(h, -1, d) == INVALID
        assert lib.gb25_average_dims(h, 0, None) == INVALID and lib.gb25_average_dims(None, 0, d) == INVALID
        for groups, k_first, k_count, word in ((0, 0, -1, b"groups"), (2, 0, -1, b"groups"), (6, 0, -1, b"groups"), (8, 0, -1, b"groups"),
                                               (-1, 0, -1, b"groups"), (7, 6, 1, b"k_first"), (7, 4, 3, b"k_count"), (7, -1, 1, b"k_first"),
                                               (7, 0, 0, b"k_count"), (7, 0, -2, b"k_count")):
            assert lib.gb25_averages_begin(h, groups, k_first, k_count) == INVALID, (groups, k_first, k_count)
            assert word in lib.gb25_last_error_string(h), (groups, k_first, k_count)
        info = binding.AveragesInfo()
        assert lib.gb25_averages_get_info(h, C.byref(info)) == 0 and info.groups == 0 and info.samples == 0
        host = (C.c_double * (48 * 25 * 7))()
        p = C.c_void_p()
        if not torch.cuda.is_available():
            assert lib.gb25_averages_begin(h, 7, 0, -1) == NO_DEVICE and b"no device" in lib.gb25_last_error_string(h)
            assert lib.gb25_averages_begin(h, 1, 5, 1) == NO_DEVICE
            assert lib.gb25_averages_accumulate(h, 1.0) == STATE and b"gb25_averages_begin" in lib.gb25_last_error_string(h)
            assert lib.gb25_get_average(h, 0, 0, host, 48 * 24 * 6) == STATE
            assert lib.gb25_average_device_ptr(h, 0, C.byref(p), d) == STATE
            assert lib.gb25_get_average(h, 17, 0, host, 1) == INVALID and lib.gb25_get_average(h, 0, 0, None, 1) == INVALID
            assert lib.gb25_averages_end(h) == 0
        lib.gb25_destroy(h)


def test_the_public_names_and_no_cpu_fallback():
    import torch
    for name in ("averages", "run_averaged", "Averages", "AveragesHost", "average_terms", "eddy_flux", "eddy_kinetic_energy",
                 "tracer_variance", "gather_averages"):
        assert callable(getattr(gb, name)), name
    for name in ("averages_begin", "averages_accumulate", "averages_info", "average_dims", "get_average", "averages_end"):
        assert callable(getattr(binding.HipBackend, name)), name
    from gb25_amd.distributed import LocalSlabEnsemble
    for name in ("averages_begin", "averages_sample", "average"):
        assert callable(getattr(LocalSlabEnsemble, name)), name
    if not torch.cuda.is_available():
        # a HIP model cannot even be made without a device: gb.averages has nothing to fall back to
        with pytest.raises(gb.GB25Error, match="no HIP device"):
            gb.averages(gb.baroclinic_instability_model(gb.GPU(), 32, 16, 8, dt=1.0))
