"""The CATKE closure on the device, cell by cell: tests/catke_spec.py (proved on the CPU oracle by tests/test_catke_spec.py, whose
inputs and drive are used here) applied to the fields a caller reads around ONE update_state and one time_step, in both builds.

Per case, after the judged update_state every interior cell within its C_<field> (catke_spec; r in units of the build's u):
G^-.e (the total tendency k_catke_tke_step leaves), L^e, e (the e slice of k_implicit_vertical_var<.., 1> / _stream: e* rebuilt
from the device's own G^-.e, the spec's kappa_e and L^e), kappa_u, kappa_c, kappa_e (from the new e as the device holds it);
previous_u, previous_v equal u, v bit for bit, halos included; J^b keeps its bits (dt_since = 0; land: zero).  After the
time_step J^b against the filter from the fields read after the step and the J^b read before it.  Exact zeros: bottom and top
faces of the three kappa, faces touching the solid, L^e in dry cells, J^b and the surface source on land.

Outside the interior, exactly this table (catke_spec.outside_table; read off k_catke_tke_step's and k_catke_diffusivities' put /
store_x_images, k_catke_surface_flux, k_catke_fold and the host path catke_tke_step_impl / catke_diffusivities_finish_impl):
    kappa_u, kappa_c, kappa_e   face levels 0 .. Nz: the H periodic x images of every written row;
    L^e                         levels 0 .. Nz-1 likewise; its bottom / top layer (levels -1, Nz) on interior rows, with x images;
    J^b                         the x images;
    beside a wall               one y layer from the neighbouring interior row, with the x images of that layer (corners included);
    folded grid                 the H rows beyond the pivot row over every parent column, (i, Ny-1+q) <- (Nx-1-i mod Nx, Ny-1-q): the
                                three kappa on face levels 0 .. Nz, L^e on levels -1 .. Nz with clamped sources, J^b;
images equal their source bit for bit and every other parent cell keeps the noise it was given.

Forms (form_of; the chunk count is the rule of catke_level_chunks written out a second time and compared with FORMS below):
Nz 6, 15 one chunk, e in place; 17 two chunks (9 + 8) and the scratch e* / ImplicitVarFields::src_e from there on; 33 four (last
of 6); 64 eight of 8; 65 eight of 9 (last of 2).  The e solve: var<32> up to 32 levels, then var<48>, var<64>, stream above 64
in Float32; stream above 32 in Float64.  (70, 13, Nz): one ragged 64-wide block, odd Ny, a one-row last block of the 64 x 4 launch.

Not covered: the single-chunk form at Nz >= 16 (600 000 columns and more; the same code as Nz < 16: tests/test_gpu_fullsize.py);
slabs and mesh ranks, which compute kappa in the first halo column / row (test_catke_on_slabs_is_the_single_domain_bit_for_bit
ties them to the single domain judged here); MODE 0 and the T / S slice of MODE 1 (tests/test_gpu_implicit.py); a build with
GB25_CATKE_FAST=1; the advection of e by k_tracer_tendencies_single beyond the still case."""
import numpy as np
import pytest

import gb25_amd as gb
import catke_spec as cs
import step_spec as ss
import test_catke_spec as tcs

pytestmark = pytest.mark.gpu

BUILDS = ["Float32", "Float64"]
FORMS = {6: (1, "var<32>", "var<32>"), 15: (1, "var<32>", "var<32>"), 17: (2, "var<32>", "var<32>"), 33: (4, "var<48>", "stream"),
         64: (8, "var<64>", "stream"), 65: (8, "stream", "stream")}      # Nz: (chunks, Float32 e solve, Float64 e solve)
CASES = [(ft, grid, Nz) for ft in BUILDS for grid in ("flat", "made") for Nz in (6, 15, 17, 33, 64, 65)]
CASES += [(ft, grid, Nz) for ft in BUILDS for grid in ("islands", "folded") for Nz in (6, 33, 65)]


def driven(float_type, grid, Nz, **kw):
    shape = tcs.shape_of(grid, Nz, device=True)
    chunks, solve = tcs.form_of(float_type, Nz, shape[0] * shape[1])
    assert (chunks, solve) == (FORMS[Nz][0], FORMS[Nz][1 if float_type == "Float32" else 2])
    m, case = tcs.drive(gb.GPU(float_type=float_type), grid, shape, **kw)
    return m, case, f"{float_type} {grid} Nz {Nz}: {chunks} chunk{'s' if chunks > 1 else ''}, e solve {solve}"


@pytest.mark.parametrize("float_type,grid,Nz", CASES)
def test_the_closure_cell_by_cell(float_type, grid, Nz):
    m, case, label = driven(float_type, grid, Nz)
    try:
        assert m.backend.dtype == (np.float32 if float_type == "Float32" else np.float64)
        if grid != "flat":
            assert (case["g"]["kbot"] > 0).any() and (case["g"]["kbot"] == 0).any(), "an immersed grid must have wet and dry cells"
        res, left = tcs.check_case(label, case, strict=False)
        tcs.report(label, res)
        worst = max(res, key=lambda n: res[n] / cs.C[n])
        assert res[worst] <= cs.C[worst], f"{label}: {worst} is {res[worst]:.4g} u of its scale away from the spec; the bound is {cs.C[worst]:.4g}"
    finally:
        m.backend.close()


@pytest.mark.parametrize("grid", ["flat", "folded"])
@pytest.mark.parametrize("float_type", BUILDS)
def test_the_edge_columns_read_the_halo_cells_of_kappa_u(float_type, grid):
    """Other noise in the halo cells of the old kappa_u: G^-.e changes in the edge columns (and in the row under the fold), and
    nowhere else by a bit."""
    runs = []
    for halo_seed in (None, 1):
        m, case, label = driven(float_type, grid, 17, halo_seed=halo_seed, step=False)
        try:
            cs.judge_update(label, case["x"], case["got"], fields=("Gm.e",))
            runs.append(case)
        finally:
            m.backend.close()
    g = runs[0]["g"]
    H, Nx, Ny = g["H"], g["Nx"], g["Ny"]
    ku = [c["before"]["kappa_u"] for c in runs]
    assert tcs.bits_equal(ku[0][H:H + Nx, H:H + Ny], ku[1][H:H + Nx, H:H + Ny]) and not np.array_equal(ku[0][H - 1], ku[1][H - 1])
    a, b = (ss.interior(c["got"]["Gm.e"], g) for c in runs)
    # (beside a wall the y face carries v = 0, now and before: its kappa_u multiplies nothing, and the row keeps its bits)
    walls = ("j = 0",) if g["folded"] else ("j = 0", "j = Ny-1")
    for name, edge in (("i = 0", np.s_[0, 1:-1]), ("i = Nx-1", np.s_[-1, 1:-1]), ("j = 0", np.s_[1:-1, 0]), ("j = Ny-1", np.s_[1:-1, -1])):
        if name in walls:
            assert tcs.bits_equal(a[edge], b[edge]), f"{label}: Gm.e at {name} depends on kappa_u beyond the wall"
        else:
            assert not np.array_equal(a[edge], b[edge]), f"{label}: Gm.e at {name} does not read the halo cells of kappa_u beside it"
    assert tcs.bits_equal(a[1:-1, 1:-1], b[1:-1, 1:-1]), f"{label}: the halo cells of kappa_u reach the interior away from the edge"


@pytest.mark.parametrize("grid", tcs.GRIDS)
@pytest.mark.parametrize("float_type", BUILDS)
def test_the_still_case(float_type, grid):
    m, case, label = driven(float_type, grid, 17, still=True, step=False)
    try:
        tcs.check_still(label + " still", case)
    finally:
        m.backend.close()


@pytest.mark.parametrize("float_type", BUILDS)
def test_stale_e_halos_change_no_interior_cell(float_type):
    """catke_stale_e_halos = 1 leaves the halos of e unfilled after the e step: no interior cell of the judged call changes by a bit
    (the next step's advection of e reads those halos, which is the option's point and is not compared)."""
    runs = []
    for options in ({}, dict(catke_stale_e_halos=1)):
        m, case, label = driven(float_type, "flat", 17, step=False, **options)
        try:
            if options:
                assert m.backend.get_option("catke_stale_e_halos") == 1
            runs.append(case)
        finally:
            m.backend.close()
    g = runs[0]["g"]
    for n in tcs.JUDGED + ("Jb", "previous_u", "previous_v"):
        assert tcs.bits_equal(ss.interior(runs[0]["got"][n], g), ss.interior(runs[1]["got"][n], g)), f"{label}: {n} depends on catke_stale_e_halos"
