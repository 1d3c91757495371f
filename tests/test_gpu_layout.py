"""What the layout of a model (csrc/model_layout.hpp) looks like from outside the library: the extents gb25_field_dims reports and
gb25_get_field fills, field by field on four small models, written out here; the default chunking of a narrow model; and that a
configuration gb25_create refuses leaves nothing on the device.  No time step is made."""
import pytest

from gb25_amd.binding import FIELD_IDS, GB25Error, HipBackend

pytestmark = pytest.mark.gpu

CENTRE_3D = ("u", "T", "S", "pHY", "Gn.u", "Gn.T", "Gn.S", "Gm.u", "Gm.T", "Gm.S")
FACE_Y_3D = ("v", "Gn.v", "Gm.v")
CENTRE_2D = ("eta", "U", "eta_bar", "U_bar", "Gn.U")
FACE_Y_2D = ("V", "V_bar", "Gn.V")
CLOSURE = dict(centre_3d=("e", "Gn.e", "Gm.e", "Le", "previous_u"), face_y_3d=("previous_v",), face_z=("kappa_u", "kappa_c", "kappa_e"),
               centre_2d=("Jb",))


def shapes(kinds, closure):
    """name -> (with halos, without) from one pair per kind of field"""
    plain = dict(centre_3d=CENTRE_3D, face_y_3d=FACE_Y_3D, face_z=("w",), centre_2d=CENTRE_2D, face_y_2d=FACE_Y_2D)
    out = {}
    for names_of in (plain, CLOSURE) if closure else (plain,):
        for kind, names in names_of.items():
            for n in names:
                out[n] = kinds[kind]
    return out


# (Nx, Ny, Nz), the keywords of the model, CATKE on, and the extents (with halos, without) by kind of field
MODELS = {
    # a wall at the northern edge: v has the row Ny
    "lat_lon": ((40, 21, 6), dict(), False,
                dict(centre_3d=((56, 37, 22), (40, 21, 6)), face_y_3d=((56, 38, 22), (40, 22, 6)), face_z=((56, 37, 23), (40, 21, 7)),
                     centre_2d=((56, 37, 1), (40, 21, 1)), face_y_2d=((56, 38, 1), (40, 22, 1)))),
    "lat_lon_catke": ((40, 21, 6), dict(), True,
                      dict(centre_3d=((56, 37, 22), (40, 21, 6)), face_y_3d=((56, 38, 22), (40, 22, 6)), face_z=((56, 37, 23), (40, 21, 7)),
                           centre_2d=((56, 37, 1), (40, 21, 1)), face_y_2d=((56, 38, 1), (40, 22, 1)))),
    # a fold: the faces beyond the last row of cells are halo cells, v has Ny rows (substeps = 12: 8 effective ones, Ny >= 11)
    "tripolar": ((40, 24, 6), dict(grid_type=3, substeps=12), False,
                 dict(centre_3d=((56, 40, 22), (40, 24, 6)), face_y_3d=((56, 40, 22), (40, 24, 6)), face_z=((56, 40, 23), (40, 24, 7)),
                      centre_2d=((56, 40, 1), (40, 24, 1)), face_y_2d=((56, 40, 1), (40, 24, 1)))),
    # a slab that is its own neighbour, halo 4 (substeps = 12: wide halos of 8 + 1 + 4 = 13 columns fit its 40)
    "self_ring": ((40, 21, 6), dict(slab_mode=1, halo=4, substeps=12), False,
                  dict(centre_3d=((48, 29, 14), (40, 21, 6)), face_y_3d=((48, 30, 14), (40, 22, 6)), face_z=((48, 29, 15), (40, 21, 7)),
                       centre_2d=((48, 29, 1), (40, 21, 1)), face_y_2d=((48, 30, 1), (40, 22, 1)))),
}


@pytest.mark.parametrize("name", list(MODELS))
def test_field_dims_and_the_shapes_of_get_field(name):
    size, kw, catke, kinds = MODELS[name]
    want = shapes(kinds, catke)
    b = HipBackend(*size, dt=600.0, **kw)
    try:
        if catke:
            b.set_catke(True)
        assert set(want) == {n for n in FIELD_IDS if catke or n not in sum(CLOSURE.values(), ())}
        for n, (with_halos, without) in want.items():
            assert (b.field_dims(n, True), b.field_dims(n, False)) == (with_halos, without), (name, n)
            assert (b.get_field(n, True).shape, b.get_field(n, False).shape) == (with_halos, without), (name, n)
        if not catke:
            for n in sum(CLOSURE.values(), ()):
                with pytest.raises(GB25Error, match="gb25_field_dims: status 1"):
                    b.field_dims(n, True)
    finally:
        b.close()


def test_a_narrow_model_marches_chunks_of_12_levels_and_accepts_both_chunkings():
    b = HipBackend(150, 70, 24, dt=600.0)   # 3 * 18 * 1 blocks with chunks of 24 levels: far from four rounds of 1024
    try:
        assert b.get_option("momentum_chunk_levels") == 12 and b.get_option("tracer_chunk_levels") == 12
        for levels in (24, 12):
            b.set_option("momentum_chunk_levels", levels)
            b.set_option("tracer_chunk_levels", levels)
            assert (b.get_option("momentum_chunk_levels"), b.get_option("tracer_chunk_levels")) == (levels, levels)
    finally:
        b.close()


def test_a_refused_configuration_leaves_nothing_on_the_device():
    """gb25_create plans and refuses before it touches the device: after the "even Nx" and the "barotropic halo" refusals of
    test_gpu_parity.py::test_error_paths the free device memory is what it was, to the byte."""
    import torch
    HipBackend(32, 16, 8, dt=1.0).close()   # (the library's runtime is up before the first reading)
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info()[0]
    with pytest.raises(GB25Error, match="even Nx"):
        HipBackend(33, 16, 8, dt=1.0, grid_type=4)
    with pytest.raises(GB25Error, match="barotropic halo"):
        HipBackend(16, 16, 8, dt=1.0, grid_type=3, slab_mode=1)
    assert torch.cuda.mem_get_info()[0] == before
