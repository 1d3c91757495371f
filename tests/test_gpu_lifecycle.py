"""gb25_create / gb25_destroy give back what a model took: six lives of a model that has switched on everything that allocates
lazily -- CATKE, a top flux, the bottom drag, a prescribed atmosphere, a bottom height, time averages, particles -- and has made two
steps, so that the look-ahead buffers have exchanged names.  The free device memory after the sixth life is that after the second,
to within ONE 3-D field of the model: a field leaked per life would show four times over.  A block freed twice leaves a HIP error
behind, which the launches of the next life (and of one more model at the end) report."""
import numpy as np
import pytest
import torch

from gb25_amd.binding import HipBackend
from gb25_amd.data_free import ATMOSPHERE_FIELDS
from gb25_amd.distributed import LocalSlabEnsemble

pytestmark = pytest.mark.gpu
Nx, Ny, Nz, H = 128, 64, 8, 8
ATMOSPHERE = dict(u=3.0, v=-1.0, T=288.15, q=0.005, p=101325.0, shortwave=-300.0, longwave=-350.0)


def bottom_height():
    """a ridge along every parallel and land over the two poles of a folded grid: the two copies of a pivot-row cell (columns i
    and Nx - 1 - i) share their bottom"""
    zb = np.repeat(-4000.0 + 2500.0 * np.sin(np.pi * (np.arange(Ny) + 0.5) / Ny)[None, :] ** 8, Nx, axis=0)
    for ip in (0, Nx // 2):
        for di in (-2, -1, 0, 1):
            zb[(ip + di) % Nx, Ny - 6:] = 100.0
    return zb


def switch_everything_on(b):
    b.set_catke(True)
    b.set_bottom_drag(0.003)
    d = b.field_dims("T", False)
    b.set_top_flux("T", np.full((d[0], d[1]), 1e-5))
    for n in ATMOSPHERE_FIELDS:
        b.set_prescribed_atmosphere(n, np.full((b.Nx_local + 2 * H, b.Ny_local + 2 * H), ATMOSPHERE[n]))
    b.set_bottom_height(bottom_height())
    b.set_baroclinic_instability()
    b.averages_begin()


def one_life(kind):
    if kind == "slabs":
        ens = LocalSlabEnsemble(Nx, Ny, Nz, 2, dt=60.0)
        for b in ens.backends:
            switch_everything_on(b)
        ens.particles_begin(np.array([3, 70]), np.array([10, 40]), np.array([Nz - 1, Nz - 1]))   # (wet cells: the top level)
        ens.first_time_step()
        ens.time_step()
        ens.synchronize()
        ens.close()
        return
    b = HipBackend(Nx, Ny, Nz, dt=60.0, grid_type=3 if kind == "tripolar" else 0)
    switch_everything_on(b)
    b.particles_begin(16)
    b.particles_set([3, 70], [10, 40], [Nz - 1, Nz - 1], [0.5, 0.5], [0.5, 0.5], [0.5, 0.5])
    b.first_time_step()
    b.time_step()
    b.synchronize()
    b.close()


@pytest.mark.parametrize("kind", ["lat_lon", "tripolar", "slabs"])
def test_six_lives_of_a_model_leave_the_device_memory_as_it_was(kind):
    field_bytes = ((Nx // 2 if kind == "slabs" else Nx) + 2 * H) * (Ny + 2 * H) * (Nz + 2 * H) * 4
    free = {}
    for life in range(1, 7):
        one_life(kind)
        if life in (2, 6):
            torch.cuda.synchronize()
            free[life] = torch.cuda.mem_get_info()[0]
    grown = free[2] - free[6]
    print(f"{kind}: free after life 2: {free[2]}, after life 6: {free[6]}, grown by {grown} bytes; one 3-D field: {field_bytes}")
    assert grown < field_bytes
    last = HipBackend(8, 8, 4, dt=60.0)   # (a HIP error the sixth destroy left behind would fail this model's launches)
    last.fill_halo_regions()
    last.synchronize()
    last.close()
