"""Host-side mirror of the GordonBell25 model API for the HydrostaticFreeSurfaceModel hot path.

Mirrors (names, argument meaning, mutation-in-place semantics):
  baroclinic_instability_model(arch, Nx, Ny, Nz; dt, halo, ...)  GB-25 src/baroclinic_instability_model.jl:17-85
  first_time_step!(model) / time_step!(model) / loop!(model, Ninner)  src/timestepping_utils.jl:21-45
  set_baroclinic_instability!(model)                              src/model_utils.jl:120-127
  the *_workload! phase wrappers                                   src/precompile.jl:44-127
Julia's `!` suffix is dropped.  The model object exposes Oceananigans-shaped accessors
(model.velocities.u, model.tracers.T, model.free_surface.eta, model.timestepper.Gn.u,
model.clock, model.grid) whose `parent` / `interior` arrays have the Oceananigans layout.

The numerical engine is injected as a *backend* object (binding.HipBackend in the product).
"""
from types import SimpleNamespace

import numpy as np


class Field:
    """View of one model field: `parent` includes halos (Oceananigans `parent(field)`),
    `interior` does not.  Index order is [i, j, k]; arrays are copies fetched from the device."""

    def __init__(self, backend, name, location):
        self._b, self.name, self.location = backend, name, location

    @property
    def parent(self):
        return self._b.get_field(self.name, True)

    @property
    def interior(self):
        return self._b.get_field(self.name, False)

    def stats(self, include_halos=False):
        """min, max, max|x| and where, sums and non-finite count, reduced on the device (binding.FieldStats)."""
        return self._b.field_stats(self.name, include_halos)

    def _moments(self, shape):
        if hasattr(self._b, "integrate_field"):
            return self._b.integrate_field(self.name, shape)
        from .integrals import integrate_host       # (a backend without the device reduction)
        return integrate_host(self._b, self.name, shape)

    def integral(self):
        """The field integrated over the wet interior with the cell measure of include/gb25.h (volume for a 3-D field, area
        for a 2-D one), reduced on the device: one record -- measure, first = the integral, second, points, nonfinite."""
        return self._moments("total")

    def horizontal_mean(self):
        """The measure-weighted mean of every level, [k] (NaN where a level has no wet point)."""
        r = self._moments("levels")
        with np.errstate(invalid="ignore", divide="ignore"):
            return r["first"] / r["measure"]

    def zonal_mean(self):
        """The measure-weighted mean of every row, [j, k] (NaN where a row has no wet point)."""
        r = self._moments("rows")
        with np.errstate(invalid="ignore", divide="ignore"):
            return r["first"] / r["measure"]

    def levels(self, k_first, k_count=1):
        """Interior levels [k_first, k_first + k_count) (0-based; k_count = -1: all from k_first on) as [i, j, k]: gathered on the
        device and copied once -- the parent array does not cross PCIe, nothing is pinned."""
        if hasattr(self._b, "get_field_levels"):
            return self._b.get_field_levels(self.name, k_first, k_count)
        a = self._b.get_field(self.name, False)       # (a backend without the device gather)
        return a[:, :, k_first:(None if k_count == -1 else k_first + k_count)]

    def surface(self):
        """The top interior level, [i, j, 1]: `indices = (:, :, Nz)` of the reference's surface writer."""
        return self.levels(self._b.field_dims(self.name, False)[2] - 1, 1)

    def at_depths(self, depths):
        """(values [i, j, n], status uint8 [i, j, n]): this field (T, S or e) interpolated to the fixed depths `depths` [m,
        positive] between cell centres, on the device (at_depths of this module)."""
        return _on_surfaces(self._b, "depth", self.name, depths)

    def coarsen(self, block):
        """The measure-weighted mean over boxes of block = (bx, by, bz) points, [I, J, K], reduced on the device (coarsen of
        this module)."""
        return _block_sums(self._b, self.name, block).mean()

    def filtered(self, radius, kernel="box", stride=(1, 1)):
        """The field smoothed by a moving window of radius = (rx, ry) grid points, measure-weighted, [I, J, K], on the device
        (filtered of this module)."""
        return _filter_sums(self._b, self.name, radius, kernel, stride).mean()

    def gradient_magnitude(self, levels=None):
        """|grad_h| of this field (T or S) at (c,c,c), [i, j, k], on the device (gradient_magnitude of this module)."""
        if self.name not in ("T", "S"):
            raise ValueError(f"gradient_magnitude: T or S, not {self.name!r}")
        from .kinematics import kinematics
        return kinematics(self._b, "gradient", self.name, levels)

    def regions(self, below=None, above=None, levels=None, carry=None, max_regions=4096):
        """The connected regions of every level where this field (T, S or e) lies below (or above) a threshold, labelled and
        measured on the device (regions of this module)."""
        from .regions import regions
        return regions(self._b, self.name, below=below, above=above, levels=levels, carry=carry, max_regions=max_regions)

    def zonal_spectrum(self, wavenumbers=None, levels=None):
        """(X [level, row, m] complex128, nonfinite_lines): the zonal wavenumber coefficients of every interior line, computed
        where the field lives (zonal_spectrum of this module)."""
        return _zonal_spectrum(self._b, self.name, wavenumbers, levels)

    def set(self, array, include_halos=False):
        a = np.asarray(array)
        if not include_halos and a.ndim >= 2:
            # A y-face field of a folded (tripolar) grid has Ny rows -- topology (Periodic, RightConnected, Bounded): the
            # faces beyond the last row of cells are halo cells.  An array shaped for a Bounded y (Ny + 1 rows) is
            # accepted and its last row, which the fold fill would overwrite anyway, is dropped.
            # Only there: a y-face field (v and its tendencies, V, G.V, ...) whose grid has no wall at the northern edge -- the
            # zipper fold, or a northern neighbour rank of a 2-D decomposition.  Any other array with a row too many is a
            # wrongly shaped array and is passed through, so that the backend rejects it.
            want = self._b.field_dims(self.name, False)
            y_face = self.name in ("v", "Gn.v", "Gm.v", "V", "V_bar", "Gn.V", "previous_v")
            no_wall = y_face and want[1] == self._b.field_dims("T", False)[1]      # (a Bounded y gives a y-face field one row more than a cell field)
            if no_wall and a.shape[0] == want[0] and a.shape[1] == want[1] + 1:
                a = np.ascontiguousarray(a[:, :want[1]])
        self._b.set_field(self.name, a, include_halos)

    def set_parent(self, array):
        self._b.set_field(self.name, array, True)

    @property
    def shape(self):
        return self._b.field_dims(self.name, False)

    def __repr__(self):
        return f"Field({self.name!r} at {self.location}, interior {self.shape})"


class Clock:
    """model.clock (time, last_dt, iteration) -- src/model_utils.jl:150-155."""

    def __init__(self, backend):
        self._b = backend

    @property
    def time(self):
        return self._b.clock()[0]

    @property
    def iteration(self):
        return self._b.clock()[1]

    @property
    def last_dt(self):
        return self._b.clock()[2]

    @last_dt.setter
    def last_dt(self, dt):
        self._b.set_dt(dt)


class LatitudeLongitudeGrid:
    """simple_latitude_longitude_grid(arch, Nx, Ny, Nz; halo) -- src/model_utils.jl:56-65."""

    def __init__(self, backend, Nx, Ny, Nz, halo):
        self._b = backend
        self.Nx, self.Ny, self.Nz = Nx, Ny, Nz
        self.halo = (halo, halo, halo)
        self.latitude, self.longitude = (-80, 80), (0, 360)

    @property
    def size(self):
        return (self.Nx, self.Ny, self.Nz)

    def metric(self, name, index):
        """1-based index like the Julia sources; names: phif phic dxc dxf azc azf fcor zf zc dzc dzf."""
        return self._b.metric(name, index)

    def z_faces(self):
        return np.array([self.metric("zf", k) for k in range(1, self.Nz + 2)])


class HydrostaticFreeSurfaceModel:
    """The object baroclinic_instability_model returns."""

    def __init__(self, backend, Nx, Ny, Nz, halo):
        b = self.backend = backend
        self.grid = LatitudeLongitudeGrid(b, Nx, Ny, Nz, halo)
        self.clock = Clock(b)
        F = lambda n, loc: Field(b, n, loc)
        self.velocities = SimpleNamespace(u=F("u", "fcc"), v=F("v", "cfc"), w=F("w", "ccf"))
        self.tracers = SimpleNamespace(T=F("T", "ccc"), S=F("S", "ccc"))
        self.pressure = SimpleNamespace(pHY=F("pHY", "ccc"))
        self.free_surface = SimpleNamespace(
            eta=F("eta", "ccf"),
            barotropic_velocities=SimpleNamespace(U=F("U", "fc"), V=F("V", "cf")),
            filtered_state=SimpleNamespace(eta=F("eta_bar", "ccf"), U=F("U_bar", "fc"), V=F("V_bar", "cf")),
            substeps=30, gravitational_acceleration=9.80665)
        G = lambda p: SimpleNamespace(u=F(p + ".u", "fcc"), v=F(p + ".v", "cfc"), T=F(p + ".T", "ccc"),
                                      S=F(p + ".S", "ccc"))
        Gn = G("Gn")
        Gn.U, Gn.V = F("Gn.U", "fc"), F("Gn.V", "cf")
        self.timestepper = SimpleNamespace(Gn=Gn, Gm=G("Gm"), chi=0.1)

        self.closure = None
        self.diffusivity_fields = None

    def enable_catke_fields(self):
        """closure = CATKEVerticalDiffusivity(): tracers = (:T, :S, :e) and model.diffusivity_fields
        (src/baroclinic_instability_model.jl:50-51, src/correctness.jl:60-67)."""
        b = self.backend
        F = lambda n, loc: Field(b, n, loc)
        self.tracers.e = F("e", "ccc")
        self.timestepper.Gn.e, self.timestepper.Gm.e = F("Gn.e", "ccc"), F("Gm.e", "ccc")
        self.diffusivity_fields = SimpleNamespace(kappa_u=F("kappa_u", "ccf"), kappa_c=F("kappa_c", "ccf"),
                                                  kappa_e=F("kappa_e", "ccf"), Le=F("Le", "ccc"), Jb=F("Jb", "cc"))

    # Oceananigans.fields(model): the set compare_states walks (src/correctness.jl:34-35)
    def fields(self):
        out = {"u": self.velocities.u, "v": self.velocities.v, "w": self.velocities.w,
               "eta": self.free_surface.eta, "T": self.tracers.T, "S": self.tracers.S}
        if hasattr(self.tracers, "e"):
            out["e"] = self.tracers.e
        return out

    def prognostic_fields(self):
        fs = self.free_surface
        return {"u": self.velocities.u, "v": self.velocities.v, "eta": fs.eta,
                "U": fs.barotropic_velocities.U, "V": fs.barotropic_velocities.V,
                "T": self.tracers.T, "S": self.tracers.S}

    def set(self, **kw):
        """set!(model, u=..., v=..., T=..., S=..., eta=...) with interior-shaped arrays."""
        allf = {**self.fields()}
        for k, v in kw.items():
            allf[k].set(v)

    def synchronize(self):
        self.backend.synchronize()

    def checkpoint(self, directory, label="checkpoint", wait=True):
        """Snapshot the restart set on the device and (wait=True) write <directory>/<label>/restart_rank<R>.gb25; wait=False
        returns a handle whose .write() finishes the checkpoint while the model steps on (gb25_amd/restart.py)."""
        from .restart import checkpoint
        return checkpoint(self, directory, label, wait)

    def __repr__(self):
        Nx, Ny, Nz = self.grid.size
        return (f"HydrostaticFreeSurfaceModel({Nx}x{Ny}x{Nz} LatitudeLongitudeGrid, halo {self.grid.halo}, "
                f"{np.dtype(getattr(self.backend, 'dtype', np.float32)).name}, MI355X)")


def budget(model):
    """Volume, heat, salt, kinetic energy and the free surface's volume and potential energy, integrated over the wet interior
    on the device (binding.Budget; include/gb25.h gb25_get_budget): `print(budget(model))`."""
    return model.backend.budget()


def _derived(model, name, param=None, levels=None):
    b = model.backend
    if hasattr(b, "get_derived"):
        return b.get_derived(name, param, levels)
    from . import derived as host                     # (a backend without the device kernels: the numpy restatement)
    if name == "vorticity":
        return host.vorticity_host(b, levels)
    if name == "kinetic_energy":
        return host.kinetic_energy_host(b, levels)
    raise NotImplementedError(f"{name} needs a backend with get_derived")


def vorticity(model, levels=None):
    """Vertical relative vorticity at (f,f,c) computed on the device (include/gb25.h, GB25_D_VORTICITY), [i, j, k] shaped like
    v's interior.  levels = (k_first, k_count), 0-based interior levels (k_count = -1: all from k_first on); only those levels
    are computed and copied: `vorticity(model, levels=(Nz - 1, 1))` is the surface."""
    return _derived(model, "vorticity", None, levels)


def kinetic_energy(model, levels=None):
    """Kinetic energy per unit mass at (c,c,c), (Ix u^2 + Iy v^2) / 2, on the device."""
    return _derived(model, "kinetic_energy", None, levels)


def density_anomaly(model, levels=None):
    """In-situ density rho(T, S, z) - rho0 (TEOS-10) at (c,c,c): what the hydrostatic pressure integrates; 0 in immersed cells."""
    return _derived(model, "density_anomaly", None, levels)


def potential_density(model, levels=None):
    """Potential density rho(T, S, 0) - rho0 referenced to the surface, at (c,c,c); 0 in immersed cells."""
    return _derived(model, "potential_density", None, levels)


def mixed_layer_depth(model, threshold=0.03):
    """Depth [m, positive] at which the potential density exceeds the top cell's by `threshold` kg/m^3, linearly interpolated
    between cell centres; the column's depth where it never does, 0 over land.  [i, j]."""
    return _derived(model, "mixed_layer_depth", threshold)[:, :, 0]


def _on_surfaces(b, variable, carried, values):
    from .surfaces import on_surfaces                # (the kernel, or the numpy restatement on a backend without it)
    return on_surfaces(b, variable, carried, values)


def isosurface_depth(model, variable, values):
    """(depth [i, j, n], status uint8 [i, j, n]): the depth [m, positive] at which `variable` -- "potential_density", "T" or
    "S" -- first takes each of `values` (1 .. 64 of them, in any order), marching down from the top and interpolating linearly
    between cell centres, on the device (include/gb25.h, gb25_get_on_surfaces): a sloping isopycnal is the baroclinic
    instability.  status: binding.SURFACE_STATUS -- found; outcrop: the surface lies above the top cell, depth = the top face;
    grounded: below the bottom cell, depth = the column's bottom face; dry: land, 0."""
    return _on_surfaces(model.backend, variable, "depth", values)


def on_isosurface(model, carried, of="potential_density", values=()):
    """(values [i, j, n], status): the quantity `carried` -- "T", "S", "e", "kinetic_energy", "density_anomaly",
    "potential_density" -- on the surfaces where `of` takes each of `values`; where a surface outcrops or is grounded, the value
    of the top or of the bottom cell."""
    return _on_surfaces(model.backend, of, carried, values)


def at_depths(model, carried, depths):
    """(values [i, j, n], status): `carried` at the fixed depths `depths` [m, positive], interpolated between cell centres -- the
    exponential vertical grid has no level at 300 m.  A depth at a cell centre returns that cell's value unchanged."""
    return _on_surfaces(model.backend, "depth", carried, depths)


def layer_thickness(model, variable, edges):
    """Thickness [m] of the layers between consecutive surfaces `variable` = edges[e], [i, j, len(edges) - 1]: differences of
    isosurface_depth (surfaces.layer_thickness)."""
    from .surfaces import layer_thickness as thickness
    return thickness(isosurface_depth(model, variable, edges)[0])


def _stability(model, kind, param, levels, host):
    from .stability import stability                 # (the kernel, or the numpy restatement on a backend without it)
    return stability(model.backend, kind, param, levels, **host)


def buoyancy_frequency(model, levels=None, **host):
    """N^2 [s^-2] at (Center, Center, Face), [i, j, face] with Nz + 1 faces, on the device (include/gb25.h, GB25_ST_N2): the
    stratification of the potential density referenced to the surface, -(g / rho0) d sigma / dz between two cell centres.  Faces
    0 and Nz and every face at or below the bottom are 0.  levels = (k_first, k_count) of the faces, 0-based (k_count = -1: all
    from k_first on); only those are computed and copied.  host: sigma = ... for a backend without the kernel and without
    get_derived (stability.stability_host)."""
    return _stability(model, "n2", None, levels, host)


def shear_squared(model, levels=None, **host):
    """The squared vertical shear (du/dz)^2 + (dv/dz)^2 [s^-2] of the velocities averaged to the cell centres, at (c,c,f)."""
    return _stability(model, "shear2", None, levels, host)


def richardson_number(model, shear_floor=1e-12, levels=None, **host):
    """Ri = N^2 / max(S^2, shear_floor) at (c,c,f).  shear_floor [s^-2] > 0 keeps a resting column finite; its default is a
    convention, not a measured number."""
    return _stability(model, "richardson", shear_floor, levels, host)


def eady_growth_rate(model, n2_floor=0.0, levels=None, **host):
    """The Eady growth rate 0.31 |f| / sqrt(Ri) = 0.31 |f| sqrt(S^2) / sqrt(N^2) [s^-1] at (c,c,f) where N^2 > n2_floor, 0
    elsewhere: how fast the baroclinic instability grows."""
    return _stability(model, "eady_rate", n2_floor, levels, host)


def ertel_pv(model, levels=None, **host):
    """The Ertel potential vorticity (f + zeta) N^2 + (du/dz db/dy - dv/dz db/dx) [s^-3] at (c,c,f); host: sigma = ...,
    vorticity = ... for a backend without the kernel."""
    return _stability(model, "ertel_pv", None, levels, host)


def baroclinic_wave_speed(model, **host):
    """The first baroclinic gravity-wave speed c1 = (1 / pi) integral of N dz [m/s] (WKB), [i, j]; 0 over land."""
    return _stability(model, "wave_speed", None, None, host)[:, :, 0]


def deformation_radius(model, **host):
    """The first baroclinic deformation radius [m], [i, j]: c1 / |f| poleward of 5 degrees, sqrt(c1 / (2 beta)) within 5 degrees
    of the equator, beta = 2 Omega cos(phi) / R, from baroclinic_wave_speed and the latitude of the cell centres.  An
    element-wise step in float64 on the HOST: it is not part of the bit-for-bit contract of the device diagnostics."""
    from .stability import cell_latitudes, deformation_radius_of
    b = model.backend
    return deformation_radius_of(baroclinic_wave_speed(model, **host), cell_latitudes(b), b.cfg.Omega, b.cfg.radius)


def eddy_resolution(model, **host):
    """deformation_radius / max(dx, dy) of every cell, [i, j]: the grid resolves the eddies where this is about 2 or more.
    Host arithmetic like deformation_radius."""
    from .stability import cell_spacings
    return deformation_radius(model, **host) / cell_spacings(model.backend)


def _kinematics(model, kind, param, levels, host):
    from .kinematics import kinematics               # (the kernel, or the numpy restatement on a backend without it)
    return kinematics(model.backend, kind, param, levels, **host)


def divergence(model, levels=None, **host):
    """The horizontal divergence du/dx + dv/dy [s^-1] at (c,c,c), [i, j, k], on the device (include/gb25.h,
    GB25_KIN_DIVERGENCE): the flux of u, v through the four faces of a cell over its area; 0 in the immersed cells.  levels =
    (k_first, k_count), 0-based (k_count = -1: all from k_first on); only those are computed and copied."""
    return _kinematics(model, "divergence", None, levels, host)


def normal_strain(model, levels=None, **host):
    """The normal strain rate du/dx - dv/dy [s^-1] at (c,c,c)."""
    return _kinematics(model, "normal_strain", None, levels, host)


def shear_strain(model, levels=None, **host):
    """The shear strain rate dv/dx + du/dy [s^-1] at (f,f,c), shaped like the vorticity: its stencil with the inner sign turned."""
    return _kinematics(model, "shear_strain", None, levels, host)


def okubo_weiss(model, levels=None, **host):
    """The Okubo-Weiss parameter W = s_n^2 + s_s^2 - zeta^2 [s^-2] at (c,c,c), the corner quantities averaged as squares to the
    cell: W < 0 in vortex cores, W > 0 in the strain-dominated filaments between them."""
    return _kinematics(model, "okubo_weiss", None, levels, host)


def rossby_number(model, levels=None, **host):
    """The local Rossby number zeta / f at (f,f,c), shaped like the vorticity; 0 where f is 0."""
    return _kinematics(model, "rossby_number", None, levels, host)


def gradient_magnitude(model, of, levels=None, **host):
    """|grad_h x| [x per m] at (c,c,c) of x = "T", "S" or "potential_density" (referenced to the surface, formed on the fly):
    centred differences that count a face into land or a wall as 0.  host: sigma = ... for a backend without get_derived."""
    return _kinematics(model, "gradient", of, levels, host)


def frontogenesis(model, of="potential_density", levels=None, **host):
    """The frontogenesis function F = -(gx^2 du/dx + gx gy (dv/dx + du/dy) + gy^2 dv/dy) at (c,c,c) of x = "T", "S" or
    "potential_density": the rate at which the horizontal flow sharpens (F > 0) or weakens the gradient of x."""
    return _kinematics(model, "frontogenesis", of, levels, host)


def _block_sums(b, source, block, levels=None, level_weights=None, param=None):
    from .blocks import block_sums                    # (the kernel, or the numpy restatement on a backend without it)
    return block_sums(b, source, block, levels, level_weights, param)


def coarsen(model, source, block, levels=None):
    """The measure-weighted mean of `source` -- a field name or "kinetic_energy", "density_anomaly", "potential_density",
    "mixed_layer_depth" -- over boxes of block = (bx, by, bz) points, [I, J, K] float64, reduced on the device (include/gb25.h,
    gb25_get_block_sums): the field on a 4x or 8x coarser grid, NaN where a box is all land.  levels = (k_first, k_count) of the
    field's own levels."""
    return _block_sums(model.backend, source, block, levels).mean()


def subgrid_variance(model, source, block):
    """The variance of `source` inside every box of block = (bx, by, bz) points, measure-weighted, [I, J, K]: what a coarser
    grid would not resolve."""
    return _block_sums(model.backend, source, block).variance()


def _column(model, source, depth_range):
    from .blocks import column_area, column_sums
    return column_sums(model.backend, source, depth_range), column_area(model.backend, source)


def column_integral(model, source, depth_range=None):
    """The vertical integral of `source` over the wet part of every column, [i, j] in units of the source times metres -- the
    column's sum of mu x over the column's area, Oceananigans' Integral(field, dims = 3) --, on the device.  depth_range = (top,
    bottom) [m, positive] restricts it, partial cells by their fraction (blocks.depth_weights); 0 over land."""
    sums, area = _column(model, source, depth_range)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(area > 0, sums.first[:, :, 0] / area, 0.0)


def depth_mean(model, source, depth_range=None):
    """The thickness-weighted mean of `source` over the wet part of every column, [i, j]; NaN where the column (or the range in
    it) is dry."""
    return _column(model, source, depth_range)[0].mean()[:, :, 0]


def heat_content(model, depth_range=None, heat_capacity=3991.86795711963, reference_temperature=0.0):
    """The heat content of every column [J m^-2], rho0 cp times the vertical integral of T - reference_temperature, [i, j]:
    `heat_content(model, depth_range=(0, 700))` is the heat content of the upper 700 m.  0 over land."""
    sums, area = _column(model, "T", depth_range)
    first = sums.first[:, :, 0] - reference_temperature * sums.measure[:, :, 0]
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(area > 0, (model.backend.cfg.rho0 * heat_capacity) * first / area, 0.0)


def _filter_sums(b, source, radius, kernel="box", stride=(1, 1), levels=None, length=None, param=None):
    from .filters import filter_sums, kernel_weights, rows_for_length   # (the kernels, or the numpy restatement on a backend without them)
    rx, ry = (int(q) for q in radius)
    rows = None if length is None else rows_for_length(b, source, length)
    wx = None if kernel == "box" or rows is not None else kernel_weights(kernel, rx)
    wy = None if kernel == "box" else kernel_weights(kernel, ry)
    return filter_sums(b, source, (rx, ry), stride, levels, wx, wy, rows, param)


def filtered(model, source, radius, kernel="box", stride=(1, 1), levels=None, length=None):
    """`source` -- a field name or "kinetic_energy", "density_anomaly", "potential_density", "mixed_layer_depth" -- smoothed level
    by level by a moving window of radius = (rx, ry) grid points around every stride-th point, measure-weighted, [I, J, K]
    float64, on the device (include/gb25.h, gb25_get_filter_sums): xbar of a scale separation, NaN where a window holds no wet
    point.  kernel: "box", "gaussian" or "triangle" (filters.kernel_weights).  The window wraps in x and is clipped at the
    southern and northern rows.  length [m]: every row gets the rx that makes its window about that wide (filters.rows_for_length;
    rx is then ignored and x is the box).  levels = (k_first, k_count) of the field's own levels."""
    return _filter_sums(model.backend, source, radius, kernel, stride, levels, length).mean()


def subfilter_variance(model, source, radius, kernel="box", stride=(1, 1), levels=None, length=None):
    """The variance of `source` inside the window of every output point, measure-weighted, [I, J, K]: what lies below the filter
    scale (of "u" and "v": twice the eddy kinetic energy below that scale, without a time mean).  Arguments as for filtered."""
    return _filter_sums(model.backend, source, radius, kernel, stride, levels, length).variance()


def eddy_part(model, source, radius, kernel="box", levels=None, length=None):
    """x' = x - xbar at every point (stride 1), [i, j, k] float64 over the rows of cell centres: the part of `source` below the
    filter scale.  NaN where the point itself is dry (its measure is 0) or its window is empty.  Arguments as for filtered."""
    from .filters import filter_sums, source_values
    b = model.backend
    sums = _filter_sums(b, source, radius, kernel, (1, 1), levels, length)
    own = filter_sums(b, source, (0, 0), (1, 1), levels).measure          # mu of the counted points
    k0 = 0 if levels is None else int(levels[0])
    x = np.asarray(source_values(b, source), np.float64)[:, :sums.dims[1], k0:k0 + sums.dims[2]]
    with np.errstate(invalid="ignore"):
        return np.where(own > 0, x - sums.mean(), np.nan)


def regions(model, source, below=None, above=None, levels=None, carry=None, max_regions=4096, param=None, labels=False):
    """The coherent regions of `source` -- "T", "S", "e"; "kinetic_energy", "density_anomaly", "potential_density"; "divergence",
    "normal_strain", "okubo_weiss", "gradient", "frontogenesis" (param: their tracer) -- below (or above) a threshold, level by
    level, labelled and measured on the device (include/gb25.h, gb25_get_regions): `regions(model, "okubo_weiss", below=-2e-11,
    levels=(Nz - 1, 1), carry="T")` counts the vortex cores of the surface.  4-connectivity, the x seam joined on a periodic grid,
    land and non-finite cells in the background.  Returns regions.Regions: .count, .records (one structured record per region:
    cells, key, box, wraps, measure, first, second, carried, centroid sums, extreme), .labels() (int32 [i, j, kk], -1: background;
    copied with the records only with labels=True, else when first asked for, which must be before the model is stepped again),
    .volume() [m^3], .area() [m^2], .mean(), .centroid(), .centroid_lonlat().  At most max_regions records per level are stored;
    .count is the true number."""
    from .regions import regions as regions_of         # (the kernels, or the numpy restatement on a backend without them)
    return regions_of(model.backend, source, below=below, above=above, levels=levels, carry=carry, max_regions=max_regions, param=param,
                      labels=labels)


def eddy_census(model, level=None, factor=0.2, carry=None, max_regions=4096, labels=False):
    """The vortex cores of one level (default: the surface) by the usual Okubo-Weiss criterion W < -factor * sigma_W, sigma_W the
    standard deviation of W over the wet cells of THAT level (regions.okubo_weiss_sigma: the level's plane of W is computed on
    the device and reduced on the host): regions.Regions."""
    from .regions import eddy_census as census
    return census(model.backend, level, factor, carry, max_regions, labels)


def _transport(model, faces, shape, window=None):
    b = model.backend
    if hasattr(b, "transport"):
        return b.transport(faces, shape, window)
    from .transports import transport_host          # (a backend without the device reduction)
    return transport_host(b, faces, shape, window)


def meridional_transport(model, window=None):
    """Volume [m^3/s], heat [degC m^3/s] and salt [(g/kg) m^3/s] transport across every row of y faces, integrated over depth
    and over the columns of `window` = (first i, count) (None: the whole row), reduced on the device (include/gb25.h,
    gb25_get_transport): records [j] with members area, volume, heat, salt, faces, nonfinite."""
    return _transport(model, "across_y", "profile", window)


def overturning(model, window=None):
    """The meridional overturning streamfunction psi [j, kf] in m^3/s at the Nz + 1 z faces of every row of y faces: the
    northward volume transport accumulated from the bottom, 0 at kf = 0 (divide by 1e6 for Sverdrups)."""
    return _transport(model, "across_y", "streamfunction", window)["volume"]


def heat_transport(model, rho0_cp=1020.0 * 3991.86795711963, window=None):
    """The meridional heat transport [W] across every row of y faces, [j]: rho0 cp times the depth-integrated sum of
    a v T (reference density and heat capacity of ClimaOcean's ocean_simulation by default)."""
    return rho0_cp * meridional_transport(model, window)["heat"]


def section_transport(model, i, j_range=None):
    """The transport through the x faces of column i (0-based interior) between the rows of j_range = (first j, count)
    (None: every row), integrated over depth: one record -- area, volume, heat, salt, faces, nonfinite."""
    return _transport(model, "across_x", "profile", j_range)[i]


def _class_sums(model, what, variable, edges, shape, window=None):
    b = model.backend
    if hasattr(b, "class_sums"):
        return b.class_sums(what, variable, edges, shape, window)
    from .classes import class_sums_host             # (a backend without the device reduction)
    return class_sums_host(b, what, variable, edges, shape, window)


def overturning_in_classes(model, edges, variable="potential_density", window=None):
    """The meridional overturning streamfunction in classes of `variable` ("potential_density", "T", "S"), psi [j, e] in m^3/s
    for every row of y faces and e = 0 .. len(edges) + 1: the northward volume transport of the water lighter (colder, fresher)
    than edge e - 1, accumulated from the first class, 0 at e = 0 -- the residual overturning of a run with eddies, binned and
    reduced on the device (include/gb25.h, gb25_get_class_sums).  edges: class_edges(lo, hi, n) or any increasing vector."""
    return _class_sums(model, "faces_y", variable, edges, "cumulative", window)["flow"]


def water_mass_census(model, edges, variable="potential_density", by_row=False):
    """How much water sits in each class of `variable`: records [b] (by_row: [j, b]) with measure = volume [m^3], heat = the
    volume integral of T, salt = that of S, count = the wet cells, reduced on the device (gb25_get_class_sums)."""
    return _class_sums(model, "cells", variable, edges, "rows" if by_row else "total")


def _zonal_spectrum(b, source, wavenumbers=None, levels=None, param=None):
    if hasattr(b, "zonal_spectrum"):
        return b.zonal_spectrum(source, wavenumbers, levels, param)
    from .spectra import spectrum_host               # (a backend without the kernel)
    return spectrum_host(b, source, wavenumbers, levels, param)


def zonal_spectrum(model, source, wavenumbers=None, levels=None, param=None):
    """(X, nonfinite_lines): the zonal wavenumber coefficients X [level, row, m] (complex128, np.fft.rfft's sign) of every
    interior line of `source` -- a field name ("u", "v", "T", "eta", ...) or a derived name ("vorticity", "kinetic_energy", ...;
    "mixed_layer_depth" with param = the threshold) --, transformed on the device (include/gb25.h, gb25_get_zonal_spectrum): a few
    kilobytes cross PCIe, not the field.  wavenumbers = (m_first, m_count), levels = (k_first, k_count), count = -1: to the end;
    `zonal_spectrum(model, "v", levels=(Nz - 1, 1))` is the surface.  Along the grid's index i: a latitude circle only on the
    LatitudeLongitudeGrid."""
    return _zonal_spectrum(model.backend, source, wavenumbers, levels, param)


def zonal_power_spectrum(model, source, wavenumbers=None, levels=None, param=None):
    """The one-sided power spectrum P [level, row, m] of `source` (spectra.power_spectrum of zonal_spectrum): summed over all
    wavenumbers it is the zonal mean of the square; of "v" the meridional kinetic-energy spectrum, of "vorticity" the enstrophy
    spectrum."""
    from .spectra import global_columns, power_spectrum
    X, _ = _zonal_spectrum(model.backend, source, wavenumbers, levels, param)
    return power_spectrum(X, global_columns(model.backend)[0], 0 if wavenumbers is None else int(wavenumbers[0]))


class Averages:
    """The handle `averages(model, ...)` returns: time averages accumulated where the fields live (include/gb25.h, "time
    averages and eddy fluxes accumulated on the device").  sample() between two composite calls adds the state, weighted, to
    fp64 accumulators on the device -- one launch, nothing downloaded --; mean / raw copy one quantity to the host.  Names:
    u v w T S eta (means), uu vv TT SS etaeta (squares), uT uS vT vS wT wS (fluxes at the faces of the velocity)."""

    def __init__(self, model, groups=("means", "squares", "fluxes"), levels=None):
        self.model = model
        b = model.backend
        self._clock = b.clock
        self._previous_iteration = None
        if hasattr(b, "averages_begin"):
            b.averages_begin(groups, levels)
            self._dev, self._host = b, None
        else:                                            # (a backend without the device kernel: the numpy restatement)
            from .averages import AveragesHost
            self._dev, self._host = None, AveragesHost(b, groups, levels)

    def sample(self, weight=None):
        """Add the model's state as it is now.  weight: default the clock's last_dt times the iterations since the previous
        sample (last_dt for the first sample), so that a mean over samples taken at uneven intervals is a time mean."""
        _, iteration, last_dt = self._clock()
        if weight is None:
            steps = 1 if self._previous_iteration is None else max(1, iteration - self._previous_iteration)
            weight = last_dt * steps
        if self._dev:
            self._dev.averages_accumulate(weight)
        else:
            self._host.sample(weight)
        self._previous_iteration = iteration
        return self

    def info(self):
        return self._dev.averages_info() if self._dev else self._host.info()

    def mean(self, name):
        """accumulator / weight_sum, float64 [i, j, k] over the window."""
        return self._dev.get_average(name, True) if self._dev else self._host.mean(name)

    def raw(self, name):
        """The accumulator itself: sum of weight * term."""
        return self._dev.get_average(name, False) if self._dev else self._host.raw(name)

    def eddy_flux(self, name):
        """<v'T'> = <vT> - <v> <T at the face> ("uT", "uS", "vT", "vS", "wT", "wS"), gb25_amd.averages.eddy_flux of the means."""
        from .averages import eddy_flux
        return eddy_flux({n: self.mean(n) for n in (name[0], name[1], name)}, name)

    def eddy_kinetic_energy(self):
        from .averages import eddy_kinetic_energy
        return eddy_kinetic_energy({n: self.mean(n) for n in ("u", "v", "uu", "vv")})

    def tracer_variance(self, name):
        from .averages import tracer_variance
        return tracer_variance({n: self.mean(n) for n in (name, name + name)}, name)

    def close(self):
        if self._dev:
            if getattr(self._dev, "h", None):
                self._dev.averages_end()
        else:
            self._host.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def averages(model, groups=("means", "squares", "fluxes"), levels=None):
    """Start accumulating time averages of `groups` ("means" must be among them) over the cell levels levels = (k_first,
    k_count), 0-based (None: all); returns the Averages handle: `a = averages(model); loop(model, 10); a.sample(); ...;
    a.mean("T"); a.eddy_flux("vT"); a.close()`."""
    return Averages(model, groups, levels)


def run_averaged(model, steps, every, **kw):
    """loop(model, every) then sample(), repeated until `steps` steps are done (a remainder shorter than `every` is stepped and
    sampled last); returns the Averages handle.  kw: groups, levels of averages()."""
    a = averages(model, **kw)
    done = 0
    while done < steps:
        n = min(int(every), steps - done)
        loop(model, n)
        a.sample()
        done += n
    return a


def state_monitor(model):
    """What the progress callback of simulations/ocean_climate_simulation.jl:95-116 prints -- max|u|, |v|, |w|, extrema(T), ...
    plus the advective CFL rate and the number of non-finite values -- reduced on the device: `print(state_monitor(model))`.
    Does not change what the model computes or how fast it steps."""
    return model.backend.state_monitor()


def resolution_to_points(resolution):
    """src/model_utils.jl:45-49."""
    Nx, Ny = 384 / resolution, 192 / resolution
    if Nx != int(Nx) or Ny != int(Ny):
        raise ValueError("resolution must divide 384 and 192")
    return int(Nx), int(Ny)


class VerticalScalarDiffusivity:
    """closure = VerticalScalarDiffusivity(VerticallyImplicitTimeDiscretization(), κ=1e-5, ν=1e-4), the alternative the
    reference keeps next to `closure = nothing` (src/baroclinic_instability_model.jl:29-31): constant vertical viscosity
    ν and diffusivity κ, stepped implicitly (one tridiagonal solve per column and field after the AB2 update)."""

    def __init__(self, nu=1e-4, kappa=1e-5):
        self.nu, self.kappa = float(nu), float(kappa)


class CATKEVerticalDiffusivity:
    """closure = Oceananigans.TurbulenceClosures.CATKEVerticalDiffusivity() (src/baroclinic_instability_model.jl:30,
    sharding/less_simple_sharding_problem.jl:84-93): a third tracer e (turbulent kinetic energy), diffusivity fields
    κu, κc, κe, Lᵉ, Jᵇ (compared by src/correctness.jl:60-67), vertically implicit mixing of u, v, T, S, e.
    Keyword arguments change parameters (names of gb25_catke_parameters in include/gb25.h), e.g. Cb=0.01."""

    def __init__(self, **parameters):
        self.parameters = parameters


def default_ocean_closure():
    """ClimaOcean.OceanSimulations.default_ocean_closure() -- what ocean_simulation(grid; ...) uses when no closure is given
    (src/data_free_ocean_climate_model.jl:26): CATKEVerticalDiffusivity with CATKEMixingLength(Cᵇ = 0.01)
    [UPSTREAM-UNVERIFIED: recalled from ClimaOcean, which is not in /root/reference]."""
    return CATKEVerticalDiffusivity(Cb=0.01)


def baroclinic_instability_model(arch, Nx=None, Ny=None, Nz=None, *, dt, halo=(8, 8, 8), grid_type="simple_lat_lon",
                                 substeps=30, resolution=None, closure=None, **backend_kw):
    """baroclinic_instability_model(arch, Nx, Ny, Nz; dt, halo, grid_type, free_surface=SplitExplicit(substeps))
    -- src/baroclinic_instability_model.jl:12-85.  `arch` is a backend factory: GPU() from this package
    (or, in tests only, an oracle-backed factory).  Physics is fixed to the reference defaults:
    TEOS-10 SeawaterBuoyancy, HydrostaticSphericalCoriolis, WENOVectorInvariant(order=5),
    WENO(order=5), closure=nothing.  The initial state is all zeros, as in the reference
    (set_baroclinic_instability! is commented out at :74-80)."""
    if resolution is not None:
        Nx, Ny = resolution_to_points(resolution)
    # grid_type (src/baroclinic_instability_model.jl:19,59-65): :simple_lat_lon | :gaussian_islands, where
    # :gaussian_islands = ImmersedBoundaryGrid(TripolarGrid, GridFittedBottom(gaussian_islands)) (src/model_utils.jl:
    # 134-146).  Also: the same mountains on the lat-lon grid, the bare tripolar grid, and (tests) the lat-lon metrics
    # sent through the curvilinear code path.
    grid_types = {"simple_lat_lon": 0, "gaussian_islands_lat_lon": 1, "lat_lon_as_curvilinear": 2, "tripolar": 3,
                  "gaussian_islands": 4}
    if grid_type not in grid_types:
        raise ValueError(f"grid_type={grid_type!r} must be one of {sorted(grid_types)}")
    if grid_types[grid_type]:
        backend_kw["grid_type"] = grid_types[grid_type]
    H = halo[0] if isinstance(halo, (tuple, list)) else halo
    if isinstance(halo, (tuple, list)) and len(set(halo)) != 1:
        raise ValueError("halo must be the same in every direction")
    # backend_kw: `options` (schedule switches, binding.OPTION_IDS) and overrides of gb25_config fields
    backend = arch(Nx, Ny, Nz, dt=dt, halo=H, substeps=substeps, **backend_kw)
    model = HydrostaticFreeSurfaceModel(backend, Nx, Ny, Nz, H)
    model.free_surface.substeps = substeps
    model.grid_type = grid_type
    model.closure = closure
    if isinstance(closure, CATKEVerticalDiffusivity):
        backend.set_catke(True)
        if closure.parameters:
            backend.set_catke_parameters(**closure.parameters)
        model.enable_catke_fields()
    elif closure is not None:
        if not isinstance(closure, VerticalScalarDiffusivity):
            raise NotImplementedError("closures: None, VerticalScalarDiffusivity(nu, kappa) or CATKEVerticalDiffusivity()")
        backend.set_vertical_diffusivity(closure.nu, closure.kappa)
    return model


def set_top_flux(model, **fluxes):
    """FluxBoundaryCondition at the top of u, v, T, S (what ClimaOcean's ocean_simulation gives the ocean model and the
    coupled model fills every step: wind stress, heat and fresh-water flux; src/data_free_ocean_climate_model.jl:26,
    src/precompile.jl:52-61).  `set_top_flux(model, T=J_T, u=tau_x)`; arrays at the interior points of the field's
    horizontal location, positive upward; None restores the default no-flux condition."""
    for name, J in fluxes.items():
        if name not in ("u", "v", "T", "S"):
            raise ValueError(f"top flux boundary conditions exist for u, v, T, S, not {name!r}")
        model.backend.set_top_flux(name, J)


def set_baroclinic_instability(model):
    """set_baroclinic_instability!(model) -- src/model_utils.jl:120-127."""
    model.backend.set_baroclinic_instability()


def first_time_step(model):
    """first_time_step!(model) -- src/timestepping_utils.jl:21-27."""
    model.backend.first_time_step()


def time_step(model):
    """time_step!(model) -- src/timestepping_utils.jl:29-35."""
    model.backend.time_step()


def loop(model, Ninner):
    """loop!(model, Ninner) -- src/timestepping_utils.jl:37-45."""
    model.backend.loop(int(Ninner))


# ---- the per-phase workloads of src/precompile.jl:44-127 ----
def tupled_fill_halo_regions_workload(model): model.backend.fill_halo_regions()
def compute_tendencies_workload(model): model.backend.compute_tendencies()
def compute_boundary_tendencies_workload(model): model.backend.compute_boundary_tendencies()
def compute_interior_momentum_tendencies_workload(model): model.backend.compute_momentum_tendencies()
def compute_interior_tracer_tendencies_workload(model): model.backend.compute_tracer_tendencies()
def compute_auxiliaries_workload(model): model.backend.compute_auxiliaries()
def fill_halo_regions_workload(model): model.backend.fill_diffusivity_halos()
def mask_immersed_model_fields_workload(model): model.backend.mask_immersed_fields()
def ab2_step_workload(model, dt): model.backend.ab2_step(dt, False)
def correct_velocities_and_cache_previous_tendencies_workload(model, dt):
    model.backend.correct_velocities_and_cache_previous_tendencies(dt)
def initialize(model): model.backend.initialize()
def update_state(model): model.backend.update_state()
