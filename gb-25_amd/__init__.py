"""gb25_amd -- MI355X-native implementation of the time-step hot path of PRONTOLab/GB-25.

Public names mirror `GordonBell25` (GB-25 src/GordonBell25.jl:3-4 and the un-exported helpers
its scripts call); Julia's trailing `!` is dropped.  Kernels live in libgb25hip.so behind the
C ABI of include/gb25.h; this package only sequences calls and moves host arrays.
"""
from .binding import GB25Error, HipBackend, LIB_PATH, load_library
from .build import build_library
from .correctness import approx_equal, combine_diffs, combine_stats, compare_states, sync_states
from .integrals import cell_measure, combine_budgets, combine_moments, fold_records, integrate_host
# (the submodule first: the name `averages` of the package is the function of .model, imported after it)
from .averages import (AveragesHost, average_terms, eddy_flux, eddy_kinetic_energy, gather_averages, tracer_variance)
from .regions import Regions, label_host, region_records_host, regions_host, regions_of_arrays
from .model import (CATKEVerticalDiffusivity, default_ocean_closure, Field, HydrostaticFreeSurfaceModel, VerticalScalarDiffusivity,
                    baroclinic_instability_model, budget, density_anomaly, first_time_step, initialize, kinetic_energy,
                    mixed_layer_depth, potential_density, vorticity,
                    at_depths, isosurface_depth, layer_thickness, on_isosurface,
                    baroclinic_wave_speed, buoyancy_frequency, deformation_radius, eady_growth_rate, eddy_resolution, ertel_pv,
                    richardson_number, shear_squared,
                    divergence, frontogenesis, gradient_magnitude, normal_strain, okubo_weiss, rossby_number, shear_strain,
                    coarsen, column_integral, depth_mean, heat_content, subgrid_variance,
                    eddy_part, filtered, subfilter_variance,
                    eddy_census, regions,
                    heat_transport, meridional_transport, overturning, section_transport,
                    overturning_in_classes, water_mass_census, zonal_power_spectrum, zonal_spectrum,
                    Averages, averages, run_averaged,
                    loop, resolution_to_points, state_monitor, set_baroclinic_instability, set_top_flux, time_step, update_state,
                    tupled_fill_halo_regions_workload, compute_tendencies_workload,
                    compute_boundary_tendencies_workload, compute_interior_momentum_tendencies_workload,
                    compute_interior_tracer_tendencies_workload, compute_auxiliaries_workload,
                    fill_halo_regions_workload, ab2_step_workload,
                    correct_velocities_and_cache_previous_tendencies_workload)
from .derived import (gather_derived, kinetic_energy_host, mixed_layer_depth_host, mixed_layer_depth_of_profiles,
                      vorticity_host)
from .transports import combine_transports, face_area, fold_transports, transport_host, transport_terms
from .classes import (class_bins, class_edges, class_sums_host, class_terms, class_values, combine_class_sums, fold_classes,
                      total_classes)
from .spectra import (combine_spectra, cospectrum, dominant_wavenumber, host_table, power_spectrum, spectrum_host,
                      zonal_coefficients)
from .surfaces import gather_surfaces, on_surfaces_host, surfaces_of_profiles
from .stability import gather_stability, stability_host, stability_of_columns
from .kinematics import gather_kinematics, kinematics_host, kinematics_pieces
from .eddies import (ZonalEddy, combine_zonal_eddy, lorenz_cycle, lorenz_cycle_of_records, zonal_eddy, zonal_eddy_host)
from .blocks import BlockSums, block_sums_host, depth_weights, gather_blocks, sums_of_blocks
from .filters import FilterSums, filter_of_planes, filter_sums_host, kernel_weights, rows_for_length
# (the submodule first, as for the averages: the name `particles` of the package is the function)
from .particles import (Particles, ParticlesHost, advance_host, exchange_particles, particle_rates, particles, run_with_particles,
                        sample_host, seed_particles, seed_positions)
from .passive import PassiveTracers, passive_tracers, passive_update_host, run_with_tracers
from .data_free import (PrescribedAtmosphere, analytic_atmosphere, data_free_ocean_climate_model_init,
                        set_prescribed_atmosphere, set_data_free_state, zonal_wind, sunlight, Tatm)
from .sharding import factors
from .arg_parsing import (float_type_from_args, float_type_from_string, interior_size, multifloat_from_args,
                          parse_baroclinic_instability_args)
from .sharded_io import load_all_fields, load_global_field, save_model_state
from .restart import checkpoint, read_checkpoint, restore, run_checkpointed


class GPU:
    """Architecture object: `baroclinic_instability_model(GPU(), Nx, Ny, Nz; dt=...)`
    (the reference passes CPU() / GPU() / ReactantState(), correctness/..._run.jl:33-34)."""

    def __init__(self, device=0, float_type="Float32"):
        self.device = device
        self.float_type = float_type   # "Float32" | "Float64" (float_type_from_args)

    def __call__(self, Nx, Ny, Nz, **kw):
        kw.setdefault("device", self.device)
        kw.setdefault("float_type", self.float_type)
        return HipBackend(Nx, Ny, Nz, **kw)


__all__ = [n for n in dir() if not n.startswith("_")]
