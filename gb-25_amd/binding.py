"""ctypes binding of libgb25hip.so (the C ABI in include/gb25.h).

This is the only place the shared library is loaded.  There is no fallback: if the
library is missing or no HIP device is visible, construction raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GB25_LIB") or os.path.join(_HERE, "libgb25hip.so")   # GB25_LIB: A/B builds while tuning
# one library per Oceananigans float type (src/arg_parsing.jl:12-16): same source, same symbols
LIB_PATHS = {"Float32": LIB_PATH, "Float64": os.path.join(_HERE, "libgb25hip_f64.so")}
DTYPES = {"Float32": np.float32, "Float64": np.float64}

FIELD_IDS = {
    "u": 0, "v": 1, "w": 2, "T": 3, "S": 4, "pHY": 5,
    "Gn.u": 6, "Gn.v": 7, "Gn.T": 8, "Gn.S": 9,
    "Gm.u": 10, "Gm.v": 11, "Gm.T": 12, "Gm.S": 13,
    "eta": 14, "U": 15, "V": 16,
    "eta_bar": 17, "U_bar": 18, "V_bar": 19,
    "Gn.U": 20, "Gn.V": 21,
    # closure = CATKEVerticalDiffusivity() only
    "e": 22, "Gn.e": 23, "Gm.e": 24, "kappa_u": 25, "kappa_c": 26, "kappa_e": 27, "Le": 28, "Jb": 29,
    "previous_u": 30, "previous_v": 31,   # diffusivity_fields.previous_velocities (CATKE)
}
METRIC2_IDS = ["dxfc", "dxcc", "dxcf", "dxff", "dyfc", "dycc", "dycf", "dyff", "azcc", "azfc", "azcf", "azff", "fff", "phicc"]
METRIC_IDS = {"phif": 0, "phic": 1, "dxc": 2, "dxf": 3, "azc": 4, "azf": 5, "fcor": 6,
              "zf": 7, "zc": 8, "dzc": 9, "dzf": 10, "dy": 11}
ATMOSPHERE_IDS = {"u": 0, "v": 1, "T": 2, "q": 3, "p": 4, "shortwave": 5, "longwave": 6}
KERNEL_IDS = {"fill_halos": 0, "compute_w": 1, "compute_p": 2, "gu": 3, "gv": 4, "tracers": 5,
              "ab2_velocities": 6, "ab2_tracers": 7, "barotropic": 8, "corrector": 9, "implicit": 10, "closure": 11,
              "fluxes": 12, "diagnostics": 13}

# every symbol include/gb25.h declares (checked by tests/test_abi.py)
ABI_SYMBOLS = [
    "gb25_default_config", "gb25_create", "gb25_destroy", "gb25_last_error_string", "gb25_version",
    "gb25_real_bytes", "gb25_config_bytes", "gb25_catke_parameters_bytes",
    "gb25_set_stream", "gb25_use_own_stream", "gb25_synchronize", "gb25_field_dims", "gb25_set_field", "gb25_get_field",
    "gb25_field_device_ptr", "gb25_get_metric", "gb25_get_metric2", "gb25_get_substepping", "gb25_set_vertical_diffusivity",
    "gb25_get_vertical_diffusivity", "gb25_set_closure_catke", "gb25_set_prescribed_atmosphere",
    "gb25_compute_atmosphere_ocean_fluxes", "gb25_get_top_flux", "gb25_default_catke_parameters",
    "gb25_set_catke_parameters", "gb25_get_catke_parameters", "gb25_set_bottom_drag", "gb25_get_bottom_drag", "gb25_set_tracer_advection_order",
    "gb25_get_tracer_advection_order",
    "gb25_set_baroclinic_instability",
    "gb25_get_clock", "gb25_set_dt", "gb25_initialize", "gb25_mask_immersed_fields",
    "gb25_fill_halo_regions", "gb25_compute_auxiliaries", "gb25_fill_diffusivity_halos",
    "gb25_compute_momentum_tendencies", "gb25_compute_tracer_tendencies", "gb25_compute_boundary_tendencies",
    "gb25_compute_tendencies", "gb25_ab2_step", "gb25_correct_velocities_and_cache_previous_tendencies",
    "gb25_update_state", "gb25_first_time_step", "gb25_time_step", "gb25_loop",
    "gb25_set_option", "gb25_get_option", "gb25_set_bottom_height", "gb25_set_curvilinear_grid", "gb25_set_vertical_faces", "gb25_get_bottom_info", "gb25_set_top_flux",
    "gb25_comm_unique_id", "gb25_comm_init_rccl", "gb25_comm_init_local", "gb25_comm_init_callback", "gb25_comm_finalize",
    "gb25_comm_info", "gb25_debug_exchange_plan",
    "gb25_lookahead_state", "gb25_debug_sequence", "gb25_save_state",
    "gb25_profile_enable", "gb25_profile_reset", "gb25_profile_get",
    "gb25_field_stats_bytes", "gb25_field_diff_bytes", "gb25_state_monitor_bytes", "gb25_get_field_stats", "gb25_compare_field",
    "gb25_get_state_monitor", "gb25_field_device_ptr_readonly",
    "gb25_integrate_field", "gb25_get_budget", "gb25_moments_bytes", "gb25_budget_bytes",
    "gb25_derived_dims", "gb25_compute_derived", "gb25_get_derived", "gb25_get_derived_stats", "gb25_get_field_levels",
    "gb25_transport_bytes", "gb25_get_transport",
    "gb25_class_sum_bytes", "gb25_get_class_sums",
    "gb25_spectral_coefficient_bytes", "gb25_get_spectrum_table", "gb25_get_zonal_spectrum", "gb25_get_derived_zonal_spectrum",
    "gb25_compute_on_surfaces", "gb25_get_on_surfaces",
    "gb25_stability_dims", "gb25_compute_stability", "gb25_get_stability", "gb25_get_stability_stats",
    "gb25_kinematics_dims", "gb25_compute_kinematics", "gb25_get_kinematics", "gb25_get_kinematics_stats",
    "gb25_zonal_eddy_bytes", "gb25_zonal_eddy_dims", "gb25_get_zonal_eddy",
    "gb25_block_info_bytes", "gb25_block_dims", "gb25_derived_block_dims", "gb25_get_block_sums", "gb25_compute_block_sums",
    "gb25_get_derived_block_sums",
    "gb25_filter_info_bytes", "gb25_filter_dims", "gb25_derived_filter_dims", "gb25_get_filter_sums", "gb25_compute_filter_sums",
    "gb25_get_derived_filter_sums",
    "gb25_region_bytes", "gb25_regions_info_bytes", "gb25_region_dims", "gb25_label_regions", "gb25_get_regions",
    "gb25_averages_info_bytes", "gb25_averages_begin", "gb25_averages_accumulate", "gb25_averages_get_info", "gb25_average_dims",
    "gb25_get_average", "gb25_average_device_ptr", "gb25_averages_end",
    "gb25_particles_info_bytes", "gb25_particles_begin", "gb25_particles_set", "gb25_particles_get", "gb25_particles_advance",
    "gb25_particles_sample", "gb25_particles_get_info", "gb25_particles_end",
    "gb25_tracer_spec_bytes", "gb25_tracers_begin", "gb25_tracers_set", "gb25_tracers_get", "gb25_tracers_advance", "gb25_tracers_stats",
    "gb25_tracers_clock", "gb25_tracers_end",
    "gb25_checkpoint_info_bytes", "gb25_restore_info_bytes", "gb25_checkpoint_snapshot", "gb25_checkpoint_write",
    "gb25_checkpoint_get_info", "gb25_checkpoint_release", "gb25_restore", "gb25_set_clock",
]
# gb25_derived (include/gb25.h)
DERIVED_IDS = {"vorticity": 0, "kinetic_energy": 1, "density_anomaly": 2, "potential_density": 3, "mixed_layer_depth": 4}
SUM_SHAPES = {"rows": 0, "levels": 1, "total": 2}   # gb25_sum_shape
TRANSPORT_FACES = {"across_y": 0, "across_x": 1}                         # gb25_transport_faces
TRANSPORT_SHAPES = {"lines": 0, "profile": 1, "streamfunction": 2}      # gb25_transport_shape
CLASS_WHAT = {"faces_y": 0, "cells": 1}                                   # gb25_class_what
CLASS_VARIABLES = {"T": 0, "S": 1, "potential_density": 2}                # gb25_class_variable
CLASS_SHAPES = {"rows": 0, "cumulative": 1, "total": 2}                   # gb25_class_shape
CLASS_MAX_BINS = 256                                                      # GB25_CLASS_MAX_BINS
# gb25_surface_variable, gb25_surface_carried, gb25_surface_status, GB25_SURFACE_MAX_VALUES
SURFACE_VARIABLES = {"T": 0, "S": 1, "potential_density": 2, "depth": 3}
SURFACE_CARRIED = {"depth": 0, "T": 1, "S": 2, "e": 3, "kinetic_energy": 4, "density_anomaly": 5, "potential_density": 6}
SURFACE_STATUS = {"found": 0, "outcrop": 1, "grounded": 2, "dry": 3}
SURFACE_MAX_VALUES = 64
# gb25_stability (include/gb25.h); the floor each takes as param when none is given (the Richardson number's 1e-12 s^-2 is a convention)
STABILITY_IDS = {"n2": 0, "shear2": 1, "richardson": 2, "eady_rate": 3, "ertel_pv": 4, "wave_speed": 5}
STABILITY_DEFAULT_PARAM = {"richardson": 1e-12}
# gb25_kinematics (include/gb25.h); the tracer the gradient and the frontogenesis function take as param
KINEMATICS_IDS = {"divergence": 0, "normal_strain": 1, "shear_strain": 2, "okubo_weiss": 3, "rossby_number": 4, "gradient": 5,
                  "frontogenesis": 6}
KINEMATICS_TRACERS = {"T": 0, "S": 1, "potential_density": 2}
# gb25_region_source, gb25_region_cmp (include/gb25.h): what the criterion of the coherent regions may be, by source
REGION_SOURCES = {"field": 0, "derived": 1, "kinematics": 2}
REGION_FIELDS = ("T", "S", "e")
REGION_DERIVED = ("kinetic_energy", "density_anomaly", "potential_density")
REGION_KINEMATICS = ("divergence", "normal_strain", "okubo_weiss", "gradient", "frontogenesis")
REGION_CMP = {"below": 0, "above": 1}
# gb25_zonal_eddy_variable (include/gb25.h): the six centred variables of a line record, in the record's order
ZONAL_EDDY_VARIABLES = {"U": 0, "V": 1, "W": 2, "T": 3, "S": 4, "SIGMA": 5}
AVERAGE_GROUPS = {"means": 1, "squares": 2, "fluxes": 4}              # gb25_average_group
# gb25_average: name -> id; the first six are the MEANS, the next five the SQUARES, the last six the FLUXES
AVERAGE_IDS = {n: q for q, n in enumerate(["u", "v", "w", "T", "S", "eta", "uu", "vv", "TT", "SS", "etaeta",
                                           "uT", "uS", "vT", "vS", "wT", "wS"])}
# gb25_particle_status, gb25_particle_counter
PARTICLE_STATUS = {"active": 0, "at_fold": 1, "outside": 2, "nonfinite": 3}
PARTICLE_COUNTERS = ("blocked", "clamped_y", "clamped_z", "at_fold", "outside", "nonfinite", "too_far")
# gb25_option (include/gb25.h)
OPTION_IDS = {"kernels": 0, "ab2_lookahead": 1, "subcycle_lookahead": 2, "subcycle_block": 3, "fill_fused": 4,
              "two_streams": 5, "store_pressure": 6, "split_tendencies": 7, "pressure_precision": 8, "immersed_kernels": 9, "fold_fills": 10,
              "lazy_corrector": 11, "momentum_chunk_levels": 12, "tracer_chunk_levels": 13, "tracers_first": 14, "w_on_the_fly": 15, "sub_stream_priority": 16, "subcycle_whole": 17, "early_strips": 18,
              "catke_stale_e_halos": 19, "comm_timeout_seconds": 20, "roctx_ranges": 21, "substep_order": 22, "fold_pivot_slaved": 23, "pressure_form": 24,
              "spectrum_table": 25}
TRACERS_MAX = 8                                                           # GB25_TRACERS_MAX
TRACER_ARRAYS = {"c": 0, "Gn": 1, "Gm": 2}                                # `which` of gb25_tracers_get
UNIQUE_ID_BYTES = 128
# int32 fn(void *user, int32 buffer_set, const void *send_w, const void *send_e, void *recv_w, void *recv_e, int64 nbytes)
EXCHANGE_FN = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64)


class CatkeParameters(C.Structure):
    """gb25_catke_parameters (include/gb25.h); the arrays are psi = u, c, e, D."""
    _fields_ = [("Cs", C.c_double), ("Cb", C.c_double), ("Csp", C.c_double), ("CRid", C.c_double), ("CRi0", C.c_double),
                ("Chi", C.c_double * 4), ("Clo", C.c_double * 4), ("Cun", C.c_double * 4), ("Cc", C.c_double * 4),
                ("Ce", C.c_double * 4), ("CWu", C.c_double), ("CWw", C.c_double), ("minimum_tke", C.c_double),
                ("minimum_convective_buoyancy_flux", C.c_double), ("negative_tke_damping_time_scale", C.c_double),
                ("CWeps", C.c_double)]

    def as_list(self):
        out = [self.Cs, self.Cb, self.Csp, self.CRid, self.CRi0]
        for a in (self.Chi, self.Clo, self.Cun, self.Cc, self.Ce):
            out += list(a)
        return out + [self.CWu, self.CWw, self.minimum_tke, self.minimum_convective_buoyancy_flux, self.negative_tke_damping_time_scale,
                      self.CWeps]


class Config(C.Structure):
    """gb25_config (include/gb25.h)."""
    _fields_ = [
        ("Nx", C.c_int32), ("Ny", C.c_int32), ("Nz", C.c_int32), ("halo", C.c_int32),
        ("substeps", C.c_int32), ("rank", C.c_int32), ("nranks", C.c_int32), ("device", C.c_int32),
        ("dt", C.c_double), ("chi", C.c_double),
        ("lat_south", C.c_double), ("lat_north", C.c_double), ("lon_west", C.c_double), ("lon_east", C.c_double),
        ("depth", C.c_double), ("zexp_h", C.c_double),
        ("g", C.c_double), ("Omega", C.c_double), ("radius", C.c_double), ("rho0", C.c_double),
        ("slab_mode", C.c_int32), ("grid_type", C.c_int32), ("ranks_y", C.c_int32),
    ]


class _Record(C.Structure):
    """A result struct of the device diagnostics: compared and printed by value."""

    def as_dict(self):
        out = {}
        for name, _ in self._fields_:
            v = getattr(self, name)
            out[name] = v.as_dict() if isinstance(v, _Record) else (tuple(v) if hasattr(v, "__len__") else v)
        out.pop("reserved", None)
        return out

    def __eq__(self, other):
        return type(other) is type(self) and bytes(self) == bytes(other)

    __hash__ = None

    def __repr__(self):
        return f"{type(self).__name__}({', '.join(f'{k}={v!r}' for k, v in self.as_dict().items())})"


class FieldStats(_Record):
    """gb25_field_stats (include/gb25.h): positions are 1-based (i, j, k) in the box; position + global_offset = 1-based
    index into the global interior."""
    _fields_ = [("min", C.c_double), ("max", C.c_double), ("max_abs", C.c_double), ("sum", C.c_double), ("sum_sq", C.c_double),
                ("count", C.c_int64), ("nonfinite", C.c_int64),
                ("at_max_abs", C.c_int32 * 3), ("first_nonfinite", C.c_int32 * 3), ("global_offset", C.c_int32 * 3),
                ("reserved", C.c_int32)]


class TracerSpec(_Record):
    """gb25_tracer_spec (include/gb25.h): the constant source per second, the value the top level is reset to (when surface_reset
    is not 0), and whether negative values are clipped after every update (such a tracer is not conserved)."""
    _fields_ = [("source", C.c_double), ("surface_value", C.c_double), ("surface_reset", C.c_int32), ("clip_negative", C.c_int32)]


class FieldDiff(_Record):
    """gb25_field_diff (include/gb25.h): a = the model's field, b = the other array, delta = a - b in fp64."""
    _fields_ = [("max_abs_a", C.c_double), ("max_abs_b", C.c_double), ("max_abs_delta", C.c_double),
                ("sum_sq_a", C.c_double), ("sum_sq_b", C.c_double), ("sum_sq_delta", C.c_double),
                ("count", C.c_int64), ("nonfinite", C.c_int64),
                ("at_max_abs_delta", C.c_int32 * 3), ("global_offset", C.c_int32 * 3)]


class StateMonitor(_Record):
    """gb25_state_monitor (include/gb25.h).  str() is one progress line in the shape of the reference's callback
    (simulations/ocean_climate_simulation.jl:95-116)."""
    _fields_ = [("u", FieldStats), ("v", FieldStats), ("w", FieldStats), ("eta", FieldStats), ("T", FieldStats), ("S", FieldStats),
                ("cfl", C.c_double), ("at_cfl", C.c_int32 * 3), ("reserved", C.c_int32),
                ("nonfinite_total", C.c_int64), ("iteration", C.c_int64), ("time", C.c_double)]

    def __str__(self):
        return ("iter: %d, time: %.6g s, max|u, v, w|: (%.2e, %.2e, %.2e) m/s, extrema(T): (%.3f, %.3f), extrema(S): (%.3f, %.3f), "
                "max|eta|: %.3e m, advective CFL rate: %.3e 1/s at (%d, %d, %d), non-finite: %d"
                % (self.iteration, self.time, self.u.max_abs, self.v.max_abs, self.w.max_abs, self.T.min, self.T.max,
                   self.S.min, self.S.max, self.eta.max_abs, self.cfl, *self.at_cfl, self.nonfinite_total))


class Moments(_Record):
    """gb25_moments (include/gb25.h): sum mu, sum mu x, sum mu x^2 over the points with mu > 0 and x finite, how many those
    are, and how many wet points were skipped because x is not finite."""
    _fields_ = [("measure", C.c_double), ("first", C.c_double), ("second", C.c_double),
                ("points", C.c_int64), ("nonfinite", C.c_int64)]


MOMENTS_DTYPE = np.dtype([("measure", np.float64), ("first", np.float64), ("second", np.float64),
                          ("points", np.int64), ("nonfinite", np.int64)])


class ZonalEddyRow(_Record):
    """gb25_zonal_eddy_row (include/gb25.h): of one line (row j, level k) the measure, the first moments and the means of the six
    centred variables, the 21 comoments of their deviations (p <= q, row-major), the counted and the skipped cells."""
    _fields_ = [("measure", C.c_double), ("first", C.c_double * 6), ("mean", C.c_double * 6), ("co", C.c_double * 21),
                ("points", C.c_int64), ("nonfinite", C.c_int64)]


ZONAL_EDDY_DTYPE = np.dtype([("measure", np.float64), ("first", np.float64, (6,)), ("mean", np.float64, (6,)),
                             ("co", np.float64, (21,)), ("points", np.int64), ("nonfinite", np.int64)])


class Blocks(C.Structure):
    """gb25_blocks (include/gb25.h): the extents of a block and the window of levels."""
    _fields_ = [("bx", C.c_int32), ("by", C.c_int32), ("bz", C.c_int32), ("k_first", C.c_int32), ("k_count", C.c_int32),
                ("reserved", C.c_int32)]


class BlockInfo(_Record):
    """gb25_block_info (include/gb25.h): the result's dims, the counted and the skipped points of all blocks, the blocks whose
    measure is 0, the global offset of the rank's fine interior."""
    _fields_ = [("dims", C.c_int32 * 3), ("reserved", C.c_int32), ("points", C.c_int64), ("nonfinite", C.c_int64),
                ("empty_blocks", C.c_int64), ("global_offset", C.c_int32 * 3), ("reserved2", C.c_int32)]


class Filter(C.Structure):
    """gb25_filter (include/gb25.h): the radii and strides of the window and the window of levels."""
    _fields_ = [("rx", C.c_int32), ("ry", C.c_int32), ("sx", C.c_int32), ("sy", C.c_int32), ("k_first", C.c_int32),
                ("k_count", C.c_int32), ("reserved", C.c_int32)]


class FilterInfo(_Record):
    """gb25_filter_info (include/gb25.h): the result's dims, the skipped source points, the outputs whose measure is 0, the
    outputs whose y window was cut, the global offset of the fine interior."""
    _fields_ = [("dims", C.c_int32 * 3), ("reserved", C.c_int32), ("nonfinite", C.c_int64), ("empty", C.c_int64),
                ("clipped", C.c_int64), ("global_offset", C.c_int32 * 3), ("reserved2", C.c_int32)]


class Region(_Record):
    """gb25_region (include/gb25.h): one connected region of a thresholded level -- its cells, key, box, whether it crosses the
    x seam, the sums weighted by the measure, the centroid sums about the key, the extreme value and its cell."""
    _fields_ = [("cells", C.c_int32), ("key_i", C.c_int32), ("key_j", C.c_int32), ("i_min", C.c_int32), ("i_max", C.c_int32),
                ("j_min", C.c_int32), ("j_max", C.c_int32), ("wraps", C.c_int32), ("extreme_i", C.c_int32), ("extreme_j", C.c_int32),
                ("measure", C.c_double), ("first", C.c_double), ("second", C.c_double), ("carried", C.c_double),
                ("sum_di", C.c_double), ("sum_dj", C.c_double), ("extreme", C.c_double)]


REGION_DTYPE = np.dtype([("cells", np.int32), ("key_i", np.int32), ("key_j", np.int32), ("i_min", np.int32), ("i_max", np.int32),
                         ("j_min", np.int32), ("j_max", np.int32), ("wraps", np.int32), ("extreme_i", np.int32), ("extreme_j", np.int32),
                         ("measure", np.float64), ("first", np.float64), ("second", np.float64), ("carried", np.float64),
                         ("sum_di", np.float64), ("sum_dj", np.float64), ("extreme", np.float64)])


class RegionsInfo(_Record):
    """gb25_regions_info (include/gb25.h), one per level: the true count of regions, how many records were stored, the foreground
    cells and the wet cells whose criterion is not finite."""
    _fields_ = [("regions", C.c_int32), ("stored", C.c_int32), ("foreground_cells", C.c_int64), ("nonfinite_cells", C.c_int64)]


REGIONS_INFO_DTYPE = np.dtype([("regions", np.int32), ("stored", np.int32), ("foreground_cells", np.int64), ("nonfinite_cells", np.int64)])


class Transport(_Record):
    """gb25_transport (include/gb25.h): sum a, sum a vel, sum a vel T, sum a vel S over the wet faces whose values are finite,
    how many those are, and how many wet faces were skipped because a value is not finite."""
    _fields_ = [("area", C.c_double), ("volume", C.c_double), ("heat", C.c_double), ("salt", C.c_double),
                ("faces", C.c_int64), ("nonfinite", C.c_int64)]


TRANSPORT_DTYPE = np.dtype([("area", np.float64), ("volume", np.float64), ("heat", np.float64), ("salt", np.float64),
                            ("faces", np.int64), ("nonfinite", np.int64)])


class ClassSum(_Record):
    """gb25_class_sum (include/gb25.h): the sums of one class (bin) -- FACES_Y: a, a v, a v T, a v S of the wet faces; CELLS: V, 0,
    V T, V S of the wet cells --, how many contributed, and (bin 0 of a row only) how many were skipped as not finite."""
    _fields_ = [("measure", C.c_double), ("flow", C.c_double), ("heat", C.c_double), ("salt", C.c_double),
                ("count", C.c_int64), ("nonfinite", C.c_int64)]


class SpectralCoefficient(C.Structure):
    """gb25_spectral_coefficient (include/gb25.h): X(m) = re + i im of one line, re = A, im = -B; a numpy complex128."""
    _fields_ = [("re", C.c_double), ("im", C.c_double)]


CLASS_SUM_DTYPE = np.dtype([("measure", np.float64), ("flow", np.float64), ("heat", np.float64), ("salt", np.float64),
                            ("count", np.int64), ("nonfinite", np.int64)])


class Budget(_Record):
    """gb25_budget (include/gb25.h): the totals of T, S, u, v, eta and what follows from them."""
    _fields_ = [("T", Moments), ("S", Moments), ("u", Moments), ("v", Moments), ("eta", Moments),
                ("volume", C.c_double), ("surface_area", C.c_double), ("kinetic_energy", C.c_double),
                ("eta_potential_energy", C.c_double), ("iteration", C.c_int64), ("time", C.c_double),
                ("global_offset", C.c_int32 * 3), ("reserved", C.c_int32)]

    def __str__(self):
        return ("iter: %d, time: %.6g s, volume: %.9e m3, heat: %.9e, salt: %.9e, kinetic energy: %.6e m5/s2, "
                "eta: volume %.3e m3, potential energy %.6e m5/s2"
                % (self.iteration, self.time, self.volume, self.T.first, self.S.first, self.kinetic_energy, self.eta.first,
                   self.eta_potential_energy))


class AveragesInfo(_Record):
    """gb25_averages_info (include/gb25.h): the groups and the window as begun, the samples and the sum of their weights so far,
    the clock at the first and at the last sample."""
    _fields_ = [("groups", C.c_int32), ("k_first", C.c_int32), ("k_count", C.c_int32), ("reserved", C.c_int32),
                ("samples", C.c_int64), ("first_iteration", C.c_int64), ("last_iteration", C.c_int64),
                ("weight_sum", C.c_double), ("first_time", C.c_double), ("last_time", C.c_double)]


class ParticlesInfo(_Record):
    """gb25_particles_info (include/gb25.h): how many particles and how much room; the accepted advance calls, their substeps and
    the model time they covered; the counters (PARTICLE_COUNTERS, then one reserved) of the last advance call and of all."""
    _fields_ = [("count", C.c_int64), ("capacity", C.c_int64), ("calls", C.c_int64), ("substeps", C.c_int64),
                ("time_advanced", C.c_double), ("last", C.c_int64 * 8), ("total", C.c_int64 * 8)]

    def counters(self, which="last"):
        """{name: count} of the last advance call (which = "last") or of all calls ("total")."""
        return dict(zip(PARTICLE_COUNTERS, getattr(self, which)))


class CheckpointInfo(_Record):
    """gb25_checkpoint_info (include/gb25.h): whether a snapshot waits to be written and whether its drain has finished; members,
    pieces and bytes of the restart set, the arena it passes through; whether averages or particles were open (they are not saved)."""
    _fields_ = [("taken", C.c_int32), ("drained", C.c_int32), ("members", C.c_int32), ("pieces", C.c_int32),
                ("bytes", C.c_int64), ("arena_bytes", C.c_int64),
                ("averages_open_not_saved", C.c_int32), ("particles_open_not_saved", C.c_int32)]


# the recorded result-changing options, in the order of the bits of gb25_restore_info.options_changed
RESTORED_OPTIONS = ("kernels", "pressure_precision", "momentum_chunk_levels", "tracer_chunk_levels", "w_on_the_fly", "substep_order",
                    "fold_pivot_slaved", "catke_stale_e_halos")


class RestoreInfo(_Record):
    """gb25_restore_info (include/gb25.h)."""
    _fields_ = [("members", C.c_int32), ("pieces", C.c_int32), ("bytes", C.c_int64), ("options_changed", C.c_uint32),
                ("tracer_rows_differ", C.c_int32), ("phy_stale", C.c_int32), ("reserved", C.c_int32)]

    def changed_options(self):
        return [n for q, n in enumerate(RESTORED_OPTIONS) if self.options_changed >> q & 1]


def average_group_of(name):
    """"means" | "squares" | "fluxes": the group a quantity of AVERAGE_IDS belongs to."""
    q = AVERAGE_IDS[name]
    return "means" if q <= AVERAGE_IDS["eta"] else "squares" if q <= AVERAGE_IDS["etaeta"] else "fluxes"


def average_groups_mask(groups):
    """The gb25_average_group mask of an iterable of group names (or of a mask)."""
    if isinstance(groups, int):
        return groups
    if isinstance(groups, str):
        groups = (groups,)
    mask = 0
    for g in groups:
        if g not in AVERAGE_GROUPS:
            raise ValueError(f"groups must be among {tuple(AVERAGE_GROUPS)}, got {g!r}")
        mask |= AVERAGE_GROUPS[g]
    return mask


class GB25Error(RuntimeError):
    pass


_libs = {}
_stale_loaded = set()   # float types whose library was loaded although its sources are newer


def library_stale(float_type="Float32"):
    """True when load_library fell back to a binary older than its sources (no compiler on the host, or GB25_ALLOW_STALE=1)."""
    return float_type in _stale_loaded


def load_library(float_type="Float32"):
    """Load libgb25hip.so (or its Float64 build); raises if it has not been built (no fallback path exists)."""
    if float_type not in LIB_PATHS:
        raise GB25Error(f"float type must be one of {sorted(LIB_PATHS)}, got {float_type!r}")
    if float_type in _libs:
        return _libs[float_type]
    path = LIB_PATHS[float_type]
    if not os.environ.get("GB25_LIB"):
        # a fresh checkout, or sources newer than the binary: compile (hipcc cross-compiles gfx950 anywhere).  The build
        # writes a temporary file and renames it under a lock, so concurrent ranks never load a half-written library.
        from .build import build_library, _stale
        if _stale(path):
            try:
                print(f"gb25_amd: building {os.path.basename(path)} with hipcc ...", flush=True)
                build_library(float_types=(float_type,))
            except Exception as e:
                if not os.path.exists(path):
                    raise GB25Error(
                        f"{path} not found and building it failed ({e}): run `python -c 'import __graft_entry__ as g; "
                        "g.build()'` (hipcc --offload-arch=gfx950).  gb25_amd has no CPU fallback.") from e
                # A loadable library exists but is older than its sources.  Loading it would let tests and bench.py report
                # numbers of a build that is not HEAD, so that is an error -- unless there is no compiler at all on this
                # host (FileNotFoundError: a box that only runs what was built elsewhere) or the caller opts in with
                # GB25_ALLOW_STALE=1.  Either way the fact is recorded (library_stale(), bench.py's "library_stale").
                no_compiler = isinstance(e, FileNotFoundError)
                if not (no_compiler or os.environ.get("GB25_ALLOW_STALE") == "1"):
                    raise GB25Error(
                        f"{path} is older than its sources and rebuilding it failed ({e}).  Fix the build, or set "
                        "GB25_ALLOW_STALE=1 (or GB25_LIB=1 to skip the check) to load the existing binary.") from e
                import warnings
                warnings.warn(f"gb25_amd: {path} is older than its sources and rebuilding it failed ({e}); "
                              "loading the existing binary", RuntimeWarning)
                _stale_loaded.add(float_type)
    if not os.path.exists(path):
        raise GB25Error(f"{path} not found.  gb25_amd has no CPU fallback.")
    # One HIP runtime per process.  PyTorch ships its own copies of libamdhip64 / libhsa-runtime64 / librccl; were this
    # library loaded first it would bind /opt/rocm's copies, a later `import torch` (gb25_amd.distributed, bench.py) would
    # bring a second runtime into the process, and the RCCL the exchanges find by soname -- torch's -- would sit on the
    # runtime that does not own the device (ncclCommInitRank: "no ROCm-capable device is detected").  With torch imported
    # first every HIP user of the process shares torch's copies.  (A host without PyTorch -- the Julia binding -- gets
    # /opt/rocm's throughout.)
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(path)
    P = C.c_void_p
    lib.gb25_version.restype = C.c_char_p
    lib.gb25_last_error_string.restype = C.c_char_p
    lib.gb25_last_error_string.argtypes = [P]
    lib.gb25_default_config.argtypes = [C.POINTER(Config), C.c_int32, C.c_int32, C.c_int32]
    lib.gb25_default_config.restype = None
    lib.gb25_create.argtypes = [C.POINTER(Config), C.POINTER(P)]
    lib.gb25_destroy.argtypes = [P]
    lib.gb25_destroy.restype = None
    lib.gb25_set_stream.argtypes = [P, P]
    lib.gb25_field_dims.argtypes = [P, C.c_int, C.c_int, C.POINTER(C.c_int32)]
    lib.gb25_set_field.argtypes = [P, C.c_int, P, C.c_int]
    lib.gb25_get_field.argtypes = [P, C.c_int, P, C.c_int]
    lib.gb25_field_device_ptr.argtypes = [P, C.c_int, C.POINTER(P)]
    lib.gb25_get_metric.argtypes = [P, C.c_int, C.c_int32, C.POINTER(C.c_double)]
    lib.gb25_get_metric2.argtypes = [P, C.c_int, C.POINTER(C.c_double), C.c_int64]
    lib.gb25_set_vertical_diffusivity.argtypes = [P, C.c_double, C.c_double]
    lib.gb25_set_closure_catke.argtypes = [P, C.c_int32]
    lib.gb25_set_tracer_advection_order.argtypes = [P, C.c_int32]
    lib.gb25_get_tracer_advection_order.argtypes = [P, C.POINTER(C.c_int32)]
    lib.gb25_set_bottom_drag.argtypes = [P, C.c_double]
    lib.gb25_get_bottom_drag.argtypes = [P, C.POINTER(C.c_double)]
    lib.gb25_default_catke_parameters.argtypes = [C.POINTER(CatkeParameters)]
    lib.gb25_default_catke_parameters.restype = None
    lib.gb25_set_catke_parameters.argtypes = [P, C.POINTER(CatkeParameters)]
    lib.gb25_get_catke_parameters.argtypes = [P, C.POINTER(CatkeParameters)]
    lib.gb25_set_prescribed_atmosphere.argtypes = [P, C.c_int, C.c_void_p]
    lib.gb25_get_vertical_diffusivity.argtypes = [P, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.gb25_get_substepping.argtypes = [P, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.gb25_get_clock.argtypes = [P, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_double)]
    lib.gb25_set_dt.argtypes = [P, C.c_double]
    lib.gb25_ab2_step.argtypes = [P, C.c_double, C.c_int]
    lib.gb25_correct_velocities_and_cache_previous_tendencies.argtypes = [P, C.c_double]
    lib.gb25_loop.argtypes = [P, C.c_int32]
    lib.gb25_save_state.argtypes = [P, C.c_char_p, C.c_char_p]
    lib.gb25_set_top_flux.argtypes = [P, C.c_int, P]
    lib.gb25_set_bottom_height.argtypes = [P, P]
    lib.gb25_set_curvilinear_grid.argtypes = [P, P, C.c_int32, C.c_int32]
    lib.gb25_set_vertical_faces.argtypes = [P, C.POINTER(C.c_double), C.c_int32]
    lib.gb25_get_bottom_info.argtypes = [P, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_double)]
    lib.gb25_set_option.argtypes = [P, C.c_int, C.c_int32]
    lib.gb25_get_option.argtypes = [P, C.c_int, C.POINTER(C.c_int32)]
    lib.gb25_comm_unique_id.argtypes = [P]
    lib.gb25_comm_info.argtypes = [P, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.gb25_debug_exchange_plan.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_char_p, C.c_int64]
    lib.gb25_debug_exchange_plan.restype = C.c_int64
    lib.gb25_comm_init_rccl.argtypes = [P, P]
    lib.gb25_comm_init_local.argtypes = [C.POINTER(P), C.c_int32]
    lib.gb25_comm_init_callback.argtypes = [P, EXCHANGE_FN, P]
    lib.gb25_comm_finalize.argtypes = [P]
    lib.gb25_debug_sequence.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_char_p, C.c_int64]
    lib.gb25_debug_sequence.restype = C.c_int64
    lib.gb25_lookahead_state.argtypes = [P, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.gb25_get_field_stats.argtypes = [P, C.c_int, C.c_int, C.POINTER(FieldStats)]
    lib.gb25_compare_field.argtypes = [P, C.c_int, C.c_int, P, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                       C.POINTER(FieldDiff)]
    lib.gb25_get_state_monitor.argtypes = [P, C.POINTER(StateMonitor)]
    lib.gb25_field_device_ptr_readonly.argtypes = [P, C.c_int, C.POINTER(P), C.POINTER(C.c_int32)]
    lib.gb25_integrate_field.argtypes = [P, C.c_int, C.c_int, P, C.c_int64]
    lib.gb25_get_budget.argtypes = [P, C.POINTER(Budget)]
    lib.gb25_derived_dims.argtypes = [P, C.c_int, C.POINTER(C.c_int32)]
    lib.gb25_compute_derived.argtypes = [P, C.c_int, C.c_double, C.c_int32, C.c_int32, C.POINTER(P), C.POINTER(C.c_int32)]
    lib.gb25_get_derived.argtypes = [P, C.c_int, C.c_double, C.c_int32, C.c_int32, P]
    lib.gb25_get_derived_stats.argtypes = [P, C.c_int, C.c_double, C.POINTER(FieldStats)]
    lib.gb25_get_field_levels.argtypes = [P, C.c_int, C.c_int32, C.c_int32, P]
    lib.gb25_get_transport.argtypes = [P, C.c_int, C.c_int, C.c_int32, C.c_int32, P, C.c_int64]
    lib.gb25_get_class_sums.argtypes = [P, C.c_int, C.c_int, P, C.c_int32, C.c_int, C.c_int32, C.c_int32, P, C.c_int64]
    lib.gb25_get_spectrum_table.argtypes = [P, P, P, C.c_int64]
    lib.gb25_get_zonal_spectrum.argtypes = [P, C.c_int, C.c_int32, C.c_int32, C.c_int32, C.c_int32, P, C.c_int64, C.POINTER(C.c_int64)]
    lib.gb25_get_derived_zonal_spectrum.argtypes = [P, C.c_int, C.c_double, C.c_int32, C.c_int32, C.c_int32, C.c_int32, P, C.c_int64,
                                                    C.POINTER(C.c_int64)]
    lib.gb25_compute_on_surfaces.argtypes = [P, C.c_int, C.c_int, P, C.c_int32, C.POINTER(P), C.POINTER(P), C.POINTER(C.c_int32)]
    lib.gb25_get_on_surfaces.argtypes = [P, C.c_int, C.c_int, P, C.c_int32, P, P]
    lib.gb25_stability_dims.argtypes = [P, C.c_int, C.POINTER(C.c_int32)]
    lib.gb25_compute_stability.argtypes = [P, C.c_int, C.c_double, C.c_int32, C.c_int32, C.POINTER(P), C.POINTER(C.c_int32)]
    lib.gb25_get_stability.argtypes = [P, C.c_int, C.c_double, C.c_int32, C.c_int32, P]
    lib.gb25_get_stability_stats.argtypes = [P, C.c_int, C.c_double, C.POINTER(FieldStats)]
    lib.gb25_kinematics_dims.argtypes = [P, C.c_int, C.POINTER(C.c_int32)]
    lib.gb25_compute_kinematics.argtypes = [P, C.c_int, C.c_int32, C.c_int32, C.c_int32, C.POINTER(P), C.POINTER(C.c_int32)]
    lib.gb25_get_kinematics.argtypes = [P, C.c_int, C.c_int32, C.c_int32, C.c_int32, P]
    lib.gb25_get_kinematics_stats.argtypes = [P, C.c_int, C.c_int32, C.POINTER(FieldStats)]
    lib.gb25_zonal_eddy_dims.argtypes = [P, C.POINTER(C.c_int32)]
    lib.gb25_get_zonal_eddy.argtypes = [P, C.c_int32, C.c_int32, P, P]
    lib.gb25_block_dims.argtypes = [P, C.c_int, C.POINTER(Blocks), C.POINTER(C.c_int32)]
    lib.gb25_derived_block_dims.argtypes = [P, C.c_int, C.POINTER(Blocks), C.POINTER(C.c_int32)]
    lib.gb25_get_block_sums.argtypes = [P, C.c_int, C.POINTER(Blocks), P, P, P, P, C.POINTER(BlockInfo)]
    lib.gb25_compute_block_sums.argtypes = [P, C.c_int, C.POINTER(Blocks), P, C.POINTER(BlockInfo), C.POINTER(P), C.POINTER(C.c_int32)]
    lib.gb25_get_derived_block_sums.argtypes = [P, C.c_int, C.c_double, C.POINTER(Blocks), P, P, P, P, C.POINTER(BlockInfo)]
    lib.gb25_filter_dims.argtypes = [P, C.c_int, C.POINTER(Filter), C.POINTER(C.c_int32)]
    lib.gb25_derived_filter_dims.argtypes = [P, C.c_int, C.POINTER(Filter), C.POINTER(C.c_int32)]
    lib.gb25_get_filter_sums.argtypes = [P, C.c_int, C.POINTER(Filter), P, P, P, P, P, P, C.POINTER(FilterInfo)]
    lib.gb25_compute_filter_sums.argtypes = [P, C.c_int, C.POINTER(Filter), P, P, P, C.POINTER(FilterInfo), C.POINTER(P), C.POINTER(C.c_int32)]
    lib.gb25_get_derived_filter_sums.argtypes = [P, C.c_int, C.c_double, C.POINTER(Filter), P, P, P, P, P, P, C.POINTER(FilterInfo)]
    lib.gb25_region_dims.argtypes = [P, C.POINTER(C.c_int32)]
    lib.gb25_label_regions.argtypes = [P, C.c_int, C.c_int32, C.c_int32, C.c_int32, C.c_int, C.c_double, C.c_int32, C.c_int32, C.c_int32,
                                       C.POINTER(P), C.POINTER(P), P]
    lib.gb25_get_regions.argtypes = [P, C.c_int, C.c_int32, C.c_int32, C.c_int32, C.c_int, C.c_double, C.c_int32, C.c_int32, C.c_int32, P, P, P]
    lib.gb25_averages_begin.argtypes = [P, C.c_int32, C.c_int32, C.c_int32]
    lib.gb25_averages_accumulate.argtypes = [P, C.c_double]
    lib.gb25_averages_get_info.argtypes = [P, C.POINTER(AveragesInfo)]
    lib.gb25_average_dims.argtypes = [P, C.c_int, C.POINTER(C.c_int32)]
    lib.gb25_get_average.argtypes = [P, C.c_int, C.c_int32, P, C.c_int64]
    lib.gb25_average_device_ptr.argtypes = [P, C.c_int, C.POINTER(P), C.POINTER(C.c_int32)]
    lib.gb25_averages_end.argtypes = [P]
    lib.gb25_checkpoint_snapshot.argtypes = [P, C.c_int64]
    lib.gb25_checkpoint_write.argtypes = [P, C.c_char_p, C.c_char_p]
    lib.gb25_checkpoint_get_info.argtypes = [P, C.POINTER(CheckpointInfo)]
    lib.gb25_checkpoint_release.argtypes = [P]
    lib.gb25_restore.argtypes = [P, C.c_char_p, C.c_char_p, C.POINTER(RestoreInfo)]
    lib.gb25_set_clock.argtypes = [P, C.c_double, C.c_int64, C.c_double]
    lib.gb25_particles_begin.argtypes = [P, C.c_int64]
    lib.gb25_particles_set.argtypes = [P, C.c_int64, C.c_int64, P, P, P, P, P, P]
    lib.gb25_particles_get.argtypes = [P, C.c_int64, C.c_int64, P, P, P, P, P, P, P]
    lib.gb25_particles_advance.argtypes = [P, C.c_double, C.c_int32]
    lib.gb25_particles_sample.argtypes = [P, C.c_int, P, C.c_int64]
    lib.gb25_particles_get_info.argtypes = [P, C.POINTER(ParticlesInfo)]
    lib.gb25_particles_end.argtypes = [P]
    lib.gb25_tracers_begin.argtypes = [P, C.c_int32, C.POINTER(TracerSpec), C.POINTER(P)]
    lib.gb25_tracers_set.argtypes = [P, P, C.c_int32, P, C.c_int]
    lib.gb25_tracers_get.argtypes = [P, P, C.c_int32, C.c_int32, P, C.c_int]
    lib.gb25_tracers_advance.argtypes = [P, P]
    lib.gb25_tracers_stats.argtypes = [P, P, C.c_int32, C.POINTER(FieldStats)]
    lib.gb25_tracers_clock.argtypes = [P, P, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    lib.gb25_tracers_end.argtypes = [P, P]
    lib.gb25_profile_enable.argtypes = [P, C.c_int]
    lib.gb25_profile_get.argtypes = [P, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_double)]
    for name in ["gb25_use_own_stream", "gb25_synchronize", "gb25_set_baroclinic_instability", "gb25_initialize",
                 "gb25_mask_immersed_fields", "gb25_fill_halo_regions", "gb25_compute_auxiliaries",
                 "gb25_fill_diffusivity_halos", "gb25_compute_momentum_tendencies",
                 "gb25_compute_tracer_tendencies", "gb25_compute_boundary_tendencies",
                 "gb25_compute_tendencies", "gb25_update_state", "gb25_first_time_step", "gb25_time_step",
                 "gb25_profile_reset"]:
        getattr(lib, name).argtypes = [P]
    lib.gb25_real_bytes.restype = C.c_int32
    if lib.gb25_real_bytes() != np.dtype(DTYPES[float_type]).itemsize:
        raise GB25Error(f"{path} holds {lib.gb25_real_bytes()}-byte elements, expected {float_type}")
    lib.gb25_config_bytes.restype = lib.gb25_catke_parameters_bytes.restype = C.c_int32
    if lib.gb25_config_bytes() != C.sizeof(Config) or lib.gb25_catke_parameters_bytes() != C.sizeof(CatkeParameters):
        raise GB25Error(f"{path}: gb25_config is {lib.gb25_config_bytes()} bytes there and {C.sizeof(Config)} in this binding "
                        f"(gb25_catke_parameters: {lib.gb25_catke_parameters_bytes()} / {C.sizeof(CatkeParameters)}): "
                        "the library and gb25_amd/binding.py are of different versions")
    for fn, struct in (("gb25_field_stats_bytes", FieldStats), ("gb25_field_diff_bytes", FieldDiff),
                       ("gb25_state_monitor_bytes", StateMonitor), ("gb25_moments_bytes", Moments),
                       ("gb25_budget_bytes", Budget), ("gb25_transport_bytes", Transport),
                       ("gb25_class_sum_bytes", ClassSum), ("gb25_spectral_coefficient_bytes", SpectralCoefficient),
                       ("gb25_averages_info_bytes", AveragesInfo), ("gb25_particles_info_bytes", ParticlesInfo),
                       ("gb25_tracer_spec_bytes", TracerSpec), ("gb25_zonal_eddy_bytes", ZonalEddyRow),
                       ("gb25_block_info_bytes", BlockInfo), ("gb25_filter_info_bytes", FilterInfo),
                       ("gb25_region_bytes", Region), ("gb25_regions_info_bytes", RegionsInfo),
                       ("gb25_checkpoint_info_bytes", CheckpointInfo), ("gb25_restore_info_bytes", RestoreInfo)):
        getattr(lib, fn).restype = C.c_int32
        if getattr(lib, fn)() != C.sizeof(struct):
            raise GB25Error(f"{path}: {fn}() = {getattr(lib, fn)()} there, {C.sizeof(struct)} bytes in this binding: "
                            "the library and gb25_amd/binding.py are of different versions")
    _libs[float_type] = lib
    return lib


class HipBackend:
    """One gb25_model handle.  Method names follow the phase list of
    GB-25 src/precompile.jl:31-42 and the entry points of src/timestepping_utils.jl:21-45."""

    def __init__(self, Nx, Ny, Nz, *, dt, halo=8, substeps=30, device=0, rank=0, nranks=1, float_type="Float32",
                 options=None, **overrides):
        float_type = getattr(float_type, "__name__", float_type)   # accepts "Float64", np.float64, ...
        float_type = {"float32": "Float32", "float64": "Float64"}.get(float_type, float_type)
        self.lib = load_library(float_type)
        self.float_type = float_type
        self.dtype = DTYPES[float_type]
        cfg = Config()
        self.lib.gb25_default_config(C.byref(cfg), Nx, Ny, Nz)
        cfg.halo, cfg.substeps, cfg.dt, cfg.device, cfg.rank, cfg.nranks = halo, substeps, dt, device, rank, nranks
        for k, v in overrides.items():
            if not hasattr(cfg, k):
                raise TypeError(f"unknown configuration field {k!r}")
            setattr(cfg, k, v)
        self.cfg = cfg
        self.h = C.c_void_p()
        st = self.lib.gb25_create(C.byref(cfg), C.byref(self.h))
        if st != 0:
            msg = self.lib.gb25_last_error_string(self.h).decode() if self.h else "gb25_create failed"
            if self.h:
                self.lib.gb25_destroy(self.h)
                self.h = None
            raise GB25Error(f"gb25_create: status {st}: {msg}")
        # Partition(Rx, Ry, 1): rank = ry Rx + rx owns Nx / Rx columns and Ny / Ry rows
        self.Ry = max(1, int(cfg.ranks_y))
        self.Rx = cfg.nranks // self.Ry
        self.rx, self.ry = cfg.rank % self.Rx, cfg.rank // self.Rx
        self.Nx_local, self.Ny_local = cfg.Nx // self.Rx, cfg.Ny // self.Ry
        self._keep = []            # ctypes callbacks handed to the library
        for k, v in (options or {}).items():
            self.set_option(k, v)

    def close(self):
        if getattr(self, "h", None):
            self.lib.gb25_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, st, what):
        if st != 0:
            raise GB25Error(f"{what}: status {st}: {self.lib.gb25_last_error_string(self.h).decode()}")

    def _call(self, name, *args):
        self._chk(getattr(self.lib, name)(self.h, *args), name)

    # ---- fields
    def field_dims(self, name, include_halos=True):
        d = (C.c_int32 * 3)()
        self._call("gb25_field_dims", FIELD_IDS[name], int(include_halos), d)
        return tuple(d)

    def get_field(self, name, include_halos=True):
        """numpy array shaped like parent(field) / interior(field), index order [i, j, k]."""
        d = self.field_dims(name, include_halos)
        out = np.empty(d[::-1], dtype=self.dtype)  # memory order is i fastest
        self._call("gb25_get_field", FIELD_IDS[name], out.ctypes.data_as(C.c_void_p), int(include_halos))
        return out.transpose(2, 1, 0)

    def set_field(self, name, array, include_halos=True):
        d = self.field_dims(name, include_halos)
        a = np.asarray(array, dtype=self.dtype)
        if a.ndim == 2:
            a = a[:, :, None]
        if a.shape != d:
            raise ValueError(f"{name}: expected shape {d}, got {a.shape}")
        buf = np.ascontiguousarray(a.transpose(2, 1, 0))
        self._call("gb25_set_field", FIELD_IDS[name], buf.ctypes.data_as(C.c_void_p), int(include_halos))

    def field_device_ptr(self, name):
        p = C.c_void_p()
        self._call("gb25_field_device_ptr", FIELD_IDS[name], C.byref(p))
        return p.value

    # ---- diagnostics on the device (no field crosses PCIe; read-only for the schedule)
    def field_stats(self, name, include_halos=False):
        """gb25_get_field_stats: min, max, max|x| and where, sums, non-finite count of the interior (or the parent)."""
        out = FieldStats()
        self._call("gb25_get_field_stats", FIELD_IDS[name], int(include_halos), C.byref(out))
        return out

    def field_device_ptr_readonly(self, name):
        """(device pointer of parent(field) for reading, the array's extents on the device); pins nothing, valid until the
        next call on this model."""
        p, d = C.c_void_p(), (C.c_int32 * 3)()
        self._call("gb25_field_device_ptr_readonly", FIELD_IDS[name], C.byref(p), d)
        return p.value, tuple(d)

    def compare_field(self, name, other, include_halos=False, *, other_name=None, real_bytes=None, dims=None, origin=None):
        """gb25_compare_field of this model's field `name` (a) against b.  other: another HipBackend of this process, of
        either float type (b = its field `other_name`, default the same name; interior against interior or parent against
        parent, b may be the larger) -- or a device pointer (int) with real_bytes, dims and origin given."""
        if isinstance(other, HipBackend):
            ptr, dims = other.field_device_ptr_readonly(other_name or name)
            real_bytes = np.dtype(other.dtype).itemsize
            h = 0 if include_halos else other.cfg.halo
            origin = (h, h, 0 if dims[2] == 1 else h)
        else:
            ptr = other
            if real_bytes is None or dims is None:
                raise TypeError("compare_field with a device pointer needs real_bytes and dims")
        out = FieldDiff()
        d = (C.c_int32 * 3)(*dims)
        o = (C.c_int32 * 3)(*origin) if origin is not None else None
        self._call("gb25_compare_field", FIELD_IDS[name], int(include_halos), C.c_void_p(ptr), int(real_bytes), d, o, C.byref(out))
        return out

    def state_monitor(self):
        """gb25_get_state_monitor: interior statistics of u, v, w, eta, T, S, the advective CFL rate, the clock."""
        out = StateMonitor()
        self._call("gb25_get_state_monitor", C.byref(out))
        return out

    def integrate_field(self, name, shape="total"):
        """gb25_integrate_field: sums weighted by the cell measure (include/gb25.h) over the interior, as numpy records of
        MOMENTS_DTYPE -- shape "rows": [j, k], one per row (zonal sums); "levels": [k]; "total": one record."""
        d = (C.c_int32 * 3)()
        if self.lib.gb25_field_dims(self.h, FIELD_IDS[name], 0, d) != 0:
            raise GB25Error(f"integrate_field: this model has no such field: {name!r} (closure = CATKEVerticalDiffusivity() only)")
        by, bz = d[1], d[2]
        n = {"rows": by * bz, "levels": bz, "total": 1}[shape]
        out = np.zeros(n, MOMENTS_DTYPE)
        self._call("gb25_integrate_field", FIELD_IDS[name], SUM_SHAPES[shape], out.ctypes.data_as(C.c_void_p), n)
        return out.reshape(bz, by).T if shape == "rows" else out if shape == "levels" else out[0]

    def budget(self):
        """gb25_get_budget: the totals of T, S, u, v, eta, volume, surface area, kinetic and free-surface potential energy."""
        out = Budget()
        self._call("gb25_get_budget", C.byref(out))
        return out

    # ---- derived fields on the device (include/gb25.h: vorticity, kinetic_energy, density_anomaly, potential_density,
    #      mixed_layer_depth); levels = (k_first, k_count), 0-based interior levels, k_count = -1 or levels = None: all
    def derived_dims(self, name):
        d = (C.c_int32 * 3)()
        self._call("gb25_derived_dims", DERIVED_IDS[name], d)
        return tuple(d)

    @staticmethod
    def _derived_args(name, param, levels):
        if name == "mixed_layer_depth" and param is None:
            param = 0.03
        k_first, k_count = (0, -1) if levels is None else levels
        return DERIVED_IDS[name], float(param or 0.0), int(k_first), int(k_count)

    def compute_derived(self, name, param=None, levels=None):
        """(device pointer, dims) of the packed result, elements of this backend's dtype, i fastest; read-only, valid until
        the next call on this model."""
        p, d = C.c_void_p(), (C.c_int32 * 3)()
        self._call("gb25_compute_derived", *self._derived_args(name, param, levels), C.byref(p), d)
        return p.value, tuple(d)

    def get_derived(self, name, param=None, levels=None):
        """numpy array [i, j, k] of the requested levels (a 2-D result: [i, j, 1]); only those are computed and copied."""
        q, param, k_first, k_count = self._derived_args(name, param, levels)
        d = self.derived_dims(name)
        nk = d[2] - k_first if k_count == -1 else k_count
        out = np.empty((max(nk, 0), d[1], d[0]), dtype=self.dtype)
        self._call("gb25_get_derived", q, param, k_first, k_count, out.ctypes.data_as(C.c_void_p))
        return out.transpose(2, 1, 0)

    def derived_stats(self, name, param=None):
        out = FieldStats()
        q, param, _, _ = self._derived_args(name, param, None)
        self._call("gb25_get_derived_stats", q, param, C.byref(out))
        return out

    def get_field_levels(self, name, k_first=0, k_count=-1):
        """Interior levels [k_first, k_first + k_count) of a field, [i, j, k]: gathered on the device, one copy."""
        d = self.field_dims(name, False)
        nk = d[2] - k_first if k_count == -1 else k_count
        out = np.empty((max(nk, 0), d[1], d[0]), dtype=self.dtype)
        self._call("gb25_get_field_levels", FIELD_IDS[name], int(k_first), int(k_count), out.ctypes.data_as(C.c_void_p))
        return out.transpose(2, 1, 0)

    def transport(self, faces, shape="lines", window=None):
        """gb25_get_transport: area, volume, heat and salt transport through the faces of v ("across_y", summed along i) or of
        u ("across_x", summed along j), as numpy records of TRANSPORT_DTYPE -- shape "lines": [n, k], one per line (row j /
        column i) and level; "profile": [n]; "streamfunction": [n, kf], the running sums at the Nz + 1 z faces.  window =
        (first, count) of the summed index, 0-based local interior, count = -1: to the end; None: all."""
        d = self.field_dims("v" if faces == "across_y" else "u", False)
        N, Nz = (d[1] if faces == "across_y" else d[0]), d[2]
        first, count = (0, -1) if window is None else window
        nk = {"lines": Nz, "profile": 1, "streamfunction": Nz + 1}[shape]
        out = np.zeros(N * nk, TRANSPORT_DTYPE)
        self._call("gb25_get_transport", TRANSPORT_FACES[faces], TRANSPORT_SHAPES[shape], int(first), int(count),
                   out.ctypes.data_as(C.c_void_p), out.size)
        return out if shape == "profile" else out.reshape(nk, N).T

    def class_sums(self, what, variable, edges, shape="rows", window=None):
        """gb25_get_class_sums: sums in the B = len(edges) + 1 classes of `variable` ("T", "S", "potential_density") over the
        faces of v ("faces_y": area, volume, heat and salt transport) or the cells of T ("cells": volume, 0, heat and salt
        content), as numpy records of CLASS_SUM_DTYPE -- shape "rows": [n, b], one per row j and bin; "cumulative": [n, e], the
        running sums over the bins from 0 (B + 1 of them); "total": [b], the rows added south to north.  window = (first,
        count) of i, 0-based local interior, count = -1: to the end; None: all."""
        N = self.field_dims("v" if what == "faces_y" else "T", False)[1]
        edges = np.ascontiguousarray(edges, np.float64).reshape(-1)
        B = edges.size + 1
        first, count = (0, -1) if window is None else window
        records = {"rows": N * B, "cumulative": N * (B + 1), "total": B}[shape]
        out = np.zeros(records, CLASS_SUM_DTYPE)
        self._call("gb25_get_class_sums", CLASS_WHAT[what], CLASS_VARIABLES[variable], edges.ctypes.data_as(C.c_void_p),
                   edges.size, CLASS_SHAPES[shape], int(first), int(count), out.ctypes.data_as(C.c_void_p), out.size)
        return out if shape == "total" else out.reshape(N, -1)

    # ---- zonal wavenumber spectra on the device (include/gb25.h: "zonal wavenumber spectra"; gb-25_amd/spectra.py)
    def spectrum_table(self):
        """gb25_get_spectrum_table: (c, s), cos and sin of 2 pi r / N for the N columns of the global grid -- the table of the
        definition, which the numpy restatement uses as it stands.  Needs no device."""
        N = int(self.cfg.Nx)
        c, s = np.empty(N, np.float64), np.empty(N, np.float64)
        self._call("gb25_get_spectrum_table", c.ctypes.data_as(C.c_void_p), s.ctypes.data_as(C.c_void_p), N)
        return c, s

    def zonal_spectrum(self, source, wavenumbers=None, levels=None, param=None):
        """gb25_get_zonal_spectrum / gb25_get_derived_zonal_spectrum: (X, nonfinite_lines), X complex128 [level, row, m], the
        coefficients A - i B of the direct transform along i of every interior line of `source` -- a field name or a derived
        name ("vorticity", "kinetic_energy", ..., "mixed_layer_depth" with param = the threshold).  wavenumbers = (m_first,
        m_count), m_count = -1 or None: up to N/2; levels = (k_first, k_count) as in get_field_levels, None: all.  A line with
        a value that is not finite has +0.0 coefficients and is counted in nonfinite_lines."""
        derived = source in DERIVED_IDS
        d = self.derived_dims(source) if derived else self.field_dims(source, False)
        m_first, m_count = (0, -1) if wavenumbers is None else (int(wavenumbers[0]), int(wavenumbers[1]))
        k_first, k_count = (0, -1) if levels is None else (int(levels[0]), int(levels[1]))
        mc = max(int(self.cfg.Nx) // 2 + 1 - m_first if m_count == -1 else m_count, 0)
        kc = max(d[2] - k_first if k_count == -1 else k_count, 0)
        out = np.zeros((kc, d[1], mc), np.complex128)
        bad = C.c_int64(0)
        tail = (m_first, m_count, k_first, k_count, out.ctypes.data_as(C.c_void_p), out.size, C.byref(bad))
        if derived:
            q, param, _, _ = self._derived_args(source, param, None)
            self._call("gb25_get_derived_zonal_spectrum", q, param, *tail)
        else:
            self._call("gb25_get_zonal_spectrum", FIELD_IDS[source], *tail)
        return out, int(bad.value)

    # ---- fields on surfaces on the device (include/gb25.h: "fields on surfaces"; gb-25_amd/surfaces.py).  variable: "T", "S",
    #      "potential_density", "depth"; carried: "depth", "T", "S", "e", "kinetic_energy", "density_anomaly", "potential_density"
    #      (or the ids of the header); values: 1 .. 64 finite targets, in any order
    @staticmethod
    def _surface_args(variable, carried, values):
        values = np.ascontiguousarray(np.atleast_1d(np.asarray(values, np.float64)).reshape(-1))
        return (int(SURFACE_VARIABLES.get(variable, variable)), int(SURFACE_CARRIED.get(carried, carried)),
                values.ctypes.data_as(C.c_void_p), values.size), values

    def compute_on_surfaces(self, variable, carried, values):
        """(device pointer of the results, device pointer of the status bytes, dims): both packed [Nx, Ny, n], i fastest, the
        results of this backend's dtype; read-only, valid until the next call on this model."""
        args, _keep = self._surface_args(variable, carried, values)
        p, ps, d = C.c_void_p(), C.c_void_p(), (C.c_int32 * 3)()
        self._call("gb25_compute_on_surfaces", *args, C.byref(p), C.byref(ps), d)
        return p.value, ps.value, tuple(d)

    def get_on_surfaces(self, variable, carried, values):
        """(result [i, j, n], status uint8 [i, j, n]): for every column and every value the depth of the surface `variable` =
        value (carried "depth") or the carried quantity interpolated onto it; status: SURFACE_STATUS."""
        args, _keep = self._surface_args(variable, carried, values)
        Nx, Ny, _ = self.field_dims("T", False)
        out = np.empty((args[3], Ny, Nx), dtype=self.dtype)
        status = np.empty((args[3], Ny, Nx), dtype=np.uint8)
        self._call("gb25_get_on_surfaces", *args, out.ctypes.data_as(C.c_void_p), status.ctypes.data_as(C.c_void_p))
        return out.transpose(2, 1, 0), status.transpose(2, 1, 0)

    # ---- stability diagnostics on the device (include/gb25.h: "stability diagnostics"; gb-25_amd/stability.py).  kind: "n2",
    #      "shear2", "richardson", "eady_rate", "ertel_pv" at (c,c,f), "wave_speed" 2-D (or the ids of the header); param: the floor
    #      of the Richardson number (on S2, > 0) or of the Eady rate (on N2, >= 0); levels = (k_first, k_count) of the Nz + 1
    #      faces, 0-based, k_count = -1 or levels = None: all
    def stability_dims(self, kind):
        d = (C.c_int32 * 3)()
        self._call("gb25_stability_dims", int(STABILITY_IDS.get(kind, kind)), d)
        return tuple(d)

    @staticmethod
    def _stability_args(kind, param, levels):
        if param is None:
            param = STABILITY_DEFAULT_PARAM.get(kind, 0.0)
        k_first, k_count = (0, -1) if levels is None else levels
        return int(STABILITY_IDS.get(kind, kind)), float(param), int(k_first), int(k_count)

    def compute_stability(self, kind, param=None, levels=None):
        """(device pointer, dims) of the packed result, elements of this backend's dtype, i fastest; read-only, valid until
        the next call on this model."""
        p, d = C.c_void_p(), (C.c_int32 * 3)()
        self._call("gb25_compute_stability", *self._stability_args(kind, param, levels), C.byref(p), d)
        return p.value, tuple(d)

    def get_stability(self, kind, param=None, levels=None):
        """numpy array [i, j, face] of the requested faces (the wave speed: [i, j, 1]); only those are computed and copied."""
        q, param, k_first, k_count = self._stability_args(kind, param, levels)
        Nx, Ny, Nz = self.field_dims("T", False)
        nf = 1 if q == STABILITY_IDS["wave_speed"] else Nz + 1
        nk = nf - k_first if k_count == -1 else k_count
        out = np.empty((max(nk, 0), Ny, Nx), dtype=self.dtype)
        self._call("gb25_get_stability", q, param, k_first, k_count, out.ctypes.data_as(C.c_void_p))
        return out.transpose(2, 1, 0)

    def stability_stats(self, kind, param=None):
        """gb25_get_stability_stats: gb25_field_stats of the whole diagnostic."""
        out = FieldStats()
        q, param, _, _ = self._stability_args(kind, param, None)
        self._call("gb25_get_stability_stats", q, param, C.byref(out))
        return out

    # ---- flow kinematics on the device (include/gb25.h: "flow kinematics"; gb-25_amd/kinematics.py).  kind: "divergence",
    #      "normal_strain", "okubo_weiss", "gradient", "frontogenesis" at (c,c,c), "shear_strain", "rossby_number" at (f,f,c) (or the
    #      ids of the header); param: the tracer of the gradient and of the frontogenesis function -- "T", "S",
    #      "potential_density" or 0 .. 2 --, None or 0 for the others; levels = (k_first, k_count), 0-based, k_count = -1 or
    #      levels = None: all
    def kinematics_dims(self, kind):
        d = (C.c_int32 * 3)()
        self._call("gb25_kinematics_dims", int(KINEMATICS_IDS.get(kind, kind)), d)
        return tuple(d)

    @staticmethod
    def _kinematics_args(kind, param, levels):
        k_first, k_count = (0, -1) if levels is None else levels
        param = 0 if param is None else KINEMATICS_TRACERS.get(param, param)
        return int(KINEMATICS_IDS.get(kind, kind)), int(param), int(k_first), int(k_count)

    def compute_kinematics(self, kind, param=None, levels=None):
        """(device pointer, dims) of the packed result, elements of this backend's dtype, i fastest; read-only, valid until
        the next diagnostics call on this model."""
        p, d = C.c_void_p(), (C.c_int32 * 3)()
        self._call("gb25_compute_kinematics", *self._kinematics_args(kind, param, levels), C.byref(p), d)
        return p.value, tuple(d)

    def get_kinematics(self, kind, param=None, levels=None):
        """numpy array [i, j, k] of the requested levels; only those are computed and copied."""
        q, param, k_first, k_count = self._kinematics_args(kind, param, levels)
        d = (C.c_int32 * 3)()
        if self.lib.gb25_kinematics_dims(self.h, q, d) != 0:          # (an unknown id: the call below says so by name)
            d[0], d[1], d[2] = self.field_dims("T", False)
        nk = d[2] - k_first if k_count == -1 else k_count
        out = np.empty((max(nk, 0), d[1], d[0]), dtype=self.dtype)
        self._call("gb25_get_kinematics", q, param, k_first, k_count, out.ctypes.data_as(C.c_void_p))
        return out.transpose(2, 1, 0)

    def kinematics_stats(self, kind, param=None):
        """gb25_get_kinematics_stats: gb25_field_stats of the whole quantity."""
        out = FieldStats()
        q, param, _, _ = self._kinematics_args(kind, param, None)
        self._call("gb25_get_kinematics_stats", q, param, C.byref(out))
        return out

    # ---- zonal-mean and eddy statistics on the device (include/gb25.h: "zonal-mean and eddy statistics"; gb-25_amd/eddies.py)
    def zonal_eddy_dims(self):
        """gb25_zonal_eddy_dims: (rows, levels) of this rank's line records.  Needs no device."""
        d = (C.c_int32 * 2)()
        self._call("gb25_zonal_eddy_dims", d)
        return tuple(d)

    def zonal_eddy(self, levels=None, means=None):
        """gb25_get_zonal_eddy: the line records of the levels (k_first, k_count) (None: all), numpy records of ZONAL_EDDY_DTYPE
        [j, kk].  means: None, or float64 [j, kk, 6] -- the means the deviations are taken about (echoed in "mean")."""
        Ny, Nz = self.zonal_eddy_dims()
        k_first, k_count = (0, -1) if levels is None else (int(levels[0]), int(levels[1]))
        nk = Nz - k_first if k_count == -1 else k_count
        out = np.zeros((max(nk, 1), Ny), ZONAL_EDDY_DTYPE)      # (a window the library will refuse still gets a buffer)
        mp = None
        if means is not None:
            mh = np.ascontiguousarray(np.asarray(means, np.float64).transpose(1, 0, 2))
            if mh.shape != (nk, Ny, 6):
                raise ValueError(f"means: expected shape {(Ny, nk, 6)}, got {np.shape(means)}")
            mp = mh.ctypes.data_as(C.c_void_p)
        self._call("gb25_get_zonal_eddy", k_first, k_count, mp, out.ctypes.data_as(C.c_void_p))
        return out.T

    # ---- block sums on the device (include/gb25.h: "block sums"; gb-25_amd/blocks.py).  source: a field name or a derived name at
    #      (c,c) ("kinetic_energy", "density_anomaly", "potential_density", "mixed_layer_depth" with param = the threshold);
    #      block = (bx, by, bz); levels = (k_first, k_count) of the field's own levels, k_count = -1 or levels = None: all;
    #      level_weights: one float64 per level of the field, or None
    @staticmethod
    def _block_args(block, levels, level_weights):
        k_first, k_count = (0, -1) if levels is None else levels
        bx, by, bz = block
        blocks = Blocks(int(bx), int(by), int(bz), int(k_first), int(k_count), 0)
        lw = None if level_weights is None else np.ascontiguousarray(level_weights, np.float64).reshape(-1)
        return blocks, lw

    def _block_levels(self, source):
        if source in DERIVED_IDS:
            return self.derived_dims(source)[2]
        if source not in FIELD_IDS:
            raise GB25Error(f"block sums: no field and no derived field {source!r}")
        return self.field_dims(source, False)[2]

    def _checked_weights(self, source, lw):
        # (the library reads one weight per level of the field: a vector of another length never reaches it)
        if lw is not None and lw.size != self._block_levels(source) and self._block_levels(source) > 1:
            raise GB25Error(f"block sums: level_weight has {lw.size} entries, {source!r} has {self._block_levels(source)} levels")
        return None if lw is None else lw.ctypes.data_as(C.c_void_p)

    def block_dims(self, source, block, levels=None):
        """gb25_block_dims / gb25_derived_block_dims: (Nx / bx, Ny / by, k_count / bz) after the checks of the blocks and the
        window.  Needs no device."""
        blocks, _ = self._block_args(block, levels, None)
        d = (C.c_int32 * 3)()
        if source in DERIVED_IDS:
            self._call("gb25_derived_block_dims", DERIVED_IDS[source], C.byref(blocks), d)
        else:
            self._block_levels(source)
            self._call("gb25_block_dims", FIELD_IDS[source], C.byref(blocks), d)
        return tuple(d)

    def block_sums(self, source, block, levels=None, level_weights=None, param=None, planes=("measure", "first", "second")):
        """gb25_get_block_sums / gb25_get_derived_block_sums: blocks.BlockSums with the planes asked for, [I, J, K] float64 each
        (the others None; only those are copied), and the info record."""
        from .blocks import BlockSums
        blocks, lw = self._block_args(block, levels, level_weights)
        dims = self.block_dims(source, block, levels)
        out = {n: (np.empty(dims[::-1], np.float64) if n in planes else None) for n in ("measure", "first", "second")}
        ptrs = [None if a is None else a.ctypes.data_as(C.c_void_p) for a in out.values()]
        info = BlockInfo()
        w = self._checked_weights(source, lw)
        if source in DERIVED_IDS:
            q, param, _, _ = self._derived_args(source, param, None)
            self._call("gb25_get_derived_block_sums", q, param, C.byref(blocks), w, *ptrs, C.byref(info))
        else:
            self._call("gb25_get_block_sums", FIELD_IDS[source], C.byref(blocks), w, *ptrs, C.byref(info))
        m, t, s = (None if a is None else a.transpose(2, 1, 0) for a in out.values())
        return BlockSums(m, t, s, block=block, dims=tuple(info.dims), points=info.points, nonfinite=info.nonfinite,
                         empty_blocks=info.empty_blocks, global_offset=tuple(info.global_offset))

    def compute_block_sums(self, field, block, levels=None, level_weights=None):
        """(device pointer, dims, BlockInfo): the planes measure | first | second one after another, dims[0] dims[1] dims[2]
        doubles each, I fastest; read-only, valid until the next call on this model."""
        blocks, lw = self._block_args(block, levels, level_weights)
        self._block_levels(field)
        p, d, info = C.c_void_p(), (C.c_int32 * 3)(), BlockInfo()
        self._call("gb25_compute_block_sums", FIELD_IDS[field], C.byref(blocks), self._checked_weights(field, lw), C.byref(info),
                   C.byref(p), d)
        return p.value, tuple(d), info

    # ---- moving-window filter on the device (include/gb25.h: "moving-window filter"; gb-25_amd/filters.py).  source: as for the
    #      block sums; radius = (rx, ry) in grid points; stride = (sx, sy); levels = (k_first, k_count) of the field's own levels;
    #      wx, wy: 2 rx + 1 and 2 ry + 1 float64 weights or None (the box); rx_of_row: one int32 per row or None
    def _filter_args(self, radius, stride, levels, wx, wy, rx_of_row):
        k_first, k_count = (0, -1) if levels is None else levels
        (rx, ry), (sx, sy) = radius, stride
        flt = Filter(int(rx), int(ry), int(sx), int(sy), int(k_first), int(k_count), 0)
        # (the library reads 2 r + 1 weights and one radius per row: a vector of another length never reaches it)
        keep = []
        for name, w, n, dtype in (("wx", wx, 2 * flt.rx + 1, np.float64), ("wy", wy, 2 * flt.ry + 1, np.float64),
                                  ("rx_of_row", rx_of_row, self.field_dims("T", False)[1], np.int32)):
            if w is None:
                keep.append(None)
                continue
            a = np.ascontiguousarray(w, dtype).reshape(-1)
            if a.size != n and n > 0:
                raise GB25Error(f"filter sums: {name} has {a.size} entries, the call needs {n}")
            keep.append(a)
        return flt, keep, [None if a is None else a.ctypes.data_as(C.c_void_p) for a in keep]

    def filter_dims(self, source, radius, stride=(1, 1), levels=None):
        """gb25_filter_dims / gb25_derived_filter_dims: (Nx / sx, Ny / sy, k_count) after the checks of the window.  Needs no
        device."""
        k_first, k_count = (0, -1) if levels is None else levels
        flt = Filter(int(radius[0]), int(radius[1]), int(stride[0]), int(stride[1]), int(k_first), int(k_count), 0)
        d = (C.c_int32 * 3)()
        if source in DERIVED_IDS:
            self._call("gb25_derived_filter_dims", DERIVED_IDS[source], C.byref(flt), d)
        else:
            self._block_levels(source)
            self._call("gb25_filter_dims", FIELD_IDS[source], C.byref(flt), d)
        return tuple(d)

    def filter_sums(self, source, radius, stride=(1, 1), levels=None, wx=None, wy=None, rx_of_row=None, param=None,
                    planes=("measure", "first", "second")):
        """gb25_get_filter_sums / gb25_get_derived_filter_sums: filters.FilterSums with the planes asked for, [I, J, K] float64
        each (the others None; only those are copied), and the info record."""
        from .filters import FilterSums
        dims = self.filter_dims(source, radius, stride, levels)
        flt, keep, w = self._filter_args(radius, stride, levels, wx, wy, rx_of_row)
        out = {n: (np.empty(dims[::-1], np.float64) if n in planes else None) for n in ("measure", "first", "second")}
        ptrs = [None if a is None else a.ctypes.data_as(C.c_void_p) for a in out.values()]
        info = FilterInfo()
        if source in DERIVED_IDS:
            q, param, _, _ = self._derived_args(source, param, None)
            self._call("gb25_get_derived_filter_sums", q, param, C.byref(flt), *w, *ptrs, C.byref(info))
        else:
            self._call("gb25_get_filter_sums", FIELD_IDS[source], C.byref(flt), *w, *ptrs, C.byref(info))
        m, t, s = (None if a is None else a.transpose(2, 1, 0) for a in out.values())
        return FilterSums(m, t, s, radius=radius, stride=stride, dims=tuple(info.dims), nonfinite=info.nonfinite, empty=info.empty,
                          clipped=info.clipped, global_offset=tuple(info.global_offset))

    def compute_filter_sums(self, field, radius, stride=(1, 1), levels=None, wx=None, wy=None, rx_of_row=None):
        """(device pointer, dims, FilterInfo): the planes measure | first | second one after another, dims[0] dims[1] dims[2]
        doubles each, I fastest; read-only, valid until the next call on this model."""
        self._block_levels(field)
        flt, keep, w = self._filter_args(radius, stride, levels, wx, wy, rx_of_row)
        p, d, info = C.c_void_p(), (C.c_int32 * 3)(), FilterInfo()
        self._call("gb25_compute_filter_sums", FIELD_IDS[field], C.byref(flt), *w, C.byref(info), C.byref(p), d)
        return p.value, tuple(d), info

    # ---- coherent regions on the device (include/gb25.h: "coherent regions"; gb-25_amd/regions.py).  source: "T", "S", "e"; a
    #      derived name at (c,c,c) ("kinetic_energy", "density_anomaly", "potential_density"); a kinematics name at (c,c,c)
    #      ("divergence", "normal_strain", "okubo_weiss", "gradient", "frontogenesis", the last two with param = their tracer) -- or
    #      (kind, id) of the header's enumerations; cmp: "below" | "above"; levels = (k_first, k_count), k_count = -1 or None: all
    def region_dims(self):
        """gb25_region_dims: (Nx, Ny, levels).  Needs no device."""
        d = (C.c_int32 * 3)()
        self._call("gb25_region_dims", d)
        return tuple(d)

    @staticmethod
    def _region_args(source, param, carry, cmp, threshold, levels, max_regions):
        if isinstance(source, tuple):
            kind, q = REGION_SOURCES.get(source[0], source[0]), source[1]
        elif source in KINEMATICS_IDS:
            kind, q = REGION_SOURCES["kinematics"], KINEMATICS_IDS[source]
        elif source in DERIVED_IDS:
            kind, q = REGION_SOURCES["derived"], DERIVED_IDS[source]
        elif source in FIELD_IDS:
            kind, q = REGION_SOURCES["field"], FIELD_IDS[source]
        else:
            raise GB25Error(f"regions: no field, derived field or kinematics quantity {source!r}")
        if carry is not None and carry not in FIELD_IDS and not isinstance(carry, int):
            raise GB25Error(f"regions: carried_field: no field {carry!r}")
        k_first, k_count = (0, -1) if levels is None else levels
        param = 0 if param is None else KINEMATICS_TRACERS.get(param, param)
        return (int(kind), int(q), int(param), -1 if carry is None else int(FIELD_IDS.get(carry, carry)), int(REGION_CMP.get(cmp, cmp)),
                float(threshold), int(k_first), int(k_count), int(max_regions))

    def _region_buffers(self, args):
        """(args with max_regions clamped, levels of the window, records per level) for the host buffers of a call.  A level holds
        at most ceil(Nx Ny / 2) regions, so a larger max_regions is clamped to that: no record is lost.  What the library will
        refuse -- a window outside the levels, max_regions < 1 -- gets the smallest buffers and is passed on for its named refusal."""
        Nx, Ny, Nz = self.region_dims()
        k_first, k_count, cap = args[6], args[7], args[8]
        nk = Nz - k_first if k_count == -1 else k_count
        if not (0 <= k_first < Nz and 1 <= nk <= Nz - k_first):
            nk = 1
        if cap >= 1:
            cap = min(cap, (Nx * Ny + 1) // 2)
        return args[:8] + (cap,), nk, max(cap, 1)

    def get_regions(self, source, cmp, threshold, levels=None, carry=None, max_regions=4096, param=None, labels=True):
        """gb25_get_regions: (labels int32 [i, j, kk] or None, records REGION_DTYPE [kk, max_regions], infos REGIONS_INFO_DTYPE
        [kk]); the records of a level beyond its `stored` are zero.  labels=False: only records and infos cross PCIe.  max_regions
        beyond ceil(Nx Ny / 2), the most a level can hold, is clamped to that."""
        args, nk, cap = self._region_buffers(self._region_args(source, param, carry, cmp, threshold, levels, max_regions))
        Nx, Ny, _ = self.region_dims()
        lab = np.empty((nk, Ny, Nx), np.int32) if labels else None
        rec = np.zeros((nk, cap), REGION_DTYPE)
        info = np.zeros(nk, REGIONS_INFO_DTYPE)
        self._call("gb25_get_regions", *args, None if lab is None else lab.ctypes.data_as(C.c_void_p), rec.ctypes.data_as(C.c_void_p),
                   info.ctypes.data_as(C.c_void_p))
        return (None if lab is None else lab.transpose(2, 1, 0)), rec, info

    def label_regions(self, source, cmp, threshold, levels=None, carry=None, max_regions=4096, param=None):
        """gb25_label_regions: (device pointer of the label planes, device pointer of the records, infos); read-only, valid until the
        next call on this model.  max_regions is clamped as for get_regions: the records of level kk start at kk times that."""
        args, nk, _ = self._region_buffers(self._region_args(source, param, carry, cmp, threshold, levels, max_regions))
        info = np.zeros(nk, REGIONS_INFO_DTYPE)
        pl, pr = C.c_void_p(), C.c_void_p()
        self._call("gb25_label_regions", *args, C.byref(pl), C.byref(pr), info.ctypes.data_as(C.c_void_p))
        return pl.value, pr.value, info

    # ---- time averages accumulated on the device (include/gb25.h: "time averages and eddy fluxes"); names: AVERAGE_IDS
    def averages_begin(self, groups=("means", "squares", "fluxes"), levels=None):
        """gb25_averages_begin: allocate and zero the accumulators of `groups` ("means" must be among them) over the cell levels
        levels = (k_first, k_count), 0-based, k_count = -1 or levels = None: all.  Starts over if averages exist."""
        k_first, k_count = (0, -1) if levels is None else levels
        self._call("gb25_averages_begin", average_groups_mask(groups), int(k_first), int(k_count))

    def averages_accumulate(self, weight=1.0):
        """gb25_averages_accumulate: acc = acc + weight * term for every quantity of the active groups, one launch."""
        self._call("gb25_averages_accumulate", float(weight))

    def averages_info(self):
        out = AveragesInfo()
        self._call("gb25_averages_get_info", C.byref(out))
        return out

    def average_dims(self, name):
        d = (C.c_int32 * 3)()
        self._call("gb25_average_dims", AVERAGE_IDS[name], d)
        return tuple(d)

    def get_average(self, name, normalized=True):
        """float64 array [i, j, k] over the active window: the accumulator (normalized = False) or accumulator / weight_sum."""
        d = self.average_dims(name)
        out = np.empty(d[::-1], np.float64)
        self._call("gb25_get_average", AVERAGE_IDS[name], int(bool(normalized)), out.ctypes.data_as(C.c_void_p), out.size)
        return out.transpose(2, 1, 0)

    def average_device_ptr(self, name):
        """(device pointer of the packed fp64 accumulator, its dims); read-only, valid until averages_begin / averages_end."""
        p, d = C.c_void_p(), (C.c_int32 * 3)()
        self._call("gb25_average_device_ptr", AVERAGE_IDS[name], C.byref(p), d)
        return p.value, tuple(d)

    def averages_end(self):
        self._call("gb25_averages_end")

    # ---- Lagrangian particles on the device (include/gb25.h: "Lagrangian particles advected and sampled on the device")
    def particles_begin(self, capacity):
        """gb25_particles_begin: room for `capacity` particles; starts over if the model has particles."""
        self._call("gb25_particles_begin", int(capacity))

    def particles_set(self, i, j, k, a, b, c, first=0):
        """gb25_particles_set: particles [first, first + len(i)) from host arrays, ACTIVE; first + len(i) becomes the count."""
        ints = [np.ascontiguousarray(x, np.int32).reshape(-1) for x in (i, j, k)]
        dbl = [np.ascontiguousarray(x, np.float64).reshape(-1) for x in (a, b, c)]
        n = ints[0].size
        if any(x.size != n for x in ints + dbl):
            raise ValueError("particles_set: i, j, k, a, b, c must have the same length")
        self._call("gb25_particles_set", int(first), n, *[x.ctypes.data_as(C.c_void_p) for x in ints + dbl])

    def particles_get(self, first=0, count=None):
        """gb25_particles_get: {"i", "j", "k" (int32), "a", "b", "c" (float64), "status" (int32)} of particles [first, first + count)."""
        n = self.particles_info().count - first if count is None else int(count)
        out = {q: np.zeros(max(n, 0), np.int32) for q in ("i", "j", "k")}
        out.update({q: np.zeros(max(n, 0), np.float64) for q in ("a", "b", "c")})
        out["status"] = np.zeros(max(n, 0), np.int32)
        self._call("gb25_particles_get", int(first), n, *[out[q].ctypes.data_as(C.c_void_p) for q in ("i", "j", "k", "a", "b", "c", "status")])
        return out

    def particles_advance(self, dt, substeps=1):
        """gb25_particles_advance: `substeps` midpoint substeps of dt / substeps on the fields as they are now; one launch."""
        self._call("gb25_particles_advance", float(dt), int(substeps))

    def particles_sample(self, name):
        """gb25_particles_sample: the value of the (c,c,c) field `name` in every particle's cell, float64 [n]."""
        out = np.zeros(self.particles_info().count, np.float64)
        self._call("gb25_particles_sample", FIELD_IDS[name], out.ctypes.data_as(C.c_void_p), out.size)
        return out

    def particles_info(self):
        out = ParticlesInfo()
        self._call("gb25_particles_get_info", C.byref(out))
        return out

    def particles_end(self):
        self._call("gb25_particles_end")

    # ---- passive tracers carried beside the run (include/gb25.h: "passive tracers carried beside a run"; gb-25_amd/passive.py)
    def tracers_begin(self, specs):
        """gb25_tracers_begin: a set of len(specs) tracers (TracerSpec, or dicts of its fields); returns the set's handle."""
        specs = [s if isinstance(s, TracerSpec) else TracerSpec(**s) for s in specs]
        arr = (TracerSpec * max(len(specs), 1))(*specs)
        out = C.c_void_p()
        self._call("gb25_tracers_begin", len(specs), arr, C.byref(out))
        return out

    def tracers_set(self, handle, n, array, include_halos=False):
        """gb25_tracers_set: tracer n from an array shaped like T's interior (or parent); the next advance is an Euler step."""
        d = self.field_dims("T", include_halos)
        a = np.asarray(array, dtype=self.dtype)
        if a.shape != d:
            raise ValueError(f"tracer {n}: expected shape {d}, got {a.shape}")
        buf = np.ascontiguousarray(a.transpose(2, 1, 0))
        self._call("gb25_tracers_set", handle, int(n), buf.ctypes.data_as(C.c_void_p), int(include_halos))

    def tracers_get(self, handle, n, which="c", include_halos=False):
        """gb25_tracers_get: "c", "Gn" (the tendency of the last advance) or "Gm" (the one before) of tracer n, index order [i, j, k]."""
        d = self.field_dims("T", include_halos)
        out = np.empty(d[::-1], dtype=self.dtype)
        self._call("gb25_tracers_get", handle, int(n), TRACER_ARRAYS[which], out.ctypes.data_as(C.c_void_p), int(include_halos))
        return out.transpose(2, 1, 0)

    def tracers_advance(self, handle):
        """gb25_tracers_advance: the set over one dt with u, v, w as they stand; before the model's step."""
        self._call("gb25_tracers_advance", handle)

    def tracers_stats(self, handle, n):
        out = FieldStats()
        self._call("gb25_tracers_stats", handle, int(n), C.byref(out))
        return out

    def tracers_clock(self, handle):
        """(time, iteration) of the set."""
        t, it = C.c_double(), C.c_int64()
        self._call("gb25_tracers_clock", handle, C.byref(t), C.byref(it))
        return t.value, it.value

    def tracers_end(self, handle):
        self._call("gb25_tracers_end", handle)

    def metric(self, name, index=1):
        v = C.c_double()
        self._call("gb25_get_metric", METRIC_IDS[name], index, C.byref(v))
        return v.value

    def set_catke(self, on=True):
        self._call("gb25_set_closure_catke", int(on))

    def catke_parameters(self):
        p = CatkeParameters()
        self._call("gb25_get_catke_parameters", C.byref(p))
        return p

    def set_catke_parameters(self, **changes):
        """Changes some of CATKE's parameters (names of gb25_catke_parameters; arrays as 4-sequences psi = u, c, e, D)."""
        p = self.catke_parameters()
        for k, v in changes.items():
            if not hasattr(p, k):
                raise TypeError(f"unknown CATKE parameter {k!r}")
            if isinstance(getattr(p, k), float):
                setattr(p, k, float(v))
            else:
                for q in range(4):
                    getattr(p, k)[q] = float(v[q])
        self._call("gb25_set_catke_parameters", C.byref(p))

    def set_vertical_diffusivity(self, nu, kappa):
        self._call("gb25_set_vertical_diffusivity", float(nu), float(kappa))

    def set_tracer_advection_order(self, order):
        """tracer_advection = WENO(order = 5) (the default) or WENO(order = 7) (ClimaOcean's ocean_simulation)."""
        self._call("gb25_set_tracer_advection_order", int(order))

    def tracer_advection_order(self):
        v = C.c_int32()
        self._call("gb25_get_tracer_advection_order", C.byref(v))
        return v.value

    def set_bottom_drag(self, Cd):
        """Quadratic bottom drag coefficient (ClimaOcean's ocean_simulation: 0.003); 0: none."""
        self._call("gb25_set_bottom_drag", float(Cd))

    def bottom_drag(self):
        v = C.c_double()
        self._call("gb25_get_bottom_drag", C.byref(v))
        return v.value

    def set_prescribed_atmosphere(self, name, values):
        """One field of the PrescribedAtmosphere at the cell centres, halo cells included: (Nx + 2H, Ny + 2H) [i, j]; None
        clears it.  name: u | v | T | q | p | shortwave | longwave."""
        f = ATMOSPHERE_IDS[name]
        if values is None:
            self._call("gb25_set_prescribed_atmosphere", f, None)
            return
        H = self.cfg.halo
        a = np.ascontiguousarray(np.asarray(values, np.float64).reshape(self.Nx_local + 2 * H, self.Ny_local + 2 * H).T)
        self._call("gb25_set_prescribed_atmosphere", f, a.ctypes.data_as(C.c_void_p))

    def compute_atmosphere_ocean_fluxes(self):
        self._call("gb25_compute_atmosphere_ocean_fluxes")

    def top_flux(self, name):
        """The top flux boundary condition of u | v | T | S as the device holds it (interior points of the field)."""
        d = self.field_dims(name, False)
        a = np.empty((d[1], d[0]), self.dtype)
        self._call("gb25_get_top_flux", FIELD_IDS[name], a.ctypes.data_as(C.c_void_p))
        return a.T

    def vertical_diffusivity(self):
        nu, kappa = C.c_double(), C.c_double()
        self._call("gb25_get_vertical_diffusivity", C.byref(nu), C.byref(kappa))
        return nu.value, kappa.value

    def metric2(self, name):
        """One horizontal metric of a curvilinear grid (grid_type >= 2): (Nx + 2H, Ny + 2H + 1) float64, [i, j]."""
        H = self.cfg.halo
        shape = (self.Ny_local + 2 * H + 1, self.Nx_local + 2 * H)
        out = np.empty(shape, np.float64)
        self._call("gb25_get_metric2", METRIC2_IDS.index(name), out.ctypes.data_as(C.POINTER(C.c_double)), out.size)
        return out.T

    def substepping(self):
        n, frac = C.c_int32(), C.c_double()
        w = (C.c_double * 4096)()
        self._call("gb25_get_substepping", C.byref(n), C.byref(frac), w)
        return n.value, frac.value, np.array(w[: n.value])

    def clock(self):
        t, it, dt = C.c_double(), C.c_int64(), C.c_double()
        self._call("gb25_get_clock", C.byref(t), C.byref(it), C.byref(dt))
        return t.value, it.value, dt.value

    def set_dt(self, dt):
        self._call("gb25_set_dt", float(dt))

    def set_stream(self, stream_ptr):
        """stream_ptr: a hipStream_t as an integer (0 / None = HIP's default stream)."""
        self._call("gb25_set_stream", C.c_void_p(stream_ptr or None))

    def use_own_stream(self):
        self._call("gb25_use_own_stream")

    # ---- phases / composites (one ABI call each)
    def synchronize(self): self._call("gb25_synchronize")
    def set_baroclinic_instability(self): self._call("gb25_set_baroclinic_instability")
    def initialize(self): self._call("gb25_initialize")
    def mask_immersed_fields(self): self._call("gb25_mask_immersed_fields")
    def fill_halo_regions(self): self._call("gb25_fill_halo_regions")
    def compute_auxiliaries(self): self._call("gb25_compute_auxiliaries")
    def fill_diffusivity_halos(self): self._call("gb25_fill_diffusivity_halos")
    def compute_momentum_tendencies(self): self._call("gb25_compute_momentum_tendencies")
    def compute_tracer_tendencies(self): self._call("gb25_compute_tracer_tendencies")
    def compute_boundary_tendencies(self): self._call("gb25_compute_boundary_tendencies")
    def compute_tendencies(self): self._call("gb25_compute_tendencies")
    def ab2_step(self, dt, euler=False): self._call("gb25_ab2_step", float(dt), int(euler))
    def correct_velocities_and_cache_previous_tendencies(self, dt=0.0):
        self._call("gb25_correct_velocities_and_cache_previous_tendencies", float(dt))
    def update_state(self): self._call("gb25_update_state")
    def first_time_step(self): self._call("gb25_first_time_step")
    def time_step(self): self._call("gb25_time_step")
    def loop(self, n): self._call("gb25_loop", int(n))

    def save_state(self, directory, label="checkpoint"):
        """save_model_state: this rank's slab -> <directory>/<label>/fields_rank<R>.npz; returns the path."""
        self._call("gb25_save_state", str(directory).encode(), str(label).encode())
        return os.path.join(str(directory), label, f"fields_rank{self.cfg.rank}.npz")

    # ---- checkpoint and restart (include/gb25.h: "checkpoint and bit-for-bit restart")
    def checkpoint_path(self, directory, label="checkpoint"):
        return os.path.join(str(directory), label, f"restart_rank{self.cfg.rank}.gb25")

    def checkpoint_snapshot(self, max_arena_bytes=0):
        """gb25_checkpoint_snapshot: the restart set into the device arena in one launch; the drain to the host runs beside whatever
        the model does next."""
        self._call("gb25_checkpoint_snapshot", int(max_arena_bytes))

    def checkpoint_write(self, directory, label="checkpoint"):
        """gb25_checkpoint_write: waits for the drain, writes the file; returns its path."""
        self._call("gb25_checkpoint_write", str(directory).encode(), str(label).encode())
        return self.checkpoint_path(directory, label)

    def checkpoint_info(self):
        out = CheckpointInfo()
        self._call("gb25_checkpoint_get_info", C.byref(out))
        return out

    def checkpoint_release(self): self._call("gb25_checkpoint_release")

    def restore(self, directory, label="checkpoint"):
        """gb25_restore: fields, clock, scalar state and recorded options of <directory>/<label>/restart_rank<R>.gb25; a refusal
        (GB25Error naming what differs) leaves the model untouched."""
        out = RestoreInfo()
        self._call("gb25_restore", str(directory).encode(), str(label).encode(), C.byref(out))
        return out

    def set_clock(self, time, iteration, last_dt):
        self._call("gb25_set_clock", float(time), int(iteration), float(last_dt))

    def set_top_flux(self, name, J):
        """FluxBoundaryCondition at the top of u | v | T | S: interior-shaped array (None: back to no-flux)."""
        if J is None:
            self._call("gb25_set_top_flux", FIELD_IDS[name], None)
            return
        d = self.field_dims(name, False)
        a = np.ascontiguousarray(np.asarray(J, dtype=self.dtype).reshape(d[0], d[1]).T)
        self._call("gb25_set_top_flux", FIELD_IDS[name], a.ctypes.data_as(C.c_void_p))

    # ---- immersed boundary
    def set_bottom_height(self, zb):
        """GridFittedBottom(zb): bottom height at the GLOBAL cell centres, shape (Nx_global, Ny) (a slab takes its columns,
        its neighbours' and its fold partner's from it: every rank passes the same array)."""
        a = np.ascontiguousarray(np.asarray(zb, dtype=np.float64).T)      # i fastest
        if a.shape != (self.cfg.Ny, self.cfg.Nx):
            raise ValueError(f"bottom height: expected shape ({self.cfg.Nx}, {self.cfg.Ny})")
        self._call("gb25_set_bottom_height", a.ctypes.data_as(C.c_void_p))

    # ---- the host's grid
    def set_curvilinear_grid(self, metrics):
        """metrics: {name: array} for the 14 names of METRIC2_IDS (dxfc ... azff, fff, phicc), each the parent array over the
        GLOBAL grid, shape (Nx_global + 2H, Ny + 2H) or (Nx_global + 2H, Ny + 2H + 1) -- grid.Δxᶠᶜᵃ etc. of the host's grid."""
        H = self.cfg.halo
        arrs = [np.ascontiguousarray(np.asarray(metrics[n], dtype=np.float64).T) for n in METRIC2_IDS]
        ny, nx = arrs[0].shape
        if nx != self.cfg.Nx + 2 * H or any(a.shape != (ny, nx) for a in arrs):
            raise ValueError(f"metrics: {len(METRIC2_IDS)} arrays of shape ({self.cfg.Nx + 2 * H}, {self.cfg.Ny + 2 * H} [+ 1])")
        ptrs = (C.POINTER(C.c_double) * len(arrs))(*[a.ctypes.data_as(C.POINTER(C.c_double)) for a in arrs])
        self._call("gb25_set_curvilinear_grid", ptrs, nx, ny)

    def set_vertical_faces(self, zf):
        """grid.z faces, bottom to top: Nz + 1 values."""
        a = np.ascontiguousarray(np.asarray(zf, dtype=np.float64))
        self._call("gb25_set_vertical_faces", a.ctypes.data_as(C.POINTER(C.c_double)), int(a.size))

    def bottom_info(self, which, i, j):
        """1-based (i, j) like the Julia sources; which: kbot | Hfc | Hcf."""
        v = C.c_double()
        self._call("gb25_get_bottom_info", {"kbot": 0, "Hfc": 1, "Hcf": 2}[which], i - 1, j - 1, C.byref(v))
        return v.value

    # ---- options (gb25_option)
    def set_option(self, name, value):
        self._call("gb25_set_option", OPTION_IDS[name], int(value))

    def get_option(self, name):
        v = C.c_int32()
        self._call("gb25_get_option", OPTION_IDS[name], C.byref(v))
        return v.value

    def lookahead_state(self):
        """(velocity look-ahead of the next step exists, stage 0 of this step adopted the sub-cycle look-ahead)"""
        a, b = C.c_int32(), C.c_int32()
        self._call("gb25_lookahead_state", C.byref(a), C.byref(b))
        return bool(a.value), bool(b.value)

    # ---- exchange context of a slab (x decomposition)
    def comm_unique_id(self):
        """128 bytes from ncclGetUniqueId (rank 0 calls this and hands them to every rank)."""
        buf = C.create_string_buffer(UNIQUE_ID_BYTES)
        st = self.lib.gb25_comm_unique_id(buf)
        if st != 0:
            raise GB25Error(f"gb25_comm_unique_id: status {st} (librccl could not be loaded?)")
        return buf.raw

    def comm_init_rccl(self, unique_id):
        if len(unique_id) != UNIQUE_ID_BYTES:
            raise ValueError("unique id must be 128 bytes")
        self._call("gb25_comm_init_rccl", C.c_char_p(bytes(unique_id)))

    def comm_info(self):
        """(transport, comm_ranks): "none" | "rccl" | "local" | "callback", and the communicator's size as RCCL reports it."""
        t, n = C.c_int32(0), C.c_int32(0)
        self._call("gb25_comm_info", C.byref(t), C.byref(n))
        return ("none", "rccl", "local", "callback")[t.value], n.value

    def comm_init_callback(self, fn):
        """fn(buffer_set, send_west, send_east, recv_west, recv_east, nbytes) with device pointers as integers."""
        def trampoline(user, b, sw, se, rw, re, nbytes):
            try:
                fn(b, sw, se, rw, re, nbytes)
                return 0
            except Exception as e:     # never let an exception cross the C frames
                print(f"gb25_amd: exchange callback failed: {e!r}", flush=True)
                return 1
        cb = EXCHANGE_FN(trampoline)
        self._keep.append(cb)
        self._call("gb25_comm_init_callback", cb, None)

    def comm_finalize(self):
        self._call("gb25_comm_finalize")

    @staticmethod
    def comm_init_local(backends):
        """All slabs of one decomposition in this process: ring of device copies; the composites of any member step all."""
        b0 = backends[0]
        arr = (C.c_void_p * len(backends))(*[b.h for b in backends])
        b0._chk(b0.lib.gb25_comm_init_local(arr, len(backends)), "gb25_comm_init_local")

    # ---- timers
    def profile_enable(self, on=True, only=None):
        """on: time every kernel; only="momentum"|"gu"|...: time that kernel alone (least perturbation)."""
        self._call("gb25_profile_enable", 2 + KERNEL_IDS[only] if only else int(on))
    def profile_reset(self): self._call("gb25_profile_reset")

    def profile_get(self, kernel):
        n, ms = C.c_int64(), C.c_double()
        self._call("gb25_profile_get", KERNEL_IDS[kernel], C.byref(n), C.byref(ms))
        return n.value, ms.value
