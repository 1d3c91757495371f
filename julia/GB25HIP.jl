# GB25HIP.jl -- Julia binding of libgb25hip.so (the C ABI of include/gb25.h).
#
# The host-language side of the drop-in boundary: GB-25 is a Julia package (src/GordonBell25.jl) and this module is
# what its maintainers would `include` to run the HydrostaticFreeSurfaceModel time-step loop on MI355X through the
# hand-written HIP library instead of through Reactant/XLA.  It keeps the GordonBell25 entry points
# (first_time_step!, time_step!, loop! -- src/timestepping_utils.jl:21-45) and the per-phase workloads
# (src/precompile.jl:31-127) as one `ccall` each.  No KernelAbstractions, no AMDGPU.jl code generation: the kernels are
# prebuilt; AMDGPU.jl is only needed if zero-copy `ROCArray` views of the fields are wanted (see `device_view`).
#
# STATUS: written against include/gb25.h without a Julia installation at hand (none exists in the build image or on
# the GPU box); it has not been executed.  The ctypes binding gb-25_amd/binding.py is the one the test-suite runs, and
# this file mirrors it call for call.
module GB25HIP

export Config, Model, create, destroy!, first_time_step!, time_step!, loop!, initialize!, update_state!,
       fill_halo_regions!, compute_auxiliaries!, compute_tendencies!, ab2_step!, mask_immersed_fields!,
       correct_velocities_and_cache_previous_tendencies!, set_baroclinic_instability!, synchronize,
       parent_array, interior_array, set_parent!, set_interior!, clock, set_dt!, set_option!, get_option,
       comm_unique_id, comm_init_rccl!, comm_finalize!, set_top_flux!, set_bottom_height!, set_vertical_diffusivity!, set_closure_catke!, CatkeParameters, default_catke_parameters, set_catke_parameters!, set_bottom_drag!, set_tracer_advection_order!, set_prescribed_atmosphere!, compute_atmosphere_ocean_fluxes!, metric2, FIELD, OPTION, METRIC2,
       FieldStats, FieldDiff, StateMonitor, field_stats, compare_field, state_monitor, device_pointer_readonly,
       Moments, Budget, integrate_field, budget, SUM_ROWS, SUM_LEVELS, SUM_TOTAL,
       Transport, transport, overturning, ACROSS_Y, ACROSS_X, TR_LINES, TR_PROFILE, TR_STREAMFUNCTION,
       DERIVED, derived_dims, compute_derived, get_derived, derived_stats, field_levels,
       STABILITY, stability_dims, compute_stability, get_stability, stability_stats,
       KINEMATICS, KIN_TRACER, kinematics_dims, compute_kinematics, get_kinematics, kinematics_stats,
       Blocks, BlockInfo, block_dims, block_sums, compute_block_sums, derived_block_sums,
       AVG_MEANS, AVG_SQUARES, AVG_FLUXES, AVERAGE, AveragesInfo, averages_begin, averages_accumulate, averages_info, average_dims,
       get_average, averages_end,
       TracerSpec, TracerSet, tracers_begin, tracers_set!, tracers_get, tracers_advance!, tracers_stats, tracers_clock, tracers_end!,
       run_with_tracers!

# One library per Oceananigans float type (src/arg_parsing.jl:12-16): Float32 -> libgb25hip.so, Float64 ->
# libgb25hip_f64.so; same symbols, gb25_real_bytes() tells them apart.
const LIBS = Dict(Float32 => get(ENV, "GB25HIP_LIB", "libgb25hip.so"),
                  Float64 => get(ENV, "GB25HIP_LIB_F64", "libgb25hip_f64.so"))

# gb25_field (include/gb25.h)
const FIELD = (u = 0, v = 1, w = 2, T = 3, S = 4, pHY = 5,
               Gn_u = 6, Gn_v = 7, Gn_T = 8, Gn_S = 9, Gm_u = 10, Gm_v = 11, Gm_T = 12, Gm_S = 13,
               eta = 14, U = 15, V = 16, eta_bar = 17, U_bar = 18, V_bar = 19, Gn_U = 20, Gn_V = 21,
               # closure = CATKEVerticalDiffusivity() (exist after set_closure_catke!)
               e = 22, Gn_e = 23, Gm_e = 24, κu = 25, κc = 26, κe = 27, Le = 28, Jb = 29,
               # diffusivity_fields.previous_velocities (u, v at the previous compute_diffusivities!)
               previous_u = 30, previous_v = 31)
# gb25_option
const OPTION = (kernels = 0, ab2_lookahead = 1, subcycle_lookahead = 2, subcycle_block = 3, fill_fused = 4,
                two_streams = 5, store_pressure = 6, split_tendencies = 7, pressure_precision = 8,
                immersed_kernels = 9, fold_fills = 10, lazy_corrector = 11, momentum_chunk_levels = 12, tracer_chunk_levels = 13,
                tracers_first = 14, w_on_the_fly = 15, sub_stream_priority = 16, subcycle_whole = 17, early_strips = 18,
                # restatement choices a Julia dump settles (DESIGN.md section 0), and two run-time knobs
                catke_stale_e_halos = 19, comm_timeout_seconds = 20, roctx_ranges = 21, substep_order = 22, fold_pivot_slaved = 23, pressure_form = 24, spectrum_table = 25)

# mirror of gb25_config; isbits, passed by reference
Base.@kwdef mutable struct Config
    Nx::Int32 = 0
    Ny::Int32 = 0
    Nz::Int32 = 0
    halo::Int32 = 8                 # halo = (8, 8, 8) in every GB-25 script
    substeps::Int32 = 30            # SplitExplicitFreeSurface(substeps=30), src/baroclinic_instability_model.jl:22
    rank::Int32 = 0
    nranks::Int32 = 1
    device::Int32 = 0
    dt::Float64 = 60.0              # model.clock.last_Δt, src/baroclinic_instability_model.jl:82
    chi::Float64 = 0.1
    lat_south::Float64 = -80.0
    lat_north::Float64 = 80.0
    lon_west::Float64 = 0.0
    lon_east::Float64 = 360.0
    depth::Float64 = 4000.0
    zexp_h::Float64 = 30.0
    g::Float64 = 9.80665
    Omega::Float64 = 7.292115e-5
    radius::Float64 = 6371e3
    rho0::Float64 = 1020.0
    slab_mode::Int32 = 0
    grid_type::Int32 = 0            # gb25_grid_type: 0 = :simple_lat_lon, 1 = the Gaussian islands on the lat-lon grid,
                                    # 3 = TripolarGrid, 4 = :gaussian_islands (TripolarGrid + GridFittedBottom)
    ranks_y::Int32 = 1              # Partition(Rx, Ry, 1) (sharding/sharded_baroclinic_instability_simulation_run.jl:65-72):
                                    # Ry; nranks = Rx Ry, rank = ry Rx + rx; 1: x slabs
end

mutable struct Model{FT}
    ptr::Ptr{Cvoid}
    lib::String
    cfg::Config
end

struct GB25Error <: Exception
    msg::String
end
Base.showerror(io::IO, e::GB25Error) = print(io, "GB25Error: ", e.msg)

function check(m::Model, status::Integer, what::AbstractString)
    status == 0 && return nothing
    msg = unsafe_string(ccall((:gb25_last_error_string, m.lib), Cstring, (Ptr{Cvoid},), m.ptr))
    throw(GB25Error("$what failed with status $status: $msg"))   # a Julia exception on the Julia side of the ABI only
end

"""
    create(FT, cfg) -> Model{FT}

`baroclinic_instability_model(arch, Nx, Ny, Nz; Δt, halo, free_surface=SplitExplicitFreeSurface(substeps=...))`
(src/baroclinic_instability_model.jl:17-85): builds the grid metrics, allocates every field zeroed on the device.
"""
function create(::Type{FT}, cfg::Config) where {FT<:Union{Float32,Float64}}
    lib = LIBS[FT]
    nbytes = ccall((:gb25_real_bytes, lib), Int32, ())
    nbytes == sizeof(FT) || throw(GB25Error("$lib holds $(nbytes)-byte elements, expected $FT"))
    # the mirror of gb25_config must be the library's struct, field for field (a field added there must not shift silently here)
    cbytes = ccall((:gb25_config_bytes, lib), Int32, ())
    cbytes == sizeof(Config) || throw(GB25Error("gb25_config is $cbytes bytes in $lib and $(sizeof(Config)) in this binding"))
    out = Ref{Ptr{Cvoid}}(C_NULL)
    st = ccall((:gb25_create, lib), Cint, (Ref{Config}, Ref{Ptr{Cvoid}}), cfg, out)
    m = Model{FT}(out[], lib, cfg)
    if st != 0
        msg = m.ptr == C_NULL ? "gb25_create failed" :
              unsafe_string(ccall((:gb25_last_error_string, lib), Cstring, (Ptr{Cvoid},), m.ptr))
        m.ptr == C_NULL || ccall((:gb25_destroy, lib), Cvoid, (Ptr{Cvoid},), m.ptr)
        throw(GB25Error("gb25_create: status $st: $msg"))
    end
    finalizer(destroy!, m)
    return m
end

"""
    create(FT, Nx, Ny, Nz; Δt, halo=8, substeps=30, kw...)
"""
function create(::Type{FT}, Nx::Integer, Ny::Integer, Nz::Integer; Δt, halo = 8, substeps = 30, kw...) where {FT}
    cfg = Config(; Nx = Nx, Ny = Ny, Nz = Nz, dt = Δt, halo = halo, substeps = substeps, kw...)
    return create(FT, cfg)
end

function destroy!(m::Model)
    if m.ptr != C_NULL
        ccall((:gb25_destroy, m.lib), Cvoid, (Ptr{Cvoid},), m.ptr)
        m.ptr = C_NULL
    end
    return nothing
end

# ---- the phases (src/precompile.jl:31-42) and the composites (src/timestepping_utils.jl:21-45): one ccall each
for (jl, c) in ((:first_time_step!, :gb25_first_time_step),
                (:time_step!, :gb25_time_step),
                (:initialize!, :gb25_initialize),
                (:update_state!, :gb25_update_state),
                (:mask_immersed_fields!, :gb25_mask_immersed_fields),
                (:fill_halo_regions!, :gb25_fill_halo_regions),
                (:compute_auxiliaries!, :gb25_compute_auxiliaries),
                (:fill_diffusivity_halos!, :gb25_fill_diffusivity_halos),
                (:compute_momentum_tendencies!, :gb25_compute_momentum_tendencies),
                (:compute_tracer_tendencies!, :gb25_compute_tracer_tendencies),
                (:compute_boundary_tendencies!, :gb25_compute_boundary_tendencies),
                (:compute_tendencies!, :gb25_compute_tendencies),
                (:set_baroclinic_instability!, :gb25_set_baroclinic_instability),
                (:synchronize, :gb25_synchronize),
                (:comm_finalize!, :gb25_comm_finalize))
    @eval $jl(m::Model) = check(m, ccall(($(QuoteNode(c)), m.lib), Cint, (Ptr{Cvoid},), m.ptr), $(string(c)))
end

loop!(m::Model, Ninner::Integer) =
    check(m, ccall((:gb25_loop, m.lib), Cint, (Ptr{Cvoid}, Int32), m.ptr, Ninner), "gb25_loop")
ab2_step!(m::Model, Δt::Real, euler::Bool = false) =
    check(m, ccall((:gb25_ab2_step, m.lib), Cint, (Ptr{Cvoid}, Float64, Cint), m.ptr, Δt, euler), "gb25_ab2_step")
correct_velocities_and_cache_previous_tendencies!(m::Model, Δt::Real = 0.0) =
    check(m, ccall((:gb25_correct_velocities_and_cache_previous_tendencies, m.lib), Cint, (Ptr{Cvoid}, Float64),
                   m.ptr, Δt), "gb25_correct_velocities_and_cache_previous_tendencies")

# ---- FluxBoundaryCondition at the top of u, v, T, S (what ocean_simulation's coupled fluxes fill every step;
# src/data_free_ocean_climate_model.jl:26, src/precompile.jl:52-61): J at the interior points, positive upward
function set_top_flux!(m::Model{FT}, field::Integer, J::Union{Nothing, AbstractMatrix}) where FT
    a = J === nothing ? nothing : convert(Matrix{FT}, J)          # values in the model's float type
    p = a === nothing ? Ptr{Cvoid}(C_NULL) : Ptr{Cvoid}(pointer(a))
    GC.@preserve a check(m, ccall((:gb25_set_top_flux, m.lib), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}), m.ptr, field, p),
                         "gb25_set_top_flux")
end
# closure = VerticalScalarDiffusivity(VerticallyImplicitTimeDiscretization(), κ, ν) (src/baroclinic_instability_model.jl:31);
# ν = κ = 0: closure = nothing
set_vertical_diffusivity!(m::Model; ν::Real = 0, κ::Real = 0) =
    check(m, ccall((:gb25_set_vertical_diffusivity, m.lib), Cint, (Ptr{Cvoid}, Float64, Float64), m.ptr, ν, κ),
          "gb25_set_vertical_diffusivity")
# closure = CATKEVerticalDiffusivity() (src/baroclinic_instability_model.jl:30): tracers = (:T, :S, :e), diffusivity fields
# κu, κc, κe, Le, Jb; once after creation, before the initial state is set
set_closure_catke!(m::Model, on::Bool = true) =
    check(m, ccall((:gb25_set_closure_catke, m.lib), Cint, (Ptr{Cvoid}, Int32), m.ptr, on), "gb25_set_closure_catke")
# data-free forcing (src/data_free_ocean_climate_model.jl:12-70): one field of the PrescribedAtmosphere at the ocean's cell
# centres, halo cells included ((Nx + 2H) x (Ny + 2H) Float64); all seven set => coupled: first_time_step! / loop! compute the
# similarity-theory fluxes after every step and keep them in the top flux boundary conditions
const ATMOSPHERE = (u = 0, v = 1, T = 2, q = 3, p = 4, shortwave = 5, longwave = 6)
set_prescribed_atmosphere!(m::Model, field::Symbol, values::AbstractMatrix) =
    check(m, ccall((:gb25_set_prescribed_atmosphere, m.lib), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}), m.ptr,
                   getproperty(ATMOSPHERE, field), convert(Matrix{Float64}, values)), "gb25_set_prescribed_atmosphere")
compute_atmosphere_ocean_fluxes!(m::Model) =
    check(m, ccall((:gb25_compute_atmosphere_ocean_fluxes, m.lib), Cint, (Ptr{Cvoid},), m.ptr), "gb25_compute_atmosphere_ocean_fluxes")
# tracer_advection = WENO(order = 5) (default) | WENO(order = 7) (ClimaOcean's ocean_simulation)
set_tracer_advection_order!(m::Model, order::Integer) =
    check(m, ccall((:gb25_set_tracer_advection_order, m.lib), Cint, (Ptr{Cvoid}, Int32), m.ptr, order), "gb25_set_tracer_advection_order")
# quadratic bottom drag (ClimaOcean's ocean_simulation: bottom_drag_coefficient = 0.003); 0: none
set_bottom_drag!(m::Model, Cd::Real) =
    check(m, ccall((:gb25_set_bottom_drag, m.lib), Cint, (Ptr{Cvoid}, Float64), m.ptr, Cd), "gb25_set_bottom_drag")
# mirror of gb25_catke_parameters (isbits; the arrays are psi = u, c, e, D); defaults: default_catke_parameters()
struct CatkeParameters
    Cs::Float64; Cb::Float64; Csp::Float64; CRid::Float64; CRi0::Float64
    Chi::NTuple{4, Float64}; Clo::NTuple{4, Float64}; Cun::NTuple{4, Float64}; Cc::NTuple{4, Float64}; Ce::NTuple{4, Float64}
    CWu::Float64; CWw::Float64
    minimum_tke::Float64; minimum_convective_buoyancy_flux::Float64; negative_tke_damping_time_scale::Float64
    CWeps::Float64      # bottom TKE flux coefficient (CATKEEquation's Cᵂϵ)
end
function default_catke_parameters(lib)
    p = Ref{CatkeParameters}()
    ccall((:gb25_default_catke_parameters, lib), Cvoid, (Ptr{CatkeParameters},), p)
    return p[]
end
set_catke_parameters!(m::Model, p::CatkeParameters) =
    check(m, ccall((:gb25_set_catke_parameters, m.lib), Cint, (Ptr{Cvoid}, Ptr{CatkeParameters}), m.ptr, Ref(p)),
          "gb25_set_catke_parameters")
# GridFittedBottom(bottom_height): heights at the GLOBAL cell centres, (Nx_global, Ny) (every rank passes the same array)
set_bottom_height!(m::Model, zb::AbstractMatrix) =
    check(m, ccall((:gb25_set_bottom_height, m.lib), Cint, (Ptr{Cvoid}, Ptr{Float64}), m.ptr, convert(Matrix{Float64}, zb)),
          "gb25_set_bottom_height")

# ---- the HOST's grid: the model steps on Oceananigans' own numbers, not on the library's stand-in generators.
# `grid` is the underlying OrthogonalSphericalShellGrid (TripolarGrid(arch; size, halo, z), src/model_utils.jl:134-137) built on
# CPU() over the GLOBAL domain; the 14 arrays go in gb25_metric2 order as the parents of grid.Δxᶠᶜᵃ ..., (Nx + 2H, Ny + 2H).
function set_curvilinear_grid!(m::Model, grid; Ω = 7.292115e-5)
    P(name) = convert(Matrix{Float64}, collect(parent(getproperty(grid, name)))[:, :, 1])
    fff = 2Ω .* sind.(P(:φᶠᶠᵃ))                                   # HydrostaticSphericalCoriolis at (Face, Face)
    arrays = [P(:Δxᶠᶜᵃ), P(:Δxᶜᶜᵃ), P(:Δxᶜᶠᵃ), P(:Δxᶠᶠᵃ), P(:Δyᶠᶜᵃ), P(:Δyᶜᶜᵃ), P(:Δyᶜᶠᵃ), P(:Δyᶠᶠᵃ),
              P(:Azᶜᶜᵃ), P(:Azᶠᶜᵃ), P(:Azᶜᶠᵃ), P(:Azᶠᶠᵃ), fff, P(:φᶜᶜᵃ)]
    nx, ny = size(arrays[1])
    ptrs = [pointer(a) for a in arrays]
    GC.@preserve arrays check(m, ccall((:gb25_set_curvilinear_grid, m.lib), Cint, (Ptr{Cvoid}, Ptr{Ptr{Float64}}, Int32, Int32),
                                       m.ptr, ptrs, nx, ny), "gb25_set_curvilinear_grid")
end
# grid.z faces, bottom to top: exponential_z_faces(Nz, depth) in the reference (src/model_utils.jl:56-62)
function set_vertical_faces!(m::Model, grid)
    Nz, Hz = grid.Nz, grid.Hz
    zf = convert(Vector{Float64}, collect(parent(grid.z.cᵃᵃᶠ))[Hz + 1:Hz + Nz + 1])
    check(m, ccall((:gb25_set_vertical_faces, m.lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int32), m.ptr, zf, length(zf)),
          "gb25_set_vertical_faces")
end
# everything an ImmersedBoundaryGrid(TripolarGrid, GridFittedBottom) holds (src/model_utils.jl:129-146), in one call
function set_grid!(m::Model, ibg)
    grid = ibg.underlying_grid
    set_curvilinear_grid!(m, grid)
    set_vertical_faces!(m, grid)
    Hx, Hy = grid.Hx, grid.Hy
    zb = collect(parent(ibg.immersed_boundary.bottom_height))[Hx + 1:Hx + grid.Nx, Hy + 1:Hy + grid.Ny, 1]
    set_bottom_height!(m, zb)
end
# gb25_metric2: horizontal metrics of an orthogonal curvilinear grid (grid_type >= 2) by location
const METRIC2 = (dxfc = 0, dxcc = 1, dxcf = 2, dxff = 3, dyfc = 4, dycc = 5, dycf = 6, dyff = 7,
                 azcc = 8, azfc = 9, azcf = 10, azff = 11, fff = 12, phicc = 13)
function metric2(m::Model, id::Integer, Nx::Integer, Ny::Integer, H::Integer)
    a = Matrix{Float64}(undef, Nx + 2H, Ny + 2H + 1)        # parent layout of a (Center, Face) field
    check(m, ccall((:gb25_get_metric2, m.lib), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}, Int64), m.ptr, id, a, length(a)),
          "gb25_get_metric2")
    return a
end

set_option!(m::Model, opt::Integer, value::Integer) =
    check(m, ccall((:gb25_set_option, m.lib), Cint, (Ptr{Cvoid}, Cint, Int32), m.ptr, opt, value), "gb25_set_option")
function get_option(m::Model, opt::Integer)
    v = Ref{Int32}(0)
    check(m, ccall((:gb25_get_option, m.lib), Cint, (Ptr{Cvoid}, Cint, Ref{Int32}), m.ptr, opt, v), "gb25_get_option")
    return v[]
end

# ---- clock: model.clock (src/model_utils.jl:150-155)
function clock(m::Model)
    t = Ref{Float64}(0); it = Ref{Int64}(0); dt = Ref{Float64}(0)
    check(m, ccall((:gb25_get_clock, m.lib), Cint, (Ptr{Cvoid}, Ref{Float64}, Ref{Int64}, Ref{Float64}),
                   m.ptr, t, it, dt), "gb25_get_clock")
    return (time = t[], iteration = it[], last_Δt = dt[])
end
set_dt!(m::Model, Δt::Real) =
    check(m, ccall((:gb25_set_dt, m.lib), Cint, (Ptr{Cvoid}, Float64), m.ptr, Δt), "gb25_set_dt")

# ---- fields: parent(field) / interior(field) as host Arrays (copies), column-major [i, j, k] like Oceananigans
function field_dims(m::Model, field::Integer, include_halos::Bool)
    d = zeros(Int32, 3)
    check(m, ccall((:gb25_field_dims, m.lib), Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{Int32}),
                   m.ptr, field, include_halos, d), "gb25_field_dims")
    return (Int(d[1]), Int(d[2]), Int(d[3]))
end
function _get(m::Model{FT}, field::Integer, include_halos::Bool) where {FT}
    a = Array{FT}(undef, field_dims(m, field, include_halos)...)
    check(m, ccall((:gb25_get_field, m.lib), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Cint),
                   m.ptr, field, a, include_halos), "gb25_get_field")
    return a
end
function _set!(m::Model{FT}, field::Integer, a::AbstractArray, include_halos::Bool) where {FT}
    dims = field_dims(m, field, include_halos)
    b = Array{FT}(reshape(a, dims))       # contiguous, converted to the library's element type
    check(m, ccall((:gb25_set_field, m.lib), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Cint),
                   m.ptr, field, b, include_halos), "gb25_set_field")
    return nothing
end
parent_array(m::Model, field::Integer) = _get(m, field, true)
interior_array(m::Model, field::Integer) = _get(m, field, false)
set_parent!(m::Model, field::Integer, a::AbstractArray) = _set!(m, field, a, true)
set_interior!(m::Model, field::Integer, a::AbstractArray) = _set!(m, field, a, false)

"""
    device_pointer(m, field) -> Ptr{FT}

Device address of `parent(field)` (exactly the Oceananigans parent layout) for zero-copy wrapping, e.g. with AMDGPU.jl
`unsafe_wrap(ROCArray, device_pointer(m, f), field_dims(m, f, true))`.  Handing out the pointer of u, v, T, S or of a
tendency pins those fields to the buffers handed out and turns the AB2 look-ahead off for this model (gb25.h).
"""
function device_pointer(m::Model{FT}, field::Integer) where {FT}
    p = Ref{Ptr{Cvoid}}(C_NULL)
    check(m, ccall((:gb25_field_device_ptr, m.lib), Cint, (Ptr{Cvoid}, Cint, Ref{Ptr{Cvoid}}), m.ptr, field, p),
          "gb25_field_device_ptr")
    return Ptr{FT}(p[])
end

# ---- x-slab decomposition: one Julia process per GPU (Config(rank=..., nranks=...)), halo exchange inside the library
"128 bytes of ncclGetUniqueId; rank 0 calls this and MPI.Bcast's the buffer."
function comm_unique_id(::Type{FT} = Float32) where {FT}
    id = zeros(UInt8, 128)
    st = ccall((:gb25_comm_unique_id, LIBS[FT]), Cint, (Ptr{UInt8},), id)
    st == 0 || throw(GB25Error("gb25_comm_unique_id: status $st (librccl could not be loaded?)"))
    return id
end
comm_init_rccl!(m::Model, id::Vector{UInt8}) =
    check(m, ccall((:gb25_comm_init_rccl, m.lib), Cint, (Ptr{Cvoid}, Ptr{UInt8}), m.ptr, id), "gb25_comm_init_rccl")

# ---- diagnostics on the device (gb25_get_field_stats / gb25_compare_field / gb25_get_state_monitor): mirrors of the three
#      result structs of include/gb25.h, checked against the library's gb25_*_bytes before the first use
struct FieldStats
    min::Float64; max::Float64; max_abs::Float64; sum::Float64; sum_sq::Float64
    count::Int64; nonfinite::Int64
    at_max_abs::NTuple{3, Int32}; first_nonfinite::NTuple{3, Int32}; global_offset::NTuple{3, Int32}
    reserved::Int32
end
struct FieldDiff
    max_abs_a::Float64; max_abs_b::Float64; max_abs_delta::Float64; sum_sq_a::Float64; sum_sq_b::Float64; sum_sq_delta::Float64
    count::Int64; nonfinite::Int64
    at_max_abs_delta::NTuple{3, Int32}; global_offset::NTuple{3, Int32}
end
struct StateMonitor
    u::FieldStats; v::FieldStats; w::FieldStats; eta::FieldStats; T::FieldStats; S::FieldStats
    cfl::Float64
    at_cfl::NTuple{3, Int32}; reserved::Int32
    nonfinite_total::Int64; iteration::Int64
    time::Float64
end
function check_diagnostic_structs(m::Model)
    sizes = (ccall((:gb25_field_stats_bytes, m.lib), Int32, ()), ccall((:gb25_field_diff_bytes, m.lib), Int32, ()),
             ccall((:gb25_state_monitor_bytes, m.lib), Int32, ()))
    sizes == (sizeof(FieldStats), sizeof(FieldDiff), sizeof(StateMonitor)) ||
        error("gb25_field_stats / gb25_field_diff / gb25_state_monitor are $sizes bytes in the library and " *
              "$((sizeof(FieldStats), sizeof(FieldDiff), sizeof(StateMonitor))) in GB25HIP.jl: different versions")
end
"min, max, max|x| and where (1-based, in the box), sums and non-finite count of a field, reduced on the device; read-only for the schedule."
function field_stats(m::Model, field::Integer, include_halos::Bool = false)
    check_diagnostic_structs(m)
    out = Ref{FieldStats}()
    check(m, ccall((:gb25_get_field_stats, m.lib), Cint, (Ptr{Cvoid}, Cint, Cint, Ref{FieldStats}), m.ptr, field, include_halos, out),
          "gb25_get_field_stats")
    return out[]
end
"parent(field) on the device for reading (and the array's extents there): nothing is pinned, valid until the next call on m."
function device_pointer_readonly(m::Model{FT}, field::Integer) where {FT}
    p, d = Ref{Ptr{Cvoid}}(C_NULL), zeros(Int32, 3)
    check(m, ccall((:gb25_field_device_ptr_readonly, m.lib), Cint, (Ptr{Cvoid}, Cint, Ref{Ptr{Cvoid}}, Ptr{Int32}), m.ptr, field, p, d),
          "gb25_field_device_ptr_readonly")
    return Ptr{FT}(p[]), Tuple(d)
end
"compare_parent / compare_interior (src/correctness.jl:4-26) against a device array of `eltype` (Float32 | Float64), `dims`, from the 0-based `origin`."
function compare_field(m::Model, field::Integer, include_halos::Bool, other::Ptr, eltype::Type, dims, origin = (0, 0, 0))
    check_diagnostic_structs(m)
    out = Ref{FieldDiff}()
    check(m, ccall((:gb25_compare_field, m.lib), Cint,
                   (Ptr{Cvoid}, Cint, Cint, Ptr{Cvoid}, Int32, Ptr{Int32}, Ptr{Int32}, Ref{FieldDiff}),
                   m.ptr, field, include_halos, other, sizeof(eltype), Int32[dims...], Int32[origin...], out), "gb25_compare_field")
    return out[]
end
"the interior statistics of u, v, w, eta, T, S, the advective CFL rate [1/s] and the clock: the numbers of the progress callback."
function state_monitor(m::Model)
    check_diagnostic_structs(m)
    out = Ref{StateMonitor}()
    check(m, ccall((:gb25_get_state_monitor, m.lib), Cint, (Ptr{Cvoid}, Ref{StateMonitor}), m.ptr, out), "gb25_get_state_monitor")
    return out[]
end

# ---- integrals on the device (gb25_integrate_field / gb25_get_budget): sums weighted by the cell measure of include/gb25.h
const SUM_ROWS, SUM_LEVELS, SUM_TOTAL = Cint(0), Cint(1), Cint(2)
struct Moments
    measure::Float64; first::Float64; second::Float64
    points::Int64; nonfinite::Int64
end
struct Budget
    T::Moments; S::Moments; u::Moments; v::Moments; eta::Moments
    volume::Float64; surface_area::Float64
    kinetic_energy::Float64
    eta_potential_energy::Float64
    iteration::Int64
    time::Float64
    global_offset::NTuple{3, Int32}; reserved::Int32
end
function check_integral_structs(m::Model)
    sizes = (ccall((:gb25_moments_bytes, m.lib), Int32, ()), ccall((:gb25_budget_bytes, m.lib), Int32, ()))
    sizes == (sizeof(Moments), sizeof(Budget)) ||
        error("gb25_moments / gb25_budget are $sizes bytes in the library and $((sizeof(Moments), sizeof(Budget))) in GB25HIP.jl: different versions")
end
"sum mu, sum mu x, sum mu x^2 of a field over its wet interior: SUM_ROWS a (by, bz) matrix of row records (zonal sums), SUM_LEVELS bz records, SUM_TOTAL one."
function integrate_field(m::Model, field::Integer, shape::Integer = SUM_TOTAL)
    check_integral_structs(m)
    d = zeros(Int32, 3)
    check(m, ccall((:gb25_field_dims, m.lib), Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{Int32}), m.ptr, field, 0, d), "gb25_field_dims")
    n = shape == SUM_ROWS ? Int(d[2]) * Int(d[3]) : shape == SUM_LEVELS ? Int(d[3]) : 1
    out = Vector{Moments}(undef, n)
    check(m, ccall((:gb25_integrate_field, m.lib), Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{Moments}, Int64), m.ptr, field, shape, out, n),
          "gb25_integrate_field")
    return shape == SUM_ROWS ? reshape(out, Int(d[2]), Int(d[3])) : shape == SUM_LEVELS ? out : out[1]
end
"the totals of T, S, u, v, eta, the volume, the surface area, the kinetic and the free surface's potential energy; read-only for the schedule."
function budget(m::Model)
    check_integral_structs(m)
    out = Ref{Budget}()
    check(m, ccall((:gb25_get_budget, m.lib), Cint, (Ptr{Cvoid}, Ref{Budget}), m.ptr, out), "gb25_get_budget")
    return out[]
end

# ---- derived fields on the device (gb25_compute_derived / gb25_get_derived / gb25_get_derived_stats / gb25_get_field_levels):
#      definitions in include/gb25.h.  k_first is 0-based like the ABI; k_count = -1: all levels from k_first on.
const DERIVED = (vorticity = Cint(0), kinetic_energy = Cint(1), density_anomaly = Cint(2), potential_density = Cint(3),
                 mixed_layer_depth = Cint(4))
"interior extents of a derived field (zeta: those of v)"
function derived_dims(m::Model, d::Integer)
    out = zeros(Int32, 3)
    check(m, ccall((:gb25_derived_dims, m.lib), Cint, (Ptr{Cvoid}, Cint, Ptr{Int32}), m.ptr, d, out), "gb25_derived_dims")
    return Tuple(Int.(out))
end
"device pointer and dims of the packed result (read-only, valid until the next call on m): what unsafe_wrap(ROCArray, ...) consumes"
function compute_derived(m::Model{FT}, d::Integer; param::Real = 0.0, k_first::Integer = 0, k_count::Integer = -1) where {FT}
    p, dims = Ref{Ptr{Cvoid}}(C_NULL), zeros(Int32, 3)
    check(m, ccall((:gb25_compute_derived, m.lib), Cint, (Ptr{Cvoid}, Cint, Float64, Int32, Int32, Ref{Ptr{Cvoid}}, Ptr{Int32}),
                   m.ptr, d, param, k_first, k_count, p, dims), "gb25_compute_derived")
    return Ptr{FT}(p[]), Tuple(Int.(dims))
end
"a derived field's requested levels as an Array{FT, 3}; only those levels are computed and copied"
function get_derived(m::Model{FT}, d::Integer; param::Real = 0.0, k_first::Integer = 0, k_count::Integer = -1) where {FT}
    nx, ny, nz = derived_dims(m, d)
    out = Array{FT}(undef, nx, ny, k_count == -1 ? nz - k_first : k_count)
    check(m, ccall((:gb25_get_derived, m.lib), Cint, (Ptr{Cvoid}, Cint, Float64, Int32, Int32, Ptr{Cvoid}),
                   m.ptr, d, param, k_first, k_count, out), "gb25_get_derived")
    return out
end
function derived_stats(m::Model, d::Integer; param::Real = 0.0)
    check_diagnostic_structs(m)
    out = Ref{FieldStats}()
    check(m, ccall((:gb25_get_derived_stats, m.lib), Cint, (Ptr{Cvoid}, Cint, Float64, Ref{FieldStats}), m.ptr, d, param, out),
          "gb25_get_derived_stats")
    return out[]
end
# ---- stability diagnostics on the device (gb25_stability_dims / gb25_compute_stability / gb25_get_stability /
#      gb25_get_stability_stats): definitions in include/gb25.h.  k_first counts FACES, 0-based like the ABI; k_count = -1: all from
#      k_first on.  param: the floor of the Richardson number (on S2, > 0) or of the Eady rate (on N2, >= 0).
const STABILITY = (n2 = Cint(0), shear2 = Cint(1), richardson = Cint(2), eady_rate = Cint(3), ertel_pv = Cint(4),
                   wave_speed = Cint(5))
"extents of a stability diagnostic: (Nx, Ny, Nz + 1), the wave speed (Nx, Ny, 1)"
function stability_dims(m::Model, q::Integer)
    out = zeros(Int32, 3)
    check(m, ccall((:gb25_stability_dims, m.lib), Cint, (Ptr{Cvoid}, Cint, Ptr{Int32}), m.ptr, q, out), "gb25_stability_dims")
    return Tuple(Int.(out))
end
"(device pointer, dims) of the packed result; read-only, valid until the next call on m"
function compute_stability(m::Model{FT}, q::Integer; param::Real = (q == STABILITY.richardson ? 1e-12 : 0.0), k_first::Integer = 0,
                           k_count::Integer = -1) where {FT}
    p, dims = Ref{Ptr{Cvoid}}(C_NULL), zeros(Int32, 3)
    check(m, ccall((:gb25_compute_stability, m.lib), Cint, (Ptr{Cvoid}, Cint, Float64, Int32, Int32, Ref{Ptr{Cvoid}}, Ptr{Int32}),
                   m.ptr, q, param, k_first, k_count, p, dims), "gb25_compute_stability")
    return Ptr{FT}(p[]), Tuple(Int.(dims))
end
"a stability diagnostic's requested faces as an Array{FT, 3}; only those faces are computed and copied"
function get_stability(m::Model{FT}, q::Integer; param::Real = (q == STABILITY.richardson ? 1e-12 : 0.0), k_first::Integer = 0,
                       k_count::Integer = -1) where {FT}
    nx, ny, nf = stability_dims(m, q)
    out = Array{FT}(undef, nx, ny, k_count == -1 ? nf - k_first : k_count)
    check(m, ccall((:gb25_get_stability, m.lib), Cint, (Ptr{Cvoid}, Cint, Float64, Int32, Int32, Ptr{Cvoid}),
                   m.ptr, q, param, k_first, k_count, out), "gb25_get_stability")
    return out
end
function stability_stats(m::Model, q::Integer; param::Real = (q == STABILITY.richardson ? 1e-12 : 0.0))
    check_diagnostic_structs(m)
    out = Ref{FieldStats}()
    check(m, ccall((:gb25_get_stability_stats, m.lib), Cint, (Ptr{Cvoid}, Cint, Float64, Ref{FieldStats}), m.ptr, q, param, out),
          "gb25_get_stability_stats")
    return out[]
end
# ---- flow kinematics on the device (gb25_kinematics_dims / gb25_compute_kinematics / gb25_get_kinematics /
#      gb25_get_kinematics_stats): definitions in include/gb25.h.  k_first counts levels, 0-based like the ABI; k_count = -1: all from
#      k_first on.  param: the tracer of the gradient and of the frontogenesis function (KIN_TRACER), 0 for the others.
const KINEMATICS = (divergence = Cint(0), normal_strain = Cint(1), shear_strain = Cint(2), okubo_weiss = Cint(3),
                    rossby_number = Cint(4), gradient = Cint(5), frontogenesis = Cint(6))
const KIN_TRACER = (T = Int32(0), S = Int32(1), potential_density = Int32(2))
"extents of a kinematics quantity: (Nx, Ny, Nz) at the cells; the shear strain and the Rossby number have the rows of v"
function kinematics_dims(m::Model, q::Integer)
    out = zeros(Int32, 3)
    check(m, ccall((:gb25_kinematics_dims, m.lib), Cint, (Ptr{Cvoid}, Cint, Ptr{Int32}), m.ptr, q, out), "gb25_kinematics_dims")
    return Tuple(Int.(out))
end
"(device pointer, dims) of the packed result; read-only, valid until the next diagnostics call on m"
function compute_kinematics(m::Model{FT}, q::Integer; param::Integer = 0, k_first::Integer = 0, k_count::Integer = -1) where {FT}
    p, dims = Ref{Ptr{Cvoid}}(C_NULL), zeros(Int32, 3)
    check(m, ccall((:gb25_compute_kinematics, m.lib), Cint, (Ptr{Cvoid}, Cint, Int32, Int32, Int32, Ref{Ptr{Cvoid}}, Ptr{Int32}),
                   m.ptr, q, param, k_first, k_count, p, dims), "gb25_compute_kinematics")
    return Ptr{FT}(p[]), Tuple(Int.(dims))
end
"a kinematics quantity's requested levels as an Array{FT, 3}; only those levels are computed and copied"
function get_kinematics(m::Model{FT}, q::Integer; param::Integer = 0, k_first::Integer = 0, k_count::Integer = -1) where {FT}
    nx, ny, nz = kinematics_dims(m, q)
    out = Array{FT}(undef, nx, ny, k_count == -1 ? nz - k_first : k_count)
    check(m, ccall((:gb25_get_kinematics, m.lib), Cint, (Ptr{Cvoid}, Cint, Int32, Int32, Int32, Ptr{Cvoid}),
                   m.ptr, q, param, k_first, k_count, out), "gb25_get_kinematics")
    return out
end
function kinematics_stats(m::Model, q::Integer; param::Integer = 0)
    check_diagnostic_structs(m)
    out = Ref{FieldStats}()
    check(m, ccall((:gb25_get_kinematics_stats, m.lib), Cint, (Ptr{Cvoid}, Cint, Int32, Ref{FieldStats}), m.ptr, q, param, out),
          "gb25_get_kinematics_stats")
    return out[]
end
# ---- block sums on the device (gb25_block_dims / gb25_derived_block_dims / gb25_get_block_sums / gb25_compute_block_sums /
#      gb25_get_derived_block_sums): definitions in include/gb25.h.  block = (bx, by, bz); k_first counts the field's own levels,
#      0-based like the ABI; k_count = -1: all from k_first on; level_weight: one Float64 per level of the field, or nothing.
struct Blocks
    bx::Int32; by::Int32; bz::Int32
    k_first::Int32; k_count::Int32
    reserved::Int32
end
struct BlockInfo
    dims::NTuple{3, Int32}; reserved::Int32
    points::Int64; nonfinite::Int64; empty_blocks::Int64
    global_offset::NTuple{3, Int32}; reserved2::Int32
end
Blocks(block; k_first::Integer = 0, k_count::Integer = -1) = Blocks(block[1], block[2], block[3], k_first, k_count, 0)
"dims of the block sums of a field: (Nx / bx, Ny / by, k_count / bz); needs no device"
function block_dims(m::Model, field::Integer, block; k_first::Integer = 0, k_count::Integer = -1)
    out = zeros(Int32, 3)
    check(m, ccall((:gb25_block_dims, m.lib), Cint, (Ptr{Cvoid}, Cint, Ref{Blocks}, Ptr{Int32}), m.ptr, field,
                   Blocks(block; k_first, k_count), out), "gb25_block_dims")
    return Tuple(Int.(out))
end
"(measure, first, second, info) of a field's blocks: three Array{Float64, 3} [I, J, K] and a BlockInfo"
function block_sums(m::Model, field::Integer, block; k_first::Integer = 0, k_count::Integer = -1,
                    level_weight::Union{Nothing, Vector{Float64}} = nothing)
    ccall((:gb25_block_info_bytes, m.lib), Int32, ()) == sizeof(BlockInfo) || error("gb25_block_info: the library and GB25HIP.jl differ")
    dims = block_dims(m, field, block; k_first, k_count)
    measure, first, second = (Array{Float64}(undef, dims...) for _ in 1:3)
    info = Ref{BlockInfo}()
    check(m, ccall((:gb25_get_block_sums, m.lib), Cint,
                   (Ptr{Cvoid}, Cint, Ref{Blocks}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{BlockInfo}), m.ptr, field,
                   Blocks(block; k_first, k_count), level_weight === nothing ? C_NULL : level_weight, measure, first, second, info),
          "gb25_get_block_sums")
    return measure, first, second, info[]
end
"(device pointer, dims, info): the planes measure | first | second one after another; read-only, valid until the next call on m"
function compute_block_sums(m::Model, field::Integer, block; k_first::Integer = 0, k_count::Integer = -1,
                            level_weight::Union{Nothing, Vector{Float64}} = nothing)
    p, dims, info = Ref{Ptr{Float64}}(C_NULL), zeros(Int32, 3), Ref{BlockInfo}()
    check(m, ccall((:gb25_compute_block_sums, m.lib), Cint,
                   (Ptr{Cvoid}, Cint, Ref{Blocks}, Ptr{Float64}, Ref{BlockInfo}, Ref{Ptr{Float64}}, Ptr{Int32}), m.ptr, field,
                   Blocks(block; k_first, k_count), level_weight === nothing ? C_NULL : level_weight, info, p, dims),
          "gb25_compute_block_sums")
    return p[], Tuple(Int.(dims)), info[]
end
"the block sums of a derived field at (c,c): DERIVED.kinetic_energy, density_anomaly, potential_density, mixed_layer_depth"
function derived_block_sums(m::Model, d::Integer, block; param::Real = 0.0, k_first::Integer = 0, k_count::Integer = -1,
                            level_weight::Union{Nothing, Vector{Float64}} = nothing)
    out = zeros(Int32, 3)
    check(m, ccall((:gb25_derived_block_dims, m.lib), Cint, (Ptr{Cvoid}, Cint, Ref{Blocks}, Ptr{Int32}), m.ptr, d,
                   Blocks(block; k_first, k_count), out), "gb25_derived_block_dims")
    measure, first, second = (Array{Float64}(undef, Int.(out)...) for _ in 1:3)
    info = Ref{BlockInfo}()
    check(m, ccall((:gb25_get_derived_block_sums, m.lib), Cint,
                   (Ptr{Cvoid}, Cint, Float64, Ref{Blocks}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{BlockInfo}), m.ptr, d,
                   param, Blocks(block; k_first, k_count), level_weight === nothing ? C_NULL : level_weight, measure, first, second, info),
          "gb25_get_derived_block_sums")
    return measure, first, second, info[]
end
"interior levels of an ordinary field, gathered on the device: field_levels(m, FIELD.T, Nz - 1, 1) is interior(T)[:, :, Nz:Nz]"
function field_levels(m::Model{FT}, field::Integer, k_first::Integer = 0, k_count::Integer = -1) where {FT}
    d = zeros(Int32, 3)
    check(m, ccall((:gb25_field_dims, m.lib), Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{Int32}), m.ptr, field, 0, d), "gb25_field_dims")
    out = Array{FT}(undef, Int(d[1]), Int(d[2]), k_count == -1 ? Int(d[3]) - k_first : k_count)
    check(m, ccall((:gb25_get_field_levels, m.lib), Cint, (Ptr{Cvoid}, Cint, Int32, Int32, Ptr{Cvoid}), m.ptr, field, k_first, k_count, out),
          "gb25_get_field_levels")
    return out
end

# ---- transports on the device (gb25_get_transport): definitions in include/gb25.h.  along_first is 0-based like the ABI;
#      along_count = -1: to the end.
const ACROSS_Y, ACROSS_X = Cint(0), Cint(1)
const TR_LINES, TR_PROFILE, TR_STREAMFUNCTION = Cint(0), Cint(1), Cint(2)
struct Transport
    area::Float64; volume::Float64; heat::Float64; salt::Float64
    faces::Int64; nonfinite::Int64
end
"area, volume, heat and salt transport through the y faces (summed along i) or the x faces (summed along j): TR_LINES an (N, Nz) matrix, TR_PROFILE N records, TR_STREAMFUNCTION (N, Nz + 1) running sums."
function transport(m::Model, faces::Integer, shape::Integer = TR_LINES; along_first::Integer = 0, along_count::Integer = -1)
    ccall((:gb25_transport_bytes, m.lib), Int32, ()) == sizeof(Transport) ||
        error("gb25_transport has another size in the library than in GB25HIP.jl: different versions")
    d = zeros(Int32, 3)
    check(m, ccall((:gb25_field_dims, m.lib), Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{Int32}), m.ptr, faces == ACROSS_Y ? FIELD.v : FIELD.u, 0, d),
          "gb25_field_dims")
    N, Nz = faces == ACROSS_Y ? Int(d[2]) : Int(d[1]), Int(d[3])
    nk = shape == TR_LINES ? Nz : shape == TR_PROFILE ? 1 : Nz + 1
    out = Vector{Transport}(undef, N * nk)
    check(m, ccall((:gb25_get_transport, m.lib), Cint, (Ptr{Cvoid}, Cint, Cint, Int32, Int32, Ptr{Transport}, Int64),
                   m.ptr, faces, shape, along_first, along_count, out, length(out)), "gb25_get_transport")
    return shape == TR_PROFILE ? out : reshape(out, N, nk)
end
"the meridional overturning streamfunction [j, kf] in m^3/s"
overturning(m::Model; kw...) = map(r -> r.volume, transport(m, ACROSS_Y, TR_STREAMFUNCTION; kw...))

# ---- time averages accumulated on the device (gb25_averages_*): definitions in include/gb25.h.  k_first is 0-based like the ABI;
#      k_count = -1: all levels from k_first on.
const AVG_MEANS, AVG_SQUARES, AVG_FLUXES = Int32(1), Int32(2), Int32(4)
const AVERAGE = (u = 0, v = 1, w = 2, T = 3, S = 4, eta = 5, uu = 6, vv = 7, TT = 8, SS = 9, etaeta = 10,
                 uT = 11, uS = 12, vT = 13, vS = 14, wT = 15, wS = 16)
struct AveragesInfo
    groups::Int32; k_first::Int32; k_count::Int32; reserved::Int32
    samples::Int64; first_iteration::Int64; last_iteration::Int64
    weight_sum::Float64; first_time::Float64; last_time::Float64
end
"allocate and zero the accumulators of `groups` (AVG_MEANS must be among them) over the cell levels k_first .. k_first + k_count - 1"
function averages_begin(m::Model, groups::Integer = AVG_MEANS | AVG_SQUARES | AVG_FLUXES; k_first::Integer = 0, k_count::Integer = -1)
    ccall((:gb25_averages_info_bytes, m.lib), Int32, ()) == sizeof(AveragesInfo) ||
        error("gb25_averages_info has another size in the library than in GB25HIP.jl: different versions")
    check(m, ccall((:gb25_averages_begin, m.lib), Cint, (Ptr{Cvoid}, Int32, Int32, Int32), m.ptr, groups, k_first, k_count), "gb25_averages_begin")
end
"acc = acc + weight * term for every quantity of the active groups: one launch, between two composite calls"
averages_accumulate(m::Model, weight::Real = 1.0) =
    check(m, ccall((:gb25_averages_accumulate, m.lib), Cint, (Ptr{Cvoid}, Float64), m.ptr, weight), "gb25_averages_accumulate")
function averages_info(m::Model)
    out = Ref{AveragesInfo}()
    check(m, ccall((:gb25_averages_get_info, m.lib), Cint, (Ptr{Cvoid}, Ptr{AveragesInfo}), m.ptr, out), "gb25_averages_get_info")
    return out[]
end
function average_dims(m::Model, a::Integer)
    d = zeros(Int32, 3)
    check(m, ccall((:gb25_average_dims, m.lib), Cint, (Ptr{Cvoid}, Cint, Ptr{Int32}), m.ptr, a, d), "gb25_average_dims")
    return (Int(d[1]), Int(d[2]), Int(d[3]))
end
"the accumulator of AVERAGE.x over the active window, or (normalized) accumulator / weight_sum: a Float64 array (i, j, k)"
function get_average(m::Model, a::Integer; normalized::Bool = true)
    out = Array{Float64}(undef, average_dims(m, a)...)
    check(m, ccall((:gb25_get_average, m.lib), Cint, (Ptr{Cvoid}, Cint, Int32, Ptr{Float64}, Int64), m.ptr, a, normalized ? 1 : 0, out, length(out)),
          "gb25_get_average")
    return out
end
averages_end(m::Model) = check(m, ccall((:gb25_averages_end, m.lib), Cint, (Ptr{Cvoid},), m.ptr), "gb25_averages_end")

# ---- checkpoint and bit-for-bit restart (include/gb25.h)
checkpoint_snapshot(m::Model; max_arena_bytes::Integer = 0) =
    check(m, ccall((:gb25_checkpoint_snapshot, m.lib), Cint, (Ptr{Cvoid}, Int64), m.ptr, max_arena_bytes), "gb25_checkpoint_snapshot")
checkpoint_write(m::Model, directory::AbstractString, label::AbstractString = "checkpoint") =
    check(m, ccall((:gb25_checkpoint_write, m.lib), Cint, (Ptr{Cvoid}, Cstring, Cstring), m.ptr, directory, label), "gb25_checkpoint_write")
checkpoint_release(m::Model) = check(m, ccall((:gb25_checkpoint_release, m.lib), Cint, (Ptr{Cvoid},), m.ptr), "gb25_checkpoint_release")
function checkpoint(m::Model, directory::AbstractString, label::AbstractString = "checkpoint")
    checkpoint_snapshot(m)
    checkpoint_write(m, directory, label)
end
# gb25_checkpoint_info / gb25_restore_info (include/gb25.h), field for field
struct CheckpointInfo
    taken::Int32; drained::Int32; members::Int32; pieces::Int32
    bytes::Int64; arena_bytes::Int64
    averages_open_not_saved::Int32; particles_open_not_saved::Int32
end
struct RestoreInfo
    members::Int32; pieces::Int32; bytes::Int64; options_changed::UInt32
    tracer_rows_differ::Int32; phy_stale::Int32; reserved::Int32
end
function checkpoint_info(m::Model)
    info = Ref(CheckpointInfo(0, 0, 0, 0, 0, 0, 0, 0))
    check(m, ccall((:gb25_checkpoint_get_info, m.lib), Cint, (Ptr{Cvoid}, Ref{CheckpointInfo}), m.ptr, info), "gb25_checkpoint_get_info")
    info[]
end
function restore!(m::Model, directory::AbstractString, label::AbstractString = "checkpoint")
    info = Ref(RestoreInfo(0, 0, 0, 0, 0, 0, 0))
    check(m, ccall((:gb25_restore, m.lib), Cint, (Ptr{Cvoid}, Cstring, Cstring, Ref{RestoreInfo}), m.ptr, directory, label, info), "gb25_restore")
    info[]
end
set_clock!(m::Model, time::Real, iteration::Integer, last_Δt::Real) =
    check(m, ccall((:gb25_set_clock, m.lib), Cint, (Ptr{Cvoid}, Float64, Int64, Float64), m.ptr, time, iteration, last_Δt), "gb25_set_clock")

# ---- passive tracers carried beside a run (include/gb25.h, "passive tracers carried beside a run"): dyes and ideal age, advanced by
# calls of their own between the model's steps; single domains, closure = nothing
struct TracerSpec      # gb25_tracer_spec, field for field
    source::Float64; surface_value::Float64; surface_reset::Int32; clip_negative::Int32
end
dye(; clip_negative::Bool = false) = TracerSpec(0.0, 0.0, 0, clip_negative ? 1 : 0)
ideal_age() = TracerSpec(1.0, 0.0, 1, 0)
mutable struct TracerSet
    ptr::Ptr{Cvoid}
    count::Int
end
const FIELD_T_ID = 3    # GB25_T: a tracer has the shapes of T
function tracers_begin(m::Model, specs::Vector{TracerSpec})
    sizeof(TracerSpec) == ccall((:gb25_tracer_spec_bytes, m.lib), Int32, ()) || error("gb25_tracer_spec: different versions")
    out = Ref{Ptr{Cvoid}}(C_NULL)
    check(m, ccall((:gb25_tracers_begin, m.lib), Cint, (Ptr{Cvoid}, Int32, Ptr{TracerSpec}, Ptr{Ptr{Cvoid}}), m.ptr, length(specs), specs, out),
          "gb25_tracers_begin")
    return TracerSet(out[], length(specs))
end
"tracer n (0-based) from an array shaped like interior(T) (or parent(T)); the next advance is an Euler step"
function tracers_set!(m::Model{FT}, s::TracerSet, n::Integer, a::AbstractArray; include_halos::Bool = false) where {FT}
    b = Array{FT}(reshape(a, field_dims(m, FIELD_T_ID, include_halos)))
    check(m, ccall((:gb25_tracers_set, m.lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ptr{Cvoid}, Cint), m.ptr, s.ptr, n, b, include_halos),
          "gb25_tracers_set")
end
"which = 0: c, 1: the tendency of the last advance, 2: the one before"
function tracers_get(m::Model{FT}, s::TracerSet, n::Integer; which::Integer = 0, include_halos::Bool = false) where {FT}
    a = Array{FT}(undef, field_dims(m, FIELD_T_ID, include_halos)...)
    check(m, ccall((:gb25_tracers_get, m.lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Int32, Ptr{Cvoid}, Cint), m.ptr, s.ptr, n, which, a,
                   include_halos), "gb25_tracers_get")
    return a
end
tracers_advance!(m::Model, s::TracerSet) =
    check(m, ccall((:gb25_tracers_advance, m.lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), m.ptr, s.ptr), "gb25_tracers_advance")
function tracers_stats(m::Model, s::TracerSet, n::Integer)
    out = Ref{FieldStats}()
    check(m, ccall((:gb25_tracers_stats, m.lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ref{FieldStats}), m.ptr, s.ptr, n, out), "gb25_tracers_stats")
    return out[]
end
function tracers_clock(m::Model, s::TracerSet)
    t = Ref{Float64}(0); it = Ref{Int64}(0)
    check(m, ccall((:gb25_tracers_clock, m.lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Int64}), m.ptr, s.ptr, t, it), "gb25_tracers_clock")
    return (time = t[], iteration = it[])
end
function tracers_end!(m::Model, s::TracerSet)
    check(m, ccall((:gb25_tracers_end, m.lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), m.ptr, s.ptr), "gb25_tracers_end")
    s.ptr = C_NULL
end
"advance, then the model's step, `steps` times; at iteration 0 initialize! and update_state! first make w and the halos of u, v"
function run_with_tracers!(m::Model, s::TracerSet, steps::Integer)
    for _ in 1:steps
        if clock(m).iteration == 0
            initialize!(m); update_state!(m); tracers_advance!(m, s); first_time_step!(m)
        else
            tracers_advance!(m, s); time_step!(m)
        end
    end
end

end # module
