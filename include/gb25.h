/*
 * gb25.h -- C ABI of libgb25hip.so: the MI355X (gfx950) implementation of the
 * Oceananigans HydrostaticFreeSurfaceModel time-step loop that GB-25's
 * baroclinic_instability_model drives.
 *
 * This is the drop-in boundary.  Each entry point names the reference interface it
 * replaces (paths relative to the GB-25 tree).  A Julia host binds these with
 * `ccall`; this repository binds them with ctypes
 * (gb-25_amd/binding.py).  Plain pointers and sizes only; no exceptions cross the ABI:
 * every call returns a gb25_status and the message is kept per handle.
 *
 * Layout contract (src/correctness.jl:4-15 compares `parent(field)` arrays):
 * every field is stored exactly like `parent(field)` of the Oceananigans Field --
 * column-major, i fastest, halo H on every side:
 *     centre/centre/centre (T, S, pHY', u(*), G.u, G.T, G.S): (Nx+2H, Ny+2H,   Nz+2H)
 *     v, G.v  (face in bounded y):                             (Nx+2H, Ny+2H+1, Nz+2H)
 *     w       (face in bounded z):                             (Nx+2H, Ny+2H,   Nz+2H+1)
 *     eta, U, etabar, Ubar, G.U:                               (Nx+2H, Ny+2H,   1)
 *     V, Vbar, G.V:                                            (Nx+2H, Ny+2H+1, 1)
 * (*) x is periodic, so u has Nx faces.  With an x-slab decomposition Nx is the
 * LOCAL slab width (Nx_global / nranks) and the x halos hold the neighbours' columns.
 * Element type: the library is built once per Oceananigans float type -- libgb25hip.so holds Float32
 * (simulations/baroclinic_instability_simulation_run.jl:13, the headline runs) and libgb25hip_f64.so Float64
 * (the default of --float-type, src/arg_parsing.jl:12-16, used by the correctness scripts).  Both export the
 * same symbols; gb25_real_bytes() tells which one is loaded, and every `void *` data pointer below addresses
 * elements of that size.
 */
#ifndef GB25_H
#define GB25_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gb25_model gb25_model; /* opaque; owns all device memory */

typedef enum {
  GB25_OK = 0,
  GB25_ERR_INVALID_ARGUMENT = 1,
  GB25_ERR_HIP = 2,          /* a HIP runtime call failed; see gb25_last_error_string */
  GB25_ERR_OUT_OF_MEMORY = 3,
  GB25_ERR_NO_DEVICE = 4,    /* no gfx950 device visible: there is NO CPU fallback */
  GB25_ERR_STATE = 5,
  GB25_ERR_COMM = 6          /* RCCL could not be loaded / a communicator or exchange call failed */
} gb25_status;

/* Field identifiers: the set compared by compare_states (src/correctness.jl:28-90)
 * plus the diagnostic pressure and the barotropic work fields. */
typedef enum {
  GB25_U = 0, GB25_V, GB25_W, GB25_T, GB25_S, GB25_PHY,
  GB25_GN_U, GB25_GN_V, GB25_GN_T, GB25_GN_S, /* timestepper.G^n */
  GB25_GM_U, GB25_GM_V, GB25_GM_T, GB25_GM_S, /* timestepper.G^- */
  GB25_ETA, GB25_BT_U, GB25_BT_V,             /* free_surface.eta, barotropic_velocities */
  GB25_ETA_BAR, GB25_U_BAR, GB25_V_BAR,       /* free_surface.filtered_state */
  GB25_GN_BT_U, GB25_GN_BT_V,                 /* timestepper.G^n.U, .V */
  /* closure = CATKEVerticalDiffusivity() only (gb25_set_closure_catke): the TKE tracer, its tendencies, and
   * model.diffusivity_fields as src/correctness.jl:60-67 compares them: kappa_u, kappa_c, kappa_e at (Center, Center,
   * Face) [Nz + 1 levels], L^e at cell centres, the surface buoyancy flux J^b (2-D) */
  GB25_E, GB25_GN_E, GB25_GM_E, GB25_KAPPA_U, GB25_KAPPA_C, GB25_KAPPA_E, GB25_LE, GB25_JB,
  /* ... and diffusivity_fields.previous_velocities (u, v at the previous compute_diffusivities!: CATKE's shear production
   * is centred between them and the current ones); not in the compared set, exposed for state transfer and tests.
   * (A single domain keeps them, between calls, in whichever buffer already holds them -- u, v themselves right after
   * compute_diffusivities!, the look-ahead's partner buffers after the AB2 step that followed -- and brings them into
   * these fields when the host reads or writes any field or asks for a device pointer: gb25_api.hip, prev_uv_src.) */
  GB25_PREV_U, GB25_PREV_V,
  GB25_FIELD_COUNT
} gb25_field;

/* Model configuration = the keyword arguments of
 * baroclinic_instability_model(arch, Nx, Ny, Nz; dt, halo, free_surface, ...)
 * (src/baroclinic_instability_model.jl:17-40) and of simple_latitude_longitude_grid
 * (src/model_utils.jl:56-65).  Fill with gb25_default_config, then override. */
typedef struct {
  int32_t Nx, Ny, Nz;   /* GLOBAL interior size */
  int32_t halo;         /* H; 8 in every GB-25 script */
  int32_t substeps;     /* SplitExplicitFreeSurface(substeps=30) */
  int32_t rank, nranks; /* x-slab decomposition: this process owns columns
                           [rank*Nx/nranks, (rank+1)*Nx/nranks); nranks=1: periodic x is local */
  int32_t device;       /* HIP device ordinal */
  double dt;            /* model.clock.last_dt (src/baroclinic_instability_model.jl:82) */
  double chi;           /* QuasiAdamsBashforth2 chi = 0.1 */
  double lat_south, lat_north; /* (-80, 80) */
  double lon_west, lon_east;   /* (0, 360) */
  double depth, zexp_h;        /* exponential_z_faces(Nz, depth=4000, h=30) */
  double g, Omega, radius, rho0; /* 9.80665, 7.292115e-5, 6371e3, 1020 (TEOS-10 reference) */
  int32_t slab_mode;    /* 0: the x halos are a local periodic copy when nranks == 1 and come from the ring neighbours
                              when nranks > 1;  1: always by exchange (nranks == 1: the slab is its own west and east
                              neighbour -- the self-ring that runs the exchange code path on one GPU) */
  int32_t grid_type;    /* gb25_grid_type: grid_type = :simple_lat_lon | :gaussian_islands
                              (src/baroclinic_instability_model.jl:19,59-65) */
  int32_t ranks_y;      /* Partition(Rx, Ry, 1) (sharding/sharded_baroclinic_instability_simulation_run.jl:65-72): Ry, the
                              ranks along y; 0 or 1 = x slabs only.  nranks = Rx Ry, rank = ry Rx + rx; the rank owns the
                              columns [rx Nx/Rx, (rx+1) Nx/Rx) and the rows [ry Ny/Ry, (ry+1) Ny/Ry) */
} gb25_config;

typedef enum {
  GB25_GRID_LAT_LON = 0,                  /* simple_latitude_longitude_grid (src/model_utils.jl:56-65), flat bottom */
  GB25_GRID_LAT_LON_GAUSSIAN_ISLANDS = 1, /* ImmersedBoundaryGrid(that grid, GridFittedBottom(gaussian_islands);
                                             active_cells_map = false): the two mountains of src/model_utils.jl:67-80 */
  GB25_GRID_LAT_LON_AS_CURVILINEAR = 2,   /* grid 0 stepped by the orthogonal-curvilinear kernels (2-D metrics): a test
                                             vehicle, results equal those of grid 0 to round-off */
  GB25_GRID_TRIPOLAR = 3,                 /* TripolarGrid(arch; size, halo, z) (src/model_utils.jl:134-137), flat bottom:
                                             poles at (70 E, 55 N) and (250 E, 55 N), southern edge lat_south, zipper
                                             fold along the northern edge.  The poles are singular without land.
                                             Decomposed in x like the other grids: the cells beyond a slab's fold line
                                             belong to the mirrored rank nranks-1-rank, an extra point-to-point partner */
  GB25_GRID_TRIPOLAR_GAUSSIAN_ISLANDS = 4, /* grid_type = :gaussian_islands of the reference (src/model_utils.jl:129-146):
                                             the tripolar grid with the two Gaussian mountains over its poles */
  GB25_GRID_COUNT
} gb25_grid_type;

/* Per-model switches (gb25_set_option).  Defaults in brackets.  None of them changes results beyond the last bits
 * (KERNELS) or at all (the rest): they select schedules, and tests use them to prove exactly that. */
typedef enum {
  GB25_OPT_KERNELS = 0,          /* [2] 2: LDS-staged / flux-sharing tendency kernels; 1: direct-stencil kernels (cross-check) */
  GB25_OPT_AB2_LOOKAHEAD,        /* [1] the tendency kernels also write the next time level: 0 off, 1 u,v,T,S, 2 T,S only */
  GB25_OPT_SUBCYCLE_LOOKAHEAD,   /* [1 from 8 M cells and on slabs] the next step's split-explicit sub-cycle runs as soon as its
                                    G.U, G.V exist: 1 = between the momentum and the tracer kernel, 2 = beside the tracer
                                    kernel on a stream of its own (slabs: on the exchange stream), 0 = inside its own step */
  GB25_OPT_SUBCYCLE_BLOCK,       /* [5] substeps per barotropic launch: 1, 3, 5, 7 */
  GB25_OPT_FILL_FUSED,           /* [1] y, z and periodic-x halo fills in one launch */
  GB25_OPT_TWO_STREAMS,          /* [1] tracer branch (AB2, halos, pressure) on a second stream */
  GB25_OPT_STORE_PRESSURE,       /* [0] store pHY' every step (1) or only its differences, pHY' on demand (0) */
  GB25_OPT_SPLIT_TENDENCIES,     /* [1] slab: interior tile columns of the momentum tendencies before the halos arrive */
  GB25_OPT_PRESSURE_PRECISION,   /* [64] THE exception to "results unchanged": 64 = equation of state + hydrostatic integral
                                    in fp64 whatever the model's float type (default; fp32 in, fp32 out); 32 = in the float
                                    type's own arithmetic, operation for operation what an all-Float32 model computes
                                    (the stated Float32 tolerance) */
  GB25_OPT_IMMERSED_KERNELS,     /* [1 iff some cell is immersed] 1: run the immersed-boundary kernel variants anyway */
  GB25_OPT_FOLD_FILLS,           /* [1] single domain: the last writers of u,v / T,S / eta,U,V write the halo cells themselves */
  GB25_OPT_LAZY_CORRECTOR,       /* [1] single flat lat-lon domain, between the steps of one gb25_loop call: the barotropic
                                    correction of u, v is added by the kernels that read them instead of by a sweep over
                                    u and v (same bits; memory holds the corrected velocities when the call returns) */
  GB25_OPT_MOMENTUM_CHUNK_LEVELS, /* [24 on models wide enough for four rounds of blocks with it -- 1440 x 720 x 48 -- and small enough that such chunks stay
                                    within the 2 GB the kernel addresses from one base, else 12] levels a
                                    block of the momentum tendency kernel marches through (>= 6); also the association of the
                                    column integrals of u, v: results change in the last bits (a bit-for-bit comparison of a wide
                                    single domain with its narrow ranks pins it on both sides) */
  GB25_OPT_TRACER_CHUNK_LEVELS,  /* [like MOMENTUM_CHUNK_LEVELS] the same for the tracer tendency kernel (bitwise neutral) */
  GB25_OPT_TRACERS_FIRST,        /* [1] single domain, composite steps: the tracer tendency kernel before the momentum kernel, so
                                    that the next step's pressure (it needs the tracer look-ahead's T, S) can run beside the next
                                    step's sub-cycle; 0: momentum first (src/precompile.jl:48-50 lists them in that order; the
                                    two evaluations are independent of each other) */
  GB25_OPT_W_ON_THE_FLY,         /* [1] with LAZY_CORRECTOR, between the steps of one gb25_loop call: the tendency kernels do not read w;
                                    they carry it up their chunks of levels from the divergence of the transports they hold, starting
                                    from 2-D chunk bases made from the column integrals of the velocity look-ahead.  No k_compute_w
                                    launch and no w traffic in those steps; the field w is recomputed from the velocities when the
                                    call returns.  Like KERNELS this changes results in the LAST BITS (another association of the
                                    vertical sum): comparisons that must be bit-exact (a decomposition against the single domain)
                                    switch it off */
  GB25_OPT_SUB_STREAM_PRIORITY,  /* [0] slab of a decomposition: the substeps of the sub-cycle look-ahead run on a HIGH-PRIORITY stream (their
                                    few blocks could be dispatched ahead of what is left of the tracer kernel's grid -- measured: no difference); 0: an ordinary stream.
                                    Read when the exchange context is built (gb25_comm_init_*) */
  GB25_OPT_SUBCYCLE_WHOLE,       /* [1] slab of a decomposition with fewer sub-cycle tiles than the device has CUs (a 180-column rank): all
                                    substeps in ONE launch, the tile and a ring as wide as the sub-cycle is long in 125 KB of LDS;
                                    0: the blocked launches (SUBCYCLE_BLOCK) */
  GB25_OPT_EARLY_STRIPS,         /* [1] x slab of a decomposition: the bundle is unpacked on the exchange stream right behind its transfer
                                    and the pressure strips next to the x halos follow it there, beside the interior momentum pass;
                                    0: unpack and strips on the main stream when it gets there */
  GB25_OPT_CATKE_STALE_E_HALOS,  /* [0] closure = CATKE, single domain: 1 = the halo cells of e are NOT refilled after e is stepped inside
                                    compute_diffusivities! (Oceananigans as recalled: the tendencies that follow see halos one e step old);
                                    0 = refilled.  A RESTATEMENT choice, not a schedule: it changes results */
  GB25_OPT_COMM_TIMEOUT_SECONDS, /* [180] gb25_comm_init_rccl: bound on ncclCommInitRank and on the first exchange with every peer; past it
                                    the call returns GB25_ERR_COMM naming the rank and the buffer set instead of hanging */
  GB25_OPT_ROCTX_RANGES,         /* [1] roctx ranges named like the reference's profiler annotations ("first_time_step", "time_step", "loop":
                                    src/timestepping_utils.jl:22,30,38) around the composites, and one per phase of src/precompile.jl:31-42
                                    around the issue of its kernels (rocprofv3 --marker-trace); free when no marker library is loaded */
  /* Two more RESTATEMENT choices (like CATKE_STALE_E_HALOS they change results; a Julia dump of tools/dump_goldens.jl decides them
   * without new kernel work; the oracle has both on every grid): */
  GB25_OPT_SUBSTEP_ORDER,        /* [0] the two halves of a split-explicit substep: 0 = eta from the old U, V, then U, V from the new eta;
                                    1 = U, V from the old eta, then eta from the new U, V (the order changed between
                                    upstream releases).  1: LatitudeLongitudeGrid only, one substep per launch */
  GB25_OPT_FOLD_PIVOT_SLAVED,    /* [0] TripolarGrid, single domain: 1 = every fold fill also overwrites the eastern half of the pivot row
                                    (cell centres of the last row, held twice) with the image of its western half, as a later upstream
                                    fix does as recalled; 0 = both copies are stepped independently */
  GB25_OPT_PRESSURE_FORM,        /* [0] which of the three launch forms of the fp64 hydrostatic pressure kernel runs (the same bits from
                                    each; tests compare every form cell by cell): 0 = the library's rule (four rows per thread for
                                    wide launches, one row per thread for narrow ones, 16 x 4 tiles for narrow lat-lon launches of
                                    at most 400 columns); 1 = tiles; 2 = one row per thread; 3 = four rows per thread, on any grid
                                    and for every launch.  PRESSURE_PRECISION = 32 ignores it */
  GB25_OPT_SPECTRUM_TABLE,       /* [0] where the kernel of the zonal spectra reads its table of cosines and sines from (the same bits
                                    from each; tests compare both): 0 = the library's rule (LDS where the table and the staged
                                    lines fit 160 KB, else global memory); 1 = global memory */
  GB25_OPT_COUNT
} gb25_option;
/* One more schedule switch is not an option but an environment variable, read once by gb25_create: GB25_TRACER_ROWS = 1 | 2, the
 * rows a lane of the tracer tendency kernel carries (2: the flux through the y face between them is reconstructed once; flat
 * lat-lon grids with WENO(order = 5) only, elsewhere it is ignored).  Unset: 2 for a whole Float32 single domain of at least 4096 blocks
 * of 63 x 8 cells per chunk of levels, 1 otherwise (every slab and every rank of a mesh).  The same bits from both. */

/* Metric identifiers for gb25_get_metric (diagnostics / tests). */
typedef enum {
  GB25_M_PHIF = 0, GB25_M_PHIC, GB25_M_DXC, GB25_M_DXF, GB25_M_AZC, GB25_M_AZF, GB25_M_FCOR,
  GB25_M_ZF, GB25_M_ZC, GB25_M_DZC, GB25_M_DZF,
  GB25_M_DY            /* the LatitudeLongitudeGrid's constant meridional spacing (the index is ignored): what k_advective_cfl divides v by */
} gb25_metric;
/* Horizontal metrics of an orthogonal curvilinear grid by location, for gb25_get_metric2 (Oceananigans' names:
 * GB25_M2_DXFC = dx at (Face, Center), ...; FFF = Coriolis parameter at (f,f); PHICC = latitude of the cell centres). */
typedef enum {
  GB25_M2_DXFC = 0, GB25_M2_DXCC, GB25_M2_DXCF, GB25_M2_DXFF, GB25_M2_DYFC, GB25_M2_DYCC, GB25_M2_DYCF, GB25_M2_DYFF,
  GB25_M2_AZCC, GB25_M2_AZFC, GB25_M2_AZCF, GB25_M2_AZFF, GB25_M2_FFF, GB25_M2_PHICC, GB25_M2_COUNT
} gb25_metric2;

/* Kernel identifiers for the built-in HIP-event timers (gb25_profile_*). */
typedef enum {
  GB25_K_FILL_HALOS = 0, GB25_K_COMPUTE_W, GB25_K_COMPUTE_P, GB25_K_GU, GB25_K_GV, GB25_K_TRACERS,
  GB25_K_AB2_VELOCITIES, GB25_K_AB2_TRACERS, GB25_K_BAROTROPIC, GB25_K_CORRECTOR,
  GB25_K_IMPLICIT,     /* implicit_step!: the vertical solves of a closure (all of a step's launches together)        */
  GB25_K_CLOSURE,      /* CATKE: advection of e, surface flux, diffusivities                                          */
  GB25_K_FLUXES,       /* data-free forcing: similarity-theory fluxes; the bottom drag's flux kernel                   */
  GB25_K_DIAGNOSTICS,  /* gb25_get_field_stats / gb25_compare_field / gb25_get_state_monitor / gb25_integrate_field /   */
                       /* gb25_get_budget / the derived fields: every launch they make, a pressure recomputed for a     */
                       /* stale GB25_PHY included                                                                       */
  GB25_K_COUNT
} gb25_kernel;

void gb25_default_config(gb25_config *cfg, int32_t Nx, int32_t Ny, int32_t Nz);

/* ---- lifecycle: replaces baroclinic_instability_model(arch, Nx, Ny, Nz; dt, ...)
 *      (src/baroclinic_instability_model.jl:17-85): builds the grid metrics, allocates every
 *      field zeroed on the device and stores dt in the clock. */
gb25_status gb25_create(const gb25_config *cfg, gb25_model **out);
void gb25_destroy(gb25_model *m);
const char *gb25_last_error_string(const gb25_model *m); /* valid until the next call on m */
const char *gb25_version(void);
int32_t gb25_real_bytes(void); /* sizeof one field element of THIS library: 4 (Float32) or 8 (Float64) */
/* sizeof(gb25_config) and sizeof(gb25_catke_parameters) as THIS library was built: a binding in another language checks its
 * mirror of the structs against them before the first gb25_create (a field added here must not shift silently there) */
int32_t gb25_config_bytes(void);
int32_t gb25_catke_parameters_bytes(void);

/* Run all kernels of this model on the caller's HIP stream (a hipStream_t passed as void*; NULL is HIP's
 * default stream, which is what torch.cuda.current_stream() is unless the host changed it).  Lets a host
 * framework order our kernels with its own work.  gb25_use_own_stream goes back to the model's private
 * non-blocking stream (the state after gb25_create). */
gb25_status gb25_set_option(gb25_model *m, gb25_option opt, int32_t value);
gb25_status gb25_get_option(const gb25_model *m, gb25_option opt, int32_t *value);
gb25_status gb25_set_stream(gb25_model *m, void *hip_stream);
gb25_status gb25_use_own_stream(gb25_model *m);
gb25_status gb25_synchronize(gb25_model *m);

/* ---- fields: replaces parent(field)/interior(field)/set!(model, ...) and sync_states!
 *      (src/correctness.jl:92-103).  dims = parent dims (include_halos != 0) or interior dims.
 *      Host pointers are borrowed for the duration of the call. */
gb25_status gb25_field_dims(const gb25_model *m, gb25_field f, int include_halos, int32_t dims[3]);
gb25_status gb25_set_field(gb25_model *m, gb25_field f, const void *host, int include_halos);
gb25_status gb25_get_field(gb25_model *m, gb25_field f, void *host, int include_halos);
/* Device pointer of parent(field) for zero-copy wrapping (e.g. unsafe_wrap(ROCArray, ...)).
 * G^n / G^- pointers are exchanged by correct_and_cache (a pointer swap replaces the copy): ask again after a step.
 * u, v, T and S normally alternate between two buffers as well (the tendency kernels write the next time level
 * ahead of ab2_step!); asking for the pointer of a prognostic 3-D field or of a tendency pins them to the buffers
 * handed out and turns that look-ahead off for this model, because writes through the pointer cannot be seen by
 * the library.
 * GB25_PHY is a diagnostic: inside the composite steps only its horizontal differences (what the momentum tendencies
 * use) are stored, and gb25_get_field(GB25_PHY) recomputes the field from T and S on demand; asking for its device
 * pointer makes every later step store it (GB25_OPT_STORE_PRESSURE = 1 does the same from the start). */
gb25_status gb25_field_device_ptr(gb25_model *m, gb25_field f, void **dev);
gb25_status gb25_get_metric(const gb25_model *m, gb25_metric id, int32_t logical_index, double *value);
/* grid_type >= 2: one horizontal metric as fp64, the parent layout of a (Center, Face) 2-D field:
 * (Nx + 2 halo) x (Ny + 2 halo + 1) values, i fastest (the role of grid.Δxᶠᶜᵃ etc. of an OrthogonalSphericalShellGrid). */
gb25_status gb25_get_metric2(const gb25_model *m, gb25_metric2 id, double *values, int64_t count);
gb25_status gb25_get_substepping(const gb25_model *m, int32_t *n_effective, double *dtau_fraction,
                                 double *weights /* >= substeps entries */);

/* ---- the HOST's grid.  In the reference the grid is built by Oceananigans on the Julia side and handed to the model:
 *      TripolarGrid(arch; size, halo, z) wrapped in ImmersedBoundaryGrid(grid, GridFittedBottom(gaussian_islands)) with
 *      z = exponential_z_faces(Nz, depth) (src/model_utils.jl:56-62,129-146).  gb25_create builds stand-ins from cfg.grid_type
 *      (an analytic bipolar cap, not necessarily Oceananigans' coordinate lines); a host that has the real grid passes it:
 *
 *      gb25_set_curvilinear_grid: the 14 horizontal metrics in gb25_metric2 order -- grid.Δxᶠᶜᵃ, Δxᶜᶜᵃ, Δxᶜᶠᵃ, Δxᶠᶠᵃ, Δyᶠᶜᵃ, Δyᶜᶜᵃ,
 *        Δyᶜᶠᵃ, Δyᶠᶠᵃ, Azᶜᶜᵃ, Azᶠᶜᵃ, Azᶜᶠᵃ, Azᶠᶠᵃ, the Coriolis parameter at (f,f) and the latitude of the cell centres φᶜᶜᵃ [degrees]
 *        -- each the PARENT array over the GLOBAL grid as fp64, (nx, ny) = (Nx_global + 2 halo, Ny + 2 halo [+ 1]), i fastest
 *        (ny = Ny + 2 halo is what a (Periodic, RightConnected, Bounded) grid holds; a Bounded y has one more row of y faces).
 *        x halo columns are taken as the host holds them; on a folded grid the rows beyond the pivot row are taken from the
 *        interior by the fold's own rule (cell rows and y-face rows mirror about the centres of the last row of cells, x
 *        faces as i -> Nx - i + 2), whatever the host's halo rows hold.  The model must have been created with a curvilinear
 *        grid_type (2, 3, 4).  A slab of a decomposition takes its columns -- halo, widened and fold-partner columns
 *        included -- from the same global arrays.
 *      gb25_set_vertical_faces: the Nz + 1 faces of grid.z, bottom to top [m]; spacings, the TEOS-10 level tables, the bottom's
 *        level tables and a closure's elimination tables are rebuilt.
 *      gb25_set_bottom_height: GridFittedBottom(bottom_height): Nx_global x Ny doubles at the GLOBAL cell centres, i fastest
 *        [m, negative down]; replaces the bottom of grid_type, masks the fields.
 *      All three are collective on a decomposed model, void every look-ahead and may be called in any order before (or
 *      between) steps.  gb25_get_bottom_info (diagnostic; 0-based local i, j): which = 0 the number of immersed cells of the
 *      column, 1 / 2 the static column depth at its U / V face. */
gb25_status gb25_set_curvilinear_grid(gb25_model *m, const double *const *metrics /* [GB25_M2_COUNT] */, int32_t nx, int32_t ny);
gb25_status gb25_set_vertical_faces(gb25_model *m, const double *z_faces, int32_t n /* Nz + 1 */);
gb25_status gb25_set_bottom_height(gb25_model *m, const double *bottom_height);
gb25_status gb25_get_bottom_info(const gb25_model *m, int32_t which, int32_t i, int32_t j, double *value);

/* ---- flux boundary conditions: what compute_hydrostatic_boundary_tendency_contributions! (src/precompile.jl:25,52-61)
 *      adds to the tendencies.  f = GB25_U | GB25_V | GB25_T | GB25_S; `flux` holds J at the interior points of the field's
 *      horizontal location (gb25_field_dims(f, 0): dims[0] x dims[1] values, i fastest), positive upward; NULL restores
 *      the default no-flux condition.  The top cell's tendency gets -J/dz inside the tendency kernels. */
gb25_status gb25_set_top_flux(gb25_model *m, gb25_field f, const void *flux);
/* the flux as the device holds it (same shape; what the coupled model last computed, or what the host set) */
gb25_status gb25_get_top_flux(gb25_model *m, gb25_field f, void *flux);

/* ---- quadratic bottom drag: what ClimaOcean's ocean_simulation (src/data_free_ocean_climate_model.jl:26) puts at the bottom
 *      of u and v -- also the immersed bottom -- with bottom_drag_coefficient = 0.003: the flux boundary condition
 *      J = -Cd u sqrt(u^2 + Ixy(v)^2) (likewise for v), evaluated before every tendency evaluation and added to the tendency of
 *      the face's first free level.  Cd = 0 (the default; baroclinic_instability_model has none): no drag.  Collective. */
gb25_status gb25_set_bottom_drag(gb25_model *m, double Cd);
/*      tracer_advection of the same ocean_simulation: WENO(order = 7) (baroclinic_instability_model: WENO(order = 5), the
 *      default here).  T, S and CATKE's e; the order-5 path where the eight-point stencil meets a wall or the immersed
 *      boundary.  Collective. */
gb25_status gb25_set_tracer_advection_order(gb25_model *m, int32_t order);
gb25_status gb25_get_tracer_advection_order(const gb25_model *m, int32_t *order);
gb25_status gb25_get_bottom_drag(const gb25_model *m, double *Cd);

/* ---- data-free forcing (src/data_free_ocean_climate_model.jl:12-70): a PrescribedAtmosphere + Radiation +
 *      SimilarityTheoryFluxes(solver_stop_criteria = FixedIterations(5)) coupled to the ocean as ClimaOcean's OceanSeaIceModel
 *      does.  The host evaluates the atmosphere at the ocean's cell centres (the reference: analytic fields on a 360 x 180
 *      grid, interpolated) and hands each field over as DOUBLES in the parent layout of a 2-D (c,c) field, halo cells
 *      included ((Nx_local + 2 halo) x (Ny + 2 halo), i fastest): the fluxes of the first halo column / row are computed
 *      from them, not exchanged.  Once all seven fields are set the model is coupled: gb25_first_time_step computes the
 *      fluxes of the initial state, every step ends with the flux computation (similarity theory per surface cell, fp64)
 *      and the results are the top flux boundary conditions of u, v, T, S.  NULL clears a field (uncoupled).
 *      Collective on a decomposed model. */
typedef enum {
  GB25_ATM_U = 0,      /* zonal wind at 10 m [m/s]                      (zonal_wind, :1)        */
  GB25_ATM_V,          /* meridional wind [m/s]                                                 */
  GB25_ATM_T,          /* air temperature [K]                           (Tatm + 273.15, :3,6)   */
  GB25_ATM_Q,          /* specific humidity [kg/kg]                     (0, :57)                */
  GB25_ATM_P,          /* surface pressure [Pa]                                                 */
  GB25_ATM_SHORTWAVE,  /* downwelling shortwave radiation [W/m2]        (sunlight, :2)          */
  GB25_ATM_LONGWAVE,   /* downwelling longwave radiation [W/m2]                                 */
  GB25_ATM_COUNT
} gb25_atmosphere_field;
gb25_status gb25_set_prescribed_atmosphere(gb25_model *m, gb25_atmosphere_field f, const double *values);
/* compute_atmosphere_ocean_fluxes! + the net fluxes, on demand (the composites call it themselves) */
gb25_status gb25_compute_atmosphere_ocean_fluxes(gb25_model *m);

/* ---- closure: `closure = nothing` (the default, src/baroclinic_instability_model.jl:29) or
 *      VerticalScalarDiffusivity(VerticallyImplicitTimeDiscretization(), κ = kappa, ν = nu) (:31): after the explicit AB2
 *      update of u, v (nu) and T, S (kappa), ab2_step! solves (1 - Δt ∂z K ∂z) φ = φ* per column (implicit_step!, batched
 *      tridiagonal solver).  nu = kappa = 0 restores closure = nothing.  [m²/s] */
gb25_status gb25_set_vertical_diffusivity(gb25_model *m, double nu, double kappa);
/*      closure = Oceananigans.TurbulenceClosures.CATKEVerticalDiffusivity() (src/baroclinic_instability_model.jl:30,
 *      sharding/less_simple_sharding_problem.jl:84-93): tracers become (T, S, e); update_state! computes the diffusivity
 *      fields (and fills their halos, src/precompile.jl:37); ab2_step! mixes u, v, T, S, e implicitly with them.  Every grid
 *      type, single domain and slabs (collective there).  on = 0: back to closure = nothing. */
gb25_status gb25_set_closure_catke(gb25_model *m, int32_t on);
/*      The closure's parameters (psi = u, c, e, D in the arrays): the defaults are those of CATKEVerticalDiffusivity();
 *      ClimaOcean's ocean_simulation (src/data_free_ocean_climate_model.jl:26) uses its default_ocean_closure(), which differs
 *      in C^b.  Collective on a decomposed model. */
typedef struct {
  double Cs, Cb, Csp;              /* mixing length: distance to the surface / to the bottom, shear-plume parameter */
  double CRid, CRi0;               /* stability function: width and centre of the step in Ri */
  double Chi[4], Clo[4], Cun[4];   /* stability function: strongly stable, weakly stable, unstable */
  double Cc[4], Ce[4];             /* convective and entrainment lengths */
  double CWu, CWw;                 /* surface TKE flux: friction velocity and convective velocity terms */
  double minimum_tke, minimum_convective_buoyancy_flux, negative_tke_damping_time_scale;
  double CWeps;                    /* bottom TKE flux J^e = -CWeps e^(3/2), implicit in the bottom cell (CATKEEquation's C^W_epsilon = 1) */
} gb25_catke_parameters;
void gb25_default_catke_parameters(gb25_catke_parameters *p);
gb25_status gb25_set_catke_parameters(gb25_model *m, const gb25_catke_parameters *p);
gb25_status gb25_get_catke_parameters(const gb25_model *m, gb25_catke_parameters *p);
gb25_status gb25_get_vertical_diffusivity(const gb25_model *m, double *nu, double *kappa);

/* ---- initial conditions: set_baroclinic_instability!(model) (src/model_utils.jl:99-127) */
gb25_status gb25_set_baroclinic_instability(gb25_model *m);

/* ---- clock: model.clock fields (src/model_utils.jl:150-155) */
gb25_status gb25_get_clock(const gb25_model *m, double *time, int64_t *iteration, double *last_dt);
gb25_status gb25_set_dt(gb25_model *m, double dt);

/* ---- the phases of one time step, in the reference's order (src/precompile.jl:31-42).
 *      Each replaces the *_workload! wrapper cited. */
gb25_status gb25_initialize(gb25_model *m);              /* Oceananigans.initialize!(model) (correctness/..._run.jl:50-51) */
gb25_status gb25_mask_immersed_fields(gb25_model *m);    /* src/precompile.jl:21,34 mask_immersed_model_fields! (nothing to do on a flat bottom) */
gb25_status gb25_fill_halo_regions(gb25_model *m);       /* src/precompile.jl:35,40,44-46 tupled_fill_halo_regions_workload! */
gb25_status gb25_compute_auxiliaries(gb25_model *m);     /* src/precompile.jl:36,113-115  compute_auxiliaries_workload! */
gb25_status gb25_fill_diffusivity_halos(gb25_model *m);  /* src/precompile.jl:37,117-119  (closure=nothing: no-op) */
gb25_status gb25_compute_momentum_tendencies(gb25_model *m); /* src/precompile.jl:63-73  */
gb25_status gb25_compute_tracer_tendencies(gb25_model *m);   /* src/precompile.jl:75-111 */
gb25_status gb25_compute_boundary_tendencies(gb25_model *m); /* src/precompile.jl:52-61: applied inside the tendency kernels (gb25_set_top_flux) */
gb25_status gb25_compute_tendencies(gb25_model *m);      /* src/precompile.jl:38,48-50 compute_tendencies_workload! */
gb25_status gb25_ab2_step(gb25_model *m, double dt, int euler); /* src/precompile.jl:39,121-123 ab2_step_workload! */
gb25_status gb25_correct_velocities_and_cache_previous_tendencies(gb25_model *m, double dt); /* src/precompile.jl:41,125-127 */
gb25_status gb25_update_state(gb25_model *m);            /* Oceananigans.TimeSteppers.update_state! (correctness/..._run.jl:53-54) */
/* (the phase entry points are for single-domain models; on a slab of a decomposition only the composites are valid) */

/* ---- composites: GordonBell25.first_time_step!/time_step!/loop! (src/timestepping_utils.jl:21-45).
 *      dt is read from the clock, the model is mutated in place, nothing is returned. */
gb25_status gb25_first_time_step(gb25_model *m);
gb25_status gb25_time_step(gb25_model *m);
gb25_status gb25_loop(gb25_model *m, int32_t n_inner);

/* ---- x-slab decomposition.  Replaces Oceananigans.Distributed(arch; partition=Partition(Rx,
 *      Ry, 1)) + XLA's collective-permutes (sharding/sharded_baroclinic_instability_simulation_run.jl:65-72): each rank
 *      creates ONE slab (cfg.rank, cfg.nranks; Nx is the global size) and gives it an exchange context; after that
 *      gb25_first_time_step / gb25_time_step / gb25_loop are valid on the slab and `loop!(model, Ninner)` stays ONE
 *      call, as in the reference (:147,162).  Inside a step: packed halo columns travel by ncclSend/ncclRecv (RCCL over
 *      xGMI) on a second HIP stream, overlapped with the own-column work and the interior momentum tendencies; the 21
 *      barotropic substeps need no exchange (wide halos, filled once).  No collective, no host synchronisation.
 *
 *      Setters of a decomposed model (gb25_set_field, gb25_set_dt, gb25_set_option, gb25_set_baroclinic_instability,
 *      gb25_field_device_ptr) are COLLECTIVE: every rank makes the same call in the same order, like set!(model, ...)
 *      on a Distributed grid.  With the RCCL transport they shake hands with both neighbours and return
 *      GB25_ERR_STATE on a mismatch.
 *
 *      2-D decomposition (cfg.ranks_y = Ry > 1; Partition(Rx, Ry, 1), config 4 of the reference: 4 x 2): rank = ry Rx + rx
 *      owns a window of columns AND rows; Nx, Ny stay the global sizes, every field is the window (a y-face field has one
 *      row more only on the ranks below a wall).  Every exchange in x is followed by one of whole rows with the southern /
 *      northern neighbour (rank -/+ Rx; none beyond the walls and the fold); the fold partner of a top-row rank is the
 *      mirrored rank of that row.  Same calls, same transports. */
#define GB25_UNIQUE_ID_BYTES 128
/* rank 0 calls this and hands the 128 bytes to every rank by whatever means the host has (MPI_Bcast, a torch.distributed
 * store, a file): ncclGetUniqueId */
gb25_status gb25_comm_unique_id(void *id_out);
/* every rank, with the same id: ncclCommInitRank(nranks = cfg.nranks, rank = cfg.rank) on cfg.device.  nranks == 1 with
 * slab_mode == 1 is the self-ring.  With GB25_REHEARSE_ALONE=1 in the environment a rank of ANY decomposition gets a communicator
 * of size one and is its own neighbour on every side (a timing proxy of one rank with a GPU to itself -- tools/slab_selfring.py
 * --mesh; what crosses the seams is not a simulation's data). */
gb25_status gb25_comm_init_rccl(gb25_model *m, const void *unique_id);
/* all `n` slabs of one decomposition live in THIS process on one device (tests of decomposition invariance; also a
 * single-process multi-slab run): slabs[r] must have cfg.rank == r, cfg.nranks == n (and the same ranks_y).  The composites called on ANY of
 * them step all of them in lock-step; the exchange is a ring of device-to-device copies. */
gb25_status gb25_comm_init_local(gb25_model *const *slabs, int32_t n);
/* the host moves the buffers: fn is called once per exchange with device pointers of this slab's two packed sends and
 * two receive buffers (nbytes each); it must return 0 after recv_west holds the west neighbour's send_east and
 * recv_east the east neighbour's send_west.  The library synchronises the issuing stream before the call (no overlap):
 * a rehearsal transport for setups where RCCL cannot run (two ranks on one device).  buffer_set 3 and 4 (tripolar grid
 * only) are exchanges with the FOLD PARTNER, rank nranks-1-rank (2-D decomposition: the mirrored rank of the same row):
 * send_west goes to it, recv_west must hold what it sent, the east pointers are NULL.  buffer_set 5, 6, 7 (2-D decomposition
 * only) are the y halos: the "west" pointers belong to the SOUTHERN neighbour (rank - Rx), the "east" pointers to the
 * NORTHERN one (rank + Rx); a side without a neighbour has NULL pointers.  buffer_set 8, 9, 10 (closure = CATKE only: the TKE
 * tracer and J^b after their step inside compute_diffusivities!) go to the ring neighbours, to the southern / northern neighbours
 * and to the fold partner respectively, with the pointer conventions above.  (Which exchange group uses which buffer set: the
 * table of groups in DESIGN.md, kGroups in csrc/slab_protocol.hpp.) */
typedef int32_t (*gb25_exchange_fn)(void *user, int32_t buffer_set, const void *send_west, const void *send_east,
                                    void *recv_west, void *recv_east, int64_t nbytes);
gb25_status gb25_comm_init_callback(gb25_model *m, gb25_exchange_fn fn, void *user);
gb25_status gb25_comm_finalize(gb25_model *m);
/* transport: 0 none, 1 RCCL, 2 local ring, 3 host callback; comm_ranks: the communicator's size as RCCL reports it
 * (ncclCommCount; 0 without RCCL).  Either pointer may be NULL. */
gb25_status gb25_comm_info(const gb25_model *m, int32_t *transport, int32_t *comm_ranks);
/* (tests) the sends / receives one rank of an Rx x Ry decomposition posts for an exchange group, in posting order, as text;
 * returns the bytes needed incl. the terminator, or -1 for a rank outside the decomposition or a `group` that is not in the table
 * of groups (0 - 4, 6, 8, 10 - 14, 20 - 22).  No GPU is touched. */
int64_t gb25_debug_exchange_plan(int32_t Rx, int32_t Ry, int32_t rank, int32_t folded_grid, int32_t group, char *out, int64_t cap);
/* velocities_ready: the momentum look-ahead of the next step exists (its sub-cycle can run beside the tracer kernel);
 * subcycle_adopted: the last step adopted the sub-cycle look-ahead instead of sub-cycling inside the step. */
gb25_status gb25_lookahead_state(const gb25_model *m, int32_t *velocities_ready, int32_t *subcycle_adopted);
/* The order of operations of one time step (bit 0 of `first`: of first_time_step!; bit 1: on a folded grid; bit 2: of a
 * coupled model; bit 3: with the previous step's look-ahead chain still in flight) of `nslabs` slabs as text, without
 * touching a GPU; bit 4: of a 2-D decomposition; bit 5: of a step that keeps the corrector inside its consumers; bit 6: with the
 * bundle unpacked on the exchange stream (tests of the sequencing on CPU-only machines).  Returns the bytes needed, incl. the terminator. */
int64_t gb25_debug_sequence(int32_t nslabs, int32_t first, int32_t adopted, int32_t ready, char *out, int64_t cap);

/* ---- state dump: save_model_state(dir, model, arch; label) (src/sharded_io.jl:70-96,122-138; called after each loop
 *      of the benchmark script, sharding/sharded_..._run.jl:151-155,167-171).  Every rank writes only its own slab --
 *      no communication -- to <directory>/<label>/fields_rank<rank>.npz (uncompressed NumPy .npz): per field of
 *      Oceananigans.fields(model) the local interior (<name>.data), its slice of the global array (<name>.slice: i0, i1,
 *      j0, j1, k0, k1) and the global shape, plus iteration, time, rank, nranks.  Offline gather (load_all_fields,
 *      src/sharded_io.jl:198-213): gb-25_amd/sharded_io.py. */
gb25_status gb25_save_state(gb25_model *m, const char *directory, const char *label);

/* ---- diagnostics on the device: reductions over the fields where they live (csrc/diagnostics_kernels.hpp).  What
 *      src/correctness.jl:4-26 (compare_parent / compare_interior) computes per field and what the progress callback of
 *      simulations/ocean_climate_simulation.jl:95-116 prints (max|u|, max|v|, max|w|, extrema(T), ...), without a field crossing
 *      PCIe.  All of them
 *        - see the state gb25_get_field would return at that moment and are ordered after the model's streams;
 *        - are READ-ONLY for the schedule: no buffer is pinned, every look-ahead stays valid, every later field is bit for bit
 *          what it would have been (unlike gb25_field_device_ptr);
 *        - are LOCAL on a rank of a decomposition (not collective): the rank's own interior or parent.  global_offset places it:
 *          reported position + global_offset = 1-based index into the global INTERIOR (combine ranks on the host:
 *          gb-25_amd/distributed.py combine_stats / combine_diffs);
 *        - are bitwise repeatable.
 *      Positions are 1-based (i, j, k) relative to the box (the interior, or the parent with include_halos != 0); among equal
 *      values the one with the smallest linear offset in memory order (i fastest) is reported, like Julia's findmax.
 *      min, max, max_abs, sum, sum_sq range over the FINITE values (none: min = +Inf, max = -Inf, max_abs = 0, position 0 0 0);
 *      first_nonfinite is 0 0 0 when nonfinite == 0.  count = elements of the box. */
typedef struct {
  double min, max, max_abs, sum, sum_sq;
  int64_t count, nonfinite;
  int32_t at_max_abs[3], first_nonfinite[3], global_offset[3];
  int32_t reserved;
} gb25_field_stats;
/* a: the model's field, b: the other array, delta = a - b formed in fp64.  max_abs_a / sum_sq_a over the finite a, likewise b;
 * max_abs_delta / sum_sq_delta over the positions where a, b and delta are finite; nonfinite counts the other positions. */
typedef struct {
  double max_abs_a, max_abs_b, max_abs_delta, sum_sq_a, sum_sq_b, sum_sq_delta;
  int64_t count, nonfinite;
  int32_t at_max_abs_delta[3], global_offset[3];
} gb25_field_diff;
/* the interior statistics of u, v, w, eta, T, S; the advective CFL rate [1/s] max(|u|/dx + |v|/dy + |w|/dz) over the interior
 * cells (multiply by dt for the Courant number; metrics: csrc/diagnostics_kernels.hpp) and its position; the clock */
typedef struct {
  gb25_field_stats u, v, w, eta, T, S;
  double cfl;
  int32_t at_cfl[3], reserved;
  int64_t nonfinite_total, iteration;
  double time;
} gb25_state_monitor;
int32_t gb25_field_stats_bytes(void);   /* sizeof the three structs as THIS library was built (like gb25_config_bytes) */
int32_t gb25_field_diff_bytes(void);
int32_t gb25_state_monitor_bytes(void);
gb25_status gb25_get_field_stats(gb25_model *m, gb25_field f, int include_halos, gb25_field_stats *out);
/* other_dev: a device pointer of this process to elements of other_real_bytes (4: float, 8: double -- whatever this library's
 * float type is), an array of other_dims (i fastest) at least as large as the box of f; other_origin: its 0-based element that
 * pairs with the first element of the box (NULL: 0 0 0) -- compare_parent's view(psi2, 1:Nx, 1:Ny, 1:Nz).  The caller orders
 * the producer of other_dev before the call (gb25_field_device_ptr_readonly does, for a field of another model). */
gb25_status gb25_compare_field(gb25_model *m, gb25_field f, int include_halos, const void *other_dev, int32_t other_real_bytes,
                               const int32_t other_dims[3], const int32_t other_origin[3], gb25_field_diff *out);
gb25_status gb25_get_state_monitor(gb25_model *m, gb25_state_monitor *out);
/* parent(field) on the device for READING, brought up to date like gb25_get_field and complete when the call returns; nothing
 * is pinned and no look-ahead is given up.  device_dims: the extents of the array as the device holds it (its pitches; a y-face
 * field of a folded grid has one row more there than gb25_field_dims reports).  Valid until the next call on m. */
gb25_status gb25_field_device_ptr_readonly(gb25_model *m, gb25_field f, const void **dev, int32_t device_dims[3]);

/* ---- integrals on the device: volume-weighted sums of a field over the rank's interior (csrc/diagnostics_kernels.hpp,
 *      k_field_moments / k_moments_fold).  How much heat, salt, volume and kinetic energy the ocean holds.  Same contract as the
 *      diagnostics above: the state gb25_get_field would return, READ-ONLY for the schedule, LOCAL on a rank (combine on the
 *      host: gb-25_amd/integrals.py combine_moments / combine_budgets), bitwise repeatable, launches under GB25_K_DIAGNOSTICS.
 *
 *      THE MEASURE of interior point (i, j, k) of a field at location LOC:
 *          mu = A_loc(i, j) * dz_loc(k) * fold(j) * wet_loc(i, j, k)
 *      formed in fp64, in that order, from the numbers gb25_get_metric / gb25_get_metric2 return ((double)(real) of the host
 *      tables, like the metrics of k_advective_cfl):
 *        location  fields                                        A                                  dz       wet
 *        (c,c,c)   T, S, e, pHY, G^n / G^- of T, S, e, L^e       AZCC  (lat-lon: GB25_M_AZC(j))     DZC(k)   k >= kbot(i,j)
 *        (f,c,c)   u, G^n / G^- u, previous u                    AZFC  (lat-lon: GB25_M_AZC(j))     DZC(k)   k >= max(kbot(i-1,j), kbot(i,j))
 *        (c,f,c)   v, G^n / G^- v, previous v                    AZCF  (lat-lon: GB25_M_AZF(j))     DZC(k)   k >= max(kbot(i,j-1), kbot(i,j)); 0 on a GLOBAL wall row
 *        (c,c,f)   w, kappa_u, kappa_c, kappa_e                  as (c,c,c)                         DZF(k)   cell k or cell k-1 is wet
 *        2-D (c,c) eta, eta_bar, J^b                             as (c,c,c)                         1        the column has a wet cell
 *        2-D (f,c) U, U_bar, G^n U                               as (f,c,c)                         1        the face column has a wet level
 *        2-D (c,f) V, V_bar, G^n V                               as (c,f,c)                         1        the face column has a wet level
 *      "lat-lon" means the LatitudeLongitudeGrid with its row tables (grid types 0 and 1).  Every grid that carries 2-D metrics takes
 *      the 2-D areas AZCC / AZFC / AZCF, GB25_GRID_LAT_LON_AS_CURVILINEAR included (its 2-D areas are the row values).
 *      kbot = the number of immersed cells of a column (gb25_get_bottom_info, which = 0); the neighbour across x is the periodic
 *      or the neighbour rank's column.  fold(j) = 1/2 on the GLOBAL pivot row (the last row of cell centres) of a folded grid
 *      for the locations whose rows are rows of cell centres ((c,c,.) and (f,c,.)), 1 elsewhere: the pivot row is held twice,
 *      each physical cell is counted once, and both copies get the 1/2 whether or not GB25_OPT_FOLD_PIVOT_SLAVED is set.  Rows
 *      of y faces are held once.  On a rank of a decomposition the box is the rank's own interior; wall rows and the pivot row
 *      are the global ones.
 *
 *      gb25_moments: measure = sum mu, first = sum mu x, second = sum mu x^2 over the points with mu > 0 and x finite; points =
 *      how many those are; nonfinite = the points with mu > 0 whose x is not finite (skipped).  A value in an immersed cell is
 *      invisible.
 *      REDUCTION ORDER: one wave per row (j, k) of the interior box; a lane takes every 64th chunk of four elements and
 *      accumulates in fp64 in the order of its elements; lanes combine by the fixed shuffle tree: that is ROWS[j + by k].
 *      LEVELS[k] = ((ROWS[0, k] + ROWS[1, k]) + ...) left to right in j, TOTAL = ((LEVELS[0] + LEVELS[1]) + ...) left to right
 *      in k, in fp64, member by member: a host that has ROWS can check LEVELS and TOTAL bit for bit.
 *      count: by * bz records for ROWS (j fastest; by, bz = gb25_field_dims(f, 0)[1..2]), bz for LEVELS, 1 for TOTAL; any
 *      other count is GB25_ERR_INVALID_ARGUMENT. */
typedef enum { GB25_SUM_ROWS = 0, GB25_SUM_LEVELS = 1, GB25_SUM_TOTAL = 2 } gb25_sum_shape;
typedef struct {
  double measure, first, second;
  int64_t points, nonfinite;
} gb25_moments;
gb25_status gb25_integrate_field(gb25_model *m, gb25_field f, gb25_sum_shape shape, gb25_moments *out, int64_t count);
/* the totals of T, S, u, v, eta (each field read once) and what follows from them; global_offset as in gb25_field_stats */
typedef struct {
  gb25_moments T, S, u, v, eta;
  double volume, surface_area;       /* measure of T [m^3], measure of eta [m^2] */
  double kinetic_energy;             /* 1/2 (second of u + second of v)  [m^5 s^-2] */
  double eta_potential_energy;       /* 1/2 g second of eta              [m^5 s^-2] */
  int64_t iteration;
  double time;
  int32_t global_offset[3], reserved;
} gb25_budget;
gb25_status gb25_get_budget(gb25_model *m, gb25_budget *out);
int32_t gb25_moments_bytes(void);       /* sizeof the two structs as THIS library was built */
int32_t gb25_budget_bytes(void);

/* ---- derived fields on the device: what the flow looks like, without a parent array crossing PCIe (csrc/diagnostics_kernels.hpp,
 *      k_derived_*, k_gather_levels).  Relative vorticity, kinetic energy per cell, in-situ and potential density, mixed-layer
 *      depth, and a few levels of any ordinary field (the surface slices `indices = (:, :, Nz)` the reference's
 *      simulations/ocean_climate_simulation.jl writes every three days).  Same contract as the diagnostics above: the state
 *      gb25_get_field would return, READ-ONLY for the schedule (nothing pinned, every look-ahead alive), LOCAL on a rank (a
 *      rank's interior; gather by global_offset: gb-25_amd/derived.py gather_derived), bitwise repeatable, launches under
 *      GB25_K_DIAGNOSTICS.
 *
 *      DEFINITIONS.  Values are read from the parent arrays as gb25_get_field(f, host, 1) returns them at that moment, halo cells
 *      included; metrics are the numbers gb25_get_metric / gb25_get_metric2 return.  Vorticity, kinetic energy and mixed-layer
 *      depth: every operation in fp64 on (double) of the stored values, in the written order, IEEE divisions, NO fused
 *      multiply-adds, the result rounded once to the float type -- gb-25_amd/derived.py restates them with numpy bit for bit.
 *      Indices below are 1-based interior; i-1, j-1, i+1, j+1 reach one halo column or row.
 *        GB25_D_VORTICITY  zeta(i,j,k) = ((dy v(i,j,k) - dy' v(i-1,j,k)) - (dx u(i,j,k) - dx' u(i,j-1,k))) / Az
 *            curvilinear grids (grid_type >= 2): dy = DYCF(i,j), dy' = DYCF(i-1,j), dx = DXFC(i,j), dx' = DXFC(i,j-1), Az = AZFF(i,j)
 *            LatitudeLongitudeGrid:               dy = dy' = GB25_M_DY, dx = DXC(j), dx' = DXC(j-1), Az = AZF(j)
 *            Az == 0 gives 0.  No masking of its own: masked velocities make zeta vanish inside land.
 *        GB25_D_KINETIC_ENERGY  KE(i,j,k) = 0.25 * ((u(i)^2 + u(i+1)^2) + (v(j)^2 + v(j+1)^2)): Oceananigans' (Ix u^2 + Iy v^2) / 2
 *        GB25_D_DENSITY_ANOMALY  the TEOS-10 polynomial folded at the level's depth, on s = sqrt((S + 32) 0.875 / 35.16504),
 *            t = T / 40 formed and evaluated in fp64 exactly as the hydrostatic pressure kernel does (FMAs as the compiler
 *            contracts them there), rounded once; 0 in the immersed cells, k < kbot
 *        GB25_D_POTENTIAL_DENSITY  the same with the one table folded at Z = 0
 *        GB25_D_MIXED_LAYER_DEPTH  sigma = the potential density as stored (rounded to the float type, then (double)); ks = the top
 *            level; d(k) = sigma(k) - sigma(ks).  Marching down from ks - 1, at the first wet k with d(k) >= param the depth is
 *              -(zc(k+1) + (zc(k) - zc(k+1)) * ((param - d(k+1)) / (d(k) - d(k+1))))
 *            with zc = GB25_M_ZC; if d never reaches param, -GB25_M_ZF of the first wet level (the column's bottom face); a dry
 *            column gives 0.  param: the density threshold in kg/m^3, > 0.
 *
 *      LEVELS: k_first, k_count select interior levels, 0-based; k_count = -1: all from k_first on.  A 2-D result takes 0, 1 or
 *      0, -1.  Only the requested levels are computed and copied.  param is ignored except by the mixed-layer depth.
 *      gb25_compute_derived: into an array the model owns (made by the first call, sized for the largest interior, freed by
 *      gb25_destroy); *dev: elements of the library's float type, PACKED, device_dims = interior extents by k_count, i fastest;
 *      read-only, complete when the call returns, valid until the next call on m (what gb25_compare_field of another model or a
 *      host framework's wrapper consumes).  gb25_get_derived: the same and one device-to-host copy of exactly those elements.
 *      gb25_get_derived_stats: gb25_field_stats of the whole derived field, positions relative to its interior.
 *      gb25_get_field_levels: interior levels of an ordinary field, gathered on the device and copied once -- a stale GB25_PHY is
 *      recomputed, previous_velocities are read where they live, the parent is not downloaded, nothing is pinned. */
typedef enum {
  GB25_D_VORTICITY = 0,      /* zeta_3 at (f,f,c); dims = dims of GB25_V */
  GB25_D_KINETIC_ENERGY,     /* (c,c,c) */
  GB25_D_DENSITY_ANOMALY,    /* (c,c,c) rho(T,S,z_k) - rho0, in situ: what the pressure kernel integrates */
  GB25_D_POTENTIAL_DENSITY,  /* (c,c,c) rho(T,S,0) - rho0, referenced to the surface */
  GB25_D_MIXED_LAYER_DEPTH,  /* 2-D (c,c), metres, positive; param = the density threshold in kg/m^3 */
  GB25_D_COUNT
} gb25_derived;
gb25_status gb25_derived_dims(const gb25_model *m, gb25_derived d, int32_t dims[3]);            /* interior; needs no device */
gb25_status gb25_compute_derived(gb25_model *m, gb25_derived d, double param, int32_t k_first, int32_t k_count,
                                 const void **dev, int32_t device_dims[3]);
gb25_status gb25_get_derived(gb25_model *m, gb25_derived d, double param, int32_t k_first, int32_t k_count, void *host);
gb25_status gb25_get_derived_stats(gb25_model *m, gb25_derived d, double param, gb25_field_stats *out);
gb25_status gb25_get_field_levels(gb25_model *m, gb25_field f, int32_t k_first, int32_t k_count, void *host);

/* ---- transports on the device: how much water, heat and salt crosses a line (csrc/diagnostics_kernels.hpp, k_transport_rows /
 *      k_transport_columns / k_transport_fold).  The meridional overturning streamfunction, the meridional heat and salt transport,
 *      the transport through a section.  Same contract as the diagnostics above: the state gb25_get_field would return, halo cells
 *      included, READ-ONLY for the schedule (nothing pinned, every look-ahead alive), LOCAL on a rank (combine on the host:
 *      gb-25_amd/transports.py combine_transports), bitwise repeatable, launches under GB25_K_DIAGNOSTICS on the model's stream.
 *
 *      THE TERMS of a face, formed in fp64 from (double) of the stored values and of the numbers gb25_get_metric / gb25_get_metric2
 *      return, in the written order, NO fused multiply-adds (gb-25_amd/transports.py restates them with numpy bit for bit):
 *        GB25_ACROSS_Y  the faces of v, (c,f,c); interior row j and level k as in gb25_field_dims(GB25_V, 0)
 *            a  = (dx * DZC(k)) * wet     dx = DXCF(i,j) on the grids with 2-D metrics, GB25_M_DXF(j) on the LatitudeLongitudeGrid;
 *                                         wet = the (c,f,c) wetness of the integrals' measure: k >= max(kbot(i,j-1), kbot(i,j)), 0 on
 *                                         a GLOBAL wall row
 *            q  = a * v(i,j,k)
 *            qT = q * (0.5 * (T(i,j-1,k) + T(i,j,k)))        qS = q * (0.5 * (S(i,j-1,k) + S(i,j,k)))
 *        GB25_ACROSS_X  the faces of u, (f,c,c); dims of GB25_U
 *            a  = ((dy * DZC(k)) * fold(j)) * wet            dy = DYFC(i,j), GB25_M_DY on the LatitudeLongitudeGrid; wet = the (f,c,c)
 *                                         wetness: k >= max(kbot(i-1,j), kbot(i,j)); fold(j) = 1/2 on the GLOBAL pivot row of a folded
 *                                         grid as in the (f,c,c) measure, 1 elsewhere (rows of y faces are held once: no factor there)
 *            q  = a * u(i,j,k),  qT and qS with the tracers averaged over i-1, i
 *      A face with a > 0 contributes area += a, volume += q, heat += qT, salt += qS, faces++.  If one of its five values (the
 *      velocity, two T, two S) is not finite the face is skipped whole and counted in nonfinite.  A dry face contributes nothing and a
 *      wet face has two wet cells: a value in an immersed cell is invisible.  Units: m^2, m^3/s, degC m^3/s, (g/kg) m^3/s.
 *
 *      WINDOW: along_first, along_count select the index that is summed -- i for GB25_ACROSS_Y (a basin, a strait), j for
 *      GB25_ACROSS_X (a section between two latitudes) --, 0-based local interior indices; along_count = -1: to the end.  An empty or
 *      out-of-range window is GB25_ERR_INVALID_ARGUMENT.
 *
 *      SHAPES AND REDUCTION ORDER.  N lines: N = by of GB25_V for GB25_ACROSS_Y (one per row j), N = bx of GB25_U for GB25_ACROSS_X
 *      (one per column i); Nz levels.
 *        GB25_TR_LINES           [n + N k].  ACROSS_Y: one wave per row (j, k); a lane takes every 64th chunk of four faces of the
 *                                window and accumulates in the order of its faces; lanes combine by the fixed shuffle tree (the order
 *                                of gb25_integrate_field's ROWS).  ACROSS_X: one thread per (i, k) walks j south to north and adds in
 *                                that order: the record is the SEQUENTIAL sum of the terms, bit for bit.
 *        GB25_TR_PROFILE         [n] = ((LINES[n, 0] + LINES[n, 1]) + ...) left to right in k, member by member, starting from 0.
 *        GB25_TR_STREAMFUNCTION  [n + N kf], kf = 0 .. Nz: the running sums at the z faces, psi[n, 0] = 0, psi[n, kf + 1] = psi[n, kf] +
 *                                LINES[n, kf] in every member, so that psi[n, Nz] == PROFILE[n] bit for bit.  For GB25_ACROSS_Y
 *                                `volume` is the meridional overturning streamfunction in m^3/s.
 *      count: N * Nz records for LINES, N for PROFILE, N * (Nz + 1) for STREAMFUNCTION; any other count is
 *      GB25_ERR_INVALID_ARGUMENT.  The records live in a buffer the model owns (made by the first call, freed by gb25_destroy); a call
 *      makes one device-to-host copy of exactly the records asked for. */
typedef enum { GB25_ACROSS_Y = 0, GB25_ACROSS_X = 1 } gb25_transport_faces;
typedef enum { GB25_TR_LINES = 0, GB25_TR_PROFILE = 1, GB25_TR_STREAMFUNCTION = 2 } gb25_transport_shape;
typedef struct {
  double area, volume, heat, salt;
  int64_t faces, nonfinite;
} gb25_transport;
int32_t gb25_transport_bytes(void);     /* sizeof the struct as THIS library was built */
gb25_status gb25_get_transport(gb25_model *m, gb25_transport_faces faces, gb25_transport_shape shape, int32_t along_first,
                               int32_t along_count, gb25_transport *out, int64_t count);

/* ---- sums in classes on the device: the overturning in density (or temperature, or salinity) classes and the water-mass census
 *      (csrc/class_kernels.hpp, k_class_rows / k_class_fold).  The transport through every row of y faces sorted by the class of
 *      the water that crosses -- the residual overturning psi(y, sigma) that a run with eddies is read by --, and how much volume,
 *      heat and salt sits in each class at each latitude, without v, T, S and a density array crossing PCIe.  Same contract as the
 *      diagnostics above: the state gb25_get_field would return, halo cells included, READ-ONLY for the schedule (nothing pinned,
 *      every look-ahead alive), LOCAL on a rank (combine on the host: gb-25_amd/classes.py combine_class_sums), bitwise
 *      repeatable, launches under GB25_K_DIAGNOSTICS on the model's stream.
 *
 *      CLASSES: edges holds n_edges finite, strictly increasing doubles, 1 <= n_edges <= GB25_CLASS_MAX_BINS - 1; B = n_edges + 1
 *      bins, the first and the last open-ended.  The bin of a class value c is the number of edges e with e <= c
 *      (np.searchsorted(edges, c, side="right")).  Anything else is GB25_ERR_INVALID_ARGUMENT.
 *      THE CLASS VALUE of a cell: GB25_CLASS_T, GB25_CLASS_S: (double) of the stored T or S.  GB25_CLASS_POTENTIAL_DENSITY:
 *      (double) of rho(T, S, 0) - rho0 rounded to the library's float type: the bits gb25_get_derived(GB25_D_POTENTIAL_DENSITY)
 *      hands out for a wet cell, evaluated by the same device function (also in the tracer halo row a rank of a mesh reads; no
 *      density array is made).  The class of a y face: 0.5 * (c(i,j-1,k) + c(i,j,k)) in fp64, no fused multiply-add.
 *      THE TERMS, fp64, in the written order, NO fused multiply-adds (gb-25_amd/classes.py restates them with numpy bit for bit):
 *        GB25_CL_FACES_Y  the faces of v; rows and levels of gb25_field_dims(GB25_V, 0); a, q, qT, qS of
 *                         gb25_get_transport(GB25_ACROSS_Y) with their wetness and wall rows:
 *                         measure += a, flow += q, heat += qT, salt += qS
 *        GB25_CL_CELLS    the cells of T; V = the measure mu of gb25_integrate_field for a (c,c,c) field (area, thickness, 1/2 on
 *                         the pivot row, wet mask): measure += V, flow += exactly 0, heat += V * T, salt += V * S
 *      A wet face (cell) contributes to the bin of its class and to count.  If one of its values -- the velocity, the two T, the
 *      two S of a face, T and S of a cell, or the class value -- is not finite it is skipped whole and counted in nonfinite of
 *      BIN 0 of its row.  A dry face (cell) contributes nothing: a value in an immersed cell is invisible.
 *      WINDOW: i_first, i_count select the columns that are summed, 0-based local interior indices; i_count = -1: to the end.  An
 *      empty or out-of-range window is GB25_ERR_INVALID_ARGUMENT.
 *
 *      SHAPES AND THE ORDER OF EVERY SUM.  N rows: by of GB25_V for GB25_CL_FACES_Y, by of GB25_T for GB25_CL_CELLS; Nz levels.
 *      The level partial p(n, k, b) is the SEQUENTIAL sum, starting from +0.0, of the terms of bin b over i ascending in the
 *      window, every member on its own.
 *        GB25_CL_ROWS             [n B + b] = ((0 + p(n, 0, b)) + p(n, 1, b)) + ..., left to right in k.
 *        GB25_CL_ROWS_CUMULATIVE  [n (B + 1) + e], e = 0 .. B: psi[n, 0] = 0, psi[n, e + 1] = psi[n, e] + ROWS[n, e], member by
 *                                 member.  With GB25_CLASS_POTENTIAL_DENSITY and GB25_CL_FACES_Y, `flow` is the overturning
 *                                 streamfunction in density classes in m^3/s, accumulated from the lightest class.
 *        GB25_CL_TOTAL            [b] = the sequential sum of ROWS[n, b] over n ascending, member by member, starting from 0.
 *      count: N B, N (B + 1) or B records; any other count is GB25_ERR_INVALID_ARGUMENT.  The records live in a buffer the model
 *      owns (made by the first call, made anew when a call asks for more bins, freed by gb25_destroy); a call makes one
 *      device-to-host copy of exactly the records asked for. */
#define GB25_CLASS_MAX_BINS 256
typedef enum { GB25_CLASS_T = 0, GB25_CLASS_S = 1, GB25_CLASS_POTENTIAL_DENSITY = 2 } gb25_class_variable;
typedef enum { GB25_CL_FACES_Y = 0, GB25_CL_CELLS = 1 } gb25_class_what;
typedef enum { GB25_CL_ROWS = 0, GB25_CL_ROWS_CUMULATIVE = 1, GB25_CL_TOTAL = 2 } gb25_class_shape;
typedef struct {
  double measure, flow, heat, salt;
  int64_t count, nonfinite;
} gb25_class_sum;
int32_t     gb25_class_sum_bytes(void);   /* sizeof the struct as THIS library was built */
gb25_status gb25_get_class_sums(gb25_model *m, gb25_class_what what, gb25_class_variable variable, const double *edges,
                                int32_t n_edges, gb25_class_shape shape, int32_t i_first, int32_t i_count, gb25_class_sum *out,
                                int64_t count);

/* ---- zonal wavenumber spectra on the device (csrc/spectrum_kernels.hpp, k_zonal_spectrum): which wavenumber grows, what the
 *      kinetic-energy spectrum looks like, which scales carry the eddy heat flux -- a few kilobytes of coefficients instead of a
 *      parent array crossing PCIe for np.fft.  Same contract as the diagnostics above: the state gb25_get_field would return,
 *      READ-ONLY for the schedule (nothing pinned, every look-ahead alive; a stale GB25_PHY is recomputed as gb25_get_field_levels
 *      does), LOCAL on a rank (combine on the host: gb-25_amd/spectra.py combine_spectra), bitwise repeatable, launches under
 *      GB25_K_DIAGNOSTICS on the model's stream.
 *
 *      THE SOURCE.  A line is interior row j and interior level k of the source, local interior columns i = 0 .. nx-1; column i sits
 *      at the global 0-based column g = i + global_offset_x of a grid of N columns.  The coefficients are taken ALONG THE GRID'S
 *      INDEX i: on the curvilinear and folded grids that is the grid line, not a latitude circle.  x(i) = (double) of the value
 *      gb25_get_field would return at that moment (gb25_get_derived for a derived source: (double) of the rounded derived value).
 *      There is no masking of its own: masked cells hold what they hold.
 *      THE TABLE.  c[r] = cos((2 pi r) / N), s[r] = sin((2 pi r) / N), r = 0 .. N-1, with 2 pi = 6.283185307179586, the product and
 *      the quotient rounded to fp64: by the host's libm; the device's copy is made once per model (again after a rebuild of
 *      the grid), the host's is handed out by gb25_get_spectrum_table (count must be N, else GB25_ERR_INVALID_ARGUMENT; needs no
 *      device and writes nothing of the model, not even its error text).  The table the library returns
 *      IS the table of the definition: a restatement takes it from there, as the others take metrics from gb25_get_metric.
 *      THE COEFFICIENTS of wavenumber m, 0 <= m <= N/2, with r(i) = (m g) mod N in exact integer arithmetic:
 *            A(m) = (((+0.0 + x(0) c[r(0)]) + x(1) c[r(1)]) + ...)   SEQUENTIAL over i ascending
 *            B(m) = the same with s
 *      every product and every sum rounded to fp64, NO fused multiply-adds (gb-25_amd/spectra.py restates them with numpy bit
 *      for bit).  X(m) = A(m) - i B(m): the sign of np.fft.rfft, and its value when the rank holds the whole row; re = A, im = -B.
 *      A line with any value that is not finite is skipped whole: every coefficient of it is exactly +0.0 (re and im), and the
 *      line is counted once in *nonfinite_lines (may be NULL).
 *
 *      WINDOWS AND RECORDS.  m_first, m_count: the wavenumbers, m_count = -1: up to N/2.  k_first, k_count: the levels, as in
 *      gb25_get_field_levels; a 2-D source (eta, the mixed-layer depth) takes 0, 1 or 0, -1.  rows = the interior by of the source.
 *      The record of (m, row j, level k) is at ((k - k_first) rows + j) m_count + (m - m_first); count must be their number.  An
 *      empty or out-of-range window, or another count, is GB25_ERR_INVALID_ARGUMENT.  gb25_get_derived_zonal_spectrum computes the
 *      derived field as gb25_compute_derived does and transforms the packed array with the same kernel: the vorticity gives the
 *      enstrophy spectrum, the kinetic energy its own.  The records live in a buffer the model owns (made by the first call, made
 *      anew when a call asks for more records -- refused with GB25_ERR_OUT_OF_MEMORY before the allocation when the device has
 *      less free --, freed by gb25_destroy); a call makes one device-to-host copy of exactly the records asked for, and one of the
 *      count of skipped lines. */
typedef struct { double re, im; } gb25_spectral_coefficient;   /* re = A, im = -B */
int32_t     gb25_spectral_coefficient_bytes(void);   /* sizeof the struct as THIS library was built */
gb25_status gb25_get_spectrum_table(const gb25_model *m, double *cos_out, double *sin_out, int64_t count);
gb25_status gb25_get_zonal_spectrum(gb25_model *m, gb25_field f, int32_t m_first, int32_t m_count, int32_t k_first, int32_t k_count,
                                    gb25_spectral_coefficient *out, int64_t count, int64_t *nonfinite_lines);
gb25_status gb25_get_derived_zonal_spectrum(gb25_model *m, gb25_derived d, double param, int32_t m_first, int32_t m_count,
                                            int32_t k_first, int32_t k_count, gb25_spectral_coefficient *out, int64_t count,
                                            int64_t *nonfinite_lines);

/* ---- fields on surfaces on the device (csrc/surface_kernels.hpp, k_on_surfaces): where a surface lies and what is on it -- the
 *      depth of an isopycnal, an isotherm or an isohaline, temperature, salinity or kinetic energy on it, the thickness of the
 *      layer between two of them (differences of two depths: gb-25_amd/surfaces.py layer_thickness), and a field at fixed depths,
 *      which on the exponential vertical grid are no model levels -- without whole parent arrays crossing PCIe for a loop over
 *      columns.  Same contract as the derived fields: the state gb25_get_field would return, READ-ONLY for the schedule (nothing
 *      pinned, every look-ahead alive), LOCAL on a rank (a rank's interior; gather by global_offset: gb-25_amd/surfaces.py
 *      gather_surfaces), bitwise repeatable, launches under GB25_K_DIAGNOSTICS on the model's stream.
 *
 *      DEFINITIONS.  Per (c,c) column: kb = the first wet level (0 on a grid without a bottom table), ks = Nz - 1, k increases
 *      upward; zc = GB25_M_ZC, zf = GB25_M_ZF as gb25_get_metric returns them.
 *      THE SEARCH VARIABLE q(k), a double:
 *        GB25_SV_T, GB25_SV_S           (double) of the stored value
 *        GB25_SV_POTENTIAL_DENSITY      (double) of the value gb25_get_derived(GB25_D_POTENTIAL_DENSITY) hands out: rounded to the
 *                                       float type first, the same bits
 *        GB25_SV_DEPTH                  -zc(k)
 *      THE CARRIED QUANTITY f(k):
 *        GB25_SC_DEPTH                  none: the result is the depth of the surface in metres, positive
 *        GB25_SC_T, GB25_SC_S           the stored value
 *        GB25_SC_E                      the stored value; GB25_ERR_INVALID_ARGUMENT unless closure = CATKEVerticalDiffusivity()
 *        GB25_SC_KINETIC_ENERGY, GB25_SC_DENSITY_ANOMALY, GB25_SC_POTENTIAL_DENSITY
 *                                       the value gb25_get_derived hands out, rounded to the float type, then (double)
 *      THE TARGETS: values[0 .. n), 1 <= n <= GB25_SURFACE_MAX_VALUES, every one finite, in any order; each is handled
 *      independently of the others.  Anything else is GB25_ERR_INVALID_ARGUMENT.
 *      THE SEARCH for one value c: for k = Nz - 2 down to kb, with qa = q(k+1), qb = q(k), fa = f(k+1), fb = f(k): the pair CROSSES
 *      when qa and qb are finite and (qa <= c && c <= qb) || (qb <= c && c <= qa) (with a NaN both comparisons are false by
 *      themselves; a pair with an infinity is skipped as well).  At the FIRST crossing from the top
 *              frac  = (qa == qb) ? 0 : (c - qa) / (qb - qa)          g = 1 - frac
 *              depth = -(zc(k+1) * g + zc(k) * frac)                  value = fa * g + fb * frac
 *      -- the two-product form is exact at both ends of a pair: a depth slice taken at a level's centre returns that level's value
 *      unchanged.  Every operation in fp64, in the written order, NO fused multiply-adds, an IEEE division, the result rounded
 *      once to the float type (gb-25_amd/surfaces.py restates it with numpy bit for bit).  Status GB25_SURF_FOUND.
 *      NO CROSSING: with down = (q(kb) >= q(ks)),
 *              (c > q(ks)) == down     GB25_SURF_GROUNDED   depth = -zf(kb)   value = f(kb)    (the surface lies below the bottom)
 *              otherwise               GB25_SURF_OUTCROP    depth = -zf(Nz)   value = f(ks)    (it lies above the top)
 *              a dry column (no wet level)   GB25_SURF_DRY      depth = 0         value = 0
 *
 *      RESULTS: PACKED, out[i + Nx (j + Ny n)] in the library's float type -- the depth for GB25_SC_DEPTH, the value for every other
 *      carried quantity --, and a status byte (gb25_surface_status) per element in an array of the same shape.  They live in a
 *      buffer the model owns (made by the first call, made anew when a call asks for more values -- refused with
 *      GB25_ERR_OUT_OF_MEMORY before the allocation when the device has less free --, freed by gb25_destroy).
 *      gb25_compute_on_surfaces: *dev, *dev_status (may be NULL) point into it, device_dims (may be NULL) = Nx, Ny, n; read-only,
 *      complete when the call returns, valid until the next call on m.  gb25_get_on_surfaces: the same and one device-to-host
 *      copy of each array; host_status may be NULL. */
#define GB25_SURFACE_MAX_VALUES 64
typedef enum { GB25_SV_T = 0, GB25_SV_S, GB25_SV_POTENTIAL_DENSITY, GB25_SV_DEPTH, GB25_SV_COUNT } gb25_surface_variable;
typedef enum {
  GB25_SC_DEPTH = 0, GB25_SC_T, GB25_SC_S, GB25_SC_E, GB25_SC_KINETIC_ENERGY, GB25_SC_DENSITY_ANOMALY, GB25_SC_POTENTIAL_DENSITY,
  GB25_SC_COUNT
} gb25_surface_carried;
typedef enum { GB25_SURF_FOUND = 0, GB25_SURF_OUTCROP = 1, GB25_SURF_GROUNDED = 2, GB25_SURF_DRY = 3 } gb25_surface_status;
gb25_status gb25_compute_on_surfaces(gb25_model *m, gb25_surface_variable v, gb25_surface_carried c, const double *values, int32_t n,
                                     const void **dev, const uint8_t **dev_status, int32_t device_dims[3]);
gb25_status gb25_get_on_surfaces(gb25_model *m, gb25_surface_variable v, gb25_surface_carried c, const double *values, int32_t n,
                                 void *host, uint8_t *host_status /* may be NULL */);

/* ---- stability diagnostics on the device (csrc/stability_kernels.hpp, k_stability_faces / k_stability_wave_speed): what the flow
 *      is about to do -- the stratification N^2, the squared vertical shear, the Richardson number, the Eady growth rate
 *      0.31 |f| / sqrt(Ri), the Ertel potential vorticity, and the first baroclinic gravity-wave speed, which gives the deformation
 *      radius and so tells whether the grid resolves the instability -- without T, S, u and v of whole columns crossing PCIe for an
 *      equation of state on the host.  Same contract as the derived fields and the fields on surfaces: the state gb25_get_field
 *      would return, READ-ONLY for the schedule (nothing pinned, every look-ahead alive, a stale GB25_PHY neither needed nor
 *      touched), LOCAL on a rank (a rank's interior; gather by global_offset: gb-25_amd/stability.py gather_stability), bitwise
 *      repeatable, no floating-point atomics, launches under GB25_K_DIAGNOSTICS on the model's stream.
 *
 *      DEFINITIONS.  Values are read from the parent arrays as gb25_get_field(f, host, 1) returns them at that moment, halo cells
 *      included; metrics are the numbers gb25_get_metric / gb25_get_metric2 return.  Every operation in fp64 on (double) of the
 *      stored values, in the written order, IEEE divisions and square roots, NO fused multiply-adds, the result rounded once to
 *      the float type -- gb-25_amd/stability.py restates them with numpy bit for bit.  Indices below are 1-based interior; i-1,
 *      j-1, i+1, j+1 reach one halo column or row.
 *        sigma(i,j,k)  (double) of the value gb25_get_derived(GB25_D_POTENTIAL_DENSITY) hands out in a wet cell: rounded to the float
 *            type first, the same bits; evaluated on the fly by the same device function, in the halo column and row too.
 *        b = -(g / rho0) * sigma, g and rho0 of gb25_config; the quotient g / rho0 is formed once.  This is stratification
 *            referenced to the SURFACE: it is not the locally referenced N^2 that CATKE forms from alpha and beta at the face.
 *        Face k lies between the cells k-1 and k; dz = zc(k) - zc(k-1), zc = GB25_M_ZC.
 *        GB25_ST_N2          N2 = (-(g / rho0) * (sigma(k) - sigma(k-1))) / dz
 *        GB25_ST_SHEAR2      ub(k) = 0.5 * (u(i) + u(i+1)), vb(k) = 0.5 * (v(j) + v(j+1)) -- v(j+1) as stored, be it a wall's, the
 *            fold's or a halo row --; du = (ub(k) - ub(k-1)) / dz, dv = (vb(k) - vb(k-1)) / dz; S2 = du * du + dv * dv
 *        GB25_ST_RICHARDSON  Ri = N2 / (S2 > param ? S2 : param).  param: a floor on S2 in s^-2, > 0 (the Python layer's default
 *            1e-12 is a convention, not a measured number)
 *        GB25_ST_EADY_RATE   N2 > param ? ((0.31 * |fc|) * sqrt(S2)) / sqrt(N2) : 0.  param: a floor on N2 in s^-2, >= 0.
 *            fc = 0.25 * ((f(i,j) + f(i+1,j)) + (f(i,j+1) + f(i+1,j+1))), f = GB25_M2_FFF; on the LatitudeLongitudeGrid the same
 *            expression with f(.,j) = GB25_M_FCOR(j)
 *        GB25_ST_ERTEL_PV    q = (fc + zb) * N2 + (du * by - dv * bx)
 *            zb = 0.125 * (Z(k-1) + Z(k)), Z(l) = (z(i,j,l) + z(i+1,j,l)) + (z(i,j+1,l) + z(i+1,j+1,l)), z = (double) of
 *                GB25_D_VORTICITY as rounded to the float type (its expression, evaluated at the four corners of the cell)
 *            bx = 0.25 * ((gx(i,k-1) + gx(i+1,k-1)) + (gx(i,k) + gx(i+1,k))), gx(i,l) = (b(i,j,l) - b(i-1,j,l)) / dx(i),
 *                dx = DXFC(i,j) on the grids with 2-D metrics, GB25_M_DXC(j) on the LatitudeLongitudeGrid; gx = 0 when either
 *                cell is immersed (l < kbot of it)
 *            by = 0.25 * ((gy(j,k-1) + gy(j+1,k-1)) + (gy(j,k) + gy(j+1,k))), gy(j,l) = (b(i,j,l) - b(i,j-1,l)) / dy(j),
 *                dy = DYCF(i,j), GB25_M_DY on the LatitudeLongitudeGrid; gy = 0 when either cell is immersed and across the
 *                southern and the northern edge of the GLOBAL grid -- a wall, or the fold, beyond which no bottom is tabulated
 *        GB25_ST_WAVE_SPEED  c1 = (sum over the wet interior faces k, bottom to top, of sqrt(N2(k) > 0 ? N2(k) : 0) * dz(k))
 *            / 3.141592653589793 -- the WKB speed of the first baroclinic mode; the one division comes last.  2-D, (c,c).
 *      A value that is not finite yields what this arithmetic yields; there is no masking beyond the following.
 *
 *      LOCATIONS, FACES AND MASKING.  The first five live at (Center, Center, Face): Nx x Ny x (Nz + 1).  k_first, k_count select
 *      faces, 0-based; k_count = -1: all from k_first on; only the requested faces are computed and copied.  The wave speed
 *      takes 0, 1 or 0, -1.  Faces 0 and Nz are 0.  In a column whose first wet cell is kb (= kbot), every face k <= kb is 0; a dry
 *      column is 0 throughout, its wave speed too.
 *      gb25_compute_stability: into an array the model owns (made by the first call, Nx x Ny x (Nz + 1) values, freed by
 *      gb25_destroy); *dev: elements of the library's float type, PACKED, device_dims = Nx, Ny, the faces of the window, i fastest;
 *      read-only, complete when the call returns, valid until the next call on m.  gb25_get_stability: the same and one
 *      device-to-host copy of exactly those elements.  gb25_get_stability_stats: gb25_field_stats of the whole diagnostic,
 *      positions relative to its box. */
typedef enum { GB25_ST_N2 = 0, GB25_ST_SHEAR2, GB25_ST_RICHARDSON, GB25_ST_EADY_RATE,
               GB25_ST_ERTEL_PV, GB25_ST_WAVE_SPEED, GB25_ST_COUNT } gb25_stability;
gb25_status gb25_stability_dims(const gb25_model *m, gb25_stability q, int32_t dims[3]);   /* needs no device */
gb25_status gb25_compute_stability(gb25_model *m, gb25_stability q, double param, int32_t k_first, int32_t k_count,
                                   const void **dev, int32_t device_dims[3]);
gb25_status gb25_get_stability(gb25_model *m, gb25_stability q, double param, int32_t k_first, int32_t k_count, void *host);
gb25_status gb25_get_stability_stats(gb25_model *m, gb25_stability q, double param, gb25_field_stats *out);

/* ---- flow kinematics on the device (csrc/kinematics_kernels.hpp, k_kinematics_centre / k_kinematics_corner): the horizontal
 *      velocity gradient beyond zeta -- the divergence, the normal and the shear strain rate, the Okubo-Weiss parameter that
 *      separates vortex cores (W < 0) from the strain-dominated filaments between them (W > 0), the local Rossby number zeta / f --
 *      and the horizontal gradient of T, S or the potential density with the frontogenesis function, which says whether the flow
 *      is sharpening that gradient -- without the parents of u, v, T and S crossing PCIe.  Same contract as the derived fields and
 *      the stability diagnostics: the state gb25_get_field would return, READ-ONLY for the schedule (nothing pinned, every
 *      look-ahead alive), LOCAL on a rank (a rank's interior, from the x and y halos a completed step leaves, as the vorticity;
 *      gather by global_offset: gb-25_amd/kinematics.py gather_kinematics), bitwise repeatable, no atomics, ONE launch per request
 *      under GB25_K_DIAGNOSTICS on the model's stream.  Every grid type, both float types, any closure.
 *
 *      DEFINITIONS.  Values are read from the parent arrays as gb25_get_field(f, host, 1) returns them at that moment, halo cells
 *      included; metrics are the numbers gb25_get_metric / gb25_get_metric2 return.  Every operation in fp64 on (double) of the
 *      stored values, in the written order with the written parentheses, IEEE divisions and square roots, NO fused multiply-adds,
 *      the result rounded once to the float type -- gb-25_amd/kinematics.py restates them with numpy bit for bit.  Indices are
 *      those of the interior; i-1, j-1, i+1, j+1 reach one halo column or row.  k is the level, the same on both sides.
 *        Metrics, grids with 2-D metrics | LatitudeLongitudeGrid:
 *            DYFC(i,j) | GB25_M_DY      DXCF(i,j) | GB25_M_DXF(j)      AZCC(i,j) | GB25_M_AZC(j)      (the cell's faces, its area)
 *            DYCF(i,j) | GB25_M_DY      DXFC(i,j) | GB25_M_DXC(j)      AZFF(i,j) | GB25_M_AZF(j)      (the corner: those of zeta)
 *            f(i,j) = GB25_M2_FFF(i,j) | GB25_M_FCOR(j), j the row of y faces
 *        at a cell (c,c,c):
 *            ax = DYFC(i+1,j) * u(i+1,j) - DYFC(i,j) * u(i,j)          ay = DXCF(i,j+1) * v(i,j+1) - DXCF(i,j) * v(i,j)
 *            GB25_KIN_DIVERGENCE     delta = (ax + ay) / AZCC(i,j)
 *            GB25_KIN_NORMAL_STRAIN  s_n   = (ax - ay) / AZCC(i,j)
 *        at a corner (f,f,c), the metrics, operands and order of GB25_D_VORTICITY:
 *            dv = DYCF(i,j) * v(i,j) - DYCF(i-1,j) * v(i-1,j)          du = DXFC(i,j) * u(i,j) - DXFC(i,j-1) * u(i,j-1)
 *            GB25_KIN_SHEAR_STRAIN   s_s  = (dv + du) / AZFF(i,j)          (zeta = (dv - du) / AZFF(i,j): the bits of GB25_D_VORTICITY
 *                                                                            before its rounding)
 *            GB25_KIN_ROSSBY_NUMBER  Ro   = zeta / f(i,j)
 *        the mean over the four corners of a cell, of the fp64 corner values before any rounding:
 *            <a> = 0.25 * ((a(i,j) + a(i+1,j)) + (a(i,j+1) + a(i+1,j+1)))
 *            GB25_KIN_OKUBO_WEISS    W = (s_n * s_n + <s_s * s_s>) - <zeta * zeta>        (every square formed before its mean)
 *        the gradient of x at a cell; x by param: 0 = T, 1 = S, 2 = sigma, (double) of the value
 *        gb25_get_derived(GB25_D_POTENTIAL_DENSITY) hands out in a wet cell (rounded to the float type first, the same bits; formed
 *        in the kernel by the same device function, in the halo column and row too, never stored):
 *            dx(i) = (x(i,j) - x(i-1,j)) / DXFC(i,j)        dy(j) = (x(i,j) - x(i,j-1)) / DYCF(i,j)
 *            gx = 0.5 * (dx(i) + dx(i+1))                     gy = 0.5 * (dy(j) + dy(j+1))
 *            GB25_KIN_GRADIENT       sqrt(gx * gx + gy * gy)
 *            GB25_KIN_FRONTOGENESIS  F = -(((gx * gx) * (0.5 * (delta + s_n)) + (gx * gy) * <s_s>) + (gy * gy) * (0.5 * (delta - s_n)))
 *                -- the rate of change of |grad x|^2 / 2 by the horizontal flow: F > 0 sharpens the front
 *      A value that is not finite yields what this arithmetic yields: nothing is clamped or counted; there is no masking beyond
 *      the following.
 *
 *      ZEROS.  Where AZCC is 0: delta, s_n, W and F are 0.  Where AZFF is 0: s_s, zeta and Ro of that corner are 0 (the rule of
 *      GB25_D_VORTICITY), in the means too.  Where f is 0: Ro is 0.  A difference dx(i) or dy(j) across a face with an immersed side
 *      (k < kbot of either cell, kbot of gb25_get_bottom_info) is 0 -- no gradient through land --, and so is dy across the southern
 *      and the northern edge of the GLOBAL grid: a wall, or the fold, beyond which no bottom is tabulated.  The zero is SELECTED:
 *      what the immersed cell holds does not enter.  The five quantities at cells are 0 in an immersed cell (k < kbot(i,j)).  The
 *      two at corners are not masked, as the vorticity is not; in <.> a corner on a wall row enters with what memory holds.
 *
 *      LOCATIONS AND LEVELS.  Divergence, normal strain, W, gradient and F live at (Center, Center, Center): Nx x Ny x Nz.  The
 *      shear strain and Ro live at (Face, Face, Center) and have the dims of GB25_D_VORTICITY (the rows of v).  k_first, k_count
 *      select levels as in gb25_get_derived (k_count = -1: all from k_first on); only the requested levels are computed, written
 *      and copied.  param: the tracer of GB25_KIN_GRADIENT and GB25_KIN_FRONTOGENESIS, 0 .. 2; 0 for the others.
 *      gb25_compute_kinematics: into the derived fields' array (made by the first call that needs it, freed by gb25_destroy); *dev:
 *      elements of the library's float type, PACKED, device_dims = the columns, the rows, the levels of the window, i fastest;
 *      read-only, complete when the call returns, valid until the next diagnostics call on m.  gb25_get_kinematics: the same and
 *      one device-to-host copy of exactly those elements.  gb25_get_kinematics_stats: gb25_field_stats of the whole quantity,
 *      positions relative to its box.  Refused by name before anything is allocated or launched: an unknown q, a param out of
 *      range, a window outside 0 .. Nz, a NULL pointer, a model without a device. */
typedef enum { GB25_KIN_DIVERGENCE = 0, GB25_KIN_NORMAL_STRAIN, GB25_KIN_SHEAR_STRAIN, GB25_KIN_OKUBO_WEISS,
               GB25_KIN_ROSSBY_NUMBER, GB25_KIN_GRADIENT, GB25_KIN_FRONTOGENESIS, GB25_KIN_COUNT } gb25_kinematics;
gb25_status gb25_kinematics_dims(const gb25_model *m, gb25_kinematics q, int32_t dims[3]);   /* needs no device */
gb25_status gb25_compute_kinematics(gb25_model *m, gb25_kinematics q, int32_t param, int32_t k_first, int32_t k_count,
                                    const void **dev, int32_t device_dims[3]);
gb25_status gb25_get_kinematics(gb25_model *m, gb25_kinematics q, int32_t param, int32_t k_first, int32_t k_count, void *host);
gb25_status gb25_get_kinematics_stats(gb25_model *m, gb25_kinematics q, int32_t param, gb25_field_stats *out);

/* ---- zonal-mean and eddy statistics on the device (csrc/zonal_eddy_kernels.hpp, k_zonal_eddy): the split of the flow into the
 *      mean along a line and the eddies about it -- the second moments about the ZONAL mean and the covariances of two different
 *      variables along a row, which no other family here has: the eddy kinetic energy, the eddy heat and momentum fluxes [V*T*],
 *      [U*V*] by latitude and depth, the terms of the Lorenz energy cycle (gb-25_amd/eddies.py, lorenz_cycle).  Same contract as
 *      every diagnostic here: the state gb25_get_field would return (the corrected velocities and the stored w a returned call
 *      leaves), READ-ONLY for the schedule (nothing pinned, every look-ahead alive), LOCAL on a rank, bitwise repeatable, no
 *      atomics, launches under GB25_K_DIAGNOSTICS on the model's stream.
 *
 *      VARIABLES.  Six per interior cell (i, j, k), fp64 on (double) of the stored values with floating-point contraction OFF (no
 *      fused multiply-adds: every product, sum and difference rounds by itself), all at the cell centre:
 *        GB25_ZE_U      0.5 (u(i,j,k) + u(i+1,j,k))
 *        GB25_ZE_V      0.5 (v(i,j,k) + v(i,j+1,k))
 *        GB25_ZE_W      0.5 (w(i,j,k) + w(i,j,k+1))
 *        GB25_ZE_T      T(i,j,k)
 *        GB25_ZE_S      S(i,j,k)
 *        GB25_ZE_SIGMA  the value gb25_get_derived(GB25_D_POTENTIAL_DENSITY) hands out for the cell, rounded to the float type first
 *      u(i+1) and v(j+1) beyond the interior are the halo cells the step leaves filled: the periodic image, a neighbour's column
 *      on a slab, the wall row, the fold's image.
 *
 *      WEIGHT.  mu(i,j,k) is THE MEASURE of gb25_integrate_field for a (c,c,c) field: area x thickness x 1/2 on the pivot row of
 *      a folded grid x wet mask, from the same tables by the same expression.  A cell COUNTS iff mu > 0 and all six values are
 *      finite; a cell with mu > 0 and any value not finite is skipped whole in both passes and counted once in `nonfinite`; an
 *      immersed cell is invisible.
 *
 *      RECORD.  A line is interior row j, level k, along the grid's index i (a latitude circle on the LatitudeLongitudeGrid only,
 *      as for the spectra; the sums are defined on every grid type).  Pass 1 over the line forms measure, first, points and
 *      nonfinite; then mean[q] = first[q] / measure, ONE IEEE division (+0.0 if measure == 0), or the caller's means; pass 2 forms
 *      d_q = x_q - mean[q] (one fp64 subtraction) and co[p, q] = sum (mu d_p) d_q for p <= q, row-major over (p, q): index
 *      p (11 - p) / 2 + q.  The deviations are taken about the ROUNDED mean, hence the two passes.
 *
 *      ORDER, fixed: that of the ROWS of gb25_integrate_field.  One wave per line; the line is cut into chunks of four cells
 *      aligned to four elements in MEMORY -- the first chunk holds the 4 - a first cells, a = (H + (Nx + 2H) ((j + H) + (Ny + 2H)
 *      (k + H))) mod 4 the element offset of the line's first cell in the parent array of T, whose allocation is aligned --; lane
 *      l takes the chunks l, l + 64, ... and adds its cells in ascending i; the 64 lanes are combined by lane l <- lane l + lane
 *      (l + off), off = 1, 2, 4, 8, 16, 32, the answer in lane 0.  Every sum starts from +0.0, a cell that does not count adds
 *      nothing.  measure and points of a line equal the ROWS record of gb25_integrate_field(GB25_T) bit for bit.
 *
 *      gb25_get_zonal_eddy: the records of the levels [k_first, k_first + k_count) (k_count = -1: all from k_first on), out[kk Ny +
 *      j] for level k_first + kk and local row j.  means: NULL, or [k_count][Ny][6] doubles -- pass 1 still runs and reports measure
 *      and first, the deviations are taken about the caller's numbers and mean echoes them: the ranks of a decomposition share one
 *      mean this way (gb-25_amd/eddies.py, combine_zonal_eddy), and eddies about a time mean are taken this way.  Refused by name,
 *      the model untouched: a NULL out, a window outside 0 .. Nz, a means entry that is not finite, a model without a device.
 *      gb25_zonal_eddy_dims: the rows and the levels of the rank, from the configuration alone. */
typedef enum { GB25_ZE_U = 0, GB25_ZE_V, GB25_ZE_W, GB25_ZE_T, GB25_ZE_S, GB25_ZE_SIGMA, GB25_ZE_COUNT } gb25_zonal_eddy_variable;
typedef struct {
  double measure;        /* sum mu over the counted cells                                                */
  double first[6];       /* sum mu x_q                                                                   */
  double mean[6];        /* first[q] / measure; +0.0 if measure == 0; or the caller's means, echoed      */
  double co[21];         /* sum (mu d_p) d_q, p <= q, row-major over (p, q); d_q = x_q - mean[q]         */
  int64_t points, nonfinite;
} gb25_zonal_eddy_row;
int32_t gb25_zonal_eddy_bytes(void);    /* sizeof the struct as THIS library was built */
gb25_status gb25_zonal_eddy_dims(const gb25_model *m, int32_t dims[2]);   /* rows, levels; needs no device */
gb25_status gb25_get_zonal_eddy(gb25_model *m, int32_t k_first, int32_t k_count, const double *means, gb25_zonal_eddy_row *out);

/* ---- block sums on the device (csrc/block_kernels.hpp, k_block_sums): the one reduction of the family that gb25_integrate_field
 *      (rows, levels, the total) does not have -- a MAP.  The interior of a field, or of a derived field, is cut into boxes of
 *      bx x by x bz points and every box gets measure = sum mu', first = sum mu' x, second = sum mu' x^2 in fp64: block means on a
 *      4x or 8x coarser grid for an output writer, the sub-grid variance, column integrals, the heat content of the upper 700 m --
 *      Oceananigans' Integral(field, dims = 3) and Average over boxes of cells -- without the parent array crossing PCIe.  Same
 *      contract as every diagnostic here: the state gb25_get_field would return (a stale GB25_PHY recomputed, previous velocities
 *      read where they live), READ-ONLY for the schedule (nothing pinned, every look-ahead alive), LOCAL on a rank (gather by
 *      global_offset: gb-25_amd/blocks.py gather_blocks), bitwise repeatable, no floating-point atomics, launches under
 *      GB25_K_DIAGNOSTICS on the model's stream.
 *
 *      BLOCKS (gb25_blocks).  bx divides the rank's interior Nx, 1 <= bx <= 256 (whole rows are what GB25_SUM_ROWS is for).  by
 *      divides the rank's Ny, the rows of cell centres: the extra wall row Ny of a (c,f) field lies in no block (its measure is
 *      0).  k_first, k_count select levels as in gb25_get_derived (k_count = -1: all from k_first on) in the field's OWN level
 *      count -- Nz + 1 for w and the kappas --; bz divides the resolved k_count.  A 2-D field takes bz = 1 and levels 0, 1 or
 *      0, -1.  The result has dims (Nx / bx, Ny / by, k_count / bz), I fastest.
 *      mu is THE MEASURE of gb25_integrate_field above, by the field's location: the same expression from the same tables.
 *      LEVEL WEIGHTS.  level_weight (may be NULL): one double per level of the FIELD (not of the window), finite and >= 0;
 *      mu' = mu * level_weight[k], one fp64 multiply.  With NULL mu' = mu and no multiply is made.  A fraction per level says
 *      "0 to 700 m" with partial cells.  A 2-D field refuses a non-NULL vector.
 *      COUNTING.  A point counts iff mu' > 0 and x = (double) of the stored value is finite.  A point with mu' > 0 whose x is
 *      not finite is skipped and counted in nonfinite.  A value in an immersed cell is invisible.
 *      TERMS.  t = mu' * x, q = t * x; fp64, NO fused multiply-adds (gb25_integrate_field forms `second` with one: the two
 *      differ in the last bits).
 *      REDUCTION ORDER, member by member, every sum starting from +0.0; a point that does not count adds nothing:
 *        1. the column partial  c(i, j) = the block's levels, ascending k
 *        2. the segment         s(I, j) = c(i, j) over the block's bx columns, ascending i
 *        3. the block           = s(I, j) over the block's by rows, ascending j
 *      gb-25_amd/blocks.py block_sums_host restates it with numpy bit for bit.
 *      gb25_block_info: the result's dims; points and nonfinite totalled over all blocks; empty_blocks = the blocks whose measure
 *      is 0; global_offset as in gb25_field_stats (of the FINE interior: block I starts at fine column I bx + 1).
 *      gb25_get_block_sums: each of measure, first, second may be NULL (all three: an error); only the planes asked for are
 *      copied.  gb25_compute_block_sums: the three planes one after another (measure, first, second; dims[0] dims[1] dims[2]
 *      doubles each) in an array the model owns (made by the first call, made anew when a call needs more, freed by
 *      gb25_destroy); read-only, complete when the call returns, valid until the next call on m.
 *      gb25_get_derived_block_sums: gb25_compute_derived into the model's packed array, then the same kernel over it; the
 *      measure is that of (c,c,c), or of 2-D (c,c) for the mixed-layer depth.  GB25_D_VORTICITY lives at (f,f,c), which has no
 *      measure in the table: GB25_ERR_INVALID_ARGUMENT.
 *      ERRORS, each GB25_ERR_INVALID_ARGUMENT with a message that names the argument: a block extent <= 0 or one that does not
 *      divide, bx > 256, a window outside the field, a weight that is negative or not finite, weights on a 2-D field, no output
 *      requested. */
#define GB25_BLOCK_MAX_BX 256
typedef struct {
  int32_t bx, by, bz;
  int32_t k_first, k_count;          /* levels of the field; k_count = -1: all from k_first on */
  int32_t reserved;
} gb25_blocks;
typedef struct {
  int32_t dims[3], reserved;
  int64_t points, nonfinite, empty_blocks;
  int32_t global_offset[3], reserved2;
} gb25_block_info;
int32_t gb25_block_info_bytes(void);
gb25_status gb25_block_dims(const gb25_model *m, gb25_field f, const gb25_blocks *blocks, int32_t dims[3]);   /* needs no device */
gb25_status gb25_derived_block_dims(const gb25_model *m, gb25_derived q, const gb25_blocks *blocks, int32_t dims[3]);   /* needs no device */
gb25_status gb25_get_block_sums(gb25_model *m, gb25_field f, const gb25_blocks *blocks, const double *level_weight /* may be NULL */,
                                double *measure, double *first, double *second, gb25_block_info *info /* may be NULL */);
gb25_status gb25_compute_block_sums(gb25_model *m, gb25_field f, const gb25_blocks *blocks, const double *level_weight,
                                    gb25_block_info *info, const double **dev, int32_t device_dims[3]);
gb25_status gb25_get_derived_block_sums(gb25_model *m, gb25_derived q, double param, const gb25_blocks *blocks,
                                        const double *level_weight, double *measure, double *first, double *second,
                                        gb25_block_info *info);

/* ---- moving-window filter on the device (csrc/filter_kernels.hpp, k_filter_x, k_filter_y): what the block sums cannot give --
 *      their boxes are disjoint, so block means jump at box edges and x - mean is not defined per point.  Here every output point
 *      has a window of its own, centred on it: the filtered field xbar on the model grid, the eddy part x' = x - xbar and the
 *      variance below the filter scale, the first step of every scale separation of an eddying run, without the parent array
 *      crossing PCIe.  HORIZONTAL, level by level, over the interior of a field or of a derived field at (c,c).  Same contract as
 *      every diagnostic here: the state gb25_get_field would return (a stale GB25_PHY recomputed, previous velocities read where
 *      they live), READ-ONLY for the schedule (nothing pinned, every look-ahead alive), bitwise repeatable, no floating-point
 *      atomics, launches under GB25_K_DIAGNOSTICS on the model's stream.  NOT on a rank of a decomposition (below).
 *
 *      MEASURE AND COUNTING.  mu is THE MEASURE of gb25_integrate_field above, by the field's location: the same tables and the
 *      same expression as the block sums (one device function serves both kernels), the pivot row's 1/2 included.  A source point
 *      counts iff mu > 0 and x = (double) of the stored value is finite; then m = mu, t = mu * x, q = t * x in fp64, NO fused
 *      multiply-adds; otherwise its m, t and q are +0.0.  A point with mu > 0 whose x is not finite is counted ONCE in nonfinite:
 *      per source point of the rows 0 .. Ny - 1 of the window of levels, not per window that contains it, and whether or not
 *      a window contains it.  A value in an immersed cell is invisible.
 *      WINDOW (gb25_filter).  Radii 0 <= rx, ry <= GB25_FILTER_MAX_RADIUS in grid points; strides sx | Nx and sy | Ny (a filtered
 *      field is smooth: a caller need not download every point).  Output point (I, J, K) is centred on the fine point
 *      (I sx, J sy, k_first + K); the result has dims (Nx / sx, Ny / sy, k_count), I fastest.  k_first, k_count select levels as
 *      in gb25_blocks (k_count = -1: all from k_first on) in the field's OWN level count; a 2-D field takes 0, 1 or 0, -1.
 *      EDGES.  x wraps modulo Nx: every grid type of this library is periodic in x (LatitudeLongitudeGrid and the tripolar grids
 *      alike have topology Periodic in x), so none is clipped there; 2 rx + 1 <= Nx is required, so that no point enters a window
 *      twice.  y is clipped to the rows 0 .. Ny - 1 of cell centres: the wall row Ny of a (c,f) field is in no window, nothing
 *      reaches across the fold; a clipped window is simply smaller, and the measure plane normalises it.
 *      WEIGHTS (both may be NULL).  wx[2 rx + 1], wy[2 ry + 1]: fp64, finite, >= 0, each with a positive sum.  NULL is the box
 *      filter, and no multiply is made.  A Gaussian and a triangle are vectors the host builds (gb-25_amd/filters.py
 *      kernel_weights).
 *      FIXED PHYSICAL WIDTH.  rx_of_row (may be NULL): Ny int32, the rx of every row j -- of the x sums s(., j), whichever y
 *      windows they then enter --, each 0 .. GB25_FILTER_MAX_RADIUS with 2 rx + 1 <= Nx; rx of gb25_filter is then ignored (but
 *      checked).  On the LatitudeLongitudeGrid dx at 80 degrees is 5.7 times smaller than at the equator.  Refused together with wx:
 *      with a radius per row x is the box.
 *      REDUCTION ORDER, plane by plane (m, t and q alike), every sum starting from +0.0:
 *        1. s(i, j) = sum over d = -rx .. rx, ascending, of [wx[d + rx] *] a(wrap(i + d), j)
 *        2. b(i, j) = sum over e = -ry .. ry, ascending, rows outside 0 .. Ny - 1 skipped, of [wy[e + ry] *] s(i, j + e)
 *      A weight times a term rounds by itself, then the addition.  measure = b of m, first = b of t, second = b of q:
 *      xbar = first / measure, the variance below the filter scale = second / measure - xbar^2.  gb-25_amd/filters.py
 *      filter_sums_host restates it with numpy bit for bit.
 *      gb25_filter_info: the result's dims; nonfinite (above); empty = the outputs whose measure is 0; clipped = the outputs whose
 *      y window was cut; global_offset as in gb25_field_stats (of the FINE interior).
 *      gb25_get_filter_sums: each of measure, first, second may be NULL (all three: an error); only the planes asked for are
 *      computed beyond the x pass's LDS and copied.  gb25_compute_filter_sums: the three planes one after another (measure, first,
 *      second; dims[0] dims[1] dims[2] doubles each) in an array the model owns (with the x pass's scratch planes ONE allocation,
 *      made by the first call, made anew when a call needs more, freed by gb25_destroy; its size is checked against the free device
 *      memory BEFORE it is allocated: GB25_ERR_OUT_OF_MEMORY leaves nothing allocated); read-only, complete when the call returns,
 *      valid until the next call on m.  gb25_get_derived_filter_sums: gb25_compute_derived into the model's packed array, then the
 *      same kernels over it; the measure is that of (c,c,c), or of 2-D (c,c) for the mixed-layer depth.  GB25_D_VORTICITY lives at
 *      (f,f,c), which has no measure in the table: GB25_ERR_INVALID_ARGUMENT.
 *      RANKS OF A DECOMPOSITION.  A window reaches beyond the rank's columns and rows, and the halo exchanges are not widened for
 *      it: on a rank (nranks > 1 or slab_mode = 1) the three device entries return GB25_ERR_STATE and say so.  The dims need no
 *      device and answer there too.  gb-25_amd/distributed.py LocalSlabEnsemble.filter_sums gathers on the host.
 *      ERRORS, each GB25_ERR_INVALID_ARGUMENT with a message that names the argument, the model stays usable: a radius that is
 *      negative or above the maximum, 2 rx + 1 > Nx, a stride that does not divide, a window of levels outside the field, a weight
 *      that is negative or not finite, weights that sum to zero, wx together with rx_of_row, no output requested. */
#define GB25_FILTER_MAX_RADIUS 32
typedef struct {
  int32_t rx, ry;                    /* radii in grid points */
  int32_t sx, sy;                    /* strides of the output; 1, 1: every point */
  int32_t k_first, k_count;          /* levels of the field; k_count = -1: all from k_first on */
  int32_t reserved;
} gb25_filter;
typedef struct {
  int32_t dims[3], reserved;
  int64_t nonfinite, empty, clipped;
  int32_t global_offset[3], reserved2;
} gb25_filter_info;
int32_t gb25_filter_info_bytes(void);
gb25_status gb25_filter_dims(const gb25_model *m, gb25_field f, const gb25_filter *filter, int32_t dims[3]);   /* needs no device */
gb25_status gb25_derived_filter_dims(const gb25_model *m, gb25_derived q, const gb25_filter *filter, int32_t dims[3]);   /* needs no device */
gb25_status gb25_get_filter_sums(gb25_model *m, gb25_field f, const gb25_filter *filter, const double *wx /* may be NULL */,
                                 const double *wy /* may be NULL */, const int32_t *rx_of_row /* may be NULL */, double *measure,
                                 double *first, double *second, gb25_filter_info *info /* may be NULL */);
gb25_status gb25_compute_filter_sums(gb25_model *m, gb25_field f, const gb25_filter *filter, const double *wx, const double *wy,
                                     const int32_t *rx_of_row, gb25_filter_info *info, const double **dev, int32_t device_dims[3]);
gb25_status gb25_get_derived_filter_sums(gb25_model *m, gb25_derived q, double param, const gb25_filter *filter, const double *wx,
                                         const double *wy, const int32_t *rx_of_row, double *measure, double *first, double *second,
                                         gb25_filter_info *info);

/* ---- coherent regions on the device (csrc/region_kernels.hpp, k_region_*): every diagnostic above reduces along an index, a box,
 *      a window or a class.  This one answers what a baroclinic-instability run is made for -- how many eddies are there, how big
 *      are they, where are they, what do they carry: a plane of a centre-located quantity is thresholded, its connected regions
 *      are labelled, and every region gets one record whose sums run in a fixed order, without the plane crossing PCIe.  Same
 *      contract as every diagnostic here: the state gb25_get_field would return, READ-ONLY for the schedule (nothing pinned, every
 *      look-ahead alive), bitwise repeatable, no floating-point atomics, launches under GB25_K_DIAGNOSTICS on the model's
 *      stream.  NOT on a rank of a decomposition (below).
 *
 *      DEFINITIONS.
 *      CRITERION.  x(i, j, k) at (Center, Center, Center) on the interior, Nx x Ny per level, from one of three sources:
 *        GB25_REGION_FIELD       id = a gb25_field: GB25_T, GB25_S or GB25_E, read where it lies; param = 0
 *        GB25_REGION_DERIVED     id = a gb25_derived: GB25_D_KINETIC_ENERGY, GB25_D_DENSITY_ANOMALY or GB25_D_POTENTIAL_DENSITY; param = 0
 *        GB25_REGION_KINEMATICS  id = a gb25_kinematics: GB25_KIN_DIVERGENCE, GB25_KIN_NORMAL_STRAIN, GB25_KIN_OKUBO_WEISS,
 *                                GB25_KIN_GRADIENT or GB25_KIN_FRONTOGENESIS with its param
 *      The bits of x are the bits gb25_get_field, gb25_get_derived and gb25_get_kinematics hand out (the last two are computed by
 *      their own launches into the model's packed array and read from there).  A quantity at the corners (GB25_D_VORTICITY,
 *      GB25_KIN_SHEAR_STRAIN, GB25_KIN_ROSSBY_NUMBER), the 2-D GB25_D_MIXED_LAYER_DEPTH and every other field (the face fields
 *      among them) are refused by name.
 *      FOREGROUND.  cmp = GB25_REGION_BELOW or GB25_REGION_ABOVE.  A cell is foreground iff x < (real)threshold (ABOVE: >), compared
 *      in the library's float type, AND x is finite AND mu(i, j, k) > 0 with mu THE MEASURE of gb25_integrate_field at (c,c,c): land
 *      and the cells below the bottom are background.  nonfinite_cells counts the cells with mu > 0 whose x is not finite.
 *      CONNECTIVITY.  Levels are labelled independently.  Within a level cells are neighbours across their four faces
 *      (4-connectivity); column Nx - 1 is the neighbour of column 0 exactly where the grid is periodic in x (every single domain of
 *      this library is).  There is NO connection across a wall (rows 0 and Ny - 1 have no neighbour beyond) and NONE across the
 *      tripolar fold: on a folded grid the two halves of the last row meet physically, here they are joined only through the cells
 *      between them.
 *      LABELS.  A region's key is the smallest linear index i + Nx j among its cells; the regions of a level are numbered 0 .. n - 1
 *      in ascending order of key.  The label plane is int32, Nx x Ny per level of the window (i fastest, then j, then the level):
 *      the region's number in a foreground cell, -1 in a background cell.  This is unique: any correct algorithm gives these bits.
 *      RECORD (gb25_region), one per region: cells; the key's (key_i, key_j); the box i_min .. i_max, j_min .. j_max of its cells
 *      (columns as stored: a region across the seam has 0 and Nx - 1); wraps = 1 iff the grid is periodic in x and some row has
 *      both its column 0 and its column Nx - 1 in the region; measure = sum mu, first = sum mu x, second = sum mu x^2, carried = sum
 *      mu y for the optional second field y (carried_field = GB25_T, GB25_S or GB25_E; -1: none, carried = 0; y is not tested for
 *      being finite); sum_di = sum mu di, sum_dj = sum mu dj with di = i - key_i, on a periodic grid wrapped into [-Nx/2, Nx/2)
 *      (di - Nx where 2 di >= Nx, di + Nx where 2 di < -Nx), and dj = j - key_j: the centroid is (key_i + sum_di / measure, key_j +
 *      sum_dj / measure); extreme = the smallest x of the region for BELOW, the largest for ABOVE, at (extreme_i, extreme_j): of
 *      equal values the cell with the smallest linear index.
 *      ARITHMETIC OF THE SUMS.  x, y = (double) of the stored values; the terms are mu, t = mu * x, q = t * x, mu * y, mu *
 *      (double)di, mu * (double)dj: fp64 products that round by themselves, NO fused multiply-adds.  Every sum starts from +0.0 and
 *      is sequential, acc = acc + term, over the region's cells in ascending linear index.  No floating-point atomics.
 *      gb-25_amd/regions.py (label_host, region_records_host) restates labels and records with numpy bit for bit.
 *      CAP.  max_regions >= 1 records per level.  gb25_regions_info, one per level: regions = the true count; stored =
 *      min(regions, max_regions): the records of the regions 0 .. stored - 1, the others are dropped; foreground_cells;
 *      nonfinite_cells.  The label plane is always complete.
 *      gb25_label_regions: the device-pointer form.  *dev_labels: int32 [Nx Ny k_count]; *dev_records: gb25_region, level kk's at
 *      kk max_regions, its first `stored` valid; in an array the model owns (made by the first call, made anew when a call needs
 *      more, freed by gb25_destroy; its size is checked against the free device memory before it is allocated); read-only,
 *      complete when the call returns, valid until the next call on m.  info: k_count records on the host.  Either pointer
 *      argument may be NULL.
 *      gb25_get_regions: the host form.  labels (may be NULL: then only the records and infos cross PCIe) [Nx Ny k_count];
 *      records [max_regions k_count], level kk's at kk max_regions, those beyond `stored` zeroed; info [k_count].
 *      k_first, k_count select levels as in gb25_get_kinematics (k_count = -1: all from k_first on).  The levels of a window are
 *      processed one after another; each equals the call of that level alone.
 *      STATIC BOUNDS.  Every device loop has one.  Should a union-find walk ever exhaust its Nx Ny hops the call returns
 *      GB25_ERR_STATE and names the level.
 *      RANKS OF A DECOMPOSITION.  A region reaches beyond the rank's columns and rows: on a rank (nranks > 1 or slab_mode = 1)
 *      the two device entries return GB25_ERR_STATE and say so.  gb25_region_dims needs no device and answers there too.
 *      ERRORS, each GB25_ERR_INVALID_ARGUMENT with a message that names the argument, refused before the device is touched, the
 *      model stays usable and an earlier result readable: an unknown source_kind, id, param or cmp, a quantity that is not at
 *      (c,c,c), a carried_field other than T, S, E or -1, a threshold that is NaN, a window outside the levels, max_regions < 1,
 *      no output requested. */
typedef enum { GB25_REGION_FIELD = 0, GB25_REGION_DERIVED = 1, GB25_REGION_KINEMATICS = 2 } gb25_region_source;
typedef enum { GB25_REGION_BELOW = 0, GB25_REGION_ABOVE = 1 } gb25_region_cmp;
typedef struct {
  int32_t cells;
  int32_t key_i, key_j;              /* 0-based local interior indices, here and below */
  int32_t i_min, i_max, j_min, j_max;
  int32_t wraps;
  int32_t extreme_i, extreme_j;
  double measure, first, second, carried;
  double sum_di, sum_dj;
  double extreme;
} gb25_region;
typedef struct {
  int32_t regions, stored;
  int64_t foreground_cells, nonfinite_cells;
} gb25_regions_info;
int32_t gb25_region_bytes(void);          /* sizeof the two structs as THIS library was built */
int32_t gb25_regions_info_bytes(void);
gb25_status gb25_region_dims(const gb25_model *m, int32_t dims[3]);   /* Nx, Ny, the levels; needs no device */
gb25_status gb25_label_regions(gb25_model *m, gb25_region_source source_kind, int32_t id, int32_t param, int32_t carried_field,
                               gb25_region_cmp cmp, double threshold, int32_t k_first, int32_t k_count, int32_t max_regions,
                               const void **dev_labels, const void **dev_records, gb25_regions_info *info);
gb25_status gb25_get_regions(gb25_model *m, gb25_region_source source_kind, int32_t id, int32_t param, int32_t carried_field,
                             gb25_region_cmp cmp, double threshold, int32_t k_first, int32_t k_count, int32_t max_regions,
                             int32_t *labels /* may be NULL */, gb25_region *records, gb25_regions_info *info);

/* ---- time averages and eddy fluxes accumulated on the device (csrc/averages_kernels.hpp, k_averages_accumulate): what the other
 *      diagnostics cannot do -- remember something between two calls.  The time-mean state, eddy kinetic energy and tracer
 *      variance, the eddy heat and salt fluxes <v'T'>, <u'T'>, <w'T'>: Oceananigans' AveragedTimeInterval, without five parent arrays
 *      crossing PCIe per sample.  A sample is taken by an explicit call between two composite calls.  Same contract as the
 *      diagnostics above: the state gb25_get_field would return, READ-ONLY for the schedule (nothing pinned, every look-ahead alive;
 *      the only memory written is the accumulators' own), LOCAL on a rank (a rank's interior; gather by global_offset:
 *      gb-25_amd/averages.py gather_averages), bitwise repeatable, launches under GB25_K_DIAGNOSTICS on the model's stream.
 *
 *      DEFINITIONS.  Values are read from the parent arrays as gb25_get_field(f, host, 1) returns them at that moment, halo cells
 *      included.  Every operation in fp64 on (double) of the stored values, in the written order, NO fused multiply-adds
 *      (gb-25_amd/averages.py restates them with numpy bit for bit).  Indices are 0-based interior; i-1, j-1 reach one halo column
 *      or row (and the wall row of v the halo row of tracers beyond it).  THE TERM of a quantity at a point:
 *        MEANS    GB25_A_U, _V, _W, _T, _S, _ETA   x, at the field's own location, with the interior dims of that field
 *        SQUARES  GB25_A_UU, _VV, _TT, _SS, _ETAETA   x * x
 *        FLUXES   GB25_A_UT, _US at (f,c,c), dims of u:  u(i,j,k) * (0.5 * (T(i-1,j,k) + T(i,j,k)))
 *                 GB25_A_VT, _VS at (c,f,c), dims of v:  v(i,j,k) * (0.5 * (T(i,j-1,k) + T(i,j,k)))
 *                 GB25_A_WT, _WS at (c,c,f), dims of w:  w(i,j,k) * (0.5 * (T(i,j,k-1) + T(i,j,k))) at the faces 1 .. Nz-1; exactly 0
 *                 at the bottom face 0 and at the top face Nz: no halo level is ever read
 *      ACCUMULATION: one sample adds acc = acc + weight * term (two roundings); weight_sum = weight_sum + weight on the host.
 *      NO MASK AND NO MEASURE: immersed cells hold what the model stores there.  A value that is not finite poisons the accumulator
 *      cells whose term reads it and nothing else.
 *      LEVEL WINDOW: k_first, k_count select CELL levels, 0-based; k_count = -1: all from k_first on (as for the derived fields).  A
 *      (c,c,f) quantity covers the k_count + 1 faces that bound them; the 2-D quantities ignore the window.  The window is what
 *      makes the accumulators of a very large model fit: 8 bytes per point and quantity.
 *      READ-OUT: gb25_get_average copies exactly the accumulator; normalized != 0: acc / weight_sum, one IEEE fp64 division per
 *      element done on the device.  PACKED, i fastest, dims as gb25_average_dims reports for the active window (before
 *      gb25_averages_begin: for the whole column); one device-to-host copy; any other count is GB25_ERR_INVALID_ARGUMENT.
 *
 *      gb25_averages_begin allocates and zeroes the accumulators of the requested groups only; GB25_AVG_MEANS must be among them
 *      (the eddy parts need the means).  The size is checked against the free device memory BEFORE anything is allocated:
 *      GB25_ERR_OUT_OF_MEMORY leaves nothing allocated.  On a model that already has averages it starts over.
 *      gb25_averages_accumulate: GB25_ERR_STATE before gb25_averages_begin; a weight that is not finite and > 0 is
 *      GB25_ERR_INVALID_ARGUMENT and touches nothing.  ONE launch per sample whatever the groups; complete when the call returns.
 *      A quantity of a group that was not asked for is GB25_ERR_INVALID_ARGUMENT.  gb25_average_device_ptr: the accumulator where
 *      it lives, read-only, valid until gb25_averages_begin / gb25_averages_end / gb25_destroy, which free the accumulators. */
typedef enum { GB25_AVG_MEANS = 1, GB25_AVG_SQUARES = 2, GB25_AVG_FLUXES = 4 } gb25_average_group;
typedef enum {
  GB25_A_U = 0, GB25_A_V, GB25_A_W, GB25_A_T, GB25_A_S, GB25_A_ETA,          /* MEANS   */
  GB25_A_UU, GB25_A_VV, GB25_A_TT, GB25_A_SS, GB25_A_ETAETA,                 /* SQUARES */
  GB25_A_UT, GB25_A_US, GB25_A_VT, GB25_A_VS, GB25_A_WT, GB25_A_WS,          /* FLUXES  */
  GB25_A_COUNT
} gb25_average;
/* groups, k_first, k_count (resolved: never -1): as begun; samples, weight_sum: so far; the clock at the first and the last sample */
typedef struct {
  int32_t groups, k_first, k_count, reserved;
  int64_t samples, first_iteration, last_iteration;
  double weight_sum, first_time, last_time;
} gb25_averages_info;
int32_t     gb25_averages_info_bytes(void);   /* sizeof the struct as THIS library was built */
gb25_status gb25_averages_begin(gb25_model *m, int32_t groups, int32_t k_first, int32_t k_count);
gb25_status gb25_averages_accumulate(gb25_model *m, double weight);
gb25_status gb25_averages_get_info(const gb25_model *m, gb25_averages_info *info);
gb25_status gb25_average_dims(const gb25_model *m, gb25_average a, int32_t dims[3]);
gb25_status gb25_get_average(gb25_model *m, gb25_average a, int32_t normalized, double *host, int64_t count);
gb25_status gb25_average_device_ptr(gb25_model *m, gb25_average a, const double **dev, int32_t device_dims[3]);
gb25_status gb25_averages_end(gb25_model *m);

/* ---- Lagrangian particles advected and sampled on the device (csrc/particle_kernels.hpp, k_particles_advance / k_particles_sample):
 *      where the water goes and what T and S it carries on the way -- Oceananigans' LagrangianParticles -- without u, v, w crossing
 *      PCIe after every step.  Same contract as the diagnostics above: the state gb25_get_field would return, halo cells included,
 *      READ-ONLY for the schedule (nothing pinned, every look-ahead alive; the only memory written is the particles' own
 *      allocation), LOCAL on a rank (the host hands particles over: gb-25_amd/particles.py exchange_particles), bitwise repeatable,
 *      launches under GB25_K_DIAGNOSTICS on the model's stream.
 *
 *      A PARTICLE is a cell (i, j, k), int32, 0-based in the rank's interior, the fractions (a, b, c), doubles in [0, 1), from the
 *      cell's western x face, southern y face and lower z face, and a status.  It sits at the index coordinates xi = i + a,
 *      eta = j + b, zeta = k + c.  A cell plus a fraction, not one double: the arithmetic does not depend on where the cell lies,
 *      so the ranks of a decomposition compute the bits of the single domain.
 *
 *      THE RATE of a position in cell (i, j, k), in cells per second: each component linear between the cell's own two faces in its
 *      own direction (the C-grid form whose normal rate vanishes on a wall or an immersed face).  fp64 on (double) of the stored
 *      values, IEEE divisions, NO fused multiply-adds, in the written order (gb-25_amd/particles.py restates all of this section
 *      with numpy bit for bit):
 *          dxi   = (1 - a) * (u(i, j, k) / dxu(i, j)) + a * (u(i+1, j, k) / dxu(i+1, j))
 *          deta  = (1 - b) * (v(i, j, k) / dyv(i, j)) + b * (v(i, j+1, k) / dyv(i, j+1))
 *          dzeta = ((1 - c) * w(i, j, k) + c * w(i, j, k+1)) / dzc(k)
 *      dxu = DXFC(i, j) on the grids with 2-D metrics, GB25_M_DXC(j) on the LatitudeLongitudeGrid; dyv = DYCF(i, j), GB25_M_DY there;
 *      dzc = GB25_M_DZC(k): the numbers gb25_get_metric / gb25_get_metric2 return.  Before a cell index enters an address it is
 *      clamped to [-halo, N + halo - 2] in its direction: no position reads outside an allocation.
 *      ONE SUBSTEP of length h = dt / substeps, a midpoint step on frozen fields, for an ACTIVE particle at p:
 *          r0 = rate(p);  pm = move(p, (0.5 * h) * r0);  r1 = rate(pm);  p <- move(p, h * r1)
 *      A displacement with a component that is not finite or not below 2^30 cells in magnitude freezes the particle where it is
 *      (at p) with GB25_PARTICLE_NONFINITE: a NaN in the fields stays where it is.
 *      move(p, d), component by component: a' = a + d; n = floor(a'); i += n; a' -= n; if a' >= 1 (a tiny negative d added to
 *      a = 1 - ulp rounds to 1) then i += 1, a' = 0.  Then, in this order:
 *        x     on a single periodic domain i wraps modulo Nx;
 *        y     below the GLOBAL southern wall: j = its row, b = 0; at or beyond the northern wall (on a folded grid: beyond the
 *              pivot row): j = the last row, b = the largest double below 1;
 *        z     below the first wet level kbot of the column the SUBSTEP STARTED IN: k = kbot, c = 0; at or above Nz: k = Nz - 1,
 *              c = the largest double below 1;
 *        dry   if kbot of the column it ends in (a halo column included) is above k: i, j, a, b return to their values at p
 *              (the horizontal move is undone, the vertical move is kept).
 *      The events of the SECOND move of a substep -- the one the particle makes -- are counted: clamped_y, clamped_z, blocked.
 *      After it:  folded grid: a particle with eta >= Ny - 0.5 (the centres of the pivot row) gets GB25_PARTICLE_AT_FOLD (also
 *      one found there when a substep starts) and is never advanced again; carrying particles through the zipper is not done.
 *      A rank with a neighbour on a side (x slabs, 2-D mesh): i may become -1 or Nx (j likewise) -- the particle keeps its
 *      rank-local position, gets GB25_PARTICLE_OUTSIDE and waits for the host to hand it over.  Either move of a substep ending
 *      more than one cell beyond the interior refuses the WHOLE CALL: GB25_ERR_STATE, "more than one cell per call: more substeps
 *      or a shorter dt", no particle is moved, last[GB25_PC_TOO_FAR] says how many particles asked for it.  A particle that leaves
 *      in one substep of a call sits out the rest of it: a rank makes ONE substep per call and the host hands over in between
 *      (gb-25_amd/distributed.py does), which by the next sentence is the single domain's advance(dt, substeps) bit for bit.
 *      Particles that are not GB25_PARTICLE_ACTIVE are not advanced; all are sampled.  advance(dt, n) equals n calls of
 *      advance(dt / n, 1) bit for bit.
 *
 *      gb25_particles_begin allocates room for `capacity` particles (two copies of the state -- a call writes the copy it does not
 *      read, which is how a refused call moves nothing --, the sample array, the per-wave counter slots, the kbot table); the size
 *      is checked against the free device memory BEFORE anything is allocated (GB25_ERR_OUT_OF_MEMORY leaves nothing allocated).
 *      On a model that already has particles it starts over.  gb25_particles_set writes particles [first, first + count) from
 *      host arrays as ACTIVE and makes first + count the number of particles (first <= the number so far: append, overwrite or
 *      truncate); a cell outside the interior, a fraction outside [0, 1) and a dry cell are refused, naming the first offender.
 *      gb25_particles_get: any of the seven arrays may be NULL.  gb25_particles_advance: ONE advance launch whatever the number
 *      of particles, complete when the call returns.  gb25_particles_sample: the value of a (c,c,c) field (T, S, e, pHY, ...) in
 *      each particle's cell as double -- a copy, hence exact; halo cells for OUTSIDE particles.  Every refused call names its
 *      argument and touches nothing; before gb25_particles_begin everything but gb25_particles_get_info is GB25_ERR_STATE. */
typedef enum {
  GB25_PARTICLE_ACTIVE = 0, GB25_PARTICLE_AT_FOLD = 1, GB25_PARTICLE_OUTSIDE = 2, GB25_PARTICLE_NONFINITE = 3
} gb25_particle_status;
typedef enum {
  GB25_PC_BLOCKED = 0, GB25_PC_CLAMPED_Y, GB25_PC_CLAMPED_Z, GB25_PC_AT_FOLD, GB25_PC_OUTSIDE, GB25_PC_NONFINITE, GB25_PC_TOO_FAR,
  GB25_PC_RESERVED, GB25_PC_COUNT
} gb25_particle_counter;
/* count, capacity; the accepted advance calls, their substeps and the model time they covered; the counters of the last advance
 * call (a too-far refusal included) and of all calls */
typedef struct {
  int64_t count, capacity, calls, substeps;
  double time_advanced;
  int64_t last[GB25_PC_COUNT], total[GB25_PC_COUNT];
} gb25_particles_info;
int32_t     gb25_particles_info_bytes(void);   /* sizeof the struct as THIS library was built */
gb25_status gb25_particles_begin(gb25_model *m, int64_t capacity);
gb25_status gb25_particles_set(gb25_model *m, int64_t first, int64_t count, const int32_t *i, const int32_t *j, const int32_t *k,
                               const double *a, const double *b, const double *c);
gb25_status gb25_particles_get(gb25_model *m, int64_t first, int64_t count, int32_t *i, int32_t *j, int32_t *k, double *a, double *b,
                               double *c, int32_t *status);
gb25_status gb25_particles_advance(gb25_model *m, double dt, int32_t substeps);
gb25_status gb25_particles_sample(gb25_model *m, gb25_field f, double *out, int64_t count);
gb25_status gb25_particles_get_info(const gb25_model *m, gb25_particles_info *info);
gb25_status gb25_particles_end(gb25_model *m);

/* ---- passive tracers carried beside a run (csrc/passive_host.hpp, csrc/passive_kernels.hpp: k_passive_update; gb-25_amd/passive.py
 *      restates the update).  A SET of 1 .. GB25_TRACERS_MAX tracers at the cell centres, advected by the model's u, v, w with the
 *      model's tracer advection scheme (WENO order 5 or 7), advanced by calls of its own BETWEEN the model's steps -- nothing inside
 *      a model step changes, and a model stepped with sets beside it gives the bits of one stepped alone: the calls are READ-ONLY for
 *      the schedule (nothing pinned, every look-ahead alive; the only memory written is the set's own allocation).  Single domains
 *      with closure = nothing.
 *      gb25_tracer_spec: `source` is added per second of model time (0: a dye; 1: an ideal age in seconds); with surface_reset != 0
 *      the top level is set to surface_value after every update (the boundary condition of ideal age); with clip_negative != 0 the
 *      update ends with c = max(c, 0) -- such a tracer is NO LONGER CONSERVED.
 *      A set has a clock of its own, started from the model's by gb25_tracers_begin.  gb25_tracers_advance moves the set over ONE
 *      step of the model's dt with u, v, w as they stand, and is valid only while the set's iteration equals the model's: call it
 *      BEFORE the model step that leaves the same state (advance, gb25_time_step, advance, ...).  Anything else is GB25_ERR_STATE with
 *      a message that names both iterations.  The first advance of a set, and the first after gb25_tracers_set, is an Euler step (as
 *      gb25_first_time_step is for the model); later ones are quasi-AB2 with the model's chi.  Per tracer: G^n = -div(U c) by the
 *      one-tracer tendency kernel of the model's grid; then ONE launch for the whole set,
 *          c <- (c + dt ((1.5 + chi) G^n - (0.5 + chi) G^-)) + dt source          (in the library's float type, NO fused multiply-add)
 *      then the surface reset, the clip, zero in immersed cells, and the halo cells the next tendency reads: the periodic x images,
 *      one layer beyond the y walls and the bottom / top, and on a folded grid the rows beyond the zipper by the rule of a centre
 *      field (cell (i, Ny-1+q) <- cell (Nx-1-i, Ny-1-q), no sign; GB25_OPT_FOLD_PIVOT_SLAVED is refused).  G^n and G^- then exchange
 *      by pointer.  The call returns when the launches are complete.  At model iteration 0 the fields hold what the host has set: w and
 *      the halo cells of u, v exist only once gb25_initialize and gb25_update_state have run (gb25_first_time_step runs them again, to
 *      the same bits), so a set that is to take the model's first step too is advanced between gb25_update_state and
 *      gb25_first_time_step (gb-25_amd/passive.py, run_with_tracers, does that).
 *      gb25_tracers_set / _get move tracer n (0-based) like gb25_set_field / gb25_get_field of GB25_T (same shapes, include_halos
 *      alike); set masks immersed cells, makes the halo cells above and makes the next advance an Euler step; get: which = 0: c,
 *      1: G^n of the last advance, 2: G^- (the one before).  gb25_tracers_stats: gb25_get_field_stats of c (interior).
 *      MEMORY: three parent arrays per tracer, one allocation per set, checked against the free device memory BEFORE it is made
 *      (GB25_ERR_OUT_OF_MEMORY leaves nothing allocated); gb25_tracers_end frees it, gb25_destroy frees the sets still open.
 *      Checkpoints do not contain tracer sets.
 *      REFUSED by name, before anything is allocated (begin) or launched (advance): a rank of a decomposition; a vertical
 *      diffusivity or CATKE (and gb25_set_vertical_diffusivity / gb25_set_closure_catke refuse to turn a closure on while a set is
 *      open); count outside 1 .. GB25_TRACERS_MAX; a set of another model (GB25_ERR_INVALID_ARGUMENT). */
#define GB25_TRACERS_MAX 8
typedef struct gb25_tracers gb25_tracers;   /* opaque; owned by the model it was begun on */
typedef struct {
  double source;            /* added per second of model time */
  double surface_value;     /* the value of the top level after every update ... */
  int32_t surface_reset;    /* ... when this is not 0 */
  int32_t clip_negative;    /* 0 | 1: c = max(c, 0) after every update (not conservative) */
} gb25_tracer_spec;
int32_t     gb25_tracer_spec_bytes(void);   /* sizeof the struct as THIS library was built */
gb25_status gb25_tracers_begin(gb25_model *m, int32_t count, const gb25_tracer_spec *specs, gb25_tracers **out);
gb25_status gb25_tracers_set(gb25_model *m, gb25_tracers *set, int32_t n, const void *host, int include_halos);
gb25_status gb25_tracers_get(gb25_model *m, gb25_tracers *set, int32_t n, int32_t which, void *host, int include_halos);
gb25_status gb25_tracers_advance(gb25_model *m, gb25_tracers *set);
gb25_status gb25_tracers_stats(gb25_model *m, gb25_tracers *set, int32_t n, gb25_field_stats *out);
gb25_status gb25_tracers_clock(gb25_model *m, gb25_tracers *set, double *time, int64_t *iteration);
gb25_status gb25_tracers_end(gb25_model *m, gb25_tracers *set);

/* ---- checkpoint and bit-for-bit restart ("Checkpoint and restart").  Single domains and ranks of a decomposition: each
 *      rank writes and reads its own file, the exchange context exists before the restore, another decomposition is refused.
 *      gb25_checkpoint_snapshot copies the restart set -- every parent array a step reads and a step wrote, halos included, bits as
 *      they are in memory (gb-25_amd/csrc/restart_plan.hpp) -- into a device arena in ONE launch on the model's stream (filed under
 *      GB25_K_DIAGNOSTICS), forming two integer checksums per member (s1 = sum x_n, s2 = sum (n + 1) x_n mod 2^64 over the bit
 *      patterns) in the same pass; a copy stream then drains the arena into pinned host memory behind an event, and the model's
 *      stream does not wait: gb25_loop may be called at once.  It voids no look-ahead and moves no buffer.  max_arena_bytes > 0
 *      bounds the arena: the set then passes through it in pieces, synchronously, and the file is the same byte for byte.
 *      gb25_checkpoint_write waits for the drain only and writes <directory>/<label>/restart_rank<R>.gb25 (to *.tmp, renamed when
 *      complete; label NULL or "": "checkpoint").  Without a snapshot it is GB25_ERR_STATE; so is a second snapshot before the
 *      first was written or released.  gb25_checkpoint_release frees the arena and the pinned buffers (gb25_destroy does too).
 *      Open averages and particle sessions are NOT saved: gb25_checkpoint_get_info says whether one was open.
 *      gb25_restore synchronises the model, and refuses with GB25_ERR_STATE and a message that names what differs: another float
 *      type, another configuration (shape, halo, rank / nranks / ranks_y, grid type, substeps, constants), a closure or the coupling
 *      on in one and off in the other, another grid (fingerprint of z faces, bottom and metrics: the host sets grid, bottom and
 *      atmosphere again BEFORE the restore), a checksum mismatch (naming the member).  A refused model is untouched.  Otherwise the
 *      fields, the clock and the scalar state are those of the snapshot, the recorded result-changing options are applied
 *      (options_changed: bit q = entry q of KERNELS, PRESSURE_PRECISION, MOMENTUM_CHUNK_LEVELS, TRACER_CHUNK_LEVELS, W_ON_THE_FLY,
 *      SUBSTEP_ORDER, FOLD_PIVOT_SLAVED, CATKE_STALE_E_HALOS), the look-aheads and column sums that were valid at the snapshot are
 *      members and valid again (everything else made ahead of time is void), and the steps that follow give the bits of the run
 *      that went on. */
typedef struct {
  int32_t taken, drained;       /* a snapshot waits to be written; its drain to the host has finished */
  int32_t members, pieces;      /* of the last snapshot (or restore) */
  int64_t bytes, arena_bytes;   /* the restart set; the device arena it passes through */
  int32_t averages_open_not_saved, particles_open_not_saved;
} gb25_checkpoint_info;
typedef struct {
  int32_t members, pieces;
  int64_t bytes;
  uint32_t options_changed;     /* which recorded options differed from the model's and were applied */
  int32_t tracer_rows_differ;   /* GB25_TRACER_ROWS was forced otherwise in the run that wrote the file (same bits either way) */
  int32_t phy_stale;            /* pHY' was not a member: it is recomputed from T, S when asked for */
  int32_t reserved;
} gb25_restore_info;
int32_t     gb25_checkpoint_info_bytes(void);   /* sizeof the structs as THIS library was built */
int32_t     gb25_restore_info_bytes(void);
gb25_status gb25_checkpoint_snapshot(gb25_model *m, int64_t max_arena_bytes /* 0: no cap */);
gb25_status gb25_checkpoint_write(gb25_model *m, const char *directory, const char *label);
gb25_status gb25_checkpoint_get_info(const gb25_model *m, gb25_checkpoint_info *info);
gb25_status gb25_checkpoint_release(gb25_model *m);
gb25_status gb25_restore(gb25_model *m, const char *directory, const char *label, gb25_restore_info *info);
gb25_status gb25_set_clock(gb25_model *m, double time, int64_t iteration, double last_dt);

/* ---- built-in per-kernel HIP-event timing (bench.py's roofline numbers) */
gb25_status gb25_profile_enable(gb25_model *m, int on); /* 0: off, 1: every kernel, 2 + k: kernel k alone */
gb25_status gb25_profile_reset(gb25_model *m);
gb25_status gb25_profile_get(gb25_model *m, gb25_kernel k, int64_t *launches, double *total_ms);

#ifdef __cplusplus
}
#endif
#endif /* GB25_H */
