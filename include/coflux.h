/*
 * coflux.h — C ABI of libcoflux: the MI355X-native surface-flux hot path of
 * ClimaOcean's OceanSeaIceModel (update_state! of the coupled model).
 *
 * Every entry point replaces one Julia function that the reference reaches through
 * multiple dispatch (there is no FFI in the reference; the seam is described in
 * SURVEY.md §8b).  All `path:line` citations are relative to the reference tree
 * (CliMA/ClimaOcean.jl v0.10.0).  The arithmetic itself lives in the un-vendored
 * NumericalEarth.jl package (Project.toml:21,31-32), so each entry cites the in-tree
 * call/config site that pins its signature and parameters.
 *
 * Conventions
 *  - plain C types only; no torch / HIP types in signatures (a stream is a `void*`
 *    holding a hipStream_t; NULL = the context's own stream).
 *  - every pointer named `d_*` or living inside a `cf_*_fields` struct is a DEVICE pointer.
 *  - ocean-grid 2-D arrays are column-major with halos, `i` fastest (Oceananigans
 *    `parent(field)` layout, omip_simulation.jl:184, KPP/kpp_surface_forcing.jl:49):
 *        element (i, j), 0-based interior index, lives at
 *        ptr[(j + hy) * (nx + 2*hx) + (i + hx)].
 *    For 3-D ocean fields pass the pointer to the k = Nz level slab.
 *  - footprints (the "Footprint:" line of each entry point): W is the ring window, cells (i, j) with −ring ≤ i < nx + ring,
 *    −ring ≤ j < ny + ring; I is the interior (ring 0).  Nothing outside the stated read set is read, nothing outside the
 *    write set is written, and pointers need only the element type's alignment (tests/test_layout_footprint.py).
 *  - all entry points return 0 on success, <0 on error; cf_last_error() explains.
 *    Nothing throws across the ABI.
 *  - a context is single-threaded; different contexts may be used from different threads.
 *    One context per GPU (one MPI rank / one process per GPU, launch.sh:229-232).
 */
#ifndef COFLUX_H
#define COFLUX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CF_ABI_VERSION 5 /* 2: cf_flux_params.shear_gustiness_coefficient; 3: CF_OPT_MAX_BLOCKS, CF_OPT_PROFILE_STRIDE, CF_OPT_FUSED_INTERP,
                          * CF_SOLVER_TABLES_R2(_OUTER) and the 768-thread geometry (CF_OPT_AO_CHUNK = 3072) retired; CF_OPT_AO_CHUNK and
                          * CF_OPT_INTERP_TILE_CAP are experiment options (COFLUX_EXPERIMENTS=1); 4: time averages accumulated on the
                          * device (cf_average_*, cf_attach_average; cf_run_schedule unchanged); 5: CF_SKIN_LINEARISED, a third
                          * value of cf_sea_ice_params.skin_temperature_scheme that older libraries reject; still 5: surface integrals and
                          * their time series (cf_integrals_*, cf_attach_integrals) are purely additive — no existing struct or
                          * entry point changed, a host finds them by symbol; likewise CF_OPT_INTERP_TILE_ROWS (an experiment option)
                          * and cf_debug_interp_grid, and the sparse surface operator (cf_regrid_*); likewise CF_OPT_LAND_ZEROS and
                          * cf_debug_land_zero_launches — with them cf_time_steps gained a contract on its outputs, stated there;
                          * likewise the surface monitor (cf_monitor_*, cf_attach_monitor); likewise cf_debug_prefetch_stats — with it
                          * a state requested ahead is matched by its source and weights as well, and a third pending request is
                          * refused when it is made: both stated at cf_prefetch_atmosphere_state; likewise the calendar-binned
                          * means (cf_climatology_*, cf_calendar_bin, cf_attach_climatology); likewise the staged dataset and
                          * the restoring that follows it (cf_dataset_*, cf_materialize_dataset_restoring,
                          * cf_attach_restoring_dataset) */

/* status codes */
#define CF_OK 0
#define CF_ERR_INVALID (-1)   /* bad argument / inconsistent config */
#define CF_ERR_HIP (-2)       /* HIP runtime error (message has file:line) */
#define CF_ERR_NODEVICE (-3)  /* no usable gfx950 device */
#define CF_ERR_COMM (-4)      /* RCCL error */

typedef struct cf_ctx cf_ctx;

/* ------------------------------------------------------------------------------------------
 * Grid / launch description.
 * Reference: LatitudeLongitudeGrid(arch; size=(1440,560,10), halo=(7,7,7)) README.md:56-61;
 * flux kernels are launched on 0:Nx+1 × 0:Ny+1 (one halo ring) in the reference
 * [UPSTREAM-RECALL interface_kernel_parameters] ⇒ ring = 1; ring = 0 computes the interior only.
 * ---------------------------------------------------------------------------------------- */
typedef struct cf_grid {
    int32_t nx, ny;      /* interior surface cells (local slab when sharded)            */
    int32_t hx, hy;      /* halo widths of every ocean-grid array handed to the library */
    int32_t ring;        /* 0 or 1: extra ring of cells the kernels also compute        */
    int32_t reserved;
} cf_grid;

/* ------------------------------------------------------------------------------------------
 * Flux formulation parameter block.
 * Mirrors SimilarityTheoryFluxes(FT; similarity_form, minimum_gustiness, gustiness_parameter,
 * stability_functions, momentum_roughness_length, temperature_roughness_length,
 * water_vapor_roughness_length) — omip_simulation.jl:42-49 (":corrected"), :63-69 (sea ice),
 * :106-113 (":ncar" sea ice), and the defaults used at README.md:75 / omip_simulation.jl:128-132
 * (":default" = Edson/COARE with constant Charnock 0.02, omip_simulation.jl:263).
 * ---------------------------------------------------------------------------------------- */

/* similarity_form */
#define CF_SIMILARITY_LOGARITHMIC 0        /* log(h/l) - psi(h/L) + psi(l/L)                */
#define CF_SIMILARITY_COARE_LOGARITHMIC 1  /* COARELogarithmicSimilarityProfile(): no psi(l/L), omip_simulation.jl:36,43 */

/* stability_functions */
#define CF_STABILITY_EDSON2013 0     /* default atmosphere–ocean (docs/climaocean.bib:1-10)            */
#define CF_STABILITY_SHEBA 1         /* atmosphere_sea_ice_stability_functions, omip_simulation.jl:56,64 */
#define CF_STABILITY_LARGE_YEAGER 2  /* large_yeager_stability_functions, omip_simulation.jl:96,107      */

/* momentum roughness */
#define CF_ROUGHNESS_CONSTANT 0        /* FT(5e-4), omip_simulation.jl:67                          */
#define CF_ROUGHNESS_CHARNOCK 1        /* MomentumRoughnessLength, constant Charnock (0.02)        */
#define CF_ROUGHNESS_WIND_CHARNOCK 2   /* WindDependentWaveFormulation, Edson 2013 eq. 13, :35,46 */

/* scalar roughness */
#define CF_SCALAR_ROUGHNESS_CONSTANT 0  /* FT(5e-5), omip_simulation.jl:68-69 */
#define CF_SCALAR_ROUGHNESS_REYNOLDS 1  /* ScalarRoughnessLength(FT; air_kinematic_viscosity), :48-49 */

/* air viscosity */
#define CF_VISCOSITY_CONSTANT 0
#define CF_VISCOSITY_TEMPERATURE_DEPENDENT 1 /* TemperatureDependentAirViscosity(FT), :41 */

/* flux formulation */
#define CF_FORMULATION_SIMILARITY 0      /* SimilarityTheoryFluxes (iteration on u★, θ★, q★ with roughness lengths) */
#define CF_FORMULATION_LARGE_YEAGER 1    /* CoefficientBasedFluxes + LargeYeagerTransferCoefficients, omip_simulation.jl:86-89 */

/* solver stop criteria */
#define CF_STOP_CONVERGENCE 0  /* default: |Δu★|+|Δθ★|+|Δq★| < tolerance or iteration ≥ maxiter */
#define CF_STOP_FIXED 1        /* FixedIterations(5), omip_simulation.jl:22,89                  */

/* velocity difference */
#define CF_VELOCITY_RELATIVE 0 /* RelativeVelocity(): Δu = u_atm − u_ocean, omip_simulation.jl:135 */
#define CF_VELOCITY_WIND 1     /* WindVelocity():     Δu = u_atm,           omip_simulation.jl:136 */

/* wet mask encoding */
#define CF_MASK_NONE 0
#define CF_MASK_U8 1            /* uint8 per cell, 1 = wet                                          */
#define CF_MASK_BOTTOM_HEIGHT 2 /* f64 bottom height; cell is land when z_surface_center <= zb      */

/* ocean albedo */
#define CF_ALBEDO_CONSTANT 0            /* SurfaceRadiationProperties(0.06, 1.00), atmosphere.jl:43 */
#define CF_ALBEDO_LATITUDE_DEPENDENT 1  /* α = a_diffuse − a_direct·cos(2φ) (Large & Yeager 2009)    */

typedef struct cf_roughness {
    int32_t kind;                 /* CF_ROUGHNESS_* (momentum) or CF_SCALAR_ROUGHNESS_* (scalars) */
    int32_t viscosity_kind;       /* CF_VISCOSITY_*                                              */
    double constant_length;       /* used when kind == *_CONSTANT                                 */
    double maximum_length;        /* cap (momentum 1.0; scalars 1.6e-4, COARE 3.6)                */
    double charnock;              /* Charnock parameter (constant form) / floor of α (wind-dependent form) */
    double laminar;               /* laminar parameter 0.11                                       */
    double wind_a1, wind_a2, wind_umax; /* wind-dependent α = max(charnock, a1·min(U,umax) + a2)  */
    double reynolds_A, reynolds_b;      /* scalar roughness ℓ = A / R★^b                            */
    double viscosity[4];          /* ν = c0 + c1 T' + c2 T'^2 + c3 T'^3 (T' in °C); c0 only if constant */
} cf_roughness;

typedef struct cf_thermodynamics {
    double gas_constant;          /* 8.3144598 */
    double dry_air_molar_mass;    /* 0.02897   */
    double water_molar_mass;      /* 0.018015  */
    double kappa_d;               /* 2/7       */
    double cp_v, cp_l, cp_i;      /* 1859, 4181, 2100 */
    double LH_v0, LH_s0;          /* 2500800, 2834400 */
    double T_0, T_triple, p_triple; /* 273.16, 273.16, 611.657 */
    double T_freeze, T_icenuc;    /* 273.15, 233 */
    double pow_icenuc;            /* 1 */
} cf_thermodynamics;

typedef struct cf_seawater {
    double water_molar_mass;      /* 18.02 (g/mol; used only as a ratio) */
    double constituent_molar_mass[4];    /* Cl 35.45, Na 22.99, SO4 96.06, Mg 24.31 */
    double constituent_mass_fraction[4]; /*    0.56,     0.31,      0.08,     0.05  */
} cf_seawater;

typedef struct cf_flux_params {
    int32_t struct_size;          /* sizeof(cf_flux_params), checked by the library */
    int32_t abi_version;          /* CF_ABI_VERSION */

    /* SimilarityTheoryFluxes */
    int32_t similarity_form;      /* CF_SIMILARITY_* */
    int32_t stability_functions;  /* CF_STABILITY_*  */
    int32_t stop_kind;            /* CF_STOP_*       */
    int32_t maxiter;              /* convergence: cap (100); fixed: the iteration count */
    int32_t velocity_difference;  /* CF_VELOCITY_*   */
    int32_t mask_kind;            /* CF_MASK_*       */
    double tolerance;             /* 1e-8 */
    double von_karman;            /* 0.4  */
    double gustiness_parameter;   /* β, 1 (0 in :ncar sea ice, omip_simulation.jl:109) */
    double minimum_gustiness;     /* 0.5 ocean :40,44; 0.2 ice :66 */
    double shear_gustiness_coefficient; /* c of the shear-aware gustiness (Mahrt & Sun 1995 / Edson 2013;
                                     experiments/OMIPSimulations/scripts/launch.sh:67-72,350, `:shear_aware`):
                                     0 (default) = off, the wind-speed scale is U² = |Δu|² + max((β w★)², U_G,min²);
                                     c > 0 (launch.sh: 0.04) = U² = |Δu|² + U_G², U_G² = (β w★)² + (c |Δu|)² + U_G,min²
                                     — the convective, shear and background terms ADD, and the shear term raises the
                                     gust at every wind speed.  The reference's own build_coupled_model rejects the
                                     symbol (omip_simulation.jl:160); the formula is the one its launcher states. */
    double similarity_profile_floor; /* guard: log(h/ℓ) − ψ(h/L) [+ψ(ℓ/L)] is floored at this value (1.0),
                                        i.e. transfer coefficients are capped at κ/floor.  Only the
                                        pathological first iterates from the 1e-4 initial guess (ζ ≈ −10⁵)
                                        ever reach it; converged states have 4 ≲ profile ≲ 20. */
    cf_roughness momentum_roughness;
    cf_roughness temperature_roughness;
    cf_roughness water_vapor_roughness;

    /* atmosphere properties (PrescribedAtmosphere) */
    double reference_height;      /* 10 m  */
    double boundary_layer_height; /* 600 m */
    double gravitational_acceleration; /* 9.81 */
    cf_thermodynamics thermo;
    cf_seawater seawater;

    /* ocean properties */
    double ocean_reference_density;   /* 1026,            visualize/common.jl:17 */
    double ocean_heat_capacity;       /* 3991.86795711963, visualize/common.jl:18 */
    double ocean_freshwater_density;  /* 1000: converts P, E mass fluxes to volume fluxes */
    double ocean_temperature_offset;  /* 273.15: ocean T is in °C                 */
    double ocean_minimum_salinity;    /* omip_simulation.jl:125,131,314; launch.sh:74-78 */
    double ocean_surface_z;           /* z of the top cell centre, for CF_MASK_BOTTOM_HEIGHT */

    /* radiation: SurfaceRadiationProperties(albedo, emissivity), atmosphere.jl:41-44 */
    int32_t ocean_albedo_kind;    /* CF_ALBEDO_* */
    int32_t penetrating_shortwave; /* 1: transmitted SW goes to the separate surface_flux field
                                      (KPP/kpp_surface_forcing.jl:47-51) and not into JT */
    double ocean_albedo;          /* 0.06 */
    double ocean_albedo_diffuse;  /* 0.069 */
    double ocean_albedo_direct;   /* 0.011 */
    double ocean_emissivity;      /* 1.0  */
    double stefan_boltzmann;      /* 5.67e-8 */

    /* CoefficientBasedFluxes(FT; transfer_coefficients = LargeYeagerTransferCoefficients(FT),
     * solver_stop_criteria = FixedIterations(5)) — omip_simulation.jl:79-89 (":ncar", OMIP-2): the
     * iteration runs on the transfer coefficients (Cd, Ch, Ce), not on roughness lengths.            */
    int32_t flux_formulation;     /* CF_FORMULATION_* */
    int32_t reserved1;
    double ly_minimum_wind;       /* 0.5 m/s floor on |Δu| (NCAR/CORE convention)                       */
    double ly_zeta_bound;         /* |ζ| ≤ 10                                                           */
    double ly_cd[4];              /* 10³·Cd_N10 = c0/U + c1 + c2·U + c3·U⁶: 2.7, 0.142, 0.0764, −3.14807e-10 */
    double ly_high_wind;          /* U ≥ 33 m/s ⇒ 10³·Cd_N10 = ly_cd_high (Large & Yeager 2009)         */
    double ly_cd_high;            /* 2.34 */
    double ly_ce;                 /* 10³·Ce_N10 = 34.6·√Cd_N10 */
    double ly_ch_stable;          /* 10³·Ch_N10 = 18.0·√Cd_N10 (ζ > 0) */
    double ly_ch_unstable;        /* 32.7·√Cd_N10 (ζ ≤ 0) */
} cf_flux_params;

/* Fill `p` with the ":default" configuration (omip_simulation.jl:128-132, :263). */
int cf_default_flux_params(cf_flux_params* p);

/* ------------------------------------------------------------------------------------------
 * Field bundles (device pointers, ocean-grid layout unless noted)
 * ---------------------------------------------------------------------------------------- */

/* Ocean surface state read by compute_atmosphere_ocean_fluxes! (k = Nz level): T (°C), S (g/kg)
 * at centres, u at x-faces, v at y-faces (src/ClimaOcean.jl:29 imports the ℑ operators).      */
typedef struct cf_ocean_surface {
    const double* T;
    const double* S;
    const double* u;
    const double* v;
    const void* mask;      /* per cf_flux_params.mask_kind; may be NULL for CF_MASK_NONE */
} cf_ocean_surface;

/* Atmosphere state on the exchange (ocean) grid: output of interpolate_atmosphere_state!,
 * input of the flux solver and of the net-flux assembly.                                       */
typedef struct cf_exchange_fields {
    double* u;   /* m/s, rotated to the grid-intrinsic frame */
    double* v;
    double* T;   /* K      (JRA55 tas)  */
    double* p;   /* Pa     (psl)        */
    double* q;   /* kg/kg  (huss)       */
    double* Qs;  /* W/m²   (rsds)       */
    double* Ql;  /* W/m²   (rlds)       */
    double* Mp;  /* kg/m²/s (prra+prsn) */
} cf_exchange_fields;

/* interface (turbulent) fluxes: model.interfaces.atmosphere_ocean_interface.fluxes.*,
 * omip_diagnostics.jl:81-82; positive = upward (ocean loses).                                  */
typedef struct cf_interface_fluxes {
    double* sensible_heat;  /* Qc  W/m²     */
    double* latent_heat;    /* Qv  W/m²     */
    double* water_vapor;    /* Fv  kg/m²/s  */
    double* x_momentum;     /* ρτx N/m²     */
    double* y_momentum;     /* ρτy N/m²     */
    double* temperature;    /* interface temperature Ts, ocean units (°C) */
    double* friction_velocity;    /* optional (may be NULL): u★ */
    double* temperature_scale;    /* optional: θ★ */
    double* humidity_scale;       /* optional: q★ */
    int32_t* iterations;          /* optional: iteration count per cell (diagnostic) */
} cf_interface_fluxes;

/* sea-ice inputs to the partition (atmosphere.jl:34-39, src/ClimaOcean.jl:62-63); all may be
 * NULL ⇒ ice-free.                                                                             */
typedef struct cf_sea_ice_fields {
    const double* concentration;   /* ℵ                        */
    const double* interface_heat;  /* Qio  W/m² (ice→ocean)    */
    const double* salt_flux;       /* Jˢio g/kg m/s            */
    const double* x_stress;        /* ice–ocean stress at u-faces, kinematic m²/s² */
    const double* y_stress;
} cf_sea_ice_fields;

/* net ocean fluxes: model.interfaces.net_fluxes.ocean.{u,v,T,S}, omip_diagnostics.jl:77-80.    */
typedef struct cf_net_ocean_fluxes {
    double* u;   /* τx kinematic m²/s² at u-faces (KPP/kpp_surface_forcing.jl:18-22) */
    double* v;   /* τy kinematic at v-faces                                           */
    double* T;   /* JT  K m/s   (hfds = JT·ρ·cp, visualize/cache.jl:359-361)          */
    double* S;   /* JS  g/kg m/s                                                      */
    double* shortwave_surface_flux; /* radiation.surface_flux (KPP/kpp_surface_forcing.jl:47-51); may be NULL */
    double* upwelling_longwave;     /* optional diagnostics, may be NULL */
    double* downwelling_longwave;
    double* downwelling_shortwave;
} cf_net_ocean_fluxes;

/* JRA55 source window on its native 640×320 grid (launch.sh:86-87), Float32, NO halos:
 *   value(var, level, js, is) = d_data[var][(level * ns_y + js) * ns_x + is].
 * Variable order follows jra55_data_staging.jl:8.                                               */
#define CF_JRA55_TAS 0
#define CF_JRA55_HUSS 1
#define CF_JRA55_PSL 2
#define CF_JRA55_UAS 3
#define CF_JRA55_VAS 4
#define CF_JRA55_RLDS 5
#define CF_JRA55_RSDS 6
#define CF_JRA55_PRRA 7
#define CF_JRA55_PRSN 8
#define CF_JRA55_NVARS 9

typedef struct cf_atmos_source {
    const float* data[CF_JRA55_NVARS]; /* device pointers, each [n_levels][ns_y][ns_x] */
    int32_t ns_x, ns_y;     /* 640, 320 */
    int32_t n_levels;       /* time indices in memory (atmosphere.jl:26, backend_size)  */
    int32_t level1, level2; /* the two bracketing snapshots n₁, n₂ (memory indices)     */
    double time_fraction;   /* ñ ∈ [0,1): value = ψ₂·ñ + ψ₁·(1−ñ)                       */
} cf_atmos_source;

/* Fractional source indices of every target cell (the reference precomputes the same pair,
 * `space_fractional_indices`).  Either separable (lat-lon → lat-lon: fi[i], fj[j]) or general
 * (tripolar: 2-D arrays in ocean-grid layout).  Optional rotation to the grid-intrinsic frame.  */
typedef struct cf_interp_weights {
    int32_t separable;      /* 1: fi has nx+2*hx entries, fj has ny+2*hy entries (halo-inclusive) */
    int32_t reserved;
    const double* fi;       /* 0-based fractional index along source x (periodic)  */
    const double* fj;       /* 0-based fractional index along source y (clamped)   */
    const double* cos_rot;  /* ocean-grid 2-D arrays or NULL (no rotation)         */
    const double* sin_rot;
    const double* latitude; /* φ (deg) per row (ny+2*hy) if separable else 2-D; needed only for
                               CF_ALBEDO_LATITUDE_DEPENDENT; may be NULL            */
} cf_interp_weights;

/* ------------------------------------------------------------------------------------------
 * Lifecycle
 * ---------------------------------------------------------------------------------------- */
int cf_version(void);
/* The first 16 hex digits of the sha256 over the library's sources (csrc/ *.hip, *.cpp, *.hpp, *.h and this header, in sorted
 * order) as they were when it was built: a host binding compares it with the tree it ships with and refuses a stale build. */
const char* cf_build_stamp(void);
/* Creates a context bound to HIP device `device`.  Fails (CF_ERR_NODEVICE) when there is no GPU. */
int cf_create(cf_ctx** out, int device, const cf_grid* grid, const cf_flux_params* params);
int cf_destroy(cf_ctx* ctx);
const char* cf_last_error(const cf_ctx* ctx); /* ctx may be NULL: last error of the calling thread */
int cf_set_flux_params(cf_ctx* ctx, const cf_flux_params* params);
/* hip_stream: a hipStream_t; NULL ⇒ the library-owned non-blocking stream; CF_STREAM_LEGACY ⇒ the
 * legacy default (null) stream, which is what torch's default stream is (its handle is 0).        */
#define CF_STREAM_LEGACY ((void*)1) /* == hipStreamLegacy */
int cf_set_stream(cf_ctx* ctx, void* hip_stream);

/* Options (cf_set_option).  None of them changes what is computed beyond the stated tolerance.  ELEVEN are part of the drop-in
 * surface: CF_OPT_SOLVER, _TRIP_HINTS, _FUSED_NET, _ICE_ORBIT_SHORTCUT, _MERGED_PREFETCH, _SOLVER_PATH, _CERTIFIED_BUDGET,
 * _ICE_FREE_CELLS, _LATENCY_LAYOUT, _HALO_IN_SOLVER_LAUNCH, _LAND_ZEROS.  Three more are EXPERIMENT options, accepted only in a
 * process started with COFLUX_EXPERIMENTS=1 (measurements, and the test-suite's schedule-invariance checks): CF_OPT_INTERP_TILE_CAP,
 * CF_OPT_AO_CHUNK, CF_OPT_INTERP_TILE_ROWS (and the value 2 of CF_OPT_LAND_ZEROS).
 * Numbers 5 and 8 were CF_OPT_PROFILE_STRIDE and _FUSED_INTERP (retired in ABI version 3: cf_set_option answers
 * CF_ERR_INVALID).  Number 2 was CF_OPT_MAX_BLOCKS until the same version (a host that still means that by it is refused at
 * cf_create by its abi_version) and is CF_OPT_LAND_ZEROS now.                                                            */
#define CF_OPT_SOLVER 0           /* CF_SOLVER_*                                                   */
#define CF_OPT_LAND_ZEROS 2       /* which launches of cf_update_state write zero_interface_state into the LAND cells of the flux and
                                   * net-flux outputs (six flux fields, `iterations`; J^T, J^S and the radiation diagnostics, τx, τy on
                                   * interior land): constants that do not depend on the step.
                                   * 0: every launch.  1 (default): every launch, except inside cf_time_steps, where only the FIRST step of a
                                   * call writes them — a later step whose solver launch goes the same way (same kernel family, same
                                   * CF_OPT_FUSED_NET decision) leaves the land cells of its chunks and of the face-stress launch alone:
                                   * they hold the first step's zeros (the contract at cf_time_steps).  cf_update_state and
                                   * cf_update_state_sea_ice called by the host always write.  A workgroup whose wet list proves stale (a
                                   * mask rewritten in place) classifies its range and writes its land whatever this says; launches that
                                   * do not know the option (CF_SOLVER_LIBM, un-fused net fluxes, the merged stress + interpolation launch,
                                   * the sea-ice interface launch) write as before.  Same bits on every cell either way
                                   * (tests/test_land_zeros.py).  2: never, not even the first step — an EXPERIMENT value
                                   * (COFLUX_EXPERIMENTS=1): one launch then shows what the skipping branch touches; land holds whatever it
                                   * held.  cf_debug_land_zero_launches counts.  -DCF_LAND_ZEROS_DEFAULT=0 builds a library whose default
                                   * is 0 (A/B runs).                                                                                     */
#define CF_OPT_INTERP_TILE_CAP 1  /* EXPERIMENT option.  Source nodes per variable in a wave's LDS JRA55 tile (128; 16…224: 4 waves × 9 variables × cap × 8 B of LDS), or 0:
                                     the LDS-free one-cell-per-lane gather kernel (≤ 56 VGPRs: small enough to run
                                     beside the resident solver workgroups from a second stream)            */
#define CF_OPT_TRIP_HINTS 3       /* order each chunk's cells by the iteration count of the previous call (batches of equal trip
                                   * counts): 0 off, 1 on, 2 (default) automatic = on for the atmosphere–sea-ice solve, whose counts span
                                   * 10…100, off for the ocean solve, where with forcing that evolves from call to call the scattered
                                   * memory access of a sorted batch costs more than the one-step-old order saves (0.085 vs 0.073 ms);
                                   * 3 = as 1, but the round-3 ocean kernel sorts each QUARTER of a chunk's list separately (a batch
                                   * stays within a quarter of the chunk's cell range: 16 instead of 64 lines per access) — measured
                                   * −2 % on the solver alone, +0.5 % on the fused cf_update_state: not the default either          */
#define CF_OPT_AO_CHUNK 4         /* EXPERIMENT option.  Wet cells per workgroup of the flux solver: 0 = automatic (arrival layers of
                                     1024 / 768 / 512 on a surface that fills the device, 256 on a slab that does not), 256 … 1280 = that
                                     size for every workgroup.  Results do not depend on it, bit for bit (tested).               */
#define CF_OPT_FUSED_NET 6        /* cf_update_state computes the cell-local net ocean fluxes in the solver's epilogue and follows
                                   * with a face-stress kernel instead of the three-launch sequence (bitwise the same results):
                                   * 0 never, 1 whenever the configuration allows it (constant ocean albedo), 2 (default) when the
                                   * round-3 ocean kernel runs — its batches are in index order, so the epilogue's nine extra
                                   * accesses per cell are coalesced: update_state 0.107 → 0.096 ms — or CoefficientBasedFluxes
                                   * (fixed trip count: index order too; 0.072 → 0.063 ms); in round 2's trip-sorted kernels
                                   * the same accesses were scattered and cost more than the net-flux kernel they save.        */
#define CF_OPT_MERGED_PREFETCH 9   /* 1: an interpolation requested ahead (cf_prefetch_atmosphere_state, cf_time_steps with pipelining) is
                                   * launched TOGETHER with the current step's face stresses — one kernel on the context's stream whose
                                   * workgroups do one or the other (same arithmetic, same bits) — instead of on the auxiliary stream: a
                                   * step is then two launches (solver; stresses + next interpolation).  Pays where launch boundaries
                                   * dominate (a latitude slab of a strongly scaled run); needs the fused net fluxes and the tiled
                                   * interpolation.  0 (default): auxiliary stream.
                                   * 2: the requested interpolation becomes extra workgroups BEHIND the solver's in the solver launch
                                   * (round-3 ocean kernel and the CoefficientBasedFluxes kernel): they take the slots the solver's
                                   * workgroups free as they retire; with a sea-ice formulation (cf_update_state_sea_ice) the riders
                                   * sit in the interface solve's launch — the longest of the step — and the OCEAN SOLVE is one of
                                   * them: one dispatch order holds its first arrival layer, the interface solve's workgroups, the
                                   * rest of its own and the interpolation's; the face stresses follow as a launch of their own
                                   * (two solver launches on two queues do not overlap on this device; workgroups of one launch do).
                                   * A context in this mode cuts its solver chunks for it (equal chunks per CU where the surface fills
                                   * one dispatch generation, so that workgroups retire staggered): meant for stepping loops that
                                   * request every next state; a lone cf_update_state without a request runs ≈ 5 µs slower on that
                                   * plan than on the default one.  Results are the same bits in every mode — with one aliasing caveat:
                                   * in this mode cf_update_state_sea_ice computes compute_net_sea_ice_fluxes! in the interface solve's
                                   * epilogue with the albedo that solve used; a caller that (a) uses the SeaIceAlbedo(hi, hs, Ts) scheme
                                   * and (b) passes the SAME buffer as cf_sea_ice_state.top_temperature and as the interface
                                   * temperature output gets, from the separate launches of the other modes, an albedo re-evaluated at
                                   * the NEW skin temperature for the net fluxes.                                                    */
#define CF_OPT_ICE_ORBIT_SHORTCUT 7 /* 1 (default): the atmosphere–sea-ice iteration stops as soon as its state repeats the state of two
                                     iterations ago bit for bit — an exact period-2 orbit, where the skin-temperature balance does not
                                     contract — and returns the iterate the remaining steps up to maxiter would end on (the same
                                     bits, tested); 0: iterate to maxiter */
#define CF_OPT_SOLVER_PATH 10      /* how the SimilarityTheoryFluxes fixed point of compute_atmosphere_ocean_fluxes! is reached
                                   * (omip_simulation.jl:42-49):
                                   * CF_SOLVER_PATH_EXACT (0, default): the reference's own iteration — same first guess (1e-4), same
                                   * update order, same stop rule, identical trip counts, results within 7e-12 of the oracle.
                                   * CF_SOLVER_PATH_CERTIFIED (1): the same map in FP64 from a neutral-profile first guess with
                                   * Anderson(2) steps (4–6 evaluations per cell instead of 8–20), and a per-cell CERTIFICATE that
                                   * the fixed point lies within CF_OPT_CERTIFIED_BUDGET of where the reference's stop rule would
                                   * have left its iterate, in the metric |Δ flux| ≤ budget · max(|flux|, floor) with the floors
                                   * 1 W m⁻² (sensible, latent heat), 1e-6 kg m⁻² s⁻¹ (water vapour), 1e-3 N m⁻² (ρτx, ρτy) — and,
                                   * because the net salinity flux J_S = −S (F_v − M_p)/ρ_f can cancel to nothing, the vapour flux also
                                   * within budget · max(|F_v − M_p|, 1e-7 ρ_f / S) of the exact path's (M_p: the interpolated rain + snow),
                                   * which holds J_S of open water to budget · max(|J_S|, 1e-7 m s⁻¹ psu).  The
                                   * bound is the worst case over every last drift the stop rule admits, from the map's Jacobian at
                                   * the fixed point (csrc/coflux_certified.hpp).  Cells that cannot be certified (≈ 2 % at the default
                                   * budget: near-neutral and dead-calm cells, where an absolute drift tolerance leaves the stopped
                                   * iterate loosely determined — half of them — and cells whose evaporation all but cancels their
                                   * precipitation) are solved by the exact path inside the same launch.
                                   * What kind of statement this is: an ESTIMATE with a measured safety factor, not a proof.
                                   * The Jacobian is a two-pair secant estimate in FP32; the bound presumes the linear regime of the map
                                   * (spectral radius of the estimate < 0.6 is required); the safety factor 1.25 is the measured ± 4 %
                                   * accuracy of that estimate (scratch/certified_study.py); and the accepted Anderson-extrapolated state is
                                   * not re-evaluated — "within 2e-8 of the fixed point" rests on the residual at the previous iterate and
                                   * the scheme's measured superlinear convergence.  Measured on the 1/4° and 1/6° surfaces every certified
                                   * cell is within 6e-7 of the exact path at the default budget (tests/test_certified.py holds 1e-6 on
                                   * the full surface); no cell outside the budget has been observed, none is excluded by construction.
                                   * That is why the path is opt-in and why bench.py's `value` is the exact path's.  Decisions are per cell: a result never
                                   * depends on which cells share its wave, chunk or rank.  Applies where the round-3 ocean kernel
                                   * runs in its narrow geometry under the convergence stop rule with tolerance ≥ 1e-9 and maxiter ≥ 40 (cf_solver_iteration_path tells);
                                   * FixedIterations(n), CoefficientBasedFluxes and the sea-ice interface always take the exact path.
                                   * In this mode the optional `iterations` output is a diagnostic: the number of map evaluations of a
                                   * certified cell, or CF_CERTIFIED_EXACT_FLAG | (the reference's trip count) for an exact-path cell;
                                   * the optional friction_velocity / temperature_scale / humidity_scale outputs are the fixed point's. */
#define CF_SOLVER_PATH_EXACT 0
#define CF_SOLVER_PATH_CERTIFIED 1
#define CF_CERTIFIED_EXACT_FLAG 0x100
#define CF_OPT_CERTIFIED_BUDGET 11 /* the certificate's budget in units of 1e-9 (default 800 = 8e-7; 50 … 1000000 — anything above ≈ 900 aims beyond the 1e-6 tolerance and is for measurements).  The solve's own
                                   * convergence error (≈ 2e-8 in the same metric) comes on top: at the default every cell measured so far
                                   * is within 1e-6 of the exact path, the north star's tolerance (worst ≈ 6e-7); see CF_OPT_SOLVER_PATH
                                   * for what the certificate does and does not establish. */
#define CF_OPT_ICE_FREE_CELLS 12   /* what compute_atmosphere_sea_ice_fluxes! does on wet cells that carry no ice (ℵ = 0 AND hᵢ = 0):
                                   * CF_ICE_FREE_ITERATE (0, default): the interface iteration runs on every wet cell, as the recalled
                                   * upstream kernel does — on a 1/4° surface with polar ice 77 % of the interface solve's time;
                                   * CF_ICE_FREE_ZERO (1): such cells get zero_interface_state — zero interface fluxes, zero iterations,
                                   * the skin temperature left at its input — and whole batches of open water skip the solve.
                                   * The five net ocean fields do not read the atmosphere–sea-ice interface, and the net sea-ice
                                   * fluxes of every cell with ℵ > 0 are the same bits in both modes (tested); the interface
                                   * fluxes and the net sea-ice fluxes of ice-free cells differ (they weight nothing: ℵ = 0).  Which of
                                   * the two upstream does is one of the forks julia/oracle_dump.jl records. */
#define CF_ICE_FREE_ITERATE 0
#define CF_OPT_LATENCY_LAYOUT 13   /* which kernels carry the EXACT path of the SimilarityTheoryFluxes ocean solve when a launch leaves every
                                   * SIMD with one or two waves (a latitude slab of a strongly scaled run, a small surface):
                                   * 1 (default, automatic): with the COARE similarity profile (`:corrected`), chunk plans of at most two
                                   * workgroups per CU take the kernels of coflux_solver_slab.hip — the same iteration laid out in big
                                   * basic blocks and re-scheduled for latency after register allocation (csrc/tools/gcn_sched.py):
                                   * 1440×70 steps in 22.0 instead of 24.3 µs; 0: never; 2: always (measurements: with three waves
                                   * per SIMD the layout buys nothing and costs occupancy, and with the plain logarithmic profile the
                                   * slowest waves sit in the per-lane branch to the general ψ at the roughness lengths, which a lone
                                   * wave issues no faster re-ordered).  Results are the same bits in every mode (tests/test_slab_line.py).  Needs gustiness_parameter != 0 (every
                                   * SimilarityTheoryFluxes preset of the reference); other parameter sets keep the production kernels. */
#define CF_ICE_FREE_ZERO 1
#define CF_OPT_HALO_IN_SOLVER_LAUNCH 14 /* 1: cf_time_steps with CF_HALO_PEER hands each step's halo rows to that step's solver launch instead of
                                   * launching the exchange kernel in front of it: 2 × 4 rider workgroups at the head of the launch run the
                                   * same mailbox protocol (one per direction and field), the chunks whose cells read halo rows — the south
                                   * ring row, the last interior row, the north ring row — are dispatched behind every other chunk and wait
                                   * for the riders' counter after their own start phase; interior chunks never wait, and the neighbours'
                                   * latency passes under interior work.  Applies where the step's solver launch is the exact path of the
                                   * round-3 ocean kernel with tail workgroups (CF_OPT_MERGED_PREFETCH = 2 inside a pipelined cf_time_steps);
                                   * any other step gets the exchange kernel as before.  The rows that arrive are the same bits
                                   * (tests/test_halo_in_launch.py: 2 and 4 ranks, lat-lon and tripolar; tests/test_halo_thin_slabs.py: slabs
                                   * of 2 to 8 rows, where no chunk lies between the boundary sets or one chunk is both).  A step's
                                   * request lives from its arming in cf_time_steps to the cf_update_state of the same step and no longer:
                                   * however the call ends, none stays behind for a cf_update_state of the host, and an exchange counts
                                   * (cf_peer_halo_stats, the sequence number its neighbours match) only once its launch is queued.
                                   * 0 (default): the exchange kernel of its
                                   * own.  What it buys on N devices is UNMEASURED: no multi-GPU node has run either form;
                                   * one launch boundary and a 3–5 µs kernel per step are what it removes from a 26 µs slab step.        */
#define CF_OPT_INTERP_TILE_ROWS 15 /* EXPERIMENT option.  Rows of 64 cells per wave tile of the tiled interpolation: 0 (default) = automatic
                                   * by surface size (4 from ≈ 307 k window cells per 256 CUs, 2 from ≈ 154 k, else 1), or 1, 2, 4 = that
                                   * instantiation on any surface — in the interpolation's own launch, the merged stress + interpolation
                                   * launch and the tail workgroups of the solver launches alike.  Results do not depend on it, bit for
                                   * bit (tests/test_weight_atlas.py); cf_debug_interp_grid reports the choice.                          */
#define CF_SOLVER_TABLES 0  /* default: reference iteration path on LDS-tabulated ψ / log / exp.  Accuracy of the tabulated primitives
                               against libm (tests/test_gpu_parity.py::test_device_primitives_accuracy): ψ_m, ψ_h ≤ 5e-12 of
                               max(|ψ|, 1) for |ζ| < 1024 (every state a converging iteration can stop on) and ≤ 2e-10 for
                               1024 ≤ |ζ| ≤ 1e9 (the first one or two iterates from the 1e-4 first guess; extremely stable sea
                               ice); log ≤ 2e-13 absolute; exp for ℓ_q ≤ 6e-10 relative.  Every solver path shares the tables.
                               What that buys in the returned fluxes (all ≥ 100 × inside the 1e-6 target): convergence mode —
                               early-iterate error is contracted away, measured worst 7e-12 scaled, identical trip counts on
                               the 1/4° surface; FixedIterations(n) — a stopped iterate can still sit in the coarse tier, the
                               tests hold 1e-9 on the ocean presets and 1e-8 on the sea-ice interface
                               (test_gpu_parity.py: sea_ice_fixed5), where the skin-temperature balance amplifies. */
#define CF_SOLVER_LIBM 1    /* same iteration on ocml's libm (slow; cross-check)                     */
int cf_set_option(cf_ctx* ctx, int option, int value);
/* *path = CF_SOLVER_PATH_* that cf_compute_atmosphere_ocean_fluxes / cf_update_state would run with the current
 * options and flux parameters (the certified path falls back to the exact one where it does not apply) — the predicate
 * the launch itself decides on.  One launch runs the exact iteration whatever this answers: cf_update_state_sea_ice with
 * CF_OPT_MERGED_PREFETCH = 2 carries the ocean solve in the interface solve's launch, whose rider is the exact kernel.   */
int cf_solver_iteration_path(cf_ctx* ctx, int* path);
/* *layout = 1 when the ocean solve's EXACT path would be carried by the kernels laid out for one or two waves per SIMD
 * (CF_OPT_LATENCY_LAYOUT; coflux_solver_slab.hip) with the current options, flux parameters and the chunk table as built
 * (cf_ensure_chunk_table first: the automatic mode looks at its workgroup count), else 0.  A measurement aid.         */
int cf_solver_latency_layout(cf_ctx* ctx, int* layout);
/* Self-test hook: y[k] = f(x[k]) with the device primitives the solver uses
 * (f: 0 log, 1 exp, 2 cbrt, 3 sqrt, 4 1/x, 5 ψ_m(ζ), 6 ψ_h(ζ)); d_x, d_y device pointers.        */
int cf_debug_eval(cf_ctx* ctx, int function, int n, const double* d_x, double* d_y);
/* Self-test hook (host arithmetic only, works without a GPU): the solver's chunk plan for a surface of total
 * cost `total_cost` (wet cell = the returned cost unit, land cell = 1) on `cu_count` compute units.
 * out[0] = number of rounds, then per round (wet cells per chunk, number of chunks).  Returns the wet-cell cost
 * unit, or −1 if `capacity` ints are too few. */
int cf_debug_chunk_plan(long long total_cost, int cu_count, int forced_wet_per_chunk, int* out, int capacity);
/* Self-test hook: the chunk table as the device built it for the context's current mask (cf_ensure_chunk_table first).
 * Synchronises the context's stream.  begins[0..n] = first window cell (row-major over the ring-inclusive window) of
 * every chunk, closed by the cell count; wet_counts[0..n-1] = wet cells listed per chunk; *n_chunks = n is always set;
 * *lists_valid = 1 when the static wet lists are in use (0: some chunk overflowed its list and every workgroup classifies
 * its range per call).  Returns CF_ERR_INVALID when no table is valid or `capacity` < n + 1 ints per array (*n_chunks is
 * still set then: retry with n + 1).  Changes no state. */
int cf_debug_chunk_table(cf_ctx* ctx, int* begins, int* wet_counts, int capacity, int* n_chunks, int* lists_valid);
/* Self-test hook (host bookkeeping only, launches nothing, changes no state): *launches = how many ocean-solver launches of the
 * context's LAST cf_time_steps call were told to write the land zeros (CF_OPT_LAND_ZEROS): 1 of n ≥ 1 steps under the
 * automatic mode, n under 0, 0 under 2 or before any call. */
int cf_debug_land_zero_launches(cf_ctx* ctx, int* launches);
/* Self-test hook (host arithmetic only, launches nothing, changes no state): the shape of the tiled interpolation on the
 * context's grid under its current options, wherever it runs (its own launch, the merged stress + interpolation launch, the
 * tail workgroups of a solver launch): *rows = rows of 64 cells per wave tile (1, 2 or 4: automatic by surface size and the
 * device's CU count, or what CF_OPT_INTERP_TILE_ROWS forces), *blocks = workgroups of four waves. */
int cf_debug_interp_grid(cf_ctx* ctx, int* rows, int* blocks);
int cf_sync(cf_ctx* ctx);

/* Device memory for callers that cannot own HIP memory themselves (Julia without AMDGPU.jl). */
void* cf_device_alloc(cf_ctx* ctx, size_t bytes);
int cf_device_free(cf_ctx* ctx, void* d_ptr);
int cf_h2d(cf_ctx* ctx, void* d_dst, const void* h_src, size_t bytes);
int cf_d2h(cf_ctx* ctx, void* h_dst, const void* d_src, size_t bytes);

/* ------------------------------------------------------------------------------------------
 * The hot path — one entry per reference function of SURVEY.md §3.1
 * ---------------------------------------------------------------------------------------- */

/* interpolate_atmosphere_state!(interfaces, atmosphere::JRA55PrescribedAtmosphere, model)
 * (construction site atmosphere.jl:20-29, README.md:74): bilinear in (λ,φ) × linear in time,
 * rain+snow summed, winds rotated to the grid frame.                                           */
/* Footprint: reads the whole source window, fi / fj at the window's columns / rows (separable) or cells, cos/sin_rot on the
 * window W (ring window); writes the eight exchange fields on W only.                                                   */
int cf_interpolate_atmosphere_state(cf_ctx* ctx, const cf_atmos_source* src,
                                    const cf_interp_weights* w, const cf_exchange_fields* out);

/* compute_atmosphere_ocean_fluxes!(coupled_model) with SimilarityTheoryFluxes
 * (omip_simulation.jl:42-49; README.md:75): the per-cell Monin–Obukhov fixed point.            */
/* Footprint: reads atmosphere u, v, T, p, q (the certified path also Mp) and ocean T, S, mask on W, ocean u also at
 * i + 1 and v also at j + 1; writes every flux output and `iterations` on W, land cells included, nothing else.       */
int cf_compute_atmosphere_ocean_fluxes(cf_ctx* ctx, const cf_ocean_surface* ocean,
                                       const cf_exchange_fields* atmos,
                                       const cf_interface_fluxes* out);

/* compute_net_ocean_fluxes!(coupled_model): radiation (atmosphere.jl:41-44) + (1−ℵ) partition +
 * unit conversion → τx, τy, JT, JS (omip_diagnostics.jl:77-80).                                 */
/* Footprint: interior I only.  Reads S, mask, the cell-local fluxes, Qs, Ql, Mp, the ice fields and latitude at the cell,
 * ρτx and ℵ also at i − 1, ρτy and ℵ also at j − 1 (ocean T, u, v and atmosphere u, v, T, p, q must be non-NULL but are
 * not read); writes the net fields on I, land included.  With ring = 0 the flux halo column i = −1 and row j = −1 are
 * not computed by anyone: the caller fills them (zeros, or a halo exchange) before the face stresses read them.       */
int cf_compute_net_ocean_fluxes(cf_ctx* ctx, const cf_ocean_surface* ocean,
                                const cf_exchange_fields* atmos,
                                const cf_interface_fluxes* fluxes,
                                const cf_sea_ice_fields* ice /* may be NULL */,
                                const cf_interp_weights* w /* latitude only; may be NULL */,
                                const cf_net_ocean_fluxes* out);

/* update_state!(coupled_model) (NEMOTKE/nemo_tke_compute_closure_fields.jl:7-8): the three
 * stages above back to back on the context's stream (three launches, no host synchronisation).  */
/* Footprint: the union of the three: writes exchange and flux fields on W, net fields on I (every option of
 * CF_OPT_FUSED_NET / _MERGED_PREFETCH / _LATENCY_LAYOUT / _SOLVER_PATH alike; cf_time_steps likewise, per step).      */
int cf_update_state(cf_ctx* ctx, const cf_atmos_source* src, const cf_interp_weights* w,
                    const cf_ocean_surface* ocean, const cf_exchange_fields* atmos,
                    const cf_interface_fluxes* fluxes, const cf_sea_ice_fields* ice,
                    const cf_net_ocean_fluxes* net);

/* ------------------------------------------------------------------------------------------
 * JRA55 snapshot window in HBM: JRA55PrescribedAtmosphere(arch; time_indices_in_memory = n,
 * prefetch = true) of atmosphere.jl:20-29 / launch.sh:86-93 — `n_slots` 3-hourly snapshots of the nine
 * variables resident on the device, refilled from host memory while the model steps.  `time_index` is the
 * monotone snapshot COUNTER ⌊t/Δt⌋ (not the index inside a repeat-year record, which jumps back at the wrap and
 * would put two consecutive snapshots into one slot); snapshot counter t lives in slot t mod n_slots.  Uploads run on the window's own copy stream out of pinned staging buffers and are
 * ordered against the context's compute stream with events in both directions: a slot is not overwritten
 * before the interpolations already queued have read it, and an interpolation does not start before the two
 * snapshots it brackets have landed.  Reading the files (NetCDF) stays on the host side of this boundary.
 * A window outlived by its context may still be destroyed, and cf_window_find / cf_window_host_buffer still answer
 * (cf_window_wait_slot, _commit, _upload and _source on it fail with CF_ERR_INVALID).
 * ---------------------------------------------------------------------------------------- */
typedef struct cf_window cf_window;
int cf_window_create(cf_ctx* ctx, int32_t ns_x, int32_t ns_y, int32_t n_slots, cf_window** out);
int cf_window_destroy(cf_window* w);
/* Pinned staging buffer [ns_y][ns_x] of (slot, variable) for readers that fill it in place.  Call
 * cf_window_wait_slot first: the previous upload out of this buffer may still be in flight. */
float* cf_window_host_buffer(cf_window* w, int32_t slot, int32_t variable);
int cf_window_wait_slot(cf_window* w, int32_t slot);
/* The slot's nine staging buffers hold snapshot `time_index`: start its asynchronous copy into HBM. */
int cf_window_commit(cf_window* w, int32_t slot, int64_t time_index);
/* Convenience: copy nine host arrays (CF_JRA55_* order) into slot time_index mod n_slots and commit. */
int cf_window_upload(cf_window* w, int64_t time_index, const float* const* host_vars);
/* Slot that holds (or is receiving) snapshot `time_index`, or -1. */
int cf_window_find(cf_window* w, int64_t time_index);
/* Source descriptor for interpolating between snapshots n1 and n2 (both must be in the window; the compute
 * stream is made to wait for their uploads).  Pass it to cf_interpolate_atmosphere_state / cf_update_state. */
int cf_window_source(cf_window* w, int64_t n1, int64_t n2, double time_fraction, cf_atmos_source* out);

/* ------------------------------------------------------------------------------------------
 * Atmosphere–sea-ice interface (config sites omip_simulation.jl:62-69 ":corrected",
 * :105-113 ":ncar", atmosphere.jl:34-44).  Same Monin–Obukhov iteration, but the interface temperature is
 * a skin temperature found inside the loop from the surface energy balance against the conductive flux
 * through the ice (SkinTemperature(ConductiveFlux)), humidity saturates over ice, latent heat is that of
 * sublimation.  The ice state itself (ClimaSeaIce) is prescribed input.
 * ---------------------------------------------------------------------------------------- */
/* flux_balance_temperature(SkinTemperature(ConductiveFlux)) inside the iteration ([UPSTREAM-RECALL]; the pin of
 * julia/oracle_dump.jl will tell which one upstream ships):
 *   EXPLICIT       T★ = Tᵢ − (h/k)(Q_v + Q_c + Q_d + εσTₛ⁴) with every flux at the previous iterate; its gain
 *                  (h/k)·∂Q/∂T exceeds 1 for ice thicker than ≈ 0.1–0.2 m in wind, where it orbits under the ±ΔT_max
 *                  limiter until maxiter;
 *   SEMI_IMPLICIT  the upwelling longwave linearised about the previous skin temperature,
 *                  T★ = (Tᵢ − (h/k)(Q_v + Q_c + Q_d)) / (1 + (h/k) εσ Tₛ³)  — the damped form;
 *   LINEARISED     one Newton step on the whole balance per iteration: all four terms linearised about the previous Tₛ,
 *                  with the previous iterate's u★ and transfer coefficients held fixed,
 *                    Q(Tₛ)  = −ρ u★ (ℒ_s q★ + c_p θ★) + Q_d + εσTₛ⁴                       (what EXPLICIT computes)
 *                    Q'(Tₛ) = 4εσTₛ³ + ρ c_p u★ χ_θ + ρ ℒ_s u★ χ_q · dq_s/dT(Tₛ)
 *                    χ_θ = κ/D_θ, χ_q = κ/D_q   (profile factors of the previous similarity step; 0 before the first)
 *                    dq_s/dT = q_s(Tₛ) ((a_i − 1)/Tₛ + b_i/Tₛ²), a_i = (c_pv − c_pi)/R_v, b_i = (ℒ_s0 − (c_pv − c_pi) T_0)/R_v
 *                    T★ = (Tᵢ − (h/k)(Q(Tₛ) − Q'(Tₛ) Tₛ)) / (1 + (h/k) Q'(Tₛ)),   h = h_eff;
 *                  it contracts where EXPLICIT orbits (the turbulent feedback (h/k) ρ c_p C_h U ≈ 10 on metre-thick ice in
 *                  wind).  A fixed point of it is a fixed point of EXPLICIT.
 * Every scheme then applies the NaN guard, the ±ΔT_max limiter and the cap at the melting point before the similarity step;
 * the stop rule, the initial scales and maxiter are the same.                                                             */
#define CF_SKIN_EXPLICIT 0
#define CF_SKIN_SEMI_IMPLICIT 1
#define CF_SKIN_LINEARISED 2
typedef struct cf_sea_ice_params {
    int32_t struct_size;                   /* sizeof(cf_sea_ice_params) */
    int32_t skin_temperature_scheme;       /* CF_SKIN_* */
    double conductivity;                   /* 2.0 W m⁻¹ K⁻¹  (ClimaSeaIce ConductiveFlux)          */
    double consolidation_thickness;        /* 0.05 m: thinner ice conducts as if this thick          */
    double maximum_temperature_change;     /* 5 K per iteration (SkinTemperature limiter)            */
    double ice_salinity;                   /* reserved (the skin is capped at the FRESHWATER melting point) */
    double liquidus_slope;                 /* 0.054 K per g/kg: ice bottom at T_fw − m·S_ocean           */
    double freshwater_melting_temperature; /* 273.15 K                                               */
    double albedo;                         /* 0.7 unless cf_sea_ice_state.albedo is given            */
    double emissivity;                     /* 1.0, SurfaceRadiationProperties(sea_ice_albedo, 1.0), atmosphere.jl:44 */
    double temperature_offset;             /* 273.15: top_surface_temperature is in °C, atmosphere.jl:38 */
} cf_sea_ice_params;

int cf_default_sea_ice_params(cf_sea_ice_params* p);

/* sea_ice.model.{ice_concentration, ice_thickness, ice_thermodynamics.top_surface_temperature, velocities}
 * (atmosphere.jl:34-39, src/ClimaOcean.jl:62-63); all at cell centres, ocean-grid layout. */
typedef struct cf_sea_ice_state {
    const double* concentration;    /* ℵ                                                             */
    const double* thickness;        /* hᵢ [m]                                                        */
    const double* top_temperature;  /* previous skin temperature [°C]: initial guess of the iteration.  May be the very buffer
                                       cf_compute_atmosphere_sea_ice_fluxes writes the new one to (out->temperature): every
                                       cell reads its guess before it writes its result — the in-place update of
                                       sea_ice.model.ice_thermodynamics.top_surface_temperature in a coupled run          */
    const double* u;                /* ice velocity [m/s] or NULL (⇒ 0)                              */
    const double* v;
    const double* albedo;           /* per-cell albedo or NULL: then cf_set_sea_ice_albedo's scheme, else the constant */
    const double* snow_thickness;   /* hₛ [m] (sea_ice.model.snow_thickness, atmosphere.jl:34) or NULL (⇒ 0): read by the
                                       CCSM3 albedo only                                                            */
} cf_sea_ice_state;

/* SeaIceAlbedo(hi, hs, Ts) — the CCSM3 sea-ice albedo the reference hands to SurfaceRadiationProperties
 * (atmosphere.jl:30-44; "reads live model fields").  The scheme itself lives in NumericalEarth; restated from its
 * source, Briegleb et al. 2004 (NCAR/TN-463) as implemented in CICE's `ccsm3` option: thickness-dependent bare-ice
 * albedo  α_ice = α_cold·f_h + α_ocean·(1 − f_h),  f_h = min(atan(4 hᵢ)/atan(4 h_max), 1);  both ice and snow darken
 * linearly over the last ΔT_melt below the melting point;  snow covers the fraction hₛ/(hₛ + h_patch);  the two
 * spectral bands are averaged with `visible_fraction` (JRA55 carries one broadband rsds).                          */
typedef struct cf_sea_ice_albedo_params {
    int32_t struct_size;
    int32_t reserved;
    double ice_visible, ice_near_infrared;     /* 0.78, 0.36  cold, thick, bare ice                       */
    double snow_visible, snow_near_infrared;   /* 0.98, 0.70  cold snow                                   */
    double ocean_albedo;                       /* 0.06        limit of vanishing thickness                */
    double reference_thickness;                /* 0.3 m       h_max                                       */
    double melt_temperature_range;             /* 1 K         ΔT_melt                                     */
    double ice_melt_change;                    /* 0.075       darkening of ice at the melting point       */
    double snow_melt_change_visible;           /* 0.10                                                    */
    double snow_melt_change_near_infrared;     /* 0.15                                                    */
    double snow_patch_thickness;               /* 0.02 m                                                  */
    double visible_fraction;                   /* 0.5         weight of the visible band in the broadband albedo [UNVERIFIED] */
    double melting_temperature;                /* 0 °C        in the units of top_temperature             */
} cf_sea_ice_albedo_params;
int cf_default_sea_ice_albedo_params(cf_sea_ice_albedo_params* p);
/* Switch the atmosphere–sea-ice interface and the net sea-ice fluxes to this scheme wherever cf_sea_ice_state.albedo
 * is NULL (params = NULL: back to the constant albedo of cf_sea_ice_params).                                       */
int cf_set_sea_ice_albedo(cf_ctx* ctx, const cf_sea_ice_albedo_params* params);
/* The albedo field on its own (diagnostics, tests): d_albedo[k] = SeaIceAlbedo(hᵢ, hₛ, Tₛ) for every ocean-grid cell. */
/* Footprint: reads and writes every cell of the parent arrays, halos included.                                      */
int cf_compute_sea_ice_albedo(cf_ctx* ctx, const cf_sea_ice_albedo_params* params, const double* d_ice_thickness,
                              const double* d_snow_thickness /* may be NULL */, const double* d_top_temperature,
                              double* d_albedo);

/* compute_sea_ice_ocean_fluxes!(coupled_model) with ThreeEquationHeatFlux(; friction_velocity =
 * MomentumBasedFrictionVelocity()) (omip_simulation.jl:71-77: "three-equation ice-ocean heat flux with momentum-based
 * friction velocity computed from actual ice-ocean stress, McPhee 1992, 2008") and frazil formation.  Per wet cell:
 *   u★   = max(√|τ_io|, u★_min),  τ_io the kinematic ice–ocean stress averaged from its faces to the cell centre:
 *           cell (i, j) reads x_stress[i], x_stress[i+1], y_stress[j], y_stress[j+1], so the two stress fields need
 *           their EAST x-halo column and NORTH halo row filled (periodic / slab exchange / tripolar fold) by whoever
 *           produces them — cf_time_steps and the halo entry points only move T, S, u, v;
 *   frazil: T_o < T_f(S_o) = −m S_o  ⇒  Q_frazil = ρ_o c_o Δz (T_o − T_f)/Δt (< 0: heat the ice model must supply by
 *           freezing), and the exchange below sees T_o = T_f;
 *   three equations (Holland & Jenkins 1999; McPhee et al. 2008) for the interface (T_b, S_b) and melt rate w:
 *           ρ_o c_o α_h u★ (T_o − T_b) = ρ_i ℒ w,   ρ_o α_s u★ (S_o − S_b) = ρ_i w (S_b − S_i),   T_b = −m S_b
 *           ⇒ a quadratic in S_b that does not depend on u★;
 *   Q_io = ℵ ρ_o c_o α_h u★ (T_o − T_b)  [W m⁻², positive = the ocean loses heat],
 *   Jˢ_io = ℵ α_s u★ (S_o − S_b)         [g/kg m s⁻¹, positive = the ocean loses salt (melt water dilutes it)].
 * The outputs are exactly the fields cf_sea_ice_fields.interface_heat / salt_flux and cf_compute_net_sea_ice_fluxes'
 * frazil_heat / interface_heat take.  Coefficients marked UNVERIFIED are the recalled ClimaSeaIce defaults.          */
typedef struct cf_ice_ocean_params {
    int32_t struct_size;
    int32_t reserved;
    double heat_transfer_coefficient;   /* α_h = 0.0095 [UNVERIFIED]                                   */
    double salt_transfer_coefficient;   /* α_s = α_h / 35 [UNVERIFIED]                                  */
    double minimum_friction_velocity;   /* 0 m/s                                                        */
    double ice_density;                 /* 917 kg m⁻³                                                   */
    double latent_heat_of_fusion;       /* 334 000 J kg⁻¹                                               */
    double ice_salinity;                /* 4 g/kg                                                       */
    double liquidus_slope;              /* m = 0.054 K per g/kg: T_f = −m S in °C, i.e. freshwater melts at 0 °C = the 273.15 K of
                                           cf_sea_ice_params.freshwater_melting_temperature (the two interfaces agree at the default) */
    double top_cell_thickness;          /* Δz of the ocean's top cell [m] (frazil)                      */
    double time_step;                   /* Δt [s] (frazil); ≤ 0 disables frazil                         */
} cf_ice_ocean_params;
int cf_default_ice_ocean_params(cf_ice_ocean_params* p);
typedef struct cf_ice_ocean_fluxes {
    double* interface_heat;   /* Q_io                                             */
    double* salt_flux;        /* Jˢ_io                                            */
    double* frazil_heat;      /* Q_frazil (may be NULL)                           */
    double* friction_velocity;/* u★ (optional diagnostic, may be NULL)           */
} cf_ice_ocean_fluxes;
/* Footprint: reads T, S, mask, ℵ on I, x_stress also at i + 1, y_stress also at j + 1; writes its outputs on I only.   */
int cf_compute_sea_ice_ocean_fluxes(cf_ctx* ctx, const cf_ice_ocean_params* params, const cf_ocean_surface* ocean,
                                    const double* d_concentration, const double* d_x_stress /* u-faces, kinematic */,
                                    const double* d_y_stress /* v-faces */, const cf_ice_ocean_fluxes* out);

/* `ice_fluxes` = the atmosphere_sea_ice_fluxes formulation (e.g. corrected_atmosphere_sea_ice_fluxes). */
int cf_set_sea_ice_formulation(cf_ctx* ctx, const cf_flux_params* ice_fluxes, const cf_sea_ice_params* ice);
/* compute_atmosphere_sea_ice_fluxes!(coupled_model): out.temperature receives the new skin temperature
 * [°C]; latent_heat uses the sublimation enthalpy.  Needs exchange fields Qs, Ql as well. */
/* Footprint: reads atmosphere u, v, T, p, q, Qs, Ql, the ice state and ocean S, mask on W; writes the interface fluxes and
 * `iterations` on W; a top_temperature that is out->temperature keeps its input bits outside W.                        */
int cf_compute_atmosphere_sea_ice_fluxes(cf_ctx* ctx, const cf_sea_ice_state* ice, const cf_ocean_surface* ocean,
                                         const cf_exchange_fields* atmos, const cf_interface_fluxes* out);

/* compute_net_sea_ice_fluxes!(coupled_model): the heat the sea-ice thermodynamics receives at its two faces,
 *   ΣQt = (Q_d + Q_u + Q_c + Q_v)·[ℵ > 0],  Q_u = εσT_s⁴ at the skin temperature just computed,
 *                                            Q_d = −(1 − α)Q_s − εQ_ℓ   (positive upward, W m⁻²),
 *   ΣQb = Q_frazil + Q_interface             (the ice–ocean exchange, taken as given: SURVEY §8f),
 * zero on land.  `ai_fluxes` is the output of cf_compute_atmosphere_sea_ice_fluxes; radiative properties are
 * those of cf_set_sea_ice_formulation.  frazil_heat / interface_heat may be NULL (⇒ 0).                  */
typedef struct cf_net_sea_ice_fluxes {
    double* top_heat;     /* ΣQt */
    double* bottom_heat;  /* ΣQb */
} cf_net_sea_ice_fluxes;
/* Footprint: reads its inputs and writes top_heat / bottom_heat on I only.                                            */
int cf_compute_net_sea_ice_fluxes(cf_ctx* ctx, const cf_sea_ice_state* ice, const cf_ocean_surface* ocean,
                                  const cf_exchange_fields* atmos, const cf_interface_fluxes* ai_fluxes,
                                  const double* frazil_heat, const double* interface_heat,
                                  const cf_net_sea_ice_fluxes* out);

/* update_state!(coupled_model) of a model WITH sea ice (BASELINE config 3; omip_simulation.jl:139-163): cf_update_state
 * followed by cf_compute_atmosphere_sea_ice_fluxes and cf_compute_net_sea_ice_fluxes on the same stream — five
 * launches, no host synchronisation.  `ice_partition` (ℵ, ice–ocean fluxes) feeds the ocean partition, `ice_state`
 * the interface solve; `ai_fluxes->temperature` receives the new skin temperature. */
/* Footprint: cf_update_state's, then the interface solve's (W) and the net sea-ice fluxes' (I).                         */
int cf_update_state_sea_ice(cf_ctx* ctx, const cf_atmos_source* src, const cf_interp_weights* w,
                            const cf_ocean_surface* ocean, const cf_exchange_fields* atmos,
                            const cf_interface_fluxes* ao_fluxes, const cf_sea_ice_fields* ice_partition,
                            const cf_net_ocean_fluxes* net, const cf_sea_ice_state* ice_state,
                            const cf_interface_fluxes* ai_fluxes, const double* frazil_heat,
                            const double* interface_heat, const cf_net_sea_ice_fluxes* net_ice);

/* ------------------------------------------------------------------------------------------
 * JRA55PrescribedLand(arch; …) (atmosphere.jl:46): river discharge `friver` and iceberg calving `licalvf`
 * (jra55_data_staging.jl:8), kg m⁻² s⁻¹ on the JRA55 grid, the last two of the eleven staged variables.  Same window
 * layout, same bilinear × linear-in-time interpolation as the atmosphere; the two are summed into ONE ocean-grid field.
 * cf_set_land_freshwater hands that field to compute_net_ocean_fluxes!: the freshwater reaches the ocean as
 *     JS += −Sₒ · (−M_land / ρ_f)      (not scaled by 1 − ℵ: rivers run under ice; the minimum-salinity guard applies)
 * [UPSTREAM-RECALL: NumericalEarth adds the land freshwater flux to the ocean's freshwater budget; the line above is
 * this library's statement of it, both oracles restate the same].  NULL switches it off.                          */
typedef struct cf_land_source {
    const float* friver;    /* device, [n_levels][ns_y][ns_x] */
    const float* licalvf;   /* device, may be NULL */
    int32_t ns_x, ns_y, n_levels, level1, level2, reserved;
    double time_fraction;
} cf_land_source;
/* Footprint (cf_interpolate_land_freshwater): reads both sources in full and fi / fj as the atmosphere does; writes d_out on W. */
int cf_interpolate_land_freshwater(cf_ctx* ctx, const cf_land_source* src, const cf_interp_weights* w, double* d_out);
int cf_set_land_freshwater(cf_ctx* ctx, const double* d_land_freshwater /* ocean-grid field, kg m⁻² s⁻¹, or NULL */);

/* SurfaceFluxRestoring(DatasetRestoring(…; rate = piston_velocity / (Δz days))) riding on the salinity top boundary
 * condition as the `additional_fluxes` of MultipleFluxes{flux_field, additional_fluxes} (omip_simulation.jl:175-206,
 * 507-523): `_materialize_top_flux!` evaluates it into a 2-D buffer, J_add = v_p (Sₒ − S★) on wet cells (positive = salt
 * leaves where the surface is saltier than the target).  The buffer is what cf_normalize_salinity_flux takes as
 * d_additional; the ocean applies flux_field + additional.                                                      */
/* Footprint: reads S★, S, mask on I; writes d_buffer on I only (0 on land).                                           */
int cf_materialize_salinity_restoring(cf_ctx* ctx, double piston_velocity /* m/s */, const double* d_target_salinity,
                                      const cf_ocean_surface* ocean, double* d_buffer);

/* NormalizeSalinity callback (src/OMIPConfigurations/omip_simulation.jl:182-220, added at :385-388):
 * subtract the global, area-weighted mean over wet cells of (salinity flux [+ additional flux]) from
 * the salinity-flux field — `compute!(mean_total); parent(flux_field) .-= mean_total`, so the constant
 * is subtracted from the whole parent array, halos and land included.  `d_area` are the horizontal cell
 * areas Az in ocean-grid layout (NULL ⇒ uniform); `d_additional` is the materialised additional top
 * flux (SurfaceFluxRestoring …) or NULL.  With an initialised communicator (cf_comm_init) the two sums
 * are all-reduced over the ranks (one RCCL all-reduce of two doubles) so that every slab subtracts the
 * same global mean.  The mean is also written to d_mean_out (device double, may be NULL).            */
/* Footprint: reads flux, additional, area, mask on I; writes EVERY cell of d_flux (halos: input − mean) and *d_mean_out. */
int cf_normalize_salinity_flux(cf_ctx* ctx, double* d_flux, const double* d_additional, const double* d_area,
                               const void* d_mask, double* d_mean_out);

/* NormalizeSalinity whose mean does not depend on how the globe is cut into slabs.  cf_normalize_salinity_flux adds in an order
 * that is a function of the slab (grid-stride partial sums of nx · ny cells), so R ranks cannot give the bits of one domain — and
 * the mean is subtracted from every cell.  Here both sums are EXACT: for every wet interior cell, with no fused multiply-add,
 *     v = fl(flux + additional)   (flux alone when d_additional is NULL),   a = area (1.0 when d_area is NULL),   t = fl(v · a),
 *     S_J = Σ t   and   S_A = Σ a   exactly,   sums = (fl(S_J), fl(S_A)) rounded once to nearest-even,
 * then, as in cf_normalize_salinity_flux, mean = sums[1] > 0 ? sums[0] / sums[1] : 0 is subtracted from every cell of the parent
 * array and written to *d_mean_out.  A sum is kept as 67 signed 64-bit digits, digit k of weight 2^(32k − 1088); a term adds one
 * 32-bit piece to each of three adjacent digits with integer atomics, so the digits depend on no order, workgroup or rank
 * (csrc/coflux_exact_sum.hpp holds the format and the rounding; it builds without HIP).  A zero sum is +0.0; beyond the largest
 * double the sum is ±Inf; with a NaN term or both infinities among the terms it is NaN, with one infinity that infinity.  Land
 * and halo cells are selected away and never multiplied: they may hold NaN.  At most 2³¹ terms over all ranks.
 * With a reduction world connected on more than one rank (cf_peer_reduce_connect) the digits of all ranks are added before the
 * rounding: every rank subtracts the bits of the single domain's mean.  The bits of this form differ from
 * cf_normalize_salinity_flux's, which keeps its order and its bits.                                                          */
/* Footprint: cf_normalize_salinity_flux's.                                                                                    */
int cf_normalize_salinity_flux_exact(cf_ctx* ctx, double* d_flux, const double* d_additional, const double* d_area,
                                     const void* d_mask, double* d_mean_out);
/* A test aid, in the family of cf_debug_chunk_table: THIS RANK's two exact sums of cf_normalize_salinity_flux_exact (no
 * reduction is issued, whatever is connected) and how many terms of S_J were NaN, +Inf, −Inf.  Synchronises the context's stream
 * and answers on the host; writes nothing to d_flux.                                                                          */
int cf_debug_salinity_sums_exact(cf_ctx* ctx, const double* d_flux, const double* d_additional, const double* d_area,
                                 const void* d_mask, double sums_out[2], unsigned long long nonfinite_out[3]);

/* The preamble of a coupled step (omip_simulation.jl:123-163, :507-523): what cf_interpolate_land_freshwater,
 * cf_compute_sea_ice_ocean_fluxes and cf_materialize_salinity_restoring do in front of cf_update_state_sea_ice, as ONE
 * launch (one thread per cell of W; the two interior jobs share one read of S and of the mask).  Every array the call
 * writes holds, on every cell of its parent array, the bits those three entry points leave when called in that order: the
 * per-cell arithmetic is theirs.  A job is absent when its output is NULL:
 *   land_freshwater                    NULL ⇒ no land job (`land` and `weights` are not read),
 *   ice_ocean_fluxes.interface_heat    NULL ⇒ no ice–ocean job (`ice_ocean`, `concentration`, the stresses, ocean.T are not read),
 *   restoring_buffer                   NULL ⇒ no restoring job (`piston_velocity`, `target_salinity` are not read);
 * with every job absent nothing is launched.  The arguments of a present job are checked as its own entry point checks them. */
typedef struct cf_coupled_prepare {
    int32_t struct_size;                  /* sizeof(cf_coupled_prepare) */
    int32_t reserved;
    cf_ocean_surface ocean;               /* S and mask: both interior jobs; T: the ice–ocean job; u, v are not read */
    cf_interp_weights weights;            /* the land job's map (separable or 2-D), as cf_interpolate_land_freshwater takes it */
    cf_land_source land;                  /* friver [+ licalvf], the two levels and the fraction */
    double* land_freshwater;              /* M_land on W */
    cf_ice_ocean_params ice_ocean;
    const double* concentration;          /* ℵ (NULL ⇒ 0) */
    const double* x_stress;               /* kinematic ice–ocean stress at u-faces / v-faces (NULL ⇒ 0): read at i + 1 / j + 1 too */
    const double* y_stress;
    cf_ice_ocean_fluxes ice_ocean_fluxes; /* Q_io, Jˢ_io on I; frazil_heat, friction_velocity may be NULL */
    double piston_velocity;               /* v_p, m/s */
    const double* target_salinity;        /* S★ */
    double* restoring_buffer;             /* J_add = v_p (Sₒ − S★) on I (0 on land) */
} cf_coupled_prepare;
/* Footprint: the union of the three entry points' — reads both land sources in full and fi / fj as the atmosphere does, writes
 * land_freshwater on W; reads T, S, mask, ℵ, S★ on I, x_stress also at i + 1, y_stress also at j + 1; writes the ice–ocean
 * outputs and restoring_buffer on I only (0 on land).  Nothing else is read or written.                                     */
int cf_prepare_coupled_step(cf_ctx* ctx, const cf_coupled_prepare* prepare);

/* ------------------------------------------------------------------------------------------
 * Measurement helper: run `launches` back-to-back launches of one stage on the context's stream
 * bracketed by HIP events ON THAT STREAM and return the average milliseconds per launch.
 * stage: 0 = interpolate, 1 = atmosphere–ocean fluxes, 2 = net ocean fluxes, 3 = update_state.  */
#define CF_STAGE_INTERPOLATE 0
#define CF_STAGE_AO_FLUXES 1
#define CF_STAGE_NET_FLUXES 2
#define CF_STAGE_UPDATE_STATE 3
#define CF_STAGE_COPY 4 /* device copy of `bytes` (calibrates the HBM denominator) */
int cf_time_stage(cf_ctx* ctx, int stage, int launches, const cf_atmos_source* src,
                  const cf_interp_weights* w, const cf_ocean_surface* ocean,
                  const cf_exchange_fields* atmos, const cf_interface_fluxes* fluxes,
                  const cf_sea_ice_fields* ice, const cf_net_ocean_fluxes* net,
                  double* ms_per_launch);
int cf_time_copy(cf_ctx* ctx, void* d_dst, const void* d_src, size_t bytes, int launches,
                 double* ms_per_launch);
/* Per-kernel timing INSIDE a caller's timed region: while enabled, cf_update_state brackets each of
 * its kernels with HIP events on the launch stream (no host sync).  cf_profile_read synchronises and
 * returns the average duration of `kernel` over the recorded steps.  cf_profile_enable(ctx, n)
 * (re)arms the recorder for n records; 0 disables.                                                 */
#define CF_KERNEL_INTERPOLATE 0
#define CF_KERNEL_AO_FLUXES 1
#define CF_KERNEL_NET_FLUXES 2
int cf_profile_enable(cf_ctx* ctx, int max_records);
int cf_profile_read(cf_ctx* ctx, int kernel, double* avg_ms, int* records);

/* ------------------------------------------------------------------------------------------
 * Multi-GPU: latitude-slab halo rows over RCCL (Partition(1,4) launch.sh:165,
 * Partition(1,8) pbs_launch.sh:51).  The unique id is produced on rank 0 and distributed by the
 * host (MPI.jl bcast in Julia; torch.distributed in the Python mirror).
 * ---------------------------------------------------------------------------------------- */
#define CF_COMM_ID_BYTES 128
int cf_comm_unique_id(void* id128);
int cf_comm_init(cf_ctx* ctx, const void* id128, int rank, int nranks);
int cf_comm_destroy(cf_ctx* ctx);
/* RCCL's own view of the communicator cf_comm_init made: the number of ranks it connected (ncclCommCount), this rank's index
 * (ncclCommUserRank) and the HIP device it sits on (ncclCommCuDevice); any of the three may be NULL.  What a launcher
 * prints beside its own WORLD_SIZE so that a run whose ranks never met shows (bench.py: config.rccl_comm_ranks).       */
int cf_comm_count(cf_ctx* ctx, int* nranks, int* rank, int* device);
/* Exchange `rows` boundary rows of `nfields` ocean-grid arrays with the south (rank−1) and north
 * (rank+1) neighbours: my first/last interior rows → their north/south halos.  With ring = 1 the kernels
 * also compute the ring row j = ny, whose cell-centre v needs the y-face at j = ny + 1: exchange
 * rows = ring + 1 of the ocean state (cf_time_steps insists on it).                                */
int cf_halo_exchange_rows(cf_ctx* ctx, double* const* d_fields, int nfields, int rows);

/* Peer-direct halo rows (the reference's analogue is the CUDA-IPC transport of its GPU-aware MPI,
 * experiments/OMIPSimulations/scripts/launch.sh:270-290).  At 46 KB per neighbour the exchange is latency bound, so
 * beside the RCCL path there is one that needs no collective library at all: every rank owns a MAILBOX in
 * fine-grained device memory, exported as a HIP IPC handle; a neighbour maps it and one kernel per step (i) stores
 * this rank's boundary rows straight into both neighbours' mailboxes over xGMI, (ii) publishes a sequence number with
 * a system-scope release, (iii) waits (bounded spin) for the neighbours' sequence numbers and (iv) copies their rows
 * into the halo rows — one launch, no host round trip.  Mailboxes are double-buffered by sequence parity; a rank can
 * only write parity p again after its own step-(s+1) wait, which implies the neighbour has drained step s.
 *   cf_peer_halo_export   allocate this rank's mailbox for at most `max_fields` fields × `max_rows` rows, write its
 *                         IPC handle (CF_PEER_HANDLE_BYTES) — the host distributes handles (MPI / torch.distributed).
 *                         Fails with CF_ERR_COMM when the device has no fine-grained memory to give (the protocol is
 *                         not safe on coarse-grained memory): use the RCCL exchange then.
 *   cf_peer_halo_connect  map the south (rank−1) and north (rank+1) mailboxes; NULL at the ends of the slab ring.
 *                         On the LAST rank of a tripolar grid the north handle is NULL too: its north boundary is the
 *                         fold (one_degree_tripolar.jl:48-51), served locally by cf_fold_north_halo, not by a peer.
 *                         ALL RANKS EXPORT ONE SHAPE ON ONE GRID WIDTH: a rank addresses its neighbour's mailbox with the
 *                         slot size of its own, max_fields · max_rows · (nx + 2hx).  Every mailbox carries the triple
 *                         (max_fields, max_rows, nx + 2hx) it was exported for, and cf_peer_halo_connect compares each
 *                         neighbour's with this context's: on a difference it returns CF_ERR_INVALID with both triples in
 *                         the message, launches nothing and leaves the context unconnected (cf_halo_exchange_rows_peer
 *                         then answers as if cf_peer_halo_connect had not been called), whatever it was connected to before.
 *   cf_halo_exchange_rows_peer   the per-step exchange, same meaning as cf_halo_exchange_rows: 1 … max_fields fields ×
 *                         1 … min(max_rows, ny) rows per call.  Inside the mailbox slot of the call's sequence parity, field f
 *                         lies at f · rows · (nx + 2hx) doubles with the call's own `rows`, so `nfields` and `rows` of a
 *                         step's call ARE THE SAME ON EVERY RANK.  That is the caller's contract and is not checked.
 * A spin that exceeds its bound sets a sticky error that the next cf_sync reports (CF_ERR_COMM).            */
#define CF_PEER_HANDLE_BYTES 64
int cf_peer_halo_export(cf_ctx* ctx, int max_fields, int max_rows, void* handle_out);
int cf_peer_halo_connect(cf_ctx* ctx, const void* south_handle, const void* north_handle, int rank, int nranks);
/* Footprint: sends the `rows` boundary rows, full width nx + 2hx, and writes the `rows` halo rows next to each neighbour,
 * full width; no other cell.                                                                                            */
int cf_halo_exchange_rows_peer(cf_ctx* ctx, double* const* d_fields, int nfields, int rows);
/* How many peer-direct exchanges this context has issued, and how many of them rode in a solver launch
 * (CF_OPT_HALO_IN_SOLVER_LAUNCH) instead of the exchange kernel of their own.  A measurement / test aid.      */
int cf_peer_halo_stats(cf_ctx* ctx, unsigned long long* exchanges, unsigned long long* in_solver_launch);

/* The tile world: the surface partitioned in BOTH directions (the reference's Distributed(GPU(), partition = Partition(2,2)),
 * examples/sixth_degree_tripolar_ocean_sea_ice.jl:22).  A rectangular world of px × py ranks, rank = p + px · q — x FASTEST.
 * Rank (p, q) owns columns [p · nx, (p + 1) · nx) of the global Nx = px · nx and one contiguous block of rows.  EVERY RANK HAS
 * THE SAME nx (the fold maps a tile onto a whole tile only then); row blocks may differ between rows of ranks; the ranks of one
 * row share ny and hy, the ranks of one column — and fold partners — share nx and hx.  x is periodic: the east neighbour of p
 * is (p + 1) mod px; with px = 2 both x-neighbours are one rank, served by separate slots and flags.  y is not periodic.  px is
 * 1 or even.  On the top row (q = py − 1) of a tripolar world the north side is the FOLD PARTNER (px − 1 − p, py − 1); with
 * px = 1 that is the rank itself, nothing is mapped and cf_fold_north_halo's kernel serves.  A context is connected to latitude
 * slabs (cf_peer_halo_connect) or to a tile world, never to both; each refuses a context the other has connected.
 *   cf_peer_tile_export   allocates this rank's tile mailbox in fine-grained device memory (CF_ERR_COMM where the device has
 *                         none to give) and writes its IPC handle: eight flags [side W, E, S, N][parity] on 64-byte lines of
 *                         their own, one line that carries the tuple the mailbox was exported for — (max_fields, max_rows,
 *                         max_cols, nx + 2hx, ny, hx, hy) —, then two parities of a slot per side: max_fields · max_cols · ny
 *                         doubles for W and E, max_fields · max_rows · (nx + 2hx) for S and N.  1 ≤ max_fields ≤ 8,
 *                         1 ≤ max_rows ≤ hy, 1 ≤ max_cols ≤ hx; a step needs max_rows ≥ ring + 1 and max_cols ≥ ring + 1, on the
 *                         top row of a tripolar world with px > 1 max_cols ≥ ring + 2 (see the footprint).
 *   cf_peer_tile_connect  `handles`: px · py × CF_PEER_HANDLE_BYTES, entry r from rank r.  Maps the W, E, S and N neighbours (each
 *                         rank once, however many sides it serves) and compares the tuple each mailbox carries with this
 *                         rank's: W and E in (ny, hy, max_*), S, N and the partner in (nx + 2hx, hx, max_*).  CF_ERR_INVALID —
 *                         with both tuples in the message where tuples differ —, nothing launched and the context left
 *                         unconnected, whatever it was connected to before, for: a difference; px, py < 1 or a rank outside
 *                         the world; px odd and greater than 1; px · py > CF_PEER_REDUCE_MAX_RANKS; tripolar with an odd
 *                         Nx = px · nx; a handle that is no tile mailbox; a context connected to latitude slabs.  A world of one
 *                         (px = py = 1) maps nothing; handles may be NULL.  Every rank of a world has issued the same number
 *                         of exchanges when it connects (zero, normally): the caller's contract, not checked.
 *   cf_halo_exchange_tile_peer  one exchange of 1 … max_fields fields × 1 … min(max_rows, ny, hy) rows.  fold_north = 1 on EVERY
 *                         rank of the top row of a tripolar world and 0 on every other rank (anything else is refused);
 *                         locations[f] ∈ CF_FOLD_*, signs[f] = ±1 as for cf_fold_north_halo, read only where fold_north = 1
 *                         (NULL otherwise).  nfields, rows and the locations ARE THE SAME ON EVERY RANK: not checked.
 *   cf_peer_tile_stats    since the context was created: exchanges issued (one sequence number each), x-phase launches (one
 *                         per exchange where px > 1, none where px = 1) and exchanges whose north side sent a fold to a partner
 *                         (every exchange on the top row of a tripolar world with px > 1, none elsewhere).  A test aid.
 * One exchange, on the context's stream, no host synchronisation, one sequence number for both phases:
 *   1. x-phase (px > 1; with px = 1 the x-halos stay the caller's), one launch of two workgroups: each side stores its ring + 1
 *      boundary COLUMNS of every field, interior rows 0 … ny − 1, into the x-neighbour's slot as [field][column][row] (a wave's
 *      remote stores are one contiguous run), publishes, waits (bounded) and copies the received columns into its x-halo columns.
 *   2. y-phase (where a south or north neighbour or a partner exists), one launch behind the first: the S and N rows travel
 *      full width nx + 2hx by the protocol of cf_halo_exchange_rows_peer — the sender's x-halos are filled, so the corner
 *      cells arrive without a diagonal message.  Towards the fold partner the SENDER writes the partner's north halo rows
 *      already mirrored and signed: the partner's halo row ny − 1 + r at its column i is sign · (this rank's value) at column
 *      nx − 1 − i, row ny − 1 − r (centres), column nx − 1 − i, row ny − r (y-faces), column nx − i, row ny − 1 − r (x-faces; sign
 *      is |sign| exactly where the GLOBAL periodic image of the partner's column is 0): cf_fold_north_halo's rule through the
 *      tile's global column offset, −0.0 surviving as there.  The x-face map reads this rank's east halo columns up to
 *      nx + ring + 1, which is why the columns travel first and why the x-phase fills ring + 2 east columns on such a rank.
 *   3. With px = 1 and fold_north the exchange ends with cf_fold_north_halo's own launch (counted by cf_debug_fold_counts).
 * A wait that exceeds its bound copies nothing and sets the sticky error the next cf_sync reports (CF_ERR_COMM), naming the
 * side: the west or east neighbour's columns, the south or north neighbour's rows, the fold partner's rows.
 * Footprint: DEFINES every halo cell within ring + 1 (= rows, as cf_time_steps passes them) of the interior, corners included —
 * what a step's kernels read.  Written beyond that: the S and N halo rows over the full width (outside the ring + 1 columns
 * they hold whatever the sender's x-halo held there); on a rank that sends a fold, east halo column nx + ring + 1 on the
 * interior rows.  The folded north rows are written over columns −(ring + 1) … nx + ring ONLY: the x-face map has no source for
 * column −hx inside the partner's array, and the outer columns of those rows are left UNTOUCHED.  No other cell: the W and E halo
 * columns of the halo rows come with the rows, never from the x-phase.  Requires nx ≥ ring + 1 and hx ≥ ring + 1 where px > 1
 * (ring + 2 both where a fold is sent), and with fold_north ny ≥ rows + 1.                                                  */
int cf_peer_tile_export(cf_ctx* ctx, int max_fields, int max_rows, int max_cols, void* handle_out);
int cf_peer_tile_connect(cf_ctx* ctx, const void* handles, int px, int py, int rank, int tripolar);
int cf_halo_exchange_tile_peer(cf_ctx* ctx, double* const* d_fields, const int* locations, const double* signs, int nfields, int rows,
                               int fold_north);
int cf_peer_tile_stats(cf_ctx* ctx, unsigned long long* exchanges, unsigned long long* column_launches, unsigned long long* folds_sent);

/* The reduction world of the exact sums (cf_normalize_salinity_flux_exact).  Halo mailboxes connect neighbours; a global sum needs
 * every rank, so every rank owns a second, small mailbox in fine-grained device memory that EVERY other rank maps: two parities ×
 * CF_PEER_REDUCE_MAX_RANKS slots (the accumulators of Σ J·A and Σ A with their non-finite counters, 140 64-bit words) and one
 * flag per parity and rank on a 64-byte line of its own.  Each reduction a context issues takes the next sequence number s: the
 * finishing workgroup stores its accumulators into slot [s mod 2][my rank] of every other rank's mailbox, fences at system scope,
 * publishes s in that rank's flag [s mod 2][my rank] (system-scope release), waits for the other nranks − 1 flags of its own
 * mailbox (one lane per flag, sleeping, with the bound of the halo rows), acquires and adds digit-wise.  A rank publishes s + 1
 * only after it has read every slot of s: two parities are enough, by the argument of the halo mailboxes.  No collective library.
 *   cf_peer_reduce_export    allocate this rank's reduce mailbox and write its IPC handle (CF_PEER_HANDLE_BYTES).  CF_ERR_COMM
 *                            when the device has no fine-grained memory to give, as cf_peer_halo_export.
 *   cf_peer_reduce_connect   `handles`: nranks × CF_PEER_HANDLE_BYTES, entry r from rank r (the rank's own entry is not opened).
 *                            nranks = 1 is valid: it maps nothing and nothing ever waits (handles may be NULL).  Every mailbox
 *                            carries its layout's version and size; a foreign one, nranks outside 1 … CF_PEER_REDUCE_MAX_RANKS
 *                            or a bad rank returns CF_ERR_INVALID and leaves the context unconnected, whatever it was connected to
 *                            before.  A context that has already reduced over a world cannot join another.
 * THE NUMBER OF REDUCTIONS IS THE SAME ON EVERY RANK — every cf_normalize_salinity_flux_exact on a connected context, every
 * step of cf_time_steps_coupled with CF_NORMALIZE_EXACT — as for the halo rows: the caller's contract, not checked.  A wait that
 * exceeds its bound sets the sticky error that the next cf_sync reports (CF_ERR_COMM); the kernel ends with this rank's own sums. */
#define CF_PEER_REDUCE_MAX_RANKS 8
int cf_peer_reduce_export(cf_ctx* ctx, void* handle_out);
int cf_peer_reduce_connect(cf_ctx* ctx, const void* handles, int rank, int nranks);

/* Tripolar fold (TripolarGrid(arch; size=(360,180,Nz)), OceanConfigurations/one_degree_tripolar.jl:48-51; the
 * fold itself lives in Oceananigans' zipper boundary condition, [UPSTREAM-RECALL] fold_north_center_center! /
 * _face_center! / _center_face!).  The northern boundary of the global grid is folded onto itself about the LAST
 * row of tracer points (that row is its own mirror image), so the north halo rows of the last latitude slab come
 * from that slab's own northern interior rows mirrored in i.  0-based interior indices, r = 1…rows:
 *   centres (T, S, fluxes):  f[i, ny−1+r] = sign · f[nx−1−i, ny−1−r]
 *   x-faces (u):             f[i, ny−1+r] = s    · f[(nx−i) mod nx, ny−1−r],  s = |sign| where nx−i wraps (i = 0)
 *   y-faces (v):             f[i, ny−1+r] = sign · f[nx−1−i, ny−r]
 * `sign` = −1 for the components of a vector (u, v change sign across the fold), +1 for scalars.  The periodic
 * x-halos of the written rows are filled from the written interior columns.  Folding is an involution on the
 * mirrored rows (tests/test_tripolar.py).                                                                    */
#define CF_FOLD_CENTER 0
#define CF_FOLD_X_FACE 1
#define CF_FOLD_Y_FACE 2
/* `nfields` fields in one launch: locations[f] ∈ CF_FOLD_*, signs[f] = ±1. */
/* Footprint: reads rows ny − 1 − rows … ny − 1 at interior columns; writes north halo rows ny … ny + rows − 1 over the full
 * width nx + 2hx; no other cell.                                                                                       */
int cf_fold_north_halo(cf_ctx* ctx, double* const* d_fields, const int* locations, const double* signs, int nfields,
                       int rows);
/* Since the context was created: the launches of the fold's own kernel (cf_fold_north_halo, and cf_time_steps / cf_time_steps_coupled
 * with fold_north where they issue it), and the peer-direct exchange launches whose north side was the fold (cf_time_steps_coupled
 * under CF_HALO_PEER with fold_north).  Either pointer may be NULL.  A measurement / test aid.                                */
int cf_debug_fold_counts(cf_ctx* ctx, long long* fold_launches, long long* exchanges_with_fold);

/* ------------------------------------------------------------------------------------------
 * run!(simulation) for a coupled model whose ocean component is prescribed (README.md:76-77): `nsteps` × time_step!
 * without returning to the host language — per step (optional halo rows) → cf_update_state.  What varies from step
 * to step is what varies in a coupled run: the clock (the JRA55 time fraction ñ advances by Δt/Δt_snapshot and the
 * bracketing snapshots move through the window) and the ocean surface state (step s reads ocean_states[s mod n]).
 * With `pipeline` ≠ 0 the atmosphere state of step s+1 is interpolated while the solver of step s runs (on the
 * auxiliary stream, or inside the step's launches: CF_OPT_MERGED_PREFETCH; the prescribed atmosphere does not depend on
 * the ocean); this needs two sets of exchange fields, step s uses atmos[s mod 2].
 *   CF_PIPELINE_WITHIN_CALL (1): only steps of this call are prefetched — the call reads the source at the levels of
 *     steps first_step … first_step + nsteps − 1 and nothing else, and leaves the other exchange set as the last-but-one
 *     step left it.
 *   CF_PIPELINE_CONTINUING (2): the last step also requests step first_step + nsteps, for a loop that goes on in the
 *     next call (which recognises the pending state by its output set and by the whole interpolation it asks for — source
 *     arrays and shape, levels, time fraction and weights, as cf_prefetch_atmosphere_state states; a call that finds anything
 *     else pending for its first step, or nothing, starts that step's interpolation itself).  The caller
 *     guarantees that the source slots of that step are resident and FINAL when this call is made (a sliding window
 *     must not recommit them in between — cf_window_commit / an upload into a level a pending request reads voids it
 *     silently), and that exchange set (first_step + nsteps) mod 2 is not read after this call's last step: it is
 *     overwritten.  A caller that stops after such a call has one unused interpolation in that set.
 * All launches are stream ordered; nothing synchronises with the host.
 * Outputs (CF_OPT_LAND_ZEROS = 1, the default): the call's FIRST step writes every cell of `fluxes` and `net` that
 * cf_update_state writes, land included; later steps of the call write the wet cells and leave the land cells alone — they
 * hold the first step's zeros, which are what every step would write.  So nothing else may write `fluxes` or `net` while the
 * call's work is on the stream (reading them, cf_attach_average / _integrals included, is fine), and the wet mask — one
 * pointer per schedule — is not rewritten in between.  Between two calls anything may happen to them: every call starts over.
 * CF_OPT_LAND_ZEROS = 0 writes the land at every step.
 * Refusals: everything one of the call's steps would refuse, at whichever step — a NULL field in any ocean state, in either
 * exchange set, in the source, the weights, `fluxes` or `net`; with fold_north, a grid the fold does not apply to (odd nx,
 * ny < ring + 2); under CF_HALO_PEER, a mailbox that does not take 4 fields × halo_rows — is refused with CF_ERR_INVALID
 * BEFORE the first launch and before anything of the context changes (behind the refusals of the schedule's own scalars
 * and of what is attached, in that order).  A refused call has written nothing, requested no atmosphere state ahead and
 * left nothing for a later call to trip over: the next cf_update_state or cf_time_steps on the context runs as if the
 * refused call had not been made (tests/test_refused_step_calls.py).
 * Tile worlds: on a context connected by cf_peer_tile_connect, halo_backend = CF_HALO_PEER runs cf_halo_exchange_tile_peer's
 * exchange of T, S, u, v per step (centre, centre, x-face, y-face; signs +, +, −, −) with halo_rows rows; fold_north = 1 is
 * passed by EVERY rank of the top row of a tripolar world and by no other.  CF_OPT_HALO_IN_SOLVER_LAUNCH arms no request
 * there: the exchange kernels run.  Refused before the first launch, under the contract above: a tile mailbox too small for
 * 4 fields × halo_rows rows × ring + 1 columns (ring + 2 where a fold is sent); fold_north that disagrees with the rank's place
 * in the world; halo_backend = CF_HALO_RCCL.  cf_time_steps_coupled refuses a tile world with px > 1 by name: the ice rows and
 * the stresses do not cross x yet (tests/test_tile_steps.py).                              */
#define CF_PIPELINE_WITHIN_CALL 1
#define CF_PIPELINE_CONTINUING 2
#define CF_HALO_NONE 0
#define CF_HALO_RCCL 1
#define CF_HALO_PEER 2
typedef struct cf_run_schedule {
    int32_t struct_size;             /* sizeof(cf_run_schedule) */
    int32_t n_ocean_states;          /* ≥ 1 */
    const cf_ocean_surface* ocean_states;
    int32_t n_atmos_sets;            /* 1, or 2 with pipeline */
    int32_t pipeline;                /* 0, CF_PIPELINE_WITHIN_CALL or CF_PIPELINE_CONTINUING */
    const cf_exchange_fields* atmos; /* n_atmos_sets entries */
    int32_t first_level;             /* memory level of snapshot n₁ at step 0; levels advance cyclically */
    int32_t halo_backend;            /* CF_HALO_* */
    int32_t halo_rows;               /* rows exchanged per step (ring + 1) */
    int32_t fold_north;              /* 1: tripolar grid, this rank owns the fold (last rank) */
    double time_fraction;            /* ñ at step 0 */
    double time_fraction_increment;  /* Δt / Δt_snapshot: 20 min / 3 h = 1/9 (README.md:76) */
} cf_run_schedule;
int cf_time_steps(cf_ctx* ctx, int64_t first_step, int nsteps, const cf_run_schedule* schedule,
                  const cf_atmos_source* src /* levels / fraction are overridden per step */,
                  const cf_interp_weights* w, const cf_interface_fluxes* fluxes, const cf_sea_ice_fields* ice,
                  const cf_net_ocean_fluxes* net);

/* run!(simulation) of the OMIP configuration — OceanSeaIceModel(ocean, sea_ice; atmosphere, land, interfaces) with the
 * salinity restoring on the top boundary condition and NormalizeSalinity at IterationInterval(1) (omip_simulation.jl:123-163,
 * :385-388, :507-523) — without returning to the host language.  cf_time_steps' arguments and clock, plus this block.  Per step
 * s (global index), on the context's stream, no host synchronisation:
 *   1. fold_north: cf_fold_north_halo on the four ocean rows, as cf_time_steps does (under CF_HALO_PEER the fold is the north
 *      side of the step's exchanges instead: "Tripolar slabs" below);
 *   2. the preamble (cf_prepare_coupled_step; each job optional): the land freshwater at the block's own clock — levels and
 *      fraction from land_first_level, land_time_fraction, land_time_fraction_increment by cf_time_steps' arithmetic — into
 *      land_freshwater, which the net ocean fluxes then read as if handed to cf_set_land_freshwater (it stays set after the
 *      call); with compute_ice_ocean the three-equation exchange and frazil from ocean state s, ℵ of ice state s and the
 *      stresses of `ice` into ice_ocean_fluxes; the restoring buffer from ocean state s;
 *   3. with a pipelined schedule the request for step s + 1's atmosphere state, exactly as cf_time_steps makes it;
 *   4. cf_update_state_sea_ice with ocean_states[s mod n_ocean_states] and ice_states[s mod n_ice_states] (ℵ, hᵢ, hₛ, velocities,
 *      albedo; its top_temperature is ignored).  The partition reads ℵ of that ice state, the stresses of `ice`, and
 *      ice_ocean_fluxes.interface_heat / salt_flux (computed in 2 or, without compute_ice_ocean, taken as given; NULL ⇒ 0;
 *      `ice`'s own interface_heat / salt_flux are not read); the net sea-ice fluxes read ice_ocean_fluxes.frazil_heat /
 *      interface_heat.  skin_temperature is CARRIED: the first guess of the interface solve and the buffer its result is
 *      written to — the in-place update cf_sea_ice_state documents; ai_fluxes.temperature is NULL or that very buffer;
 *   5. normalize_salinity = 1: cf_normalize_salinity_flux on net->S with restoring_buffer (or NULL), `area` and `mean_out`;
 *      CF_NORMALIZE_EXACT (2): cf_normalize_salinity_flux_exact with the same arguments (single-domain callers may use it too);
 *   6. the attached averager, integrator and monitor, by cf_time_steps' rule.
 * Land cells are written at every step (CF_OPT_LAND_ZEROS does not apply to this loop).
 * CF_ERR_INVALID, with the field named, before anything is launched — the outputs are untouched — for: a NULL block or a
 * wrong struct_size; cf_set_sea_ice_formulation not called; n_ice_states < 1 or ice_states NULL; an ice state without
 * concentration or thickness; `ice`->concentration that is neither NULL nor the concentration of every ice state (the
 * partition and the interface solve would disagree); land_first_level outside the land source's levels, a negative or
 * non-finite land_time_fraction / _increment, a bad land shape; NULL among skin_temperature, ai_fluxes, net_ice, the
 * land_freshwater of a land job, the ice_ocean_fluxes of compute_ice_ocean, `fluxes`, `net`, the exchange sets or the
 * ocean states; an ai_fluxes.temperature that is another buffer; mean_out inside any array of the call; normalize_salinity
 * outside 0 … 2; and what the next paragraph refuses.
 * Latitude slabs: halo_backend = CF_HALO_PEER.  What crosses a slab boundary: the interface solve reads the ice state on W, the
 * partition reads ℵ at j − 1, the ice–ocean exchange reads y_stress at j + 1, and the carried skin temperature is first guess and
 * result on W.  So, through the exchange kernel of cf_halo_exchange_rows_peer, halo_rows rows each:
 *   per step, in front of the fold and the preamble: the four ocean fields of the step's ocean state, as cf_time_steps exchanges
 *     them, and the non-NULL fields of the step's ice state in the order concentration, thickness, snow_thickness, u, v, albedo.
 *     The list is cut into exchanges of at most 8 fields: one exchange up to 8 fields, two beyond;
 *   once per call with nsteps > 0, in front of the first step: the non-NULL ones of ice->x_stress, ice->y_stress, and
 *     skin_temperature, as one exchange.  After that both neighbours recompute the ring rows of the skin temperature from
 *     identical inputs: they stay the neighbour's bits (tests/test_coupled_slabs.py).
 * cf_peer_halo_stats' exchange count therefore grows by 1 + nsteps · (1 or 2) per call.  The split depends only on which optional
 * fields are non-NULL: THAT THOSE ARE THE SAME ON EVERY RANK, like the number of steps, is the caller's contract and is not
 * checked.  CF_OPT_HALO_IN_SOLVER_LAUNCH arms no request in this loop: its solver launch is not the one that carries riders.  The
 * x-halos of all these fields stay the caller's.  Attached collections collect per rank, as in cf_time_steps.
 * Tripolar slabs: the LAST rank (no north mailbox) passes fold_north = 1 with CF_HALO_PEER, the others 0.  On that rank every
 * exchange above is the SAME launch with the fold as its north side: workgroup 0 exchanges with the south neighbour, the others
 * fold the north halo_rows rows of the exchange's own fields by cf_fold_north_halo's arithmetic, bit for bit, each field with its
 * own location and sign —
 *     T, S: centre, +1      ocean u: x-face, −1      ocean v: y-face, −1      ℵ, hᵢ, hₛ, albedo: centre, +1
 *     ice u, v: centre, −1 (cf_sea_ice_state holds them at cell centres)
 *     x_stress: x-face, −1      y_stress: y-face, −1      skin_temperature: centre, +1
 * (coflux/distributed.py: coupled_fold_plan states the same table).  The four ocean fields ride in the step's first exchange: the
 * rank issues no launch of cf_fold_north_halo's kernel in this loop, every rank issues the same number of launches per step, and
 * cf_peer_halo_stats grows as above on every rank; cf_debug_fold_counts counts the exchanges that carried a fold.  The stresses and
 * the skin temperature are folded once per call, exactly as a neighbour delivers them once per call; afterwards the skin
 * temperature's north ring row is the solve's own result on the ring, computed from folded inputs.  Where a neighbour's rows leave
 * the x-halos of the written rows to the sender's, the fold writes them itself, from the periodic image.  Under CF_HALO_NONE
 * fold_north folds the four ocean rows by a launch of its own and the ice halos stay the caller's (tests/test_coupled_fold_*.py).
 * Refused with CF_ERR_INVALID before the first launch, outputs and cf_peer_halo_stats unchanged, the field named:
 *   halo_backend = CF_HALO_RCCL: nothing has exercised the ice rows or the global mean over RCCL;
 *   halo_backend = CF_HALO_PEER on a context whose halo mailboxes are not connected (cf_peer_halo_connect) or too small for the
 *     call's exchanges (the largest of them × halo_rows);
 *   fold_north on a grid the fold does not apply to (odd nx, ny < ring + 2), under either backend;
 *   fold_north together with CF_HALO_PEER on a context whose north mailbox is connected: the last rank owns the fold;
 *   normalize_salinity = 1 under CF_HALO_PEER: its summation order depends on the slab;
 *   normalize_salinity = CF_NORMALIZE_EXACT under CF_HALO_PEER without a reduction world (cf_peer_reduce_connect).            */
#define CF_NORMALIZE_EXACT 2
typedef struct cf_coupled_step {
    int32_t struct_size;                  /* sizeof(cf_coupled_step) */
    int32_t n_ice_states;                 /* ≥ 1 */
    const cf_sea_ice_state* ice_states;   /* step s reads ice_states[s mod n_ice_states] */
    double* skin_temperature;             /* carried top surface temperature [°C] */
    cf_interface_fluxes ai_fluxes;        /* atmosphere–sea-ice interface fluxes (temperature: NULL or skin_temperature) */
    cf_net_sea_ice_fluxes net_ice;
    cf_land_source land;                  /* friver NULL ⇒ no land job; level1, level2, time_fraction are overridden per step */
    int32_t land_first_level;             /* memory level of the land snapshot n₁ at step 0; levels advance cyclically */
    int32_t compute_ice_ocean;            /* 1: the preamble computes ice_ocean_fluxes from `ice_ocean`; 0: they are inputs */
    double land_time_fraction;            /* ñ of the land record at step 0 */
    double land_time_fraction_increment;
    double* land_freshwater;              /* M_land on W */
    cf_ice_ocean_params ice_ocean;
    cf_ice_ocean_fluxes ice_ocean_fluxes; /* Q_io, Jˢ_io, Q_frazil[, u★] */
    double piston_velocity;               /* restoring: v_p [m/s], S★, J_add; restoring_buffer NULL ⇒ no restoring job */
    const double* target_salinity;
    double* restoring_buffer;
    int32_t normalize_salinity;           /* NormalizeSalinity after every step: 0 none, 1 cf_normalize_salinity_flux, CF_NORMALIZE_EXACT */
    int32_t reserved;
    const double* area;                   /* cell areas for the normalisation (NULL ⇒ uniform) */
    double* mean_out;                     /* device double: the mean the last step subtracted (may be NULL) */
} cf_coupled_step;
/* Footprint: per step cf_fold_north_halo's (fold_north), cf_prepare_coupled_step's, cf_update_state_sea_ice's,
 * cf_normalize_salinity_flux's (every cell of net->S, and *mean_out) and those of the attached collections; under CF_HALO_PEER
 * cf_halo_exchange_rows_peer's on the exchanged fields (the ice states' and the stresses' halo rows are WRITTEN); with fold_north
 * under CF_HALO_PEER cf_fold_north_halo's on every exchanged field: the north halo_rows rows over the full width nx + 2hx, the
 * x-halo columns of those rows included.                                                                                    */
int cf_time_steps_coupled(cf_ctx* ctx, int64_t first_step, int nsteps, const cf_run_schedule* schedule,
                          const cf_atmos_source* src, const cf_interp_weights* w, const cf_interface_fluxes* fluxes,
                          const cf_sea_ice_fields* ice, const cf_net_ocean_fluxes* net, const cf_coupled_step* coupled);

/* ------------------------------------------------------------------------------------------
 * Time averages of surface fields on the device: the output that every reference configuration writes, e.g. the OMIP
 * surface diagnostics tauuo, tauvo, hfds, wfo, hfss, hfls as 5-day means (OMIPConfigurations/omip_diagnostics.jl:125-130,
 * JLD2Writer(…; schedule = AveragedTimeInterval(surface_averaging_interval)) :152-158).  An averager holds up to
 * CF_AVERAGE_MAX_FIELDS (source, mean) pairs of ocean-grid arrays in the usual halo layout and a window's total weight.
 * A collection of weight w is ONE launch over the interior I of every field, the running-mean form of Oceananigans'
 * WindowedTimeAverage / integrate_average! [UPSTREAM-RECALL]:
 *     first collection of a window:  m = f                       (m is not read: a fresh buffer may hold NaNs)
 *     every later one:               m = (m · c_prev) + (f · c_new),  c_prev = T_prev / T_cur, c_new = w / T_cur, T_cur = T_prev + w
 * with c_prev and c_new computed on the host in double and two products and one sum on the device, each rounded (no FMA).
 * The mean is therefore valid after every collection: Σ w f / Σ w up to rounding.
 *   cf_average_create   CF_ERR_INVALID if nfields is outside 1…CF_AVERAGE_MAX_FIELDS, a pointer is NULL, or the parent
 *                       array of a mean ((nx + 2hx)(ny + 2hy) doubles from its pointer) overlaps a source's or another mean's.
 *   cf_average_destroy  detaches the averager if it is attached; an averager outlived by its context may still be destroyed
 *                       (every other call on it then fails).
 *   cf_average_reset    a new window: total weight 0, the next collection stores.  No device work.
 *   cf_average_collect  one launch on the context's stream; weight > 0 and finite.  No host synchronisation.
 *   cf_average_weight   the window's total weight and number of collections (either pointer may be NULL).
 *   cf_attach_average   cf_time_steps collects `a` after the cf_update_state of every step s (global index) with
 *                       (s + 1) % stride == 0, weight stride · step_weight; NULL detaches.  One averager per context:
 *                       attaching another replaces it.  Stream order puts the collection behind every write of the step
 *                       (every CF_OPT_MERGED_PREFETCH / _HALO_IN_SOLVER_LAUNCH / _SOLVER_PATH / _FUSED_NET mode alike), so a
 *                       run split into CF_PIPELINE_CONTINUING calls collects the same steps as one call.  Window boundaries
 *                       are call boundaries: the caller reads the means, then calls cf_average_reset.
 * ---------------------------------------------------------------------------------------- */
#define CF_AVERAGE_MAX_FIELDS 16
typedef struct cf_average cf_average;
int cf_average_create(cf_ctx* ctx, int nfields, const double* const* d_sources, double* const* d_means, cf_average** out);
int cf_average_destroy(cf_average* a);
int cf_average_reset(cf_average* a);
/* Footprint: reads the sources on I; reads and writes the means on I (the first collection of a window only writes them).
 * Nothing else is read or written, the halos of the means included.                                                    */
int cf_average_collect(cf_average* a, double weight);
int cf_average_weight(cf_average* a, double* total, int64_t* samples);
/* Footprint: cf_time_steps' own, and cf_average_collect's at every collected step.                                     */
int cf_attach_average(cf_ctx* ctx, cf_average* a, int32_t stride, double step_weight);

/* ------------------------------------------------------------------------------------------
 * Derived surface quantities averaged in the collection launch: what a reference run averages beyond arrays that exist —
 * the squares tossq, sossq (omip_diagnostics.jl:111-123; variances are mean(x²) − mean(x)², visualize/cache.jl:366-370),
 * the centred squares of the face velocities and the kinetic energy (uu_at_ccc = ℑx(u²), vv_at_ccc = ℑy(v²),
 * ke_at_ccc = (ℑx(u²) + ℑy(v²))/2, omip_diagnostics.jl:13-25) — and what every figure does to a time mean, all of it linear
 * and so commuting with the mean: face → centre (cache.jl:378-386), rotation to geographic east / north with the grid's
 * (cos θ, sin θ) (cache.jl:406-466), scaling to CMIP units (cache.jl:359-361,378).
 *
 * cf_average_create_derived returns an ordinary cf_average: cf_average_collect / _reset / _weight / _destroy and
 * cf_attach_average work on it unchanged.  Each of its n_terms (1 … CF_AVERAGE_MAX_FIELDS) turns arrays into one SAMPLE per
 * interior cell (i, j), and the sample enters the recurrence above in place of f: the first collection of a window stores
 * m = sample and never reads m, every later one computes m = (m · c_prev) + (sample · c_new).  With x per kind as in the
 * table below — [i+1] the cell's east neighbour, [j+1] its north neighbour, the convention of cf_ocean_surface.u / v —
 *     sample = x · scale        (always multiplied: scale = 1.0 is exact and keeps −0.0 and NaN)
 * (a NaN stays a NaN; its sign and payload are not part of the contract — IEEE 754 leaves them open, and a subtraction is
 * an addition of the negated operand on this device)
 * and every product, sum and · 0.5 rounded on its own, in the order written (no FMA).  For EAST / NORTH, p = CENTER_X(a)
 * and q = CENTER_Y(b), or p = a and q = b with CF_TERM_AT_CENTERS; c and s are cos_rotation and sin_rotation at the cell.
 * All arrays are float64 in the context's halo layout, 8-byte aligned.  There is no mask: every interior cell is evaluated
 * and land values pass through (the reference masks after the time mean).  Where a term reads [i+1] / [j+1] the caller
 * has filled the first east halo column / north halo row of that array: periodic wrap, neighbour slab or cf_fold_north_halo.
 * The library's own outputs (cf_interface_fluxes, cf_net_ocean_fluxes) are written on the interior (and ring) only: a term
 * that reads their [i+1] / [j+1] needs those halos filled after every step and before the collection, which a caller can do
 * between cf_update_state and cf_average_collect but NOT inside cf_time_steps — attach such terms only on arrays whose halos
 * the caller keeps (the ocean state), and keep face → centre terms on flux fields to the host-driven loop.
 *
 * CF_ERR_INVALID, with nothing allocated or launched: wrong struct_size; max_workgroups < 0 or reserved != 0; n_terms outside 1 … CF_AVERAGE_MAX_FIELDS or
 * terms NULL; an unknown kind, a flag bit other than CF_TERM_AT_CENTERS, or that flag on a kind other than EAST / NORTH;
 * NULL a or mean; NULL b where the kind reads it (PRODUCT, KINETIC_ENERGY, EAST, NORTH); NULL cos_rotation / sin_rotation
 * with an EAST / NORTH term; a non-finite scale; a kind that reads [i+1] on a context with hx < 1 or [j+1] with hy < 1;
 * more than CF_DERIVED_MAX_SOURCES distinct source arrays (the rotation arrays count when a term reads them); a mean
 * whose parent array ((nx + 2hx)(ny + 2hy) doubles from its pointer) overlaps a source, a rotation array or another mean.
 * The descriptor and its term table are host memory, read during the call only.
 *
 * Footprint of a collection (ONE launch for all terms; each distinct source array is loaded once per cell however many
 * terms name it, the [i+1] value comes from the neighbouring lane): reads each source on I, plus column nx (rows
 * 0 … ny − 1) where a term reads its [i+1], plus row ny (columns 0 … nx − 1) where a term reads its [j+1]; reads and writes
 * the means on I (the first collection of a window only writes them).  Nothing else is read or written.  The bits of
 * every mean depend on those values and the weights alone — not on halo widths, base alignment, the launched grid or on
 * which other terms ride along.  Algorithmic bytes per cell: 8 · (distinct source arrays) + 16 · n_terms accumulating,
 * 8 · (distinct source arrays) + 8 · n_terms storing.
 * ---------------------------------------------------------------------------------------- */
#define CF_TERM_FIELD            0  /* x = a                                             */
#define CF_TERM_PRODUCT          1  /* x = a·b            (b == a: a square)             */
#define CF_TERM_CENTER_X         2  /* x = (a[i,j] + a[i+1,j]) · 0.5        ℑx           */
#define CF_TERM_CENTER_Y         3  /* x = (a[i,j] + a[i,j+1]) · 0.5        ℑy           */
#define CF_TERM_CENTER_X_SQUARE  4  /* x = (a[i,j]·a[i,j] + a[i+1,j]·a[i+1,j]) · 0.5     */
#define CF_TERM_CENTER_Y_SQUARE  5  /* same with j+1                                     */
#define CF_TERM_KINETIC_ENERGY   6  /* x = (X_SQUARE(a) + Y_SQUARE(b)) · 0.5             */
#define CF_TERM_EAST             7  /* x = p·c − q·s                                     */
#define CF_TERM_NORTH            8  /* x = p·s + q·c                                     */
#define CF_TERM_AT_CENTERS       1  /* flag for EAST / NORTH                             */
#define CF_DERIVED_MAX_SOURCES   16
typedef struct cf_average_term {
    int32_t kind, flags;
    const double* a;
    const double* b;
    double scale;
    double* mean;
} cf_average_term;
typedef struct cf_average_desc {
    int32_t struct_size, n_terms;
    const cf_average_term* terms;   /* HOST array */
    const double* cos_rotation;     /* ocean-grid layout; EAST / NORTH only */
    const double* sin_rotation;
    int32_t max_workgroups;         /* cap of a collection's launch, 0 = the library's (scheduling only, never results) */
    int32_t reserved;               /* 0 */
} cf_average_desc;
int cf_average_create_derived(cf_ctx* ctx, const cf_average_desc* desc, cf_average** out);

/* ------------------------------------------------------------------------------------------
 * The net heat and salt flux budget averaged in the collection launch: the parts of hfds and wfo that the reference's
 * `:surface` writer averages beside them — JTao, JTio, JTf, JTn, JSn, JSio (omip_diagnostics.jl:84-89,135-140) — and the
 * finer split of the atmosphere–ocean part (shortwave, longwave up / down, sensible, latent; evaporation, precipitation,
 * land).  compute_net_ocean_fluxes! forms every one of them per cell and stores only the two sums; here each is evaluated
 * again per cell inside the averager's launch from the arrays that compute_net_ocean_fluxes! itself read, and no part is
 * ever written to memory.
 *
 * cf_average_create_budget returns an ordinary cf_average: cf_average_collect / _reset / _weight / _destroy,
 * cf_attach_average and cf_attach_average_slot work on it unchanged.  Each of its n_terms (1 … CF_AVERAGE_MAX_FIELDS) names
 * one KIND of the table below and gives one SAMPLE per interior cell, which enters the recurrence of cf_average_collect in
 * place of f (the first collection of a window stores and never reads the mean):
 *     sample = x · scale        (always multiplied: scale = 1.0 is exact and keeps −0.0 and NaN)
 * The inputs are compute_net_ocean_fluxes!'s: Sₒ = ocean->S, Qs / Ql / Mp of `exchange`, Qc = fluxes->sensible_heat,
 * Qv = fluxes->latent_heat, Mv = fluxes->water_vapor, Ts = fluxes->temperature + the context's temperature offset,
 * ℵ = ice->concentration, Qio = ice->interface_heat, Jsio = ice->salt_flux, q_fr = frazil_heat, Mland = land_freshwater;
 * ℵ, Qio, Jsio, q_fr and Mland are 0.0 where their pointer (or `ice`) is NULL.  The parameters (emissivity ε, σ, albedo,
 * penetrating_shortwave, ρ_f⁻¹, ρₒ⁻¹, cₒ⁻¹, the salinity floor S_min, the wet mask's kind) are the context's
 * (cf_set_flux_params), read at each collection.  Order of operations, every product and sum rounded on its own in the
 * order written (no FMA), the intermediates exactly compute_net_ocean_fluxes!'s:
 *     om  = 1.0 − ℵ                    roc = ρₒ⁻¹ · cₒ⁻¹                 T2 = Ts · Ts
 *     Qu  = ((ε · σ) · T2) · T2        Qal = (−ε) · Ql                   Qts = ((−(1.0 − α)) · Qs) · om
 *     Qss = penetrating_shortwave ? 0.0 : Qts                            SQao = (((Qu + Qc) + Qv) + Qal) · om + Qss
 *     Fp  = (−Mp) · ρ_f⁻¹              Fe  = Mv · ρ_f⁻¹                  SFao = Fp + Fe
 *     floor = Sₒ < S_min and SFao < 0.0 (net freshening of water already at the floor: the SUM decides, not a part)
 *     SFs = floor ? 0.0 : SFao         SFl = (−Mland) · ρ_f⁻¹            SFls = (Sₒ < S_min and SFl < 0.0) ? 0.0 : SFl
 * α is the constant albedo or, with CF_ALBEDO_LATITUDE_DEPENDENT, compute_net_ocean_fluxes!'s own expression at the cell's
 * latitude (weights->latitude: per row with weights->separable, per cell otherwise) — the one device function both share.
 *
 *   kind                              x                                          reads
 *   CF_BUDGET_HEAT_SHORTWAVE          Qts · roc   (= net shortwave_surface_flux) Qs, ℵ (+ latitude)
 *   CF_BUDGET_HEAT_LONGWAVE_UP        (Qu · om) · roc                            Ts, ℵ
 *   CF_BUDGET_HEAT_LONGWAVE_DOWN      (Qal · om) · roc                           Ql, ℵ
 *   CF_BUDGET_HEAT_SENSIBLE           (Qc · om) · roc                            Qc, ℵ
 *   CF_BUDGET_HEAT_LATENT             (Qv · om) · roc                            Qv, ℵ
 *   CF_BUDGET_HEAT_ATMOSPHERE_OCEAN   SQao · roc                        JTao     Qs, Ts, Ql, Qc, Qv, ℵ (+ latitude)
 *   CF_BUDGET_HEAT_ICE_OCEAN          Qio · roc                         JTio     Qio
 *   CF_BUDGET_HEAT_FRAZIL             q_fr · roc                        JTf      q_fr
 *   CF_BUDGET_HEAT_NET                SQao · roc + Qio · roc  (= net T) JTn      those of JTao and JTio
 *   CF_BUDGET_SALT_EVAPORATION        om · ((−Sₒ) · (floor ? 0.0 : Fe))          Sₒ, Mv, Mp, ℵ
 *   CF_BUDGET_SALT_PRECIPITATION      om · ((−Sₒ) · (floor ? 0.0 : Fp))          Sₒ, Mv, Mp, ℵ
 *   CF_BUDGET_SALT_ATMOSPHERE_OCEAN   om · ((−Sₒ) · SFs)                         Sₒ, Mv, Mp, ℵ
 *   CF_BUDGET_SALT_ICE_OCEAN          Jsio                              JSio     Jsio
 *   CF_BUDGET_SALT_LAND               (−Sₒ) · SFls                               Sₒ, Mland
 *   CF_BUDGET_SALT_NET                (om · ((−Sₒ) · SFs) + Jsio) + (−Sₒ) · SFls  (= net S)   JSn    those of the three above
 * The five heat parts sum to JTao (without the shortwave under penetrating_shortwave, which leaves it out of SQao) and
 * evaporation + precipitation to SALT_ATMOSPHERE_OCEAN, each up to the roundings of the formulas; HEAT_NET and SALT_NET
 * are bit for bit what cf_compute_net_ocean_fluxes and cf_update_state store in net T and S from the same inputs, and
 * HEAT_SHORTWAVE what they store in shortwave_surface_flux.  A cell that is land by the context's mask (ocean->mask, both
 * mask kinds; no mask: none) gives the sample 0.0 · scale whatever its inputs hold.  The restoring buffer and
 * NormalizeSalinity's mean are an array and a scalar of their own and so are no kinds.
 *
 * CF_ERR_INVALID, with nothing allocated or launched: wrong struct_size; max_workgroups < 0 or reserved != 0; n_terms
 * outside 1 … CF_AVERAGE_MAX_FIELDS or terms NULL; an unknown kind or a term whose reserved is not 0; a NULL mean; a NULL
 * required input of a requested kind — Sₒ, Qs, Ql, Mp, Qc, Qv, Mv, Ts where the table's "reads" column names them (ℵ, Qio,
 * Jsio, q_fr and Mland are optional: 0.0); a non-finite scale; a mean whose parent array ((nx + 2hx)(ny + 2hy) doubles
 * from its pointer) overlaps an input that some requested kind reads, the wet mask or another mean; a kind that reads the albedo on a
 * context with CF_ALBEDO_LATITUDE_DEPENDENT and no weights->latitude (cf_average_collect also returns it, launching
 * nothing, when the parameters were changed to that later).  The descriptor, its term table and the bundles are host
 * memory, read during the call only; the device arrays they name are borrowed.
 *
 * Footprint of a collection (ONE launch for all terms; each distinct input is loaded once per cell however many terms
 * read it, and an input that no requested kind reads is never touched and may be NULL): reads on I the arrays of the
 * "reads" column of the requested kinds, the wet mask on I when the context has one, and the latitude (row j of the
 * interior with weights->separable, the cell otherwise) when a requested kind reads the albedo and it depends on
 * latitude; reads and writes the means on I (the first collection of a window only writes them).  Nothing else is read or
 * written.  The bits of every mean depend on those values, the parameters and the weights alone — not on halo widths, the
 * launched grid or on which other terms ride along.  Algorithmic bytes per cell: 8 · (distinct inputs read) + the mask's
 * 1 or 8 + 16 · n_terms accumulating, 8 · n_terms storing.
 * ---------------------------------------------------------------------------------------- */
#define CF_BUDGET_HEAT_SHORTWAVE          0
#define CF_BUDGET_HEAT_LONGWAVE_UP        1
#define CF_BUDGET_HEAT_LONGWAVE_DOWN      2
#define CF_BUDGET_HEAT_SENSIBLE           3
#define CF_BUDGET_HEAT_LATENT             4
#define CF_BUDGET_HEAT_ATMOSPHERE_OCEAN   5   /* JTao */
#define CF_BUDGET_HEAT_ICE_OCEAN          6   /* JTio */
#define CF_BUDGET_HEAT_FRAZIL             7   /* JTf  */
#define CF_BUDGET_HEAT_NET                8   /* JTn  */
#define CF_BUDGET_SALT_EVAPORATION        9
#define CF_BUDGET_SALT_PRECIPITATION      10
#define CF_BUDGET_SALT_ATMOSPHERE_OCEAN   11
#define CF_BUDGET_SALT_ICE_OCEAN          12  /* JSio */
#define CF_BUDGET_SALT_LAND               13
#define CF_BUDGET_SALT_NET                14  /* JSn  */
#define CF_BUDGET_KINDS                   15
typedef struct cf_budget_term {
    int32_t kind, reserved;         /* CF_BUDGET_*; 0 */
    double scale;
    double* mean;
} cf_budget_term;
typedef struct cf_budget_desc {
    int32_t struct_size, n_terms;
    const cf_budget_term* terms;    /* HOST array */
    const cf_ocean_surface* ocean;          /* S, mask (T, u, v are not read); any bundle may be NULL */
    const cf_exchange_fields* exchange;     /* Qs, Ql, Mp */
    const cf_interface_fluxes* fluxes;      /* sensible_heat, latent_heat, water_vapor, temperature */
    const cf_sea_ice_fields* ice;           /* concentration, interface_heat, salt_flux */
    const double* frazil_heat;
    const double* land_freshwater;
    const cf_interp_weights* weights;       /* latitude, separable: read only for the latitude-dependent albedo */
    int32_t max_workgroups;         /* cap of a collection's launch, 0 = the library's (scheduling only, never results) */
    int32_t reserved;               /* 0 */
} cf_budget_desc;
int cf_average_create_budget(cf_ctx* ctx, const cf_budget_desc* desc, cf_average** out);

/* Several attached averagers: the OMIP surface set is two averagers and its budget a third.  A context has
 * CF_ATTACHED_AVERAGES_MAX slots, each with its own stride and step weight; cf_time_steps and cf_time_steps_coupled collect
 * the occupied slots in slot order at the point where cf_attach_average's averager is collected, slot s at every step with
 * (step + 1) % stride_s == 0 and weight stride_s · step_weight_s.  Slot 0 IS cf_attach_average's slot: that call replaces
 * slot 0 and leaves the others alone.  a = NULL empties the slot; cf_average_destroy empties whichever slot holds the
 * averager.  CF_ERR_INVALID: a slot outside 0 … CF_ATTACHED_AVERAGES_MAX − 1, an averager of another context, one that
 * another slot already holds, stride < 1, a step weight that is not > 0 and finite.
 * Footprint: cf_time_steps' own, and cf_average_collect's of each occupied slot at every step it collects.              */
#define CF_ATTACHED_AVERAGES_MAX 4
int cf_attach_average_slot(cf_ctx* ctx, int32_t slot, cf_average* a, int32_t stride, double step_weight);

/* ------------------------------------------------------------------------------------------
 * Area-weighted surface integrals and their time series on the device: the scalars every reference run derives from the
 * surface — the global means of the `:averages` writer (OMIPConfigurations/omip_diagnostics.jl:194-218) and the Arctic /
 * Antarctic sea-ice volume ∫ hᵢ ℵ dA, area ∫ ℵ dA and extent ∫ [ℵ > 0.15] dA of compute_ice_diagnostics
 * (experiments/OMIPSimulations/scripts/visualize/common.jl:715-787, Integral(field; condition)).  An integrator holds the
 * weights (cell areas, wet mask, region bits), up to CF_INTEGRALS_MAX_ENTRIES entries and a series of `capacity` records in
 * device memory that the library owns.  The value of entry e in a record is
 *     Σ A · x   over the interior cells that are wet AND have bit `region_bit` set in `region`,
 *     x = 1 (CF_INTEGRAND_ONE) | a (_FIELD) | a·b (_PRODUCT; b = a gives a square) | 1 if a > threshold else 0 (_ABOVE, strict).
 * Excluded cells (land, outside the region, halos) do not contribute at all: their values are selected away, so they may
 * be NaN or Inf, the area's included.  An entry whose region is empty is exactly 0.0.  A cell may be in several regions
 * or in none.
 * One collection is one pass over the interior plus a tiny combination launch; every distinct `a` / `b` array is loaded
 * once per cell however many entries name it (at most CF_INTEGRALS_MAX_FIELDS distinct arrays): 8·(distinct fields) + 8
 * (area) + mask + 1 (region) bytes per cell.
 * Reproducibility: the bits of a record depend only on the interior values, the weights and (nx, ny) — not on the halo
 * widths or where the arrays start in memory, not on `max_workgroups` or the device's CU count, not on whether the host
 * or cf_time_steps made the collection, not on what else is attached, not on the run.  No floating-point atomics: fixed
 * tiles of 1024 consecutive interior cells (row by row) → per-tile partial sums → a fixed-order combination
 * (csrc/coflux_integrals.hip states the order).  a·b, ·A and every addition are rounded separately (no FMA).
 *   cf_integrals_create   CF_ERR_INVALID for a wrong struct_size, n_entries outside 1…CF_INTEGRALS_MAX_ENTRIES, an unknown
 *                         kind, a NULL `a` (every kind but _ONE) or NULL `b` (_PRODUCT), a region bit outside 0…7, a
 *                         non-finite threshold (_ABOVE), more than CF_INTEGRALS_MAX_FIELDS distinct arrays, max_workgroups < 0
 *                         or capacity < 1.  The pointers are borrowed: the arrays outlive the integrator.
 *   cf_integrals_destroy  detaches the integrator if it is attached; an integrator outlived by its context may still be
 *                         destroyed (every other call on it then fails).
 *   cf_integrals_collect  record number `count` is written, stream ordered, no host synchronisation; `time` is kept on the
 *                         host.  CF_ERR_INVALID, and nothing is launched or written, when the series is full.
 *   cf_integrals_count    the number of records since the last reset.
 *   cf_integrals_read     synchronises the context's stream and copies records first … first + n − 1 (n × n_entries doubles,
 *                         record-major) and their times (h_times may be NULL).  Any sub-range; reading does not consume.
 *   cf_integrals_reset    the series is empty again.  No device work.
 *   cf_attach_integrals   cf_time_steps collects `q` after the cf_update_state of every step s (global index) with
 *                         (s + 1) % stride == 0, stamped time_origin + (s + 1) · step_seconds; NULL detaches.  One integrator
 *                         per context, independent of the averager of cf_attach_average: both may be attached, the averager
 *                         collects first.  Stream order puts the collection behind every write of the step (every
 *                         CF_OPT_MERGED_PREFETCH / _HALO_IN_SOLVER_LAUNCH / _SOLVER_PATH / _FUSED_NET mode alike); a run split
 *                         into CF_PIPELINE_CONTINUING calls yields the same records as one call.  A cf_time_steps call whose
 *                         collections (they follow from first_step, nsteps and stride) would not fit the series fails with
 *                         CF_ERR_INVALID before it launches anything.  CF_ERR_INVALID for stride < 1, a non-finite time
 *                         origin or step, or an integrator of another context.
 * Each context integrates its own slab; combining slabs is the host's sum of a few doubles.
 * ---------------------------------------------------------------------------------------- */
#define CF_INTEGRALS_MAX_ENTRIES 32
#define CF_INTEGRALS_MAX_FIELDS 32
#define CF_INTEGRAND_ONE 0
#define CF_INTEGRAND_FIELD 1
#define CF_INTEGRAND_PRODUCT 2
#define CF_INTEGRAND_ABOVE 3
typedef struct cf_integral_entry {
    int32_t kind;          /* CF_INTEGRAND_* */
    int32_t region_bit;    /* 0…7: the bit of `region` a cell must carry */
    const double* a;       /* ocean-grid f64 array (every kind but _ONE) */
    const double* b;       /* _PRODUCT only */
    double threshold;      /* _ABOVE only */
} cf_integral_entry;
typedef struct cf_integrals_desc {
    int32_t struct_size;   /* sizeof(cf_integrals_desc) */
    int32_t n_entries;     /* 1…CF_INTEGRALS_MAX_ENTRIES */
    const double* area;    /* ocean-grid f64 cell areas Az; NULL: 1 */
    const void* mask;      /* wet mask of the context's mask kind (CF_MASK_U8 / _BOTTOM_HEIGHT); NULL or CF_MASK_NONE: all wet */
    const uint8_t* region; /* ocean-grid uint8 array of region bits; NULL: every cell is in region bit 0 only */
    int32_t max_workgroups; /* 0: one workgroup per tile; > 0 caps the launch (scheduling only: never a bit of a record) */
    int32_t reserved;
    cf_integral_entry entries[CF_INTEGRALS_MAX_ENTRIES];
} cf_integrals_desc;
typedef struct cf_integrals cf_integrals;
int cf_integrals_create(cf_ctx* ctx, const cf_integrals_desc* desc, int32_t capacity, cf_integrals** out);
int cf_integrals_destroy(cf_integrals* q);
/* Footprint: reads the entries' arrays, the area, the mask and the region on I; writes no caller array (the record goes to
 * the library's own series).                                                                                           */
int cf_integrals_collect(cf_integrals* q, double time);
int cf_integrals_count(cf_integrals* q, int64_t* records);
int cf_integrals_read(cf_integrals* q, int64_t first, int64_t n, double* h_values, double* h_times);
int cf_integrals_reset(cf_integrals* q);
/* Footprint: cf_time_steps' own, and cf_integrals_collect's at every collected step.                                   */
int cf_attach_integrals(cf_ctx* ctx, cf_integrals* q, int32_t stride, double time_origin, double step_seconds);

/* ------------------------------------------------------------------------------------------
 * Surface extrema, non-finite counts and state hashes on the device: what the reference's progress callback looks at on
 * every iteration — max(h), max(ℵ), extrema(T, S), maximum(u) of ClimaOcean.Progress (src/ClimaOcean.jl:48-88) and
 * omip_progress_callback (OMIPConfigurations/omip_simulation.jl:644-691), the STATE_HASH determinism probe of the latter
 * (:671-683) and the NaNChecker every Oceananigans Simulation carries.  A monitor holds up to CF_MONITOR_MAX_ENTRIES
 * entries (an ocean-grid f64 field x and a kind: y = x, or y = |x| with the sign bit cleared, so |−0| = +0, |−Inf| = +Inf)
 * and a series of `capacity` records in device memory that the library owns; one collection appends one record of
 * n_entries values of type cf_monitor_value, 64 bytes each.  Interior cell (i, j) is numbered
 * c = first_cell + j·row_length + i, where row_length = 0 stands for the context's own nx: a context that holds a whole
 * surface, or whole rows of one, leaves it 0.
 *   Order.  minimum / maximum are taken over the wet interior cells whose x is not NaN, in the IEEE total order of the
 *     non-NaN doubles: −0.0 < +0.0, and ±Inf take part.  A field that holds both zeros and nothing smaller has minimum
 *     −0.0 at the index of its first −0.0.  Ties go to the smallest c.  The device compares the order-preserving integer
 *     key of the bits (bits ^ (sign ? all ones : the sign bit)), never with floating-point min / max instructions, whose
 *     NaN and signed-zero behaviour is a mode, not a definition.  With no such cell: +Inf, −Inf, argmin = argmax = −1.
 *   Counts.  nan_count / inf_count: wet interior cells with x NaN (any sign, any payload) / x = ±Inf; first_nonfinite the
 *     smallest c of either, −1 when there is none.
 *   Land.  Excluded cells (land, halos) are selected away: a NaN, an Inf or a huge value there reaches neither the
 *     extrema nor the counts nor first_nonfinite.  u and v are masked by the wetness of the CENTRE cell (i, j), like
 *     every masked quantity of this library.
 *   Hash.  Over ALL interior cells, wet or not, of the raw bits of x (never of y; the mask does not enter):
 *         hash = Σ_c mix64(bits(x_c) XOR (K·(c + 1) mod 2⁶⁴)) mod 2⁶⁴,      K = 0x9E3779B97F4A7C15,
 *         mix64(z):  z = (z ^ z>>30) · 0xBF58476D1CE4E5B9;  z = (z ^ z>>27) · 0x94D049BB133111EB;  z ^ z>>31.
 *     Known answers: the cells [0.0, −0.0, 1.0, NaN 0x7FF8000000000000, +Inf, −1.5] with first_cell = 0 hash to
 *     0xbc9733db8e1747df, with first_cell = 1000 to 0x05c59e8be3d701d6; [0.0] to 0xe220a8397b1dcdaf; no cells to 0.
 *     For a fixed cell mix64 is a bijection of the bits: changing any single cell always changes the hash.  The library's
 *     own hash, not Julia's hash(::Array); it serves the same purpose, comparing two runs without moving a field.
 *   Exactness.  Every quantity is an exact, associative and commutative reduction (integer-key min / max with an index
 *     tie-break, integer sums, a wrapping sum): the bits of a record depend only on the interior values, the mask and
 *     first_cell and row_length — not on the launch geometry or `max_workgroups`, the halo widths, where the arrays
 *     start in memory, the device's CU count, or on whether the host or cf_time_steps made the collection.  No
 *     floating-point atomics.
 *   Slabs and tiles.  Each context monitors its own part of an Nx × Ny surface: the rank whose interior cell (0, 0) is
 *     the surface's cell (i0, j0) passes first_cell = j0·Nx + i0 and row_length = Nx (a latitude slab, i0 = 0 and
 *     nx = Nx, may leave row_length 0), so that c is the cell's number on the whole surface on every rank.  The hash is
 *     a wrapping sum: the hashes of the parts add up, mod 2⁶⁴, to the hash of the whole surface; nan_count / inf_count
 *     add; minimum / maximum combine in the same order with the smaller argmin / argmax on ties, first_nonfinite is the
 *     smallest that is not −1 — the host's combination of a few words.  With row_length = nx < Nx on a tile, c is not
 *     the global number and none of this holds.
 *   One collection is one pass per entry over the interior plus a single-workgroup combination launch: 8 bytes per cell
 *   and entry, and the mask once per ENTRY (not once per cell): n_entries · (8 + mask bytes) per cell in all.
 *   cf_monitor_create   CF_ERR_INVALID for a wrong struct_size, n_entries outside 1…CF_MONITOR_MAX_ENTRIES, a NULL `a`, an
 *                       unknown kind, max_workgroups < 0, capacity < 1, row_length < 0 or 0 < row_length < nx (the
 *                       message names the field); nothing is allocated.  The pointers are borrowed: the arrays outlive
 *                       the monitor.  The same array may be named by several entries.
 *   cf_monitor_destroy  detaches the monitor if it is attached; a monitor outlived by its context may still be destroyed
 *                       (every other call on it then fails).
 *   cf_monitor_collect  record number `count` is written, stream ordered, no host synchronisation; `time` is kept on the
 *                       host.  CF_ERR_INVALID, and nothing is launched or written, when the series is full.
 *   cf_monitor_count    the number of records since the last reset.
 *   cf_monitor_read     synchronises the context's stream and copies records first … first + n − 1 (n × n_entries values,
 *                       record-major) and their times (h_times may be NULL).  Any sub-range; reading does not consume.
 *   cf_monitor_status   synchronises the context's stream and reads 16 bytes: the index, since the last reset, of the FIRST
 *                       record in which any entry had nan_count + inf_count > 0, and the bit mask (bit e: entry e) of the
 *                       entries that did in that record; −1 and 0 when there is none.  A long cf_time_steps call is
 *                       checked without reading the series.  The status is written by one thread of the
 *                       single-workgroup combination launch: no data race.  Either output may be NULL.
 *   cf_monitor_reset    the series is empty again and the status is cleared; the clear is stream ordered.
 *   cf_attach_monitor   cf_time_steps collects `m` after the cf_update_state of every step s (global index) with
 *                       (s + 1) % stride == 0, stamped time_origin + (s + 1) · step_seconds; NULL detaches.  One monitor
 *                       per context, independent of the averager and the integrator: all three may be attached, the
 *                       monitor collects after both.  A run split into CF_PIPELINE_CONTINUING calls yields the same
 *                       records as one call.  A cf_time_steps call whose collections would not fit the series fails with
 *                       CF_ERR_INVALID before it launches anything.  CF_ERR_INVALID for stride < 1, a non-finite time
 *                       origin or step, or a monitor of another context.
 * Still ABI 5: additive.
 * ---------------------------------------------------------------------------------------- */
#define CF_MONITOR_MAX_ENTRIES 16
#define CF_MONITOR_VALUE 0   /* y = x */
#define CF_MONITOR_ABS 1     /* y = |x| (sign bit cleared): maximum(abs, u) */
typedef struct cf_monitor_entry {
    const double* a;       /* ocean-grid f64 array */
    int32_t kind;          /* CF_MONITOR_VALUE / _ABS */
    int32_t reserved;
} cf_monitor_entry;
typedef struct cf_monitor_desc {
    int32_t struct_size;   /* sizeof(cf_monitor_desc) */
    int32_t n_entries;     /* 1…CF_MONITOR_MAX_ENTRIES */
    const void* mask;      /* wet mask of the context's mask kind (CF_MASK_U8 / _BOTTOM_HEIGHT); NULL or CF_MASK_NONE: all wet */
    int64_t first_cell;    /* global index of this slab's or tile's interior cell (0, 0): j0·Nx + i0 */
    int32_t max_workgroups; /* 0: the library's choice; > 0 caps the launch (scheduling only: never a bit of a record) */
    int32_t row_length;    /* 0: nx; else the global row length Nx ≥ nx (it took the place of a reserved word: additive) */
    cf_monitor_entry entries[CF_MONITOR_MAX_ENTRIES];
} cf_monitor_desc;
typedef struct cf_monitor_value {   /* 64 bytes */
    double minimum;           /* of y over the wet interior cells whose x is not NaN; +Inf when there is none */
    double maximum;           /* −Inf when there is none */
    int64_t argmin;           /* the SMALLEST c that holds the minimum; −1 when there is none */
    int64_t argmax;
    int64_t nan_count;        /* wet interior cells with x NaN */
    int64_t inf_count;        /* … with x = ±Inf */
    int64_t first_nonfinite;  /* the smallest c of those; −1 */
    uint64_t hash;            /* over ALL interior cells, wet or not, of the raw bits of x */
} cf_monitor_value;
typedef struct cf_monitor cf_monitor;
int cf_monitor_create(cf_ctx* ctx, const cf_monitor_desc* desc, int32_t capacity, cf_monitor** out);
int cf_monitor_destroy(cf_monitor* m);
/* Footprint: reads the entries' arrays and the mask on I; writes no caller array (the record goes to the library's own
 * series).                                                                                                             */
int cf_monitor_collect(cf_monitor* m, double time);
int cf_monitor_count(cf_monitor* m, int64_t* records);
int cf_monitor_read(cf_monitor* m, int64_t first, int64_t n, cf_monitor_value* h_values, double* h_times);
int cf_monitor_status(cf_monitor* m, int64_t* first_bad_record, uint32_t* bad_entries);
int cf_monitor_reset(cf_monitor* m);
/* Footprint: cf_time_steps' own, and cf_monitor_collect's at every collected step.                                     */
int cf_attach_monitor(cf_ctx* ctx, cf_monitor* m, int32_t stride, double time_origin, double step_seconds);

/* ------------------------------------------------------------------------------------------
 * Calendar-binned means of surface fields on the device: the monthly climatologies under every monthly figure of a
 * reference analysis — compute_monthly_means / compute_mean_and_monthly (experiments/OMIPSimulations/scripts/visualize/
 * common.jl:176-208) add each saved sample into one of twelve calendar-month bins and into a total, the month being
 * month(reference_date + Second(round(Int, t))); the March / September sea-ice maps (visualize/cache.jl:634-686) and the
 * per-cell minimum / maximum over the available months, reduce_monthly (cache.jl:696-712), sit on top.  A climatology
 * holds up to CF_CLIMATOLOGY_MAX_FIELDS fields; per field a source, an optional TOTAL mean and a block of n_bins
 * (1 … CF_CLIMATOLOGY_MAX_BINS) BIN means, every one an ocean-grid f64 array in the usual halo layout; bin b of field f
 * starts (nx + 2hx)(ny + 2hy) · b doubles into bins[f].  Still ABI 5: additive.
 *   Collection.  cf_climatology_collect of (bin, weight) is ONE launch over the interior I of every field: the source is
 *     loaded once per cell and enters two running means by the recurrence of cf_average_collect, each with its OWN
 *     coefficients computed on the host in double — the total's from the weight of every collection since the reset,
 *     bin `bin`'s from the weight that bin has received.  The total stores without reading on the first collection since
 *     the reset, the bin stores without reading on ITS first collection (a fresh buffer may hold NaNs); no other bin is
 *     touched.  bin = −1: nothing is collected — no launch, no weight changes (a sample outside the analysis window).
 *   Contract.  After any sequence of collections the total holds, bit for bit, what a cf_average collecting the same
 *     samples and weights holds, and bin b what a cf_average collecting only bin b's subsequence holds.  The bits do not
 *     depend on the halo widths, where the arrays start in memory, the launched grid (`max_workgroups`), or which other
 *     fields ride along.
 *   Footprint of a collection: reads the sources on I; reads and writes — or, where it stores, only writes — the totals
 *     and the one bin on I.  Nothing else is accessed: the halos of every mean, the gaps between the bins of a block and
 *     all other bins included.  40 algorithmic bytes per cell and field when both accumulate, 24 when both store.
 *   Extremes.  cf_climatology_extremes is one launch for one field: per interior cell the minimum and maximum over the bins
 *     that have at least one sample, taken in ascending bin order with Julia's min / max (what reduce_monthly applies): a NaN
 *     in any non-empty bin gives NaN (its payload is not part of the contract), −0.0 < +0.0.  d_argmin / d_argmax (int32
 *     arrays indexed like the halo layout) receive the smallest bin index that attains the result, or the first NaN bin.
 *     Any of the four outputs may be NULL; only I of an output is written.  Empty bins are never read: they may be poison.
 *     CF_ERR_INVALID when every bin is empty (the reference raises "has no available monthly bins").
 *   Calendar.  A table is n_edges strictly increasing times `edges` [s]; interval k = [edges[k], edges[k+1]) carries
 *     bin_of_interval[k] in −1 … n_bins − 1 (−1: not collected — how a start_time / stop_time window is expressed).  The
 *     lookup rounds first, as the reference does: t_r = rint(time), ties to even (Julia's round(Int, ·)), then finds k with
 *     edges[k] ≤ t_r < edges[k+1].  cf_calendar_bin is that lookup as a pure host function (no context, no device): a time
 *     outside the table — below edges[0], at or beyond the last edge, or not finite — is CF_ERR_INVALID, and so are
 *     n_edges < 2, a NULL argument, edges that are not strictly increasing and finite, and an interval bin below −1.
 *   cf_attach_climatology copies the table.  cf_time_steps and cf_time_steps_coupled then collect `c` at every step s
 *     (global index) with (s + 1) % stride == 0, stamped time_origin + (s + 1) · step_seconds (cf_attach_integrals' clock),
 *     into the bin the lookup gives, with weight stride · step_weight — after the averager slots, before the integrator and
 *     the monitor.  One climatology per context; NULL detaches; cf_climatology_destroy detaches too.  A call any of whose
 *     collected steps falls outside the table fails with CF_ERR_INVALID before it launches anything.  A run split into
 *     CF_PIPELINE_CONTINUING calls collects what one call collects.  With nothing attached the step loops issue exactly the
 *     launches they issued before.
 *   Errors (CF_ERR_INVALID, nothing allocated or launched).  create: a wrong struct_size, n_fields outside
 *     1 … CF_CLIMATOLOGY_MAX_FIELDS, n_bins outside 1 … CF_CLIMATOLOGY_MAX_BINS, a NULL source or bins, a total or a bin
 *     block whose bytes (a parent array; n_bins parent arrays) overlap a source's parent array or another output,
 *     max_workgroups < 0, reserved != 0.  collect: a bin outside −1 … n_bins − 1, a weight that is not > 0 and finite.
 *     extremes: a field outside 0 … n_fields − 1, every bin empty.  attach: a climatology of another context, stride < 1,
 *     a step weight that is not > 0 and finite, a non-finite origin or step, a bad table (above) or an interval bin beyond
 *     n_bins − 1.  A climatology outlived by its context may still be destroyed; every other call on it fails.
 *   cf_climatology_reset   all weights 0: the next collection stores into the total and into its bin.  No device work.
 *   cf_climatology_weights the total weight and collection count since the reset, and per bin (arrays of n_bins); any
 *                          pointer may be NULL.  Host bookkeeping only.
 * Slabs: each context bins its own rows; there is nothing to combine.  Only fields that exist are binned (no derived or
 * budget terms), and the calendar is the caller's table (coflux.models.calendar_bins builds the proleptic Gregorian one).
 * ---------------------------------------------------------------------------------------- */
#define CF_CLIMATOLOGY_MAX_FIELDS 16
#define CF_CLIMATOLOGY_MAX_BINS 32
typedef struct cf_climatology_desc {
    int32_t struct_size;      /* sizeof(cf_climatology_desc) */
    int32_t n_fields;         /* 1…CF_CLIMATOLOGY_MAX_FIELDS */
    int32_t n_bins;           /* 1…CF_CLIMATOLOGY_MAX_BINS */
    int32_t max_workgroups;   /* 0: the library's choice; > 0 caps the launch (scheduling only: never a bit of a result) */
    const double* sources[CF_CLIMATOLOGY_MAX_FIELDS];   /* ocean-grid f64, halo layout, borrowed */
    double* totals[CF_CLIMATOLOGY_MAX_FIELDS];          /* mean over every collected sample; NULL: this field keeps no total */
    double* bins[CF_CLIMATOLOGY_MAX_FIELDS];            /* n_bins parent arrays back to back */
    int32_t reserved[2];
} cf_climatology_desc;
typedef struct cf_climatology cf_climatology;
int cf_climatology_create(cf_ctx* ctx, const cf_climatology_desc* desc, cf_climatology** out);
int cf_climatology_destroy(cf_climatology* c);
int cf_climatology_reset(cf_climatology* c);
/* Footprint: reads the sources on I; reads and writes (or only writes) the totals and bin `bin` on I.  Nothing else.   */
int cf_climatology_collect(cf_climatology* c, int32_t bin, double weight);
int cf_climatology_weights(cf_climatology* c, double* total, int64_t* samples, double* bin_totals, int64_t* bin_samples);
/* Footprint: reads the non-empty bins of `field` on I; writes the outputs that are not NULL on I.                      */
int cf_climatology_extremes(cf_climatology* c, int32_t field, double* d_min, double* d_max, int32_t* d_argmin, int32_t* d_argmax);
int cf_calendar_bin(const double* edges, const int32_t* bin_of_interval, int32_t n_edges, double time, int32_t* bin);
/* Footprint: the step loops' own, and cf_climatology_collect's at every collected step.                                */
int cf_attach_climatology(cf_ctx* ctx, cf_climatology* c, int32_t stride, double step_weight, double time_origin,
                          double step_seconds, const double* edges, const int32_t* bin_of_interval, int32_t n_edges);

/* ------------------------------------------------------------------------------------------
 * A dataset staged on the device and followed in time: what salinity_surface_restoring builds —
 * DatasetRestoring(Metadata(:salinity; dataset = WOAMonthly()), …; time_indices_in_memory = length(Smetadata))
 * (omip_simulation.jl:507-523): twelve monthly fields, all resident, each land-inpainted on the dataset's own
 * latitude–longitude grid, interpolated to the ocean grid and blended linearly in time, cyclically over the year — and what
 * set!(T_init, Metadatum(…)) does for the initial conditions (omip_simulation.jl:614-615, :634-635; n_levels = 1).
 * Still ABI 5: additive.  A dataset owns two f64 planes of the source grid and n_levels ocean-grid f64 arrays in the usual
 * halo layout, zero-filled at create.
 *   Staging.  cf_dataset_stage(d, level, h_plane) takes a host float[ns_y][ns_x], NaN = missing (the caller has mapped
 *     _FillValue to NaN), and queues on the context's stream:
 *       convert   the plane to f64, exactly;
 *       inpaint   [UPSTREAM-RECALL inpaint_mask!, NearestNeighborInpainting; the definition here is this library's contract]
 *                 one sweep reads plane p and writes plane q.  A cell that is not NaN is copied.  A NaN cell looks at its donors
 *                 in the fixed order W (i − 1), S (j − 1), E (i + 1), N (j + 1); W and E wrap when periodic_x and are absent at
 *                 the edge otherwise, S and N are absent beyond the first and last row.  With c ≥ 1 donors that are not NaN in
 *                 p, q = (those donors added left to right in that order, starting from the first valid one) / (double)c in
 *                 plain IEEE arithmetic (no contraction); with none q stays NaN.  The number of sweeps is
 *                 min(max_sweeps, depth), depth = the largest 4-connected distance of a NaN cell from the nearest cell that is
 *                 not NaN (x wraps when periodic) — the host holds the plane and finds it by one breadth-first pass, so
 *                 exactly that many sweeps are queued: no device counter, no test of the plane, no synchronisation.  Cells
 *                 still NaN afterwards (beyond max_sweeps; a plane with no valid cell) become fill_value.  A plane without
 *                 NaN launches no sweep.  (An Inf is a valid donor.  Donors that sum to NaN — infinities of both signs — leave
 *                 a NaN the sweep count does not know of: it stays in the plane, and stage_info counts the cell as filled.)
 *                 sweeps_per_launch: 1 = one launch per sweep over the plane; 2 … 8 = that many sweeps per launch on
 *                 overlapped LDS tiles (core + a halo of as many cells, wrapped or cut at the plane's edges; only the core is
 *                 written back); 0 = the library's choice.  Same bits either way, and on any max_workgroups.
 *       regrid    bilinear interpolation of the inpainted f64 plane onto the ring window W of the level's array through
 *                 `weights` (fi / fj index the dataset's grid: periodic x, clamped y — cf_interpolate_land_freshwater's index
 *                 arithmetic, no time blend).  Cells outside W keep their zeros.
 *     The only host wait is for the upload of the stage call two before, should it still be in flight (two pinned slots).
 *   Clock.  cf_dataset_time_index is a pure host function (no context, no device).  Cyclical (period > 0):
 *     r = fmod(time − times[0], period), + period when r < 0; τ = times[0] + r; k with times[k] ≤ τ < times[k+1] gives
 *     (k, k+1, (τ − times[k]) / (times[k+1] − times[k])); τ ≥ times[n−1] gives (n−1, 0, (τ − times[n−1]) / (times[0] + period −
 *     times[n−1])).  Clamped (period == 0): below times[0] (0, 0, 0.0), at or beyond times[n−1] (n−1, n−1, 0.0).  n == 1:
 *     always (0, 0, 0.0).  CF_ERR_INVALID for a time that is not finite or a bad table (times not finite or not strictly
 *     increasing, n < 1, a period that is negative, not finite, or > 0 but not above times[n−1] − times[0], a NULL argument).
 *   Evaluation.  S★ at a cell is level1's value when the fraction is 0.0 (level2 is not read), else b·f + a·(1 − f) in f64.
 *     cf_dataset_evaluate writes it on W of d_out (a Metadatum initial condition: n_levels = 1).
 *     cf_materialize_dataset_restoring is cf_materialize_salinity_restoring with S★ formed per cell: bit for bit
 *     cf_dataset_evaluate followed by cf_materialize_salinity_restoring on that array, without the array.
 *   cf_attach_restoring_dataset(ctx, d, time_origin, step_seconds): while attached, step s (global index) of
 *     cf_time_steps_coupled runs its restoring job at time_origin + s · step_seconds — the time of the ocean state it reads —
 *     inside the preamble's one launch: one more 8-byte load per wet cell on steps between two levels, no extra launch; a step
 *     whose fraction is 0.0 runs the static target's own form on that level.  cf_coupled_step.target_salinity must then be
 *     NULL (both given: CF_ERR_INVALID before anything is launched); with nothing attached a NULL target is refused as before.
 *     A block without restoring_buffer has no restoring job and does not look at the dataset.  cf_time_steps ignores the
 *     attachment.  The clock is the global step index and the dataset has no state that moves, so a run split into
 *     CF_PIPELINE_CONTINUING calls, or across a checkpoint and pickup, restores toward the same bits.  One dataset per context;
 *     NULL detaches; cf_dataset_destroy detaches too.
 *   Accessors.  cf_dataset_level: a borrowed device pointer to a level's ocean-grid array.  cf_dataset_read_source: the
 *     inpainted f64 plane of the most recently staged level into h_out[ns_y][ns_x]; synchronises (tests and debugging).
 *     cf_dataset_stage_info: host bookkeeping of a staged level — sweeps queued, cells filled by a sweep, cells given fill_value.
 *   Errors (CF_ERR_INVALID, nothing allocated or launched): a wrong struct_size, ns_x or ns_y < 2 or more than 2³¹ cells,
 *     n_levels outside 1 … CF_DATASET_MAX_LEVELS, sweeps_per_launch outside 0 … 8, max_workgroups < 0, a fill_value that is
 *     NaN, a bad times table or period, weights without fi / fj, a NULL plane, a level out of range, a dataset of another
 *     context, evaluation / materialisation / attachment / a coupled call before every level is staged, a non-finite clock.
 * Slabs: each context stages its own rows through its own weights; there is nothing to combine.
 * ---------------------------------------------------------------------------------------- */
#define CF_DATASET_MAX_LEVELS 32
typedef struct cf_dataset_desc {
    int32_t struct_size;        /* sizeof(cf_dataset_desc) */
    int32_t ns_x, ns_y;         /* the dataset's own grid, ≥ 2 each */
    int32_t n_levels;           /* 1 … CF_DATASET_MAX_LEVELS */
    int32_t periodic_x;         /* 1: W / E donors wrap in x */
    int32_t max_sweeps;         /* < 0: no limit */
    int32_t sweeps_per_launch;  /* 0: the library's choice; 1 … 8 (scheduling only: never a bit of a result) */
    int32_t max_workgroups;     /* 0: the library's choice; > 0 caps every launch (scheduling only) */
    double fill_value;          /* what cells no sweep reached receive */
    double period;              /* 0: clamped; else cyclical, above times[n_levels − 1] − times[0] */
    const double* times;        /* host, n_levels finite strictly increasing level times; copied */
    cf_interp_weights weights;  /* this context's grid → the dataset's grid, separable or 2-D; device arrays, borrowed */
} cf_dataset_desc;
typedef struct cf_dataset cf_dataset;
int cf_dataset_create(cf_ctx* ctx, const cf_dataset_desc* desc, cf_dataset** out);
int cf_dataset_destroy(cf_dataset* d);
/* Footprint: reads h_plane in full and fi / fj as the atmosphere does; writes the level's array on W.                  */
int cf_dataset_stage(cf_dataset* d, int32_t level, const float* h_plane);
int cf_dataset_level(cf_dataset* d, int32_t level, const double** d_field);
int cf_dataset_read_source(cf_dataset* d, double* h_out);
int cf_dataset_stage_info(cf_dataset* d, int32_t level, int32_t* sweeps, int64_t* filled, int64_t* defaulted);
int cf_dataset_time_index(const double* times, int32_t n, double period, double time, int32_t* level1, int32_t* level2, double* fraction);
/* Footprint: reads one or two levels on W; writes d_out on W only.                                                     */
int cf_dataset_evaluate(cf_dataset* d, double time, double* d_out);
/* Footprint: reads one or two levels, S, mask on I; writes d_buffer on I only (0 on land).                             */
int cf_materialize_dataset_restoring(cf_ctx* ctx, double piston_velocity /* m/s */, cf_dataset* d, double time,
                                     const cf_ocean_surface* ocean, double* d_buffer);
int cf_attach_restoring_dataset(cf_ctx* ctx, cf_dataset* d, double time_origin, double step_seconds);

/* ------------------------------------------------------------------------------------------
 * A fixed sparse surface operator applied on the device: the conservative regridding of surface fields onto the shared
 * 360 × 180 latitude–longitude grid behind every figure of a reference run (regrid_surface_to_latlon,
 * experiments/OMIPSimulations/scripts/visualize/cache.jl:983-1011, applied to SURFACE_LATLON_FIELDS, :1026-1042) and its
 * zonal means (compute_zonal_mean, cache.jl:918-937).  Both are one sparse matrix applied to `field · mask` and to `mask`
 * and a division; the operator is fixed per grid, the apply runs for every field of every record.  Still ABI 5: additive.
 * The operator is CSR over destination rows: row r owns entries row_ptr[r] … row_ptr[r + 1] − 1, entry k names the source
 * cell col[k] = j·nx + i of the interior (the numbering of the surface integrals) with weight[k] ≥ 0.  Empty rows and
 * repeated columns within a row are legal.  With W(r) the entries of row r whose source cell is wet,
 *     D = Σ_{k∈W} weight[k],        N_f = Σ_{k∈W} weight[k] · src_f[col[k]],        coverage[r] = D,
 *     dst_f[r] = N_f / D, NaN where D == 0 (CF_REGRID_MEAN: cache.jl:1006-1009) | N_f, exactly +0.0 for an empty or all-land
 *     row (CF_REGRID_SUM).
 * Excluded entries (land) are selected away, never multiplied by zero: a land cell's field value may be NaN or Inf; a NaN
 * in a wet cell propagates.  One apply serves up to CF_REGRID_MAX_FIELDS fields in one pass: the entry's column, weight and
 * mask byte are loaded once for all of them and each field costs one 8-byte gather per entry —
 * nnz · (13 + 8 K) + 8 · n_rows · (K + 1) algorithmic bytes for K fields.
 * Reproducibility: weight·x, every addition and the division are rounded separately (no FMA), there are no floating-point
 * atomics, and THE SUMMATION ORDER OF A ROW IS A FUNCTION OF THAT ROW'S ENTRY COUNT n ALONE (land entries keep their place
 * and add a selected +0.0):
 *     n ≤ 64: 16 lanes; lane g adds entries g, g + 16, g + 32, g + 48 in that order to +0.0 (an absent entry adds +0.0), the
 *             lanes are combined by the butterfly v += shfl_xor(v, 8), 4, 2, 1;
 *     n > 64: segments of 256 consecutive entries; in a segment lane l of 64 adds its entries l, l + 64, l + 128, l + 192 to
 *             +0.0, then the butterfly 32 … 1; the segment partials are added in segment order, ((p₀ + p₁) + p₂) + ….
 * D is summed in the same order (csrc/coflux_regrid.hip).  The bits of dst_f[r] therefore depend only on the row's (col,
 * weight) in the order given, the mask and the interior values — not on the row's index or its neighbours in the operator,
 * the halo widths or where the arrays start in memory, `max_workgroups` or the device's CU count, n_fields or which other
 * fields ride along, or the run.
 *   cf_regrid_create   copies the operator to the device (the host arrays may be freed afterwards; `mask` is borrowed and
 *                      read at every apply).  CF_ERR_INVALID, with nothing allocated or launched, for a wrong struct_size,
 *                      n_rows < 1, nnz < 0, n_rows or nnz ≥ 2³¹, a NULL row_ptr (or NULL col / weight with nnz > 0),
 *                      row_ptr[0] != 0, a row_ptr that is not monotone, row_ptr[n_rows] != nnz, a column outside
 *                      0 … nx·ny − 1, a negative or non-finite weight, an unknown mode or max_workgroups < 0.
 *   cf_regrid_apply    stream ordered on the context's stream, no host synchronisation.  `src` and `dst` are HOST arrays of
 *                      n_fields device pointers.  CF_ERR_INVALID, and nothing is launched or written, for n_fields outside
 *                      1 … CF_REGRID_MAX_FIELDS or a NULL array or entry of `src` / `dst`; `coverage` may be NULL.
 *   cf_regrid_destroy  a regridder outlived by its context may still be destroyed (an apply on it fails).
 * Slabs: each context applies the operator restricted to its own columns (renumbered to its interior) in CF_REGRID_SUM mode
 * with `coverage`; the host adds the per-slab numerators and coverages and divides.  The library does not combine slabs.
 * ---------------------------------------------------------------------------------------- */
#define CF_REGRID_MAX_FIELDS 16
#define CF_REGRID_MEAN 0
#define CF_REGRID_SUM 1
typedef struct cf_regrid_desc {
    int32_t struct_size;     /* sizeof(cf_regrid_desc) */
    int32_t mode;            /* CF_REGRID_MEAN / CF_REGRID_SUM */
    int64_t n_rows;          /* destination cells, ≥ 1 */
    int64_t nnz;             /* entries, = row_ptr[n_rows] */
    const int64_t* row_ptr;  /* HOST, n_rows + 1 entries, non-decreasing, row_ptr[0] = 0 */
    const int32_t* col;      /* HOST, nnz interior cell numbers c = j·nx + i */
    const double* weight;    /* HOST, nnz weights, finite and ≥ 0 */
    const void* mask;        /* DEVICE wet mask of the context's mask kind (CF_MASK_U8 / _BOTTOM_HEIGHT); NULL or CF_MASK_NONE: all wet */
    int32_t max_workgroups;  /* 0: automatic; > 0 caps the launch (scheduling only: never a bit of a result) */
    int32_t reserved;
} cf_regrid_desc;
typedef struct cf_regrid cf_regrid;
int cf_regrid_create(cf_ctx* ctx, const cf_regrid_desc* desc, cf_regrid** out);
int cf_regrid_destroy(cf_regrid* rg);
/* Footprint: reads every src[f] and the mask on I only (at the cells the operator names); writes exactly n_rows doubles of
 * every dst[f] and, unless it is NULL, of coverage.                                                                     */
int cf_regrid_apply(cf_regrid* rg, int32_t n_fields, const double* const* src, double* const* dst, double* coverage);

/* Builds the flux solver's schedule for `mask` (the cost-balanced chunk table and the wet lists, three tiny kernels and
 * two 4-byte read-backs) ahead of the first step instead of inside it.  Optional: cf_compute_atmosphere_ocean_fluxes,
 * cf_update_state and cf_time_steps build it on first use and whenever the mask pointer, its kind or the surface z
 * changes.  A mask rewritten in place keeps the old schedule: slower at worst, never wrong.                          */
int cf_ensure_chunk_table(cf_ctx* ctx, const void* mask);

/* Which kernels cf_update_state launches for the context's current formulation and options (a measurement aid:
 * bench.py names the dominant kernel and its algorithmic bytes from it).  *lean_kernel = 1: the round-3 ocean kernel
 * (coflux_solver_lean.hip), 0: the general solver; *fused_net = 1: the solver's epilogue also writes the cell-local net
 * ocean fluxes and a face-stress kernel follows (2: and interpolates the atmosphere state in its prologue), 0:
 * compute_net_ocean_fluxes! is its own launch.                                                                       */
int cf_solver_path(cf_ctx* ctx, int* lean_kernel, int* fused_net);

/* The pipelined form of update_state! for callers that drive the steps themselves: start the interpolation of the
 * NEXT step's atmosphere state into `out` on the auxiliary stream now; the next cf_update_state whose (levels, time
 * fraction, exchange fields) match finds it done (it waits on an event instead of launching the interpolation).
 * `out` must not be the set the current step's kernels still read.  cf_update_state's signature — the reference
 * seam — is unchanged.
 * The life of a request.  It is PENDING from this call on, and ends in exactly one of five ways:
 *   consumed    the next cf_update_state / cf_update_state_sea_ice into `out` asks for the same interpolation — the same source
 *               (its nine data pointers, ns_x, ns_y, n_levels), the same level1, level2 and time_fraction, and the same weights
 *               (every pointer of cf_interp_weights and `separable`): the step does not interpolate.
 *   mismatched  that step asks for anything else: it is ordered behind the request's kernel and interpolates itself.
 *   voided      cf_window_commit rewrites a slot whose NUMBER is level1 or level2 of the request (of whichever source: a false
 *               void only costs an interpolation).  The next step into `out` interpolates itself, from the new contents.
 *   superseded  a later request into the same `out` arrives first.
 *   discarded   cf_discard_prefetched_atmosphere_state.
 * A step into another exchange set leaves the request pending.  At most one request per exchange set and two in all are
 * pending: a request into a third set while two others are pending is refused with CF_ERR_INVALID before anything is launched
 * or booked for it, and the two stay pending (one of them that has not left yet leaves on the auxiliary stream, as it does
 * before any new request).  While a request is pending the host writes neither `out` nor the source levels it
 * reads, other than by cf_window_commit.
 * Where the kernel runs does not change a bit of any result, and depends on CF_OPT_MERGED_PREFETCH at the moment the request
 * LEAVES, not when it was made.  It leaves with the next step into another set than `out`:
 *   0  on the auxiliary stream, right behind that step's solver launch;
 *   1  inside that step's face-stress launch, with or without sea ice (CF_OPT_FUSED_NET ≠ 0 and the default solver);
 *   2  as tail workgroups of that step's solver launch (cf_update_state, CF_OPT_FUSED_NET ≠ 0 and the default solver), or in
 *      the tail of the sea-ice interface launch (cf_update_state_sea_ice, whatever CF_OPT_FUSED_NET says);
 *   1 or 2 where that form does not apply: a launch of its own on the context's stream behind the step.  That is with
 *      CF_OPT_FUSED_NET = 0 (but for the sea-ice tail), and wherever the tiled interpolation's tile — 4 waves × 9 variables ×
 *      CF_OPT_INTERP_TILE_CAP doubles of LDS (default 128 cells; an experiment option) — does not fit the launch that would carry
 *      it: 64 KiB in the face-stress launch (every cap but 0, which turns the tiled interpolation off), 40 KiB in the tail
 *      workgroups of either solver launch (a cap of 1 … 142 cells).  CF_OPT_INTERP_TILE_ROWS does not enter.
 * Before such a step it leaves on the auxiliary stream when cf_sync is called, when another request is made, or when the next
 * step is into `out` itself.  cf_debug_prefetch_stats counts every one of these.                                        */
int cf_prefetch_atmosphere_state(cf_ctx* ctx, const cf_atmos_source* src_next, const cf_interp_weights* w,
                                 const cf_exchange_fields* out);
/* Forget every atmosphere state that was requested ahead and not consumed (cf_prefetch_atmosphere_state, cf_time_steps with
 * CF_PIPELINE_CONTINUING): a caller that leaves its stepping loop, overwrites an exchange set that holds such a state, or
 * changes the clock calls this so that no later cf_update_state mistakes the set's contents for the state it asks for.
 * An interpolation already running on the auxiliary stream is ordered ahead of whatever follows on the context's stream. */
int cf_discard_prefetched_atmosphere_state(cf_ctx* ctx);

/* Self-test hook (host bookkeeping only, launches nothing, changes no state): which way every atmosphere state requested ahead
 * went since cf_create — requests of cf_prefetch_atmosphere_state and of a pipelined cf_time_steps alike (which makes one per
 * step but the first of a call that finds its state pending, and under CF_PIPELINE_CONTINUING one more for the step behind its
 * last).  Every accepted request leaves at most once (the launched_* counters) and ends exactly once, so at every point
 *   requests = consumed + mismatched + voided + superseded + discarded + pending.
 * Set struct_size = sizeof(cf_prefetch_stats) before the call.                                                          */
typedef struct cf_prefetch_stats {
    int32_t struct_size;
    int32_t pending;               /* requests neither ended nor refused, launched or not (0, 1 or 2) */
    uint64_t requests;             /* accepted */
    uint64_t launched_aux;         /* left on the auxiliary stream */
    uint64_t launched_tail;        /* … as tail workgroups of an ocean solver launch */
    uint64_t launched_merged;      /* … inside a face-stress launch */
    uint64_t launched_ice_tail;    /* … in the tail of a sea-ice interface launch */
    uint64_t launched_own;         /* … as a launch of its own on the context's stream */
    uint64_t consumed, mismatched, voided, superseded, discarded;   /* how they ended (cf_prefetch_atmosphere_state) */
    uint64_t step_interpolations;  /* interpolations cf_update_state / _sea_ice launched for their own step */
} cf_prefetch_stats;
int cf_debug_prefetch_stats(cf_ctx* ctx, cf_prefetch_stats* out);

/* ------------------------------------------------------------------------------------------
 * Checkpoint and pickup: every production launch of the reference ends in run!(sim; pickup = true) (experiments/
 * OMIPSimulations/scripts/launch.sh:154-173, omip_simulation.jl:241-247) and add_omip_diagnostics! always installs a
 * Checkpointer (omip_diagnostics.jl:220-225).  A checkpoint handle packs device arrays of the caller and the library-private
 * state of averagers, climatologies, integrators and monitors into one self-describing byte string, and puts such an image
 * back.  A run split in two PROCESSES by capture → restore yields, bit for bit, what the unsplit run yields.  The format is
 * this library's own (not JLD2).  Still ABI 5: additive.
 *   Registration.  Sections are named (1 … 47 bytes, unique per handle); their order is the caller's and part of the image; at
 *     most CF_CHECKPOINT_MAX_SECTIONS.  cf_checkpoint_add_array: a caller-owned device array, `bytes` long (any length, 0
 *     included), base 8-byte aligned, borrowed — whole parent arrays, halos included; an array that shares a byte with an
 *     earlier array section is CF_ERR_INVALID.  cf_checkpoint_add_average / _climatology / _integrals / _monitor: a handle of
 *     the same context (borrowed: it outlives the checkpoint handle), each at most once; what goes into the image is
 *       average      total (f64), samples (i64)
 *       climatology  weight, samples, bin_weight[n_bins] (f64), bin_samples[n_bins] (i64)
 *       integrals    records [count][n_entries] f64 from the device, zero padded to 16 bytes, then times[count]
 *       monitor      the 16-byte status and the records [count][n_entries] × 64 bytes from the device, then times[count]
 *     The arrays those handles write into (means, totals, bin blocks) are the caller's: register them as arrays.
 *     cf_checkpoint_set_host_blob: opaque caller bytes carried in the image (copied at the call; clocks, schedules).
 *   Image, little endian.  Header, 96 bytes: magic "CFLXCKPT" | u32 version (1) | u32 n_sections | u64 total_bytes | i32 nx, ny,
 *     hx, hy | u64 directory_hash (the section hash of the directory's bytes) | u64 blob_bytes | u64 blob_offset | u64
 *     blob_hash | 16 reserved zero bytes | u64 header_hash (of the 88 bytes before it).  Directory: one 96-byte entry per
 *     section: name[48] NUL padded | u32 kind (0 array, 1 average, 2 climatology, 3 integrals, 4 monitor) | u32 n_entries
 *     (climatology: n_bins; arrays, averages: 0) | u64 payload bytes | u64 payload offset | u64 hash | i64 count (records of a
 *     series, else 0) | 8 reserved zero bytes.  Then the payloads in directory order, each at the next multiple of 16 and
 *     zero padded to one, then the host blob likewise; total_bytes ends there.  An image has exactly one encoding.
 *   Section hash.  hash = Σ_k mix64(w_k XOR (K·(k + 1) mod 2⁶⁴)) mod 2⁶⁴ over the payload's 8-byte little-endian words w_k, the
 *     last one zero padded; K and mix64 are the surface monitor's (above).  Known answers: the doubles [0.0, −0.0, 1.0, NaN
 *     0x7FF8000000000000, +Inf, −1.5] hash to 0xbc9733db8e1747df (the monitor's), [0.0] to 0xe220a8397b1dcdaf, no bytes to 0,
 *     the bytes 01 02 … 0b to 0x21e51a3dd06edc89, the byte 01 to 0xe4d971771b652c20.  cf_checkpoint_hash is that function on
 *     the host.
 *   cf_checkpoint_capture  stream ordered on the context's stream, no host synchronisation.  The host-kept state (weights,
 *     counts, times, the blob) is copied at the call; ONE launch packs every device byte into a device staging image and forms
 *     every section's hash (wrapping 64-bit sums: lane → wave → one integer atomic per section and workgroup; the bits depend
 *     on the bytes alone, never on max_workgroups, the tile size, the CU count or the form); the image then drains to a pinned
 *     host buffer on a stream the handle owns, behind an event: steps issued after the call run meanwhile and cannot change
 *     the image.  Staging and pinned buffers are sized by the first capture — with every registered series at its
 *     capacity, so that a filling series never makes a later capture allocate — and reused.  With CF_CHECKPOINT_DIRECT there is
 *     no staging image (no extra device memory): the same kernel forms the hashes only and the sections are copied to the
 *     pinned image one by one on the CONTEXT's stream, which holds later steps back for as long.  Both forms give the same
 *     bytes.  A second capture before cf_checkpoint_wait is CF_ERR_INVALID.
 *   cf_checkpoint_wait     synchronises the drain only, completes the image (header, directory, host-kept bytes) and hands
 *     out the pinned image: valid until the next capture, restore or destroy.  Either output may be NULL.
 *   cf_checkpoint_verify   a pure host function (no context, no device): the magic, the version, the total length, the header's,
 *     the directory's, every section's and the blob's hash, every name (terminated, unique), kind, n_entries / count / payload
 *     size combination, every offset and length against the image size without overflow, and that all padding is zero.
 *     CF_ERR_INVALID with a message that names the header field or the section.  cf_checkpoint_host_blob verifies likewise and
 *     points at the blob inside the image.
 *   cf_checkpoint_restore  refuses — CF_ERR_INVALID, the message names the section, nothing written or launched — an image
 *     that fails the verification, another grid (nx, ny, hx, hy), a directory that differs from the registration in number,
 *     name, kind or order, an array of another length, a climatology with other n_bins, a series with other n_entries or more
 *     records than the handle's capacity, and a capture in flight.  Otherwise: one host-to-device copy and ONE unpack launch on
 *     the context's stream (with CF_CHECKPOINT_DIRECT: one copy per section and the hash-only launch), no host synchronisation;
 *     the handles' weights, counts and times are set at once.  The launch hashes what it wrote; a mismatch with the image is
 *     reported — CF_ERR_HIP, naming the section — by the next cf_checkpoint_wait or cf_sync.
 *   What is not in an image: records the caller has read and reset away, the atmosphere window and whatever was requested
 *     ahead (cf_discard_prefetched_atmosphere_state after a pickup), trip hints and chunk tables — rebuilt, never a bit.
 *   max_workgroups caps the launch (scheduling only: never a bit).
 * Slabs: each context writes its own image; section hashes of slabs add mod 2⁶⁴ as the monitor's do.
 * ---------------------------------------------------------------------------------------- */
#define CF_CHECKPOINT_MAX_SECTIONS 256
#define CF_CHECKPOINT_DIRECT 1
typedef struct cf_checkpoint_desc {
    int32_t struct_size;     /* sizeof(cf_checkpoint_desc) */
    int32_t flags;           /* 0 or CF_CHECKPOINT_DIRECT */
    int32_t max_workgroups;  /* 0: the library's choice; > 0 caps the launch */
    int32_t reserved;
} cf_checkpoint_desc;
typedef struct cf_checkpoint cf_checkpoint;
int cf_checkpoint_create(cf_ctx* ctx, const cf_checkpoint_desc* desc, cf_checkpoint** out);
int cf_checkpoint_destroy(cf_checkpoint* cp);
int cf_checkpoint_add_array(cf_checkpoint* cp, const char* name, void* d_ptr, size_t bytes);
int cf_checkpoint_add_average(cf_checkpoint* cp, const char* name, cf_average* a);
int cf_checkpoint_add_climatology(cf_checkpoint* cp, const char* name, cf_climatology* c);
int cf_checkpoint_add_integrals(cf_checkpoint* cp, const char* name, cf_integrals* q);
int cf_checkpoint_add_monitor(cf_checkpoint* cp, const char* name, cf_monitor* m);
int cf_checkpoint_set_host_blob(cf_checkpoint* cp, const void* h_blob, size_t bytes);
/* Footprint: reads exactly the registered bytes; writes no caller array.                                               */
int cf_checkpoint_capture(cf_checkpoint* cp);
int cf_checkpoint_wait(cf_checkpoint* cp, const void** h_image, size_t* bytes);
/* Footprint: writes exactly the registered bytes (of a series: the image's records), nothing beside them.              */
int cf_checkpoint_restore(cf_checkpoint* cp, const void* h_image, size_t bytes);
int cf_checkpoint_verify(const void* h_image, size_t bytes);
int cf_checkpoint_hash(const void* h_bytes, size_t n, uint64_t* out);
int cf_checkpoint_host_blob(const void* h_image, size_t bytes, const void** h_blob, size_t* blob_bytes);

#ifdef __cplusplus
}
#endif
#endif /* COFLUX_H */
