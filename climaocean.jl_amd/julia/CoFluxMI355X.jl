# CoFluxMI355X.jl — the reference-side binding of libcoflux (include/coflux.h).
#
# NOT EXECUTED IN THIS REPOSITORY: the build image has no Julia toolchain (SURVEY.md F3), so this
# file is the stub a ClimaOcean / NumericalEarth maintainer would add; every ccall below is kept
# one-to-one with a C entry point that IS exercised (through ctypes) by tests/.
#
# Seam: the reference reaches the flux path by multiple dispatch, not through an FFI
# (SURVEY.md §8b).  `update_state!(::OceanSeaIceModel)` calls, in order,
#     interpolate_atmosphere_state!, compute_atmosphere_ocean_fluxes!, compute_net_ocean_fluxes!
# (NEMOTKE/nemo_tke_compute_closure_fields.jl:7-8 names the call; the bodies live in
# NumericalEarth.EarthSystemModels).  A coupled model whose `interfaces` carry a `CoFluxBackend`
# dispatches those three functions here; nothing else in the user's script changes:
#
#     ocean      = ocean_simulation(grid)                        # README.md:67
#     atmosphere = JRA55PrescribedAtmosphere(arch)               # README.md:74
#     coupled    = OceanSeaIceModel(ocean; atmosphere,
#                      interfaces = CoFluxMI355X.interfaces(atmosphere, ocean))
#     run!(Simulation(coupled, Δt = 20minutes, stop_time = 30days))
#
# Host code stays Julia; no AMDGPU.jl / KernelAbstractions: device buffers are raw pointers owned
# by libcoflux (cf_device_alloc) and wrapped in `unsafe_wrap`-free handle structs.
module CoFluxMI355X

using Dates: Dates, DateTime, Second, month   # the calendar table of the climatologies (monthly_table)

const libcoflux = get(ENV, "LIBCOFLUX", "libcoflux.so")

# ---- mirrors of the POD structs in include/coflux.h (field order is the ABI) -----------------
struct CfGrid
    nx::Int32; ny::Int32; hx::Int32; hy::Int32; ring::Int32; reserved::Int32
end

struct CfRoughness
    kind::Int32; viscosity_kind::Int32
    constant_length::Float64; maximum_length::Float64; charnock::Float64; laminar::Float64
    wind_a1::Float64; wind_a2::Float64; wind_umax::Float64
    reynolds_A::Float64; reynolds_b::Float64
    viscosity::NTuple{4, Float64}
end

struct CfThermodynamics
    gas_constant::Float64; dry_air_molar_mass::Float64; water_molar_mass::Float64; kappa_d::Float64
    cp_v::Float64; cp_l::Float64; cp_i::Float64; LH_v0::Float64; LH_s0::Float64
    T_0::Float64; T_triple::Float64; p_triple::Float64; T_freeze::Float64; T_icenuc::Float64; pow_icenuc::Float64
end

struct CfSeawater
    water_molar_mass::Float64
    constituent_molar_mass::NTuple{4, Float64}
    constituent_mass_fraction::NTuple{4, Float64}
end

mutable struct CfFluxParams
    struct_size::Int32; abi_version::Int32
    similarity_form::Int32; stability_functions::Int32; stop_kind::Int32; maxiter::Int32
    velocity_difference::Int32; mask_kind::Int32
    tolerance::Float64; von_karman::Float64; gustiness_parameter::Float64; minimum_gustiness::Float64
    shear_gustiness_coefficient::Float64
    similarity_profile_floor::Float64
    momentum_roughness::CfRoughness; temperature_roughness::CfRoughness; water_vapor_roughness::CfRoughness
    reference_height::Float64; boundary_layer_height::Float64; gravitational_acceleration::Float64
    thermo::CfThermodynamics; seawater::CfSeawater
    ocean_reference_density::Float64; ocean_heat_capacity::Float64; ocean_freshwater_density::Float64
    ocean_temperature_offset::Float64; ocean_minimum_salinity::Float64; ocean_surface_z::Float64
    ocean_albedo_kind::Int32; penetrating_shortwave::Int32
    ocean_albedo::Float64; ocean_albedo_diffuse::Float64; ocean_albedo_direct::Float64
    ocean_emissivity::Float64; stefan_boltzmann::Float64
    flux_formulation::Int32; reserved1::Int32            # 0 SimilarityTheoryFluxes, 1 CoefficientBasedFluxes (Large–Yeager)
    ly_minimum_wind::Float64; ly_zeta_bound::Float64; ly_cd::NTuple{4, Float64}
    ly_high_wind::Float64; ly_cd_high::Float64; ly_ce::Float64; ly_ch_stable::Float64; ly_ch_unstable::Float64
    CfFluxParams() = new()
end

struct CfOceanSurface;   T::Ptr{Float64}; S::Ptr{Float64}; u::Ptr{Float64}; v::Ptr{Float64}; mask::Ptr{Cvoid}; end
struct CfExchangeFields; u::Ptr{Float64}; v::Ptr{Float64}; T::Ptr{Float64}; p::Ptr{Float64}; q::Ptr{Float64}
                         Qs::Ptr{Float64}; Ql::Ptr{Float64}; Mp::Ptr{Float64}; end
struct CfInterfaceFluxes
    sensible_heat::Ptr{Float64}; latent_heat::Ptr{Float64}; water_vapor::Ptr{Float64}
    x_momentum::Ptr{Float64}; y_momentum::Ptr{Float64}; temperature::Ptr{Float64}
    friction_velocity::Ptr{Float64}; temperature_scale::Ptr{Float64}; humidity_scale::Ptr{Float64}
    iterations::Ptr{Int32}
end
struct CfSeaIceFields
    concentration::Ptr{Float64}; interface_heat::Ptr{Float64}; salt_flux::Ptr{Float64}
    x_stress::Ptr{Float64}; y_stress::Ptr{Float64}
end
struct CfNetOceanFluxes
    u::Ptr{Float64}; v::Ptr{Float64}; T::Ptr{Float64}; S::Ptr{Float64}; shortwave_surface_flux::Ptr{Float64}
    upwelling_longwave::Ptr{Float64}; downwelling_longwave::Ptr{Float64}; downwelling_shortwave::Ptr{Float64}
end
struct CfAtmosSource
    data::NTuple{9, Ptr{Float32}}            # tas huss psl uas vas rlds rsds prra prsn (jra55_data_staging.jl:8)
    ns_x::Int32; ns_y::Int32; n_levels::Int32; level1::Int32; level2::Int32
    time_fraction::Float64
end
struct CfInterpWeights
    separable::Int32; reserved::Int32
    fi::Ptr{Float64}; fj::Ptr{Float64}; cos_rot::Ptr{Float64}; sin_rot::Ptr{Float64}; latitude::Ptr{Float64}
end

# ---- error handling: Julia exceptions on the Julia side, status codes across the ABI ----------
struct CoFluxError <: Exception; code::Cint; msg::String; end
last_error(ctx) = unsafe_string(ccall((:cf_last_error, libcoflux), Cstring, (Ptr{Cvoid},), ctx))
check(ctx, rc) = rc == 0 ? nothing : throw(CoFluxError(rc, last_error(ctx)))

# ---- lifecycle ---------------------------------------------------------------------------------
mutable struct CoFluxBackend
    ctx::Ptr{Cvoid}
    grid::CfGrid
    params::CfFluxParams
end

function CoFluxBackend(device::Integer, grid::CfGrid, params::CfFluxParams)
    ctx = Ref{Ptr{Cvoid}}(C_NULL)
    rc = ccall((:cf_create, libcoflux), Cint, (Ref{Ptr{Cvoid}}, Cint, Ref{CfGrid}, Ref{CfFluxParams}),
               ctx, device, grid, params)
    rc == 0 || throw(CoFluxError(rc, last_error(C_NULL)))
    backend = CoFluxBackend(ctx[], grid, params)
    finalizer(b -> ccall((:cf_destroy, libcoflux), Cint, (Ptr{Cvoid},), b.ctx), backend)
    return backend
end

# sha256[:16] of the sources the loaded library was built from (include/coflux.h): compare with the tree the stub ships with
build_stamp() = unsafe_string(ccall((:cf_build_stamp, libcoflux), Cstring, ()))

default_flux_params() = (p = CfFluxParams(); ccall((:cf_default_flux_params, libcoflux), Cint, (Ref{CfFluxParams},), p); p)

device_alloc(b, bytes) = ccall((:cf_device_alloc, libcoflux), Ptr{Cvoid}, (Ptr{Cvoid}, Csize_t), b.ctx, bytes)
h2d!(b, dst, src::Array) = check(b.ctx, ccall((:cf_h2d, libcoflux), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Csize_t),
                                              b.ctx, dst, src, sizeof(src)))
d2h!(b, dst::Array, src) = check(b.ctx, ccall((:cf_d2h, libcoflux), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Csize_t),
                                              b.ctx, dst, src, sizeof(dst)))
sync(b) = check(b.ctx, ccall((:cf_sync, libcoflux), Cint, (Ptr{Cvoid},), b.ctx))

# How the SimilarityTheoryFluxes fixed point is reached (include/coflux.h, CF_OPT_SOLVER_PATH): the reference's own
# iteration (:exact, default) or the certified reduced-iteration solve with per-cell exact-path fallback (:certified,
# every cell within `budget` — default 8e-7, in the flux metric of coflux.h — of the exact path's result).
const CF_OPT_SOLVER_PATH = Cint(10)
const CF_OPT_CERTIFIED_BUDGET = Cint(11)
const CF_OPT_LATENCY_LAYOUT = Cint(13)   # 0 never, 1 automatic (default), 2 always: the exact path's kernels for one or two waves per SIMD
set_option!(b, option, value) = check(b.ctx, ccall((:cf_set_option, libcoflux), Cint, (Ptr{Cvoid}, Cint, Cint), b.ctx, option, value))
function set_solver_path!(b, path::Symbol; budget = 8e-7)
    path in (:exact, :certified) || throw(ArgumentError("solver path must be :exact or :certified"))
    set_option!(b, CF_OPT_SOLVER_PATH, path == :certified ? 1 : 0)
    path == :certified && set_option!(b, CF_OPT_CERTIFIED_BUDGET, round(Cint, budget * 1e9))
    return b
end
solver_iteration_path(b) = (p = Ref{Cint}(0); check(b.ctx, ccall((:cf_solver_iteration_path, libcoflux), Cint, (Ptr{Cvoid}, Ref{Cint}), b.ctx, p));
                            p[] == 1 ? :certified : :exact)

solver_latency_layout(b) = (p = Ref{Cint}(0); check(b.ctx, ccall((:cf_solver_latency_layout, libcoflux), Cint, (Ptr{Cvoid}, Ref{Cint}), b.ctx, p)); p[] == 1)
# CF_OPT_HALO_IN_SOLVER_LAUNCH: a step's peer-direct halo rows as rider workgroups of its solver launch (include/coflux.h)
const CF_OPT_HALO_IN_SOLVER_LAUNCH = Cint(14)
halo_in_solver_launch!(b, on::Bool) = set_option!(b, CF_OPT_HALO_IN_SOLVER_LAUNCH, on ? 1 : 0)
# CF_OPT_LAND_ZEROS: 0 every launch writes the land cells' zeros, 1 (default) inside time_steps! only a call's first step does —
# nothing else may write the flux and net-flux outputs while such a call's work is on the stream (include/coflux.h)
const CF_OPT_LAND_ZEROS = Cint(2)
land_zeros!(b, mode::Integer) = set_option!(b, CF_OPT_LAND_ZEROS, mode)
function peer_halo_stats(b)
    n = Ref{Culonglong}(0); m = Ref{Culonglong}(0)
    check(b.ctx, ccall((:cf_peer_halo_stats, libcoflux), Cint, (Ptr{Cvoid}, Ref{Culonglong}, Ref{Culonglong}), b.ctx, n, m))
    return (exchanges = n[], in_solver_launch = m[])
end
# fold launches of their own, and exchange launches whose north side was the tripolar fold (the last rank of time_steps_coupled!
# under CF_HALO_PEER with fold_north), since the context was created
function fold_counts(b)
    n = Ref{Clonglong}(0); m = Ref{Clonglong}(0)
    check(b.ctx, ccall((:cf_debug_fold_counts, libcoflux), Cint, (Ptr{Cvoid}, Ref{Clonglong}, Ref{Clonglong}), b.ctx, n, m))
    return (fold_launches = n[], exchanges_with_fold = m[])
end

# ---- the three functions of update_state! ------------------------------------------------------
# Each body is ONE ccall; these are the methods a maintainer adds for
#   interpolate_atmosphere_state!(interfaces::…{<:CoFluxBackend}, atmosphere, coupled_model) etc.
interpolate_atmosphere_state!(b::CoFluxBackend, src::CfAtmosSource, w::CfInterpWeights, out::CfExchangeFields) =
    check(b.ctx, ccall((:cf_interpolate_atmosphere_state, libcoflux), Cint,
                       (Ptr{Cvoid}, Ref{CfAtmosSource}, Ref{CfInterpWeights}, Ref{CfExchangeFields}), b.ctx, src, w, out))

compute_atmosphere_ocean_fluxes!(b::CoFluxBackend, ocean::CfOceanSurface, atmos::CfExchangeFields, out::CfInterfaceFluxes) =
    check(b.ctx, ccall((:cf_compute_atmosphere_ocean_fluxes, libcoflux), Cint,
                       (Ptr{Cvoid}, Ref{CfOceanSurface}, Ref{CfExchangeFields}, Ref{CfInterfaceFluxes}), b.ctx, ocean, atmos, out))

compute_net_ocean_fluxes!(b::CoFluxBackend, ocean, atmos, fluxes, ice::Union{CfSeaIceFields, Nothing}, w, out::CfNetOceanFluxes) =
    check(b.ctx, ccall((:cf_compute_net_ocean_fluxes, libcoflux), Cint,
                       (Ptr{Cvoid}, Ref{CfOceanSurface}, Ref{CfExchangeFields}, Ref{CfInterfaceFluxes}, Ptr{CfSeaIceFields},
                        Ref{CfInterpWeights}, Ref{CfNetOceanFluxes}),
                       b.ctx, ocean, atmos, fluxes, ice === nothing ? C_NULL : Ref(ice), w, out))

# update_state!(coupled_model): the fused path (one launch for interpolation + solver, one for the net fluxes)
update_state!(b::CoFluxBackend, src, w, ocean, atmos, fluxes, ice, net) =
    check(b.ctx, ccall((:cf_update_state, libcoflux), Cint,
                       (Ptr{Cvoid}, Ref{CfAtmosSource}, Ref{CfInterpWeights}, Ref{CfOceanSurface}, Ref{CfExchangeFields},
                        Ref{CfInterfaceFluxes}, Ptr{CfSeaIceFields}, Ref{CfNetOceanFluxes}),
                       b.ctx, src, w, ocean, atmos, fluxes, ice === nothing ? C_NULL : Ref(ice), net))

# NormalizeSalinity callback (src/OMIPConfigurations/omip_simulation.jl:182-220): flux .-= ⟨flux + additional⟩_A,wet
normalize_salinity_flux!(b::CoFluxBackend, flux::Ptr{Float64}, additional, area, mask, mean_out = C_NULL) =
    check(b.ctx, ccall((:cf_normalize_salinity_flux, libcoflux), Cint,
                       (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Cvoid}, Ptr{Float64}),
                       b.ctx, flux, additional, area, mask, mean_out))

# NormalizeSalinity with exact sums: the mean's bits do not depend on the slab decomposition; over the reduction world when one
# is connected on more than one rank (peer_reduce_connect!).  CF_NORMALIZE_EXACT is the value of CfCoupledStep.normalize_salinity
const CF_NORMALIZE_EXACT = Int32(2)
normalize_salinity_flux_exact!(b::CoFluxBackend, flux::Ptr{Float64}, additional, area, mask, mean_out = C_NULL) =
    check(b.ctx, ccall((:cf_normalize_salinity_flux_exact, libcoflux), Cint,
                       (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Cvoid}, Ptr{Float64}),
                       b.ctx, flux, additional, area, mask, mean_out))
# test aid: this rank's exact sums (Σ J·A, Σ A) and the counts of NaN / +Inf / −Inf terms of the first; synchronises
function debug_salinity_sums_exact(b::CoFluxBackend, flux::Ptr{Float64}, additional, area, mask)
    sums = zeros(Float64, 2); counts = zeros(Culonglong, 3)
    check(b.ctx, ccall((:cf_debug_salinity_sums_exact, libcoflux), Cint,
                       (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Culonglong}),
                       b.ctx, flux, additional, area, mask, sums, counts))
    return (sums = (sums[1], sums[2]), nonfinite = (counts[1], counts[2], counts[3]))
end
# ---- atmosphere–sea-ice interface: compute_atmosphere_sea_ice_fluxes!(coupled_model) ---------------
const CF_SKIN_EXPLICIT = Int32(0)
const CF_SKIN_SEMI_IMPLICIT = Int32(1)
const CF_SKIN_LINEARISED = Int32(2)      # one Newton step on the surface energy balance per iteration (include/coflux.h)
# SkinTemperature(ConductiveFlux) + SurfaceRadiationProperties(sea_ice_albedo, 1.0) (atmosphere.jl:34-44)
mutable struct CfSeaIceParams
    struct_size::Int32; skin_temperature_scheme::Int32       # CF_SKIN_EXPLICIT = 0 / CF_SKIN_SEMI_IMPLICIT = 1 / CF_SKIN_LINEARISED = 2
    conductivity::Float64; consolidation_thickness::Float64; maximum_temperature_change::Float64
    ice_salinity::Float64; liquidus_slope::Float64; freshwater_melting_temperature::Float64
    albedo::Float64; emissivity::Float64; temperature_offset::Float64
    CfSeaIceParams() = new()
end
struct CfSeaIceState   # sea_ice.model.{ice_concentration, ice_thickness, top_surface_temperature, velocities}
    concentration::Ptr{Float64}; thickness::Ptr{Float64}; top_temperature::Ptr{Float64}
    u::Ptr{Float64}; v::Ptr{Float64}; albedo::Ptr{Float64}; snow_thickness::Ptr{Float64}   # snow: atmosphere.jl:34
end
function default_sea_ice_params()
    p = CfSeaIceParams()
    ccall((:cf_default_sea_ice_params, libcoflux), Cint, (Ref{CfSeaIceParams},), p)
    return p
end
# `ice_fluxes` = corrected_atmosphere_sea_ice_fluxes(FT) / ncar_atmosphere_sea_ice_fluxes(FT) lowered to CfFluxParams
set_sea_ice_formulation!(b::CoFluxBackend, ice_fluxes::CfFluxParams, ice::CfSeaIceParams = default_sea_ice_params()) =
    check(b.ctx, ccall((:cf_set_sea_ice_formulation, libcoflux), Cint,
                       (Ptr{Cvoid}, Ref{CfFluxParams}, Ref{CfSeaIceParams}), b.ctx, ice_fluxes, ice))
compute_atmosphere_sea_ice_fluxes!(b::CoFluxBackend, ice::CfSeaIceState, ocean::CfOceanSurface,
                                   atmos::CfExchangeFields, out::CfInterfaceFluxes) =
    check(b.ctx, ccall((:cf_compute_atmosphere_sea_ice_fluxes, libcoflux), Cint,
                       (Ptr{Cvoid}, Ref{CfSeaIceState}, Ref{CfOceanSurface}, Ref{CfExchangeFields}, Ref{CfInterfaceFluxes}),
                       b.ctx, ice, ocean, atmos, out))

struct CfNetSeaIceFluxes; top_heat::Ptr{Float64}; bottom_heat::Ptr{Float64}; end
# compute_net_sea_ice_fluxes!(coupled_model): ΣQt, ΣQb handed to the sea-ice thermodynamics (frazil / interface may be C_NULL)
compute_net_sea_ice_fluxes!(b::CoFluxBackend, ice::CfSeaIceState, ocean::CfOceanSurface, atmos::CfExchangeFields,
                            ai::CfInterfaceFluxes, frazil::Ptr{Float64}, interface::Ptr{Float64}, out::CfNetSeaIceFluxes) =
    check(b.ctx, ccall((:cf_compute_net_sea_ice_fluxes, libcoflux), Cint,
                       (Ptr{Cvoid}, Ref{CfSeaIceState}, Ref{CfOceanSurface}, Ref{CfExchangeFields}, Ref{CfInterfaceFluxes},
                        Ptr{Float64}, Ptr{Float64}, Ref{CfNetSeaIceFluxes}), b.ctx, ice, ocean, atmos, ai, frazil, interface, out))

# update_state!(coupled_model) with sea ice: ocean path + atmosphere–sea-ice interface + net sea-ice fluxes, five launches
update_state_sea_ice!(b::CoFluxBackend, src::CfAtmosSource, w::CfInterpWeights, ocean::CfOceanSurface, atmos::CfExchangeFields,
                      ao::CfInterfaceFluxes, partition::CfSeaIceFields, net::CfNetOceanFluxes, ice::CfSeaIceState,
                      ai::CfInterfaceFluxes, frazil::Ptr{Float64}, interface::Ptr{Float64}, net_ice::CfNetSeaIceFluxes) =
    check(b.ctx, ccall((:cf_update_state_sea_ice, libcoflux), Cint,
                       (Ptr{Cvoid}, Ref{CfAtmosSource}, Ref{CfInterpWeights}, Ref{CfOceanSurface}, Ref{CfExchangeFields},
                        Ref{CfInterfaceFluxes}, Ref{CfSeaIceFields}, Ref{CfNetOceanFluxes}, Ref{CfSeaIceState},
                        Ref{CfInterfaceFluxes}, Ptr{Float64}, Ptr{Float64}, Ref{CfNetSeaIceFluxes}),
                       b.ctx, src, w, ocean, atmos, ao, partition, net, ice, ai, frazil, interface, net_ice))

# ---- JRA55 snapshot window in HBM: JRA55PrescribedAtmosphere(arch; time_indices_in_memory, prefetch) ---------
mutable struct CoFluxWindow
    ptr::Ptr{Cvoid}
    backend::CoFluxBackend
    nsx::Int; nsy::Int; nslots::Int
end
function CoFluxWindow(b::CoFluxBackend, nsx, nsy, nslots)
    out = Ref{Ptr{Cvoid}}(C_NULL)
    check(b.ctx, ccall((:cf_window_create, libcoflux), Cint, (Ptr{Cvoid}, Int32, Int32, Int32, Ref{Ptr{Cvoid}}),
                       b.ctx, nsx, nsy, nslots, out))
    w = CoFluxWindow(out[], b, nsx, nsy, nslots)
    finalizer(x -> ccall((:cf_window_destroy, libcoflux), Cint, (Ptr{Cvoid},), x.ptr), w)
    return w
end
# pinned staging buffer of (slot, variable) as a Julia array the NetCDF reader fills in place (0-based slot/variable)
staging(w::CoFluxWindow, slot, var) =
    unsafe_wrap(Array, ccall((:cf_window_host_buffer, libcoflux), Ptr{Float32}, (Ptr{Cvoid}, Int32, Int32), w.ptr, slot, var),
                (w.nsx, w.nsy))
wait_slot!(w::CoFluxWindow, slot) =
    check(w.backend.ctx, ccall((:cf_window_wait_slot, libcoflux), Cint, (Ptr{Cvoid}, Int32), w.ptr, slot))
# time_index = the monotone snapshot counter ⌊t/Δt⌋ (slot = counter mod nslots), not the index inside a repeat-year record
commit!(w::CoFluxWindow, slot, time_index) =
    check(w.backend.ctx, ccall((:cf_window_commit, libcoflux), Cint, (Ptr{Cvoid}, Int32, Int64), w.ptr, slot, time_index))
resident(w::CoFluxWindow, time_index) = ccall((:cf_window_find, libcoflux), Cint, (Ptr{Cvoid}, Int64), w.ptr, time_index) >= 0
function source(w::CoFluxWindow, n₁, n₂, ñ)          # → CfAtmosSource for update_state!
    src = Ref{CfAtmosSource}()
    check(w.backend.ctx, ccall((:cf_window_source, libcoflux), Cint, (Ptr{Cvoid}, Int64, Int64, Float64, Ref{CfAtmosSource}),
                               w.ptr, n₁, n₂, ñ, src))
    return src[]
end

# ---- latitude-slab halo rows over RCCL (Distributed(GPU(), partition = Partition(1, R))) -------
comm_unique_id() = (id = zeros(UInt8, 128); ccall((:cf_comm_unique_id, libcoflux), Cint, (Ptr{UInt8},), id); id)
# (nranks, rank, device) as RCCL itself reports them for this backend's communicator — beside MPI.Comm_size in a launcher's log
function comm_count(b)
    n, r, d = Ref{Cint}(0), Ref{Cint}(0), Ref{Cint}(0)
    check(b.ctx, ccall((:cf_comm_count, libcoflux), Cint, (Ptr{Cvoid}, Ref{Cint}, Ref{Cint}, Ref{Cint}), b.ctx, n, r, d))
    return (n[], r[], d[])
end
comm_init!(b, id::Vector{UInt8}, rank, nranks) =   # `id` is MPI.bcast from rank 0
    check(b.ctx, ccall((:cf_comm_init, libcoflux), Cint, (Ptr{Cvoid}, Ptr{UInt8}, Cint, Cint), b.ctx, id, rank, nranks))
halo_exchange_rows!(b, fields::Vector{Ptr{Float64}}, rows = 2) =   # rows = ring + 1: the ring row reads v[j+1]
    check(b.ctx, ccall((:cf_halo_exchange_rows, libcoflux), Cint, (Ptr{Cvoid}, Ptr{Ptr{Float64}}, Cint, Cint),
                       b.ctx, fields, length(fields), rows))

# ---- peer-direct halo rows (HIP IPC mailboxes; handles travel by MPI.Allgather) and the tripolar fold ----------------
peer_halo_export!(b, max_fields = 4, max_rows = 2) = (h = zeros(UInt8, 64);
    check(b.ctx, ccall((:cf_peer_halo_export, libcoflux), Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{UInt8}), b.ctx, max_fields, max_rows, h)); h)
peer_halo_connect!(b, south::Union{Nothing, Vector{UInt8}}, north::Union{Nothing, Vector{UInt8}}, rank, nranks) =
    check(b.ctx, ccall((:cf_peer_halo_connect, libcoflux), Cint, (Ptr{Cvoid}, Ptr{UInt8}, Ptr{UInt8}, Cint, Cint), b.ctx,
                       isnothing(south) ? C_NULL : south, isnothing(north) ? C_NULL : north, rank, nranks))
# the reduction world of the exact sums: every rank's reduce mailbox, mapped by every other rank (handles in rank order,
# 64 bytes each; `nothing` for a world of one).  Every rank issues the same number of reductions.
const CF_PEER_REDUCE_MAX_RANKS = 8
peer_reduce_export!(b) = (h = zeros(UInt8, 64);
    check(b.ctx, ccall((:cf_peer_reduce_export, libcoflux), Cint, (Ptr{Cvoid}, Ptr{UInt8}), b.ctx, h)); h)
peer_reduce_connect!(b, handles::Union{Nothing, Vector{Vector{UInt8}}}, rank, nranks) =
    check(b.ctx, ccall((:cf_peer_reduce_connect, libcoflux), Cint, (Ptr{Cvoid}, Ptr{UInt8}, Cint, Cint), b.ctx,
                       isnothing(handles) ? C_NULL : reduce(vcat, handles), rank, nranks))
halo_exchange_rows_peer!(b, fields::Vector{Ptr{Float64}}, rows = 2) =
    check(b.ctx, ccall((:cf_halo_exchange_rows_peer, libcoflux), Cint, (Ptr{Cvoid}, Ptr{Ptr{Float64}}, Cint, Cint),
                       b.ctx, fields, length(fields), rows))
# TripolarGrid: the last rank's north halo (T, S centres; u x-faces, v y-faces; vectors change sign) — one_degree_tripolar.jl:48-51
fold_north_halo!(b, fields::Vector{Ptr{Float64}}, locations::Vector{Cint}, signs::Vector{Float64}, rows = 2) =
    check(b.ctx, ccall((:cf_fold_north_halo, libcoflux), Cint, (Ptr{Cvoid}, Ptr{Ptr{Float64}}, Ptr{Cint}, Ptr{Float64}, Cint, Cint),
                       b.ctx, fields, locations, signs, length(fields), rows))
# The tile world, Distributed(GPU(), partition = Partition(px, py)): rank = p + px · q, x fastest, every tile nx columns wide.  A
# context joins latitude slabs (peer_halo_connect!) or a tile world, not both.  max_cols: ring + 1, and one more on the top row of
# a tripolar world with px > 1.  `handles`: every rank's handle in rank order (MPI.Allgather), `nothing` for a world of one.
peer_tile_export!(b, max_fields = 4, max_rows = 2, max_cols = 3) = (h = zeros(UInt8, 64);
    check(b.ctx, ccall((:cf_peer_tile_export, libcoflux), Cint, (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{UInt8}), b.ctx, max_fields, max_rows, max_cols, h)); h)
peer_tile_connect!(b, handles::Union{Nothing, Vector{Vector{UInt8}}}, px, py, rank, tripolar::Bool) =
    check(b.ctx, ccall((:cf_peer_tile_connect, libcoflux), Cint, (Ptr{Cvoid}, Ptr{UInt8}, Cint, Cint, Cint, Cint), b.ctx,
                       isnothing(handles) ? C_NULL : reduce(vcat, handles), px, py, rank, tripolar ? 1 : 0))
# fold_north: true on every rank of the top row of a tripolar world, false on every other; locations and signs as fold_north_halo!
halo_exchange_tile_peer!(b, fields::Vector{Ptr{Float64}}, locations::Vector{Cint}, signs::Vector{Float64}, rows = 2, fold_north::Bool = false) =
    check(b.ctx, ccall((:cf_halo_exchange_tile_peer, libcoflux), Cint, (Ptr{Cvoid}, Ptr{Ptr{Float64}}, Ptr{Cint}, Ptr{Float64}, Cint, Cint, Cint),
                       b.ctx, fields, locations, signs, length(fields), rows, fold_north ? 1 : 0))
function peer_tile_stats(b)
    n = Ref{Culonglong}(0); m = Ref{Culonglong}(0); k = Ref{Culonglong}(0)
    check(b.ctx, ccall((:cf_peer_tile_stats, libcoflux), Cint, (Ptr{Cvoid}, Ref{Culonglong}, Ref{Culonglong}, Ref{Culonglong}), b.ctx, n, m, k))
    return (exchanges = n[], column_launches = m[], folds_sent = k[])
end

# ---- pipelined update_state!: the prescribed atmosphere of the NEXT step on the auxiliary stream ---------------------
prefetch_atmosphere_state!(b, src_next::CfAtmosSource, w::CfInterpWeights, out::CfExchangeFields) =
    check(b.ctx, ccall((:cf_prefetch_atmosphere_state, libcoflux), Cint,
                       (Ptr{Cvoid}, Ref{CfAtmosSource}, Ref{CfInterpWeights}, Ref{CfExchangeFields}), b.ctx, src_next, w, out))

# on leaving the stepping loop: no later update_state! may mistake a requested-ahead state for the one it asks for
discard_prefetched_atmosphere_state!(b) =
    check(b.ctx, ccall((:cf_discard_prefetched_atmosphere_state, libcoflux), Cint, (Ptr{Cvoid},), b.ctx))

# the solver's schedule for a wet mask, built ahead of the first step (optional: the first call builds it otherwise)
ensure_chunk_table!(b, mask::Ptr{Cvoid}) =
    check(b.ctx, ccall((:cf_ensure_chunk_table, libcoflux), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), b.ctx, mask))

# self-test hook: the table as built — (begins, wet cells per chunk, static lists in use); after ensure_chunk_table!
function debug_chunk_table(b; capacity::Integer = 1024)
    n, valid = Ref{Cint}(0), Ref{Cint}(0)
    while true
        begins, counts = zeros(Cint, capacity), zeros(Cint, capacity)
        rc = ccall((:cf_debug_chunk_table, libcoflux), Cint, (Ptr{Cvoid}, Ptr{Cint}, Ptr{Cint}, Cint, Ref{Cint}, Ref{Cint}),
                   b.ctx, begins, counts, capacity, n, valid)
        if rc != 0 && n[] + 1 > capacity
            capacity = n[] + 1
            continue
        end
        check(b.ctx, rc)
        return begins[1:n[] + 1], counts[1:n[]], valid[] == 1
    end
end

# self-test hook: (rows of 64 cells per wave tile, workgroups) of the tiled interpolation on this context's grid and options
function debug_interp_grid(b)
    rows, blocks = Ref{Cint}(0), Ref{Cint}(0)
    check(b.ctx, ccall((:cf_debug_interp_grid, libcoflux), Cint, (Ptr{Cvoid}, Ref{Cint}, Ref{Cint}), b.ctx, rows, blocks))
    return Int(rows[]), Int(blocks[])
end

# self-test hook: how many ocean-solver launches of the last time_steps! call wrote the land zeros (CF_OPT_LAND_ZEROS)
function debug_land_zero_launches(b)
    n = Ref{Cint}(0)
    check(b.ctx, ccall((:cf_debug_land_zero_launches, libcoflux), Cint, (Ptr{Cvoid}, Ref{Cint}), b.ctx, n))
    return Int(n[])
end

# self-test hook: which way every atmosphere state requested ahead went since the context was made (cf_prefetch_stats);
# requests == consumed + mismatched + voided + superseded + discarded + pending at every point
mutable struct CfPrefetchStats
    struct_size::Int32; pending::Int32
    requests::UInt64
    launched_aux::UInt64; launched_tail::UInt64; launched_merged::UInt64; launched_ice_tail::UInt64; launched_own::UInt64
    consumed::UInt64; mismatched::UInt64; voided::UInt64; superseded::UInt64; discarded::UInt64
    step_interpolations::UInt64
end
function debug_prefetch_stats(b)
    st = CfPrefetchStats(Int32(sizeof(CfPrefetchStats)), 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)
    check(b.ctx, ccall((:cf_debug_prefetch_stats, libcoflux), Cint, (Ptr{Cvoid}, Ref{CfPrefetchStats}), b.ctx, st))
    return st
end

# ---- run!(simulation) of a prescribed-ocean model inside the library (bench / offline forcing runs) -------------------
struct CfRunSchedule
    struct_size::Int32; n_ocean_states::Int32
    ocean_states::Ptr{CfOceanSurface}
    n_atmos_sets::Int32; pipeline::Int32
    atmos::Ptr{CfExchangeFields}
    first_level::Int32; halo_backend::Int32; halo_rows::Int32; fold_north::Int32
    time_fraction::Float64; time_fraction_increment::Float64
end
time_steps!(b, first_step, nsteps, sched::CfRunSchedule, src, w, fluxes, ice, net) =
    check(b.ctx, ccall((:cf_time_steps, libcoflux), Cint,
                       (Ptr{Cvoid}, Int64, Cint, Ref{CfRunSchedule}, Ref{CfAtmosSource}, Ref{CfInterpWeights}, Ref{CfInterfaceFluxes},
                        Ptr{CfSeaIceFields}, Ref{CfNetOceanFluxes}), b.ctx, first_step, nsteps, sched, src, w, fluxes, ice, net))

# ---- time averages on the device: AveragedTimeInterval output of surface fields (omip_diagnostics.jl:152-158) -----------
# An averager keeps running means of up to 16 ocean-grid fields (one launch per collection); the caller reads the means at
# the end of a window, then reset!s.  attach_average! makes time_steps! collect it every `stride` steps.
mutable struct CoFluxAverage
    ptr::Ptr{Cvoid}
    backend::CoFluxBackend
    sources::Vector{Ptr{Float64}}; means::Vector{Ptr{Float64}}
end
function CoFluxAverage(b::CoFluxBackend, sources::Vector{Ptr{Float64}}, means::Vector{Ptr{Float64}})
    out = Ref{Ptr{Cvoid}}(C_NULL)
    check(b.ctx, ccall((:cf_average_create, libcoflux), Cint, (Ptr{Cvoid}, Cint, Ptr{Ptr{Float64}}, Ptr{Ptr{Float64}}, Ref{Ptr{Cvoid}}),
                       b.ctx, length(sources), sources, means, out))
    a = CoFluxAverage(out[], b, sources, means)
    finalizer(x -> ccall((:cf_average_destroy, libcoflux), Cint, (Ptr{Cvoid},), x.ptr), a)
    return a
end
reset!(a::CoFluxAverage) = check(C_NULL, ccall((:cf_average_reset, libcoflux), Cint, (Ptr{Cvoid},), a.ptr))
collect!(a::CoFluxAverage, weight) = check(C_NULL, ccall((:cf_average_collect, libcoflux), Cint, (Ptr{Cvoid}, Float64), a.ptr, weight))
function average_weight(a::CoFluxAverage)
    total = Ref{Float64}(0); samples = Ref{Int64}(0)
    check(C_NULL, ccall((:cf_average_weight, libcoflux), Cint, (Ptr{Cvoid}, Ref{Float64}, Ref{Int64}), a.ptr, total, samples))
    return (total = total[], samples = samples[])
end
attach_average!(b, a::Union{Nothing, CoFluxAverage}, stride = 1, step_weight = 1.0) =
    check(b.ctx, ccall((:cf_attach_average, libcoflux), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Float64),
                       b.ctx, isnothing(a) ? C_NULL : a.ptr, stride, step_weight))

# ---- derived quantities averaged in the collection launch (omip_diagnostics.jl:13-25,111-123; visualize/cache.jl:359-466) --
# Squares, face → centre means, centred squares, kinetic energy and the rotation to geographic east / north, each times a
# scale, evaluated per cell inside the averager's launch: the derived array never exists in memory.  The result is an
# ordinary CoFluxAverage (collect!, reset!, average_weight, attach_average!).
const CF_TERM_FIELD, CF_TERM_PRODUCT, CF_TERM_CENTER_X, CF_TERM_CENTER_Y = Int32(0), Int32(1), Int32(2), Int32(3)
const CF_TERM_CENTER_X_SQUARE, CF_TERM_CENTER_Y_SQUARE, CF_TERM_KINETIC_ENERGY = Int32(4), Int32(5), Int32(6)
const CF_TERM_EAST, CF_TERM_NORTH = Int32(7), Int32(8)
const CF_TERM_AT_CENTERS = Int32(1)
struct CfAverageTerm
    kind::Int32; flags::Int32
    a::Ptr{Float64}; b::Ptr{Float64}
    scale::Float64
    mean::Ptr{Float64}
end
struct CfAverageDesc
    struct_size::Int32; n_terms::Int32
    terms::Ptr{CfAverageTerm}
    cos_rotation::Ptr{Float64}; sin_rotation::Ptr{Float64}
    max_workgroups::Int32; reserved::Int32
end
function CoFluxAverage(b::CoFluxBackend, terms::Vector{CfAverageTerm}; cos_rotation = C_NULL, sin_rotation = C_NULL, max_workgroups = 0)
    out = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve terms begin
        desc = CfAverageDesc(sizeof(CfAverageDesc), length(terms), pointer(terms), cos_rotation, sin_rotation, max_workgroups, 0)
        check(b.ctx, ccall((:cf_average_create_derived, libcoflux), Cint, (Ptr{Cvoid}, Ref{CfAverageDesc}, Ref{Ptr{Cvoid}}), b.ctx, desc, out))
    end
    a = CoFluxAverage(out[], b, unique(vcat([t.a for t in terms], [t.b for t in terms if t.b != C_NULL])), [t.mean for t in terms])
    finalizer(x -> ccall((:cf_average_destroy, libcoflux), Cint, (Ptr{Cvoid},), x.ptr), a)
    return a
end

# ---- the net heat and salt flux budget averaged in the collection launch (omip_diagnostics.jl:84-89,135-140) ---------------
# JTao, JTio, JTf, JTn, JSn, JSio and the finer parts of compute_net_ocean_fluxes!'s two sums, evaluated per cell inside the
# averager's launch from the arrays the net fluxes were computed from (include/coflux.h: cf_average_create_budget has the
# table).  The result is an ordinary CoFluxAverage.  attach_average_slot! attaches up to CF_ATTACHED_AVERAGES_MAX averagers
# to the step loops; slot 0 is attach_average!'s.
const CF_BUDGET_HEAT_SHORTWAVE, CF_BUDGET_HEAT_LONGWAVE_UP, CF_BUDGET_HEAT_LONGWAVE_DOWN = Int32(0), Int32(1), Int32(2)
const CF_BUDGET_HEAT_SENSIBLE, CF_BUDGET_HEAT_LATENT, CF_BUDGET_HEAT_ATMOSPHERE_OCEAN = Int32(3), Int32(4), Int32(5)
const CF_BUDGET_HEAT_ICE_OCEAN, CF_BUDGET_HEAT_FRAZIL, CF_BUDGET_HEAT_NET = Int32(6), Int32(7), Int32(8)
const CF_BUDGET_SALT_EVAPORATION, CF_BUDGET_SALT_PRECIPITATION, CF_BUDGET_SALT_ATMOSPHERE_OCEAN = Int32(9), Int32(10), Int32(11)
const CF_BUDGET_SALT_ICE_OCEAN, CF_BUDGET_SALT_LAND, CF_BUDGET_SALT_NET = Int32(12), Int32(13), Int32(14)
const CF_ATTACHED_AVERAGES_MAX = 4
struct CfBudgetTerm
    kind::Int32; reserved::Int32
    scale::Float64
    mean::Ptr{Float64}
end
struct CfBudgetDesc
    struct_size::Int32; n_terms::Int32
    terms::Ptr{CfBudgetTerm}
    ocean::Ptr{CfOceanSurface}; exchange::Ptr{CfExchangeFields}; fluxes::Ptr{CfInterfaceFluxes}; ice::Ptr{CfSeaIceFields}
    frazil_heat::Ptr{Float64}; land_freshwater::Ptr{Float64}
    weights::Ptr{CfInterpWeights}
    max_workgroups::Int32; reserved::Int32
end
function CoFluxAverage(b::CoFluxBackend, terms::Vector{CfBudgetTerm}; ocean = nothing, exchange = nothing, fluxes = nothing, ice = nothing,
                       frazil_heat = C_NULL, land_freshwater = C_NULL, weights = nothing, max_workgroups = 0)
    out = Ref{Ptr{Cvoid}}(C_NULL)
    bundles = [isnothing(x) ? nothing : Ref(x) for x in (ocean, exchange, fluxes, ice, weights)]
    GC.@preserve terms bundles begin
        ptr(k, T) = isnothing(bundles[k]) ? Ptr{T}(C_NULL) : Base.unsafe_convert(Ptr{T}, bundles[k])
        desc = CfBudgetDesc(sizeof(CfBudgetDesc), length(terms), pointer(terms), ptr(1, CfOceanSurface), ptr(2, CfExchangeFields),
                            ptr(3, CfInterfaceFluxes), ptr(4, CfSeaIceFields), frazil_heat, land_freshwater, ptr(5, CfInterpWeights),
                            max_workgroups, 0)
        check(b.ctx, ccall((:cf_average_create_budget, libcoflux), Cint, (Ptr{Cvoid}, Ref{CfBudgetDesc}, Ref{Ptr{Cvoid}}), b.ctx, desc, out))
    end
    a = CoFluxAverage(out[], b, Ptr{Float64}[], [t.mean for t in terms])
    finalizer(x -> ccall((:cf_average_destroy, libcoflux), Cint, (Ptr{Cvoid},), x.ptr), a)
    return a
end
attach_average_slot!(b, slot, a::Union{Nothing, CoFluxAverage}, stride = 1, step_weight = 1.0) =
    check(b.ctx, ccall((:cf_attach_average_slot, libcoflux), Cint, (Ptr{Cvoid}, Int32, Ptr{Cvoid}, Int32, Float64),
                       b.ctx, slot, isnothing(a) ? C_NULL : a.ptr, stride, step_weight))

# ---- surface integrals on the device: scalar time series (omip_diagnostics.jl:194-218, visualize/common.jl:715-787) -----
# An integrator turns surface fields into records of area-weighted, masked, regional integrals (one pass per collection)
# and keeps the series on the device; read_integrals is the only host synchronisation.  attach_integrals! makes
# time_steps! append a record every `stride` steps.
const CF_INTEGRAND_ONE, CF_INTEGRAND_FIELD, CF_INTEGRAND_PRODUCT, CF_INTEGRAND_ABOVE = Int32(0), Int32(1), Int32(2), Int32(3)
struct CfIntegralEntry
    kind::Int32; region_bit::Int32
    a::Ptr{Float64}; b::Ptr{Float64}
    threshold::Float64
end
CfIntegralEntry() = CfIntegralEntry(CF_INTEGRAND_ONE, 0, C_NULL, C_NULL, 0.0)
struct CfIntegralsDesc
    struct_size::Int32; n_entries::Int32
    area::Ptr{Float64}; mask::Ptr{Cvoid}; region::Ptr{UInt8}
    max_workgroups::Int32; reserved::Int32
    entries::NTuple{32, CfIntegralEntry}
end
function CfIntegralsDesc(entries::Vector{CfIntegralEntry}; area = C_NULL, mask = C_NULL, region = C_NULL, max_workgroups = 0)
    length(entries) <= 32 || error("CoFluxMI355X: at most 32 integral entries")
    padded = ntuple(k -> k <= length(entries) ? entries[k] : CfIntegralEntry(), 32)
    return CfIntegralsDesc(sizeof(CfIntegralsDesc), length(entries), area, mask, region, max_workgroups, 0, padded)
end
mutable struct CoFluxIntegrals
    ptr::Ptr{Cvoid}
    backend::CoFluxBackend
    n_entries::Int
end
function CoFluxIntegrals(b::CoFluxBackend, desc::CfIntegralsDesc, capacity)
    out = Ref{Ptr{Cvoid}}(C_NULL)
    check(b.ctx, ccall((:cf_integrals_create, libcoflux), Cint, (Ptr{Cvoid}, Ref{CfIntegralsDesc}, Int32, Ref{Ptr{Cvoid}}),
                       b.ctx, desc, capacity, out))
    q = CoFluxIntegrals(out[], b, desc.n_entries)
    finalizer(x -> ccall((:cf_integrals_destroy, libcoflux), Cint, (Ptr{Cvoid},), x.ptr), q)
    return q
end
collect!(q::CoFluxIntegrals, time) = check(C_NULL, ccall((:cf_integrals_collect, libcoflux), Cint, (Ptr{Cvoid}, Float64), q.ptr, time))
reset!(q::CoFluxIntegrals) = check(C_NULL, ccall((:cf_integrals_reset, libcoflux), Cint, (Ptr{Cvoid},), q.ptr))
function integrals_count(q::CoFluxIntegrals)
    n = Ref{Int64}(0)
    check(C_NULL, ccall((:cf_integrals_count, libcoflux), Cint, (Ptr{Cvoid}, Ref{Int64}), q.ptr, n))
    return n[]
end
function read_integrals(q::CoFluxIntegrals, first = 0, n = integrals_count(q) - first)
    values = zeros(Float64, q.n_entries, n); times = zeros(Float64, n)   # column r is record first + r
    check(C_NULL, ccall((:cf_integrals_read, libcoflux), Cint, (Ptr{Cvoid}, Int64, Int64, Ptr{Float64}, Ptr{Float64}),
                        q.ptr, first, n, values, times))
    return (values = values, times = times)
end
attach_integrals!(b, q::Union{Nothing, CoFluxIntegrals}, stride = 1, time_origin = 0.0, step_seconds = 1.0) =
    check(b.ctx, ccall((:cf_attach_integrals, libcoflux), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Float64, Float64),
                       b.ctx, isnothing(q) ? C_NULL : q.ptr, stride, time_origin, step_seconds))

# ---- surface extrema, non-finite counts and state hashes on the device (ClimaOcean.jl:48-88, omip_simulation.jl:644-691) ----
# A monitor turns up to 16 surface fields into records of CfMonitorValue (one pass per collection) and keeps the series on
# the device: what Progress / omip_progress_callback print, the STATE_HASH words and what a NaNChecker asks, without moving a
# field.  read_monitor and monitor_status are the only host synchronisations; attach_monitor! makes time_steps! append a
# record every `stride` steps.  The hash is the library's own (include/coflux.h), not Base.hash.
const CF_MONITOR_VALUE, CF_MONITOR_ABS = Int32(0), Int32(1)
const CF_MONITOR_MAX_ENTRIES = 16
struct CfMonitorEntry
    a::Ptr{Float64}
    kind::Int32; reserved::Int32
end
CfMonitorEntry() = CfMonitorEntry(C_NULL, CF_MONITOR_VALUE, 0)
CfMonitorEntry(a, kind = CF_MONITOR_VALUE) = CfMonitorEntry(a, kind, 0)
struct CfMonitorDesc
    struct_size::Int32; n_entries::Int32
    mask::Ptr{Cvoid}
    first_cell::Int64
    max_workgroups::Int32; row_length::Int32
    entries::NTuple{16, CfMonitorEntry}
end
# first_cell = j0·Nx + i0 and row_length = Nx on a slab or tile of an Nx-wide surface; row_length = 0: the context's nx
function CfMonitorDesc(entries::Vector{CfMonitorEntry}; mask = C_NULL, first_cell = 0, max_workgroups = 0, row_length = 0)
    length(entries) <= 16 || error("CoFluxMI355X: at most 16 monitor entries")
    padded = ntuple(k -> k <= length(entries) ? entries[k] : CfMonitorEntry(), 16)
    return CfMonitorDesc(sizeof(CfMonitorDesc), length(entries), mask, first_cell, max_workgroups, row_length, padded)
end
struct CfMonitorValue      # 64 bytes
    minimum::Float64; maximum::Float64
    argmin::Int64; argmax::Int64          # global cell numbers first_cell + j·row_length + i (0-based), -1: none
    nan_count::Int64; inf_count::Int64
    first_nonfinite::Int64
    hash::UInt64
end
mutable struct CoFluxMonitor
    ptr::Ptr{Cvoid}
    backend::CoFluxBackend
    n_entries::Int
end
function CoFluxMonitor(b::CoFluxBackend, desc::CfMonitorDesc, capacity)
    out = Ref{Ptr{Cvoid}}(C_NULL)
    check(b.ctx, ccall((:cf_monitor_create, libcoflux), Cint, (Ptr{Cvoid}, Ref{CfMonitorDesc}, Int32, Ref{Ptr{Cvoid}}),
                       b.ctx, desc, capacity, out))
    m = CoFluxMonitor(out[], b, desc.n_entries)
    finalizer(x -> ccall((:cf_monitor_destroy, libcoflux), Cint, (Ptr{Cvoid},), x.ptr), m)
    return m
end
collect!(m::CoFluxMonitor, time) = check(C_NULL, ccall((:cf_monitor_collect, libcoflux), Cint, (Ptr{Cvoid}, Float64), m.ptr, time))
reset!(m::CoFluxMonitor) = check(C_NULL, ccall((:cf_monitor_reset, libcoflux), Cint, (Ptr{Cvoid},), m.ptr))
function monitor_count(m::CoFluxMonitor)
    n = Ref{Int64}(0)
    check(C_NULL, ccall((:cf_monitor_count, libcoflux), Cint, (Ptr{Cvoid}, Ref{Int64}), m.ptr, n))
    return n[]
end
function read_monitor(m::CoFluxMonitor, first = 0, n = monitor_count(m) - first)
    values = Matrix{CfMonitorValue}(undef, m.n_entries, n); times = zeros(Float64, n)   # column r is record first + r
    check(C_NULL, ccall((:cf_monitor_read, libcoflux), Cint, (Ptr{Cvoid}, Int64, Int64, Ptr{CfMonitorValue}, Ptr{Float64}),
                        m.ptr, first, n, values, times))
    return (values = values, times = times)
end
function monitor_status(m::CoFluxMonitor)   # (first bad record or -1, bit mask of its non-finite entries)
    record = Ref{Int64}(-1); entries = Ref{UInt32}(0)
    check(C_NULL, ccall((:cf_monitor_status, libcoflux), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{UInt32}), m.ptr, record, entries))
    return (record = record[], entries = entries[])
end
attach_monitor!(b, m::Union{Nothing, CoFluxMonitor}, stride = 1, time_origin = 0.0, step_seconds = 1.0) =
    check(b.ctx, ccall((:cf_attach_monitor, libcoflux), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Float64, Float64),
                       b.ctx, isnothing(m) ? C_NULL : m.ptr, stride, time_origin, step_seconds))

# ---- calendar-binned means on the device (visualize/common.jl:176-208, cache.jl:634-712) -----------------------------------
# A climatology bins up to 16 surface fields by calendar month (or any table of time intervals) while the model runs: one
# launch per sample adds the source to the field's mean over all samples and to its bin's, each the running mean a
# CoFluxAverager keeps.  `bins[f]` is a device block of n_bins ocean-grid arrays back to back; `totals[f]` may be C_NULL.
# The calendar table is (edges, bin_of_interval): strictly increasing seconds and one bin (0-based, -1: not collected) per
# interval; month(reference_date + Second(round(Int, t))) becomes the month starts as edges (monthly_table below).
const CF_CLIMATOLOGY_MAX_FIELDS, CF_CLIMATOLOGY_MAX_BINS = 16, 32
struct CfClimatologyDesc
    struct_size::Int32; n_fields::Int32; n_bins::Int32; max_workgroups::Int32
    sources::NTuple{16, Ptr{Float64}}
    totals::NTuple{16, Ptr{Float64}}
    bins::NTuple{16, Ptr{Float64}}
    reserved::NTuple{2, Int32}
end
function CfClimatologyDesc(sources, totals, bins, n_bins; max_workgroups = 0)
    n = length(sources)
    (n <= 16 && length(totals) == n && length(bins) == n) || error("CoFluxMI355X: at most 16 climatology fields, one total and one bin block each")
    pad(v) = ntuple(k -> k <= n ? Ptr{Float64}(v[k]) : Ptr{Float64}(C_NULL), 16)
    return CfClimatologyDesc(sizeof(CfClimatologyDesc), n, n_bins, max_workgroups, pad(sources), pad(totals), pad(bins), (Int32(0), Int32(0)))
end
mutable struct CoFluxClimatology
    ptr::Ptr{Cvoid}
    backend::CoFluxBackend
    n_fields::Int
    n_bins::Int
end
function CoFluxClimatology(b::CoFluxBackend, desc::CfClimatologyDesc)
    out = Ref{Ptr{Cvoid}}(C_NULL)
    check(b.ctx, ccall((:cf_climatology_create, libcoflux), Cint, (Ptr{Cvoid}, Ref{CfClimatologyDesc}, Ref{Ptr{Cvoid}}), b.ctx, desc, out))
    c = CoFluxClimatology(out[], b, desc.n_fields, desc.n_bins)
    finalizer(x -> ccall((:cf_climatology_destroy, libcoflux), Cint, (Ptr{Cvoid},), x.ptr), c)
    return c
end
# bin: 0-based, -1 collects nothing
collect!(c::CoFluxClimatology, bin, weight) =
    check(C_NULL, ccall((:cf_climatology_collect, libcoflux), Cint, (Ptr{Cvoid}, Int32, Float64), c.ptr, bin, weight))
reset!(c::CoFluxClimatology) = check(C_NULL, ccall((:cf_climatology_reset, libcoflux), Cint, (Ptr{Cvoid},), c.ptr))
function climatology_weights(c::CoFluxClimatology)
    total = Ref{Float64}(0); samples = Ref{Int64}(0); bin_totals = zeros(Float64, c.n_bins); bin_samples = zeros(Int64, c.n_bins)
    check(C_NULL, ccall((:cf_climatology_weights, libcoflux), Cint, (Ptr{Cvoid}, Ref{Float64}, Ref{Int64}, Ptr{Float64}, Ptr{Int64}),
                        c.ptr, total, samples, bin_totals, bin_samples))
    return (total = total[], samples = samples[], bin_totals = bin_totals, bin_samples = bin_samples)
end
# per interior cell min / max over the non-empty bins (Base.min / max semantics) and the 0-based bin of each; any output C_NULL
climatology_extremes!(c::CoFluxClimatology, field, d_min, d_max, d_argmin = C_NULL, d_argmax = C_NULL) =
    check(C_NULL, ccall((:cf_climatology_extremes, libcoflux), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}),
                        c.ptr, field, d_min, d_max, d_argmin, d_argmax))
function calendar_bin(edges::Vector{Float64}, bin_of_interval::Vector{Int32}, time)
    bin = Ref{Int32}(-1)
    check(C_NULL, ccall((:cf_calendar_bin, libcoflux), Cint, (Ptr{Float64}, Ptr{Int32}, Int32, Float64, Ref{Int32}),
                        edges, bin_of_interval, length(edges), time, bin))
    return bin[]
end
# the month table of compute_monthly_means for the years `years` (bins 0 … 11): monthly_table(DateTime(1958, 1, 1), 1958:1961)
function monthly_table(reference_date, years)
    starts = [DateTime(y, m, 1) for y in years for m in 1:12]
    push!(starts, DateTime(last(years) + 1, 1, 1))
    edges = Float64[Dates.value(Second(d - reference_date)) for d in starts]
    return edges, Int32[month(d) - 1 for d in starts[1:end-1]]
end
function attach_climatology!(b, c::Union{Nothing, CoFluxClimatology}, edges::Vector{Float64} = Float64[], bin_of_interval::Vector{Int32} = Int32[];
                             stride = 1, step_weight = 1.0, time_origin = 0.0, step_seconds = 1.0)
    check(b.ctx, ccall((:cf_attach_climatology, libcoflux), Cint,
                       (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Float64, Float64, Float64, Ptr{Float64}, Ptr{Int32}, Int32),
                       b.ctx, isnothing(c) ? C_NULL : c.ptr, stride, step_weight, time_origin, step_seconds, edges, bin_of_interval, length(edges)))
end

# ---- a dataset staged on the device and followed in time (omip_simulation.jl:507-523, :614-615, :634-635) ----------------
# DatasetRestoring(Metadata(:salinity; dataset = WOAMonthly()), …): stage!(d, level, plane) takes a host Matrix{Float32} of
# the dataset's own grid (ns_x × ns_y, NaN = missing), inpaints it by nearest-neighbour sweeps and interpolates it onto the
# level's ocean-grid array, with no host synchronisation; evaluate!(d, time, out) writes S★; attach_restoring_dataset! makes
# time_steps_coupled! follow it (the block's target_salinity is then C_NULL).  Levels are 0-based, as in the C ABI.
struct CfDatasetDesc
    struct_size::Int32; ns_x::Int32; ns_y::Int32; n_levels::Int32
    periodic_x::Int32; max_sweeps::Int32; sweeps_per_launch::Int32; max_workgroups::Int32
    fill_value::Float64; period::Float64
    times::Ptr{Float64}
    weights::CfInterpWeights
end
mutable struct CoFluxDataset
    ptr::Ptr{Cvoid}
    backend::CoFluxBackend
    ns_x::Int
    ns_y::Int
    times::Vector{Float64}
    period::Float64
end
function CoFluxDataset(b::CoFluxBackend, ns_x, ns_y, times::Vector{Float64}, weights::CfInterpWeights; period = 0.0, periodic_x = true,
                       max_sweeps = -1, fill_value = 0.0, sweeps_per_launch = 0, max_workgroups = 0)
    out = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve times begin
        desc = CfDatasetDesc(sizeof(CfDatasetDesc), ns_x, ns_y, length(times), periodic_x ? 1 : 0, max_sweeps, sweeps_per_launch,
                             max_workgroups, fill_value, period, pointer(times), weights)
        check(b.ctx, ccall((:cf_dataset_create, libcoflux), Cint, (Ptr{Cvoid}, Ref{CfDatasetDesc}, Ref{Ptr{Cvoid}}), b.ctx, desc, out))
    end
    d = CoFluxDataset(out[], b, ns_x, ns_y, copy(times), period)
    finalizer(x -> ccall((:cf_dataset_destroy, libcoflux), Cint, (Ptr{Cvoid},), x.ptr), d)
    return d
end
function stage!(d::CoFluxDataset, level, plane::Matrix{Float32})
    size(plane) == (d.ns_x, d.ns_y) || error("CoFluxMI355X: the plane is $(d.ns_x) × $(d.ns_y)")
    check(C_NULL, ccall((:cf_dataset_stage, libcoflux), Cint, (Ptr{Cvoid}, Int32, Ptr{Float32}), d.ptr, level, plane))
end
function dataset_level(d::CoFluxDataset, level)
    p = Ref{Ptr{Float64}}(C_NULL)
    check(C_NULL, ccall((:cf_dataset_level, libcoflux), Cint, (Ptr{Cvoid}, Int32, Ref{Ptr{Float64}}), d.ptr, level, p))
    return p[]
end
function read_source(d::CoFluxDataset)
    out = zeros(Float64, d.ns_x, d.ns_y)
    check(C_NULL, ccall((:cf_dataset_read_source, libcoflux), Cint, (Ptr{Cvoid}, Ptr{Float64}), d.ptr, out))
    return out
end
function stage_info(d::CoFluxDataset, level)
    sweeps = Ref{Int32}(0); filled = Ref{Int64}(0); defaulted = Ref{Int64}(0)
    check(C_NULL, ccall((:cf_dataset_stage_info, libcoflux), Cint, (Ptr{Cvoid}, Int32, Ref{Int32}, Ref{Int64}, Ref{Int64}),
                        d.ptr, level, sweeps, filled, defaulted))
    return (sweeps = sweeps[], filled = filled[], defaulted = defaulted[])
end
function dataset_time_index(times::Vector{Float64}, period, time)
    level1 = Ref{Int32}(-1); level2 = Ref{Int32}(-1); fraction = Ref{Float64}(NaN)
    check(C_NULL, ccall((:cf_dataset_time_index, libcoflux), Cint, (Ptr{Float64}, Int32, Float64, Float64, Ref{Int32}, Ref{Int32}, Ref{Float64}),
                        times, length(times), period, time, level1, level2, fraction))
    return (level1[], level2[], fraction[])
end
evaluate!(d::CoFluxDataset, time, out) =
    check(C_NULL, ccall((:cf_dataset_evaluate, libcoflux), Cint, (Ptr{Cvoid}, Float64, Ptr{Float64}), d.ptr, time, out))
materialize_dataset_restoring!(b, piston_velocity, d::CoFluxDataset, time, ocean::CfOceanSurface, buffer) =
    check(b.ctx, ccall((:cf_materialize_dataset_restoring, libcoflux), Cint,
                       (Ptr{Cvoid}, Float64, Ptr{Cvoid}, Float64, Ref{CfOceanSurface}, Ptr{Float64}), b.ctx, piston_velocity, d.ptr, time, ocean, buffer))
attach_restoring_dataset!(b, d::Union{Nothing, CoFluxDataset}; time_origin = 0.0, step_seconds = 1.0) =
    check(b.ctx, ccall((:cf_attach_restoring_dataset, libcoflux), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Float64, Float64),
                       b.ctx, isnothing(d) ? C_NULL : d.ptr, time_origin, step_seconds))

# ---- a fixed sparse surface operator on the device (visualize/cache.jl:918-937, 983-1011) ---------------------------------
# CSR over destination rows: `row_ptr` (0-based, n_rows + 1 entries), `col` (0-based interior cell numbers j·nx + i) and
# `weight` (≥ 0) are host arrays, copied to the device at construction — a SparseMatrixCSC of ConservativeRegridding.jl goes
# in through its transpose.  regrid!(rg, sources, destinations; coverage) applies it to up to 16 ocean-grid device fields
# in one pass: Σ w x / Σ w over the wet entries of a row (CF_REGRID_MEAN; NaN where no entry is wet) or Σ w x (CF_REGRID_SUM).
const CF_REGRID_MEAN, CF_REGRID_SUM = Int32(0), Int32(1)
const CF_REGRID_MAX_FIELDS = 16
struct CfRegridDesc
    struct_size::Int32; mode::Int32
    n_rows::Int64; nnz::Int64
    row_ptr::Ptr{Int64}; col::Ptr{Int32}; weight::Ptr{Float64}; mask::Ptr{Cvoid}
    max_workgroups::Int32; reserved::Int32
end
mutable struct CoFluxRegridder
    ptr::Ptr{Cvoid}
    backend::CoFluxBackend
    n_rows::Int
end
function CoFluxRegridder(b::CoFluxBackend, row_ptr::Vector{Int64}, col::Vector{Int32}, weight::Vector{Float64};
                         mask = C_NULL, mode = CF_REGRID_MEAN, max_workgroups = 0)
    out = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve row_ptr col weight begin
        desc = CfRegridDesc(sizeof(CfRegridDesc), mode, length(row_ptr) - 1, length(col), pointer(row_ptr), pointer(col),
                            pointer(weight), mask, max_workgroups, 0)
        check(b.ctx, ccall((:cf_regrid_create, libcoflux), Cint, (Ptr{Cvoid}, Ref{CfRegridDesc}, Ref{Ptr{Cvoid}}), b.ctx, desc, out))
    end
    rg = CoFluxRegridder(out[], b, length(row_ptr) - 1)
    finalizer(x -> ccall((:cf_regrid_destroy, libcoflux), Cint, (Ptr{Cvoid},), x.ptr), rg)
    return rg
end
function regrid!(rg::CoFluxRegridder, sources::Vector{Ptr{Float64}}, destinations::Vector{Ptr{Float64}}; coverage = C_NULL)
    length(sources) == length(destinations) || error("CoFluxMI355X: one destination per source")
    check(C_NULL, ccall((:cf_regrid_apply, libcoflux), Cint, (Ptr{Cvoid}, Int32, Ptr{Ptr{Float64}}, Ptr{Ptr{Float64}}, Ptr{Float64}),
                        rg.ptr, length(sources), sources, destinations, coverage))
end

# ---- SeaIceAlbedo(hi, hs, Ts) (atmosphere.jl:30-44) and compute_sea_ice_ocean_fluxes! (omip_simulation.jl:71-77) ------
mutable struct CfSeaIceAlbedoParams
    struct_size::Int32; reserved::Int32
    ice_visible::Float64; ice_near_infrared::Float64; snow_visible::Float64; snow_near_infrared::Float64; ocean_albedo::Float64
    reference_thickness::Float64; melt_temperature_range::Float64; ice_melt_change::Float64
    snow_melt_change_visible::Float64; snow_melt_change_near_infrared::Float64; snow_patch_thickness::Float64
    visible_fraction::Float64; melting_temperature::Float64
    CfSeaIceAlbedoParams() = new()
end
default_sea_ice_albedo_params() = (p = CfSeaIceAlbedoParams();
    ccall((:cf_default_sea_ice_albedo_params, libcoflux), Cint, (Ref{CfSeaIceAlbedoParams},), p); p)
set_sea_ice_albedo!(b, p::CfSeaIceAlbedoParams) =
    check(b.ctx, ccall((:cf_set_sea_ice_albedo, libcoflux), Cint, (Ptr{Cvoid}, Ref{CfSeaIceAlbedoParams}), b.ctx, p))
compute_sea_ice_albedo!(b, p, hi, hs, Ts, out) =
    check(b.ctx, ccall((:cf_compute_sea_ice_albedo, libcoflux), Cint,
                       (Ptr{Cvoid}, Ref{CfSeaIceAlbedoParams}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), b.ctx, p, hi, hs, Ts, out))
mutable struct CfIceOceanParams   # ThreeEquationHeatFlux(; friction_velocity = MomentumBasedFrictionVelocity())
    struct_size::Int32; reserved::Int32
    heat_transfer_coefficient::Float64; salt_transfer_coefficient::Float64; minimum_friction_velocity::Float64
    ice_density::Float64; latent_heat_of_fusion::Float64; ice_salinity::Float64; liquidus_slope::Float64
    top_cell_thickness::Float64; time_step::Float64
    CfIceOceanParams() = new()
end
struct CfIceOceanFluxes; interface_heat::Ptr{Float64}; salt_flux::Ptr{Float64}; frazil_heat::Ptr{Float64}; friction_velocity::Ptr{Float64}; end
default_ice_ocean_params() = (p = CfIceOceanParams(); ccall((:cf_default_ice_ocean_params, libcoflux), Cint, (Ref{CfIceOceanParams},), p); p)
compute_sea_ice_ocean_fluxes!(b, p::CfIceOceanParams, ocean::CfOceanSurface, concentration, x_stress, y_stress, out::CfIceOceanFluxes) =
    check(b.ctx, ccall((:cf_compute_sea_ice_ocean_fluxes, libcoflux), Cint,
                       (Ptr{Cvoid}, Ref{CfIceOceanParams}, Ref{CfOceanSurface}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{CfIceOceanFluxes}),
                       b.ctx, p, ocean, concentration, x_stress, y_stress, out))

# ---- JRA55PrescribedLand (atmosphere.jl:46) and the MultipleFluxes additional flux (omip_simulation.jl:175-206, 507-523) --
struct CfLandSource
    friver::Ptr{Float32}; licalvf::Ptr{Float32}
    ns_x::Int32; ns_y::Int32; n_levels::Int32; level1::Int32; level2::Int32; reserved::Int32
    time_fraction::Float64
end
interpolate_land_freshwater!(b, src::CfLandSource, w::CfInterpWeights, out) =
    check(b.ctx, ccall((:cf_interpolate_land_freshwater, libcoflux), Cint, (Ptr{Cvoid}, Ref{CfLandSource}, Ref{CfInterpWeights}, Ptr{Float64}),
                       b.ctx, src, w, out))
set_land_freshwater!(b, field) = check(b.ctx, ccall((:cf_set_land_freshwater, libcoflux), Cint, (Ptr{Cvoid}, Ptr{Float64}), b.ctx, field))
materialize_salinity_restoring!(b, piston_velocity, target, ocean::CfOceanSurface, buffer) =
    check(b.ctx, ccall((:cf_materialize_salinity_restoring, libcoflux), Cint,
                       (Ptr{Cvoid}, Float64, Ptr{Float64}, Ref{CfOceanSurface}, Ptr{Float64}), b.ctx, piston_velocity, target, ocean, buffer))

# ---- the coupled step: OceanSeaIceModel(ocean, sea_ice; atmosphere, land, interfaces) + restoring + NormalizeSalinity ---------
# prepare_coupled_step! is the three calls above (land freshwater, ice–ocean exchange, restoring buffer) as ONE launch, same
# bits; a job is absent when its output pointer is C_NULL.  A host that steps its own ocean calls it, then update_state_sea_ice!.
struct CfIceOceanParamsData   # the isbits twin of CfIceOceanParams: a mutable struct is a reference when it is a field
    struct_size::Int32; reserved::Int32
    heat_transfer_coefficient::Float64; salt_transfer_coefficient::Float64; minimum_friction_velocity::Float64
    ice_density::Float64; latent_heat_of_fusion::Float64; ice_salinity::Float64; liquidus_slope::Float64
    top_cell_thickness::Float64; time_step::Float64
end
CfIceOceanParamsData(p::CfIceOceanParams) = CfIceOceanParamsData(ntuple(i -> getfield(p, i), fieldcount(CfIceOceanParams))...)
struct CfCoupledPrepare
    struct_size::Int32; reserved::Int32
    ocean::CfOceanSurface
    weights::CfInterpWeights
    land::CfLandSource
    land_freshwater::Ptr{Float64}
    ice_ocean::CfIceOceanParamsData
    concentration::Ptr{Float64}; x_stress::Ptr{Float64}; y_stress::Ptr{Float64}
    ice_ocean_fluxes::CfIceOceanFluxes
    piston_velocity::Float64
    target_salinity::Ptr{Float64}; restoring_buffer::Ptr{Float64}
end
prepare_coupled_step!(b, p::CfCoupledPrepare) =
    check(b.ctx, ccall((:cf_prepare_coupled_step, libcoflux), Cint, (Ptr{Cvoid}, Ref{CfCoupledPrepare}), b.ctx, p))
# time_steps_coupled!: time_steps! of that configuration — per step the preamble, update_state_sea_ice! on ice state
# s mod n_ice_states with the CARRIED skin temperature, and NormalizeSalinity — without returning to Julia.
struct CfCoupledStep
    struct_size::Int32; n_ice_states::Int32
    ice_states::Ptr{CfSeaIceState}
    skin_temperature::Ptr{Float64}
    ai_fluxes::CfInterfaceFluxes
    net_ice::CfNetSeaIceFluxes
    land::CfLandSource
    land_first_level::Int32; compute_ice_ocean::Int32
    land_time_fraction::Float64; land_time_fraction_increment::Float64
    land_freshwater::Ptr{Float64}
    ice_ocean::CfIceOceanParamsData
    ice_ocean_fluxes::CfIceOceanFluxes
    piston_velocity::Float64
    target_salinity::Ptr{Float64}; restoring_buffer::Ptr{Float64}
    normalize_salinity::Int32; reserved::Int32
    area::Ptr{Float64}; mean_out::Ptr{Float64}
end
time_steps_coupled!(b, first_step, nsteps, sched::CfRunSchedule, src, w, fluxes, ice, net, coupled::CfCoupledStep) =
    check(b.ctx, ccall((:cf_time_steps_coupled, libcoflux), Cint,
                       (Ptr{Cvoid}, Int64, Cint, Ref{CfRunSchedule}, Ref{CfAtmosSource}, Ref{CfInterpWeights}, Ref{CfInterfaceFluxes},
                        Ptr{CfSeaIceFields}, Ref{CfNetOceanFluxes}, Ref{CfCoupledStep}),
                       b.ctx, first_step, nsteps, sched, src, w, fluxes, ice, net, coupled))

# ---- checkpoint and pickup (run!(sim; pickup = true), omip_simulation.jl:241-247; Checkpointer, omip_diagnostics.jl:220-225) ----
# A checkpoint packs registered device arrays (whole parent arrays) and the private state of averagers, climatologies,
# integrators and monitors into one byte string — this library's own format, not JLD2 — and puts it back bit for bit:
#   cp = CoFluxCheckpoint(b); add!(cp, "T", pointer(T), sizeof(T)); add!(cp, "averages", avg); set_host_blob!(cp, codeunits(json))
#   capture!(cp); …further steps…; write(io, wait_image(cp))          # the image drains while the steps run
#   restore!(cp, read(path)); sync(b)                                 # in the next process, after the same registration
const CF_CHECKPOINT_MAX_SECTIONS, CF_CHECKPOINT_DIRECT = 256, 1
struct CfCheckpointDesc
    struct_size::Int32; flags::Int32; max_workgroups::Int32; reserved::Int32
end
mutable struct CoFluxCheckpoint
    ptr::Ptr{Cvoid}
    backend::CoFluxBackend
    kept::Vector{Any}   # the registered handles and the blob stay alive with the checkpoint
end
function CoFluxCheckpoint(b::CoFluxBackend; direct = false, max_workgroups = 0)
    desc = CfCheckpointDesc(sizeof(CfCheckpointDesc), direct ? CF_CHECKPOINT_DIRECT : 0, max_workgroups, 0)
    out = Ref{Ptr{Cvoid}}(C_NULL)
    check(b.ctx, ccall((:cf_checkpoint_create, libcoflux), Cint, (Ptr{Cvoid}, Ref{CfCheckpointDesc}, Ref{Ptr{Cvoid}}), b.ctx, desc, out))
    cp = CoFluxCheckpoint(out[], b, Any[])
    finalizer(x -> ccall((:cf_checkpoint_destroy, libcoflux), Cint, (Ptr{Cvoid},), x.ptr), cp)
    return cp
end
add!(cp::CoFluxCheckpoint, name::String, d_ptr::Ptr, bytes::Integer) =
    check(C_NULL, ccall((:cf_checkpoint_add_array, libcoflux), Cint, (Ptr{Cvoid}, Cstring, Ptr{Cvoid}, Csize_t), cp.ptr, name, d_ptr, bytes))
function add!(cp::CoFluxCheckpoint, name::String, a::CoFluxAverage)
    check(C_NULL, ccall((:cf_checkpoint_add_average, libcoflux), Cint, (Ptr{Cvoid}, Cstring, Ptr{Cvoid}), cp.ptr, name, a.ptr)); push!(cp.kept, a); nothing
end
function add!(cp::CoFluxCheckpoint, name::String, c::CoFluxClimatology)
    check(C_NULL, ccall((:cf_checkpoint_add_climatology, libcoflux), Cint, (Ptr{Cvoid}, Cstring, Ptr{Cvoid}), cp.ptr, name, c.ptr)); push!(cp.kept, c); nothing
end
function add!(cp::CoFluxCheckpoint, name::String, q::CoFluxIntegrals)
    check(C_NULL, ccall((:cf_checkpoint_add_integrals, libcoflux), Cint, (Ptr{Cvoid}, Cstring, Ptr{Cvoid}), cp.ptr, name, q.ptr)); push!(cp.kept, q); nothing
end
function add!(cp::CoFluxCheckpoint, name::String, m::CoFluxMonitor)
    check(C_NULL, ccall((:cf_checkpoint_add_monitor, libcoflux), Cint, (Ptr{Cvoid}, Cstring, Ptr{Cvoid}), cp.ptr, name, m.ptr)); push!(cp.kept, m); nothing
end
set_host_blob!(cp::CoFluxCheckpoint, blob::AbstractVector{UInt8}) =
    check(C_NULL, ccall((:cf_checkpoint_set_host_blob, libcoflux), Cint, (Ptr{Cvoid}, Ptr{UInt8}, Csize_t), cp.ptr, blob, length(blob)))
capture!(cp::CoFluxCheckpoint) = check(C_NULL, ccall((:cf_checkpoint_capture, libcoflux), Cint, (Ptr{Cvoid},), cp.ptr))
# the finished image (a copy: the library's pinned buffer is reused by the next capture)
function wait_image(cp::CoFluxCheckpoint)
    p = Ref{Ptr{Cvoid}}(C_NULL); n = Ref{Csize_t}(0)
    check(C_NULL, ccall((:cf_checkpoint_wait, libcoflux), Cint, (Ptr{Cvoid}, Ref{Ptr{Cvoid}}, Ref{Csize_t}), cp.ptr, p, n))
    return copy(unsafe_wrap(Array, Ptr{UInt8}(p[]), Int(n[])))
end
restore!(cp::CoFluxCheckpoint, image::Vector{UInt8}) =
    check(C_NULL, ccall((:cf_checkpoint_restore, libcoflux), Cint, (Ptr{Cvoid}, Ptr{UInt8}, Csize_t), cp.ptr, image, length(image)))
checkpoint_verify(image::Vector{UInt8}) = check(C_NULL, ccall((:cf_checkpoint_verify, libcoflux), Cint, (Ptr{UInt8}, Csize_t), image, length(image)))
function checkpoint_hash(bytes::Vector{UInt8})
    h = Ref{UInt64}(0)
    check(C_NULL, ccall((:cf_checkpoint_hash, libcoflux), Cint, (Ptr{UInt8}, Csize_t, Ref{UInt64}), bytes, length(bytes), h))
    return h[]
end
function checkpoint_host_blob(image::Vector{UInt8})
    p = Ref{Ptr{Cvoid}}(C_NULL); n = Ref{Csize_t}(0)
    check(C_NULL, ccall((:cf_checkpoint_host_blob, libcoflux), Cint, (Ptr{UInt8}, Csize_t, Ref{Ptr{Cvoid}}, Ref{Csize_t}), image, length(image), p, n))
    return image[(Int(p[] - pointer(image)) + 1):(Int(p[] - pointer(image)) + Int(n[]))]
end

end # module
