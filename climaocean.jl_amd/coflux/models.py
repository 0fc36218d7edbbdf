"""Host-side mirror of the user-facing API around the flux path — same names, argument meaning
and call order as the reference:

    grid       = LatitudeLongitudeGrid(size=(1440, 560, 10), halo=(7, 7, 7), longitude=(0, 360),
                                       latitude=(-70, 70), z=(-3000, 0))          # README.md:56-61
    ocean      = ocean_simulation(grid)                                            # README.md:67
    atmosphere = JRA55PrescribedAtmosphere()                                       # README.md:74
    coupled    = OceanSeaIceModel(ocean; atmosphere)                               # README.md:75
    simulation = Simulation(coupled, Δt=20minutes, stop_time=30days); run!(sim)    # README.md:76-77

Only the flux path is implemented: `time_step!(coupled)` advances the clock, lets
the ocean component step (the hydrostatic dynamical core is OUT OF SCOPE — `ocean_simulation`
returns a prescribed-state ocean whose step is a no-op unless a callback is given) and then runs
`update_state!`, which is the accelerated part: interpolate_atmosphere_state! →
compute_atmosphere_ocean_fluxes! → compute_net_ocean_fluxes!, all inside libcoflux on the GPU.
The net fluxes land in the ocean's top-boundary-condition fields exactly where the reference puts
them (model.interfaces.net_fluxes.ocean.{u,v,T,S}, omip_diagnostics.jl:77-80).

The atmosphere holds a window of snapshots in HBM filled from a provider: synthetic in tests/bench, or the raw
Float32 plane files of coflux/jra55.py (`omip_forcing`; NetCDF decoding itself is not possible in this image).

This module is the facade: the components, the interfaces, the model, its steps and run!(simulation) are here; the grids
(grids.py), the forcing components (forcing.py), the clocks (clocks.py), the schedules (schedules.py), the output writers and
callbacks (outputs.py) and the Checkpointer (checkpointing.py) are re-exported under the names they have always had here.
"""
import sys
from dataclasses import dataclass, field
from types import SimpleNamespace
from typing import Optional

import numpy as np
import torch

from . import abi, synthetic  # noqa: F401
from . import interface_computations as ic
from .checkpointing import Checkpointer
from .clocks import calendar_bins, days, device_stretches, hours, minutes  # noqa: F401
from .forcing import JRA55PrescribedAtmosphere, JRA55PrescribedLand, JRA55PrescribedRadiation, Radiation, omip_forcing  # noqa: F401
from .grids import EARTH_RADIUS, LatitudeLongitudeGrid, TripolarGrid  # noqa: F401
from .outputs import (BUDGET_OUTPUTS, CP_OCEAN, MONITOR_COLUMNS, REGION_GLOBAL, REGION_NORTH, REGION_SOUTH, RHO_OCEAN,  # noqa: F401
                      SURFACE_FLUX_OUTPUTS, BudgetTerm, CenteredX, CenteredXSquare, CenteredY, CenteredYSquare, East, KineticEnergy,
                      MonthlyClimatology, NaNChecker, North, OmipProgress, Product, Progress, Scaled, Squared, SurfaceExpression,
                      SurfaceExtrema, SurfaceFluxAverages, SurfaceIntegrals, budget_inputs, geographic_surface_outputs, grid_rotation,
                      hemisphere_regions, omip_budget_outputs, omip_progress_callback, omip_surface_outputs, prettytime,
                      _julia, _SeriesWriter, sea_ice_concentration_climatology, sea_ice_integrals, surface_global_means, variance)
from .runtime import BUDGET_KINDS, EXCHANGE_NAMES, FLUX_NAMES, FLUX_OPTIONAL, NET_NAMES, FluxContext, calendar_bin  # noqa: F401
from .schedules import AveragedTimeInterval, IterationInterval, TimeInterval, actuates, as_schedule, open_at  # noqa: F401


# ---------------------------------------------------------------------------------------------
# ocean (boundary only: surface state in, top-BC flux fields out)
# ---------------------------------------------------------------------------------------------
@dataclass
class SurfaceFluxRestoring:
    """SurfaceFluxRestoring(DatasetRestoring(…; rate = piston_velocity / (Δz days))) — salinity_surface_restoring,
    omip_simulation.jl:507-523: a surface-only restoring toward `target` (2-D, halo-inclusive device array, g/kg) that rides
    on the ocean's top-flux boundary condition through `additional_surface_fluxes`.  piston_velocity in m/day as there."""
    target: object   # a 2-D device array, or a DatasetRestoring: S★ then follows the dataset in time
    piston_velocity: float = 1.0 / 6.0

    @property
    def velocity(self):
        return self.piston_velocity / days


class DatasetRestoring:
    """DatasetRestoring(Metadata(:salinity; dataset = WOAMonthly()), arch; time_indices_in_memory = length(metadata)) —
    salinity_surface_restoring, omip_simulation.jl:507-523: every level of the dataset resident on the device, each
    land-inpainted on the dataset's own grid and interpolated to the ocean grid, blended linearly in time — cyclically over
    `period` [s] when it is > 0, clamped at the ends otherwise.  `planes`: host array [n, ns_y, ns_x] on a global regular
    latitude–longitude grid laid out as the JRA55 record is (NaN = missing); `times` [s]: the levels' times on the model's
    clock.  Given as the `target` of a SurfaceFluxRestoring.  Staged once per context, on first use (cf_dataset_*)."""

    def __init__(self, planes, times, period=0.0, *, periodic_x=True, max_sweeps=-1, fill_value=0.0, sweeps_per_launch=0):
        self.planes = np.asarray(planes, dtype=np.float32)
        self.times = [float(t) for t in times]
        if self.planes.ndim != 3 or self.planes.shape[0] != len(self.times):
            raise ValueError(f"DatasetRestoring: planes is [n, ns_y, ns_x] with one time per level, got {self.planes.shape} and {len(self.times)} times")
        self.period = float(period)
        self.options = dict(periodic_x=periodic_x, max_sweeps=max_sweeps, fill_value=fill_value, sweeps_per_launch=sweeps_per_launch)
        self._staged = None   # (context, Dataset)

    def dataset(self, ctx, grid):
        """The staged runtime.Dataset on `ctx` (the levels are uploaded, inpainted and regridded the first time)."""
        if self._staged is None or self._staged[0] is not ctx:
            ns_y, ns_x = self.planes.shape[1:]
            d = ctx.dataset(ns_x, ns_y, self.times, grid.interpolation_weights(ctx.to_device, ns_x, ns_y), period=self.period, **self.options)
            for level, plane in enumerate(self.planes):
                d.stage(level, plane)
            self._staged = (ctx, d)
        return self._staged[1]


def set_from_dataset(field, plane, ctx, grid, *, periodic_x=True, max_sweeps=-1, fill_value=0.0):
    """set!(field, Metadatum(…)) — the initial conditions of omip_simulation.jl:614-615, :634-635: one plane of a dataset
    (host array [ns_y, ns_x], NaN = missing) inpainted and interpolated onto the ring window of `field`, a halo-inclusive 2-D
    device array of the context's shape (the top level of a 3-D field, say)."""
    plane = np.asarray(plane, dtype=np.float32)
    ns_y, ns_x = plane.shape
    d = ctx.dataset(ns_x, ns_y, [0.0], grid.interpolation_weights(ctx.to_device, ns_x, ns_y), periodic_x=periodic_x, max_sweeps=max_sweeps,
                    fill_value=fill_value)
    try:
        d.stage(0, plane)
        d.evaluate(0.0, field)
        ctx.sync()
    finally:
        d.close()
    return field


@dataclass
class MultipleFluxes:
    """MultipleFluxes{flux_field, additional_fluxes} (omip_simulation.jl:175-206): the top boundary condition of a tracer
    when `ocean_simulation(grid; additional_surface_fluxes = (; S = …))` is used.  The coupled model writes the bulk flux
    into `flux_field`; the ocean applies flux_field + additional_fluxes."""
    flux_field: torch.Tensor
    additional_fluxes: object


class OceanSimulation:
    """What `ocean_simulation(grid)` returns: `.model.tracers.{T,S}`, `.model.velocities.{u,v}` as
    (Nz+2Hz, Ny+2Hy, Nx+2Hx) device arrays (k slowest), `.model.clock`, and the top boundary
    condition fields the coupled model writes (omip_simulation.jl:175-206: a bare 2-D field, or MultipleFluxes when
    `additional_surface_fluxes` is given)."""

    def __init__(self, grid, step_callback=None, additional_surface_fluxes=None):
        dev = torch.device("cuda", grid.device)
        nz, hz = grid.size[2], grid.halo[2]
        shape3 = (nz + 2 * hz,) + grid.surface_shape
        z3 = lambda: torch.zeros(shape3, dtype=torch.float64, device=dev)  # noqa: E731
        z2 = lambda: torch.zeros(grid.surface_shape, dtype=torch.float64, device=dev)  # noqa: E731
        self.grid = grid
        self.k_top = hz + nz - 1
        self.model = SimpleNamespace(
            grid=grid,
            tracers=SimpleNamespace(T=z3(), S=z3()),
            velocities=SimpleNamespace(u=z3(), v=z3()),
            clock=SimpleNamespace(time=0.0, iteration=0),
            wet_mask=torch.ones(grid.surface_shape, dtype=torch.uint8, device=dev),
            top_boundary_conditions=SimpleNamespace(u=z2(), v=z2(), T=z2(), S=z2()),
            shortwave_surface_flux=z2())  # radiation.surface_flux, KPP/kpp_surface_forcing.jl:47-51
        self.step_callback = step_callback
        for name, extra in (additional_surface_fluxes or {}).items():
            bc = self.model.top_boundary_conditions
            setattr(bc, name, MultipleFluxes(getattr(bc, name), extra))

    def surface_state(self):
        m, k = self.model, self.k_top
        return dict(T=m.tracers.T[k], S=m.tracers.S[k], u=m.velocities.u[k], v=m.velocities.v[k], mask=m.wet_mask)

    def time_step(self, dt):
        if self.step_callback is not None:
            self.step_callback(self, dt)
        self.model.clock.time += dt
        self.model.clock.iteration += 1


def ocean_simulation(grid, **kw):
    """README.md:67; OceanConfigurations/latitude_longitude.jl:50-55."""
    return OceanSimulation(grid, **kw)


def set_surface(ocean, *, T=None, S=None, u=None, v=None, mask=None):
    """set!(ocean.model, T=…, S=…) for the top level (README.md:69-71), from host arrays with halos."""
    m, k = ocean.model, ocean.k_top
    for tgt, src in ((m.tracers.T, T), (m.tracers.S, S), (m.velocities.u, u), (m.velocities.v, v)):
        if src is not None:
            tgt[k].copy_(torch.as_tensor(np.ascontiguousarray(src)))
    if mask is not None:
        m.wet_mask.copy_(torch.as_tensor(np.ascontiguousarray(mask)))


@dataclass
class PrescribedSeaIce:
    """The sea-ice inputs the partition reads (atmosphere.jl:34-39, src/ClimaOcean.jl:62-63); a
    prognostic ClimaSeaIce model is out of scope, its fields are taken as given."""
    concentration: torch.Tensor
    interface_heat: Optional[torch.Tensor] = None
    salt_flux: Optional[torch.Tensor] = None
    x_stress: Optional[torch.Tensor] = None
    y_stress: Optional[torch.Tensor] = None
    # sea_ice.model.{ice_thickness, ice_thermodynamics.top_surface_temperature, velocities} (atmosphere.jl:34-39):
    # with these the atmosphere–sea-ice interface is solved too and top_surface_temperature is updated in place
    thickness: Optional[torch.Tensor] = None
    top_surface_temperature: Optional[torch.Tensor] = None   # °C
    u: Optional[torch.Tensor] = None
    v: Optional[torch.Tensor] = None
    albedo: Optional[torch.Tensor] = None
    frazil_heat: Optional[torch.Tensor] = None
    snow_thickness: Optional[torch.Tensor] = None            # sea_ice.model.snow_thickness (atmosphere.jl:34)

    def fields(self):
        return {k: getattr(self, k) for k in ("concentration", "interface_heat", "salt_flux", "x_stress", "y_stress")
                if getattr(self, k) is not None}

    def has_surface_state(self):
        return self.thickness is not None and self.top_surface_temperature is not None

    def surface_state(self):
        st = dict(concentration=self.concentration, thickness=self.thickness, top_temperature=self.top_surface_temperature)
        for k in ("u", "v", "albedo", "snow_thickness"):
            if getattr(self, k) is not None:
                st[k] = getattr(self, k)
        return st


# ---------------------------------------------------------------------------------------------
# ComponentInterfaces / OceanSeaIceModel
# ---------------------------------------------------------------------------------------------
class ExchangeStates:
    """The two sets of exchange fields behind interfaces.exchange_atmosphere_state, and everything that decides which of them
    holds the state at the model's clock.  The reference updates ONE field set in place.  Here, outside run!(simulation) the
    state is always in set 0 (`stable`: tensors that a writer or a diagnostic may hold on to); inside run! the clock is known
    one step ahead, so every step's solver launch also interpolates the NEXT step's state, into the other set, and the
    current state alternates between the two — read it through `current` there, do not keep the dict or its tensors across
    steps.  settle() is the way out of run!: the final state in set 0, nothing requested, the context's options as they were."""

    def __init__(self, context, stable):
        self.context = context
        self._sets = [stable, None]    # (the other set is made by the first request)
        self._current = 0
        self._requested = False        # the next step's state has been requested into the other set
        self._tail_option = False      # CF_OPT_MERGED_PREFETCH = 2 is set on the context
        self.stepping_dt = None        # the Δt run!(simulation) steps with; None outside it

    @property
    def stable(self):
        return self._sets[0]

    @property
    def current(self):
        return self._sets[self._current]

    @property
    def other(self):
        """The set that is not current; None until a request has made it."""
        return self._sets[1 - self._current]

    @property
    def inside_run(self):
        return self.stepping_dt is not None or self._requested

    def begin_step(self):
        """A step begins: the state the previous step requested is this step's, and it is in the other set."""
        if self._requested:
            self._current = 1 - self._current
            self._requested = False

    def request_next(self, atmosphere, weights, time):
        """The atmosphere state at `time`, the next step's, is requested into the other set and rides in this step's solver
        launch (CF_OPT_MERGED_PREFETCH = 2: tail workgroups; the same bits as interpolating it when its step comes)."""
        if self.other is None:
            self._sets[1 - self._current] = self.context.field_set(EXCHANGE_NAMES)
        if not self._tail_option:   # (restored by settle: a lone update_state! is ≈ 5 µs slower on the tail plan)
            self.context.set_option(abi.OPT_MERGED_PREFETCH, 2)
            self._tail_option = True
        src, n1, n2, frac = atmosphere.source(self.context, time)
        self.context.prefetch_atmosphere_state(src, weights, self.other, level1=n1, level2=n2, time_fraction=frac)
        self._requested = True      # (the next begin_step swaps the sets: until then `current` is the state at the model's clock)

    def drop_request(self):
        """The requested state of a step that will not run is forgotten, here and in the library."""
        self._requested = False
        self.context.discard_prefetched_atmosphere_state()

    def restore(self, fields):
        """Set 0 ← `fields` (a checkpoint's exchange state), and set 0 is current."""
        self._current = 0
        for k, t in fields.items():
            self._sets[0][k].copy_(t)

    def settle(self):
        """The state at the model's clock goes back to set 0 (what callers may hold), the pending request is dropped, and the
        context returns to the options it had: the chunk plan of a lone update_state!, the auxiliary-stream prefetch."""
        self.stepping_dt = None
        self.drop_request()
        if self._current != 0:
            for k, t in self._sets[0].items():
                t.copy_(self._sets[1][k])
            self._current = 0
        if self._tail_option:
            self.context.set_option(abi.OPT_MERGED_PREFETCH, 0)
            self._tail_option = False


class ComponentInterfaces:
    """ComponentInterfaces(atmosphere, ocean, sea_ice; radiation, atmosphere_ocean_fluxes,
    atmosphere_ocean_velocity_difference, ocean_minimum_salinity) — omip_simulation.jl:128-158."""

    @property
    def exchange_atmosphere_state(self):
        return self.exchange.current

    def require_land_freshwater(self):
        """interfaces.land_freshwater, made when a model with land first needs it."""
        if self.land_freshwater is None:
            self.land_freshwater = self.context.zeros()
        return self.land_freshwater

    def __init__(self, atmosphere, ocean, sea_ice=None, *, radiation=None, atmosphere_ocean_fluxes=None,
                 atmosphere_sea_ice_fluxes=None, atmosphere_ocean_velocity_difference=None,
                 atmosphere_sea_ice_velocity_difference=None, sea_ice_properties=None, ocean_minimum_salinity=0.0,
                 ocean_properties=None, store_similarity_scales=False, sea_ice_ocean_heat_flux=None,
                 sea_ice_albedo=None, time_step=20 * minutes, solver_path="exact", certified_budget=8e-7,
                 ice_free_cells="iterate"):
        grid = ocean.grid
        (nx, ny, _), (hx, hy, _) = grid.size, grid.halo
        self.radiation = radiation or Radiation()
        self.atmosphere_ocean_fluxes = atmosphere_ocean_fluxes or ic.SimilarityTheoryFluxes()
        props = ocean_properties or ic.OceanProperties(surface_z=grid.surface_z)
        params = ic.flux_params(self.atmosphere_ocean_fluxes,
                                velocity_difference=atmosphere_ocean_velocity_difference,
                                ocean=props, ocean_surface=self.radiation.ocean_surface,
                                reference_height=atmosphere.reference_height,
                                boundary_layer_height=atmosphere.boundary_layer_height,
                                ocean_minimum_salinity=ocean_minimum_salinity,
                                stefan_boltzmann_constant=self.radiation.stefan_boltzmann_constant)
        self.context = FluxContext(nx, ny, hx, hy, params, ring=1, device=grid.device)
        ctx = self.context
        # implementation choices of this backend, not reference keywords (include/coflux.h): how the similarity fixed point is
        # reached — "exact" = the reference's iteration, "certified" = the reduced-iteration solve, every cell within
        # `certified_budget` of the exact path's fluxes — and what the sea-ice interface does on open water
        if solver_path not in ("exact", "certified") or ice_free_cells not in ("iterate", "zero"):
            raise ValueError(f"solver_path = {solver_path!r} (exact | certified), ice_free_cells = {ice_free_cells!r} (iterate | zero)")
        if solver_path == "certified":
            ctx.set_option(abi.OPT_CERTIFIED_BUDGET, int(round(certified_budget * 1e9)))
            ctx.set_option(abi.OPT_SOLVER_PATH, abi.SOLVER_PATH_CERTIFIED)
        if ice_free_cells == "zero":
            ctx.set_option(abi.OPT_ICE_FREE_CELLS, abi.ICE_FREE_ZERO)
        self.weights = grid.interpolation_weights(ctx.to_device)
        self.fold_north = bool(getattr(grid, "fold_north", False))
        self.exchange = ExchangeStates(ctx, ctx.field_set(EXCHANGE_NAMES))   # behind interfaces.exchange_atmosphere_state
        self.land_freshwater = None    # require_land_freshwater()
        self._grid_rotation = None     # outputs.grid_rotation(model)
        fluxes = ctx.field_set(FLUX_NAMES, FLUX_OPTIONAL if store_similarity_scales else ())
        self.atmosphere_ocean_interface = SimpleNamespace(fluxes=SimpleNamespace(**fluxes), _fields=fluxes)
        bc = ocean.model.top_boundary_conditions
        field_of = lambda b: b.flux_field if isinstance(b, MultipleFluxes) else b  # noqa: E731
        net = dict(u=field_of(bc.u), v=field_of(bc.v), T=field_of(bc.T), S=field_of(bc.S),
                   shortwave_surface_flux=ocean.model.shortwave_surface_flux,
                   upwelling_longwave=ctx.zeros(), downwelling_longwave=ctx.zeros(), downwelling_shortwave=ctx.zeros())
        self.net_fluxes = SimpleNamespace(ocean=SimpleNamespace(**net), _ocean_fields=net)
        # atmosphere–sea-ice interface (omip_simulation.jl:145,154; atmosphere.jl:34-44)
        self.atmosphere_sea_ice_interface = None
        if sea_ice is not None and sea_ice.has_surface_state():
            self.atmosphere_sea_ice_fluxes = atmosphere_sea_ice_fluxes or ic.SimilarityTheoryFluxes(
                stability_functions=ic.atmosphere_sea_ice_stability_functions())
            ice_params = ic.flux_params(self.atmosphere_sea_ice_fluxes,
                                        velocity_difference=atmosphere_sea_ice_velocity_difference, ocean=props,
                                        reference_height=atmosphere.reference_height,
                                        boundary_layer_height=atmosphere.boundary_layer_height,
                                        stefan_boltzmann_constant=self.radiation.stefan_boltzmann_constant)
            self.sea_ice_properties = sea_ice_properties or ic.SeaIceInterfaceProperties()
            ctx.set_sea_ice_formulation(ice_params, self.sea_ice_properties.to_params())
            ai = ctx.field_set(FLUX_NAMES, FLUX_OPTIONAL if store_similarity_scales else ())
            self.atmosphere_sea_ice_interface = SimpleNamespace(fluxes=SimpleNamespace(**ai), _fields=ai)
            net_ice = ctx.field_set(("top_heat", "bottom_heat"))
            self.net_fluxes.sea_ice = SimpleNamespace(**net_ice)
            self.net_fluxes._sea_ice_fields = net_ice
            # SurfaceRadiationProperties(SeaIceAlbedo(hi, hs, Ts), 1.0), atmosphere.jl:39-44
            if sea_ice_albedo is not None:
                ctx.set_sea_ice_albedo(sea_ice_albedo.to_params())
        # sea_ice_ocean_heat_flux = ThreeEquationHeatFlux(...) (omip_simulation.jl:145,154): the ice–ocean exchange and
        # frazil are then computed here each step instead of being taken from the sea-ice component
        self.sea_ice_ocean_heat_flux = None
        if sea_ice is not None and sea_ice_ocean_heat_flux is not None:
            dz = (grid.z[1] - grid.z[0]) / grid.size[2]
            self.sea_ice_ocean_heat_flux = sea_ice_ocean_heat_flux
            self.ice_ocean_params = sea_ice_ocean_heat_flux.to_params(dz, time_step)
            self.sea_ice_ocean_fluxes = ctx.field_set(("interface_heat", "salt_flux", "frazil_heat", "friction_velocity"))


class OceanSeaIceModel:
    """OceanSeaIceModel(ocean[, sea_ice]; atmosphere, radiation, interfaces) — README.md:75,
    examples/one_degree_tripolar_ocean_sea_ice.jl:42, omip_simulation.jl:132,163."""

    def __init__(self, ocean, sea_ice=None, *, atmosphere, radiation=None, interfaces=None, land=None):
        self.ocean, self.sea_ice, self.atmosphere, self.land = ocean, sea_ice, atmosphere, land
        self.interfaces = interfaces or ComponentInterfaces(atmosphere, ocean, sea_ice, radiation=radiation)
        self.clock = SimpleNamespace(time=0.0, iteration=0)
        update_state(self)


def build_coupled_model(ocean, sea_ice, atmosphere, radiation, land, flux_configuration, *, velocity_formulation="relative",
                        ocean_minimum_salinity=1, allow_shear_aware=False, shear_gustiness_coefficient=0.04):
    """build_coupled_model(ocean, sea_ice, atmosphere, radiation, land, flux_configuration; velocity_formulation = :relative,
    ocean_minimum_salinity = 1) — /root/reference/src/OMIPConfigurations/omip_simulation.jl:115-164, the same three-way
    switch and the same error strings.  Options for `flux_configuration`: "default", "corrected", "ncar" (Julia symbols
    as strings); for `velocity_formulation`: "relative", "wind".  With allow_shear_aware=True (not a reference keyword)
    "shear_aware" — the configuration launch.sh:67-72,350 describes and the reference's own switch rejects — builds the
    `:corrected` interfaces with the shear-aware gustiness (c = shear_gustiness_coefficient); without the flag it raises
    the reference's error."""
    flux_configuration = str(flux_configuration).lstrip(":")
    velocity_formulation = str(velocity_formulation).lstrip(":")
    albedo = getattr(getattr(radiation, "sea_ice_surface", None), "albedo", None)
    common = dict(radiation=radiation, ocean_minimum_salinity=float(ocean_minimum_salinity),
                  sea_ice_albedo=albedo if isinstance(albedo, ic.SeaIceAlbedo) else None)
    if flux_configuration == "default":
        interfaces = ComponentInterfaces(atmosphere, ocean, sea_ice, **common)
        return OceanSeaIceModel(ocean, sea_ice, atmosphere=atmosphere, land=land, interfaces=interfaces)
    if velocity_formulation == "relative":
        velocity_difference = ic.RelativeVelocity()
    elif velocity_formulation == "wind":
        velocity_difference = ic.WindVelocity()
    else:
        raise ValueError(f"Unknown velocity_formulation: {velocity_formulation}. Options: :relative, :wind")
    if flux_configuration == "corrected":
        ao, ai = ic.corrected_atmosphere_ocean_fluxes(), ic.corrected_atmosphere_sea_ice_fluxes()
    elif flux_configuration == "ncar":
        ao, ai = ic.ncar_atmosphere_ocean_fluxes(), ic.ncar_atmosphere_sea_ice_fluxes()
    elif flux_configuration == "shear_aware" and allow_shear_aware:
        ao = ic.shear_aware_atmosphere_ocean_fluxes(shear_gustiness_coefficient=shear_gustiness_coefficient)
        ai = ic.corrected_atmosphere_sea_ice_fluxes()
    else:
        raise ValueError(f"Unknown flux_configuration: {flux_configuration}. Options: :default, :corrected, :ncar")
    interfaces = ComponentInterfaces(atmosphere, ocean, sea_ice, atmosphere_ocean_fluxes=ao, atmosphere_sea_ice_fluxes=ai,
                                     sea_ice_ocean_heat_flux=ic.corrected_ice_ocean_heat_flux() if sea_ice is not None else None,
                                     atmosphere_ocean_velocity_difference=velocity_difference,
                                     atmosphere_sea_ice_velocity_difference=velocity_difference, **common)
    return OceanSeaIceModel(ocean, sea_ice, atmosphere=atmosphere, land=land, interfaces=interfaces)


def OceanOnlyModel(ocean, *, atmosphere, **kw):
    """docs/src/index.md:64 alias."""
    return OceanSeaIceModel(ocean, None, atmosphere=atmosphere, **kw)


def update_state(model):
    """update_state!(coupled_model) — the accelerated path."""
    itf, atm = model.interfaces, model.atmosphere
    src, n1, n2, frac = atm.source(itf.context, model.clock.time)
    if itf.fold_north:
        # TripolarGrid: the north halo of the ocean surface state is the fold of its own rows (Oceananigans' zipper
        # boundary fills it in the reference; here cf_fold_north_halo, ring + 1 rows: the solver's ring row reads v[j+1])
        st = model.ocean.surface_state()
        itf.context.fold_north_halo([st["T"], st["S"], st["u"], st["v"]],
                                    [abi.FOLD_CENTER, abi.FOLD_CENTER, abi.FOLD_X_FACE, abi.FOLD_Y_FACE], [1.0, 1.0, -1.0, -1.0], rows=2)
    if getattr(model, "land", None) is not None:
        # JRA55PrescribedLand: river discharge + calving at the model time, handed to compute_net_ocean_fluxes!
        land, freshwater = model.land, itf.require_land_freshwater()
        l1, l2, lfrac = land.levels(model.clock.time)   # (the record's calendar: cyclic repeat year / clamped multi-year)
        itf.context.interpolate_land_freshwater(land.data["friver"], land.data.get("licalvf"), itf.weights, freshwater,
                                                level1=l1, level2=l2, time_fraction=lfrac)
        itf.context.set_land_freshwater(freshwater)
    if model.sea_ice is not None and itf.sea_ice_ocean_heat_flux is not None:
        # compute_sea_ice_ocean_fluxes!: the three-equation exchange and frazil from the current ocean surface and the
        # ice–ocean stress; its outputs ARE the partition's interface_heat / salt_flux and the ice's frazil heat
        si, f = model.sea_ice, itf.sea_ice_ocean_fluxes
        itf.context.compute_sea_ice_ocean_fluxes(itf.ice_ocean_params, model.ocean.surface_state(), si.concentration,
                                                 si.x_stress, si.y_stress, f)
        si.interface_heat, si.salt_flux, si.frazil_heat = f["interface_heat"], f["salt_flux"], f["frazil_heat"]
    ice = model.sea_ice.fields() if model.sea_ice is not None else None
    # Inside run!(simulation) the clock is known one step ahead: the NEXT step's atmosphere state is requested into the other
    # set of exchange fields (ExchangeStates).  A sliding window needs a third slot for that: the request makes the next
    # bracketing snapshots resident while this step may still read the current ones.
    exchange = itf.exchange
    exchange.begin_step()
    if exchange.stepping_dt is not None and (atm.provider is None or atm.n_slots >= 3):
        exchange.request_next(atm, itf.weights, model.clock.time + exchange.stepping_dt)
    if itf.atmosphere_sea_ice_interface is not None:
        # the ocean path, then compute_atmosphere_sea_ice_fluxes! + compute_net_sea_ice_fluxes! in one ABI call; the
        # skin temperature found by the iteration becomes the sea ice's top surface temperature (and the next step's
        # first guess)
        si, ai = model.sea_ice, itf.atmosphere_sea_ice_interface._fields
        itf.context.update_state_sea_ice(src, itf.weights, model.ocean.surface_state(), itf.exchange_atmosphere_state,
                                         itf.atmosphere_ocean_interface._fields, itf.net_fluxes._ocean_fields, ice,
                                         si.surface_state(), ai, itf.net_fluxes._sea_ice_fields,
                                         frazil_heat=si.frazil_heat, interface_heat=si.interface_heat,
                                         level1=n1, level2=n2, time_fraction=frac)
        si.top_surface_temperature.copy_(ai["temperature"])
    else:
        itf.context.update_state(src, itf.weights, model.ocean.surface_state(), itf.exchange_atmosphere_state,
                                 itf.atmosphere_ocean_interface._fields, itf.net_fluxes._ocean_fields, ice=ice,
                                 level1=n1, level2=n2, time_fraction=frac)


def time_step(model, dt):
    """time_step!(coupled_model, Δt): component steps, tick, update_state!."""
    model.ocean.time_step(dt)
    model.clock.time += dt
    model.clock.iteration += 1
    update_state(model)


def time_steps(model, dt, nsteps, normalize=None, averages=None, climatology=None):
    """`nsteps` × time_step!(coupled_model, Δt), each followed by `normalize(model)` (a NormalizeSalinity) when one is given,
    inside libcoflux (cf_time_steps_coupled): no host work between the steps.  For a model whose ocean has no step_callback,
    whose atmosphere and land are whole records in memory, and which has sea ice with a surface state; anything else raises
    ValueError with the reason.  Both clocks advance by nsteps · Δt and every field of the model — the sea ice's
    top_surface_temperature and interfaces.land_freshwater included — is left as the host loop leaves it, bit for bit: the
    device loop's clock (fraction + step · increment) is held to time_step!'s own (t / Δt_snapshot) on the host first, and
    where the two would part in the last bit — Δt / Δt_snapshot is not a binary fraction — the run continues in a further
    call from a re-based clock.  One call when they agree throughout.  Steps are numbered by model.clock.iteration, which is
    what the context's attached averagers, integrator and monitor collect on.  `averages`: a SurfaceFluxAverages writer — ALL
    of its averagers are attached for the length of the call, one per slot from slot 0 (at most abi.ATTACHED_AVERAGES_MAX), and
    collect every step with weight Δt; the slots are emptied again on the way out.  Its window is the caller's: read
    `averages.means` and reset the averagers.  `climatology`: a MonthlyClimatology writer — attached for the length of the call
    (cf_attach_climatology): every step its schedule takes is binned by the calendar month of origin + (s + 1) · Δt, rounded to
    the second, and collected behind the averagers; detached again on the way out.  The stamp is a product where the model's
    clock is a repeated sum: after the rounding the two name the same second unless a step lies within their rounding error of
    an x.5-second tie.  Every sample has the writer's `sample_weight`, stride · (1 / stride) as the library forms it from the
    stride and a per-step weight — 1 but for rounding (exactly 1 for stride 1), and the same number that run!(simulation)
    collects with, so the two paths weigh alike."""
    itf, atm, ocean, si, land = model.interfaces, model.atmosphere, model.ocean, model.sea_ice, getattr(model, "land", None)
    if ocean.step_callback is not None:
        raise ValueError("time_steps: the ocean has a step_callback (host work between the steps); use time_step")
    if atm.provider is not None:
        raise ValueError("time_steps: the atmosphere is a sliding window (provider); only a whole record in memory is supported")
    if land is not None and land.provider is not None:
        raise ValueError("time_steps: the land is a sliding window (provider); only a whole record in memory is supported")
    if si is None or itf.atmosphere_sea_ice_interface is None:
        raise ValueError("time_steps: the model has no sea ice with a surface state (thickness, top_surface_temperature); "
                         "the ocean-only loop is FluxContext.time_steps")
    if itf.exchange.inside_run:
        raise ValueError("time_steps: called inside run!(simulation)")
    if normalize is not None and normalize.flux_field is not itf.net_fluxes.ocean.S:
        raise ValueError("time_steps: normalize is not the NormalizeSalinity of this model's salinity flux")
    ctx = itf.context
    attached = list(averages.averagers) if averages is not None else []
    if len(attached) > abi.ATTACHED_AVERAGES_MAX:
        raise ValueError(f"time_steps: the writer has {len(attached)} averagers, the step loop collects {abi.ATTACHED_AVERAGES_MAX}")
    if averages is not None and (averages._east or averages._north):
        raise ValueError("time_steps: the writer reads [i+1] / [j+1] of fields the library writes (halos filled between steps); use run")
    first = model.clock.iteration
    t0 = model.clock.time
    times = []
    t = t0
    for _ in range(nsteps):   # (the clock of time_step!: repeated addition)
        t += dt
        times.append(t)
    increment = dt / atm.time_interval
    clocks = [([atm.time_indices(t) for t in times], atm.n_levels, increment)]
    ai = itf.atmosphere_sea_ice_interface._fields
    exchange = itf.sea_ice_ocean_heat_flux is not None
    if exchange:
        f = itf.sea_ice_ocean_fluxes
        si.interface_heat, si.salt_flux, si.frazil_heat = f["interface_heat"], f["salt_flux"], f["frazil_heat"]
        ice_ocean = dict(f)
    else:
        ice_ocean = {k: v for k, v in (("interface_heat", si.interface_heat), ("salt_flux", si.salt_flux), ("frazil_heat", si.frazil_heat))
                     if v is not None}
    # what every stretch hands cf_make_coupled_step; only the clocks (and the dataset's origin) change from stretch to stretch
    step = dict(ice_ocean_params=itf.ice_ocean_params if exchange else None, ice_ocean_fluxes=ice_ocean)
    if land is not None:
        clocks.append(([land.levels(t) for t in times], land.n_levels, dt / land.time_interval))
        step.update(friver=land.data["friver"], licalvf=land.data.get("licalvf"), land_out=itf.require_land_freshwater(),
                    land_time_fraction_increment=clocks[1][2])
    restoring = normalize.additional_fluxes if normalize is not None else None
    follows_dataset = restoring is not None and isinstance(restoring.target, DatasetRestoring)
    if restoring is not None:
        step.update(piston_velocity=restoring.velocity, target=None if follows_dataset else restoring.target,
                    restoring_out=normalize.additional_buffer)
    if normalize is not None:
        step.update(normalize=True, area=normalize.area, mean_out=normalize.mean_total)
    # the carried skin temperature is the interface's own `temperature`: time_step! writes the result there and copies the whole
    # array to the sea ice — so the first guess goes in on the window the solve reads, and the array comes back whole
    W = (slice(ocean.grid.halo[1] - 1, ocean.grid.halo[1] + ocean.grid.size[1] + 1), slice(ocean.grid.halo[0] - 1, ocean.grid.halo[0] + ocean.grid.size[0] + 1))
    ai["temperature"][W].copy_(si.top_surface_temperature[W])
    state = {k: v for k, v in si.surface_state().items() if k != "top_temperature"}
    stresses = {k: v for k, v in (("x_stress", si.x_stress), ("y_stress", si.y_stress)) if v is not None}
    # a writer with budget outputs lends the loop its Qs, Ql, Mp (SurfaceFluxAverages: the fields its averagers are bound to)
    current = itf.exchange.current
    lent = dict(current, **averages._budget_atmos) if averages is not None and averages._budget_atmos else current
    for slot, averager in enumerate(attached):
        ctx.attach_average(averager, 1, dt, slot=slot)
    if climatology is not None:
        if not isinstance(climatology.schedule, IterationInterval):
            raise ValueError("time_steps: the climatology's schedule is not an IterationInterval")
        stride = climatology.schedule.interval
        ctx.attach_climatology(climatology.climatology, climatology.table(t0, t0 + (nsteps + 1) * dt), stride, 1.0 / stride,
                               t0 - first * dt, dt)
    try:
        # a restoring that follows a dataset: the host loop materialises it at the model clock after the step (times[k], a
        # repeated sum); the device loop's clock for it is origin + step · Δt, held to the same doubles stretch by stretch
        dataset = restoring.target.dataset(ctx, ocean.grid) if follows_dataset else None
        # one call of cf_time_steps_coupled per stretch of steps on which the device loop's clocks agree with the host's
        for a, b, based, origin in device_stretches(clocks, first, nsteps, times if follows_dataset else None, dt):
            if follows_dataset:
                ctx.attach_restoring_dataset(dataset, time_origin=origin, step_seconds=dt)
            sch = ctx.make_schedule([ocean.surface_state()], [lent], first_level=based[0][0], time_fraction=based[0][1],
                                    time_fraction_increment=increment, fold_north=itf.fold_north)
            if land is not None:
                step.update(land_first_level=based[1][0], land_time_fraction=based[1][1])
            block = ctx.make_coupled_step([state], ai["temperature"], ai, itf.net_fluxes._sea_ice_fields, **step)
            ctx.time_steps_coupled(first + a, b - a, sch, atm.data, itf.weights, itf.atmosphere_ocean_interface._fields,
                                   itf.net_fluxes._ocean_fields, stresses or None, block)
    finally:
        ctx.attach_restoring_dataset(None)
        for slot in range(len(attached)):
            ctx.attach_average(None, slot=slot)
        if climatology is not None:
            ctx.attach_climatology(None)
        if lent is not current:
            for name, t in averages._budget_atmos.items():
                current[name].copy_(t)
    si.top_surface_temperature.copy_(ai["temperature"])
    for _ in range(nsteps):
        ocean.time_step(dt)
        model.clock.time += dt
        model.clock.iteration += 1


@dataclass
class Simulation:
    model: OceanSeaIceModel
    dt: float = 20 * minutes          # README.md:76
    stop_time: float = float("inf")
    stop_iteration: int = 2 ** 62
    output_writers: dict = field(default_factory=dict)   # simulation.output_writers[:surface] = … (omip_diagnostics.jl:152-158)
    callbacks: dict = field(default_factory=dict)        # name → Callback: add_callback!(simulation, f, schedule)
    running: bool = True                                 # a callback stops run! by setting it False (NaNChecker does)


@dataclass
class Callback:
    func: object       # func(simulation)
    schedule: object   # asked through schedules.actuates: a TimeInterval with the time, any other with the iteration


def add_callback(simulation, callback, schedule=None, name=None):
    """add_callback!(simulation, callback, schedule = IterationInterval(1); name): run! calls callback(simulation) after the
    output writers of every iteration at which `schedule` actuates (omip_simulation.jl:392)."""
    schedule = as_schedule(schedule)
    name = name or f"callback{len(simulation.callbacks) + 1}"
    simulation.callbacks[name] = Callback(callback, schedule)
    return name


def run(simulation, pickup=False):
    """run!(simulation; pickup = false) — README.md:77, omip_simulation.jl:241-247.  After every time_step! each of
    `simulation.output_writers` is given the clock, then each of `simulation.callbacks` whose schedule actuates is called; the
    loop ends early when one of them clears `simulation.running`.  Checkpointers among the writers are given the clock last —
    after every other writer AND the callbacks of the iteration — so that their collections and a NormalizeSalinity are in the
    image.  `pickup`: True or "latest" restores the file with the highest iteration that the simulation's Checkpointer finds
    (none: a warning and a start from scratch — launch scripts pass pickup on the first launch too); an int that iteration's
    file, any other str that path (a missing file raises FileNotFoundError).  After a pickup the state at the model's clock
    lies in exchange set 0 and nothing is requested ahead."""
    m = simulation.model
    everyone = list(simulation.output_writers.values())
    writers = [w for w in everyone if not isinstance(w, Checkpointer)]
    checkpointers = [w for w in everyone if isinstance(w, Checkpointer)]
    callbacks = list(simulation.callbacks.values())
    for writer in writers + checkpointers:
        writer.initialize(simulation)
    if pickup is not False and pickup is not None:
        if not checkpointers:
            raise ValueError("run: pickup needs a Checkpointer among simulation.output_writers")
        checkpointers[0].pickup(pickup)
    for cb in callbacks:
        open_at(cb.schedule, m.clock.time, simulation.dt)
    # (stand-in interfaces that are only a context — run! is driven with such, under a replaced time_step — have no exchange
    #  states: an owner without field sets requests nothing, and its settle() is the discard call that every exit makes)
    exchange = getattr(m.interfaces, "exchange", None) or ExchangeStates(m.interfaces.context, None)
    exchange.stepping_dt = simulation.dt   # (update_state requests every next atmosphere state: see there)
    simulation.running = True
    try:
        while simulation.running and m.clock.time < simulation.stop_time and m.clock.iteration < simulation.stop_iteration:
            time_step(m, simulation.dt)
            for writer in writers:
                writer.write(m.clock)
            for cb in callbacks:
                if actuates(cb.schedule, m.clock):
                    cb.func(simulation)
            for writer in checkpointers:
                writer.write(m.clock)
    finally:
        failing = sys.exc_info()[0] is not None
        for writer in checkpointers:   # the last capture's file is on disk when run! returns
            try:
                writer.flush()
            except Exception:
                if not failing:        # (an error of the loop is the one to report, not what it did to the drain)
                    raise
        exchange.settle()
    m.interfaces.context.sync()


class NormalizeSalinity:
    """NormalizeSalinity (omip_simulation.jl:187-220): callable on the coupled model; subtracts the area-weighted global
    mean of (bulk salinity flux + materialised additional flux) from the bulk flux field.  Dispatches on the salinity top
    boundary condition as `salinity_normalizer` does: MultipleFluxes ⇒ the additional flux is materialised into a buffer
    first (`_materialize_top_flux!`), bare field ⇒ no additional flux."""

    def __init__(self, ocean, area=None):
        bc = ocean.model.top_boundary_conditions.S
        self.flux_field = bc.flux_field if isinstance(bc, MultipleFluxes) else bc
        self.additional_fluxes = bc.additional_fluxes if isinstance(bc, MultipleFluxes) else None
        self.additional_buffer = torch.zeros_like(self.flux_field) if self.additional_fluxes is not None else None
        self.area = area
        self.mean_total = torch.zeros(1, dtype=torch.float64, device=self.flux_field.device)

    def checkpoint_arrays(self):
        """The device state a Checkpointer registers for this callback, by name."""
        return dict(additional=self.additional_buffer, mean=self.mean_total)

    def __call__(self, model):
        if isinstance(model, Simulation):   # as a callback of run!: add_callback(simulation, normalize), as the reference installs it
            model = model.model
        ctx, ocean = model.interfaces.context, model.ocean
        if self.additional_fluxes is not None:
            r = self.additional_fluxes
            if isinstance(r.target, DatasetRestoring):   # S★ at the model clock, formed per cell from the dataset's two levels
                ctx.materialize_dataset_restoring(r.velocity, r.target.dataset(ctx, ocean.grid), model.clock.time, ocean.surface_state(),
                                                  self.additional_buffer)
            else:
                ctx.materialize_salinity_restoring(r.velocity, r.target, ocean.surface_state(), self.additional_buffer)
        ctx.normalize_salinity_flux(self.flux_field, ocean.model.wet_mask, additional=self.additional_buffer, area=self.area,
                                    mean_out=self.mean_total)
