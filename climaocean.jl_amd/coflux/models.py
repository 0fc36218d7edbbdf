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
"""
import datetime as _dt
import logging
import math
import time
from dataclasses import dataclass, field
from types import SimpleNamespace
from typing import Optional

import numpy as np
import torch

from . import abi, synthetic
from . import interface_computations as ic
from .runtime import BUDGET_KINDS, EXCHANGE_NAMES, FLUX_NAMES, FLUX_OPTIONAL, NET_NAMES, FluxContext, calendar_bin

minutes, hours, days = 60.0, 3600.0, 86400.0
EARTH_RADIUS = 6.371e6   # m (Oceananigans' R_Earth)


# ---------------------------------------------------------------------------------------------
# grid
# ---------------------------------------------------------------------------------------------
@dataclass
class LatitudeLongitudeGrid:
    """README.md:56-61 (only the metadata the surface path needs)."""
    size: tuple = (1440, 560, 10)
    halo: tuple = (7, 7, 7)
    longitude: tuple = (0.0, 360.0)
    latitude: tuple = (-70.0, 70.0)
    z: tuple = (-3000.0, 0.0)
    device: int = 0

    @property
    def surface_shape(self):
        (nx, ny, _), (hx, hy, _) = self.size, self.halo
        return (ny + 2 * hy, nx + 2 * hx)

    @property
    def surface_z(self):
        nz = self.size[2]
        dz = (self.z[1] - self.z[0]) / nz
        return self.z[1] - 0.5 * dz  # centre of the top cell (uniform spacing)

    def fractional_indices(self, nsx=synthetic.JRA55_NX, nsy=synthetic.JRA55_NY):
        nx, ny, _ = self.size
        hx, hy, _ = self.halo
        return synthetic.latlon_fractional_indices(nx, ny, hx, hy, latitude=self.latitude, nsx=nsx, nsy=nsy)

    fold_north = False

    def interpolation_weights(self, to_device, nsx=synthetic.JRA55_NX, nsy=synthetic.JRA55_NY):
        """cf_interp_weights for this grid: separable fractional indices into the JRA55 grid (no rotation)."""
        fi, fj, phi = self.fractional_indices(nsx, nsy)
        return dict(separable=True, fi=to_device(fi), fj=to_device(fj), latitude=to_device(phi))

    def cell_latitudes(self):
        """φ [deg] of the cell centres in the halo layout (ny + 2hy, nx + 2hx)."""
        (nx, ny, _), (hx, hy, _) = self.size, self.halo
        phi = self.latitude[0] + (np.arange(-hy, ny + hy) + 0.5) * (self.latitude[1] - self.latitude[0]) / ny
        return np.ascontiguousarray(np.broadcast_to(phi[:, None], self.surface_shape))

    def cell_areas(self):
        """Az = R² Δλ (sin φ_f[j+1] − sin φ_f[j]) [m²] in the halo layout (the formula runs on through the halo rows)."""
        (nx, ny, _), (hx, hy, _) = self.size, self.halo
        dlam = np.deg2rad((self.longitude[1] - self.longitude[0]) / nx)
        faces = np.deg2rad(self.latitude[0] + np.arange(-hy, ny + hy + 1) * (self.latitude[1] - self.latitude[0]) / ny)
        rows = EARTH_RADIUS ** 2 * dlam * np.diff(np.sin(faces))
        return np.ascontiguousarray(np.broadcast_to(rows[:, None], self.surface_shape))


@dataclass
class TripolarGrid:
    """TripolarGrid(arch; size = (360, 180, Nz), halo = (5, 5, 4), z, …) — OceanConfigurations/one_degree_tripolar.jl:32,48-51
    (1°), half_degree_tripolar.jl:48-51 (720×360), sixth_degree_tripolar.jl:33-36 (2160×1080, halo 7), tenth_degree… (3600×1800).
    Only what the surface path needs: cell-centre positions → general (2-D) fractional indices into the JRA55 grid, the
    rotation of the grid's i-axis against geographic east (visualize/cache.jl:406-427: the winds are rotated into the
    grid frame) and the north fold (the last row of tracer points is its own mirror image; Oceananigans' zipper
    boundary).  The mesh itself comes from `synthetic.tripolar_mesh` (a bipolar cap with the real fold topology) unless
    `longitude` / `latitude` / rotation arrays of the real grid are handed in."""
    size: tuple = (360, 180, 10)
    halo: tuple = (5, 5, 4)
    z: tuple = (-3000.0, 0.0)
    southernmost_latitude: float = -80.0
    first_pole_longitude: float = 75.0
    north_poles_latitude: float = 55.0
    device: int = 0
    longitude: Optional[np.ndarray] = None     # (ny, nx) cell-centre λ [deg] of a real grid (else synthetic)
    latitude: Optional[np.ndarray] = None      # (ny, nx) cell-centre φ [deg]
    cos_rotation: Optional[np.ndarray] = None
    sin_rotation: Optional[np.ndarray] = None
    area: Optional[np.ndarray] = None          # (ny, nx) cell areas Az [m²] of a real grid (nothing is guessed without them)

    fold_north = True

    def _halo_layout(self, a, fill):
        (nx, ny, _), (hx, hy, _) = self.size, self.halo
        g = np.full(self.surface_shape, fill, dtype=np.asarray(a).dtype)
        g[hy:hy + ny, hx:hx + nx] = a
        return g

    def cell_latitudes(self):
        """φ [deg] of the cell centres in the halo layout; the halos hold NaN (no cell there belongs to a hemisphere)."""
        return self._halo_layout(np.asarray(self.mesh()[1], dtype=np.float64), np.nan)

    def cell_areas(self):
        """The `area` array of the real grid in the halo layout (halos 0)."""
        if self.area is None:
            raise ValueError("TripolarGrid: cell areas are not derived from the synthetic mesh; pass TripolarGrid(area=Az) "
                             "(ny × nx, m²) or hand an area array to the integrals")
        return self._halo_layout(np.asarray(self.area, dtype=np.float64), 0.0)

    @property
    def surface_shape(self):
        (nx, ny, _), (hx, hy, _) = self.size, self.halo
        return (ny + 2 * hy, nx + 2 * hx)

    @property
    def surface_z(self):
        nz = self.size[2]
        dz = (self.z[1] - self.z[0]) / nz
        return self.z[1] - 0.5 * dz

    def mesh(self):
        nx, ny, _ = self.size
        if self.longitude is not None:
            if self.latitude is None or self.cos_rotation is None or self.sin_rotation is None:
                raise ValueError("TripolarGrid: longitude, latitude, cos_rotation and sin_rotation come together")
            return self.longitude, self.latitude, self.cos_rotation, self.sin_rotation
        return synthetic.tripolar_mesh(nx, ny, southernmost_latitude=self.southernmost_latitude,
                                       cap_latitude=self.north_poles_latitude, pole_longitude=self.first_pole_longitude)

    def interpolation_weights(self, to_device, nsx=synthetic.JRA55_NX, nsy=synthetic.JRA55_NY, rows=2):
        """General weights + rotation, halo-inclusive: periodic in x, the north halo rows are the fold images of the
        interior rows (their i-axis points the other way: rotation reversed), as synthetic.tripolar_case builds them."""
        (nx, ny, _), (hx, hy, _) = self.size, self.halo
        lam, phi, cos_t, sin_t = self.mesh()

        def halo2d(a):
            g = np.empty((ny + 2 * hy, nx + 2 * hx))
            g[hy:hy + ny, hx:hx + nx] = a
            g[:hy] = g[hy:hy + 1]
            g[hy + ny:] = g[hy + ny - 1:hy + ny]
            g[:, :hx], g[:, hx + nx:] = g[:, nx:nx + hx], g[:, hx:2 * hx]
            return g
        LAM, PHI, COS, SIN = (halo2d(a) for a in (lam, phi, cos_t, sin_t))
        r = min(rows, hy)
        for a in (LAM, PHI, COS, SIN):
            synthetic.fold_north(a, nx, ny, hx, hy, r, "center", 1)
        COS[hy + ny:hy + ny + r] *= -1.0
        SIN[hy + ny:hy + ny + r] *= -1.0
        fi = LAM / (360.0 / nsx)
        fj = (PHI - synthetic.JRA55_LAT0) / (2 * 89.57 / (nsy - 1))
        c = np.ascontiguousarray
        return dict(separable=False, fi=to_device(c(fi)), fj=to_device(c(fj)), cos_rot=to_device(c(COS)), sin_rot=to_device(c(SIN)),
                    latitude=to_device(c(PHI)))


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


# ---------------------------------------------------------------------------------------------
# atmosphere / radiation
# ---------------------------------------------------------------------------------------------
class JRA55PrescribedAtmosphere:
    """JRA55PrescribedAtmosphere(arch; dir, dataset, start_date, end_date, time_indices_in_memory,
    prefetch) — atmosphere.jl:20-29, README.md:74.  Holds `time_indices_in_memory` 3-hourly
    snapshots of the 9 variables (jra55_data_staging.jl:8) as Float32 640×320 fields in HBM.

    Two backends, as in the reference: everything in memory (`snapshots` = dict var -> [n, 320, 640]), or a
    sliding window (`provider(n) -> dict var -> [320, 640]` reads snapshot n from wherever the files are;
    `total_snapshots` per repeat-year/multi-year record).  With `prefetch` the snapshots the clock will reach next
    are read by a background thread straight into the window's pinned staging buffers and committed to HBM by the
    stepping thread, so file reads and PCIe copies overlap the flux kernels (launch.sh:86-93)."""

    def __init__(self, snapshots=None, *, provider=None, total_snapshots=None, time_indices_in_memory=2,
                 prefetch=True, time_interval=3 * hours, device=0, reference_height=10.0, boundary_layer_height=600.0,
                 cyclic=True, source_size=(synthetic.JRA55_NX, synthetic.JRA55_NY)):
        self.time_interval = time_interval
        self.reference_height = reference_height
        self.boundary_layer_height = boundary_layer_height
        self.cyclic = cyclic  # RepeatYearJRA55-style cyclic time indexing vs clamped (MultiYearJRA55 record ends)
        self.provider, self.prefetch = provider, prefetch
        self.window = None
        self._pending = {}   # time index -> Future of a background read into the pinned buffers
        self._reader = None
        if provider is not None:
            if total_snapshots is None:
                raise ValueError("a snapshot provider needs total_snapshots (2920 for a repeat year of 3-hourly JRA55)")
            if time_indices_in_memory < 2:
                raise ValueError("time_indices_in_memory must be >= 2")
            self.n_levels = total_snapshots
            self.n_slots = time_indices_in_memory
            self.source_size = source_size
            self.data = None
            return
        dev = torch.device("cuda", device)
        if snapshots is None:
            snapshots = synthetic.jra55_snapshots(time_indices_in_memory)
        self.data = {k: torch.as_tensor(np.ascontiguousarray(v, dtype=np.float32)).to(dev) for k, v in snapshots.items()}
        self.n_levels = next(iter(self.data.values())).shape[0]

    def time_indices(self, t):
        """(n₁, n₂, ñ): the bracketing snapshots and the fractional position between them."""
        x = t / self.time_interval
        n = int(np.floor(x))
        frac = x - n
        if self.cyclic:
            return n % self.n_levels, (n + 1) % self.n_levels, frac
        n1 = min(max(n, 0), self.n_levels - 1)
        n2 = min(max(n + 1, 0), self.n_levels - 1)
        return n1, n2, (frac if 0 <= n < self.n_levels - 1 else 0.0)

    # ---- sliding-window backend ---------------------------------------------------------------
    def _wrap(self, n):
        return n % self.n_levels if self.cyclic else min(max(n, 0), self.n_levels - 1)

    def _read_into_staging(self, k):
        """Snapshot COUNTER k (monotone in time, not wrapped) → the provider's record index wrap(k), staged in slot
        k mod n_slots.  Slots follow the counter, not the record index: at the end of a repeat year the indices
        jump from total−1 to 0, and two consecutive snapshots must never share a slot."""
        slot = k % self.n_slots
        self.window.wait_slot(slot)          # the previous copy out of these pinned buffers has finished
        snap = self.provider(self._wrap(k))
        for v in abi.JRA55_VARIABLES:
            np.copyto(self.window.host_view(slot, v), snap[v], casting="same_kind")
        return slot

    def source(self, context, t):
        """The cf_atmos_source for time t.  In-memory backend: (data, n₁, n₂, ñ).  Window backend: makes n₁, n₂
        resident (blocking only if the prefetch has not delivered them), commits finished prefetches and queues
        the reads for the snapshots ahead."""
        n1, n2, frac = self.time_indices(t)
        if self.provider is None:
            return self.data, n1, n2, frac
        if self.window is None:
            from . import runtime
            self.window = runtime.SnapshotWindow(context, self.source_size[0], self.source_size[1], self.n_slots)
            if self.prefetch and self.n_slots > 2:
                from concurrent.futures import ThreadPoolExecutor
                self._reader = ThreadPoolExecutor(max_workers=1, thread_name_prefix="jra55-prefetch")
        w = self.window
        base = int(np.floor(t / self.time_interval))
        if self.cyclic:
            k1, k2 = base, base + 1
        else:   # clamped record: the counters stop at its ends
            k1 = min(max(base, 0), self.n_levels - 1)
            k2 = min(max(base + 1, 0), self.n_levels - 1)
        for k in (k1, k2):
            if w.find(k) >= 0:
                continue
            fut = self._pending.pop(k, None)
            slot = fut.result() if fut is not None else self._read_into_staging(k)
            w.commit(slot, k)
        for k, fut in list(self._pending.items()):      # prefetches that have landed in pinned memory
            if fut.done():
                w.commit(fut.result(), k)
                del self._pending[k]
        if self._reader is not None:
            for ahead in range(2, self.n_slots):        # the slots that hold neither k₁ nor k₂
                k = base + ahead
                if not self.cyclic and not (0 <= k < self.n_levels):
                    continue
                if k in (k1, k2) or w.find(k) >= 0 or k in self._pending:
                    continue
                if any((m % self.n_slots) == (k % self.n_slots) for m in list(self._pending) + [k1, k2]):
                    continue
                self._pending[k] = self._reader.submit(self._read_into_staging, k)
        return w.source(k1, k2, frac), n1, n2, frac

    def close(self):
        if self._reader is not None:
            self._reader.shutdown(wait=True)
            self._reader = None
        self._pending.clear()
        if self.window is not None:
            self.window.close()
            self.window = None


@dataclass
class Radiation:
    """JRA55PrescribedRadiation(arch; ocean_surface = SurfaceRadiationProperties(0.06, 1.00), …),
    atmosphere.jl:41-44 (the downwelling fields themselves ride in the atmosphere window)."""
    ocean_surface: ic.SurfaceRadiationProperties = field(default_factory=ic.SurfaceRadiationProperties)
    stefan_boltzmann_constant: float = 5.67e-8
    sea_ice_surface: Optional[ic.SurfaceRadiationProperties] = None   # SurfaceRadiationProperties(SeaIceAlbedo(hi, hs, Ts), 1.0)


JRA55PrescribedRadiation = Radiation


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
class ComponentInterfaces:  # noqa: D101 — documented below
    @property
    def exchange_atmosphere_state(self):
        return self._exchange_sets[self._exchange_current]

    @property
    def _exchange_other(self):
        return self._exchange_sets[1 - self._exchange_current]

    """ComponentInterfaces(atmosphere, ocean, sea_ice; radiation, atmosphere_ocean_fluxes,
    atmosphere_ocean_velocity_difference, ocean_minimum_salinity) — omip_simulation.jl:128-158."""

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
        # interfaces.exchange_atmosphere_state — the reference updates ONE field set in place.  Here it is a property over two
        # private sets: outside run!(simulation) it is always set 0 (stable tensors: what a writer or a diagnostic may hold
        # on to); inside run! every step's solver launch also interpolates the NEXT step's state, into the other set, so the
        # current state alternates between the two — read it through the property there, do not keep the dict or its tensors
        # across steps.  run! leaves the final state in set 0 and restores the context's options.
        self._exchange_sets = [ctx.field_set(EXCHANGE_NAMES), None]
        self._exchange_current = 0
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


def omip_forcing(arch, sea_ice, *, forcing_dir, start_date, end_date, repeat_year_forcing=False, backend_size=30, device=0):
    """omip_forcing(arch, sea_ice; forcing_dir, start_date, end_date, repeat_year_forcing = false, backend_size = 30)
    — /root/reference/src/OMIPConfigurations/atmosphere.jl:13-49: the prescribed forcing components of an OMIP-2
    simulation.  Returns `(atmosphere, radiation, land)`: the JRA55-do atmosphere on a sliding window of `backend_size`
    snapshots with prefetch, the downwelling radiation with the OMIP-2 ocean surface (albedo 0.06, emissivity 1) and
    the CCSM3 `SeaIceAlbedo(hi, hs, Ts)` over ice, and the land freshwater (river runoff + iceberg calving).
    `arch` is accepted for signature parity (the device is `device`).  Files: raw Float32 planes, see coflux/jra55.py."""
    from . import jra55
    dataset = jra55.RepeatYearJRA55(year=start_date.year) if repeat_year_forcing else jra55.MultiYearJRA55()
    calendar = jra55.SnapshotCalendar(dataset, start_date, end_date)
    files = jra55.RawPlaneFiles(forcing_dir)
    atmosphere = JRA55PrescribedAtmosphere(provider=jra55.atmosphere_provider(forcing_dir, calendar, files), total_snapshots=calendar.total,
                                           time_indices_in_memory=backend_size, prefetch=True, cyclic=dataset.cyclic, device=device)
    atmosphere.dataset, atmosphere.calendar = dataset, calendar
    sea_ice_albedo = ic.SeaIceAlbedo() if sea_ice is not None else None   # SeaIceAlbedo(hi, hs, Ts): reads the live ice fields
    radiation = Radiation(ocean_surface=ic.SurfaceRadiationProperties(0.06, 1.00),
                          sea_ice_surface=ic.SurfaceRadiationProperties(sea_ice_albedo, 1.0) if sea_ice is not None else None)
    # JRA55PrescribedLand(arch; …) streams the whole record like the atmosphere: same calendar, same window length
    land = JRA55PrescribedLand(provider=jra55.land_provider(forcing_dir, calendar, files), total_snapshots=calendar.total,
                               time_indices_in_memory=max(2, backend_size), cyclic=dataset.cyclic, device=device)
    land.dataset, land.calendar = dataset, calendar
    return atmosphere, radiation, land


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
        land = model.land
        if not hasattr(itf, "land_freshwater"):
            itf.land_freshwater = itf.context.zeros()
        l1, l2, lfrac = land.levels(model.clock.time)   # (the record's calendar: cyclic repeat year / clamped multi-year)
        itf.context.interpolate_land_freshwater(land.data["friver"], land.data.get("licalvf"), itf.weights, itf.land_freshwater,
                                                level1=l1, level2=l2, time_fraction=lfrac)
        itf.context.set_land_freshwater(itf.land_freshwater)
    if model.sea_ice is not None and itf.sea_ice_ocean_heat_flux is not None:
        # compute_sea_ice_ocean_fluxes!: the three-equation exchange and frazil from the current ocean surface and the
        # ice–ocean stress; its outputs ARE the partition's interface_heat / salt_flux and the ice's frazil heat
        si, f = model.sea_ice, itf.sea_ice_ocean_fluxes
        itf.context.compute_sea_ice_ocean_fluxes(itf.ice_ocean_params, model.ocean.surface_state(), si.concentration,
                                                 si.x_stress, si.y_stress, f)
        si.interface_heat, si.salt_flux, si.frazil_heat = f["interface_heat"], f["salt_flux"], f["frazil_heat"]
    ice = model.sea_ice.fields() if model.sea_ice is not None else None
    # Inside run!(simulation) the clock is known one step ahead: the NEXT step's atmosphere state is requested into the other
    # set of exchange fields and rides in this step's solver launch (CF_OPT_MERGED_PREFETCH = 2: tail workgroups; the same
    # bits as interpolating it when its step comes).  A sliding window needs a third slot for that: the request makes the
    # next bracketing snapshots resident while this step may still read the current ones.
    if getattr(itf, "_next_state_in_other", False):   # requested by the previous step: this step's state is in the other set
        itf._exchange_current = 1 - itf._exchange_current
        itf._next_state_in_other = False
    dt_next = getattr(model, "_pipeline_dt", None)
    pipelined = dt_next is not None and (atm.provider is None or atm.n_slots >= 3)
    if pipelined:
        if itf._exchange_other is None:
            itf._exchange_sets[1 - itf._exchange_current] = itf.context.field_set(EXCHANGE_NAMES)
        if not getattr(itf, "_tail_mode", False):   # (restored by run!: a lone update_state! is ≈ 5 µs slower on the tail plan)
            itf.context.set_option(abi.OPT_MERGED_PREFETCH, 2)
            itf._tail_mode = True
        src_n, n1n, n2n, frac_n = atm.source(itf.context, model.clock.time + dt_next)
        itf.context.prefetch_atmosphere_state(src_n, itf.weights, itf._exchange_other, level1=n1n, level2=n2n, time_fraction=frac_n)
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
    itf._next_state_in_other = pipelined   # (the next update_state! swaps the sets first: until then
                                           #  `exchange_atmosphere_state` is the state at the model's clock)


def time_step(model, dt):
    """time_step!(coupled_model, Δt): component steps, tick, update_state!."""
    model.ocean.time_step(dt)
    model.clock.time += dt
    model.clock.iteration += 1
    update_state(model)


def _device_clock(level1, fraction, n_levels, step, increment):
    """(first_level, time_fraction) with which the device loop's clock — total = time_fraction + step · increment, level1 =
    (first_level + ⌊total⌋) mod n_levels, ñ = total − ⌊total⌋ (cf_time_steps) — gives exactly (level1, fraction) at `step`,
    or None.  The sum is simulated in the same double arithmetic, so a returned pair is verified, not estimated."""
    base = float(step) * increment
    shift = max(0, math.ceil(base - fraction))
    guess = fraction + shift - base
    for tf in (guess, np.nextafter(guess, np.inf), np.nextafter(guess, -np.inf)):
        tf = float(tf)
        total = tf + base
        whole = math.floor(total)
        if tf >= 0.0 and total - whole == fraction:
            return (level1 - int(whole)) % n_levels, tf
    return None


def _clock_at(first_level, time_fraction, n_levels, step, increment):
    total = time_fraction + float(step) * increment
    whole = math.floor(total)
    level1 = (first_level + int(whole)) % n_levels
    return level1, (level1 + 1) % n_levels, total - whole


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
    if getattr(model, "_pipeline_dt", None) is not None or getattr(itf, "_next_state_in_other", False):
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
    clocks = [(atm, [atm.time_indices(t) for t in times], dt / atm.time_interval)]
    if land is not None:
        clocks.append((land, [land.levels(t) for t in times], dt / land.time_interval))
    ai = itf.atmosphere_sea_ice_interface._fields
    exchange = itf.sea_ice_ocean_heat_flux is not None
    if exchange:
        f = itf.sea_ice_ocean_fluxes
        si.interface_heat, si.salt_flux, si.frazil_heat = f["interface_heat"], f["salt_flux"], f["frazil_heat"]
        ice_ocean = dict(f)
    else:
        ice_ocean = {k: v for k, v in (("interface_heat", si.interface_heat), ("salt_flux", si.salt_flux), ("frazil_heat", si.frazil_heat))
                     if v is not None}
    if land is not None and not hasattr(itf, "land_freshwater"):
        itf.land_freshwater = ctx.zeros()
    restoring = normalize.additional_fluxes if normalize is not None else None
    # the carried skin temperature is the interface's own `temperature`: time_step! writes the result there and copies the whole
    # array to the sea ice — so the first guess goes in on the window the solve reads, and the array comes back whole
    W = (slice(ocean.grid.halo[1] - 1, ocean.grid.halo[1] + ocean.grid.size[1] + 1), slice(ocean.grid.halo[0] - 1, ocean.grid.halo[0] + ocean.grid.size[0] + 1))
    ai["temperature"][W].copy_(si.top_surface_temperature[W])
    state = {k: v for k, v in si.surface_state().items() if k != "top_temperature"}
    stresses = {k: v for k, v in (("x_stress", si.x_stress), ("y_stress", si.y_stress)) if v is not None}
    # a writer with budget outputs lends the loop its Qs, Ql, Mp (SurfaceFluxAverages: the fields its averagers are bound to)
    current = itf._exchange_sets[itf._exchange_current]
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
        _device_steps(model, dt, nsteps, normalize, clocks, first, lent, ai, state, stresses, exchange, ice_ocean, restoring, times)
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


def _dataset_origin(time, step, dt):
    """time_origin with which the dataset clock of the device loop, origin + step · Δt, gives exactly `time` at `step`, or None"""
    base = float(step) * dt
    guess = time - base
    for origin in (guess, float(np.nextafter(guess, np.inf)), float(np.nextafter(guess, -np.inf))):
        if origin + base == time:
            return origin
    return None


def _device_steps(model, dt, nsteps, normalize, clocks, first, exchange_set, ai, state, stresses, exchange, ice_ocean, restoring, times=None):
    """time_steps' calls of cf_time_steps_coupled: one per stretch of steps on which the device loop's clocks agree with the host's"""
    itf, atm, ocean, land = model.interfaces, model.atmosphere, model.ocean, getattr(model, "land", None)
    ctx = itf.context
    # a restoring that follows a dataset: the host loop materialises it at the model clock after the step (times[k], a repeated
    # sum); the device loop's clock for it is origin + step · Δt, held to the same doubles stretch by stretch
    dataset = restoring.target.dataset(ctx, ocean.grid) if restoring is not None and isinstance(restoring.target, DatasetRestoring) else None
    a = 0
    while a < nsteps:
        g = first + a
        based = []
        for comp, want, inc in clocks:
            n1, n2, frac = want[a]
            c = _device_clock(n1, frac, comp.n_levels, g, inc)
            if c is None or _clock_at(c[0], c[1], comp.n_levels, g, inc) != (n1, n2, frac):
                raise ValueError(f"time_steps: the device loop's clock cannot take the snapshots ({n1}, {n2}) at fraction {frac!r} "
                                 f"of step {g} (a clamped record at its end?); use time_step")
            based.append(c)
        b = a + 1
        while b < nsteps and all(_clock_at(c[0], c[1], comp.n_levels, first + b, inc) == tuple(want[b])
                                 for (comp, want, inc), c in zip(clocks, based)):
            b += 1
        if dataset is not None:
            origin = _dataset_origin(times[a], g, dt)
            if origin is None:
                raise ValueError(f"time_steps: the dataset clock origin + step · Δt cannot give the model time {times[a]!r} at step {g}; use time_step")
            b = next((k for k in range(a + 1, b) if origin + float(first + k) * dt != times[k]), b)
            ctx.attach_restoring_dataset(dataset, time_origin=origin, step_seconds=dt)
        sch = ctx.make_schedule([ocean.surface_state()], [exchange_set], first_level=based[0][0],
                                time_fraction=based[0][1], time_fraction_increment=clocks[0][2], fold_north=itf.fold_north)
        kw = {}
        if land is not None:
            kw.update(friver=land.data["friver"], licalvf=land.data.get("licalvf"), land_out=itf.land_freshwater,
                      land_first_level=based[1][0], land_time_fraction=based[1][1], land_time_fraction_increment=clocks[1][2])
        if restoring is not None:
            kw.update(piston_velocity=restoring.velocity, target=None if dataset is not None else restoring.target,
                      restoring_out=normalize.additional_buffer)
        if normalize is not None:
            kw.update(normalize=True, area=normalize.area, mean_out=normalize.mean_total)
        block = ctx.make_coupled_step([state], ai["temperature"], ai, itf.net_fluxes._sea_ice_fields,
                                      ice_ocean_params=itf.ice_ocean_params if exchange else None, ice_ocean_fluxes=ice_ocean, **kw)
        ctx.time_steps_coupled(g, b - a, sch, atm.data, itf.weights, itf.atmosphere_ocean_interface._fields, itf.net_fluxes._ocean_fields,
                               stresses or None, block)
        a = b


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
    schedule: object   # .actuate(iteration)


def add_callback(simulation, callback, schedule=None, name=None):
    """add_callback!(simulation, callback, schedule = IterationInterval(1); name): run! calls callback(simulation) after the
    output writers of every iteration at which `schedule` actuates (omip_simulation.jl:392)."""
    schedule = IterationInterval(schedule) if isinstance(schedule, int) else (schedule or IterationInterval(1))
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
    m._pipeline_dt = simulation.dt   # (update_state requests every next atmosphere state: see there)
    simulation.running = True
    try:
        while simulation.running and m.clock.time < simulation.stop_time and m.clock.iteration < simulation.stop_iteration:
            time_step(m, simulation.dt)
            for writer in writers:
                writer.write(m.clock)
            for cb in callbacks:
                if cb.schedule.actuate(m.clock.iteration):
                    cb.func(simulation)
            for writer in checkpointers:
                writer.write(m.clock)
    finally:
        import sys
        failing = sys.exc_info()[0] is not None
        for writer in checkpointers:   # the last capture's file is on disk when run! returns
            try:
                writer.flush()
            except Exception:
                if not failing:        # (an error of the loop is the one to report, not what it did to the drain)
                    raise
        m._pipeline_dt = None
        itf = m.interfaces
        # the state at the model's clock goes back to set 0 (what callers may hold), the pending request is dropped, and the
        # context returns to the options it had: the chunk plan of a lone update_state!, the auxiliary-stream prefetch
        if getattr(itf, "_next_state_in_other", False):
            itf._next_state_in_other = False     # (the requested state of a step that will not run; the next run! asks again)
        itf.context.discard_prefetched_atmosphere_state()
        if itf._exchange_current != 0:
            for k, t in itf._exchange_sets[0].items():
                t.copy_(itf._exchange_sets[1][k])
            itf._exchange_current = 0
        if getattr(itf, "_tail_mode", False):
            itf.context.set_option(abi.OPT_MERGED_PREFETCH, 0)
            itf._tail_mode = False
    m.interfaces.context.sync()


# ---------------------------------------------------------------------------------------------
# time-averaged output (Oceananigans' AveragedTimeInterval / WindowedTimeAverage, accumulated on the device)
# ---------------------------------------------------------------------------------------------
class AveragedTimeInterval:
    """AveragedTimeInterval(interval; window = interval, stride = 1) — the schedule of the reference's averaged writers
    (omip_diagnostics.jl:152-158, examples/latitude_longitude_ocean_sea_ice.jl:60-66).  Window k is (t_k − window, t_k] with
    t_k = k · interval.  Inside a window a step's sample is taken when iteration % stride == 0, and always at t_k; its
    weight is the time since the previous sample or since the window opened, t_n − max(t_prev, t_k − window).  The time
    step must divide `interval`.  Host bookkeeping only: sample() says what to collect, the writer collects it."""

    def __init__(self, interval, window=None, stride=1):
        window = interval if window is None else window
        if not (interval > 0) or not (0 < window <= interval):
            raise ValueError(f"AveragedTimeInterval: interval = {interval}, window = {window} (0 < window ≤ interval)")
        if int(stride) != stride or stride < 1:
            raise ValueError(f"AveragedTimeInterval: stride = {stride} (an integer ≥ 1)")
        self.interval, self.window, self.stride = float(interval), float(window), int(stride)
        self.k = None             # the open window ends at k · interval
        self.previous = None      # time of the last sample

    def initialize(self, time, dt):
        """Checks the time step; the first call also opens the first window that ends after `time` (an open window survives
        the end of run!, as in Oceananigans)."""
        ratio = self.interval / dt if dt > 0 else 0.0
        if round(ratio) < 1 or abs(ratio - round(ratio)) > 1e-9 * ratio:
            raise ValueError(f"AveragedTimeInterval: the time step {dt} does not divide the interval {self.interval}")
        self._tol = 1e-6 * dt
        if self.k is None:
            self.k = int(np.floor((time + self._tol) / self.interval)) + 1
            self.previous = float(time)

    def sample(self, time, iteration):
        """(weight, t_k) for the step that has just reached `time`: weight is None when nothing is collected, t_k is the end
        of the window that this sample completes (None while it stays open)."""
        t_k = self.k * self.interval
        end = time >= t_k - self._tol
        if end:
            time = t_k
        start = t_k - self.window
        if time <= start + self._tol or (not end and iteration % self.stride != 0):
            return None, None
        weight = time - max(self.previous, start)
        self.previous = time
        if not end:
            return weight, None
        self.k += 1
        return weight, t_k


# the OMIP surface diagnostics (omip_diagnostics.jl:125-130): CMIP name → interface field
SURFACE_FLUX_OUTPUTS = (("tauuo", "net", "u"), ("tauvo", "net", "v"), ("hfds", "net", "T"), ("wfo", "net", "S"),
                        ("hfss", "atmosphere_ocean", "sensible_heat"), ("hfls", "atmosphere_ocean", "latent_heat"))


# derived outputs (cf_average_create_derived): small expression objects over ocean-grid device fields.  Each lowers to one
# term of the collection launch — the derived array is never written to memory — and `Scaled` multiplies the term's scale.
class SurfaceExpression:
    kind, flags, rotates = None, 0, False
    fold_sign = -1.0   # of a y-face operand under the tripolar fold: a vector component changes sign (cf_fold_north_halo)

    def __init__(self, a, b=None):
        self.a, self.b = a, b

    def term(self):
        """(kind, flags, a, b, scale) as cf_average_term has them."""
        return self.kind, self.flags, self.a, self.b, 1.0

    def neighbours(self):
        """(fields read at [i+1], fields read at [j+1])"""
        kind, flags, a, b, _ = self.term()
        faces = kind in (abi.TERM_EAST, abi.TERM_NORTH) and not flags & abi.TERM_AT_CENTERS
        east = [a] if kind in (abi.TERM_CENTER_X, abi.TERM_CENTER_X_SQUARE, abi.TERM_KINETIC_ENERGY) or faces else []
        north = [a] if kind in (abi.TERM_CENTER_Y, abi.TERM_CENTER_Y_SQUARE) else [b] if kind == abi.TERM_KINETIC_ENERGY or faces else []
        return east, north


class Product(SurfaceExpression):
    """Product(a, b): a·b at the cell."""
    kind = abi.TERM_PRODUCT

    def __init__(self, a, b):
        super().__init__(a, b)


class Squared(Product):
    """Squared(f): f·f — tossq = Squared(tos) (omip_diagnostics.jl:111-113)."""

    def __init__(self, f):
        super().__init__(f, f)


class CenteredX(SurfaceExpression):
    """CenteredX(u): ℑx u = (u[i] + u[i+1])/2, an x-face field at the cell centre."""
    kind = abi.TERM_CENTER_X

    def __init__(self, u):
        super().__init__(u)


class CenteredY(SurfaceExpression):
    """CenteredY(v, fold_sign=-1): ℑy v = (v[j] + v[j+1])/2; fold_sign = +1 for a y-face field that is no vector component."""
    kind = abi.TERM_CENTER_Y

    def __init__(self, v, fold_sign=-1.0):
        super().__init__(v)
        self.fold_sign = float(fold_sign)


class CenteredXSquare(CenteredX):
    """CenteredXSquare(u): ℑx(u²), uu_at_ccc (omip_diagnostics.jl:13-25)."""
    kind = abi.TERM_CENTER_X_SQUARE


class CenteredYSquare(CenteredY):
    """CenteredYSquare(v): ℑy(v²), vv_at_ccc."""
    kind = abi.TERM_CENTER_Y_SQUARE


class KineticEnergy(SurfaceExpression):
    """KineticEnergy(u, v): (ℑx(u²) + ℑy(v²))/2, ke_at_ccc."""
    kind = abi.TERM_KINETIC_ENERGY

    def __init__(self, u, v):
        super().__init__(u, v)


class East(SurfaceExpression):
    """East(u, v, at_centers=False): the geographic east component p·cos θ − q·sin θ of a grid-aligned vector, p = ℑx u and
    q = ℑy v (face fields) or p = u, q = v with at_centers (visualize/cache.jl:462-464)."""
    kind, rotates = abi.TERM_EAST, True

    def __init__(self, u, v, at_centers=False):
        super().__init__(u, v)
        self.flags = abi.TERM_AT_CENTERS if at_centers else 0


class North(East):
    """North(u, v, at_centers=False): p·sin θ + q·cos θ."""
    kind = abi.TERM_NORTH


class Scaled(SurfaceExpression):
    """Scaled(expr, factor): factor · expr, as the scale of the term (a field alone: a FIELD term); nested factors are
    multiplied on the host."""

    def __init__(self, expr, factor):
        inner = isinstance(expr, SurfaceExpression)
        super().__init__(expr.a if inner else expr, expr.b if inner else None)
        self.expr, self.factor = expr, float(factor)
        self.rotates, self.fold_sign = getattr(expr, "rotates", False), getattr(expr, "fold_sign", -1.0)

    def term(self):
        if isinstance(self.expr, SurfaceExpression):
            kind, flags, a, b, scale = self.expr.term()
            return kind, flags, a, b, scale * self.factor
        return abi.TERM_FIELD, 0, self.expr, None, self.factor


def variance(mean_sq, mean):
    """mean(x²) − mean(x)² from two window means (visualize/cache.jl:370), host arrays; rounding may leave it slightly negative."""
    mean = np.asarray(mean)
    return np.asarray(mean_sq) - mean * mean


def grid_rotation(model):
    """(cos θ, sin θ) of the grid's i-axis against geographic east as ocean-grid device arrays: the interpolation weights'
    on a TripolarGrid, identity arrays (1, 0) on a LatitudeLongitudeGrid.  Made once per model."""
    itf = model.interfaces
    if getattr(itf, "_grid_rotation", None) is None:
        w, ctx = itf.weights, itf.context
        if w.get("cos_rot") is not None:
            itf._grid_rotation = (w["cos_rot"], w["sin_rot"])
        else:
            itf._grid_rotation = (ctx.zeros() + 1.0, ctx.zeros())
    return itf._grid_rotation


def omip_surface_outputs(model):
    """The reference's `:surface` writer (omip_diagnostics.jl:106-141) for the fields this repository has, by its names: tos,
    sos, uos, vos, the squares tossq, sossq, the centred squares uosq = ℑx(u²), vosq = ℑy(v²) and kes = ke_at_ccc
    (omip_diagnostics.jl:13-25,166-167,197), the fluxes tauuo, tauvo, hfds, wfo, hfss, hfls, and siconc / sithick with sea
    ice.  uosq, vosq and kes read u at [i+1] and v at [j+1]: the ocean fills those halos."""
    itf, st = model.interfaces, model.ocean.surface_state()
    net, ao = itf.net_fluxes._ocean_fields, itf.atmosphere_ocean_interface._fields
    T, S, u, v = st["T"], st["S"], st["u"], st["v"]
    out = dict(tos=T, sos=S, uos=u, vos=v, tossq=Squared(T), sossq=Squared(S),
               uosq=CenteredXSquare(u), vosq=CenteredYSquare(v), kes=KineticEnergy(u, v))
    groups = dict(net=net, atmosphere_ocean=ao)
    out.update({name: groups[group][key] for name, group, key in SURFACE_FLUX_OUTPUTS})
    ice = model.sea_ice
    if ice is not None:
        out["siconc"] = ice.concentration
        if ice.thickness is not None:
            out["sithick"] = ice.thickness
    return out


RHO_OCEAN, CP_OCEAN = 1026.0, 3991.86795711963   # visualize/common.jl:17-18


class BudgetTerm:
    """BudgetTerm(kind, scale=1.0): one part of the net heat or salt flux as an averaged output (cf_average_create_budget) —
    `kind` a name of runtime.BUDGET_KINDS ("heat_atmosphere_ocean", "salt_net", …) or abi.BUDGET_*; the sample is part · scale.
    The part is evaluated per cell inside the collection launch from the arrays the net fluxes were computed from; it is
    never written to memory."""

    def __init__(self, kind, scale=1.0):
        self.kind = BUDGET_KINDS[kind] if isinstance(kind, str) else int(kind)
        if not 0 <= self.kind < abi.BUDGET_KINDS:
            raise ValueError(f"BudgetTerm: kind = {kind!r}")
        self.scale = float(scale)


# the reference's budget fields (omip_diagnostics.jl:84-89,135-140) by its names, then the finer parts
BUDGET_OUTPUTS = (("JTao", "heat_atmosphere_ocean"), ("JTio", "heat_ice_ocean"), ("JTf", "heat_frazil"), ("JTn", "heat_net"),
                  ("JSn", "salt_net"), ("JSio", "salt_ice_ocean"),
                  ("heat_shortwave", "heat_shortwave"), ("heat_longwave_up", "heat_longwave_up"),
                  ("heat_longwave_down", "heat_longwave_down"), ("heat_sensible", "heat_sensible"), ("heat_latent", "heat_latent"),
                  ("salt_evaporation", "salt_evaporation"), ("salt_precipitation", "salt_precipitation"),
                  ("salt_atmosphere_ocean", "salt_atmosphere_ocean"), ("salt_land", "salt_land"))


def omip_budget_outputs(model):
    """The budget fields of the reference's `:surface` writer — JTao, JTio, JTf, JTn, JSn, JSio (omip_diagnostics.jl:84-89,
    135-140) — and the finer parts of the atmosphere–ocean terms under descriptive names: heat_shortwave, heat_longwave_up,
    heat_longwave_down, heat_sensible, heat_latent (they sum to JTao; the shortwave is left out of it under
    penetrating_shortwave), salt_evaporation, salt_precipitation (they sum to salt_atmosphere_ocean) and salt_land.  Fifteen
    BudgetTerm outputs: one more averager of a SurfaceFluxAverages writer."""
    return {name: BudgetTerm(kind) for name, kind in BUDGET_OUTPUTS}


def budget_inputs(model):
    """The arrays compute_net_ocean_fluxes! reads in this model, as the keywords of FluxContext.budget_average.  The exchange
    fields are interfaces' set 0: the state at the model's clock everywhere outside run!(simulation)."""
    itf, ice = model.interfaces, model.sea_ice
    kw = dict(ocean=model.ocean.surface_state(), atmos=itf._exchange_sets[0], fluxes=itf.atmosphere_ocean_interface._fields,
              weights=itf.weights)
    if ice is not None:
        kw["ice"] = {k: v for k, v in ice.fields().items() if k in ("concentration", "interface_heat", "salt_flux")}
        kw["frazil_heat"] = ice.frazil_heat
    if getattr(itf, "land_freshwater", None) is not None:
        kw["land_freshwater"] = itf.land_freshwater
    return kw


def geographic_surface_outputs(model):
    """What the reference's figures make of the time means before regridding (linear, so averaged directly): the wind stress
    in N m⁻² as geographic east / north components, −ρ · (ℑx tauuo, ℑy tauvo) rotated (cache.jl:372-386); the surface
    current the same way (cache.jl:430-466); hfds in W m⁻², ρ · cp · JT (cache.jl:359-361).  The rotation is grid_rotation's.
    The stress terms read tauuo at [i+1] and tauvo at [j+1], halo cells the library does not write: SurfaceFluxAverages fills
    them before every collection (see there).  The current's terms read the ocean's own u and v halos."""
    itf, st = model.interfaces, model.ocean.surface_state()
    net = itf.net_fluxes._ocean_fields
    return dict(tauuo_east=Scaled(East(net["u"], net["v"]), -RHO_OCEAN), tauvo_north=Scaled(North(net["u"], net["v"]), -RHO_OCEAN),
                uos_east=East(st["u"], st["v"]), vos_north=North(st["u"], st["v"]), hfds=Scaled(net["T"], RHO_OCEAN * CP_OCEAN))


class SurfaceFluxAverages:
    """An averaged output writer for surface fields: SurfaceFluxAverages(model; outputs, schedule = AveragedTimeInterval(5days)).
    The default outputs are the OMIP set tauuo, tauvo, hfds, wfo (the ocean's net u, v, T, S fluxes) and hfss, hfls (the
    atmosphere–ocean interface's sensible and latent heat); any dict name → ocean-grid device field works, sea-ice fields
    included.  The means are accumulated on the device (cf_average_collect: one launch per sample); a completed window is
    appended to `windows` as (t_k, {name: interior numpy array}) and handed to `on_window(t_k, arrays)`.  No file format.
    An output may also be a derived quantity — Squared, Product, CenteredX/Y, CenteredX/YSquare, KineticEnergy, East, North,
    Scaled (omip_surface_outputs and geographic_surface_outputs are presets): the outputs then go through
    cf_average_create_derived, abi.AVERAGE_MAX_FIELDS terms per launch, with `rotation` = (cos θ, sin θ) device arrays
    (default: grid_rotation(model)) for East / North.  More outputs than that make several averagers (`averagers`);
    `averager` is only the first of them, so attaching it to time_steps() collects the first sixteen outputs alone —
    models.time_steps(…, averages=writer) attaches them all.  BudgetTerm outputs (omip_budget_outputs is the preset) are parts
    of the net heat and salt flux evaluated inside the collection launch (cf_average_create_budget); they are grouped into
    averagers of their own after the others.
    Halos: a term that reads [i+1] / [j+1] of a field the LIBRARY writes (the net fluxes, the interface fluxes: written on the
    interior only) gets that field's first east halo column / north halo row filled here before every collection —
    periodic wrap in x (zero on a grid that does not close in longitude: the face is a wall), the tripolar fold
    (cf_fold_north_halo, y-face, the expression's fold_sign) or zero on a grid without a fold (the north wall).  A single
    slab only: neighbour slabs are not exchanged.  Every other field's halos (the ocean state's) are the caller's."""

    def __init__(self, model, outputs=None, schedule=None, on_window=None, rotation=None):
        itf = model.interfaces
        if outputs is None:
            groups = dict(net=itf.net_fluxes._ocean_fields, atmosphere_ocean=itf.atmosphere_ocean_interface._fields)
            outputs = {name: groups[group][key] for name, group, key in SURFACE_FLUX_OUTPUTS}
        self.model, self.outputs = model, dict(outputs)
        self.schedule = schedule if schedule is not None else AveragedTimeInterval(5 * days)
        self.on_window = on_window
        ctx = itf.context
        self.means = {name: ctx.zeros() for name in self.outputs}
        others = {name: o for name, o in self.outputs.items() if not isinstance(o, BudgetTerm)}
        if not others:
            self.averagers = []
        elif not any(isinstance(o, SurfaceExpression) for o in others.values()):
            self.averagers = [ctx.average(list(others.values()), [self.means[name] for name in others])]
        else:
            if rotation is None and any(getattr(o, "rotates", False) for o in others.values()):
                rotation = grid_rotation(model)
            self.averagers = [ctx.derived_average(terms, *(rotation or (None, None))) for terms in self.descriptor()]
            self._plan_halo_fills()
        # budget outputs: their own averagers, after the others.  They read the shortwave, longwave and precipitation of the
        # exchange state at the model's clock — inside run!(simulation) that state alternates between two field sets, so the
        # averagers are bound to three fields of the writer's, which write() fills from the current set before it collects
        # and models.time_steps lends to the device loop as that loop's Qs, Ql, Mp
        budget = self.budget_descriptor()
        if budget:
            self._budget_atmos = {name: ctx.zeros() for name in ("Qs", "Ql", "Mp")}
            inputs = dict(budget_inputs(model), atmos=self._budget_atmos)
            self.averagers += [ctx.budget_average(terms, **inputs) for terms in budget]
        self.averager = self.averagers[0]
        self.windows = []
        g = model.ocean.grid
        (self._nx, self._ny, _), (self._hx, self._hy, _) = g.size, g.halo

    def descriptor(self):
        """The term tables (kind, a, b, scale, flags, mean) of the outputs that are no BudgetTerm, abi.AVERAGE_MAX_FIELDS terms
        per averager."""
        terms = []
        for name, o in self.outputs.items():
            if isinstance(o, BudgetTerm):
                continue
            kind, flags, a, b, scale = o.term() if isinstance(o, SurfaceExpression) else (abi.TERM_FIELD, 0, o, None, 1.0)
            terms.append((kind, a, b, scale, flags, self.means[name]))
        n = abi.AVERAGE_MAX_FIELDS
        return [terms[k:k + n] for k in range(0, len(terms), n)]

    def budget_descriptor(self):
        """The term tables (kind, scale, mean) of the BudgetTerm outputs, abi.AVERAGE_MAX_FIELDS terms per averager."""
        terms = [(o.kind, o.scale, self.means[name]) for name, o in self.outputs.items() if isinstance(o, BudgetTerm)]
        n = abi.AVERAGE_MAX_FIELDS
        return [terms[k:k + n] for k in range(0, len(terms), n)]

    _budget_atmos = None

    def stage_exchange(self, exchange):
        """The Qs, Ql, Mp that the budget averagers read ← those of the exchange set `exchange` (three device copies)."""
        if self._budget_atmos is not None:
            for name, t in self._budget_atmos.items():
                if t.data_ptr() != exchange[name].data_ptr():
                    t.copy_(exchange[name])

    _east, _north = (), ()

    def _plan_halo_fills(self):
        itf = self.model.interfaces
        groups = [itf.net_fluxes._ocean_fields, itf.atmosphere_ocean_interface._fields, getattr(itf.net_fluxes, "_sea_ice_fields", {})]
        if getattr(itf, "atmosphere_sea_ice_interface", None) is not None:
            groups.append(itf.atmosphere_sea_ice_interface._fields)
        written = {t.data_ptr() for g in groups for t in g.values() if t is not None}
        east, north = {}, {}
        for o in self.outputs.values():
            if isinstance(o, SurfaceExpression):
                e, n = o.neighbours()
                east.update({t.data_ptr(): t for t in e if t.data_ptr() in written})
                north.update({t.data_ptr(): (t, o.fold_sign) for t in n if t.data_ptr() in written})
        self._east, self._north = list(east.values()), list(north.values())

    def fill_halos(self):
        """The first east halo column / north halo row of the library-written fields that a term reads there (class docstring)."""
        if not (self._east or self._north):
            return
        g, itf = self.model.ocean.grid, self.model.interfaces
        nx, ny, hx, hy = self._nx, self._ny, self._hx, self._hy
        lon = getattr(g, "longitude", None)
        periodic = getattr(g, "fold_north", False) or not isinstance(lon, tuple) or abs(abs(lon[1] - lon[0]) - 360.0) < 1e-9
        for t in self._east:
            if periodic:
                t[hy:hy + ny, hx + nx] = t[hy:hy + ny, hx]
            else:
                t[hy:hy + ny, hx + nx] = 0.0
        if self._north and getattr(itf, "fold_north", False):
            fields = [t for t, _ in self._north]
            itf.context.fold_north_halo(fields, [abi.FOLD_Y_FACE] * len(fields), [s for _, s in self._north], rows=1)
        else:
            for t, _ in self._north:
                t[hy + ny, hx:hx + nx] = 0.0

    def initialize(self, simulation):
        self.schedule.initialize(self.model.clock.time, simulation.dt)

    def write(self, clock):
        weight, t_k = self.schedule.sample(clock.time, clock.iteration)
        if weight is not None:
            self.fill_halos()
            if self._budget_atmos is not None:
                self.stage_exchange(self.model.interfaces.exchange_atmosphere_state)
            for averager in self.averagers:
                averager.collect(weight)
        if t_k is not None:
            hx, hy = self._hx, self._hy
            arrays = {name: m[hy:hy + self._ny, hx:hx + self._nx].to("cpu", copy=True).numpy() for name, m in self.means.items()}
            for averager in self.averagers:
                averager.reset()
            self.windows.append((t_k, arrays))
            if self.on_window is not None:
                self.on_window(t_k, arrays)


# ---------------------------------------------------------------------------------------------
# scalar time series: area-weighted surface integrals on the device (cf_integrals_*)
# ---------------------------------------------------------------------------------------------
REGION_GLOBAL, REGION_NORTH, REGION_SOUTH = 0, 1, 2   # bits of hemisphere_regions


def hemisphere_regions(grid):
    """The uint8 region array of the sea-ice diagnostics in the halo layout: bit 0 everywhere, bit 1 where φ > 0, bit 2 where
    φ < 0 — both strict, like arctic_condition / antarctic_condition (visualize/common.jl:715-787): a cell at exactly
    φ = 0 is in neither hemisphere."""
    phi = grid.cell_latitudes()
    return (1 + 2 * (phi > 0) + 4 * (phi < 0)).astype(np.uint8)


class IterationInterval:
    """IterationInterval(n): every n-th iteration."""

    def __init__(self, interval):
        if int(interval) != interval or interval < 1:
            raise ValueError(f"IterationInterval: interval = {interval} (an integer ≥ 1)")
        self.interval = int(interval)

    def actuate(self, iteration):
        return iteration % self.interval == 0


class _SeriesWriter:
    """What SurfaceIntegrals and SurfaceExtrema share: an output writer that appends one record to the device series of its
    recorder (the runtime.SurfaceIntegrator / SurfaceMonitor in the attribute `_recorder_name`) per scheduled iteration and
    moves a full series to the host."""
    _recorder_name = None
    _recorder = property(lambda self: getattr(self, self._recorder_name))

    def _begin(self, schedule):
        self.schedule = IterationInterval(schedule) if isinstance(schedule, int) else (schedule or IterationInterval(1))
        self._values, self._times = [], []

    def initialize(self, simulation):
        pass

    def _drain(self):
        values, times = self._recorder.read()
        if len(times):
            self._values.append(values)
            self._times.append(times)
            self._recorder.reset()

    def write(self, clock):
        if not self.schedule.actuate(clock.iteration):
            return
        if self._recorder.count() == self._recorder.capacity:
            self._drain()
        self._recorder.collect(clock.time)

    def records(self):
        """(values[n, n_entries] of the recorder's record type, times[n]): every record so far, raw entries in the order given."""
        self._drain()
        if not self._times:
            return np.zeros((0, self._recorder.n_entries), dtype=self._recorder._dtype), np.zeros(0)
        self._values, self._times = [np.concatenate(self._values)], [np.concatenate(self._times)]
        return self._values[0], self._times[0]

    @property
    def times(self):
        return self.records()[1]

    def close(self):
        self._recorder.close()


class SurfaceIntegrals(_SeriesWriter):
    """An output writer of scalar time series: SurfaceIntegrals(model, outputs; schedule = IterationInterval(1), regions, area).
    `outputs`: name → (kind, a[, b[, threshold[, region bit]]]) with kind "one" | "field" | "product" | "above" as in
    FluxContext.integrals, or "mean": ∫ a dA / ∫ dA over the same region, formed on the host from a "field" entry and the
    "one" entry of that region (added once per region).  Every collection is one record on the device
    (cf_integrals_collect: no host synchronisation); series() reads them.  A full device series is moved to the host and
    started again, so `capacity` bounds memory, not the length of a run.  `regions`: uint8 region bits (default: every cell in
    bit 0), `area`: cell areas (default: grid.cell_areas()), both host or device arrays in the halo layout."""

    _recorder_name = "integrator"

    def __init__(self, model, outputs, schedule=None, regions=None, area=None, capacity=4096):
        itf = model.interfaces
        ctx = self.ctx = itf.context
        self.model = model
        self._begin(schedule)
        on_device = lambda a: a if isinstance(a, torch.Tensor) else ctx.to_device(a)  # noqa: E731
        self.area = on_device(model.ocean.grid.cell_areas() if area is None else area)
        self.regions = None if regions is None else on_device(regions)
        mask = model.ocean.model.wet_mask if ctx.params.mask_kind == abi.MASK_U8 else None
        entries, self._columns, ones = [], {}, {}
        pad = lambda spec: tuple(spec) + ("one", None, None, 0.0, 0)[len(spec):]  # noqa: E731
        for name, spec in outputs.items():
            kind, a, b, threshold, bit = pad(spec)
            if kind == "mean":
                if bit not in ones:
                    ones[bit] = len(entries)
                    entries.append(("one", None, None, 0.0, bit))
                self._columns[name] = (len(entries), ones[bit])
                entries.append(("field", a, None, 0.0, bit))
            else:
                self._columns[name] = (len(entries), None)
                entries.append((kind, a, b, threshold, bit))
        self.entries = entries
        self.integrator = ctx.integrals(entries, area=self.area, mask=mask, region=self.regions, capacity=capacity)

    def series(self):
        """{name: np.ndarray[n]}: the integrals, and for "mean" outputs integral / integral of 1 over the same region."""
        values, _ = self.records()
        return {name: values[:, c] if one is None else values[:, c] / values[:, one] for name, (c, one) in self._columns.items()}


def sea_ice_integrals(model, threshold=0.15, **kw):
    """compute_ice_diagnostics (visualize/common.jl:715-787) as a writer: arctic_ / antarctic_ × volume ∫ hᵢ ℵ dA, area ∫ ℵ dA
    and extent ∫ [ℵ > 0.15] dA (threshold: common.jl:721), per step instead of from the 5-day means."""
    si = model.sea_ice
    if si is None or si.thickness is None:
        raise ValueError("sea_ice_integrals: the model has no sea ice with a thickness")
    outputs = {}
    for prefix, bit in (("arctic", REGION_NORTH), ("antarctic", REGION_SOUTH)):
        outputs[prefix + "_volume"] = ("product", si.thickness, si.concentration, 0.0, bit)
        outputs[prefix + "_area"] = ("field", si.concentration, None, 0.0, bit)
        outputs[prefix + "_extent"] = ("above", si.concentration, None, threshold, bit)
    kw.setdefault("regions", hemisphere_regions(model.ocean.grid))
    return SurfaceIntegrals(model, outputs, **kw)


def surface_global_means(model, **kw):
    """The global means of the reference's `:averages` writer (omip_diagnostics.jl:194-218) that live on the surface: hfds,
    wfo (the ocean's net T and S fluxes), hfss, hfls, tos, sos — area-weighted over the wet cells of region 0."""
    itf, st = model.interfaces, model.ocean.surface_state()
    net, ao = itf.net_fluxes._ocean_fields, itf.atmosphere_ocean_interface._fields
    fields = dict(hfds=net["T"], wfo=net["S"], hfss=ao["sensible_heat"], hfls=ao["latent_heat"], tos=st["T"], sos=st["S"])
    return SurfaceIntegrals(model, {name: ("mean", f, None, 0.0, REGION_GLOBAL) for name, f in fields.items()}, **kw)


# ---------------------------------------------------------------------------------------------
# calendar-binned means on the device (cf_climatology_*): the monthly climatologies under the reference's monthly figures
# ---------------------------------------------------------------------------------------------
def _month_start_seconds(reference_date, year, month):
    d = _dt.datetime(year, month, 1) - reference_date
    return d.days * 86400 + d.seconds


def calendar_bins(reference_date, first_time, last_time, kind="month", start_time=0, stop_time=math.inf):
    """The calendar table (edges, bin_of_interval) of cf_attach_climatology / cf_calendar_bin for times first_time … last_time
    [s since reference_date]: month(reference_date + Second(round(Int, t))) of compute_monthly_means (visualize/common.jl:184)
    as intervals of whole seconds in the proleptic Gregorian calendar (`datetime`, like Julia's Dates).  kind "month": bin
    m − 1 for calendar month m; "season": 0 DJF, 1 MAM, 2 JJA, 3 SON.  The edges are the month starts from the month of
    first_time to the end of the month of last_time; a rounded time outside [start_time, stop_time] (in_window, common.jl:161,
    applied to the rounded time) lies in an interval of bin −1: not collected."""
    if kind not in ("month", "season"):
        raise ValueError(f"calendar_bins: kind = {kind!r} (\"month\" or \"season\")")
    if not (math.isfinite(first_time) and math.isfinite(last_time) and first_time <= last_time):
        raise ValueError(f"calendar_bins: times {first_time} … {last_time}")
    first = reference_date + _dt.timedelta(seconds=round(first_time))
    last = reference_date + _dt.timedelta(seconds=round(last_time))
    months = []   # (start second, bin) from the month of `first` to the month after `last`
    y, m = first.year, first.month
    while True:
        months.append((_month_start_seconds(reference_date, y, m), m - 1 if kind == "month" else (m % 12) // 3))
        if (y, m) > (last.year, last.month):
            break
        y, m = (y, m + 1) if m < 12 else (y + 1, 1)
    lo = math.ceil(start_time) if math.isfinite(start_time) else (-math.inf if start_time < 0 else math.inf)
    hi = math.floor(stop_time) + 1 if math.isfinite(stop_time) else (math.inf if stop_time > 0 else -math.inf)
    cuts = sorted({s for s, _ in months} | {c for c in (lo, hi) if months[0][0] < c < months[-1][0]})
    edges, bins = np.array(cuts, dtype=np.float64), np.zeros(len(cuts) - 1, dtype=np.int32)
    starts = [s for s, _ in months]
    for k, a in enumerate(cuts[:-1]):
        owner = months[int(np.searchsorted(starts, a, side="right")) - 1][1]
        bins[k] = owner if lo <= a < hi else -1
    return edges, bins


class MonthlyClimatology:
    """An output writer of calendar-binned means: MonthlyClimatology(model, outputs; schedule = IterationInterval(1),
    reference_date = DateTime(1958, 1, 1), start_time = 0, stop_time = Inf) — compute_mean_and_monthly (visualize/common.jl:
    191-208) taken while the model runs instead of from stored snapshots.  `outputs`: name → ocean-grid device field (at most
    abi.CLIMATOLOGY_MAX_FIELDS).  Every scheduled iteration is one sample of equal weight (`sample_weight`: 1 but for the
    rounding of stride · (1 / stride)) — the reference counts snapshots —
    binned by month(reference_date + Second(round(Int, clock.time))) and collected in ONE launch (cf_climatology_collect) into
    the field's mean over all samples and into its month; samples outside [start_time, stop_time] are not collected.
    mean(name) / month(name, m) / extremes(name) read the device."""

    def __init__(self, model, outputs, schedule=None, reference_date=_dt.datetime(1958, 1, 1), start_time=0, stop_time=math.inf):
        ctx = self.ctx = model.interfaces.context
        self.model, self.outputs = model, dict(outputs)
        self.schedule = IterationInterval(schedule) if isinstance(schedule, int) else (schedule or IterationInterval(1))
        self.reference_date, self.start_time, self.stop_time = reference_date, start_time, stop_time
        self.n_bins = 12
        self.names = list(self.outputs)
        self.totals = {name: ctx.zeros() for name in self.names}
        self.bins = {name: torch.zeros((self.n_bins,) + tuple(ctx.shape), dtype=torch.float64, device=ctx.device) for name in self.names}
        self.climatology = ctx.climatology([self.outputs[n] for n in self.names], [self.totals[n] for n in self.names],
                                           [self.bins[n] for n in self.names], self.n_bins)
        self._table = None
        # every sample weighs the same: the product the step loop forms from a stride and a per-step weight (1 but for rounding)
        stride = getattr(self.schedule, "interval", 1)
        self.sample_weight = stride * (1.0 / stride)
        g = model.ocean.grid
        (self._nx, self._ny, _), (self._hx, self._hy, _) = g.size, g.halo

    def table(self, first_time, last_time):
        """The calendar table that covers first_time … last_time (kept and reused while it does)."""
        t = self._table
        if t is None or not (t[0][0] <= round(first_time) and round(last_time) < t[0][-1]):
            self._table = calendar_bins(self.reference_date, first_time, max(last_time, first_time + 400 * days), "month",
                                        self.start_time, self.stop_time)
        return self._table

    def initialize(self, simulation):
        pass

    def write(self, clock):
        if self.schedule.actuate(clock.iteration):
            self.climatology.collect(calendar_bin(self.table(clock.time, clock.time), clock.time), self.sample_weight)

    def _interior(self, t):
        hx, hy = self._hx, self._hy
        return t[hy:hy + self._ny, hx:hx + self._nx].to("cpu", copy=True).numpy()

    def mean(self, name):
        """The mean over every collected sample (interior, host array); None before the first."""
        return self._interior(self.totals[name]) if self.climatology.weights()[1] else None

    def month(self, name, m):
        """The mean over the samples of calendar month m = 1 … 12; None for a bin that received nothing — the
        reference's `nothing`."""
        if not 1 <= m <= self.n_bins:
            raise ValueError(f"month: m = {m} (1 … {self.n_bins})")
        return self._interior(self.bins[name][m - 1]) if self.climatology.weights()[3][m - 1] else None

    def extremes(self, name):
        """(min, max, argmin_month, argmax_month) over the available months per interior cell — reduce_monthly(c, sym, min | max)
        (visualize/cache.jl:696-712) with the month (1-based) that attains each; host arrays.  ValueError when no month is
        available, as the reference raises."""
        if not self.climatology.weights()[1]:
            raise ValueError(f"{name} has no available monthly bins")
        lo, hi, alo, ahi = self.climatology.extremes(self.names.index(name))
        return self._interior(lo), self._interior(hi), self._interior(alo) + 1, self._interior(ahi) + 1

    def close(self):
        self.climatology.close()


def sea_ice_concentration_climatology(model, **kw):
    """What sic_mean, sic_march and sic_september read (visualize/cache.jl:634-648): the writer of the sea-ice concentration's
    mean and monthly means — w.mean("sic"), w.month("sic", 3), w.month("sic", 9)."""
    si = model.sea_ice
    if si is None or si.concentration is None:
        raise ValueError("sea_ice_concentration_climatology: the model has no sea ice")
    return MonthlyClimatology(model, {"sic": si.concentration}, **kw)


# ---------------------------------------------------------------------------------------------
# extrema, non-finite counts and state hashes on the device (cf_monitor_*): the progress callbacks and the NaN checker
# ---------------------------------------------------------------------------------------------
MONITOR_COLUMNS = ("min", "max", "argmin", "argmax", "nan_count", "inf_count", "first_nonfinite", "hash")
_log = logging.getLogger("coflux")


def _model_monitor(model, fields, capacity):
    """A SurfaceMonitor over `fields` (name → field or (field, kind)) of `model`, under its wet mask."""
    ctx = model.interfaces.context
    mask = model.ocean.model.wet_mask if ctx.params.mask_kind == abi.MASK_U8 else None
    return ctx.monitor(list(fields.values()), mask=mask, capacity=capacity)


def _cell(c, nx):
    """(j, i) of the interior cell numbered c = j·nx + i; (−1, −1) for none"""
    return (int(c) // nx, int(c) % nx) if c >= 0 else (-1, -1)


class SurfaceExtrema(_SeriesWriter):
    """An output writer of extrema, non-finite counts and hashes: SurfaceExtrema(model, outputs; schedule = IterationInterval(1)).
    `outputs`: name → field or (field, "value" | "abs").  Every collection is one record on the device (cf_monitor_collect: no
    host synchronisation); series() reads them.  A full device series is moved to the host and started again, so `capacity`
    bounds memory, not the length of a run."""

    _recorder_name = "monitor"

    def __init__(self, model, outputs, schedule=None, capacity=4096):
        self.model, self.names = model, list(outputs)
        self._begin(schedule)
        self.nx = model.ocean.grid.size[0]
        self.monitor = _model_monitor(model, outputs, capacity)

    def series(self):
        """{name: {"min", "max", "argmin", "argmax", "nan_count", "inf_count", "first_nonfinite", "hash"}}: arrays of n records;
        the three indices are (j, i) pairs, (−1, −1) where there is none."""
        values, _ = self.records()
        out = {}
        for k, name in enumerate(self.names):
            v = values[:, k]
            pairs = lambda c: np.array([_cell(x, self.nx) for x in c], dtype=np.int64).reshape(len(c), 2)  # noqa: E731
            out[name] = {"min": v["minimum"].copy(), "max": v["maximum"].copy(), "argmin": pairs(v["argmin"]), "argmax": pairs(v["argmax"]),
                         "nan_count": v["nan_count"].copy(), "inf_count": v["inf_count"].copy(),
                         "first_nonfinite": pairs(v["first_nonfinite"]), "hash": v["hash"].copy()}
        return out


def prettytime(t):
    """Oceananigans.Utils.prettytime: the largest unit that keeps the value ≥ 1, an integer printed as one, else three decimals."""
    if t == 0:
        return "0 seconds"
    for unit, name in ((365 * days, "year"), (days, "day"), (hours, "hour"), (minutes, "minute"), (1.0, "second"), (1e-3, "ms"),
                       (1e-6, "μs"), (1e-9, "ns")):
        if abs(t) >= unit or unit == 1e-9:
            value = t / unit
            break
    if unit >= 1.0 and value != 1:
        name += "s"
    return f"{int(value)} {name}" if float(value).is_integer() else f"{value:.3f} {name}"


def _julia(fmt, x):
    """@sprintf(fmt, x) of a Float64: Julia prints NaN, Inf and -Inf where C prints nan, inf and -inf"""
    return "NaN" if x != x else ("Inf" if x == float("inf") else ("-Inf" if x == -float("inf") else fmt % x))


class Progress:
    """ClimaOcean.Progress (src/ClimaOcean.jl:48-88) as a callback of run!: add_callback(simulation, Progress(), schedule).
    One monitor over hᵢ and ℵ (when the model has sea ice with a thickness) and T, S, u, v is collected once per call — one
    pass on the device, 64 bytes per field read back; no field is copied to the host.  The message is the reference's, format
    strings included; it is logged (logger "coflux", INFO), kept in `message` and returned.  maximum and minimum follow Julia:
    NaN when the field holds a NaN on a wet cell.  The extrema are over the wet surface cells.  The surface mirror has no w:
    the velocity part prints two components, maximum(u): (umax, vmax), where the reference prints three."""

    def __init__(self):
        self.wall_time = time.perf_counter()
        self.monitor, self.message, self.record = None, None, None

    def _fields(self, model):
        st, si = model.ocean.surface_state(), model.sea_ice
        fields = {}
        if si is not None and getattr(si, "thickness", None) is not None:
            fields.update({"h": si.thickness, "ℵ": si.concentration})   # (a literal key: a keyword ℵ would be NFKC-normalised)
        fields.update(T=st["T"], S=st["S"], u=st["u"], v=st["v"])
        return fields

    def _collect(self, model):
        """{name: (maximum, minimum, value)} of one collection at the model's clock"""
        if self.monitor is None:
            self.names = list(self._fields(model))
            self.monitor = _model_monitor(model, self._fields(model), 1)
        self.monitor.reset()
        self.monitor.collect(model.clock.time)
        values, _ = self.monitor.read()
        self.record = dict(zip(self.names, values[0]))
        nan = float("nan")
        return {k: (nan if v["nan_count"] > 0 else float(v["maximum"]), nan if v["nan_count"] > 0 else float(v["minimum"]))
                for k, v in self.record.items()}

    def _head(self, sim):
        return "time: %s, iteration: %d, Δt: %s, " % (prettytime(sim.model.clock.time), sim.model.clock.iteration, prettytime(sim.dt))

    def _ice(self, x):
        return "max(h): %s m, max(ℵ): %s " % (_julia("%.2e", x["h"][0]), _julia("%.2e", x["ℵ"][0])) if "h" in x else ""

    def _emit(self, message):
        self.message = message
        _log.info(message)
        self.wall_time = time.perf_counter()
        return message

    def __call__(self, sim):
        x = self._collect(sim.model)
        step_time = time.perf_counter() - self.wall_time
        msg4 = "extrema(T, S): (%s, %s) ᵒC, (%s, %s) psu, " % tuple(_julia("%.2f", v) for v in x["T"] + x["S"])   # (max, min)
        msg5 = "maximum(u): (%s, %s) m/s, " % (_julia("%.2e", x["u"][0]), _julia("%.2e", x["v"][0]))
        msg6 = "wall time: %s \n" % prettytime(step_time)
        return self._emit(self._head(sim) + self._ice(x) + msg4 + msg5 + msg6)

    def close(self):
        if self.monitor is not None:
            self.monitor.close()


class OmipProgress(Progress):
    """omip_progress_callback (OMIPConfigurations/omip_simulation.jl:644-691): the same collection as Progress with that
    callback's message — extrema(T, S) as (Tmin, Tmax), (Smin, Smax) — and, at iterations 1, 5, 100 and 1000, the determinism
    probe `STATE_HASH iter=%d  T=%016x  S=%016x  u=%016x  h=%016x` (:671-683).  The four words are the hashes of the SAME
    record (include/coflux.h, cf_monitor_value.hash: the library's hash, not Julia's hash(::Array)), so no field is copied to
    the host; h is 0 for a model without sea-ice thickness.  `hashes` keeps {iteration: line}."""
    HASH_ITERATIONS = (1, 5, 100, 1000)

    def __init__(self):
        super().__init__()
        self.hashes = {}

    def __call__(self, sim):
        x = self._collect(sim.model)
        step_time = time.perf_counter() - self.wall_time
        (Tmax, Tmin), (Smax, Smin) = x["T"], x["S"]
        msg3 = "extrema(T, S): (%s, %s) ᵒC, (%s, %s) psu " % tuple(_julia("%.2f", v) for v in (Tmin, Tmax, Smin, Smax))
        msg4 = "maximum(u): (%s, %s) m/s, " % (_julia("%.2e", x["u"][0]), _julia("%.2e", x["v"][0]))
        msg5 = "wall time: %s" % prettytime(step_time)
        message = self._head(sim) + self._ice(x) + msg3 + msg4 + msg5
        it = sim.model.clock.iteration
        if it in self.HASH_ITERATIONS:
            r = self.record
            line = "STATE_HASH iter=%d  T=%016x  S=%016x  u=%016x  h=%016x" % (it, int(r["T"]["hash"]), int(r["S"]["hash"]), int(r["u"]["hash"]),
                                                                              int(r["h"]["hash"]) if "h" in r else 0)
            self.hashes[it] = line
            _log.info(line)
        return self._emit(message)


def omip_progress_callback():
    """omip_progress_callback(wall_time) of the reference: a callback for add_callback(simulation, …, IterationInterval(1))."""
    return OmipProgress()


class NaNChecker:
    """Oceananigans' NaNChecker as a callback: NaNChecker(fields; schedule = IterationInterval(100)), added with
    add_callback(simulation, checker, checker.schedule).  `fields`: name → ocean-grid field; default: the ocean's net fluxes
    (u, v, T, S) and the surface temperature T.  One collection per call and 16 bytes read back (cf_monitor_status); on a
    non-finite wet cell it clears `simulation.running` and keeps `first` = (iteration, name, (j, i)) — the first such field in
    the order of `fields` and its first such cell.  Deviation: it also stops on ±Inf, where Oceananigans looks for NaN only."""

    def __init__(self, fields=None, schedule=None):
        self.fields = fields
        self.schedule = IterationInterval(schedule) if isinstance(schedule, int) else (schedule or IterationInterval(100))
        self.monitor, self.first = None, None

    def __call__(self, sim):
        model = sim.model
        if self.monitor is None:
            if self.fields is None:
                net = model.interfaces.net_fluxes._ocean_fields
                self.fields = {"net_" + k: net[k] for k in ("u", "v", "T", "S")}
                self.fields["T"] = model.ocean.surface_state()["T"]
            self.names = list(self.fields)
            self.monitor = _model_monitor(model, self.fields, 1)
        self.monitor.reset()
        self.monitor.collect(model.clock.time)
        record, entries = self.monitor.status()
        if record < 0:
            return
        e = (entries & -entries).bit_length() - 1          # the lowest entry that had one
        value = self.monitor.read()[0][0, e]
        if self.first is None:
            self.first = (model.clock.iteration, self.names[e], _cell(value["first_nonfinite"], model.ocean.grid.size[0]))
        _log.error("NaNChecker: %s is not finite at %s, iteration %d: the simulation stops", self.names[e], self.first[2], model.clock.iteration)
        sim.running = False

    def close(self):
        if self.monitor is not None:
            self.monitor.close()


class JRA55PrescribedLand:
    """JRA55PrescribedLand(arch; …) — atmosphere.jl:46: river discharge and calving (friver, licalvf of
    jra55_data_staging.jl:8) as 3-hourly Float32 windows on the JRA55 grid; OceanSeaIceModel(…; land) interpolates them
    each step and the freshwater reaches the salinity flux.

    Two backends, like the atmosphere: the whole record in memory (`snapshots` = {friver, licalvf}: [n, 320, 640]), or a
    sliding window of `time_indices_in_memory` device slots fed by `provider(n) -> {friver, licalvf}: [320, 640]`
    (`total_snapshots` records; `cyclic` = RepeatYearJRA55, clamped = MultiYearJRA55).  The window follows the monotone
    snapshot COUNTER (slot = counter mod slots), so a repeat year whose length is no multiple of the slot count never
    puts two consecutive snapshots in one slot.  Two 0.8 MB planes per 3 h: read synchronously, no prefetch thread."""

    def __init__(self, snapshots=None, *, provider=None, total_snapshots=None, time_indices_in_memory=2, time_interval=3 * hours,
                 device=0, cyclic=True, source_size=(synthetic.JRA55_NX, synthetic.JRA55_NY)):
        dev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        self.time_interval = time_interval
        self.cyclic = cyclic
        self.provider = provider
        if provider is not None:
            if total_snapshots is None:
                raise ValueError("a snapshot provider needs total_snapshots")
            if time_indices_in_memory < 2:
                raise ValueError("time_indices_in_memory must be >= 2")
            self.n_levels = total_snapshots
            self.n_slots = time_indices_in_memory
            shape = (self.n_slots, source_size[1], source_size[0])
            self.data = {k: torch.zeros(shape, dtype=torch.float32, device=dev) for k in ("friver", "licalvf")}
            self._slot_counter = [None] * self.n_slots   # which snapshot counter each slot holds
            return
        if snapshots is None:
            snapshots = synthetic.jra55_land_snapshots(time_indices_in_memory)
        self.data = {k: torch.as_tensor(np.ascontiguousarray(v, dtype=np.float32)).to(dev) for k, v in snapshots.items()}
        self.n_levels = self.data["friver"].shape[0]

    def _wrap(self, n):
        return n % self.n_levels if self.cyclic else min(max(n, 0), self.n_levels - 1)

    def levels(self, t):
        """(level1, level2, ñ) into `self.data` for model time t — the bracketing snapshots made resident first on the
        sliding-window backend.  Cyclic (repeat year) or clamped (multi-year record ends) like the atmosphere."""
        x = t / self.time_interval
        base = int(np.floor(x))
        frac = x - base
        if self.cyclic:
            k1, k2 = base, base + 1
        else:
            k1 = min(max(base, 0), self.n_levels - 1)
            k2 = min(max(base + 1, 0), self.n_levels - 1)
            if not (0 <= base < self.n_levels - 1):
                frac = 0.0
        if self.provider is None:
            return self._wrap(k1), self._wrap(k2), frac
        for k in (k1, k2):
            slot = k % self.n_slots
            if self._slot_counter[slot] != k:
                snap = self.provider(self._wrap(k))
                for v, dst in self.data.items():
                    plane = snap.get(v)
                    if plane is None:
                        dst[slot].zero_()
                    else:
                        dst[slot].copy_(torch.from_numpy(np.array(plane, dtype=np.float32)))  # (a copy: memory-mapped planes are read-only)
                self._slot_counter[slot] = k
        return k1 % self.n_slots, k2 % self.n_slots, frac


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


# ---------------------------------------------------------------------------------------------
# checkpoint and pickup (cf_checkpoint_*): Checkpointer, run!(simulation; pickup = true)
# ---------------------------------------------------------------------------------------------
class TimeInterval:
    """TimeInterval(interval): actuates when the clock reaches k · interval, k = 1, 2, … — the schedule of the reference's
    Checkpointer (omip_diagnostics.jl:220-225).  A step counts as having reached k · interval when it is within 1e-6 · Δt of
    it, AveragedTimeInterval's rule.  Host bookkeeping only."""

    def __init__(self, interval):
        if not (interval > 0):
            raise ValueError(f"TimeInterval: interval = {interval} (> 0)")
        self.interval = float(interval)
        self.k = None   # the next actuation is at k · interval
        self._tol = 0.0

    def initialize(self, time, dt):
        """Opens the first interval that ends after `time` (called again after a pickup, with the restored clock)."""
        self._tol = 1e-6 * dt
        self.k = int(np.floor((time + self._tol) / self.interval)) + 1

    def actuate(self, time):
        if self.k is None:
            self.initialize(0.0, 0.0)
        if time >= self.k * self.interval - self._tol:
            self.k = int(np.floor((time + self._tol) / self.interval)) + 1
            return True
        return False


class Checkpointer:
    """Checkpointer(model; schedule = TimeInterval(…) | IterationInterval(n), dir = ".", prefix = "checkpoint", cleanup =
    false) — the output writer every reference launch installs (omip_diagnostics.jl:220-225), for run!(simulation; pickup).
    The files `<dir>/<prefix>_iteration<N>.cfck` are images of cf_checkpoint_capture: THIS LIBRARY'S OWN FORMAT, NOT JLD2.
    initialize(simulation) registers every device field of the model — the ocean's T, S, u, v (whole 3-D arrays), wet_mask, the
    top boundary condition fields and the shortwave flux, every sea-ice field that is set, the exchange state at the model's
    clock (through a staging set of the writer's: inside run! the current state alternates between two sets), the interface
    and net-flux fields, land_freshwater, the ice–ocean fluxes, and the buffers of a NormalizeSalinity among the callbacks —
    and, of every SurfaceFluxAverages, MonthlyClimatology, SurfaceIntegrals and SurfaceExtrema among the simulation's writers,
    the device arrays and the library handles (weights, counts, times, records, the monitor's status).  The image's host blob
    is JSON: both clocks, each writer's schedule state (AveragedTimeInterval.k / .previous, the climatology's window), the
    registered names.
    write() captures — stream ordered, one launch — and returns; the image drains while the next steps run, and the file is
    written (to a temporary name, then renamed; `cleanup` then removes the previous file — after a pickup that is the file
    picked up, once the next one is whole) by the next write(), by flush() or by close().
    NOT in a checkpoint: what a writer has already delivered to the host — SurfaceFluxAverages.windows, the drained chunks of
    a series writer (`_values`, `_times`) — which is the caller's, as the reference's output files are; the
    atmosphere and land windows, which are re-read for the restored clock; the solver's schedules and hints, which are rebuilt
    and never change a bit."""
    SUFFIX = ".cfck"

    def __init__(self, model, schedule=None, dir=".", prefix="checkpoint", cleanup=False, direct=False):
        self.model = model
        self.schedule = IterationInterval(schedule) if isinstance(schedule, int) else (schedule or TimeInterval(30 * days))
        self.dir, self.prefix, self.cleanup, self.direct = str(dir), str(prefix), bool(cleanup), bool(direct)
        self.checkpoint = None      # the runtime.Checkpoint, made by initialize
        self.names = []
        self._simulation = None
        self._pending = None        # iteration of the capture whose image is still draining
        self._previous_file = None
        self._exchange = None

    # -- files ------------------------------------------------------------------------------------
    def path(self, iteration):
        import os
        return os.path.join(self.dir, f"{self.prefix}_iteration{int(iteration)}{self.SUFFIX}")

    def iterations(self):
        """The iterations of this writer's files in `dir`, ascending."""
        import os
        import re
        pattern = re.compile(re.escape(self.prefix) + r"_iteration(\d+)" + re.escape(self.SUFFIX) + "$")
        found = [pattern.match(name) for name in (os.listdir(self.dir) if os.path.isdir(self.dir) else [])]
        return sorted(int(m.group(1)) for m in found if m)

    def latest(self):
        """The path of the file with the highest iteration, or None."""
        its = self.iterations()
        return self.path(its[-1]) if its else None

    def _write_file(self, iteration, image):
        import os
        os.makedirs(self.dir, exist_ok=True)
        path = self.path(iteration)
        tmp = path + ".tmp"
        with open(tmp, "wb") as f:
            f.write(image)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)   # a reader finds the old file or the whole new one, never a part
        if self.cleanup and self._previous_file and self._previous_file != path and os.path.exists(self._previous_file):
            os.remove(self._previous_file)
        self._previous_file = path

    # -- registration -----------------------------------------------------------------------------
    def _add(self, name, tensor):
        """Registers `tensor` unless its bytes are already part of a registered array (the top boundary conditions ARE the net
        fluxes, the sea ice's interface_heat IS the ice–ocean exchange's)."""
        if tensor is None or not isinstance(tensor, torch.Tensor):
            return
        lo, hi = tensor.data_ptr(), tensor.data_ptr() + tensor.numel() * tensor.element_size()
        if any(a <= lo and hi <= b for a, b in self._ranges):
            return
        self.checkpoint.add_array(name, tensor)
        self._ranges.append((lo, hi))
        self.names.append(name)

    def initialize(self, simulation):
        if self.checkpoint is not None:
            if isinstance(self.schedule, TimeInterval):
                self.schedule.initialize(self.model.clock.time, simulation.dt)
            return
        self._simulation = simulation
        m, itf = self.model, self.model.interfaces
        ctx = itf.context
        self.checkpoint = ctx.checkpoint(direct=self.direct)
        self._ranges, self.names = [], []
        om = m.ocean.model
        for name, t in (("ocean.T", om.tracers.T), ("ocean.S", om.tracers.S), ("ocean.u", om.velocities.u), ("ocean.v", om.velocities.v),
                        ("ocean.wet_mask", om.wet_mask), ("ocean.shortwave_surface_flux", om.shortwave_surface_flux)):
            self._add(name, t)
        for k in ("u", "v", "T", "S"):
            bc = getattr(om.top_boundary_conditions, k)
            self._add(f"ocean.top.{k}", bc.flux_field if isinstance(bc, MultipleFluxes) else bc)
        if m.sea_ice is not None:
            for k in ("concentration", "interface_heat", "salt_flux", "x_stress", "y_stress", "thickness", "top_surface_temperature", "u", "v",
                      "albedo", "frazil_heat", "snow_thickness"):
                self._add(f"sea_ice.{k}", getattr(m.sea_ice, k))
        self._exchange = ctx.field_set(EXCHANGE_NAMES)
        for k, t in self._exchange.items():
            self._add(f"exchange.{k}", t)
        groups = [("atmosphere_ocean", itf.atmosphere_ocean_interface._fields), ("net.ocean", itf.net_fluxes._ocean_fields)]
        if itf.atmosphere_sea_ice_interface is not None:
            groups += [("atmosphere_sea_ice", itf.atmosphere_sea_ice_interface._fields), ("net.sea_ice", itf.net_fluxes._sea_ice_fields)]
        if getattr(itf, "sea_ice_ocean_heat_flux", None) is not None:
            groups.append(("sea_ice_ocean", itf.sea_ice_ocean_fluxes))
        for group, fields in groups:
            for k, t in fields.items():
                self._add(f"{group}.{k}", t)
        self._add("land_freshwater", getattr(itf, "land_freshwater", None))
        for cname, cb in simulation.callbacks.items():
            if isinstance(cb.func, NormalizeSalinity):
                self._add(f"callback.{cname}.additional", cb.func.additional_buffer)
                self._add(f"callback.{cname}.mean", cb.func.mean_total)
        for wname, w in simulation.output_writers.items():
            if isinstance(w, SurfaceFluxAverages):
                for k, t in w.means.items():
                    self._add(f"{wname}.mean.{k}", t)
                for k, t in (w._budget_atmos or {}).items():
                    self._add(f"{wname}.budget.{k}", t)
                for n, a in enumerate(w.averagers):
                    self._add_handle(f"{wname}.averager{n}", a)
            elif isinstance(w, MonthlyClimatology):
                for k in w.names:
                    self._add(f"{wname}.total.{k}", w.totals[k])
                    self._add(f"{wname}.bins.{k}", w.bins[k])
                self._add_handle(f"{wname}.climatology", w.climatology)
            elif isinstance(w, _SeriesWriter):
                self._add_handle(f"{wname}.series", w._recorder)
        too_long = [n for n in self.names if len(n.encode()) > 47]
        assert not too_long, too_long
        if isinstance(self.schedule, TimeInterval):
            self.schedule.initialize(m.clock.time, simulation.dt)

    def _add_handle(self, name, handle):
        self.checkpoint.add(name, handle)
        self.names.append(name)

    # -- the host blob ----------------------------------------------------------------------------
    def _state(self):
        """What the image's host blob holds (JSON): both clocks, every writer's schedule state, the registered names."""
        m = self.model
        writers = {}
        for wname, w in (self._simulation.output_writers.items() if self._simulation is not None else ()):
            s = getattr(w, "schedule", None)
            if isinstance(s, AveragedTimeInterval):
                writers[wname] = dict(kind="averaged", k=s.k, previous=s.previous)
            elif isinstance(w, MonthlyClimatology):
                writers[wname] = dict(kind="climatology", start_time=w.start_time, stop_time=w.stop_time, reference_date=w.reference_date.isoformat())
        return dict(format="coflux-checkpoint", clock=dict(time=m.clock.time, iteration=m.clock.iteration),
                    ocean_clock=dict(time=m.ocean.model.clock.time, iteration=m.ocean.model.clock.iteration), writers=writers,
                    names=list(self.names))

    def _check_state(self, state, path):
        """ValueError unless the blob is this simulation's: the same registration, the same writers, the same climatology window."""
        if state.get("names") != list(self.names):
            raise ValueError(f"pickup: {path} was written by another registration than this simulation's")
        for wname, s in state["writers"].items():
            w = self._simulation.output_writers.get(wname)
            if w is None:
                raise ValueError(f"pickup: {path} has the state of a writer {wname!r} that this simulation lacks")
            if s["kind"] == "climatology" and (s["start_time"], s["stop_time"]) != (w.start_time, w.stop_time):
                raise ValueError(f"pickup: the climatology {wname!r} of {path} was collected over another window")

    def _set_state(self, state):
        m = self.model
        m.clock.time, m.clock.iteration = float(state["clock"]["time"]), int(state["clock"]["iteration"])
        m.ocean.model.clock.time, m.ocean.model.clock.iteration = float(state["ocean_clock"]["time"]), int(state["ocean_clock"]["iteration"])
        for wname, s in state["writers"].items():
            if s["kind"] == "averaged":
                w = self._simulation.output_writers[wname]
                w.schedule.k, w.schedule.previous = int(s["k"]), float(s["previous"])

    # -- the writer -------------------------------------------------------------------------------
    def _actuates(self, clock):
        return self.schedule.actuate(clock.time) if isinstance(self.schedule, TimeInterval) else self.schedule.actuate(clock.iteration)

    def write(self, clock):
        self.flush()
        if not self._actuates(clock):
            return
        import json
        if self._exchange is not None:   # the exchange state at the model's clock, wherever run! keeps it at this step
            current = self.model.interfaces.exchange_atmosphere_state
            for k, t in self._exchange.items():
                t.copy_(current[k])
        self.checkpoint.set_host_blob(json.dumps(self._state()).encode())
        self.checkpoint.capture()
        self._pending = int(clock.iteration)

    def flush(self):
        """Waits for the image of the last capture, if one is still draining, and writes its file."""
        if self._pending is None:
            return
        iteration, self._pending = self._pending, None
        self._write_file(iteration, self.checkpoint.wait(copy=False))

    def close(self):
        self.flush()
        if self.checkpoint is not None:
            self.checkpoint.close()

    # -- pickup -----------------------------------------------------------------------------------
    def pickup(self, which=True):
        """Restores the model, the other writers and the clocks from a file: True / "latest" the highest iteration (None found:
        a warning, nothing restored, returns None), an int that iteration, any other str that path.  Returns the path."""
        import json
        import os
        import warnings
        from .runtime import checkpoint_host_blob
        if which is True or which == "latest":
            path = self.latest()
            if path is None:
                warnings.warn(f"pickup: no {self.prefix}_iteration*{self.SUFFIX} in {self.dir!r}; starting from scratch")
                return None
        else:
            path = self.path(which) if isinstance(which, (int, np.integer)) else str(which)
            if not os.path.exists(path):
                raise FileNotFoundError(f"pickup: {path} does not exist")
        with open(path, "rb") as f:
            image = f.read()
        state = json.loads(checkpoint_host_blob(image).decode())   # (verifies the whole image first)
        self._check_state(state, path)                             # nothing is restored from a file of another simulation
        self.checkpoint.restore(image)
        self._set_state(state)
        itf = self.model.interfaces
        # the state at the model's clock lies in exchange set 0, nothing is requested ahead: what run!'s own exit establishes
        itf._next_state_in_other = False
        itf.context.discard_prefetched_atmosphere_state()
        itf._exchange_current = 0
        for k, t in self._exchange.items():
            itf._exchange_sets[0][k].copy_(t)
        if getattr(self.model, "land", None) is not None and hasattr(itf, "land_freshwater"):
            itf.context.set_land_freshwater(itf.land_freshwater)
        if isinstance(self.schedule, TimeInterval) and self._simulation is not None:
            self.schedule.initialize(self.model.clock.time, self._simulation.dt)
        itf.context.sync()   # the restore's device-side hashes are checked here
        self._previous_file = path
        return path
