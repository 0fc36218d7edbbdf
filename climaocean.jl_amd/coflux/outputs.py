"""Output writers and callbacks of run!(simulation): the surface expressions and SurfaceFluxAverages, the scalar series
(SurfaceIntegrals, SurfaceExtrema), MonthlyClimatology, their presets, Progress / OmipProgress and NaNChecker.  All of them
collect on the device; this is the bookkeeping around the library's handles."""
import datetime as _dt
import logging
import math
import time

import numpy as np
import torch

from . import abi
from .clocks import calendar_bins, days, hours, minutes
from .runtime import BUDGET_KINDS, calendar_bin
from .schedules import AveragedTimeInterval, IterationInterval, actuates, as_schedule

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
    if itf._grid_rotation is None:
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
    kw = dict(ocean=model.ocean.surface_state(), atmos=itf.exchange.stable, fluxes=itf.atmosphere_ocean_interface._fields,
              weights=itf.weights)
    if ice is not None:
        kw["ice"] = {k: v for k, v in ice.fields().items() if k in ("concentration", "interface_heat", "salt_flux")}
        kw["frazil_heat"] = ice.frazil_heat
    if itf.land_freshwater is not None:
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



class _SeriesWriter:
    """What SurfaceIntegrals and SurfaceExtrema share: an output writer that appends one record to the device series of its
    recorder (the runtime.SurfaceIntegrator / SurfaceMonitor in the attribute `_recorder_name`) per scheduled iteration and
    moves a full series to the host."""
    _recorder_name = None
    _recorder = property(lambda self: getattr(self, self._recorder_name))

    def _begin(self, schedule):
        self.schedule = as_schedule(schedule)
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
        if not actuates(self.schedule, clock):
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
        self.schedule = as_schedule(schedule)
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
        if actuates(self.schedule, clock):
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


def _cell(c, row_length):
    """(j, i) on the whole surface of the cell numbered c = j·row_length + i; (−1, −1) for none"""
    return (int(c) // row_length, int(c) % row_length) if c >= 0 else (-1, -1)


def _row_length(monitor, model):
    """The row length `monitor` numbers its cells with: its own, or the model grid's nx where it left that 0 (or is a
    monitor that knows no row length: one made with first_cell alone numbers its rows with nx)"""
    return getattr(monitor, "row_length", 0) or model.ocean.grid.size[0]


class SurfaceExtrema(_SeriesWriter):
    """An output writer of extrema, non-finite counts and hashes: SurfaceExtrema(model, outputs; schedule = IterationInterval(1)).
    `outputs`: name → field or (field, "value" | "abs").  Every collection is one record on the device (cf_monitor_collect: no
    host synchronisation); series() reads them.  A full device series is moved to the host and started again, so `capacity`
    bounds memory, not the length of a run."""

    _recorder_name = "monitor"

    def __init__(self, model, outputs, schedule=None, capacity=4096):
        self.model, self.names = model, list(outputs)
        self._begin(schedule)
        self.monitor = _model_monitor(model, outputs, capacity)
        self.row_length = _row_length(self.monitor, model)

    def series(self):
        """{name: {"min", "max", "argmin", "argmax", "nan_count", "inf_count", "first_nonfinite", "hash"}}: arrays of n records;
        the three indices are (j, i) pairs, (−1, −1) where there is none."""
        values, _ = self.records()
        out = {}
        for k, name in enumerate(self.names):
            v = values[:, k]
            pairs = lambda c: np.array([_cell(x, self.row_length) for x in c], dtype=np.int64).reshape(len(c), 2)  # noqa: E731
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
        self.schedule = as_schedule(schedule, IterationInterval(100))
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
            self.first = (model.clock.iteration, self.names[e], _cell(value["first_nonfinite"], _row_length(self.monitor, model)))
        _log.error("NaNChecker: %s is not finite at %s, iteration %d: the simulation stops", self.names[e], self.first[2], model.clock.iteration)
        sim.running = False

    def close(self):
        if self.monitor is not None:
            self.monitor.close()
