"""CPU tests of the budget averager's reference and host side (include/coflux.h: cf_average_create_budget,
cf_attach_average_slot).  The NumPy restatement (tests/budget_reference.py) is qualified alone: against the C oracle's net
fluxes on the designed case, against the definitions evaluated exactly, and by the closure of the parts with the roundings
counted in the restatement's header (n_T = 8, n_S = 5).  Five defects seeded into copies of it are each caught by a named cell.
The mirrors (abi.py, runtime.py, models.py, the Julia stub) are held to the header."""
import ctypes as C
import re
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import budget_reference as br
import oracle
import util
from coflux import abi
from coflux import interface_computations as ic
from coflux import models as cm
from coflux import runtime as rt
from test_julia_stub import HEADER, julia_structs, struct_size

NX, NY, HX, HY = 67, 5, 3, 2
TOL_NET = 1e-12           # the project's net-flux tolerance in the scaled metric of util.rel_err
DEFINITION_ROUNDINGS = 20   # no leaf of any kind passes more than 17 roundings (T⁴ of a rounded sum: 4 + 2 + 3, om, roc, 4 sums …)


def params(penetrating, latitude_dependent=False):
    surface = ic.SurfaceRadiationProperties(ic.LatitudeDependentAlbedo() if latitude_dependent else 0.06, 0.97)
    return ic.flux_params(ocean_surface=surface, ocean_minimum_salinity=br.S_MIN, penetrating_shortwave=penetrating)


def latitudes(ny):
    return np.linspace(-61.0, 74.5, ny)


def case(p, nx=NX, ny=NY):
    I = br.designed_case(nx, ny)
    I["alb"] = br.albedo_of(p, np.repeat(latitudes(ny)[:, None], nx, axis=1))
    return I


def oracle_net(p, I, nx=NX, ny=NY):
    """oracle_compute_net_ocean_fluxes on the designed case: (T, S, shortwave_surface_flux) on the interior"""
    H = lambda a, fill=0.0: br.halo_layout(a, HX, HY, fill)  # noqa: E731
    zero = np.zeros((ny, nx))
    ocean = dict(T=H(zero), S=H(I["S"]), u=H(zero), v=H(zero), mask=H(I["wet"].astype(np.uint8), 0))
    atmos = dict(u=H(zero), v=H(zero), T=H(zero), p=H(zero), q=H(zero), Qs=H(I["Qs"]), Ql=H(I["Ql"]), Mp=H(I["Mp"]))
    fluxes = dict(sensible_heat=H(I["Qc"]), latent_heat=H(I["Qv"]), water_vapor=H(I["Mv"]), x_momentum=H(zero), y_momentum=H(zero),
                  temperature=H(I["temperature"]))
    ice = dict(concentration=H(I["aice"]), interface_heat=H(I["Qio"]), salt_flux=H(I["Jsio"]))
    lat = np.zeros(ny + 2 * HY)
    lat[HY:HY + ny] = latitudes(ny)
    out = oracle.compute_net_ocean_fluxes(oracle.make_grid(nx, ny, HX, HY), p, ocean, atmos, fluxes, ice=ice,
                                          weights=dict(separable=True, latitude=lat), land=H(I["land"]))
    return tuple(out[k][HY:HY + ny, HX:HX + nx] for k in ("T", "S", "shortwave_surface_flux"))


def net_agrees(model, p, I, cell=None):
    """the restatement's HEAT_NET / SALT_NET against the oracle, in the scaled metric, everywhere or at one named cell"""
    T, S, _ = oracle_net(p, I)
    sel = (slice(None), slice(None)) if cell is None else (slice(0, 1), slice(br.CELLS[cell], br.CELLS[cell] + 1))
    return (util.rel_err(model.sample(br.HEAT_NET, I)[sel], T[sel], util.FIELD_SCALE["T"]) <= TOL_NET and
            util.rel_err(model.sample(br.SALT_NET, I)[sel], S[sel], util.FIELD_SCALE["S"]) <= TOL_NET)


@pytest.mark.parametrize("latitude_dependent", [False, True])
@pytest.mark.parametrize("penetrating", [False, True])
def test_restatement_agrees_with_the_oracle_on_the_designed_case(penetrating, latitude_dependent):
    p = params(penetrating, latitude_dependent)
    I = case(p)
    assert net_agrees(br.BudgetModel(p), p, I)
    sw = oracle_net(p, I)[2]
    assert util.rel_err(br.BudgetModel(p).sample(br.HEAT_SHORTWAVE, I), sw, util.FIELD_SCALE["shortwave_surface_flux"]) <= TOL_NET
    # the designed cells are what they are named
    c, m = br.CELLS, br.BudgetModel(p)
    assert not I["wet"][0, c["land"]] and I["aice"][0, c["full_ice"]] == 1.0 and 0.0 < I["aice"][0, c["partial_ice"]] < 1.0
    gate = m.floor_gate(I)
    assert gate[0, c["floor_freshening"]] and not gate[0, c["floor_evaporation"]] and I["S"][0, c["floor_evaporation"]] < br.S_MIN
    assert m.SFls(I)[0, c["floor_land"]] == 0.0 and I["land"][0, c["floor_land"]] > 0.0
    assert I["temperature"][0, c["frazil"]] < -1.9 and I["frazil"][0, c["frazil"]] > 0.0 and I["Qs"][0, c["dark"]] == 0.0
    assert all(np.all(m.sample(k, I)[0, c["land"]] == 0.0) for k in range(15))


def closure_excess(model, I):
    """(worst |Σ heat parts − JTao| / bound, worst |evaporation + precipitation − SALT_ATMOSPHERE_OCEAN| / bound) over the
    cells, the parts summed exactly; bound = n · 2⁻⁵³ · Σ|parts| (0 / 0 counts as 0: every part is then ±0)"""
    V = {k: model.sample(k, I) for k in range(15)}
    heat = [k for k in br.HEAT_PARTS if not (k == br.HEAT_SHORTWAVE and model.P.penetrating)]
    worst = [Fraction(0), Fraction(0)]
    for j, i in np.ndindex(I["wet"].shape):
        for n, (parts, whole, count) in enumerate(((heat, br.HEAT_ATMOSPHERE_OCEAN, br.N_T),
                                                   ((br.SALT_EVAPORATION, br.SALT_PRECIPITATION), br.SALT_ATMOSPHERE_OCEAN, br.N_S))):
            values = [V[k][j, i] for k in parts]
            diff = abs(br.exact_sum(values) - Fraction(float(V[whole][j, i])))
            bound = count * br.U * br.exact_sum(np.abs(values))
            if diff > 0:
                worst[n] = max(worst[n], diff / bound if bound > 0 else Fraction(10 ** 9))
    return float(worst[0]), float(worst[1])


@pytest.mark.parametrize("penetrating", [False, True])
def test_parts_close_within_the_counted_roundings(penetrating):
    p = params(penetrating)
    I, m = case(p), br.BudgetModel(p)
    heat, salt = closure_excess(m, I)
    assert heat <= 1.0 and salt <= 1.0, (heat, salt)
    # the net kinds are their parts with one / two more additions, bit for bit
    with np.errstate(all="ignore"):
        JTn = m.sample(br.HEAT_ATMOSPHERE_OCEAN, I) + m.sample(br.HEAT_ICE_OCEAN, I)
        JSn = m.sample(br.SALT_ATMOSPHERE_OCEAN, I) + m.sample(br.SALT_ICE_OCEAN, I) + m.sample(br.SALT_LAND, I)
    assert np.array_equal(JTn.view(np.int64), m.sample(br.HEAT_NET, I).view(np.int64))
    assert np.array_equal(JSn.view(np.int64), m.sample(br.SALT_NET, I).view(np.int64))


@pytest.mark.parametrize("penetrating", [False, True])
def test_restatement_is_the_definition_within_its_roundings(penetrating):
    p = params(penetrating)
    I, m = case(p), br.BudgetModel(p)
    V = {k: m.sample(k, I) for k in range(15)}
    for j, i in np.ndindex(I["wet"].shape):
        if not I["wet"][j, i]:
            continue
        exact = br.exact_parts(p, {name: I[name][j, i] for name in br.INPUT_NAMES + ("alb",)})
        for k, (x, mag) in exact.items():
            assert abs(Fraction(float(V[k][j, i])) - x) <= DEFINITION_ROUNDINGS * br.U * mag, (br.KIND_NAMES[k], j, i)


def test_scale_multiplies_the_selected_part_and_land_stays_zero():
    p = params(False)
    I, m = case(p), br.BudgetModel(p)
    x = m.sample(br.HEAT_NET, I, -cm.RHO_OCEAN * cm.CP_OCEAN)
    assert np.array_equal(x, m.sample(br.HEAT_NET, I) * np.float64(-cm.RHO_OCEAN * cm.CP_OCEAN))
    land = br.CELLS["land"]
    assert x[0, land] == 0.0 and np.signbit(x[0, land]) and not np.signbit(m.sample(br.HEAT_NET, I)[0, land])
    # a kind sees only what it reads: the other inputs absent (the library's NULL pointers) change nothing
    for k in range(15):
        assert np.array_equal(m.sample(k, br.only(I, [k])).view(np.int64), m.sample(k, I).view(np.int64)), br.KIND_NAMES[k]


# ---- planted defects: each copy of the model is caught by its named cell ----------------------------------------------------
class SensibleWithoutOm(br.BudgetModel):
    def heat_sensible(self, I):
        return self.get(I, "Qc") * self.roc()


class GatePerPart(br.BudgetModel):
    def part_gate(self, I, F):
        return (self.get(I, "S") < self.P.S_min) & (F < br.ZERO)


class LandIceMasked(br.BudgetModel):
    def salt_land(self, I):
        return self.om(I) * super().salt_land(I)

    def salt_net(self, I):
        So = self.get(I, "S")
        return self.om(I) * (-So * self.SFs(I)) + self.get(I, "Jsio") + self.om(I) * (-So * self.SFls(I))


class ShortwaveKeptWhenPenetrating(br.BudgetModel):
    def Qss(self, I):
        return self.Qts(I)


class FrazilInTheNet(br.BudgetModel):
    def heat_net(self, I):
        return super().heat_net(I) + self.heat_frazil(I)


def _cell_only(I, name):
    """the designed case cut down to one named cell (a 1 × 1 surface)"""
    c = br.CELLS[name]
    return {k: np.asarray(v)[0:1, c:c + 1] for k, v in I.items()}


def test_om_dropped_from_one_part_is_caught_at_the_partial_ice_cell():
    p = params(False)
    I = _cell_only(case(p), "partial_ice")
    assert closure_excess(br.BudgetModel(p), I)[0] <= 1.0 < closure_excess(SensibleWithoutOm(p), I)[0]
    open_water = _cell_only(case(p), "open_water")     # om = 1: the defect cannot show there
    assert closure_excess(SensibleWithoutOm(p), open_water)[0] <= 1.0


def test_floor_gate_per_part_is_caught_at_the_floor_evaporation_cell():
    """below the floor with net evaporation nothing is zeroed; a gate per part zeroes the precipitation alone"""
    p = params(False)
    I = _cell_only(case(p), "floor_evaporation")
    assert closure_excess(br.BudgetModel(p), I)[1] <= 1.0 < closure_excess(GatePerPart(p), I)[1]
    # and with net freshening both parts are zeroed; per part the evaporation survives
    I = _cell_only(case(p), "floor_freshening")
    assert closure_excess(br.BudgetModel(p), I)[1] <= 1.0 < closure_excess(GatePerPart(p), I)[1]
    assert br.BudgetModel(p).sample(br.SALT_EVAPORATION, I)[0, 0] == 0.0 != GatePerPart(p).sample(br.SALT_EVAPORATION, I)[0, 0]


def test_ice_masked_land_is_caught_at_the_partial_ice_cell():
    p = params(False)
    I = case(p)
    assert net_agrees(br.BudgetModel(p), p, I, "partial_ice") and not net_agrees(LandIceMasked(p), p, I, "partial_ice")
    assert net_agrees(LandIceMasked(p), p, I, "open_water")    # no ice, no land freshwater there


def test_shortwave_kept_under_penetrating_shortwave_is_caught_at_the_open_water_cell():
    p = params(True)
    I = case(p)
    assert net_agrees(br.BudgetModel(p), p, I, "open_water") and not net_agrees(ShortwaveKeptWhenPenetrating(p), p, I, "open_water")
    assert net_agrees(ShortwaveKeptWhenPenetrating(p), p, I, "dark")     # Qs = 0: nothing to keep
    q = params(False)
    assert net_agrees(ShortwaveKeptWhenPenetrating(q), q, case(q))        # not penetrating: it belongs in the sum


def test_frazil_added_into_the_net_is_caught_at_the_frazil_cell():
    p = params(False)
    I = case(p)
    assert net_agrees(br.BudgetModel(p), p, I, "frazil") and not net_agrees(FrazilInTheNet(p), p, I, "frazil")
    assert net_agrees(FrazilInTheNet(p), p, I, "open_water")


# ---- the mirrors --------------------------------------------------------------------------------------------------------------
def test_constants_structs_and_symbols_are_the_headers_and_the_stubs():
    for k, name in enumerate(br.KIND_NAMES):
        value = int(re.search(rf"#define CF_BUDGET_{name.upper()}\s+(\d+)", HEADER).group(1))
        assert getattr(abi, "BUDGET_" + name.upper()) == value == k == rt.BUDGET_KINDS[name], name
    assert abi.BUDGET_KINDS == int(re.search(r"#define CF_BUDGET_KINDS\s+(\d+)", HEADER).group(1)) == len(br.KIND_NAMES)
    assert abi.ATTACHED_AVERAGES_MAX == int(re.search(r"#define CF_ATTACHED_AVERAGES_MAX\s+(\d+)", HEADER).group(1)) == 4
    assert {"cf_average_create_budget", "cf_attach_average_slot"} <= set(abi.EXPORTED_SYMBOLS)
    structs = julia_structs()
    for name, twin in (("CfBudgetTerm", abi.BudgetTerm), ("CfBudgetDesc", abi.BudgetDesc)):
        assert struct_size(name, structs)[0] == C.sizeof(twin), name
        assert [f for f, _t in structs[name]] == [f for f, *_ in twin._fields_], name
    assert C.sizeof(abi.BudgetTerm) == 24 and C.sizeof(abi.BudgetDesc) == 80
    # the header's structs, field by field
    for c_name, twin in (("cf_budget_term", abi.BudgetTerm), ("cf_budget_desc", abi.BudgetDesc)):
        body = re.search(r"typedef struct " + c_name + r" \{(.*?)\} " + c_name + ";", HEADER, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [piece.split()[-1].lstrip("*") for decl in body.split(";") if decl.strip() for piece in decl.split(",")]
        assert fields == [f for f, *_ in twin._fields_], (c_name, fields)
    lib = abi.load_library()
    assert hasattr(lib, "cf_average_create_budget") and hasattr(lib, "cf_attach_average_slot")
    assert [n for n, _ in cm.BUDGET_OUTPUTS[:6]] == list(br.REFERENCE_SIX) and \
        [rt.BUDGET_KINDS[k] for _, k in cm.BUDGET_OUTPUTS[:6]] == list(br.REFERENCE_SIX.values())


class FakeLib:
    """records the attach calls of FluxContext.attach_average"""
    def __init__(self):
        self.calls, self.rc = [], 0

    def cf_attach_average(self, ctx, h, stride, weight):
        self.calls.append(("cf_attach_average", h, stride, weight))
        return self.rc

    def cf_attach_average_slot(self, ctx, slot, h, stride, weight):
        self.calls.append(("cf_attach_average_slot", slot, h, stride, weight))
        return self.rc

    def cf_last_error(self, ctx):
        return b"refused"


def test_attach_average_keeps_the_slots_books():
    ctx = rt.FluxContext.__new__(rt.FluxContext)
    ctx.lib, ctx._h = FakeLib(), None
    a, b = SimpleNamespace(_h=11), SimpleNamespace(_h=22)
    ctx.attach_average(a, 2, 600.0)                    # slot 0 goes through cf_attach_average itself
    ctx.attach_average(b, 3, 1200.0, slot=1)
    assert ctx.lib.calls == [("cf_attach_average", 11, 2, 600.0), ("cf_attach_average_slot", 1, 22, 3, 1200.0)]
    assert ctx._attached_averages == {0: a, 1: b}      # kept alive while attached
    ctx.attach_average(None, slot=1)
    assert ctx.lib.calls[-1][:3] == ("cf_attach_average_slot", 1, None) and ctx._attached_averages == {0: a, 1: None}
    ctx.attach_average(b)                              # replaces slot 0 only
    assert ctx._attached_averages == {0: b, 1: None}
    ctx.lib.rc = -1                                    # a refusal leaves the books as they were
    with pytest.raises(rt.CofluxError):
        ctx.attach_average(a, slot=7)
    assert ctx._attached_averages == {0: b, 1: None}
    ctx._h = None                                      # (nothing to destroy)


class FakeContext:
    """records what SurfaceFluxAverages asks the context for"""
    def __init__(self):
        self.calls = []

    def zeros(self):
        return torch.zeros((NY + 2 * HY, NX + 2 * HX), dtype=torch.float64)

    def average(self, sources, means):
        self.calls.append(("average", sources, means))
        return SimpleNamespace()

    def derived_average(self, terms, cos_rotation=None, sin_rotation=None):
        self.calls.append(("derived_average", terms))
        return SimpleNamespace()

    def budget_average(self, terms, **inputs):
        self.calls.append(("budget_average", terms, inputs))
        return SimpleNamespace()


def fake_model(sea_ice=True):
    ctx = FakeContext()
    z = ctx.zeros
    grid = SimpleNamespace(size=(NX, NY, 1), halo=(HX, HY, 1), longitude=(0.0, 360.0))
    itf = SimpleNamespace(context=ctx, weights=dict(latitude=z()), _grid_rotation=None, net_fluxes=SimpleNamespace(_ocean_fields={}),
                          atmosphere_ocean_interface=SimpleNamespace(_fields=dict(sensible_heat=z(), latent_heat=z(), water_vapor=z(), temperature=z())),
                          exchange=cm.ExchangeStates(ctx, dict(Qs=z(), Ql=z(), Mp=z())), land_freshwater=z())
    itf.exchange_atmosphere_state = itf.exchange.stable
    ice = SimpleNamespace(fields=lambda: dict(concentration=conc, interface_heat=qio, x_stress=tx), frazil_heat=z()) if sea_ice else None
    conc, qio, tx = z(), z(), z()
    ocean = SimpleNamespace(grid=grid, surface_state=lambda: dict(T=z(), S=z(), u=z(), v=z(), mask=None))
    return SimpleNamespace(interfaces=itf, ocean=ocean, sea_ice=ice), ctx


def test_surface_flux_averages_groups_budget_terms_after_the_others():
    model, ctx = fake_model()
    a = ctx.zeros()
    outputs = dict(x=a, **cm.omip_budget_outputs(model), xx=cm.Squared(a), big=cm.BudgetTerm("heat_net", cm.RHO_OCEAN * cm.CP_OCEAN),
                   again=cm.BudgetTerm(abi.BUDGET_SALT_NET))
    assert list(cm.omip_budget_outputs(model))[:6] == ["JTao", "JTio", "JTf", "JTn", "JSn", "JSio"] and len(cm.omip_budget_outputs(model)) == 15
    w = cm.SurfaceFluxAverages(model, outputs=outputs)
    assert [c[0] for c in ctx.calls] == ["derived_average", "budget_average", "budget_average"] and len(w.averagers) == 3
    assert [t[5] is w.means[n] for t, n in zip(ctx.calls[0][1], ("x", "xx"))] == [True, True]
    first, second = ctx.calls[1][1], ctx.calls[2][1]
    assert len(first) == 16 and len(second) == 1                     # fifteen of the preset and `big`; `again` alone
    assert [t[0] for t in first[:6]] == list(br.REFERENCE_SIX.values()) and all(t[1] == 1.0 for t in first[:15])
    assert first[15][:2] == (abi.BUDGET_HEAT_NET, cm.RHO_OCEAN * cm.CP_OCEAN) and first[15][2] is w.means["big"]
    assert second[0][0] == abi.BUDGET_SALT_NET and second[0][2] is w.means["again"]
    inputs = ctx.calls[1][2]
    assert set(inputs) == {"ocean", "atmos", "fluxes", "weights", "ice", "frazil_heat", "land_freshwater"}
    assert set(inputs["ice"]) == {"concentration", "interface_heat"}                 # the stresses are no input
    # the exchange fields are the writer's own three, filled from the current set before a collection
    assert inputs["atmos"] is w._budget_atmos and set(w._budget_atmos) == {"Qs", "Ql", "Mp"}
    live = model.interfaces.exchange.stable
    live["Qs"] += 3.0
    w.stage_exchange(live)
    assert torch.equal(w._budget_atmos["Qs"], live["Qs"]) and w._budget_atmos["Qs"].data_ptr() != live["Qs"].data_ptr()
    # budget outputs alone: no other averager; none: no budget averager, no staging
    model, ctx = fake_model(sea_ice=False)
    w = cm.SurfaceFluxAverages(model, outputs=dict(JTn=cm.BudgetTerm("heat_net")))
    assert [c[0] for c in ctx.calls] == ["budget_average"] and "ice" not in ctx.calls[0][2] and w.averager is w.averagers[0]
    model, ctx = fake_model()
    w = cm.SurfaceFluxAverages(model, outputs=dict(x=a))
    assert [c[0] for c in ctx.calls] == ["average"] and w._budget_atmos is None
    with pytest.raises(ValueError):
        cm.BudgetTerm(15)
    with pytest.raises(KeyError):
        cm.BudgetTerm("heat")
