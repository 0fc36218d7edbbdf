"""GPU tests of the budget averager (include/coflux.h: cf_average_create_budget; coflux_budget.hip) and of the attach slots
(cf_attach_average_slot).  Every case is held to tests/budget_reference.py bit for bit on the designed case of that module:
67 × 5 interior with halos (3, 2) — rows that are no multiple of the wave, a partial second workgroup — with land, open
water, ℵ = 1, 0 < ℵ < 1, the three salinity-floor cells, a supercooled frazil cell and a cell with Qs = 0 in the first wave;
and 1 × 1.  Inputs carry NaN in their halos, means start as NaN everywhere and their halos are checked untouched.

The latitude-dependent albedo is compared with the restatement at latitudes 0, ±90 and 180 only, where cos(2φ) = ±1 in any
faithful cosine: the restatement uses NumPy's cosine, the device its own, and away from such points the two may differ in the
last bit.  At general latitudes the albedo's bits are held to the net-flux kernel's instead (test 2), device against device."""
import ctypes as C

import numpy as np
import pytest
import torch

import budget_reference as br
import coupled_case as cc
from coflux import abi
from coflux import interface_computations as ic
from coflux import models as cm
from coflux import runtime as rt
from coflux.runtime import EXCHANGE_NAMES, FLUX_NAMES, NET_NAMES, FluxContext
from derived_reference import recurrence
from test_coupled_steps import Outputs, Rig, _model_fields, coupled, host_case, replay
from test_coupled_steps import _model as _coupled_model
from test_derived_average import Recorder, bits, raw
from test_steps import H as STEPS_H
from test_steps import INC, _setup
from test_time_average import _model

pytestmark = pytest.mark.gpu

NX, NY, HX, HY = 67, 5, 3, 2
INVALID = -1
ALL = tuple(range(15))
SIX = tuple(br.REFERENCE_SIX.values())
SCALES = (1.0, -1.0, cm.RHO_OCEAN * cm.CP_OCEAN, 0.5, 1026.0, 1.0, 1.0, 1.0, 3.0, 1.0, -2.5, 1.0, 1.0, 1e3, 1.0)
EXACT_LATITUDES = np.array([0.0, 90.0, -90.0, 180.0, 0.0, -90.0, 90.0])


def params(penetrating=False, latitude_dependent=False, mask_kind=abi.MASK_U8):
    surface = ic.SurfaceRadiationProperties(ic.LatitudeDependentAlbedo() if latitude_dependent else 0.06, 0.97)
    return ic.flux_params(ocean_surface=surface, ocean_minimum_salinity=br.S_MIN, penetrating_shortwave=penetrating, mask_kind=mask_kind)


class Inputs:
    """The designed case on the device: every input in the halo layout with NaN halos; `null` names inputs left out (the
    library's NULL pointers), `poison` names inputs that are passed but hold NaN everywhere."""

    def __init__(self, ctx, g, I, *, mask_kind=abi.MASK_U8, latitude=None, separable=True, null=(), poison=()):
        nx, ny, hx, hy = g
        self.g, self.I = g, dict(I)

        def dev(name):
            if name in null:
                self.I[name] = None
                return None
            a = br.halo_layout(I[name], hx, hy)
            if name in poison:
                a[:] = np.nan
            return ctx.to_device(a)
        mask = None
        if mask_kind == abi.MASK_U8:
            mask = ctx.to_device(br.halo_layout(I["wet"].astype(np.uint8), hx, hy, 0))
        elif mask_kind == abi.MASK_BOTTOM_HEIGHT:
            mask = ctx.to_device(br.halo_layout(np.where(I["wet"], -1000.0, 10.0), hx, hy))
        else:
            self.I["wet"] = np.ones_like(I["wet"])
        self.ocean = dict(S=dev("S"), mask=mask)
        self.atmos = dict(Qs=dev("Qs"), Ql=dev("Ql"), Mp=dev("Mp"))
        self.fluxes = dict(sensible_heat=dev("Qc"), latent_heat=dev("Qv"), water_vapor=dev("Mv"), temperature=dev("temperature"))
        self.ice = dict(concentration=dev("aice"), interface_heat=dev("Qio"), salt_flux=dev("Jsio"))
        self.frazil, self.land = dev("frazil"), dev("land")
        self.weights = None
        cells = np.zeros((ny, nx))
        if latitude is not None:
            rows = np.resize(latitude, ny)
            if separable:
                cells = np.repeat(rows[:, None], nx, axis=1)
                lat = np.full(ny + 2 * hy, np.nan)
                lat[hy:hy + ny] = rows
            else:
                cells = np.resize(latitude, nx * ny + 1)[1:].reshape(ny, nx)      # varies along a row as well
                lat = br.halo_layout(cells, hx, hy)
            self.weights = dict(separable=separable, latitude=ctx.to_device(lat))
        self.I["alb"] = br.albedo_of(ctx.params, cells)

    def keywords(self):
        drop = lambda d: {k: v for k, v in d.items() if v is not None} or None  # noqa: E731
        return dict(ocean=drop(self.ocean), atmos=drop(self.atmos), fluxes=drop(self.fluxes), ice=drop(self.ice),
                    frazil_heat=self.frazil, land_freshwater=self.land, weights=self.weights)


def nan_means(ctx, n):
    return [torch.full(ctx.shape, float("nan"), dtype=torch.float64, device="cuda") for _ in range(n)]


def check_means(means, want, g, what):
    nx, ny, hx, hy = g
    out = []
    for t, (m, w) in enumerate(zip(means, want)):
        got = m.cpu().numpy()
        np.testing.assert_array_equal(bits(got[hy:hy + ny, hx:hx + nx]), bits(w), err_msg=f"{what}: term {t}")
        halo = np.ones(got.shape, bool)
        halo[hy:hy + ny, hx:hx + nx] = False
        assert np.isnan(got[halo]).all(), f"{what}: term {t}: a halo cell of the mean was written"
        out.append(got[hy:hy + ny, hx:hx + nx].copy())
    return out


def run_budget(g=(NX, NY, HX, HY), kinds=ALL, scales=SCALES, *, penetrating=False, mask_kind=abi.MASK_U8, latitude=None, separable=True,
               null=(), weights=(1.0,), max_workgroups=0):
    """one averager of `kinds` on the designed case, collected len(weights) times on fresh backgrounds; checks the means
    against the restatement's recurrence and returns their interiors"""
    nx, ny, hx, hy = g
    P = params(penetrating, latitude is not None, mask_kind)
    ctx = FluxContext(nx, ny, hx, hy, P, ring=0)
    model = br.BudgetModel(P)
    means = nan_means(ctx, len(kinds))
    terms = [(k, scales[k], m) for k, m in zip(kinds, means)]
    samples = [[] for _ in kinds]
    first = Inputs(ctx, g, br.designed_case(nx, ny, 0), mask_kind=mask_kind, latitude=latitude, separable=separable, null=null)
    avg = ctx.budget_average(terms, max_workgroups=max_workgroups, **first.keywords())
    for c, w in enumerate(weights):
        fresh = first if c == 0 else Inputs(ctx, g, br.designed_case(nx, ny, c), mask_kind=mask_kind, latitude=latitude, separable=separable, null=null)
        if c:   # new values into the arrays the averager borrowed
            for a, b in zip(_tensors(first), _tensors(fresh)):
                a.copy_(b)
        avg.collect(w)
        ctx.sync()
        for t, k in enumerate(kinds):
            samples[t].append((model.sample(k, fresh.I, scales[k]), w))
    assert avg.weight() == (float(sum(weights)), len(weights))
    out = check_means(means, [recurrence(s) for s in samples], g, f"{g} kinds {kinds}")
    avg.close()
    ctx.close()
    return out


def _tensors(inputs):
    groups = (inputs.ocean, inputs.atmos, inputs.fluxes, inputs.ice, dict(frazil=inputs.frazil, land=inputs.land))
    return [t for d in groups for t in d.values() if t is not None]


# ---- 1. every kind against the restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("penetrating", [False, True], ids=["absorbed", "penetrating"])
@pytest.mark.parametrize("mask_kind", [abi.MASK_U8, abi.MASK_BOTTOM_HEIGHT], ids=["u8", "bottom_height"])
@pytest.mark.parametrize("albedo", ["constant", "latitude_rows", "latitude_cells"])
def test_every_kind_bit_for_bit(albedo, mask_kind, penetrating):
    lat = dict(constant=dict(), latitude_rows=dict(latitude=EXACT_LATITUDES), latitude_cells=dict(latitude=EXACT_LATITUDES, separable=False))[albedo]
    run_budget(penetrating=penetrating, mask_kind=mask_kind, **lat)
    run_budget((1, 1, HX, HY), penetrating=penetrating, mask_kind=mask_kind, **lat)


def test_every_kind_without_ice_land_and_frazil_and_without_a_mask():
    run_budget(null=("aice", "Qio", "Jsio", "land", "frazil"))
    run_budget(null=("aice", "Qio", "Jsio", "land", "frazil"), mask_kind=abi.MASK_NONE)


# ---- 2. the whole kinds against the library's own net fluxes ------------------------------------------------------------------
@pytest.mark.parametrize("penetrating", [False, True], ids=["absorbed", "penetrating"])
@pytest.mark.parametrize("separable", [True, False], ids=["rows", "cells"])
def test_whole_kinds_are_the_net_flux_kernels_bits(separable, penetrating):
    """general latitudes: the albedo's cosine is the device's in both kernels"""
    g = (NX, NY, HX, HY)
    P = params(penetrating, True)
    ctx = FluxContext(NX, NY, HX, HY, P, ring=0)
    inp = Inputs(ctx, g, br.designed_case(), latitude=np.linspace(-77.3, 81.9, 11), separable=separable)
    zero = ctx.zeros
    ocean = dict(T=zero(), S=inp.ocean["S"], u=zero(), v=zero(), mask=inp.ocean["mask"])
    atmos = dict({k: zero() for k in EXCHANGE_NAMES}, **inp.atmos)
    fluxes = dict({k: zero() for k in FLUX_NAMES}, **inp.fluxes)
    net = ctx.field_set(NET_NAMES)
    ctx.set_land_freshwater(inp.land)
    ctx.compute_net_ocean_fluxes(ocean, atmos, fluxes, net, ice=dict(inp.ice, x_stress=zero(), y_stress=zero()), weights=inp.weights)
    means = nan_means(ctx, 3)
    avg = ctx.budget_average([(abi.BUDGET_HEAT_NET, 1.0, means[0]), ("salt_net", 1.0, means[1]), ("heat_shortwave", 1.0, means[2])],
                             **inp.keywords())
    avg.collect(1.0)
    ctx.sync()
    inner = (slice(HY, HY + NY), slice(HX, HX + NX))
    for m, name in zip(means, ("T", "S", "shortwave_surface_flux")):
        got, want = m.cpu().numpy()[inner], net[name].cpu().numpy()[inner]
        np.testing.assert_array_equal(raw(got), raw(want), err_msg=name)
        assert np.count_nonzero(want) > NX * NY // 2
    ctx.close()


def test_whole_kinds_after_an_update_state_on_the_fused_lean_path():
    ctx, states, src, w, np_states = _setup(90, 40)
    assert ctx.solver_path()[0] and ctx.solver_path()[1] >= 1
    ice = {k: ctx.to_device(np_states[0]["ice_" + k]) for k in ("concentration", "interface_heat", "salt_flux", "x_stress", "y_stress")}
    atmos, fl, net = ctx.field_set(EXCHANGE_NAMES), ctx.field_set(FLUX_NAMES), ctx.field_set(NET_NAMES)
    ctx.update_state(src, w, states[0], atmos, fl, net, ice=ice, time_fraction=0.37)
    means = nan_means(ctx, 3)
    avg = ctx.budget_average([("heat_net", 1.0, means[0]), ("salt_net", 1.0, means[1]), ("heat_shortwave", 1.0, means[2])],
                             ocean=states[0], atmos=atmos, fluxes=fl, ice=ice, weights=w)
    avg.collect(1.0)
    ctx.sync()
    inner = (slice(STEPS_H, STEPS_H + 40), slice(STEPS_H, STEPS_H + 90))
    for m, name in zip(means, ("T", "S", "shortwave_surface_flux")):
        want = net[name].cpu().numpy()[inner]
        np.testing.assert_array_equal(raw(m.cpu().numpy()[inner]), raw(want), err_msg=name)
        assert np.count_nonzero(want) > 90 * 40 // 2
    ctx.close()


# ---- 3. the recurrence; company, launched grid and halo widths do not reach the bits --------------------------------------------
def test_three_collections_and_the_bits_do_not_depend_on_company_grid_or_halos():
    W = (1.0, 2.5, 0.25)
    probe = br.HEAT_NET
    all15 = run_budget(weights=W)
    alone = run_budget(kinds=(probe,), weights=W)[0]
    six = run_budget(kinds=SIX, weights=W)
    np.testing.assert_array_equal(raw(alone), raw(all15[probe]))
    for k, m in zip(SIX, six):
        np.testing.assert_array_equal(raw(m), raw(all15[k]), err_msg=br.KIND_NAMES[k])
    one_workgroup = run_budget(weights=W, max_workgroups=1)        # 335 cells: two trips of the stride loop, the second partial
    narrow = run_budget((NX, NY, 1, 1), weights=W)
    for k in ALL:
        np.testing.assert_array_equal(raw(one_workgroup[k]), raw(all15[k]), err_msg=br.KIND_NAMES[k])
        np.testing.assert_array_equal(raw(narrow[k]), raw(all15[k]), err_msg=br.KIND_NAMES[k])


# ---- 4. footprint -----------------------------------------------------------------------------------------------------------
def test_an_averager_of_jtio_and_jsio_reads_nothing_else():
    g = (NX, NY, HX, HY)
    kinds = (br.HEAT_ICE_OCEAN, br.SALT_ICE_OCEAN)
    ctx = FluxContext(NX, NY, HX, HY, params(), ring=0)
    model = br.BudgetModel(ctx.params)
    I = br.designed_case()
    want = [model.sample(k, br.only(I, kinds)) for k in kinds]
    # every other input NULL — the bundles too
    inp = Inputs(ctx, g, I)
    means = nan_means(ctx, 2)
    avg = ctx.budget_average([(k, 1.0, m) for k, m in zip(kinds, means)], ocean=dict(mask=inp.ocean["mask"]),
                             ice=dict(interface_heat=inp.ice["interface_heat"], salt_flux=inp.ice["salt_flux"]))
    avg.collect(1.0)
    ctx.sync()
    lean = check_means(means, want, g, "NULL inputs")
    # the same with NaN-poisoned arrays in every slot the kinds do not read
    unused = [n for n in br.INPUT_NAMES if n not in ("Qio", "Jsio")]
    poisoned = Inputs(ctx, g, I, poison=unused, latitude=EXACT_LATITUDES)
    means = nan_means(ctx, 2)
    avg2 = ctx.budget_average([(k, 1.0, m) for k, m in zip(kinds, means)], **poisoned.keywords())
    avg2.collect(1.0)
    ctx.sync()
    full = check_means(means, want, g, "poisoned inputs")
    for a, b in zip(lean, full):
        np.testing.assert_array_equal(raw(a), raw(b))
    ctx.close()


# ---- 5. attach slots ---------------------------------------------------------------------------------------------------------
def _budget_on(ctx, ocean, atmos, fl, ice, w, kinds=SIX, **more):
    means = nan_means(ctx, len(kinds))
    return ctx.budget_average([(k, SCALES[k], m) for k, m in zip(kinds, means)], ocean=ocean, atmos=atmos, fluxes=fl, ice=ice, weights=w, **more), means


def test_time_steps_collects_two_slots_with_their_own_strides():
    n, step_weight = 6, 1200.0
    ctx, states, src, w, np_states = _setup(90, 40)
    ice = {k: ctx.to_device(np_states[0]["ice_" + k]) for k in ("concentration", "interface_heat", "salt_flux", "x_stress", "y_stress")}
    # the host loop: cf_update_state + cf_average_collect after the same steps
    atmos, rfl, rnet = ctx.field_set(EXCHANGE_NAMES), ctx.field_set(FLUX_NAMES), ctx.field_set(NET_NAMES)
    rplain_means = nan_means(ctx, 2)
    rplain = ctx.average([rnet["T"], rnet["S"]], rplain_means)
    rbudget, rbudget_means = _budget_on(ctx, states[0], atmos, rfl, ice, w)
    for s in range(n):
        tot = s * INC
        l1 = int(tot) % 4
        ctx.update_state(src, w, states[s % 2], atmos, rfl, rnet, ice=ice, level1=l1, level2=(l1 + 1) % 4, time_fraction=tot - int(tot))
        if (s + 1) % 2 == 0:
            rplain.collect(2 * step_weight)
        if (s + 1) % 3 == 0:
            rbudget.collect(3 * step_weight)
    ctx.sync()
    sets = [ctx.field_set(EXCHANGE_NAMES)]
    fl, net = ctx.field_set(FLUX_NAMES), ctx.field_set(NET_NAMES)
    sched = ctx.make_schedule(states, sets, first_level=0, time_fraction=0.0, time_fraction_increment=INC)
    plain_means = nan_means(ctx, 2)
    plain = ctx.average([net["T"], net["S"]], plain_means)
    budget, budget_means = _budget_on(ctx, states[0], sets[0], fl, ice, w)
    ctx.attach_average(plain, 2, step_weight)
    ctx.attach_average(budget, 3, step_weight, slot=1)
    for first, count in ((0, 4), (4, n - 4)):
        ctx.time_steps(first, count, sched, src, w, fl, net, ice=ice)
    ctx.sync()
    assert plain.weight() == rplain.weight() == (n * step_weight, 3) and budget.weight() == rbudget.weight() == (n * step_weight, 2)
    for k, (m, r) in enumerate(zip(plain_means + budget_means, rplain_means + rbudget_means)):
        np.testing.assert_array_equal(raw(m.cpu().numpy()), raw(r.cpu().numpy()), err_msg=f"mean {k}")
    assert np.isfinite(budget_means[0].cpu().numpy()[STEPS_H:-STEPS_H, STEPS_H:-STEPS_H]).all()
    # cf_attach_average replaces slot 0 only: slot 1 goes on collecting, the old slot-0 averager stops
    other_means = nan_means(ctx, 1)
    other = ctx.average([net["u"]], other_means)
    ctx.attach_average(other, 1, step_weight)
    ctx.time_steps(n, 3, sched, src, w, fl, net, ice=ice)
    ctx.sync()
    assert plain.weight() == (n * step_weight, 3) and other.weight() == (3 * step_weight, 3) and budget.weight() == ((n + 3) * step_weight, 3)
    # the same averager in two slots is refused; so is a slot that does not exist
    for bad in (lambda: ctx.attach_average(other, slot=2), lambda: ctx.attach_average(budget, slot=abi.ATTACHED_AVERAGES_MAX),
                lambda: ctx.attach_average(budget, slot=-1)):
        with pytest.raises(rt.CofluxError):
            bad()
    # destroying an attached averager empties its slot: the loop runs on and the slot can be taken again
    budget.close()
    ctx.time_steps(n + 3, 1, sched, src, w, fl, net, ice=ice)
    ctx.attach_average(plain, 1, step_weight, slot=1)
    ctx.time_steps(n + 4, 1, sched, src, w, fl, net, ice=ice)
    ctx.sync()
    assert plain.weight() == ((n + 1) * step_weight, 4) and other.weight() == (5 * step_weight, 5)
    ctx.close()


class BudgetCollectors:
    """an ordinary averager in slot 0 (stride 2) and a budget averager in slot 1 (stride 3) on one Outputs of the coupled case"""
    STEP = 1200.0

    def __init__(self, rig, out):
        ctx = rig.ctx
        self.plain_means = nan_means(ctx, 2)
        self.plain = ctx.average([out.net["T"], out.net_ice["bottom_heat"]], self.plain_means)
        ice = dict(concentration=rig.ice_states[0]["concentration"], interface_heat=out.iof["interface_heat"], salt_flux=out.iof["salt_flux"])
        self.budget, self.budget_means = _budget_on(ctx, rig.oceans[0], out.sets[0], out.fl, ice, rig.w, kinds=ALL,
                                                    frazil_heat=out.iof["frazil_heat"], land_freshwater=out.land)

    def attach(self, ctx):
        ctx.attach_average(self.plain, 2, self.STEP)
        ctx.attach_average(self.budget, 3, self.STEP, slot=1)

    def collect(self, step):
        if (step + 1) % 2 == 0:
            self.plain.collect(2 * self.STEP)
        if (step + 1) % 3 == 0:
            self.budget.collect(3 * self.STEP)


def test_time_steps_coupled_collects_two_slots_like_the_host_loop():
    rig = Rig(host_case(70, 23, 3, 2))
    ctx = rig.ctx
    try:
        want_out, got_out = Outputs(rig), Outputs(rig)
        by_hand, attached = BudgetCollectors(rig, want_out), BudgetCollectors(rig, got_out)
        replay(rig, want_out, 0, cc.N_STEPS, pipeline=abi.PIPELINE_WITHIN_CALL, collectors=by_hand)
        attached.attach(ctx)
        coupled(rig, got_out, [(0, cc.N_STEPS, abi.PIPELINE_WITHIN_CALL)])
        ctx.attach_average(None)
        ctx.attach_average(None, slot=1)
        assert attached.plain.weight() == by_hand.plain.weight() == (cc.N_STEPS * 1200.0, cc.N_STEPS // 2)
        assert attached.budget.weight() == by_hand.budget.weight() == (cc.N_STEPS * 1200.0, cc.N_STEPS // 3)
        for k, (a, b) in enumerate(zip(attached.plain_means + attached.budget_means, by_hand.plain_means + by_hand.budget_means)):
            np.testing.assert_array_equal(raw(a.cpu().numpy()), raw(b.cpu().numpy()), err_msg=f"mean {k}")
        frazil = attached.budget_means[br.HEAT_FRAZIL].cpu().numpy()[2:-2, 3:-3]
        assert np.isfinite(frazil).all() and np.count_nonzero(frazil) > 0
    finally:
        rig.close()


# ---- 6. errors: CF_ERR_INVALID, cf_last_error set, nothing launched ------------------------------------------------------------
def test_every_invalid_descriptor_is_refused_and_launches_nothing():
    g = (40, 12, 2, 2)
    ctx = FluxContext(*g, params(), ring=0)
    lat_ctx = FluxContext(*g, params(latitude_dependent=True), ring=0)
    n = ctx.shape[0] * ctx.shape[1]
    means = nan_means(ctx, 17)
    P = lambda t: t.data_ptr()  # noqa: E731
    T = abi.BudgetTerm
    f = {k: ctx.zeros() + 1.0 for k in ("S", "Qs", "Ql", "Mp", "Qc", "Qv", "Mv", "Ts", "ice", "Qio", "Jsio", "land", "frazil")}

    def bundles(**without):
        o = abi.OceanSurface(S=P(f["S"]))
        e = abi.ExchangeFields(Qs=P(f["Qs"]), Ql=P(f["Ql"]), Mp=P(f["Mp"]))
        fl = abi.InterfaceFluxes(sensible_heat=P(f["Qc"]), latent_heat=P(f["Qv"]), water_vapor=P(f["Mv"]), temperature=P(f["Ts"]))
        i = abi.SeaIceFields(concentration=P(f["ice"]), interface_heat=P(f["Qio"]), salt_flux=P(f["Jsio"]))
        for struct, name in without.get("null", ()):
            setattr(dict(ocean=o, exchange=e, fluxes=fl, ice=i)[struct], name, None)
        return o, e, fl, i

    def refused(terms, match, *, n_terms=None, struct_size=None, context=ctx, weights=None, null=(), no_bundle=(), max_workgroups=0, reserved=0):
        table = (T * max(len(terms), 1))(*terms)
        o, e, fl, i = bundles(null=null)
        ref = lambda name, s: None if name in no_bundle else C.pointer(s)  # noqa: E731
        desc = abi.BudgetDesc(C.sizeof(abi.BudgetDesc) if struct_size is None else struct_size, len(terms) if n_terms is None else n_terms,
                              table, ref("ocean", o), ref("exchange", e), ref("fluxes", fl), ref("ice", i), P(f["frazil"]), P(f["land"]),
                              C.pointer(weights) if weights is not None else None, max_workgroups, reserved)
        h = C.c_void_p()
        rc = context.lib.cf_average_create_budget(context._h, C.byref(desc), C.byref(h))
        assert rc == INVALID and not h.value, match
        assert match in context.lib.cf_last_error(context._h).decode(), (match, context.lib.cf_last_error(context._h).decode())

    good = T(abi.BUDGET_HEAT_NET, 0, 1.0, P(means[0]))
    refused([good], "struct_size", struct_size=C.sizeof(abi.BudgetDesc) + 8)
    refused([good], "0 terms", n_terms=0)
    refused([good] * 2, "17 terms", n_terms=17)
    refused([good], "max_workgroups", max_workgroups=-1)
    refused([good], "max_workgroups", reserved=1)
    refused([T(15, 0, 1.0, P(means[0]))], "unknown kind")
    refused([T(-1, 0, 1.0, P(means[0]))], "unknown kind")
    refused([T(abi.BUDGET_HEAT_NET, 1, 1.0, P(means[0]))], "unknown kind")          # a term's reserved word
    refused([T(abi.BUDGET_HEAT_NET, 0, 1.0, None)], "NULL mean")
    for scale in (float("nan"), float("inf"), -float("inf")):
        refused([T(abi.BUDGET_HEAT_NET, 0, scale, P(means[0]))], "scale")
    # a NULL required input of a requested kind: every (kind, input) of the table's "reads" column that is not optional
    required = {"S": ("ocean", "S"), "temperature": ("fluxes", "temperature"), "Mp": ("exchange", "Mp"), "Qs": ("exchange", "Qs"),
                "Ql": ("exchange", "Ql"), "Qc": ("fluxes", "sensible_heat"), "Qv": ("fluxes", "latent_heat"), "Mv": ("fluxes", "water_vapor")}
    for kind in ALL:
        for name in sorted(br.READS[kind] & set(required)):
            refused([T(kind, 0, 1.0, P(means[0]))], "which is NULL", null=[required[name]])
        for struct in sorted({required[name][0] for name in br.READS[kind] & set(required)}):
            refused([T(kind, 0, 1.0, P(means[0]))], "which is NULL", no_bundle=(struct,))
    # a mean over an input, over another mean (by one element of its parent array)
    refused([T(abi.BUDGET_HEAT_NET, 0, 1.0, P(f["Qs"]))], "overlaps")
    refused([T(abi.BUDGET_HEAT_ICE_OCEAN, 0, 1.0, P(f["Qio"]) + 8 * (n - 1))], "overlaps")
    buf = torch.zeros(2 * n, dtype=torch.float64, device="cuda")
    refused([T(abi.BUDGET_HEAT_NET, 0, 1.0, buf.data_ptr()), T(abi.BUDGET_SALT_NET, 0, 1.0, buf.data_ptr() + 8 * (n - 1))], "overlap")
    # the latitude-dependent albedo without a latitude array: no weights, or weights without it — only for kinds that read the albedo
    for kind in (abi.BUDGET_HEAT_SHORTWAVE, abi.BUDGET_HEAT_ATMOSPHERE_OCEAN, abi.BUDGET_HEAT_NET):
        refused([T(kind, 0, 1.0, P(means[0]))], "latitude", context=lat_ctx)
        refused([T(kind, 0, 1.0, P(means[0]))], "latitude", context=lat_ctx, weights=abi.InterpWeights(separable=1))
    assert ctx.lib.cf_average_create_budget(ctx._h, None, C.byref(C.c_void_p())) == INVALID
    assert ctx.lib.cf_average_create_budget(None, None, None) == INVALID
    ctx.sync()
    lat_ctx.sync()
    assert all(torch.isnan(m).all().item() for m in means), "a refused descriptor launched"
    # a kind that does not read the albedo needs no latitude; and one made before the albedo became latitude-dependent is
    # refused at the collection, launching nothing
    o, e, fl, i = bundles()
    for context, kind, collects in ((lat_ctx, abi.BUDGET_HEAT_SENSIBLE, True), (ctx, abi.BUDGET_HEAT_NET, False)):
        desc = abi.BudgetDesc(C.sizeof(abi.BudgetDesc), 1, (T * 1)(T(kind, 0, 1.0, P(means[1]))), C.pointer(o), C.pointer(e), C.pointer(fl),
                              C.pointer(i), None, None, None, 0, 0)
        h = C.c_void_p()
        assert context.lib.cf_average_create_budget(context._h, C.byref(desc), C.byref(h)) == 0 and h.value
        if not collects:
            context.set_flux_params(params(latitude_dependent=True))
        assert (context.lib.cf_average_collect(h, 1.0) == 0) == collects
        context.sync()
        assert torch.isnan(means[1][0, 0]).item() and torch.isnan(means[1][2:-2, 2:-2]).any().item() != collects
        assert context.lib.cf_average_destroy(h) == 0
        means[1].fill_(float("nan"))
    ctx.close()
    lat_ctx.close()


# ---- 7. model level ----------------------------------------------------------------------------------------------------------
def test_simulation_with_omip_budget_outputs_matches_the_restatement():
    model = _model(True)
    NX_, NY_, H, DT = 90, 40, 3, 20 * cm.minutes
    itf, si = model.interfaces, model.sea_ice
    outputs = cm.omip_budget_outputs(model)
    assert list(outputs)[:6] == ["JTao", "JTio", "JTf", "JTn", "JSn", "JSio"]
    outputs["hfds_watts"] = cm.BudgetTerm("heat_net", cm.RHO_OCEAN * cm.CP_OCEAN)
    outputs["hfds"] = itf.net_fluxes.ocean.T                      # an ordinary field beside them: two averagers
    ao, st = itf.atmosphere_ocean_interface._fields, model.ocean.surface_state()

    class ExchangeRecorder(Recorder):
        """the step's own exchange state: run! alternates between two sets"""
        def write(self, clock):
            live = itf.exchange_atmosphere_state
            self.steps.append(dict({k: v.cpu().numpy().copy() for k, v in self.fields.items()},
                                   **{k: live[k].cpu().numpy().copy() for k in ("Qs", "Ql", "Mp")}))

    recorder = ExchangeRecorder(dict(S=st["S"], temperature=ao["temperature"], Qc=ao["sensible_heat"], Qv=ao["latent_heat"], Mv=ao["water_vapor"],
                                     aice=si.concentration, Qio=si.interface_heat, Jsio=si.salt_flux, T=itf.net_fluxes.ocean.T))
    writer = cm.SurfaceFluxAverages(model, outputs=outputs, schedule=cm.AveragedTimeInterval(6 * DT))
    assert len(writer.averagers) == 2
    cm.run(cm.Simulation(model, dt=DT, stop_iteration=6, output_writers={"record": recorder, "surface": writer}))
    assert len(writer.windows) == 1 and len(recorder.steps) == 6
    inner = (slice(H, H + NY_), slice(H, H + NX_))
    wet = model.ocean.model.wet_mask.cpu().numpy()[inner] != 0
    ref = br.BudgetModel(itf.context.params)
    samples = {name: [] for name in outputs}
    for step in recorder.steps:
        I = {k: v[inner] for k, v in step.items()}
        I["wet"], I["alb"] = wet, np.full(wet.shape, itf.context.params.ocean_albedo)
        for name, o in outputs.items():
            x = I["T"] if name == "hfds" else ref.sample(o.kind, I, o.scale)
            samples[name].append((x, DT))
    arrays = writer.windows[0][1]
    for name in outputs:
        np.testing.assert_array_equal(bits(arrays[name]), bits(recurrence(samples[name])), err_msg=name)
    # JTn is hfds: the budget's whole is what the step stored, through six collections
    np.testing.assert_array_equal(raw(arrays["JTn"]), raw(arrays["hfds"]))
    assert np.count_nonzero(arrays["JTio"]) > 0 and np.count_nonzero(arrays["heat_shortwave"]) > 0
    itf.context.close()


def test_models_time_steps_attaches_every_averager_of_a_writer():
    """The OMIP surface set with sea ice is two averagers, its budget a third: models.time_steps(…, averages=writer) collects
    all three every step of the device loop (20-minute steps: several cf_time_steps_coupled calls from re-based clocks), as a
    host loop of time_step, NormalizeSalinity and three collections does — and leaves the model's fields as that loop does,
    the exchange fields the writer lent to the loop included."""
    dt, n = 1200.0, 6

    def writer_of(model):
        outputs = dict(cm.omip_surface_outputs(model), **cm.omip_budget_outputs(model))
        return cm.SurfaceFluxAverages(model, outputs=outputs)
    host, host_norm = _coupled_model()
    host_writer = writer_of(host)
    assert len(host_writer.averagers) == 3 and list(host_writer.means)[-15:-9] == ["JTao", "JTio", "JTf", "JTn", "JSn", "JSio"]
    for _ in range(n):
        cm.time_step(host, dt)
        host_norm(host)
        host_writer.stage_exchange(host.interfaces.exchange_atmosphere_state)
        for averager in host_writer.averagers:
            averager.collect(dt)
    host.interfaces.context.sync()
    device, device_norm = _coupled_model()
    device_writer = writer_of(device)
    cm.time_steps(device, dt, n, normalize=device_norm, averages=device_writer)
    device.interfaces.context.sync()
    for a, b in zip(device_writer.averagers, host_writer.averagers):
        assert a.weight() == b.weight() == (n * dt, n)
    for name in host_writer.means:
        got, want = device_writer.means[name].cpu().numpy(), host_writer.means[name].cpu().numpy()
        np.testing.assert_array_equal(raw(got), raw(want), err_msg=name)
    assert np.count_nonzero(device_writer.means["JTf"].cpu().numpy()) > 0
    want, got = _model_fields(host, host_norm), _model_fields(device, device_norm)
    for k in want:
        assert torch.equal(got[k].view(torch.int64), want[k].view(torch.int64)), k
    # the slots are empty again: a further call collects nothing
    cm.time_steps(device, dt, 1, normalize=device_norm)
    assert device_writer.averagers[0].weight() == (n * dt, n)
    host.interfaces.context.close()
    device.interfaces.context.close()
