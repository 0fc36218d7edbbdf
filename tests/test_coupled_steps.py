"""GPU tests of the coupled step on the device (include/coflux.h): cf_prepare_coupled_step — the land freshwater, the ice–ocean
exchange with frazil and the restoring buffer as one launch — against the three entry points it stands for, and
cf_time_steps_coupled — the OMIP configuration's step loop — against a host replay of the existing entry points, on the
designed case of tests/coupled_case.py.  Every output starts sentinel-filled in a guarded buffer, and whole buffers (parent
array, halos and guard space) are compared bit for bit."""
import functools

import numpy as np
import pytest
import torch

import coupled_case as cc
import util
from coflux import abi
from coflux import interface_computations as ic
from coflux.runtime import EXCHANGE_NAMES, FLUX_NAMES, NET_NAMES, CofluxError, FluxContext

pytestmark = pytest.mark.gpu

GUARD = 96
IOF_NAMES = ("interface_heat", "salt_flux", "frazil_heat", "friction_velocity")
AI_NAMES = tuple(k for k in FLUX_NAMES if k != "temperature")
FORMULATIONS = {"corrected_explicit": ("sea_ice_corrected", abi.SKIN_EXPLICIT), "corrected_linearised": ("sea_ice_corrected", abi.SKIN_LINEARISED),
                "ncar": ("sea_ice_ncar", abi.SKIN_EXPLICIT)}


@functools.lru_cache(maxsize=None)
def host_case(nx, ny, hx, hy, weights="latlon"):
    """The designed case, built once per shape and never written to."""
    return cc.build(nx, ny, hx, hy, weights)


def sentinel_field(shape):
    return util.guarded(tuple(shape), torch.float64, offset=1, guard=GUARD, fill=util.SENTINEL64)


def raw_bits(view):
    """The bits of the whole buffer behind a guarded view: the parent array with its halos, and the guard space around it."""
    return util.buffer_of(view)[0].view(torch.int64).clone()


class Rig:
    """One context on the designed case with its inputs on the device."""

    def __init__(self, case, *, formulation="corrected_explicit", mask_kind=abi.MASK_U8, ice_free=abi.ICE_FREE_ITERATE, merged=0,
                 sea_ice=True):
        self.case = case
        nx, ny, hx, hy = case["nx"], case["ny"], case["hx"], case["hy"]
        params = ic.flux_params(ocean_minimum_salinity=cc.MIN_SALINITY, mask_kind=mask_kind)
        self.ctx = ctx = FluxContext(nx, ny, hx, hy, params, ring=1)
        if sea_ice:
            config, skin = FORMULATIONS[formulation]
            fluxes, velocity = util.ICE_CONFIGS[config]()
            ctx.set_sea_ice_formulation(ic.flux_params(fluxes, velocity_difference=velocity, mask_kind=mask_kind),
                                        ic.SeaIceInterfaceProperties(skin_temperature_scheme=skin).to_params())
        ctx.set_option(abi.OPT_ICE_FREE_CELLS, ice_free)
        ctx.set_option(abi.OPT_MERGED_PREFETCH, merged)
        mask = ctx.to_device(case["bottom_height"] if mask_kind == abi.MASK_BOTTOM_HEIGHT else case["oceans"][0]["mask"])
        self.oceans = [dict({k: ctx.to_device(o[k]) for k in ("T", "S", "u", "v")}, mask=mask) for o in case["oceans"]]
        shared = {k: ctx.to_device(case["ice_state"][k]) for k in ("thickness", "u", "v", "albedo")}
        self.ice_states = [dict(shared, concentration=ctx.to_device(c)) for c in case["concentrations"]]
        self.top_temperature = ctx.to_device(case["ice_state"]["top_temperature"])
        self.tx, self.ty = ctx.to_device(case["x_stress"]), ctx.to_device(case["y_stress"])
        w = case["weights"]
        self.w = {k: (ctx.to_device(v) if isinstance(v, np.ndarray) else v) for k, v in w.items()}
        self.src = {k: ctx.to_device(v) for k, v in case["src"].items()}
        self.friver, self.licalvf = ctx.to_device(case["land"]["friver"]), ctx.to_device(case["land"]["licalvf"])
        self.target, self.area = ctx.to_device(case["target"]), ctx.to_device(case["area"])
        self.iop = ctx.default_ice_ocean_params(time_step=cc.ICE_OCEAN_TIME_STEP, top_cell_thickness=10.0)
        self.stresses = dict(x_stress=self.tx, y_stress=self.ty)

    def close(self):
        self.ctx.close()


class Outputs:
    """Every array a coupled step writes, sentinel-filled in guarded buffers; the carried skin temperature starts from the
    sea ice's top temperature (its guard space keeps the sentinel)."""

    def __init__(self, rig):
        shape = rig.ctx.shape
        f = lambda: sentinel_field(shape)  # noqa: E731
        self.sets = [{k: f() for k in EXCHANGE_NAMES} for _ in range(2)]
        self.fl = {k: f() for k in FLUX_NAMES}
        self.net = {k: f() for k in NET_NAMES}
        self.ai = {k: f() for k in AI_NAMES}
        self.skin = f()
        self.skin.copy_(rig.top_temperature)
        self.net_ice = {k: f() for k in ("top_heat", "bottom_heat")}
        self.iof = {k: f() for k in IOF_NAMES}
        self.land, self.restoring = f(), f()
        self.mean = sentinel_field((1,))

    def views(self):
        out = {"skin": self.skin, "land": self.land, "restoring": self.restoring, "mean": self.mean}
        for name, d in (("set0", self.sets[0]), ("set1", self.sets[1]), ("fl", self.fl), ("net", self.net), ("ai", self.ai),
                        ("net_ice", self.net_ice), ("iof", self.iof)):
            out.update({f"{name}.{k}": v for k, v in d.items()})
        return out

    def bits(self):
        return {k: raw_bits(v) for k, v in self.views().items()}


def assert_same_bits(got, want, what):
    assert got.keys() == want.keys()
    for k in want:
        assert torch.equal(got[k], want[k]), f"{what}: {k} differs in {int((got[k] != want[k]).sum())} of {want[k].numel()} words"


class Collectors:
    """An averager (stride 3), an integrator (stride 2) and a monitor (stride 4) on the net fluxes of one Outputs: attached to
    the context's loop, or collected by hand after the steps the loop would collect."""
    AVERAGE_STRIDE, INTEGRALS_STRIDE, MONITOR_STRIDE = 3, 2, 4
    STEP_SECONDS, ORIGIN = 1200.0, 100.0

    def __init__(self, rig, out):
        ctx = rig.ctx
        self.means = [sentinel_field(ctx.shape) for _ in range(3)]
        self.average = ctx.average([out.net["T"], out.net["S"], out.net_ice["bottom_heat"]], self.means)
        mask = rig.oceans[0]["mask"]
        self.integrals = ctx.integrals([("field", out.net["T"]), ("product", out.net["S"], rig.ice_states[0]["concentration"]),
                                        ("above", rig.ice_states[0]["concentration"], None, 0.15), ("field", out.iof["frazil_heat"])],
                                       area=rig.area, mask=mask, capacity=64)
        self.monitor = ctx.monitor([out.net["T"], (out.net["u"], "abs"), out.skin], mask=mask, capacity=64)

    def attach(self, ctx):
        ctx.attach_average(self.average, stride=self.AVERAGE_STRIDE, step_weight=self.STEP_SECONDS)
        ctx.attach_integrals(self.integrals, stride=self.INTEGRALS_STRIDE, time_origin=self.ORIGIN, step_seconds=self.STEP_SECONDS)
        ctx.attach_monitor(self.monitor, stride=self.MONITOR_STRIDE, time_origin=self.ORIGIN, step_seconds=self.STEP_SECONDS)

    @staticmethod
    def detach(ctx):
        ctx.attach_average(None)
        ctx.attach_integrals(None)
        ctx.attach_monitor(None)

    def collect(self, step):
        """What cf_time_steps' rule collects after global step `step`, in its order."""
        if (step + 1) % self.AVERAGE_STRIDE == 0:
            self.average.collect(self.AVERAGE_STRIDE * self.STEP_SECONDS)
        if (step + 1) % self.INTEGRALS_STRIDE == 0:
            self.integrals.collect(self.ORIGIN + (step + 1) * self.STEP_SECONDS)
        if (step + 1) % self.MONITOR_STRIDE == 0:
            self.monitor.collect(self.ORIGIN + (step + 1) * self.STEP_SECONDS)

    def record(self):
        iv, it = self.integrals.read()
        mv, mt = self.monitor.read()
        return dict(means=[raw_bits(m) for m in self.means], weight=self.average.weight(), integrals=iv.view(np.int64).copy(),
                    integral_times=it.copy(), monitor=mv.tobytes(), monitor_times=mt.copy(),
                    counts=(self.integrals.count(), self.monitor.count()))

    def close(self):
        for h in (self.average, self.integrals, self.monitor):
            h.close()


VARIANTS = {"restoring_area": dict(restoring=True, area=True), "bare": dict(restoring=False, area=False)}


def replay(rig, out, first, n, *, pipeline=0, restoring=True, area=True, collectors=None):
    """The host loop of the existing entry points, in the order cf_time_steps_coupled documents; with `pipeline` the same
    requests for the next step's atmosphere state as the loop makes."""
    ctx = rig.ctx
    for s in range(first, first + n):
        o, st = rig.oceans[s % len(rig.oceans)], rig.ice_states[s % len(rig.ice_states)]
        l1, l2, lf = cc.clock_levels(cc.LAND_CLOCK, 1, s)[0]
        ctx.interpolate_land_freshwater(rig.friver, rig.licalvf, rig.w, out.land, level1=l1, level2=l2, time_fraction=lf)
        ctx.set_land_freshwater(out.land)
        ctx.compute_sea_ice_ocean_fluxes(rig.iop, o, st["concentration"], rig.tx, rig.ty, out.iof)
        if restoring:
            ctx.materialize_salinity_restoring(cc.PISTON_VELOCITY, rig.target, o, out.restoring)
        if pipeline and (s + 1 < first + n or pipeline == abi.PIPELINE_CONTINUING):
            n1, n2, nf = cc.clock_levels(cc.ATMOS_CLOCK, 1, s + 1)[0]
            ctx.prefetch_atmosphere_state(rig.src, rig.w, out.sets[(s + 1) % 2], level1=n1, level2=n2, time_fraction=nf)
        a1, a2, af = cc.clock_levels(cc.ATMOS_CLOCK, 1, s)[0]
        partition = dict(rig.stresses, concentration=st["concentration"], interface_heat=out.iof["interface_heat"],
                         salt_flux=out.iof["salt_flux"])
        ctx.update_state_sea_ice(rig.src, rig.w, o, out.sets[s % 2], out.fl, out.net, partition, dict(st, top_temperature=out.skin),
                                 dict(out.ai, temperature=out.skin), out.net_ice, frazil_heat=out.iof["frazil_heat"],
                                 interface_heat=out.iof["interface_heat"], level1=a1, level2=a2, time_fraction=af)
        ctx.normalize_salinity_flux(out.net["S"], o["mask"], additional=out.restoring if restoring else None,
                                    area=rig.area if area else None, mean_out=out.mean)
        if collectors is not None:
            collectors.collect(s)
    ctx.sync()
    ctx.discard_prefetched_atmosphere_state()


def coupled_arguments(rig, out, *, pipeline=0, restoring=True, area=True, normalize=True):
    ctx = rig.ctx
    sch = ctx.make_schedule(rig.oceans, out.sets, first_level=cc.ATMOS_CLOCK["first_level"], time_fraction=cc.ATMOS_CLOCK["fraction"],
                            time_fraction_increment=cc.ATMOS_CLOCK["increment"], pipeline=pipeline)
    block = ctx.make_coupled_step(rig.ice_states, out.skin, out.ai, out.net_ice, friver=rig.friver, licalvf=rig.licalvf, land_out=out.land,
                                  land_first_level=cc.LAND_CLOCK["first_level"], land_time_fraction=cc.LAND_CLOCK["fraction"],
                                  land_time_fraction_increment=cc.LAND_CLOCK["increment"], ice_ocean_params=rig.iop,
                                  ice_ocean_fluxes=out.iof, piston_velocity=cc.PISTON_VELOCITY, target=rig.target,
                                  restoring_out=out.restoring if restoring else None, normalize=normalize,
                                  area=rig.area if area else None, mean_out=out.mean)
    return sch, block


def coupled(rig, out, calls, **kw):
    """cf_time_steps_coupled over `calls` = [(first_step, nsteps, pipeline), …] on one set of outputs."""
    ctx = rig.ctx
    for first, n, pipeline in calls:
        sch, block = coupled_arguments(rig, out, pipeline=pipeline, **kw)
        ctx.time_steps_coupled(first, n, sch, rig.src, rig.w, out.fl, out.net, rig.stresses, block)
    ctx.sync()
    ctx.discard_prefetched_atmosphere_state()


# ---------------------------------------------------------------------------------------------
# 1. the preamble == the three entry points
# ---------------------------------------------------------------------------------------------
PREAMBLE_VARIANTS = {
    "all": {},
    "no_land": dict(land=False),
    "no_ice_ocean": dict(ice=False),
    "no_restoring": dict(restoring=False),
    "no_licalvf": dict(licalvf=False),
    "no_frazil_field": dict(iof=("interface_heat", "salt_flux", "friction_velocity")),
    "no_frazil": dict(time_step=0.0),
    "second_states": dict(ocean=1, ice=2, land_step=11),
}


@pytest.mark.parametrize("weights", ["latlon", "tripolar"])
@pytest.mark.parametrize("mask_kind", [abi.MASK_U8, abi.MASK_BOTTOM_HEIGHT], ids=["u8", "bottom_height"])
@pytest.mark.parametrize("nx, ny, hx, hy", [(70, 23, 3, 2), (64, 2, 2, 2), (131, 37, 4, 3), (257, 5, 2, 3)])
def test_preamble_is_the_three_entry_points_bit_for_bit(nx, ny, hx, hy, mask_kind, weights):
    """cf_prepare_coupled_step leaves in every array it writes — on the whole parent array and the guard space around it — the
    bits cf_interpolate_land_freshwater, cf_compute_sea_ice_ocean_fluxes and cf_materialize_salinity_restoring leave, with each
    job absent in turn, without licalvf, without a frazil field (friction velocity given) and with frazil switched off."""
    rig = Rig(host_case(nx, ny, hx, hy, weights), mask_kind=mask_kind, sea_ice=False)
    ctx = rig.ctx
    try:
        for name, v in PREAMBLE_VARIANTS.items():
            o, st = rig.oceans[v.get("ocean", 0)], rig.ice_states[v.get("ice", 0)]
            l1, l2, lf = cc.clock_levels(cc.LAND_CLOCK, 1, v.get("land_step", 3))[0]
            licalvf = rig.licalvf if v.get("licalvf", True) else None
            iop = ctx.default_ice_ocean_params(time_step=v.get("time_step", cc.ICE_OCEAN_TIME_STEP), top_cell_thickness=10.0)
            three, fused = Outputs(rig), Outputs(rig)
            pick = lambda out: {k: out.iof[k] for k in v.get("iof", IOF_NAMES)}  # noqa: E731
            if v.get("land", True):
                ctx.interpolate_land_freshwater(rig.friver, licalvf, rig.w, three.land, level1=l1, level2=l2, time_fraction=lf)
            if v.get("ice", True):
                ctx.compute_sea_ice_ocean_fluxes(iop, o, st["concentration"], rig.tx, rig.ty, pick(three))
            if v.get("restoring", True):
                ctx.materialize_salinity_restoring(cc.PISTON_VELOCITY, rig.target, o, three.restoring)
            ctx.prepare_coupled_step(o, weights=rig.w, friver=rig.friver, licalvf=licalvf, land_out=fused.land if v.get("land", True) else None,
                                     level1=l1, level2=l2, time_fraction=lf, ice_ocean_params=iop, concentration=st["concentration"],
                                     x_stress=rig.tx, y_stress=rig.ty, ice_ocean_out=pick(fused) if v.get("ice", True) else None,
                                     piston_velocity=cc.PISTON_VELOCITY, target=rig.target,
                                     restoring_out=fused.restoring if v.get("restoring", True) else None)
            ctx.sync()
            assert_same_bits(fused.bits(), three.bits(), name)
            if name == "all":   # … and the case did reach the branches it was designed for
                inner = (slice(hy, hy + ny), slice(hx, hx + nx))
                # (under supercooled water the exchange sees T_o = T_f: its heat flux is zero to rounding, its u★ is not)
                frazil, ustar, heat = (fused.iof[k][inner] for k in ("frazil_heat", "friction_velocity", "interface_heat"))
                assert int((frazil < 0).sum()) >= 16 and int(((frazil < 0) & (ustar > 0)).sum()) >= 8
                assert int(((frazil == 0) & (heat != 0)).sum()) >= 8
                assert int((fused.land[inner] > 0).sum()) >= 8 and int((fused.restoring[inner] != 0).sum()) >= 8
                sentinel = int(np.array([util.SENTINEL64], dtype=np.uint64).view(np.int64)[0])
                for k in ("land", "restoring", "iof.interface_heat"):
                    buf = fused.bits()[k]
                    assert bool((buf[:GUARD] == sentinel).all()) and bool((buf[-GUARD:] == sentinel).all()), k
                outside = torch.ones(ctx.shape, dtype=torch.bool, device="cuda")
                outside[inner] = False
                assert bool((fused.restoring.view(torch.int64)[outside] == sentinel).all())
    finally:
        rig.close()


# ---------------------------------------------------------------------------------------------
# 2. the loop == the host replay
# ---------------------------------------------------------------------------------------------
MODES = {"unpipelined": (0, 0), "pipelined": (abi.PIPELINE_WITHIN_CALL, 0), "pipelined_tail": (abi.PIPELINE_WITHIN_CALL, 2)}


@pytest.mark.parametrize("ice_free", [abi.ICE_FREE_ITERATE, abi.ICE_FREE_ZERO], ids=["iterate", "zero"])
@pytest.mark.parametrize("formulation", sorted(FORMULATIONS))
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("nx, ny, hx, hy", [(131, 37, 4, 3), (192, 48, 4, 4)])
def test_loop_is_the_host_replay_bit_for_bit(nx, ny, hx, hy, mode, formulation, ice_free):
    """cf_time_steps_coupled — 12 steps as one call, 5 + 7 steps (CF_PIPELINE_CONTINUING when pipelined), and a single step —
    leaves the bits of the host loop of the existing entry points in both exchange sets, the interface and net ocean fluxes, the
    sea-ice interface fluxes and the carried skin temperature, top and bottom heat, Q_io, Jˢ_io, Q_frazil, the land field, the
    restoring buffer and the mean; with the normalisation on, with and without the restoring buffer and the areas."""
    pipeline, merged = MODES[mode]
    rig = Rig(host_case(nx, ny, hx, hy), formulation=formulation, ice_free=ice_free, merged=merged)
    try:
        for vname, v in VARIANTS.items():
            want = Outputs(rig)
            replay(rig, want, 0, cc.N_STEPS, pipeline=pipeline, **v)
            got = Outputs(rig)
            coupled(rig, got, [(0, cc.N_STEPS, pipeline)], **v)
            assert_same_bits(got.bits(), want.bits(), f"{vname}: 12 steps")
            if pipeline:
                want = Outputs(rig)
                replay(rig, want, 0, cc.N_STEPS, pipeline=abi.PIPELINE_CONTINUING, **v)
            split = abi.PIPELINE_CONTINUING if pipeline else 0
            got = Outputs(rig)
            coupled(rig, got, [(0, 5, split), (5, 7, split)], **v)
            assert_same_bits(got.bits(), want.bits(), f"{vname}: 5 + 7 steps")
            want, got = Outputs(rig), Outputs(rig)
            replay(rig, want, 0, 1, pipeline=pipeline, **v)
            coupled(rig, got, [(0, 1, pipeline)], **v)
            assert_same_bits(got.bits(), want.bits(), f"{vname}: 1 step")
    finally:
        rig.close()


# ---------------------------------------------------------------------------------------------
# 3. attachments
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("calls", [[(0, 12)], [(0, 5), (5, 7)]], ids=["one_call", "5+7"])
def test_attached_collections_hold_the_replays_bits_and_counts(calls):
    """An averager (stride 3), an integrator (stride 2) and a monitor (stride 4) attached to the coupled loop: the means, the
    records, their stamps and their counts are those of a replay that collects by hand after the same global steps."""
    rig = Rig(host_case(131, 37, 4, 3), merged=2)
    ctx = rig.ctx
    try:
        want_out, got_out = Outputs(rig), Outputs(rig)
        by_hand, attached = Collectors(rig, want_out), Collectors(rig, got_out)
        replay(rig, want_out, 0, cc.N_STEPS, pipeline=abi.PIPELINE_CONTINUING if len(calls) > 1 else abi.PIPELINE_WITHIN_CALL,
               collectors=by_hand)
        attached.attach(ctx)
        coupled(rig, got_out, [(a, n, abi.PIPELINE_CONTINUING if len(calls) > 1 else abi.PIPELINE_WITHIN_CALL) for a, n in calls])
        Collectors.detach(ctx)
        want, got = by_hand.record(), attached.record()
        assert got["counts"] == want["counts"] == (cc.N_STEPS // Collectors.INTEGRALS_STRIDE, cc.N_STEPS // Collectors.MONITOR_STRIDE)
        assert got["weight"] == want["weight"] == (cc.N_STEPS * Collectors.STEP_SECONDS, cc.N_STEPS // Collectors.AVERAGE_STRIDE)
        for a, b in zip(got["means"], want["means"]):
            assert torch.equal(a, b)
        assert np.array_equal(got["integrals"], want["integrals"]) and np.array_equal(got["integral_times"], want["integral_times"])
        assert got["monitor"] == want["monitor"] and np.array_equal(got["monitor_times"], want["monitor_times"])
        assert_same_bits(got_out.bits(), want_out.bits(), "outputs under attachments")
        by_hand.close()
        attached.close()
    finally:
        rig.close()


# ---------------------------------------------------------------------------------------------
# 4. validation
# ---------------------------------------------------------------------------------------------
def _null(struct, name):
    setattr(struct, name, None)


REJECTIONS = {
    "struct_size": lambda sch, block, ice, out, rig: setattr(block, "struct_size", 8),
    "n_ice_states": lambda sch, block, ice, out, rig: setattr(block, "n_ice_states", 0),
    "land_time_fraction": lambda sch, block, ice, out, rig: setattr(block, "land_time_fraction", -0.25),
    "land_first_level": lambda sch, block, ice, out, rig: setattr(block, "land_first_level", cc.LAND_CLOCK["n_levels"]),
    "skin_temperature": lambda sch, block, ice, out, rig: _null(block, "skin_temperature"),
    "ai_fluxes.temperature": lambda sch, block, ice, out, rig: setattr(block.ai_fluxes, "temperature", out.land.data_ptr()),
    "ai_fluxes": lambda sch, block, ice, out, rig: _null(block.ai_fluxes, "sensible_heat"),
    "net_ice": lambda sch, block, ice, out, rig: _null(block.net_ice, "top_heat"),
    "land_freshwater": lambda sch, block, ice, out, rig: _null(block, "land_freshwater"),
    "ice_ocean_fluxes": lambda sch, block, ice, out, rig: _null(block.ice_ocean_fluxes, "salt_flux"),
    "concentration": lambda sch, block, ice, out, rig: ice.update(concentration=rig.ice_states[0]["concentration"]),
    "mean_out": lambda sch, block, ice, out, rig: setattr(block, "mean_out", out.net["S"].data_ptr() + 8 * 17),
    "halo_backend": lambda sch, block, ice, out, rig: (setattr(sch, "halo_backend", abi.HALO_PEER), setattr(sch, "halo_rows", 2)),
}


def test_every_rejection_names_its_field_and_leaves_the_outputs_untouched():
    rig = Rig(host_case(131, 37, 4, 3))
    bare = Rig(host_case(131, 37, 4, 3), sea_ice=False)
    try:
        out = Outputs(rig)
        untouched = out.bits()

        def refused(ctx_rig, field, first=0, n=3, *, block_is_null=False, mutate=None):
            sch, block = coupled_arguments(ctx_rig, out, pipeline=abi.PIPELINE_WITHIN_CALL)
            ice = dict(ctx_rig.stresses)
            if mutate is not None:
                mutate(sch, block, ice, out, ctx_rig)
            with pytest.raises(CofluxError) as err:
                ctx_rig.ctx.time_steps_coupled(first, n, sch, ctx_rig.src, ctx_rig.w, out.fl, out.net, ice, None if block_is_null else block)
            text = str(err.value)
            assert f"({abi_err_invalid()})" in text and field in text, (field, text)
            ctx_rig.ctx.sync()
            assert_same_bits(out.bits(), untouched, f"rejected for {field}")

        refused(rig, "coupled", block_is_null=True)
        refused(bare, "cf_set_sea_ice_formulation")
        for field, mutate in REJECTIONS.items():
            refused(rig, field, mutate=mutate)
        # … and the same arguments unchanged are accepted
        sch, block = coupled_arguments(rig, out, pipeline=abi.PIPELINE_WITHIN_CALL)
        rig.ctx.time_steps_coupled(0, 1, sch, rig.src, rig.w, out.fl, out.net, rig.stresses, block)
        rig.ctx.sync()
        assert not torch.equal(out.bits()["net.T"], untouched["net.T"])
    finally:
        rig.close()
        bare.close()


def abi_err_invalid():
    return -1   # CF_ERR_INVALID


# ---------------------------------------------------------------------------------------------
# 5. models.time_steps
# ---------------------------------------------------------------------------------------------
def _model(step_callback=None):
    from coflux import models as cm
    from coflux import synthetic as syn
    nx, ny, nz, h = 48, 24, 4, 3
    grid = cm.LatitudeLongitudeGrid(size=(nx, ny, nz), halo=(h, h, h), latitude=(-75, 75), z=(-40, 0))
    case = host_case(nx, ny, h, h)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to("cuda")  # noqa: E731
    restoring = cm.SurfaceFluxRestoring(dev(case["target"]), piston_velocity=1.0 / 6.0)
    ocean = cm.ocean_simulation(grid, step_callback=step_callback, additional_surface_fluxes=dict(S=restoring))
    o = case["oceans"][0]
    cm.set_surface(ocean, T=o["T"], S=o["S"], u=o["u"], v=o["v"], mask=o["mask"])
    si = case["ice_state"]
    sea_ice = cm.PrescribedSeaIce(concentration=dev(case["concentrations"][0]), x_stress=dev(case["x_stress"]), y_stress=dev(case["y_stress"]),
                                  thickness=dev(si["thickness"]), top_surface_temperature=dev(si["top_temperature"]), u=dev(si["u"]),
                                  v=dev(si["v"]), albedo=dev(si["albedo"]))
    atmosphere = cm.JRA55PrescribedAtmosphere(syn.jra55_snapshots(3))
    land = cm.JRA55PrescribedLand(syn.jra55_land_snapshots(3))
    model = cm.build_coupled_model(ocean, sea_ice, atmosphere, cm.Radiation(), land, "corrected", ocean_minimum_salinity=cc.MIN_SALINITY)
    return model, cm.NormalizeSalinity(ocean, area=dev(case["area"]))


def _model_fields(model, normalize):
    itf, si = model.interfaces, model.sea_ice
    out = {"land": itf.land_freshwater, "additional": normalize.additional_buffer, "mean": normalize.mean_total,
           "top_surface_temperature": si.top_surface_temperature, "interface_heat": si.interface_heat, "salt_flux": si.salt_flux,
           "frazil_heat": si.frazil_heat}
    for name, d in (("exchange", itf.exchange_atmosphere_state), ("ao", itf.atmosphere_ocean_interface._fields),
                    ("ai", itf.atmosphere_sea_ice_interface._fields), ("net", itf.net_fluxes._ocean_fields),
                    ("net_ice", itf.net_fluxes._sea_ice_fields), ("ice_ocean", itf.sea_ice_ocean_fluxes)):
        out.update({f"{name}.{k}": v for k, v in d.items()})
    return out


@pytest.mark.parametrize("dt", [1350.0, 1200.0], ids=["binary_fraction", "twenty_minutes"])
def test_models_time_steps_is_twelve_time_steps_and_the_callable(dt):
    """models.time_steps(model, Δt, 12, normalize) on a 48 × 24 model with sea ice, JRA55PrescribedLand, a SurfaceFluxRestoring on
    S and NormalizeSalinity leaves every field of the model and both clocks as 12 × (time_step; normalize) does.  Δt = 3 h / 8:
    the device loop's clock is time_step!'s own and the run is one cf_time_steps_coupled call; Δt = 20 min: the clocks are
    held together by re-basing."""
    from coflux import models as cm
    host, host_norm = _model()
    for _ in range(12):
        cm.time_step(host, dt)
        host_norm(host)
    host.interfaces.context.sync()
    device, device_norm = _model()
    ctx = device.interfaces.context
    calls = []
    inner = ctx.time_steps_coupled
    ctx.time_steps_coupled = lambda *a, **k: (calls.append(a[:2]), inner(*a, **k))[1]
    cm.time_steps(device, dt, 12, normalize=device_norm)
    ctx.sync()
    assert sum(n for _first, n in calls) == 12 and [f for f, _n in calls] == sorted(f for f, _n in calls)
    if dt == 1350.0:
        assert calls == [(0, 12)]
    assert (device.clock.time, device.clock.iteration) == (host.clock.time, host.clock.iteration) == (12 * dt, 12)
    assert (device.ocean.model.clock.time, device.ocean.model.clock.iteration) == (host.ocean.model.clock.time, host.ocean.model.clock.iteration)
    want, got = _model_fields(host, host_norm), _model_fields(device, device_norm)
    assert got.keys() == want.keys()
    for k in want:
        assert torch.equal(got[k].view(torch.int64), want[k].view(torch.int64)), k
    assert float((want["frazil_heat"] < 0).sum()) >= 8     # the designed cells are in the model


def test_models_time_steps_refuses_a_model_with_host_work_between_the_steps():
    from coflux import models as cm
    model, normalize = _model(step_callback=lambda ocean, dt: None)
    with pytest.raises(ValueError, match="step_callback"):
        cm.time_steps(model, 1200.0, 2, normalize=normalize)
