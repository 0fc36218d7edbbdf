"""GPU tests of the coupled loop following a staged dataset (cf_attach_restoring_dataset, include/coflux.h) on the designed case
of tests/coupled_case.py: three levels at (0, 1000, 2500) s under a period of 4000 s and a clock of 700 s steps — seven steps
that start on a level time, cross a level boundary and cross the year's wrap.  cf_time_steps_coupled with the dataset attached
is held, bit for bit on every whole output buffer, to a replay of one-step calls each restoring toward a static target that
cf_dataset_evaluate filled for that step."""
import numpy as np
import pytest
import torch

import coupled_case as cc
import dataset_case as case
import dataset_reference as ref
from coflux import abi
from coflux.runtime import CofluxError
from test_coupled_steps import Outputs, Rig, assert_same_bits, host_case

pytestmark = pytest.mark.gpu

TIMES, PERIOD, STEP_SECONDS, N_STEPS = (0.0, 1000.0, 2500.0), 4000.0, 700.0, 7
SHAPE = (131, 37, 4, 3)


def planes():
    small = case.full_plane()
    small[3:8, [22, 23, 0, 1]] = np.nan       # a continent across the seam, to be inpainted
    small[0, 5:9] = np.nan
    return [small, np.roll(small, 5, axis=1) * np.float32(1.015625), np.flipud(small) + np.float32(0.375)]


def staged_dataset(rig, times=TIMES, period=PERIOD, stage=True):
    ctx, g = rig.ctx, rig.ctx.grid
    fi, fj = case.fractional_indices(g.nx, g.ny, g.hx, g.hy, 24, 12)
    w = dict(separable=True, fi=ctx.to_device(fi), fj=ctx.to_device(fj))
    d = ctx.dataset(24, 12, times, w, period=period, periodic_x=True, fill_value=35.0)
    if stage:
        for level, plane in enumerate(planes()[:len(times)]):
            d.stage(level, plane)
    return d


def arguments(rig, out, target, pipeline=0):
    ctx = rig.ctx
    sch = ctx.make_schedule(rig.oceans, out.sets, first_level=cc.ATMOS_CLOCK["first_level"], time_fraction=cc.ATMOS_CLOCK["fraction"],
                            time_fraction_increment=cc.ATMOS_CLOCK["increment"], pipeline=pipeline)
    block = ctx.make_coupled_step(rig.ice_states, out.skin, out.ai, out.net_ice, friver=rig.friver, licalvf=rig.licalvf, land_out=out.land,
                                  land_first_level=cc.LAND_CLOCK["first_level"], land_time_fraction=cc.LAND_CLOCK["fraction"],
                                  land_time_fraction_increment=cc.LAND_CLOCK["increment"], ice_ocean_params=rig.iop,
                                  ice_ocean_fluxes=out.iof, piston_velocity=cc.PISTON_VELOCITY, target=target,
                                  restoring_out=out.restoring, normalize=True, area=rig.area, mean_out=out.mean)
    return sch, block


def run(rig, out, calls, target=None):
    for first, n, pipeline in calls:
        sch, block = arguments(rig, out, target, pipeline)
        rig.ctx.time_steps_coupled(first, n, sch, rig.src, rig.w, out.fl, out.net, rig.stresses, block)
    rig.ctx.sync()
    rig.ctx.discard_prefetched_atmosphere_state()


def test_the_clock_of_the_case_lands_where_it_was_designed_to():
    index = [ref.time_index(list(TIMES), PERIOD, STEP_SECONDS * s) for s in range(N_STEPS)]
    assert [(a, b) for a, b, _f in index] == [(0, 1), (0, 1), (1, 2), (1, 2), (2, 0), (2, 0), (0, 1)]
    assert index[0][2] == 0.0 and all(0.0 < f < 1.0 for _a, _b, f in index[1:])


def test_the_attached_loop_is_the_replay_toward_evaluated_targets_bit_for_bit():
    rig = Rig(host_case(*SHAPE))
    ctx = rig.ctx
    try:
        d = staged_dataset(rig)
        want = Outputs(rig)
        target = ctx.zeros()
        restoring = []
        for s in range(N_STEPS):
            d.evaluate(STEP_SECONDS * s, target)
            run(rig, want, [(s, 1, 0)], target=target)
            restoring.append(want.restoring.clone())
        assert not torch.equal(restoring[0], restoring[1]) and not torch.equal(restoring[3], restoring[5])   # the target moves
        ctx.attach_restoring_dataset(d, time_origin=0.0, step_seconds=STEP_SECONDS)
        got = Outputs(rig)
        run(rig, got, [(0, N_STEPS, 0)])
        assert_same_bits(got.bits(), want.bits(), "7 steps attached")
        # the clock is origin + s · step with the GLOBAL step index: an origin that puts step 2 one period after level 0's time
        ctx.attach_restoring_dataset(d, time_origin=PERIOD - 2.0 * STEP_SECONDS, step_seconds=STEP_SECONDS)
        shifted, static = Outputs(rig), Outputs(rig)
        run(rig, shifted, [(2, 1, 0)])
        ctx.attach_restoring_dataset(None)
        d.evaluate(PERIOD, target)
        run(rig, static, [(2, 1, 0)], target=target)
        assert_same_bits(shifted.bits(), static.bits(), "step 2 under a shifted origin")
        d.close()
    finally:
        rig.close()


def test_one_call_is_three_plus_four_continuing_calls():
    rig = Rig(host_case(*SHAPE), merged=2)
    try:
        d = staged_dataset(rig)
        rig.ctx.attach_restoring_dataset(d, time_origin=0.0, step_seconds=STEP_SECONDS)
        one, split = Outputs(rig), Outputs(rig)
        run(rig, one, [(0, N_STEPS, abi.PIPELINE_CONTINUING)])
        run(rig, split, [(0, 3, abi.PIPELINE_CONTINUING), (3, 4, abi.PIPELINE_CONTINUING)])
        assert_same_bits(split.bits(), one.bits(), "3 + 4 steps")
        rig.ctx.attach_restoring_dataset(None)
        d.close()
    finally:
        rig.close()


def test_a_one_level_dataset_is_the_static_target():
    rig = Rig(host_case(*SHAPE))
    try:
        d = staged_dataset(rig, times=(123.0,), period=0.0)
        static = d.level(0)
        want, got = Outputs(rig), Outputs(rig)
        run(rig, want, [(0, N_STEPS, 0)], target=static)
        rig.ctx.attach_restoring_dataset(d, time_origin=-1e6, step_seconds=STEP_SECONDS)
        run(rig, got, [(0, N_STEPS, 0)])
        assert_same_bits(got.bits(), want.bits(), "one level")
        rig.ctx.attach_restoring_dataset(None)
        d.close()
    finally:
        rig.close()


@pytest.mark.parametrize("dt", [1350.0, 1200.0], ids=["binary_fraction", "twenty_minutes"])
def test_models_time_steps_follow_a_dataset_restoring(dt):
    """models.time_steps on a model whose SurfaceFluxRestoring targets a DatasetRestoring leaves every field as 12 ×
    (time_step; normalize) does, which materialises the restoring at the model clock through cf_materialize_dataset_restoring;
    set_from_dataset gives the level a one-level dataset holds."""
    from coflux import models as cm
    from test_coupled_steps import _model, _model_fields

    def build():
        model, normalize = _model()
        normalize.additional_fluxes.target = cm.DatasetRestoring(np.stack(planes()), TIMES, PERIOD, fill_value=35.0)
        return model, normalize

    host, host_norm = build()
    buffers = []
    for _ in range(12):
        cm.time_step(host, dt)
        host_norm(host)
        buffers.append(host_norm.additional_buffer.clone())
    host.interfaces.context.sync()
    assert not torch.equal(buffers[0], buffers[1])   # the target moves
    device, device_norm = build()
    cm.time_steps(device, dt, 12, normalize=device_norm)
    device.interfaces.context.sync()
    want, got = _model_fields(host, host_norm), _model_fields(device, device_norm)
    for k in want:
        assert torch.equal(got[k].view(torch.int64), want[k].view(torch.int64)), k
    ctx, grid = device.interfaces.context, device.ocean.grid
    field = ctx.zeros()
    cm.set_from_dataset(field, planes()[0], ctx, grid, fill_value=35.0)
    level = device_norm.additional_fluxes.target.dataset(ctx, grid).level(0)
    assert torch.equal(field.view(torch.int64), level.view(torch.int64)) and float(field.abs().max()) > 30.0


def test_refusals_leave_the_outputs_untouched():
    rig, other = Rig(host_case(*SHAPE)), Rig(host_case(*SHAPE), sea_ice=False)
    ctx = rig.ctx
    try:
        out = Outputs(rig)
        untouched = out.bits()

        def refused(word, target):
            sch, block = arguments(rig, out, target)
            with pytest.raises(CofluxError, match=word):
                ctx.time_steps_coupled(0, 3, sch, rig.src, rig.w, out.fl, out.net, rig.stresses, block)
            ctx.sync()
            assert_same_bits(out.bits(), untouched, word)

        d = staged_dataset(rig)
        ctx.attach_restoring_dataset(d, step_seconds=STEP_SECONDS)
        refused("target_salinity", rig.target)                 # both targets given
        ctx.attach_restoring_dataset(None)
        refused("target_salinity", None)                       # none attached: a NULL target is refused as before
        partly = staged_dataset(rig, stage=False)
        partly.stage(0, planes()[0])
        partly.stage(2, planes()[2])
        with pytest.raises(CofluxError, match="level 1"):      # not every level is staged
            ctx.attach_restoring_dataset(partly, step_seconds=STEP_SECONDS)
        refused("target_salinity", None)
        foreign = staged_dataset(other)
        with pytest.raises(CofluxError, match="another context"):
            ctx.attach_restoring_dataset(foreign, step_seconds=STEP_SECONDS)
        refused("target_salinity", None)
        # … and with the dataset attached and no static target the call is accepted
        ctx.attach_restoring_dataset(d, step_seconds=STEP_SECONDS)
        run(rig, out, [(0, 1, 0)])
        assert not torch.equal(out.bits()["restoring"], untouched["restoring"])
        ctx.attach_restoring_dataset(None)
        for h in (d, partly, foreign):
            h.close()
    finally:
        rig.close()
        other.close()
