"""cf_time_steps_coupled with fold_north under CF_HALO_PEER in one process (include/coflux.h: "Tripolar slabs"): the context is
connected as rank 0 of 1 in both worlds — it is the last rank, nothing can wait —, so every exchange of the loop is the launch
whose north side folds the exchange's own fields (csrc/coflux_halo.hip: peer_halo_fold_kernel).  Against the CF_HALO_NONE run
with fold_north = 1 whose nine ice-side fields were folded on the host before upload (tests/coupled_fold_case.py), bit for bit,
whole guarded buffers; and what the form refuses.  The slabs themselves are tests/test_coupled_fold_slabs.py's."""
import numpy as np
import pytest
import torch

import coupled_fold_case as fc
import test_coupled_steps as tcs
from coflux import abi
from coflux import synthetic as syn
from coflux.distributed import connect_coupled_slabs
from coflux.runtime import CofluxError

pytestmark = pytest.mark.gpu

# ny = ring + 2, the smallest slab the fold admits; several rows; nx / 2 odd and no multiple of the wave
SURFACES = [(64, 3), (64, 24), (130, 37)]


def connected_rig(nx, ny):
    rig = fc.make_rig(fc.global_case(nx, ny))
    assert connect_coupled_slabs(rig.ctx) == (0, 1)
    return rig


def cpu_bits(out):
    return {k: v.cpu() for k, v in out.bits().items()}


@pytest.mark.parametrize("nx,ny", SURFACES)
def test_the_exchanges_fold_and_leave_the_reference_runs_bits(nx, ny):
    """Seven pipelined steps.  The north halo rows of all thirteen fields start as NaNs that name field and row; afterwards every
    output, the mean and the skin temperature are the reference's bits in whole guarded buffers, the north halo rows of every
    folded field hold the host fold's bits over the full width, cf_peer_halo_stats grew by (1 + 2 · 7, 0) and
    cf_debug_fold_counts by (0, 1 + 2 · 7): no fold launch of its own.  The reference run grew them by (0, 0) and (7, 0)."""
    want = fc.single_domain(nx, ny)
    assert want["grown"] == (0, 0, fc.STEPS, 0)
    rig = connected_rig(nx, ny)
    try:
        out = tcs.Outputs(rig)
        fields = fc.exchanged_fields(rig, out, nx, ny)
        assert len(fields) == 2 * 4 + 3 + 5 + 2 + 1
        fc.stamp(fields, 0, 1, ny)
        assert all(bool(torch.isnan(t[fc.HY + ny:fc.HY + ny + fc.ROWS]).all()) for t, _g in fields.values())
        before = fc.counters(rig.ctx)
        fc.run(rig, out, fc.SEVEN, abi.HALO_PEER, True)
        assert fc.grown(before, fc.counters(rig.ctx)) == (1 + 2 * fc.STEPS, 0, 0, 1 + 2 * fc.STEPS)
        tcs.assert_same_bits(cpu_bits(out), want["bits"], f"{nx} x {ny}: CF_HALO_PEER with the fold in the exchanges")
        assert not fc.undelivered(fields, 0, 0, ny), fc.undelivered(fields, 0, 0, ny)
        # the fold wrote something: −1 · the mirrored ice drift in the first north halo row, its x-halo columns included
        u = rig.ice_states[0]["u"].cpu().numpy()
        assert np.array_equal(u[fc.HY + ny, fc.HX:fc.HX + nx], -u[fc.HY + ny - 2, fc.HX:fc.HX + nx][::-1])
        assert np.array_equal(u[fc.HY + ny, :fc.HX], u[fc.HY + ny, nx:nx + fc.HX])
    finally:
        rig.close()


@pytest.mark.parametrize("nx,ny", SURFACES)
def test_split_calls_fold_the_call_fields_once_per_call(nx, ny):
    """5 + 2 CF_PIPELINE_CONTINUING steps under the new form equal 5 steps under CF_HALO_NONE, then the caller's own fold of the
    stresses and the skin temperature, then 2 more steps: the once-per-call fields are folded at the head of every call, exactly
    as a neighbour delivers them once per call."""
    ref = fc.make_rig(fc.folded_case(nx, ny))
    rig = connected_rig(nx, ny)
    try:
        want = tcs.Outputs(ref)

        def callers_fold():
            for t, name in ((ref.tx, "x_stress"), (ref.ty, "y_stress"), (want.skin, "skin_temperature")):
                location, sign = fc.CONVENTION[name]
                a = syn.fold_north(t.cpu().numpy(), nx, ny, fc.HX, fc.HY, fc.ROWS, location, sign)
                t.view(torch.int64).copy_(torch.from_numpy(a.view(np.int64)))

        fc.run(ref, want, fc.FIVE_TWO, abi.HALO_NONE, True, between=callers_fold)
        out = tcs.Outputs(rig)
        fields = fc.exchanged_fields(rig, out, nx, ny)
        fc.stamp(fields, 0, 1, ny)
        before = fc.counters(rig.ctx)
        fc.run(rig, out, fc.FIVE_TWO, abi.HALO_PEER, True)
        assert fc.grown(before, fc.counters(rig.ctx)) == (2 + 2 * fc.STEPS, 0, 0, 2 + 2 * fc.STEPS)
        tcs.assert_same_bits(cpu_bits(out), cpu_bits(want), f"{nx} x {ny}: 5 + 2 steps")
        assert not fc.undelivered(fields, 0, 0, ny, skip=("skin",))
    finally:
        ref.close()
        rig.close()


def refused(rig, out, untouched, backend, what):
    sch, block = tcs.coupled_arguments(rig, out, pipeline=abi.PIPELINE_WITHIN_CALL, normalize="exact")
    sch.halo_backend, sch.halo_rows, sch.fold_north = backend, fc.ROWS if backend != abi.HALO_NONE else 0, 1
    before = fc.counters(rig.ctx)
    with pytest.raises(CofluxError) as err:
        rig.ctx.time_steps_coupled(0, fc.STEPS, sch, rig.src, rig.w, out.fl, out.net, rig.stresses, block)
    text = str(err.value)
    assert "(-1)" in text and "fold_north" in text, (what, text)
    rig.ctx.sync()
    tcs.assert_same_bits(cpu_bits(out), untouched, f"refused: {what}")
    assert fc.counters(rig.ctx) == before == (0, 0, 0, 0), what


def test_a_slab_of_two_rows_is_refused_before_the_first_launch():
    """ny = 2 < ring + 2: the fold would read below the slab.  Refused under CF_HALO_PEER and under CF_HALO_NONE alike, naming
    fold_north, with the outputs and every counter untouched."""
    rig = connected_rig(64, 2)
    try:
        out = tcs.Outputs(rig)
        untouched = cpu_bits(out)
        refused(rig, out, untouched, abi.HALO_PEER, "ny = 2 under CF_HALO_PEER")
        refused(rig, out, untouched, abi.HALO_NONE, "ny = 2 under CF_HALO_NONE")
    finally:
        rig.close()


def test_a_rank_with_a_north_neighbour_does_not_own_the_fold():
    """rank 0 of a world of two contexts in one process: its north mailbox is connected, fold_north is the last rank's"""
    rigs = [fc.make_rig(fc.global_case(64, 24)) for _ in range(2)]
    try:
        handles = [r.ctx.peer_halo_export(8, fc.ROWS) for r in rigs]
        rigs[0].ctx.peer_halo_connect(None, handles[1], 0, 2)
        rigs[1].ctx.peer_halo_connect(handles[0], None, 1, 2)
        out = tcs.Outputs(rigs[0])
        refused(rigs[0], out, cpu_bits(out), abi.HALO_PEER, "rank 0 of 2")
    finally:
        for r in rigs:
            r.close()
