"""A cf_time_steps call that is refused must leave the context as it found it (include/coflux.h, cf_time_steps): no launch, no
request-ahead interpolation, no halo request left armed for the next cf_update_state.  Single process, no neighbour: a context
connected as rank 0 of 1 has nobody on either side, so its riders and its exchange kernel return at once and nothing here can
wait — while cf_peer_halo_stats still counts every exchange issued, which is the observable.

Two contexts built alike run the same calls, one of them with a refused call in the middle: after it, and after everything that
follows, the two must agree in every counter and every output bit."""
import ctypes as C
import functools

import pytest
import torch

from coflux import abi
from coflux import interface_computations as ic
from coflux import synthetic as syn
from coflux.runtime import EXCHANGE_NAMES, FLUX_NAMES, NET_NAMES, FluxContext

pytestmark = pytest.mark.gpu

NX, NY, H, RING = 72, 12, 4, 1
N_LEVELS, INC = 4, 1.0 / 9.0
FIELDS = ("T", "S", "u", "v")
ERR_INVALID = -1   # CF_ERR_INVALID (include/coflux.h)
MODES = {"off": 0, "within_call": abi.PIPELINE_WITHIN_CALL, "continuing": abi.PIPELINE_CONTINUING}


@functools.lru_cache(maxsize=None)
def _host_case(nx, ny):
    """Built once per shape and never written to: two ocean states a step apart (with land), the snapshots, the weights."""
    o0 = syn.ocean_state(nx, ny, H, H)
    o1 = syn.evolved_ocean_state(o0, nx, ny, H, H, 1)
    assert (o0["mask"][H:H + ny, H:H + nx] == 0).any() and (o0["mask"][H:H + ny, H:H + nx] != 0).any()
    return (o0, o1), syn.jra55_snapshots(N_LEVELS), syn.latlon_fractional_indices(nx, ny, H, H)


class _Rig:
    """One context, connected as rank 0 of 1, with CF_OPT_HALO_IN_SOLVER_LAUNCH and the tail workgroups on."""

    def __init__(self, nx=NX, ny=NY):
        oceans, src, (fi, fj, phi) = _host_case(nx, ny)
        self.ctx = ctx = FluxContext(nx, ny, H, H, ic.flux_params(), ring=RING)
        ctx.peer_halo_export(4, RING + 1)
        ctx.peer_halo_connect(None, None, 0, 1)
        ctx.set_option(abi.OPT_HALO_IN_SOLVER_LAUNCH, 1)
        ctx.set_option(abi.OPT_MERGED_PREFETCH, 2)
        self.states = [{k: ctx.to_device(o[k]) for k in FIELDS + ("mask",)} for o in oceans]
        self.states[1]["mask"] = self.states[0]["mask"]
        self.src = {k: ctx.to_device(v) for k, v in src.items()}
        self.w = dict(separable=True, fi=ctx.to_device(fi), fj=ctx.to_device(fj), latitude=ctx.to_device(phi))
        self.sets = [ctx.field_set(EXCHANGE_NAMES) for _ in range(2)]
        self.plain_set = ctx.field_set(EXCHANGE_NAMES)
        self.fl, self.net = ctx.field_set(FLUX_NAMES), ctx.field_set(NET_NAMES)

    def arguments(self, pipeline, *, fold_north=False):
        """The ctypes arguments of a cf_time_steps call, every one of them valid: (schedule, source, weights, fluxes, net)."""
        ctx = self.ctx
        sched = ctx.make_schedule(self.states, self.sets if pipeline else self.sets[:1], time_fraction_increment=INC, pipeline=pipeline,
                                  halo_backend=abi.HALO_PEER, halo_rows=RING + 1, fold_north=fold_north)
        return [sched, ctx.source_struct(self.src, 0, 0, 0.0), ctx.weights_struct(self.w), ctx.fluxes_struct(self.fl), ctx.net_struct(self.net)]

    def time_steps(self, first, n, args):
        """(return code, message) of cf_time_steps with `args`"""
        sched, s, w, f, net = args
        rc = self.ctx.lib.cf_time_steps(self.ctx._h, first, n, C.byref(sched), C.byref(s), C.byref(w), C.byref(f), None, C.byref(net))
        return rc, self.ctx.lib.cf_last_error(self.ctx._h).decode()

    def valid_steps(self, first, n, pipeline):
        rc, text = self.time_steps(first, n, self.arguments(pipeline))
        assert rc == 0, text

    def plain_update(self):
        """A cf_update_state of the host that has nothing to do with the loop: its own exchange set, its own clock."""
        self.ctx.update_state(self.src, self.w, self.states[0], self.plain_set, self.fl, self.net, level1=2, level2=3, time_fraction=0.625)

    def counters(self):
        return dict(halo=self.ctx.peer_halo_stats(), land_zero_launches=self.ctx.debug_land_zero_launches(), prefetch=self.ctx.prefetch_stats())

    def bits(self):
        """Every array the context's calls write, as it stands once the stream has drained"""
        self.ctx.sync()
        torch.cuda.synchronize()
        out = {"fl." + k: v for k, v in self.fl.items()} | {"net." + k: v for k, v in self.net.items()}
        for n, d in (("set0", self.sets[0]), ("set1", self.sets[1]), ("plain", self.plain_set)):
            out.update({f"{n}.{k}": v for k, v in d.items()})
        for n, st in enumerate(self.states):
            out.update({f"ocean{n}.{k}": st[k] for k in FIELDS})
        return {k: v.view(torch.int64).clone() for k, v in out.items()}


def _same_bits(got, want, what):
    assert got.keys() == want.keys()
    for k in want:
        assert torch.equal(got[k], want[k]), f"{what}: {k} differs in {int((got[k] != want[k]).sum())} of {want[k].numel()} words"


# what makes the call refuse: (shape of the context, first step of the refused call, mutation of the valid arguments, words of the
# message).  `args` = [schedule, source, weights, fluxes, net]; the rig is there for the schedules that have to be made anew.
def _null_ocean_state_1(rig, args, pipeline):
    broken = [rig.states[0], dict(rig.states[1], S=None)]
    args[0] = rig.ctx.make_schedule(broken, rig.sets if pipeline else rig.sets[:1], time_fraction_increment=INC, pipeline=pipeline,
                                    halo_backend=abi.HALO_PEER, halo_rows=RING + 1)


def _null_second_set(rig, args, pipeline):
    broken = [rig.sets[0], dict(rig.sets[1], Qs=None)]
    args[0] = rig.ctx.make_schedule(rig.states, broken, time_fraction_increment=INC, pipeline=pipeline, halo_backend=abi.HALO_PEER,
                                    halo_rows=RING + 1)


def _fold(rig, args, pipeline):
    args[0].fold_north = 1


def _null_source_variable(rig, args, pipeline):
    args[1].data[2] = None


REFUSALS = {
    "fluxes_member": ((NX, NY), 3, lambda rig, args, pipeline: setattr(args[3], "latent_heat", None), "interface flux fields"),
    "net_member": ((NX, NY), 3, lambda rig, args, pipeline: setattr(args[4], "S", None), "net ocean flux fields"),
    # first step 4: ocean state 0 is whole, the refusal is that of the call's SECOND step
    "ocean_state_1_field": ((NX, NY), 4, _null_ocean_state_1, "ocean surface fields"),
    "second_exchange_set_member": ((NX, NY), 3, _null_second_set, "exchange fields"),
    "source_variable": ((NX, NY), 3, _null_source_variable, "atmosphere source variable 2"),
    "weights_member": ((NX, NY), 3, lambda rig, args, pipeline: setattr(args[2], "fj", None), "interpolation weights"),
    "fold_on_ring_plus_1_rows": ((NX, RING + 1), 3, _fold, "cf_fold_north_halo: rows"),
    "fold_on_odd_nx": ((NX - 1, NY), 3, _fold, "even number of columns"),
}
CASES = [(name, mode) for name in REFUSALS for mode in MODES if not (name == "second_exchange_set_member" and mode == "off")]


@pytest.mark.parametrize("name,mode", CASES, ids=[f"{n}-{m}" for n, m in CASES])
def test_a_refused_step_call_leaves_the_context_as_it_found_it(name, mode):
    """X: 3 steps, the refused call, a plain cf_update_state, 3 more steps.  Y: the same without the refused call.
    The refused call returns CF_ERR_INVALID naming its argument; X's counters (exchanges, land-zero launches, the ledger of
    requested states — validation runs before the first request, so they are equal, not merely compatible) are Y's right after
    it; the plain cf_update_state issues no exchange on either; at the end X holds Y's bits and Y's exchange counts; and the
    refused call wrote to nothing."""
    (nx, ny), first, mutate, words = REFUSALS[name]
    pipeline = MODES[mode]
    x, y = _Rig(nx, ny), _Rig(nx, ny)
    try:
        for rig in (x, y):
            rig.valid_steps(0, 3, pipeline)
        assert x.counters()["halo"][0] == 3, "every step of a CF_HALO_PEER loop issues one exchange, neighbours or not"
        if pipeline:
            assert x.counters()["halo"][1] >= 2, ("the exchanges of steps with a request behind them ride in the solver launch", x.counters())
        before = x.bits()
        args = x.arguments(pipeline)
        mutate(x, args, pipeline)
        rc, text = x.time_steps(first, 3, args)
        assert rc == ERR_INVALID and words in text, (rc, text)
        _same_bits(x.bits(), before, "the refused call wrote")
        y.bits()   # (drains Y as X was drained)
        assert x.counters() == y.counters(), "after the refused call"
        for rig in (x, y):
            exchanges = rig.counters()["halo"][0]
            rig.plain_update()
            assert rig.counters()["halo"][0] == exchanges, "a cf_update_state outside any loop issued a halo exchange: a request was left armed"
        for rig in (x, y):
            rig.valid_steps(3, 3, pipeline)
        _same_bits(x.bits(), y.bits(), "after three more steps")
        assert x.counters() == y.counters(), "after three more steps"
        assert x.counters()["halo"][0] == 6
    finally:
        x.ctx.close()
        y.ctx.close()


def test_a_refused_coupled_call_leaves_the_context_as_it_found_it():
    """cf_time_steps_coupled shares the loop and validated its block before the first launch all along (CF_HALO_NONE: nothing
    moves ice rows between ranks): the same X / Y comparison, as a guard on the shared loop."""
    import test_coupled_steps as tcs
    pipeline = abi.PIPELINE_WITHIN_CALL
    rigs = [tcs.Rig(tcs.host_case(72, 12, 4, 3), merged=2) for _ in range(2)]
    try:
        outs = [tcs.Outputs(rig) for rig in rigs]

        def steps(rig, out, first, mutate=None):
            sch, block = tcs.coupled_arguments(rig, out, pipeline=pipeline)
            if mutate:
                mutate(block)
            s, w = rig.ctx.source_struct(rig.src, 0, 0, 0.0), rig.ctx.weights_struct(rig.w)
            f, n, i = rig.ctx.fluxes_struct(out.fl), rig.ctx.net_struct(out.net), rig.ctx.ice_struct(rig.stresses)
            rc = rig.ctx.lib.cf_time_steps_coupled(rig.ctx._h, first, 3, C.byref(sch), C.byref(s), C.byref(w), C.byref(f), C.byref(i), C.byref(n),
                                                   C.byref(block))
            return rc, rig.ctx.lib.cf_last_error(rig.ctx._h).decode()

        def settled(rig, out):
            rig.ctx.sync()
            return out.bits()

        for rig, out in zip(rigs, outs):
            assert steps(rig, out, 0)[0] == 0
        (x, xo), (y, yo) = zip(rigs, outs)
        before = settled(x, xo)
        rc, text = steps(x, xo, 3, lambda block: setattr(block.net_ice, "top_heat", None))
        assert rc == ERR_INVALID and "net_ice" in text, (rc, text)
        tcs.assert_same_bits(settled(x, xo), before, "the refused call wrote")
        assert x.ctx.prefetch_stats() == y.ctx.prefetch_stats() and x.ctx.peer_halo_stats() == y.ctx.peer_halo_stats() == (0, 0)
        for rig, out in zip(rigs, outs):
            plain = rig.ctx.field_set(EXCHANGE_NAMES)
            rig.ctx.update_state(rig.src, rig.w, rig.oceans[0], plain, out.fl, out.net, level1=0, level2=1, time_fraction=0.625)
            assert steps(rig, out, 3)[0] == 0
        tcs.assert_same_bits(settled(x, xo), settled(y, yo), "after three more steps")
        assert x.ctx.prefetch_stats() == y.ctx.prefetch_stats() and x.ctx.peer_halo_stats() == (0, 0)
    finally:
        for rig in rigs:
            rig.close()
