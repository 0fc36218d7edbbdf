"""Every request-ahead interpolation sequence of tests/prefetch_model.py on the device, against a plain replay.

The context under test executes a case — requests, steps, commits, discards, syncs, option and stream switches, cf_time_steps
calls — and after EVERY operation its cf_debug_prefetch_stats must equal what the host model of the contract predicts (which
way each request left, how it ended, how many interpolations the steps launched themselves), with
requests = consumed + mismatched + voided + superseded + discarded + pending.  After every step
  * the exchange set the step used, every interface flux and every net flux (and a sea-ice step's interface and net sea-ice
    fluxes) equal, bit for bit and halos included, those of a second context that never requests ahead, keeps
    CF_OPT_MERGED_PREFETCH = 0, gets the same commits at the same points and interpolates in every step itself;
  * the exchange fields agree to 1e-12 (util.rel_err with util.ATMOS_SCALE, as test_window.py) with the oracle's interpolation
    of the atmosphere the MODEL says the step must see — which ties the replay to something that is not the library.
A step forced by the atmosphere of another time, snapshot generation, source or map is off by ≥ 1e-3 (the margins of
test_prefetch_model_cpu.py), so a mix-up of the bookkeeping shows in both — at the steps whose outputs are still there to be
read.  Of a cf_time_steps call that is its LAST step: what an inner step computed is overwritten before the call returns.  So
every continuing case comes twice, as 8 + 13 steps and as 8 + 1 + 12, where the step that meets the pending (stale, voided,
foreign) state is a call of its own and its numbers are compared; the 8 + 13 form is held by the counters and the call's last
step alone (test_prefetch_model_cpu.py asserts which cases show which defect in a compared step).

Ordering.  A missing event wait changes bits only when the race is lost.  Cases that overwrite a set or a slot first queue
three steps that read it, and results are copied on the stream and compared only at the end of a case, so that nothing
drains the queues in between: that makes a lost race LIKELY, not certain.  There are no repetition loops to raise the odds."""
import numpy as np
import pytest
import torch

import oracle as orc
import prefetch_model as pm
import util
from coflux import abi
from coflux import interface_computations as ic
from coflux import synthetic as syn
from coflux.runtime import EXCHANGE_NAMES, FLUX_NAMES, NET_NAMES, CofluxError, FluxContext, SnapshotWindow

pytestmark = pytest.mark.gpu

NX, NY, H = pm.NX, pm.NY, pm.H
ICE_PARTITION = ("concentration", "interface_heat", "salt_flux", "x_stress", "y_stress")


class Bench:
    """One context with everything a case touches on the device: two windows, two in-memory atmospheres, three maps, two ocean
    states, the exchange sets and the outputs."""

    def __init__(self, ice):
        self.ctx = ctx = FluxContext(NX, NY, H, H, ic.flux_params(), ring=pm.RING)
        o0 = syn.ocean_state(NX, NY, H, H)
        o1 = syn.evolved_ocean_state(o0, NX, NY, H, H, 1)
        self.states = [{k: ctx.to_device(o[k]) for k in ("T", "S", "u", "v", "mask")} for o in (o0, o1)]
        self.states[1]["mask"] = self.states[0]["mask"]
        nsy, nsx = pm.source_shape()
        self.windows = {w: SnapshotWindow(ctx, nsx, nsy, pm.N_SLOTS) for w in pm.WINDOWS}
        self.slots = {w: [None] * pm.N_SLOTS for w in pm.WINDOWS}
        self.memory = {}
        for m in pm.MEMORY:
            levels = [pm.snapshot(m, n, 0) for n in range(pm.N_SLOTS)]
            self.memory[m] = {v: ctx.to_device(np.stack([lv[v] for lv in levels])) for v in pm.VARIABLES}
        self.weights = {name: {k: (ctx.to_device(a) if isinstance(a, np.ndarray) else a) for k, a in pm.weights(name).items()}
                        for name in pm.WEIGHTS}
        self.sets = {s: ctx.field_set(EXCHANGE_NAMES) for s in pm.SETS}
        self.fl, self.net = ctx.field_set(FLUX_NAMES), ctx.field_set(NET_NAMES)
        self.ice = None
        if ice:
            ctx.set_sea_ice_formulation(ic.flux_params(ic.corrected_atmosphere_sea_ice_fluxes()))
            si = syn.sea_ice_state(NX, NY, H, H)
            self.ice = {k: ctx.to_device(o0["ice_" + k]) for k in ICE_PARTITION}
            self.ice_state = dict(concentration=self.ice["concentration"],
                                  **{k: ctx.to_device(si[k]) for k in ("thickness", "top_temperature", "u", "v", "albedo")})
            self.ai, self.net_ice = ctx.field_set(FLUX_NAMES), ctx.field_set(("top_heat", "bottom_heat"))
            self.skin0 = self.ice_state["top_temperature"].clone()
            self.ice_state["top_temperature"] = self.ai["temperature"]      # the skin temperature is carried from step to step
        self.side = torch.cuda.Stream(device=ctx.device)

    def close(self):
        torch.cuda.synchronize()
        torch.cuda.set_stream(torch.cuda.default_stream(self.ctx.device))
        for w in self.windows.values():
            w.close()
        self.ctx.close()

    def commit(self, window, slot, n, g):
        assert n % pm.N_SLOTS == slot
        self.windows[window].upload(n, pm.snapshot(window, n, g))
        self.slots[window][slot] = (n, g)

    def reset(self, mode):
        """Between two cases: nothing pending, the windows as the model starts them, the case's starting options, torch's stream."""
        ctx = self.ctx
        ctx.discard_prefetched_atmosphere_state()
        ctx.sync()
        torch.cuda.synchronize()
        torch.cuda.set_stream(torch.cuda.default_stream(ctx.device))
        ctx.use_torch_stream()
        assert ctx.prefetch_stats()["pending"] == 0
        for w in pm.WINDOWS:
            for s in range(pm.N_SLOTS):
                if self.slots[w][s] != (s, 0):
                    self.commit(w, s, s, 0)
        ctx.set_option(abi.OPT_MERGED_PREFETCH, mode)
        ctx.set_option(abi.OPT_FUSED_NET, 2)
        ctx.set_option(abi.OPT_INTERP_TILE_CAP, pm.TILE_CAP_DEFAULT)
        if self.ice is not None:
            self.ai["temperature"].copy_(self.skin0)

    # -- what the operations name ---------------------------------------------------------------
    def source(self, src, l1, l2, tf):
        """(source, keyword arguments) for the runtime's calls."""
        if src in pm.WINDOWS:
            return self.windows[src].source(self.slots[src][l1][0], self.slots[src][l2][0], tf), {}
        return self.memory[src], dict(level1=l1, level2=l2, time_fraction=tf)

    def loop_source(self, src):
        """The source of a cf_time_steps call, which reads whatever level its clock reaches: every slot is ordered first."""
        if src in pm.WINDOWS:
            n = [c[0] for c in self.slots[src]]
            self.windows[src].source(n[2], n[3], 0.0)
            return self.windows[src].source(n[0], n[1], 0.0)
        return self.memory[src]

    def step(self, op, atmos):
        src, kw = self.source(op.src, op.l1, op.l2, op.tf)
        if op.ice:
            self.ctx.update_state_sea_ice(src, self.weights[op.w], self.states[op.ocean], atmos, self.fl, self.net, self.ice, self.ice_state,
                                          self.ai, self.net_ice, **kw)
        else:
            self.ctx.update_state(src, self.weights[op.w], self.states[op.ocean], atmos, self.fl, self.net, ice=self.ice, **kw)

    def outputs(self, atmos, ice_step):
        """Copies, on the stream, of everything a step wrote."""
        groups = [("atmos", atmos), ("fluxes", self.fl), ("net", self.net)]
        if ice_step:
            groups += [("ice_fluxes", self.ai), ("net_ice", self.net_ice)]
        return {"%s.%s" % (g, k): v.clone() for g, d in groups for k, v in d.items()}


def replay(ref, ops, pred):
    """The reference: no request ahead, one exchange set, every step interpolates for itself — the same commits at the same points."""
    R, out = ref.sets["A"], []
    for op, p in zip(ops, pred):
        rec = None
        if isinstance(op, pm.Commit):
            ref.commit(op.window, op.slot, op.n, ref.slots[op.window][op.slot][1] + 1)
        elif isinstance(op, pm.Step):
            src, kw = ref.source(op.src, op.l1, op.l2, op.tf)
            ref.ctx.interpolate_atmosphere_state(src, ref.weights[op.w], R, **kw)
            ref.step(op, R)
            ref.ctx.sync()
            rec = ref.outputs(R, op.ice)
        elif isinstance(op, pm.TimeSteps):
            for step in range(op.first, op.first + op.n):
                l1, l2, tf = pm.clock(op, step)
                ref.step(pm.Step("A", op.src, op.w, l1, l2, tf, step % 2, False), R)
                ref.ctx.sync()
            rec = ref.outputs(R, False) if op.n else None
        out.append(rec)
    return out


def execute(bench, ops, pred):
    """The context under test runs the case; the counters are held to the model after every operation."""
    ctx = bench.ctx
    base = ctx.prefetch_stats()
    assert base["pending"] == 0
    out = []
    for k, (op, p) in enumerate(zip(ops, pred)):
        rec = None
        if isinstance(op, pm.Request):
            src, kw = bench.source(op.src, op.l1, op.l2, op.tf)
            if p["refused"]:
                with pytest.raises(CofluxError, match="two prefetched atmosphere states are already pending"):
                    ctx.prefetch_atmosphere_state(src, bench.weights[op.w], bench.sets[op.set], **kw)
            else:
                ctx.prefetch_atmosphere_state(src, bench.weights[op.w], bench.sets[op.set], **kw)
        elif isinstance(op, pm.Step):
            bench.step(op, bench.sets[op.set])
            rec = bench.outputs(bench.sets[op.set], op.ice)
        elif isinstance(op, pm.Write):
            src, kw = bench.source(op.src, op.l1, op.l2, op.tf)
            ctx.interpolate_atmosphere_state(src, bench.weights[op.w], bench.sets[op.set], **kw)
        elif isinstance(op, pm.Commit):
            bench.commit(op.window, op.slot, op.n, bench.slots[op.window][op.slot][1] + 1)
        elif isinstance(op, pm.Discard):
            ctx.discard_prefetched_atmosphere_state()
        elif isinstance(op, pm.Sync):
            ctx.sync()
        elif isinstance(op, pm.SetMode):
            ctx.set_option(abi.OPT_MERGED_PREFETCH, op.mode)
        elif isinstance(op, pm.SetFusedNet):
            ctx.set_option(abi.OPT_FUSED_NET, op.value)
        elif isinstance(op, pm.SetTileCap):
            ctx.set_option(abi.OPT_INTERP_TILE_CAP, op.cap)
        elif isinstance(op, pm.SetStream):
            old = torch.cuda.current_stream(ctx.device)
            new = bench.side if op.which == "side" else torch.cuda.default_stream(ctx.device)
            # A state that left on the old stream and is still pending: cf_set_stream itself must order the new stream behind it,
            # and (an event at the end of the old stream) behind everything else with it.  Nothing such pending: the library
            # promises nothing, and the test orders the streams itself.
            if not (k and pred[k - 1]["on_main"]):
                new.wait_stream(old)
            torch.cuda.set_stream(new)
            ctx.use_torch_stream()
        elif isinstance(op, pm.TimeSteps):
            names = ("A", "B") if op.pipeline else ("A",)
            sched = ctx.make_schedule(bench.states, [bench.sets[s] for s in names], first_level=op.first_level, time_fraction=op.tf0,
                                      time_fraction_increment=op.inc, pipeline=op.pipeline)
            ctx.time_steps(op.first, op.n, sched, bench.loop_source(op.src), bench.weights[op.w], bench.fl, bench.net, ice=bench.ice)
            if op.n:
                rec = bench.outputs(bench.sets[names[(op.first + op.n - 1) % len(names)]], False)
        else:
            raise TypeError(op)
        now = ctx.prefetch_stats()
        got = {c: now[c] - (0 if c == "pending" else base[c]) for c in pm.COUNTERS}
        assert got == p["counters"], (k, op, {c: (got[c], p["counters"][c]) for c in pm.COUNTERS if got[c] != p["counters"][c]})
        assert got["requests"] == sum(got[c] for c in pm.OUTCOMES) + got["pending"], (k, op, got)
        out.append(rec)
    return out


_GRID = orc.make_grid(NX, NY, H, H, pm.RING)
_ORACLE = {}


def oracle_exchange(atmos):
    if atmos not in _ORACLE:
        ref = orc.interpolate_atmosphere_state(_GRID, pm.two_levels(atmos), pm.weights(atmos.w), 0, 1, atmos.tf)
        _ORACLE[atmos] = {k: pm.ring_window(ref[k]) for k in EXCHANGE_NAMES}
    return _ORACLE[atmos]


@pytest.fixture(scope="module")
def benches():
    made = {}

    def get(ice):
        if ice not in made:
            made[ice] = (Bench(ice), Bench(ice))
        return made[ice]
    yield get
    for pair in made.values():
        for b in pair:
            b.close()


CASES = {name: (mode, ops) for name, mode, ops in pm.atlas()}


@pytest.mark.parametrize("name", list(CASES))
def test_sequence_on_the_device(benches, name):
    mode, ops = CASES[name]
    pred = pm.predict(mode, ops)
    test, ref = benches(any(isinstance(op, pm.Step) and op.ice for op in ops))
    ref.reset(0)
    test.reset(mode)
    want = replay(ref, ops, pred)
    try:
        got = execute(test, ops, pred)
        torch.cuda.synchronize()
    finally:
        torch.cuda.set_stream(torch.cuda.default_stream(test.ctx.device))
    for k, (op, p, g, w) in enumerate(zip(ops, pred, got, want)):
        if g is None:
            assert w is None
            continue
        assert set(g) == set(w)
        for field in g:
            assert torch.equal(g[field], w[field]), (k, op, field, "differs from the replay")
        ref_atmos = oracle_exchange(p["sees"][-1])
        for f in EXCHANGE_NAMES:
            e = util.rel_err(pm.ring_window(g["atmos." + f].cpu().numpy()), ref_atmos[f], util.ATMOS_SCALE[f])
            assert e <= 1e-12, (k, op, f, e, p["sees"][-1])
