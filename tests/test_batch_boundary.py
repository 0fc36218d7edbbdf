"""The lean ocean solver's batch boundary (csrc/coflux_lean_kernel.hpp, ao_lean_body) on the smallest surfaces on which it can
go wrong.

A wave of the solver pulls 64 wet cells at a time from its workgroup's list.  Between two batches it claims the next one,
requests the fused net fluxes' inputs of the batch it has just iterated TOGETHER with the inputs of the batch it has claimed,
waits once, stores, and runs the next batch's prologue.  What can go wrong there is a cell skipped or written twice with another
cell's values at a batch edge, a ragged last batch, a wave that finds no batch at all, and a request for a batch that does not
exist.  So: one workgroup (CF_OPT_AO_CHUNK = 1280 on a 200 × 12 window holds every wet cell in ONE chunk — asserted on the table
as built) whose wet count is 0, 1, 63, 64, 65, 128, 129, 255, 256, 257 and 600: no batch; one lane; a lane short of a batch,
exactly one, one over; two; two and a lane; one wave idle, every wave one batch, a ragged fifth batch; several batches per wave.
The batch loop's exits are all among them: `start >= limit` on a wave's first claim (every count below 193), after one batch
(256, 257), after several (600).  The wet run starts five cells before the end of the south ring row, so every count above 6
mixes ring cells (no net fluxes) and interior cells within a batch.

Every case runs the three-launch cf_update_state (the reference: no fused epilogue), the fused form, both with and without the
optional outputs (friction velocity, temperature and humidity scales, trip counts, the four radiation diagnostics: they change
the number of stores behind the boundary's loads), CF_OPT_TRIP_HINTS 0 – 3 (1 and 3 with two calls: the second runs in the
first's order), the tail-workgroup forms (cf_time_steps with CF_OPT_MERGED_PREFETCH = 2, and a host loop with the next state requested
ahead), a mask rewritten in place (the classification path: no valid list; and, rewritten to all ocean, its two-piece retry:
2400 wet cells in a range whose list holds 1280), and `:corrected` with CF_OPT_LATENCY_LAYOUT = 2 (the line kernels).

Every output is filled with NaN sentinel bits before every call.  A run is held (1) to the CPU oracle at the suite's 1e-9
(tests/test_gpu_parity.TOL_SOLVER; util.rel_err) with identical trip counts, (2) bit for bit to the three-launch reference,
(3) to its footprint: the ring window (fluxes) or the interior (net fluxes) written everywhere, every cell outside still
holding the sentinel.

Wall time on the MI355X: the 22 GPU cases take 3.5 s as a pytest run of their own (the first 0.6 s, the others 0.05 – 0.1 s).
Each kind of check was seen to fail on a deliberately wrong scratch build (not committed): the next batch requested at the
current batch's list position → all 22 cases (counts from 257 up against the oracle at the reference already, the smaller ones
where the mask is rewritten to all ocean and a wave takes a second batch); the net fluxes stored without the interior's east
bound → the 11 `default` cases, "a cell outside the footprint was written" (profiles/batch_boundary_experiments.md §4)."""
import functools

import numpy as np
import pytest

import mask_atlas as ma
import util
from coflux import abi
from coflux import interface_computations as ic
from coflux.runtime import EXCHANGE_NAMES, FLUX_NAMES, FLUX_OPTIONAL, NET_NAMES

gpu = pytest.mark.gpu

NX, NY, H, RING = 198, 10, ma.HALO, ma.RING
WX, WY = NX + 2 * RING, NY + 2 * RING      # 200 × 12
START = 195                                # window index of the first wet cell: 5 ring cells, a ring column, then row 0
WET_COUNTS = (0, 1, 63, 64, 65, 128, 129, 255, 256, 257, 600)
TOL = 1e-9                                 # test_gpu_parity.TOL_SOLVER
N_LEVELS, INC = 4, 1.0 / 9.0
NET_REQUIRED, NET_DIAGNOSTICS = NET_NAMES[:4], NET_NAMES[4:]
CONFIGS = {"default": (), "corrected_line": ((abi.OPT_LATENCY_LAYOUT, 2),)}


def wet_window(count, start=START):
    wet = np.zeros(WX * WY, bool)
    wet[start:start + count] = True
    return wet.reshape(WY, WX)


def test_the_wet_runs_are_what_the_cases_are_named_for():
    """CPU: the counts; a run longer than six cells has ring cells AND interior cells in its first batch."""
    for count in WET_COUNTS:
        wet = wet_window(count)
        inside = int(wet[RING:-RING, RING:-RING].sum())
        assert wet.sum() == count and wet.reshape(-1)[START:START + count].all()
        assert inside == 0 if count <= 6 else 0 < inside < count
        assert not wet_window(count, START + 7).reshape(-1)[:START + 7].any()
    assert START + 7 + max(WET_COUNTS) < WX * WY and 1280 * 64 > 64 * max(WET_COUNTS) + WX * WY   # one chunk of the capacity plan
    assert WX * WY > 1280 and WX * WY > 8 * 256   # all ocean overflows the list; the range outlasts the strips requested up front


@functools.lru_cache(maxsize=None)
def _case():
    case = util.build_case(NX, NY, H, H, land=False, n_levels=N_LEVELS)
    return case


def _params(config):
    fluxes, vd = util.CONFIGS["corrected" if config == "corrected_line" else "default"]()
    return ic.flux_params(fluxes, velocity_difference=vd)


def _clock(step):
    tot = step * INC
    l1 = int(tot) % N_LEVELS
    return l1, (l1 + 1) % N_LEVELS, tot - int(tot)


@functools.lru_cache(maxsize=None)
def _oracle(config, count, start, step):
    import oracle as orc
    case, params = _case(), _params(config)
    g = orc.make_grid(NX, NY, H, H, RING)
    l1, l2, tf = _clock(step)
    at = orc.interpolate_atmosphere_state(g, case["src"], case["weights"], l1, l2, tf)
    wet = np.ones((WY, WX), bool) if count is None else wet_window(count, start)
    oc = dict(case["ocean"], mask=ma.embed(wet, NX, NY))
    fl = orc.compute_atmosphere_ocean_fluxes(g, params, oc, at, nthreads=0)
    net = orc.compute_net_ocean_fluxes(g, params, oc, at, fl, ice=None, weights=case["weights"])
    assert int(util.window(fl["iterations"], H, H, NX, NY, RING).max(initial=0)) < 100   # the reference converges everywhere
    return dict(fluxes=fl, net=net, wet=wet)


def _outputs(ctx, optional):
    import torch
    fill = lambda dtype, bits: util._fill(torch.empty(ctx.shape, dtype=dtype, device=ctx.device), bits)   # noqa: E731
    fl = {k: fill(torch.float64, util.SENTINEL64) for k in FLUX_NAMES + (FLUX_OPTIONAL if optional else ())}
    if optional:
        fl["iterations"] = fill(torch.int32, util.SENTINEL32)
    net = {k: fill(torch.float64, util.SENTINEL64) for k in NET_REQUIRED + (NET_DIAGNOSTICS if optional else ())}
    return fl, net


def _untouched(a):
    return a == np.int32(util.SENTINEL32) if a.dtype == np.int32 else a.view(np.uint64) == np.uint64(util.SENTINEL64)


def _host(d):
    return {k: (v if isinstance(v, np.ndarray) else v.cpu().numpy()) for k, v in d.items()}


def _check(label, fl, net, ref, oracle):
    """`fl`, `net`: the outputs of one run (device tensors or host arrays); `ref`: host copies of the three-launch reference
    (every optional output); `oracle`: _oracle(...)."""
    wet = oracle["wet"]
    for group, got, ring, want in (("fluxes", _host(fl), RING, oracle["fluxes"]), ("net", _host(net), 0, oracle["net"])):
        for k, g in got.items():
            lab = (label, group, k)
            inside = np.zeros(g.shape, bool)
            util.window(inside, H, H, NX, NY, ring)[...] = True
            left = int(_untouched(g)[inside].sum())
            assert left == 0, (lab, "cells of the footprint left unwritten", left)
            assert _untouched(g)[~inside].all(), (lab, "a cell outside the footprint was written", int((~_untouched(g)[~inside]).sum()))
            r = ref[group][k]
            same = g[inside].view(np.uint64) == r[inside].view(np.uint64) if g.dtype == np.float64 else g[inside] == r[inside]
            assert same.all(), (lab, "differs from the three-launch reference", int((~same).sum()))
            w, o = util.window(g, H, H, NX, NY, ring), util.window(want[k], H, H, NX, NY, ring)
            if k == "iterations":
                np.testing.assert_array_equal(w, o, err_msg=str(lab))
                continue
            if group == "fluxes":
                assert np.array_equal(w[~wet], o[~wet]), (lab, "land differs from the oracle")
                w, o = w[wet], o[wet]
            e = util.rel_err(w, o, util.FIELD_SCALE[k]) if w.size else 0.0
            assert e <= TOL, (lab, e)


class _Run:
    """One context per (configuration, forced reference or not) with the case's inputs on the device."""

    def __init__(self, config, reference=False):
        from coflux.runtime import FluxContext
        case = _case()
        self.ctx = ctx = FluxContext(NX, NY, H, H, _params(config), ring=RING)
        ctx.set_option(abi.OPT_AO_CHUNK, 1280)
        if reference:
            ctx.set_option(abi.OPT_FUSED_NET, 0)
            ctx.set_option(abi.OPT_LATENCY_LAYOUT, 0)
        else:
            for opt, val in CONFIGS[config]:
                ctx.set_option(opt, val)
        dev = ctx.to_device
        self.ocean = {k: dev(case["ocean"][k]) for k in ("T", "S", "u", "v")}
        self.src = {k: dev(v) for k, v in case["src"].items()}
        self.w = {k: (dev(v) if isinstance(v, np.ndarray) else v) for k, v in case["weights"].items()}

    def update(self, mask, optional, step=0, atmos=None):
        ctx = self.ctx
        fl, net = _outputs(ctx, optional)
        atmos = ctx.field_set(EXCHANGE_NAMES) if atmos is None else atmos
        l1, l2, tf = _clock(step)
        ctx.update_state(self.src, self.w, dict(self.ocean, mask=mask), atmos, fl, net, level1=l1, level2=l2, time_fraction=tf)
        ctx.sync()
        return fl, net


def _reference(ref_run, mask_np, steps=(0,)):
    """The three-launch cf_update_state with every optional output, per step: host copies (a fresh mask tensor: a fresh table)."""
    mask = ref_run.ctx.to_device(mask_np)
    out = {}
    for step in steps:
        fl, net = ref_run.update(mask, True, step)
        out[step] = dict(fluxes=_host(fl), net=_host(net))
    assert not ref_run.ctx.solver_latency_layout()
    return out


@gpu
@pytest.mark.parametrize("count", WET_COUNTS)
@pytest.mark.parametrize("config", list(CONFIGS))
def test_boundary_forms_of_one_workgroup(config, count):
    wet = wet_window(count)
    mask_np = ma.embed(wet, NX, NY)
    ref_run = _Run(config, reference=True)
    ref = _reference(ref_run, mask_np, steps=(0, 1, 2))
    line = config == "corrected_line"
    run = _Run(config)
    ctx = run.ctx
    mask = ctx.to_device(mask_np)
    # the premise: ONE workgroup holds every wet cell
    ctx.ensure_chunk_table(mask)
    begins, counts, lists_valid = ctx.debug_chunk_table()
    assert lists_valid and int(np.sum(counts)) == count and int(np.max(counts, initial=0)) == count, (counts, begins)
    assert len(counts) == 1 and begins[0] == 0 and begins[-1] == WX * WY, (counts, begins)
    orc0 = _oracle(config, count, START, 0)
    # the reference itself, against the oracle (and its own footprint)
    _check(("reference", config, count), ref[0]["fluxes"], ref[0]["net"], ref[0], orc0)
    # fused / un-fused × optional outputs × trip hints, two calls each
    for hints in (2, 0, 1, 3):
        ctx.set_option(abi.OPT_TRIP_HINTS, hints)
        for fused in (2, 0):
            ctx.set_option(abi.OPT_FUSED_NET, fused)
            for optional in (True, False):
                for call in range(2 if hints in (1, 3) else 1):
                    fl, net = run.update(mask, optional)
                    _check((config, count, "hints", hints, "fused", fused, "optional", optional, "call", call), fl, net, ref[0], orc0)
            assert ctx.solver_latency_layout() == line
    ctx.set_option(abi.OPT_TRIP_HINTS, 2)
    ctx.set_option(abi.OPT_FUSED_NET, 2)
    # tail workgroups, (a): the next state requested ahead of a host step
    ctx.set_option(abi.OPT_MERGED_PREFETCH, 2)
    sets = [ctx.field_set(EXCHANGE_NAMES) for _ in range(2)]
    before = ctx.prefetch_stats()
    for step in range(3):
        l1, l2, tf = _clock(step + 1)
        ctx.prefetch_atmosphere_state(run.src, run.w, sets[(step + 1) % 2], level1=l1, level2=l2, time_fraction=tf)
        fl, net = run.update(mask, step != 1, step, atmos=sets[step % 2])
        _check((config, count, "requested ahead, step", step), fl, net, ref[step], _oracle(config, count, START, step))
    ctx.discard_prefetched_atmosphere_state()
    moved = {k: v - before[k] for k, v in ctx.prefetch_stats().items() if v != before[k]}
    assert moved.get("launched_tail", 0) >= 2, moved     # the requests rode behind the solver's workgroups
    # (b): cf_time_steps, pipelined
    for optional in (True, False):
        fl, net = _outputs(ctx, optional)
        states = [dict(run.ocean, mask=mask)]
        sched = ctx.make_schedule(states, sets, first_level=0, time_fraction=0.0, time_fraction_increment=INC, pipeline=True)
        ctx.time_steps(0, 3, sched, run.src, run.w, fl, net)
        ctx.sync()
        _check((config, count, "cf_time_steps", "optional", optional), fl, net, ref[2], _oracle(config, count, START, 2))
    ctx.set_option(abi.OPT_MERGED_PREFETCH, 0)
    # the mask rewritten IN PLACE: the list is stale — classification; then all ocean: 2400 wet cells, the two-piece retry
    for new_count, new_start in ((count, START + 7), (None, 0)):
        new_wet = np.ones((WY, WX), bool) if new_count is None else wet_window(new_count, new_start)
        new_np = ma.embed(new_wet, NX, NY)
        mask.copy_(ctx.to_device(new_np))
        new_ref = _reference(ref_run, new_np)[0]
        orc_new = _oracle(config, new_count, new_start, 0)
        for fused in (2, 0):
            ctx.set_option(abi.OPT_FUSED_NET, fused)
            for optional in (True, False):
                fl, net = run.update(mask, optional)
                _check((config, count, "rewritten to", new_count, new_start, "fused", fused, "optional", optional), fl, net, new_ref, orc_new)
    ctx.close()
    ref_run.ctx.close()
