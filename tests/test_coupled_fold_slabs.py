"""cf_time_steps_coupled across latitude slabs of a TRIPOLAR surface (include/coflux.h: "Tripolar slabs"): one slab per process
over HIP IPC on the one device, the last rank passing fold_north = 1 — its exchanges fold their own fields as their north side —
against the single-domain tripolar reference of tests/coupled_fold_case.py, bit for bit.

Every rank holds rows [j0 − hy, j1 + hy) of every global array.  Before each run the halo rows towards a neighbour and towards the
fold of all thirteen exchanged fields are overwritten with NaNs whose payload names rank, field and row; afterwards they must
hold the neighbour's interior rows, or the host fold of the global rows.  One spawn per world; every shape inside the workers."""
import os
import time

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

import coupled_fold_case as fc
import util
from coflux import abi

pytestmark = pytest.mark.gpu

HX, HY, STEPS = fc.HX, fc.HY, fc.STEPS
# measured on the MI355X: the worlds of 2, 3 and 4 ranks take 3.3, 3.5 and 3.7 s from spawn to the last join, 1.1 to 1.3 s of it
# inside the worker function (process start-up is the rest); every worker is joined under three times the slowest, killed beyond
# it and never retried
MEASURED_SECONDS = 3.7
JOIN_LIMIT = 3 * MEASURED_SECONDS


def shapes(world):
    """three rows per rank (= ring + 2, the least the fold admits on the last); equal slabs of several rows; nx / 2 odd, unequal slabs"""
    return [(64, 3 * world), (64, 24), (130, 37)]


def results(rig, out):
    nx, ny = rig.case["nx"], rig.case["ny"]
    fields = {k: v.cpu().numpy() for k, v in fc.output_fields(out).items()}
    return dict(interior={k: np.ascontiguousarray(v[HY:HY + ny, HX:HX + nx]) for k, v in fields.items()},
                ring=(fields["skin"][HY - 1, HX - 1:HX + nx + 1].copy(), fields["skin"][HY + ny, HX - 1:HX + nx + 1].copy()),
                mean=float(out.mean[0]))


def _worker(rank, world, init, out):
    import test_coupled_steps as tcs
    from coflux.distributed import connect_coupled_slabs
    started = time.perf_counter()
    os.environ.update(HSA_ENABLE_IPC_MODE_LEGACY="0")
    dist.init_process_group("gloo", init_method=init, rank=rank, world_size=world)
    try:
        report = {}
        last = rank == world - 1
        for nx, ny_global in shapes(world):
            j0, case = fc.slab_case(nx, ny_global, rank, world)
            ny = case["ny"]
            rig = fc.make_rig(case)
            assert connect_coupled_slabs(rig.ctx) == (rank, world)
            res = {}
            for name, calls in (("seven", fc.SEVEN), ("five_two", fc.FIVE_TWO)):
                o = tcs.Outputs(rig)
                fields = fc.exchanged_fields(rig, o, nx, ny_global)
                fc.stamp(fields, rank, world, ny)
                dist.barrier()
                before = fc.counters(rig.ctx)
                fc.run(rig, o, calls, abi.HALO_PEER, last)          # (cf_sync: a rank that never arrived raises here)
                grown = fc.grown(before, fc.counters(rig.ctx))
                dist.barrier()
                res[name] = dict(results(rig, o), grown=grown,
                                 undelivered=fc.undelivered(fields, rank, j0, ny, skip=("skin",) if len(calls) > 1 else ()))
            report[(nx, ny_global)] = dict(res, j0=j0, ny=ny)
            rig.close()
        out[rank] = (report, time.perf_counter() - started)
    finally:
        dist.destroy_process_group()


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.int64), np.asarray(b).view(np.int64))


@pytest.mark.parametrize("world", [2, 3, 4])
def test_tripolar_slabs_hold_the_single_domains_bits(world):
    """Seven pipelined steps over two ocean states and three ice states with snow, land, restoring, the ice–ocean exchange and the
    exact normalisation, per shape and rank: the interior rows of every output equal the single-domain tripolar run's rows; the
    mean is the single domain's on every rank; the stamped halo rows hold the neighbour's interior rows or, on the last rank, the
    host fold of the global rows, full width; the ring rows of the carried skin temperature are the neighbour's first and last
    interior rows — on the last rank the single domain's row ny beyond the fold; cf_peer_halo_stats grows by 1 + 2 · nsteps per
    call on every rank (ten fields per step as exchanges of eight and two), no rank launches the fold's own kernel, and only
    the last rank's exchanges carry a fold, all of them; 5 + 2 steps in CF_PIPELINE_CONTINUING form leave the bits of the 7.

    Join limit: three times the 3.7 s the slowest world takes from spawn to join on the MI355X (MEASURED_SECONDS), 11.1 s; the test
    prints what it took.  With the parent, at most five processes hold the GPU."""
    ctxm = mp.get_context("spawn")
    out = ctxm.Manager().dict()
    init = util.rendezvous()
    procs = [ctxm.Process(target=_worker, args=(r, world, init, out)) for r in range(world)]
    started = time.perf_counter()
    for p in procs:
        p.start()
    try:
        for p in procs:
            p.join(JOIN_LIMIT)
        codes = [p.exitcode for p in procs]
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    assert codes == [0] * world, f"slab worker exit codes {codes} (None: still running at the join limit of {JOIN_LIMIT} s)"
    print(f"{world} workers: {time.perf_counter() - started:.1f} s from spawn to join, of which in the worker function",
          [round(out[r][1], 1) for r in range(world)])
    reports = [out[r][0] for r in range(world)]
    for nx, ny_global in shapes(world):
        single = fc.single_domain(nx, ny_global)
        want, want_mean = single["fields"], single["mean"]
        for r in range(world):
            rep = reports[r][(nx, ny_global)]
            j0, ny = rep["j0"], rep["ny"]
            label = f"{nx} x {ny_global}, rank {r} of {world} (rows {j0} … {j0 + ny - 1})"
            seven, split = rep["seven"], rep["five_two"]
            for k, rows in seven["interior"].items():
                ref = want[k][HY + j0:HY + j0 + ny, HX:HX + nx]
                same = rows.view(np.int64) == ref.view(np.int64)
                assert same.all(), (label, k, "differs from the single-domain run in", int((~same).sum()), "of", same.size, "cells")
            assert same_bits(seven["mean"], want_mean), (label, seven["mean"], want_mean)
            assert not seven["undelivered"] and not split["undelivered"], (label, seven["undelivered"], split["undelivered"])
            cols = slice(HX - 1, HX + nx + 1)
            if r > 0:
                assert same_bits(seven["ring"][0], want["skin"][HY + j0 - 1, cols]), (label, "south ring row of the skin temperature")
            assert same_bits(seven["ring"][1], want["skin"][HY + j0 + ny, cols]), (label, "north ring row of the skin temperature")
            folds = lambda calls: (1 + 2 * STEPS + calls - 1) if r == world - 1 else 0  # noqa: E731
            assert seven["grown"] == (1 + 2 * STEPS, 0, 0, folds(1)) and split["grown"] == (2 + 2 * STEPS, 0, 0, folds(2)), \
                (label, seven["grown"], split["grown"])
            differing = [k for k in seven["interior"] if not same_bits(seven["interior"][k], split["interior"][k])]
            assert not differing and same_bits(split["mean"], seven["mean"]), (label, "5 + 2 steps differ from 7 in", differing)
