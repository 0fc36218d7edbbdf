"""cf_time_steps_coupled across latitude slabs (include/coflux.h: CF_HALO_PEER in the coupled form, CF_NORMALIZE_EXACT): one slab
per process over HIP IPC on the one device — the halo mailboxes between neighbours, the reduction world of the exact sums
between all ranks — against the same library on the single domain, bit for bit.

The case is tests/coupled_case.py's designed case built on the GLOBAL surface and sliced by slab_bounds: every rank holds rows
[j0 − hy, j1 + hy) of every global array, so what a neighbour must deliver is known.  Before each run the halo rows next to a
neighbour of every exchanged field are overwritten with a NaN whose payload names rank, field and row; afterwards they must hold
the neighbour's interior rows.  One spawn per world; every shape inside the workers."""
import functools
import os
import time

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import coupled_case as cc
import util
from coflux import abi
from coflux.distributed import slab_bounds

pytestmark = pytest.mark.gpu

HX, HY, ROWS, STEPS = 4, 3, 2, 7
OCEAN_FIELDS = ("T", "S", "u", "v")
ICE_FIELDS = ("concentration", "thickness", "u", "v", "albedo")     # the designed case has no snow
# measured on the MI355X: the worlds of 2, 3 and 4 ranks take 3.2, 3.6 and 3.7 s from spawn to the last join, 1.1 to 1.3 s of it
# inside the worker function (process start-up is the rest); every worker is joined under three times the slowest, killed beyond
# it and never retried
MEASURED_SECONDS = 3.7
JOIN_LIMIT = 3 * MEASURED_SECONDS
PATTERN = 0x7FF8000000000000


def shapes(world):
    """two rows per rank (= halo_rows); equal slabs of several rows; odd width and unequal slabs"""
    return [(64, 2 * world), (64, 24), (131, 37)]


@functools.lru_cache(maxsize=None)
def global_case(nx, ny_global):
    return cc.build(nx, ny_global, HX, HY)


def slab_case(nx, ny_global, rank, world):
    """rows [j0 − hy, j1 + hy) of every ocean-grid array of the global case; the sources are global"""
    g = global_case(nx, ny_global)
    j0, j1 = slab_bounds(ny_global, rank, world)
    rows = slice(j0, j1 + 2 * HY)
    cut = lambda a: np.ascontiguousarray(a[rows])  # noqa: E731
    w = dict(g["weights"])
    assert w["separable"]
    w["fj"], w["latitude"] = cut(w["fj"]), cut(w["latitude"])
    case = dict(nx=nx, ny=j1 - j0, hx=HX, hy=HY, oceans=[{k: cut(v) for k, v in o.items()} for o in g["oceans"]],
                ice_state={k: cut(v) for k, v in g["ice_state"].items()}, concentrations=[cut(c) for c in g["concentrations"]],
                x_stress=cut(g["x_stress"]), y_stress=cut(g["y_stress"]), weights=w, src=g["src"], land=g["land"], target=cut(g["target"]),
                area=cut(g["area"]), bottom_height=cut(g["bottom_height"]))
    return j0, case


def output_fields(out):
    """what the slabs are compared in: the interface fluxes of both interfaces, the net ocean and sea-ice fluxes, the ice–ocean
    fluxes, the land freshwater, the restoring buffer and the skin temperature"""
    fields = {"land": out.land, "restoring": out.restoring, "skin": out.skin}
    for name, d in (("fl", out.fl), ("ai", out.ai), ("net", out.net), ("net_ice", out.net_ice), ("iof", out.iof)):
        fields.update({f"{name}.{k}": v for k, v in d.items()})
    return fields


def exchanged_fields(rig, out):
    """{name: (device tensor, the global host array it is a slab of)} of everything the coupled loop exchanges"""
    g = global_case(rig.case["nx"], rig.ny_global)
    fields = {}
    for n, (o, go) in enumerate(zip(rig.oceans, g["oceans"])):
        fields.update({f"ocean{n}.{k}": (o[k], go[k]) for k in OCEAN_FIELDS})
    for n, st in enumerate(rig.ice_states):
        fields[f"ice{n}.concentration"] = (st["concentration"], g["concentrations"][n])
    fields.update({f"ice.{k}": (rig.ice_states[0][k], g["ice_state"][k]) for k in ICE_FIELDS if k != "concentration"})
    fields["x_stress"], fields["y_stress"] = (rig.tx, g["x_stress"]), (rig.ty, g["y_stress"])
    fields["skin"] = (out.skin, g["ice_state"]["top_temperature"])
    return fields


def stamp(fields, rank, world, ny):
    """a NaN that names rank, field and row into the halo rows next to a neighbour"""
    for f, (t, _g) in enumerate(fields.values()):
        b = t.view(torch.int64)
        for r in range(ROWS):
            if rank > 0:
                b[HY - 1 - r, :] = PATTERN | (rank << 40) | (f << 8) | r
            if rank < world - 1:
                b[HY + ny + r, :] = PATTERN | (rank << 40) | (f << 8) | 0x80 | r
    torch.cuda.synchronize()


def undelivered(fields, rank, world, j0, ny, skip=()):
    """the exchanged fields whose halo rows next to a neighbour do not hold the neighbour's interior rows.  (The skin temperature's
    ring rows are results by then: its outer exchanged row is compared, with the initial field — in a run of one call.)"""
    bad = []
    for name, (t, g) in fields.items():
        if name in skip:
            continue
        got = t.cpu().numpy().view(np.int64)
        want = g[j0:j0 + ny + 2 * HY].view(np.int64)
        sides = ([slice(HY - ROWS, HY - 1 if name == "skin" else HY)] if rank > 0 else []) + \
                ([slice(HY + ny + (1 if name == "skin" else 0), HY + ny + ROWS)] if rank < world - 1 else [])
        if any(not np.array_equal(got[s], want[s]) for s in sides):
            bad.append(name)
    return bad


def run(rig, out, calls, backend):
    import test_coupled_steps as tcs
    for first, n, pipeline in calls:
        sch, block = tcs.coupled_arguments(rig, out, pipeline=pipeline, normalize="exact")
        sch.halo_backend, sch.halo_rows = backend, ROWS if backend != abi.HALO_NONE else 0
        rig.ctx.time_steps_coupled(first, n, sch, rig.src, rig.w, out.fl, out.net, rig.stresses, block)
    rig.ctx.sync()
    rig.ctx.discard_prefetched_atmosphere_state()


def results(rig, out):
    nx, ny = rig.case["nx"], rig.case["ny"]
    fields = {k: v.cpu().numpy() for k, v in output_fields(out).items()}
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
        for nx, ny_global in shapes(world):
            j0, case = slab_case(nx, ny_global, rank, world)
            ny = case["ny"]
            rig = tcs.Rig(case, merged=2)
            rig.ny_global = ny_global
            assert connect_coupled_slabs(rig.ctx) == (rank, world)
            res = {}
            for name, calls in (("seven", [(0, STEPS, abi.PIPELINE_WITHIN_CALL)]),
                                ("five_two", [(0, 5, abi.PIPELINE_CONTINUING), (5, 2, abi.PIPELINE_CONTINUING)])):
                o = tcs.Outputs(rig)
                fields = exchanged_fields(rig, o)
                stamp(fields, rank, world, ny)
                dist.barrier()
                before = rig.ctx.peer_halo_stats()
                run(rig, o, calls, abi.HALO_PEER)          # (cf_sync: a rank that never arrived raises here)
                after = rig.ctx.peer_halo_stats()
                dist.barrier()
                res[name] = dict(results(rig, o), stats=(after[0] - before[0], after[1] - before[1]), undelivered=undelivered(fields, rank, world, j0, ny, skip=("skin",) if len(calls) > 1 else ()))
            report[(nx, ny_global)] = dict(res, j0=j0, ny=ny)
            rig.close()
        out[rank] = (report, time.perf_counter() - started)
    finally:
        dist.destroy_process_group()


_SINGLE = {}


def single_domain(nx, ny_global):
    """the same seven steps on the global case in one context: CF_HALO_NONE, the exact normalisation; once per surface"""
    import test_coupled_steps as tcs
    key = (nx, ny_global)
    if key not in _SINGLE:
        rig = tcs.Rig(global_case(nx, ny_global), merged=2)
        o = tcs.Outputs(rig)
        run(rig, o, [(0, STEPS, abi.PIPELINE_WITHIN_CALL)], abi.HALO_NONE)
        fields = {k: v.cpu().numpy() for k, v in output_fields(o).items()}
        _SINGLE[key] = (fields, float(o.mean[0]))
        rig.close()
    return _SINGLE[key]


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.int64), np.asarray(b).view(np.int64))


@pytest.mark.parametrize("world", [2, 3, 4])
def test_slabs_hold_the_single_domains_bits(world):
    """Seven pipelined steps over two ocean states and three ice states with land, restoring, the ice–ocean exchange and the exact
    normalisation, per shape and rank: the interior rows of every output equal the single-domain run's rows; the mean is the
    single domain's on every rank; the exchanged halo rows hold the neighbour's interior rows; the ring rows of the carried skin
    temperature are the neighbour's first and last interior rows after the last step; cf_peer_halo_stats grows by
    1 + 2 · nsteps per call (the stresses and the skin temperature once, nine fields per step as exchanges of eight and one);
    and 5 + 2 steps in CF_PIPELINE_CONTINUING form leave the bits of the 7.

    Join limit: three times the 3.7 s the slowest world takes from spawn to join on the MI355X (MEASURED_SECONDS), 11.1 s; the test
    prints what it took."""
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
        want, want_mean = single_domain(nx, ny_global)
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
            if r < world - 1:
                assert same_bits(seven["ring"][1], want["skin"][HY + j0 + ny, cols]), (label, "north ring row of the skin temperature")
            assert seven["stats"] == (1 + 2 * STEPS, 0) and split["stats"] == (2 + 2 * STEPS, 0), (label, seven["stats"], split["stats"])
            differing = [k for k in seven["interior"] if not same_bits(seven["interior"][k], split["interior"][k])]
            assert not differing and same_bits(split["mean"], seven["mean"]), (label, "5 + 2 steps differ from 7 in", differing)
