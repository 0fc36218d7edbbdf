"""cf_time_steps on px × py tile worlds (include/coflux.h: "Tile worlds"): one tile per PROCESS over HIP IPC on the one device,
five pipelined steps over two ocean states under CF_HALO_PEER — per step the x-phase, the y-phase and, on the top row of the
tripolar surface, the fold sent to the partner tile — against the single-domain run of the library on the same surface
(CF_HALO_NONE, caller-periodic x-halos, fold_north on the tripolar case: an existing, tested path), bit for bit on the interior of
every field of `fluxes` and `net` of every rank.  The tripolar tiles are the cuts of coflux.synthetic.tripolar_case, the others
of the latitude–longitude case.  Every halo cell an exchange must deliver is NaN before the run.

Before its valid run on each surface every rank makes the calls cf_time_steps refuses on a tile world — fold_north that disagrees
with its place, CF_HALO_RCCL: CF_ERR_INVALID naming the field, nothing counted, and the valid run that follows holds the single
domain's bits as if they had not been made.  The same refusals and a mailbox too small run on a world of one in this process;
cf_time_steps_coupled's refusal of a world two tiles wide in a spawn of two."""
import ctypes as C
import functools
import os
import time

import numpy as np
import pytest

import util
from coflux import abi
from coflux import interface_computations as ic
from coflux import synthetic as syn
from coflux.distributed import tile_bounds, tile_coords

pytestmark = pytest.mark.gpu

H, RING, STEPS = 5, 1, 5
ROWS = RING + 1
INC = 1200.0 / 10800.0
FIELDS = ("T", "S", "u", "v")
WORLDS = [(2, 1), (2, 2), (4, 1)]
ERR_INVALID = -1
# measured on the MI355X: the worlds (2,1), (2,2) and (4,1) take 3.8, 4.4 and 4.7 s from spawn to the last join, 1.6 to 1.9 s of it
# inside the worker function (process start-up is the rest), the coupled refusal's two processes 3.1 s; every worker is joined
# under three times the slowest, killed beyond it and never retried
MEASURED_SECONDS = 4.7
JOIN_LIMIT = 3 * MEASURED_SECONDS


def surfaces(py):
    """global (nx, ny): 64 × 24; 68 × 37 — unequal row blocks, nxl / 2 odd on two columns of tiles, nxl odd on four —; and three
    rows per top-row rank, the least the fold admits"""
    return [(64, 24), (68, 37), (64, 3 * py)]


def _params():
    return ic.flux_params(ic.corrected_atmosphere_ocean_fluxes(), ocean_surface=ic.SurfaceRadiationProperties(0.06, 1.0))


@functools.lru_cache(maxsize=None)
def global_case(grid, nx, ny):
    """two ocean states a step apart, the weights and the source on the whole surface; never written to"""
    if grid == "tripolar":
        case = syn.tripolar_case(nx, ny, H, H)
        first = case["ocean"]
        evolved = syn.evolved_ocean_state(syn.ocean_state(nx, ny, H, H, latitude=(-80.0, 90.0)), nx, ny, H, H, 1)
        second = {}
        for k in FIELDS:
            second[k] = syn.fold_north(evolved[k].copy(), nx, ny, H, H, ROWS, syn.FOLD_LOCATION[k], syn.FOLD_SIGN[k])
        return [first, second], case["weights"], case["src"]
    first = syn.ocean_state(nx, ny, H, H)
    second = syn.evolved_ocean_state(first, nx, ny, H, H, 1)
    fi, fj, phi = syn.latlon_fractional_indices(nx, ny, H, H)
    return [first, second], dict(separable=True, fi=fi, fj=fj, latitude=phi), syn.jra55_snapshots(2)


def tile_case(grid, nx, ny, i0, i1, j0, j1):
    """the tile's two states, weights and source through the tile cuts of coflux.synthetic"""
    if grid == "tripolar":
        case = syn.tripolar_tile_case(nx, ny, H, H, i0=i0, i1=i1, j0=j0, j1=j1)
        second = {k: np.ascontiguousarray(global_case(grid, nx, ny)[0][1][k][j0:j1 + 2 * H, i0:i1 + 2 * H]) for k in FIELDS}
        return [dict(case["ocean"]), second], case["weights"], case["src"]
    cases = [syn.latlon_tile_case(nx, ny, H, H, i0=i0, i1=i1, j0=j0, j1=j1, step=s) for s in (0, 1)]
    return [dict(c["ocean"]) for c in cases], cases[0]["weights"], cases[0]["src"]


def _poison(states, px, py, p, q, nxl, ny, fold):
    """NaN into every halo cell a neighbour, the partner or the fold must deliver: the x-halo columns (px > 1) and the halo rows
    towards a neighbour or the fold, corners included; what lies beyond the world's south edge, or its north edge without a
    fold, is nobody's and stays"""
    lo = 0 if q > 0 else H
    hi = ny + 2 * H if (q < py - 1 or fold) else ny + H
    for st in states:
        for k in FIELDS:
            a = st[k] = np.array(st[k])
            if px > 1:
                a[lo:hi, :H] = np.nan
                a[lo:hi, H + nxl:] = np.nan
            a[lo:H] = np.nan
            a[H + ny:hi] = np.nan


class _Run:
    """one context on a case, its inputs on the device, fresh outputs per run"""

    def __init__(self, nx, ny, states, weights, src):
        from coflux.runtime import EXCHANGE_NAMES, FluxContext
        self.ctx = ctx = FluxContext(nx, ny, H, H, _params(), ring=RING)
        self.states = [{k: ctx.to_device(s[k]) for k in FIELDS} for s in states]
        mask = ctx.to_device(states[0]["mask"])
        for st in self.states:
            st["mask"] = mask
        self.src = {k: ctx.to_device(v) for k, v in src.items()}
        self.w = {k: (ctx.to_device(v) if isinstance(v, np.ndarray) else v) for k, v in weights.items()}
        self.sets = [ctx.field_set(EXCHANGE_NAMES) for _ in range(2)]
        self.outputs()

    def outputs(self):
        from coflux.runtime import FLUX_NAMES, NET_NAMES
        self.fl, self.net = self.ctx.field_set(FLUX_NAMES), self.ctx.field_set(NET_NAMES)

    def schedule(self, backend, fold):
        return self.ctx.make_schedule(self.states, self.sets, time_fraction_increment=INC, pipeline=True, halo_backend=backend,
                                      halo_rows=ROWS if backend != abi.HALO_NONE else 0, fold_north=fold)

    def steps_raw(self, backend, fold):
        """(return code, message) of five steps of cf_time_steps"""
        ctx = self.ctx
        sched, s, w = self.schedule(backend, fold), ctx.source_struct(self.src, 0, 0, 0.0), ctx.weights_struct(self.w)
        f, n = ctx.fluxes_struct(self.fl), ctx.net_struct(self.net)
        rc = ctx.lib.cf_time_steps(ctx._h, 0, STEPS, C.byref(sched), C.byref(s), C.byref(w), C.byref(f), None, C.byref(n))
        return rc, ctx.lib.cf_last_error(ctx._h).decode()

    def interior(self):
        nx, ny = self.ctx.grid.nx, self.ctx.grid.ny
        out = {"fl." + k: v for k, v in self.fl.items()} | {"net." + k: v for k, v in self.net.items()}
        return {k: np.ascontiguousarray(v.cpu().numpy()[H:H + ny, H:H + nx]) for k, v in out.items()}

    def counters(self):
        return self.ctx.tile_stats() + self.ctx.fold_counts() + self.ctx.peer_halo_stats()


@functools.lru_cache(maxsize=None)
def single_domain(grid, nx, ny):
    """the five steps on the whole surface in one context, once per surface: {field: interior}"""
    states, weights, src = global_case(grid, nx, ny)
    run = _Run(nx, ny, states, weights, src)
    rc, text = run.steps_raw(abi.HALO_NONE, grid == "tripolar")
    assert rc == 0, text
    run.ctx.sync()
    fields = run.interior()
    run.ctx.close()
    assert all(np.isfinite(v).all() for v in fields.values()) and np.abs(fields["fl.x_momentum"]).max() > 0   # a run, not a trace of NaNs
    return fields


def _refused(run, backend, fold, words, problems, label):
    """a call cf_time_steps must refuse: CF_ERR_INVALID with `words`, no counter moved"""
    before = run.counters()
    rc, text = run.steps_raw(backend, fold)
    if rc != ERR_INVALID or any(w not in text for w in words):
        problems.append((label, "not refused by name", rc, text))
    if run.counters() != before:
        problems.append((label, "something was counted", before, run.counters()))


def _worker(rank, world, init, out, px, py):
    import torch
    import torch.distributed as dist
    from coflux.distributed import connect_tiles
    from coflux.runtime import CofluxError
    started = time.perf_counter()
    os.environ.update(HSA_ENABLE_IPC_MODE_LEGACY="0")
    dist.init_process_group("gloo", init_method=init, rank=rank, world_size=world)
    try:
        report = dict(fields={}, grown={}, problems=[], error=None)
        p, q = tile_coords(rank, px)
        for grid in ("tripolar", "latlon"):
            tripolar = grid == "tripolar"
            fold = tripolar and q == py - 1
            for nx, ny_global in surfaces(py):
                label = (grid, nx, ny_global)
                i0, i1, j0, j1 = tile_bounds(nx, ny_global, rank, px, py)
                nxl, ny = i1 - i0, j1 - j0
                states, weights, src = tile_case(grid, nx, ny_global, i0, i1, j0, j1)
                _poison(states, px, py, p, q, nxl, ny, fold)
                run = _Run(nxl, ny, states, weights, src)
                connect_tiles(run.ctx, px, py, tripolar)
                # refused before the first launch: the context is as it was, on every rank
                _refused(run, abi.HALO_PEER, not fold, ("cf_time_steps", "fold_north"), report["problems"], label)
                _refused(run, abi.HALO_RCCL, fold, ("cf_time_steps", "CF_HALO_RCCL"), report["problems"], label)
                torch.cuda.synchronize()
                dist.barrier()
                before = run.counters()
                rc, text = run.steps_raw(abi.HALO_PEER, fold)
                if rc != 0:
                    report["error"] = (label, text)
                    break
                try:
                    run.ctx.sync()
                except CofluxError as e:   # CF_ERR_COMM: somebody never arrived.  Nothing more is started on the device.
                    report["error"] = (label, str(e))
                    break
                report["grown"][label] = tuple(a - b for a, b in zip(run.counters(), before))
                report["fields"][label] = dict(run.interior(), bounds=(i0, i1, j0, j1))
                dist.barrier()              # a mailbox outlives its neighbours' last exchange
                run.ctx.close()
            if report["error"] is not None:
                break
        report["seconds"] = time.perf_counter() - started
        out[rank] = report
    finally:
        dist.destroy_process_group()


def _run_workers(target, world, *args):
    import torch.multiprocessing as mp
    ctxm = mp.get_context("spawn")
    out = ctxm.Manager().dict()
    init = util.rendezvous()
    procs = [ctxm.Process(target=target, args=(r, world, init, out) + args) for r in range(world)]
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
    reports = {r: out.get(r) for r in range(world)}
    assert codes == [0] * world, (f"worker exit codes {codes} (None: still running after {JOIN_LIMIT} s)",
                                  {r: (rep or {}).get("error") for r, rep in reports.items()})
    return reports, time.perf_counter() - started


@pytest.mark.parametrize("px,py", WORLDS)
def test_tile_worlds_hold_the_single_domains_bits(px, py):
    """Per surface and rank: the interior of every field of `fluxes` and `net` equals the same columns and rows of the
    single-domain run; cf_peer_tile_stats grows by (5, 5, 5 where the rank sends a fold); no rank launches the fold's own kernel
    and no slab exchange is counted; the refused calls in front of the run left no trace.

    Join limit: three times MEASURED_SECONDS; the test prints what the world took.  With the parent, at most five processes
    hold the GPU."""
    world = px * py
    reports, seconds = _run_workers(_worker, world, px, py)
    print(f"{px} x {py} world: {seconds:.1f} s from spawn to join, of which in the worker function", [round(reports[r]["seconds"], 1) for r in range(world)])
    for grid in ("tripolar", "latlon"):
        for nx, ny_global in surfaces(py):
            want = single_domain(grid, nx, ny_global)
            for r in range(world):
                rep = reports[r]
                assert rep["error"] is None, (r, rep["error"])
                assert not rep["problems"], (r, rep["problems"])
                label = (grid, nx, ny_global)
                got = rep["fields"][label]
                i0, i1, j0, j1 = got["bounds"]
                for k, ref in want.items():
                    same = got[k].view(np.uint8) == np.ascontiguousarray(ref[j0:j1, i0:i1]).view(np.uint8)
                    assert same.all(), (label, "rank", r, k, "differs from the single-domain run in", int((~same).sum()), "of", same.size, "bytes")
                sends_fold = grid == "tripolar" and r // px == py - 1
                assert rep["grown"][label] == (STEPS, STEPS, STEPS if sends_fold else 0, 0, 0, 0, 0), (label, r, rep["grown"][label])


# ---------------------------------------------------------------------------------------------
# refusals in a world of one (this process) and of the coupled loop in a world of two
# ---------------------------------------------------------------------------------------------
def _world_of_one(grid, nx, ny, **export):
    states, weights, src = global_case(grid, nx, ny)
    states = [dict(s) for s in states]
    _poison(states, 1, 1, 0, 0, nx, ny, grid == "tripolar")
    run = _Run(nx, ny, states, weights, src)
    run.ctx.peer_tile_connect([run.ctx.peer_tile_export(**export)], 1, 1, 0, grid == "tripolar")
    return run


ONE = {
    "fold_missing_on_the_tripolar_world": ("tripolar", {}, abi.HALO_PEER, False, ("fold_north = 0", "tripolar")),
    "fold_on_the_latlon_world": ("latlon", {}, abi.HALO_PEER, True, ("fold_north = 1", "latitude-longitude")),
    "rccl": ("tripolar", {}, abi.HALO_RCCL, True, ("CF_HALO_RCCL", "tile world")),
    "mailbox_of_three_fields": ("tripolar", dict(max_fields=3), abi.HALO_PEER, True, ("tile mailbox", "3 fields", "4 fields")),
    "mailbox_of_one_row": ("latlon", dict(max_rows=1), abi.HALO_PEER, False, ("tile mailbox", "1 rows", "2 rows")),
}


@pytest.mark.parametrize("name", list(ONE))
def test_a_refused_step_call_on_a_world_of_one_leaves_no_trace(name):
    """px = py = 1: nobody to wait for, the x-halos stay the caller's and the tripolar fold is the rank's own.  The refused call
    returns CF_ERR_INVALID naming the field and moves no counter; the valid call that follows (on a mailbox that takes it)
    holds the single domain's bits, with one exchange and — tripolar — one fold launch per step."""
    grid, export, backend, fold, words = ONE[name]
    nx, ny = 64, 24
    run = _world_of_one(grid, nx, ny, **export)
    problems = []
    _refused(run, backend, fold, ("cf_time_steps",) + words, problems, name)
    assert not problems, problems
    if export:
        run.ctx.close()
        run = _world_of_one(grid, nx, ny)
    before = run.counters()
    rc, text = run.steps_raw(abi.HALO_PEER, grid == "tripolar")
    assert rc == 0, text
    run.ctx.sync()
    folds = STEPS if grid == "tripolar" else 0
    assert tuple(a - b for a, b in zip(run.counters(), before)) == (STEPS, 0, 0, folds, 0, 0, 0)
    want = single_domain(grid, nx, ny)
    got = run.interior()
    for k, ref in want.items():
        assert np.array_equal(got[k].view(np.uint8), ref.view(np.uint8)), (name, k)
    run.ctx.close()


def _coupled_worker(rank, world, init, out):
    import torch.distributed as dist
    import coupled_fold_case as fc
    import test_coupled_steps as tcs
    from coflux.distributed import connect_tiles
    from coflux.runtime import CofluxError
    started = time.perf_counter()
    os.environ.update(HSA_ENABLE_IPC_MODE_LEGACY="0")
    dist.init_process_group("gloo", init_method=init, rank=rank, world_size=world)
    try:
        problems = []
        _j0, case = fc.slab_case(32, 12, 0, 1)     # (every rank holds the same 32 × 12 tile: nothing is exchanged)
        rig = fc.make_rig(case)
        connect_tiles(rig.ctx, 2, 1, True, max_fields=8)
        o = tcs.Outputs(rig)
        bits = {k: v.clone() for k, v in fc.output_fields(o).items()}
        for backend in (abi.HALO_PEER, abi.HALO_NONE):
            before = rig.ctx.tile_stats() + fc.counters(rig.ctx)
            sch, block = tcs.coupled_arguments(rig, o, pipeline=abi.PIPELINE_WITHIN_CALL, normalize="exact")
            sch.halo_backend, sch.halo_rows, sch.fold_north = backend, fc.ROWS if backend else 0, 1
            try:
                rig.ctx.time_steps_coupled(0, 2, sch, rig.src, rig.w, o.fl, o.net, rig.stresses, block)
                problems.append((backend, "not refused"))
            except CofluxError as e:
                if "(-1)" not in str(e) or "cf_time_steps_coupled" not in str(e) or "px = 2" not in str(e):
                    problems.append((backend, "not refused by name", str(e)))
            if rig.ctx.tile_stats() + fc.counters(rig.ctx) != before:
                problems.append((backend, "something was counted"))
        rig.ctx.sync()
        import torch
        for k, v in fc.output_fields(o).items():
            if not torch.equal(v.view(torch.int64), bits[k].view(torch.int64)):
                problems.append(("an output was written", k))
        # … and the tile world is still there: one exchange of the four ocean fields with the fold sent to the other rank
        fields = [rig.oceans[0][k] for k in fc.OCEAN_FIELDS]
        rig.ctx.halo_exchange_tile_peer(fields, [abi.FOLD_CENTER, abi.FOLD_CENTER, abi.FOLD_X_FACE, abi.FOLD_Y_FACE], [1.0, 1.0, -1.0, -1.0],
                                        rows=fc.ROWS, fold_north=True)
        rig.ctx.sync()
        if rig.ctx.tile_stats() != (1, 1, 1):
            problems.append(("the exchange after the refusals", rig.ctx.tile_stats()))
        out[rank] = dict(problems=problems, error=None, seconds=time.perf_counter() - started)
        dist.barrier()
        rig.close()
    finally:
        dist.destroy_process_group()


def test_the_coupled_loop_refuses_a_world_two_tiles_wide_by_name():
    """cf_time_steps_coupled on a context connected to a (2,1) world, under CF_HALO_PEER and CF_HALO_NONE: CF_ERR_INVALID naming
    px, before anything is launched — no output written, no counter moved —, and the tile exchange that follows runs."""
    reports, seconds = _run_workers(_coupled_worker, 2)
    print(f"coupled refusal across two processes: {seconds:.1f} s from spawn to join")
    for r in range(2):
        assert reports[r]["problems"] == [], (r, reports[r]["problems"])
