"""cf_halo_exchange_tile_peer on px × py worlds (include/coflux.h: cf_peer_tile_*): one rank per PROCESS over HIP IPC on the one
device, gloo for the host side, one spawn per world with every shape inside the workers.  Worlds (2,1), (2,2) and (4,1) — in
(4,1) the fold partner of ranks 1 and 2 is neither of their x-neighbours —, each as a latitude–longitude world (no fold) and as a
tripolar one, on the three per-tile shapes of tests/tile_case.py, with 1, 4 and 8 origin-stamped fields in three consecutive
exchanges (both mailbox parities, the first one twice).

Every rank holds eight fields as views at an odd element offset inside guarded buffers; every halo cell is poisoned with a
pattern that names rank, field and cell.  After each exchange, over WHOLE buffers, guards included: the exchanged fields hold
what the plain NumPy exchange (coflux.distributed.exchange_tile_halos_reference) leaves of the same tiles — so the cells outside
the documented footprint hold what the header says: untouched, or the sender's own poison where rows travel full width —, the
fields not passed are untouched, and on the ring + 1 footprint every cell holds the GLOBAL array's bits (periodic x,
coflux.synthetic.fold_north beyond the top row).  cf_peer_tile_stats grows by (1, px > 1, fold sent) per exchange.

Also, launching nothing: every refusal of cf_peer_tile_connect, in a world of one and — where a neighbour's mailbox is read —
across two processes."""
import ctypes as C
import os
import time

import numpy as np
import pytest

import tile_case as tc
import util
from coflux import abi
from coflux.distributed import tile_bounds, tile_coords

pytestmark = pytest.mark.gpu

WORLDS = [(2, 1), (2, 2), (4, 1)]
FIELD_COUNTS = (1, 4, 8)
# measured on the MI355X: the worlds (2,1), (2,2) and (4,1) take 2.4, 2.7 and 2.6 s from spawn to the last join, 0.3 to 0.5 s of it
# inside the worker function (process start-up is the rest); every worker is joined under three times the slowest, killed beyond
# it and never retried
MEASURED_SECONDS = 2.7
JOIN_LIMIT = 3 * MEASURED_SECONDS
GUARD = 64
ERR_INVALID, ERR_COMM = -1, -4
LOCATION = {"center": abi.FOLD_CENTER, "x_face": abi.FOLD_X_FACE, "y_face": abi.FOLD_Y_FACE}


def _images(fields):
    import torch
    return [util.buffer_of(t)[0].view(torch.int64).cpu().numpy().copy() for t in fields]


def _expected_image(t, array):
    flat, start = util.buffer_of(t)
    image = np.full(flat.numel(), np.array([util.SENTINEL64], np.uint64).view(np.int64)[0], np.int64)
    image[start:start + t.numel()] = np.ascontiguousarray(array).view(np.int64).reshape(-1)
    return image


def _worker(rank, world, init, out, px, py):
    import torch
    import torch.distributed as dist
    from coflux import interface_computations as ic
    from coflux.distributed import connect_tiles, exchange_tile_halos_reference
    from coflux.runtime import CofluxError, FluxContext
    started = time.perf_counter()
    os.environ.update(HSA_ENABLE_IPC_MODE_LEGACY="0")
    dist.init_process_group("gloo", init_method=init, rank=rank, world_size=world)
    try:
        report = dict(failures=[], grown={}, error=None)
        p, q = tile_coords(rank, px)
        nall = len(tc.FIELDS)
        locations, signs = [LOCATION[loc] for loc, _ in tc.FIELDS], [sg for _, sg in tc.FIELDS]
        for tripolar in (False, True):
            for nxl, nyg in tc.shapes(py):
                nxg = px * nxl
                case = ("tripolar" if tripolar else "latlon", nxl, nyg)
                i0, i1, j0, j1 = tile_bounds(nxg, nyg, rank, px, py)
                ny = j1 - j0
                ctx = FluxContext(nxl, ny, tc.HX, tc.HY, ic.flux_params(), ring=tc.RING)
                assert connect_tiles(ctx, px, py, tripolar, max_fields=nall) == (rank, p, q)
                shape = (ny + 2 * tc.HY, nxl + 2 * tc.HX)
                fields = [util.guarded(shape, torch.float64, offset=1, guard=GUARD, fill=util.SENTINEL64) for _ in range(nall)]
                fold = tripolar and q == py - 1
                rows, cols = tc.defined_window(rank, px, py, ny, tripolar)
                for call, nfields in enumerate(FIELD_COUNTS):
                    glob = tc.global_fields(nxg, nyg, nall, tripolar, call)
                    tiles = tc.cut_tiles(glob, nxg, nyg, px, py)
                    for t, a in zip(fields, tiles[rank]):
                        t.view(torch.int64).copy_(torch.from_numpy(a.view(np.int64)))
                    torch.cuda.synchronize()
                    before = ctx.tile_stats()
                    try:   # every rank makes the same calls in the same order: no barrier in between
                        ctx.halo_exchange_tile_peer(fields[:nfields], locations[:nfields], signs[:nfields], rows=tc.ROWS, fold_north=fold)
                        ctx.sync()
                    except CofluxError as e:   # CF_ERR_COMM: somebody never arrived.  Nothing more is started on the device.
                        report["error"] = (case, nfields, str(e))
                        break
                    report["grown"][case + (nfields,)] = tuple(a - b for a, b in zip(ctx.tile_stats(), before))
                    want = [[a.copy() for a in mine[:nfields]] for mine in tiles]
                    exchange_tile_halos_reference(want, px, py, tc.HX, tc.HY, ring=tc.RING, rows=tc.ROWS, tripolar=tripolar,
                                                  locations=[loc for loc, _ in tc.FIELDS[:nfields]], signs=signs[:nfields])
                    got = _images(fields)
                    for f in range(nall):
                        array = want[rank][f] if f < nfields else tiles[rank][f]
                        image = _expected_image(fields[f], array)
                        start = util.buffer_of(fields[f])[1]
                        for k in np.flatnonzero(got[f] != image)[:4]:
                            report["failures"].append((case, nfields, "field", f, "element of the view", int(k) - start,
                                                       got[f][k:k + 1].view(np.float64)[0], image[k:k + 1].view(np.float64)[0]))
                        if f < nfields:   # … and the reference itself is the global array on the footprint
                            held = got[f][start:start + fields[f].numel()].reshape(shape)
                            wanted = glob[f][j0:j1 + 2 * tc.HY, i0:i1 + 2 * tc.HX].view(np.int64)
                            if not np.array_equal(held[rows, cols], wanted[rows, cols]):
                                report["failures"].append((case, nfields, "field", f, "differs from the global array on the footprint"))
                if report["error"] is not None:
                    break
                dist.barrier()                      # a mailbox outlives its neighbours' last exchange
                ctx.close()
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
    assert codes == [0] * world, (f"worker exit codes {codes} (None: still running after {JOIN_LIMIT} s)", reports)
    return reports, time.perf_counter() - started


@pytest.mark.parametrize("px,py", WORLDS)
def test_tile_exchange_leaves_the_global_arrays_bits_in_whole_guarded_buffers(px, py):
    """Join limit: three times MEASURED_SECONDS; the test prints what the world took.  With the parent, at most five processes
    hold the GPU."""
    world = px * py
    reports, seconds = _run_workers(_worker, world, px, py)
    print(f"{px} x {py} world: {seconds:.1f} s from spawn to join, of which in the worker function", [round(reports[r]["seconds"], 1) for r in range(world)])
    for r in range(world):
        rep = reports[r]
        assert rep["error"] is None, (r, rep["error"])
        assert not rep["failures"], (r, rep["failures"][:12])
        _p, q = tile_coords(r, px)
        cases = 0
        for (grid, nxl, nyg, nfields), grown in rep["grown"].items():
            sends_fold = grid == "tripolar" and q == py - 1
            assert grown == (1, 1, 1 if sends_fold else 0), (r, grid, nxl, nyg, nfields, grown)
            cases += 1
        assert cases == 2 * len(tc.shapes(py)) * len(FIELD_COUNTS)


# ---------------------------------------------------------------------------------------------
# launching nothing: cf_peer_tile_connect refuses
# ---------------------------------------------------------------------------------------------
def _context(nx=6, ny=4, max_fields=4, max_rows=tc.ROWS, max_cols=tc.COLS + 1):
    from coflux import interface_computations as ic
    from coflux.runtime import FluxContext
    ctx = FluxContext(nx, ny, tc.HX, tc.HY, ic.flux_params(), ring=tc.RING)
    return ctx, ctx.peer_tile_export(max_fields, max_rows, max_cols)


def _connect_raw(ctx, handles, px, py, rank, tripolar):
    blob = C.create_string_buffer(b"".join(handles), len(handles) * abi.PEER_HANDLE_BYTES) if handles else None
    rc = ctx.lib.cf_peer_tile_connect(ctx._h, blob, px, py, rank, tripolar)
    return rc, ctx.lib.cf_last_error(ctx._h).decode()


def _is_unconnected(ctx):
    """an exchange answers as if cf_peer_tile_connect had not been called, and counts nothing"""
    import torch
    t = torch.zeros((ctx.grid.ny + 2 * tc.HY, ctx.grid.nx + 2 * tc.HX), dtype=torch.float64, device="cuda")
    arr = (C.c_void_p * 1)(t.data_ptr())
    before = ctx.tile_stats()
    rc = ctx.lib.cf_halo_exchange_tile_peer(ctx._h, arr, None, None, 1, 1, 0)
    return rc == ERR_COMM and "has not been called" in ctx.lib.cf_last_error(ctx._h).decode() and ctx.tile_stats() == before == (0, 0, 0)


# (px, py, rank, tripolar, nx of the context) and words of the message
WORLD_REFUSALS = {
    "px_zero": ((0, 1, 0, 0, 6), "px = 0"),
    "py_zero": ((1, 0, 0, 0, 6), "py = 0"),
    "rank_beyond_the_world": ((2, 2, 4, 0, 6), "rank = 4"),
    "rank_negative": ((2, 2, -1, 0, 6), "rank = -1"),
    "px_odd": ((3, 1, 0, 0, 6), "px = 3"),
    "more_ranks_than_the_exact_mean_takes": ((2, 5, 0, 0, 6), "px = 2, py = 5"),
    "tripolar_with_odd_global_nx": ((1, 1, 0, 1, 7), "odd global Nx"),
}


@pytest.mark.parametrize("name", list(WORLD_REFUSALS))
def test_connect_refuses_a_world_it_does_not_step(name):
    """CF_ERR_INVALID naming the argument; nothing is mapped or launched, the context is left unconnected, and the valid connect
    that follows (a world of one) exchanges: on the tripolar one its north halo is the fold of its own rows."""
    import torch
    (px, py, rank, tripolar, nx), words = WORLD_REFUSALS[name]
    ctx, handle = _context(nx=nx)
    rc, text = _connect_raw(ctx, [handle] * max(px * py, 1), px, py, rank, tripolar)
    assert rc == ERR_INVALID and "cf_peer_tile_connect" in text and words in text, (rc, text)
    assert _is_unconnected(ctx)
    if nx % 2 == 0:
        ctx.peer_tile_connect(None, 1, 1, 0, True)
        g = tc.global_fields(nx, 4, 3, True)
        tiles = tc.cut_tiles(g, nx, 4, 1, 1)
        fields = [ctx.to_device(a) for a in tiles[0]]
        ctx.halo_exchange_tile_peer(fields, [LOCATION[loc] for loc, _ in tc.FIELDS[:3]], [sg for _, sg in tc.FIELDS[:3]], rows=tc.ROWS, fold_north=True)
        ctx.sync()
        assert ctx.tile_stats() == (1, 0, 0) and ctx.fold_counts()[0] == 1
        for f in range(3):
            top = slice(tc.HY + 4, tc.HY + 4 + tc.ROWS)
            assert np.array_equal(fields[f].cpu().numpy()[top].view(np.int64), g[f][top].view(np.int64)), f
    ctx.close()
    torch.cuda.synchronize()


def test_slabs_and_tiles_refuse_each_others_contexts():
    from coflux.runtime import CofluxError
    from coflux import interface_computations as ic
    from coflux.runtime import FluxContext
    bare = FluxContext(6, 4, tc.HX, tc.HY, ic.flux_params(), ring=tc.RING)
    with pytest.raises(CofluxError, match="cf_peer_tile_export first"):
        bare.peer_tile_connect(None, 1, 1, 0, False)
    bare.close()
    ctx, handle = _context()
    ctx.peer_halo_export(4, tc.ROWS)
    ctx.peer_halo_connect(None, None, 0, 1)
    rc, text = _connect_raw(ctx, [], 1, 1, 0, 0)
    assert rc == ERR_INVALID and "latitude slabs" in text, (rc, text)
    assert _is_unconnected(ctx)
    assert ctx.peer_halo_stats()[0] == 0
    ctx.close()
    other, _ = _context()
    other.peer_tile_connect(None, 1, 1, 0, False)
    other.peer_halo_export(4, tc.ROWS)
    with pytest.raises(CofluxError, match="tile world"):
        other.peer_halo_connect(None, None, 0, 1)
    other.halo_exchange_tile_peer([other.to_device(np.zeros((4 + 2 * tc.HY, 6 + 2 * tc.HX)))], rows=tc.ROWS)   # still a world of one
    other.sync()
    assert other.tile_stats() == (1, 0, 0)
    other.close()


# what rank 1 exports differently from rank 0 in a (2,1) world — they are each other's W and E —, and the words of the refusal
PAIRS = (
    ("another_ny", dict(ny=5), True),
    ("another_max_fields", dict(max_fields=3), True),
    ("another_max_cols", dict(max_cols=tc.COLS), True),
    ("the_same", dict(), False),
)


def _tuple_text(nx=6, ny=4, max_fields=4, max_rows=tc.ROWS, max_cols=tc.COLS + 1):
    return "(%d, %d, %d, %d, %d, %d, %d)" % (max_fields, max_rows, max_cols, nx + 2 * tc.HX, ny, tc.HX, tc.HY)


def _connect_worker(rank, world, init, out):
    import torch.distributed as dist
    os.environ.update(HSA_ENABLE_IPC_MODE_LEGACY="0")
    dist.init_process_group("gloo", init_method=init, rank=rank, world_size=world)
    try:
        wrong = {}
        for what, different, refused in PAIRS:
            specs = [dict(), different]
            ctx, handle = _context(**specs[rank])
            handles = [None] * world
            dist.all_gather_object(handles, handle)
            rc, text = _connect_raw(ctx, handles, 2, 1, rank, 0)
            problems = []
            if refused:
                if rc != ERR_INVALID or _tuple_text(**specs[rank]) not in text or _tuple_text(**specs[1 - rank]) not in text:
                    problems.append(("the refusal does not name CF_ERR_INVALID and both tuples", rc, text))
                if not _is_unconnected(ctx):
                    problems.append("the context is not left unconnected")
            elif rc != 0:
                problems.append(("refused", rc, text))
            wrong[what] = problems
            ctx.sync()
            dist.barrier()       # a mailbox outlives its neighbour's look at it
            ctx.close()
        out[rank] = dict(wrong=wrong, seconds=0.0)
    finally:
        dist.destroy_process_group()


def test_connect_refuses_a_neighbour_exported_for_another_tuple_across_two_processes():
    """The neighbour's mailbox is opened through HIP IPC and its tuple read from there; both tuples are in the message; nothing
    is launched."""
    reports, seconds = _run_workers(_connect_worker, 2)
    print(f"connect across two processes, {len(PAIRS)} pairs: {seconds:.2f} s from spawn to join")
    for r in range(2):
        assert reports[r]["wrong"] == {what: [] for what, *_ in PAIRS}, (r, reports[r]["wrong"])
