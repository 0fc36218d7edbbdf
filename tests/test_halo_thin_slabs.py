"""CF_OPT_HALO_IN_SOLVER_LAUNCH on the slabs of a strongly scaled run: a few rows per rank, where the boundary-chunk dispatch of
ao_lean_body<…, HALO> leaves the branch every taller slab takes.  ensure_chunk_table classifies the chunks by the rows they
read — [0, cs) read south halo rows, [cn, n) read north halo rows — and the kernel remaps dispatch position to chunk for
cs <= cn (inner chunks, then the south set, then the north set) and not at all for cs > cn (a chunk in [cn, cs) waits on both
counters).  The slabs of tests/test_halo_in_launch.py are 30 rows or taller: cs < cn always.  Here the shapes are chosen from
the library's own table so that all three classes — cs < cn (the control), cs == cn (no inner chunk), cs > cn (a launch of one
chunk among them) — run, on lat-lon slabs down to ny = halo_rows and on tripolar slabs down to the fold's minimum
ny = ring + 2, the only height that guards the fold-then-exchange order of the deferred exchange.

One latitude slab per process (HIP IPC mailboxes; the ranks share the one device), as in tests/test_halo_in_launch.py; one
spawn per world, every shape and configuration inside the workers.  Against something that is not the halo machinery: the
same seven steps on the single-domain surface, whose rows every rank's interior rows must equal bit for bit."""
import functools
import os
import time

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import util
from coflux import abi, interface_computations as ic, synthetic as syn
from coflux.distributed import slab_bounds

pytestmark = pytest.mark.gpu

H, RING, NSTEPS = 5, 1, 7
FIELDS = ("T", "S", "u", "v")
INC = 1200.0 / 10800.0
CONFIGS = ("default", "corrected")
# what a world of tests/test_halo_in_launch.py takes from spawn to the last join on the MI355X (the slowest of its six cases, four
# ranks), and three times that: the limit under which each worker here is joined
MEASURED_SECONDS = 3.1
JOIN_LIMIT = 3 * MEASURED_SECONDS


def shapes(world):
    """(grid, nx, ny_global): lat-lon slabs of 2 to 8 rows per rank (halo 5: ny < hy occurs), narrow and wide; tripolar slabs
    whose LAST rank holds ring + 2 = 3 rows (4·world − 1 rows: 4 on every other rank), and a taller one.  By the table the library
    builds for them under the automatic plan (2 and 4 ranks alike): 64 × 2 one chunk, 64 × 4 two chunks with cs > cn, 64 × 8
    and some ranks of 360 × 2 and 360 × 3 cs == cn, 360 × 8 and the wide tripolar slabs cs < cn, the narrow tripolar slab
    cs > cn with one chunk on the last rank — asserted below, not relied on."""
    latlon = [("latlon", nx, ny * world) for nx, ny in ((64, 2), (64, 4), (64, 8), (360, 2), (360, 3), (360, 8))]
    return latlon + [("tripolar", 64, 4 * world - 1), ("tripolar", 360, 4 * world - 1), ("tripolar", 360, 8 * world)]


@functools.lru_cache(maxsize=None)
def _snapshots():
    return syn.jra55_snapshots(2)     # (seven steps of a ninth of a snapshot interval stay between the first two)


@functools.lru_cache(maxsize=None)
def _case(grid, nx, ny_global, rank, world):
    """(built once per process and never written to)  two ocean states of this rank's slab (one step apart), the weights, the source; rank 0 of 1: the single-domain surface"""
    j0, j1 = slab_bounds(ny_global, rank, world)
    ny = j1 - j0
    if grid == "tripolar":
        tc = syn.tripolar_case(nx, ny_global, H, H, j0=j0, j1=j1)
        first = dict(tc["ocean"])
        evolved = syn.evolved_ocean_state(syn.ocean_state(nx, ny_global, H, H, latitude=(-80.0, 90.0)), nx, ny_global, H, H, 1)
        second = {}
        for k in FIELDS:
            g = evolved[k].copy()
            syn.fold_north(g, nx, ny_global, H, H, 2, syn.FOLD_LOCATION[k], syn.FOLD_SIGN[k])
            second[k] = np.ascontiguousarray(g[j0:j1 + 2 * H])
        second["mask"] = first["mask"]
        return j0, ny, [first, second], tc["weights"], _snapshots()
    first = syn.ocean_state(nx, ny, H, H, ny_global=ny_global, j_offset=j0)
    second = syn.evolved_ocean_state(first, nx, ny, H, H, 1, ny_global=ny_global, j_offset=j0)
    fi, fj, phi = syn.latlon_fractional_indices(nx, ny, H, H, ny_global=ny_global, j_offset=j0)
    return j0, ny, [first, second], dict(separable=True, fi=fi, fj=fj, latitude=phi), _snapshots()


def _params(config):
    fluxes = ic.corrected_atmosphere_ocean_fluxes() if config == "corrected" else ic.SimilarityTheoryFluxes()
    return ic.flux_params(fluxes, ocean_surface=ic.SurfaceRadiationProperties(0.06, 1.0))


def boundary_chunks(begins, nx, ny):
    """(cs, cn) as ensure_chunk_table derives them from the table's begins (csrc/coflux_abi.cpp)"""
    n = len(begins) - 1
    wx = nx + 2 * RING
    south_cells, north_from = RING * wx, (ny - 1 + RING) * wx
    cs, cn = 0, n
    while cs < n and begins[cs] < south_cells:
        cs += 1
    while cn > 0 and begins[cn] > north_from:
        cn -= 1
    return cs, cn


class _Slab:
    """One context with its case on the device and the stepping loop's launch configured as bench.py does at N > 1."""

    def __init__(self, config, grid, nx, ny_global, rank, world):
        from coflux.runtime import EXCHANGE_NAMES, FluxContext
        self.rank, self.world, self.nx = rank, world, nx
        self.j0, self.ny, states_np, w_np, src_np = _case(grid, nx, ny_global, rank, world)
        self.ctx = ctx = FluxContext(nx, self.ny, H, H, _params(config), ring=RING)
        ctx.set_option(abi.OPT_MERGED_PREFETCH, 2)
        self.states = [{k: ctx.to_device(s[k]) for k in FIELDS + ("mask",)} for s in states_np]
        self.states[1]["mask"] = self.states[0]["mask"]
        self.src = {k: ctx.to_device(v) for k, v in src_np.items()}
        self.w = {k: (ctx.to_device(v) if isinstance(v, np.ndarray) else v) for k, v in w_np.items()}
        self.sets = [ctx.field_set(EXCHANGE_NAMES) for _ in range(2)]
        self.fold = grid == "tripolar" and rank == world - 1

    def steps(self, halo_backend):
        """(schedule, fluxes, net) of NSTEPS pipelined steps: the outputs NaN-filled, and so the halo rows a neighbour or the fold
        must deliver"""
        from coflux.runtime import FLUX_NAMES, NET_NAMES
        ctx, ny = self.ctx, self.ny
        for st in self.states:
            for k in FIELDS:
                if self.rank > 0:
                    st[k][:H] = float("nan")
                if self.rank < self.world - 1 or self.fold:
                    st[k][H + ny:] = float("nan")
        fl = {k: torch.full(ctx.shape, float("nan"), dtype=torch.float64, device=ctx.device) for k in FLUX_NAMES}
        net = {k: torch.full(ctx.shape, float("nan"), dtype=torch.float64, device=ctx.device) for k in NET_NAMES}
        sched = ctx.make_schedule(self.states, self.sets, time_fraction_increment=INC, pipeline=True, halo_backend=halo_backend,
                                  halo_rows=RING + 1 if halo_backend != abi.HALO_NONE else 0, fold_north=self.fold)
        torch.cuda.synchronize()
        return sched, fl, net

    def run(self, sched, fl, net):
        """{name: array} of every interface flux and of net u, v, T, S after the steps (cf_sync raises on a sticky status)"""
        from coflux.runtime import FLUX_NAMES
        self.ctx.time_steps(0, NSTEPS, sched, self.src, self.w, fl, net)
        self.ctx.sync()
        return {("f." + k): fl[k].cpu().numpy() for k in FLUX_NAMES} | {("n." + k): net[k].cpu().numpy() for k in ("u", "v", "T", "S")}

    def interior(self, result):
        return {k: np.ascontiguousarray(v[H:H + self.ny, H:H + self.nx]) for k, v in result.items()}


def _worker(rank, world, init, out):
    from coflux.distributed import SlabHaloExchanger
    started = time.perf_counter()
    os.environ.update(HSA_ENABLE_IPC_MODE_LEGACY="0")
    dist.init_process_group("gloo", init_method=init, rank=rank, world_size=world)
    try:
        report = {}
        for config in CONFIGS:
            for shape in shapes(world):
                slab = _Slab(config, *shape, rank, world)
                ctx, nx, ny = slab.ctx, slab.nx, slab.ny
                SlabHaloExchanger(ctx, ny, H, backend="peer")
                ctx.ensure_chunk_table(slab.states[0]["mask"])
                begins, _counts, _valid = ctx.debug_chunk_table()
                cs, cn = boundary_chunks(begins, nx, ny)
                results, stats = [], []
                for in_launch in (0, 1, 1):                      # (twice with the option: sequence parity and counters carry over)
                    ctx.set_option(abi.OPT_HALO_IN_SOLVER_LAUNCH, in_launch)
                    sched, fl, net = slab.steps(abi.HALO_PEER)
                    dist.barrier()
                    before = ctx.peer_halo_stats()
                    results.append(slab.run(sched, fl, net))     # (cf_sync: a neighbour that never arrived raises here)
                    after = ctx.peer_halo_stats()
                    stats.append((after[0] - before[0], after[1] - before[1]))
                    dist.barrier()
                lo = H if rank == 0 else H - 1                    # (the southernmost ring row reads outer halos nobody exchanges)
                finite = all(bool(np.isfinite(v[lo:H + ny + 1, H - 1:H + nx + 1]).all()) for k, v in results[0].items() if k.startswith("f."))
                differing = sorted({k for n in (1, 2) for k in results[0] if not np.array_equal(results[0][k], results[n][k], equal_nan=True)})
                report[(config,) + shape] = dict(table=(cs, cn, len(begins) - 1), ny=ny, j0=slab.j0, stats=stats, finite=finite, differing=differing,
                                                 layout=bool(ctx.solver_latency_layout()), interior=slab.interior(results[1]))
                ctx.close()
        out[rank] = (report, time.perf_counter() - started)
    finally:
        dist.destroy_process_group()


_GLOBAL = {}


def _single_domain(config, grid, nx, ny_global):
    """The same steps on the whole surface in one context with no halo backend (the tripolar fold is the fold kernel's), computed
    once per surface and configuration and never written to."""
    key = (config, grid, nx, ny_global)
    if key not in _GLOBAL:
        slab = _Slab(config, grid, nx, ny_global, 0, 1)
        _GLOBAL[key] = slab.run(*slab.steps(abi.HALO_NONE))
        for v in _GLOBAL[key].values():
            v.setflags(write=False)
        slab.ctx.close()
    return _GLOBAL[key]


def _class(cs, cn):
    return "cs < cn" if cs < cn else "cs == cn" if cs == cn else "cs > cn"


@pytest.mark.parametrize("world", [2, 4])
def test_thin_slabs_take_every_branch_of_the_boundary_dispatch_and_keep_the_bits(world):
    """Per shape, configuration and rank: (1) seven pipelined steps with the option on leave the bits of the run with it off,
    NaNs included; (2) the exchanges really rode — cf_peer_halo_stats deltas (7, 0) off and (7, 6) on, twice; (3) every cell a
    neighbour or the fold feeds is finite; (4) the interior rows equal the single-domain run's rows bit for bit.  And the shapes
    cover cs < cn, cs == cn and cs > cn (a single-chunk launch included) in both configurations, by the library's own table:
    the automatic plan reaches all three, CF_OPT_AO_CHUNK is not needed.

    Join limit: the workers of tests/test_halo_in_launch.py take 3.1 s from spawn to the last join on the MI355X (the slowest
    of its six cases, four ranks; 2.7 s with two; that test and the library's device code are the parent commit's); each worker
    here is joined under three times that, 9.3 s.  The workers here take 3.3 s (2 ranks) and 3.8 s (4 ranks) from spawn to join,
    1.0 to 1.3 s of it inside the worker function: process start-up is the rest."""
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
    classes = {config: {} for config in CONFIGS}
    for key in reports[0]:
        config, grid, nx, ny_global = key
        want = _single_domain(config, grid, nx, ny_global)
        for r in range(world):
            res = reports[r][key]
            cs, cn, n = res["table"]
            label = f"{key} rank {r} of {world}: ny = {res['ny']}, (cs, cn, n_chunks) = {(cs, cn, n)}, {_class(cs, cn)}"
            print(label, res["stats"], "latency layout" if res["layout"] else "")
            classes[config].setdefault(_class(cs, cn), []).append((key[1:], r, n))
            assert not res["differing"], (label, "the riders left other bits than the exchange kernel in", res["differing"])
            # every step exchanged once; with the option all but the call's last step (no request rides behind it: no tail
            # workgroups, hence the exchange kernel) rode in the solver launch
            assert res["stats"] == [(NSTEPS, 0), (NSTEPS, NSTEPS - 1), (NSTEPS, NSTEPS - 1)], (label, res["stats"])
            assert res["finite"], (label, "a halo row was not delivered")
            for k, rows in res["interior"].items():
                ref = want[k][H + res["j0"]:H + res["j0"] + res["ny"], H:H + nx]
                same = (rows.view(np.int64) == ref.view(np.int64))
                assert same.all(), (label, k, "differs from the single-domain run in", int((~same).sum()), "of", same.size, "cells")
    for config in CONFIGS:
        found = classes[config]
        assert set(found) == {"cs < cn", "cs == cn", "cs > cn"}, (config, world, {k: len(v) for k, v in found.items()})
        assert any(n == 1 for _shape, _r, n in found["cs > cn"]), (config, "no single-chunk launch", found["cs > cn"])
    # (the COARE profile on these small slabs runs the latency-layout kernels: their HALO variants are the ones exercised)
    assert any(reports[r][key]["layout"] for r in range(world) for key in reports[r] if key[0] == "corrected")
    assert not any(reports[r][key]["layout"] for r in range(world) for key in reports[r] if key[0] == "default")
