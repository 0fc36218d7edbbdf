"""A sharded run's attached diagnostics against the single domain's (include/coflux.h: the "Slabs" sentences of the integrals,
monitor, climatology and regrid sections; coflux.distributed: combine_monitor_records, combine_integral_records,
restrict_operator, combine_regridded).

Every rank — one PROCESS over HIP IPC on the one device — and the single domain attach the same diagnostics to cf_time_steps:
two averagers (plain means, stride 1; derived terms on ocean state 0 that read [i+1] and [j+1] of it, stride 2), a climatology of
net.T over two bins, an integrator with area, wet mask and a region, and a monitor with the rank's first_cell and row_length
whose third entry is the designed array of tests/sharded_case.py cut per rank.  Six steps over two alternating ocean states whose
every halo cell a neighbour, the partner or the fold must deliver is NaN before the run: state 0 is exchanged on the even steps,
so the derived terms' first collection, after step 1, reads halos that step 0 delivered.  cf_time_steps_coupled runs on two tripolar
slabs with a budget averager in place of the derived one and a monitor on net.S and the skin temperature.

The reference of every assertion is the single-domain run of the library with the same attachments, a path that
test_time_average, test_derived_average, test_climatology, test_surface_integrals and test_surface_monitor hold to NumPy
references; the integrals are held to math.fsum within derived bounds as well, the monitor's last record to
tests/monitor_reference.py."""
import functools
import os
import time
from types import SimpleNamespace

import numpy as np
import pytest

import monitor_reference as mr
import regrid_reference as rr
import sharded_case as sc
import test_tile_steps as tts
import util
from coflux import abi
from coflux import distributed as cd
from coflux import regridding
from coflux.distributed import tile_bounds, tile_coords

pytestmark = pytest.mark.gpu

H, ROWS, INC, FIELDS = tts.H, tts.ROWS, tts.INC, tts.FIELDS
STEPS = 6
CALLS_ONE = [(0, STEPS, True)]
CALLS_FOUR_TWO = [(0, 4, abi.PIPELINE_CONTINUING), (4, 2, abi.PIPELINE_CONTINUING)]
STEP_SECONDS = 10.0
# the calendar table: step s is stamped 10 · (s + 1); bins 0, 1, 0, none, 1, 0
CLIM_TABLE = (np.arange(STEPS + 1) * STEP_SECONDS + 5.0, np.array([0, 1, 0, -1, 1, 0], dtype=np.int32))
CLIM_BINS = 2
MEAN_NAMES = ("fl.x_momentum", "fl.sensible_heat", "net.T", "net.S")
DERIVED = (("center_x", "u", None), ("center_y", "v", None), ("kinetic_energy", "u", "v"), ("product", "T", "T"))
INTEGRANDS = (("one", None, None, 0.0, 0), ("field", "net.T", None, 0.0, 0), ("product", "fl.x_momentum", "fl.x_momentum", 0.0, 0),
              ("above", "net.S", None, 0.0, 0), ("field", "net.T", None, 0.0, 1))
SLAB_SURFACES = [(64, 24), (68, 37)]       # a rank of three holds 512 cells of the first; two unequal integral tiles on the second
TILE_SURFACES = [(68, 37)]                 # tiles 34 and 17 wide: a pair of cells straddles a row end
GRIDS = ("tripolar", "latlon")
# measured on the MI355X: the tile worlds (2,2) and (4,1) take 3.6 and 3.7 s from spawn to the last join, the slabs 3.7 s (2 ranks) and
# 3.6 s (3 ranks) with the exchange kernel and 4.1 s and 3.7 s with the riders, the coupled loop's two slabs 3.2 s, 0.6 to 1.8 s of it
# inside the worker function (process start-up is the rest); every worker is joined under three times the slowest, killed beyond it
# and never retried
MEASURED_SECONDS = 4.1
JOIN_LIMIT = 3 * MEASURED_SECONDS


# ---- static arrays of a surface: area, region bits, the designed monitor array -----------------------------------------------
@functools.lru_cache(maxsize=None)
def static_arrays(nx, ny):
    """halo-inclusive global arrays; the halos hold what nothing may read (NaN area, 7e77 in the designed array)"""
    rng = np.random.default_rng(1000 * nx + ny)
    area = np.full((ny + 2 * H, nx + 2 * H), np.nan)
    area[H:H + ny, H:H + nx] = (0.5 + rng.random((ny, nx))) * 1.0e9
    region = np.zeros((ny + 2 * H, nx + 2 * H), dtype=np.uint8)
    region[H:H + ny, H:H + nx] = 1 | (2 * (rng.random((ny, nx)) < 0.4).astype(np.uint8))
    designed = np.full((ny + 2 * H, nx + 2 * H), 7.0e77)
    designed[H:H + ny, H:H + nx] = sc.monitor_fixture()[0][:ny, :nx]          # (the 64 × 24 surface holds its south-west part)
    return dict(area=area, region=region, designed=designed)


def cut(a, i0, i1, j0, j1):
    return np.ascontiguousarray(a[j0:j1 + 2 * H, i0:i1 + 2 * H])


class Diagnostics:
    """the attachments of one context: on `run` (tts._Run) or on loose device fields of a fresh context"""

    def __init__(self, ctx, fl, net, state0, mask, static, first_cell, row_length):
        import torch
        self.ctx = ctx
        nan = lambda *lead: torch.full(tuple(lead) + tuple(ctx.shape), float("nan"), dtype=torch.float64, device=ctx.device)  # noqa: E731
        named = {"fl." + k: v for k, v in fl.items()} | {"net." + k: v for k, v in net.items()}
        self.static = {k: ctx.to_device(v) for k, v in static.items()}
        self.means = [nan() for _ in MEAN_NAMES]
        self.average = ctx.average([named[k] for k in MEAN_NAMES], self.means)
        self.derived_means = [nan() for _ in DERIVED]
        self.derived = None
        if state0 is not None:
            self.derived = ctx.derived_average([(kind, state0[a], state0[b] if b else None, 1.0, 0, m) for (kind, a, b), m in zip(DERIVED, self.derived_means)])
        self.total, self.bins = nan(), nan(CLIM_BINS)
        self.clim = ctx.climatology([named["net.T"]], [self.total], [self.bins], CLIM_BINS)
        self.integrals = ctx.integrals([(k, named.get(a), named.get(b), thr, bit) for k, a, b, thr, bit in INTEGRANDS], area=self.static["area"],
                                       mask=mask, region=self.static["region"], capacity=STEPS)
        self.monitor = ctx.monitor([(named["net.T"], "value"), (named["fl.x_momentum"], "abs"), (self.static["designed"], "value")], mask=mask,
                                   first_cell=first_cell, row_length=row_length, capacity=STEPS)

    def attach(self):
        ctx = self.ctx
        ctx.attach_average(self.average, stride=1, step_weight=STEP_SECONDS, slot=0)
        ctx.attach_average(self.derived, stride=2, step_weight=STEP_SECONDS, slot=1)
        ctx.attach_climatology(self.clim, CLIM_TABLE, 1, STEP_SECONDS, 0.0, STEP_SECONDS)
        ctx.attach_integrals(self.integrals, 1, 0.0, STEP_SECONDS)
        ctx.attach_monitor(self.monitor, 1, 0.0, STEP_SECONDS)

    def results(self):
        """everything as host arrays (after a cf_sync): whole buffers, halos included"""
        host = lambda t: t.cpu().numpy()  # noqa: E731
        total, samples, bin_totals, bin_samples = self.clim.weights()
        return dict(means=[host(m) for m in self.means], derived=[host(m) for m in self.derived_means], weights=(self.average.weight(), self.derived.weight()),
                    clim_total=host(self.total), clim_bins=host(self.bins), clim_weights=(total, samples, bin_totals.tolist(), bin_samples.tolist()),
                    integrals=self.integrals.read(), monitor=self.monitor.read())


def run_calls(run, calls, backend, fold):
    """cf_time_steps over `calls` = [(first, nsteps, pipeline)]; (return code, message) of the first that fails"""
    import ctypes as C
    ctx = run.ctx
    for first, nsteps, pipeline in calls:
        sched = ctx.make_schedule(run.states, run.sets, time_fraction_increment=INC, pipeline=pipeline, halo_backend=backend,
                                  halo_rows=ROWS if backend != abi.HALO_NONE else 0, fold_north=fold)
        s, w, f, n = ctx.source_struct(run.src, 0, 0, 0.0), ctx.weights_struct(run.w), ctx.fluxes_struct(run.fl), ctx.net_struct(run.net)
        rc = ctx.lib.cf_time_steps(ctx._h, first, nsteps, C.byref(sched), C.byref(s), C.byref(w), C.byref(f), None, C.byref(n))
        if rc != 0:
            return rc, ctx.lib.cf_last_error(ctx._h).decode()
    return 0, ""


def whole_fields(run):
    return {k: v.cpu().numpy() for k, v in ({"fl." + k: v for k, v in run.fl.items()} | {"net." + k: v for k, v in run.net.items()}).items()}


_SINGLE = {}


def single_domain(grid, nx, ny):
    """Once per surface: the six steps on the whole surface in one context with the diagnostics attached (first_cell = 0,
    row_length = 0) → dict(diag, final — whole buffers of fluxes and net —, per_step — the interiors of the integrands' fields after
    every step, from a second, plain context stepped one CF_PIPELINE_CONTINUING call at a time, whose final bits are the first's)."""
    key = (grid, nx, ny)
    if key in _SINGLE:
        return _SINGLE[key]
    states, weights, src = tts.global_case(grid, nx, ny)
    fold = grid == "tripolar"
    run = tts._Run(nx, ny, states, weights, src)
    diag = Diagnostics(run.ctx, run.fl, run.net, run.states[0], run.states[0]["mask"], static_arrays(nx, ny), 0, 0)
    diag.attach()
    rc, text = run_calls(run, CALLS_ONE, abi.HALO_NONE, fold)
    assert rc == 0, text
    run.ctx.sync()
    out = dict(diag=diag.results(), final=whole_fields(run), wet=np.asarray(states[0]["mask"])[H:H + ny, H:H + nx] != 0)
    run.ctx.close()
    plain = tts._Run(nx, ny, states, weights, src)
    per_step = []
    for s in range(STEPS):
        rc, text = run_calls(plain, [(s, 1, abi.PIPELINE_CONTINUING)], abi.HALO_NONE, fold)
        assert rc == 0, text
        plain.ctx.sync()
        per_step.append({k: v[H:H + ny, H:H + nx].copy() for k, v in whole_fields(plain).items() if k in ("net.T", "net.S", "fl.x_momentum")})
    for k, v in per_step[-1].items():
        assert np.array_equal(v.view(np.int64), out["final"][k][H:H + ny, H:H + nx].view(np.int64)), (key, k, "the stepped run differs")
    plain.ctx.close()
    out["per_step"] = per_step
    assert np.isfinite(out["final"]["net.T"][H:H + ny, H:H + nx]).all()
    _SINGLE[key] = out
    return out


# ---- the workers -----------------------------------------------------------------------------------------------------------
def _worker(rank, world, init, out, px, py, slabs, in_launch):
    """One rank of a px × py world.  `slabs`: px = 1, the peer-direct slab exchange (SlabHaloExchanger), the six steps as 4 + 2
    continuing calls with CF_OPT_HALO_IN_SOLVER_LAUNCH = `in_launch`; else the tile exchange, one call.  Per surface a run with
    nothing attached, then — on fresh outputs, the halos poisoned again — the attached run: the counters grow alike."""
    import torch
    import torch.distributed as dist
    from coflux.distributed import SlabHaloExchanger, connect_tiles
    from coflux.runtime import CofluxError
    started = time.perf_counter()
    os.environ.update(HSA_ENABLE_IPC_MODE_LEGACY="0")
    dist.init_process_group("gloo", init_method=init, rank=rank, world_size=world)
    try:
        report = dict(results={}, grown={}, error=None)
        p, q = tile_coords(rank, px)
        for grid in GRIDS:
            tripolar = grid == "tripolar"
            fold = tripolar and q == py - 1
            for nx, ny_global in (SLAB_SURFACES if slabs else TILE_SURFACES):
                label = (grid, nx, ny_global)
                i0, i1, j0, j1 = bounds = tile_bounds(nx, ny_global, rank, px, py)
                nxl, ny = i1 - i0, j1 - j0
                states, weights, src = tts.tile_case(grid, nx, ny_global, i0, i1, j0, j1)
                poisoned = [dict(s) for s in states]
                tts._poison(poisoned, px, py, p, q, nxl, ny, fold)
                run = tts._Run(nxl, ny, poisoned, weights, src)
                if slabs:
                    exchanger = SlabHaloExchanger(run.ctx, ny, H, backend="peer")
                    assert exchanger.backend == "peer", getattr(exchanger, "peer_fallback_reason", None)
                    run.ctx.set_option(abi.OPT_MERGED_PREFETCH, 2)
                    run.ctx.set_option(abi.OPT_HALO_IN_SOLVER_LAUNCH, in_launch)
                else:
                    connect_tiles(run.ctx, px, py, tripolar)
                static = {k: cut(v, *bounds) for k, v in static_arrays(nx, ny_global).items()}
                grown = []
                for attached in (False, True):
                    if attached:
                        for st, host in zip(run.states, poisoned):          # the halos are NaN again; fresh outputs
                            for k in FIELDS:
                                st[k].copy_(torch.from_numpy(host[k]))
                        run.outputs()
                        diag = Diagnostics(run.ctx, run.fl, run.net, run.states[0], run.states[0]["mask"], static, j0 * nx + i0, nx)
                        diag.attach()
                    torch.cuda.synchronize()
                    dist.barrier()
                    before = run.counters()
                    rc, text = run_calls(run, CALLS_FOUR_TWO if slabs else CALLS_ONE, abi.HALO_PEER, fold)
                    if rc != 0:
                        report["error"] = (label, text)
                        break
                    try:
                        run.ctx.sync()
                    except CofluxError as e:   # CF_ERR_COMM: somebody never arrived.  Nothing more is started on the device.
                        report["error"] = (label, str(e))
                        break
                    grown.append(tuple(a - b for a, b in zip(run.counters(), before)))
                    run.ctx.discard_prefetched_atmosphere_state()      # (a continuing call leaves a request for the step after it)
                    dist.barrier()
                if report["error"] is not None:
                    break
                report["grown"][label] = grown
                report["results"][label] = dict(diag.results(), fields=whole_fields(run), bounds=bounds)
                dist.barrier()              # a mailbox outlives its neighbours' last exchange
                run.ctx.close()
            if report["error"] is not None:
                break
        report["seconds"] = time.perf_counter() - started
        out[rank] = report
    finally:
        dist.destroy_process_group()


def _run_workers(target, world, *args):
    """test_tile_steps.py's pattern: one spawn, every worker joined under JOIN_LIMIT, killed beyond it, never retried"""
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


# ---- the assertions ----------------------------------------------------------------------------------------------------------
def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def interior(a, nxl, ny):
    return a[..., H:H + ny, H:H + nxl]


def halo_is_nan(a, nxl, ny):
    keep = np.ones(a.shape[-2:], dtype=bool)
    keep[H:H + ny, H:H + nxl] = False
    return bool(np.isnan(a[..., keep]).all())


def check_integral_series(label, series, single_series, per_step, area, wet, region, bounds, integrands):
    """Per record and entry, with t_k the kernel's per-cell terms formed in NumPy from `per_step[s]` (interiors of the single domain's
    fields after step s) and the exact sum math.fsum of them: a rank's record within γ(n_r − 1) · Σ|t_k| of the exact sum over its
    own cells (`bounds`: per rank (i0, i1, j0, j1)), the single domain's the same way over all cells, and the combined record
    (combine_integral_records) within the sum of those bounds, the ranks' and the single domain's — γ(n) is the bound of a sum in
    any order; the single domain's term also covers the one rounding of the combination, u · |result| ≤ u · Σ|t_k|."""
    combined = cd.combine_integral_records(series)
    assert single_series.shape == combined.shape == (len(per_step), len(integrands)), (label, single_series.shape, combined.shape)
    for s, fields in enumerate(per_step):
        bound_sum = np.zeros(len(integrands))
        for r, (i0, i1, j0, j1) in enumerate(bounds):
            C = lambda a: a[j0:j1, i0:i1]  # noqa: E731
            for e, terms in enumerate(integrand_terms({k: C(v) for k, v in fields.items()}, C(area), C(wet), C(region), integrands)):
                exact, bound = sc.sum_bound(terms)
                bound_sum[e] += bound
                assert abs(series[r][s, e] - exact) <= bound, (label, "rank", r, "step", s, "entry", e, series[r][s, e], exact, bound)
        for e, terms in enumerate(integrand_terms(fields, area, wet, region, integrands)):
            exact, bound = sc.sum_bound(terms)
            assert terms.size > 1 and abs(single_series[s, e] - exact) <= bound, (label, "single domain", s, e, single_series[s, e], exact, bound)
            assert abs(combined[s, e] - exact) <= bound_sum[e] + bound, (label, "combined", s, e, combined[s, e], exact, bound_sum[e] + bound)


def fresh_context_integrals(shape, named, area, mask, region, integrands):
    """one host-driven cf_integrals_collect on a fresh, unconnected context of `shape` = (nx, ny, hx, hy) that holds the given
    halo-layout host arrays: the record"""
    from coflux.runtime import FluxContext
    ctx = FluxContext(*shape, tts._params(), ring=tts.RING)
    named = {k: ctx.to_device(np.ascontiguousarray(v)) for k, v in named.items()}
    area, mask, region = (ctx.to_device(np.ascontiguousarray(a)) for a in (area, mask, region))
    q = ctx.integrals([(k, named.get(a), named.get(b), thr, bit) for k, a, b, thr, bit in integrands], area=area, mask=mask, region=region, capacity=1)
    q.collect(0.0)
    got = q.read()[0][0]
    q.close()
    ctx.close()
    return got


def integrand_terms(fields, area, wet, region, integrands=INTEGRANDS):
    """[entry] → the kernel's per-cell terms over the selected cells (coflux_integrals.hip: x · A with x = a · b rounded first)"""
    out = []
    for kind, a, b, thr, bit in integrands:
        sel = wet & ((region >> bit) & 1 != 0)
        if kind == "one":
            x = np.ones_like(area)
        elif kind == "field":
            x = fields[a]
        elif kind == "product":
            x = fields[a] * fields[b]
        else:
            x = (fields[a] > thr).astype(np.float64)
        out.append((x * area)[sel])
    return out


def check_fields_and_means(label, rep, want):
    i0, i1, j0, j1 = rep["bounds"]
    nxl, ny = i1 - i0, j1 - j0
    G = lambda a: a[..., H + j0:H + j1, H + i0:H + i1]  # noqa: E731
    for k, ref in want["final"].items():
        assert same_bytes(interior(rep["fields"][k], nxl, ny), G(ref)), (label, k, "the field differs from the single domain's")
    wd = want["diag"]
    for name, got, ref in ([(n, g, r) for n, g, r in zip(MEAN_NAMES, rep["means"], wd["means"])]
                           + [(d[0] + str(d[1:]), g, r) for d, g, r in zip(DERIVED, rep["derived"], wd["derived"])]
                           + [("climatology total", rep["clim_total"], wd["clim_total"]), ("climatology bins", rep["clim_bins"], wd["clim_bins"])]):
        same = interior(got, nxl, ny).view(np.int64) == G(ref).view(np.int64)
        assert same.all(), (label, name, "differs from the single domain's in", int((~same).sum()), "of", same.size, "cells")
        assert not np.isnan(interior(got, nxl, ny)).any(), (label, name, "a NaN from a halo that was not delivered, or a mean never stored")
        assert halo_is_nan(got, nxl, ny), (label, name, "a halo cell of the buffer was written")
    assert rep["weights"] == wd["weights"] and rep["weights"][0] == (STEPS * STEP_SECONDS, STEPS) and rep["weights"][1] == (STEPS * STEP_SECONDS, STEPS // 2), (label, rep["weights"])
    assert rep["clim_weights"] == wd["clim_weights"] and rep["clim_weights"][3] == [3, 2], (label, rep["clim_weights"])


def check_series(label, reports, want, nx, ny_global):
    """the monitor's combined records, all eight words at every step; the integrals within their derived bounds"""
    statics = static_arrays(nx, ny_global)
    values, times = zip(*[rep["monitor"] for rep in reports])
    want_values, want_times = want["diag"]["monitor"]
    combined = cd.combine_monitor_records(values)
    assert combined.shape == (STEPS, 3)
    for s in range(STEPS):
        for e, entry in enumerate(("net.T", "|fl.x_momentum|", "designed")):
            for word in mr.DTYPE.names:
                assert combined[s, e][word].tobytes() == want_values[s, e][word].tobytes(), \
                    (label, "step", s, entry, word, combined[s, e][word], "single domain:", want_values[s, e][word])
    assert all(np.array_equal(t, want_times) for t in times) and np.array_equal(want_times, STEP_SECONDS * np.arange(1, STEPS + 1))
    # the last record against the definition, on the cut of the single domain's final fields
    designed, final = statics["designed"], want["final"]
    for r, rep in enumerate(reports):
        i0, i1, j0, j1 = rep["bounds"]
        G = lambda a: a[H + j0:H + j1, H + i0:H + i1]  # noqa: E731
        wet = want["wet"][j0:j1, i0:i1]
        ref = [mr.monitor_value(G(a), wet, kind, first_cell=j0 * nx + i0, row_length=nx)
               for a, kind in ((final["net.T"], "value"), (final["fl.x_momentum"], "abs"), (designed, "value"))]
        assert mr.same(values[r][-1], np.array(ref, dtype=mr.DTYPE)), (label, "rank", r, "last monitor record", values[r][-1], ref)
    check_integral_series(label, [rep["integrals"][0] for rep in reports], want["diag"]["integrals"][0], want["per_step"], statics["area"][H:-H, H:-H],
                          want["wet"], statics["region"][H:-H, H:-H], [rep["bounds"] for rep in reports], INTEGRANDS)
    assert all(np.array_equal(rep["integrals"][1], want["diag"]["integrals"][1]) for rep in reports)


def check_last_integrals_on_a_fresh_context(label, reports, want, nx, ny_global):
    """"depends only on the interior values, the weights and (nx, ny)": the rank's last record, byte for byte, from a host-driven
    cf_integrals_collect on a fresh, unconnected context of the rank's shape that holds the cut of the single domain's final fields"""
    statics = static_arrays(nx, ny_global)
    states = tts.global_case(label[0], nx, ny_global)[0]
    for r, rep in enumerate(reports):
        bounds = i0, i1, j0, j1 = rep["bounds"]
        got = fresh_context_integrals((i1 - i0, j1 - j0, H, H), {k: cut(want["final"][k], *bounds) for k in ("net.T", "net.S", "fl.x_momentum")},
                                      cut(statics["area"], *bounds), cut(np.asarray(states[0]["mask"]), *bounds), cut(statics["region"], *bounds), INTEGRANDS)
        assert same_bytes(got, rep["integrals"][0][-1]), (label, "rank", r, got, rep["integrals"][0][-1])


def _regrid_operators(nx, ny):
    src = SimpleNamespace(size=(nx, ny, 1), longitude=(0.0, 360.0), latitude=(-70.0, 70.0))
    return dict(zonal=regridding.zonal_mean_weights(src, nlat=12, latitude=(-90.0, 90.0)),       # bands beyond ±70°: NaN rows
                latlon=regridding.conservative_latlon_weights(src, nlon=8, nlat=9))


def check_regridded_means(label, reports, want, nx, ny_global):
    """After the run: the slot-0 means of every rank through restrict_operator in CF_REGRID_SUM with the coverage, combined by
    combine_regridded, against the single domain's CF_REGRID_MEAN of its means; tolerance per row by sharded_case.regrid_row_bounds
    (the derivation is stated there), NaN rows coincide exactly."""
    from coflux.runtime import FluxContext
    states = tts.global_case(label[0], nx, ny_global)[0]
    mask_np = np.asarray(states[0]["mask"])

    def apply(op, bounds, means, mode):
        i0, i1, j0, j1 = bounds
        ctx = FluxContext(i1 - i0, j1 - j0, H, H, tts._params(), ring=tts.RING)
        mask = ctx.to_device(cut(mask_np, *bounds))
        g = ctx.regridder(*op, mask=mask, mode=mode)
        dst = g.apply([ctx.to_device(np.ascontiguousarray(m)) for m in means])
        ctx.sync()
        got = np.stack([d.cpu().numpy() for d in dst]), g.coverage.cpu().numpy()
        g.close()
        ctx.close()
        return got

    whole_bounds = (0, nx, 0, ny_global)
    for name, op in _regrid_operators(nx, ny_global).items():
        whole_means = want["diag"]["means"]
        single, _cov = apply(tuple(op), whole_bounds, whole_means, "mean")
        wet_whole = mask_np != 0
        definitions, numerators, coverages = [], [], []
        for rep in reports:
            b = i0, i1, j0, j1 = rep["bounds"]
            local = cd.restrict_operator(op, nx, i0, i1, j0, j1)
            N, D = apply(local, b, rep["means"], "sum")
            numerators.append(N)
            coverages.append(D)
            definitions.append(rr.definition(*local, rep["means"], cut(wet_whole, *b), (i1 - i0, j1 - j0, H, H)))
        definitions.append(rr.definition(*op, whole_means, wet_whole, (nx, ny_global, H, H)))
        tol = sc.regrid_row_bounds(definitions)
        got = cd.combine_regridded(numerators, coverages)
        nan_rows = np.array([d["D"] == 0 for d in definitions[-1]])
        assert np.array_equal(np.isnan(got), np.broadcast_to(nan_rows, got.shape)) and np.array_equal(np.isnan(single), np.isnan(got)), (label, name, "NaN rows")
        assert nan_rows.any() and not nan_rows.all(), (label, name)
        ok = ~np.isnan(got)
        worst = float(np.max(np.abs(got - single)[ok] / tol[ok]))
        print(f"{label} {name}: worst |combined - single| / tolerance = {worst:.3f}")
        assert (np.abs(got - single)[ok] <= tol[ok]).all(), (label, name, worst)


def check_world(reports, px, py, slabs, counters):
    world = px * py
    for r in range(world):
        assert reports[r]["error"] is None, (r, reports[r]["error"])
    for grid in GRIDS:
        for nx, ny_global in (SLAB_SURFACES if slabs else TILE_SURFACES):
            label = (grid, nx, ny_global)
            want = single_domain(grid, nx, ny_global)
            reps = [reports[r]["results"][label] for r in range(world)]
            for r, rep in enumerate(reps):
                check_fields_and_means(label + ("rank", r), rep, want)
                plain, attached = reports[r]["grown"][label]
                assert plain == attached, (label, r, "attaching changed what the exchange counters count", plain, attached)
                counters(label, r, attached)
            check_series(label, reps, want, nx, ny_global)
            check_last_integrals_on_a_fresh_context(label, reps, want, nx, ny_global)
            if not slabs:
                check_regridded_means(label, reps, want, nx, ny_global)


@pytest.mark.parametrize("in_launch", [0, 1])
@pytest.mark.parametrize("world", [2, 3])
def test_latitude_slabs_hold_the_single_domains_diagnostics(world, in_launch):
    """cf_time_steps on 2 and 3 latitude slabs, the exchange a peer kernel (0) or rider workgroups of the solver launch (1), six
    steps as continuing calls of 4 and 2: every mean, total and bin on the rank's interior is the single domain's, byte for byte,
    the buffers' halos still NaN, weights and sample counts equal; the combined monitor records are the single domain's in all
    eight words at every step; the integrals lie within their derived bounds; the last records are those of a fresh context.
    Every step exchanges once, with or without attachments; with the option on some of them ride."""
    reports, seconds = _run_workers(_worker, world, 1, world, True, in_launch)
    print(f"{world} slabs, in-launch {in_launch}: {seconds:.1f} s from spawn to join, of which in the worker function", [round(reports[r]["seconds"], 1) for r in range(world)])

    def counters(label, r, grown):
        # (tile exchanges, x-phases, folds sent, fold launches, exchanges with a fold | …, slab exchanges, of which in the solver launch)
        assert grown[:3] == (0, 0, 0) and grown[-2] == STEPS, (label, r, grown)
        assert grown[-1] == 0 if in_launch == 0 else 0 < grown[-1] <= STEPS, (label, r, grown)
    check_world(reports, 1, world, True, counters)


@pytest.mark.parametrize("px,py", sc.WORLDS)
def test_tile_worlds_hold_the_single_domains_diagnostics(px, py):
    """cf_time_steps on the tile worlds (2,2) and (4,1) of the 68 × 37 surface, six steps in one call: as the slabs' test, with the
    monitor's cells numbered first_cell + j·row_length + i (the tile's own nx cannot pass: tests/sharded_case.py), and the slot-0
    means regridded per rank and combined against the single domain's CF_REGRID_MEAN.  cf_peer_tile_stats grows by (6, 6, 6 where
    the rank sends a fold) with or without attachments; no fold launch, no slab exchange."""
    world = px * py
    reports, seconds = _run_workers(_worker, world, px, py, False, 0)
    print(f"{px} x {py} world: {seconds:.1f} s from spawn to join, of which in the worker function", [round(reports[r]["seconds"], 1) for r in range(world)])

    def counters(label, r, grown):
        sends_fold = label[0] == "tripolar" and r // px == py - 1
        assert grown == (STEPS, STEPS, STEPS if sends_fold else 0, 0, 0, 0, 0), (label, r, grown)
    check_world(reports, px, py, False, counters)


# ---- the coupled loop on two tripolar slabs --------------------------------------------------------------------------------------
COUPLED_SURFACE = (64, 6)                  # tests/coupled_fold_case.py's smallest: three rows per rank, the least the fold admits
BUDGET = ("heat_atmosphere_ocean", "salt_atmosphere_ocean", "heat_ice_ocean")      # SQao, SFao and an ice term
COUPLED_FIELDS = ("net.T", "net.S", "fl.x_momentum", "skin")


@functools.lru_cache(maxsize=None)
def coupled_region(nx, ny):
    """region bits on the whole surface in coupled_fold_case's halo layout: bit 0 everywhere, bit 1 on four cells of ten; halos 0"""
    import coupled_fold_case as fc
    rng = np.random.default_rng(1000 * nx + ny + 1)
    region = np.zeros((ny + 2 * fc.HY, nx + 2 * fc.HX), dtype=np.uint8)
    region[fc.HY:fc.HY + ny, fc.HX:fc.HX + nx] = 1 | (2 * (rng.random((ny, nx)) < 0.4).astype(np.uint8))
    return region


def coupled_fields(out):
    host = lambda t: t.cpu().numpy()  # noqa: E731
    return {"net.T": host(out.net["T"]), "net.S": host(out.net["S"]), "fl.x_momentum": host(out.fl["x_momentum"]), "skin": host(out.skin)}


class CoupledDiagnostics:
    """on a test_coupled_steps.Rig and its Outputs: plain means in slot 0, a budget averager in slot 1 (stride 2), a climatology of
    net.T, the integrator of INTEGRANDS with the case's area and wet mask and `region`, a monitor on net.S and the carried skin
    temperature"""

    def __init__(self, rig, out, region, first_cell, row_length):
        import coupled_fold_case as fc
        import torch
        self.ctx = ctx = rig.ctx
        self.steps = fc.STEPS
        nan = lambda *lead: torch.full(tuple(lead) + tuple(ctx.shape), float("nan"), dtype=torch.float64, device=ctx.device)  # noqa: E731
        named = {"fl." + k: v for k, v in out.fl.items()} | {"net." + k: v for k, v in out.net.items()}
        mask = rig.oceans[0]["mask"]
        self.region = ctx.to_device(np.ascontiguousarray(region))
        self.means = [nan() for _ in MEAN_NAMES]
        self.average = ctx.average([named[k] for k in MEAN_NAMES], self.means)
        self.budget_means = [nan() for _ in BUDGET]
        ice = dict(concentration=rig.ice_states[0]["concentration"], interface_heat=out.iof["interface_heat"], salt_flux=out.iof["salt_flux"])
        self.budget = ctx.budget_average([(k, 1.0, m) for k, m in zip(BUDGET, self.budget_means)], ocean=rig.oceans[0], atmos=out.sets[0], fluxes=out.fl,
                                         ice=ice, weights=rig.w, frazil_heat=out.iof["frazil_heat"], land_freshwater=out.land)
        self.total, self.bins = nan(), nan(CLIM_BINS)
        self.clim = ctx.climatology([named["net.T"]], [self.total], [self.bins], CLIM_BINS)
        self.integrals = ctx.integrals([(k, named.get(a), named.get(b), thr, bit) for k, a, b, thr, bit in INTEGRANDS], area=rig.area, mask=mask,
                                       region=self.region, capacity=self.steps)
        self.monitor = ctx.monitor([(named["net.S"], "value"), (out.skin, "value")], mask=mask, first_cell=first_cell, row_length=row_length, capacity=self.steps)

    def attach(self):
        ctx, n = self.ctx, self.steps
        table = (np.arange(n + 1) * STEP_SECONDS + 5.0, np.array([0, 1, 0, -1, 1, 0, 1], dtype=np.int32)[:n])
        ctx.attach_average(self.average, stride=1, step_weight=STEP_SECONDS, slot=0)
        ctx.attach_average(self.budget, stride=2, step_weight=STEP_SECONDS, slot=1)
        ctx.attach_climatology(self.clim, table, 1, STEP_SECONDS, 0.0, STEP_SECONDS)
        ctx.attach_integrals(self.integrals, 1, 0.0, STEP_SECONDS)
        ctx.attach_monitor(self.monitor, 1, 0.0, STEP_SECONDS)

    def results(self, out):
        host = lambda t: t.cpu().numpy()  # noqa: E731
        total, samples, bin_totals, bin_samples = self.clim.weights()
        return dict(means=[host(m) for m in self.means], budget=[host(m) for m in self.budget_means], weights=(self.average.weight(), self.budget.weight()),
                    clim_total=host(self.total), clim_bins=host(self.bins), clim_weights=(total, samples, bin_totals.tolist(), bin_samples.tolist()),
                    integrals=self.integrals.read(), monitor=self.monitor.read(), fields=coupled_fields(out))


_COUPLED_SINGLE = {}


def coupled_single_domain(nx, ny):
    """Once: the seven steps on the whole tripolar surface in one context with the diagnostics attached; and `per_step`, the
    interiors of the integrands' and the monitor's fields after every step, from a second, plain rig stepped one
    CF_PIPELINE_CONTINUING call at a time (coupled_fold_case.run's `between`), whose final bits are the first's."""
    import coupled_fold_case as fc
    import test_coupled_steps as tcs
    if (nx, ny) not in _COUPLED_SINGLE:
        rig = fc.make_rig(fc.folded_case(nx, ny))
        out = tcs.Outputs(rig)
        diag = CoupledDiagnostics(rig, out, coupled_region(nx, ny), 0, 0)
        diag.attach()
        fc.run(rig, out, fc.SEVEN, abi.HALO_NONE, True)
        single = dict(diag.results(out), mean=float(out.mean[0]))
        rig.close()
        inner = lambda a: a[fc.HY:fc.HY + ny, fc.HX:fc.HX + nx].copy()  # noqa: E731
        plain = fc.make_rig(fc.folded_case(nx, ny))
        plain_out = tcs.Outputs(plain)
        per_step = []
        take = lambda: per_step.append({k: inner(v) for k, v in coupled_fields(plain_out).items()})  # noqa: E731
        fc.run(plain, plain_out, [(s, 1, abi.PIPELINE_CONTINUING) for s in range(fc.STEPS)], abi.HALO_NONE, True, between=take)
        take()
        plain.close()
        assert len(per_step) == fc.STEPS
        for k, v in per_step[-1].items():
            assert same_bytes(v, inner(single["fields"][k])), (k, "the stepped coupled run differs from the one call")
        single["per_step"] = per_step
        _COUPLED_SINGLE[(nx, ny)] = single
    return _COUPLED_SINGLE[(nx, ny)]


def _coupled_worker(rank, world, init, out):
    import coupled_fold_case as fc
    import test_coupled_steps as tcs
    import torch.distributed as dist
    from coflux.distributed import connect_coupled_slabs
    started = time.perf_counter()
    os.environ.update(HSA_ENABLE_IPC_MODE_LEGACY="0")
    dist.init_process_group("gloo", init_method=init, rank=rank, world_size=world)
    try:
        nx, ny_global = COUPLED_SURFACE
        j0, case = fc.slab_case(nx, ny_global, rank, world)
        rig = fc.make_rig(case)
        assert connect_coupled_slabs(rig.ctx) == (rank, world)
        o = tcs.Outputs(rig)
        fc.stamp(fc.exchanged_fields(rig, o, nx, ny_global), rank, world, case["ny"])       # every halo row to deliver is a naming NaN
        diag = CoupledDiagnostics(rig, o, coupled_region(nx, ny_global)[j0:j0 + case["ny"] + 2 * fc.HY], j0 * nx, nx)
        diag.attach()
        dist.barrier()
        before = fc.counters(rig.ctx)
        fc.run(rig, o, fc.SEVEN, abi.HALO_PEER, rank == world - 1)          # (cf_sync: a rank that never arrived raises here; nothing follows)
        grown = fc.grown(before, fc.counters(rig.ctx))
        dist.barrier()
        out[rank] = dict(diag.results(o), grown=grown, j0=j0, ny=case["ny"], mean=float(o.mean[0]), seconds=time.perf_counter() - started, error=None)
        rig.close()
    finally:
        dist.destroy_process_group()


def test_coupled_tripolar_slabs_hold_the_single_domains_diagnostics():
    """cf_time_steps_coupled with CF_NORMALIZE_EXACT on two tripolar slabs (the last rank's exchanges fold), seven steps: plain and
    budget means, the climatology and their weights are the single domain's bytes on the rank's rows with NaN halos; the monitor's
    combined records of net.S and of the skin temperature are the single domain's at every step, a rank's last record the
    definition's on the cut of the single domain's final fields; every integral record lies within γ(n − 1) · Σ|t| of math.fsum,
    per rank, for the single domain and combined (check_integral_series); a rank's last integrals are those of a fresh context
    that holds the cut of the single domain's final fields; the exchange counters grow as tests/test_coupled_fold_slabs.py asserts
    without attachments: (1 + 2 · steps, 0, 0, all of them on the last rank)."""
    import coupled_fold_case as fc
    world = 2
    nx, ny_global = COUPLED_SURFACE
    reports, seconds = _run_workers(_coupled_worker, world)
    print(f"coupled, {world} tripolar slabs: {seconds:.1f} s from spawn to join, of which in the worker function", [round(reports[r]["seconds"], 1) for r in range(world)])
    want = coupled_single_domain(nx, ny_global)
    HX, HY = fc.HX, fc.HY
    steps = fc.STEPS
    g = fc.global_case(nx, ny_global)
    whole = lambda a: np.asarray(a)[HY:HY + ny_global, HX:HX + nx]  # noqa: E731
    mask, region = np.asarray(g["oceans"][0]["mask"]), coupled_region(nx, ny_global)
    wet = whole(mask) != 0
    for r in range(world):
        rep = reports[r]
        j0, ny = rep["j0"], rep["ny"]
        label = ("coupled", nx, ny_global, "rank", r)
        inner = lambda a: a[..., HY:HY + ny, HX:HX + nx]  # noqa: E731
        rows = lambda a: a[..., HY + j0:HY + j0 + ny, HX:HX + nx]  # noqa: E731
        slab = lambda a: np.asarray(a)[j0:j0 + ny + 2 * HY]  # noqa: E731
        assert rep["mean"] == want["mean"], (label, rep["mean"], want["mean"])
        for k in COUPLED_FIELDS:
            assert same_bytes(inner(rep["fields"][k]), rows(want["fields"][k])), (label, k, "the field differs from the single domain's")
        for name, got, ref in ([(n, a, b) for n, a, b in zip(MEAN_NAMES, rep["means"], want["means"])] + [(n, a, b) for n, a, b in zip(BUDGET, rep["budget"], want["budget"])]
                               + [("climatology total", rep["clim_total"], want["clim_total"]), ("climatology bins", rep["clim_bins"], want["clim_bins"])]):
            same = inner(got).view(np.int64) == rows(ref).view(np.int64)
            assert same.all(), (label, name, "differs from the single domain's in", int((~same).sum()), "of", same.size, "cells")
            keep = np.ones(got.shape[-2:], dtype=bool)
            keep[HY:HY + ny, HX:HX + nx] = False
            assert np.isnan(got[..., keep]).all(), (label, name, "a halo cell of the buffer was written")
        assert rep["weights"] == want["weights"] == ((steps * STEP_SECONDS, steps), (2 * STEP_SECONDS * (steps // 2), steps // 2)), (label, rep["weights"])
        assert rep["clim_weights"] == want["clim_weights"] and rep["clim_weights"][3] == [3, 3], (label, rep["clim_weights"])
        folds = 1 + 2 * steps if r == world - 1 else 0
        assert rep["grown"] == (1 + 2 * steps, 0, 0, folds), (label, rep["grown"])
        # the last records from the interior values alone: the monitor's by the definition, the integrals' on a fresh context
        ref = [mr.monitor_value(rows(want["fields"][k]), wet[j0:j0 + ny], "value", first_cell=j0 * nx, row_length=nx) for k in ("net.S", "skin")]
        assert mr.same(rep["monitor"][0][-1], np.array(ref, dtype=mr.DTYPE)), (label, "last monitor record", rep["monitor"][0][-1], ref)
        got = fresh_context_integrals((nx, ny, HX, HY), {k: slab(want["fields"][k]) for k in ("net.T", "net.S", "fl.x_momentum")}, slab(g["area"]), slab(mask),
                                      slab(region), INTEGRANDS)
        assert same_bytes(got, rep["integrals"][0][-1]), (label, "last integrals", got, rep["integrals"][0][-1])
    values, times = zip(*[reports[r]["monitor"] for r in range(world)])
    combined = cd.combine_monitor_records(values)
    assert combined.shape == (steps, 2)
    for s in range(steps):
        for e, entry in enumerate(("net.S", "skin temperature")):
            for word in mr.DTYPE.names:
                assert combined[s, e][word].tobytes() == want["monitor"][0][s, e][word].tobytes(), \
                    ("coupled", "step", s, entry, word, combined[s, e][word], "single domain:", want["monitor"][0][s, e][word])
    assert all(np.array_equal(t, want["monitor"][1]) for t in times) and np.array_equal(want["monitor"][1], STEP_SECONDS * np.arange(1, steps + 1))
    check_integral_series(("coupled", nx, ny_global), [reports[r]["integrals"][0] for r in range(world)], want["integrals"][0], want["per_step"], whole(g["area"]), wet,
                          whole(region), [(0, nx, reports[r]["j0"], reports[r]["j0"] + reports[r]["ny"]) for r in range(world)], INTEGRANDS)
    assert all(np.array_equal(reports[r]["integrals"][1], want["integrals"][1]) for r in range(world))


# ---- in this process -------------------------------------------------------------------------------------------------------------
KNOWN = np.array([[0.0, -0.0, 1.0], [np.nan, np.inf, -1.5]])


def _monitor_record(ctx, arrays, first_cell, row_length, mask=None, hx=H, hy=H):
    dev = [ctx.to_device(rr.embed(a, hx, hy, 7.0e77)) for a in arrays]
    m = ctx.monitor([(d, "value") for d in dev], mask=mask, first_cell=first_cell, row_length=row_length, capacity=1)
    m.collect(0.0)
    got = m.read()[0][0]
    m.close()
    return got


def test_known_answer_hashes_under_every_row_length():
    """the header's known cells as a 3 × 2 interior: row_length 0 and nx = 3 give the header's hashes, nx + 5 the reference's of
    the wider numbering, with and without a first_cell"""
    from coflux.runtime import FluxContext
    ctx = FluxContext(3, 2, H, H, tts._params(), ring=tts.RING)
    for first, known in ((0, 0xbc9733db8e1747df), (1000, 0x05c59e8be3d701d6)):
        for row_length in (0, 3, 8):
            got = _monitor_record(ctx, [KNOWN], first, row_length)[0]
            want = mr.monitor_value(KNOWN, None, "value", first_cell=first, row_length=row_length)
            assert mr.same(got, want), (first, row_length, got, want)
            assert (int(got["hash"]) == known) == (row_length != 8), (first, row_length, hex(int(got["hash"])))
    ctx.close()


def test_a_negative_or_too_short_row_length_is_refused_by_name():
    import ctypes as C
    from coflux.runtime import CofluxError, FluxContext
    ctx = FluxContext(34, 5, H, H, tts._params(), ring=tts.RING)
    a = ctx.zeros()
    for row_length in (-1, 1, 33):
        with pytest.raises(CofluxError, match="row_length") as e:
            ctx.monitor([a], row_length=row_length, capacity=4)
        assert "(-1)" in str(e.value) and "cf_monitor_create" in str(e.value), str(e.value)
        desc = abi.MonitorDesc()
        desc.struct_size, desc.n_entries, desc.row_length = C.sizeof(abi.MonitorDesc), 1, row_length
        desc.entries[0].a = a.data_ptr()
        h = C.c_void_p(0xdead)
        assert ctx.lib.cf_monitor_create(ctx._h, C.byref(desc), 4, C.byref(h)) == -1 and not h.value, "no handle comes back"
    for row_length in (0, 34, 35):
        ctx.monitor([a], row_length=row_length, capacity=1).close()
    ctx.close()


@pytest.mark.parametrize("px,py", sc.WORLDS)
@pytest.mark.parametrize("masked", [False, True])
def test_tile_shaped_contexts_combine_to_the_whole_designed_array(px, py, masked):
    """every tile of the world as a context of its own in this process, holding its cut of the designed array: the combined
    record is the whole array's — the device's whole-array record and the reference's"""
    from coflux.runtime import FluxContext
    x, wet = sc.monitor_fixture()
    wet = wet if masked else None
    P = tts._params()

    def record(bounds, row_length):
        i0, i1, j0, j1 = bounds
        ctx = FluxContext(i1 - i0, j1 - j0, H, H, P, ring=tts.RING)
        mask = ctx.to_device(rr.embed(wet[j0:j1, i0:i1], H, H, 1)) if masked else None
        got = _monitor_record(ctx, [x[j0:j1, i0:i1]], j0 * sc.NX + i0, row_length, mask)
        ctx.close()
        return got

    whole = record((0, sc.NX, 0, sc.NY), 0)
    want = np.array([mr.monitor_value(x, wet, "value")], dtype=mr.DTYPE)
    assert mr.same(whole, want), (whole, want)
    per_rank = [record(tile_bounds(sc.NX, sc.NY, r, px, py), sc.NX) for r in range(px * py)]
    for r, got in enumerate(per_rank):
        i0, i1, j0, j1 = tile_bounds(sc.NX, sc.NY, r, px, py)
        ref = mr.monitor_value(x[j0:j1, i0:i1], None if wet is None else wet[j0:j1, i0:i1], "value", first_cell=j0 * sc.NX + i0, row_length=sc.NX)
        assert mr.same(got, np.array([ref], dtype=mr.DTYPE)), ((px, py), r, got, ref)
    combined = cd.combine_monitor_records(per_rank)
    for word in mr.DTYPE.names:
        assert combined[0][word].tobytes() == want[0][word].tobytes(), ((px, py), word, combined[0][word], want[0][word])
