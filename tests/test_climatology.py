"""GPU tests of the calendar-binned means accumulated on the device (include/coflux.h: cf_climatology_*, cf_attach_climatology;
the host mirror's Climatology / MonthlyClimatology).  The collection is held bit for bit to the NumPy restatement of
tests/climatology_reference.py and to real cf_average handles fed the same subsequences; every destination starts as a NaN
pattern in a guarded buffer and whole buffers are compared, so the footprint is part of every comparison; the extremes are
held to Julia's min / max restated; the step loops with an attached climatology are held to the host loop of the existing
entry points; run!(simulation) with a MonthlyClimatology is held to compute_mean_and_monthly restated on per-step fields.

The restatement is a function of the interior samples, the bins and the weights alone.  Equality with it under every halo,
offset, max_workgroups and field count is therefore the claim that the bits depend on none of those."""
import ctypes as C
import datetime as dt
import functools

import numpy as np
import pytest
import torch

import climatology_reference as cr
import util
from coflux import abi
from coflux import interface_computations as ic
from coflux import models as cm
from coflux.runtime import EXCHANGE_NAMES, FLUX_NAMES, NET_NAMES, CofluxError, FluxContext

pytestmark = pytest.mark.gpu

GUARD = 64
WINDOWS = [(5, 3), (64, 2), (65, 4), (130, 3)]       # odd and even row strides; (130, 3): more than one workgroup per field
HALOS = [(2, 7), (7, 2), (1, 1)]
NAN64 = np.array([util.SENTINEL64], dtype=np.uint64).view(np.float64)[0]


def bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def whole(view):
    """The bits of the whole buffer behind a guarded view: parent array(s), halos, gaps and guard space."""
    return util.buffer_of(view)[0].view(util.bits_dtype(view.dtype)).cpu().numpy().copy()


def poisoned(shape, offset, dtype=torch.float64):
    return util.guarded(tuple(shape), dtype, offset=offset, guard=GUARD, fill=util.SENTINEL64 if dtype == torch.float64 else util.SENTINEL32)


def expected_buffer(view, interiors, geom):
    """The buffer behind `view` (shape [..., ny + 2hy, nx + 2hx]) if nothing but the given interiors were written: `interiors`
    maps a leading index (() for a single parent array, (b,) for bin b) to the interior's values."""
    nx, ny, hx, hy = geom
    buf, first = util.buffer_of(view)
    want = np.full(buf.numel(), NAN64)
    parent = want[first:first + view.numel()].reshape(tuple(view.shape))
    for lead, values in interiors.items():
        parent[lead + (slice(hy, hy + ny), slice(hx, hx + nx))] = values
    return want.view(np.int64)


@functools.lru_cache(maxsize=None)
def samples_of(nx, ny, n_fields, n_records):
    """[record][field] → the interior sample; seeded by the window alone, shared by every halo, offset and grid."""
    rng = np.random.default_rng(1000 * nx + ny)
    out = []
    for _ in range(n_records):
        base = rng.standard_normal((ny, nx)) * 10.0 ** rng.integers(-3, 4, (ny, nx)) + rng.integers(-3, 3)
        out.append([base * (1.0 + 0.125 * f) - f for f in range(n_fields)])
    return out


class Case:
    """A climatology of n_fields fields on a context of window (nx, ny) and halos (hx, hy): sources NaN outside the interior,
    totals (None for the odd fields when `sparse_totals`) and bin blocks sentinel-filled in guarded buffers at the 8-byte
    offsets given."""

    def __init__(self, window, halo, n_fields, n_bins, max_workgroups=0, offsets=(0, 1, 0), sparse_totals=False, averagers=()):
        (nx, ny), (hx, hy) = window, halo
        self.geom = (nx, ny, hx, hy)
        self.n_fields, self.n_bins = n_fields, n_bins
        self.ctx = ctx = FluxContext(nx, ny, hx, hy, ic.flux_params(), ring=0)
        so, to, bo = offsets
        self.sources = [poisoned(ctx.shape, so) for _ in range(n_fields)]
        self.totals = [None if sparse_totals and f % 2 else poisoned(ctx.shape, to) for f in range(n_fields)]
        self.blocks = [poisoned((n_bins,) + ctx.shape, bo) for _ in range(n_fields)]
        self.clim = ctx.climatology(self.sources, self.totals, self.blocks, n_bins, max_workgroups=max_workgroups)
        self.ref = [cr.Climatology((ny, nx), n_bins, keep_total=self.totals[f] is not None) for f in range(n_fields)]
        # real cf_average handles on the fields `averagers`: one for the total, one per bin, fed the same subsequences
        self.avg = {}
        for f in averagers:
            means = [poisoned(ctx.shape, 1) for _ in range(n_bins + 1)]
            self.avg[f] = (means, [ctx.average([self.sources[f]], [m]) for m in means])

    def load(self, record):
        nx, ny, hx, hy = self.geom
        for f in range(self.n_fields):
            a = np.full(self.ctx.shape, np.nan)
            a[hy:hy + ny, hx:hx + nx] = record[f]
            self.sources[f].copy_(torch.from_numpy(a))

    def run(self, sequence):
        records = samples_of(self.geom[0], self.geom[1], self.n_fields, len(sequence))
        for item, record in zip(sequence, records):
            if item == cr.RESET:
                self.clim.reset()
                for f in range(self.n_fields):
                    self.ref[f].reset()
                for _, handles in self.avg.values():
                    for h in handles:
                        h.reset()
                continue
            b, w = item
            self.load(record)
            self.clim.collect(b, w)
            for f in range(self.n_fields):
                self.ref[f].collect(b, w, record[f])
            if b >= 0:
                for _, handles in self.avg.values():
                    handles[0].collect(w)
                    handles[1 + b].collect(w)
        self.ctx.sync()

    def check(self, what):
        """Whole buffers against the restatement: the interiors of the totals and of the bins ever hit hold its bits, every
        other word — halos, gaps between the bins, never-hit bins, guard space — holds the sentinel it started with."""
        nx, ny, hx, hy = self.geom
        inner = (slice(hy, hy + ny), slice(hx, hx + nx))
        for f in range(self.n_fields):
            ref = self.ref[f]
            hit = {b: ref.bins[b] for b in range(self.n_bins) if not np.isnan(ref.bins[b]).all()}
            got = whole(self.blocks[f])
            assert np.array_equal(got, expected_buffer(self.blocks[f], {(b,): v for b, v in hit.items()}, self.geom)), (what, f, "bins")
            if self.totals[f] is not None:
                assert np.array_equal(whole(self.totals[f]), expected_buffer(self.totals[f], {(): ref.total}, self.geom)), (what, f, "total")
            src = self.sources[f].cpu().numpy()
            halo = np.ones(self.ctx.shape, bool)
            halo[inner] = False
            assert np.isnan(src[halo]).all() and np.isfinite(src[inner]).all(), (what, f, "source")
        total, samples, bin_totals, bin_samples = self.clim.weights()
        ref = self.ref[0]
        assert (total, samples) == (ref.weight, ref.samples), what
        assert bin_totals.tolist() == ref.bin_weight and bin_samples.tolist() == ref.bin_samples, what
        for f, (means, _) in self.avg.items():
            ref = self.ref[f]
            if ref.keep_total:
                assert torch.equal(bits(means[0][inner]), bits(self.totals[f][inner])), (what, f, "cf_average total")
            for b in range(self.n_bins):
                if ref.bin_samples[b]:
                    assert torch.equal(bits(means[1 + b][inner]), bits(self.blocks[f][b][inner])), (what, f, b, "cf_average bin")

    def close(self):
        for _, handles in self.avg.values():
            for h in handles:
                h.close()
        self.clim.close()
        self.ctx.close()


# ---- 1. collection: bits and footprint -----------------------------------------------------------------------------------------
CONFIGS = {"1_field_12_bins": dict(n_fields=1, n_bins=12, max_workgroups=0, offsets=(0, 1, 0), averagers=(0,)),
           "16_fields_12_bins_7_groups": dict(n_fields=16, n_bins=12, max_workgroups=7, offsets=(1, 0, 1), sparse_totals=True, averagers=(0, 15)),
           "16_fields_1_bin_1_group": dict(n_fields=16, n_bins=1, max_workgroups=1, offsets=(1, 1, 0)),
           "1_field_32_bins": dict(n_fields=1, n_bins=32, max_workgroups=0, offsets=(0, 0, 1), averagers=(0,))}


@pytest.mark.parametrize("config", sorted(CONFIGS))
@pytest.mark.parametrize("halo", HALOS, ids=lambda h: f"halo{h[0]}x{h[1]}")
@pytest.mark.parametrize("window", WINDOWS, ids=lambda w: f"{w[0]}x{w[1]}")
def test_designed_sequence_is_the_restatement_and_the_averagers_bit_for_bit(window, halo, config):
    """The designed sequence — a bin hit once, a bin never hit, two alternating bins, unequal weights 31 / 28 / 30, −1 records,
    a reset halfway — leaves in the total and in every bin the bits of the restatement and of cf_average handles fed the same
    subsequences, under every halo, 8-mod-16 offset of source, totals and bins, max_workgroups 0 / 1 / 7, alone or with
    fifteen other fields (whose odd ones keep no total), and nothing anywhere else."""
    kw = CONFIGS[config]
    case = Case(window, halo, **kw)
    try:
        case.run(cr.designed_sequence(kw["n_bins"]))
        case.check(config)
        # field 0 holds the same bits whichever other fields ride along: its samples are the same in every config
        ref0 = cr.Climatology((window[1], window[0]), kw["n_bins"])
        for item, record in zip(cr.designed_sequence(kw["n_bins"]), samples_of(window[0], window[1], 1, len(cr.designed_sequence(kw["n_bins"])))):
            ref0.reset() if item == cr.RESET else ref0.collect(item[0], item[1], record[0])
        nx, ny, hx, hy = case.geom
        inner = (slice(hy, hy + ny), slice(hx, hx + nx))
        for b in cr.hit_after_reset(kw["n_bins"]):
            assert np.array_equal(case.blocks[0][b][inner].cpu().numpy().view(np.int64), ref0.bins[b].view(np.int64)), b
    finally:
        case.close()


@pytest.mark.parametrize("halo", HALOS, ids=lambda h: f"halo{h[0]}x{h[1]}")
@pytest.mark.parametrize("window", [(5, 3), (65, 4), (130, 3)], ids=lambda w: f"{w[0]}x{w[1]}")
def test_footprint_of_a_run_that_never_hits_most_bins(window, halo):
    """Only what follows the reset of the designed sequence, on fresh NaN-pattern buffers: bins 0, 1, 5 and 11 of twelve are
    hit.  The eight never-hit bins, the halos of every array, the gaps between consecutive bins of a block and the guard space
    keep their bits; the sources' surroundings are NaN and never enter; `weights` reports the totals and counts."""
    sequence = cr.designed_sequence(12)
    sequence = sequence[sequence.index(cr.RESET) + 1:]
    case = Case(window, halo, n_fields=3, n_bins=12, offsets=(1, 0, 1), sparse_totals=True)
    try:
        case.run(sequence)
        case.check("tail")
        total, samples, bin_totals, bin_samples = case.clim.weights()
        hit = [(b, w) for b, w in sequence if b >= 0]
        assert samples == len(hit) and total == sum(w for _, w in hit)
        assert sorted(np.nonzero(bin_samples)[0].tolist()) == [0, 1, 5, 11] == cr.hit_after_reset(12)
        for b in range(12):
            assert bin_totals[b] == sum(w for bb, w in hit if bb == b) and bin_samples[b] == sum(bb == b for bb, _ in hit)
        never = [b for b in range(12) if b not in (0, 1, 5, 11)]
        block = case.blocks[0].cpu().numpy().view(np.int64)
        assert (block[never] == np.int64(np.array([util.SENTINEL64], dtype=np.uint64).view(np.int64)[0])).all()
    finally:
        case.close()


# ---- 2. extremes --------------------------------------------------------------------------------------------------------------
def designed_bins(nx, ny):
    """Bins 1, 4, 5, 9 of twelve are non-empty.  Interior cells cycle through seven classes, so every class meets every path of
    the kernel: generic values; a NaN in bin 4; ties across bins 1, 4, 5; ±0.0 (−0.0 first in bin 4, +0.0 first in bin 1); +Inf
    and −Inf; a NaN in two bins (the first one's index); all four equal."""
    rng = np.random.default_rng(nx + 7 * ny)
    cells = nx * ny
    v = {b: rng.standard_normal(cells) * 10.0 ** rng.integers(-2, 3, cells) for b in (1, 4, 5, 9)}
    cls = np.arange(cells) % 7
    v[4][cls == 1] = np.nan
    for b in (1, 4, 5):
        v[b][cls == 2] = -2.5
    v[9][cls == 2] = 7.0
    for b, z in ((1, 0.0), (4, -0.0), (5, 0.0), (9, -0.0)):
        v[b][cls == 3] = z
    v[1][cls == 4], v[4][cls == 4], v[5][cls == 4], v[9][cls == 4] = 1.0, np.inf, -np.inf, np.inf
    v[5][cls == 5] = np.nan
    v[9][cls == 5] = np.nan
    for b in v:
        v[b][cls == 6] = 3.25
    return {b: a.reshape(ny, nx) for b, a in v.items()}


def _fill_bins(case, designed):
    """One collection into each designed bin stores the source: the bin then holds the designed values exactly."""
    for b, values in designed.items():
        case.load([values])
        case.clim.collect(b, 1.0)
        case.ref[0].collect(b, 1.0, values)


@pytest.mark.parametrize("window, halo", [((5, 3), (2, 7)), ((65, 4), (7, 2)), ((130, 3), (1, 1))], ids=["5x3", "65x4", "130x3"])
def test_extremes_are_julias_min_and_max_over_the_non_empty_bins(window, halo):
    case = Case(window, halo, n_fields=1, n_bins=12, offsets=(0, 0, 1))
    nx, ny, hx, hy = case.geom
    try:
        with pytest.raises(CofluxError, match="no available bins"):     # all empty: the reference raises too
            case.clim.extremes(0)
        designed = designed_bins(nx, ny)
        _fill_bins(case, designed)
        want = cr.julia_extremes([designed.get(b) for b in range(12)])
        assert np.isnan(want[0]).any() and np.isinf(want[0]).any() and np.signbit(want[0][want[0] == 0]).all()
        # the empty bins hold the NaN pattern they started with: poison that must not matter
        assert np.isnan(case.blocks[0][0].cpu().numpy()).all()
        for mask in range(16):      # NULL outputs in every combination
            outs = [poisoned(case.ctx.shape, k % 2, torch.float64 if k < 2 else torch.int32) if mask >> k & 1 else None for k in range(4)]
            ptrs = [C.c_void_p(t.data_ptr()) if t is not None else None for t in outs]
            assert case.ctx.lib.cf_climatology_extremes(case.clim._h, 0, *ptrs) == 0
            case.ctx.sync()
            for k, t in enumerate(outs):
                if t is None:
                    continue
                got = t[hy:hy + ny, hx:hx + nx].cpu().numpy()
                if k < 2:
                    assert cr.same_bits_but_nan_payload(got, want[k]), (mask, k)
                    # halos and guards untouched: the buffer is the sentinel but for the interior
                    inside = expected_buffer(t, {(): got}, case.geom)
                    assert np.array_equal(whole(t), inside), (mask, k)
                else:
                    assert got.dtype == np.int32 and np.array_equal(got, want[k]), (mask, k)
                    buf = whole(t)
                    first = util.buffer_of(t)[1]
                    keep = np.ones(buf.size, bool)
                    parent = keep[first:first + t.numel()].reshape(tuple(t.shape))
                    parent[hy:hy + ny, hx:hx + nx] = False
                    assert (buf[keep] == util.SENTINEL32).all(), (mask, k)
        # the mirror's call: fresh zero arrays, the same interior
        lo, hi, alo, ahi = case.clim.extremes(0)
        assert cr.same_bits_but_nan_payload(lo[hy:hy + ny, hx:hx + nx].cpu().numpy(), want[0])
        assert np.array_equal(ahi[hy:hy + ny, hx:hx + nx].cpu().numpy(), want[3])
        # a single non-empty bin: both extremes are that bin, both indices its number
        case.clim.reset()
        case.load([designed[5]])
        case.clim.collect(5, 2.0)
        lo, hi, alo, ahi = (t[hy:hy + ny, hx:hx + nx].cpu().numpy() for t in case.clim.extremes(0))
        assert cr.same_bits_but_nan_payload(lo, designed[5]) and cr.same_bits_but_nan_payload(hi, designed[5])
        assert (alo == 5).all() and (ahi == 5).all()
    finally:
        case.close()


# ---- 3. in the step loops -------------------------------------------------------------------------------------------------------
REF_DATE = dt.datetime(1958, 1, 1)
STEP_SECONDS = 10 * cm.days
ORIGIN = 15 * cm.days          # the 8 steps are stamped day 25 (Jan), 35, 45, 55 (Feb), 65, 75, 85 (Mar), 95 (Apr): three boundaries
N_STEPS = 8
TABLE = cm.calendar_bins(REF_DATE, ORIGIN, ORIGIN + (N_STEPS + 1) * STEP_SECONDS)


def step_bins(stride):
    return {s: cr.calendar_bin(*TABLE, ORIGIN + (s + 1) * STEP_SECONDS) for s in range(N_STEPS) if (s + 1) % stride == 0}


class LoopOutputs:
    """Fresh outputs of a step loop on `ctx` with what is collected from them: a climatology on three of them, an averager for
    slot 0, an integrator."""

    def __init__(self, ctx, pipeline, mask):
        self.ctx = ctx
        self.sets = [ctx.field_set(EXCHANGE_NAMES) for _ in range(2 if pipeline else 1)]
        self.fl, self.net = ctx.field_set(FLUX_NAMES), ctx.field_set(NET_NAMES)
        self.sources = [self.net["T"], self.net["S"], self.fl["sensible_heat"]]
        self.totals = [poisoned(ctx.shape, 0), None, poisoned(ctx.shape, 1)]
        self.blocks = [poisoned((12,) + ctx.shape, 1) for _ in self.sources]
        self.clim = ctx.climatology(self.sources, self.totals, self.blocks, 12)
        self.means = [poisoned(ctx.shape, 1) for _ in range(2)]
        self.average = ctx.average([self.net["u"], self.fl["latent_heat"]], self.means)
        self.integrals = ctx.integrals([("field", self.net["T"]), ("product", self.net["S"], self.fl["latent_heat"])], mask=mask, capacity=32)

    def record(self):
        iv, it = self.integrals.read()
        return dict(blocks=[whole(b) for b in self.blocks], totals=[whole(t) for t in self.totals if t is not None],
                    weights=[np.asarray(x).tolist() for x in self.clim.weights()], means=[whole(m) for m in self.means],
                    average=self.average.weight(), integrals=iv.view(np.int64).copy(), times=it.copy(),
                    fields={k: bits(v).cpu().numpy().copy() for k, v in list(self.fl.items()) + list(self.net.items())})

    def close(self):
        for h in (self.clim, self.average, self.integrals):
            h.close()


def same_record(got, want, what, keys=None):
    for k in keys or want:
        a, b = got[k], want[k]
        if isinstance(b, dict):
            assert all(np.array_equal(a[n], b[n]) for n in b), (what, k)
        elif isinstance(b, list) and b and isinstance(b[0], np.ndarray):
            assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b)), (what, k)
        elif isinstance(b, np.ndarray):
            assert np.array_equal(a, b), (what, k)
        else:
            assert a == b, (what, k)


def _host_loop(ctx, states, src, w, stride, climatology=True):
    from test_steps import INC
    out = LoopOutputs(ctx, False, states[0]["mask"])
    bins = step_bins(stride)
    for s in range(N_STEPS):
        tot = s * INC
        l1 = int(tot) % 4
        ctx.update_state(src, w, states[s % 2], out.sets[0], out.fl, out.net, level1=l1, level2=(l1 + 1) % 4, time_fraction=tot - int(tot))
        if (s + 1) % 2 == 0:
            out.average.collect(2 * 600.0)
        if climatology and s in bins:
            out.clim.collect(bins[s], stride * 1.5)
        if (s + 1) % 3 == 0:
            out.integrals.collect(ORIGIN + (s + 1) * STEP_SECONDS)
    ctx.sync()
    return out


def _device_loop(ctx, states, src, w, stride, calls, pipeline, climatology=True, table=TABLE):
    from test_steps import INC
    out = LoopOutputs(ctx, bool(pipeline), states[0]["mask"])
    sched = ctx.make_schedule(states, out.sets, first_level=0, time_fraction=0.0, time_fraction_increment=INC, pipeline=pipeline)
    ctx.attach_average(out.average, 2, 600.0)
    ctx.attach_integrals(out.integrals, 3, ORIGIN, STEP_SECONDS)
    if climatology:
        ctx.attach_climatology(out.clim, table, stride, 1.5, ORIGIN, STEP_SECONDS)
    try:
        for first, count in calls:
            ctx.time_steps(first, count, sched, src, w, out.fl, out.net)
        ctx.sync()
    finally:
        ctx.attach_average(None)
        ctx.attach_integrals(None)
        ctx.attach_climatology(None)
    return out


@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("pipeline", [False, True, "merged", "tail"])
def test_time_steps_with_an_attached_climatology_equals_the_host_loop(pipeline, stride):
    """cf_time_steps on the 24 × 12 tile, 8 steps of 10 days across three month boundaries, with the climatology attached, an
    averager in slot 0 and an integrator: the bits of the host loop of cf_update_state + cf_climatology_collect with
    Python-computed bins, whole buffers; the averager's means and the integrator's records are what they are without the
    climatology; two CF_PIPELINE_CONTINUING calls split across a month boundary give the same bits."""
    from test_steps import _setup
    assert sorted(set(step_bins(1).values())) == [0, 1, 2, 3] and len(set(step_bins(3).values())) == 2
    ctx, states, src, w, _ = _setup(nx=24, ny=12)
    try:
        want = _host_loop(ctx, states, src, w, stride).record()
        assert sum(want["weights"][3]) == N_STEPS // stride
        if pipeline in ("merged", "tail"):
            ctx.set_option(abi.OPT_MERGED_PREFETCH, 1 if pipeline == "merged" else 2)
        got = _device_loop(ctx, states, src, w, stride, [(0, N_STEPS)], bool(pipeline)).record()
        same_record(got, want, "one call")
        plain = _device_loop(ctx, states, src, w, stride, [(0, N_STEPS)], bool(pipeline), climatology=False).record()
        same_record(plain, got, "without the climatology", keys=("means", "average", "integrals", "times", "fields"))
        if pipeline:
            ctx.discard_prefetched_atmosphere_state()
            split = _device_loop(ctx, states, src, w, stride, [(0, 4), (4, 4)], abi.PIPELINE_CONTINUING).record()
            ctx.discard_prefetched_atmosphere_state()
            same_record(split, want, "4 + 4 steps, continuing")
    finally:
        ctx.close()


def test_a_call_that_would_step_past_the_table_fails_and_touches_nothing():
    from test_steps import INC, _setup
    ctx, states, src, w, _ = _setup(nx=24, ny=12)
    try:
        short = cm.calendar_bins(REF_DATE, ORIGIN, ORIGIN + 6 * STEP_SECONDS)      # ends on 1 April: step 7 (day 95) is outside
        assert short[0][-1] == 90 * cm.days
        out = LoopOutputs(ctx, False, states[0]["mask"])
        for t in list(out.fl.values()) + list(out.net.values()) + list(out.sets[0].values()):
            t.fill_(float("nan"))
        before = out.record()
        sched = ctx.make_schedule(states, out.sets, first_level=0, time_fraction=0.0, time_fraction_increment=INC)
        ctx.attach_average(out.average, 2, 600.0)
        ctx.attach_climatology(out.clim, short, 1, 1.5, ORIGIN, STEP_SECONDS)
        with pytest.raises(CofluxError, match="outside the attached climatology's calendar table"):
            ctx.time_steps(0, N_STEPS, sched, src, w, out.fl, out.net)
        ctx.sync()
        same_record(out.record(), before, "refused call")
        assert all(torch.isnan(t).all() for t in out.sets[0].values())
        ctx.time_steps(0, N_STEPS - 1, sched, src, w, out.fl, out.net)       # the steps inside the table run
        ctx.sync()
        assert out.clim.weights()[1] == N_STEPS - 1
        # with stride 3 the loop collects steps 2 and 5 only: step 7 is not collected, so the short table suffices
        ctx.attach_climatology(out.clim, short, 3, 1.5, ORIGIN, STEP_SECONDS)
        out.clim.reset()
        ctx.time_steps(0, N_STEPS, sched, src, w, out.fl, out.net)
        ctx.sync()
        assert out.clim.weights()[1] == 2
        ctx.attach_climatology(None)
        ctx.attach_average(None)
    finally:
        ctx.close()


def test_time_steps_coupled_with_an_attached_climatology_equals_the_replay():
    """The same through cf_time_steps_coupled on the designed coupled case: twelve steps in one call and as 5 + 7, against the
    host replay of the existing entry points that collects by hand, with −1 intervals in the table."""
    import coupled_case as cc
    import test_coupled_steps as tc
    rig = tc.Rig(tc.host_case(131, 37, 4, 3), merged=2)
    ctx = rig.ctx
    edges, table_bins = cm.calendar_bins(REF_DATE, ORIGIN, ORIGIN + 13 * STEP_SECONDS, start_time=ORIGIN + 2.5 * STEP_SECONDS)
    assert table_bins[0] == -1 and (table_bins >= 0).sum() >= 4

    class ByHand:
        def __init__(self, out):
            self.blocks = [poisoned((12,) + ctx.shape, 1) for _ in range(3)]
            self.totals = [poisoned(ctx.shape, 0), poisoned(ctx.shape, 1), None]
            self.clim = ctx.climatology([out.net["T"], out.net_ice["bottom_heat"], out.iof["frazil_heat"]], self.totals, self.blocks, 12)

        def collect(self, step):
            if (step + 1) % 2 == 0:
                self.clim.collect(cr.calendar_bin(edges, table_bins, ORIGIN + (step + 1) * STEP_SECONDS), 2 * 0.75)

        def record(self):
            return dict(blocks=[whole(b) for b in self.blocks], totals=[whole(t) for t in self.totals if t is not None],
                        weights=[np.asarray(x).tolist() for x in self.clim.weights()])

    try:
        want_out = tc.Outputs(rig)
        by_hand = ByHand(want_out)
        tc.replay(rig, want_out, 0, cc.N_STEPS, pipeline=abi.PIPELINE_WITHIN_CALL, collectors=by_hand)
        want = by_hand.record()
        assert want["weights"][1] == 5 and sum(want["weights"][3]) == 5       # step 1 (day 35) lies before start_time: −1
        for calls in ([(0, 12, abi.PIPELINE_WITHIN_CALL)], [(0, 5, abi.PIPELINE_CONTINUING), (5, 7, abi.PIPELINE_CONTINUING)]):
            if len(calls) == 2:
                want_out = tc.Outputs(rig)
                by_hand.clim.close()
                by_hand = ByHand(want_out)
                tc.replay(rig, want_out, 0, cc.N_STEPS, pipeline=abi.PIPELINE_CONTINUING, collectors=by_hand)
                want = by_hand.record()
            got_out = tc.Outputs(rig)
            attached = ByHand(got_out)
            ctx.attach_climatology(attached.clim, (edges, table_bins), 2, 0.75, ORIGIN, STEP_SECONDS)
            tc.coupled(rig, got_out, calls)
            ctx.attach_climatology(None)
            same_record(attached.record(), want, f"{len(calls)} call(s)")
            tc.assert_same_bits(got_out.bits(), want_out.bits(), "outputs under the attached climatology")
            attached.clim.close()
        by_hand.clim.close()
    finally:
        rig.close()


# ---- 4. the mirror -------------------------------------------------------------------------------------------------------------
def _reference_mean_and_monthly(times, fields):
    """compute_mean_and_monthly (visualize/common.jl:191-208) restated: sums and counts, in extended precision so that the
    reference's own rounding (2⁻⁶⁴ per addition) is far below the bound the device's recurrence is held to."""
    total = sum(f.astype(np.longdouble) for f in fields) / len(fields)
    monthly = {}
    for t, f in zip(times, fields):
        m = (REF_DATE + dt.timedelta(seconds=round(t))).month
        monthly.setdefault(m, []).append(f.astype(np.longdouble))
    return total, {m: sum(fs) / len(fs) for m, fs in monthly.items()}


def _within_bound(got, want, members):
    """|got − want| ≤ (3n + 2) · 2⁻⁵³ · M per cell, M the cell's largest |sample| (tests/test_climatology_cpu.py counts it)."""
    M = np.max(np.abs(np.stack(members)), axis=0).astype(np.longdouble)
    bound = (3 * len(members) + 2) * np.longdouble(2.0) ** -53 * M
    return bool((np.abs(got.astype(np.longdouble) - want) <= bound).all())


def test_run_with_a_monthly_climatology_matches_compute_mean_and_monthly():
    """run!(simulation) with a MonthlyClimatology on the sea-ice concentration and two flux fields, 8 steps of 10 days: January,
    February and March are visited; .month is None exactly for the other nine; the visited months and .mean are within the
    counted bound of compute_mean_and_monthly restated on the per-step fields of a host loop; models.time_steps with the
    writer attached gives means within the same bound; sea_ice_concentration_climatology gives what sic_mean, sic_march and
    sic_september read."""
    from test_time_average import NX, NY, H, _model, interior
    dt_step = 10 * cm.days

    def outputs(model):
        itf = model.interfaces
        return dict(sic=model.sea_ice.concentration, hfds=itf.net_fluxes.ocean.T, hfss=itf.atmosphere_ocean_interface.fluxes.sensible_heat)

    ref = _model(True)
    per_step, times = {k: [] for k in outputs(ref)}, []
    for _ in range(8):
        cm.time_step(ref, dt_step)
        times.append(ref.clock.time)
        for k, v in outputs(ref).items():
            per_step[k].append(interior(v.cpu().numpy(), NX, NY, H, H).copy())
    ref.interfaces.context.close()
    assert [(REF_DATE + dt.timedelta(seconds=t)).month for t in times] == [1, 1, 1, 2, 2, 3, 3, 3]

    def check(writer, what):
        for name in ("sic", "hfds", "hfss"):
            mean, monthly = _reference_mean_and_monthly(times, per_step[name])
            assert _within_bound(writer.mean(name), mean, per_step[name]), (what, name)
            for m in range(1, 13):
                got = writer.month(name, m)
                assert (got is None) == (m not in monthly), (what, name, m)
                if got is not None:
                    members = [f for t, f in zip(times, per_step[name]) if (REF_DATE + dt.timedelta(seconds=round(t))).month == m]
                    assert got.shape == (NY, NX) and _within_bound(got, monthly[m], members), (what, name, m)
        lo, hi, alo, ahi = writer.extremes("hfds")
        want = cr.julia_extremes([writer.month("hfds", m) for m in range(1, 13)])
        assert cr.same_bits_but_nan_payload(lo, want[0]) and cr.same_bits_but_nan_payload(hi, want[1])
        assert np.array_equal(alo, want[2] + 1) and np.array_equal(ahi, want[3] + 1) and set(np.unique(alo)) <= {1, 2, 3}

    model = _model(True)
    writer = cm.MonthlyClimatology(model, outputs(model))
    with pytest.raises(ValueError, match="no available monthly bins"):
        writer.extremes("sic")
    assert writer.mean("sic") is None and writer.month("sic", 3) is None
    sic = cm.sea_ice_concentration_climatology(model)
    sim = cm.Simulation(model, dt=dt_step, stop_iteration=8, output_writers={"monthly": writer, "sic": sic})
    cm.run(sim)
    check(writer, "run")
    assert writer.climatology.weights()[1] == 8 and writer.climatology.weights()[3].tolist() == [3, 2, 3] + [0] * 9
    assert sic.month("sic", 9) is None and np.array_equal(sic.month("sic", 3), writer.month("sic", 3)) and np.array_equal(sic.mean("sic"), writer.mean("sic"))
    writer.close()
    sic.close()
    model.interfaces.context.close()

    model = _model(True)
    writer = cm.MonthlyClimatology(model, outputs(model))
    cm.time_steps(model, dt_step, 8, climatology=writer)
    model.interfaces.context.sync()
    check(writer, "time_steps")
    assert writer.climatology.weights()[3].tolist() == [3, 2, 3] + [0] * 9
    writer.close()
    model.interfaces.context.close()


# ---- 5. errors ----------------------------------------------------------------------------------------------------------------
def test_errors():
    ctx = FluxContext(40, 12, 2, 2, ic.flux_params(), ring=1)
    lib, n = ctx.lib, 16 * 44
    a, b, t = ctx.zeros(), ctx.zeros(), ctx.zeros()
    block = torch.zeros((12,) + ctx.shape, dtype=torch.float64, device="cuda")

    def create(**kw):
        desc = abi.ClimatologyDesc()
        desc.struct_size, desc.n_fields, desc.n_bins = C.sizeof(abi.ClimatologyDesc), 1, 12
        desc.sources[0], desc.totals[0], desc.bins[0] = a.data_ptr(), t.data_ptr(), block.data_ptr()
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(desc, k)[v[0]] = v[1]
            else:
                setattr(desc, k, v)
        h = C.c_void_p()
        rc = lib.cf_climatology_create(ctx._h, C.byref(desc), C.byref(h))
        assert (rc == 0) == bool(h.value)
        if h.value:
            lib.cf_climatology_destroy(h)
        return rc, lib.cf_last_error(None).decode()

    assert create()[0] == 0
    for kw, text in ((dict(struct_size=400), "struct_size"), (dict(n_fields=0), "0 fields"), (dict(n_fields=17), "17 fields"),
                     (dict(n_bins=0), "0 bins"), (dict(n_bins=33), "33 bins"), (dict(sources=(0, None)), "NULL source or bins"),
                     (dict(bins=(0, None)), "NULL source or bins"), (dict(max_workgroups=-1), "max_workgroups"),
                     (dict(reserved=(1, 1)), "reserved"), (dict(totals=(0, a.data_ptr())), "total of field 0 overlaps source 0"),
                     (dict(bins=(0, a.data_ptr()), totals=(0, None)), "bin block of field 0 overlaps source 0"),
                     # the whole block is the bin's parent-array rule: a total that starts inside the LAST bin overlaps it
                     (dict(totals=(0, block.data_ptr() + 8 * (11 * n + 5))), "overlaps the bin block"),
                     # … and a source one element before the block's end does
                     (dict(sources=(0, block.data_ptr() + 8 * (12 * n - 1))), "overlaps source 0")):
        rc, msg = create(**kw)
        assert rc == -1 and text in msg, (kw, msg)
    # two fields whose bin blocks share bytes
    desc = abi.ClimatologyDesc()
    desc.struct_size, desc.n_fields, desc.n_bins = C.sizeof(abi.ClimatologyDesc), 2, 6
    desc.sources[0], desc.sources[1], desc.bins[0], desc.bins[1] = a.data_ptr(), b.data_ptr(), block.data_ptr(), block.data_ptr() + 8 * (5 * n + 3)
    h = C.c_void_p()
    assert lib.cf_climatology_create(ctx._h, C.byref(desc), C.byref(h)) == -1 and not h.value and "overlaps the bin block of field 1" in lib.cf_last_error(None).decode()
    desc.bins[1] = block.data_ptr() + 8 * 6 * n       # back to back: legal
    assert lib.cf_climatology_create(ctx._h, C.byref(desc), C.byref(h)) == 0
    lib.cf_climatology_destroy(h)
    assert lib.cf_climatology_create(None, C.byref(desc), C.byref(h)) == -1 and lib.cf_climatology_create(ctx._h, None, C.byref(h)) == -1

    clim = ctx.climatology([a], [t], [block], 12)
    for bin_ in (-2, 12, 100):
        with pytest.raises(CofluxError, match="bin"):
            clim.collect(bin_, 1.0)
    for wgt in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(CofluxError, match="weight"):
            clim.collect(3, wgt)
        with pytest.raises(CofluxError, match="weight"):
            clim.collect(-1, wgt)
    clim.collect(-1, 1.0)
    assert clim.weights()[:2] == (0.0, 0) and not clim.weights()[3].any()
    with pytest.raises(CofluxError, match="field"):
        clim.extremes(1)
    with pytest.raises(CofluxError, match="no available bins"):
        clim.extremes(0)
    table = (np.array([0.0, 10.0, 20.0]), np.array([0, 11], dtype=np.int32))
    ctx.attach_climatology(clim, table, 1, 1.0, 0.0, 1.0)
    for args, text in (((0, 1.0, 0.0, 1.0), "stride"), ((1, 0.0, 0.0, 1.0), "step weight"), ((1, float("inf"), 0.0, 1.0), "step weight"),
                       ((1, 1.0, float("nan"), 1.0), "time origin"), ((1, 1.0, 0.0, float("inf")), "step")):
        with pytest.raises(CofluxError, match=text):
            ctx.attach_climatology(clim, table, *args)
    for bad, text in (((np.array([0.0, 10.0, 10.0]), table[1]), "strictly increasing"), ((np.array([0.0, 20.0, 10.0]), table[1]), "strictly increasing"),
                      ((np.array([5.0]), np.zeros(0, dtype=np.int32)), "n_edges"), ((table[0], np.array([0, 12], dtype=np.int32)), "12 bins"),
                      ((table[0], np.array([-2, 1], dtype=np.int32)), "−1 or a bin")):
        with pytest.raises(CofluxError, match=text):
            ctx.attach_climatology(clim, bad, 1, 1.0, 0.0, 1.0)
    assert lib.cf_attach_climatology(ctx._h, clim._h, 1, 1.0, 0.0, 1.0, None, None, 3) == -1
    other = FluxContext(40, 12, 2, 2, ic.flux_params(), ring=1)
    with pytest.raises(CofluxError, match="another context"):
        other.attach_climatology(clim, table, 1, 1.0, 0.0, 1.0)
    other.close()
    # destroying an attached climatology detaches it; one outlived by its context fails every call but destroy
    clim.close()
    orphan = ctx.climatology([a], [t], [block], 12)
    ctx.attach_climatology(orphan, table, 1, 1.0, 0.0, 1.0)
    ctx.close()
    for call in (lambda: orphan.collect(0, 1.0), orphan.reset, orphan.weights, lambda: orphan.extremes(0)):
        with pytest.raises(CofluxError, match="destroyed"):
            call()
    orphan.close()


def test_destroying_an_attached_climatology_detaches_it():
    from test_steps import INC, _setup
    ctx, states, src, w, _ = _setup(nx=24, ny=12)
    try:
        out = LoopOutputs(ctx, False, states[0]["mask"])
        sched = ctx.make_schedule(states, out.sets, first_level=0, time_fraction=0.0, time_fraction_increment=INC)
        ctx.attach_climatology(out.clim, TABLE, 1, 1.0, ORIGIN, STEP_SECONDS)
        out.clim.close()
        before = [whole(b) for b in out.blocks]
        ctx.time_steps(0, 3, sched, src, w, out.fl, out.net)
        ctx.sync()
        assert all(np.array_equal(x, whole(b)) for x, b in zip(before, out.blocks))
        assert torch.isfinite(out.net["T"]).all()
    finally:
        ctx.close()
