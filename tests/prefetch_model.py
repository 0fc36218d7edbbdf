"""The contract of an atmosphere state requested AHEAD of its step, as a plain host model — written from the text of
include/coflux.h (cf_prefetch_atmosphere_state, cf_discard_prefetched_atmosphere_state, cf_window_commit, cf_time_steps with
CF_PIPELINE_*), not from the library's sources — and the atlas of operation sequences that tests/test_prefetch_sequences.py
runs on the device and tests/test_prefetch_model_cpu.py checks on the host.  No GPU, nothing of coflux.runtime.

What the model tracks:
  * per window slot its contents (time index n, generation g); every commit of a slot bumps its generation;
  * per exchange set the request that is pending for it — source, weights, levels, fraction, and the slot contents at the time
    of the request — and what the set's memory holds once everything queued has run;
  * CF_OPT_MERGED_PREFETCH and CF_OPT_FUSED_NET.
For a sequence of operations it predicts, per step, the atmosphere that step must see — Atmos(source, contents of level 1,
contents of level 2, weights, level1, level2, fraction) — and the counters of cf_debug_prefetch_stats after every operation.
The route counters follow from the mode, CF_OPT_FUSED_NET, whether the step is a sea-ice step and whether the tiled
interpolation fits the launch that would carry it (CF_OPT_INTERP_TILE_CAP), nothing else.

Designed data (snapshot()): variable v of time index n in generation g of source s is the synthetic JRA55 snapshot n plus
n·A_V[v] + g·B_V[v] and a zonal wave of amplitude B_V[v] whose wavenumber names the source, and every commit of the atlas
brings a time index its slot has not held, so that two different Atmos tuples of the atlas are different fields by far more
than any tolerance (tests/test_prefetch_model_cpu.py asserts the margins on the reference alone).

DEFECTS are seven deliberately wrong variants of the model; each must predict another atmosphere for some named step of the
atlas (test_prefetch_model_cpu.py records which), or the atlas is missing a case."""
import functools
import math
import random
from collections import namedtuple

import numpy as np

NX, NY, H, RING = 192, 48, 4, 1          # the step shape of tests/test_steps.py: the tail and merged forms engage here
N_SLOTS = 4                              # slots of a window = levels of an in-memory atmosphere
N_BASE = 12                              # synthetic snapshots behind the time indices 0 … 11: every commit brings a new one
INC, TF0 = 1.0 / 8.0, 1.0 / 16.0         # clock of the cf_time_steps cases: odd sixteenths, never 0 (where level 2 would not count)
WINDOWS = ("W", "V")                     # two snapshot windows …
MEMORY = ("M", "N")                      # … and two in-memory atmospheres of the same shape and levels, all with other data
SOURCES = WINDOWS + MEMORY
WEIGHTS = ("lat", "lat_half", "general")  # the lat-lon map, the same half a source row further north, a rotated general map
SETS = ("A", "B", "C")
# the tile of the tiled interpolation is 4 waves × 9 variables × cap doubles of LDS: the face-stress launch has 64 KiB for it,
# the tail workgroups of a solver launch 40 KiB (include/coflux.h, cf_prefetch_atmosphere_state)
TILE_CAP_DEFAULT, TILE_CAP_MERGED, TILE_CAP_TAIL = 128, 65536 // 288, 40960 // 288

ROUTES = ("launched_aux", "launched_tail", "launched_merged", "launched_ice_tail", "launched_own")
OUTCOMES = ("consumed", "mismatched", "voided", "superseded", "discarded")
COUNTERS = ("requests",) + ROUTES + OUTCOMES + ("step_interpolations", "pending")

DEFECTS = ("ignore_commits", "ignore_fraction", "ignore_source", "ignore_weights", "discard_forgets_deferred_only",
           "supersede_keeps_old", "continuing_trusts_pending")

# ---------------------------------------------------------------------------------------------
# operations
# ---------------------------------------------------------------------------------------------
Request = namedtuple("Request", "set src w l1 l2 tf")
Step = namedtuple("Step", "set src w l1 l2 tf ocean ice", defaults=(0, False))
Write = namedtuple("Write", "set src w l1 l2 tf")            # the host interpolates into a set itself (legal only when nothing is pending for it)
Commit = namedtuple("Commit", "window slot n")               # upload time index n into the slot: a new generation
Discard = namedtuple("Discard", "")
Sync = namedtuple("Sync", "")
SetMode = namedtuple("SetMode", "mode")                      # CF_OPT_MERGED_PREFETCH
SetFusedNet = namedtuple("SetFusedNet", "value")             # CF_OPT_FUSED_NET: 0 or 2
SetStream = namedtuple("SetStream", "which")                 # "side": a torch side stream, "own": back
SetTileCap = namedtuple("SetTileCap", "cap")                 # CF_OPT_INTERP_TILE_CAP (an experiment option): 0 or 16 … 224 cells
# cf_time_steps over the sets (A, B) — (A) alone without pipelining — and the two ocean states, step s at fraction tf0 + s·inc
TimeSteps = namedtuple("TimeSteps", "first n pipeline src w first_level tf0 inc", defaults=(0, TF0, INC))

Atmos = namedtuple("Atmos", "src c1 c2 w l1 l2 tf")          # c = (time index, generation) of the level's contents


class ContractViolation(Exception):
    """The sequence does what include/coflux.h forbids (the host writes a set a request is pending for, …)."""


def clock(op, step):
    """(level1, level2, fraction) of global step `step` of a TimeSteps operation: cf_run_schedule's arithmetic."""
    total = op.tf0 + float(step) * op.inc
    whole = math.floor(total)
    l1 = (op.first_level + int(whole)) % N_SLOTS
    return l1, (l1 + 1) % N_SLOTS, total - whole


class _Req:
    __slots__ = ("src", "w", "l1", "l2", "tf", "atmos", "route")

    def __init__(self, src, w, l1, l2, tf, atmos):
        self.src, self.w, self.l1, self.l2, self.tf, self.atmos, self.route = src, w, l1, l2, tf, atmos, None


class Model:
    def __init__(self, mode=0, fused_net=2, defects=()):
        assert set(defects) <= set(DEFECTS)
        self.mode, self.fused_net, self.defects = mode, fused_net, frozenset(defects)
        self.tile_cap = TILE_CAP_DEFAULT
        self.slots = {w: [(s, 0) for s in range(N_SLOTS)] for w in WINDOWS}
        self.pending = {}      # set → _Req
        self.waiting = None    # the set whose request has not left yet (at most one)
        self.holds = {}        # set → Atmos in its memory once everything queued has run
        self.c = dict.fromkeys(COUNTERS, 0)

    # -- what a source holds -------------------------------------------------------------------
    def content(self, src, level):
        return self.slots[src][level] if src in WINDOWS else (level, 0)

    def atmosphere(self, src, w, l1, l2, tf):
        return Atmos(src, self.content(src, l1), self.content(src, l2), w, l1, l2, tf)

    # -- the life of a request -----------------------------------------------------------------
    def _leaves(self, route):
        s, self.waiting = self.waiting, None
        self.c[route] += 1
        self.pending[s].route = route
        self.holds[s] = self.pending[s].atmos

    def _flush(self):
        """cf_sync, another request, a step into the request's own set: a request that has not left leaves on the auxiliary stream."""
        if self.waiting is not None:
            self._leaves("launched_aux")

    def _route(self, ice):
        if self.mode == 0:
            return "launched_aux"
        if self.mode == 1:
            return "launched_merged" if self.fused_net != 0 and 0 < self.tile_cap <= TILE_CAP_MERGED else "launched_own"
        if not 0 < self.tile_cap <= TILE_CAP_TAIL:
            return "launched_own"
        if ice:
            return "launched_ice_tail"
        return "launched_tail" if self.fused_net != 0 else "launched_own"

    def _matches(self, r, src, w, l1, l2, tf):
        return ((r.src == src or "ignore_source" in self.defects) and (r.w == w or "ignore_weights" in self.defects) and
                (r.l1, r.l2) == (l1, l2) and (r.tf == tf or "ignore_fraction" in self.defects))

    def _end(self, s, outcome):
        del self.pending[s]
        self.c[outcome] += 1
        if self.waiting == s:
            self.waiting = None

    def _room(self, s):
        return s in self.pending or len(self.pending) < 2

    def _request(self, s, src, w, l1, l2, tf):
        """False: refused (two other sets are pending)."""
        self._flush()
        if not self._room(s):
            return False
        atmos = self.atmosphere(src, w, l1, l2, tf)
        self.c["requests"] += 1
        if s in self.pending and "supersede_keeps_old" in self.defects:
            self.c["superseded"] += 1       # (the NEW request is forgotten; its kernel still writes the set)
            self.holds[s] = atmos
            return True
        if s in self.pending:
            self._end(s, "superseded")
        self.pending[s] = _Req(src, w, l1, l2, tf, atmos)
        self.waiting = s
        return True

    def _step(self, s, src, w, l1, l2, tf, ice, trust=False):
        if self.waiting == s:
            self._flush()
        now = self.atmosphere(src, w, l1, l2, tf)
        r = self.pending.get(s)
        if r is not None and (trust or self._matches(r, src, w, l1, l2, tf)):
            self._end(s, "consumed")
            sees = self.holds[s]
            assert self.defects or sees == now, (sees, now)
        else:
            if r is not None:
                self._end(s, "mismatched")
            self.c["step_interpolations"] += 1
            self.holds[s] = sees = now
        if self.waiting is not None:      # a request into another set leaves with this step
            self._leaves(self._route(ice))
        return sees

    def _time_steps(self, op):
        sets = ("A", "B") if op.pipeline else ("A",)
        end, sees, trust = op.first + op.n, [], False
        if op.pipeline and op.n > 0:      # the first step's atmosphere, unless it is pending already
            s0, k0 = sets[op.first % 2], clock(op, op.first)
            r = self.pending.get(s0)
            trust = r is not None and "continuing_trusts_pending" in self.defects
            if r is not None and (trust or self._matches(r, op.src, op.w, *k0)):
                if self.waiting == s0:
                    self._flush()
            else:
                self._flush()
                if not self._room(s0):
                    raise ContractViolation("cf_time_steps with two other sets pending")
                if s0 in self.pending:
                    self._end(s0, "superseded")
                atmos = self.atmosphere(op.src, op.w, *k0)
                self.c["requests"] += 1
                self.pending[s0] = _Req(op.src, op.w, *k0, atmos)
                self.waiting = s0
                self._leaves("launched_aux" if self.mode == 0 else "launched_own")
        for step in range(op.first, end):
            if op.pipeline and (step + 1 < end or op.pipeline == 2):
                if not self._request(sets[(step + 1) % 2], op.src, op.w, *clock(op, step + 1)):
                    raise ContractViolation("cf_time_steps with a third set pending")
            sees.append(self._step(sets[step % len(sets)], op.src, op.w, *clock(op, step), False, trust and step == op.first))
        return sees

    def legal(self, op):
        if isinstance(op, Write):
            return op.set not in self.pending
        if isinstance(op, TimeSteps):
            return "C" not in self.pending
        if isinstance(op, Commit):
            return op.n % N_SLOTS == op.slot and self.slots[op.window][op.slot][0] < op.n < N_BASE
        return True

    def apply(self, op):
        """Runs one operation; returns dict(sees = the Atmos of every step it ran, refused, counters = a copy after it, on_main)."""
        if not self.defects and not self.legal(op):      # (a defective variant may think a set pending that is not)
            raise ContractViolation(repr(op))
        sees, refused = [], False
        if isinstance(op, Request):
            refused = not self._request(*op)
        elif isinstance(op, Step):
            sees = [self._step(op.set, op.src, op.w, op.l1, op.l2, op.tf, op.ice)]
        elif isinstance(op, Write):
            self.holds[op.set] = self.atmosphere(*op[1:])
        elif isinstance(op, Commit):
            if "ignore_commits" not in self.defects:
                for s, r in list(self.pending.items()):      # by slot NUMBER, of whichever source
                    if op.slot in (r.l1, r.l2):
                        self._end(s, "voided")
            self.slots[op.window][op.slot] = (op.n, self.slots[op.window][op.slot][1] + 1)
        elif isinstance(op, Discard):
            for s in list(self.pending):
                if "discard_forgets_deferred_only" not in self.defects or s == self.waiting:
                    self._end(s, "discarded")
        elif isinstance(op, Sync):
            self._flush()
        elif isinstance(op, SetMode):
            self.mode = op.mode
        elif isinstance(op, SetFusedNet):
            self.fused_net = op.value
        elif isinstance(op, SetTileCap):
            self.tile_cap = op.cap
        elif isinstance(op, SetStream):
            pass
        elif isinstance(op, TimeSteps):
            sees = self._time_steps(op)
        else:
            raise TypeError(op)
        self.c["pending"] = len(self.pending)
        assert self.c["requests"] == sum(self.c[k] for k in OUTCOMES) + self.c["pending"], self.c
        on_main = any(r.route not in (None, "launched_aux") for r in self.pending.values())   # left on the context's stream, not consumed yet
        return dict(sees=sees, refused=refused, counters=dict(self.c), on_main=on_main)


def predict(mode, ops, defects=()):
    m = Model(mode, defects=defects)
    return [m.apply(op) for op in ops]


# ---------------------------------------------------------------------------------------------
# the atlas
# ---------------------------------------------------------------------------------------------
K0, K1, K2 = (0, 1, 0.25), (1, 2, 0.75), (0, 1, 0.5)
K1L, K1T = (2, 3, 0.75), (1, 2, 0.5)     # K1's fraction at other levels, K1's levels at another fraction


def S(s, k, src="W", w="lat", ocean=0, ice=False):
    return Step(s, src, w, k[0], k[1], k[2], ocean, ice)


def R(s, k, src="W", w="lat"):
    return Request(s, src, w, *k)


def readers(s, k=K0, ice=False):
    """Three steps that read set `s`, queued ahead of whatever overwrites it (or a slot they read) next: a missing order then
    LIKELY shows in their results — not certainly."""
    return [S(s, k, ocean=n % 2, ice=ice) for n in range(3)]


def _consume(m):
    return [R("B", K1), S("A", K0), S("B", K1, ocean=1)]


def _time_mismatch(m):
    return [R("B", K1), S("A", K0), S("B", K1T, ocean=1)]


def _level_mismatch(m):
    return [R("B", K1), S("A", K0), S("B", K1L, ocean=1)]


def _source_mismatch(m):
    return [R("B", K1, src="M"), S("A", K0), S("B", K1, src="N"),          # two in-memory atmospheres
            R("A", K1, src="W"), S("B", K0), S("A", K1, src="V"),          # two windows
            R("B", K1, src="W"), S("A", K0), S("B", K1, src="M")]          # a window and a re-bound in-memory one


def _weights_mismatch(m):
    return [R("B", K1, w="lat"), S("A", K0), S("B", K1, w="lat_half"),
            R("A", K1, w="lat"), S("B", K0), S("A", K1, w="general"),
            R("B", K1, w="general"), S("A", K0, w="general"), S("B", K1, w="general", ocean=1)]   # (and the general map consumed)


def _commit_voids_aux(m):
    return readers("B") + [R("B", K1), Sync(), Commit("W", 1, 5), S("B", K1)]


def _commit_voids_deferred(m):
    return readers("B") + [R("B", K1), Commit("W", 1, 5), S("B", K1)]


def _commit_voids_on_main(m):       # (mode 0: the auxiliary stream again, this time behind a step)
    return readers("B") + [R("B", K1), S("A", K0), Commit("W", 2, 6), S("B", K1)]


def _commit_other_slot_keeps(m):
    return [R("B", K1), S("A", K0), Commit("W", 3, 7), S("B", K1, ocean=1)]


def _commit_of_another_window(m):   # voiding goes by slot number alone: a false void, an interpolation more, the right field
    return [R("B", K1), S("A", K0), Commit("V", 1, 5), S("B", K1, ocean=1)]


FIRST_CALL = TimeSteps(0, 8, 2, "W", "lat")


def _continuing(between=(), one_step=False, **second):
    """21 steps in continuing calls: 8, whatever happens in between, then 13 — or, so that the step that meets the pending
    state is the LAST of a call and what it computed is there to be compared, 1 and 12."""
    call = TimeSteps(8, 13, 2, "W", "lat")._replace(**second)
    rest = [call._replace(n=1), call._replace(first=9, n=12)] if one_step else [call]
    return lambda m: [FIRST_CALL] + list(between) + rest


# step 8 (fraction 1/16 + 8/8: levels 1 and 2) would consume what the first call's last step requested
_CONTINUING = {
    "continuing_split": dict(),
    "continuing_split_recommit": dict(between=[Commit("W", 1, 5)]),
    "continuing_split_clock_change": dict(tf0=2 * TF0),
    "continuing_split_source_change": dict(src="V"),
    "continuing_split_weights_change": dict(w="lat_half"),
}


def _continuing_stop_discard(m):    # step 8 would have used set A
    return [FIRST_CALL, Discard(), Write("A", "W", "lat", *K2), S("A", clock(FIRST_CALL, 8)), S("A", K1, ocean=1)]


def _within_call(m):                # (not continuing: nothing is pending behind the call)
    return [TimeSteps(0, 5, 1, "M", "lat"), TimeSteps(5, 4, 0, "M", "lat"), TimeSteps(9, 3, 1, "M", "lat")]


def _discard(how):
    def build(m):
        out = {"aux": [Sync()], "deferred": [], "on_main": [S("A", K0)]}[how]
        return (readers("B") + [R("B", K1)] + out + [Discard(), Write("B", "W", "lat", *K2), S("B", K1)] +     # at the discarded clock
                [R("B", K1)] + out + [Discard(), S("B", K2, ocean=1)])                                        # and at another
    return build


def _mode_switch(a, b):
    return lambda m: [SetMode(a), R("B", K1), SetMode(b), S("A", K0), S("B", K1, ocean=1)]


def _mode_switch_direct(a, b):
    return lambda m: [SetMode(a)] + readers("B") + [R("B", K1), SetMode(b), S("B", K1, ocean=1)]


def _mode_switch_supersede(a, b):   # an auxiliary-stream launch nobody consumed, superseded under the other mode
    return lambda m: [SetMode(a), R("B", K1), Sync(), SetMode(b), R("B", K2), S("A", K0), S("B", K2, ocean=1)]


def _no_merged_form(m):
    return [SetFusedNet(0), R("B", K1), S("A", K0), S("B", K1, ocean=1), SetFusedNet(2)]


def _tile_does_not_fit(m):          # 224 cells fit the face-stress launch, not the tail workgroups; 0: no tiled interpolation at all
    return [SetTileCap(224), R("B", K1), S("A", K0), S("B", K1, ocean=1), SetTileCap(0), R("A", K2), S("B", K1), S("A", K2, ocean=1),
            SetTileCap(TILE_CAP_DEFAULT)]


def _ice_tile_does_not_fit(m):
    return [SetTileCap(224), R("B", K1), S("A", K0, ice=True), S("B", K1, ocean=1, ice=True), SetTileCap(TILE_CAP_DEFAULT)]


def _request_into_current_set(m):
    return readers("A") + [R("A", K1), S("A", K1, ocean=1), R("A", K2), S("A", K0)]     # consumed; then the existing mismatch case


def _both_sets_pending(m):
    return [R("A", K0), R("B", K1), R("C", K2), S("A", K0), S("B", K1, ocean=1), S("C", K2),
            R("A", K0), S("C", K2), R("B", K1), R("C", K2), R("A", K2), S("B", K1), S("A", K2, ocean=1)]


def _sync_flush(m):
    return readers("B") + [R("B", K1), Sync(), S("B", K1, ocean=1)]


def _set_stream_pending(m):
    return [R("B", K1), S("A", K0), SetStream("side"), S("B", K1, ocean=1), SetStream("own")]


def _supersede_then_old_clock(m):
    return [R("B", K1), S("A", K0), R("B", K2), S("A", K0, ocean=1), S("B", K1)]


def _ice_consume(m):
    return [R("B", K1), S("A", K0, ice=True), S("B", K1, ocean=1, ice=True)]


def _ice_time_mismatch(m):
    return [R("B", K1), S("A", K0, ice=True), S("B", K1T, ocean=1, ice=True)]


def _ice_commit_voids_deferred(m):
    return readers("B", ice=True) + [R("B", K1), Commit("W", 1, 5), S("B", K1, ice=True)]


def _ice_commit_voids_tail(m):
    return readers("B", ice=True) + [R("B", K1), S("A", K0, ice=True), Commit("W", 2, 6), S("B", K1, ice=True)]


def _ice_and_ocean_steps(m):        # an ocean-only step carries the request of a sea-ice step and the other way round
    return [R("B", K1), S("A", K0), S("B", K1, ocean=1, ice=True), R("A", K2), S("B", K1, ice=True), S("A", K2)]


ALL_MODES = (0, 1, 2)
_NAMED = {
    "consume": (ALL_MODES, _consume), "time_mismatch": (ALL_MODES, _time_mismatch), "level_mismatch": (ALL_MODES, _level_mismatch),
    "source_mismatch": (ALL_MODES, _source_mismatch), "weights_mismatch": (ALL_MODES, _weights_mismatch),
    "commit_voids_aux": (ALL_MODES, _commit_voids_aux), "commit_voids_deferred": (ALL_MODES, _commit_voids_deferred),
    "commit_voids_on_main": (ALL_MODES, _commit_voids_on_main), "commit_other_slot_keeps": (ALL_MODES, _commit_other_slot_keeps),
    "commit_of_another_window": (ALL_MODES, _commit_of_another_window),
    "continuing_stop_discard": (ALL_MODES, _continuing_stop_discard), "within_call": (ALL_MODES, _within_call),
    "discard_aux": (ALL_MODES, _discard("aux")), "discard_deferred": (ALL_MODES, _discard("deferred")),
    "discard_on_main": (ALL_MODES, _discard("on_main")),
    "no_merged_form": ((1, 2), _no_merged_form), "tile_does_not_fit": (ALL_MODES, _tile_does_not_fit),
    "ice_tail_tile_does_not_fit": ((2,), _ice_tile_does_not_fit), "request_into_current_set": (ALL_MODES, _request_into_current_set),
    "both_sets_pending": (ALL_MODES, _both_sets_pending), "sync_flush": (ALL_MODES, _sync_flush),
    "set_stream_pending": (ALL_MODES, _set_stream_pending), "supersede_then_old_clock": (ALL_MODES, _supersede_then_old_clock),
    "ice_tail_consume": (ALL_MODES, _ice_consume), "ice_tail_time_mismatch": ((2,), _ice_time_mismatch),
    "ice_tail_commit_voids_deferred": ((2,), _ice_commit_voids_deferred), "ice_tail_commit_voids_tail": ((2,), _ice_commit_voids_tail),
    "ice_and_ocean_steps": (ALL_MODES, _ice_and_ocean_steps),
}
for _a in ALL_MODES:
    for _b in ALL_MODES:
        _NAMED["mode_switch_%dto%d" % (_a, _b)] = ((_a,), _mode_switch(_a, _b))
        _NAMED["mode_switch_direct_%dto%d" % (_a, _b)] = ((_a,), _mode_switch_direct(_a, _b))
        _NAMED["mode_switch_supersede_%dto%d" % (_a, _b)] = ((_a,), _mode_switch_supersede(_a, _b))
for _one, _suffix in ((False, ""), (True, "_8_1_12")):
    for _name, _kw in _CONTINUING.items():
        _NAMED[_name + _suffix] = (ALL_MODES, _continuing(one_step=_one, **_kw))
    # the continuing call whose pending state left on the auxiliary stream, found stale by a call under a merged mode
    for _b in (1, 2):
        _NAMED["continuing_split_clock_and_mode_change_0to%d%s" % (_b, _suffix)] = ((0,), _continuing([SetMode(_b)], _one, tf0=2 * TF0))

WALK_SEEDS = tuple(range(24))
WALK_LENGTH = 40


def walk(seed, length=WALK_LENGTH):
    """(starting mode, operations): a seeded random LEGAL sequence — the model refuses what the contract forbids."""
    rng = random.Random(1000 + seed)
    mode = seed % 3
    m, ops = Model(mode), []
    tfs, srcs, ws = (0.25, 0.75), ("W", "W", "W", "V", "M", "N"), ("lat", "lat", "lat", "lat_half", "general")

    def key():
        l1 = rng.randrange(N_SLOTS)
        return rng.choice(srcs), rng.choice(ws), l1, (l1 + 1) % N_SLOTS, rng.choice(tfs)

    while len(ops) < length:
        x = rng.random()
        if x < 0.30:
            s = rng.choice(SETS[:2] * 3 + SETS[2:])
            r = m.pending.get(s)
            k = (r.src, r.w, r.l1, r.l2, r.tf) if r is not None and rng.random() < 0.65 else key()
            op = Step(s, *k, rng.randrange(2), False)
        elif x < 0.58:
            op = Request(rng.choice(SETS[:2] * 3 + SETS[2:]), *key())
        elif x < 0.68:
            w, slot = rng.choice(WINDOWS), rng.randrange(N_SLOTS)
            op = Commit(w, slot, m.slots[w][slot][0] + N_SLOTS)
        elif x < 0.72:
            op = Discard()
        elif x < 0.78:
            op = Sync()
        elif x < 0.86:
            op = SetMode(rng.randrange(3))
        elif x < 0.89:
            op = SetFusedNet(rng.choice((0, 2)))
        elif x < 0.92:
            op = SetStream(rng.choice(("side", "own")))
        elif x < 0.96:
            op = Write(rng.choice(SETS), *key())
        else:
            # (fractions 1/8 + s/4: a sixteenth or more from every other fraction of the atlas, and never 0)
            op = TimeSteps(rng.randrange(3), rng.randrange(1, 4), rng.randrange(3), rng.choice(("W", "M")), "lat", rng.randrange(N_SLOTS), 0.125, 0.25)
        if m.legal(op):
            m.apply(op)
            ops.append(op)
    return mode, ops


def atlas(ice=None):
    """[(case id, starting mode, operations)].  ice = True / False: only the cases with / without sea-ice steps."""
    out = []
    for name, (modes, build) in _NAMED.items():
        for mode in modes:
            ops = build(mode)
            uses_ice = any(isinstance(op, Step) and op.ice for op in ops)
            if ice is None or ice == uses_ice:
                out.append(("%s/mode%d" % (name, mode), mode, ops))
    if not ice:
        for seed in WALK_SEEDS:
            mode, ops = walk(seed)
            out.append(("walk%02d/mode%d" % (seed, mode), mode, ops))
    return out


# ---------------------------------------------------------------------------------------------
# designed data and the reference of one atmosphere
# ---------------------------------------------------------------------------------------------
VARIABLES = ("tas", "huss", "psl", "uas", "vas", "rlds", "rsds", "prra", "prsn")
B_V = dict(tas=2.0, huss=1e-4, psl=600.0, uas=0.5, vas=0.5, rlds=5.0, rsds=5.0, prra=1e-6, prsn=0.0)   # per generation
A_V = {k: 0.09 * v for k, v in B_V.items()}                                                            # per time index
SOURCE_WAVE = dict(W=0, V=3, M=5, N=7)     # what tells the sources apart: B_V[v]·cos(2π k i / ns_x) on top, k waves round the globe (W: none)


@functools.lru_cache(maxsize=4)
def _base(row0=0, row1=None):
    from coflux import synthetic as syn
    return syn.jra55_snapshots(N_BASE, rows=None if row1 is None else (row0, row1))


def source_shape():
    from coflux import synthetic as syn
    return syn.JRA55_NY, syn.JRA55_NX


@functools.lru_cache(maxsize=24)
def snapshot(src, n, g, row0=0, row1=None):
    """dict variable → float32 [ns_y, ns_x]: time index n in generation g of source `src` (rows row0 … row1 − 1 of it)."""
    base = _base(row0, row1)
    k, nsx = SOURCE_WAVE[src], source_shape()[1]
    wave = np.cos(2.0 * np.pi * k * np.arange(nsx) / nsx)[None, :] if k else 0.0
    return {v: (base[v][n].astype(np.float64) + (n * A_V[v] + (g + wave) * B_V[v])).astype(np.float32) for v in VARIABLES}


@functools.lru_cache(maxsize=None)
def weights(name):
    """The three maps in the library's host layout (numpy)."""
    from coflux import synthetic as syn
    fi, fj, phi = syn.latlon_fractional_indices(NX, NY, H, H)
    if name == "lat":
        return dict(separable=True, fi=fi, fj=fj, latitude=phi)
    if name == "lat_half":
        return dict(separable=True, fi=fi, fj=fj + 0.5, latitude=phi)
    import weight_atlas
    return weight_atlas.weight_map("tripolar", source_shape()[::-1], (NX, NY, H, H, RING))


def two_levels(atmos):
    """The source of one Atmos as a two-level in-memory atmosphere (levels 0 and 1)."""
    a, b = snapshot(atmos.src, *atmos.c1), snapshot(atmos.src, *atmos.c2)
    return {v: np.stack([a[v], b[v]]) for v in VARIABLES}


def ring_window(a):
    return a[H - RING:H + NY + RING, H - RING:H + NX + RING]
