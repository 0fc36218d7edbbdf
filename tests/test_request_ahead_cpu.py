"""The books of the atmosphere states requested ahead (csrc/coflux_request_ahead.hpp) held on the CPU against the host model of
the contract, tests/prefetch_model.py.  Every case of the model's atlas — the named cases in all their modes, the sea-ice
cases, the 24 walks — is translated into the ledger's primitive calls the way the library's host code makes them (Replay below:
a cf_time_steps operation becomes the first-step decision, then per step the request for the next step and the step), with
sources, maps and sets as small integers standing in for pointers.  Which launch carries a waiting request that leaves with a
step is the launch code's decision, not the ledger's: the test supplies it from the model (Model._route); a flush to the
auxiliary stream is the ledger's own and is not supplied.  tests/request_ahead_driver.cpp includes the header and nothing else
of the library; it is compiled alone with -fsanitize=address,undefined, the runtimes linked statically (nothing is preloaded),
and run once as a subprocess that answers every command of every case."""
import os
import re
import shutil
import struct
import subprocess
from collections import namedtuple

import pytest

import prefetch_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "climaocean.jl_amd", "csrc")
SRC = {name: n + 1 for n, name in enumerate(pm.SOURCES)}
MAP = {name: n + 1 for n, name in enumerate(pm.WEIGHTS)}
SET = {name: n + 1 for n, name in enumerate(pm.SETS)}
NO_SET = 0      # (the first step of a call under a merged mode leaves in a launch of its own before any step: no set to spare)
AUX = "launched_aux"

# a primitive call: the driver's command, what the model did meanwhile — [("leave", request, route) | ("end", request, outcome)]
# — and what the call must answer: request → the model's request, or None where it is refused (gate: recorded at request
# time); first → needed; step → interpolates; leave_main → the request that left
Prim = namedtuple("Prim", "cmd log answer gate", defaults=(None, None))


def hx(v):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", v))[0]


SET_OF = {}     # id(a request of the model that left) → its exchange set (the logs keep the requests alive)


class Traced(pm.Model):
    """The model with a log of what happened to every request and, per step, whether it interpolated itself"""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.log, self.interpolated = [], []

    def _leaves(self, route):
        r = self.pending[self.waiting]
        SET_OF[id(r)] = self.waiting
        super()._leaves(route)
        self.log.append(("leave", r, route))

    def _end(self, s, outcome):
        r = self.pending[s]
        super()._end(s, outcome)
        self.log.append(("end", r, outcome))

    def _step(self, *args, **kwargs):
        before = self.c["step_interpolations"]
        sees = super()._step(*args, **kwargs)
        self.interpolated.append(self.c["step_interpolations"] - before)
        return sees


class Replay:
    """Applies operations to the (sound) model through the model's own rules, one primitive call of the ledger at a time"""

    def __init__(self, mode):
        self.m = Traced(mode)

    def _cut(self):
        log, self.m.log = self.m.log, []
        return log

    def request(self, s, src, w, l1, l2, tf, defer=True):
        m = self.m
        ok = m._request(s, src, w, l1, l2, tf)
        return Prim("request %d %d %d %d %d %s %d %d" % (SRC[src], MAP[w], SET[s], l1, l2, hx(tf), m.mode, defer), self._cut(),
                    m.pending[s] if ok else None, not (defer and m.mode != 0))

    def step(self, s, src, w, l1, l2, tf, ice):
        m = self.m
        carried = m.pending[m.waiting] if m.waiting not in (None, s) else None
        route = m._route(ice)
        sees = m._step(s, src, w, l1, l2, tf, ice)
        log = self._cut()
        prims = [Prim("step %d %d %d %d %d %s" % (SET[s], SRC[src], MAP[w], l1, l2, hx(tf)), log[:-1] if carried else log, m.interpolated[-1])]
        if carried:
            assert log[-1] == ("leave", carried, route)
            prims.append(Prim("leave_aux", log[-1:]) if route == AUX else Prim("leave_main %d %d" % (SET[s], pm.ROUTES.index(route)), log[-1:], carried))
        return prims, sees

    def time_steps(self, op):
        """cf_time_steps in the order include/coflux.h gives: the first step's state unless it is pending, then per step the request
        for the next step and the step"""
        m, prims, sees = self.m, [], []
        sets, end = ("A", "B") if op.pipeline else ("A",), op.first + op.n
        if op.pipeline and op.n > 0:
            s0, k0 = sets[op.first % 2], pm.clock(op, op.first)
            r = m.pending.get(s0)
            needed = not (r is not None and m._matches(r, op.src, op.w, *k0))
            if not needed and m.waiting == s0:
                m._flush()
            prims.append(Prim("first %d %d %d %d %d %s" % (SET[s0], SRC[op.src], MAP[op.w], k0[0], k0[1], hx(k0[2])), self._cut(), int(needed)))
            if needed:      # a merged mode keeps it on the context's stream, without a gate; else it leaves on the auxiliary stream at once
                prims.append(self.request(s0, op.src, op.w, *k0, defer=m.mode != 0))
                assert prims[-1].answer is not None
                m._leaves("launched_own" if m.mode != 0 else AUX)
                prims.append(Prim("leave_main %d %d" % (NO_SET, pm.ROUTES.index("launched_own")), self._cut(), m.pending[s0]) if m.mode != 0
                             else Prim("leave_aux", self._cut()))
        for step in range(op.first, end):
            if op.pipeline and (step + 1 < end or op.pipeline == 2):
                prims.append(self.request(sets[(step + 1) % 2], op.src, op.w, *pm.clock(op, step + 1)))
                assert prims[-1].answer is not None
            more, saw = self.step(sets[step % len(sets)], op.src, op.w, *pm.clock(op, step), False)
            prims += more
            sees.append(saw)
        return prims, sees

    def apply(self, op):
        """(the primitive calls of one operation, what Model.apply returns for it)"""
        m, prims, sees, refused = self.m, [], [], False
        assert m.legal(op)
        if isinstance(op, pm.Request):
            prims = [self.request(*op)]
            refused = prims[0].answer is None
        elif isinstance(op, pm.Step):
            prims, saw = self.step(op.set, op.src, op.w, op.l1, op.l2, op.tf, op.ice)
            sees = [saw]
        elif isinstance(op, pm.TimeSteps):
            prims, sees = self.time_steps(op)
        elif isinstance(op, pm.Sync):
            m._flush()
            prims = [Prim("leave_aux", self._cut())]
        elif isinstance(op, (pm.Commit, pm.Discard)):
            m.apply(op)
            prims = [Prim("commit %d" % op.slot if isinstance(op, pm.Commit) else "discard", self._cut())]
        else:       # options, a stream, a host write: nothing of the ledger's
            m.apply(op)
        counters = dict(m.c, pending=len(m.pending))
        on_main = any(r.route not in (None, AUX) for r in m.pending.values())
        return prims, dict(sees=sees, refused=refused, counters=counters, on_main=on_main)


def _first_step_still_waiting():
    """Not in the atlas: the state of a call's first step was requested by the host and has not left when the call begins — the
    first-step decision finds it and sends it off on the auxiliary stream"""
    call = pm.TimeSteps(0, 3, 1, "W", "lat")
    return [pm.Request("A", call.src, call.w, *pm.clock(call, 0)), call]


@pytest.fixture(scope="module")
def atlas():
    return pm.atlas() + [("first_step_still_waiting/mode%d" % mode, mode, _first_step_still_waiting()) for mode in pm.ALL_MODES]


@pytest.fixture(scope="module")
def replays(atlas):
    """[(case, mode, [(operation, primitive calls, the model's answer)])]"""
    out = []
    for name, mode, ops in atlas:
        R = Replay(mode)
        out.append((name, mode, [(op, *R.apply(op)) for op in ops]))
    return out


def test_the_translation_is_the_model(atlas, replays):
    """Model against model, before any ledger: every operation of the atlas, replayed primitive by primitive, leaves the model
    where Model.apply leaves it — the atmosphere every step sees included."""
    assert len(atlas) == len(replays) > 150 and sum(name.startswith("walk") for name, *_x in atlas) == 24
    assert any(op.ice for *_x, ops in atlas for op in ops if isinstance(op, pm.Step))
    for (name, mode, ops), (_n, _m, replay) in zip(atlas, replays):
        assert [want for want in pm.predict(mode, ops)] == [got for _op, _prims, got in replay], name
    cmds = {p.cmd.split()[0] for *_x, replay in replays for _op, prims, _got in replay for p in prims}
    assert cmds == {"request", "first", "step", "leave_aux", "leave_main", "commit", "discard"}


@pytest.fixture(scope="module")
def answers(tmp_path_factory, replays):
    """[[parsed answer line per primitive call] per case], from one run of the sanitizer build"""
    compiler = shutil.which("g++") or shutil.which("clang++")
    if compiler is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("request_ahead") / "request_ahead_driver")
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(compiler) == "g++" else ["-static-libsan"]
    build = subprocess.run([compiler, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static, "-I", CSRC,
                            os.path.join(ROOT, "tests", "request_ahead_driver.cpp"), "-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and re.search(r"cannot find.*(asan|ubsan|clang_rt)|libasan|libubsan|asan_preinit|static-lib", build.stderr):
        pytest.skip("the sanitizer runtime does not link here: " + build.stderr.strip().splitlines()[-1])
    assert build.returncode == 0, build.stderr
    commands = []
    for _name, _mode, replay in replays:
        commands += ["case"] + [p.cmd for _op, prims, _got in replay for p in prims]
    run = subprocess.run([exe], input="\n".join(commands) + "\n", capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    lines = run.stdout.splitlines()
    assert len(lines) == len(commands)
    out = []
    for cmd, line in zip(commands, lines):
        if cmd == "case":
            out.append([])
            continue
        work, answer, state = (part.split() for part in line.split("|"))
        assert len(state) == len(pm.COUNTERS) + 2
        counters = dict(zip(("pending",) + pm.COUNTERS[:-1], map(int, state[:-2])))
        out[-1].append(dict(work=work, answer=answer[0] if answer else None, counters=counters, on_main=state[-2] == "1", records=state[-1]))
    return out


FRESH = dict(counters=dict.fromkeys(pm.COUNTERS, 0), on_main=False, records="FF")


def by_operation(replay, lines):
    """[(operation, the model's answer, dict(counters, on_main, refused, interpolated) of the driver after it)]"""
    out, last, lines = [], FRESH, iter(lines)
    for op, prims, want in replay:
        mine = [next(lines) for _p in prims]
        last = mine[-1] if mine else last
        out.append((op, want, dict(counters=last["counters"], on_main=last["on_main"], refused=any(a["answer"] == "refused" for a in mine),
                                   interpolated=[int(a["answer"]) for p, a in zip(prims, mine) if p.cmd.startswith("step ")])))
    return out


def agrees(want, interpolated, got):
    """the compared items of one operation: every counter, refused, on_main, and of every step whether it interpolated itself"""
    return (got["counters"] == want["counters"] and got["refused"] == want["refused"] and got["on_main"] == want["on_main"] and
            got["interpolated"] == interpolated)


def test_the_ledger_answers_as_the_model_after_every_operation(replays, answers):
    steps = 0
    for (name, mode, replay), lines in zip(replays, answers):
        traced = Traced(mode)
        for n, (op, want, got) in enumerate(by_operation(replay, lines)):
            del traced.interpolated[:]
            assert traced.apply(op) == want
            assert got["counters"] == want["counters"], (name, n, op)
            assert agrees(want, traced.interpolated, got), (name, n, op, got, traced.interpolated)
            c = got["counters"]
            assert c["requests"] == sum(c[k] for k in pm.OUTCOMES) + c["pending"]
            steps += len(traced.interpolated)
    assert steps > 1000


def test_waits_and_gates_are_where_the_models_routes_put_them(replays, answers):
    """Per primitive call, from the route the MODEL gives every request:
      1. a request that left on the auxiliary stream and ends — consumed, mismatched, voided, superseded or discarded — yields
         exactly one wait of the context's stream on its own record's event, in the call that ends it and behind its launch
         where that call also launched it; one that left on the context's stream or never left yields none;
      2. every leave on the auxiliary stream has exactly one gate record between its request and its launch: at the request, or
         late, with the launch; a deferred request under CF_OPT_MERGED_PREFETCH 1 or 2 records none when it is made.
    Every launch on the auxiliary stream — supplied by the test or the ledger's own flush — is one the model has, of that record."""
    seen = dict.fromkeys(("aux_end", "main_end", "unlaunched_end", "late_gate", "early_gate", "flush", "flush_by_first") + pm.OUTCOMES, 0)
    for (name, _mode, replay), lines in zip(replays, answers):
        lines, records = iter(lines), "FF"
        record_of, gates = {}, {}
        for n, (op, prims, _want) in enumerate(replay):
            for p in prims:
                a, where = next(lines), (name, n, op, p.cmd)
                launches = [(w.split(":")[0][-1], w[0] == "g") for w in a["work"] if "L" in w]
                launched = [w.split(":", 1)[1] for w in a["work"] if "L" in w]
                waits = [w[1] for w in a["work"] if w[0] == "W"]
                assert len(launches) + len(waits) + a["work"].count("G") == len(a["work"]), where
                # the request's own answer
                verb = p.cmd.split()[0]
                if verb == "request":
                    assert (a["answer"] == "refused") == (p.answer is None), where
                    assert ("G" in a["work"]) == (p.answer is not None and p.gate), where
                    if p.answer is not None:
                        k = a["answer"]
                        assert a["records"][int(k)] == "W", where
                        record_of[id(p.answer)], gates[id(p.answer)] = k, int(p.gate)
                elif verb == "leave_main":
                    assert a["answer"] == record_of[id(p.answer)] and a["records"][int(a["answer"])] == "M", where
                elif verb in ("first", "step"):
                    assert int(a["answer"]) == p.answer, where
                # the model's events of this call
                left = [r for what, r, route in p.log if what == "leave" and route == AUX]
                ended = [(r, how) for what, r, how in p.log if what == "end"]
                assert launches == [(record_of[id(r)], gates[id(r)] == 0) for r in left], where      # (2): one gate, early or late
                # … and what it launches is the request the model says left, not whatever its record holds by the time it is queued
                assert launched == ["%d:%d:%d:%d:%d:%s" % (SRC[r.src], MAP[r.w], SET[SET_OF[id(r)]], r.l1, r.l2, hx(r.tf)) for r in left], where
                for r in left:
                    seen["late_gate" if gates[id(r)] == 0 else "early_gate"] += 1
                    seen["flush"] += verb != "leave_aux"
                    seen["flush_by_first"] += verb == "first"
                    gates[id(r)] = 1
                    assert a["records"][int(record_of[id(r)])] in "AF" or (verb == "request" and a["answer"] == record_of[id(r)]), where
                assert sorted(waits) == sorted(record_of[id(r)] for r, _how in ended if r.route == AUX), where      # (1)
                for r, how in ended:
                    k = record_of.pop(id(r))
                    before = "W" if r.route is None or r in left else "A" if r.route == AUX else "M"
                    assert records[int(k)] == before, where
                    assert a["records"][int(k)] == "F" or (verb == "request" and a["answer"] == k), where
                    if r in left:       # launched and ended by one call (a step into its own set): the wait comes behind the launch
                        assert a["work"].index("W" + k) > [w.split(":")[0][-1] for w in a["work"]].index(k), where
                    seen["unlaunched_end" if r.route is None else "aux_end" if r.route == AUX else "main_end"] += 1
                    seen[how] += r.route == AUX
                records = a["records"]
    # every kind of end behind a launch on the auxiliary stream, both kinds of gate and the ledger's own flushes were met
    assert all(seen[k] > 0 for k in seen), seen


# the case of the atlas (in its order) that first tells the ledger from each wrong model
FIRST_SHOWN = {
    "ignore_commits": "commit_voids_aux/mode0",                         # voided, and the step behind it consumes
    "ignore_fraction": "time_mismatch/mode0",                           # consumed for mismatched
    "ignore_source": "source_mismatch/mode0",
    "ignore_weights": "weights_mismatch/mode0",
    "discard_forgets_deferred_only": "continuing_stop_discard/mode0",   # discarded and pending
    "supersede_keeps_old": "both_sets_pending/mode0",                   # the step at the new clock: mismatched for consumed
    "continuing_trusts_pending": "continuing_split_clock_change/mode0",
}


@pytest.mark.parametrize("defect", pm.DEFECTS)
def test_the_ledger_stands_apart_from_each_wrong_model(atlas, replays, answers, defect):
    """The seven seeded defects of the model (tests/test_prefetch_model_cpu.py holds them against the atmospheres the steps see):
    the model with each must disagree with the ledger in a compared item — a counter, refused, on_main, or whether a step
    interpolated itself — of some operation of some case.  None of the seven is invisible to the host bookkeeping: each shifts
    a request between two outcomes."""
    shown = []
    for (name, mode, ops), (_n, _m, replay), lines in zip(atlas, replays, answers):
        wrong = Traced(mode, defects=(defect,))
        for op, _want, got in by_operation(replay, lines):
            del wrong.interpolated[:]
            if not agrees(wrong.apply(op), wrong.interpolated, got):
                shown.append(name)
                break
    assert shown and shown[0] == FIRST_SHOWN[defect], (defect, shown[:3])
    assert any(not name.startswith("walk") for name in shown), defect
