"""Host side of the surface monitor — no GPU.  The NumPy reference (monitor_reference.py) against the header's known answers
and its own algebra; the three hand-kept copies of the new ABI (header, abi.py, Julia stub); and the mirror's callbacks
(Simulation.callbacks, SurfaceExtrema, Progress, omip_progress_callback, NaNChecker) driven through a stand-in context whose
monitor IS the NumPy reference."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import monitor_reference as mr
from coflux import abi
from coflux import models as cm
from test_julia_stub import HEADER, STUB, julia_structs, struct_size

NEW_SYMBOLS = ("cf_monitor_create", "cf_monitor_destroy", "cf_monitor_collect", "cf_monitor_count", "cf_monitor_read",
               "cf_monitor_status", "cf_monitor_reset", "cf_attach_monitor")
KNOWN = mr.from_bits(np.array([0, 1 << 63, 0x3FF0000000000000, 0x7FF8000000000000, 0x7FF0000000000000, 0xBFF8000000000000], dtype=np.uint64))


# ---- the reference -----------------------------------------------------------------------------------------------------------
def test_the_reference_reproduces_the_known_answers():
    assert list(KNOWN[:3]) == [0.0, 0.0, 1.0] and np.signbit(KNOWN[1]) and np.isnan(KNOWN[3]) and KNOWN[4] == np.inf and KNOWN[5] == -1.5
    assert mr.state_hash(KNOWN) == 0xbc9733db8e1747df
    assert mr.state_hash(KNOWN, first_cell=1000) == 0x05c59e8be3d701d6
    assert mr.state_hash(np.array([0.0])) == 0xe220a8397b1dcdaf
    assert mr.state_hash(np.zeros(0)) == 0
    # the header states the same four words
    for word in ("0xbc9733db8e1747df", "0x05c59e8be3d701d6", "0xe220a8397b1dcdaf", "0x9E3779B97F4A7C15", "0xBF58476D1CE4E5B9", "0x94D049BB133111EB"):
        assert word in HEADER, word


def test_a_single_cell_change_at_designed_positions_changes_the_hash():
    rng = np.random.default_rng(0)
    x = rng.standard_normal(1025)
    base = mr.state_hash(x)
    for c in (0, 1, 63, 64, 511, 512, 1023, 1024):
        for flip in (1, 1 << 31, 1 << 32, 1 << 52, 1 << 63):          # lowest bit, both halves, the exponent, the sign
            y = mr.bits(x).copy()
            y[c] ^= np.uint64(flip)
            assert mr.state_hash(mr.from_bits(y)) != base, (c, flip)
    y = x.copy()
    y[[3, 700]] = y[[700, 3]]
    assert mr.state_hash(y) != base, "the position enters the hash"
    assert mr.state_hash(np.array([0.0])) != mr.state_hash(np.array([-0.0]))


def test_slab_hashes_taken_with_first_cell_add_up_to_the_whole():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((11, 13))
    x[2, 3], x[9, 0] = np.nan, -np.inf
    wet = rng.random((11, 13)) < 0.8
    whole = mr.monitor_value(x, wet)
    south, north = mr.monitor_value(x[:5], wet[:5]), mr.monitor_value(x[5:], wet[5:], first_cell=5 * 13)
    assert (int(south["hash"]) + int(north["hash"])) % (1 << 64) == int(whole["hash"])
    assert mr.same(mr.combine(south, north), whole)
    assert mr.state_hash(x[5:], 5 * 13) != mr.state_hash(x[5:], 0)


def test_the_order_is_the_ieee_total_order_of_the_non_nan_doubles():
    v = np.array([-np.inf, -1.7976931348623157e308, -1.0, -5e-324, -0.0, 0.0, 5e-324, 2.2250738585072014e-308, 1.0, 1.7976931348623157e308, np.inf])
    k = mr.order_key(mr.bits(v))
    assert (k[1:] > k[:-1]).all(), "strictly increasing, −0.0 < +0.0 included"
    assert np.array_equal(mr.bits(mr.key_value(k)), mr.bits(v))
    both = mr.monitor_value(np.array([1.0, 0.0, -0.0, 0.0, -0.0]))
    assert np.signbit(both["minimum"]) and both["minimum"] == 0 and both["argmin"] == 2 and both["argmax"] == 0
    assert mr.monitor_value(np.array([0.0, -0.0]), kind="abs")["argmin"] == 0 and not np.signbit(mr.monitor_value(np.array([-0.0]), kind="abs")["minimum"])
    none = mr.monitor_value(np.array([np.nan, 1.0]), wet=np.array([1, 0]))
    assert (none["minimum"], none["maximum"], none["argmin"], none["argmax"], none["nan_count"]) == (np.inf, -np.inf, -1, -1, 1)
    assert none["first_nonfinite"] == 0 and none["inf_count"] == 0


# ---- header, abi.py and the Julia stub ---------------------------------------------------------------------------------------
def test_the_three_copies_of_the_abi_list_the_new_names():
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    declared = set(re.findall(r"\b(cf_\w+)\s*\(", code))
    called = set(re.findall(r"\(:(cf_\w+), libcoflux\)", STUB))
    for name in NEW_SYMBOLS:
        assert name in declared and name in abi.EXPORTED_SYMBOLS and name in called, name
    assert re.search(r"#define CF_ABI_VERSION 5\b", HEADER) and abi.ABI_VERSION == 5
    for macro, value in (("CF_MONITOR_MAX_ENTRIES", abi.MONITOR_MAX_ENTRIES), ("CF_MONITOR_VALUE", abi.MONITOR_VALUE), ("CF_MONITOR_ABS", abi.MONITOR_ABS)):
        assert re.search(rf"#define {macro} {value}\b", HEADER), macro
        assert re.search(rf"\b{macro}\b[^\n]*\b{value}\b", STUB), macro
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for doc in ("INTEGRATION.md", "DESIGN.md"):
        text = open(os.path.join(root, doc)).read()
        for name in NEW_SYMBOLS:
            assert name in text, (doc, name)


def test_the_struct_sizes_agree_and_a_value_is_64_bytes():
    structs = julia_structs()
    # (UInt64 has the size and alignment of Int64)
    structs = {k: [(f, "Int64" if t == "UInt64" else t) for f, t in v] for k, v in structs.items()}
    twins = (("CfMonitorEntry", "cf_monitor_entry", abi.MonitorEntry), ("CfMonitorDesc", "cf_monitor_desc", abi.MonitorDesc),
             ("CfMonitorValue", "cf_monitor_value", abi.MonitorValue))
    for name, struct, twin in twins:
        assert name in structs, f"{name} missing from the stub"
        assert struct_size(name, structs)[0] == C.sizeof(twin), (name, struct_size(name, structs)[0], C.sizeof(twin))
        assert [f for f, _t in structs[name]] == [f for f, *_ in twin._fields_], name
        body = re.search(rf"typedef struct {struct} \{{(.*?)\}} {struct};", HEADER, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [f for decl in body.split(";") for f in re.findall(r"(\w+)(?:\[\w+\])?\s*(?:,|$)", decl.strip())]
        assert fields == [f for f, *_ in twin._fields_], (struct, fields)
    assert C.sizeof(abi.MonitorValue) == 64 == abi.MONITOR_VALUE_DTYPE.itemsize and C.sizeof(abi.MonitorEntry) == 16
    assert C.sizeof(abi.MonitorDesc) == 32 + 16 * abi.MONITOR_MAX_ENTRIES
    assert list(abi.MONITOR_VALUE_DTYPE.names) == [f for f, *_ in abi.MonitorValue._fields_]
    assert [abi.MONITOR_VALUE_DTYPE.fields[f][1] for f in abi.MONITOR_VALUE_DTYPE.names] == [getattr(abi.MonitorValue, f).offset for f, *_ in abi.MonitorValue._fields_]


# ---- the mirror, on a stand-in context -------------------------------------------------------------------------------------
class _Monitor:
    """cf_monitor_* restated on the CPU with monitor_reference (the stand-in fields have no halos)"""

    def __init__(self, entries, mask=None, first_cell=0, capacity=1024, max_workgroups=0):
        self.entries = [tuple(e) if isinstance(e, (tuple, list)) else (e, "value") for e in entries]
        self.mask, self.first_cell, self.capacity = mask, first_cell, capacity
        self.values, self.time, self.collections, self.resets, self.bad = [], [], 0, 0, (-1, 0)

    def collect(self, time=0.0):
        assert len(self.values) < self.capacity, "the writer drains a full series before it collects"
        wet = None if self.mask is None else self.mask.numpy()
        rec = [mr.monitor_value(a.numpy(), wet, kind, self.first_cell) for a, kind in self.entries]
        entries = sum(1 << e for e, v in enumerate(rec) if v["nan_count"] + v["inf_count"] > 0)
        if entries and self.bad[0] < 0:
            self.bad = (len(self.values), entries)
        self.values.append(rec)
        self.time.append(time)
        self.collections += 1

    def count(self):
        return len(self.values)

    def read(self, first=0, n=None):
        n = len(self.values) - first if n is None else n
        return np.array(self.values[first:first + n], dtype=mr.DTYPE).reshape(n, len(self.entries)), np.array(self.time[first:first + n])

    def status(self):
        return self.bad

    def reset(self):
        self.values, self.time, self.resets, self.bad = [], [], self.resets + 1, (-1, 0)

    def close(self):
        pass


NX, NY = 6, 4


def _fake_model(sea_ice=True):
    shape = (NY, NX)
    f = lambda v=0.0: torch.full(shape, float(v), dtype=torch.float64)  # noqa: E731
    made = []

    def monitor(*a, **kw):
        made.append(_Monitor(*a, **kw))
        return made[-1]

    calls = []
    ctx = SimpleNamespace(monitor=monitor, made=made, params=SimpleNamespace(mask_kind=abi.MASK_U8), calls=calls,
                          discard_prefetched_atmosphere_state=lambda: calls.append("discard"), sync=lambda: calls.append("sync"))
    net = {k: f() for k in ("u", "v", "T", "S")}
    itf = SimpleNamespace(context=ctx, net_fluxes=SimpleNamespace(_ocean_fields=net), _exchange_current=0)
    wet = torch.ones(shape, dtype=torch.uint8)
    wet[0, 0] = 0
    state = dict(T=f(10.0), S=f(35.0), u=f(0.0), v=f(0.0))
    grid = SimpleNamespace(size=(NX, NY, 1), halo=(0, 0, 0))
    ocean = SimpleNamespace(grid=grid, model=SimpleNamespace(wet_mask=wet), surface_state=lambda: state)
    ice = SimpleNamespace(thickness=f(2.0), concentration=f(0.5)) if sea_ice else None
    return SimpleNamespace(interfaces=itf, ocean=ocean, sea_ice=ice, clock=SimpleNamespace(time=0.0, iteration=0)), state, net


def _stepper(state, net, log=None):
    def fake_step(m, dt):           # T takes the value of the step's iteration, the net heat flux its negative
        m.clock.time += dt
        m.clock.iteration += 1
        state["T"].fill_(float(m.clock.iteration))
        net["T"].fill_(-float(m.clock.iteration))
        if log is not None:
            log.append(("step", m.clock.iteration))
    return fake_step


def test_surface_extrema_drains_a_full_series_and_keeps_the_order_of_records(monkeypatch):
    model, state, net = _fake_model()
    monkeypatch.setattr(cm, "time_step", _stepper(state, net))
    state["u"][2, 3], state["u"][0, 0], state["u"][3, 5] = -7.0, -99.0, 7.0      # (0, 0) is land
    w = cm.SurfaceExtrema(model, dict(T=state["T"], speed=(state["u"], "abs"), u=state["u"]), schedule=cm.IterationInterval(2), capacity=3)
    assert w.monitor.mask is model.ocean.model.wet_mask and [k for _, k in w.monitor.entries] == ["value", "abs", "value"]
    cm.run(cm.Simulation(model, dt=10.0, stop_iteration=16, output_writers=dict(extrema=w)))
    assert list(w.times) == [20.0 * k for k in range(1, 9)] and w.monitor.collections == 8 and w.monitor.resets >= 2
    s = w.series()
    assert list(s) == ["T", "speed", "u"] and set(s["T"]) == set(cm.MONITOR_COLUMNS)
    assert np.array_equal(s["T"]["min"], 2.0 * np.arange(1, 9)) and np.array_equal(s["T"]["max"], s["T"]["min"])
    assert (s["T"]["argmin"] == (0, 1)).all(), "the first wet cell, as (j, i)"
    assert (s["speed"]["max"] == 7.0).all() and (s["speed"]["argmax"] == (2, 3)).all(), "|−7| at the smaller index wins the tie with 7"
    assert (s["u"]["min"] == -7.0).all() and (s["u"]["argmin"] == (2, 3)).all() and (s["u"]["argmax"] == (3, 5)).all()
    assert (s["u"]["first_nonfinite"] == (-1, -1)).all() and not s["u"]["nan_count"].any()
    want = [mr.state_hash(np.full((NY, NX), 2.0 * k)) for k in range(1, 9)]
    assert [int(h) for h in s["T"]["hash"]] == want and s["T"]["hash"].dtype == np.uint64
    assert len(set(want)) == 8
    w.close()


def _designed(state, model):
    T, S, u, v = state["T"].numpy(), state["S"].numpy(), state["u"].numpy(), state["v"].numpy()
    T[:] = np.linspace(-1.8, 29.996, NX * NY).reshape(NY, NX)
    S[:] = np.linspace(5.004, 40.0, NX * NY).reshape(NY, NX)
    u[:] = np.linspace(-1.5, 0.25, NX * NY).reshape(NY, NX)
    v[:] = np.linspace(-0.125, 3.0e-3, NX * NY).reshape(NY, NX)
    model.sea_ice.thickness.numpy()[:] = np.linspace(0.0, 4.321, NX * NY).reshape(NY, NX)
    model.sea_ice.concentration.numpy()[:] = np.linspace(0.0, 0.987, NX * NY).reshape(NY, NX)


def test_progress_produces_the_reference_message_on_a_designed_state(caplog):
    model, state, net = _fake_model()
    _designed(state, model)
    T = state["T"].numpy()
    wet_min_T = T[0, 1]                      # (0, 0) is land: the minimum is the second cell's
    model.clock.time, model.clock.iteration = 3 * 3600.0, 9
    sim = cm.Simulation(model, dt=20 * 60.0)
    p = cm.Progress()
    with caplog.at_level("INFO", logger="coflux"):
        msg = p(sim)
    assert msg == p.message and msg in caplog.text
    head = "time: 3 hours, iteration: 9, Δt: 20 minutes, max(h): 4.32e+00 m, max(ℵ): 9.87e-01 "
    want = head + "extrema(T, S): (%.2f, %.2f) ᵒC, (%.2f, %.2f) psu, " % (29.996, wet_min_T, 40.0, state["S"].numpy()[0, 1])
    want += "maximum(u): (2.50e-01, 3.00e-03) m/s, wall time: "
    assert msg.startswith(want), (msg, want)
    assert re.fullmatch(r"wall time: [0-9.]+ (ns|μs|ms|seconds?|minutes?) \n", msg[len(want) - len("wall time: "):])
    assert len(model.interfaces.context.made) == 1 and [k for _, k in p.monitor.entries] == ["value"] * 6
    # a NaN on a wet cell: Julia's maximum and minimum are NaN; on land it leaves no trace
    T[2, 2] = np.nan
    state["S"].numpy()[0, 0] = np.nan
    msg = p(sim)
    assert "extrema(T, S): (NaN, NaN) ᵒC, (40.00, %.2f) psu, " % state["S"].numpy()[0, 1] in msg
    assert len(model.interfaces.context.made) == 1 and p.monitor.collections == 2, "one monitor, one collection per call"
    # without sea ice the ice part is empty (ClimaOcean.jl:61-67)
    ocean_only, st, _ = _fake_model(sea_ice=False)
    msg = cm.Progress()(cm.Simulation(ocean_only, dt=90.0))
    assert msg.startswith("time: 0 seconds, iteration: 0, Δt: 1.500 minutes, extrema(T, S): (10.00, 10.00) ᵒC, (35.00, 35.00) psu, maximum(u): (0.00e+00, 0.00e+00) m/s, ")
    assert cm.prettytime(86400.0) == "1 day" and cm.prettytime(1.0) == "1 second" and cm.prettytime(2.5 * 86400) == "2.500 days"


def test_omip_progress_emits_state_hash_at_iterations_1_5_100_and_1000_only(monkeypatch, caplog):
    model, state, net = _fake_model()
    _designed(state, model)
    monkeypatch.setattr(cm, "time_step", _stepper(state, net))
    sim = cm.Simulation(model, dt=60.0, stop_iteration=1001)
    cb = cm.omip_progress_callback()
    assert cm.add_callback(sim, cb, cm.IterationInterval(1), name="progress") == "progress" and list(sim.callbacks) == ["progress"]
    with caplog.at_level("INFO", logger="coflux"):
        cm.run(sim)
    lines = [r.getMessage() for r in caplog.records if r.getMessage().startswith("STATE_HASH")]
    assert [int(re.match(r"STATE_HASH iter=(\d+)  ", line).group(1)) for line in lines] == [1, 5, 100, 1000]
    assert sorted(cb.hashes) == [1, 5, 100, 1000] and cb.monitor.collections == 1001
    h = {k: mr.state_hash(t.numpy()) for k, t in (("S", state["S"]), ("u", state["u"]), ("h", model.sea_ice.thickness))}
    for it, line in zip((1, 5, 100, 1000), lines):
        want = "STATE_HASH iter=%d  T=%016x  S=%016x  u=%016x  h=%016x" % (it, mr.state_hash(np.full((NY, NX), float(it))), h["S"], h["u"], h["h"])
        assert line == want == cb.hashes[it]
    # the message of the last iteration: (Tmin, Tmax), (Smin, Smax), no comma after psu
    S = state["S"].numpy()
    assert cb.message.startswith("time: 16.683 hours, iteration: 1001, Δt: 1 minute, max(h): 4.32e+00 m, max(ℵ): 9.87e-01 "
                                 "extrema(T, S): (1001.00, 1001.00) ᵒC, (%.2f, 40.00) psu maximum(u): (2.50e-01, 3.00e-03) m/s, wall time: " % S[0, 1])


def test_nan_checker_stops_run_at_the_right_iteration_name_and_cell(monkeypatch):
    model, state, net = _fake_model()
    step = _stepper(state, net)

    def stepping(m, dt):
        step(m, dt)
        if m.clock.iteration == 7:
            net["S"][2, 4] = float("inf")
            net["S"][3, 1] = float("nan")
            net["v"][0, 0] = float("nan")       # land: no trace
        if m.clock.iteration == 8:
            state["T"][1, 1] = float("nan")     # a later, other field: `first` stays

    monkeypatch.setattr(cm, "time_step", stepping)
    chk = cm.NaNChecker(schedule=cm.IterationInterval(3))
    sim = cm.Simulation(model, dt=1.0, stop_iteration=30)
    cm.add_callback(sim, chk, chk.schedule)
    cm.run(sim)
    assert model.clock.iteration == 9 and sim.running is False, "iterations 3 and 6 are clean, 9 is the first check that sees it"
    assert chk.names == ["net_u", "net_v", "net_T", "net_S", "T"]
    assert chk.first == (9, "net_S", (2, 4)), chk.first
    assert cm.NaNChecker().schedule.interval == 100
    # chosen fields; a clean run goes to its end and run! may be called again
    model, state, net = _fake_model()
    monkeypatch.setattr(cm, "time_step", _stepper(state, net))
    chk = cm.NaNChecker(dict(T=state["T"]), schedule=1)
    sim = cm.Simulation(model, dt=1.0, stop_iteration=4)
    cm.add_callback(sim, chk, chk.schedule)
    cm.run(sim)
    assert model.clock.iteration == 4 and sim.running and chk.first is None and chk.monitor.collections == 4
    state["T"][3, 5] = float("-inf")
    monkeypatch.setattr(cm, "time_step", lambda m, dt: (setattr(m.clock, "iteration", m.clock.iteration + 1), setattr(m.clock, "time", m.clock.time + dt)))
    sim.stop_iteration = 10
    cm.run(sim)
    assert model.clock.iteration == 5 and chk.first == (5, "T", (3, 5)), "±Inf stops it too"


def test_run_with_no_callbacks_makes_the_same_calls_as_before(monkeypatch):
    class Writer:
        def __init__(self, log):
            self.log = log

        def initialize(self, simulation):
            self.log.append("initialize")

        def write(self, clock):
            self.log.append(("write", clock.iteration))

    def trace(with_callback):
        model, state, net = _fake_model()
        log = model.interfaces.context.calls
        monkeypatch.setattr(cm, "time_step", _stepper(state, net, log))
        sim = cm.Simulation(model, dt=5.0, stop_iteration=3, output_writers=dict(w=Writer(log)))
        assert sim.callbacks == {} and sim.running is True
        if with_callback:
            cm.add_callback(sim, lambda s: log.append(("callback", s.model.clock.iteration)), cm.IterationInterval(2))
            assert list(sim.callbacks) == ["callback1"]
        cm.run(sim)
        assert model.interfaces.context.made == [], "no monitor is made unless a callback asks for one"
        return log

    before = ["initialize", ("step", 1), ("write", 1), ("step", 2), ("write", 2), ("step", 3), ("write", 3), "discard", "sync"]
    assert trace(False) == before
    assert trace(True) == before[:5] + [("callback", 2)] + before[5:], "a callback runs after the writers of its iteration"
