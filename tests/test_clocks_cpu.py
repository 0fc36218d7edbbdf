"""The host clocks and schedules of the model layer (coflux/clocks.py, coflux/schedules.py): pure arithmetic, no GPU, no library.

The record clock is held, bit for bit, to the three formulas it replaced — JRA55PrescribedAtmosphere.time_indices, the counters
of the atmosphere's sliding window and JRA55PrescribedLand.levels, restated below as they stood — because time_steps needs all
of them to give the same doubles.  The stretch finder is held to what it promises: the device loop's clock
fraction + step · increment reproduces the host's clock on every step of a stretch, and no stretch could be longer."""
import math
from types import SimpleNamespace

import numpy as np
import pytest

from coflux import clocks, schedules

HOURS = 3600.0
INTERVAL = 3 * HOURS


# ---- (a) the record clock against the formulas it replaced ---------------------------------------------------------------
def atmosphere_time_indices(t, n_levels, time_interval, cyclic):
    x = t / time_interval
    n = int(np.floor(x))
    frac = x - n
    if cyclic:
        return n % n_levels, (n + 1) % n_levels, frac
    n1 = min(max(n, 0), n_levels - 1)
    n2 = min(max(n + 1, 0), n_levels - 1)
    return n1, n2, (frac if 0 <= n < n_levels - 1 else 0.0)


def atmosphere_window_counters(t, n_levels, time_interval, cyclic):
    base = int(np.floor(t / time_interval))
    if cyclic:
        return base, base, base + 1
    return base, min(max(base, 0), n_levels - 1), min(max(base + 1, 0), n_levels - 1)


def land_levels(t, n_levels, time_interval, cyclic):
    wrap = lambda n: n % n_levels if cyclic else min(max(n, 0), n_levels - 1)  # noqa: E731
    x = t / time_interval
    base = int(np.floor(x))
    frac = x - base
    if cyclic:
        k1, k2 = base, base + 1
    else:
        k1 = min(max(base, 0), n_levels - 1)
        k2 = min(max(base + 1, 0), n_levels - 1)
        if not (0 <= base < n_levels - 1):
            frac = 0.0
    return (k1, k2), (wrap(k1), wrap(k2), frac)


def bits(values):
    return tuple(float(v).hex() if isinstance(v, float) else v for v in values)


def sweep_times(n_levels):
    """−2 … n_levels + 2 intervals in steps of 20 min and of 3 h / 8, reached by multiplication and by repeated addition"""
    for dt in (1200.0, INTERVAL / 8):
        count = int(round((n_levels + 4) * INTERVAL / dt))
        start = -2 * INTERVAL
        t = start
        for k in range(count + 1):
            yield start + k * dt
            yield t
            t += dt


@pytest.mark.parametrize("cyclic", (True, False))
@pytest.mark.parametrize("n_levels", (2, 7))
def test_the_record_clock_gives_the_tuples_of_the_three_formulas_it_replaced(n_levels, cyclic):
    clock = clocks.RecordClock(n_levels, INTERVAL, cyclic)
    times = list(sweep_times(n_levels))
    exact = [k * INTERVAL for k in range(-2, n_levels + 3)]
    assert set(exact) <= set(times), "the sweep by multiplication holds every exact multiple of the interval"
    last = [t for t in times if (n_levels - 2) * INTERVAL <= t < (n_levels - 1) * INTERVAL]
    assert len(last) > 16, "… and the last interval of the record"
    for t in times + [np.nextafter(e, s) for e in exact for s in (-np.inf, np.inf)]:
        t = float(t)
        r = clock.at(t)
        assert bits((r.n1, r.n2, r.fraction)) == bits(atmosphere_time_indices(t, n_levels, INTERVAL, cyclic)), t
        assert (r.base, r.k1, r.k2) == atmosphere_window_counters(t, n_levels, INTERVAL, cyclic), t
        counters, levels = land_levels(t, n_levels, INTERVAL, cyclic)
        assert (r.k1, r.k2) == counters and bits((r.n1, r.n2, r.fraction)) == bits(levels), t
        assert (clock.wrap(r.k1), clock.wrap(r.k2)) == (r.n1, r.n2)
    if not cyclic:   # the ends of a clamped record: both snapshots the same, fraction 0
        for t, n in ((-0.5 * INTERVAL, 0), ((n_levels - 1) * INTERVAL, n_levels - 1), ((n_levels + 1.25) * INTERVAL, n_levels - 1)):
            r = clock.at(t)
            assert (r.k1, r.k2, r.n1, r.n2, r.fraction) == (n, n, n, n, 0.0)
        r = clock.at((n_levels - 1.5) * INTERVAL)
        assert (r.n1, r.n2, r.fraction) == (n_levels - 2, n_levels - 1, 0.5)


# ---- (b) the stretch finder ----------------------------------------------------------------------------------------------
def host_clock(record, first, dt, nsteps):
    """(wanted, n_levels, increment) of `record` and the model times, as time_steps forms them: the model's clock is a repeated
    sum, `first` steps old when the call begins"""
    t = 0.0
    for _ in range(first):
        t += dt
    wanted, times = [], []
    for _ in range(nsteps):
        t += dt
        r = record.at(t)
        wanted.append((r.n1, r.n2, r.fraction))
        times.append(t)
    return (wanted, record.n_levels, dt / record.time_interval), times


def check_stretches(stretches, clock_list, first, nsteps, times=None, dt=None):
    """the three promises: a partition of [0, nsteps) in order; the based clocks give the wanted tuples on every step inside;
    every stretch is maximal"""
    assert stretches and stretches[0][0] == 0 and stretches[-1][1] == nsteps
    assert all(a < b for a, b, _, _ in stretches) and all(p[1] == q[0] for p, q in zip(stretches, stretches[1:]))
    for a, b, based, origin in stretches:
        assert len(based) == len(clock_list)

        def holds(k):
            clocks_hold = all(bits(clocks.clock_at(c[0], c[1], n, first + k, inc)) == bits(want[k])
                              for (want, n, inc), c in zip(clock_list, based))
            return clocks_hold and (times is None or origin + float(first + k) * dt == times[k])
        assert all(holds(k) for k in range(a, b)), (a, b)
        assert b == nsteps or not holds(b), (a, b)
        assert (origin is None) == (times is None)


def test_a_step_that_is_a_binary_fraction_of_the_interval_is_one_stretch():
    for first in (0, 5, 26279):
        clock, _ = host_clock(clocks.RecordClock(7, INTERVAL, True), first, INTERVAL / 8, 40)
        stretches = list(clocks.device_stretches([clock], first, 40))
        check_stretches(stretches, [clock], first, 40)
        assert [(a, b) for a, b, _, _ in stretches] == [(0, 40)]


@pytest.mark.parametrize("first", (5, 1000, 26279))
def test_twenty_minute_steps_are_cut_where_the_device_clock_would_part_from_the_host(first):
    dt, nsteps = 1200.0, 40
    clock, times = host_clock(clocks.RecordClock(7, INTERVAL, True), first, dt, nsteps)
    stretches = list(clocks.device_stretches([clock], first, nsteps))
    check_stretches(stretches, [clock], first, nsteps)
    # with a dataset clock, origin + step · Δt is held to the model times as well
    with_dataset = list(clocks.device_stretches([clock], first, nsteps, times, dt))
    check_stretches(with_dataset, [clock], first, nsteps, times, dt)


def test_a_clamped_record_stepped_past_its_end_raises_with_the_text_of_time_steps():
    record = clocks.RecordClock(3, INTERVAL, False)
    clock, _ = host_clock(record, 0, 1200.0, 30)    # 10 h over a record that ends at 6 h
    handed_out = []
    with pytest.raises(ValueError, match=r"time_steps: the device loop's clock cannot take the snapshots \(2, 2\) at fraction 0\.0 of step 17 "
                                         r"\(a clamped record at its end\?\); use time_step"):
        for stretch in clocks.device_stretches([clock], 0, 30):
            handed_out.append(stretch)
    # a generator: the stretches before the end of the record have been handed out, and they are good
    assert handed_out and handed_out[-1][1] == 17
    check_stretches(handed_out, [clock], 0, 17)
    times = [1200.0 * (k + 1) for k in range(4)]
    with pytest.raises(ValueError, match="the dataset clock origin"):
        list(clocks.device_stretches([([(0, 1, 0.25)] * 4, 7, 0.0)], 0, 4, [math.nan] + times[1:], 1200.0))


@pytest.mark.parametrize("dt", (1200.0, 1000.0, 700.0))
@pytest.mark.parametrize("first", (0, 5, 1000))
def test_two_clocks_are_cut_where_either_of_them_would_be(first, dt):
    """Atmosphere 3-hourly, land hourly.  Every cut is the earlier of the cuts that each clock alone would make from the same
    start: from the same bases, the boundaries are the union of the two clocks' boundaries."""
    nsteps = 40
    atmosphere, _ = host_clock(clocks.RecordClock(7, INTERVAL, True), first, dt, nsteps)
    land, _ = host_clock(clocks.RecordClock(24, HOURS, True), first, dt, nsteps)
    both = list(clocks.device_stretches([atmosphere, land], first, nsteps))
    check_stretches(both, [atmosphere, land], first, nsteps)
    for a, b, based, _ in both:
        alone = []
        for (want, n, inc), c in zip((atmosphere, land), based):
            a1, b1, based1, _ = next(clocks.device_stretches([(want[a:], n, inc)], first + a, nsteps - a))
            assert a1 == 0 and based1 == [c]
            alone.append(a + b1)
        assert b == min(alone), (a, b, alone)


@pytest.mark.parametrize("first", (0, 5, 1000, 26279))
def test_at_twenty_minutes_the_cuts_of_two_clocks_are_the_union_of_their_own(first):
    """The same over the whole call, at the model's own Δt = 20 min: the cuts with both clocks are those of the atmosphere alone
    and those of the land alone together.  (This holds at 20 min; it is no law — a clock re-based at the other's cut can
    part from the host at other steps afterwards than it would have alone, as it does at Δt = 1000 s, which is why the test
    above compares from the same start.)"""
    dt, nsteps = 1200.0, 40
    atmosphere, _ = host_clock(clocks.RecordClock(7, INTERVAL, True), first, dt, nsteps)
    land, _ = host_clock(clocks.RecordClock(24, HOURS, True), first, dt, nsteps)
    cuts = lambda clock_list: {b for _, b, _, _ in clocks.device_stretches(clock_list, first, nsteps)}  # noqa: E731
    assert cuts([atmosphere, land]) == cuts([atmosphere]) | cuts([land])


def test_the_dataset_origin_reproduces_a_repeated_sum_or_says_that_it_cannot():
    t = 0.0
    for step in range(1, 200):
        t += 1200.0
        origin = clocks.dataset_origin(t, step, 1200.0)
        assert origin is not None and origin + float(step) * 1200.0 == t
    assert clocks.dataset_origin(math.nan, 3, 1200.0) is None


# ---- (c) schedules -------------------------------------------------------------------------------------------------------
def test_actuates_gives_a_time_interval_the_time_and_every_other_schedule_the_iteration():
    asked = []
    recording = lambda cls: type("Recording", (cls,), dict(actuate=lambda self, x: asked.append(x) or True))  # noqa: E731
    clock = SimpleNamespace(time=3600.0, iteration=3)
    assert schedules.actuates(recording(schedules.TimeInterval)(7.0), clock) and asked == [3600.0]
    assert schedules.actuates(recording(schedules.IterationInterval)(7), clock) and asked == [3600.0, 3]
    assert schedules.actuates(SimpleNamespace(actuate=lambda x: asked.append(x) or False), clock) is False and asked[-1] == 3
    s = schedules.TimeInterval(3600.0)
    s.initialize(0.0, 1200.0)
    assert [schedules.actuates(s, SimpleNamespace(time=1200.0 * k, iteration=k)) for k in range(1, 7)] == [False, False, True] * 2
    assert [schedules.actuates(schedules.IterationInterval(2), SimpleNamespace(time=7.0, iteration=k)) for k in range(1, 5)] == [False, True] * 2


def test_as_schedule_is_the_idiom_it_replaced():
    idiom = lambda s, default: schedules.IterationInterval(s) if isinstance(s, int) else (s or default)  # noqa: E731
    three = schedules.as_schedule(3)
    assert type(three) is schedules.IterationInterval and three.interval == idiom(3, None).interval == 3
    every = schedules.as_schedule(None)
    assert type(every) is schedules.IterationInterval and every.interval == 1
    default = schedules.TimeInterval(30 * 86400.0)
    assert schedules.as_schedule(None, default) is default is idiom(None, default)
    assert schedules.as_schedule(5, default).interval == 5
    for existing in (schedules.IterationInterval(4), schedules.TimeInterval(60.0), schedules.AveragedTimeInterval(60.0)):
        assert schedules.as_schedule(existing) is existing and schedules.as_schedule(existing, default) is existing
    with pytest.raises(ValueError):
        schedules.as_schedule(0)


def test_a_time_interval_callback_fires_at_its_times(monkeypatch):
    """add_callback(simulation, f, TimeInterval(3 Δt)) under run!: iterations 3, 6 and 9 — the schedule is asked with the time (it
    used to be asked with the iteration count and misfired).  Δt = 0.1: the clock is a repeated sum that arrives a rounding
    error early or late, which the schedule's tolerance of 1e-6 Δt (set when run! opens it) absorbs."""
    from coflux import models as cm
    ctx = SimpleNamespace(discard_prefetched_atmosphere_state=lambda: None, sync=lambda: None)
    itf = SimpleNamespace(context=ctx, exchange=cm.ExchangeStates(ctx, {}))
    for dt in (1200.0, 0.1):
        model = SimpleNamespace(interfaces=itf, clock=SimpleNamespace(time=0.0, iteration=0))

        def fake_step(m, dt):
            m.clock.time += dt
            m.clock.iteration += 1

        monkeypatch.setattr(cm, "time_step", fake_step)
        sim = cm.Simulation(model, dt=dt, stop_iteration=10)
        fired, counted = [], []
        cm.add_callback(sim, lambda s: fired.append(s.model.clock.iteration), cm.TimeInterval(3 * dt))
        cm.add_callback(sim, lambda s: counted.append(s.model.clock.iteration), 4)
        cm.run(sim)
        assert fired == [3, 6, 9] and counted == [4, 8]
        # a second run! goes on from the clock: the next multiple of the interval, not the one just passed
        sim.stop_iteration = 13
        cm.run(sim)
        assert fired == [3, 6, 9, 12] and counted == [4, 8, 12]
