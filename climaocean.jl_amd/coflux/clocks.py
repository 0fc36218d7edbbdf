"""Host clocks of the model layer, in plain double arithmetic (no torch, no library): the record clock that takes a model time
to two bracketing snapshots, the device loop's clock (cf_time_steps) held to it stretch by stretch, and the calendar table of
the monthly climatologies.  Every expression here decides bits of a result: the device receives these doubles."""
import datetime as _dt
import math
from collections import namedtuple

import numpy as np

minutes, hours, days = 60.0, 3600.0, 86400.0

# base: ⌊t / Δt_snapshot⌋ as it is; k1, k2: the snapshot COUNTERS (monotone in time; they stop at the ends of a clamped record);
# n1, n2: the record indices wrap(k1), wrap(k2); fraction: the position between them
RecordTime = namedtuple("RecordTime", "base k1 k2 n1 n2 fraction")


class RecordClock:
    """RecordClock(n_levels, time_interval, cyclic): the snapshot clock of a prescribed record — RepeatYearJRA55-style cyclic
    time indexing, or clamped at the ends of a multi-year record, where the fraction is 0."""

    def __init__(self, n_levels, time_interval, cyclic):
        self.n_levels, self.time_interval, self.cyclic = n_levels, time_interval, cyclic

    def wrap(self, k):
        """The record index of snapshot counter k."""
        return k % self.n_levels if self.cyclic else min(max(k, 0), self.n_levels - 1)

    def at(self, t):
        x = t / self.time_interval
        n = int(np.floor(x))
        frac = x - n
        if self.cyclic:
            k1, k2 = n, n + 1
        else:
            k1 = min(max(n, 0), self.n_levels - 1)
            k2 = min(max(n + 1, 0), self.n_levels - 1)
            if not (0 <= n < self.n_levels - 1):
                frac = 0.0
        return RecordTime(n, k1, k2, self.wrap(k1), self.wrap(k2), frac)


def device_clock(level1, fraction, n_levels, step, increment):
    """(first_level, time_fraction) with which the device loop's clock — total = time_fraction + step · increment, level1 =
    (first_level + ⌊total⌋) mod n_levels, ñ = total − ⌊total⌋ (cf_time_steps) — gives exactly (level1, fraction) at `step`,
    or None.  The sum is simulated in the same double arithmetic, so a returned pair is verified, not estimated."""
    base = float(step) * increment
    shift = max(0, math.ceil(base - fraction))
    guess = fraction + shift - base
    for tf in (guess, np.nextafter(guess, np.inf), np.nextafter(guess, -np.inf)):
        tf = float(tf)
        total = tf + base
        whole = math.floor(total)
        if tf >= 0.0 and total - whole == fraction:
            return (level1 - int(whole)) % n_levels, tf
    return None


def clock_at(first_level, time_fraction, n_levels, step, increment):
    """(level1, level2, ñ) of the device loop's clock at `step`."""
    total = time_fraction + float(step) * increment
    whole = math.floor(total)
    level1 = (first_level + int(whole)) % n_levels
    return level1, (level1 + 1) % n_levels, total - whole


def dataset_origin(time, step, dt):
    """time_origin with which the dataset clock of the device loop, origin + step · Δt, gives exactly `time` at `step`, or None"""
    base = float(step) * dt
    guess = time - base
    for origin in (guess, float(np.nextafter(guess, np.inf)), float(np.nextafter(guess, -np.inf))):
        if origin + base == time:
            return origin
    return None


def device_stretches(clocks, first, nsteps, times=None, dt=None):
    """The stretches of steps on which the device loop's clocks reproduce the host's, as (a, b, based, origin): steps a … b − 1
    of the call run from the re-based clocks `based` = [(first_level, time_fraction) per clock].  `clocks`: one (wanted,
    n_levels, increment) per clock, wanted[k] = the host's (n1, n2, fraction) after step k; the device numbers step k as
    first + k.  With `times` (the model time after each step, a repeated sum) and Δt, a dataset clock origin + step · Δt is
    held to those times too and `origin` is its origin for the stretch; None without.  A generator: a step that no re-based
    clock can take raises ValueError when the stretches before it have been handed out."""
    a = 0
    while a < nsteps:
        g = first + a
        based = []
        for want, n_levels, inc in clocks:
            n1, n2, frac = want[a]
            c = device_clock(n1, frac, n_levels, g, inc)
            if c is None or clock_at(c[0], c[1], n_levels, g, inc) != (n1, n2, frac):
                raise ValueError(f"time_steps: the device loop's clock cannot take the snapshots ({n1}, {n2}) at fraction {frac!r} "
                                 f"of step {g} (a clamped record at its end?); use time_step")
            based.append(c)
        b = a + 1
        while b < nsteps and all(clock_at(c[0], c[1], n_levels, first + b, inc) == tuple(want[b])
                                 for (want, n_levels, inc), c in zip(clocks, based)):
            b += 1
        origin = None
        if times is not None:
            origin = dataset_origin(times[a], g, dt)
            if origin is None:
                raise ValueError(f"time_steps: the dataset clock origin + step · Δt cannot give the model time {times[a]!r} at step {g}; use time_step")
            b = next((k for k in range(a + 1, b) if origin + float(first + k) * dt != times[k]), b)
        yield a, b, based, origin
        a = b


# ---------------------------------------------------------------------------------------------
# the calendar table of cf_attach_climatology / cf_calendar_bin
# ---------------------------------------------------------------------------------------------
def _month_start_seconds(reference_date, year, month):
    d = _dt.datetime(year, month, 1) - reference_date
    return d.days * 86400 + d.seconds


def calendar_bins(reference_date, first_time, last_time, kind="month", start_time=0, stop_time=math.inf):
    """The calendar table (edges, bin_of_interval) of cf_attach_climatology / cf_calendar_bin for times first_time … last_time
    [s since reference_date]: month(reference_date + Second(round(Int, t))) of compute_monthly_means (visualize/common.jl:184)
    as intervals of whole seconds in the proleptic Gregorian calendar (`datetime`, like Julia's Dates).  kind "month": bin
    m − 1 for calendar month m; "season": 0 DJF, 1 MAM, 2 JJA, 3 SON.  The edges are the month starts from the month of
    first_time to the end of the month of last_time; a rounded time outside [start_time, stop_time] (in_window, common.jl:161,
    applied to the rounded time) lies in an interval of bin −1: not collected."""
    if kind not in ("month", "season"):
        raise ValueError(f"calendar_bins: kind = {kind!r} (\"month\" or \"season\")")
    if not (math.isfinite(first_time) and math.isfinite(last_time) and first_time <= last_time):
        raise ValueError(f"calendar_bins: times {first_time} … {last_time}")
    first = reference_date + _dt.timedelta(seconds=round(first_time))
    last = reference_date + _dt.timedelta(seconds=round(last_time))
    months = []   # (start second, bin) from the month of `first` to the month after `last`
    y, m = first.year, first.month
    while True:
        months.append((_month_start_seconds(reference_date, y, m), m - 1 if kind == "month" else (m % 12) // 3))
        if (y, m) > (last.year, last.month):
            break
        y, m = (y, m + 1) if m < 12 else (y + 1, 1)
    lo = math.ceil(start_time) if math.isfinite(start_time) else (-math.inf if start_time < 0 else math.inf)
    hi = math.floor(stop_time) + 1 if math.isfinite(stop_time) else (math.inf if stop_time > 0 else -math.inf)
    cuts = sorted({s for s, _ in months} | {c for c in (lo, hi) if months[0][0] < c < months[-1][0]})
    edges, bins = np.array(cuts, dtype=np.float64), np.zeros(len(cuts) - 1, dtype=np.int32)
    starts = [s for s, _ in months]
    for k, a in enumerate(cuts[:-1]):
        owner = months[int(np.searchsorted(starts, a, side="right")) - 1][1]
        bins[k] = owner if lo <= a < hi else -1
    return edges, bins
