"""Schedules of output writers and callbacks (Oceananigans' IterationInterval, TimeInterval, AveragedTimeInterval): host
bookkeeping only.  `actuates(schedule, clock)` is how run!(simulation) and every writer ask a schedule."""
import numpy as np


class IterationInterval:
    """IterationInterval(n): every n-th iteration."""

    def __init__(self, interval):
        if int(interval) != interval or interval < 1:
            raise ValueError(f"IterationInterval: interval = {interval} (an integer ≥ 1)")
        self.interval = int(interval)

    def actuate(self, iteration):
        return iteration % self.interval == 0


class TimeInterval:
    """TimeInterval(interval): actuates when the clock reaches k · interval, k = 1, 2, … — the schedule of the reference's
    Checkpointer (omip_diagnostics.jl:220-225).  A step counts as having reached k · interval when it is within 1e-6 · Δt of
    it, AveragedTimeInterval's rule.  Host bookkeeping only."""

    def __init__(self, interval):
        if not (interval > 0):
            raise ValueError(f"TimeInterval: interval = {interval} (> 0)")
        self.interval = float(interval)
        self.k = None   # the next actuation is at k · interval
        self._tol = 0.0

    def initialize(self, time, dt):
        """Opens the first interval that ends after `time` (called again after a pickup, with the restored clock)."""
        self._tol = 1e-6 * dt
        self.k = int(np.floor((time + self._tol) / self.interval)) + 1

    def actuate(self, time):
        if self.k is None:
            self.initialize(0.0, 0.0)
        if time >= self.k * self.interval - self._tol:
            self.k = int(np.floor((time + self._tol) / self.interval)) + 1
            return True
        return False


class AveragedTimeInterval:
    """AveragedTimeInterval(interval; window = interval, stride = 1) — the schedule of the reference's averaged writers
    (omip_diagnostics.jl:152-158, examples/latitude_longitude_ocean_sea_ice.jl:60-66).  Window k is (t_k − window, t_k] with
    t_k = k · interval.  Inside a window a step's sample is taken when iteration % stride == 0, and always at t_k; its
    weight is the time since the previous sample or since the window opened, t_n − max(t_prev, t_k − window).  The time
    step must divide `interval`.  Host bookkeeping only: sample() says what to collect, the writer collects it."""

    def __init__(self, interval, window=None, stride=1):
        window = interval if window is None else window
        if not (interval > 0) or not (0 < window <= interval):
            raise ValueError(f"AveragedTimeInterval: interval = {interval}, window = {window} (0 < window ≤ interval)")
        if int(stride) != stride or stride < 1:
            raise ValueError(f"AveragedTimeInterval: stride = {stride} (an integer ≥ 1)")
        self.interval, self.window, self.stride = float(interval), float(window), int(stride)
        self.k = None             # the open window ends at k · interval
        self.previous = None      # time of the last sample

    def initialize(self, time, dt):
        """Checks the time step; the first call also opens the first window that ends after `time` (an open window survives
        the end of run!, as in Oceananigans)."""
        ratio = self.interval / dt if dt > 0 else 0.0
        if round(ratio) < 1 or abs(ratio - round(ratio)) > 1e-9 * ratio:
            raise ValueError(f"AveragedTimeInterval: the time step {dt} does not divide the interval {self.interval}")
        self._tol = 1e-6 * dt
        if self.k is None:
            self.k = int(np.floor((time + self._tol) / self.interval)) + 1
            self.previous = float(time)

    def sample(self, time, iteration):
        """(weight, t_k) for the step that has just reached `time`: weight is None when nothing is collected, t_k is the end
        of the window that this sample completes (None while it stays open)."""
        t_k = self.k * self.interval
        end = time >= t_k - self._tol
        if end:
            time = t_k
        start = t_k - self.window
        if time <= start + self._tol or (not end and iteration % self.stride != 0):
            return None, None
        weight = time - max(self.previous, start)
        self.previous = time
        if not end:
            return weight, None
        self.k += 1
        return weight, t_k


def as_schedule(schedule, default=None):
    """An int n is IterationInterval(n); None is `default` (IterationInterval(1) unless one is given); a schedule is itself."""
    if isinstance(schedule, int):
        return IterationInterval(schedule)
    return schedule or default or IterationInterval(1)


def actuates(schedule, clock):
    """Whether `schedule` actuates at `clock`: a TimeInterval is asked with the time, every other schedule with the iteration."""
    return schedule.actuate(clock.time if isinstance(schedule, TimeInterval) else clock.iteration)


def open_at(schedule, time, dt):
    """A TimeInterval opens its first interval after `time`, with Δt for its tolerance; an iteration schedule has nothing to open."""
    if isinstance(schedule, TimeInterval):
        schedule.initialize(time, dt)
