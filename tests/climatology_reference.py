"""The NumPy restatement of the calendar-binned means (include/coflux.h: cf_climatology_*, cf_calendar_bin): the running-mean
recurrence per destination with its products and its sum rounded separately, the calendar lookup, and Julia's min / max over
the non-empty bins with the index that attains each.  NumPy only: tests/test_climatology_cpu.py qualifies it without a GPU,
tests/test_climatology.py holds the device to it bit for bit.

`defect` seeds one of four defects into the restatement; test_climatology_cpu.py shows that each is caught by a named case:
    "bin_uses_total_coefficients"   the bin is blended with the total's (c_prev, c_new)
    "bin_first_blends"              a bin's first sample is blended into what the buffer held instead of stored
    "lookup_without_rounding"       the lookup compares the unrounded time with the edges
    "min_drops_nan"                 min / max skip NaNs (numpy's fmin / fmax) instead of propagating them
"""
import numpy as np

DEFECTS = ("bin_uses_total_coefficients", "bin_first_blends", "lookup_without_rounding", "min_drops_nan")


def coefficients(before, samples, weight):
    """(store, c_prev, c_new) of a destination that has received the weight `before` in `samples` collections and now receives
    `weight`: the host arithmetic of cf_average_collect, in double."""
    total = before + weight
    if samples == 0:
        return True, 0.0, 1.0
    return False, before / total, weight / total


def blend(m, f, c_prev, c_new):
    """m · c_prev + f · c_new with both products and the sum rounded (numpy never contracts)."""
    with np.errstate(invalid="ignore"):     # (Inf − Inf and Inf · 0 are NaN on the device too)
        a = np.asarray(m, dtype=np.float64) * np.float64(c_prev)
        b = np.asarray(f, dtype=np.float64) * np.float64(c_new)
        return a + b


class Climatology:
    """One field's total and bins under a sequence of collect(bin, weight, sample) / reset().  `total` and `bins[b]` start
    as the arrays given (default: NaN-filled — a fresh buffer) and are only ever replaced on collection."""

    def __init__(self, shape, n_bins, keep_total=True, initial=None, defect=None):
        assert defect is None or defect in DEFECTS
        fresh = lambda: np.full(shape, np.nan) if initial is None else np.array(initial, dtype=np.float64)  # noqa: E731
        self.n_bins, self.defect, self.keep_total = n_bins, defect, keep_total
        self.total = fresh() if keep_total else None
        self.bins = [fresh() for _ in range(n_bins)]
        self.reset()

    def reset(self):
        self.weight, self.samples = 0.0, 0
        self.bin_weight, self.bin_samples = [0.0] * self.n_bins, [0] * self.n_bins

    def collect(self, b, weight, sample):
        assert -1 <= b < self.n_bins and weight > 0 and np.isfinite(weight)
        if b < 0:
            return
        f = np.asarray(sample, dtype=np.float64)
        t_store, t_prev, t_new = coefficients(self.weight, self.samples, weight)
        b_store, b_prev, b_new = coefficients(self.bin_weight[b], self.bin_samples[b], weight)
        if self.defect == "bin_uses_total_coefficients" and not b_store:
            b_prev, b_new = t_prev, t_new
        if self.keep_total:
            self.total = f.copy() if t_store else blend(self.total, f, t_prev, t_new)
        if b_store and self.defect == "bin_first_blends":
            self.bins[b] = blend(self.bins[b], f, 0.0, 1.0)   # NaN · 0 is NaN: a fresh buffer poisons the mean
        else:
            self.bins[b] = f.copy() if b_store else blend(self.bins[b], f, b_prev, b_new)
        self.weight += weight
        self.samples += 1
        self.bin_weight[b] += weight
        self.bin_samples[b] += 1

    def extremes(self):
        return julia_extremes([self.bins[b] if self.bin_samples[b] else None for b in range(self.n_bins)], defect=self.defect)


def calendar_bin(edges, bin_of_interval, time, defect=None):
    """The bin of `time`: t_r = rint(time) (ties to even: Julia's round(Int, ·)), then k with edges[k] ≤ t_r < edges[k + 1].
    ValueError for a bad table or a time outside it."""
    edges = np.asarray(edges, dtype=np.float64)
    bins = np.asarray(bin_of_interval)
    if edges.size < 2 or bins.size != edges.size - 1 or not np.isfinite(edges).all() or not (np.diff(edges) > 0).all() or (bins < -1).any():
        raise ValueError("bad calendar table")
    if not np.isfinite(time):
        raise ValueError("time outside the table")
    t = float(time) if defect == "lookup_without_rounding" else float(np.rint(np.float64(time)))
    if t < edges[0] or not t < edges[-1]:
        raise ValueError("time outside the table")
    return int(bins[int(np.searchsorted(edges, t, side="right")) - 1])


def _negative(x):
    return np.signbit(x)


def julia_extremes(bins, defect=None):
    """(min, max, argmin, argmax) per cell over the bins that are not None, in ascending bin order with Julia's min / max: a NaN
    in any of them gives NaN, −0.0 < +0.0; the index is the smallest bin that attains the result, or the first NaN bin.
    ValueError when every bin is None (the reference: "has no available monthly bins")."""
    avail = [b for b, a in enumerate(bins) if a is not None]
    if not avail:
        raise ValueError("no available bins")
    first = np.asarray(bins[avail[0]], dtype=np.float64)
    mn, mx = first.copy(), first.copy()
    imin = np.full(first.shape, avail[0], dtype=np.int32)
    imax = imin.copy()
    for b in avail[1:]:
        v = np.asarray(bins[b], dtype=np.float64)
        with np.errstate(invalid="ignore"):
            lower = (v < mn) | ((v == mn) & _negative(v) & ~_negative(mn))
            upper = (v > mx) | ((v == mx) & ~_negative(v) & _negative(mx))
        if defect == "min_drops_nan":
            lower |= np.isnan(mn) & ~np.isnan(v)
            upper |= np.isnan(mx) & ~np.isnan(v)
        else:
            lower = (lower | np.isnan(v)) & ~np.isnan(mn)
            upper = (upper | np.isnan(v)) & ~np.isnan(mx)
        mn, imin = np.where(lower, v, mn), np.where(lower, b, imin).astype(np.int32)
        mx, imax = np.where(upper, v, mx), np.where(upper, b, imax).astype(np.int32)
    return mn, mx, imin, imax


def same_bits_but_nan_payload(a, b):
    """Equal bit for bit wherever neither is NaN, and NaN in the same places."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.int64), b[~nan].view(np.int64)))


# ---- the designed sequence of the bitwise tests: (bin, weight) records and a reset --------------------------------------------
RESET = "reset"


def designed_sequence(n_bins):
    """Records (bin, weight) | RESET that exercise, after the reset: a bin hit once, a bin never hit, two alternating bins,
    unequal weights 31 / 28 / 30, −1 records; before the reset every bin is hit so that stale means lie in all of them.  Bin
    numbers are folded into n_bins: with one bin everything alternates with itself (and nothing is never hit)."""
    fold = lambda b: b % n_bins  # noqa: E731
    head = [(fold(b), 1.0 + 0.5 * b) for b in range(min(n_bins, 12))] + [(-1, 2.0), (fold(3), 0.25)]
    tail = [(fold(0), 31.0), (fold(1), 28.0), (-1, 31.0), (fold(0), 30.0), (fold(1), 31.0), (fold(5), 30.0), (fold(0), 31.0),
            (-1, 1.0), (fold(1), 28.0), (fold(0), 0.75), (fold(n_bins - 1), 31.0) if n_bins > 8 else (fold(1), 3.0)]
    return head + [RESET] + tail


def hit_after_reset(n_bins):
    seq = designed_sequence(n_bins)
    tail = seq[seq.index(RESET) + 1:]
    return sorted({b for b, _ in tail if b >= 0})
