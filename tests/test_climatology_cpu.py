"""CPU-side checks of the calendar-binned means (include/coflux.h: cf_climatology_*, cf_calendar_bin, cf_attach_climatology):
the new symbols in the header, the ctypes mirror and the Julia stub; cf_calendar_bin — a pure host function — against
coflux.models.calendar_bins and a brute-force `datetime` month on designed times; calendar_bins itself; the NumPy restatement
of tests/climatology_reference.py qualified alone against exact rational arithmetic; and four defects seeded into the
restatement, each caught by a named case.  No GPU."""
import ctypes as C
import datetime as dt
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import climatology_reference as cr
from coflux import abi
from coflux import models as cm
from coflux.runtime import calendar_bin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("cf_climatology_create", "cf_climatology_destroy", "cf_climatology_reset", "cf_climatology_collect", "cf_climatology_weights",
           "cf_climatology_extremes", "cf_calendar_bin", "cf_attach_climatology")
REF = dt.datetime(1958, 1, 1)
DAY = 86400


# ---- symbols and structs ------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "coflux.h")).read()
    stub = open(os.path.join(ROOT, "climaocean.jl_amd", "julia", "CoFluxMI355X.jl")).read()
    lib = abi.load_library()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"\bint " + name + r"\s*\(", code), f"{name} is not declared in include/coflux.h"
        assert name in abi.EXPORTED_SYMBOLS and hasattr(lib, name), name
        assert f"(:{name}, libcoflux)" in stub, f"{name} is not bound in CoFluxMI355X.jl"
    assert "#define CF_ABI_VERSION 5" in header and lib.cf_version() == 5
    assert "#define CF_CLIMATOLOGY_MAX_FIELDS 16" in header and abi.CLIMATOLOGY_MAX_FIELDS == 16
    assert "#define CF_CLIMATOLOGY_MAX_BINS 32" in header and abi.CLIMATOLOGY_MAX_BINS == 32


def test_descriptor_has_one_size_in_the_three_copies():
    import test_julia_stub as tj
    structs = tj.julia_structs()
    assert "CfClimatologyDesc" in structs
    size = C.sizeof(abi.ClimatologyDesc)
    assert size == 4 * 4 + 3 * 16 * 8 + 2 * 4 == 408
    assert tj.struct_size("CfClimatologyDesc", structs)[0] == size
    assert [f for f, _ in structs["CfClimatologyDesc"]] == [f for f, *_ in abi.ClimatologyDesc._fields_]
    # without a context the create call is refused and hands no handle out
    lib = abi.load_library()
    desc = abi.ClimatologyDesc()
    h = C.c_void_p()
    assert lib.cf_climatology_create(None, C.byref(desc), C.byref(h)) == -1 and not h.value


# ---- cf_calendar_bin ----------------------------------------------------------------------------------------------------------
def brute_month(t):
    """month(reference_date + Second(round(Int, t))) — Python's round() of a float is to nearest, ties to even, like Julia's."""
    return (REF + dt.timedelta(seconds=round(t))).month


def seconds(*ymd):
    d = dt.datetime(*ymd) - REF
    return d.days * DAY + d.seconds


TABLE = cm.calendar_bins(REF, 0, seconds(1961, 12, 31))


def test_designed_times_against_the_brute_force_month():
    edges = TABLE[0]
    even = next(e for e in edges[1:] if e % 2 == 0)
    odd_table = cm.calendar_bins(REF + dt.timedelta(seconds=1), 0, 400 * DAY)     # every edge of this one is odd
    odd = odd_table[0][2]
    assert even % 2 == 0 and odd % 2 == 1
    feb1 = float(seconds(1958, 2, 1))
    times = {"an exact edge": feb1, "edge − 0.4 s rounds into the next month": feb1 - 0.4, "edge − 0.6 s": feb1 - 0.6,
             "even edge − 0.5 (tie → the edge)": even - 0.5, "even edge + 0.5 (tie → the edge)": even + 0.5,
             "29 Feb 1960": seconds(1960, 2, 29) + 12 * 3600.0, "1 Mar 1960": float(seconds(1960, 3, 1)),
             "31 Dec 23:59:59.4": seconds(1959, 1, 1) - 0.6, "31 Dec → 1 Jan": seconds(1959, 1, 1) - 0.4, "t = 0": 0.0}
    for what, t in times.items():
        assert calendar_bin(TABLE, t) + 1 == brute_month(t), what
        assert cr.calendar_bin(*TABLE, t) + 1 == brute_month(t), what
    assert calendar_bin(TABLE, feb1 - 0.4) == 1 and calendar_bin(TABLE, feb1 - 0.6) == 0
    assert calendar_bin(TABLE, seconds(1960, 2, 29) + 5.0) == 1 and calendar_bin(TABLE, seconds(1959, 1, 1) - 0.4) == 0
    # ties to even: even − 0.5 and even + 0.5 both round TO the even edge, odd ± 0.5 both round AWAY from the odd edge
    k = int(np.searchsorted(edges, even))
    assert calendar_bin(TABLE, even - 0.5) == calendar_bin(TABLE, even + 0.5) == TABLE[1][k]
    ref2 = REF + dt.timedelta(seconds=1)
    for t in (odd - 0.5, odd + 0.5):
        want = (ref2 + dt.timedelta(seconds=round(t))).month - 1
        assert calendar_bin(odd_table, t) == cr.calendar_bin(*odd_table, t) == want
    assert calendar_bin(odd_table, odd - 0.5) != calendar_bin(odd_table, odd + 0.5)


def test_a_sweep_of_times_against_the_brute_force_month():
    rng = np.random.default_rng(7)
    last = TABLE[0][-1]
    times = np.concatenate([rng.uniform(0, last - 1, 400), rng.integers(0, int(last) - 1, 200) + 0.5, TABLE[0][:-1]])
    for t in times:
        assert calendar_bin(TABLE, float(t)) + 1 == brute_month(float(t)), t


def test_not_collected_intervals_and_errors():
    edges, bins = np.array([10.0, 20.0, 30.0, 45.0]), np.array([0, -1, 2], dtype=np.int32)
    assert [calendar_bin((edges, bins), t) for t in (10.0, 19.4, 19.6, 29.5, 30.5, 44.4)] == [0, 0, -1, 2, 2, 2]
    for t in (9.4, 44.6, 45.0, 1e30, float("nan"), float("inf")):       # below the first edge, at and beyond the last, not finite
        with pytest.raises(ValueError, match="outside the table"):
            calendar_bin((edges, bins), t)
        with pytest.raises(ValueError):
            cr.calendar_bin(edges, bins, t)
    assert calendar_bin((edges, bins), 9.6) == 0                         # rounds onto the first edge
    for bad in (np.array([10.0, 20.0, 20.0, 45.0]), np.array([10.0, 30.0, 20.0, 45.0]), np.array([10.0, np.nan, 30.0, 45.0])):
        with pytest.raises(ValueError, match="strictly increasing|not finite"):
            calendar_bin((bad, bins), 15.0)
        with pytest.raises(ValueError):
            cr.calendar_bin(bad, bins, 15.0)
    with pytest.raises(ValueError, match="n_edges"):
        calendar_bin((np.array([10.0]), np.zeros(0, dtype=np.int32)), 10.0)
    with pytest.raises(ValueError, match="−1 or a bin"):
        calendar_bin((edges, np.array([0, -2, 1], dtype=np.int32)), 15.0)
    lib = abi.load_library()
    out = C.c_int32()
    e, b = edges.ctypes.data_as(abi.c_double_p), bins.ctypes.data_as(abi.c_int32_p)
    assert lib.cf_calendar_bin(None, b, 4, 15.0, C.byref(out)) == -1 and lib.cf_calendar_bin(e, None, 4, 15.0, C.byref(out)) == -1
    assert lib.cf_calendar_bin(e, b, 4, 15.0, None) == -1 and lib.cf_calendar_bin(e, b, 4, 15.0, C.byref(out)) == 0 and out.value == 0


# ---- calendar_bins ------------------------------------------------------------------------------------------------------------
def test_calendar_bins_months_of_1958_to_1961():
    edges, bins = TABLE
    assert edges[0] == 0 and (np.diff(edges) > 0).all() and len(bins) == len(edges) - 1 == 48
    assert sorted(set(bins.tolist())) == list(range(12))
    assert bins.tolist() == [m % 12 for m in range(48)]
    lengths = np.diff(edges) / DAY
    common = [31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31]
    leap = common[:1] + [29] + common[2:]
    assert lengths.tolist() == common + common + leap + common       # 1960 is the leap year
    # a table starts at the month of first_time and ends behind the month of last_time
    e2, b2 = cm.calendar_bins(REF, seconds(1958, 3, 15), seconds(1958, 5, 2))
    assert e2.tolist() == [seconds(1958, 3, 1), seconds(1958, 4, 1), seconds(1958, 5, 1), seconds(1958, 6, 1)] and b2.tolist() == [2, 3, 4]
    # the proleptic Gregorian rule at a century: 1900 is no leap year, 2000 is
    for year, feb in ((1900, 28), (2000, 29)):
        e3, _ = cm.calendar_bins(dt.datetime(year, 1, 1), 0, 100 * DAY)
        assert (e3[2] - e3[1]) / DAY == feb


def test_calendar_bins_seasons_and_window():
    edges, bins = cm.calendar_bins(REF, 0, seconds(1959, 12, 31), kind="season")
    assert sorted(set(bins.tolist())) == [0, 1, 2, 3]
    assert bins[:12].tolist() == [0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3, 0]          # DJF = 0: Jan, Feb, …, Dec
    start, stop = seconds(1958, 2, 10) + 0.25, float(seconds(1958, 4, 20))
    e, b = cm.calendar_bins(REF, 0, seconds(1958, 12, 31), start_time=start, stop_time=stop)
    assert math.ceil(start) in e and stop + 1 in e
    for t in np.arange(0.0, seconds(1958, 12, 31), 0.37 * DAY).tolist() + [start - 1, math.ceil(start), stop, stop + 1]:
        inside = start <= round(t) <= stop
        assert calendar_bin((e, b), t) == (brute_month(t) - 1 if inside else -1), t
    with pytest.raises(ValueError):
        cm.calendar_bins(REF, 0, 10, kind="week")


# ---- the restatement alone ----------------------------------------------------------------------------------------------------
def designed_samples(n, cells=64, seed=11):
    """n samples of `cells` values spanning 1e-8 … 1e5 with mixed sign, and integer weights (every running total is exact)."""
    rng = np.random.default_rng(seed)
    samples = [rng.choice([-1.0, 1.0], cells) * 10.0 ** rng.uniform(-8, 5, cells) for _ in range(n)]
    weights = [float(w) for w in rng.integers(1, 32, n)]
    return samples, weights


@pytest.mark.parametrize("n", [1, 2, 7, 40])
def test_restated_recurrence_stays_within_its_counted_bound_of_the_exact_mean(n):
    """The bound is counted from the recurrence.  The first collection stores: exact.  Every later one computes
    fl(fl(m · c_prev) + fl(f · c_new)) with c_prev = fl(T_prev / T_cur), c_new = fl(w / T_cur) and exact T (integer weights): to
    first order the carried error is multiplied by c_prev ≤ 1 and the collection adds 2u·(c_prev + c_new)·M = 2u·M for the
    coefficient and the product of either term and u·M for the sum, u = 2⁻⁵³, M the cell's largest |sample| (every mean is a
    convex combination, so it is bounded by M).  Recount: 3(n − 1)·u·M to first order — within the (3n + 2)·u·M the issue
    states, whose 5u·M of slack covers the second-order terms (≤ (3n·u)²·M for n ≤ 40).  The stated bound is asserted."""
    samples, weights = designed_samples(n)
    bins = [k % 3 for k in range(n)]
    c = cr.Climatology((64,), 3)
    for f, w, b in zip(samples, weights, bins):
        c.collect(b, w, f)
    u = Fraction(1, 2 ** 53)

    def check(got, members):
        for cell in range(64):
            exact = sum(Fraction(weights[k]) * Fraction(float(samples[k][cell])) for k in members) / sum(Fraction(weights[k]) for k in members)
            M = max(abs(Fraction(float(samples[k][cell]))) for k in members)
            assert abs(Fraction(float(got[cell])) - exact) <= (3 * len(members) + 2) * u * M, (cell, len(members))

    check(c.total, range(n))
    for b in range(3):
        members = [k for k in range(n) if bins[k] == b]
        if members:
            check(c.bins[b], members)
        else:
            assert np.isnan(c.bins[b]).all() and c.bin_samples[b] == 0
    assert c.weight == sum(weights) and c.samples == n


def test_a_bin_is_the_recurrence_of_its_own_subsequence():
    samples, weights = designed_samples(20)
    seq = [(k * 5) % 4 - 1 for k in range(20)]      # −1 records among bins 0 … 2
    c = cr.Climatology((64,), 3)
    alone = [cr.Climatology((64,), 1) for _ in range(3)]
    everything = cr.Climatology((64,), 1)
    for f, w, b in zip(samples, weights, seq):
        c.collect(b, w, f)
        if b >= 0:
            alone[b].collect(0, w, f)
            everything.collect(0, w, f)
    for b in range(3):
        assert np.array_equal(c.bins[b].view(np.int64), alone[b].total.view(np.int64))
    assert np.array_equal(c.total.view(np.int64), everything.total.view(np.int64))
    assert c.samples == sum(b >= 0 for b in seq)


# ---- seeded defects ----------------------------------------------------------------------------------------------------------
def _run(defect, n_bins=3):
    samples, weights = designed_samples(12, seed=5)
    seq = [0, 1, 0, 1, 2, 0, 1, 0, -1, 1, 0, 1]
    good, bad = cr.Climatology((64,), n_bins), cr.Climatology((64,), n_bins, defect=defect)
    for f, w, b in zip(samples, weights, seq):
        good.collect(b, w, f)
        bad.collect(b, w, f)
    return good, bad


def test_defect_bin_blended_with_the_totals_coefficients_is_caught():
    """Caught by: two alternating bins with unequal weights — the bin's bits differ from its own subsequence's mean."""
    good, bad = _run("bin_uses_total_coefficients")
    assert np.array_equal(good.total.view(np.int64), bad.total.view(np.int64))
    assert not np.array_equal(good.bins[0].view(np.int64), bad.bins[0].view(np.int64))
    assert np.array_equal(good.bins[2].view(np.int64), bad.bins[2].view(np.int64))      # hit once: stored either way


def test_defect_first_sample_of_a_bin_blended_is_caught_on_a_nan_buffer():
    """Caught by: NaN-filled (fresh) buffers — a bin's first sample must be stored without reading what was there."""
    good, bad = _run("bin_first_blends")
    assert np.isfinite(good.bins[0]).all() and np.isfinite(good.bins[2]).all()
    assert np.isnan(bad.bins[0]).all() and np.isnan(bad.bins[2]).all()
    zeroed = cr.Climatology((64,), 3, initial=np.zeros(64), defect="bin_first_blends")    # a zero-filled buffer would hide it
    zeroed.collect(0, 1.0, np.ones(64))
    assert np.array_equal(zeroed.bins[0], np.ones(64))


def test_defect_lookup_without_rounding_is_caught():
    """Caught by: edge − 0.4 s, which rounds into the next month."""
    t = seconds(1958, 2, 1) - 0.4
    assert cr.calendar_bin(*TABLE, t) == 1 == brute_month(t) - 1
    assert cr.calendar_bin(*TABLE, t, defect="lookup_without_rounding") == 0


def test_defect_min_that_drops_nan_is_caught():
    """Caught by: a NaN in one non-empty bin — Julia's min / max give NaN there and the index of the NaN bin."""
    bins = [np.array([1.0, 2.0, -0.0, 5.0]), None, np.array([np.nan, 1.0, 0.0, 5.0]), np.array([0.5, 3.0, 0.0, 5.0])]
    mn, mx, imin, imax = cr.julia_extremes(bins)
    assert np.isnan(mn[0]) and np.isnan(mx[0]) and imin[0] == imax[0] == 2
    assert mn[1:].tolist() == [1.0, -0.0, 5.0] and np.signbit(mn[2]) and imin[1:].tolist() == [2, 0, 0]
    assert mx[1:].tolist() == [3.0, 0.0, 5.0] and not np.signbit(mx[2]) and imax[1:].tolist() == [3, 2, 0]
    bad = cr.julia_extremes(bins, defect="min_drops_nan")
    assert bad[0][0] == 0.5 and bad[1][0] == 1.0
    with pytest.raises(ValueError):
        cr.julia_extremes([None, None])
