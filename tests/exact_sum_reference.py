"""The reference of the exact sum (csrc/coflux_exact_sum.hpp): the terms as fractions.Fraction, summed and rounded ONCE.

`sum_bits` answers what xs_round gives for a list of doubles, as the 64 bits of a double; `scaled_integer` is the sum of the
finite terms as the integer Σ · 2¹⁰⁸⁸, which an accumulator's 67 digits spell in base 2³² (digit k weighs 2^(32k − 1088)).
`salinity_terms` lays out the terms of cf_normalize_salinity_flux_exact for a case of the normalisation tests."""
import math
import struct
from fractions import Fraction

import numpy as np

DIGITS, BIAS, WORDS = 67, 1088, 70
NAN_BITS, PINF_BITS, NINF_BITS = 0x7FF8000000000000, 0x7FF0000000000000, 0xFFF0000000000000
LARGEST = 1.7976931348623157e308


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def from_bits(u):
    return struct.unpack("<d", struct.pack("<Q", u))[0]


def nonfinite_counts(values):
    """[NaN terms, +Inf terms, −Inf terms]"""
    v = np.asarray(values, dtype=np.float64)
    return [int(np.isnan(v).sum()), int(np.isposinf(v).sum()), int(np.isneginf(v).sum())]


def exact(values):
    """Σ of the finite terms, exactly (repeats of one value are multiplied, not added one by one)"""
    v = np.asarray(values, dtype=np.float64).ravel()
    v = v[np.isfinite(v)]
    uniq, count = np.unique(v, return_counts=True)
    total = Fraction(0)
    for x, c in zip(uniq.tolist(), count.tolist()):
        total += Fraction(x) * c
    return total


def round_once(total):
    """a Fraction to the bits of the nearest double, ties to even; ±Inf beyond the largest double; a zero is +0.0"""
    if total == 0:
        return 0
    try:
        return bits(total.numerator / total.denominator)   # int / int is correctly rounded, subnormals included
    except OverflowError:
        return PINF_BITS if total > 0 else NINF_BITS


def sum_bits(values):
    nan, pinf, ninf = nonfinite_counts(values)
    if nan or (pinf and ninf):
        return NAN_BITS
    if pinf:
        return PINF_BITS
    if ninf:
        return NINF_BITS
    return round_once(exact(values))


def scaled_integer(values):
    scaled = exact(values) * 2**BIAS
    assert scaled.denominator == 1   # every double is a multiple of 2⁻¹⁰⁷⁴
    return scaled.numerator


def digits_value(digits):
    """what 67 signed digits spell, carried or not"""
    assert len(digits) == DIGITS
    return sum(int(d) << (32 * k) for k, d in enumerate(digits))


def wet_interior(case):
    """boolean parent-shaped array: the wet interior cells of a case {nx, ny, hx, hy, mask_kind, mask, z_surface}"""
    nx, ny, hx, hy = case["nx"], case["ny"], case["hx"], case["hy"]
    wet = np.zeros((ny + 2 * hy, nx + 2 * hx), dtype=bool)
    inner = (slice(hy, hy + ny), slice(hx, hx + nx))
    if case["mask"] is None:
        wet[inner] = True
    elif case["mask"].dtype == np.uint8:
        wet[inner] = case["mask"][inner] != 0
    else:
        wet[inner] = ~(case["z_surface"] <= case["mask"][inner])
    return wet


def salinity_terms(case):
    """(t, a) over the wet interior: v = fl(flux + additional), t = fl(v · a), a = area or 1.0 — two roundings, no fused form"""
    wet = wet_interior(case)
    v = case["flux"][wet].astype(np.float64)
    if case["additional"] is not None:
        v = v + case["additional"][wet]
    a = case["area"][wet].astype(np.float64) if case["area"] is not None else np.ones(v.shape)
    return v * a, a


def mean_bits(sj_bits, sa_bits):
    """salinity_subtract_kernel: mean = sums[1] > 0 ? sums[0] / sums[1] : 0"""
    sj, sa = from_bits(sj_bits), from_bits(sa_bits)
    if not sa > 0.0:
        return 0
    with np.errstate(all="ignore"):
        return bits(np.float64(sj) / np.float64(sa))


# ---- designed lists (tests/test_exact_sum_cpu.py; laid into wet cells by tests/test_exact_normalization.py) -------------------
def designed_lists():
    rng = np.random.default_rng(20240607)
    sub = 5e-324
    lists = {
        "cancel_1e300": [1e300, 1e-300, -1e300] * 5 + [-1e300, 1e300],
        "subnormals": [sub * int(k) for k in rng.integers(1, 2**52, 40)] + [-sub * int(k) for k in rng.integers(1, 2**52, 23)],
        "subnormal_to_normal": [2.0**-1023] * 6 + [sub] * 3,
        "huge_partials_small_end": [LARGEST, LARGEST, 3.0, -LARGEST, 2.0**-40, -LARGEST, -1.0, 1e308, 1e308, -1e308, -1e308],
        "zeros": [0.0, -0.0, 0.0, -0.0, -0.0],
        "negative_zero": [-0.0],
        "tie_to_even_down": [2.0**53, 1.0],
        "tie_to_even_up": [2.0**53 + 2.0, 1.0],
        "tie_broken_far_below": [2.0**53, 1.0, sub],
        "tie_broken_negative": [-(2.0**53), -1.0, -sub],
        "round_up_to_power": [2.0**53 - 1.0, 2.0**53 - 1.0, 1.0, 0.5],
        "overflow_by_rounding": [LARGEST, 2.0**970],
        "just_below_overflow": [LARGEST, 2.0**969],
        "negative_overflow": [-LARGEST, -LARGEST],
        "mixed": (rng.standard_normal(300) * 10.0 ** rng.integers(-300, 300, 300)).tolist(),
        "salt_like": (rng.standard_normal(700) * 1e-5 * 3e9).tolist(),
    }
    for name, v in lists.items():
        assert all(math.isfinite(x) for x in v), name
    return lists


def nonfinite_lists():
    """NaN and ±Inf in every combination, among finite terms"""
    out = {}
    for nan in (0, 1, 2):
        for pinf in (0, 1, 3):
            for ninf in (0, 1, 2):
                if nan + pinf + ninf:
                    out[f"nan{nan}_pinf{pinf}_ninf{ninf}"] = ([1.5, -2.25e10] + [math.nan] * nan + [7.0] + [math.inf] * pinf +
                                                              [-math.inf] * ninf + [1e-310])
    return out
