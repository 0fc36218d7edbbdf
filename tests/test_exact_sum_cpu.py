"""The exact sum's format and rounding (csrc/coflux_exact_sum.hpp) held on the CPU against fractions.Fraction, summed and rounded
once (tests/exact_sum_reference.py).  tests/exact_sum_driver.cpp includes that header and nothing else; it is compiled alone with
-fsanitize=address,undefined, the runtimes linked statically (nothing is preloaded), and run once as a subprocess that answers
every question of this file.  Checked: the bits of the rounded sum, that the digits spell the exact sum, and that the digits of a
list are the digit-wise sum of the digits of its parts, however it is split."""
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import exact_sum_reference as xs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "climaocean.jl_amd", "csrc")

LISTS = xs.designed_lists()
NONFINITE = xs.nonfinite_lists()
# a single term of every exponent: the smallest subnormal 2⁻¹⁰⁷⁴ … 2¹⁰²³, and a full mantissa at every exponent field
POWERS = [math.ldexp(1.0, e) for e in range(-1074, 1024)]
FULL = [math.ldexp(1.0 + 0.5 + 2.0**-52, e) for e in range(-1022, 1024)]
MANY_LARGEST = 2**20


def tokens(values):
    return " ".join("%016x" % xs.bits(v) for v in values)


def split_points(n, parts, rng):
    cuts = sorted(rng.integers(0, n + 1, parts - 1).tolist())
    return [0] + cuts + [n]


def splits_of(name, values):
    """the list as 1, 2, 3 and 4 parts (empty parts occur)"""
    rng = np.random.default_rng(len(values) * 1000003 + len(name))
    out = []
    for parts in (1, 2, 3, 4):
        at = split_points(len(values), parts, rng)
        out.append("sum " + " | ".join(tokens(values[a:b]) for a, b in zip(at, at[1:])))
    return out


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    """{question line: (bits of the rounded sum, digits, counters)}, from one run of the sanitizer build"""
    compiler = shutil.which("g++") or shutil.which("clang++")
    if compiler is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("exact_sum") / "exact_sum_driver")
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(compiler) == "g++" else ["-static-libsan"]
    build = subprocess.run([compiler, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static, "-I", CSRC,
                            os.path.join(ROOT, "tests", "exact_sum_driver.cpp"), "-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and re.search(r"cannot find.*(asan|ubsan|clang_rt)|libasan|libubsan|asan_preinit|static-lib", build.stderr):
        pytest.skip("the sanitizer runtime does not link here: " + build.stderr.strip().splitlines()[-1])
    assert build.returncode == 0, build.stderr
    questions = ["sum " + tokens([v]) for v in POWERS + FULL] + ["sum " + tokens([-v]) for v in POWERS[::17] + FULL[::13]]
    for name, values in {**LISTS, **NONFINITE}.items():
        questions += splits_of(name, values)
    questions.append("sum %016x*%d" % (xs.bits(xs.LARGEST), MANY_LARGEST))
    questions.append("sum %016x*%d | %016x*%d" % (xs.bits(xs.LARGEST), MANY_LARGEST, xs.bits(-xs.LARGEST), MANY_LARGEST - 1))
    questions.append("sum")
    run = subprocess.run([exe], input="\n".join(questions) + "\n", capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    lines = run.stdout.splitlines()
    assert len(lines) == len(questions)
    out = {}
    for q, line in zip(questions, lines):
        f = line.split()
        assert len(f) == 1 + xs.WORDS, line
        out[q] = (int(f[0], 16), [int(d) for d in f[1:1 + xs.DIGITS]], [int(c) for c in f[1 + xs.DIGITS:]])
    return out


def test_a_single_term_of_every_exponent_comes_back_as_itself(answers):
    for v in POWERS + FULL + [-x for x in POWERS[::17] + FULL[::13]]:
        got, digits, counters = answers["sum " + tokens([v])]
        assert got == xs.bits(v), (v, hex(got))
        assert xs.digits_value(digits) == xs.scaled_integer([v]) and counters == [0, 0, 0], v
        assert sum(1 for d in digits if d) <= 3, v   # three adjacent digits at the most


@pytest.mark.parametrize("name", sorted(LISTS))
def test_designed_lists_round_once_to_the_references_bits(answers, name):
    values = LISTS[name]
    want = xs.sum_bits(values)
    for q in splits_of(name, values):
        got, digits, counters = answers[q]
        assert got == want, (name, q.count("|") + 1, hex(got), hex(want))
        assert xs.digits_value(digits) == xs.scaled_integer(values) and counters == [0, 0, 0]


@pytest.mark.parametrize("name", sorted({**LISTS, **NONFINITE}))
def test_the_digits_of_a_list_are_the_digitwise_sum_of_its_parts(answers, name):
    values = {**LISTS, **NONFINITE}[name]
    whole, *split = splits_of(name, values)
    for q in split:
        assert answers[q] == answers[whole], (name, q.count("|") + 1)


def test_zero_sums_are_positive_zero(answers):
    for name in ("zeros", "negative_zero", "cancel_1e300"):
        got, digits, _ = answers[splits_of(name, LISTS[name])[0]]
        if name == "cancel_1e300":
            assert got == xs.bits(5e-300) and got == xs.sum_bits(LISTS[name])   # the residue, not a zero
        else:
            assert got == 0 and not any(digits), name
    assert answers["sum"][0] == 0


def test_many_copies_of_the_largest_double_overflow_to_infinity_and_cancel_exactly(answers):
    got, digits, counters = answers["sum %016x*%d" % (xs.bits(xs.LARGEST), MANY_LARGEST)]
    assert got == xs.PINF_BITS and counters == [0, 0, 0]
    assert xs.digits_value(digits) == xs.scaled_integer([xs.LARGEST]) * MANY_LARGEST
    got, digits, _ = answers["sum %016x*%d | %016x*%d" % (xs.bits(xs.LARGEST), MANY_LARGEST, xs.bits(-xs.LARGEST), MANY_LARGEST - 1)]
    assert got == xs.bits(xs.LARGEST) and xs.digits_value(digits) == xs.scaled_integer([xs.LARGEST])


@pytest.mark.parametrize("name", sorted(NONFINITE))
def test_nan_and_infinities_in_every_combination(answers, name):
    values = NONFINITE[name]
    got, digits, counters = answers[splits_of(name, values)[0]]
    assert counters == xs.nonfinite_counts(values)
    assert got == xs.sum_bits(values), (name, hex(got))
    assert xs.digits_value(digits) == xs.scaled_integer(values)   # the finite terms are summed all the same
    nan, pinf, ninf = counters
    assert got == (xs.NAN_BITS if nan or (pinf and ninf) else xs.PINF_BITS if pinf else xs.NINF_BITS)
