"""The two host rules of the collected diagnostics (csrc/coflux_collect.hpp) held on the CPU: the running-mean weight against
tests/climatology_reference.py::coefficients, the step schedule against a brute-force count and Python's floats, and the
checkpoint form of the weights against the bytes tests/checkpoint_reference.py lays out.  tests/collect_rules_driver.cpp
includes that header and nothing else of the library; it is compiled alone with -fsanitize=address,undefined, the runtimes
linked statically (nothing is preloaded), and run once as a subprocess that answers every question of this file."""
import math
import os
import re
import shutil
import struct
import subprocess

import pytest

import checkpoint_reference as ckref
from climatology_reference import coefficients

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "climaocean.jl_amd", "csrc")
RESET = "reset"

SEQUENCES = {
    "equal": [1.0] * 9,
    "dt_300": [300.0] * 12,
    "third": [1.0 / 3.0] * 12,
    "spanning": [1e-300, 1e-200, 1e-100, 1.0, 1e100, 1e200, 1e300, 1e-300, 1.0, 1e300],
    "reset_in_the_middle": [31.0, 28.0, 1.0 / 3.0, RESET, 30.0, 300.0, 1e-300, RESET, RESET, 1e300, 0.75],
    # refused: 0, −0, negatives, NaN, ±Inf — and the second 1.7e308, which would take the total to Inf
    "refusals": [0.0, -0.0, -1.0, -1e-300, math.nan, math.inf, -math.inf, 2.0, 0.0, math.nan, 1.7e308, 1.7e308, 1e300, 1e-300],
}
STRIDES = (1, 2, 3, 7, 4096)
FIRSTS = list(range(21)) + [2**40 - 3]
STAMPS = [(0.0, 300.0, 0), (0.0, 0.1, 2), (-1e9 / 3.0, 1200.0, 17), (86400.0 * 365.25, 1.0 / 3.0, 2**40 - 3), (1e-300, 1e300, 5),
          (7.25, -0.7, 2**31), (0.1, 0.2, 0), (3600.0, 1e-9, 2**52)]
WEIGHTS = [(0.0, 0), (3600.0, 3), (1e300, 2**40), (5e-324, 1), (1.0 / 3.0, 2**62), (1.7976931348623157e308, 2**63 - 1)]


def hx(v):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", v))[0]


def unhx(s):
    return struct.unpack("<d", struct.pack("<Q", int(s, 16)))[0]


def tails():
    """{bins: (weight, samples, bin weights, bin samples)}: unequal numbers in every place, an empty bin where there are several"""
    out = {}
    for n in (1, 12, 32):
        bw = [0.0 if (n > 1 and b == 1) else 28.0 + b + 1.0 / (3.0 + b) for b in range(n)]
        bs = [0 if w == 0.0 else 1 + 7 * b for b, w in enumerate(bw)]
        out[n] = (math.fsum(bw) * (1.0 + 2.0**-40), sum(bs) + 2**33, bw, bs)
    return out


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    """{question line: the driver's answer line}, from one run of the sanitizer build"""
    compiler = shutil.which("g++") or shutil.which("clang++")
    if compiler is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("collect_rules") / "collect_rules_driver")
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(compiler) == "g++" else ["-static-libsan"]
    build = subprocess.run([compiler, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static, "-I", CSRC,
                            os.path.join(ROOT, "tests", "collect_rules_driver.cpp"), "-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and re.search(r"cannot find.*(asan|ubsan|clang_rt)|libasan|libubsan|asan_preinit|static-lib", build.stderr):
        pytest.skip("the sanitizer runtime does not link here: " + build.stderr.strip().splitlines()[-1])
    assert build.returncode == 0, build.stderr
    questions = ["weights " + " ".join(w if w == RESET else hx(w) for w in seq) for seq in SEQUENCES.values()]
    questions += [f"collections {stride} {first} {n}" for stride in STRIDES for first in FIRSTS for n in range(21)]
    questions += [f"stamp {hx(origin)} {hx(seconds)} {step}" for origin, seconds, step in STAMPS]
    questions += [f"weight {hx(total)} {samples}" for total, samples in WEIGHTS]
    for n, (weight, samples, bw, bs) in tails().items():
        questions.append(f"tail {n} {hx(weight)} {samples} " + " ".join(f"{hx(w)} {s}" for w, s in zip(bw, bs)))
    run = subprocess.run([exe], input="\n".join(questions) + "\n", capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    lines = run.stdout.splitlines()
    assert len(lines) == len(questions)
    return dict(zip(questions, lines))


def replay(answers, name):
    """[(weight, before, samples before, (accepted, store, c_prev, c_new, total, samples) of the driver)] of a sequence, with the
    weight's history kept in Python floats"""
    seq = SEQUENCES[name]
    fields = answers["weights " + " ".join(w if w == RESET else hx(w) for w in seq)].split()
    weights = [w for w in seq if w != RESET]
    assert len(fields) == 6 * len(weights)
    out, before, samples, k = [], 0.0, 0, 0
    for w in seq:
        if w == RESET:
            before, samples = 0.0, 0
            continue
        f = fields[6 * k:6 * k + 6]
        k += 1
        got = (f[0] == "1", f[1] == "1", f[2], f[3], f[4], int(f[5]))
        out.append((w, before, samples, got))
        if got[0]:
            before, samples = before + w, samples + 1
        assert (got[4], got[5]) == (hx(before), samples), (name, k)
    return out


@pytest.mark.parametrize("name", ["equal", "dt_300", "third", "spanning", "reset_in_the_middle"])
def test_running_mean_coefficients_are_the_references_bit_for_bit(answers, name):
    records = replay(answers, name)
    for w, before, samples, (accepted, store, c_prev, c_new, _, _) in records:
        want_store, want_prev, want_new = coefficients(before, samples, w)
        assert accepted and (store, c_prev, c_new) == (want_store, hx(want_prev), hx(want_new)), (name, w, before, samples)
    assert records[0][3][1] and not any(r[3][1] for r in records[1:] if r[2] > 0)


def test_the_first_sample_after_a_reset_stores(answers):
    records = replay(answers, "reset_in_the_middle")
    firsts = [r for r in records if r[2] == 0]
    assert len(firsts) == 3
    for w, before, samples, (accepted, store, c_prev, c_new, total, n) in firsts:
        assert accepted and store and (c_prev, c_new) == (hx(0.0), hx(1.0)) and (total, n) == (hx(w), 1)
    assert all(not r[3][1] for r in records if r[2] > 0)


def test_accepts_refuses_what_is_not_a_positive_finite_weight_and_a_total_that_overflows(answers):
    records = replay(answers, "refusals")
    accepted = [r[0] for r in records if r[3][0]]
    assert accepted == [2.0, 1.7e308, 1e300, 1e-300]
    for w, before, samples, got in records:
        assert got[0] == (w > 0.0 and math.isfinite(w) and math.isfinite(before + w)), (w, before)
    # the weight that overflows the total is refused although it is itself finite, and leaves the total as it was
    overflow = [r for r in records if r[0] == 1.7e308 and not r[3][0]]
    assert len(overflow) == 1 and overflow[0][1] == 2.0 + 1.7e308 and overflow[0][3][4] == hx(overflow[0][1])


def test_collections_is_the_brute_force_count_of_due_steps(answers):
    for stride in STRIDES:
        for first in FIRSTS:
            for n in range(21):
                brute = sum(1 for s in range(first, first + n) if (s + 1) % stride == 0)
                assert answers[f"collections {stride} {first} {n}"].split() == [str(brute), str(brute)], (stride, first, n)
    # (step 2⁴⁰ − 1 is due under every stride: the third step from 2⁴⁰ − 3)
    assert [answers[f"collections 4096 {2**40 - 3} {n}"].split()[0] for n in (2, 3, 20)] == ["0", "1", "1"]
    assert answers[f"collections 7 {2**40 - 3} 20"].split()[0] == "3"


def test_stamp_is_origin_plus_steps_times_seconds_in_python_floats(answers):
    for origin, seconds, step in STAMPS:
        assert answers[f"stamp {hx(origin)} {hx(seconds)} {step}"] == hx(origin + float(step + 1) * seconds), (origin, seconds, step)


def test_the_16_byte_weight_form_round_trips_and_is_the_averages_payload(answers):
    for total, samples in WEIGHTS:
        raw, back_total, back_samples = answers[f"weight {hx(total)} {samples}"].split()
        assert bytes.fromhex(raw) == ckref.average_payload(total, samples) and len(raw) == 32
        assert (back_total, int(back_samples)) == (hx(total), samples)


@pytest.mark.parametrize("n_bins", [1, 12, 32])
def test_a_climatology_tail_is_the_reference_payload(answers, n_bins):
    weight, samples, bw, bs = tails()[n_bins]
    question = f"tail {n_bins} {hx(weight)} {samples} " + " ".join(f"{hx(w)} {s}" for w, s in zip(bw, bs))
    raw, again = answers[question].split()
    want = ckref.climatology_payload(weight, samples, bw, bs)
    assert len(want) == 16 + 16 * n_bins and bytes.fromhex(raw) == want
    assert bytes.fromhex(again) == want   # read back and written again: the same bytes
