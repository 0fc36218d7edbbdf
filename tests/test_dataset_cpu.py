"""The host rules of a staged dataset (csrc/coflux_dataset_rules.hpp) held on the CPU against tests/dataset_reference.py: the
clock bit for bit, and the sweep plan — depth by one breadth-first pass — against the number of sweeps the reference's sweep
loop needs and the cells it fills, on every designed plane.  tests/dataset_rules_driver.cpp includes that header and nothing else
of the library; it is compiled alone with -fsanitize=address,undefined, the runtimes linked statically (nothing is preloaded),
and run once as a subprocess that answers every question of this file.  cf_dataset_time_index itself — a pure host function of
the library — is asked the same questions."""
import ctypes as C
import math
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import dataset_case as case
import dataset_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "climaocean.jl_amd", "csrc")
DAY = 86400.0
MONTH_DAYS = [31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31]
MID_MONTHS = [DAY * (sum(MONTH_DAYS[:m]) + MONTH_DAYS[m] / 2.0) for m in range(12)]
YEAR = 365.0 * DAY


def hx(v):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", v))[0]


def hx32(v):
    return "%08x" % struct.unpack("<I", struct.pack("<f", v))[0]


def below(t):
    return math.nextafter(t, -math.inf)


def clock_cases():
    """[(times, period, time)] on good tables"""
    out = []
    three, uneven = [0.0, 1000.0, 2500.0], [-3.5, 0.1, 1.0 / 3.0, 7.0, 1e4]
    for times, period in ((three, 4000.0), (three, 2500.0000001), (uneven, 2e4), (MID_MONTHS, YEAR), (three, 0.0), (uneven, 0.0),
                          (MID_MONTHS, 0.0), ([12.5], 0.0), ([12.5], 3.0)):
        probes = []
        for t in times:                                 # exact level times, the last ulp before and the first after
            probes += [t, below(t), math.nextafter(t, math.inf)]
        probes += [times[0] + period, below(times[0] + period), times[-1] + 0.5 * (times[0] + period - times[-1])]   # the wrap segment
        probes += [-1.0, -1e-300, -0.0, 0.0, -12345.678, -1e9, 1e9, 1e9 + 1.0 / 3.0, 5e-324, 1e300, -1e300]
        probes += [times[0] - k * max(period, 1.0) for k in (1, 2, 1000)] + [times[-1] + k * max(period, 1.0) for k in (1, 7)]
        probes += [0.5 * (a + b) for a, b in zip(times, times[1:])]
        probes += [k * 700.0 for k in range(8)]
        out += [(times, period, t) for t in probes]
    # a year of 20-minute steps' worth of model times, thinned: December → January included
    out += [(MID_MONTHS, YEAR, 1200.0 * s) for s in range(0, 3 * 26280, 997)]
    out += [(three, 4000.0, -750.0), (MID_MONTHS, YEAR, YEAR - 1200.0), (MID_MONTHS, YEAR, 3.0 * YEAR - 1200.0)]
    return out


BAD_TABLES = [
    ([0.0, 1.0], 4.0, math.nan), ([0.0, 1.0], 4.0, math.inf), ([0.0, 1.0], 0.0, -math.inf),      # the time
    ([0.0, 0.0], 4.0, 0.5), ([1.0, 0.0], 4.0, 0.5), ([0.0, math.nan], 4.0, 0.5), ([0.0, math.inf], 0.0, 0.5),   # the table
    ([-math.inf, 0.0], 0.0, 0.5), ([math.nan], 0.0, 0.5),
    ([0.0, 1.0], 1.0, 0.5), ([0.0, 1.0], 0.5, 0.5), ([0.0, 1.0], -1.0, 0.5), ([0.0, 1.0], math.nan, 0.5), ([0.0, 1.0], math.inf, 0.5),   # the period
    ([], 0.0, 0.5),
]


def time_question(times, period, time):
    return f"time {len(times)} {hx(period)} {hx(time)} " + " ".join(hx(t) for t in times)


def plan_question(plane, periodic, max_sweeps):
    ny, nx = plane.shape
    return f"plan {nx} {ny} {int(periodic)} {max_sweeps} " + " ".join(hx32(v) for v in plane.ravel())


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    """{question line: the driver's answer line}, from one run of the sanitizer build"""
    compiler = shutil.which("g++") or shutil.which("clang++")
    if compiler is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("dataset_rules") / "dataset_rules_driver")
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(compiler) == "g++" else ["-static-libsan"]
    build = subprocess.run([compiler, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static, "-I", CSRC,
                            os.path.join(ROOT, "tests", "dataset_rules_driver.cpp"), "-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and re.search(r"cannot find.*(asan|ubsan|clang_rt)|libasan|libubsan|asan_preinit|static-lib", build.stderr):
        pytest.skip("the sanitizer runtime does not link here: " + build.stderr.strip().splitlines()[-1])
    assert build.returncode == 0, build.stderr
    questions = [time_question(*c) for c in clock_cases()] + [time_question(*c) for c in BAD_TABLES]
    questions += [plan_question(*c) for c in case.staging_cases().values()]
    questions = list(dict.fromkeys(questions))
    run = subprocess.run([exe], input="\n".join(questions) + "\n", capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    lines = run.stdout.splitlines()
    assert len(lines) == len(questions)
    return dict(zip(questions, lines))


def want_clock(times, period, time):
    l1, l2, f = ref.time_index(times, period, time)
    return f"{l1} {l2} {hx(f)}"


def test_the_clock_is_the_references_bit_for_bit(answers):
    cases = clock_cases()
    assert len(cases) > 400
    for times, period, time in cases:
        assert answers[time_question(times, period, time)] == want_clock(times, period, time), (times, period, time)


def test_the_clock_at_its_designed_points(answers):
    three = [0.0, 1000.0, 2500.0]
    ask = lambda times, period, t: answers[time_question(times, period, t)].split()   # noqa: E731
    assert ask(three, 4000.0, 1000.0) == ["1", "2", hx(0.0)]                      # an exact level time: fraction 0.0
    assert ask(three, 4000.0, below(1000.0))[:2] == ["0", "1"]                    # the last ulp before it: still the segment below
    assert ask(three, 4000.0, 2500.0) == ["2", "0", hx(0.0)]                      # the last level opens the wrap segment
    assert ask(three, 4000.0, 3250.0) == ["2", "0", hx(0.5)]
    assert ask(three, 4000.0, 4000.0) == ["0", "1", hx(0.0)]                      # one period on
    assert ask(three, 4000.0, -750.0) == ["2", "0", hx(0.5)]                      # negative times wrap backwards
    assert ask(three, 0.0, -1.0) == ["0", "0", hx(0.0)] and ask(three, 0.0, 2500.0) == ["2", "2", hx(0.0)]   # clamped ends
    assert ask(three, 0.0, 1e9) == ["2", "2", hx(0.0)]
    assert ask([12.5], 3.0, 1e9) == ["0", "0", hx(0.0)]                           # one level
    dec_jan = ask(MID_MONTHS, YEAR, YEAR - 1200.0)                                 # 31 December, 23:40
    assert dec_jan[:2] == ["11", "0"] and 0.49 < struct.unpack("<d", bytes.fromhex(dec_jan[2])[::-1])[0] < 0.5
    seven = [ask(three, 4000.0, 700.0 * s)[:2] for s in range(7)]
    assert seven == [["0", "1"], ["0", "1"], ["1", "2"], ["1", "2"], ["2", "0"], ["2", "0"], ["0", "1"]]


def test_every_refusal(answers):
    for times, period, time in BAD_TABLES:
        assert answers[time_question(times, period, time)] == "invalid", (times, period, time)
        assert not (ref.times_ok(times, period) and math.isfinite(time))


def test_the_librarys_entry_point_answers_the_same():
    from coflux import abi
    lib = abi.load_library()
    for times, period, time in clock_cases()[::3] + BAD_TABLES:
        a = np.array(times, dtype=np.float64)
        l1, l2, f = C.c_int32(-9), C.c_int32(-9), C.c_double(-9.0)
        rc = lib.cf_dataset_time_index(a.ctypes.data_as(abi.c_double_p) if a.size else None, int(a.size), period, time, C.byref(l1),
                                       C.byref(l2), C.byref(f))
        if ref.times_ok(times, period) and math.isfinite(time):
            assert rc == 0 and f"{l1.value} {l2.value} {hx(f.value)}" == want_clock(times, period, time), (times, period, time)
        else:
            assert rc == -1 and b"cf_dataset_time_index" in lib.cf_last_error(None), (times, period, time)
    assert lib.cf_dataset_time_index(None, 2, 0.0, 0.0, None, None, None) == -1


@pytest.mark.parametrize("name", list(case.staging_cases()))
def test_the_sweep_plan_is_what_the_sweep_loop_needs(answers, name):
    plane, periodic, max_sweeps = case.staging_cases()[name]
    depth, sweeps, filled, defaulted = (int(v) for v in answers[plan_question(plane, periodic, max_sweeps)].split())
    needed = ref.sweeps_needed(plane, periodic)
    assert depth == needed == ref.depth(plane, periodic), name
    _, want_sweeps, want_filled, want_defaulted = ref.inpaint(plane, periodic, max_sweeps, case.FILL_VALUE)
    assert (sweeps, filled, defaulted) == (want_sweeps, want_filled, want_defaulted), name
    assert filled + defaulted == int(np.isnan(plane).sum())


def test_the_designed_planes_have_their_features():
    s = case.small_plane().astype(np.float64)
    assert ref.depth(s, True) == 5 and ref.depth(s, False) == 5 and ref.depth(case.large_plane(), True) == 14
    assert ref.depth(case.full_plane(), True) == 0 and ref.depth(case.empty_plane(), True) == 0
    once_p, once_c = ref.sweep(s, True), ref.sweep(s, False)
    assert once_p[2, 4] == (((s[2, 3] + s[1, 4]) + s[2, 5]) + s[3, 4]) / 4.0          # the island: all four donors
    assert once_p[0, 4] == s[1, 4] and once_c[0, 4] == s[1, 4]                         # N alone
    assert once_p[0, 0] == ((s[0, 23] + s[0, 1]) + s[1, 0]) / 3.0 and once_c[0, 0] == (s[0, 1] + s[1, 0]) / 2.0   # a corner
    assert once_p[11, 3] == math.inf                                                    # an Inf among the donors
    full_p, full_c = ref.inpaint(s, True, -1, 0.0)[0], ref.inpaint(s, False, -1, 0.0)[0]
    assert full_p[6, 23] != full_c[6, 23] and not np.isnan(full_p).any() and not np.isnan(full_c).any()   # the seam matters
