"""A plain C consumer drives the library from include/coflux.h alone (tests/c_consumer.c: C99, no HIP header, device memory
through cf_device_alloc / cf_h2d / cf_d2h) — what every `ccall` of the Julia binding relies on.  The test compiles it with
-std=c99 -pedantic -Wall -Wextra -Werror, links it against the built libcoflux.so and runs it ONCE as a fresh child
process; the same calls are made through coflux.runtime (ctypes) in this process.  It is the same library, the same inputs
and the same launches, so every output array must be the same BITS, and the monitor's record must be the one
tests/monitor_reference.py states.

The case is the smallest that crosses every kind of argument (struct by pointer, int, int32_t, int64_t above 2³², size_t,
double, a returned pointer, a returned string, NULL for an optional struct): nx = 8, ny = 4, halos 2 × 2, ring 1, a 6 × 4
source with two levels at time fraction 0.37, a uint8 mask with two land cells; the synthetic fields of coflux.synthetic.

A second run with cf_monitor_desc.struct_size one word short must be refused with a message that names struct_size, and
must write nothing.

Two processes hold the GPU while the child runs.  The child's time limit is three times what it took on the MI355X:
MEASURED_SECONDS = 0.37 (the slowest of three runs, start to exit, HIP start-up included, while the parent held the GPU),
CHILD_LIMIT = 1.11 s; each run prints what it took.  A child that ends on the limit, or on anything but exit status 0 or
its own error exits (2, 3), stops the test there; nothing is retried."""
import os
import subprocess
import time

import numpy as np
import pytest
import torch

import abi_model as am
import monitor_reference as mr
from coflux import abi
from coflux import interface_computations as ic
from coflux import synthetic as syn
from coflux.runtime import EXCHANGE_NAMES, FLUX_NAMES, FLUX_OPTIONAL, NET_NAMES, FluxContext

pytestmark = pytest.mark.gpu

MEASURED_SECONDS = 0.37
CHILD_LIMIT = 3 * MEASURED_SECONDS

NX, NY, HX, HY, RING = 8, 4, 2, 2, 1
NSX, NSY, LEVELS = 6, 4, 2
TIME_FRACTION = 0.37
MONITOR_TIME = 1234.5
FIRST_CELL = (1 << 32) + 5
SHAPE = (NY + 2 * HY, NX + 2 * HX)
LAND = ((HY + 1, HX + 2), (HY + 3, HX + 6))            # two interior land cells (row, column of the halo-inclusive array)
OWN_ERROR_EXITS = (2, 3)                               # c_consumer.c: 2 a file, 3 the library refused a call


@pytest.fixture(scope="module")
def case():
    ocean = syn.ocean_state(NX, NY, HX, HY, land_fraction=False)
    mask = np.ones(SHAPE, np.uint8)
    for cell in LAND:
        mask[cell] = 0
    fi, fj, phi = syn.latlon_fractional_indices(NX, NY, HX, HY, nsx=NSX, nsy=NSY)
    return dict(ocean=dict(T=ocean["T"], S=ocean["S"], u=ocean["u"], v=ocean["v"], mask=mask),
                src=syn.jra55_snapshots(LEVELS, nsx=NSX, nsy=NSY), weights=dict(fi=fi, fj=fj, latitude=phi))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    compiler = am.c_compiler()
    assert compiler, "no host C compiler (cc, gcc, clang, nor a ROCm tree's clang)"
    lib_dir = os.path.dirname(abi.LIB_PATH)
    exe = str(tmp_path_factory.mktemp("c_consumer") / "c_consumer")
    build = subprocess.run([compiler] + am.C_FLAGS + ["-I", os.path.join(am.ROOT, "include"), os.path.join(am.ROOT, "tests", "c_consumer.c"),
                            "-o", exe, "-L" + lib_dir, "-lcoflux", "-Wl,-rpath," + lib_dir], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    return exe


@pytest.fixture(scope="module")
def inputs(case, tmp_path_factory):
    """the case as raw little-endian arrays, the way c_consumer.c names them"""
    d = tmp_path_factory.mktemp("c_consumer_inputs")
    for name in ("T", "S", "u", "v"):
        case["ocean"][name].astype("<f8").tofile(str(d / (name + ".f64")))
    case["ocean"]["mask"].astype("u1").tofile(str(d / "mask.u8"))
    for name in ("fi", "fj", "latitude"):
        case["weights"][name].astype("<f8").tofile(str(d / (name + ".f64")))
    for name in abi.JRA55_VARIABLES:
        assert case["src"][name].shape == (LEVELS, NSY, NSX)
        case["src"][name].astype("<f4").tofile(str(d / (name + ".f32")))
    return str(d)


def run_child(program, inputs, out_path, shortfall):
    """One fresh child under its limit.  Returns (exit status, stderr, seconds); a child that ends on the limit or on
    anything but 0 or its own error exits fails the test here."""
    assert CHILD_LIMIT > 0, "MEASURED_SECONDS has not been measured"
    start = time.perf_counter()
    try:
        done = subprocess.run([program, inputs, out_path, str(shortfall), str(FIRST_CELL)], capture_output=True, text=True,
                              timeout=CHILD_LIMIT)
    except subprocess.TimeoutExpired as late:
        pytest.fail("c_consumer did not end within %.1f s (three times the %.1f s measured): %s" % (CHILD_LIMIT, MEASURED_SECONDS, late.stderr))
    seconds = time.perf_counter() - start
    print("[c consumer] exit %d after %.2f s (limit %.1f s)" % (done.returncode, seconds, CHILD_LIMIT))
    if done.returncode != 0 and done.returncode not in OWN_ERROR_EXITS:
        pytest.fail("c_consumer ended with status %d, none of its own: %s" % (done.returncode, done.stderr))
    return done.returncode, done.stderr, seconds


def through_ctypes(case):
    """the same calls through coflux.runtime: {name: host array} of every output, and the monitor's record and time"""
    ctx = FluxContext(NX, NY, HX, HY, ic.flux_params(), ring=RING)
    try:
        ocean = {k: ctx.to_device(v) for k, v in case["ocean"].items()}
        src = {k: ctx.to_device(v) for k, v in case["src"].items()}
        weights = dict(separable=True, **{k: ctx.to_device(v) for k, v in case["weights"].items()})
        atmos, fluxes, net = ctx.field_set(EXCHANGE_NAMES), ctx.field_set(FLUX_NAMES, FLUX_OPTIONAL), ctx.field_set(NET_NAMES)
        fluxes["iterations"] = ctx.zeros(torch.int32)
        ctx.interpolate_atmosphere_state(src, weights, atmos, 0, 1, TIME_FRACTION)
        ctx.compute_atmosphere_ocean_fluxes(ocean, atmos, fluxes)
        ctx.compute_net_ocean_fluxes(ocean, atmos, fluxes, net, ice=None, weights=weights)
        monitor = ctx.monitor([(fluxes["latent_heat"], "value"), (net["T"], "abs")], mask=ocean["mask"], first_cell=FIRST_CELL, capacity=4)
        monitor.collect(MONITOR_TIME)
        values, times = monitor.read()
        monitor.close()
        ctx.sync()
        out = {"exchange." + k: atmos[k].cpu().numpy() for k in EXCHANGE_NAMES}
        out.update({"fluxes." + k: fluxes[k].cpu().numpy() for k in FLUX_NAMES + FLUX_OPTIONAL + ("iterations",)})
        out.update({"net." + k: net[k].cpu().numpy() for k in NET_NAMES})
        return out, values, times
    finally:
        ctx.close()


def read_outputs(path):
    """the output file of c_consumer.c: 8 exchange fields, 9 flux fields, iterations, 8 net fields, 2 values, 1 time"""
    raw = open(path, "rb").read()
    cells, out, at = SHAPE[0] * SHAPE[1], {}, 0
    layout = [("exchange." + k, "<f8") for k in EXCHANGE_NAMES] + [("fluxes." + k, "<f8") for k in FLUX_NAMES + FLUX_OPTIONAL]
    layout += [("fluxes.iterations", "<i4")] + [("net." + k, "<f8") for k in NET_NAMES]
    for name, dtype in layout:
        out[name] = np.frombuffer(raw, dtype, cells, at).reshape(SHAPE)
        at += cells * np.dtype(dtype).itemsize
    values = np.frombuffer(raw, mr.DTYPE, 2, at)
    times = np.frombuffer(raw, "<f8", 1, at + 2 * mr.DTYPE.itemsize)
    assert at + 2 * mr.DTYPE.itemsize + 8 == len(raw), (at, len(raw))
    return out, values, times


def test_c_consumer_gives_the_bits_of_the_ctypes_path_and_the_reference_record(case, program, inputs, tmp_path):
    out_path = str(tmp_path / "outputs.bin")
    status, stderr, seconds = run_child(program, inputs, out_path, 0)
    assert status == 0, stderr
    got, values, times = read_outputs(out_path)
    want, want_values, want_times = through_ctypes(case)
    assert sorted(got) == sorted(want) and len(got) == 26
    interior = (slice(HY, HY + NY), slice(HX, HX + NX))
    wet = case["ocean"]["mask"][interior]
    assert int((wet == 0).sum()) == 2
    for name in sorted(want):
        assert got[name].dtype == want[name].dtype and got[name].tobytes() == want[name].tobytes(), name
    # the comparison is not of zeros with zeros: the solver ran on the wet cells and left the land cells at zero
    latent, iterations = want["fluxes.latent_heat"][interior], want["fluxes.iterations"][interior]
    assert np.all(iterations[wet == 1] >= 1) and np.all(iterations[wet == 0] == 0)
    assert np.all(np.isfinite(latent)) and np.all(latent[wet == 1] != 0.0) and np.all(latent[wet == 0] == 0.0)
    assert np.all(want["net.T"][interior][wet == 1] != 0.0) and np.all(want["exchange.T"][interior] > 200.0)
    # the record: against the NumPy restatement on the arrays themselves, and against the ctypes path's
    record = np.array([mr.monitor_value(latent, wet, "value", FIRST_CELL), mr.monitor_value(want["net.T"][interior], wet, "abs", FIRST_CELL)],
                      dtype=mr.DTYPE)
    assert mr.same(values, record), (values, record)
    assert mr.same(want_values[0], record), (want_values, record)
    assert np.all(values["argmin"] > 1 << 32) and np.all(values["argmax"] > 1 << 32)
    assert list(times) == [MONITOR_TIME] == list(want_times)
    assert seconds < CHILD_LIMIT


def test_c_consumer_with_a_short_struct_size_is_refused_and_writes_nothing(program, inputs, tmp_path):
    out_dir = tmp_path / "refused"
    out_dir.mkdir()
    status, stderr, _seconds = run_child(program, inputs, str(out_dir / "outputs.bin"), 4)
    assert status == 3, (status, stderr)
    assert "cf_monitor_create" in stderr and "struct_size" in stderr, stderr
    assert str(abi.C.sizeof(abi.MonitorDesc) - 4) in stderr and str(abi.C.sizeof(abi.MonitorDesc)) in stderr, stderr
    assert os.listdir(str(out_dir)) == []
