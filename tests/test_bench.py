"""bench.py's plain run and --dump-outputs: exactly --steps timed steps in one region, nothing of --full's, and the fields the
last timed step returned written as float64 .npy files that hold the CPU oracle's result for that step and are the same bits
from run to run (the inputs of every timed step depend on the arguments alone)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle as orc
import util
from coflux import interface_computations as ic
from coflux import synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NX, NY, H = 360, 120, 7


def _bench(*args, timeout=600):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def _oracle_step(step):
    """bench.py's synthetic 1-GPU lat-lon workload (:default) at one step: the clock and the ocean state of that step"""
    params = ic.flux_params(ic.SimilarityTheoryFluxes(), ocean_surface=ic.SurfaceRadiationProperties(0.06, 1.0))
    src = syn.jra55_snapshots(4, temporal_correlation=0.95)
    first = syn.ocean_state(NX, NY, H, H, ny_global=NY, j_offset=0)
    ocean = first if step % 2 == 0 else syn.evolved_ocean_state(first, NX, NY, H, H, 1, ny_global=NY, j_offset=0)
    fi, fj, phi = syn.latlon_fractional_indices(NX, NY, H, H, ny_global=NY, j_offset=0)
    w = dict(separable=True, fi=fi, fj=fj, latitude=phi)
    total = 0.0 + float(step) * (1200.0 / 10800.0)
    whole = int(np.floor(total))
    g = orc.make_grid(NX, NY, H, H, 1)
    atm = orc.interpolate_atmosphere_state(g, src, w, whole % 4, (whole + 1) % 4, total - whole)
    fl = orc.compute_atmosphere_ocean_fluxes(g, params, ocean, atm, nthreads=min(32, orc.max_threads()), scales=False)
    net = orc.compute_net_ocean_fluxes(g, params, ocean, atm, fl, weights=w)
    return dict(fluxes=fl, net=net)


def test_dump_outputs_is_refused_outside_the_throughput_run():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--days", "1", "--dump-outputs", "unused"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--dump-outputs" in r.stderr
    assert not os.path.exists("unused")


@pytest.mark.gpu
def test_plain_run_times_exactly_the_steps_and_dumps_the_last_step(tmp_path):
    size = ["--nx", str(NX), "--ny", str(NY), "--halo", str(H)]
    lines = [_bench("--gpus", "1", "--steps", "30", "--warmup", "5", *size, "--dump-outputs", str(tmp_path / d)) for d in ("a", "b")]
    for line in lines:
        assert line["steps"] == 30 and line["warmup"] == 5 and line["repetitions"] == 1 and len(line["ms_per_step_samples"]) == 1
        assert line["ms_per_step"] > 0 and line["value"] == pytest.approx(NX * NY / (line["ms_per_step"] * 1e-3))
        assert line["unit"] == "cells/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
        assert line["config"]["solver_path"] == "exact" and set(line["solver_paths_ms_per_step"]) == {"exact"}
        for key in ("roofline", "stages_ms", "cpu_baseline", "device_copy_GBs", "parity_measured"):
            assert key not in line, key
        assert line["dumped_outputs"]["step"] == 5 + 30 - 1 and line["dumped_outputs"]["rows"] == "all interior rows"
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(f + ".npy" for f in lines[0]["dumped_outputs"]["fields"]) and len(names) == 11
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= 64 * 10 ** 6
    ref = _oracle_step(lines[0]["dumped_outputs"]["step"])
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype == np.float64 and a.shape == (NY, NX)
        assert np.array_equal(a, b), n                               # same arguments, same bits
        group, field = n[:-4].split(".")
        want = ref[group][field][H:H + NY, H:H + NX]
        err = np.max(np.abs(a - want) / np.maximum(np.abs(want), util.FIELD_SCALE[field]))
        assert err <= 1e-9, (n, err)


@pytest.mark.gpu
def test_full_run_keeps_the_measurements_beyond_the_headline():
    line = _bench("--gpus", "1", "--steps", "20", "--warmup", "5", "--nx", str(NX), "--ny", str(NY), "--full", "--cpu-seconds", "1")
    assert line["steps"] == 20 and 3 <= line["repetitions"] <= 9 and len(line["ms_per_step_samples"]) == line["repetitions"]
    assert line["config"]["solver_path"] == "exact" and "exact" in line["solver_paths_ms_per_step"]
    assert line["roofline"]["avg_launch_ms"] > 0 and line["stages_ms"]["ao_fluxes_standalone"] > 0
    assert line["cpu_baseline"]["value"] > 0 and line["parity_measured"]["max"] <= 1e-9
