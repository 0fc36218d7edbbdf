"""Cost of staging a dataset on the device (cf_dataset_stage) -> profiles/dataset_probe.json.

    python tools/dataset_probe.py [--out PATH]

The driver starts the GPU step as a child under its own `timeout`; nothing follows a step that failed.  The step: one process,
warm-up first, the arms interleaved, medians of ROUNDS rounds.  Per source grid (360 x 180 and 1440 x 720, twelve levels on a
designed continent across the x seam, a second one inland and islands) and per ocean grid it is staged onto:
  (a) cf_dataset_stage of the twelve levels with sweeps_per_launch = 1 (one launch per sweep), 2, 4 and 8 (LDS tiles) and 0 (the
      library's choice): wall time from the first call to the end of a synchronisation — the host's breadth-first pass, the
      upload, every launch — and the sweeps queued per level;
  (b) a torch stand-in of the same definition that finds out when to stop the reference's way — isnan(sum(plane)) read back on
      the host before every sweep — followed by the library's own regridding: what a caller of the library had before.
`ratio` is (b) / (a) at the library's choice.  Nothing here is a threshold."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "climaocean.jl_amd"))

ROUNDS = 5
N_LEVELS = 12
FORMS = (0, 1, 2, 4, 8)
SOURCES = {"360x180": (360, 180, (360, 140, 5)), "1440x720": (1440, 720, (1440, 560, 7))}


def designed_planes(ns_x, ns_y):
    import numpy as np
    i, j = np.meshgrid(np.arange(ns_x, dtype=np.float64), np.arange(ns_y, dtype=np.float64))
    s = ns_x / 360.0
    land = np.zeros((ns_y, ns_x), dtype=bool)
    land[int(40 * s):int(140 * s), int(300 * s):] = True      # a continent across the seam: 120 x 100 degrees
    land[int(40 * s):int(140 * s), :int(60 * s)] = True
    land[int(20 * s):int(95 * s), int(150 * s):int(215 * s)] = True
    land[:int(12 * s), :] = True                               # a polar cap
    land[(i.astype(int) * 7 + j.astype(int) * 13) % 97 == 0] = True   # islands
    planes = []
    for level in range(N_LEVELS):
        p = (34.0 + 2.0 * np.sin(0.05 * i / s + 0.3 * level) + 0.01 * j / s).astype(np.float32)
        p[land] = np.nan
        planes.append(p)
    return planes


def torch_inpaint(p, periodic):
    """The same definition in torch, stopped the reference's way: a host read of isnan(sum(p)) before every sweep."""
    import torch
    sweeps = 0
    nan_row = torch.full_like(p[:1], float("nan"))
    while bool(torch.isnan(p.sum())) and sweeps < 100000:
        w, e = torch.roll(p, 1, 1), torch.roll(p, -1, 1)
        if not periodic:
            w[:, 0], e[:, -1] = float("nan"), float("nan")
        s, n = torch.cat((nan_row, p[:-1]), 0), torch.cat((p[1:], nan_row), 0)
        total, count = torch.zeros_like(p), torch.zeros_like(p)
        for d in (w, s, e, n):
            ok = ~torch.isnan(d)
            total = total + torch.where(ok, d, torch.zeros_like(d))
            count = count + ok
        q = torch.where(torch.isnan(p) & (count > 0), total / count, p)
        if bool((torch.isnan(q) == torch.isnan(p)).all()):
            break
        p, sweeps = q, sweeps + 1
    return p, sweeps


def measure():
    import numpy as np
    import torch
    from coflux import interface_computations as ic
    from coflux import synthetic
    from coflux.runtime import FluxContext

    med = statistics.median
    result = dict(levels=N_LEVELS, rounds=ROUNDS, sources={})
    for name, (ns_x, ns_y, (nx, ny, h)) in SOURCES.items():
        ctx = FluxContext(nx, ny, h, h, ic.flux_params(), ring=1)
        planes = designed_planes(ns_x, ns_y)
        fi, fj, _phi = synthetic.latlon_fractional_indices(nx, ny, h, h, latitude=(-75.0, 65.0), nsx=ns_x, nsy=ns_y)
        w = dict(separable=True, fi=ctx.to_device(fi), fj=ctx.to_device(fj))
        times = [float(k) for k in range(N_LEVELS)]
        datasets = {f: ctx.dataset(ns_x, ns_y, times, w, period=float(N_LEVELS), sweeps_per_launch=f) for f in FORMS}
        stand_in = ctx.dataset(ns_x, ns_y, times, w, period=float(N_LEVELS), max_sweeps=0)

        def stage_all(d):
            ctx.sync()
            t0 = time.perf_counter()
            for level, p in enumerate(planes):
                d.stage(level, p)
            ctx.sync()
            return 1e3 * (time.perf_counter() - t0)

        def stand_in_all():
            ctx.sync()
            t0 = time.perf_counter()
            sweeps = 0
            for level, p in enumerate(planes):
                filled, sweeps = torch_inpaint(torch.from_numpy(p).to(ctx.device).to(torch.float64), True)
                stand_in.stage(level, filled.to(torch.float32).cpu().numpy())   # (regridding by the library: no NaN is left, no sweep runs)
            ctx.sync()
            return 1e3 * (time.perf_counter() - t0), sweeps

        for d in datasets.values():
            stage_all(d)
        stand_in_all()
        ms = {f: [] for f in FORMS}
        ms_torch, torch_sweeps = [], 0
        for _ in range(ROUNDS):   # interleaved
            for f in FORMS:
                ms[f].append(stage_all(datasets[f]))
            t, torch_sweeps = stand_in_all()
            ms_torch.append(t)
        # the forms agree bit for bit on the last level staged
        planes_read = {f: d.read_source().view(np.int64) for f, d in datasets.items()}
        same = all(np.array_equal(planes_read[f], planes_read[1]) for f in FORMS)
        entry = dict(ns_x=ns_x, ns_y=ns_y, ocean_grid=[nx, ny, h], sweeps_per_level=datasets[0].stage_info(0)[0], torch_sweeps=torch_sweeps,
                     forms_agree=bool(same),
                     forms={str(f): dict(ms=round(med(v), 3), spread_ms=round(max(v) - min(v), 3), ms_all=[round(x, 3) for x in v]) for f, v in ms.items()},
                     torch_stand_in=dict(ms=round(med(ms_torch), 3), spread_ms=round(max(ms_torch) - min(ms_torch), 3),
                                         ms_all=[round(x, 3) for x in ms_torch]),
                     ratio=round(med(ms_torch) / med(ms[0]), 2))
        result["sources"][name] = entry
        for d in list(datasets.values()) + [stand_in]:
            d.close()
        ctx.close()
        torch.cuda.empty_cache()
    print("DATASET_PROBE " + json.dumps(result))


def child(args, limit):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), *args]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=ROOT)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-4000:])
        raise SystemExit(f"dataset_probe: step {' '.join(args)} ended with status {p.returncode}; nothing further is run")
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("DATASET_PROBE ")]
    return json.loads(lines[-1][len("DATASET_PROBE "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--measure", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dataset_probe.json"))
    a = ap.parse_args()
    if a.measure:
        return measure()
    result = child(["--measure"], 400)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
