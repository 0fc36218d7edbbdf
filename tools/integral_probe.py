"""Cost of the surface integrals on the 1/4-degree surface (1440 x 560, halo 7) -> profiles/integral_probe.json.

    python tools/integral_probe.py [--trace] [--out PATH]

The driver starts each GPU step as a child under its own `timeout`; nothing follows a step that failed.  Steps:
  measure   one process, warm-up first, the variants it compares alternating:
            * cf_integrals_collect of the sea-ice preset (6 entries: 2 fields, area, uint8 mask, uint8 region = 26 B/cell) and
              of a 32-entry case (4 fields), HIP events over >= 1000 back-to-back launches, bytes / time;
            * cf_time_copy of the same footprint in the same process;
            * the same six quantities as torch reductions on the device fields, one per entry — what a caller had before;
            * ms_per_step of cf_time_steps (the bench's pipelined schedule) without and with an attached integrator
              (stride 1), four alternating pairs.
  trace     (--trace) the same child, fewer launches, under `rocprofv3 --kernel-trace --memory-copy-trace --stats`: the kernels
            by name, and the copies it saw."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "climaocean.jl_amd"))

NX, NY, H = 1440, 560, 7
ROUNDS = 4


def measure(launches, steps_per_arm):
    import numpy as np
    import torch
    from coflux import abi, models as cm, synthetic as syn, interface_computations as ic
    from coflux.runtime import EXCHANGE_NAMES, FLUX_NAMES, NET_NAMES, FluxContext

    def events_ms(fn, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / n

    ctx = FluxContext(NX, NY, H, H, ic.flux_params(), ring=1)
    cells = NX * NY
    grid = cm.LatitudeLongitudeGrid(size=(NX, NY, 10), halo=(H, H, H))
    state, ice = syn.ocean_state(NX, NY, H, H), syn.sea_ice_state(NX, NY, H, H)
    area, region = ctx.to_device(grid.cell_areas()), ctx.to_device(cm.hemisphere_regions(grid))
    mask = ctx.to_device(state["mask"])
    h, c = ctx.to_device(ice["thickness"]), ctx.to_device(state["ice_concentration"])
    gen = torch.Generator(device=ctx.device).manual_seed(0)
    extra = [torch.randn(ctx.shape, dtype=torch.float64, device=ctx.device, generator=gen) for _ in range(2)]
    preset = [(k, a, b, t, bit) for bit in (1, 2) for k, a, b, t in (("product", h, c, 0.0), ("field", c, None, 0.0), ("above", c, None, 0.15))]
    pool = preset + [("one", None, None, 0.0, 0), ("field", extra[0], None, 0.0, 0), ("product", extra[0], extra[1], 0.0, 1),
                     ("product", extra[1], extra[1], 0.0, 2), ("above", extra[0], None, 0.5, 0)]
    wide = [pool[k % len(pool)] for k in range(32)]
    capacity = 3 * launches + 64
    q6 = ctx.integrals(preset, area=area, mask=mask, region=region, capacity=capacity)
    q32 = ctx.integrals(wide, area=area, mask=mask, region=region, capacity=capacity)
    bytes6, bytes32 = cells * (8 * 2 + 8 + 1 + 1), cells * (8 * 4 + 8 + 1 + 1)

    inner = (slice(H, H + NY), slice(H, H + NX))
    sel = {bit: ((mask != 0) & ((region & (1 << bit)) != 0))[inner] for bit in (1, 2)}
    hi, ci, ai = h[inner], c[inner], area[inner]

    def torch_form():
        out = []
        for bit in (1, 2):
            out.append((hi * ci * ai)[sel[bit]].sum())
            out.append((ci * ai)[sel[bit]].sum())
            out.append(((ci > 0.15) * ai)[sel[bit]].sum())
        return out

    for _ in range(50):
        q6.collect()
        q32.collect()
        torch_form()
    t6, t32, ttorch, tcopy = [], [], [], []
    for _ in range(3):     # alternating
        q6.reset()
        q32.reset()
        t6.append(events_ms(q6.collect, launches))
        tcopy.append(ctx.time_copy(bytes6 // 2, launches))
        t32.append(events_ms(q32.collect, launches))
        ttorch.append(events_ms(torch_form, max(launches // 10, 20)))
    got = q6.read(0, 1)[0][0]
    want = [float(x) for x in torch_form()]
    agreement = max(abs(g - w) / max(abs(w), 1e-300) for g, w in zip(got, want))
    rate = lambda nbytes, ms: nbytes / (ms * 1e-3) / 1e12  # noqa: E731  TB/s
    q6.close()
    q32.close()

    # the stepping loop: bench.py's schedule (two ocean states, two exchange sets, CF_PIPELINE_CONTINUING, tail form)
    o1 = syn.evolved_ocean_state(state, NX, NY, H, H, 1)
    states = [{k: ctx.to_device(o[k]) for k in ("T", "S", "u", "v", "mask")} for o in (state, o1)]
    states[1]["mask"] = states[0]["mask"]
    src = {k: ctx.to_device(v) for k, v in syn.jra55_snapshots(4).items()}
    fi, fj, phi = syn.latlon_fractional_indices(NX, NY, H, H)
    w = dict(separable=True, fi=ctx.to_device(fi), fj=ctx.to_device(fj), latitude=ctx.to_device(phi))
    sets = [ctx.field_set(EXCHANGE_NAMES) for _ in range(2)]
    fl, net = ctx.field_set(FLUX_NAMES), ctx.field_set(NET_NAMES)
    ctx.set_option(abi.OPT_MERGED_PREFETCH, 2)
    sched = ctx.make_schedule(states, sets, first_level=0, time_fraction=0.0, time_fraction_increment=1.0 / 9.0,
                              pipeline=abi.PIPELINE_CONTINUING)
    means = [("one", None, None, 0.0, 0)] + [("field", f, None, 0.0, 0) for f in (net["T"], net["S"], fl["sensible_heat"], fl["latent_heat"],
                                                                                   states[0]["T"], states[0]["S"])]
    step_q = ctx.integrals(means, area=area, mask=states[0]["mask"], region=region, capacity=steps_per_arm)
    step = [0]

    def steps(n):
        ctx.time_steps(step[0], n, sched, src, w, fl, net)
        step[0] += n

    steps(steps_per_arm)   # warm-up: chunk table, code load, clocks
    arms = {"without": [], "with": []}
    for _ in range(ROUNDS):
        for arm in ("without", "with"):
            step_q.reset()
            ctx.attach_integrals(step_q if arm == "with" else None, 1, 0.0, 1200.0)
            arms[arm].append(events_ms(lambda: steps(steps_per_arm), 1) / steps_per_arm)
    ctx.attach_integrals(None)
    ctx.sync()
    collected = step_q.count()
    series = step_q.read()[0]
    result = dict(
        grid=[NX, NY, H], launches=launches,
        collect6_us=round(1e3 * min(t6), 2), collect6_bytes=bytes6, collect6_tbps=round(rate(bytes6, min(t6)), 3),
        collect32_us=round(1e3 * min(t32), 2), collect32_bytes=bytes32, collect32_tbps=round(rate(bytes32, min(t32)), 3),
        copy_same_bytes_us=round(1e3 * min(tcopy), 2), collect6_over_copy=round(min(t6) / min(tcopy), 3),
        torch_six_reductions_us=round(1e3 * min(ttorch), 2), torch_over_collect6=round(min(ttorch) / min(t6), 2),
        collect6_us_all=[round(1e3 * x, 2) for x in t6], torch_us_all=[round(1e3 * x, 2) for x in ttorch],
        collect6_vs_torch_relative_difference=agreement,
        steps_per_arm=steps_per_arm, step_entries=len(means), ms_per_step_without=[round(x, 5) for x in arms["without"]],
        ms_per_step_with=[round(x, 5) for x in arms["with"]],
        overhead_us=round(1e3 * (min(arms["with"]) - min(arms["without"])), 2),
        overhead_us_pairs=[round(1e3 * (a - b), 2) for a, b in zip(arms["with"], arms["without"])],
        collected_steps=collected, series_finite=bool(np.isfinite(series).all()))
    step_q.close()
    ctx.close()
    print("INTEGRAL_PROBE " + json.dumps(result))


def child(args, limit, prefix=()):
    cmd = ["timeout", "-k", "10", str(limit), *prefix, sys.executable, os.path.abspath(__file__), *args]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=ROOT)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-4000:])
        raise SystemExit(f"integral_probe: step {' '.join(args)} ended with status {p.returncode}; nothing further is run")
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("INTEGRAL_PROBE ")]
    return json.loads(lines[-1][len("INTEGRAL_PROBE "):])


def trace():
    with tempfile.TemporaryDirectory() as d:
        child(["--measure", "--launches", "100", "--steps", "50"], 420,
              prefix=("rocprofv3", "--kernel-trace", "--memory-copy-trace", "--stats", "--output-format", "csv", "-d", d, "--"))
        kernels, copies = {}, 0
        for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                name = row.get("Name") or row.get("KernelName") or ""
                if "integrals" in name or "lean" in name or "copy" in name.lower():
                    kernels[name.replace("(anonymous namespace)::", "").split("(")[0][:96]] = dict(calls=int(float(row.get("Calls", 0))),
                                                            average_us=round(float(row.get("AverageNs", row.get("Average", 0))) / 1e3, 2))
        for f in glob.glob(os.path.join(d, "**", "*memory_copy_trace.csv"), recursive=True):
            copies += sum(1 for _ in csv.DictReader(open(f)))
        return dict(kernels=kernels, memory_copies_in_the_whole_run=copies)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--measure", action="store_true")
    ap.add_argument("--launches", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "integral_probe.json"))
    a = ap.parse_args()
    if a.measure:
        return measure(a.launches, a.steps)
    result = child(["--measure", "--launches", str(a.launches), "--steps", str(a.steps)], 420)
    if a.trace:
        result["trace"] = trace()
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
