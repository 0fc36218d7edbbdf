"""Cost of the surface monitor on the 1/4-degree surface (1440 x 560, halo 7) -> profiles/monitor_probe.json.

    python tools/monitor_probe.py [--out PATH]

The driver starts the GPU step as a child under its own `timeout`; nothing follows a step that failed.  The step:
  measure   one process, warm-up first, the arms it compares alternating:
            * cf_monitor_collect of the progress preset (6 entries: h, ℵ, T, S, u, v; 8 B of field + 1 B of mask per cell and
              entry = 54 B/cell) and of a 16-entry case, HIP events over >= 1000 back-to-back launches, bytes / time;
            * cf_time_copy of the same footprint in the same process;
            * the same quantities as torch reductions on the same fields — amin, amax and an isnan / isinf count per field,
              read back — what a caller has today (it has no hash and no index);
            * ms_per_step of cf_time_steps (the bench's pipelined schedule) without and with an attached monitor (stride 1),
              four alternating pairs.
The one bar: the collection's median is below the torch arm's median by more than the spread (max − min) of the torch
arm's own repeats; `bar_met` says whether it was."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "climaocean.jl_amd"))

NX, NY, H = 1440, 560, 7
ROUNDS = 4
REPEATS = 5


def measure(launches, steps_per_arm):
    import torch
    from coflux import abi, synthetic as syn, interface_computations as ic
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
    state, ice = syn.ocean_state(NX, NY, H, H), syn.sea_ice_state(NX, NY, H, H)
    mask = ctx.to_device(state["mask"])
    fields = [ctx.to_device(ice["thickness"]), ctx.to_device(state["ice_concentration"])] + [ctx.to_device(state[k]) for k in ("T", "S", "u", "v")]
    gen = torch.Generator(device=ctx.device).manual_seed(0)
    extra = [torch.randn(ctx.shape, dtype=torch.float64, device=ctx.device, generator=gen) for _ in range(10)]
    wide = [(f, ("value", "abs")[k % 2]) for k, f in enumerate(fields + extra)]
    capacity = REPEATS * launches + 64
    m6 = ctx.monitor(fields, mask=mask, capacity=capacity)
    m16 = ctx.monitor(wide, mask=mask, capacity=capacity)
    bytes6, bytes16 = cells * 6 * (8 + 1), cells * 16 * (8 + 1)

    inner = (slice(H, H + NY), slice(H, H + NX))
    wet = (mask != 0)[inner]
    views = [f[inner] for f in fields]
    inf = torch.tensor(float("inf"), dtype=torch.float64, device=ctx.device)

    def torch_form():
        out = []
        for x in views:
            out.append(torch.where(wet, x, inf).amin())
            out.append(torch.where(wet, x, -inf).amax())
            out.append((torch.isnan(x) & wet).sum())
            out.append((torch.isinf(x) & wet).sum())
        return [float(v) for v in torch.stack([o.to(torch.float64) for o in out]).cpu()]     # read back: one synchronisation

    for _ in range(50):
        m6.collect()
        m16.collect()
    for _ in range(5):
        torch_form()
    t6, t16, ttorch, tcopy = [], [], [], []
    for _ in range(REPEATS):     # alternating
        m6.reset()
        m16.reset()
        t6.append(events_ms(m6.collect, launches))
        tcopy.append(ctx.time_copy(bytes6 // 2, launches))
        t16.append(events_ms(m16.collect, launches))
        ttorch.append(events_ms(torch_form, max(launches // 10, 20)))
    got = m6.read(0, 1)[0][0]
    want = torch_form()
    agree = all(float(g["minimum"]) == want[4 * k] and float(g["maximum"]) == want[4 * k + 1] and g["nan_count"] == want[4 * k + 2]
                and g["inf_count"] == want[4 * k + 3] for k, g in enumerate(got))
    rate = lambda nbytes, ms: nbytes / (ms * 1e-3) / 1e12  # noqa: E731  TB/s
    m6.close()
    m16.close()

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
    watched = [net["T"], net["S"], net["u"], net["v"], states[0]["T"], states[0]["S"]]
    step_m = ctx.monitor(watched, mask=states[0]["mask"], capacity=steps_per_arm)
    step = [0]

    def steps(n):
        ctx.time_steps(step[0], n, sched, src, w, fl, net)
        step[0] += n

    steps(steps_per_arm)   # warm-up: chunk table, code load, clocks
    arms = {"without": [], "with": []}
    for _ in range(ROUNDS):
        for arm in ("without", "with"):
            step_m.reset()
            ctx.attach_monitor(step_m if arm == "with" else None, 1, 0.0, 1200.0)
            arms[arm].append(events_ms(lambda: steps(steps_per_arm), 1) / steps_per_arm)
    ctx.attach_monitor(None)
    ctx.sync()
    collected, status = step_m.count(), step_m.status()
    med = statistics.median
    spread = max(ttorch) - min(ttorch)
    result = dict(
        grid=[NX, NY, H], launches=launches, repeats=REPEATS,
        collect6_us=round(1e3 * med(t6), 2), collect6_bytes=bytes6, collect6_tbps=round(rate(bytes6, med(t6)), 3),
        collect16_us=round(1e3 * med(t16), 2), collect16_bytes=bytes16, collect16_tbps=round(rate(bytes16, med(t16)), 3),
        copy_same_bytes_us=round(1e3 * med(tcopy), 2), collect6_over_copy=round(med(t6) / med(tcopy), 3),
        torch_reductions_us=round(1e3 * med(ttorch), 2), torch_spread_us=round(1e3 * spread, 2),
        torch_over_collect6=round(med(ttorch) / med(t6), 2), bar_met=bool(med(ttorch) - med(t6) > spread),
        collect6_us_all=[round(1e3 * x, 2) for x in t6], collect16_us_all=[round(1e3 * x, 2) for x in t16],
        torch_us_all=[round(1e3 * x, 2) for x in ttorch], copy_us_all=[round(1e3 * x, 2) for x in tcopy],
        collect6_equals_torch=bool(agree),
        steps_per_arm=steps_per_arm, step_entries=len(watched), ms_per_step_without=[round(x, 5) for x in arms["without"]],
        ms_per_step_with=[round(x, 5) for x in arms["with"]],
        overhead_us=round(1e3 * (med(arms["with"]) - med(arms["without"])), 2),
        overhead_us_pairs=[round(1e3 * (a - b), 2) for a, b in zip(arms["with"], arms["without"])],
        collected_steps=collected, status_after_the_steps=list(status))
    step_m.close()
    ctx.close()
    print("MONITOR_PROBE " + json.dumps(result))


def child(args, limit):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), *args]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=ROOT)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-4000:])
        raise SystemExit(f"monitor_probe: step {' '.join(args)} ended with status {p.returncode}; nothing further is run")
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("MONITOR_PROBE ")]
    return json.loads(lines[-1][len("MONITOR_PROBE "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--measure", action="store_true")
    ap.add_argument("--launches", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "monitor_probe.json"))
    a = ap.parse_args()
    if a.measure:
        return measure(a.launches, a.steps)
    result = child(["--measure", "--launches", str(a.launches), "--steps", str(a.steps)], 420)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
