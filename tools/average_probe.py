"""Cost of the time averages on the 1/4-degree surface (1440 x 560, halo 7): one JSON line with
  * cf_average_collect for K = 6 fields, HIP events over >= 200 back-to-back launches after warm-up (accumulating and storing
    collections), algorithmic bytes (cells x K x 24 B; 16 B for a storing one) and the achieved rate;
  * cf_time_copy in the same process: a copy that moves the same bytes as an accumulating collection, and 256 MiB;
  * ms_per_step of cf_time_steps (the bench's pipelined schedule) without and with an attached averager (stride 1), the two
    arms alternating ROUNDS times."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "climaocean.jl_amd"))
import torch  # noqa: E402

from coflux import abi, synthetic as syn, interface_computations as ic  # noqa: E402
from coflux.runtime import EXCHANGE_NAMES, FLUX_NAMES, NET_NAMES, FluxContext  # noqa: E402

NX, NY, H, K = 1440, 560, 7, 6
LAUNCHES, STEPS, ROUNDS = 400, 200, 4


def events_ms(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def main():
    ctx = FluxContext(NX, NY, H, H, ic.flux_params(), ring=1)
    cells = NX * NY
    gen = torch.Generator(device=ctx.device).manual_seed(0)
    sources = [torch.randn(ctx.shape, dtype=torch.float64, device=ctx.device, generator=gen) for _ in range(K)]
    means = [ctx.zeros() for _ in range(K)]
    avg = ctx.average(sources, means)
    for _ in range(50):
        avg.collect(1.0)
    collect_ms = min(events_ms(lambda: avg.collect(1.0), LAUNCHES) for _ in range(3))

    def store():
        avg.reset()
        avg.collect(1.0)
    store_ms = min(events_ms(store, LAUNCHES) for _ in range(3))
    accumulate_bytes, store_bytes = cells * K * 24, cells * K * 16
    copy_ms = min(ctx.time_copy(accumulate_bytes // 2, LAUNCHES) for _ in range(3))
    copy256_ms = min(ctx.time_copy(256 << 20, 200) for _ in range(3))
    rate = lambda nbytes, ms: nbytes / (ms * 1e-3) / 1e12  # noqa: E731  TB/s
    avg.close()
    del sources, means

    # the stepping loop: bench.py's schedule (two ocean states, two exchange sets, CF_PIPELINE_CONTINUING, tail form)
    o0 = syn.ocean_state(NX, NY, H, H)
    o1 = syn.evolved_ocean_state(o0, NX, NY, H, H, 1)
    states = [{k: ctx.to_device(o[k]) for k in ("T", "S", "u", "v", "mask")} for o in (o0, o1)]
    states[1]["mask"] = states[0]["mask"]
    src = {k: ctx.to_device(v) for k, v in syn.jra55_snapshots(4).items()}
    fi, fj, phi = syn.latlon_fractional_indices(NX, NY, H, H)
    w = dict(separable=True, fi=ctx.to_device(fi), fj=ctx.to_device(fj), latitude=ctx.to_device(phi))
    sets = [ctx.field_set(EXCHANGE_NAMES) for _ in range(2)]
    fl, net = ctx.field_set(FLUX_NAMES), ctx.field_set(NET_NAMES)
    ctx.set_option(abi.OPT_MERGED_PREFETCH, 2)
    sched = ctx.make_schedule(states, sets, first_level=0, time_fraction=0.0, time_fraction_increment=1.0 / 9.0,
                              pipeline=abi.PIPELINE_CONTINUING)
    outs = [net[k] for k in ("u", "v", "T", "S")] + [fl["sensible_heat"], fl["latent_heat"]]
    step_avg = ctx.average(outs, [ctx.zeros() for _ in outs])
    step = [0]

    def steps(n):
        ctx.time_steps(step[0], n, sched, src, w, fl, net)
        step[0] += n

    steps(STEPS)   # warm-up: chunk table, code load, clocks
    arms = {"without": [], "with": []}
    for _ in range(ROUNDS):
        for arm in ("without", "with"):
            ctx.attach_average(step_avg if arm == "with" else None, 1, 1200.0)
            arms[arm].append(events_ms(lambda: steps(STEPS), 1) / STEPS)
    ctx.attach_average(None)
    ctx.sync()
    _, collected = step_avg.weight()
    print(json.dumps(dict(
        grid=[NX, NY, H], fields=K, launches=LAUNCHES,
        collect_us=round(1e3 * collect_ms, 2), collect_bytes=accumulate_bytes, collect_tbps=round(rate(accumulate_bytes, collect_ms), 3),
        store_us=round(1e3 * store_ms, 2), store_bytes=store_bytes, store_tbps=round(rate(store_bytes, store_ms), 3),
        copy_same_bytes_us=round(1e3 * copy_ms, 2), copy_same_bytes_tbps=round(rate(accumulate_bytes, copy_ms), 3),
        copy_256mib_tbps=round(rate(2 * (256 << 20), copy256_ms), 3),
        collect_over_copy=round(copy_ms / collect_ms, 3),
        steps_per_arm=STEPS, ms_per_step_without=[round(x, 5) for x in arms["without"]],
        ms_per_step_with=[round(x, 5) for x in arms["with"]],
        overhead_us=round(1e3 * (min(arms["with"]) - min(arms["without"])), 2), collected_steps=collected)))
    step_avg.close()
    ctx.close()


if __name__ == "__main__":
    main()
