"""Cost of the derived averager on the 1/4-degree surface (1440 x 560, halo 7).  Two term sets: the seven velocity outputs
(uos, vos, uosq, vosq, kes, east, north from u, v, cos, sin) and the fifteen of omip_surface_outputs (ten source arrays).
For each, alternating in one process, ROUNDS times, HIP events over LAUNCHES back-to-back launches:
  * an accumulating and a storing collection of cf_average_create_derived;
  * (a) cf_time_copy of the accumulating collection's algorithmic bytes (8 per distinct source + 16 per term, per cell);
  * (b) what a caller could do without it: torch launches that materialise every derived field, then cf_average_collect.
Writes profiles/derived_average_probe.json (and prints it): per arm the median and the [min, max] of the rounds in
microseconds, the collection as a fraction of the copy's rate and its ratio to (b)."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "climaocean.jl_amd"))
import torch  # noqa: E402

from coflux import interface_computations as ic  # noqa: E402
from coflux.runtime import FluxContext  # noqa: E402

NX, NY, H = 1440, 560, 7
LAUNCHES, ROUNDS = 500, 5
RHO = 1026.0


def events_us(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b) / n


def velocity_set(f):
    u, v = f["u"], f["v"]
    return [("field", u, None, 1.0, 0), ("field", v, None, 1.0, 0), ("center_x_square", u, None, 1.0, 0),
            ("center_y_square", v, None, 1.0, 0), ("kinetic_energy", u, v, 1.0, 0), ("east", u, v, 1.0, 0), ("north", u, v, 1.0, 0)]


def omip_set(f):
    T, S, u, v = f["T"], f["S"], f["u"], f["v"]
    plain = [f[k] for k in ("taux", "tauy", "JT", "JS", "Qc", "Qv")]
    return ([("field", x, None, 1.0, 0) for x in (T, S, u, v)] + [("product", T, T, 1.0, 0), ("product", S, S, 1.0, 0),
            ("center_x_square", u, None, 1.0, 0), ("center_y_square", v, None, 1.0, 0), ("kinetic_energy", u, v, 1.0, 0)]
            + [("field", x, None, 1.0, 0) for x in plain])


def materialise(ctx, terms, cos, sin):
    """the torch launches of arm (b): every term that is not a plain field is written to an array of its own"""
    I = (slice(H, H + NY), slice(H, H + NX))
    E = (slice(H, H + NY), slice(H + 1, H + NX + 1))
    N = (slice(H + 1, H + NY + 1), slice(H, H + NX))
    sources, work = [], []
    for kind, a, b, scale, _flags in terms:
        if kind == "field":
            sources.append(a)
            continue
        out = ctx.zeros()
        sources.append(out)
        work.append((kind, a, b, out))

    def run():
        for kind, a, b, out in work:
            if kind == "product":
                torch.mul(a[I], b[I], out=out[I])
            elif kind == "center_x_square":
                out[I] = (a[I] * a[I] + a[E] * a[E]) * 0.5
            elif kind == "center_y_square":
                out[I] = (a[I] * a[I] + a[N] * a[N]) * 0.5
            elif kind == "kinetic_energy":
                out[I] = ((a[I] * a[I] + a[E] * a[E]) * 0.5 + (b[I] * b[I] + b[N] * b[N]) * 0.5) * 0.5
            else:
                p, q = (a[I] + a[E]) * 0.5, (b[I] + b[N]) * 0.5
                out[I] = p * cos[I] - q * sin[I] if kind == "east" else p * sin[I] + q * cos[I]
    return sources, run


def probe(ctx, name, terms, fields, cos, sin):
    cells = NX * NY
    distinct = {t.data_ptr() for _, a, b, _, _ in terms for t in (a, b) if t is not None}
    if any(k in ("east", "north") for k, *_ in terms):
        distinct |= {cos.data_ptr(), sin.data_ptr()}
    accumulate_bytes = cells * (8 * len(distinct) + 16 * len(terms))
    store_bytes = cells * (8 * len(distinct) + 8 * len(terms))
    means = [ctx.zeros() for _ in terms]
    avg = ctx.derived_average([t + (m,) for t, m in zip(terms, means)], cos, sin)
    sources_b, run_b = materialise(ctx, terms, cos, sin)
    plain = ctx.average(sources_b, [ctx.zeros() for _ in terms])

    def store():
        avg.reset()
        avg.collect(1.0)

    def unfused():
        run_b()
        plain.collect(1.0)
    arms = dict(accumulate=lambda: events_us(lambda: avg.collect(1.0), LAUNCHES), store=lambda: events_us(store, LAUNCHES),
                copy_same_bytes=lambda: 1e3 * ctx.time_copy(accumulate_bytes // 2, LAUNCHES),
                torch_then_collect=lambda: events_us(unfused, LAUNCHES))
    for fn in arms.values():   # warm-up: code load, clocks, allocator
        fn()
    rounds = {k: [] for k in arms}
    for _ in range(ROUNDS):
        for k, fn in arms.items():
            rounds[k].append(fn())
    ctx.sync()
    med = {k: statistics.median(v) for k, v in rounds.items()}
    out = dict(terms=len(terms), distinct_sources=len(distinct), accumulate_bytes=accumulate_bytes, store_bytes=store_bytes)
    for k, v in rounds.items():
        out[k + "_us"] = dict(median=round(med[k], 2), min=round(min(v), 2), max=round(max(v), 2))
    out["accumulate_tbps"] = round(accumulate_bytes / med["accumulate"] / 1e6, 3)
    out["store_tbps"] = round(store_bytes / med["store"] / 1e6, 3)
    out["copy_tbps"] = round(accumulate_bytes / med["copy_same_bytes"] / 1e6, 3)
    out["fraction_of_copy"] = round(med["copy_same_bytes"] / med["accumulate"], 3)
    out["torch_then_collect_over_accumulate"] = round(med["torch_then_collect"] / med["accumulate"], 2)
    avg.close()
    plain.close()
    return out


def main():
    ctx = FluxContext(NX, NY, H, H, ic.flux_params(), ring=1)
    gen = torch.Generator(device=ctx.device).manual_seed(0)
    f = {k: torch.randn(ctx.shape, dtype=torch.float64, device=ctx.device, generator=gen)
         for k in ("T", "S", "u", "v", "taux", "tauy", "JT", "JS", "Qc", "Qv")}
    theta = torch.rand(ctx.shape, dtype=torch.float64, device=ctx.device, generator=gen) * 6.283185307179586
    cos, sin = torch.cos(theta), torch.sin(theta)
    result = dict(grid=[NX, NY, H], launches=LAUNCHES, rounds=ROUNDS, device=torch.cuda.get_device_name(0),
                  velocity=probe(ctx, "velocity", velocity_set(f), f, cos, sin), omip=probe(ctx, "omip", omip_set(f), f, cos, sin))
    ctx.close()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "derived_average_probe.json"), "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
