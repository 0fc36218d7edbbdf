"""Cost of the calendar-binned means on the 1/4-degree surface (1440 x 560, halo 7) and on a 1440 x 70 slab
-> profiles/climatology_probe.json.

    python tools/climatology_probe.py [--out PATH]

The driver starts the GPU step as a child under its own `timeout`; nothing follows a step that failed.  The step: one
process, warm-up first, the arms interleaved, medians of ROUNDS rounds, every arm by HIP events over back-to-back launches:
  (a) one accumulating cf_climatology_collect of 2, 6 and 16 fields into 12 bins (40 algorithmic bytes per cell and field);
  (b) the two cf_average_collect launches that produce the same two results today — one averager on the totals, one on
      the bin — on the same fields (2 x 24 bytes per cell and field);
  (c) cf_time_copy of (a)'s bytes in the same process: the device's copy rate, of which (a) achieves `fraction_of_copy`;
  (d) cf_climatology_extremes of one field with 12 non-empty bins (12 x 8 bytes read, 2 x 8 + 2 x 4 written per cell).
The yardstick is (b): `within_spread` says whether (a)'s median exceeds (b)'s by no more than the spread (max - min) of (b)'s
own rounds."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "climaocean.jl_amd"))

NX, H = 1440, 7
ROUNDS = 5
N_BINS = 12


def measure(launches):
    import torch
    from coflux import interface_computations as ic
    from coflux.runtime import FluxContext

    def events_ms(fn, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / n

    med = statistics.median
    result = dict(grid_x=NX, halo=H, n_bins=N_BINS, launches=launches, rounds=ROUNDS, surfaces={})
    for ny in (560, 70):
        ctx = FluxContext(NX, ny, H, H, ic.flux_params(), ring=1)
        cells = NX * ny
        gen = torch.Generator(device=ctx.device).manual_seed(ny)
        arms, out = {}, {}
        for n in (2, 6, 16):
            sources = [torch.randn(ctx.shape, dtype=torch.float64, device=ctx.device, generator=gen) for _ in range(n)]
            totals = [ctx.zeros() for _ in range(n)]
            blocks = [torch.zeros((N_BINS,) + tuple(ctx.shape), dtype=torch.float64, device=ctx.device) for _ in range(n)]
            clim = ctx.climatology(sources, totals, blocks, N_BINS)
            avg_total = ctx.average(sources, [ctx.zeros() for _ in range(n)])
            avg_bin = ctx.average(sources, [ctx.zeros() for _ in range(n)])
            turn = [0]

            def collect(clim=clim, turn=turn):
                clim.collect(turn[0] % N_BINS, 1.0)
                turn[0] += 1

            def two_launches(avg_total=avg_total, avg_bin=avg_bin):
                avg_total.collect(1.0)
                avg_bin.collect(1.0)

            for _ in range(3 * N_BINS):     # every bin and both averagers accumulate from here on
                collect()
                two_launches()
            arms[n] = (collect, two_launches, clim, avg_total, avg_bin, blocks)
            out[n] = dict(a=[], b=[], c=[])
        lo, hi = ctx.zeros(), ctx.zeros()
        alo, ahi = (torch.zeros(ctx.shape, dtype=torch.int32, device=ctx.device) for _ in range(2))
        extremes = lambda: arms[2][2].extremes(0, out=(lo, hi, alo, ahi))  # noqa: E731
        extremes()
        t_ext, t_ext_copy = [], []
        ext_bytes = cells * (N_BINS * 8 + 2 * 8 + 2 * 4)
        for _ in range(ROUNDS):     # interleaved
            for n in (2, 6, 16):
                collect, two_launches = arms[n][:2]
                out[n]["a"].append(events_ms(collect, launches))
                out[n]["b"].append(events_ms(two_launches, launches))
                out[n]["c"].append(ctx.time_copy(cells * n * 40 // 2, launches))
            t_ext.append(events_ms(extremes, launches))
            t_ext_copy.append(ctx.time_copy(ext_bytes // 2, launches))
        surface = dict(ny=ny, cells=cells, fields={})
        for n in (2, 6, 16):
            a, b, c = out[n]["a"], out[n]["b"], out[n]["c"]
            spread_b = max(b) - min(b)
            surface["fields"][str(n)] = dict(
                climatology_us=round(1e3 * med(a), 2), climatology_bytes=cells * n * 40, climatology_spread_us=round(1e3 * (max(a) - min(a)), 2),
                two_averagers_us=round(1e3 * med(b), 2), two_averagers_bytes=cells * n * 48, two_averagers_spread_us=round(1e3 * spread_b, 2),
                copy_same_bytes_us=round(1e3 * med(c), 2), copy_spread_us=round(1e3 * (max(c) - min(c)), 2),
                fraction_of_copy=round(med(c) / med(a), 3), climatology_over_two_averagers=round(med(a) / med(b), 3),
                within_spread=bool(med(a) - med(b) <= spread_b),
                climatology_us_all=[round(1e3 * x, 2) for x in a], two_averagers_us_all=[round(1e3 * x, 2) for x in b],
                copy_us_all=[round(1e3 * x, 2) for x in c])
        surface["extremes"] = dict(us=round(1e3 * med(t_ext), 2), bytes=ext_bytes, spread_us=round(1e3 * (max(t_ext) - min(t_ext)), 2),
                                   copy_same_bytes_us=round(1e3 * med(t_ext_copy), 2), fraction_of_copy=round(med(t_ext_copy) / med(t_ext), 3),
                                   us_all=[round(1e3 * x, 2) for x in t_ext])
        result["surfaces"][f"{NX}x{ny}"] = surface
        for n in (2, 6, 16):
            for h in arms[n][2:5]:
                h.close()
        ctx.close()
        del arms
        torch.cuda.empty_cache()
    print("CLIMATOLOGY_PROBE " + json.dumps(result))


def child(args, limit):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), *args]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=ROOT)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-4000:])
        raise SystemExit(f"climatology_probe: step {' '.join(args)} ended with status {p.returncode}; nothing further is run")
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("CLIMATOLOGY_PROBE ")]
    return json.loads(lines[-1][len("CLIMATOLOGY_PROBE "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--measure", action="store_true")
    ap.add_argument("--launches", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "climatology_probe.json"))
    a = ap.parse_args()
    if a.measure:
        return measure(a.launches)
    result = child(["--measure", "--launches", str(a.launches)], 420)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
