"""Cost of the budget averager (cf_average_create_budget) on the 1/4-degree surface (1440 x 560, halo 7) and on the
1440 x 140 slab of a four-way split.  Per surface three cases, alternating in one process, ROUNDS times, HIP events over
LAUNCHES back-to-back launches of an accumulating collection:
  * the six terms of the reference's `:surface` writer (JTao, JTio, JTf, JTn, JSn, JSio: all thirteen inputs are read);
  * all fifteen kinds;
  * an ordinary cf_average of the same number of fields (six, fifteen): what averaging the parts would cost if they existed
    as arrays — and they do not: materialising them is a further pass that is not priced here.
Each is priced at its algorithmic bytes against the device-copy calibration of the same run (cf_time_copy, CF_STAGE_COPY's
kernel): budget 8 per distinct input + 1 (the uint8 mask) + 16 per term and cell, ordinary 24 per field and cell.
Writes profiles/budget_probe.json (or --out) and prints it: per arm the median and the [min, max] of the rounds in
microseconds, its rate and its fraction of the copy's rate."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "climaocean.jl_amd"))
import torch  # noqa: E402

from coflux import abi  # noqa: E402
from coflux import interface_computations as ic  # noqa: E402
from coflux.runtime import FluxContext  # noqa: E402

H = 7
SURFACES = {"1440x560": (1440, 560), "1440x140": (1440, 140)}
LAUNCHES, ROUNDS = 500, 5
SIX = (abi.BUDGET_HEAT_ATMOSPHERE_OCEAN, abi.BUDGET_HEAT_ICE_OCEAN, abi.BUDGET_HEAT_FRAZIL, abi.BUDGET_HEAT_NET, abi.BUDGET_SALT_NET,
       abi.BUDGET_SALT_ICE_OCEAN)
INPUTS = 13


def events_us(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b) / n


def probe(nx, ny):
    ctx = FluxContext(nx, ny, H, H, ic.flux_params(ocean_minimum_salinity=1.0), ring=1)
    gen = torch.Generator(device=ctx.device).manual_seed(0)
    rand = lambda lo, hi: lo + (hi - lo) * torch.rand(ctx.shape, dtype=torch.float64, device=ctx.device, generator=gen)  # noqa: E731
    mask = (torch.rand(ctx.shape, device=ctx.device, generator=gen) > 0.3).to(torch.uint8)
    inputs = dict(ocean=dict(S=rand(30.0, 37.0), mask=mask), atmos=dict(Qs=rand(0.0, 900.0), Ql=rand(150.0, 450.0), Mp=rand(0.0, 2e-4)),
                  fluxes=dict(sensible_heat=rand(-80.0, 40.0), latent_heat=rand(-300.0, 20.0), water_vapor=rand(-1e-5, 1.2e-4),
                              temperature=rand(-1.8, 29.0)),
                  ice=dict(concentration=rand(0.0, 1.0), interface_heat=rand(-30.0, 30.0), salt_flux=rand(-1e-6, 1e-6)),
                  frazil_heat=rand(0.0, 50.0), land_freshwater=rand(0.0, 3e-4))
    cells = nx * ny
    arms, bytes_of, keep = {}, {}, []
    for name, kinds in (("budget_6", SIX), ("budget_15", tuple(range(abi.BUDGET_KINDS)))):
        avg = ctx.budget_average([(k, 1.0, ctx.zeros()) for k in kinds], **inputs)
        plain = ctx.average([rand(-1.0, 1.0) for _ in kinds], [ctx.zeros() for _ in kinds])
        keep += [avg, plain]
        for arm, handle, per_cell in ((name, avg, 8 * INPUTS + 1 + 16 * len(kinds)), (f"plain_{len(kinds)}", plain, 24 * len(kinds))):
            handle.collect(1.0)   # the window is open: every timed collection accumulates
            arms[arm] = (lambda h=handle: events_us(lambda: h.collect(1.0), LAUNCHES))
            bytes_of[arm] = cells * per_cell
            arms[arm + "_copy_same_bytes"] = (lambda b=cells * per_cell: 1e3 * ctx.time_copy(b // 2, LAUNCHES))
    for fn in arms.values():   # warm-up: code load, clocks, allocator
        fn()
    rounds = {k: [] for k in arms}
    for _ in range(ROUNDS):
        for k, fn in arms.items():
            rounds[k].append(fn())
    ctx.sync()
    med = {k: statistics.median(v) for k, v in rounds.items()}
    out = {}
    for arm, nbytes in bytes_of.items():
        copy = arm + "_copy_same_bytes"
        out[arm] = dict(algorithmic_bytes=nbytes, bytes_per_cell=nbytes // cells,
                        us=dict(median=round(med[arm], 2), min=round(min(rounds[arm]), 2), max=round(max(rounds[arm]), 2)),
                        copy_same_bytes_us=dict(median=round(med[copy], 2), min=round(min(rounds[copy]), 2), max=round(max(rounds[copy]), 2)),
                        tbps=round(nbytes / med[arm] / 1e6, 3), copy_tbps=round(nbytes / med[copy] / 1e6, 3),
                        fraction_of_copy=round(med[copy] / med[arm], 3))
    for h in keep:
        h.close()
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "budget_probe.json"))
    args = ap.parse_args()
    result = dict(halo=H, launches=LAUNCHES, rounds=ROUNDS, device=torch.cuda.get_device_name(0),
                  surfaces={name: probe(nx, ny) for name, (nx, ny) in SURFACES.items()})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
