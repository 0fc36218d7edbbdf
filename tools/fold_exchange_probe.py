"""What the tripolar fold costs inside the coupled loop's exchange launches, measured: writes profiles/fold_exchange_probe.json
(`--out` writes elsewhere) and prints it as one JSON line.

One process, one context connected as rank 0 of 1 in both worlds (it is the last rank: nothing waits).  Two surfaces: the
1440 x 560 workload of tools/coupled_step_probe.py, and 2160 x 135, the northernmost 8-way slab of the 2160 x 1080 tripolar
surface (BASELINE config 5).  Both with halo 7, CF_OPT_MERGED_PREFETCH = 2, two exchange sets, the skin carried, land freshwater,
restoring and the exact normalisation, and an ice state with all six fields: ten fields per step as exchanges of eight and two,
three per call.  cf_time_steps_coupled, CALLS steps per call, in three forms:
  (a) none_fold   CF_HALO_NONE, fold_north = 1: the fold's own launch per step, four ocean fields (the form before the fold rode);
  (b) peer        CF_HALO_PEER, fold_north = 0: two exchange launches per step whose workgroups return at once;
  (c) peer_fold   CF_HALO_PEER, fold_north = 1: the same two launches, their north sides folding the ten fields' rows.
By events on the context's stream, ROUNDS alternating rounds after a warm-up, reported as the median and the min ... max of the
rounds' microseconds per step.  (c) - (b) is what the fold costs inside launches already issued.  Reported, not gated: ranks that
share a device say nothing about the multi-rank step over xGMI."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "climaocean.jl_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch  # noqa: E402

from coflux import abi, synthetic as syn, interface_computations as ic  # noqa: E402
from coflux.distributed import connect_coupled_slabs  # noqa: E402
from coflux.runtime import EXCHANGE_NAMES, FLUX_NAMES, NET_NAMES, FluxContext  # noqa: E402

H = 7
SURFACES = {"1440x560": (1440, 560, None, 0), "2160x135": (2160, 135, 1080, 945)}   # nx, ny, ny_global, j_offset
ROUNDS, CALLS, WARMUP = 5, 300, 50
N_LEVELS, INC = 4, 1.0 / 9.0
PISTON = 1.0 / 6.0 / 86400.0
FORMS = {"none_fold": (abi.HALO_NONE, True), "peer": (abi.HALO_PEER, False), "peer_fold": (abi.HALO_PEER, True)}


def events_us(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn(n)
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b) / n


def summary(rounds):
    return dict(median_us=round(statistics.median(rounds), 3), min_us=round(min(rounds), 3), max_us=round(max(rounds), 3),
                rounds_us=[round(r, 3) for r in rounds])


def surface(nx, ny, ny_global, j_offset):
    params = ic.flux_params(ic.SimilarityTheoryFluxes(), ocean_surface=ic.SurfaceRadiationProperties(0.06, 1.0))
    ctx = FluxContext(nx, ny, H, H, params, ring=1)
    kw = dict(ny_global=ny_global, j_offset=j_offset)
    o0 = syn.ocean_state(nx, ny, H, H, **kw)
    o1 = syn.evolved_ocean_state(o0, nx, ny, H, H, 1, **kw)
    states = [{k: ctx.to_device(o[k]) for k in ("T", "S", "u", "v", "mask")} for o in (o0, o1)]
    states[1]["mask"] = states[0]["mask"]
    src = {k: ctx.to_device(v) for k, v in syn.jra55_snapshots(N_LEVELS, temporal_correlation=0.95).items()}
    land = {k: ctx.to_device(v) for k, v in syn.jra55_land_snapshots(N_LEVELS).items()}
    fi, fj, phi = syn.latlon_fractional_indices(nx, ny, H, H, **kw)
    w = dict(separable=True, fi=ctx.to_device(fi), fj=ctx.to_device(fj), latitude=ctx.to_device(phi))
    ctx.set_option(abi.OPT_MERGED_PREFETCH, 2)
    ctx.set_sea_ice_formulation(ic.flux_params(ic.corrected_atmosphere_sea_ice_fluxes()))
    si = syn.sea_ice_state(nx, ny, H, H, **kw)
    stresses = dict(x_stress=ctx.to_device(o0["ice_x_stress"]), y_stress=ctx.to_device(o0["ice_y_stress"]))
    ice_state = dict(concentration=ctx.to_device(o0["ice_concentration"]), snow_thickness=ctx.to_device(0.2 * si["thickness"]),
                     **{k: ctx.to_device(si[k]) for k in ("thickness", "u", "v", "albedo")})
    skin0 = ctx.to_device(si["top_temperature"])
    iop = ctx.default_ice_ocean_params(time_step=1200.0, top_cell_thickness=10.0)
    target = ctx.to_device(o0["S"] + 0.1)
    out = dict(sets=[ctx.field_set(EXCHANGE_NAMES) for _ in range(2)], fl=ctx.field_set(FLUX_NAMES), net=ctx.field_set(NET_NAMES[:5]),
               ai=ctx.field_set(tuple(k for k in FLUX_NAMES if k != "temperature")), skin=skin0.clone(),
               net_ice=ctx.field_set(("top_heat", "bottom_heat")),
               iof=ctx.field_set(("interface_heat", "salt_flux", "frazil_heat")), land=ctx.zeros(), restoring=ctx.zeros(),
               mean=torch.zeros(1, dtype=torch.float64, device=ctx.device))
    assert connect_coupled_slabs(ctx) == (0, 1)
    block = ctx.make_coupled_step([ice_state], out["skin"], out["ai"], out["net_ice"], friver=land["friver"], licalvf=land["licalvf"],
                                  land_out=out["land"], land_first_level=1, land_time_fraction=0.8, land_time_fraction_increment=INC,
                                  ice_ocean_params=iop, ice_ocean_fluxes=out["iof"], piston_velocity=PISTON, target=target,
                                  restoring_out=out["restoring"], normalize="exact", mean_out=out["mean"])
    step = [0]

    def form(backend, fold):
        sch = ctx.make_schedule(states, out["sets"], first_level=0, time_fraction=0.0, time_fraction_increment=INC,
                                pipeline=abi.PIPELINE_CONTINUING, halo_backend=backend, halo_rows=2 if backend != abi.HALO_NONE else 0,
                                fold_north=fold)

        def loop(n):
            ctx.time_steps_coupled(step[0], n, sch, src, w, out["fl"], out["net"], stresses, block)
            step[0] += n
        return loop

    loops = {name: form(*spec) for name, spec in FORMS.items()}
    rounds = {name: [] for name in loops}
    counts = {}
    for name, fn in loops.items():
        out["skin"].copy_(skin0)
        before = ctx.peer_halo_stats() + ctx.fold_counts()
        fn(WARMUP)
        ctx.sync()
        ctx.discard_prefetched_atmosphere_state()
        after = ctx.peer_halo_stats() + ctx.fold_counts()
        # per WARMUP steps: (exchange launches, of which in a solver launch, fold launches, exchanges that carried a fold)
        counts[name] = [a - b for a, b in zip(after, before)]
    for _ in range(ROUNDS):
        for name, fn in loops.items():
            rounds[name].append(events_us(fn, CALLS))
            ctx.sync()
            ctx.discard_prefetched_atmosphere_state()
    result = {name: dict(summary(v), launches_per_warmup=counts[name]) for name, v in rounds.items()}
    result["peer_fold_minus_peer_us"] = round(result["peer_fold"]["median_us"] - result["peer"]["median_us"], 3)
    result["peer_fold_minus_none_fold_us"] = round(result["peer_fold"]["median_us"] - result["none_fold"]["median_us"], 3)
    ctx.close()
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fold_exchange_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fold_exchange_probe needs a HIP device: nothing is measured without one")
    out = dict(halo=H, rounds=ROUNDS, steps_per_call=CALLS, warmup=WARMUP, device=torch.cuda.get_device_name(0),
               surfaces={name: surface(*shape) for name, shape in SURFACES.items()})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
