"""The coupled step on the device, measured: writes profiles/coupled_step_probe.json and prints it as one JSON line.

Two surfaces: the 1440 x 560 `--config sea_ice` workload of bench.py (halo 7, syn.sea_ice_state, CF_OPT_MERGED_PREFETCH = 2, two
exchange sets, the skin carried) plus land freshwater, salinity restoring and normalisation, and a 1440 x 140 slab of it.
Two measurements, both by events on the context's stream, ROUNDS alternating rounds of CALLS calls after a warm-up, reported
as the median and the min ... max of the rounds' microseconds per call:
  (a) preamble: cf_interpolate_land_freshwater + cf_compute_sea_ice_ocean_fluxes + cf_materialize_salinity_restoring back to
      back, against cf_prepare_coupled_step.  `fused_wins`: the fused median is below the three launches' median by more than
      the three launches' own min ... max spread (the rule by which the step loop uses the fused kernel: DESIGN 5.14);
  (b) step: the host loop of the entry points a coupled step needs, against cf_time_steps_coupled (CALLS steps per call).
      Reported, not gated."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "climaocean.jl_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch  # noqa: E402

from coflux import abi, synthetic as syn, interface_computations as ic  # noqa: E402
from coflux.runtime import EXCHANGE_NAMES, FLUX_NAMES, NET_NAMES, FluxContext  # noqa: E402

H = 7
SURFACES = {"1440x560": (1440, 560, None, 0), "1440x140": (1440, 140, 560, 280)}   # nx, ny, ny_global, j_offset
ROUNDS, CALLS, WARMUP = 5, 500, 50
N_LEVELS, INC = 4, 1.0 / 9.0
PISTON = 1.0 / 6.0 / 86400.0


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


def clock(step, first_level=0, fraction=0.0):
    total = fraction + step * INC
    whole = int(total)
    l1 = (first_level + whole) % N_LEVELS
    return l1, (l1 + 1) % N_LEVELS, total - whole


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
    conc = ctx.to_device(o0["ice_concentration"])
    stresses = dict(x_stress=ctx.to_device(o0["ice_x_stress"]), y_stress=ctx.to_device(o0["ice_y_stress"]))
    ice_state = dict(concentration=conc, **{k: ctx.to_device(si[k]) for k in ("thickness", "u", "v", "albedo")})
    skin0 = ctx.to_device(si["top_temperature"])
    iop = ctx.default_ice_ocean_params(time_step=1200.0, top_cell_thickness=10.0)
    target = ctx.to_device(o0["S"] + 0.1)
    out = dict(sets=[ctx.field_set(EXCHANGE_NAMES) for _ in range(2)], fl=ctx.field_set(FLUX_NAMES), net=ctx.field_set(NET_NAMES[:5]),
               ai=ctx.field_set(tuple(k for k in FLUX_NAMES if k != "temperature")), skin=skin0.clone(),
               net_ice=ctx.field_set(("top_heat", "bottom_heat")),
               iof=ctx.field_set(("interface_heat", "salt_flux", "frazil_heat")), land=ctx.zeros(), restoring=ctx.zeros(),
               mean=torch.zeros(1, dtype=torch.float64, device=ctx.device))

    # (a) the preamble
    def three(n):
        for s in range(n):
            l1, l2, lf = clock(s % 27, 1, 0.8)
            o = states[s % 2]
            ctx.interpolate_land_freshwater(land["friver"], land["licalvf"], w, out["land"], level1=l1, level2=l2, time_fraction=lf)
            ctx.compute_sea_ice_ocean_fluxes(iop, o, conc, stresses["x_stress"], stresses["y_stress"], out["iof"])
            ctx.materialize_salinity_restoring(PISTON, target, o, out["restoring"])

    def fused(n):
        for s in range(n):
            l1, l2, lf = clock(s % 27, 1, 0.8)
            ctx.prepare_coupled_step(states[s % 2], weights=w, friver=land["friver"], licalvf=land["licalvf"], land_out=out["land"],
                                     level1=l1, level2=l2, time_fraction=lf, ice_ocean_params=iop, concentration=conc,
                                     x_stress=stresses["x_stress"], y_stress=stresses["y_stress"], ice_ocean_out=out["iof"],
                                     piston_velocity=PISTON, target=target, restoring_out=out["restoring"])

    # (b) the step
    step = [0]

    def host_loop(n):
        for _ in range(n):
            s = step[0]
            o = states[s % 2]
            l1, l2, lf = clock(s, 1, 0.8)
            ctx.interpolate_land_freshwater(land["friver"], land["licalvf"], w, out["land"], level1=l1, level2=l2, time_fraction=lf)
            ctx.set_land_freshwater(out["land"])
            ctx.compute_sea_ice_ocean_fluxes(iop, o, conc, stresses["x_stress"], stresses["y_stress"], out["iof"])
            ctx.materialize_salinity_restoring(PISTON, target, o, out["restoring"])
            n1, n2, nf = clock(s + 1)
            ctx.prefetch_atmosphere_state(src, w, out["sets"][(s + 1) % 2], level1=n1, level2=n2, time_fraction=nf)
            a1, a2, af = clock(s)
            partition = dict(stresses, concentration=conc, interface_heat=out["iof"]["interface_heat"], salt_flux=out["iof"]["salt_flux"])
            ctx.update_state_sea_ice(src, w, o, out["sets"][s % 2], out["fl"], out["net"], partition, dict(ice_state, top_temperature=out["skin"]),
                                     dict(out["ai"], temperature=out["skin"]), out["net_ice"], frazil_heat=out["iof"]["frazil_heat"],
                                     interface_heat=out["iof"]["interface_heat"], level1=a1, level2=a2, time_fraction=af)
            ctx.normalize_salinity_flux(out["net"]["S"], o["mask"], additional=out["restoring"], mean_out=out["mean"])
            step[0] += 1

    sch = ctx.make_schedule(states, out["sets"], first_level=0, time_fraction=0.0, time_fraction_increment=INC, pipeline=abi.PIPELINE_CONTINUING)
    block = ctx.make_coupled_step([ice_state], out["skin"], out["ai"], out["net_ice"], friver=land["friver"], licalvf=land["licalvf"],
                                  land_out=out["land"], land_first_level=1, land_time_fraction=0.8, land_time_fraction_increment=INC,
                                  ice_ocean_params=iop, ice_ocean_fluxes=out["iof"], piston_velocity=PISTON, target=target,
                                  restoring_out=out["restoring"], normalize=True, mean_out=out["mean"])

    def device_loop(n):
        ctx.time_steps_coupled(step[0], n, sch, src, w, out["fl"], out["net"], stresses, block)
        step[0] += n

    result = {}
    for name, pair in (("preamble", (("three_launches", three), ("fused", fused))), ("step", (("host_loop", host_loop), ("device_loop", device_loop)))):
        rounds = {k: [] for k, _ in pair}
        for k, fn in pair:
            out["skin"].copy_(skin0)
            fn(WARMUP)
            ctx.sync()
            ctx.discard_prefetched_atmosphere_state()
        for _ in range(ROUNDS):
            for k, fn in pair:
                rounds[k].append(events_us(fn, CALLS))
                ctx.sync()
                ctx.discard_prefetched_atmosphere_state()
        result[name] = {k: summary(v) for k, v in rounds.items()}
    p = result["preamble"]
    spread = p["three_launches"]["max_us"] - p["three_launches"]["min_us"]
    p["fused_wins"] = bool(p["three_launches"]["median_us"] - p["fused"]["median_us"] > spread)
    ctx.close()
    return result


def main():
    if not torch.cuda.is_available():
        raise SystemExit("coupled_step_probe needs a HIP device: nothing is measured without one")
    out = dict(halo=H, rounds=ROUNDS, calls=CALLS, warmup=WARMUP, device=torch.cuda.get_device_name(0),
               surfaces={name: surface(*shape) for name, shape in SURFACES.items()})
    out["fused_preamble_wins_on_both"] = all(s["preamble"]["fused_wins"] for s in out["surfaces"].values())
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "coupled_step_probe.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
