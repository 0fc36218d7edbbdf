"""The exact NormalizeSalinity, measured in one process: writes profiles/exact_normalization_probe.json and prints it as one JSON
line.

Surfaces and method are tools/coupled_step_probe.py's: the 1440 x 560 `--config sea_ice` workload of bench.py with land
freshwater, salinity restoring and normalisation, and a 1440 x 140 slab of it; events on the context's stream, ROUNDS alternating
rounds of CALLS calls after a warm-up, reported as the median and the min ... max of the rounds' microseconds per call:
  (a) normalisation: cf_normalize_salinity_flux (unchanged: the baseline) against cf_normalize_salinity_flux_exact, on the net
      salt flux of one coupled step with the restoring buffer as the additional flux, with and without cell areas;
  (b) step: cf_time_steps_coupled (CALLS steps per call) with normalize_salinity = 1 against CF_NORMALIZE_EXACT.
The exact form is opt-in: reported, not gated.  Nothing here says anything about several ranks — the reduction over HIP-IPC
mailboxes between devices is unmeasured."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "climaocean.jl_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import torch  # noqa: E402

from coflux import abi, synthetic as syn, interface_computations as ic  # noqa: E402
from coflux.runtime import EXCHANGE_NAMES, FLUX_NAMES, NET_NAMES, FluxContext  # noqa: E402
from coupled_step_probe import CALLS, H, INC, N_LEVELS, PISTON, ROUNDS, SURFACES, WARMUP, events_us, summary  # noqa: E402


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
    i, j = syn.ocean_indices(nx, ny, H, H)
    area = ctx.to_device(1.2e10 * (0.05 + syn.uniform("hi", i, j, 5)))
    out = dict(sets=[ctx.field_set(EXCHANGE_NAMES) for _ in range(2)], fl=ctx.field_set(FLUX_NAMES), net=ctx.field_set(NET_NAMES[:5]),
               ai=ctx.field_set(tuple(k for k in FLUX_NAMES if k != "temperature")), skin=skin0.clone(),
               net_ice=ctx.field_set(("top_heat", "bottom_heat")),
               iof=ctx.field_set(("interface_heat", "salt_flux", "frazil_heat")), land=ctx.zeros(), restoring=ctx.zeros(),
               mean=torch.zeros(1, dtype=torch.float64, device=ctx.device))
    sch = ctx.make_schedule(states, out["sets"], first_level=0, time_fraction=0.0, time_fraction_increment=INC, pipeline=abi.PIPELINE_CONTINUING)

    def block(normalize):
        return ctx.make_coupled_step([ice_state], out["skin"], out["ai"], out["net_ice"], friver=land["friver"], licalvf=land["licalvf"],
                                     land_out=out["land"], land_first_level=1, land_time_fraction=0.8, land_time_fraction_increment=INC,
                                     ice_ocean_params=iop, ice_ocean_fluxes=out["iof"], piston_velocity=PISTON, target=target,
                                     restoring_out=out["restoring"], normalize=normalize, area=area, mean_out=out["mean"])

    blocks = {"ordered": block(True), "exact": block("exact")}
    step = [0]

    def loop(which):
        def go(n):
            ctx.time_steps_coupled(step[0], n, sch, src, w, out["fl"], out["net"], stresses, blocks[which])
            step[0] += n
        return go

    # one coupled step leaves a net salt flux and a restoring buffer to normalise (each call subtracts a mean of about zero after
    # the first: the field stays what it is)
    loop("ordered")(1)
    ctx.sync()
    ctx.discard_prefetched_atmosphere_state()
    mask = states[0]["mask"]

    def normalise(exact, with_area):
        fn = ctx.normalize_salinity_flux_exact if exact else ctx.normalize_salinity_flux

        def go(n):
            for _ in range(n):
                fn(out["net"]["S"], mask, additional=out["restoring"], area=area if with_area else None, mean_out=out["mean"])
        return go

    groups = (("normalisation_with_areas", (("ordered", normalise(False, True)), ("exact", normalise(True, True)))),
              ("normalisation_uniform", (("ordered", normalise(False, False)), ("exact", normalise(True, False)))),
              ("step", (("ordered", loop("ordered")), ("exact", loop("exact")))))
    result = {}
    for name, pair in groups:
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
        result[name]["exact_minus_ordered_us"] = round(result[name]["exact"]["median_us"] - result[name]["ordered"]["median_us"], 3)
    ctx.close()
    return result


def main():
    if not torch.cuda.is_available():
        raise SystemExit("exact_normalization_probe needs a HIP device: nothing is measured without one")
    out = dict(halo=H, rounds=ROUNDS, calls=CALLS, warmup=WARMUP, device=torch.cuda.get_device_name(0),
               surfaces={name: surface(*shape) for name, shape in SURFACES.items()},
               multi_rank="unmeasured: ranks that time-share one device say nothing about xGMI")
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "exact_normalization_probe.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
