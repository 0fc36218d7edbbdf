"""The three skin-temperature schemes of the atmosphere–sea-ice interface (CF_SKIN_EXPLICIT, CF_SKIN_SEMI_IMPLICIT,
CF_SKIN_LINEARISED) side by side, one JSON line.  Per scheme:
  * step_ms: cf_update_state_sea_ice per step on `bench.py --config sea_ice`'s workload (1440 x 560, halo 7, syn.sea_ice_state,
    the skin carried from step to step, the next step's interpolation and the ocean solve riding in the interface launch),
    HIP events over STEPS steps after WARMUP, the skin restored to the same first guess for every scheme;
  * solve_ms: cf_compute_atmosphere_sea_ice_fluxes alone on the full-size polar surface of tests/test_full_size.py
    (util.build_case(1440, 560, 7, 7) under util.polar_atmosphere, sea_ice_corrected), HIP events over SOLVES launches;
  * on both surfaces the share of wet cells at maxiter and the mean and median trip count (the step workload: its last step)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "climaocean.jl_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch  # noqa: E402

import oracle as orc  # noqa: E402
import util  # noqa: E402
from coflux import abi, synthetic as syn, interface_computations as ic  # noqa: E402
from coflux.runtime import EXCHANGE_NAMES, FLUX_NAMES, FLUX_OPTIONAL, NET_NAMES, FluxContext  # noqa: E402

NX, NY, H = 1440, 560, 7
WARMUP, STEPS, SOLVES, MAXITER = 20, 100, 20, 100
SCHEMES = {"explicit": abi.SKIN_EXPLICIT, "semi_implicit": abi.SKIN_SEMI_IMPLICIT, "linearised": abi.SKIN_LINEARISED}


def events_ms(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def trips(its, wet):
    t = its[wet]
    return dict(at_maxiter=round(float((t >= MAXITER).mean()), 4), mean_trips=round(float(t.mean()), 2),
                median_trips=float(np.median(t)))


def step_workload(results):
    """bench.py --config sea_ice's host-driven loop (tail pipeline: CF_OPT_MERGED_PREFETCH = 2, two exchange sets)."""
    params = ic.flux_params(ic.SimilarityTheoryFluxes(), ocean_surface=ic.SurfaceRadiationProperties(0.06, 1.0))
    ctx = FluxContext(NX, NY, H, H, params, ring=1)
    o0 = syn.ocean_state(NX, NY, H, H)
    o1 = syn.evolved_ocean_state(o0, NX, NY, H, H, 1)
    states = [{k: ctx.to_device(o[k]) for k in ("T", "S", "u", "v", "mask")} for o in (o0, o1)]
    states[1]["mask"] = states[0]["mask"]
    n_levels = 4
    src = {k: ctx.to_device(v) for k, v in syn.jra55_snapshots(n_levels, temporal_correlation=0.95).items()}
    fi, fj, phi = syn.latlon_fractional_indices(NX, NY, H, H)
    w = dict(separable=True, fi=ctx.to_device(fi), fj=ctx.to_device(fj), latitude=ctx.to_device(phi))
    ctx.set_option(abi.OPT_MERGED_PREFETCH, 2)
    sets = [ctx.field_set(EXCHANGE_NAMES) for _ in range(2)]
    fl, net = ctx.field_set(FLUX_NAMES), ctx.field_set(NET_NAMES[:5])
    si = syn.sea_ice_state(NX, NY, H, H)
    ice = {k: ctx.to_device(o0["ice_" + k]) for k in ("concentration", "interface_heat", "salt_flux", "x_stress", "y_stress")}
    ice_state = dict(concentration=ice["concentration"], **{k: ctx.to_device(si[k]) for k in ("thickness", "top_temperature", "u", "v", "albedo")})
    ai = ctx.field_set(FLUX_NAMES)
    ai["iterations"] = ctx.zeros(torch.int32)
    net_ice = ctx.field_set(("top_heat", "bottom_heat"))
    ai["temperature"].copy_(ice_state["top_temperature"])
    ice_state["top_temperature"] = ai["temperature"]
    skin0 = ai["temperature"].clone()
    inc = 1.0 / 9.0
    wet = o0["mask"][H:H + NY, H:H + NX] != 0
    for name, scheme in SCHEMES.items():
        ctx.set_sea_ice_formulation(ic.flux_params(ic.corrected_atmosphere_sea_ice_fluxes()),
                                    ic.SeaIceInterfaceProperties(skin_temperature_scheme=scheme).to_params())
        ai["temperature"].copy_(skin0)
        step = [0]

        def one():
            s = step[0]
            tot, nxt = s * inc, (s + 1) * inc
            l1, l1n = int(tot) % n_levels, int(nxt) % n_levels
            ctx.prefetch_atmosphere_state(src, w, sets[(s + 1) % 2], level1=l1n, level2=(l1n + 1) % n_levels, time_fraction=nxt - int(nxt))
            ctx.update_state_sea_ice(src, w, states[s % 2], sets[s % 2], fl, net, ice, ice_state, ai, net_ice,
                                     level1=l1, level2=(l1 + 1) % n_levels, time_fraction=tot - int(tot))
            step[0] += 1
        for _ in range(WARMUP):
            one()
        ctx.sync()
        ms = events_ms(one, STEPS)
        ctx.sync()
        its = ai["iterations"].cpu().numpy()[H:H + NY, H:H + NX]
        results[name]["step_ms"] = round(ms, 4)
        results[name]["step_surface"] = trips(its, wet)
    ctx.close()


def polar_solve(results):
    case = util.build_case(NX, NY, H, H)
    fluxes_f, vd = util.ICE_CONFIGS["sea_ice_corrected"]()
    ice_params = ic.flux_params(fluxes_f, velocity_difference=vd)
    g = orc.make_grid(NX, NY, H, H, 1)
    at = util.polar_atmosphere(orc.interpolate_atmosphere_state(g, case["src"], case["weights"], 0, 1, 0.37))
    ctx = FluxContext(NX, NY, H, H, ic.flux_params(), ring=1)
    dev = ctx.to_device
    ocean = {k: dev(case["ocean"][k]) for k in ("T", "S", "u", "v", "mask")}
    atmos = {k: dev(at[k]) for k in EXCHANGE_NAMES}
    st = {k: dev(v) for k, v in case["ice_state"].items() if v is not None}
    out = ctx.field_set(FLUX_NAMES, FLUX_OPTIONAL)
    out["iterations"] = ctx.zeros(torch.int32)
    wet = util.window(case["ocean"]["mask"], H, H, NX, NY, 0) != 0
    for name, scheme in SCHEMES.items():
        ctx.set_sea_ice_formulation(ice_params, ic.SeaIceInterfaceProperties(skin_temperature_scheme=scheme).to_params())
        for _ in range(3):
            ctx.compute_atmosphere_sea_ice_fluxes(st, ocean, atmos, out)
        ctx.sync()
        ms = events_ms(lambda: ctx.compute_atmosphere_sea_ice_fluxes(st, ocean, atmos, out), SOLVES)
        ctx.sync()
        its = util.window(out["iterations"].cpu().numpy(), H, H, NX, NY, 0)
        results[name]["solve_ms"] = round(ms, 4)
        results[name]["polar_surface"] = trips(its, wet)
    ctx.close()


def main():
    results = {name: {} for name in SCHEMES}
    step_workload(results)
    polar_solve(results)
    print(json.dumps(dict(grid=[NX, NY, H], warmup=WARMUP, steps=STEPS, solves=SOLVES, device=torch.cuda.get_device_name(0),
                          schemes=results)))


if __name__ == "__main__":
    main()
