"""Cost of a checkpoint on the coupled configuration of tools/coupled_step_probe.py (1440 x 560 and the 1440 x 140 slab, halo 7)
-> profiles/checkpoint_probe.json, printed as one JSON line.

    python tools/checkpoint_probe.py [--out PATH]

Registered: every array the coupled loop reads as state or writes (two ocean states and the mask, both exchange sets, the
interface, net, sea-ice and ice-ocean fluxes, the skin temperature, land, restoring, mean), the sixteen means of an OMIP
surface writer with its averager, and a 12-bin climatology of one field with its handle.  One process, HIP events on torch's
current stream — which IS the context's stream (FluxContext.use_torch_stream) —, the arms interleaved round by round and taken
in the opposite order every other round, median with min ... max of ROUNDS rounds:
  (a) stall: the time the STEPPING stream is held by one cf_checkpoint_capture — events around the call, so the upload of the
      tables AND the pack launch, not the launch alone — in the packed form with plain stores, in the packed form with streaming
      stores (COFLUX_CHECKPOINT_STORES, an experiment variable read when a handle is made; same bytes), and with
      CF_CHECKPOINT_DIRECT (the hash launch + one copy per section, all on the stepping stream).  The drain of the packed forms
      runs on the handle's stream;
  (b) cf_time_copy of the image's device bytes in the same process: the device's copy rate next to the rate the stall implies;
  (c) us per step of cf_time_steps_coupled (STEPS steps per call) with no checkpoint and with a packed drain of either store
      form in flight.
The rules, set beforehand.  The packed form stays the Checkpointer's default only if its median stall is below the direct
form's by more than the direct form's own min ... max spread, on both surfaces and with either store form
(`packed_stays_default`).  Streaming stores are used only if they measure no worse: they count as worse on a surface where
every round of theirs took longer than every round of the plain arm (`streaming_stores_worse`), and one such surface decides
for plain stores (`streaming_stores_kept`)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "climaocean.jl_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
os.environ.setdefault("COFLUX_EXPERIMENTS", "1")   # COFLUX_CHECKPOINT_STORES is an experiment variable of the library
import torch  # noqa: E402

from coflux import abi, synthetic as syn, interface_computations as ic  # noqa: E402
from coflux.runtime import EXCHANGE_NAMES, FLUX_NAMES, NET_NAMES, Checkpoint, FluxContext  # noqa: E402

H = 7
SURFACES = {"1440x560": (1440, 560, None, 0), "1440x140": (1440, 140, 560, 280)}   # nx, ny, ny_global, j_offset
ROUNDS, STEPS, WARMUP = 8, 50, 50
N_LEVELS, INC = 4, 1.0 / 9.0
PISTON = 1.0 / 6.0 / 86400.0
N_BINS, N_MEANS = 12, 16


def summary(rounds):
    return dict(median_us=round(statistics.median(rounds), 3), min_us=round(min(rounds), 3), max_us=round(max(rounds), 3),
                rounds_us=[round(r, 3) for r in rounds])


def events_us(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b)


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
    iop = ctx.default_ice_ocean_params(time_step=1200.0, top_cell_thickness=10.0)
    target = ctx.to_device(o0["S"] + 0.1)
    out = dict(sets=[ctx.field_set(EXCHANGE_NAMES) for _ in range(2)], fl=ctx.field_set(FLUX_NAMES), net=ctx.field_set(NET_NAMES[:5]),
               ai=ctx.field_set(tuple(k for k in FLUX_NAMES if k != "temperature")), skin=ctx.to_device(si["top_temperature"]),
               net_ice=ctx.field_set(("top_heat", "bottom_heat")), iof=ctx.field_set(("interface_heat", "salt_flux", "frazil_heat")),
               land=ctx.zeros(), restoring=ctx.zeros(), mean=torch.zeros(1, dtype=torch.float64, device=ctx.device))
    sch = ctx.make_schedule(states, out["sets"], first_level=0, time_fraction=0.0, time_fraction_increment=INC, pipeline=abi.PIPELINE_CONTINUING)
    block = ctx.make_coupled_step([ice_state], out["skin"], out["ai"], out["net_ice"], friver=land["friver"], licalvf=land["licalvf"],
                                  land_out=out["land"], land_first_level=1, land_time_fraction=0.8, land_time_fraction_increment=INC,
                                  ice_ocean_params=iop, ice_ocean_fluxes=out["iof"], piston_velocity=PISTON, target=target,
                                  restoring_out=out["restoring"], normalize=True, mean_out=out["mean"])
    step = [0]

    def steps():
        ctx.time_steps_coupled(step[0], STEPS, sch, src, w, out["fl"], out["net"], stresses, block)
        step[0] += STEPS

    # the writers' state: sixteen means with their averager, one field's total and twelve bins with their climatology
    sources = (list(out["net"].values()) + list(out["fl"].values()) + list(out["ai"].values()))[:N_MEANS]
    means = [ctx.zeros() for _ in sources]
    averager = ctx.average(sources, means)
    total, bins = ctx.zeros(), torch.zeros((N_BINS,) + tuple(ctx.shape), dtype=torch.float64, device=ctx.device)
    climatology = ctx.climatology([out["net"]["T"]], [total], [bins], N_BINS)

    def register(cp):
        for s, o in enumerate(states):
            for k in ("T", "S", "u", "v"):
                cp.add_array(f"ocean{s}.{k}", o[k])
        cp.add_array("mask", states[0]["mask"])
        for s, d in enumerate(out["sets"]):
            for k, t in d.items():
                cp.add_array(f"set{s}.{k}", t)
        for group in ("fl", "net", "ai", "net_ice", "iof"):
            for k, t in out[group].items():
                cp.add_array(f"{group}.{k}", t)
        for k in ("skin", "land", "restoring", "mean"):
            cp.add_array(k, out[k])
        for n, t in enumerate(means):
            cp.add_array(f"mean{n}", t)
        cp.add_array("climatology.total", total)
        cp.add_array("climatology.bins", bins)
        cp.add("averager", averager)
        cp.add("climatology", climatology)
        return cp

    def with_stores(form, **kw):
        os.environ["COFLUX_CHECKPOINT_STORES"] = form      # read by cf_checkpoint_create
        try:
            return register(Checkpoint(ctx, **kw))
        finally:
            del os.environ["COFLUX_CHECKPOINT_STORES"]

    forms = dict(packed_plain=with_stores("plain"), packed_streaming=with_stores("streaming"), direct=with_stores("plain", direct=True))
    for _ in range(WARMUP // STEPS + 1):
        steps()
    averager.collect(1.0)
    climatology.collect(3, 1.0)
    images = {}
    for name, cp in forms.items():      # warm-up: buffers are sized here
        cp.capture()
        images[name] = cp.wait()
    assert images["packed_plain"] == images["direct"] == images["packed_streaming"]
    image_bytes = len(images["packed_plain"])
    device_bytes = sum(t.numel() * t.element_size() for t in forms["direct"]._keep if isinstance(t, torch.Tensor))
    del images
    stall = {k: [] for k in forms}
    step_arms = ("no_checkpoint", "drain_in_flight_plain", "drain_in_flight_streaming")
    step_us = {k: [] for k in step_arms}
    copy_us = []

    def step_arm(name):
        ctx.sync()
        cp = forms["packed_" + name.rsplit("_", 1)[1]] if name != "no_checkpoint" else None
        if cp is not None:
            cp.capture()
        step_us[name].append(events_us(steps) / STEPS)
        if cp is not None:
            cp.wait(copy=False)

    for r in range(ROUNDS):             # interleaved; every other round in the opposite order
        flip = (lambda x: list(reversed(list(x)))) if r % 2 else list
        for name in flip(forms):
            stall[name].append(events_us(forms[name].capture))
            forms[name].wait(copy=False)
        copy_us.append(1e3 * ctx.time_copy(device_bytes // 8 * 8, 5))
        for name in flip(step_arms):
            step_arm(name)
        ctx.sync()
    ctx.discard_prefetched_atmosphere_state()
    med = statistics.median
    result = dict(image_bytes=image_bytes, device_bytes=device_bytes, extra_device_memory_packed_bytes=image_bytes, sections=len(forms["direct"].names),
                  stall={k: summary(v) for k, v in stall.items()}, copy_same_bytes=summary(copy_us),
                  stall_implied_GB_per_s={k: round(2e-3 * device_bytes / med(stall[k]), 1) for k in ("packed_plain", "packed_streaming")},
                  copy_GB_per_s=round(2e-3 * device_bytes / med(copy_us), 1),
                  stall_implied_fraction_of_copy={k: round(med(copy_us) / med(stall[k]), 3) for k in ("packed_plain", "packed_streaming")},
                  step_us=dict({k: summary(v) for k, v in step_us.items()}, steps_per_call=STEPS))
    d = result["stall"]["direct"]
    result["packed_wins"] = all(d["median_us"] - result["stall"][k]["median_us"] > d["max_us"] - d["min_us"] for k in ("packed_plain", "packed_streaming"))
    result["streaming_stores_worse"] = bool(result["stall"]["packed_streaming"]["min_us"] > result["stall"]["packed_plain"]["max_us"])
    for cp in forms.values():
        cp.close()
    averager.close()
    climatology.close()
    ctx.close()
    torch.cuda.empty_cache()
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "checkpoint_probe.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("checkpoint_probe needs a HIP device: nothing is measured without one")
    out = dict(halo=H, rounds=ROUNDS, steps_per_call=STEPS, tile_bytes=16384, device=torch.cuda.get_device_name(0),
               surfaces={name: surface(*shape) for name, shape in SURFACES.items()})
    out["packed_stays_default"] = all(s["packed_wins"] for s in out["surfaces"].values())
    out["streaming_stores_kept"] = not any(s["streaming_stores_worse"] for s in out["surfaces"].values())
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
