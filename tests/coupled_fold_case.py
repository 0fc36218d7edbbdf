"""What the tests of the coupled loop on tripolar slabs share (tests/test_coupled_fold_world_of_one.py, test_coupled_fold_slabs.py):
tests/coupled_case.py's designed case with a snow field — thirteen exchanged fields per step and call: four ocean, six of the ice
state, two stresses, the skin temperature —, the host statement of what the fold must leave in every north halo row
(coflux.synthetic.fold_north with the triples of coflux.distributed.coupled_fold_plan), the naming NaNs, and the single-domain
tripolar reference run, made once per surface and never written to afterwards.

The reference run is CF_HALO_NONE with fold_north = 1: the library folds the four ocean rows by a launch of its own at every step,
and the north halo rows of the nine ice-side fields are folded on the host before upload."""
import functools

import numpy as np
import torch

import coupled_case as cc
from coflux import abi
from coflux import synthetic as syn
from coflux.distributed import coupled_fold_plan, slab_bounds

HX, HY, ROWS, STEPS = 4, 3, 2, 7      # halo_rows = ring + 1
OCEAN_FIELDS = ("T", "S", "u", "v")
ICE_FIELDS = ("concentration", "thickness", "snow_thickness", "u", "v", "albedo")
PATTERN = 0x7FF8000000000000
SEVEN = [(0, STEPS, abi.PIPELINE_WITHIN_CALL)]
FIVE_TWO = [(0, 5, abi.PIPELINE_CONTINUING), (5, 2, abi.PIPELINE_CONTINUING)]

_CALL, _STEP = coupled_fold_plan(OCEAN_FIELDS, ICE_FIELDS, ("x_stress", "y_stress", "skin_temperature"))
CONVENTION = {name: (location, sign) for exchange in _CALL + _STEP for name, location, sign in exchange}
assert len(CONVENTION) == 13


@functools.lru_cache(maxsize=None)
def global_case(nx, ny):
    """the designed case on the whole surface, plus snow; never written to"""
    case = dict(cc.build(nx, ny, HX, HY))
    i, j = syn.ocean_indices(nx, ny, HX, HY)
    case["snow"] = np.ascontiguousarray(0.3 * syn.uniform("hi", i, j, 9))      # (a stream of its own: not the thickness)
    return case


def _fold(a, nx, ny, name):
    location, sign = CONVENTION[name]
    return syn.fold_north(np.array(a), nx, ny, HX, HY, ROWS, location, sign)


@functools.lru_cache(maxsize=None)
def folded_case(nx, ny):
    """global_case with the north halo rows of the nine ice-side fields folded on the host (the ocean rows stay as they are: the
    reference run folds them on the device)"""
    g = global_case(nx, ny)
    f = lambda a, name: _fold(a, nx, ny, name)  # noqa: E731
    si = g["ice_state"]
    ice_state = dict(si, thickness=f(si["thickness"], "thickness"), u=f(si["u"], "ice_u"), v=f(si["v"], "ice_v"),
                     albedo=f(si["albedo"], "albedo"), top_temperature=f(si["top_temperature"], "skin_temperature"))
    return dict(g, ice_state=ice_state, concentrations=[f(c, "concentration") for c in g["concentrations"]],
                snow=f(g["snow"], "snow_thickness"), x_stress=f(g["x_stress"], "x_stress"), y_stress=f(g["y_stress"], "y_stress"))


def slab_case(nx, ny_global, rank, world):
    """rows [j0 − hy, j1 + hy) of every ocean-grid array of the (unfolded) global case; the sources are global"""
    g = global_case(nx, ny_global)
    j0, j1 = slab_bounds(ny_global, rank, world)
    rows = slice(j0, j1 + 2 * HY)
    cut = lambda a: np.ascontiguousarray(a[rows])  # noqa: E731
    w = dict(g["weights"])
    assert w["separable"]
    w["fj"], w["latitude"] = cut(w["fj"]), cut(w["latitude"])
    case = dict(nx=nx, ny=j1 - j0, hx=HX, hy=HY, oceans=[{k: cut(v) for k, v in o.items()} for o in g["oceans"]],
                ice_state={k: cut(v) for k, v in g["ice_state"].items()}, concentrations=[cut(c) for c in g["concentrations"]],
                x_stress=cut(g["x_stress"]), y_stress=cut(g["y_stress"]), weights=w, src=g["src"], land=g["land"], target=cut(g["target"]),
                area=cut(g["area"]), bottom_height=cut(g["bottom_height"]), snow=cut(g["snow"]))
    return j0, case


def make_rig(case):
    """test_coupled_steps.Rig on `case`, every ice state with the case's snow"""
    import test_coupled_steps as tcs
    rig = tcs.Rig(case, merged=2)
    snow = rig.ctx.to_device(case["snow"])
    for st in rig.ice_states:
        st["snow_thickness"] = snow
    return rig


def exchanged_fields(rig, out, nx, ny_global):
    """{name: (device tensor, the global host array it is a slab of with its north halo rows folded)} of the thirteen fields the
    coupled loop exchanges, every ocean and ice state counted: what a neighbour or the fold must deliver is known"""
    g = global_case(nx, ny_global)
    f = lambda a, name: _fold(a, nx, ny_global, name)  # noqa: E731
    fields = {}
    for n, (o, go) in enumerate(zip(rig.oceans, g["oceans"])):
        fields.update({f"ocean{n}.{k}": (o[k], f(go[k], k)) for k in OCEAN_FIELDS})
    for n, st in enumerate(rig.ice_states):
        fields[f"ice{n}.concentration"] = (st["concentration"], f(g["concentrations"][n], "concentration"))
    st = rig.ice_states[0]
    fields["ice.thickness"] = (st["thickness"], f(g["ice_state"]["thickness"], "thickness"))
    fields["ice.snow_thickness"] = (st["snow_thickness"], f(g["snow"], "snow_thickness"))
    fields["ice.u"] = (st["u"], f(g["ice_state"]["u"], "ice_u"))
    fields["ice.v"] = (st["v"], f(g["ice_state"]["v"], "ice_v"))
    fields["ice.albedo"] = (st["albedo"], f(g["ice_state"]["albedo"], "albedo"))
    fields["x_stress"], fields["y_stress"] = (rig.tx, f(g["x_stress"], "x_stress")), (rig.ty, f(g["y_stress"], "y_stress"))
    fields["skin"] = (out.skin, f(g["ice_state"]["top_temperature"], "skin_temperature"))
    return fields


def stamp(fields, rank, world, ny):
    """a NaN that names rank, field and row into the halo rows towards a neighbour and, on the last rank, towards the fold"""
    for f, (t, _g) in enumerate(fields.values()):
        b = t.view(torch.int64)
        for r in range(ROWS):
            if rank > 0:
                b[HY - 1 - r, :] = PATTERN | (rank << 40) | (f << 8) | r
            b[HY + ny + r, :] = PATTERN | (rank << 40) | (f << 8) | 0x80 | r
    torch.cuda.synchronize()


def undelivered(fields, rank, j0, ny, skip=()):
    """the exchanged fields whose halo rows towards a neighbour or the fold do not hold the expected bits over the full width.  (The
    skin temperature's ring rows are results by then: its outer exchanged row is compared, with the initial field — in a run of
    one call.)"""
    bad = []
    for name, (t, g) in fields.items():
        if name in skip:
            continue
        got = t.cpu().numpy().view(np.int64)
        want = g[j0:j0 + ny + 2 * HY].view(np.int64)
        skin = 1 if name == "skin" else 0
        sides = ([slice(HY - ROWS, HY - skin)] if rank > 0 else []) + [slice(HY + ny + skin, HY + ny + ROWS)]
        if any(not np.array_equal(got[s], want[s]) for s in sides):
            bad.append(name)
    return bad


def run(rig, out, calls, backend, fold, between=None):
    """cf_time_steps_coupled over `calls` with the exact normalisation; `between`: called before every call but the first, after
    a cf_sync"""
    import test_coupled_steps as tcs
    for n, (first, steps, pipeline) in enumerate(calls):
        if n and between is not None:
            rig.ctx.sync()
            between()
        sch, block = tcs.coupled_arguments(rig, out, pipeline=pipeline, normalize="exact")
        sch.halo_backend, sch.halo_rows = backend, ROWS if backend != abi.HALO_NONE else 0
        sch.fold_north = 1 if fold else 0
        rig.ctx.time_steps_coupled(first, steps, sch, rig.src, rig.w, out.fl, out.net, rig.stresses, block)
    rig.ctx.sync()
    rig.ctx.discard_prefetched_atmosphere_state()


def output_fields(out):
    """the arrays the slabs are compared in"""
    fields = {"land": out.land, "restoring": out.restoring, "skin": out.skin}
    for name, d in (("fl", out.fl), ("ai", out.ai), ("net", out.net), ("net_ice", out.net_ice), ("iof", out.iof)):
        fields.update({f"{name}.{k}": v for k, v in d.items()})
    return fields


def counters(ctx):
    return ctx.peer_halo_stats() + ctx.fold_counts()


def grown(before, after):
    return tuple(a - b for a, b in zip(after, before))


_SINGLE = {}


def single_domain(nx, ny):
    """the seven pipelined steps on the whole tripolar surface in one context, once per surface: dict(bits — whole guarded
    buffers —, fields, mean, grown — how (exchanges, in solver launch, fold launches, exchanges with a fold) grew)"""
    import test_coupled_steps as tcs
    key = (nx, ny)
    if key not in _SINGLE:
        rig = make_rig(folded_case(nx, ny))
        out = tcs.Outputs(rig)
        before = counters(rig.ctx)
        run(rig, out, SEVEN, abi.HALO_NONE, True)
        _SINGLE[key] = dict(bits={k: v.cpu() for k, v in out.bits().items()}, fields={k: v.cpu().numpy() for k, v in output_fields(out).items()},
                            mean=float(out.mean[0]), grown=grown(before, counters(rig.ctx)))
        rig.close()
    return _SINGLE[key]
