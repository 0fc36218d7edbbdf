"""GPU tests of the time averages accumulated on the device (include/coflux.h: cf_average_*, cf_attach_average; the host
mirror's AveragedTimeInterval / SurfaceFluxAverages).  The kernel's recurrence is restated here in numpy and held to it bit
for bit; the stepping loop with an attached averager is held to the host-driven update_state + collect loop bit for bit;
run!(simulation) with an averaged writer is held to the weighted mean of a host loop's per-step fields."""
import ctypes as C

import numpy as np
import pytest
import torch

from coflux import abi
from coflux import interface_computations as ic
from coflux import models as cm
from coflux import synthetic as syn
from coflux.runtime import CofluxError, FLUX_NAMES, NET_NAMES, EXCHANGE_NAMES, FluxContext
from test_layout_footprint import Geom, footprint
from test_steps import INC, _setup

pytestmark = pytest.mark.gpu


def restated(samples):
    """the kernel's recurrence in numpy: [(f, w)] → m; the first sample stores, each later one m·c_prev + f·c_new"""
    m, total = None, 0.0
    for f, w in samples:
        cur = total + w
        m = f.copy() if m is None else m * (total / cur) + f * (w / cur)
        total = cur
    return m


def interior(a, nx, ny, hx, hy):
    return a[hy:hy + ny, hx:hx + nx]


@pytest.mark.parametrize("nfields", [1, 16])
def test_collect_is_the_restated_recurrence_bit_for_bit(nfields):
    nx, ny, hx, hy = 77, 23, 3, 2
    ctx = FluxContext(nx, ny, hx, hy, ic.flux_params(), ring=1)
    rng = np.random.default_rng(nfields)
    sources = [ctx.zeros() for _ in range(nfields)]
    means = [torch.full(ctx.shape, float("nan"), dtype=torch.float64, device="cuda") for _ in range(nfields)]
    avg = ctx.average(sources, means)
    windows = ([0.7, 1.3, 2.0, 0.25, 3.1, 1.0], [1e-3, 5.0, 0.5, 2.5, 7.0])   # a reset in between
    for weights in windows:
        avg.reset()
        assert avg.weight() == (0.0, 0)
        samples = [[] for _ in range(nfields)]
        for w in weights:
            for f in range(nfields):
                a = rng.standard_normal(ctx.shape) * 10.0 ** rng.integers(-3, 4) + rng.integers(-5, 5)
                sources[f].copy_(torch.from_numpy(a))
                samples[f].append((interior(a, nx, ny, hx, hy), w))
            avg.collect(w)
        ctx.sync()
        total, n = avg.weight()
        assert n == len(weights) and total == pytest.approx(sum(weights), rel=1e-15)
        for f in range(nfields):
            got = means[f].cpu().numpy()
            want = restated(samples[f])
            assert np.array_equal(interior(got, nx, ny, hx, hy).view(np.int64), want.view(np.int64)), f
            exact = sum(x * w for x, w in samples[f]) / sum(w for _, w in samples[f])
            scale = max(np.abs(x).max() for x, _ in samples[f])
            assert np.abs(interior(got, nx, ny, hx, hy) - exact).max() <= 1e-13 * scale, f
            halo = np.ones(ctx.shape, bool)
            interior(halo, nx, ny, hx, hy)[:] = False
            assert np.isnan(got[halo]).all(), f"field {f}: a halo cell of the mean was written"
    avg.close()
    ctx.close()


def _average_call(mem, G, weights):
    ctx = FluxContext(G.nx, G.ny, G.hx, G.hy, ic.flux_params(), ring=0)
    rng = np.random.default_rng(3)
    sources = [mem.inp(f"f{k}", rng.standard_normal(G.shape) + k, read=G.interior) for k in range(3)]
    means = [mem.out(f"m{k}", G.shape, G.interior) for k in range(3)]
    avg = ctx.average(sources, means)

    def run():
        for w in weights:
            avg.collect(w)

    out = mem.run(run, ctx)
    avg.close()
    ctx.close()
    return out


@pytest.mark.parametrize("halo", [(2, 7), (7, 2), (1, 1)])
def test_collect_footprint_under_poisons_unequal_halos_and_odd_offsets(halo):
    """Sources poisoned outside I, means at odd element offsets inside guarded buffers with sentinel halos: the means' halos,
    the guards and every source cell keep their bits, and the write set equals the plain call's."""
    G = Geom(halo[0], halo[1], 0, nx=77, ny=23)
    res = footprint(_average_call, G, [0.5, 2.0, 1.25, 3.0])
    for k in range(3):
        assert np.isfinite(interior(res[f"m{k}"], G.nx, G.ny, G.hx, G.hy)).all()


OUTS = ("sensible_heat", "latent_heat")


def _averaged(ctx, fl, net):
    srcs = [net[k] for k in ("u", "v", "T", "S")] + [fl[k] for k in OUTS]
    means = [ctx.zeros() for _ in srcs]
    return ctx.average(srcs, means), means


def _host_reference(ctx, states, src, w, n, stride, step_weight, n_levels=4):
    atmos, fl, net = ctx.field_set(EXCHANGE_NAMES), ctx.field_set(FLUX_NAMES), ctx.field_set(NET_NAMES)
    avg, means = _averaged(ctx, fl, net)
    for s in range(n):
        tot = s * INC
        l1 = int(tot) % n_levels
        ctx.update_state(src, w, states[s % 2], atmos, fl, net, level1=l1, level2=(l1 + 1) % n_levels, time_fraction=tot - int(tot))
        if (s + 1) % stride == 0:
            avg.collect(stride * step_weight)
    ctx.sync()
    return fl, net, means, avg


def _stepped(ctx, states, src, w, calls, pipeline, attach=None):
    sets = [ctx.field_set(EXCHANGE_NAMES) for _ in range(2 if pipeline else 1)]
    fl, net = ctx.field_set(FLUX_NAMES), ctx.field_set(NET_NAMES)
    sched = ctx.make_schedule(states, sets, first_level=0, time_fraction=0.0, time_fraction_increment=INC, pipeline=pipeline)
    avg = means = None
    if attach is not None:
        avg, means = _averaged(ctx, fl, net)
        ctx.attach_average(avg, *attach)
    for first, count in calls:
        ctx.time_steps(first, count, sched, src, w, fl, net)
    ctx.sync()
    ctx.attach_average(None)
    return fl, net, means, avg


@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("pipeline", [False, True, "merged", "tail"])
def test_time_steps_with_an_attached_averager_equals_the_host_loop(pipeline, stride):
    n, step_weight = 13, 1200.0
    ctx, states, src, w, _ = _setup()
    rfl, rnet, rmeans, ravg = _host_reference(ctx, states, src, w, n, stride, step_weight)
    if pipeline in ("merged", "tail"):
        ctx.set_option(abi.OPT_MERGED_PREFETCH, 1 if pipeline == "merged" else 2)
    plain_fl, plain_net, _, _ = _stepped(ctx, states, src, w, [(0, n)], bool(pipeline))
    fl, net, means, avg = _stepped(ctx, states, src, w, [(0, 5), (5, n - 5)], bool(pipeline), attach=(stride, step_weight))
    for k in FLUX_NAMES:
        assert torch.equal(fl[k], plain_fl[k]) and torch.equal(fl[k], rfl[k]), k
    for k in NET_NAMES:
        assert torch.equal(net[k], plain_net[k]) and torch.equal(net[k], rnet[k]), k
    for k, (m, r) in enumerate(zip(means, rmeans)):
        assert torch.equal(m.view(torch.int64), r.view(torch.int64)), k
    assert avg.weight() == ravg.weight() == ((n // stride) * stride * step_weight, n // stride)
    ctx.close()


def test_continuing_calls_collect_what_one_call_collects():
    ctx, states, src, w, _ = _setup()
    ctx.set_option(abi.OPT_MERGED_PREFETCH, 2)
    one = _stepped(ctx, states, src, w, [(0, 12)], abi.PIPELINE_CONTINUING, attach=(3, 600.0))
    ctx.discard_prefetched_atmosphere_state()
    three = _stepped(ctx, states, src, w, [(0, 4), (4, 3), (7, 5)], abi.PIPELINE_CONTINUING, attach=(3, 600.0))
    for a, b in zip(one[2], three[2]):
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    for k in NET_NAMES:
        assert torch.equal(one[1][k], three[1][k]), k
    assert one[3].weight() == three[3].weight() == (4 * 3 * 600.0, 4)
    ctx.close()


# ---- run!(simulation) with SurfaceFluxAverages ------------------------------------------------------------------------------
NX, NY, NZ, H = 90, 40, 10, 3
DT = 20 * cm.minutes


def _model(sea_ice):
    grid = cm.LatitudeLongitudeGrid(size=(NX, NY, NZ), halo=(H, H, H), latitude=(-70, 70), z=(-3000, 0))
    ocean = cm.ocean_simulation(grid)
    state = syn.ocean_state(NX, NY, H, H)
    cm.set_surface(ocean, T=state["T"], S=state["S"], u=state["u"], v=state["v"], mask=state["mask"])
    atmosphere = cm.JRA55PrescribedAtmosphere(syn.jra55_snapshots(4))
    if not sea_ice:
        return cm.OceanSeaIceModel(ocean, atmosphere=atmosphere)
    ice_np = syn.sea_ice_state(NX, NY, H, H)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to("cuda")  # noqa: E731
    si = cm.PrescribedSeaIce(concentration=dev(state["ice_concentration"]), interface_heat=dev(state["ice_interface_heat"]),
                             salt_flux=dev(state["ice_salt_flux"]), x_stress=dev(state["ice_x_stress"]),
                             y_stress=dev(state["ice_y_stress"]), thickness=dev(ice_np["thickness"]),
                             top_surface_temperature=dev(ice_np["top_temperature"]), u=dev(ice_np["u"]), v=dev(ice_np["v"]),
                             albedo=dev(ice_np["albedo"]))
    interfaces = cm.ComponentInterfaces(atmosphere, ocean, si, atmosphere_ocean_fluxes=ic.corrected_atmosphere_ocean_fluxes(),
                                        atmosphere_sea_ice_fluxes=ic.corrected_atmosphere_sea_ice_fluxes(),
                                        ocean_minimum_salinity=1.0)
    return cm.OceanSeaIceModel(ocean, si, atmosphere=atmosphere, interfaces=interfaces)


def _outputs(model, sea_ice):
    if not sea_ice:
        return None     # the OMIP default set
    itf = model.interfaces
    return dict(hfds=itf.net_fluxes.ocean.T, hfss=itf.atmosphere_ocean_interface.fluxes.sensible_heat,
                ice_top_heat=itf.net_fluxes.sea_ice.top_heat, ice_sensible_heat=itf.atmosphere_sea_ice_interface.fluxes.sensible_heat)


@pytest.mark.parametrize("sea_ice", [False, True])
def test_run_with_surface_flux_averages_matches_the_host_loop(sea_ice):
    """Two windows of 2 hours (6 steps of 20 minutes).  Ocean only: every step, the OMIP default outputs.  With sea ice: a
    1-hour window and stride 2, so window k collects iterations 6k − 2 (weight 20 min: since the window opened) and 6k
    (40 min), and the outputs include sea-ice fields."""
    if sea_ice:
        schedule, weights = cm.AveragedTimeInterval(2 * cm.hours, window=1 * cm.hours, stride=2), {4: 20, 6: 40, 10: 20, 12: 40}
    else:
        schedule, weights = cm.AveragedTimeInterval(2 * cm.hours), {n: 20 for n in range(1, 13)}
    # the host loop: time_step! by hand, every step's fields read back
    ref = _model(sea_ice)
    writer_ref = cm.SurfaceFluxAverages(ref, outputs=_outputs(ref, sea_ice), schedule=cm.AveragedTimeInterval(2 * cm.hours))
    per_step = {}
    for n in range(1, 13):
        cm.time_step(ref, DT)
        per_step[n] = {k: interior(v.cpu().numpy(), NX, NY, H, H).copy() for k, v in writer_ref.outputs.items()}
    ref.interfaces.context.close()

    model = _model(sea_ice)
    seen = []
    writer = cm.SurfaceFluxAverages(model, outputs=_outputs(model, sea_ice), schedule=schedule,
                                    on_window=lambda t_k, arrays: seen.append(t_k))
    if not sea_ice:
        assert list(writer.outputs) == ["tauuo", "tauvo", "hfds", "wfo", "hfss", "hfls"]
    sim = cm.Simulation(model, dt=DT, stop_iteration=12, output_writers={"surface": writer})
    cm.run(sim)
    assert seen == [7200.0, 14400.0] and [t for t, _ in writer.windows] == [7200.0, 14400.0]
    for k, (t_k, arrays) in enumerate(writer.windows):
        steps = [n for n in weights if 6 * k < n <= 6 * (k + 1)]
        for name, got in arrays.items():
            want = sum(per_step[n][name] * weights[n] for n in steps) / sum(weights[n] for n in steps)
            scale = max(np.abs(per_step[n][name]).max() for n in steps)
            assert got.shape == (NY, NX) and np.abs(got - want).max() <= 1e-12 * scale, (t_k, name)
    # the open window survives the end of run!
    sim.stop_iteration = 14
    cm.run(sim)
    assert len(writer.windows) == 2
    assert writer.averager.weight() == ((2 * DT, 2) if not sea_ice else (0.0, 0))
    model.interfaces.context.close()


def test_errors():
    ctx = FluxContext(40, 12, 2, 2, ic.flux_params(), ring=1)
    a, b = ctx.zeros(), ctx.zeros()
    with pytest.raises(CofluxError, match="overlaps source"):
        ctx.average([a], [a])
    buf = torch.zeros(2 * a.numel(), dtype=torch.float64, device="cuda")
    v0, v1 = buf[:a.numel()].view(ctx.shape), buf[17:17 + a.numel()].view(ctx.shape)
    with pytest.raises(CofluxError, match="overlap"):
        ctx.average([a, b], [v0, v1])
    with pytest.raises(CofluxError, match="0 fields"):
        ctx.average([], [])
    with pytest.raises(CofluxError, match="17 fields"):
        ctx.average([a] * 17, [ctx.zeros() for _ in range(17)])
    h = C.c_void_p()
    null = (C.c_void_p * 1)(None)
    assert ctx.lib.cf_average_create(ctx._h, 1, null, (C.c_void_p * 1)(b.data_ptr()), C.byref(h)) == -1 and not h.value   # CF_ERR_INVALID
    avg = ctx.average([a], [b])
    for w in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(CofluxError, match="weight"):
            avg.collect(w)
    assert avg.weight() == (0.0, 0)
    with pytest.raises(CofluxError, match="stride"):
        ctx.attach_average(avg, 0, 1.0)
    with pytest.raises(CofluxError, match="stride"):
        ctx.attach_average(avg, 1, 0.0)
    other = FluxContext(40, 12, 2, 2, ic.flux_params(), ring=1)
    with pytest.raises(CofluxError, match="another context"):
        other.attach_average(avg, 1, 1.0)
    other.close()
    ctx.close()
    # destroying an attached averager detaches it: cf_time_steps goes on as without one
    ctx, states, src, w, _ = _setup()
    plain = _stepped(ctx, states, src, w, [(0, 4)], False)
    fl, net = ctx.field_set(FLUX_NAMES), ctx.field_set(NET_NAMES)
    avg, _ = _averaged(ctx, fl, net)
    ctx.attach_average(avg, 1, 1.0)
    avg.close()
    sched = ctx.make_schedule(states, [ctx.field_set(EXCHANGE_NAMES)], time_fraction_increment=INC)
    ctx.time_steps(0, 4, sched, src, w, fl, net)
    ctx.sync()
    for k in NET_NAMES:
        assert torch.equal(net[k], plain[1][k]), k
    # an averager outlived by its context: every call fails, destroying it does not
    avg, _ = _averaged(ctx, fl, net)
    ctx.close()
    with pytest.raises(CofluxError, match="destroyed"):
        avg.collect(1.0)
    avg.close()
