"""GPU tests of the area-weighted surface integrals and their time series (include/coflux.h: cf_integrals_*,
cf_attach_integrals; the host mirror's SurfaceIntegrals writer and its presets).

Values are held to math.fsum over the selected cells within the worst-case bound of a sum of n terms in ANY order,
(n + 8) · 2⁻⁵³ · fsum(|A·x|): n − 1 rounded additions, at most two rounded products per term on the device and two in the
reference's own terms; the second-order part is n² · 2⁻¹⁰⁶.  The bound is derived, not measured; each test prints the worst
ratio error / bound it saw.  Bits are held across halo widths, odd-offset views, the number of workgroups, repeated
collections, the stepping loop against the host loop, split calls and an attached averager."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import util
from coflux import abi
from coflux import interface_computations as ic
from coflux import models as cm
from coflux.runtime import CofluxError, EXCHANGE_NAMES, FLUX_NAMES, NET_NAMES, FluxContext
from test_layout_footprint import Geom, footprint
from test_steps import INC, _setup
from test_time_average import DT, H, NX, NY, _model, interior

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
THRESHOLD = 0.15
KINDS = ("one", "field", "product", "above")


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def make_data(nx, ny, seed=0):
    """interior arrays (ny, nx): fields, area, wet, region.  h, c > 0; s signed; g is only ever named with region bit 1;
    some c are exactly the threshold; bit 7 is set nowhere; some cells are in no region at all."""
    rng = np.random.default_rng(seed)
    c = rng.random((ny, nx))
    c[rng.random((ny, nx)) < 0.1] = THRESHOLD
    d = dict(h=np.exp(rng.standard_normal((ny, nx))), c=c, s=rng.standard_normal((ny, nx)) * 300.0,
             g=1.0 + rng.random((ny, nx)))
    area = (1.0 + rng.random((ny, nx))) * 4e8
    wet = (rng.random((ny, nx)) < 0.8).astype(np.uint8)
    region = rng.integers(0, 128, (ny, nx)).astype(np.uint8)
    region[rng.random((ny, nx)) < 0.05] = 0
    return d, area, wet, region


def entry_specs(n, kind=None):
    """n entries (kind, a, b, threshold, bit) by field NAME; one kind throughout when `kind` is given"""
    pool = [("one", None, None, 0.0, 0), ("field", "c", None, 0.0, 1), ("product", "h", "c", 0.0, 1), ("above", "c", None, THRESHOLD, 1),
            ("field", "s", None, 0.0, 0), ("product", "s", "s", 0.0, 2), ("one", None, None, 0.0, 7), ("field", "g", None, 0.0, 1),
            ("product", "g", "h", 0.0, 1), ("above", "s", None, 0.0, 3), ("field", "h", None, 0.0, 7), ("one", None, None, 0.0, 4)]
    if kind is not None:
        pool = [p for p in pool if p[0] == kind]
    specs = [pool[k % len(pool)] for k in range(n)]
    return [(k, a, b, t, (bit + q // len(pool)) % 8 if a != "g" and bit != 7 else bit) for q, (k, a, b, t, bit) in enumerate(specs)]


def embed(a, hx, hy, fill):
    ny, nx = a.shape
    g = np.full((ny + 2 * hy, nx + 2 * hx), fill, dtype=a.dtype)
    g[hy:hy + ny, hx:hx + nx] = a
    return g


def poisoned(d, area, wet, region):
    """NaN in every land cell and every cell that is in no region, of every field and of the area; g also wherever bit 1 is
    not set (out of its entries' region).  The halos get NaN in embed()."""
    dead = (wet == 0) | (region == 0)
    out = {k: np.where(dead | ((region & 2) == 0 if k == "g" else False), np.nan, v) for k, v in d.items()}
    return out, np.where(dead, np.nan, area)


def reference(specs, d, area, wet, region):
    """[(fsum(A·x), bound)] over the selected cells, from the clean arrays"""
    out = []
    for kind, a, b, thr, bit in specs:
        sel = (wet != 0) & ((region >> bit) & 1 != 0)
        if kind == "one":
            x = np.ones_like(area)
        elif kind == "field":
            x = d[a]
        elif kind == "product":
            x = d[a] * d[b]
        else:
            x = (d[a] > thr).astype(np.float64)
        terms = (area * x)[sel]
        out.append((math.fsum(terms.tolist()), (terms.size + 8) * EPS * math.fsum(np.abs(terms).tolist()), terms.size))
    return out


def device_integrator(ctx, specs, dev, **kw):
    return ctx.integrals([(k, dev.get(a), dev.get(b), t, bit) for k, a, b, t, bit in specs], **kw)


def check_values(got, ref, what):
    worst = 0.0
    for e, (g, (want, bound, n)) in enumerate(zip(got, ref)):
        if n == 0:
            assert g == 0.0 and not math.copysign(1.0, g) < 0, (what, e, g)
            continue
        err = abs(g - want)
        worst = max(worst, err / bound if bound > 0 else (0.0 if err == 0 else np.inf))
        assert err <= bound, (what, e, g, want, err, bound)
    print(f"{what}: worst error / bound = {worst:.3e}")
    return worst


CASES = [(1, k) for k in KINDS] + [(12, None), (32, None)]


@pytest.mark.parametrize("n_entries,kind", CASES)
@pytest.mark.parametrize("size", [(77, 23, 3, 2), (1440, 560, 7, 7)])
def test_values_against_fsum(size, n_entries, kind):
    nx, ny, hx, hy = size
    d, area, wet, region = make_data(nx, ny, seed=n_entries)
    specs = entry_specs(n_entries, kind)
    ref = reference(specs, d, area, wet, region)
    assert n_entries == 1 or any(n == 0 for _, _, n in ref), "an entry with an empty region is part of the case"
    pd, parea = poisoned(d, area, wet, region)
    ctx = FluxContext(nx, ny, hx, hy, ic.flux_params(), ring=0)
    dev = {k: ctx.to_device(embed(v, hx, hy, np.nan)) for k, v in pd.items()}
    q = device_integrator(ctx, specs, dev, area=ctx.to_device(embed(parea, hx, hy, np.nan)), mask=ctx.to_device(embed(wet, hx, hy, 1)),
                          region=ctx.to_device(embed(region, hx, hy, 0xFF)), capacity=2)
    q.collect(1.5)
    q.collect(2.5)
    values, times = q.read()
    assert values.shape == (2, n_entries) and list(times) == [1.5, 2.5]
    assert np.array_equal(bits(values[0]), bits(values[1])), "a second collection of unchanged inputs"
    check_values(values[0], ref, f"{nx}x{ny}, {n_entries} entries {kind or 'mixed'}")
    if kind == "above":   # cells at exactly the threshold do not count: the extent is the area of c > threshold alone
        sel = (wet != 0) & ((region >> specs[0][4]) & 1 != 0)
        assert (d["c"][sel] == THRESHOLD).any()
        with_equal = math.fsum(area[sel & (d["c"] >= THRESHOLD)].tolist())
        assert abs(values[0][0] - with_equal) > 1e3 * ref[0][1]
    q.close()
    ctx.close()


def test_defaults_no_area_no_mask_no_region():
    nx, ny, hx, hy = 77, 23, 3, 2
    d, _, _, _ = make_data(nx, ny, seed=5)
    ctx = FluxContext(nx, ny, hx, hy, ic.flux_params(), ring=0)
    dev = {k: ctx.to_device(embed(v, hx, hy, np.nan)) for k, v in d.items()}
    specs = [("one", None, None, 0.0, 0), ("field", "s", None, 0.0, 0), ("one", None, None, 0.0, 1), ("product", "h", "c", 0.0, 0)]
    q = device_integrator(ctx, specs, dev, capacity=1)
    q.collect()
    got = q.read()[0][0]
    ones, everywhere = np.ones((ny, nx)), np.ones((ny, nx), np.uint8)
    ref = reference(specs, d, ones, everywhere, everywhere)
    assert got[0] == nx * ny and got[2] == 0.0
    check_values(got, ref, "no weights")
    q.close()
    ctx.close()


# ---- bits ------------------------------------------------------------------------------------------------------------------
def _record(nx, ny, hx, hy, specs, pd, parea, wet, region, views=False, max_workgroups=0):
    ctx = FluxContext(nx, ny, hx, hy, ic.flux_params(), ring=0)
    shape = (ny + 2 * hy, nx + 2 * hx)
    n = [0]

    def put(a, tdtype, fill):
        t = torch.from_numpy(np.ascontiguousarray(a))
        if not views:
            return t.cuda()
        n[0] += 1
        v = util.guarded(shape, tdtype, offset=(1, 3, 5)[n[0] % 3], guard=64, fill=fill)
        v.copy_(t)
        return v

    dev = {k: put(embed(v, hx, hy, np.nan), torch.float64, float("nan")) for k, v in pd.items()}
    q = device_integrator(ctx, specs, dev, area=put(embed(parea, hx, hy, np.nan), torch.float64, float("nan")),
                          mask=put(embed(wet, hx, hy, 1), torch.uint8, 1), region=put(embed(region, hx, hy, 0xFF), torch.uint8, 0xFF),
                          capacity=1, max_workgroups=max_workgroups)
    q.collect()
    rec = q.read()[0][0].copy()
    q.close()
    ctx.close()
    return rec


@pytest.mark.parametrize("size", [(77, 23), (130, 40)])
def test_bits_do_not_depend_on_halos_offsets_or_workgroups(size):
    nx, ny = size
    d, area, wet, region = make_data(nx, ny, seed=11)
    specs = entry_specs(12)
    pd, parea = poisoned(d, area, wet, region)
    base = _record(nx, ny, 1, 1, specs, pd, parea, wet, region)
    check_values(base, reference(specs, d, area, wet, region), f"{nx}x{ny} halo (1, 1)")
    for hx, hy in ((2, 7), (7, 2), (4, 4)):
        for views in (False, True):
            got = _record(nx, ny, hx, hy, specs, pd, parea, wet, region, views=views)
            assert np.array_equal(bits(got), bits(base)), (hx, hy, views, got, base)
    for cap in (1, 3, 100000):
        got = _record(nx, ny, 2, 7, specs, pd, parea, wet, region, max_workgroups=cap)
        assert np.array_equal(bits(got), bits(base)), cap


# ---- the stepping loop -----------------------------------------------------------------------------------------------------
def _step_integrator(ctx, fl, net, states, capacity=64):
    (ny2, nx2) = ctx.shape
    rng = np.random.default_rng(2)
    area = ctx.to_device((1.0 + rng.random(ctx.shape)) * 1e8)
    phi = np.broadcast_to(np.linspace(-60, 60, ny2)[:, None], ctx.shape)
    region = ctx.to_device((1 + 2 * (phi > 0) + 4 * (phi < 0)).astype(np.uint8))
    entries = [("one", None, None, 0.0, 0), ("field", net["T"], None, 0.0, 0), ("product", fl["sensible_heat"], fl["latent_heat"], 0.0, 1),
               ("above", net["S"], None, 0.0, 2), ("field", fl["latent_heat"], None, 0.0, 2), ("product", net["u"], net["u"], 0.0, 0)]
    return ctx.integrals(entries, area=area, mask=states[0]["mask"], region=region, capacity=capacity)


def _host_loop(ctx, states, src, w, n, stride, n_levels=4):
    atmos, fl, net = ctx.field_set(EXCHANGE_NAMES), ctx.field_set(FLUX_NAMES), ctx.field_set(NET_NAMES)
    q = _step_integrator(ctx, fl, net, states)
    for s in range(n):
        tot = s * INC
        l1 = int(tot) % n_levels
        ctx.update_state(src, w, states[s % 2], atmos, fl, net, level1=l1, level2=(l1 + 1) % n_levels, time_fraction=tot - int(tot))
        if (s + 1) % stride == 0:
            q.collect(100.0 + (s + 1) * 1200.0)
    return fl, net, q.read()


def _stepped(ctx, states, src, w, calls, pipeline, stride=None, averager=False):
    sets = [ctx.field_set(EXCHANGE_NAMES) for _ in range(2 if pipeline else 1)]
    fl, net = ctx.field_set(FLUX_NAMES), ctx.field_set(NET_NAMES)
    sched = ctx.make_schedule(states, sets, first_level=0, time_fraction=0.0, time_fraction_increment=INC, pipeline=pipeline)
    q = avg = None
    if stride is not None:
        q = _step_integrator(ctx, fl, net, states)
        ctx.attach_integrals(q, stride, 100.0, 1200.0)
    if averager:
        avg = ctx.average([net["T"], fl["latent_heat"]], [ctx.zeros(), ctx.zeros()])
        ctx.attach_average(avg, 2, 1200.0)
    for first, count in calls:
        ctx.time_steps(first, count, sched, src, w, fl, net)
    ctx.attach_integrals(None)
    ctx.attach_average(None)
    return fl, net, (q.read() if q is not None else None)


@pytest.mark.parametrize("pipeline", [False, True, "merged", "tail"])
def test_time_steps_with_an_attached_integrator_equals_the_host_loop(pipeline):
    n = 13
    ctx, states, src, w, _ = _setup()
    rfl, rnet, (r1, t1) = _host_loop(ctx, states, src, w, n, 1)
    _, _, (r3, t3) = _host_loop(ctx, states, src, w, n, 3)
    assert r1.shape == (13, 6) and r3.shape == (4, 6) and list(t3) == [100.0 + k * 1200.0 for k in (3, 6, 9, 12)]
    assert np.array_equal(bits(r3), bits(r1[2::3])), "stride 3 collects what stride 1 collects at the same steps"
    assert np.isfinite(r1).all() and (r1[:, 0] > 0).all() and (r1[:, 1] != 0).all() and (r1[:, 5] > 0).all()
    if pipeline in ("merged", "tail"):
        ctx.set_option(abi.OPT_MERGED_PREFETCH, 1 if pipeline == "merged" else 2)
    plain_fl, plain_net, _ = _stepped(ctx, states, src, w, [(0, n)], bool(pipeline))
    for stride, (want, times) in ((1, (r1, t1)), (3, (r3, t3))):
        fl, net, (got, got_t) = _stepped(ctx, states, src, w, [(0, 5), (5, n - 5)], bool(pipeline), stride=stride)
        assert np.array_equal(bits(got), bits(want)) and np.array_equal(got_t, times), stride
        for k in FLUX_NAMES:
            assert torch.equal(fl[k], plain_fl[k]) and torch.equal(fl[k], rfl[k]), k
        for k in NET_NAMES:
            assert torch.equal(net[k], plain_net[k]) and torch.equal(net[k], rnet[k]), k
    fl, net, (got, _) = _stepped(ctx, states, src, w, [(0, n)], bool(pipeline), stride=1, averager=True)
    assert np.array_equal(bits(got), bits(r1)), "with an averager attached next to it"
    for k in NET_NAMES:
        assert torch.equal(net[k], plain_net[k]), k
    ctx.close()


def test_continuing_calls_yield_the_records_of_one_call():
    ctx, states, src, w, _ = _setup()
    ctx.set_option(abi.OPT_MERGED_PREFETCH, 2)
    one = _stepped(ctx, states, src, w, [(0, 12)], abi.PIPELINE_CONTINUING, stride=2)
    ctx.discard_prefetched_atmosphere_state()
    three = _stepped(ctx, states, src, w, [(0, 4), (4, 3), (7, 5)], abi.PIPELINE_CONTINUING, stride=2)
    assert one[2][0].shape == (6, 6)
    assert np.array_equal(bits(one[2][0]), bits(three[2][0])) and np.array_equal(one[2][1], three[2][1])
    for k in NET_NAMES:
        assert torch.equal(one[1][k], three[1][k]), k
    ctx.close()


# ---- footprint ---------------------------------------------------------------------------------------------------------------
_seen = []


def _integrals_call(mem, G):
    ctx = FluxContext(G.nx, G.ny, G.hx, G.hy, ic.flux_params(), ring=0)
    d, area, wet, region = make_data(G.nx, G.ny, seed=7)
    wide = lambda a, fill: embed(a, G.hx, G.hy, fill)  # noqa: E731
    dev = {k: mem.inp(k, wide(v, 1.0), read=G.interior) for k, v in d.items()}
    q = device_integrator(ctx, entry_specs(12), dev, area=mem.inp("area", wide(area, 1.0), read=G.interior),
                          mask=mem.inp("mask", wide(wet, 1), read=G.interior), region=mem.inp("region", wide(region, 0), read=G.interior),
                          capacity=2)

    def run():
        q.collect()
        q.collect()

    out = mem.run(run, ctx)
    _seen.append(q.read()[0])
    q.close()
    ctx.close()
    return out


@pytest.mark.parametrize("halo", [(2, 7), (7, 2), (1, 1)])
def test_collect_reads_the_interior_only_and_writes_no_caller_array(halo):
    """Every array poisoned outside I (NaN, then a finite absurd value; masks and regions 0xFF / random), at odd offsets inside
    guarded buffers: no byte of any caller buffer changes, and the records are the plain call's bit for bit."""
    _seen.clear()
    G = Geom(halo[0], halo[1], 0, nx=77, ny=23)
    footprint(_integrals_call, G)
    assert len(_seen) == 3
    for rec in _seen[1:]:
        assert np.array_equal(bits(rec), bits(_seen[0]))


# ---- the series and the errors ---------------------------------------------------------------------------------------------
def test_series_capacity_subranges_reset_and_overflow():
    ctx, states, src, w, _ = _setup()
    fl, net = ctx.field_set(FLUX_NAMES), ctx.field_set(NET_NAMES)
    sched = ctx.make_schedule(states, [ctx.field_set(EXCHANGE_NAMES)], time_fraction_increment=INC)
    ctx.time_steps(0, 2, sched, src, w, fl, net)
    q = _step_integrator(ctx, fl, net, states, capacity=3)
    for k in range(3):
        net["T"].mul_(1.5)
        q.collect(float(k))
    values, times = q.read()
    assert q.count() == 3 and values.shape == (3, 6) and list(times) == [0.0, 1.0, 2.0]
    assert values[0, 1] != values[1, 1] != values[2, 1]
    with pytest.raises(CofluxError, match="full"):
        q.collect(3.0)
    assert q.count() == 3 and np.array_equal(bits(q.read()[0]), bits(values))
    sub, sub_t = q.read(1, 2)
    assert np.array_equal(bits(sub), bits(values[1:])) and list(sub_t) == [1.0, 2.0]
    assert np.array_equal(bits(q.read(2, 1)[0]), bits(values[2:])) and q.read(3, 0)[0].shape == (0, 6)
    assert q.lib.cf_integrals_read(q._h, 1, 1, sub.ctypes.data_as(abi.c_double_p), None) == 0      # times may be NULL
    for first, n in ((0, 4), (-1, 1), (3, 1), (2, -1)):
        with pytest.raises(CofluxError, match="cf_integrals_read"):
            q.read(first, n)
    # cf_time_steps that would overflow fails before its first launch
    q.reset()
    assert q.count() == 0
    q.collect(9.0)
    ctx.attach_integrals(q, 2, 0.0, 1.0)
    ctx.sync()
    marks = {k: v.clone() for k, v in list(fl.items()) + [("net." + k, v) for k, v in net.items()]}
    with pytest.raises(CofluxError, match="series"):
        ctx.time_steps(3, 6, sched, src, w, fl, net)        # steps 3 … 8 collect after steps 3, 5, 7: three records, two fit
    ctx.sync()
    for k, v in list(fl.items()) + [("net." + k, v) for k, v in net.items()]:
        assert torch.equal(v.view(torch.int64), marks[k].view(torch.int64)), k
    assert q.count() == 1
    ctx.time_steps(3, 4, sched, src, w, fl, net)            # steps 3 … 6: two records
    assert q.count() == 3 and list(q.read()[1]) == [9.0, 4.0, 6.0]
    ctx.attach_integrals(None)
    ctx.time_steps(0, 3, sched, src, w, fl, net)            # detached: no record
    assert q.count() == 3
    q.close()
    ctx.close()


def test_errors():
    ctx = FluxContext(40, 12, 2, 2, ic.flux_params(), ring=1)
    a, b = ctx.zeros(), ctx.zeros()
    bad = [([], "0 entries"), ([("field", a, None, 0.0, 0)] * 33, None), ([("field", None, None, 0.0, 0)], "NULL a"),
           ([("product", a, None, 0.0, 0)], "NULL b"), ([("field", a, None, 0.0, 8)], "region bit"), ([("field", a, None, 0.0, -1)], "region bit"),
           ([("above", a, None, float("nan"), 0)], "threshold"), ([("above", a, None, float("inf"), 0)], "threshold"),
           ([(4, a, None, 0.0, 0)], "unknown kind"), ([(-1, a, None, 0.0, 0)], "unknown kind")]
    for entries, match in bad:
        with pytest.raises((CofluxError, ValueError), match=match):
            ctx.integrals(entries)
    for capacity in (0, -3):
        with pytest.raises(CofluxError, match="capacity"):
            ctx.integrals([("field", a, None, 0.0, 0)], capacity=capacity)
    with pytest.raises(CofluxError, match="max_workgroups"):
        ctx.integrals([("field", a, None, 0.0, 0)], max_workgroups=-1)
    desc = abi.IntegralsDesc()
    desc.n_entries, desc.entries[0].kind, desc.entries[0].a = 1, abi.INTEGRAND_FIELD, a.data_ptr()
    h = C.c_void_p()
    for size in (0, C.sizeof(abi.IntegralsDesc) - 8, C.sizeof(abi.IntegralsDesc) + 8):
        desc.struct_size = size
        assert ctx.lib.cf_integrals_create(ctx._h, C.byref(desc), 4, C.byref(h)) == -1 and not h.value     # CF_ERR_INVALID
    desc.struct_size, desc.n_entries = C.sizeof(abi.IntegralsDesc), 33
    assert ctx.lib.cf_integrals_create(ctx._h, C.byref(desc), 4, C.byref(h)) == -1 and not h.value
    desc.n_entries = 1
    assert ctx.lib.cf_integrals_create(ctx._h, C.byref(desc), 4, C.byref(h)) == 0 and h.value
    assert ctx.lib.cf_integrals_destroy(h) == 0
    q = ctx.integrals([("product", a, b, 0.0, 0), ("one",)], capacity=2)
    for stride in (0, -2):
        with pytest.raises(CofluxError, match="stride"):
            ctx.attach_integrals(q, stride, 0.0, 1.0)
    with pytest.raises(CofluxError, match="finite"):
        ctx.attach_integrals(q, 1, float("nan"), 1.0)
    other = FluxContext(40, 12, 2, 2, ic.flux_params(), ring=1)
    with pytest.raises(CofluxError, match="another context"):
        other.attach_integrals(q, 1, 0.0, 1.0)
    other.close()
    ctx.close()
    # an integrator outlived by its context: every call fails, destroying it does not
    for call in (q.collect, q.count, q.read, q.reset):
        with pytest.raises(CofluxError, match="destroyed"):
            call()
    q.close()
    # destroying an attached integrator detaches it: cf_time_steps goes on as without one
    ctx, states, src, w, _ = _setup()
    fl, net = ctx.field_set(FLUX_NAMES), ctx.field_set(NET_NAMES)
    q = _step_integrator(ctx, fl, net, states)
    ctx.attach_integrals(q, 1, 0.0, 1.0)
    q.close()
    sched = ctx.make_schedule(states, [ctx.field_set(EXCHANGE_NAMES)], time_fraction_increment=INC)
    ctx.time_steps(0, 3, sched, src, w, fl, net)
    ctx.sync()
    ctx.close()


# ---- run!(simulation) with the presets ---------------------------------------------------------------------------------------
def test_run_with_sea_ice_integrals_and_global_means_next_to_an_averaged_writer():
    """12 steps of 20 minutes on the sea-ice configuration.  Every record against fsum on the fields of an identical
    host-driven run, copied out after each step; and the one linear case where the two outputs must agree: the time mean of
    the hfds global-mean series over a window equals the global mean of the window's averaged hfds field within
    (n + 8 + 4K) · 2⁻⁵³ · Σ A·max_k|hfds_k| / Σ A  (K samples; 4K: the averager's three roundings per sample and cell,
    m·c_prev + f·c_new, and the host's mean of K numbers)."""
    K, steps = 6, 12
    grid_of = lambda m: m.ocean.grid  # noqa: E731
    inner = lambda a: interior(a, NX, NY, H, H)  # noqa: E731

    def fields_of(m):
        itf, st, si = m.interfaces, m.ocean.surface_state(), m.sea_ice
        net, ao = itf.net_fluxes._ocean_fields, itf.atmosphere_ocean_interface._fields
        return dict(hfds=net["T"], wfo=net["S"], hfss=ao["sensible_heat"], hfls=ao["latent_heat"], tos=st["T"], sos=st["S"],
                    h=si.thickness, c=si.concentration)

    ref = _model(True)
    per_step = []
    for _ in range(steps):
        cm.time_step(ref, DT)
        per_step.append({k: inner(v.cpu().numpy()).copy() for k, v in fields_of(ref).items()})
    wet = inner(ref.ocean.model.wet_mask.cpu().numpy()).copy()
    ref.interfaces.context.close()
    area = inner(grid_of(ref).cell_areas())
    region = inner(cm.hemisphere_regions(grid_of(ref)))
    assert wet.min() == 0 and ((region & 2) != 0).any() and ((region & 4) != 0).any()

    model = _model(True)
    ice, means = cm.sea_ice_integrals(model, capacity=5), cm.surface_global_means(model)   # (capacity 5: the series is drained twice)
    averages = cm.SurfaceFluxAverages(model, outputs=dict(hfds=model.interfaces.net_fluxes.ocean.T), schedule=cm.AveragedTimeInterval(K * DT))
    sim = cm.Simulation(model, dt=DT, stop_iteration=steps, output_writers=dict(ice=ice, means=means, surface=averages))
    cm.run(sim)
    assert list(ice.times) == list(means.times) == [DT * (k + 1) for k in range(steps)]

    ice_specs = [(k, a, b, t, bit) for bit in (1, 2) for k, a, b, t in (("product", "h", "c", 0.0), ("field", "c", None, 0.0), ("above", "c", None, 0.15))]
    names = [p + s for p in ("arctic", "antarctic") for s in ("_volume", "_area", "_extent")]
    assert list(ice.series()) == names
    mean_names = ["hfds", "wfo", "hfss", "hfls", "tos", "sos"]
    mean_specs = [("one", None, None, 0.0, 0)] + [("field", n, None, 0.0, 0) for n in mean_names]
    worst = 0.0
    for s in range(steps):
        worst = max(worst, check_values(ice.records()[0][s], reference(ice_specs, per_step[s], area, wet, region), f"sea ice, step {s + 1}"))
        worst = max(worst, check_values(means.records()[0][s], reference(mean_specs, per_step[s], area, wet, np.ones_like(region)),
                                        f"global means, step {s + 1}"))
    print(f"model level: worst error / bound = {worst:.3e}")
    raw = means.records()[0]
    for k, n in enumerate(mean_names):
        assert np.array_equal(means.series()[n], raw[:, k + 1] / raw[:, 0]), n
    assert np.ptp(means.series()["hfds"]) > 0 and np.abs(means.series()["hfds"]).min() > 0, "the series moves with the forcing"
    for s, name in ((0, "arctic_extent"), (3, "antarctic_volume")):
        assert ice.series()[name][s] > 0

    sel = wet != 0
    total_area = math.fsum(area[sel].tolist())
    assert len(averages.windows) == steps // K
    for k, (t_k, arrays) in enumerate(averages.windows):
        want = math.fsum((area * arrays["hfds"])[sel].tolist()) / total_area
        got = math.fsum(means.series()["hfds"][K * k:K * (k + 1)].tolist()) / K
        peak = np.max([np.abs(per_step[s]["hfds"]) for s in range(K * k, K * (k + 1))], axis=0)
        tol = (int(sel.sum()) + 8 + 4 * K) * EPS * math.fsum((area * peak)[sel].tolist()) / total_area
        print(f"window {t_k}: |time mean of the series - mean of the averaged field| = {abs(got - want):.3e}, tolerance {tol:.3e}")
        assert abs(got - want) <= tol, (t_k, got, want, tol)
    for wr in (ice, means):
        wr.close()
    model.interfaces.context.close()
