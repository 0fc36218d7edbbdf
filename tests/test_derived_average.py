"""GPU tests of the derived averager (include/coflux.h: cf_average_create_derived; coflux_derived.hip).  Every case is held
to tests/derived_reference.py bit for bit on the raw bytes.  The raw-ABI cases place every array inside a guarded buffer:
sources carry NaN in every halo cell the averager may not read, means carry 7.0e77 in theirs and start at an odd element
offset, so that a mean's row starts 8 bytes into a 16-byte line while the sources' rows do not.  Host against device, the
bytes are compared with NaNs made canonical (see bits()); device against device they are compared as they are."""
import ctypes as C

import numpy as np
import pytest
import torch

import derived_reference as dr
from coflux import abi
from coflux import interface_computations as ic
from coflux import models as cm
from coflux import regridding as rg
from coflux import synthetic as syn
from coflux.runtime import CofluxError, EXCHANGE_NAMES, FLUX_NAMES, NET_NAMES, FluxContext
from test_steps import INC, _setup
from test_time_average import _model

pytestmark = pytest.mark.gpu

GUARD, GUARD_VALUE, MEAN_HALO = 64, 3.0e33, 7.0e77
INVALID = -1


def raw(a):
    return np.ascontiguousarray(a).view(np.int64)


def bits(a):
    """the raw bytes, every NaN as the one canonical quiet NaN: IEEE 754 leaves the sign and payload of a NaN result open, and
    the host and the device use that freedom differently (an invalid operation gives −NaN on x86 and +NaN on gfx950; a
    subtraction is an addition with a negated operand there, which flips a propagated NaN's sign).  Which cells are NaN, and
    every bit of every other cell, −0.0 and ±Inf included, is compared."""
    a = np.array(a, dtype=np.float64, order="C")
    a[np.isnan(a)] = np.nan
    return a.view(np.int64)


class Arena:
    """device arrays of the halo layout inside guarded buffers; `odd`: the array starts at an odd element of its buffer"""
    def __init__(self, nx, ny, hx, hy):
        self.g = (nx, ny, hx, hy)
        self.shape = (ny + 2 * hy, nx + 2 * hx)
        self.n = self.shape[0] * self.shape[1]
        self.buffers = {}

    def place(self, name, odd):
        buf = torch.full((self.n + 2 * GUARD + 2,), GUARD_VALUE, dtype=torch.float64, device="cuda")
        off = GUARD + (1 if ((buf.data_ptr() // 8 + GUARD) % 2 == 0) == odd else 0)   # parity of the array's first element
        self.buffers[name] = (buf, off)
        return buf[off:off + self.n].view(self.shape)

    def guards_intact(self, name):
        buf, off = self.buffers[name]
        return bool((buf[:off] == GUARD_VALUE).all().item() and (buf[off + self.n:] == GUARD_VALUE).all().item())


def source_array(rng, g, east, north, specials=True):
    """random interior with ±0.0, NaN and Inf at known cells; NaN halos except column nx / row ny where they are read"""
    nx, ny, hx, hy = g
    a = np.full((ny + 2 * hy, nx + 2 * hx), np.nan)
    a[hy:hy + ny, hx:hx + nx] = rng.standard_normal((ny, nx)) * 10.0 ** rng.integers(-2, 3, (ny, nx))
    if specials:
        cells = rng.permutation(nx * ny)[:4]
        for c, v in zip(cells, (0.0, -0.0, np.nan, np.inf)):
            a[hy + c // nx, hx + c % nx] = v
    if east:
        a[hy:hy + ny, hx + nx] = rng.standard_normal(ny)
    if north:
        a[hy + ny, hx:hx + nx] = rng.standard_normal(nx)
    return a


def needs(terms, n_sources):
    east, north = [False] * n_sources, [False] * n_sources
    for kind, flags, a, b, _scale in terms:
        east[a] |= dr.reads_east(kind, flags)
        an, bn = dr.reads_north(kind, flags)
        north[a] |= an
        if dr.reads_b(kind):
            north[b] |= bn
    return east, north


def raw_create(ctx, table, n, cos=None, sin=None, struct_size=None, max_workgroups=0, reserved=0):
    desc = abi.AverageDesc(C.sizeof(abi.AverageDesc) if struct_size is None else struct_size, n, table, cos, sin, max_workgroups, reserved)
    h = C.c_void_p()
    rc = ctx.lib.cf_average_create_derived(ctx._h, C.byref(desc), C.byref(h))
    return rc, h


def run_terms(g, terms, n_sources, weights=(0.7, 2.0, 1.25), seed=0, rotation=(None, None), max_workgroups=0):
    """terms: (kind, flags, a, b, scale) with a / b source numbers; rotation: source numbers of (cos, sin).  Collects
    len(weights) times with fresh source values and checks means, halos, guards and sources; returns the interior means."""
    nx, ny, hx, hy = g
    ctx = FluxContext(nx, ny, hx, hy, ic.flux_params(), ring=0)
    arena, model = Arena(*g), dr.DerivedModel(*g)
    east, north = needs(terms, n_sources)
    src = [arena.place(f"s{k}", odd=False) for k in range(n_sources)]
    means = [arena.place(f"m{k}", odd=((hy * (nx + 2 * hx) + hx) % 2 == 0)) for k in range(len(terms))]   # interior rows 8 bytes into a line
    for m in means:
        assert (m.data_ptr() + 8 * (hy * (nx + 2 * hx) + hx)) % 16 == 8
        m.fill_(MEAN_HALO)
        m[hy:hy + ny, hx:hx + nx] = float("nan")
    table = (abi.AverageTerm * len(terms))()
    for t, (kind, flags, a, b, scale) in enumerate(terms):
        table[t] = abi.AverageTerm(kind, flags, src[a].data_ptr(), src[b].data_ptr() if dr.reads_b(kind) else None, scale, means[t].data_ptr())
    cos, sin = rotation
    rc, h = raw_create(ctx, table, len(terms), src[cos].data_ptr() if cos is not None else None, src[sin].data_ptr() if sin is not None else None,
                       max_workgroups=max_workgroups)
    assert rc == 0, ctx.lib.cf_last_error(ctx._h).decode()
    samples = [[] for _ in terms]
    for c, w in enumerate(weights):
        # a generator per (collection, source): a source's values do not depend on which others ride along
        host = [source_array(np.random.default_rng([seed, c, k]), g, east[k], north[k]) for k in range(n_sources)]
        for k in range(n_sources):
            src[k].copy_(torch.from_numpy(host[k]))
        assert ctx.lib.cf_average_collect(h, w) == 0
        ctx.sync()
        with np.errstate(all="ignore"):
            for t, (kind, flags, a, b, scale) in enumerate(terms):
                x = model.sample(kind, flags, host[a], host[b], scale, host[cos] if cos is not None else None,
                                 host[sin] if sin is not None else None)
                samples[t].append((x, w))
        for k in range(n_sources):
            assert np.array_equal(raw(src[k].cpu().numpy()), raw(host[k])), f"source {k} was written"
    out = []
    for t in range(len(terms)):
        got = means[t].cpu().numpy()
        want = dr.recurrence(samples[t])
        np.testing.assert_array_equal(bits(got[hy:hy + ny, hx:hx + nx]), bits(want), err_msg=f"term {t}: {terms[t]} on {g}")
        halo = np.ones(got.shape, bool)
        halo[hy:hy + ny, hx:hx + nx] = False
        assert (got[halo] == MEAN_HALO).all(), f"term {t}: a halo cell of the mean was written"
        out.append(got[hy:hy + ny, hx:hx + nx].copy())
    for name in arena.buffers:
        assert arena.guards_intact(name), f"the guard of {name} was written"
    assert ctx.lib.cf_average_destroy(h) == 0
    ctx.close()
    return out


# every kind once, sources shared between terms: 0 = a, 1 = b, 2 = cos, 3 = sin
ALL_KINDS = [(dr.FIELD, 0, 0, 0, 1.0), (dr.PRODUCT, 0, 0, 1, 1.0), (dr.PRODUCT, 0, 1, 1, -2.5), (dr.CENTER_X, 0, 0, 0, 1.0),
             (dr.CENTER_Y, 0, 1, 1, 1.0), (dr.CENTER_X_SQUARE, 0, 0, 0, 1.0), (dr.CENTER_Y_SQUARE, 0, 1, 1, 3.0),
             (dr.KINETIC_ENERGY, 0, 0, 1, 1.0), (dr.EAST, 0, 0, 1, -1026.0), (dr.NORTH, 0, 0, 1, -1026.0),
             (dr.EAST, dr.AT_CENTERS, 0, 1, 1.0), (dr.NORTH, dr.AT_CENTERS, 1, 0, 0.5)]
HALOS = [(1, 1), (2, 7), (7, 2), (3, 2)]
# the issue's shapes, and two with more rows than one thread's band so that several bands and a partial last one occur
SHAPES = [(nx, ny) for nx in (1, 2, 3, 67, 130, 1030) for ny in (1, 3)] + [(67, 9), (130, 6)]


@pytest.mark.parametrize("nx,ny", SHAPES)
def test_every_kind_bit_for_bit_with_footprint(nx, ny):
    for hx, hy in (HALOS if (nx, ny) in ((67, 3), (3, 1)) else [HALOS[(nx + ny) % 4]]):
        run_terms((nx, ny, hx, hy), ALL_KINDS, 4, seed=nx + ny, rotation=(2, 3))


@pytest.mark.parametrize("nx,ny,caps", [(130, 9, (1,)), (1030, 3, (1, 2, 3)), (300, 21, (1, 2, 5))])
def test_bits_do_not_depend_on_the_launched_grid(nx, ny, caps):
    """A workgroup of 256 threads holds 256 (band, column) items; capped below what the surface needs, every workgroup makes
    several trips of its grid-stride loop (1030 × 3: five with one workgroup, three and two with two and three, the last
    partial; 300 × 21: six bands, eight trips with one workgroup), and a row's neighbour hand-over crosses trips.  The bits are
    those of the uncapped launch, which makes one trip — and both are the restatement's (run_terms)."""
    g = (nx, ny, 3, 2)
    free = run_terms(g, ALL_KINDS, 4, seed=nx, rotation=(2, 3))
    for cap in caps:
        assert cap * 256 < -(-ny // 4) * nx, "the cap does not force a second trip"
        capped = run_terms(g, ALL_KINDS, 4, seed=nx, rotation=(2, 3), max_workgroups=cap)
        for t, (a, b) in enumerate(zip(free, capped)):
            np.testing.assert_array_equal(raw(a), raw(b), err_msg=f"term {t}, {cap} workgroups")


@pytest.mark.parametrize("halo", HALOS)
def test_averagers_without_neighbour_terms_read_no_halo(halo):
    """FIELD / PRODUCT / at-centres rotation only: column nx and row ny of every source are NaN as well"""
    terms = [(dr.FIELD, 0, 0, 0, 2.0), (dr.PRODUCT, 0, 0, 1, 1.0), (dr.EAST, dr.AT_CENTERS, 0, 1, 1.0), (dr.NORTH, dr.AT_CENTERS, 0, 1, 1.0)]
    run_terms((67, 3) + halo, terms, 4, rotation=(2, 3))
    # x-only and y-only averagers: the other neighbour's halo stays NaN
    run_terms((67, 3) + halo, [(dr.CENTER_X, 0, 0, 0, 1.0), (dr.CENTER_X_SQUARE, 0, 1, 1, 1.0)], 2)
    run_terms((67, 3) + halo, [(dr.CENTER_Y, 0, 0, 0, 1.0), (dr.CENTER_Y_SQUARE, 0, 1, 1, 1.0)], 2)


@pytest.mark.parametrize("n_terms", [1, 7, 16])
def test_the_probed_term_does_not_depend_on_its_place_or_its_company(n_terms):
    g, probe = (130, 3, 3, 2), (dr.KINETIC_ENERGY, 0, 0, 1, 0.25)
    # the fillers name the same sources again and others of their own (buckets of 4, 8 and 16 sources)
    fillers = [(dr.FIELD, 0, 0, 0, 1.0), (dr.PRODUCT, 0, 1, 1, 1.0)] + [(dr.PRODUCT, 0, 2 + k, 0, 1.0 + k) for k in range(13)]
    alone = run_terms(g, [probe], 2, seed=9)[0]
    for place in sorted({0, n_terms // 2, n_terms - 1}):
        terms = fillers[:n_terms - 1]
        terms.insert(place, probe)
        n_sources = max(max(t[2], t[3]) for t in terms) + 1
        got = run_terms(g, terms, n_sources, seed=9)[place]
        np.testing.assert_array_equal(raw(got), raw(alone))


def test_field_only_equals_cf_average_create():
    nx, ny, hx, hy = 130, 9, 3, 2
    ctx = FluxContext(nx, ny, hx, hy, ic.flux_params(), ring=1)
    rng = np.random.default_rng(4)
    src = [ctx.zeros() for _ in range(3)]
    plain = [torch.full(ctx.shape, float("nan"), dtype=torch.float64, device="cuda") for _ in range(3)]
    derived = [torch.full(ctx.shape, float("nan"), dtype=torch.float64, device="cuda") for _ in range(3)]
    a = ctx.average(src, plain)
    d = ctx.derived_average([("field", s, None, 1.0, 0, m) for s, m in zip(src, derived)])
    for w in (0.5, 2.0, 1.25, 3.0):
        for s in src:
            s.copy_(torch.from_numpy(source_array(rng, (nx, ny, hx, hy), False, False)))
        a.collect(w)
        d.collect(w)
    ctx.sync()
    assert a.weight() == d.weight()
    for p, q in zip(plain, derived):
        np.testing.assert_array_equal(raw(p.cpu().numpy()), raw(q.cpu().numpy()))
    d.reset()
    assert d.weight() == (0.0, 0)
    ctx.close()


# ---- cf_time_steps with an attached derived averager ------------------------------------------------------------------------------
def _derived_on(ctx, fl, net, rot, ocean):
    """A step fills no halo of the flux fields, so they enter at the cell only (field, product, rotation at centres); the
    terms that read [i+1] / [j+1] are on the ocean state, whose halos the caller keeps."""
    tx, ty, u, v = fl["x_momentum"], fl["y_momentum"], ocean["u"], ocean["v"]
    C_ = abi.TERM_AT_CENTERS
    spec = [("field", net["T"], None, cm.RHO_OCEAN * cm.CP_OCEAN, 0), ("product", fl["sensible_heat"], fl["sensible_heat"], 1.0, 0),
            ("product", net["u"], tx, 1.0, 0), ("east", tx, ty, -1.0, C_), ("north", tx, ty, -1.0, C_),
            ("center_x", u, None, 1.0, 0), ("center_y", v, None, 1.0, 0), ("kinetic_energy", u, v, 1.0, 0),
            ("east", u, v, 1.0, 0), ("north", u, v, 1.0, 0), ("center_x_square", u, None, 1.0, 0)]
    means = [torch.full(ctx.shape, float("nan"), dtype=torch.float64, device="cuda") for _ in spec]
    return ctx.derived_average([(k, a, b, s, f, m) for (k, a, b, s, f), m in zip(spec, means)], *rot), means


@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("pipeline", ["within_call", "continuing"])
def test_time_steps_with_an_attached_derived_averager_equals_the_host_loop(pipeline, stride):
    n, step_weight = 6, 1200.0
    ctx, states, src, w, _ = _setup(90, 40)
    rng = np.random.default_rng(1)
    theta = rng.uniform(0, 2 * np.pi, ctx.shape)
    rot = (ctx.to_device(np.cos(theta)), ctx.to_device(np.sin(theta)))
    # the host loop: cf_update_state + cf_average_collect
    atmos, rfl, rnet = ctx.field_set(EXCHANGE_NAMES), ctx.field_set(FLUX_NAMES), ctx.field_set(NET_NAMES)
    ravg, rmeans = _derived_on(ctx, rfl, rnet, rot, states[0])
    for s in range(n):
        tot = s * INC
        l1 = int(tot) % 4
        ctx.update_state(src, w, states[s % 2], atmos, rfl, rnet, level1=l1, level2=(l1 + 1) % 4, time_fraction=tot - int(tot))
        if (s + 1) % stride == 0:
            ravg.collect(stride * step_weight)
    ctx.sync()
    if pipeline == "continuing":
        ctx.set_option(abi.OPT_MERGED_PREFETCH, 2)
    sets = [ctx.field_set(EXCHANGE_NAMES) for _ in range(2)]
    fl, net = ctx.field_set(FLUX_NAMES), ctx.field_set(NET_NAMES)
    sched = ctx.make_schedule(states, sets, first_level=0, time_fraction=0.0, time_fraction_increment=INC,
                              pipeline=abi.PIPELINE_CONTINUING if pipeline == "continuing" else True)
    avg, means = _derived_on(ctx, fl, net, rot, states[0])
    ctx.attach_average(avg, stride, step_weight)
    for first, count in ((0, 4), (4, n - 4)):
        ctx.time_steps(first, count, sched, src, w, fl, net)
    ctx.sync()
    ctx.attach_average(None)
    assert avg.weight() == ravg.weight() == ((n // stride) * stride * step_weight, n // stride)
    for k, (m, r) in enumerate(zip(means, rmeans)):
        got, want = m.cpu().numpy(), r.cpu().numpy()
        np.testing.assert_array_equal(raw(got), raw(want), err_msg=f"term {k}")
        assert np.isfinite(got[3:-3, 3:-3]).any()
    ctx.close()


# ---- model level ---------------------------------------------------------------------------------------------------------------
class Recorder:
    """a writer that keeps every step's full source arrays on the host"""
    def __init__(self, fields):
        self.fields, self.steps = fields, []

    def initialize(self, simulation):
        pass

    def write(self, clock):
        self.steps.append({k: v.cpu().numpy().copy() for k, v in self.fields.items()})


def _restate(outputs, steps, weights, g, rotation=None):
    """the window means of `outputs` (name → field or expression) from the recorded steps, by the NumPy restatement"""
    model, names = dr.DerivedModel(*g), {}
    tensors = {}
    for name, o in outputs.items():
        kind, flags, a, b, scale = o.term() if isinstance(o, cm.SurfaceExpression) else (abi.TERM_FIELD, 0, o, None, 1.0)
        for t in (a, b):
            if t is not None:
                tensors[t.data_ptr()] = t
        names[name] = (kind, flags, a.data_ptr(), b.data_ptr() if b is not None else a.data_ptr(), scale)
    out = {}
    with np.errstate(all="ignore"):
        for name, (kind, flags, a, b, scale) in names.items():
            samples = [(model.sample(kind, flags, s[a], s[b], scale, *(rotation or (None, None))), w) for s, w in zip(steps, weights)]
            out[name] = dr.recurrence(samples)
    return out, tensors


@pytest.mark.parametrize("sea_ice", [False, True])
def test_simulation_with_omip_surface_outputs_matches_the_restatement(sea_ice):
    """with sea ice: siconc and sithick make seventeen outputs, two averagers"""
    model = _model(sea_ice)
    NX, NY, H, DT = 90, 40, 3, 20 * cm.minutes
    outputs = cm.omip_surface_outputs(model)
    assert list(outputs) == ["tos", "sos", "uos", "vos", "tossq", "sossq", "uosq", "vosq", "kes", "tauuo", "tauvo", "hfds", "wfo", "hfss",
                             "hfls"] + (["siconc", "sithick"] if sea_ice else [])
    if not sea_ice:   # the geographic preset rides along: identity rotation, wrapped east column, zero on the north wall
        outputs.update({"geo_" + k: v for k, v in cm.geographic_surface_outputs(model).items()})
    rot = tuple(t.cpu().numpy() for t in cm.grid_rotation(model))
    _, tensors = _restate(outputs, [], [], (NX, NY, H, H))
    recorder = Recorder(tensors)
    writer = cm.SurfaceFluxAverages(model, outputs=outputs, schedule=cm.AveragedTimeInterval(6 * DT))
    cm.run(cm.Simulation(model, dt=DT, stop_iteration=6, output_writers={"record": recorder, "surface": writer}))
    assert len(writer.windows) == 1 and len(recorder.steps) == 6 and len(writer.averagers) == 2
    _independent_stress_halos(model, recorder.steps, (NX, NY, H, H), fold=False)
    want, _ = _restate(outputs, recorder.steps, [DT] * 6, (NX, NY, H, H), rot)
    if not sea_ice:
        assert np.isfinite(want["geo_tauuo_east"][:, -1]).all() and np.isfinite(want["geo_tauvo_north"][-1, :]).all()
    arrays = writer.windows[0][1]
    for name in outputs:
        np.testing.assert_array_equal(bits(arrays[name]), bits(want[name]), err_msg=name)
    # mean(tos²) − mean(tos)² ≥ −(rounding): each mean carries at most 2 roundings per collection (6) and tossq one more,
    # the square of the mean one, the difference one
    wet = model.ocean.model.wet_mask.cpu().numpy()[H:H + NY, H:H + NX] != 0
    var = cm.variance(arrays["tossq"], arrays["tos"])
    bound = (2 * 6 + 1 + 2 * (2 * 6) + 1 + 1) * 2.0 ** -53 * np.maximum(arrays["tossq"], arrays["tos"] ** 2)
    assert (var[wet] >= -bound[wet]).all(), float((var[wet] / bound[wet]).min())
    model.interfaces.context.close()


def _independent_stress_halos(model, steps, g, fold):
    """Forget whatever the recorded east / north halos of the net stresses held and rebuild the cells a face → centre term
    reads from INTERIOR values alone: the periodic wrap of tauuo's first column, and for tauvo's row ny the tripolar fold in
    its NumPy statement (synthetic.fold_north, y-face, sign −1) or, without a fold, the north wall's zero."""
    nx, ny, hx, hy = g
    net = model.interfaces.net_fluxes._ocean_fields
    for s in steps:
        tu, tv = s[net["u"].data_ptr()], s[net["v"].data_ptr()]
        tu[:, hx + nx:] = np.nan
        tv[hy + ny:, :] = np.nan
        tu[hy:hy + ny, hx + nx] = tu[hy:hy + ny, hx]
        if fold:
            syn.fold_north(tv, nx, ny, hx, hy, 1, "y_face", -1.0)
        else:
            tv[hy + ny, hx:hx + nx] = 0.0


def test_geographic_outputs_on_the_tripolar_slab_feed_the_regridder():
    nx, ny, h, DT = 36, 18, 3, 20 * cm.minutes
    grid = cm.TripolarGrid(size=(nx, ny, 4), halo=(h, h, 2), area=np.ones((ny, nx)))
    case = syn.tripolar_case(nx, ny, h, h)
    ocean = cm.ocean_simulation(grid)
    o = case["ocean"]
    cm.set_surface(ocean, T=o["T"], S=o["S"], u=o["u"], v=o["v"], mask=o["mask"])
    model = cm.build_coupled_model(ocean, None, cm.JRA55PrescribedAtmosphere(syn.jra55_snapshots(2)), None, None, "corrected",
                                   velocity_formulation="relative", ocean_minimum_salinity=0)
    outputs = cm.geographic_surface_outputs(model)
    assert list(outputs) == ["tauuo_east", "tauvo_north", "uos_east", "vos_north", "hfds"]
    cos, sin = cm.grid_rotation(model)
    _, tensors = _restate(outputs, [], [], (nx, ny, h, h))
    recorder = Recorder(tensors)
    writer = cm.SurfaceFluxAverages(model, outputs=outputs, schedule=cm.AveragedTimeInterval(3 * DT))
    seen = []
    regridded = rg.RegriddedSurfaceMeans(model, writer, None, zonal=rg.zonal_band_weights(grid, nlat=9),
                                         on_window=lambda t, m, z, c: seen.append((t, z)))
    cm.run(cm.Simulation(model, dt=DT, stop_iteration=3, output_writers={"record": recorder, "surface": writer}))
    rot = (cos.cpu().numpy(), sin.cpu().numpy())
    _independent_stress_halos(model, recorder.steps, (nx, ny, h, h), fold=True)
    want, _ = _restate(outputs, recorder.steps, [DT] * 3, (nx, ny, h, h), rot)
    assert np.isfinite(want["tauuo_east"][:, -1]).all() and np.isfinite(want["tauvo_north"][-1, :]).all()
    arrays = writer.windows[0][1]
    for name in outputs:
        np.testing.assert_array_equal(bits(arrays[name]), bits(want[name]), err_msg=name)
    assert len(seen) == 1 and list(seen[0][1]) == list(outputs) and seen[0][1]["hfds"].shape == (9,)
    assert np.isfinite(seen[0][1]["tauuo_east"]).any()
    # where the grid is aligned with the geographic axes the east stress is −ρ · ℑx(tauuo)
    c, s = rot[0][h:h + ny, h:h + nx], rot[1][h:h + ny, h:h + nx]
    aligned = (c == 1.0) & (s == 0.0)
    assert aligned.any()
    tau = next(t for t in tensors.values() if t.data_ptr() == model.interfaces.net_fluxes._ocean_fields["u"].data_ptr())
    only_x, _ = _restate(dict(x=cm.Scaled(cm.CenteredX(tau), -cm.RHO_OCEAN)), recorder.steps, [DT] * 3, (nx, ny, h, h))
    np.testing.assert_array_equal(arrays["tauuo_east"][aligned], only_x["x"][aligned])
    regridded.close()
    model.interfaces.context.close()


# ---- errors: CF_ERR_INVALID, cf_last_error set, nothing launched ------------------------------------------------------------------
def test_every_invalid_descriptor_is_refused_and_launches_nothing():
    ctx = FluxContext(40, 12, 2, 2, ic.flux_params(), ring=1)
    n = ctx.shape[0] * ctx.shape[1]
    src = [ctx.zeros() + (k + 1.0) for k in range(18)]
    means = [torch.full(ctx.shape, MEAN_HALO, dtype=torch.float64, device="cuda") for _ in range(17)]
    P = lambda t: t.data_ptr()  # noqa: E731
    T = abi.AverageTerm

    def refused(terms, match, cos=None, sin=None, n_terms=None, struct_size=None, context=ctx):
        table = (T * max(len(terms), 1))(*terms)
        rc, h = raw_create(context, table if terms is not None else None, len(terms) if n_terms is None else n_terms, cos, sin, struct_size)
        assert rc == INVALID and not h.value, match
        assert match in context.lib.cf_last_error(context._h).decode(), (match, context.lib.cf_last_error(context._h).decode())

    good = T(abi.TERM_FIELD, 0, P(src[0]), None, 1.0, P(means[0]))
    refused([good], "struct_size", struct_size=C.sizeof(abi.AverageDesc) + 8)
    refused([good], "0 terms", n_terms=0)
    for bad in (dict(max_workgroups=-1), dict(reserved=1)):
        rc, h = raw_create(ctx, (T * 1)(good), 1, **bad)
        assert rc == INVALID and not h.value and "max_workgroups" in ctx.lib.cf_last_error(ctx._h).decode()
    refused([good] * 2, "17 terms", n_terms=17)
    refused([T(9, 0, P(src[0]), None, 1.0, P(means[0]))], "unknown kind")
    refused([T(-1, 0, P(src[0]), None, 1.0, P(means[0]))], "unknown kind")
    refused([T(abi.TERM_EAST, 2, P(src[0]), P(src[1]), 1.0, P(means[0]))], "flags", cos=P(src[2]), sin=P(src[3]))
    refused([T(abi.TERM_FIELD, abi.TERM_AT_CENTERS, P(src[0]), None, 1.0, P(means[0]))], "flags")
    refused([T(abi.TERM_FIELD, 0, None, None, 1.0, P(means[0]))], "NULL pointer")
    refused([T(abi.TERM_FIELD, 0, P(src[0]), None, 1.0, None)], "NULL pointer")
    for kind in (abi.TERM_PRODUCT, abi.TERM_KINETIC_ENERGY, abi.TERM_EAST, abi.TERM_NORTH):
        refused([T(kind, 0, P(src[0]), None, 1.0, P(means[0]))], "NULL pointer", cos=P(src[2]), sin=P(src[3]))
    for kind in (abi.TERM_EAST, abi.TERM_NORTH):
        refused([T(kind, 0, P(src[0]), P(src[1]), 1.0, P(means[0]))], "cos_rotation", cos=P(src[2]))
        refused([T(kind, 0, P(src[0]), P(src[1]), 1.0, P(means[0]))], "cos_rotation", sin=P(src[3]))
    for scale in (float("nan"), float("inf"), -float("inf")):
        refused([T(abi.TERM_FIELD, 0, P(src[0]), None, scale, P(means[0]))], "scale")
    # 8 products of 16 distinct sources and a rotation: 18 arrays
    many = [T(abi.TERM_PRODUCT, 0, P(src[2 * k]), P(src[2 * k + 1]), 1.0, P(means[k])) for k in range(8)]
    refused(many + [T(abi.TERM_EAST, abi.TERM_AT_CENTERS, P(src[0]), P(src[1]), 1.0, P(means[8]))], "distinct source arrays",
            cos=P(src[16]), sin=P(src[17]))
    # a mean over a source, over a rotation array, over another mean (by one element of its parent array)
    refused([T(abi.TERM_FIELD, 0, P(src[0]), None, 1.0, P(src[0]))], "overlaps")
    refused([T(abi.TERM_EAST, abi.TERM_AT_CENTERS, P(src[0]), P(src[1]), 1.0, P(src[3]))], "overlaps", cos=P(src[2]), sin=P(src[3]))
    buf = torch.zeros(2 * n, dtype=torch.float64, device="cuda")
    refused([T(abi.TERM_FIELD, 0, P(src[0]), None, 1.0, buf.data_ptr()), T(abi.TERM_FIELD, 0, P(src[1]), None, 1.0, buf.data_ptr() + 8 * (n - 1))],
            "overlap")
    assert ctx.lib.cf_average_create_derived(ctx._h, None, C.byref(C.c_void_p())) == INVALID
    assert ctx.lib.cf_average_create_derived(None, None, None) == INVALID
    # a kind that reads a neighbour needs hx ≥ 1 / hy ≥ 1: cf_create itself makes no context with a narrower halo (ring + 1
    # cells at least), so that refusal of the descriptor cannot be reached through the ABI — the context's is checked instead
    with pytest.raises(CofluxError):
        FluxContext(40, 12, 0, 0, ic.flux_params(), ring=0)
    ctx.sync()
    assert all((m == MEAN_HALO).all().item() for m in means), "a refused descriptor launched"
    ctx.close()
