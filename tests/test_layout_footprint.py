"""Every entry point under the memory layouts a caller hands it (include/coflux.h: the read and write set of each entry
point): unequal halos hx != hy, the ABI's minimum halo ring + 1, views that start at odd offsets inside larger buffers,
uint8 masks at odd byte addresses, and the k = top level of a 3-D array, whose slab holds an odd number of doubles.

Each call runs three times: once on plain exact-size allocations, and twice on such views whose cells OUTSIDE the
documented read set, and the buffers around them, hold poison.  The first poison is NaN; the second is a finite absurd value,
because v_max_f64 / v_min_f64 return the other operand of a NaN and can hide a NaN read.  The outputs start as sentinel bits.  The
write set must come out bit-identical to the plain call, and every other byte of every buffer must be unchanged.

The halo matrix holds each geometry to the oracle and the windows of all geometries to each other, bit for bit:
coflux.synthetic keys every value on the global (i, j), so the interior inputs are the same bits whatever the halo."""
import numpy as np
import pytest
import torch

import oracle as orc
import util
from coflux import abi
from coflux import interface_computations as ic
from coflux import synthetic as syn
from coflux.distributed import fold_north_halo_torch, slab_bounds
from coflux.runtime import EXCHANGE_NAMES, FLUX_NAMES, FLUX_OPTIONAL, NET_NAMES, FluxContext
from test_gpu_parity import compare

gpu = pytest.mark.gpu

NX, NY = 77, 23        # odd: nx + 2hx and (nx + 2hx)(ny + 2hy) are odd for every halo below
NZ, HZ = 4, 2          # the 3-D parent of the slab views: level HZ + NZ − 1 = 5, an odd number of odd slabs in
GUARD = 64
POISONS = ("nan", "absurd")
ABSURD = -3e5
TF = 0.37


def geometries(ring):
    return [(ring + 1, ring + 1), (2, 7), (7, 2), (8, 3)]


class Geom:
    def __init__(self, hx, hy, ring, nx=NX, ny=NY):
        self.nx, self.ny, self.hx, self.hy, self.ring = nx, ny, hx, hy, ring
        self.shape = (ny + 2 * hy, nx + 2 * hx)

    def box(self, r=None, di=0, dj=0):
        """cells (i + di, j + dj) for every cell (i, j) of the ring-r window"""
        r = self.ring if r is None else r
        m = np.zeros(self.shape, bool)
        m[self.hy - r + dj:self.hy + self.ny + r + dj, self.hx - r + di:self.hx + self.nx + r + di] = True
        return m

    @property
    def win(self):
        return self.box()

    @property
    def interior(self):
        return self.box(0)

    def cols(self, r):
        m = np.zeros(self.nx + 2 * self.hx, bool)
        m[self.hx - r:self.hx + self.nx + r] = True
        return m

    def rows(self, r):
        m = np.zeros(self.ny + 2 * self.hy, bool)
        m[self.hy - r:self.hy + self.ny + r] = True
        return m

    def W(self, a, r=None):
        return util.window(a, self.hx, self.hy, self.nx, self.ny, self.ring if r is None else r)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.int64, 4: np.int32, 1: np.uint8}[a.itemsize])


class Mem:
    """The fields of one call.  mode "plain": exact-size fresh allocations, inputs in full, outputs zero.  "nan" / "absurd":
    every field a view at an odd offset inside a guarded buffer, or (ocean T and u) the top slab of a 3-D array; inputs
    poisoned outside their read set, outputs pre-filled with sentinel bits.  run() calls the entry point and checks that
    nothing outside the declared write sets changed, guard bands included."""

    OFFSETS = {8: (1, 3, 5), 4: (1, 3), 1: (1, 3, 2)}

    def __init__(self, mode, seed=0):
        self.mode, self.plain = mode, mode == "plain"
        self.rng = np.random.default_rng(seed)
        self.n = 0
        self.outs, self.watch = {}, []

    def _poison(self, dtype, shape):
        if dtype == np.uint8:    # a mask: 0xFF (wet) or random 0/1
            return np.full(shape, 0xFF, np.uint8) if self.mode == "nan" else self.rng.integers(0, 2, shape).astype(np.uint8)
        return np.full(shape, np.nan if self.mode == "nan" else ABSURD, dtype)

    def _alloc(self, shape, tdtype, fill, slab):
        self.n += 1
        if slab:
            g = self.G
            return util.top_slab(g.nx, g.ny, g.hx, g.hy, nz=NZ, hz=HZ, dtype=tdtype, fill=fill)
        size = torch.empty((), dtype=tdtype).element_size()
        offs = self.OFFSETS[size]
        return util.guarded(shape, tdtype, offset=offs[self.n % len(offs)], guard=GUARD, fill=fill)

    def inp(self, name, a, read=None, slab=False):
        """an input field; `read`: its read set (bool, a's shape), None = read in full"""
        a = np.ascontiguousarray(a)
        if self.plain:
            return torch.from_numpy(a.copy()).cuda()
        b = a.copy()
        if read is not None:
            b[~read] = self._poison(a.dtype, a.shape)[~read]
        fill = 0xFF if a.dtype == np.uint8 and self.mode == "nan" else (1 if a.dtype == np.uint8 else
                                                                          (float("nan") if self.mode == "nan" else ABSURD))
        t = self._alloc(a.shape, torch.from_numpy(a[:0]).dtype, fill, slab)
        t.copy_(torch.from_numpy(b))
        self.watch.append((name, t, None))
        return t

    def out(self, name, shape, write, dtype=torch.float64, init=None):
        """an output field with write set `write`; `init`: what the caller put there before (else zero / sentinel)"""
        if self.plain:
            t = torch.zeros(shape, dtype=dtype, device="cuda")
        else:
            t = self._alloc(shape, dtype, util.SENTINEL32 if dtype == torch.int32 else util.SENTINEL64, False)
        if init is not None:
            t.copy_(torch.from_numpy(np.ascontiguousarray(init)))
        self.outs[name] = (t, write)
        self.watch.append((name, t, write))
        return t

    def inout(self, name, a, read, write):
        """a field updated in place: poisoned outside `read`, and outside `write` it must keep its input bits"""
        t = self.inp(name, a, read)
        if not self.plain:
            self.watch[-1] = (name, t, write)
        self.outs[name] = (t, write)
        return t

    def run(self, fn, ctx):
        snaps = [] if self.plain else [(name, t, w, bits(util.buffer_of(t)[0].cpu().numpy())) for name, t, w in self.watch]
        torch.cuda.synchronize()
        fn()
        ctx.sync()
        torch.cuda.synchronize()
        for name, t, write, before in snaps:
            flat, start = util.buffer_of(t)
            after = bits(flat.cpu().numpy())
            allowed = np.zeros(after.shape, bool)
            if write is not None:
                allowed[start:start + t.numel()] = write.reshape(-1)
            bad = (after != before) & ~allowed
            if bad.any():
                where = np.flatnonzero(bad)[:6] - start
                g = self.G
                cells = [divmod(int(k), t.shape[-1]) if 0 <= k < t.numel() else ("guard", int(k)) for k in where]
                cells = [(c[0] - g.hy, c[1] - g.hx) if c[0] != "guard" else c for c in cells]
                raise AssertionError(f"[{self.mode}] {name}: {int(bad.sum())} element(s) outside the write set changed, "
                                     f"first (j, i) / guard offsets: {cells}")
        return {name: t.cpu().numpy() for name, (t, _) in self.outs.items()}


def footprint(call, G, *args, **kw):
    """call(mem, G, ...) on plain memory and under both poisons; the write sets must agree bit for bit.  Returns the
    plain call's outputs."""
    res = {}
    for mode in ("plain",) + POISONS:
        mem = Mem(mode)
        mem.G = G
        res[mode] = call(mem, G, *args, **kw)
        if mode == "plain":
            writes = {k: w for k, (_, w) in mem.outs.items()}
    for mode in POISONS:
        for k, w in writes.items():
            a, b = bits(res["plain"][k]), bits(res[mode][k])
            bad = (a != b) & w
            assert not bad.any(), (f"[{mode}] {k}: {int(bad.sum())} cell(s) of the write set differ from the plain call, "
                                   f"first (j, i): {[(j - G.hy, i - G.hx) for j, i in np.argwhere(bad)[:6]]}")
    return res["plain"]


# ---------------------------------------------------------------------------------------------
# read sets (include/coflux.h)
# ---------------------------------------------------------------------------------------------
def ocean_reads(G, names=("T", "S", "u", "v", "mask"), r=None):
    """The ocean solve on the ring window: T, S, mask at the cell, u also at i + 1, v also at j + 1."""
    w = G.box(r)
    rd = dict(T=w, S=w, mask=w, u=w | G.box(r, di=1), v=w | G.box(r, dj=1))
    return {k: rd[k] for k in names}


def mask_input(case, params):
    m = case["ocean"]["mask"]
    if params.mask_kind == abi.MASK_BOTTOM_HEIGHT:
        return np.where(m != 0, -4000.0, 0.0)   # land where surface_z (−150 m) ≤ bottom height
    return m


def oracle_ocean(case, params):
    o = dict(case["ocean"])
    if params.mask_kind == abi.MASK_NONE:
        o["mask"] = None
    else:
        o["mask"] = mask_input(case, params)
    return o


def put_ocean(mem, G, case, params, reads):
    o = {}
    for k, rd in reads.items():
        if k == "mask":
            if params.mask_kind != abi.MASK_NONE:
                o[k] = mem.inp("ocean.mask", mask_input(case, params), rd)
        else:
            o[k] = mem.inp("ocean." + k, case["ocean"][k], rd, slab=k in ("T", "u"))
    return o


def put_weights(mem, G, case, r, latitude_rows=False):
    w = case["weights"]
    if w["separable"]:
        out = dict(separable=True, fi=mem.inp("fi", w["fi"], G.cols(r)), fj=mem.inp("fj", w["fj"], G.rows(r)))
        if latitude_rows:
            out["latitude"] = mem.inp("latitude", w["latitude"], G.rows(0))
        return out
    win = G.box(r)
    out = dict(separable=False, **{k: mem.inp(k, w[k], win) for k in ("fi", "fj", "cos_rot", "sin_rot")})
    if latitude_rows:
        out["latitude"] = mem.inp("latitude", w["latitude"], G.interior)
    return out


def put_ice(mem, G, case):
    """the ocean partition: ℵ at the cell and its west and south neighbours, the rest at the cell (interior)"""
    c = G.interior
    reads = dict(concentration=c | G.box(0, di=-1) | G.box(0, dj=-1), interface_heat=c, salt_flux=c, x_stress=c, y_stress=c)
    return {k: mem.inp("ice." + k, case["ice"][k], rd) for k, rd in reads.items()}


def put_src(mem, case):
    return {k: mem.inp("src." + k, v) for k, v in case["src"].items()}


def net_reads(G):
    c = G.interior
    return dict(x_momentum=c | G.box(0, di=-1), y_momentum=c | G.box(0, dj=-1))


def flux_outputs(mem, G, prefix="fluxes", optional=True, iterations=True, face_halos=False):
    """the solver's outputs on the ring window.  face_halos: at ring 0 the face stresses of the same call read ρτx at
    i = −1 and ρτy at j = −1, which nobody computes: the caller fills them (here with zeros, what the oracle has)."""
    out = {}
    for k in FLUX_NAMES + (FLUX_OPTIONAL if optional else ()):
        init = None
        if face_halos and k in ("x_momentum", "y_momentum") and G.ring == 0:
            init = np.zeros(G.shape) if mem.plain else np.array(np.full(G.shape, util.SENTINEL64, np.uint64).view(np.float64))
            init[net_reads(G)[k] & ~G.interior] = 0.0
        out[k] = mem.out(f"{prefix}.{k}", G.shape, G.win, init=init)
    if iterations:
        out["iterations"] = mem.out(f"{prefix}.iterations", G.shape, G.win, dtype=torch.int32)
    return out


def make_ctx(G, params, options=()):
    ctx = FluxContext(G.nx, G.ny, G.hx, G.hy, params, ring=G.ring)
    for o, v in options:
        ctx.set_option(o, v)
    return ctx


# ---------------------------------------------------------------------------------------------
# 4. the halo geometry matrix: whole steps against the oracle, bitwise across geometries
# ---------------------------------------------------------------------------------------------
def _latlon_albedo():
    return dict(ocean_surface=ic.SurfaceRadiationProperties(ic.LatitudeDependentAlbedo(), 0.97))


# name: (flux config, params extras, weights, options, ice partition, entry)
PATHS = {
    "tables_tiled_u8": ("default", {}, "latlon", ((abi.OPT_INTERP_TILE_CAP, 128), (abi.OPT_FUSED_NET, 0)), True, "update"),
    "libm_gather_general_bottom": ("corrected", dict(mask_kind=abi.MASK_BOTTOM_HEIGHT, **_latlon_albedo()), "tripolar",
                                   ((abi.OPT_INTERP_TILE_CAP, 0), (abi.OPT_SOLVER, abi.SOLVER_LIBM)), False, "three"),
    "certified_none": ("default", dict(mask_kind=abi.MASK_NONE), "latlon",
                       ((abi.OPT_SOLVER_PATH, abi.SOLVER_PATH_CERTIFIED), (abi.OPT_INTERP_TILE_CAP, 0)), True, "update"),
    "latency_layout": ("corrected", {}, "tripolar", ((abi.OPT_LATENCY_LAYOUT, 2), (abi.OPT_FUSED_NET, 1)), False, "update"),
    "ncar_fused": ("ncar", dict(mask_kind=abi.MASK_BOTTOM_HEIGHT), "latlon", ((abi.OPT_FUSED_NET, 1),), True, "update"),
    "fixed5_latitude_albedo": ("fixed5", dict(mask_kind=abi.MASK_U8, **_latlon_albedo()), "tripolar",
                               ((abi.OPT_INTERP_TILE_CAP, 0),), True, "three"),
}


def path_params(name):
    config, extra, *_ = PATHS[name]
    fluxes, vd = util.CONFIGS[config]()
    return ic.flux_params(fluxes, velocity_difference=vd, **extra)


def step_call(mem, G, case, params, options, ice, entry, expect=None):
    """interpolate → ocean solve → net fluxes, as one cf_update_state or as the three entry points"""
    ctx = make_ctx(G, params, options)
    lat = params.ocean_albedo_kind == abi.ALBEDO_LATITUDE_DEPENDENT
    src = put_src(mem, case)
    w = put_weights(mem, G, case, G.ring, latitude_rows=lat)
    ocean = put_ocean(mem, G, case, params, ocean_reads(G))
    icef = put_ice(mem, G, case) if ice else None
    atmos = {k: mem.out("atmos." + k, G.shape, G.win) for k in EXCHANGE_NAMES}
    fl = flux_outputs(mem, G, face_halos=True)
    net = {k: mem.out("net." + k, G.shape, G.interior) for k in NET_NAMES}
    if expect:
        if "mask" in ocean:
            ctx.ensure_chunk_table(ocean["mask"])
        expect(ctx)
    if entry == "update":
        fn = lambda: ctx.update_state(src, w, ocean, atmos, fl, net, ice=icef, time_fraction=TF)
    else:
        def fn():
            ctx.interpolate_atmosphere_state(src, w, atmos, 0, 1, TF)
            ctx.compute_atmosphere_ocean_fluxes(ocean, atmos, fl)
            ctx.compute_net_ocean_fluxes(ocean, atmos, fl, net, ice=icef, weights=w)
    out = mem.run(fn, ctx)
    ctx.close()
    return out


def _expectation(name):
    if name == "certified_none":
        return lambda ctx: assert_path(ctx.solver_iteration_path() == abi.SOLVER_PATH_CERTIFIED, "certified path")
    if name == "latency_layout":
        return lambda ctx: assert_path(ctx.solver_latency_layout(), "latency-layout kernels")
    return None


def assert_path(ok, what):
    assert ok, f"the {what} did not run"


@gpu
@pytest.mark.parametrize("ring", [0, 1])
@pytest.mark.parametrize("path", list(PATHS))
def test_halo_geometry_matrix(path, ring):
    """(hx, hy) ∈ {(ring+1, ring+1), (2, 7), (7, 2), (8, 3)}: poisoned footprint, sentinel write sets, the oracle's
    tolerances, and the same window bits in every geometry."""
    config, _, weights, options, ice, entry = PATHS[path]
    params = path_params(path)
    tol = 1e-6 if path == "certified_none" else None
    first = None
    for hx, hy in geometries(ring):
        G = Geom(hx, hy, ring)
        case = util.build_case(NX, NY, hx, hy, weights=weights)
        got = footprint(step_call, G, case, params, options, ice, entry, expect=_expectation(path))
        g = orc.make_grid(NX, NY, hx, hy, ring)
        atmos = orc.interpolate_atmosphere_state(g, case["src"], case["weights"], 0, 1, TF)
        oo = oracle_ocean(case, params)
        fl = orc.compute_atmosphere_ocean_fluxes(g, params, oo, atmos, nthreads=0)
        if ring == 0:    # the oracle's flux halos are zero, as the caller's are here
            for k in ("x_momentum", "y_momentum"):
                fl[k][~G.win] = 0.0
        net = orc.compute_net_ocean_fluxes(g, params, oo, atmos, fl, ice=case["ice"] if ice else None,
                                           weights=case["weights"])
        shaped = dict(atmos={k: got["atmos." + k] for k in EXCHANGE_NAMES},
                      fluxes={k: got["fluxes." + k] for k in FLUX_NAMES + FLUX_OPTIONAL},
                      net={k: got["net." + k] for k in NET_NAMES})
        compare(case, shaped, dict(atmos=atmos, fluxes=fl, net=net), ring, **({"tol_solver": tol} if tol else {}))
        wins = {k: G.W(v, 0 if k.startswith("net.") else ring) for k, v in got.items()}
        if first is None:
            first = (hx, hy, wins)
        else:
            for k, v in wins.items():
                np.testing.assert_array_equal(bits(v), bits(first[2][k]),
                                              err_msg=f"{k}: halo ({hx}, {hy}) vs ({first[0]}, {first[1]})")


@pytest.mark.parametrize("config", ["default", "corrected"])
def test_c_and_numpy_oracles_agree_with_unequal_halos(config):
    """The reference itself in the matrix's geometry: the C and NumPy restatements at (hx, hy) = (2, 7), ring 1."""
    import numpy_oracle as npo
    hx, hy = 2, 7
    case = util.build_case(NX, NY, hx, hy)
    g = orc.make_grid(NX, NY, hx, hy, 1)
    fluxes, vd = util.CONFIGS[config]()
    params = ic.flux_params(fluxes, velocity_difference=vd)
    at = orc.interpolate_atmosphere_state(g, case["src"], case["weights"], 0, 1, TF)
    fi2d = np.broadcast_to(case["weights"]["fi"][None, :], at["T"].shape)
    fj2d = np.broadcast_to(case["weights"]["fj"][:, None], at["T"].shape)
    at_np = npo.interpolate_atmosphere_state(case["src"], fi2d, fj2d, 0, 1, TF)
    G = Geom(hx, hy, 1)
    for k in EXCHANGE_NAMES:
        assert util.rel_err(G.W(at[k]), G.W(at_np[k]), util.ATMOS_SCALE[k]) < 1e-13, k
    a = orc.compute_atmosphere_ocean_fluxes(g, params, case["ocean"], at)
    with np.errstate(all="ignore"):
        b = npo.atmosphere_ocean_fluxes(fluxes, case["ocean"], at, hx=hx, hy=hy, ring=1,
                                        thermodynamics=ic.AtmosphereThermodynamicsParameters(),
                                        seawater=ic.SeawaterComposition(), ocean_properties=ic.OceanProperties(),
                                        velocity_difference="wind" if isinstance(vd, ic.WindVelocity) else "relative")
    tol = 1e-6 if a["iterations"].max() >= 100 else 1e-12
    for k in FLUX_NAMES + FLUX_OPTIONAL:
        bk = b[k] if b[k].shape == G.W(a[k]).shape else G.W(b[k])
        assert util.rel_err(G.W(a[k]), bk, util.FIELD_SCALE[k]) < tol, k
    net_c = orc.compute_net_ocean_fluxes(g, params, case["ocean"], at, a, ice=case["ice"], weights=case["weights"])
    net_n = npo.net_ocean_fluxes(case["ocean"], at, a, hx=hx, hy=hy, ocean_properties=ic.OceanProperties(),
                                 albedo=0.06, ice=case["ice"])
    for k in ("u", "v", "T", "S"):
        nk = net_n[k] if net_n[k].shape == G.W(net_c[k], 0).shape else G.W(net_n[k], 0)
        assert util.rel_err(G.W(net_c[k], 0), nk, util.FIELD_SCALE[k]) < 1e-12, k


# ---------------------------------------------------------------------------------------------
# 2–3. each entry point on its own: read sets poisoned, write sets fenced
# ---------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("hx, hy, ring", [(2, 7, 1), (1, 1, 0), (8, 3, 0)])
@pytest.mark.parametrize("weights", ["latlon", "tripolar"])
@pytest.mark.parametrize("cap", [128, 0])
def test_interpolate_atmosphere_state(cap, weights, hx, hy, ring):
    """Reads the whole source, fi / fj (and the rotation) at the window's indices; writes the eight fields on the window."""
    G = Geom(hx, hy, ring)
    case = util.build_case(NX, NY, hx, hy, weights=weights)

    def call(mem, G):
        ctx = make_ctx(G, ic.flux_params(), ((abi.OPT_INTERP_TILE_CAP, cap),))
        src, w = put_src(mem, case), put_weights(mem, G, case, ring)
        atmos = {k: mem.out(k, G.shape, G.win) for k in EXCHANGE_NAMES}
        out = mem.run(lambda: ctx.interpolate_atmosphere_state(src, w, atmos, 0, 1, TF), ctx)
        ctx.close()
        return out
    got = footprint(call, G)
    ref = orc.interpolate_atmosphere_state(orc.make_grid(NX, NY, hx, hy, ring), case["src"], case["weights"], 0, 1, TF)
    for k in EXCHANGE_NAMES:
        assert util.rel_err(G.W(got[k]), G.W(ref[k]), util.ATMOS_SCALE[k]) <= 1e-12, k


AO_PATHS = {   # config, params extras, options, atmosphere fields read besides u, v, T, p, q
    "tables_u8": ("default", {}, (), ()),
    "libm_bottom": ("default", dict(mask_kind=abi.MASK_BOTTOM_HEIGHT), ((abi.OPT_SOLVER, abi.SOLVER_LIBM),), ()),
    "certified_none": ("default", dict(mask_kind=abi.MASK_NONE), ((abi.OPT_SOLVER_PATH, abi.SOLVER_PATH_CERTIFIED),), ("Mp",)),
    "latency_layout_u8": ("corrected", {}, ((abi.OPT_LATENCY_LAYOUT, 2),), ()),
    "ncar_bottom": ("ncar", dict(mask_kind=abi.MASK_BOTTOM_HEIGHT), (), ()),
    "fixed5_none": ("fixed5", dict(mask_kind=abi.MASK_NONE), (), ()),
}


@gpu
@pytest.mark.parametrize("hx, hy, ring", [(8, 3, 1), (1, 1, 0)])
@pytest.mark.parametrize("path", list(AO_PATHS))
def test_compute_atmosphere_ocean_fluxes(path, hx, hy, ring):
    """Reads the atmosphere (u, v, T, p, q; the certified path also M_p) and ocean T, S, mask on the window, u also at i + 1,
    v also at j + 1; writes every flux output and `iterations` on the window, land cells included."""
    config, extra, options, more = AO_PATHS[path]
    fluxes, vd = util.CONFIGS[config]()
    params = ic.flux_params(fluxes, velocity_difference=vd, **extra)
    G = Geom(hx, hy, ring)
    case = util.build_case(NX, NY, hx, hy)
    at = orc.interpolate_atmosphere_state(orc.make_grid(NX, NY, hx, hy, ring), case["src"], case["weights"], 0, 1, TF)
    read = ("u", "v", "T", "p", "q") + more

    def call(mem, G):
        ctx = make_ctx(G, params, options)
        ocean = put_ocean(mem, G, case, params, ocean_reads(G))
        atmos = {k: mem.inp("atmos." + k, at[k], G.win if k in read else np.zeros(G.shape, bool)) for k in EXCHANGE_NAMES}
        fl = flux_outputs(mem, G)
        if "mask" in ocean:
            ctx.ensure_chunk_table(ocean["mask"])
        if path.startswith("certified"):
            assert_path(ctx.solver_iteration_path() == abi.SOLVER_PATH_CERTIFIED, "certified path")
        if path.startswith("latency"):
            assert_path(ctx.solver_latency_layout(), "latency-layout kernels")
        out = mem.run(lambda: ctx.compute_atmosphere_ocean_fluxes(ocean, atmos, fl), ctx)
        ctx.close()
        return out
    got = footprint(call, G)
    ref = orc.compute_atmosphere_ocean_fluxes(orc.make_grid(NX, NY, hx, hy, ring), params, oracle_ocean(case, params), at)
    unconv = np.any(G.W(ref["iterations"]) >= params.maxiter)
    tol = 1e-6 if path.startswith("certified") or unconv else 1e-9
    for k in FLUX_NAMES + FLUX_OPTIONAL:
        assert util.rel_err(G.W(got["fluxes." + k]), G.W(ref[k]), util.FIELD_SCALE[k]) <= tol, k


@gpu
@pytest.mark.parametrize("hx, hy", [(2, 7), (7, 2), (1, 1)])
@pytest.mark.parametrize("variant", ["plain", "ice", "ice_latitude_albedo_general"])
def test_compute_net_ocean_fluxes(variant, hx, hy):
    """Interior cells only.  Reads S, mask, the cell-local fluxes, Q_s, Q_ℓ, M_p and the ice partition at the cell, ρτx also
    at i − 1, ρτy and ℵ also at j − 1 (ℵ at i − 1 too), the latitude at the cell's row (separable) or cell; writes the
    eight net fields on the interior, land cells included."""
    ring = 0 if hx == 1 else 1
    G = Geom(hx, hy, ring)
    lat = variant.endswith("general")
    params = ic.flux_params(**(_latlon_albedo() if lat else {}), ocean_minimum_salinity=34.0)
    case = util.build_case(NX, NY, hx, hy, weights="tripolar" if lat else "latlon")
    g = orc.make_grid(NX, NY, hx, hy, 0)
    at = orc.interpolate_atmosphere_state(g, case["src"], case["weights"], 0, 1, TF)
    # the flux inputs with their i = −1 column and j = −1 row computed: the ring-1 solve of the same surface on a halo one
    # wider (a ring-1 solve on this halo would read u, v beyond the array at hx = hy = 1), cropped to this halo
    wide = util.build_case(NX, NY, hx + 1, hy + 1, weights="tripolar" if lat else "latlon")
    gw = orc.make_grid(NX, NY, hx + 1, hy + 1, 1)
    at_w = orc.interpolate_atmosphere_state(gw, wide["src"], wide["weights"], 0, 1, TF)
    fl = {k: np.ascontiguousarray(v[1:-1, 1:-1])
          for k, v in orc.compute_atmosphere_ocean_fluxes(gw, params, wide["ocean"], at_w).items()}
    ice = variant != "plain"
    c = G.interior

    def call(mem, G):
        ctx = make_ctx(G, params)
        none = np.zeros(G.shape, bool)     # the ABI asks for ocean T, u, v and atmosphere u, v, T, p, q; none is read
        ocean = put_ocean(mem, G, case, params, dict(T=none, S=c, u=none, v=none, mask=c))
        atmos = {k: mem.inp("atmos." + k, at[k], c if k in ("Qs", "Ql", "Mp") else none) for k in EXCHANGE_NAMES}
        rd = dict(net_reads(G), sensible_heat=c, latent_heat=c, water_vapor=c, temperature=c)
        fluxes = {k: mem.inp("fluxes." + k, fl[k], rd[k]) for k in FLUX_NAMES}
        icef = put_ice(mem, G, case) if ice else None
        w = put_weights(mem, G, case, 0, latitude_rows=True) if lat else None
        net = {k: mem.out("net." + k, G.shape, c) for k in NET_NAMES}
        out = mem.run(lambda: ctx.compute_net_ocean_fluxes(ocean, atmos, fluxes, net, ice=icef, weights=w), ctx)
        ctx.close()
        return out
    got = footprint(call, G)
    ref = orc.compute_net_ocean_fluxes(g, params, case["ocean"], at, fl, ice=case["ice"] if ice else None, weights=case["weights"])
    for k in NET_NAMES:
        assert util.rel_err(G.W(got["net." + k], 0), G.W(ref[k], 0), util.FIELD_SCALE[k]) <= 1e-12, k


@gpu
@pytest.mark.parametrize("merged", [0, 1, 2])
def test_time_steps(merged):
    """cf_time_steps (pipelined, two ocean states, two exchange sets) under unequal halos: the same footprint as
    cf_update_state, step after step, whatever carries the next interpolation."""
    hx, hy, ring = 7, 2, 1
    G = Geom(hx, hy, ring)
    case = util.build_case(NX, NY, hx, hy, n_levels=4)
    o1 = syn.evolved_ocean_state(case["ocean"], NX, NY, hx, hy, 1)
    params = ic.flux_params(ic.corrected_atmosphere_ocean_fluxes(), velocity_difference=ic.RelativeVelocity())

    def call(mem, G):
        ctx = make_ctx(G, params, ((abi.OPT_MERGED_PREFETCH, merged),))
        src, w = put_src(mem, case), put_weights(mem, G, case, ring)
        states = [put_ocean(mem, G, case, params, ocean_reads(G))]
        second = dict(case, ocean=dict(o1, mask=case["ocean"]["mask"]))
        states.append(put_ocean(mem, G, second, params, ocean_reads(G, ("T", "S", "u", "v"))))
        states[1]["mask"] = states[0]["mask"]
        sets = [{k: mem.out(f"atmos{n}.{k}", G.shape, G.win) for k in EXCHANGE_NAMES} for n in range(2)]
        fl = flux_outputs(mem, G, optional=False, iterations=False)
        net = {k: mem.out("net." + k, G.shape, G.interior) for k in NET_NAMES}
        sched = ctx.make_schedule(states, sets, first_level=0, time_fraction=0.0, time_fraction_increment=1.0 / 9.0, pipeline=True)
        out = mem.run(lambda: ctx.time_steps(0, 5, sched, src, w, fl, net), ctx)
        ctx.close()
        return out
    got = footprint(call, G)
    # the last step (4: snapshots 0 → 1 at 4/9, ocean state 0) against the oracle; its exchange fields are in set 0
    g = orc.make_grid(NX, NY, hx, hy, ring)
    at = orc.interpolate_atmosphere_state(g, case["src"], case["weights"], 0, 1, 4.0 / 9.0)
    fl = orc.compute_atmosphere_ocean_fluxes(g, params, case["ocean"], at, nthreads=0)
    net = orc.compute_net_ocean_fluxes(g, params, case["ocean"], at, fl, weights=case["weights"])
    tol = 1e-6 if np.any(G.W(fl["iterations"]) >= params.maxiter) else 1e-9
    for k in EXCHANGE_NAMES:
        assert util.rel_err(G.W(got["atmos0." + k]), G.W(at[k]), util.ATMOS_SCALE[k]) <= 1e-12, k
    for k in FLUX_NAMES:
        assert util.rel_err(G.W(got["fluxes." + k]), G.W(fl[k]), util.FIELD_SCALE[k]) <= tol, k
    for k in NET_NAMES:
        assert util.rel_err(G.W(got["net." + k], 0), G.W(net[k], 0), util.FIELD_SCALE[k]) <= tol, k


# ---------------------------------------------------------------------------------------------
# sea ice
# ---------------------------------------------------------------------------------------------
ICE_STATE_READS = ("thickness", "top_temperature", "u", "v", "albedo")


def _ice_setup(G, case):
    fluxes_f, vd = util.ICE_CONFIGS["sea_ice_corrected"]()
    ice_params = ic.flux_params(fluxes_f, velocity_difference=vd)
    g = orc.make_grid(G.nx, G.ny, G.hx, G.hy, G.ring)
    at = util.polar_atmosphere(orc.interpolate_atmosphere_state(g, case["src"], case["weights"], 0, 1, TF))
    return ice_params, g, at


@gpu
@pytest.mark.parametrize("hx, hy, ring", [(2, 7, 1), (1, 1, 0)])
@pytest.mark.parametrize("scheme", [abi.SKIN_EXPLICIT, abi.SKIN_SEMI_IMPLICIT])
def test_compute_atmosphere_sea_ice_fluxes_in_place_skin(scheme, hx, hy, ring):
    """Reads the atmosphere (u, v, T, p, q, Q_s, Q_ℓ), the ice state and ocean S, mask on the window; writes the interface
    fluxes and `iterations` on the window.  The skin temperature is updated IN PLACE (top_temperature is
    out.temperature): outside the window it keeps its input bits."""
    G = Geom(hx, hy, ring)
    case = util.build_case(NX, NY, hx, hy)
    ice_params, g, at = _ice_setup(G, case)
    props = ic.SeaIceInterfaceProperties(skin_temperature_scheme=scheme)
    state = case["ice_state"]

    def call(mem, G):
        ctx = make_ctx(G, ic.flux_params())
        ctx.set_sea_ice_formulation(ice_params, props.to_params())
        ocean = put_ocean(mem, G, case, ice_params, dict(S=G.win, mask=G.win))
        atmos = {k: mem.inp("atmos." + k, at[k], G.win if k not in ("Mp",) else np.zeros(G.shape, bool)) for k in EXCHANGE_NAMES}
        st = {k: mem.inp("ice." + k, state[k], G.win) for k in ICE_STATE_READS if k != "top_temperature"}
        skin = mem.inout("skin", state["top_temperature"], G.win, G.win)
        st["top_temperature"] = skin
        out = flux_outputs(mem, G, prefix="ai")
        del mem.outs["ai.temperature"]
        mem.watch = [x for x in mem.watch if x[0] != "ai.temperature"]
        out["temperature"] = skin
        res = mem.run(lambda: ctx.compute_atmosphere_sea_ice_fluxes(st, ocean, atmos, out), ctx)
        ctx.close()
        return res
    got = footprint(call, G)
    ref = orc.compute_atmosphere_sea_ice_fluxes(g, ice_params, props.to_params(), state, case["ocean"], at)
    gw = {k: G.W(got["ai." + k]) for k in util.ICE_FLUX_FIELDS if k != "temperature"}
    gw["temperature"], gw["iterations"] = G.W(got["skin"]), G.W(got["ai.iterations"])
    util.compare_ice_fluxes(gw, {k: G.W(v) for k, v in ref.items()}, 1e-9)


@gpu
@pytest.mark.parametrize("hx, hy", [(7, 2), (1, 1)])
def test_sea_ice_albedo_net_and_ice_ocean_fluxes(hx, hy):
    """cf_compute_sea_ice_albedo reads and writes every cell of the parent arrays (halos included);
    cf_compute_net_sea_ice_fluxes reads its inputs and writes top / bottom heat on the interior;
    cf_compute_sea_ice_ocean_fluxes reads T, S, mask, ℵ on the interior, τx also at i + 1, τy also at j + 1, and writes
    its outputs on the interior."""
    G = Geom(hx, hy, 0)
    case = util.build_case(NX, NY, hx, hy)
    ice_params, g, at = _ice_setup(G, case)
    props = ic.SeaIceInterfaceProperties()
    state = case["ice_state"]
    c = G.interior
    full = np.ones(G.shape, bool)
    rng = np.random.default_rng(5)
    hs = np.abs(rng.normal(0.05, 0.05, G.shape))
    Qf, Qi = rng.normal(size=G.shape), rng.normal(size=G.shape)
    ai = orc.compute_atmosphere_sea_ice_fluxes(g, ice_params, props.to_params(), state, case["ocean"], at)
    tau = dict(x=rng.normal(0, 1e-4, G.shape), y=rng.normal(0, 1e-4, G.shape))

    def call(mem, G):
        ctx = make_ctx(G, ic.flux_params())
        ctx.set_sea_ice_formulation(ice_params, props.to_params())
        A = ctx.default_sea_ice_albedo_params()
        hi = mem.inp("albedo.hi", state["thickness"], full)
        hsn = mem.inp("albedo.hs", hs, full)
        ts = mem.inp("albedo.Ts", state["top_temperature"], full)
        alb = mem.out("albedo", G.shape, full)
        ocean = put_ocean(mem, G, case, ice_params, dict(T=c, S=c, mask=c))
        st = dict(concentration=mem.inp("ice.concentration", state["concentration"], c),
                  albedo=mem.inp("ice.albedo", state["albedo"], c))
        atmos = {k: mem.inp("atmos." + k, at[k], c) for k in ("Qs", "Ql")}
        aif = {k: mem.inp("ai." + k, ai[k], c) for k in ("sensible_heat", "latent_heat", "temperature")}
        qf, qi = mem.inp("frazil", Qf, c), mem.inp("interface", Qi, c)
        nice = dict(top_heat=mem.out("top_heat", G.shape, c), bottom_heat=mem.out("bottom_heat", G.shape, c))
        tx = mem.inp("tau_x", tau["x"], c | G.box(0, di=1))
        ty = mem.inp("tau_y", tau["y"], c | G.box(0, dj=1))
        conc = mem.inp("conc", state["concentration"], c)
        io = {k: mem.out("io." + k, G.shape, c) for k in ("interface_heat", "salt_flux", "frazil_heat", "friction_velocity")}
        P = ctx.default_ice_ocean_params(time_step=600.0, top_cell_thickness=10.0)

        def fn():
            ctx.compute_sea_ice_albedo(A, hi, hsn, ts, alb)
            ctx.compute_net_sea_ice_fluxes(st, ocean, atmos, aif, nice, frazil_heat=qf, interface_heat=qi)
            ctx.compute_sea_ice_ocean_fluxes(P, ocean, conc, tx, ty, io)
        res = mem.run(fn, ctx)
        store.update(A=A, P=P)
        ctx.close()
        return res
    store = {}
    got = footprint(call, G)
    ref = orc.compute_net_sea_ice_fluxes(g, ice_params, props.to_params(), state, case["ocean"], at, ai, Qf, Qi)
    for k in ("top_heat", "bottom_heat"):
        assert util.rel_err(G.W(got[k], 0), G.W(ref[k], 0), 1.0) <= 1e-12, k
    want = orc.sea_ice_albedo(store["A"], state["thickness"], hs, state["top_temperature"])
    assert util.rel_err(got["albedo"], want, 1.0) <= 1e-12
    io = orc.sea_ice_ocean_fluxes(g, ice_params, store["P"], case["ocean"], state["concentration"], tau["x"], tau["y"])
    for k in ("interface_heat", "salt_flux", "frazil_heat", "friction_velocity"):
        assert util.rel_err(G.W(got["io." + k], 0), G.W(io[k], 0), 1e-9) <= 1e-12, k


@gpu
def test_update_state_sea_ice():
    """cf_update_state_sea_ice: the footprint of cf_update_state, then the interface solve and the net sea-ice fluxes (the
    skin temperature in place: top_temperature is the interface temperature output)."""
    hx, hy, ring = 8, 3, 1
    G = Geom(hx, hy, ring)
    case = util.build_case(NX, NY, hx, hy)
    fluxes_f, vd = util.ICE_CONFIGS["sea_ice_ncar"]()
    ice_params = ic.flux_params(fluxes_f, velocity_difference=vd)
    params = ic.flux_params()
    props = ic.SeaIceInterfaceProperties()
    state = case["ice_state"]
    Qf, Qi = case["ocean"]["T"] * 0.1, case["ocean"]["S"] * 0.01

    def call(mem, G):
        ctx = make_ctx(G, params)
        ctx.set_sea_ice_formulation(ice_params, props.to_params())
        src, w = put_src(mem, case), put_weights(mem, G, case, ring)
        ocean = put_ocean(mem, G, case, params, ocean_reads(G))
        icef = put_ice(mem, G, case)
        atmos = {k: mem.out("atmos." + k, G.shape, G.win) for k in EXCHANGE_NAMES}
        fl = flux_outputs(mem, G)
        net = {k: mem.out("net." + k, G.shape, G.interior) for k in NET_NAMES}
        st = {k: mem.inp("ice." + k, state[k], G.win) for k in ICE_STATE_READS if k != "top_temperature"}
        st["concentration"] = mem.inp("ice.state_concentration", state["concentration"], G.win)
        skin = mem.inout("skin", state["top_temperature"], G.win, G.win)
        st["top_temperature"] = skin
        ai = {k: mem.out("ai." + k, G.shape, G.win) for k in FLUX_NAMES + FLUX_OPTIONAL if k != "temperature"}
        ai["iterations"] = mem.out("ai.iterations", G.shape, G.win, dtype=torch.int32)
        ai["temperature"] = skin
        qf, qi = mem.inp("frazil", Qf, G.interior), mem.inp("interface", Qi, G.interior)
        nice = dict(top_heat=mem.out("top_heat", G.shape, G.interior), bottom_heat=mem.out("bottom_heat", G.shape, G.interior))
        out = mem.run(lambda: ctx.update_state_sea_ice(src, w, ocean, atmos, fl, net, icef, st, ai, nice, frazil_heat=qf,
                                                       interface_heat=qi, time_fraction=TF), ctx)
        ctx.close()
        return out
    got = footprint(call, G)
    # the ocean path against the oracle ...
    g = orc.make_grid(NX, NY, hx, hy, ring)
    at = orc.interpolate_atmosphere_state(g, case["src"], case["weights"], 0, 1, TF)
    fl = orc.compute_atmosphere_ocean_fluxes(g, params, case["ocean"], at, nthreads=0)
    net = orc.compute_net_ocean_fluxes(g, params, case["ocean"], at, fl, ice=case["ice"], weights=case["weights"])
    shaped = dict(atmos={k: got["atmos." + k] for k in EXCHANGE_NAMES},
                  fluxes={k: got["fluxes." + k] for k in FLUX_NAMES + FLUX_OPTIONAL},
                  net={k: got["net." + k] for k in NET_NAMES})
    compare(case, shaped, dict(atmos=at, fluxes=fl, net=net), ring)
    # ... and the sea-ice stages are, bit for bit, the two entry points on the exchange fields the step computed (which
    # test_compute_atmosphere_sea_ice_fluxes_in_place_skin and test_sea_ice_albedo_net_and_ice_ocean_fluxes hold to the
    # oracle on a polar atmosphere; on this warm one the slow skin-temperature cells amplify table rounding past 1e-6)
    ctx = make_ctx(G, params)
    ctx.set_sea_ice_formulation(ice_params, props.to_params())
    dev = ctx.to_device
    atmos = {k: dev(got["atmos." + k]) for k in EXCHANGE_NAMES}
    ocean = {k: dev(case["ocean"][k]) for k in ("T", "S", "u", "v", "mask")}
    st = {k: dev(v) for k, v in state.items()}
    ai = ctx.field_set(FLUX_NAMES, FLUX_OPTIONAL)
    ai["iterations"] = ctx.zeros(torch.int32)
    ctx.compute_atmosphere_sea_ice_fluxes(st, ocean, atmos, ai)
    nice = ctx.field_set(("top_heat", "bottom_heat"))
    ctx.compute_net_sea_ice_fluxes(st, ocean, atmos, ai, nice, frazil_heat=dev(Qf), interface_heat=dev(Qi))
    ctx.sync()
    for k, v in ai.items():
        name = "skin" if k == "temperature" else "ai." + k
        np.testing.assert_array_equal(bits(G.W(got[name])), bits(G.W(v.cpu().numpy())), err_msg=k)
    for k, v in nice.items():
        np.testing.assert_array_equal(bits(G.W(got[k], 0)), bits(G.W(v.cpu().numpy(), 0)), err_msg=k)
    ctx.close()


# ---------------------------------------------------------------------------------------------
# land freshwater, salinity restoring and normalisation
# ---------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("hx, hy, ring", [(2, 7, 1), (7, 2, 0)])
def test_land_freshwater_and_salinity(hx, hy, ring):
    """cf_interpolate_land_freshwater reads the whole window of both sources and writes the ring window;
    cf_materialize_salinity_restoring reads S★, S, mask on the interior and writes the interior;
    cf_normalize_salinity_flux reads flux, additional, area and mask on the interior and subtracts the mean from EVERY
    cell of the parent array, halos included (poison there comes out as poison − mean)."""
    G = Geom(hx, hy, ring)
    case = util.build_case(NX, NY, hx, hy)
    land = syn.jra55_land_snapshots(2)
    params = ic.flux_params()
    c = G.interior
    rng = np.random.default_rng(11)
    target = case["ocean"]["S"] + rng.normal(0, 0.1, G.shape)
    flux0 = rng.normal(0, 1e-5, G.shape)
    area = 1.0 + rng.random(G.shape)
    vp = 1.0 / 6.0 / 86400.0
    full = np.ones(G.shape, bool)

    def call(mem, G):
        ctx = make_ctx(G, params)
        fr = mem.inp("friver", land["friver"])
        lc = mem.inp("licalvf", land["licalvf"])
        w = put_weights(mem, G, case, ring)
        Mr = mem.out("land", G.shape, G.win)
        ocean = put_ocean(mem, G, case, params, dict(S=c, mask=c))
        tgt = mem.inp("target", target, c)
        add = mem.out("additional", G.shape, c)
        flux = mem.inout("flux", flux0, c, full)
        ar = mem.inp("area", area, c)
        mean = mem.out("mean", (1,), np.ones(1, bool))

        def fn():
            ctx.interpolate_land_freshwater(fr, lc, w, Mr, 0, 1, TF)
            ctx.materialize_salinity_restoring(vp, tgt, ocean, add)
            ctx.normalize_salinity_flux(flux, ocean["mask"], add, ar, mean)
        out = mem.run(fn, ctx)
        ctx.close()
        return out

    res = {}
    for mode in ("plain",) + POISONS:     # footprint() with the normalised halo checked as input − mean
        mem = Mem(mode)
        mem.G = G
        res[mode] = call(mem, G)
        if mode != "plain":
            poisoned = res[mode]["flux"]
            m = res[mode]["mean"][0]
            assert m == res["plain"]["mean"][0]
            for k in ("land", "additional"):
                wset = G.win if k == "land" else c
                np.testing.assert_array_equal(bits(res[mode][k])[wset], bits(res["plain"][k])[wset], err_msg=f"[{mode}] {k}")
            np.testing.assert_array_equal(bits(poisoned)[c], bits(res["plain"]["flux"])[c], err_msg=f"[{mode}] flux")
            inp = flux0.copy()
            inp[~c] = np.nan if mode == "nan" else ABSURD
            np.testing.assert_array_equal(bits(poisoned), bits(inp - m), err_msg=f"[{mode}] flux outside the interior")
    got = res["plain"]
    g = orc.make_grid(NX, NY, hx, hy, ring)
    ref = orc.interpolate_land_freshwater(g, land["friver"], land["licalvf"], case["weights"], 0, 1, TF)
    assert util.rel_err(G.W(got["land"]), G.W(ref), 1e-9) <= 1e-12
    want_add = np.where(case["ocean"]["mask"] != 0, vp * (case["ocean"]["S"] - target), 0.0)
    assert util.rel_err(G.W(got["additional"], 0), G.W(want_add, 0), 1e-12) <= 1e-12
    want, m = orc.normalize_salinity_flux(g, params, flux0, case["ocean"]["mask"], got["additional"], area)
    assert abs(got["mean"][0] - m) <= 1e-12 * max(abs(m), 1e-12)
    assert util.rel_err(got["flux"], want, 1e-7) <= 1e-12


# ---------------------------------------------------------------------------------------------
# halo rows: the tripolar fold and the peer-direct exchange
# ---------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("hx, hy, rows", [(7, 2, 2), (2, 7, 2), (3, 1, 1)])
def test_fold_north_halo(hx, hy, rows):
    """Reads interior rows ny − 1 − rows … ny − 1 (interior columns); writes the `rows` north halo rows over the full
    width nx + 2hx; every other cell keeps its bits.  (A tripolar grid has an even number of columns.)"""
    nx = NX + 1
    G = Geom(hx, hy, 0, nx=nx)
    rng = np.random.default_rng(2)
    host = [rng.normal(size=G.shape) for _ in range(4)]
    locs = [abi.FOLD_CENTER, abi.FOLD_CENTER, abi.FOLD_X_FACE, abi.FOLD_Y_FACE]
    names = ("center", "center", "x_face", "y_face")
    signs = [1.0, -1.0, -1.0, -1.0]
    read = np.zeros(G.shape, bool)
    read[hy + NY - 1 - rows:hy + NY, hx:hx + nx] = True
    write = np.zeros(G.shape, bool)
    write[hy + NY:hy + NY + rows, :] = True

    def call(mem, G):
        ctx = make_ctx(G, ic.flux_params())
        ts = [mem.inout(f"f{n}", a, read, write) for n, a in enumerate(host)]
        out = mem.run(lambda: ctx.fold_north_halo(ts, locs, signs, rows=rows), ctx)
        ctx.close()
        return out
    got = footprint(call, G)
    for n, (a, loc, sg) in enumerate(zip(host, names, signs)):
        t = torch.from_numpy(a.copy())
        fold_north_halo_torch(t, nx, NY, hx, hy, rows, loc, sg)
        np.testing.assert_array_equal(got[f"f{n}"], t.numpy(), err_msg=loc)


@gpu
@pytest.mark.parametrize("mode", POISONS)
def test_peer_halo_rows_unequal_halos(mode):
    """Two latitude slabs as two contexts in one process, hx = 7 != hy = 2: the exchange reads the `rows` boundary rows over
    the full width nx + 2hx and writes the `rows` halo rows next to the neighbour, full width; no other cell changes.  The
    rows that arrive are held to the single-domain state itself (a copy: there is no plain call to compare with)."""
    hx, hy, rows, world, ny_g = 7, 2, 2, 2, 2 * NY
    full = syn.ocean_state(NX, ny_g, hx, hy)
    mems = [Mem(mode, seed=r) for r in range(world)]
    slabs = []
    for r in range(world):
        j0, j1 = slab_bounds(ny_g, r, world)
        ny = j1 - j0
        G = Geom(hx, hy, 1, ny=ny)
        mems[r].G = G
        o = syn.ocean_state(NX, ny, hx, hy, ny_global=ny_g, j_offset=j0)
        read = np.zeros(G.shape, bool)
        write = np.zeros(G.shape, bool)
        if r == 0:
            read[hy + ny - rows:hy + ny] = True
            write[hy + ny:hy + ny + rows] = True
        else:
            read[hy:hy + rows] = True
            write[hy - rows:hy] = True
        ctx = make_ctx(G, ic.flux_params())
        ctx._check(ctx.lib.cf_set_stream(ctx._h, None), "cf_set_stream")
        fields = [mems[r].inout(k, o[k], read, write) for k in ("T", "S", "u", "v")]
        slabs.append((ctx, fields, j0, j1, G))
    handles = [s[0].peer_halo_export(4, rows) for s in slabs]
    for r, s in enumerate(slabs):
        s[0].peer_halo_connect(handles[r - 1] if r > 0 else None, handles[r + 1] if r < world - 1 else None, r, world)
    before = [s[0].peer_halo_stats()[0] for s in slabs]
    torch.cuda.synchronize()
    snaps = [[(n, t, w, bits(util.buffer_of(t)[0].cpu().numpy())) for n, t, w in m.watch] for m in mems]
    for ctx, fields, *_ in slabs:      # both launched before either is waited for
        ctx.halo_exchange_rows_peer(fields, rows=rows)
    for r, (ctx, fields, j0, j1, G) in enumerate(slabs):
        ctx.sync()
        assert ctx.peer_halo_stats()[0] == before[r] + 1
        for n, t, write, snap in snaps[r]:
            flat, start = util.buffer_of(t)
            after = bits(flat.cpu().numpy())
            allowed = np.zeros(after.shape, bool)
            allowed[start:start + t.numel()] = write.reshape(-1)
            assert not ((after != snap) & ~allowed).any(), (r, n)
            got = t.cpu().numpy()
            lo, hi = (hy + G.ny, hy + G.ny + rows) if r == 0 else (hy - rows, hy)
            np.testing.assert_array_equal(got[lo:hi], full[n][j0 + lo:j0 + hi], err_msg=f"rank {r} {n}")
    for s in slabs:
        s[0].close()
