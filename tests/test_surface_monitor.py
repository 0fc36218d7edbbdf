"""GPU tests of the surface monitor (include/coflux.h: cf_monitor_*, cf_attach_monitor; the host mirror's SurfaceExtrema,
Progress, omip_progress_callback and NaNChecker).

Every comparison is an equality of bits against the NumPy restatement in monitor_reference.py: the minima and maxima in the
IEEE total order with their smallest indices, the counts, the first non-finite index and the 64-bit hash.  There is no
tolerance anywhere — every quantity is an exact reduction, so the bits may not depend on the launch geometry, the halo
widths, where the arrays start, or on who made the collection, and the tests show that."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import monitor_reference as mr
import util
from coflux import abi
from coflux import interface_computations as ic
from coflux import models as cm
from coflux.runtime import CofluxError, EXCHANGE_NAMES, FLUX_NAMES, NET_NAMES, FluxContext
from test_layout_footprint import Geom, footprint
from test_steps import H as STEP_H
from test_steps import INC, _setup
from test_time_average import DT, H, NX, NY, _model, interior

pytestmark = pytest.mark.gpu

DBL_MAX = 1.7976931348623157e308
NAN = float("nan")


def embed(a, hx, hy, fill):
    ny, nx = a.shape
    g = np.full((ny + 2 * hy, nx + 2 * hx), fill, dtype=a.dtype)
    g[hy:hy + ny, hx:hx + nx] = a
    return g


def reference(fields, wet, first_cell=0):
    """the record (array of n_entries values) of `fields` = [(interior array, kind)]"""
    return np.array([mr.monitor_value(x, wet, kind, first_cell) for x, kind in fields], dtype=mr.DTYPE)


class Surface:
    """One context of a shape with device copies of interior arrays, plain or as odd-offset views inside guarded buffers."""

    def __init__(self, nx, ny, hx, hy):
        self.nx, self.ny, self.hx, self.hy = nx, ny, hx, hy
        self.ctx = FluxContext(nx, ny, hx, hy, ic.flux_params(), ring=0)
        self.shape, self.n = (ny + 2 * hy, nx + 2 * hx), 0

    def put(self, a, fill, views=False):
        t = torch.from_numpy(np.ascontiguousarray(embed(a, self.hx, self.hy, fill)))
        if not views:
            return t.cuda()
        self.n += 1
        v = util.guarded(self.shape, t.dtype, offset=(1, 3, 5)[self.n % 3], guard=64, fill=fill)
        v.copy_(t)
        return v

    def record(self, fields, wet=None, views=False, first_cell=0, **kw):
        """one collection of [(interior array, kind)] under the interior uint8 mask `wet`; each distinct array is uploaded once"""
        dev = {}
        for x, _ in fields:
            if id(x) not in dev:
                dev[id(x)] = self.put(x, NAN, views)
        mask = None if wet is None else self.put(wet.astype(np.uint8), 1, views)
        m = self.ctx.monitor([(dev[id(x)], kind) for x, kind in fields], mask=mask, first_cell=first_cell, capacity=1, **kw)
        m.collect(0.5)
        values, times = m.read()
        assert values.shape == (1, len(fields)) and list(times) == [0.5]
        before = {k: t.clone() for k, t in dev.items()}
        m.close()
        for k, t in dev.items():
            assert torch.equal(t.view(torch.int64), before[k].view(torch.int64))
        return values[0].copy()

    def close(self):
        self.ctx.close()


def mixed_field(rng, nx, ny, specials=True):
    """finite values of many magnitudes with both zeros, ties, denormals, and a few NaN / ±Inf"""
    x = rng.standard_normal((ny, nx)) * 10.0 ** rng.integers(-3, 4, (ny, nx))
    if specials and x.size >= 16:
        flat = x.reshape(-1)
        pos = rng.permutation(flat.size)[:max(8, flat.size // 50)]
        kinds = [0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, -5e-324, 7.0, 7.0, -7.0]
        flat[pos] = (kinds + list(rng.choice(kinds, pos.size)))[:pos.size]        # (the first eight: one of each kind)
    return x


# ---- shapes and launch geometry ----------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 1, 1), (2, 1, 1, 1), (64, 16, 2, 2), (41, 25, 3, 2), (77, 23, 3, 2), (331, 67, 2, 1), (1440, 560, 7, 7)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_shape_gives_the_reference_bits_under_every_launch_geometry(shape):
    nx, ny, hx, hy = shape
    rng = np.random.default_rng(nx * 1000 + ny)
    a, b, c = mixed_field(rng, nx, ny), mixed_field(rng, nx, ny), mixed_field(rng, nx, ny, specials=False)
    wet = (rng.random((ny, nx)) < 0.8).astype(np.uint8)
    fields = [(a, "value"), (a, "abs"), (b, "value"), (c, "abs"), (c, "value")]
    want = reference(fields, wet, first_cell=12345)
    if nx * ny > 1000:
        assert want["nan_count"][0] > 0 and want["inf_count"][0] > 0 and want["nan_count"][4] == 0
    s = Surface(nx, ny, hx, hy)
    for views in (False, True):
        for cap in (0, 1, 3):
            got = s.record(fields, wet, views=views, first_cell=12345, max_workgroups=cap)
            assert mr.same(got, want), (views, cap, got, want)
    assert mr.same(s.record(fields[:1], None, first_cell=0), reference(fields[:1], None)), "no mask: all wet"
    s.close()


# ---- designed fields ---------------------------------------------------------------------------------------------------------
DNX, DNY, DHX, DHY = 77, 23, 3, 2          # 1771 cells: cells 1023 and 1024 exist, four slices of 256 pairs
DN = DNX * DNY


def _base(seed):
    return np.random.default_rng(seed).uniform(-100.0, 100.0, DN)       # no ties, no specials, |x| < 100


def designed_cases(wet):
    """name → (flat interior array, {property: expected value under THIS mask}) — the expectation is stated only where the
    designed cells are wet; the reference is compared in every case"""
    w = wet.reshape(-1) != 0
    all_wet = bool(w.all())
    cases = {}

    def case(name, x, **expect):
        cases[name] = (x, expect if all_wet else {})

    x = _base(1); x[0], x[DN - 1] = 1e6, -1e6
    case("first and last cell", x, argmax=0, argmin=DN - 1)
    x = _base(2); x[DNX - 1], x[DNX] = 1e6, -1e6
    case("a row's last cell and the next row's first", x, argmax=DNX - 1, argmin=DNX)
    x = _base(3); x[1023], x[1024] = 1e6, -1e6
    case("cells 1023 and 1024", x, argmax=1023, argmin=1024)
    x = _base(4); x[128], x[127] = 1e6, -1e6                       # thread 64 = lane 0 of wave 1; thread 63 = lane 63 of wave 0
    case("lane 0 and lane 63", x, argmax=128, argmin=127)
    x = _base(5); x[200] = x[201] = 1e6; x[10] = x[138] = -1e6    # one thread's pair; lane 5 of waves 0 and 1
    case("ties in a pair and in two waves", x, argmax=200, argmin=10)
    x = _base(6); x[1700] = x[5] = 1e6; x[1769] = x[3] = -1e6
    case("ties far apart", x, argmax=5, argmin=3)
    x = np.abs(_base(7)) + 1.0; x[7], x[40], x[900], x[1000] = 0.0, -0.0, -0.0, 0.0
    case("both zeros below", x, argmin=40, minimum=-0.0)
    x = -np.abs(_base(8)) - 1.0; x[9], x[33], x[901], x[1001] = -0.0, 0.0, 0.0, -0.0
    case("both zeros above", x, argmax=33, maximum=0.0)
    x = _base(9); x[300], x[301], x[50] = np.inf, -np.inf, np.inf
    case("infinities are extrema", x, argmax=50, argmin=301, maximum=np.inf, minimum=-np.inf, inf_count=3, first_nonfinite=50)
    x = np.random.default_rng(10).choice([5e-324, -5e-324, 2.2250738585072014e-308, 1e-310, -1e-310], DN); x[77], x[78] = -DBL_MAX, DBL_MAX
    case("-DBL_MAX and denormals", x, argmin=77, argmax=78, minimum=-DBL_MAX)
    x = _base(11); x[w] = np.nan
    cases["NaN on every wet cell"] = (x, dict(minimum=np.inf, maximum=-np.inf, argmin=-1, argmax=-1, nan_count=int(w.sum()),
                                              first_nonfinite=int(np.flatnonzero(w)[0]) if w.any() else -1))
    b = mr.bits(_base(12)).copy(); b[100], b[101], b[102] = 0xFFF8000000000001, 0x7FF0000000000001, 0x7FF8DEAD00000000
    case("signed NaN and payloads", mr.from_bits(b), nan_count=3, inf_count=0, first_nonfinite=100)
    b = b.copy(); b[100], b[101], b[102] = 0x7FF8000000000000, 0xFFFFFFFFFFFFFFFF, 0x7FF8DEAD00000001
    case("other payloads", mr.from_bits(b), nan_count=3, inf_count=0, first_nonfinite=100)
    x = _base(13); x[444], x[445] = -1e7, 1e6
    case("the largest |x| is negative", x, argmin=444)
    x = _base(14)
    land = np.flatnonzero(~w)
    if land.size >= 3:
        x[land[0]], x[land[1]], x[land[-1]] = np.nan, np.inf, 1e308
    cases["NaN, Inf and 1e308 on land only"] = (x, dict(nan_count=0, inf_count=0, first_nonfinite=-1) if land.size >= 3 else {})
    x = _base(15); x[1500], x[600], x[1200] = np.nan, np.inf, np.nan
    case("the first non-finite cell", x, first_nonfinite=600, nan_count=2, inf_count=1)
    return cases


@pytest.fixture(scope="module")
def designed_surface():
    s = Surface(DNX, DNY, DHX, DHY)
    yield s
    s.close()


MASKS = {"all wet": lambda: np.ones((DNY, DNX), np.uint8), "80 % wet": lambda: (np.random.default_rng(80).random((DNY, DNX)) < 0.8).astype(np.uint8),
         "all land": lambda: np.zeros((DNY, DNX), np.uint8)}


@pytest.mark.parametrize("mask", list(MASKS))
def test_designed_fields_as_value_and_abs(designed_surface, mask):
    wet = MASKS[mask]()
    cases = designed_cases(wet)
    assert len(cases) == 16
    arrays = {name: x.reshape(DNY, DNX) for name, (x, _) in cases.items()}
    for kind in ("value", "abs"):
        fields = [(arrays[name], kind) for name in cases]
        got = designed_surface.record(fields, wet)
        want = reference(fields, wet)
        for k, (name, (x, expect)) in enumerate(cases.items()):
            assert mr.same(got[k], want[k]), (mask, kind, name, got[k], want[k])
            if mask == "all land":
                assert (got[k]["minimum"], got[k]["maximum"], got[k]["argmin"], got[k]["argmax"]) == (np.inf, -np.inf, -1, -1)
                assert got[k]["nan_count"] == got[k]["inf_count"] == 0 and got[k]["first_nonfinite"] == -1 and got[k]["hash"] == mr.state_hash(x)
                continue
            for prop, value in expect.items():
                if kind == "abs" and prop in ("argmin", "argmax", "minimum", "maximum"):
                    continue            # stated for y = x; under ABS the reference alone speaks, but for the cases below
                assert mr.bits(np.float64(got[k][prop])) == mr.bits(np.float64(value)) if prop in ("minimum", "maximum") else got[k][prop] == value, \
                    (mask, kind, name, prop, got[k][prop], value)
        byname = dict(zip(cases, got))
        if mask == "all wet" and kind == "abs":
            v = byname["the largest |x| is negative"]
            assert v["maximum"] == 1e7 and v["argmax"] == 444
            v = byname["infinities are extrema"]
            assert v["maximum"] == np.inf and v["argmax"] == 50, "|−Inf| = +Inf ties with +Inf: the smaller index"
            v = byname["both zeros below"]
            assert v["minimum"] == 0 and not np.signbit(v["minimum"]) and v["argmin"] == 7, "|−0| = +0: the first zero of either sign"
        if mask != "all land":
            a, b = byname["signed NaN and payloads"], byname["other payloads"]
            assert a["nan_count"] == b["nan_count"] and a["inf_count"] == b["inf_count"] and a["hash"] != b["hash"], "counted alike, hashed differently"
            assert mr.bits(a["minimum"]) == mr.bits(b["minimum"]) and a["argmax"] == b["argmax"]
        if mask == "80 % wet":
            v, clean = byname["NaN, Inf and 1e308 on land only"], mr.monitor_value(_base(14), wet, kind)
            for prop in ("minimum", "maximum", "argmin", "argmax", "nan_count", "inf_count", "first_nonfinite"):
                assert mr.bits(np.float64(v[prop])) == mr.bits(np.float64(clean[prop])), prop
            assert v["hash"] != clean["hash"], "no trace but in the hash"


# ---- the hash ----------------------------------------------------------------------------------------------------------------
def test_the_hash_ignores_the_mask_and_sees_a_swap(designed_surface):
    rng = np.random.default_rng(21)
    x = mixed_field(rng, DNX, DNY)
    hashes = [designed_surface.record([(x, "value"), (x, "abs")], MASKS[m]())["hash"] for m in MASKS]
    hashes.append(designed_surface.record([(x, "value"), (x, "abs")], None)["hash"])
    for h in hashes:
        assert list(h) == [mr.state_hash(x)] * 2, "of the raw bits of x, never of y, whatever the mask"
    y = x.copy().reshape(-1)
    i, j = 17, 1203
    assert mr.bits(y[i]) != mr.bits(y[j])
    y[[i, j]] = y[[j, i]]
    swapped = designed_surface.record([(y.reshape(DNY, DNX), "value")], None)
    assert swapped["hash"][0] == mr.state_hash(y) != hashes[0][0]


def test_slabs_with_their_first_cell_combine_to_the_whole():
    nx, rows = 37, (5, 6)
    rng = np.random.default_rng(22)
    x, wet = mixed_field(rng, nx, sum(rows)), (rng.random((sum(rows), nx)) < 0.8).astype(np.uint8)
    x[x == np.inf] = 5.0
    x[7, 3] = x[2, 30] = np.inf               # the maximum twice, once per slab: the south slab's index wins
    wet[7, 3] = wet[2, 30] = 1
    fields = lambda a: [(a, "value"), (a, "abs")]  # noqa: E731
    whole = Surface(nx, sum(rows), 2, 3)
    south, north = Surface(nx, rows[0], 2, 3), Surface(nx, rows[1], 3, 2)
    W = whole.record(fields(x), wet)
    S = south.record(fields(x[:rows[0]]), wet[:rows[0]])
    N = north.record(fields(x[rows[0]:]), wet[rows[0]:], first_cell=rows[0] * nx)
    assert mr.same(W, reference(fields(x), wet))
    for e in range(2):
        assert (int(S["hash"][e]) + int(N["hash"][e])) % (1 << 64) == int(W["hash"][e]), "the wrapping sum of the slabs' hashes"
        assert mr.same(mr.combine(S[e], N[e]), W[e]), (e, S[e], N[e], W[e])
    assert W["argmax"][0] == 2 * nx + 30 and N["argmax"][0] == 7 * nx + 3
    for s in (whole, south, north):
        s.close()


# ---- footprint ---------------------------------------------------------------------------------------------------------------
_seen = []


def _monitor_call(mem, G):
    ctx = FluxContext(G.nx, G.ny, G.hx, G.hy, ic.flux_params(), ring=0)
    rng = np.random.default_rng(7)
    data = [mixed_field(rng, G.nx, G.ny, specials=False) for _ in range(3)]
    wet = (rng.random((G.ny, G.nx)) < 0.8).astype(np.uint8)
    dev = [mem.inp(f"f{k}", embed(a, G.hx, G.hy, 1.0), read=G.interior) for k, a in enumerate(data)]
    mask = mem.inp("mask", embed(wet, G.hx, G.hy, 1), read=G.interior)
    # 16 entries: every array is named more than once, as VALUE and as ABS
    m = ctx.monitor([(dev[k % 3], ("value", "abs")[(k // 3) % 2]) for k in range(16)], mask=mask, capacity=2)

    def run():
        m.collect()
        m.collect()

    out = mem.run(run, ctx)
    values = m.read()[0]
    assert mr.same(values[0], values[1]), "a second collection of unchanged inputs"
    assert mr.same(values[0], reference([(data[k % 3], ("value", "abs")[(k // 3) % 2]) for k in range(16)], wet))
    _seen.append(values[0].copy())
    m.close()
    ctx.close()
    return out


@pytest.mark.parametrize("halo", [(2, 7), (7, 2), (1, 1)])
def test_collect_reads_the_interior_only_and_writes_no_caller_array(halo):
    """Every array poisoned outside I (NaN, then a finite absurd value; masks 0xFF / random), at odd offsets inside guarded
    buffers: no byte of any caller buffer changes, and the records are the plain call's — and the reference's — bit for bit."""
    _seen.clear()
    G = Geom(halo[0], halo[1], 0, nx=77, ny=23)
    footprint(_monitor_call, G)
    assert len(_seen) == 3
    for rec in _seen[1:]:
        assert mr.same(rec, _seen[0])


def test_nan_halos_of_unequal_widths_change_nothing():
    rng = np.random.default_rng(31)
    x, wet = mixed_field(rng, 41, 25), (rng.random((25, 41)) < 0.8).astype(np.uint8)
    fields = [(x, "value"), (x, "abs")]
    want = reference(fields, wet)
    for hx, hy in ((1, 1), (2, 7), (7, 2), (3, 4)):
        s = Surface(41, 25, hx, hy)
        for views in (False, True):
            assert mr.same(s.record(fields, wet, views=views), want), (hx, hy, views)
        s.close()


# ---- the series, the status and the errors -------------------------------------------------------------------------------------
def test_series_collect_count_subranges_reading_twice_reset_and_a_full_series():
    ctx = FluxContext(40, 12, 2, 2, ic.flux_params(), ring=0)
    a, b = ctx.zeros(), ctx.zeros()
    m = ctx.monitor([a, (b, "abs")], capacity=3)
    assert m.count() == 0 and m.capacity == 3 and m.read()[0].shape == (0, 2)
    want = []
    for k in range(3):
        a.fill_(float(k + 1))
        b.fill_(-float(k + 1))
        m.collect(10.0 * k)
        want.append(reference([(np.full((12, 40), k + 1.0), "value"), (np.full((12, 40), -(k + 1.0)), "abs")], None))
    values, times = m.read()
    assert m.count() == 3 and values.dtype == abi.MONITOR_VALUE_DTYPE and list(times) == [0.0, 10.0, 20.0]
    assert mr.same(values, np.array(want)) and list(values["maximum"][:, 1]) == [1.0, 2.0, 3.0]
    with pytest.raises(CofluxError, match="full"):
        m.collect(30.0)
    assert m.count() == 3 and mr.same(m.read()[0], values), "a full series fails with nothing written; reading does not consume"
    sub, sub_t = m.read(1, 2)
    assert mr.same(sub, values[1:]) and list(sub_t) == [10.0, 20.0] and mr.same(m.read(2, 1)[0], values[2:]) and m.read(3, 0)[0].shape == (0, 2)
    assert m.lib.cf_monitor_read(m._h, 1, 1, sub.ctypes.data, None) == 0      # times may be NULL
    for first, n in ((0, 4), (-1, 1), (3, 1), (2, -1)):
        with pytest.raises(CofluxError, match="cf_monitor_read"):
            m.read(first, n)
    m.reset()
    assert m.count() == 0
    m.collect(7.0)
    values2, times2 = m.read()
    assert mr.same(values2[0], values[2]) and list(times2) == [7.0]
    m.close()
    ctx.close()


def test_status_names_the_first_bad_record_and_its_entries_and_reset_clears_it():
    ctx = FluxContext(40, 12, 2, 2, ic.flux_params(), ring=0)
    a, b, c = ctx.zeros(), ctx.zeros(), ctx.zeros()
    wet = torch.ones(ctx.shape, dtype=torch.uint8, device="cuda")
    wet[2 + 3, 2 + 5] = 0
    m = ctx.monitor([a, b, (c, "abs")], mask=wet, capacity=8)
    a[2 + 3, 2 + 5] = float("nan")            # land: never bad
    a[0, 0] = float("nan")                    # halo
    for _ in range(3):
        m.collect()
    assert m.status() == (-1, 0)
    c[2 + 4, 2 + 1] = float("inf")            # planted before collection 3 (the fourth), entries 0 and 2
    a[2 + 7, 2 + 9] = float("nan")
    m.collect()
    assert m.status() == (3, 0b101)
    b[2 + 1, 2 + 1] = float("-inf")           # a later record with other entries does not move it
    m.collect()
    a[2 + 7, 2 + 9], c[2 + 4, 2 + 1], b[2 + 1, 2 + 1] = 0.0, 0.0, 0.0      # nor does cleaning the fields
    m.collect()
    assert m.status() == (3, 0b101)
    values = m.read()[0]
    assert list(values["nan_count"][:, 0]) == [0, 0, 0, 1, 1, 0] and list(values["inf_count"][:, 1]) == [0, 0, 0, 0, 1, 0]
    assert values["first_nonfinite"][3, 0] == 7 * 40 + 9 and values["first_nonfinite"][3, 2] == 4 * 40 + 1
    m.reset()
    assert m.status() == (-1, 0) and m.count() == 0
    a[2 + 2, 2 + 2] = float("nan")
    m.collect()
    assert m.status() == (0, 0b001), "record numbers count from the reset"
    assert m.lib.cf_monitor_status(m._h, None, None) == 0
    m.close()
    ctx.close()


def test_errors_of_create_attach_and_an_orphaned_monitor():
    ctx = FluxContext(40, 12, 2, 2, ic.flux_params(), ring=1)
    a = ctx.zeros()
    for entries, match in (([], "0 entries"), ([a] * 17, "17 entries"), ([(None, "value")], "NULL a"), ([(a, 2)], "unknown kind"), ([(a, -1)], "unknown kind")):
        with pytest.raises((CofluxError, ValueError), match=match):
            ctx.monitor(entries)
    for capacity in (0, -3):
        with pytest.raises(CofluxError, match="capacity"):
            ctx.monitor([a], capacity=capacity)
    with pytest.raises(CofluxError, match="max_workgroups"):
        ctx.monitor([a], max_workgroups=-1)
    desc = abi.MonitorDesc()
    desc.n_entries, desc.entries[0].kind, desc.entries[0].a = 1, abi.MONITOR_VALUE, a.data_ptr()
    h = C.c_void_p()
    for size in (0, C.sizeof(abi.MonitorDesc) - 8, C.sizeof(abi.MonitorDesc) + 8):
        desc.struct_size = size
        assert ctx.lib.cf_monitor_create(ctx._h, C.byref(desc), 4, C.byref(h)) == -1 and not h.value     # CF_ERR_INVALID
    desc.struct_size, desc.n_entries = C.sizeof(abi.MonitorDesc), 17
    assert ctx.lib.cf_monitor_create(ctx._h, C.byref(desc), 4, C.byref(h)) == -1 and not h.value
    desc.n_entries = 1
    assert ctx.lib.cf_monitor_create(ctx._h, C.byref(desc), 4, C.byref(h)) == 0 and h.value
    assert ctx.lib.cf_monitor_destroy(h) == 0
    m = ctx.monitor([a, (a, "abs")], capacity=2)
    for stride in (0, -2):
        with pytest.raises(CofluxError, match="stride"):
            ctx.attach_monitor(m, stride, 0.0, 1.0)
    with pytest.raises(CofluxError, match="finite"):
        ctx.attach_monitor(m, 1, float("nan"), 1.0)
    other = FluxContext(40, 12, 2, 2, ic.flux_params(), ring=1)
    with pytest.raises(CofluxError, match="another context"):
        other.attach_monitor(m, 1, 0.0, 1.0)
    other.close()
    ctx.close()
    # a monitor outlived by its context: every call fails, destroying it does not
    for call in (m.collect, m.count, m.read, m.status, m.reset):
        with pytest.raises(CofluxError, match="context has been destroyed"):
            call()
    m.close()
    # destroying an attached monitor detaches it: cf_time_steps goes on as without one
    ctx, states, src, w, _ = _setup()
    fl, net = ctx.field_set(FLUX_NAMES), ctx.field_set(NET_NAMES)
    m = _step_monitor(ctx, fl, net, states)
    ctx.attach_monitor(m, 1, 0.0, 1.0)
    m.close()
    sched = ctx.make_schedule(states, [ctx.field_set(EXCHANGE_NAMES)], time_fraction_increment=INC)
    ctx.time_steps(0, 3, sched, src, w, fl, net)
    ctx.sync()
    ctx.close()


# ---- the stepping loop -----------------------------------------------------------------------------------------------------
def _step_monitor(ctx, fl, net, states, capacity=64):
    return ctx.monitor([net["T"], net["S"], (net["u"], "abs"), (net["v"], "abs"), fl["latent_heat"], states[0]["T"]], mask=states[0]["mask"],
                       capacity=capacity)


def _step_integrator(ctx, fl, net, states):
    return ctx.integrals([("one",), ("field", net["T"]), ("product", fl["sensible_heat"], fl["latent_heat"])], mask=states[0]["mask"], capacity=64)


def _host_loop(ctx, states, src, w, n, stride, n_levels=4):
    atmos, fl, net = ctx.field_set(EXCHANGE_NAMES), ctx.field_set(FLUX_NAMES), ctx.field_set(NET_NAMES)
    m = _step_monitor(ctx, fl, net, states)
    for s in range(n):
        tot = s * INC
        l1 = int(tot) % n_levels
        ctx.update_state(src, w, states[s % 2], atmos, fl, net, level1=l1, level2=(l1 + 1) % n_levels, time_fraction=tot - int(tot))
        if (s + 1) % stride == 0:
            m.collect(100.0 + (s + 1) * 1200.0)
    return fl, net, m.read()


def _stepped(ctx, states, src, w, calls, pipeline, stride=None, others=False):
    sets = [ctx.field_set(EXCHANGE_NAMES) for _ in range(2 if pipeline else 1)]
    fl, net = ctx.field_set(FLUX_NAMES), ctx.field_set(NET_NAMES)
    sched = ctx.make_schedule(states, sets, first_level=0, time_fraction=0.0, time_fraction_increment=INC, pipeline=pipeline)
    m = q = avg = None
    if stride is not None:
        m = _step_monitor(ctx, fl, net, states)
        ctx.attach_monitor(m, stride, 100.0, 1200.0)
    means = [ctx.zeros(), ctx.zeros()]
    if others:
        avg = ctx.average([net["T"], fl["latent_heat"]], means)
        ctx.attach_average(avg, 2, 1200.0)
        q = _step_integrator(ctx, fl, net, states)
        ctx.attach_integrals(q, 3, 0.0, 1.0)
    for first, count in calls:
        ctx.time_steps(first, count, sched, src, w, fl, net)
    ctx.attach_monitor(None)
    ctx.attach_integrals(None)
    ctx.attach_average(None)
    ctx.sync()
    return fl, net, (m.read() if m is not None else None), (q.read()[0] if q is not None else None), means


@pytest.mark.parametrize("pipeline", [False, True, "merged"])
def test_time_steps_with_an_attached_monitor_equals_the_host_loop(pipeline):
    n = 13
    ctx, states, src, w, (o0, _) = _setup()
    rfl, rnet, (r1, t1) = _host_loop(ctx, states, src, w, n, 1)
    _, _, (r3, t3) = _host_loop(ctx, states, src, w, n, 3)
    assert r1.shape == (13, 6) and r3.shape == (4, 6) and list(t3) == [100.0 + k * 1200.0 for k in (3, 6, 9, 12)]
    assert mr.same(r3, r1[2::3]), "stride 3 collects what stride 1 collects at the same steps"
    assert not r1["nan_count"].any() and (r1["argmin"] >= 0).all() and len(set(r1["hash"][:, 0].tolist())) == 13
    # the last record against the reference on the downloaded fields
    ny, nx = ctx.shape[0] - 2 * STEP_H, ctx.shape[1] - 2 * STEP_H
    down = lambda t: interior(t.cpu().numpy(), nx, ny, STEP_H, STEP_H)  # noqa: E731
    wet = down(states[0]["mask"])
    last = [(down(rnet["T"]), "value"), (down(rnet["S"]), "value"), (down(rnet["u"]), "abs"), (down(rnet["v"]), "abs"),
            (down(rfl["latent_heat"]), "value"), (down(states[0]["T"]), "value")]
    assert mr.same(r1[-1], reference(last, wet)) and 0 < wet.mean() < 1
    if pipeline == "merged":
        ctx.set_option(abi.OPT_MERGED_PREFETCH, 1)
    plain_fl, plain_net, _, _, _ = _stepped(ctx, states, src, w, [(0, n)], bool(pipeline))
    for stride, (want, times) in ((1, (r1, t1)), (3, (r3, t3))):
        fl, net, (got, got_t), _, _ = _stepped(ctx, states, src, w, [(0, 5), (5, n - 5)], bool(pipeline), stride=stride)
        assert mr.same(got, want) and np.array_equal(got_t, times), stride
        for k in FLUX_NAMES:
            assert torch.equal(fl[k], plain_fl[k]) and torch.equal(fl[k], rfl[k]), k
        for k in NET_NAMES:
            assert torch.equal(net[k], plain_net[k]) and torch.equal(net[k], rnet[k]), k
    # beside an averager and an integrator: the monitor's records and the others' own results keep their bits
    _, _, _, q_alone, means_alone = _stepped(ctx, states, src, w, [(0, n)], bool(pipeline), others=True)
    _, net, (got, _), q_with, means_with = _stepped(ctx, states, src, w, [(0, n)], bool(pipeline), stride=1, others=True)
    assert mr.same(got, r1), "with an averager and an integrator attached next to it"
    assert q_alone.shape == (4, 3) and np.array_equal(q_with.view(np.int64), q_alone.view(np.int64))
    for a, b in zip(means_with, means_alone):
        assert torch.equal(a.view(torch.int64), b.view(torch.int64)) and a.abs().sum() > 0
    ctx.close()


def test_continuing_calls_yield_the_records_of_one_call():
    ctx, states, src, w, _ = _setup()
    ctx.set_option(abi.OPT_MERGED_PREFETCH, 2)
    one = _stepped(ctx, states, src, w, [(0, 12)], abi.PIPELINE_CONTINUING, stride=2)
    ctx.discard_prefetched_atmosphere_state()
    three = _stepped(ctx, states, src, w, [(0, 4), (4, 3), (7, 5)], abi.PIPELINE_CONTINUING, stride=2)
    assert one[2][0].shape == (6, 6)
    assert mr.same(one[2][0], three[2][0]) and np.array_equal(one[2][1], three[2][1])
    for k in NET_NAMES:
        assert torch.equal(one[1][k], three[1][k]), k
    ctx.close()


def test_a_call_that_would_overflow_the_series_fails_before_any_launch():
    ctx, states, src, w, _ = _setup()
    fl, net = ctx.field_set(FLUX_NAMES), ctx.field_set(NET_NAMES)
    sched = ctx.make_schedule(states, [ctx.field_set(EXCHANGE_NAMES)], time_fraction_increment=INC)
    ctx.time_steps(0, 2, sched, src, w, fl, net)
    launches = ctx.debug_land_zero_launches()
    assert launches >= 1
    m = _step_monitor(ctx, fl, net, states, capacity=3)
    m.collect(9.0)
    ctx.attach_monitor(m, 2, 0.0, 1.0)
    ctx.sync()
    marks = {k: v.clone() for k, v in list(fl.items()) + [("net." + k, v) for k, v in net.items()]}
    with pytest.raises(CofluxError, match="monitor's series"):
        ctx.time_steps(3, 6, sched, src, w, fl, net)        # steps 3 … 8 collect after steps 3, 5, 7: three records, two fit
    ctx.sync()
    assert ctx.debug_land_zero_launches() == launches, "the step loop was never opened"
    for k, v in list(fl.items()) + [("net." + k, v) for k, v in net.items()]:
        assert torch.equal(v.view(torch.int64), marks[k].view(torch.int64)), k
    assert m.count() == 1
    ctx.time_steps(3, 4, sched, src, w, fl, net)            # steps 3 … 6: two records
    assert m.count() == 3 and list(m.read()[1]) == [9.0, 4.0, 6.0] and m.status() == (-1, 0)
    ctx.attach_monitor(None)
    ctx.time_steps(0, 3, sched, src, w, fl, net)            # detached: no record
    assert m.count() == 3
    m.close()
    ctx.close()


# ---- run!(simulation) with the callbacks -------------------------------------------------------------------------------------
def _surface_fields(model):
    st, si = model.ocean.surface_state(), model.sea_ice
    return {"h": si.thickness, "ℵ": si.concentration, "T": st["T"], "S": st["S"], "u": st["u"], "v": st["v"]}


def test_progress_and_omip_progress_through_run_equal_the_reference_on_the_downloaded_fields(caplog):
    model = _model(True)
    inner = lambda t: interior(t.cpu().numpy(), NX, NY, H, H).copy()  # noqa: E731
    wet = inner(model.ocean.model.wet_mask)
    downloads = {}
    sim = cm.Simulation(model, dt=DT, stop_iteration=5)
    progress, omip = cm.Progress(), cm.omip_progress_callback()
    extrema = cm.SurfaceExtrema(model, dict(T=model.ocean.surface_state()["T"], speed=(model.ocean.surface_state()["u"], "abs")), capacity=2)
    sim.output_writers["extrema"] = extrema
    cm.add_callback(sim, lambda s: downloads.__setitem__(s.model.clock.iteration, {k: inner(t) for k, t in _surface_fields(s.model).items()}))
    messages = {}
    cm.add_callback(sim, lambda s: messages.__setitem__(s.model.clock.iteration, (progress(s), omip(s))))
    with caplog.at_level("INFO", logger="coflux"):
        cm.run(sim)
    assert sorted(downloads) == sorted(messages) == [1, 2, 3, 4, 5] and 0 < wet.mean() < 1
    j = cm._julia
    for it in range(1, 6):
        v = {k: mr.monitor_value(x, wet) for k, x in downloads[it].items()}
        assert all(x["nan_count"] == 0 for x in v.values())
        head = "time: %s, iteration: %d, Δt: 20 minutes, " % (cm.prettytime(it * DT), it)
        ice = "max(h): %s m, max(ℵ): %s " % (j("%.2e", v["h"]["maximum"]), j("%.2e", v["ℵ"]["maximum"]))
        want = head + ice + "extrema(T, S): (%.2f, %.2f) ᵒC, (%.2f, %.2f) psu, " % (v["T"]["maximum"], v["T"]["minimum"], v["S"]["maximum"], v["S"]["minimum"])
        want += "maximum(u): (%.2e, %.2e) m/s, wall time: " % (v["u"]["maximum"], v["v"]["maximum"])
        assert messages[it][0].startswith(want), (messages[it][0], want)
        want = head + ice + "extrema(T, S): (%.2f, %.2f) ᵒC, (%.2f, %.2f) psu " % (v["T"]["minimum"], v["T"]["maximum"], v["S"]["minimum"], v["S"]["maximum"])
        want += "maximum(u): (%.2e, %.2e) m/s, wall time: " % (v["u"]["maximum"], v["v"]["maximum"])
        assert messages[it][1].startswith(want), (messages[it][1], want)
        for k in v:
            assert mr.same(progress.record[k], v[k]) if it == 5 else True
    assert sorted(omip.hashes) == [1, 5]
    for it in (1, 5):
        d = downloads[it]
        want = "STATE_HASH iter=%d  T=%016x  S=%016x  u=%016x  h=%016x" % (it, mr.state_hash(d["T"]), mr.state_hash(d["S"]), mr.state_hash(d["u"]), mr.state_hash(d["h"]))
        assert omip.hashes[it] == want and want in caplog.text
    assert re.findall(r"STATE_HASH iter=(\d+)", caplog.text) == ["1", "5"]
    # the writer beside them: five records through a series of two
    s = extrema.series()
    assert list(extrema.times) == [DT * k for k in range(1, 6)]
    for it in range(1, 6):
        T, speed = mr.monitor_value(downloads[it]["T"], wet), mr.monitor_value(downloads[it]["u"], wet, "abs")
        assert s["T"]["min"][it - 1] == T["minimum"] and tuple(s["T"]["argmax"][it - 1]) == divmod(int(T["argmax"]), NX)
        assert s["speed"]["max"][it - 1] == speed["maximum"] and int(s["speed"]["hash"][it - 1]) == mr.state_hash(downloads[it]["u"])
    for c in (progress, omip, extrema):
        c.close()
    model.interfaces.context.close()


def test_nan_checker_stops_run_on_the_device():
    model = _model(False)
    wet = interior(model.ocean.model.wet_mask.cpu().numpy(), NX, NY, H, H)
    jw, iw = [int(v) for v in np.argwhere(wet != 0)[len(np.argwhere(wet != 0)) // 2]]
    jl, il = [int(v) for v in np.argwhere(wet == 0)[0]]
    net = model.interfaces.net_fluxes._ocean_fields

    def plant(sim):
        if sim.model.clock.iteration == 2:
            net["u"][H + jl, H + il] = float("nan")      # land: no trace
        if sim.model.clock.iteration == 4:
            net["S"][H + jw, H + iw] = float("nan")

    sim = cm.Simulation(model, dt=DT, stop_iteration=9)
    chk = cm.NaNChecker(schedule=cm.IterationInterval(2))
    cm.add_callback(sim, plant)
    cm.add_callback(sim, chk, chk.schedule)
    cm.run(sim)
    assert model.clock.iteration == 4 and sim.running is False and chk.first == (4, "net_S", (jw, iw)), chk.first
    chk.close()
    model.interfaces.context.close()
