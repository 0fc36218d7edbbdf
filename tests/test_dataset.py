"""GPU tests of the staged dataset (include/coflux.h: cf_dataset_*, cf_materialize_dataset_restoring) on the designed planes
of tests/dataset_case.py against the definition in tests/dataset_reference.py: the inpainted source plane bit for bit under
every kernel form and grid size, the host's counts, the regridded levels within the rounding of four products and three
additions and bit for bit across halo widths, weight forms and alignments, S★ and the restoring buffer formed from it."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import dataset_case as case
import dataset_reference as ref
import util
from coflux import abi
from coflux import interface_computations as ic
from coflux.runtime import CofluxError, FluxContext

pytestmark = pytest.mark.gpu

GUARD = 96
EPS = 2.0 ** -53
TIMES, PERIOD = (0.0, 1000.0, 2500.0), 4000.0
SENTINEL = int(np.array([util.SENTINEL64], dtype=np.uint64).view(np.int64)[0])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@functools.lru_cache(maxsize=None)
def staged_reference(name):
    """(plane f64, sweeps, filled, defaulted) of a staging case by the NumPy definition, computed once and never written to."""
    plane, periodic, max_sweeps = case.staging_cases()[name]
    out = ref.inpaint(plane, periodic, max_sweeps, case.FILL_VALUE)
    out[0].setflags(write=False)
    return out


def context(nx, ny, hx, hy, mask_kind=abi.MASK_NONE):
    return FluxContext(nx, ny, hx, hy, ic.flux_params(mask_kind=mask_kind), ring=1)


def device_weights(ctx, fi, fj, separable, offset=0):
    """The weight map on the device; offset 1: in guarded views 8 but not 16 bytes off the allocation's alignment."""
    if not separable:
        fi, fj = case.weights_2d(fi, fj)

    def put(a):
        if not offset:
            return ctx.to_device(a)
        t = util.guarded(a.shape, torch.float64, offset=offset, guard=GUARD, fill=util.SENTINEL64)
        t.copy_(ctx.to_device(a))
        return t
    return dict(separable=separable, fi=put(fi), fj=put(fj))


def make_dataset(ctx, plane_shape, periodic, max_sweeps, *, times=(0.0,), period=0.0, separable=True, offset=0, **kw):
    ns_y, ns_x = plane_shape
    g = ctx.grid
    fi, fj = case.fractional_indices(g.nx, g.ny, g.hx, g.hy, ns_x, ns_y)
    w = device_weights(ctx, fi, fj, separable, offset)
    return ctx.dataset(ns_x, ns_y, times, w, period=period, periodic_x=periodic, max_sweeps=max_sweeps, fill_value=case.FILL_VALUE, **kw)


# ---------------------------------------------------------------------------------------------
# 1. staging: the inpainted plane and the host's counts
# ---------------------------------------------------------------------------------------------
FORMS = [dict(), dict(sweeps_per_launch=1), dict(sweeps_per_launch=3), dict(sweeps_per_launch=8), dict(max_workgroups=1),
         dict(sweeps_per_launch=1, max_workgroups=1), dict(sweeps_per_launch=3, max_workgroups=1), dict(sweeps_per_launch=8, max_workgroups=1)]


@pytest.mark.parametrize("name", list(case.staging_cases()))
def test_the_staged_plane_is_the_numpy_inpainting_bit_for_bit(name):
    """cf_dataset_read_source after cf_dataset_stage holds the reference's bits with the library's choice of form, with one
    sweep per launch, with three and eight sweeps per launch on LDS tiles, each on one workgroup and on all; stage_info holds
    the reference's counts."""
    plane, periodic, max_sweeps = case.staging_cases()[name]
    want, sweeps, filled, defaulted = staged_reference(name)
    ctx = context(17, 9, 2, 3)
    try:
        for form in FORMS:
            d = make_dataset(ctx, plane.shape, periodic, max_sweeps, **form)
            d.stage(0, plane)
            got = d.read_source()
            wrong = int((bits(got) != bits(want)).sum())
            assert wrong == 0, f"{name} {form}: {wrong} of {want.size} cells differ"
            assert d.stage_info(0) == (sweeps, filled, defaulted), (name, form)
            d.close()
    finally:
        ctx.close()


def test_a_level_restaged_holds_the_new_plane():
    """Staging is repeatable: level 0 staged with the large plane, then level 1 and level 0 again with others — the planes'
    ping-pong and the upload slots carry nothing over."""
    ctx = context(17, 9, 2, 3)
    try:
        large = case.staging_cases()["large_periodic"][0]
        other = np.roll(large, 17, axis=1)
        d = make_dataset(ctx, large.shape, True, -1, times=(0.0, 1.0))
        for level, plane in ((0, large), (1, other), (0, other), (1, large), (0, large)):
            d.stage(level, plane)
        assert np.array_equal(bits(d.read_source()), bits(staged_reference("large_periodic")[0]))
        first = d.level(0)
        d.stage(1, large)
        assert torch.equal(d.level(1).view(torch.int64), first.view(torch.int64))
        d.close()
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------
# 2. regridding
# ---------------------------------------------------------------------------------------------
def window(a, g):
    return a[g.hy - g.ring:g.hy + g.ny + g.ring, g.hx - g.ring:g.hx + g.nx + g.ring]


@pytest.mark.parametrize("name", ["small_periodic", "large_periodic", "large_nine_sweeps"])
@pytest.mark.parametrize("nx, ny", sorted(case.OCEAN_GRIDS))
def test_levels_are_the_bilinear_reference_and_the_same_bits_on_every_layout(nx, ny, name):
    """Against the reference the tolerance per cell is 8 · 2⁻⁵³ · max |corner| — four products and three additions of weights in
    [0, 1], contracted or not.  Across halo widths, between separable and 2-D weights holding the same numbers, and with the
    weights in odd-offset guarded views, the window W is bit for bit the same; outside W the level keeps its zeros."""
    plane, periodic, max_sweeps = case.staging_cases()[name]
    staged = staged_reference(name)[0]
    windows = []
    for hx, hy in case.OCEAN_GRIDS[(nx, ny)]:
        ctx = context(nx, ny, hx, hy)
        try:
            g = ctx.grid
            fi, fj = case.fractional_indices(nx, ny, hx, hy, plane.shape[1], plane.shape[0])
            fi2, fj2 = case.weights_2d(fi, fj)
            want, bound = ref.regrid(staged, fi2, fj2, nx, ny, hx, hy, g.ring)
            for separable, offset in ((True, 0), (False, 0), (True, 1), (False, 1)):
                d = make_dataset(ctx, plane.shape, periodic, max_sweeps, separable=separable, offset=offset)
                d.stage(0, plane)
                got = d.level(0).cpu().numpy()
                finite = np.isfinite(want)
                err = np.abs(got[finite] - want[finite])
                assert np.all(err <= 8.0 * EPS * bound[finite]), (name, separable, offset, float(err.max()))
                assert np.array_equal(np.isposinf(got), np.isposinf(want)) and not np.isnan(got[finite]).any()
                outside = np.ones(got.shape, dtype=bool)
                window(outside, g)[...] = False
                assert np.all(bits(got)[outside] == 0), "a cell outside W was written"
                windows.append(bits(window(got, g)).copy())
                d.close()
        finally:
            ctx.close()
    for w in windows[1:]:
        assert np.array_equal(w, windows[0])


def test_an_ocean_cell_over_land_alone_gets_a_finite_target():
    plane, periodic, _ = case.staging_cases()["large_periodic"]
    nx, ny, hx, hy = 77, 23, 7, 2
    ctx = context(nx, ny, hx, hy)
    try:
        fi, fj = case.fractional_indices(nx, ny, hx, hy, plane.shape[1], plane.shape[0])
        over_land = np.zeros((ny + 2 * hy, nx + 2 * hx), dtype=bool)
        for j in range(ny):
            for i in range(nx):
                nodes, _w = ref.stencil(float(fi[i + hx]), float(fj[j + hy]), plane.shape[1], plane.shape[0])
                over_land[j + hy, i + hx] = all(np.isnan(plane[n]) for n in nodes)
        assert int(over_land.sum()) >= 100
        d = make_dataset(ctx, plane.shape, periodic, -1)
        d.stage(0, plane)
        got = d.level(0).cpu().numpy()
        assert np.isfinite(got[over_land]).all() and np.all(got[over_land] > 30.0)   # the plane's own values, not the fill
        d.close()
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------
# 3. evaluation and the restoring buffer
# ---------------------------------------------------------------------------------------------
def three_levels(ctx, **kw):
    small = case.small_plane()
    planes = [small, np.roll(small, 5, axis=1) * np.float32(1.03125), np.flipud(small) + np.float32(0.75)]
    d = make_dataset(ctx, small.shape, True, -1, times=TIMES, period=PERIOD, **kw)
    return d, planes


def sentinel_field(shape):
    return util.guarded(tuple(shape), torch.float64, offset=1, guard=GUARD, fill=util.SENTINEL64)


def whole(view):
    return util.buffer_of(view)[0].view(torch.int64).clone()


def test_evaluate_writes_the_window_and_nothing_else():
    """At fraction 0.0 — a level time, one period on, one level — the window is the level bit for bit; between levels it is
    b·f + a·(1 − f) within 4 · 2⁻⁵³ · max(|a|, |b|) (a product, a difference, a product and a sum, contracted or not).  The
    output starts sentinel-filled in an odd-offset guarded buffer whose every other word is still the sentinel afterwards."""
    ctx = context(17, 9, 2, 3)
    try:
        g = ctx.grid
        d, planes = three_levels(ctx)
        for level, plane in enumerate(planes):
            d.stage(level, plane)
        levels = [d.level(k) for k in range(3)]
        inside = torch.zeros(ctx.shape, dtype=torch.bool, device="cuda")
        window(inside, g)[...] = True
        for time in (0.0, 1000.0, 2500.0, 4000.0, -3000.0, 700.0, 1400.0, 2800.0, 3999.0, -1.0):
            l1, l2, f = ref.time_index(list(TIMES), PERIOD, time)
            assert d.time_index(time) == (l1, l2, f)
            out = sentinel_field(ctx.shape)
            want = whole(out)
            d.evaluate(time, out)
            ctx.sync()
            got = whole(out)
            first = util.buffer_of(out)[1]
            view = got[first:first + out.numel()].view(ctx.shape)
            assert bool((view[~inside] == SENTINEL).all()) and torch.equal(got[:first], want[:first])
            assert torch.equal(got[first + out.numel():], want[first + out.numel():])
            a, b = levels[l1][inside].cpu().numpy(), levels[l2][inside].cpu().numpy()
            o = out[inside].cpu().numpy()
            if f == 0.0:
                assert np.array_equal(bits(o), bits(a)), time
            else:
                finite = np.isfinite(a) & np.isfinite(b)
                err = np.abs(o[finite] - ref.blend(a[finite], b[finite], f))
                assert np.all(err <= 4.0 * EPS * np.maximum(np.abs(a[finite]), np.abs(b[finite]))), (time, float(err.max()))
        one = make_dataset(ctx, planes[0].shape, True, -1, times=(5.0,), period=0.0)
        one.stage(0, planes[0])
        out = ctx.zeros()
        one.evaluate(1e9, out)
        assert torch.equal(out[inside].view(torch.int64), one.level(0)[inside].view(torch.int64))
        d.close()
        one.close()
    finally:
        ctx.close()


@pytest.mark.parametrize("nx, ny, hx, hy", [(17, 9, 2, 3), (77, 23, 7, 2)])
def test_the_dataset_restoring_is_evaluate_then_the_static_restoring_bit_for_bit(nx, ny, hx, hy):
    ctx = context(nx, ny, hx, hy, mask_kind=abi.MASK_U8)
    try:
        rng = np.random.default_rng(11)
        d, planes = three_levels(ctx)
        for level, plane in enumerate(planes):
            d.stage(level, plane)
        mask = (rng.random(ctx.shape) > 0.3).astype(np.uint8)
        ocean = dict(T=ctx.zeros(), S=ctx.to_device(34.0 + rng.standard_normal(ctx.shape)), u=ctx.zeros(), v=ctx.zeros(), mask=ctx.to_device(mask))
        vp = 1.0 / 6.0 / 86400.0
        for time in (0.0, 700.0, 1400.0, 2500.0, 2800.0, 3999.0, 4700.0):
            target = ctx.zeros()
            d.evaluate(time, target)
            want, got = sentinel_field(ctx.shape), sentinel_field(ctx.shape)
            ctx.materialize_salinity_restoring(vp, target, ocean, want)
            ctx.materialize_dataset_restoring(vp, d, time, ocean, got)
            ctx.sync()
            assert torch.equal(whole(got), whole(want)), time
        d.close()
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------
# 4. refusals
# ---------------------------------------------------------------------------------------------
def test_refusals():
    ctx, other = context(17, 9, 2, 3), context(17, 9, 2, 3)
    lib = ctx.lib
    try:
        fi, fj = case.fractional_indices(17, 9, 2, 3, 24, 12)
        w = device_weights(ctx, fi, fj, True)
        good = dict(ns_x=24, ns_y=12, times=(0.0, 1.0), weights=w, period=0.0)
        for change, word in ((dict(ns_x=1), "shape"), (dict(ns_y=0), "shape"), (dict(times=()), "levels"), (dict(times=tuple(range(33))), "levels"),
                             (dict(times=(1.0, 1.0)), "times"), (dict(times=(0.0, float("nan"))), "times"), (dict(period=1.0), "period"),
                             (dict(period=-2.0), "period"), (dict(sweeps_per_launch=9), "sweeps_per_launch"), (dict(max_workgroups=-1), "max_workgroups"),
                             (dict(fill_value=float("nan")), "fill_value"), (dict(weights=dict(separable=True, fi=w["fi"])), "weights")):
            with pytest.raises(CofluxError, match=word):
                ctx.dataset(**dict(good, **change))
        desc = abi.DatasetDesc()
        out = C.c_void_p()
        assert lib.cf_dataset_create(ctx._h, C.byref(desc), C.byref(out)) == -1 and b"struct_size" in lib.cf_last_error(None)
        d = ctx.dataset(**good)
        plane = case.small_plane()
        for level in (-1, 2):
            with pytest.raises(CofluxError, match="level"):
                d.stage(level, plane)
        assert lib.cf_dataset_stage(d._h, 0, None) == -1 and b"plane" in lib.cf_last_error(None)
        with pytest.raises(CofluxError, match="staged"):
            d.read_source()
        d.stage(0, plane)
        target = sentinel_field(ctx.shape)
        untouched = whole(target)
        ocean = dict(T=ctx.zeros(), S=ctx.zeros(), u=ctx.zeros(), v=ctx.zeros())
        with pytest.raises(CofluxError, match="level 1"):      # not every level is staged
            d.evaluate(0.5, target)
        with pytest.raises(CofluxError, match="level 1"):
            ctx.materialize_dataset_restoring(1e-6, d, 0.5, ocean, target)
        with pytest.raises(CofluxError, match="level 1"):
            ctx.attach_restoring_dataset(d)
        with pytest.raises(CofluxError, match="staged"):
            d.stage_info(1)
        d.stage(1, plane)
        for bad in (float("nan"), float("inf")):
            with pytest.raises(CofluxError, match="finite"):
                d.evaluate(bad, target)
            with pytest.raises(CofluxError, match="finite"):
                ctx.attach_restoring_dataset(d, time_origin=bad)
        with pytest.raises(CofluxError, match="another context"):
            other.attach_restoring_dataset(d)
        with pytest.raises(CofluxError, match="another context"):
            other.materialize_dataset_restoring(1e-6, d, 0.5, ocean, target)
        ctx.sync()
        assert torch.equal(whole(target), untouched)
        ctx.attach_restoring_dataset(d, time_origin=0.0, step_seconds=0.25)
        d.close()                                  # destroying detaches
        ctx.attach_restoring_dataset(None)
    finally:
        ctx.close()
        other.close()
