"""GPU tests of the exact NormalizeSalinity (include/coflux.h: cf_normalize_salinity_flux_exact, cf_debug_salinity_sums_exact;
csrc/coflux_exact_sum.hip) against fractions.Fraction summed and rounded once (tests/exact_sum_reference.py), bit for bit:
on synthetic fields of four shapes under three halos, every mask kind, `area` and `additional` each absent and given, with NaN
in every land and halo cell of flux, additional and area; and on the designed lists of tests/test_exact_sum_cpu.py laid into wet
cells, inside one workgroup and across several.  cf_normalize_salinity_flux on the same inputs keeps the bits of its documented
order (a NumPy replay of salinity_partial_sums_kernel / salinity_final_sums_kernel)."""
import numpy as np
import pytest
import torch

import exact_sum_reference as xs
import util
from coflux import abi
from coflux import interface_computations as ic
from coflux.runtime import FluxContext

pytestmark = pytest.mark.gpu

GUARD = 64
SHAPES = [(1, 1), (64, 1), (77, 23), (131, 37)]
HALOS = [(1, 1), (2, 7), (4, 4)]
MASK_KINDS = {"none": abi.MASK_NONE, "u8": abi.MASK_U8, "bottom_height": abi.MASK_BOTTOM_HEIGHT}
BLOCK, MAX_BLOCKS = 256, 512     # both sum kernels: min(512, ⌈nx·ny / 256⌉) workgroups of 256
SENTINEL = int(np.array([util.SENTINEL64], dtype=np.uint64).view(np.int64)[0])


def make_case(nx, ny, hx, hy, mask_name, *, area, additional, wet_fraction=0.7, seed=0):
    """Host arrays of one normalisation: NaN in every land and halo cell of flux, additional and area."""
    rng = np.random.default_rng(1000 * nx + 10 * ny + hx + seed)
    shape = (ny + 2 * hy, nx + 2 * hx)
    inner = (slice(hy, hy + ny), slice(hx, hx + nx))
    params = ic.flux_params(mask_kind=MASK_KINDS[mask_name])
    wet_inner = np.ones((ny, nx), bool) if mask_name == "none" else rng.random((ny, nx)) < wet_fraction
    if nx * ny == 1 and wet_fraction > 0:
        wet_inner[:] = True
    z = params.ocean_surface_z
    if mask_name == "none":
        mask = None
    elif mask_name == "u8":
        mask = np.zeros(shape, np.uint8)
        mask[inner] = wet_inner
    else:   # land: z_surface ≤ z_b — exactly at the surface and above it
        mask = np.full(shape, z + 10.0)
        mask[inner] = np.where(wet_inner, z - 4000.0, np.where(rng.random((ny, nx)) < 0.5, z, z + 10.0))
    case = dict(nx=nx, ny=ny, hx=hx, hy=hy, shape=shape, inner=inner, mask=mask, z_surface=z, params=params, mask_name=mask_name)
    wet = xs.wet_interior(case)
    assert np.array_equal(wet[inner], wet_inner)

    def field(values):
        out = np.full(shape, np.nan)
        out[wet] = values[wet]
        return out

    # salt fluxes of ±1e-6 over six decades, a restoring flux an order below, cell areas of a one-degree grid
    case["flux"] = field(1e-6 * rng.standard_normal(shape) * 10.0 ** rng.uniform(-3.0, 3.0, shape))
    case["additional"] = field(1e-7 * rng.standard_normal(shape)) if additional else None
    case["area"] = field(1.2e10 * (0.05 + rng.random(shape))) if area else None
    case["wet"] = wet
    return case


def context(case):
    return FluxContext(case["nx"], case["ny"], case["hx"], case["hy"], case["params"], ring=0)


def on_device(ctx, case):
    return {k: (None if case[k] is None else ctx.to_device(case[k])) for k in ("mask", "additional", "area")}


def guarded_flux(ctx, case):
    t = util.guarded(case["shape"], torch.float64, offset=1, guard=GUARD, fill=util.SENTINEL64)
    t.copy_(ctx.to_device(case["flux"]))
    return t


def reference(case):
    """bits of (fl(Σ t), fl(Σ a), mean) and the non-finite counts of the t"""
    t, a = xs.salinity_terms(case)
    sj, sa = xs.sum_bits(t), xs.sum_bits(a)
    return sj, sa, xs.mean_bits(sj, sa), xs.nonfinite_counts(t)


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.int64)


def assert_flux_minus_mean(buffer_after, case, mean_bits_, what):
    """the whole guarded buffer: NumPy's flux − mean on every cell of the parent array (NaN where the input is NaN), the guard
    space untouched"""
    n = int(np.prod(case["shape"]))
    assert np.all(buffer_after[:GUARD + 1].view(np.int64) == SENTINEL) and np.all(buffer_after[GUARD + 1 + n:].view(np.int64) == SENTINEL), what
    got = buffer_after[GUARD + 1:GUARD + 1 + n].reshape(case["shape"])
    with np.errstate(invalid="ignore"):
        want = case["flux"] - xs.from_bits(mean_bits_)
    finite = ~np.isnan(want)
    assert np.array_equal(np.isnan(got), ~finite), what
    assert np.array_equal(bits(got[finite]), bits(want[finite])), (what, int((bits(got[finite]) != bits(want[finite])).sum()))


def butterfly(x):
    """lane 0 of `for m in 32 … 1: x += shfl_xor(x, m)` along the last axis (64 lanes)"""
    lanes = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        x = x + x[..., lanes ^ m]
    return x[..., 0]


def replay_documented_order(case):
    """cf_normalize_salinity_flux's mean by its documented order, for surfaces of at most 512 · 256 cells (one trip of the
    grid-stride loop, so a thread's fma(v, a, 0) is fl(v · a)): per wave a butterfly, per workgroup its four waves in order, then one
    wave that adds the workgroups' partials lane by lane in index order and a butterfly."""
    nx, ny = case["nx"], case["ny"]
    n = nx * ny
    assert n <= BLOCK * MAX_BLOCKS
    nblocks = max(1, -(-n // BLOCK))
    wet = case["wet"][case["inner"]].ravel()
    with np.errstate(invalid="ignore"):
        v = case["flux"][case["inner"]].ravel() + (case["additional"][case["inner"]].ravel() if case["additional"] is not None else 0.0)
        a = case["area"][case["inner"]].ravel() if case["area"] is not None else np.ones(n)
        tj, ta = np.zeros(nblocks * BLOCK), np.zeros(nblocks * BLOCK)
        tj[:n], ta[:n] = np.where(wet, v * a, 0.0), np.where(wet, a, 0.0)
    sums = []
    for t in (tj, ta):
        waves = butterfly(t.reshape(nblocks, BLOCK // 64, 64))
        partial = waves[:, 0]
        for w in range(1, BLOCK // 64):
            partial = partial + waves[:, w]
        lanes = np.zeros(64)
        for k in range(nblocks):
            lanes[k % 64] += partial[k]
        sums.append(float(butterfly(lanes)))
    return sums[0] / sums[1] if sums[1] > 0.0 else 0.0


@pytest.mark.parametrize("hx, hy", HALOS)
@pytest.mark.parametrize("nx, ny", SHAPES)
def test_sums_and_mean_are_the_references_bits_on_synthetic_fields(nx, ny, hx, hy):
    """Every mask kind × area × additional: the debug sums, the mean, every cell of the guarded parent buffer; a repeat call gives
    the same bits; cf_normalize_salinity_flux on the same input gives the bits of its documented order."""
    for mask_name in MASK_KINDS:
        ctx = None
        for area in (False, True):
            for additional in (False, True):
                case = make_case(nx, ny, hx, hy, mask_name, area=area, additional=additional)
                what = f"{nx}x{ny} halo ({hx},{hy}) {mask_name} area={area} additional={additional}"
                ctx = ctx or context(case)
                dev = on_device(ctx, case)
                want_sj, want_sa, want_mean, want_counts = reference(case)
                flux = guarded_flux(ctx, case)
                before = util.buffer_of(flux)[0].clone()
                (sj, sa), counts = ctx.debug_salinity_sums_exact(flux, dev["mask"], additional=dev["additional"], area=dev["area"])
                assert (xs.bits(sj), xs.bits(sa)) == (want_sj, want_sa), (what, sj, sa, xs.from_bits(want_sj), xs.from_bits(want_sa))
                assert list(counts) == want_counts == [0, 0, 0], what
                assert torch.equal(util.buffer_of(flux)[0].view(torch.int64), before.view(torch.int64)), what + ": the debug call wrote"
                runs = []
                for _ in range(2):
                    flux = guarded_flux(ctx, case)
                    mean = util.guarded((1,), torch.float64, offset=1, guard=GUARD, fill=util.SENTINEL64)
                    ctx.normalize_salinity_flux_exact(flux, dev["mask"], additional=dev["additional"], area=dev["area"], mean_out=mean)
                    ctx.sync()
                    runs.append((util.buffer_of(flux)[0].cpu().numpy(), util.buffer_of(mean)[0].cpu().numpy()))
                after, mean_buffer = runs[0]
                assert int(mean_buffer.view(np.uint64)[GUARD + 1]) == want_mean, (what, mean_buffer[GUARD + 1], xs.from_bits(want_mean))
                assert int((bits(mean_buffer) == SENTINEL).sum()) == mean_buffer.size - 1, what
                assert_flux_minus_mean(after, case, want_mean, what)
                assert np.array_equal(bits(runs[1][0]), bits(after)) and np.array_equal(bits(runs[1][1]), bits(mean_buffer)), what + ": repeat"
                # the old entry point keeps its order and its bits
                flux = guarded_flux(ctx, case)
                mean = torch.zeros(1, dtype=torch.float64, device=ctx.device)
                ctx.normalize_salinity_flux(flux, dev["mask"], additional=dev["additional"], area=dev["area"], mean_out=mean)
                ctx.sync()
                old = float(mean.cpu()[0])
                assert xs.bits(old) == xs.bits(replay_documented_order(case)), (what, old, replay_documented_order(case))
                assert_flux_minus_mean(util.buffer_of(flux)[0].cpu().numpy(), case, xs.bits(old), what + ": cf_normalize_salinity_flux")
        ctx.close()


LISTS = {**xs.designed_lists(), **xs.nonfinite_lists()}
LAYOUTS = {"one_workgroup": (77, 3, 2, 7), "several_workgroups": (131, 37, 4, 4)}


@pytest.mark.parametrize("mask_name", ["none", "u8"])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_designed_lists_laid_into_wet_cells(layout, mask_name):
    """The CPU test's lists — cancellation around a residue, subnormals, ties, sums that pass through huge partials, overflow by
    rounding, NaN and ±Inf in every combination — as the terms of wet cells spread over the surface: once as the flux (area
    NULL: t = flux), once as the areas under a flux of 1.0 (t = a: both sums are the list's)."""
    nx, ny, hx, hy = LAYOUTS[layout]
    assert (nx * ny <= BLOCK) == (layout == "one_workgroup") and (layout == "one_workgroup" or nx * ny > 4 * BLOCK)
    base = make_case(nx, ny, hx, hy, mask_name, area=False, additional=False, wet_fraction=0.8, seed=7)
    ctx = context(base)
    mask = None if base["mask"] is None else ctx.to_device(base["mask"])
    wet_cells = np.flatnonzero(base["wet"].ravel())
    ran = 0
    for name, values in LISTS.items():
        if len(values) > len(wet_cells):
            assert layout == "one_workgroup", name
            continue
        ran += 1
        at = wet_cells[np.linspace(0, len(wet_cells) - 1, len(values)).round().astype(int)]   # spread: the first and the last wet cell included
        assert len(set(at.tolist())) == len(values), name
        laid = np.where(base["wet"], 0.0, np.nan).ravel()
        laid[at] = values
        laid = laid.reshape(base["shape"])
        want, want_counts = xs.sum_bits(values), xs.nonfinite_counts(values)
        # as the flux
        (sj, sa), counts = ctx.debug_salinity_sums_exact(ctx.to_device(laid), mask)
        assert xs.bits(sj) == want and list(counts) == want_counts, (layout, name, "flux", sj, xs.from_bits(want), counts)
        assert sa == float(len(wet_cells)), (layout, name)
        # as the areas (the other wet cells have area 0: their terms are zeros)
        ones = np.where(base["wet"], 1.0, np.nan)
        (sj, sa), counts = ctx.debug_salinity_sums_exact(ctx.to_device(ones), mask, area=ctx.to_device(laid))
        assert xs.bits(sj) == want and xs.bits(sa) == want and list(counts) == want_counts, (layout, name, "area", sj, sa, xs.from_bits(want))
        # … and the normalisation that follows from them
        case = dict(base, flux=laid, additional=None, area=None)
        mean_bits_ = xs.mean_bits(want, xs.bits(float(len(wet_cells))))
        flux = guarded_flux(ctx, case)
        mean = torch.zeros(1, dtype=torch.float64, device=ctx.device)
        ctx.normalize_salinity_flux_exact(flux, mask, mean_out=mean)
        ctx.sync()
        got = float(mean.cpu()[0])
        if np.isnan(xs.from_bits(mean_bits_)):
            assert np.isnan(got), (layout, name)
        else:
            assert xs.bits(got) == mean_bits_, (layout, name, got, xs.from_bits(mean_bits_))
    assert ran >= (20 if layout == "one_workgroup" else len(LISTS))
    ctx.close()


@pytest.mark.parametrize("nx, ny, hx, hy", [(1, 1, 1, 1), (131, 37, 2, 7)])
def test_an_empty_wet_set_gives_a_mean_of_positive_zero(nx, ny, hx, hy):
    for mask_name in ("u8", "bottom_height"):
        case = make_case(nx, ny, hx, hy, mask_name, area=True, additional=True, wet_fraction=0.0)
        assert not case["wet"].any() and np.isnan(case["flux"]).all()
        case["flux"] = np.where(np.isnan(case["flux"]), 1.5, 0.0) * np.arange(case["flux"].size).reshape(case["shape"])
        ctx = context(case)
        dev = on_device(ctx, case)
        flux = guarded_flux(ctx, case)
        (sj, sa), counts = ctx.debug_salinity_sums_exact(flux, dev["mask"], additional=dev["additional"], area=dev["area"])
        assert (xs.bits(sj), xs.bits(sa), list(counts)) == (0, 0, [0, 0, 0])
        mean = torch.full((1,), -1.0, dtype=torch.float64, device=ctx.device)
        ctx.normalize_salinity_flux_exact(flux, dev["mask"], additional=dev["additional"], area=dev["area"], mean_out=mean)
        ctx.sync()
        assert xs.bits(float(mean.cpu()[0])) == 0
        assert_flux_minus_mean(util.buffer_of(flux)[0].cpu().numpy(), case, 0, mask_name)
        ctx.close()
