"""GPU tests of the fixed sparse surface operator (include/coflux.h: cf_regrid_*; FluxContext.regridder, coflux.regridding).

An operator atlas on a 67 × 5 source (regrid_reference.build_atlas: every row a named case) is held to the NumPy model of the
stated summation order bit for bit and to the definition (math.fsum of exact terms) within (2n + 4) · 2⁻⁵³ · Σ|w·x| / D, n the
wet entries of the row; every halo cell and every land cell of every field holds NaN or 7.0e77.  The same bits are held across
halo widths, odd-offset views, workgroup caps, field counts and positions, both mask kinds, repeated calls and row indices.
The bound is derived (regrid_reference.py), not measured; each test prints the worst error / bound it saw."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import regrid_reference as rr
import util
from coflux import abi
from coflux import interface_computations as ic
from coflux import models as cm
from coflux import regridding as rg
from coflux import synthetic as syn
from coflux.runtime import CofluxError, FluxContext
from test_time_average import DT, H, NX, NY, _model

pytestmark = pytest.mark.gpu

SENTINEL = -1234.5
PAD = 8
ATLAS = rr.build_atlas()
NXA, NYA = rr.ATLAS_NX, rr.ATLAS_NY
Z_SURFACE = -5.0
MODES = {"mean": rr.MEAN, "sum": rr.SUM}


def padded(n):
    return torch.full((n + PAD,), SENTINEL, dtype=torch.float64, device="cuda")


def run_atlas(hx=3, hy=2, *, mode="mean", fields=range(16), views=False, max_workgroups=0, mask_kind=abi.MASK_U8, operator=None,
              coverage=True, repeats=1):
    """One context, one regridder, `repeats` applies → dict(dst [K, n_rows], coverage, everything the write-set checks need)"""
    params = ic.flux_params(mask_kind=mask_kind)
    params.ocean_surface_z = Z_SURFACE
    ctx = FluxContext(NXA, NYA, hx, hy, params, ring=0)
    all_fields, wet = rr.atlas_arrays(ATLAS, hx, hy)
    host = [all_fields[f] for f in fields]
    count = [0]

    def put(a, tdtype, fill):
        t = torch.from_numpy(np.ascontiguousarray(a))
        if not views:
            return t.cuda()
        count[0] += 1
        v = util.guarded(a.shape, tdtype, offset=(1, 3, 5)[count[0] % 3], guard=64, fill=fill)
        v.copy_(t)
        return v

    src = [put(a, torch.float64, float("nan")) for a in host]
    if mask_kind == abi.MASK_U8:
        mask_host, mask = wet, put(wet, torch.uint8, 1)
    elif mask_kind == abi.MASK_BOTTOM_HEIGHT:
        zb = ATLAS["zb"].copy()
        zb.ravel()[np.flatnonzero(ATLAS["wet"].ravel() == 0)[0]] = Z_SURFACE    # land exactly at the surface: z_surface <= zb
        mask_host = rr.embed(zb, hx, hy, -1.0e4)
        mask = put(mask_host, torch.float64, -1.0e4)
    else:
        mask_host, mask = None, None
    op = operator if operator is not None else (ATLAS["row_ptr"], ATLAS["col"], ATLAS["weight"])
    n_rows = len(op[0]) - 1
    regridder = ctx.regridder(*op, mask=mask, mode=mode, max_workgroups=max_workgroups)
    results = []
    for _ in range(repeats):
        dst, cov = [padded(n_rows) for _ in src], (padded(n_rows) if coverage else None)
        regridder.apply(src, out=dst, coverage=cov if coverage else False)
        ctx.sync()
        results.append((np.stack([d.cpu().numpy() for d in dst]), None if cov is None else cov.cpu().numpy()))
    for a, t in zip(host, src):
        assert rr.same_bits(t.cpu().numpy(), a), "a source was written"
    if mask is not None:
        assert np.array_equal(mask.cpu().numpy(), mask_host), "the mask was written"
    regridder.close()
    ctx.close()
    for dst, cov in results:
        assert (dst[:, n_rows:] == SENTINEL).all() and (cov is None or (cov[n_rows:] == SENTINEL).all()), "written past n_rows"
        assert rr.same_bits(dst, results[0][0]) and (cov is None or rr.same_bits(cov, results[0][1])), "a repeated call"
    dst, cov = results[0]
    return dict(dst=dst[:, :n_rows], coverage=None if cov is None else cov[:n_rows], fields=host, wet=wet, grid=(NXA, NYA, hx, hy))


def check_against_definition(dst, cov, definition, mode, what):
    worst = 0.0
    for r, d in enumerate(definition):
        if cov is not None:
            assert abs(cov[r] - d["D"]) <= rr.coverage_bound(d), (what, r, cov[r], d["D"])
        for f in range(dst.shape[0]):
            want, b = rr.expected(d, f, mode), rr.bound(d, f, mode)
            if math.isnan(want):
                assert math.isnan(dst[f, r]), (what, r, f, dst[f, r])
                continue
            err = abs(dst[f, r] - want)
            worst = max(worst, err / b if b > 0 else (0.0 if err == 0 else np.inf))
            assert err <= b, (what, r, f, dst[f, r], want, err, b)
    print(f"{what}: worst error / bound = {worst:.3e}")


@pytest.fixture(scope="module")
def atlas_reference():
    """the definition and the order model of the atlas on halos (3, 2), computed once: {mode: (model dst, model coverage)}"""
    fields, wet = rr.atlas_arrays(ATLAS, 3, 2)
    grid = (NXA, NYA, 3, 2)
    op = (ATLAS["row_ptr"], ATLAS["col"], ATLAS["weight"])
    return dict(definition=rr.definition(*op, fields, wet, grid),
                model={name: rr.order_model(*op, fields, wet, grid, mode=m) for name, m in MODES.items()})


@pytest.mark.parametrize("mode", ["mean", "sum"])
def test_atlas_is_the_order_model_bit_for_bit_and_within_the_bound(mode, atlas_reference):
    got = run_atlas(mode=mode, repeats=2)
    model_dst, model_cov = atlas_reference["model"][mode]
    for name, r in ATLAS["names"].items():
        assert rr.same_bits(got["dst"][:, r], model_dst[:, r]), (name, got["dst"][:, r], model_dst[:, r])
        assert rr.same_bits(got["coverage"][r:r + 1], model_cov[r:r + 1]), (name, got["coverage"][r], model_cov[r])
    check_against_definition(got["dst"], got["coverage"], atlas_reference["definition"], MODES[mode], f"atlas, {mode}")
    names = ATLAS["names"]
    for empty in ("n0", "all_land"):
        r = names[empty]
        assert got["coverage"][r] == 0.0
        if mode == "mean":
            assert np.isnan(got["dst"][:, r]).all(), empty
        else:
            assert (got["dst"][:, r].view(np.int64) == 0).all(), f"{empty}: exactly +0.0 in SUM mode"
    r = names["zero_weight"]      # wet entries, D == 0: NaN as a mean; 0 · x = ±0 summed from +0.0 as a sum
    assert got["coverage"][r] == 0.0 and (np.isnan(got["dst"][:, r]).all() if mode == "mean" else (got["dst"][:, r] == 0.0).all())
    for stem in ("same_short", "same_long"):
        a, b, c = (got["dst"][:, names[f"{stem}_{k}"]] for k in "abc")
        assert rr.same_bits(a, b) and rr.same_bits(a, c), stem
    assert np.isfinite(got["dst"][:, names["partly_land"]]).all() and np.isfinite(got["dst"][:, names["partly_land_long"]]).all()


def test_mean_is_sum_over_coverage_with_one_division():
    mean, total = run_atlas(mode="mean"), run_atlas(mode="sum")
    assert rr.same_bits(mean["coverage"], total["coverage"])
    with np.errstate(invalid="ignore", divide="ignore"):
        want = np.where(total["coverage"] == 0.0, np.nan, total["dst"] / total["coverage"])
    assert rr.same_bits(mean["dst"], want)


def test_null_coverage_is_accepted():
    base, without = run_atlas(), run_atlas(coverage=False)
    assert without["coverage"] is None and rr.same_bits(without["dst"], base["dst"])


def test_bits_do_not_depend_on_layout_workgroups_fields_or_mask_kind():
    base = run_atlas()
    for hx, hy in ((1, 1), (2, 7), (7, 2)):
        for views in (False, True):
            got = run_atlas(hx, hy, views=views)
            assert rr.same_bits(got["dst"], base["dst"]) and rr.same_bits(got["coverage"], base["coverage"]), (hx, hy, views)
    for cap in (1, 3):
        got = run_atlas(max_workgroups=cap)
        assert rr.same_bits(got["dst"], base["dst"]) and rr.same_bits(got["coverage"], base["coverage"]), cap
    # field 2 alone, fifth of six, last of sixteen (every bucket of the kernel); the others ride along or not
    for fields in ([2], [5, 7, 0, 9, 2, 11], [k for k in range(16) if k != 2] + [2], [2, 3], [1, 2, 3, 4, 5, 6, 7, 8, 9]):
        got = run_atlas(fields=fields)
        assert rr.same_bits(got["dst"][fields.index(2)], base["dst"][2]), fields
        assert rr.same_bits(got["coverage"], base["coverage"]), fields
    got = run_atlas(mask_kind=abi.MASK_BOTTOM_HEIGHT, views=True)
    assert rr.same_bits(got["dst"], base["dst"]) and rr.same_bits(got["coverage"], base["coverage"]), "bottom-height mask"


def test_no_mask_means_all_wet():
    """CF_MASK_NONE: the poisoned land cells are read — rows over wet cells only keep their bits, the all-land row is not empty"""
    base, got = run_atlas(), run_atlas(mask_kind=abi.MASK_NONE)
    names = ATLAS["names"]
    for n in rr.ATLAS_COUNTS:
        r = names[f"n{n}"]
        assert rr.same_bits(got["dst"][:, r], base["dst"][:, r]), n
    assert got["coverage"][names["all_land"]] > 0.0
    assert np.isnan(got["dst"][0, names["all_land"]]) and np.isnan(got["dst"][0, names["partly_land"]]), "a NaN in a wet cell propagates"


def test_one_row_and_a_second_grid_stride_trip():
    fields, wet = rr.atlas_arrays(ATLAS, 3, 2, 3)
    grid = (NXA, NYA, 3, 2)
    rng = np.random.default_rng(7)
    one = (np.array([0, 90], dtype=np.int64), rng.integers(0, NXA * NYA, 90).astype(np.int32), 1.0 + rng.random(90))
    got = run_atlas(operator=one, fields=range(3))
    want, cov = rr.order_model(*one, fields, wet, grid)
    assert got["dst"].shape == (3, 1) and rr.same_bits(got["dst"], want) and rr.same_bits(got["coverage"], cov)
    # 70 000 one-entry rows: 17 500 wave units against an automatic launch of at most 8 workgroups per compute unit
    n = 70000
    col = rng.integers(0, NXA * NYA, n).astype(np.int32)
    many = (np.arange(n + 1, dtype=np.int64), col, 1.0 + rng.random(n))
    for cap in (0, 5):
        got = run_atlas(operator=many, fields=range(3), mode="sum", max_workgroups=cap)
        keep = wet.ravel()[rr.offsets(col, grid)] != 0
        for f in range(3):
            with np.errstate(invalid="ignore", over="ignore"):
                want = np.where(keep, many[2] * fields[f].ravel()[rr.offsets(col, grid)], 0.0)
            assert rr.same_bits(got["dst"][f], want), (cap, f)
        assert rr.same_bits(got["coverage"], np.where(keep, many[2], 0.0)), cap


# ---- rejections ----------------------------------------------------------------------------------------------------------------
def _raw_create(ctx, row_ptr, col, weight, *, mode=abi.REGRID_MEAN, max_workgroups=0, struct_size=None, n_rows=None, nnz=None):
    row_ptr, col, weight = np.asarray(row_ptr, np.int64), np.asarray(col, np.int32), np.asarray(weight, np.float64)
    d = abi.RegridDesc()
    d.struct_size = C.sizeof(abi.RegridDesc) if struct_size is None else struct_size
    d.mode, d.max_workgroups = mode, max_workgroups
    d.n_rows = row_ptr.size - 1 if n_rows is None else n_rows
    d.nnz = col.size if nnz is None else nnz
    d.row_ptr, d.col, d.weight = row_ptr.ctypes.data, col.ctypes.data, weight.ctypes.data
    h = C.c_void_p()
    rc = ctx.lib.cf_regrid_create(ctx._h, C.byref(d), C.byref(h))
    return rc, h


def test_rejections_leave_everything_untouched():
    nx, ny = 12, 4
    ctx = FluxContext(nx, ny, 2, 2, ic.flux_params(), ring=0)
    rp, col, w = [0, 2, 2, 5], [0, 5, 47, 3, 3], [1.0, 2.0, 0.0, 4.0, 5.0]
    bad = dict(
        struct_size=dict(struct_size=C.sizeof(abi.RegridDesc) - 8),
        not_monotone=dict(row_ptr=[0, 3, 2, 5]),
        last_is_not_nnz=dict(row_ptr=[0, 2, 2, 4]),
        first_is_not_zero=dict(row_ptr=[1, 2, 2, 5]),
        column_too_large=dict(col=[0, 5, nx * ny, 3, 3]),
        column_negative=dict(col=[0, -1, 47, 3, 3]),
        weight_negative=dict(weight=[1.0, -2.0, 0.0, 4.0, 5.0]),
        weight_nan=dict(weight=[1.0, float("nan"), 0.0, 4.0, 5.0]),
        weight_inf=dict(weight=[1.0, float("inf"), 0.0, 4.0, 5.0]),
        mode=dict(mode=2),
        max_workgroups=dict(max_workgroups=-1),
        no_rows=dict(n_rows=0),
    )
    for name, change in bad.items():
        args = dict(row_ptr=rp, col=col, weight=w)
        args.update({k: v for k, v in change.items() if k in args})
        rc, h = _raw_create(ctx, args["row_ptr"], args["col"], args["weight"], **{k: v for k, v in change.items() if k not in args})
        assert rc == -1 and not h.value, (name, rc)     # CF_ERR_INVALID
        assert b"cf_regrid" in ctx.lib.cf_last_error(ctx._h), name
    rc, h = _raw_create(ctx, rp, col, w)
    assert rc == 0 and h.value
    src = [torch.ones(ctx.shape, dtype=torch.float64, device="cuda") for _ in range(17)]
    dst = [padded(3) for _ in range(17)]
    cov = padded(3)

    def apply(n, s, d):
        sp = (C.c_void_p * 17)(*[t.data_ptr() if t is not None else None for t in s])
        dp = (C.c_void_p * 17)(*[t.data_ptr() if t is not None else None for t in d])
        return ctx.lib.cf_regrid_apply(h, n, sp, dp, C.c_void_p(cov.data_ptr()))

    assert apply(0, src, dst) == -1 and apply(17, src, dst) == -1 and apply(-1, src, dst) == -1
    assert apply(3, src[:1] + [None] + src[2:], dst) == -1 and apply(3, src, dst[:2] + [None] + dst[3:]) == -1
    assert ctx.lib.cf_regrid_apply(h, 1, None, None, None) == -1 and ctx.lib.cf_regrid_apply(None, 1, None, None, None) == -1
    ctx.sync()
    assert all((t == SENTINEL).all().item() for t in dst + [cov]), "a rejected apply wrote"
    assert apply(16, src, dst) == 0
    ctx.sync()
    assert dst[15][0].item() == 1.0 and math.isnan(dst[15][1].item()) and dst[15][2].item() == 1.0 and (dst[15][3:] == SENTINEL).all().item()
    assert cov[:3].tolist() == [3.0, 0.0, 9.0] and (cov[3:] == SENTINEL).all().item()
    with pytest.raises(CofluxError, match="17"):
        ctx.regridder(rp, col, w).apply(src)
    assert ctx.lib.cf_regrid_destroy(h) == 0 and ctx.lib.cf_regrid_destroy(None) == 0
    # a regridder outlived by its context: apply fails, destroy works
    rc, h = _raw_create(ctx, rp, col, w)
    ctx.close()
    sp = (C.c_void_p * 1)(src[0].data_ptr())
    dp = (C.c_void_p * 1)(dst[0].data_ptr())
    assert ctx.lib.cf_regrid_apply(h, 1, sp, dp, None) == -1 and ctx.lib.cf_regrid_destroy(h) == 0


# ---- model level ---------------------------------------------------------------------------------------------------------------
def test_regridded_surface_means_under_run():
    model = _model(False)
    grid = model.ocean.grid
    ctx = model.interfaces.context
    averages = cm.SurfaceFluxAverages(model, schedule=cm.AveragedTimeInterval(3 * DT))
    map_op = rg.conservative_latlon_weights(grid, nlon=36, nlat=18)
    zonal_op = rg.zonal_mean_weights(grid, nlat=18)
    seen = []
    writer = rg.RegriddedSurfaceMeans(model, averages, map_op, zonal=zonal_op, on_window=lambda t, m, z, c: seen.append(t))
    cm.run(cm.Simulation(model, dt=DT, stop_iteration=6, output_writers={"surface": averages}))
    assert seen == [3 * DT, 6 * DT] and [w[0] for w in writer.windows] == seen and len(averages.windows) == 2
    wet_host = model.ocean.model.wet_mask.cpu().numpy() if ctx.params.mask_kind == abi.MASK_U8 else None
    assert wet_host is not None and (wet_host == 0).any()
    g = (NX, NY, H, H)
    for (t_k, arrays), (_, maps, zonal, coverage) in zip(averages.windows, writer.windows):
        names = list(arrays)
        assert list(maps) == names and list(zonal) == names
        fields = [rr.embed(arrays[n], H, H, np.nan) for n in names]
        for op, got, cov, shape in ((map_op, maps, coverage["map"], (18, 36)), (zonal_op, zonal, coverage["zonal"], (18,))):
            definition = rr.definition(*op, fields, wet_host, g)
            dst = np.stack([got[n].reshape(-1) for n in names])
            assert all(got[n].shape == shape for n in names) and cov.shape == shape
            check_against_definition(dst, cov.reshape(-1), definition, rr.MEAN, f"window {t_k}, {shape}")
            # the coverage is the regridded mask
            ones = rr.definition(*op, [np.ones_like(fields[0])], wet_host, g)
            assert all(abs(c - d["N"][0]) <= rr.coverage_bound(d) for c, d in zip(cov.reshape(-1), ones))
        assert np.isnan(maps[names[0]][0]).all() and np.isnan(zonal[names[0]][0]), "poleward of the source"
    writer.close()
    ctx.close()


# ---- the full surface, once ----------------------------------------------------------------------------------------------------
def test_full_quarter_degree_surface_against_fsum():
    nx, ny, h, K = 1440, 560, 7, 6
    grid = cm.LatitudeLongitudeGrid(size=(nx, ny, 10), halo=(h, h, h))
    ctx = FluxContext(nx, ny, h, h, ic.flux_params(), ring=1)
    wet = syn.ocean_state(nx, ny, h, h)["mask"]
    rng = np.random.default_rng(3)
    fields = [np.where(wet != 0, rng.standard_normal(wet.shape) * 10.0 ** (k - 2) + k, np.nan) for k in range(K)]
    src, mask = [ctx.to_device(f) for f in fields], ctx.to_device(wet)
    map_op, zonal_op = rg.conservative_latlon_weights(grid), rg.zonal_mean_weights(grid)
    lengths = np.diff(map_op.row_ptr)
    assert map_op.col.size == nx * ny and lengths.max() == 16 and (lengths == 16).sum() == 360 * 140
    assert zonal_op.col.size == nx * ny and (np.diff(zonal_op.row_ptr) == 4 * nx).sum() == 140
    g = (nx, ny, h, h)
    for op, rows, what in ((map_op, np.sort(rng.choice(np.flatnonzero(lengths > 0), 1000, replace=False)), "map"),
                           (zonal_op, np.arange(180), "zonal")):
        regridder = ctx.regridder(*op, mask=mask)
        dst = regridder.apply(src)
        ctx.sync()
        got = np.stack([d.cpu().numpy() for d in dst])
        cov = regridder.coverage.cpu().numpy()
        check_against_definition(got[:, rows], cov[rows], rr.definition(*op, fields, wet, g, rows=rows), rr.MEAN, f"1/4 degree {what}")
        empty = np.diff(op.row_ptr) == 0
        assert np.isnan(got[:, empty]).all() and (cov[empty] == 0.0).all()
        regridder.close()
    ctx.close()
