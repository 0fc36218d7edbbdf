"""The solver's index machinery under designed wet masks (tests/mask_atlas.py).

Every flux solver launch is steered by the chunk table (csrc/coflux_solver.hip: chunk_block_costs / chunk_scan /
chunk_begins / chunk_wet_fill kernels, csrc/coflux_solver_lean.hip: lean_list_build_kernel), and the wet mask decides how
that table cuts the surface.  "A stale or overflowing table costs time, never correctness" hides a wrong builder from every
parity test, so here the table AS BUILT is read back (cf_debug_chunk_table) and held against a NumPy partition, and every
solver body runs on masks that put a wet cell exactly on a chunk or batch edge, behind a land run longer than the strips a
workgroup requests up front, in the window's last cell, only in the ring, on a window four cells wide.

CPU part (no marker): the partition worked by hand, the atlas entries' own properties, the partition's invariants.
GPU part: (a) table == reference partition, (b) eleven solver bodies × the atlas against the CPU oracle per cell, land
exactly as the oracle's, no sentinel left in the window, wet cells bitwise independent of the mask around them, (c) the
net-flux kernels where every face has a land neighbour, ring 1 and ring 0, (d) the step loop with tail workgroups.

Tolerances are the project's own (test_gpu_parity.TOL_SOLVER = 1e-9, TOL_LINEAR = 1e-12, the metric of tests/util.py) and
are met by the reference alone: on all four shapes with every cell wet no cell of the oracle reaches the 100-iteration cap
under default / corrected / ncar / sea_ice_corrected / fixed5 (largest trip count 36), and every atlas mask's wet set is a
subset of that — so compare()'s loosening for unconverged cells is not used and no cell is left out.

Wall time on the MI355X: this file's 32 GPU tests take 5.0 s as a pytest run of their own (no test above 0.5 s); the
`-m gpu` suite without the file ran 327 tests in 179 s, with it 359 tests in 201 s and 189 s in two runs (shared machines: the
multi-process tests vary by more than the file takes) — the file is under 3 % of the suite.

Each kind of check was seen to fail on a deliberately broken scratch build (not committed): an off-by-one in
chunk_begins_kernel's prev_cost → test_table_as_built_is_the_reference_partition[base_u8] (odd_columns: 5 of 12 begins
off by up to 39 cells, results still correct); the loop behind the LAND_UNROLL strips skipped, lean and fast kernel →
test_solver_body_under_the_atlas[default-base] and [ncar-base] (single_first: 3139 window cells left unwritten); row_of
without its q + 1 correction → test_solver_body_under_the_atlas[default-base] (38 cells, one per row, left unwritten)."""
import ctypes as C
import functools

import numpy as np
import pytest

import mask_atlas as ma
import util
from coflux import abi
from coflux import interface_computations as ic
from coflux.runtime import EXCHANGE_NAMES, FLUX_NAMES, FLUX_OPTIONAL, NET_NAMES

gpu = pytest.mark.gpu

H, RING = ma.HALO, ma.RING
TOL_SOLVER = 1e-9    # test_gpu_parity.TOL_SOLVER
TOL_LINEAR = 1e-12   # test_gpu_parity.TOL_LINEAR
FORCED = (256, 512, 768, 1024, 1280)
CELL_FIELDS = FLUX_NAMES + FLUX_OPTIONAL
ZERO_ON_LAND = tuple(k for k in CELL_FIELDS if k != "temperature")   # (land `temperature` is 0 K in ocean units, as in the oracle)


def plan(total_cost, cus=256, forced=0):
    """([(wet cells per chunk, chunks)], unit) of cf_debug_chunk_plan: host arithmetic, no GPU."""
    out = (C.c_int * 32)()
    unit = abi.load_library().cf_debug_chunk_plan(int(total_cost), int(cus), int(forced), out, 32)
    assert unit > 0
    return [(out[1 + 2 * r], out[2 + 2 * r]) for r in range(out[0])], unit


def total_cost(wet, unit=64):
    return int(wet.sum()) * unit + int((~wet).sum())


def window_of(shape):
    nx, ny = ma.SHAPES[shape]
    return ma.window_shape(nx, ny, RING)


# =============================================================================================
# CPU: the partition by hand, the atlas, the partition's invariants
# =============================================================================================
def test_hand_worked_partitions():
    rounds, unit = plan(300 * 64, 256, forced=256)
    assert unit == 64 and rounds == [(256, 2)]
    # 300 wet cells, chunks of 256: cell k has prefix 64 k, id k // 256
    begins, counts = ma.reference_partition(np.ones(300, bool), rounds, unit)
    assert begins.tolist() == [0, 256, 300] and counts.tolist() == [256, 44]
    # 3000 land cells (prefix 0 … 2999), then wet cell m at prefix 3000 + 64 m: below 256 · 64 = 16384 for m ≤ 209, so the
    # first chunk takes the land run and 210 wet cells, the second the other 90
    wet = np.arange(3300) >= 3000
    begins, counts = ma.reference_partition(wet, plan(total_cost(wet), 256, forced=256)[0], 64)
    assert begins.tolist() == [0, 3210, 3300] and counts.tolist() == [210, 90]
    # two rounds on 700 wet cells: two chunks of 256 cover prefixes below 2 · 16384 = cells 0 … 511; from base 32768 on,
    # chunks of 64 wet cells: 512, 576, 640, and the open-ended last round takes the rest
    begins, counts, sizes = ma.reference_partition(np.ones(700, bool), [(256, 2), (64, 3)], 64, with_sizes=True)
    assert begins.tolist() == [0, 256, 512, 576, 640, 700] and counts.tolist() == [256, 256, 64, 64, 60]
    assert sizes.tolist() == [256, 256, 64, 64, 64]
    # the last round is open-ended: a count that is too small changes nothing
    again, _ = ma.reference_partition(np.ones(700, bool), [(256, 2), (64, 1)], 64)
    assert again.tolist() == begins.tolist()
    # a land cell costs 1: 100 land cells between two wet runs move the cut by 100 / 64 of a wet cell
    wet = np.r_[np.ones(200, bool), np.zeros(100, bool), np.ones(200, bool)]
    begins, counts = ma.reference_partition(wet, [(256, 2)], 64)
    # wet cell m of the second run sits at prefix 12800 + 100 + 64 m ≥ 16384 from m = 55 on (12900 + 3520 = 16420)
    assert begins.tolist() == [0, 355, 500] and counts.tolist() == [255, 145]


def test_atlas_entries_have_the_property_they_are_named_for():
    nx, ny = ma.SHAPES["base"]
    wx, wy = window_of("base")
    n = wx * wy
    assert (wx, wy, n) == (133, 39, 5187)
    A = dict(ma.atlas(wx, wy))
    assert tuple(A) == ma.ATLAS_NAMES and len(A) == 18
    for wet in A.values():
        assert wet.shape == (wy, wx) and wet.dtype == bool and wet.flags.c_contiguous
    flat = {k: v.reshape(-1) for k, v in A.items()}
    where = lambda k: np.flatnonzero(flat[k]).tolist()   # noqa: E731
    assert where("single_first") == [0] and where("single_last") == [n - 1]
    assert where("four_corners") == [0, wx - 1, n - wx, n - 1]
    cb = A["checkerboard"]
    assert cb.sum() == 2594 and cb[0, 0] and not (cb[:, 1:] & cb[:, :-1]).any() and not (cb[1:] & cb[:-1]).any()
    assert not (~cb[:, 1:] & ~cb[:, :-1]).any() and not (~cb[1:] & ~cb[:-1]).any()
    assert A["odd_columns"].sum() == 66 * wy and A["odd_columns"][:, 1::2].all() and not A["odd_columns"][:, 0::2].any()
    assert A["odd_rows"].sum() == 19 * wx and A["odd_rows"][1::2].all() and not A["odd_rows"][0::2].any()
    assert A["one_row"].sum() == wx and A["one_row"][wy // 2].all()
    assert A["one_column"].sum() == wy and A["one_column"][:, wx // 2].all()
    assert A["ring_only"].sum() == n - nx * ny == 340 and not A["ring_only"][RING:-RING, RING:-RING].any()
    assert np.array_equal(A["interior_only"], ~A["ring_only"]) and A["interior_only"].sum() == nx * ny
    for name, m in (("first_256k", 768), ("first_256k_plus1", 769), ("first_256k_minus1", 767), ("first_64k_plus1", 321)):
        assert where(name) == list(range(m)), name
    assert where("land_run_then_wet") == list(range(3000, n))
    assert np.array_equal(flat["wet_then_land_run"], flat["land_run_then_wet"][::-1])
    assert where("every_97th") == list(range(0, n, 97)) and flat["every_97th"].sum() == 54
    blob = util.window(util.build_case(nx, ny, H, H)["ocean"]["mask"], H, H, nx, ny, RING) != 0
    assert np.array_equal(A["blob"], blob) and 0.2 < 1.0 - blob.mean() < 0.4
    # the ranges the issue describes, with chunks of 256 wet cells
    rounds, unit = plan(total_cost(A["land_run_then_wet"]), 256, forced=256)
    begins, counts = ma.reference_partition(A["land_run_then_wet"], rounds, unit)
    assert begins[1] == 3210 and counts[0] == 210              # all 210 wet cells lie beyond the eight strips of 256
    assert where("land_run_then_wet")[0] >= 8 * 256
    rounds, unit = plan(total_cost(A["every_97th"]), 256, forced=256)
    begins, counts = ma.reference_partition(A["every_97th"], rounds, unit)
    assert begins.tolist() == [0, n] and counts.tolist() == [54]
    # the embeddings: every wet byte value occurs, land is 0 / a bottom at or above the surface, and the window sits at the halo
    m8 = ma.embed(cb, nx, ny, kind="u8")
    assert m8.dtype == np.uint8 and m8.shape == (ny + 2 * H, nx + 2 * H)
    assert np.array_equal(util.window(m8, H, H, nx, ny, RING) != 0, cb) and set(np.unique(m8)) == {0, 1, 2, 255}
    outside = np.ones(m8.shape, bool)
    outside[H - RING:H + ny + RING, H - RING:H + nx + RING] = False
    assert not m8[outside].any()
    zb = ma.embed(cb, nx, ny, kind="bottom_height", z_surface=0.0)
    assert zb.dtype == np.float64 and set(np.unique(zb)) == {-3000.0, 0.0, 10.0}
    assert np.array_equal(util.window(~(0.0 <= zb), H, H, nx, ny, RING), cb) and np.all(0.0 <= zb[outside])


@pytest.mark.parametrize("shape", list(ma.SHAPES))
def test_reference_partition_properties(shape):
    """No chunk is empty, none holds more wet cells than its round's size, none is longer than unit × that size — for every
    atlas mask, the forced sizes and the automatic plan at 256 CUs."""
    wx, wy = window_of(shape)
    masks = list(ma.atlas(wx, wy)) + [("all_ocean", np.ones((wy, wx), bool))]
    for name, wet in masks:
        for forced in (0,) + FORCED:
            rounds, unit = plan(total_cost(wet), 256, forced)
            begins, counts, sizes = ma.reference_partition(wet, rounds, unit, with_sizes=True)
            label = (shape, name, forced, rounds)
            assert begins[0] == 0 and begins[-1] == wet.size and np.all(np.diff(begins) > 0), label
            assert np.all(counts <= sizes), label
            assert np.all(np.diff(begins) <= unit * sizes), label
            assert counts.sum() == wet.sum(), label
            assert len(counts) <= sum(c for _, c in rounds), label   # the plan's own count covers every chunk
            if forced:
                assert np.all(sizes == forced), label


# =============================================================================================
# GPU
# =============================================================================================
@functools.lru_cache(maxsize=None)
def _case(shape):
    nx, ny = ma.SHAPES[shape]
    return util.build_case(nx, ny, H, H, land=False)   # every cell's state; the masks come from the atlas


@functools.lru_cache(maxsize=None)
def _masks(shape):
    wx, wy = window_of(shape)
    out = dict(ma.atlas(wx, wy))
    out["all_ocean"] = np.ones((wy, wx), bool)
    return out


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _check_table(ctx, mask_dev, wet, forced, label):
    ctx.ensure_chunk_table(mask_dev)
    begins, counts, lists_valid = ctx.debug_chunk_table()
    rounds, unit = plan(total_cost(wet), _cus(), forced)
    ref_begins, ref_counts = ma.reference_partition(wet, rounds, unit)
    assert begins[0] == 0 and begins[-1] == wet.size and np.all(np.diff(begins.astype(np.int64)) > 0), (label, begins)
    assert len(begins) == len(ref_begins), (label, len(begins) - 1, len(ref_begins) - 1)
    np.testing.assert_array_equal(begins, ref_begins, err_msg=str(label))
    np.testing.assert_array_equal(counts, ref_counts, err_msg=str(label))
    assert lists_valid is True, label
    return rounds


TABLE_CASES = {
    # group: (shape, mask kind, mask names, forced sizes)
    "base_u8": ("base", "u8", ma.ATLAS_NAMES, (0, 256, 768, 1280)),
    "base_bottom_height": ("base", "bottom_height", ("checkerboard", "land_run_then_wet", "single_last"), (0, 256, 768, 1280)),
    "narrow": ("narrow", "u8", ("checkerboard", "odd_columns", "single_last"), (0, 256, 768, 1280)),
    "split": ("split", "u8", ("all_ocean", "checkerboard", "every_97th"), (0,)),
    "split_one_chunk": ("split", "u8", ("single_last",), (1280,)),
    "layered": ("layered", "u8", ("all_ocean", "checkerboard", "every_97th"), (0,)),
}


@gpu
@pytest.mark.parametrize("group", list(TABLE_CASES))
def test_table_as_built_is_the_reference_partition(group):
    """(a) begins and per-chunk wet counts of the device-built table == reference_partition, exactly; begins start at 0,
    rise strictly and end at the cell count; the static lists are in use."""
    from coflux.runtime import FluxContext
    shape, kind, names, forced_sizes = TABLE_CASES[group]
    nx, ny = ma.SHAPES[shape]
    params = ic.flux_params(mask_kind=abi.MASK_BOTTOM_HEIGHT if kind == "bottom_height" else abi.MASK_U8)
    masks = _masks(shape)
    for forced in forced_sizes:
        ctx = FluxContext(nx, ny, H, H, params, ring=RING)
        if forced:
            ctx.set_option(abi.OPT_AO_CHUNK, forced)
        keep = []   # every mask stays allocated: a fresh pointer each, so the table is rebuilt
        for name in names:
            wet = masks[name]
            keep.append(ctx.to_device(ma.embed(wet, nx, ny, kind=kind, z_surface=params.ocean_surface_z)))
            rounds = _check_table(ctx, keep[-1], wet, forced, (group, name, forced))
            if name == "all_ocean" and _cus() == 256:
                # what the shapes are sized for: a second round of one-wave chunks / the 768 and 512 arrival layers
                assert [w for w, _ in rounds] == ([256, 64] if shape == "split" else [768, 512]), rounds
            if group == "split_one_chunk":
                assert rounds == [(1280, 1)], rounds      # one chunk of 67 648 cells: the longest list offset in range
        ctx.close()


def test_debug_chunk_table_is_declared_like_its_neighbours():
    """The hook is exported, declared in the header and bound with six arguments (no GPU needed to see that)."""
    lib = abi.load_library()
    assert "cf_debug_chunk_table" in abi.EXPORTED_SYMBOLS and hasattr(lib, "cf_debug_chunk_table")
    assert len(lib.cf_debug_chunk_table.argtypes) == 6
    assert lib.cf_version() == abi.ABI_VERSION           # additive: no version bump came with it


@gpu
def test_debug_chunk_table_reports_missing_table_and_short_buffers():
    from coflux.runtime import CofluxError, FluxContext
    nx, ny = ma.SHAPES["base"]
    ctx = FluxContext(nx, ny, H, H, ic.flux_params(), ring=RING)
    with pytest.raises(CofluxError, match="no chunk table"):
        ctx.debug_chunk_table()
    wet = _masks("base")["checkerboard"]
    mask = ctx.to_device(ma.embed(wet, nx, ny))
    ctx.ensure_chunk_table(mask)
    n, valid = C.c_int(-1), C.c_int(-1)
    small = (C.c_int * 4)()
    rc = ctx.lib.cf_debug_chunk_table(ctx._h, small, small, 4, C.byref(n), C.byref(valid))
    assert rc != 0 and n.value == 11 and valid.value == 1     # too few ints: the count still comes back
    begins, counts, lists_valid = ctx.debug_chunk_table()
    assert len(begins) == 12 and len(counts) == 11 and lists_valid
    again = ctx.debug_chunk_table()                            # changes no state
    assert np.array_equal(again[0], begins) and np.array_equal(again[1], counts)
    ctx.close()


# ---------------------------------------------------------------------------------------------
# (b) every solver body under the atlas
# ---------------------------------------------------------------------------------------------
# name: (CONFIGS key, mode, options, solver) — mode "unfused": interpolate once, then solver + net launches per mask;
# "fused": cf_update_state; "hints": three solver calls per mask; "certified": cf_update_state on the certified path
BODIES = {
    "default": ("default", "unfused", (), abi.SOLVER_TABLES),                      # the lean kernel, log profile
    "corrected": ("corrected", "unfused", (), abi.SOLVER_TABLES),                  # the lean kernel, COARE profile
    "ncar": ("ncar", "unfused", (), abi.SOLVER_TABLES),                            # the fast kernel, Large–Yeager iteration
    "constant_roughness": ("sea_ice_corrected", "unfused", (), abi.SOLVER_TABLES),  # the fast kernel's constant-roughness body
    "fixed5": ("fixed5", "unfused", (), abi.SOLVER_TABLES),
    "default_libm": ("default", "unfused", (), abi.SOLVER_LIBM),
    "default_fused": ("default", "fused", (), abi.SOLVER_TABLES),
    "corrected_line": ("corrected", "fused", ((abi.OPT_LATENCY_LAYOUT, 2),), abi.SOLVER_TABLES),   # the line kernels
    "default_hints": ("default", "hints", ((abi.OPT_TRIP_HINTS, 1),), abi.SOLVER_TABLES),
    "default_certified": ("default", "certified", ((abi.OPT_SOLVER_PATH, abi.SOLVER_PATH_CERTIFIED),), abi.SOLVER_TABLES),
}
ELSEWHERE = ("checkerboard", "single_last")     # the masks of narrow, split and layered
BODY_CASES = [(b, "base") for b in BODIES] + [(b, s) for s in ("narrow", "split", "layered") for b in ("default", "corrected", "ncar")]

_oracle_cache = {}


def _params(config):
    fluxes, vd = util.CONFIGS[config]()
    return ic.flux_params(fluxes, velocity_difference=vd)


def _oracle_atmos(shape, ring=RING):
    import oracle as orc
    key = ("atmos", shape, ring)
    if key not in _oracle_cache:
        nx, ny = ma.SHAPES[shape]
        case = _case(shape)
        _oracle_cache[key] = orc.interpolate_atmosphere_state(orc.make_grid(nx, ny, H, H, ring), case["src"], case["weights"], 0, 1, 0.37)
    return _oracle_cache[key]


def _oracle(shape, config, name, ring=RING):
    """The CPU oracle under atlas mask `name` (computed once per (shape, formulation, mask), shared by the bodies)."""
    import oracle as orc
    key = (shape, config, name, ring)
    if key not in _oracle_cache:
        nx, ny = ma.SHAPES[shape]
        case, params = _case(shape), _params(config)
        g = orc.make_grid(nx, ny, H, H, ring)
        at = _oracle_atmos(shape, ring)
        oc = dict(case["ocean"], mask=ma.embed(_masks(shape)[name], nx, ny))
        fl = orc.compute_atmosphere_ocean_fluxes(g, params, oc, at, nthreads=0)
        net = orc.compute_net_ocean_fluxes(g, params, oc, at, fl, ice=None, weights=case["weights"])
        _oracle_cache[key] = dict(atmos=at, fluxes=fl, net=net)
    return _oracle_cache[key]


def _sentinel_fields(ctx, names, with_iterations=False):
    import torch
    out = {k: util._fill(torch.empty(ctx.shape, dtype=torch.float64, device=ctx.device), util.SENTINEL64) for k in names}
    if with_iterations:
        out["iterations"] = util._fill(torch.empty(ctx.shape, dtype=torch.int32, device=ctx.device), util.SENTINEL32)
    return out


def _untouched(a):
    """Cells that still hold the sentinel's bits."""
    if a.dtype == np.int32:
        return a == np.int32(util.SENTINEL32)
    return a.view(np.uint64) == np.uint64(util.SENTINEL64)


def _host(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _check_cells(shape, label, got, ref, wet, *, ring=RING, certified=False):
    """Checks 1-3 on the cell-local flux fields of one run (`got`, `ref`: halo-inclusive host arrays)."""
    nx, ny = ma.SHAPES[shape]
    W = lambda a: util.window(a, H, H, nx, ny, ring)   # noqa: E731
    land = ~wet
    for k in CELL_FIELDS + ("iterations",):
        left = int(_untouched(W(got[k])).sum())
        assert left == 0, (label, k, "window cells left unwritten", left)
    for k in CELL_FIELDS:
        g, r = W(got[k]), W(ref[k])
        assert np.array_equal(g[land], r[land]), (label, k, "land differs from the oracle")
        if k in ZERO_ON_LAND:
            nonzero = int(np.count_nonzero(g[land]))
            assert nonzero == 0, (label, k, "land is not exactly zero", nonzero)
    if certified:
        return
    it_g, it_r = W(got["iterations"]), W(ref["iterations"])
    np.testing.assert_array_equal(it_g, it_r, err_msg=f"{label} iterations")
    assert it_r.max(initial=0) < 100, (label, "the reference itself left a cell at the cap")
    for k in CELL_FIELDS:
        e = util.rel_err(W(got[k])[wet], W(ref[k])[wet], util.FIELD_SCALE[k])
        assert e <= TOL_SOLVER, (label, k, e)


def _check_net(shape, label, got_net, ref_net, tol=TOL_SOLVER):
    nx, ny = ma.SHAPES[shape]
    for k in NET_NAMES:
        g, r = util.window(got_net[k], H, H, nx, ny, 0), util.window(ref_net[k], H, H, nx, ny, 0)
        left = int(_untouched(g).sum())
        assert left == 0, (label, "net." + k, "interior cells left unwritten", left)
        e = util.rel_err(g, r, util.FIELD_SCALE[k])
        assert e <= tol, (label, "net." + k, e)


def _check_atmos(shape, label, got_atmos, ref_atmos):
    nx, ny = ma.SHAPES[shape]
    for k in EXCHANGE_NAMES:
        g, r = util.window(got_atmos[k], H, H, nx, ny, RING), util.window(ref_atmos[k], H, H, nx, ny, RING)
        left = int(_untouched(g).sum())
        assert left == 0, (label, "atmos." + k, "window cells left unwritten", left)
        e = util.rel_err(g, r, util.ATMOS_SCALE[k])
        assert e <= TOL_LINEAR, (label, "atmos." + k, e)


def _check_mask_independence(shape, label, got, ocean_run, wet):
    """Check 4: a wet cell's cell-local fields and trip count are the same BITS whatever the mask around it."""
    nx, ny = ma.SHAPES[shape]
    for k in CELL_FIELDS + ("iterations",):
        g, a = util.window(got[k], H, H, nx, ny, RING)[wet], util.window(ocean_run[k], H, H, nx, ny, RING)[wet]
        same = g.view(np.uint64) == a.view(np.uint64) if g.dtype == np.float64 else g == a
        assert same.all(), (label, k, "wet cells differ from the all-ocean run", int((~same).sum()))


@gpu
@pytest.mark.parametrize("body,shape", BODY_CASES, ids=[f"{b}-{s}" for b, s in BODY_CASES])
def test_solver_body_under_the_atlas(body, shape):
    """(b) One context per (shape, body), the masks looped inside on fresh device tensors (the table is rebuilt for each),
    every output pre-filled with sentinel bits.  Per run: (1) every window cell written, (2) land as in the oracle — the
    fluxes and similarity scales exactly 0.0, `temperature` the oracle's 0 K, trip counts the oracle's (0 under the
    convergence stop rule; FixedIterations and the coefficient-based fluxes count their fixed trips on land in the oracle
    too), (3) wet cells within TOL_SOLVER of the oracle per cell, identical trip counts, the net fields within TOL_SOLVER,
    the interpolated atmosphere within TOL_LINEAR, (4) wet cells bitwise the same body's all-ocean run.
    The certified path keeps the tolerances of tests/test_certified.py (compare_certified)."""
    import torch
    from coflux.runtime import FluxContext
    config, mode, options, solver = BODIES[body]
    nx, ny = ma.SHAPES[shape]
    case, params, masks = _case(shape), _params(config), _masks(shape)
    names = ("all_ocean",) + (ma.ATLAS_NAMES if shape == "base" else ELSEWHERE)
    ctx = FluxContext(nx, ny, H, H, params, ring=RING)
    ctx.set_option(abi.OPT_SOLVER, solver)
    for opt, val in options:
        ctx.set_option(opt, val)
    dev = ctx.to_device
    ocean = {k: dev(case["ocean"][k]) for k in ("T", "S", "u", "v")}
    src = {k: dev(v) for k, v in case["src"].items()}
    w = {k: (dev(v) if isinstance(v, np.ndarray) else v) for k, v in case["weights"].items()}
    atmos = None
    if mode in ("unfused", "hints"):
        atmos = _sentinel_fields(ctx, EXCHANGE_NAMES)
        ctx.interpolate_atmosphere_state(src, w, atmos, 0, 1, 0.37)
        ctx.sync()
        _check_atmos(shape, (body, shape), _host(atmos), _oracle_atmos(shape))
    keep, ocean_run = [], None
    for name in names:
        wet, label = masks[name], (body, shape, name)
        keep.append(dev(ma.embed(wet, nx, ny)))
        oc = dict(ocean, mask=keep[-1])
        ref = _oracle(shape, config, name)
        runs = []
        for call in range(3 if mode == "hints" else 1):
            fl = _sentinel_fields(ctx, CELL_FIELDS, with_iterations=True)
            net = _sentinel_fields(ctx, NET_NAMES)
            if mode in ("fused", "certified"):
                atmos = _sentinel_fields(ctx, EXCHANGE_NAMES)
                ctx.update_state(src, w, oc, atmos, fl, net, level1=0, level2=1, time_fraction=0.37)
            else:
                ctx.compute_atmosphere_ocean_fluxes(oc, atmos, fl)
                ctx.compute_net_ocean_fluxes(oc, atmos, fl, net, weights=w)
            ctx.sync()
            torch.cuda.synchronize()
            runs.append(dict(fluxes=_host(fl), net=_host(net), atmos=_host(atmos)))
        if body == "corrected_line":
            assert ctx.solver_latency_layout(), label
        if mode == "certified":
            assert ctx.solver_iteration_path() == abi.SOLVER_PATH_CERTIFIED
        for call, got in enumerate(runs):
            lab = label + (f"call {call}",)
            _check_cells(shape, lab, got["fluxes"], ref["fluxes"], wet, certified=mode == "certified")
            if mode == "certified":
                from test_certified import compare_certified
                ccase = dict(case, ocean=dict(case["ocean"], mask=ma.embed(wet, nx, ny)))
                compare_certified(ccase, got, ref, expect_certified=False, max_exact_share=1.0, label=str(lab))
            else:
                _check_net(shape, lab, got["net"], ref["net"])
            if mode in ("fused", "certified"):
                _check_atmos(shape, lab, got["atmos"], ref["atmos"])
            if name == "all_ocean":
                ocean_run = runs[0]["fluxes"]
            _check_mask_independence(shape, lab, got["fluxes"], ocean_run, wet)
    ctx.close()


@gpu
def test_sea_ice_interface_solve_under_the_atlas():
    """(b) 11: compute_atmosphere_sea_ice_fluxes with sea_ice_corrected, CF_SKIN_LINEARISED and the polar atmosphere, set up as
    tests/test_skin_linearised_gpu.py does.  Every mask: the window written, land zero (skin temperature 0 K, no trips), wet
    cells bitwise the all-ocean run.  blob, checkerboard and land_run_then_wet are also held to the NumPy restatement
    (tests/skin_linearised_reference.py) through util.compare_ice_fluxes at 1e-9, as
    test_linearised_interface_90x40_matches_the_reference does."""
    import skin_linearised_reference as slr
    from coflux.runtime import FluxContext
    shape = "base"
    nx, ny = ma.SHAPES[shape]
    case, masks = _case(shape), _masks(shape)
    fluxes_f, vd = util.ICE_CONFIGS["sea_ice_corrected"]()
    ice_params = ic.flux_params(fluxes_f, velocity_difference=vd)
    props = ic.SeaIceInterfaceProperties(skin_temperature_scheme=abi.SKIN_LINEARISED)
    at = util.polar_atmosphere(_oracle_atmos(shape))
    state = dict(case["ice_state"])
    ctx = FluxContext(nx, ny, H, H, ic.flux_params(), ring=RING)
    ctx.set_sea_ice_formulation(ice_params, props.to_params())
    dev = ctx.to_device
    ocean = {k: dev(case["ocean"][k]) for k in ("T", "S", "u", "v")}
    atmos = {k: dev(at[k]) for k in EXCHANGE_NAMES}
    st = {k: dev(v) for k, v in state.items() if v is not None}
    W = lambda a: util.window(a, H, H, nx, ny, RING)   # noqa: E731
    keep, ocean_run = [], None
    for name in ("all_ocean",) + ma.ATLAS_NAMES:
        wet, label = masks[name], ("interface", name)
        mask_np = ma.embed(wet, nx, ny)
        keep.append(dev(mask_np))
        out = _sentinel_fields(ctx, CELL_FIELDS, with_iterations=True)
        ctx.compute_atmosphere_sea_ice_fluxes(st, dict(ocean, mask=keep[-1]), atmos, out)
        ctx.sync()
        got = _host(out)
        for k in got:
            left = int(_untouched(W(got[k])).sum())
            assert left == 0, (label, k, "window cells left unwritten", left)
        land = ~wet
        for k in ZERO_ON_LAND:
            assert not np.any(W(got[k])[land]), (label, k, "land is not exactly zero")
        assert np.all(W(got["temperature"])[land] == -273.15) and not np.any(W(got["iterations"])[land]), label
        if name == "all_ocean":
            ocean_run = got
        _check_mask_independence(shape, label, got, ocean_run, wet)
        if name in ("blob", "checkerboard", "land_run_then_wet"):
            with np.errstate(all="ignore"):
                ref = slr.interface_fluxes(fluxes_f, props, state, dict(case["ocean"], mask=mask_np), at, hx=H, hy=H, ring=RING,
                                           scheme=abi.SKIN_LINEARISED, thermodynamics=ic.AtmosphereThermodynamicsParameters(),
                                           velocity_difference="wind" if isinstance(vd, ic.WindVelocity) else "relative")
            util.compare_ice_fluxes({k: W(v) for k, v in got.items()}, {k: W(v) for k, v in ref.items()}, 1e-9)
    ctx.close()


# ---------------------------------------------------------------------------------------------
# (c) the net-flux kernels at land / wet contacts
# ---------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("ring", [1, 0])
def test_net_fluxes_where_every_face_has_a_land_neighbour(ring):
    """(c) checkerboard, odd_columns, odd_rows and ring_only put a land neighbour on every face: the unfused
    compute_net_ocean_fluxes and the fused epilogue + face-stress kernel against the oracle.  The masks are the ring-1
    window's in both cases; with ring 0 the solver's window is the interior, so ring_only leaves it all land beside wet
    cells nobody solves.  (Ring 0: the flux fields start as zeros, not sentinels — the face averages at i = 0 / j = 0 read
    flux halos that nobody computed, zeros on both sides, as in test_ring0_and_ragged_sizes.)"""
    import oracle as orc
    import torch
    from coflux.runtime import FluxContext
    shape, config = "base", "default"
    nx, ny = ma.SHAPES[shape]
    case, params, masks = _case(shape), _params(config), _masks(shape)
    g = orc.make_grid(nx, ny, H, H, ring)
    at = orc.interpolate_atmosphere_state(g, case["src"], case["weights"], 0, 1, 0.37)
    for fused in (False, True):
        ctx = FluxContext(nx, ny, H, H, params, ring=ring)
        assert ctx.solver_path() == (True, 1)      # the lean kernel; cf_update_state fuses the net fluxes into its epilogue
        dev = ctx.to_device
        ocean = {k: dev(case["ocean"][k]) for k in ("T", "S", "u", "v")}
        src = {k: dev(v) for k, v in case["src"].items()}
        w = {k: (dev(v) if isinstance(v, np.ndarray) else v) for k, v in case["weights"].items()}
        keep = []
        for name in ("checkerboard", "odd_columns", "odd_rows", "ring_only"):
            label = (name, "ring", ring, "fused" if fused else "unfused")
            mask_np = ma.embed(masks[name], nx, ny)
            keep.append(dev(mask_np))
            oc = dict(ocean, mask=keep[-1])
            oc_np = dict(case["ocean"], mask=mask_np)
            ref_fl = orc.compute_atmosphere_ocean_fluxes(g, params, oc_np, at, nthreads=0)
            ref_net = orc.compute_net_ocean_fluxes(g, params, oc_np, at, ref_fl, ice=None, weights=case["weights"])
            if ring:
                fl = _sentinel_fields(ctx, CELL_FIELDS, with_iterations=True)
            else:
                fl = ctx.field_set(CELL_FIELDS)
                fl["iterations"] = ctx.zeros(torch.int32)
            net, atmos = _sentinel_fields(ctx, NET_NAMES), _sentinel_fields(ctx, EXCHANGE_NAMES)
            if fused:
                ctx.update_state(src, w, oc, atmos, fl, net, level1=0, level2=1, time_fraction=0.37)
            else:
                ctx.interpolate_atmosphere_state(src, w, atmos, 0, 1, 0.37)
                ctx.compute_atmosphere_ocean_fluxes(oc, atmos, fl)
                ctx.compute_net_ocean_fluxes(oc, atmos, fl, net, weights=w)
            ctx.sync()
            _check_net(shape, label, _host(net), ref_net)
            wet_in = util.window(mask_np, H, H, nx, ny, 0) != 0
            got_net = _host(net)
            for k in ("u", "v", "T", "S"):      # land cells of the interior take no flux
                assert not np.any(util.window(got_net[k], H, H, nx, ny, 0)[~wet_in]), (label, k)
            got_fl = _host(fl)
            for k in CELL_FIELDS:
                e = util.rel_err(util.window(got_fl[k], H, H, nx, ny, ring), util.window(ref_fl[k], H, H, nx, ny, ring), util.FIELD_SCALE[k])
                assert e <= TOL_SOLVER, (label, k, e)
        ctx.close()


# ---------------------------------------------------------------------------------------------
# (d) the step loop
# ---------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", ["checkerboard", "land_run_then_wet", "single_last"])
def test_time_steps_with_tail_workgroups_is_the_host_loop_bitwise(name):
    """(d) cf_time_steps with CF_OPT_MERGED_PREFETCH = 2 (the next step's interpolation in the solver launch's tail
    workgroups, the chunk plan made for them) == the host loop of cf_update_state calls, bit for bit, as
    test_steps.test_time_steps_reproduces_host_loop_bitwise["tail"] asserts for the blob."""
    import torch
    from coflux import synthetic as syn
    from coflux.runtime import FluxContext
    shape = "base"
    nx, ny = ma.SHAPES[shape]
    n, n_levels, inc = 21, 4, 1.0 / 9.0     # crosses two snapshot boundaries (9 steps per snapshot interval)
    ctx = FluxContext(nx, ny, H, H, ic.flux_params(), ring=RING)
    o0 = _case(shape)["ocean"]
    o1 = syn.evolved_ocean_state(o0, nx, ny, H, H, 1)
    mask = ctx.to_device(ma.embed(_masks(shape)[name], nx, ny))
    states = [dict({k: ctx.to_device(o[k]) for k in ("T", "S", "u", "v")}, mask=mask) for o in (o0, o1)]
    src = {k: ctx.to_device(v) for k, v in syn.jra55_snapshots(n_levels).items()}
    fi, fj, phi = syn.latlon_fractional_indices(nx, ny, H, H)
    w = dict(separable=True, fi=ctx.to_device(fi), fj=ctx.to_device(fj), latitude=ctx.to_device(phi))
    ref_atmos, ref_fl, ref_net = ctx.field_set(EXCHANGE_NAMES), ctx.field_set(FLUX_NAMES), ctx.field_set(NET_NAMES)
    for s in range(n):
        tot = s * inc
        l1 = int(tot) % n_levels
        ctx.update_state(src, w, states[s % 2], ref_atmos, ref_fl, ref_net, level1=l1, level2=(l1 + 1) % n_levels,
                         time_fraction=tot - int(tot))
    ctx.sync()
    ctx.set_option(abi.OPT_MERGED_PREFETCH, 2)
    sets = [ctx.field_set(EXCHANGE_NAMES) for _ in range(2)]
    fl, net = ctx.field_set(FLUX_NAMES), ctx.field_set(NET_NAMES)
    sched = ctx.make_schedule(states, sets, first_level=0, time_fraction=0.0, time_fraction_increment=inc, pipeline=True)
    ctx.time_steps(0, 8, sched, src, w, fl, net)      # in two calls: the step counter carries the clock
    ctx.time_steps(8, n - 8, sched, src, w, fl, net)
    ctx.sync()
    last = sets[(n - 1) % 2]
    for k in EXCHANGE_NAMES:
        assert torch.equal(last[k], ref_atmos[k]), (name, k)
    for k in FLUX_NAMES:
        assert torch.equal(fl[k], ref_fl[k]), (name, k)
    for k in NET_NAMES:
        assert torch.equal(net[k], ref_net[k]), (name, k)
    wet_in = util.window(mask.cpu().numpy(), H, H, nx, ny, 0) != 0
    assert np.any(util.window(fl["latent_heat"].cpu().numpy(), H, H, nx, ny, RING) != 0.0)   # the wet cells were solved
    assert not np.any(util.window(net["T"].cpu().numpy(), H, H, nx, ny, 0)[~wet_in])
    ctx.close()
