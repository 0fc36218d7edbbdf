"""Every interpolation path under a designed atlas of weight maps (tests/weight_atlas.py).

interpolate_atmosphere_state! is the first kernel of every step and exists in four hand-written copies; the tiled one is
instantiated for ROWS = 1, 2, 4 and runs in four launches.  ROWS follows the surface size alone, so before this file every
small-shape interpolation test ran interpolate_tiles<1>, ROWS = 4 met smooth geographic weights only, and the comparison was
to the C oracle at 1e-12 of a global field scale.  Here CF_OPT_INTERP_TILE_ROWS picks the instantiation on small windows, the
maps force the situations the index logic has code for, and the yardstick is the definition evaluated exactly, with a bound
against each cell's own corner values.

The bound is counted, not measured.  A result is Σ wₖ cₖ with Σ wₖ = 1 and |cₖ| ≤ M, so a relative rounding of any
intermediate moves it by at most 2⁻⁵³ M.  The device formula (and, in another order, the oracles') takes
  · the blend c = b·tf + a·(1 − tf): 1 − tf, two products, one sum                                     4
  · one weight (1 − ξ)(1 − η): two differences, one product                                            3
  · the product w·c and the three additions of the four corners                                        4
  · ξ = f − floor(f), exact for f ≥ 0 and for every f ≤ −1 that matters here, rounds for a tiny negative f      1
= 12 roundings, and the reference's own rounding to double is half an ulp more: |Δ| ≤ 13 · 2⁻⁵³ M < 16 · 2⁻⁵³ M, the accepted
bound for a scalar.  (A fused multiply-add only removes roundings.)  Mp adds one sum to two such results: ≤ 13 (+ 1) of
2⁻⁵³ (M_rain + M_snow) < 20.  A rotated wind u·cos + v·sin with |cos|, |sin| ≤ 1 carries 12 from each component, two products
and one sum: ≤ 15 (+ 1) of 2⁻⁵³ (M_u + M_v) < 24.  The land field is a scalar, twice when both sources are summed.

CPU part: every entry has its property under the tile model for ROWS 1 / 2 / 4 and caps 16 / 128 / 224; the clean model is
within the bound of the exact reference; every defect flag of the model is caught by named entries (the evidence that the
atlas discriminates); the C oracle and the NumPy oracle are within the bound on the whole atlas.
GPU part: cf_debug_interp_grid; cf_interpolate_atmosphere_state under ROWS × cap and the gather kernel, within the bound and
all ten bit for bit equal; the same through the pipelined cf_time_steps (auxiliary stream, merged stress + interpolation
launch, tail workgroups of both solver kernels) and cf_prefetch_atmosphere_state; cf_interpolate_land_freshwater.

Which entries catch which defect of the model (test_each_defect_is_caught prints the list; ROWS 4 and 1, cap 128, source
grids 16 × 8 and 17 × 9): ξ from trunc — the entries with a negative fractional index outside a clamped row (seam_west,
north_clamp, tiny, random); i⁺ = i⁻ + 1 — entries with negative fractional indices, seam_west and random among them; w01 / w10
swapped, tf swapped — the entries with fractional weights in both directions; rotation sign — every rotated entry; snow
dropped — all; row 0's clamp for every row — the entries whose fj varies from row to row, with ROWS > 1 only.

The GPU tests below were written without a device at hand and had not run on one when this file was committed.
"""
import functools

import numpy as np
import pytest

import weight_atlas as wa
from coflux import abi
from coflux import interface_computations as ic

gpu = pytest.mark.gpu

ACCEPTED_WINDOWS = tuple(w for w in wa.WINDOWS if w[2] >= w[4] + 1 and w[3] >= w[4] + 1)    # hx, hy ≥ ring + 1 (cf_create)
TILED = tuple((rows, cap) for rows in wa.ROWS for cap in wa.CAPS)


@functools.lru_cache(maxsize=None)
def _values(grid, kind="jra"):
    return wa.node_values(grid[0], grid[1], kind)


class _Entry:
    """One atlas entry with what the tests of this module share about it (kept while the entry is the current parameter)."""

    def __init__(self, name):
        self.name = name
        self._maps, self._exact, self._land = {}, {}, {}

    def maps(self, grid, win):
        key = (grid, win)
        if key not in self._maps:
            w = wa.weight_map(self.name, grid, win)
            self._maps[key] = (w, wa.window_maps(w, win))
        return self._maps[key]

    def exact(self, grid, win, blends=wa.BLENDS, kind="jra"):
        """{blend: (fields, M)}: the exact reference of every requested blend, computed once."""
        key = (grid, win, kind)
        have = self._exact.setdefault(key, {})
        missing = [b for b in blends if b not in have]
        if missing:
            _, (fi, fj, cs, sn) = self.maps(grid, win)
            cache = {}
            for (l1, l2, tf) in missing:
                have[(l1, l2, tf)] = wa.exact_interpolate(_values(grid, kind), fi, fj, l1, l2, tf, cs, sn, cache)
        return have

    def exact_land(self, grid, win, blends=wa.BLENDS):
        key = (grid, win)
        if key not in self._land:
            _, (fi, fj, _, _) = self.maps(grid, win)
            cache = {}
            self._land[key] = {(b, calving): wa.exact_land(_values(grid), fi, fj, *b, calving=calving, cache=cache)
                               for b in blends for calving in (False, True)}
        return self._land[key]


@pytest.fixture(scope="module", params=wa.NAMES)
def entry(request):
    return _Entry(request.param)      # (module scope: pytest runs the tests of one entry together, so its reference is computed once)


def _excess(got, ref, bound):
    """The largest |got − ref| / bound over the cells (0 / 0 = 0: where M is zero the result must be the reference's bits)."""
    d = np.abs(np.asarray(got, dtype=np.float64) - ref)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(bound > 0, d / bound, np.where(d == 0, 0.0, np.inf))
    r = np.where(np.isnan(d), np.inf, r)
    return float(r.max(initial=0.0))


def _worst(got, exact, M, rotated):
    b = wa.bounds(M, rotated)
    return {k: _excess(got[k], exact[k], b[k]) for k in wa.EXCHANGE_NAMES}


def _assert_within(got, exact, M, rotated, label):
    worst = _worst(got, exact, M, rotated)
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, (label, "|Δ| / bound", bad)


# =============================================================================================
# CPU
# =============================================================================================
def test_node_values_are_distinct_and_at_their_magnitudes():
    for grid in wa.SOURCE_GRIDS:
        v = _values(grid)
        assert set(v) == set(wa.VARIABLES) | {"friver", "licalvf"}
        for name, a in v.items():      # a wrong node or level of a variable is a different number
            assert np.unique(a).size == a.size, (grid, name)
        assert v["psl"].min() > 9e4 and v["prra"].max() < 1e-4 and v["prsn"].max() < 3e-5 and v["tas"].dtype == np.float32
        wide = _values(grid, "wide")
        for name in wa.VARIABLES:
            a = np.abs(wide[name].astype(np.float64))
            assert a.max() > 1e38 and (grid[0] * grid[1] < 2 or np.any((a > 0) & (a < 2.0 ** -126))), (grid, name)


def test_the_integer_reference_is_the_definition_in_fractions():
    """exact_interpolate's integers over a power-of-two denominator against fractions.Fraction, cell by cell: the same
    rational, so the same double."""
    rng = np.random.default_rng(3)
    for name, grid, win, kind in (("random", (17, 9), wa.WINDOWS[1], "jra"), ("tiny", (16, 8), wa.WINDOWS[4], "jra"),
                                  ("seam_west", (5, 3), wa.WINDOWS[1], "wide"), ("exact_nodes", (2, 2), wa.WINDOWS[2], "jra"),
                                  ("north_clamp", (1, 1), wa.WINDOWS[3], "wide")):
        _, (fi, fj, cs, sn) = _Entry(name).maps(grid, win)
        vals = _values(grid, kind)
        for (l1, l2, tf) in ((0, 1, 0.37), (2, 0, 2.0 ** -60), (1, 1, 1.0)):
            fields, _ = wa.exact_interpolate(vals, fi, fj, l1, l2, tf)
            land, _ = wa.exact_land(vals, fi, fj, l1, l2, tf)
            for _ in range(6):
                j, i = rng.integers(fi.shape[0]), rng.integers(fi.shape[1])
                cell = {v: wa.exact_cell(vals, v, fi[j, i], fj[j, i], l1, l2, tf) for v in wa.VARIABLES + ("friver", "licalvf")}
                for field, v in wa.SCALAR_FIELDS.items():
                    assert float(cell[v]) == fields[field][j, i], (name, field, j, i)
                assert float(cell["prra"] + cell["prsn"]) == fields["Mp"][j, i]
                assert float(cell["uas"]) == fields["u"][j, i] and float(cell["vas"]) == fields["v"][j, i]
                assert float(cell["friver"] + cell["licalvf"]) == land[j, i]
    # the rotation, in fractions as well
    from fractions import Fraction
    _, (fi, fj, cs, sn) = _Entry("seam_west").maps((16, 8), wa.WINDOWS[1])
    fields, M = wa.exact_interpolate(_values((16, 8)), fi, fj, 0, 1, 0.37, cs, sn)
    for (j, i) in ((0, 0), (3, 40), (6, 64)):
        u, v = (wa.exact_cell(_values((16, 8)), n, fi[j, i], fj[j, i], 0, 1, 0.37) for n in ("uas", "vas"))
        c, s = Fraction(float(cs[j, i])), Fraction(float(sn[j, i]))
        assert float(u * c + v * s) == fields["u"][j, i] and float(-u * s + v * c) == fields["v"][j, i]


def test_entry_has_its_property_for_every_instantiation(entry):
    """The situation an entry is in the atlas for is there — under the tile model — for ROWS 1 / 2 / 4 and caps 16 / 128 / 224:
    on at least one source grid and window each, and wherever it is listed below on all of them."""
    record = {}
    for rows, cap in TILED:
        hits = []
        for grid in wa.SOURCE_GRIDS[:5]:
            for n, win in enumerate(wa.WINDOWS):
                _, (fi, fj, _, _) = entry.maps(grid, win)
                if wa.has_property(entry.name, wa.tile_model(fi, fj, grid[0], grid[1], rows, cap), grid, rows, cap):
                    hits.append((grid, n))
        record[(rows, cap)] = hits
        assert hits, (entry.name, "ROWS", rows, "cap", cap, "no source grid and window shows the property")
    # the situations that need neither a small circle nor a large cap hold on the three larger grids, every multi-lane window
    base = entry.name.split("/")[0]
    if base in ("seam_east", "seam_west", "exact_nodes", "zeros", "one_node", "tiny", "north_clamp"):
        for (rows, cap), hits in record.items():
            for grid in wa.SOURCE_GRIDS[:3]:
                for n in (0, 1, 2, 4):
                    assert (grid, n) in hits, (entry.name, rows, cap, grid, n)
    print("[weight atlas] %s: (grid, window) pairs with the property per (ROWS, cap): %s" % (
        entry.name, {k: len(v) for k, v in record.items()}))


def test_every_instantiation_sees_both_the_staged_and_the_fallback_path():
    seen = {rc: set() for rc in TILED}
    for name in ("fold", "multi_row_fold", "random", "seam_east", "more_than_circle"):
        e = _Entry(name)
        for grid in wa.SOURCE_GRIDS[:3]:
            for win in wa.WINDOWS:
                _, (fi, fj, _, _) = e.maps(grid, win)
                for rows, cap in TILED:
                    seen[(rows, cap)] |= set(np.unique(wa.tile_model(fi, fj, grid[0], grid[1], rows, cap)["fits"]).tolist())
    assert all(s == {False, True} for s in seen.values()), seen


def test_clean_model_is_within_the_bound_of_the_exact_reference(entry):
    """The tile model reads its corners through the staged offsets (or the fallback's wrapped indices); with no defect flag it
    must land within the counted bound of the definition — for every instantiation, on every source grid and window."""
    blends = ((0, 1, 0.37), (2, 0, 2.0 ** -60))
    for grid in wa.SOURCE_GRIDS:
        for win in wa.WINDOWS:
            _, (fi, fj, cs, sn) = entry.maps(grid, win)
            for rows, cap in TILED:
                m = wa.tile_model(fi, fj, grid[0], grid[1], rows, cap)
                for b in (wa.BLENDS if (rows, cap) == (4, 128) else blends):
                    exact, M = entry.exact(grid, win)[b]
                    _assert_within(wa.model_values(m, _values(grid), *b, cs, sn), exact, M, cs is not None,
                                   (entry.name, grid, win, rows, cap, b))


@functools.lru_cache(maxsize=None)
def _defect_cases():
    """(name, grid, window, blend) → (maps, exact, M) of the cases the defects are tried on."""
    out = {}
    for name in wa.NAMES:
        e = _Entry(name)
        for grid in ((16, 8), (17, 9)):
            for win in (wa.WINDOWS[1], wa.WINDOWS[2]):
                for b in ((0, 1, 0.37), (2, 0, 0.37)):
                    out[(name, grid, win, b)] = (e.maps(grid, win)[1], e.exact(grid, win, (b,))[b])
    return out


@pytest.mark.parametrize("defect", wa.DEFECTS)
def test_each_defect_is_caught(defect):
    """A model with one defect — each keeps every index in range — exceeds the bound on at least one named entry: the atlas
    tells a subtly wrong index logic from the right one.  (The clean model passes the same cases: the test above.)"""
    catches = {}
    for (name, grid, win, b), ((fi, fj, cs, sn), (exact, M)) in _defect_cases().items():
        for rows in (4, 1):
            m = wa.tile_model(fi, fj, grid[0], grid[1], rows, 128, defects=(defect,))
            got = wa.model_values(m, _values(grid), *b, cs, sn, defects=(defect,))
            worst = _worst(got, exact, M, cs is not None)
            if max(worst.values()) > 1.0:
                catches.setdefault(name, set()).add(rows)
    print("[weight atlas] defect %s is caught by: %s" % (defect, {k: sorted(v) for k, v in sorted(catches.items())}))
    assert catches, (defect, "no atlas entry notices this defect: extend the atlas")
    if defect == "row0_clamp":      # one row per tile has no other row to take the clamp from
        assert all(v == {4} for v in catches.values()), catches
    if defect in ("xi_from_trunc", "plus_is_always_east"):
        assert {"seam_west", "random"} <= set(catches), catches      # (south_clamp's rows of negative fj are clamped: j⁻ = j⁺)
    if defect == "rotation_sign":
        assert {n for n in wa.NAMES if n.endswith("/2d")} <= set(catches), catches


def test_oracles_are_within_the_bound_of_the_exact_reference(entry):
    """The C oracle and the NumPy oracle are every other test's yardstick: on the whole atlas they are within the counted
    bound of the definition evaluated exactly (their order — every level interpolated, then blended — is the reference's)."""
    import numpy_oracle
    import oracle as orc
    for grid in wa.SOURCE_GRIDS:
        vals = _values(grid)
        src = {k: vals[k] for k in wa.VARIABLES}
        for win in wa.WINDOWS:
            w, (fi, fj, cs, sn) = entry.maps(grid, win)
            g = orc.make_grid(*win)
            for b in wa.BLENDS:
                exact, M = entry.exact(grid, win)[b]
                c_oracle = orc.interpolate_atmosphere_state(g, src, w, *b)
                _assert_within({k: wa.cut(v, win) for k, v in c_oracle.items()}, exact, M, cs is not None, ("C oracle", entry.name, grid, win, b))
                with np.errstate(over="ignore"):
                    np_oracle = numpy_oracle.interpolate_atmosphere_state(src, fi, fj, *b, cos_rot=cs, sin_rot=sn)
                _assert_within(np_oracle, exact, M, cs is not None, ("NumPy oracle", entry.name, grid, win, b))
                for calving in (False, True):
                    ref, Ml = entry.exact_land(grid, win)[(b, calving)]
                    got = orc.interpolate_land_freshwater(g, vals["friver"], vals["licalvf"] if calving else None, w, *b)
                    assert _excess(wa.cut(got, win), ref, wa.BOUND_SCALAR * wa.U * Ml) <= 1.0, ("C oracle, land", entry.name, grid, win, b, calving)


@pytest.mark.parametrize("name", ["random", "seam_west", "fold", "tiny"])
def test_wide_range_values_against_the_local_magnitude(name):
    """Nodes near the float32 maximum beside float32 subnormals: the clean model and both oracles stay within the bound taken
    against each cell's own corners (a global field scale would accept any error in the small cells)."""
    import numpy_oracle
    import oracle as orc
    e = _Entry(name)
    for grid in wa.SOURCE_GRIDS:
        vals = _values(grid, "wide")
        src = {k: vals[k] for k in wa.VARIABLES}
        for win in (wa.WINDOWS[1], wa.WINDOWS[3]):
            w, (fi, fj, cs, sn) = e.maps(grid, win)
            for b in ((0, 1, 0.37), (2, 0, 2.0 ** -60)):
                exact, M = e.exact(grid, win, (b,), "wide")[b]
                label = (name, grid, win, b)
                _assert_within(wa.model_values(wa.tile_model(fi, fj, grid[0], grid[1], 4, 128), vals, *b, cs, sn), exact, M, cs is not None, label)
                got = orc.interpolate_atmosphere_state(orc.make_grid(*win), src, w, *b)
                _assert_within({k: wa.cut(v, win) for k, v in got.items()}, exact, M, cs is not None, ("C oracle",) + label)
                _assert_within(numpy_oracle.interpolate_atmosphere_state(src, fi, fj, *b, cos_rot=cs, sin_rot=sn), exact, M, cs is not None,
                               ("NumPy oracle",) + label)


def test_the_new_option_and_hook_are_mirrored():
    lib = abi.load_library()
    assert abi.OPT_INTERP_TILE_ROWS == 15 and "cf_debug_interp_grid" in abi.EXPORTED_SYMBOLS and hasattr(lib, "cf_debug_interp_grid")
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "coflux.h")).read()
    numbers = [int(n) for n in re.findall(r"^#define CF_OPT_[A-Z_]+ (\d+)", header, flags=re.M)]
    assert re.search(r"^#define CF_OPT_INTERP_TILE_ROWS 15\b", header, flags=re.M) and max(numbers) == 15 and len(set(numbers)) == len(numbers)


# =============================================================================================
# GPU
# =============================================================================================
def _ctx(win, params=None):
    from coflux.runtime import FluxContext
    nx, ny, hx, hy, ring = win
    return FluxContext(nx, ny, hx, hy, params if params is not None else ic.flux_params(), ring=ring)


def _params(config):
    import util
    fluxes, vd = util.CONFIGS[config]()
    return ic.flux_params(fluxes, velocity_difference=vd)


def _device_weights(ctx, w):
    return {k: (ctx.to_device(v) if isinstance(v, np.ndarray) else v) for k, v in w.items()}


def _device_source(ctx, grid, kind="jra"):
    return {k: ctx.to_device(_values(grid, kind)[k]) for k in wa.VARIABLES}


def _set(ctx, rows, cap):
    ctx.set_option(abi.OPT_INTERP_TILE_CAP, cap)
    ctx.set_option(abi.OPT_INTERP_TILE_ROWS, rows)


class _Outputs:
    """n sets of the eight exchange fields in one tensor, NaN outside what a launch writes."""

    def __init__(self, ctx, n):
        import torch
        self.all = torch.empty((n, len(wa.EXCHANGE_NAMES)) + ctx.shape, dtype=torch.float64, device=ctx.device)
        self.sets = [{k: self.all[c, f] for f, k in enumerate(wa.EXCHANGE_NAMES)} for c in range(n)]

    def clear(self):
        self.all.fill_(float("nan"))

    def same_bits(self):
        import torch
        bits = self.all.view(torch.int64)
        return bool((bits[1:] == bits[:1]).all().item())

    def host(self, c, win):
        a = self.all[c].cpu().numpy()
        return {k: wa.cut(a[f], win) for f, k in enumerate(wa.EXCHANGE_NAMES)}


@gpu
def test_interp_grid_reports_the_rows():
    """cf_debug_interp_grid: automatic mode takes one row per tile on every atlas window, a forced 1 / 2 / 4 is what
    interpolate_grid returns (every launch form asks it), other values are refused; with the device's CU count the
    automatic choice is 2 rows at 1440 × 140 and 4 at 1440 × 560.  Nothing is launched."""
    import torch
    from coflux.runtime import CofluxError
    with pytest.raises(CofluxError, match="too small"):
        _ctx(wa.WINDOWS[0])                        # hx = hy = 1 with ring 1: the face stencils need ring + 1
    for win in ACCEPTED_WINDOWS:
        ctx = _ctx(win)
        wy, wx = wa.window_shape(win)
        assert ctx.debug_interp_grid() == (1, -(-((wx + 63) // 64 * wy) // 4)), win
        for rows in (1, 2, 4):
            ctx.set_option(abi.OPT_INTERP_TILE_ROWS, rows)
            assert ctx.debug_interp_grid() == (rows, -(-((wx + 63) // 64 * (-(-wy // rows))) // 4)), (win, rows)
        for bad in (-1, 3, 5, 8, 64):
            with pytest.raises(CofluxError, match="interp tile rows"):
                ctx.set_option(abi.OPT_INTERP_TILE_ROWS, bad)
        assert ctx.debug_interp_grid()[0] == 4      # a refused value changes nothing
        ctx.set_option(abi.OPT_INTERP_TILE_ROWS, 0)
        assert ctx.debug_interp_grid()[0] == 1
        ctx.close()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for (nx, ny), want in (((1440, 140), 2), ((1440, 560), 4)):
        ctx = _ctx((nx, ny, 2, 2, 1))
        tiles4 = ((nx + 2 + 63) // 64) * ((ny + 2 + 3) // 4) * 256 // cus
        rows, blocks = ctx.debug_interp_grid()
        assert rows == (4 if tiles4 >= 1200 else 2 if tiles4 >= 600 else 1) and rows == want, (nx, ny, cus, rows)
        ctx.set_option(abi.OPT_INTERP_TILE_ROWS, 1)
        assert ctx.debug_interp_grid()[0] == 1
        ctx.close()


@gpu
def test_interpolate_atmosphere_state_on_the_atlas(entry):
    """cf_interpolate_atmosphere_state on every source grid × window × blend under ROWS 1 / 2 / 4 × cap 16 / 128 / 224 and under
    cap 0 (the gather kernel): every result within the counted bound of the exact reference on the ring window, nothing of
    the window left unwritten, and the ten results equal bit for bit."""
    configs = TILED + ((0, 0),)
    for win in ACCEPTED_WINDOWS:
        ctx = _ctx(win)
        out = _Outputs(ctx, len(configs))
        for grid in wa.SOURCE_GRIDS:
            src = _device_source(ctx, grid)
            w, (_, _, cs, _) = entry.maps(grid, win)
            dw = _device_weights(ctx, w)
            for b in wa.BLENDS:
                out.clear()
                for c, (rows, cap) in enumerate(configs):
                    _set(ctx, rows, cap)
                    ctx.interpolate_atmosphere_state(src, dw, out.sets[c], *b)
                ctx.sync()
                exact, M = entry.exact(grid, win)[b]
                _assert_within(out.host(0, win), exact, M, cs is not None, (entry.name, grid, win, b))
                assert out.same_bits(), (entry.name, grid, win, b, "ROWS × cap and the gather kernel differ in bits")
        ctx.close()


@gpu
@pytest.mark.parametrize("name", ["random", "seam_west", "fold", "tiny"])
def test_wide_range_values_on_the_device(name):
    e = _Entry(name)
    configs = ((1, 128), (2, 16), (4, 224), (0, 0))
    for win in (wa.WINDOWS[1], wa.WINDOWS[3]):
        ctx = _ctx(win)
        out = _Outputs(ctx, len(configs))
        for grid in wa.SOURCE_GRIDS:
            src = _device_source(ctx, grid, "wide")
            w, (_, _, cs, _) = e.maps(grid, win)
            dw = _device_weights(ctx, w)
            for b in ((0, 1, 0.37), (2, 0, 2.0 ** -60)):
                out.clear()
                for c, (rows, cap) in enumerate(configs):
                    _set(ctx, rows, cap)
                    ctx.interpolate_atmosphere_state(src, dw, out.sets[c], *b)
                ctx.sync()
                exact, M = e.exact(grid, win, (b,), "wide")[b]
                _assert_within(out.host(0, win), exact, M, cs is not None, (name, grid, win, b))
                assert out.same_bits(), (name, grid, win, b)
        ctx.close()


STEP_ENTRIES = ("seam_east", "seam_west", "fold", "multi_row_fold", "south_clamp", "north_clamp", "random")
STEP_CASES = (((16, 8), wa.WINDOWS[1]), ((17, 9), wa.WINDOWS[2]))


def _ocean_states(ctx, win):
    from coflux import synthetic as syn
    nx, ny, hx, hy, ring = win
    o0 = syn.ocean_state(nx, ny, hx, hy, land_fraction=True)
    o1 = syn.evolved_ocean_state(o0, nx, ny, hx, hy, 1)
    mask = ctx.to_device(o0["mask"])
    return [dict({k: ctx.to_device(o[k]) for k in ("T", "S", "u", "v")}, mask=mask) for o in (o0, o1)]


@gpu
@pytest.mark.parametrize("solver", ["similarity", "large_yeager"])
@pytest.mark.parametrize("merged", [0, 1, 2])
def test_time_steps_on_the_atlas(merged, solver):
    """Two pipelined steps of cf_time_steps with two exchange sets, as test_layout_footprint.py::test_time_steps sets it up:
    step 0's state is interpolated by the stand-alone launch into set 0, step 1's is requested ahead into set 1 and goes out
    — CF_OPT_MERGED_PREFETCH = 0 — on the auxiliary stream, — 1 — in the merged stress + interpolation launch, — 2 — in the
    tail workgroups of the solver launch: the lean ocean kernel's (coflux_lean_kernel.hpp) under SimilarityTheoryFluxes, the
    CoefficientBasedFluxes kernel's (coflux_solver.hip) under the Large–Yeager formulation.  Forced ROWS 1 / 2 / 4 on the
    seam, fold, clamp and random entries; both sets within the bound of the exact reference and equal, bit for bit, to the
    stand-alone launch.

    That the intended form ran is asserted as far as the library can be asked: cf_solver_path says which solver kernel runs
    and that the net fluxes are fused into it — the two conditions, with a tile that fits the carrying launch's LDS (cap 128:
    36 864 B of the solver launch's 40 960), under which update_state_impl takes the merged and the tail form; nothing on a
    small surface switches them off (there is no size condition).  No query reports the launch itself."""
    import torch
    from coflux.runtime import FLUX_NAMES, NET_NAMES
    params = _params("default" if solver == "similarity" else "ncar")
    tf0, inc = 0.37, 0.75
    steps = []
    for s in range(2):
        total = tf0 + float(s) * inc
        whole = int(np.floor(total))
        steps.append((whole % wa.N_LEVELS, (whole % wa.N_LEVELS + 1) % wa.N_LEVELS, total - whole))
    for grid, win in STEP_CASES:
        ctx = _ctx(win, params)
        lean, fused = ctx.solver_path()
        assert fused == 1 and lean == (solver == "similarity")
        assert (params.flux_formulation == abi.FORMULATION_LARGE_YEAGER) == (solver == "large_yeager")
        ctx.set_option(abi.OPT_MERGED_PREFETCH, merged)
        states = _ocean_states(ctx, win)
        src = _device_source(ctx, grid)
        alone, sets = _Outputs(ctx, 2), _Outputs(ctx, 2)
        fl, net = ctx.field_set(FLUX_NAMES), ctx.field_set(NET_NAMES)
        for name in STEP_ENTRIES:
            e = _Entry(name)
            w, (_, _, cs, _) = e.maps(grid, win)
            dw = _device_weights(ctx, w)
            exact = e.exact(grid, win, tuple(steps))
            for rows in wa.ROWS:
                _set(ctx, rows, 128)
                assert ctx.debug_interp_grid()[0] == rows
                alone.clear()
                sets.clear()
                for s, b in enumerate(steps):
                    ctx.interpolate_atmosphere_state(src, dw, alone.sets[s], *b)
                sched = ctx.make_schedule(states, sets.sets, first_level=0, time_fraction=tf0, time_fraction_increment=inc, pipeline=True)
                ctx.time_steps(0, 2, sched, src, dw, fl, net)
                ctx.sync()
                for s, b in enumerate(steps):
                    _assert_within(sets.host(s, win), exact[b][0], exact[b][1], cs is not None, (name, grid, win, "merged", merged, "ROWS", rows, "step", s))
                assert torch.equal(sets.all.view(torch.int64), alone.all.view(torch.int64)), (name, grid, win, merged, rows)
                assert bool(torch.isfinite(wa.cut(fl["latent_heat"], win)).all())
        ctx.close()


@gpu
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_prefetch_atmosphere_state_on_the_atlas(mode):
    """cf_prefetch_atmosphere_state: a request that no solver launch follows is flushed by cf_sync and goes out on the auxiliary
    stream, whatever CF_OPT_MERGED_PREFETCH says; followed by cf_update_state it rides as that mode decides — the counters of
    cf_debug_prefetch_stats say that it did: one launch on the auxiliary stream, one by the mode's own route.  Both ways the
    requested set is within the bound of the exact reference and has the stand-alone launch's bits."""
    import torch
    from coflux.runtime import FLUX_NAMES, NET_NAMES
    first, ahead = (0, 1, 0.37), (2, 0, 2.0 ** -60)
    for grid, win in STEP_CASES:
        ctx = _ctx(win)
        ctx.set_option(abi.OPT_MERGED_PREFETCH, mode)
        states = _ocean_states(ctx, win)
        src = _device_source(ctx, grid)
        out = _Outputs(ctx, 4)            # stand-alone; flushed request; current step's set; request that rides with a step
        fl, net = ctx.field_set(FLUX_NAMES), ctx.field_set(NET_NAMES)
        for name in ("seam_east", "fold", "south_clamp", "random"):
            e = _Entry(name)
            w, (_, _, cs, _) = e.maps(grid, win)
            dw = _device_weights(ctx, w)
            exact, M = e.exact(grid, win, (ahead,))[ahead]
            for rows, cap in ((1, 128), (2, 128), (4, 128), (4, 16), (0, 0)):
                if cap == 0 and mode != 0:
                    continue               # the merged forms need the tiled interpolation
                _set(ctx, rows, cap)
                out.clear()
                before = ctx.prefetch_stats()
                ctx.interpolate_atmosphere_state(src, dw, out.sets[0], *ahead)
                ctx.prefetch_atmosphere_state(src, dw, out.sets[1], *ahead)
                ctx.sync()
                ctx.prefetch_atmosphere_state(src, dw, out.sets[3], *ahead)
                ctx.update_state(src, dw, states[0], out.sets[2], fl, net, level1=first[0], level2=first[1], time_fraction=first[2])
                ctx.sync()
                label = (name, grid, win, "mode", mode, "ROWS", rows, "cap", cap)
                moved = {k: v - before[k] for k, v in ctx.prefetch_stats().items() if k.startswith("launched_") and v != before[k]}
                route = ("launched_aux", "launched_merged", "launched_tail")[mode]
                assert moved == ({"launched_aux": 2} if mode == 0 else {"launched_aux": 1, route: 1}), (label, moved)
                _assert_within(out.host(1, win), exact, M, cs is not None, label)
                bits = out.all.view(torch.int64)
                assert torch.equal(bits[1], bits[0]) and torch.equal(bits[3], bits[0]), label
        ctx.close()


@gpu
def test_interpolate_land_freshwater_on_the_atlas(entry):
    """cf_interpolate_land_freshwater (interpolate_land_kernel, the fourth copy of the index logic) with and without licalvf
    against the exact reference: the scalar bound, twice when both sources are summed."""
    import torch
    for win in ACCEPTED_WINDOWS:
        ctx = _ctx(win)
        out = torch.empty(ctx.shape, dtype=torch.float64, device=ctx.device)
        for grid in wa.SOURCE_GRIDS:
            friver, licalvf = (ctx.to_device(_values(grid)[k]) for k in ("friver", "licalvf"))
            w, _ = entry.maps(grid, win)
            dw = _device_weights(ctx, w)
            for b in wa.BLENDS:
                for calving in (False, True):
                    out.fill_(float("nan"))
                    ctx.interpolate_land_freshwater(friver, licalvf if calving else None, dw, out, *b)
                    ctx.sync()
                    ref, M = entry.exact_land(grid, win)[(b, calving)]
                    assert _excess(wa.cut(out.cpu().numpy(), win), ref, wa.BOUND_SCALAR * wa.U * M) <= 1.0, (entry.name, grid, win, b, calving)
        ctx.close()
