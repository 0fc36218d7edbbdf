"""The host's combination of a sharded run's diagnostics (coflux.distributed: combine_monitor_records,
combine_integral_records, restrict_operator, combine_regridded) against whole-array references, without a GPU: the monitor's
definition (tests/monitor_reference.py) on the whole 68 × 37 designed array and on every tile of the worlds (2,2) and (4,1), the
regridding's definition and order model (tests/regrid_reference.py) on a whole operator and on its restrictions.  The designed
array is tests/sharded_case.py's: numbering a tile's cells with the tile's own nx cannot pass it."""
import math
from types import SimpleNamespace

import numpy as np
import pytest

import monitor_reference as mr
import regrid_reference as rr
import sharded_case as sc
from coflux import distributed as cd
from coflux import regridding
from coflux.distributed import tile_bounds

NX, NY = sc.NX, sc.NY
KINDS = ("value", "abs")


def tiles(px, py):
    return [tile_bounds(NX, NY, r, px, py) for r in range(px * py)]


def tile_records(x, wet, px, py, row_length):
    """[rank] → record [kind] of the rank's cut, numbered with first_cell = j0·NX + i0 and `row_length`"""
    out = []
    for i0, i1, j0, j1 in tiles(px, py):
        w = None if wet is None else wet[j0:j1, i0:i1]
        out.append(np.array([mr.monitor_value(x[j0:j1, i0:i1], w, kind, first_cell=j0 * NX + i0, row_length=row_length) for kind in KINDS], dtype=mr.DTYPE))
    return out


def whole_record(x, wet):
    return np.array([mr.monitor_value(x, wet, kind) for kind in KINDS], dtype=mr.DTYPE)


def test_the_designed_array_holds_what_its_description_says():
    x, wet = sc.monitor_fixture()
    whole = whole_record(x, None)
    v, a = whole[0], whole[1]
    assert v["maximum"] == sc.MAXIMUM and v["argmax"] == sc.cell_number("max_first") < sc.cell_number("max_second")
    assert v["minimum"] == -np.inf and v["argmin"] == sc.cell_number("inf")
    assert (v["nan_count"], v["inf_count"], v["first_nonfinite"]) == (1, 1, sc.cell_number("nan"))
    assert a["maximum"] == np.inf and a["minimum"] == 0.0 and a["argmin"] == sc.cell_number("plus_zero")
    dry = whole_record(x, wet)[0]
    assert np.signbit(dry["minimum"]) and dry["minimum"] == 0.0 and dry["argmin"] == sc.cell_number("minus_zero") > sc.cell_number("plus_zero")
    assert (dry["nan_count"], dry["inf_count"], dry["first_nonfinite"]) == (0, 0, -1)
    # the ranks that hold them: the smaller index of each pair lies in the HIGHER rank, on both worlds
    for (px, py), ranks in (((2, 2), dict(max_first=1, max_second=0, plus_zero=1, minus_zero=2, nan=3, inf=2)),
                            ((4, 1), dict(max_first=2, max_second=0, plus_zero=3, minus_zero=0, nan=2, inf=0))):
        for name, rank in ranks.items():
            j, i = sc.CELLS[name]
            i0, i1, j0, j1 = tiles(px, py)[rank]
            assert i0 <= i < i1 and j0 <= j < j1, ((px, py), name, rank)


@pytest.mark.parametrize("px,py", sc.WORLDS)
@pytest.mark.parametrize("masked", [False, True])
def test_tile_records_numbered_with_the_global_row_length_combine_to_the_whole(px, py, masked):
    x, wet = sc.monitor_fixture()
    wet = wet if masked else None
    got = cd.combine_monitor_records(tile_records(x, wet, px, py, NX))
    want = whole_record(x, wet)
    for k, kind in enumerate(KINDS):
        for word in mr.DTYPE.names:
            assert got[k][word].tobytes() == want[k][word].tobytes(), ((px, py), kind, word, got[k][word], want[k][word])
    assert mr.same(got, want)


@pytest.mark.parametrize("px,py", sc.WORLDS)
def test_the_tiles_own_row_length_cannot_pass_the_designed_array(px, py):
    """row_length = 0 (the tile's nx), first_cell = j0·NX + i0 — the numbering before cf_monitor_desc had a row length: the tiles'
    hashes do not add up to the whole's, and argmax and first_nonfinite are not the whole's.  The fixture tells the two apart."""
    x, _ = sc.monitor_fixture()
    got = cd.combine_monitor_records(tile_records(x, None, px, py, 0))
    want = whole_record(x, None)
    assert int(got[0]["hash"]) != int(want[0]["hash"])
    assert int(got[0]["argmax"]) != int(want[0]["argmax"])
    assert int(got[0]["first_nonfinite"]) != int(want[0]["first_nonfinite"])
    assert (got[0]["nan_count"], got[0]["inf_count"], got[0]["maximum"]) == (want[0]["nan_count"], want[0]["inf_count"], want[0]["maximum"])


def test_a_row_length_equal_to_nx_or_zero_is_the_flat_numbering():
    x, wet = sc.monitor_fixture()
    for first in (0, 1000):
        flat = mr.monitor_value(x, wet, "value", first_cell=first)
        assert mr.same(flat, mr.monitor_value(x, wet, "value", first_cell=first, row_length=NX))
        assert not mr.same(flat, mr.monitor_value(x, wet, "value", first_cell=first, row_length=NX + 5))
    known = np.array([[0.0, -0.0, 1.0], [np.nan, np.inf, -1.5]])
    assert mr.state_hash(known.ravel()) == mr.state_hash(known, row_length=3) == 0xbc9733db8e1747df


def test_the_mirror_turns_a_tiles_cell_numbers_into_global_rows_and_columns():
    """coflux.outputs (SurfaceExtrema.series, NaNChecker.first) turns c into (j, i) with the monitor's row length: a tile's record,
    numbered with row_length = NX, gives the cell's place on the whole surface; 0, or a monitor without the attribute, stands for
    the model grid's nx"""
    from coflux import outputs
    model = SimpleNamespace(ocean=SimpleNamespace(grid=SimpleNamespace(size=(34, 19, 1))))
    assert outputs._row_length(SimpleNamespace(row_length=NX), model) == NX
    assert outputs._row_length(SimpleNamespace(row_length=0), model) == 34 == outputs._row_length(SimpleNamespace(), model)
    x, _ = sc.monitor_fixture()
    for (px, py), rank in (((2, 2), 1), ((4, 1), 2)):                       # the tile that holds the first maximum
        i0, i1, j0, j1 = tiles(px, py)[rank]
        v = mr.monitor_value(x[j0:j1, i0:i1], None, "value", first_cell=j0 * NX + i0, row_length=NX)
        tile = SimpleNamespace(row_length=NX)
        assert outputs._cell(v["argmax"], outputs._row_length(tile, model)) == sc.CELLS["max_first"]
        assert outputs._cell(v["argmax"], i1 - i0) != sc.CELLS["max_first"], "the tile's own nx gives another cell"
    assert outputs._cell(-1, NX) == (-1, -1)


def test_combine_monitor_records_on_series_and_on_empty_ranks():
    x, wet = sc.monitor_fixture()
    land = np.zeros_like(wet)
    per_rank = tile_records(x, land, 2, 2, NX)
    got = cd.combine_monitor_records(per_rank)
    assert mr.same(got, whole_record(x, land))
    assert (got[0]["minimum"], got[0]["maximum"], got[0]["argmin"], got[0]["argmax"], got[0]["first_nonfinite"]) == (np.inf, -np.inf, -1, -1, -1)
    # a series [n, n_entries] combines record by record; one all-land rank among wet ones does not enter the extrema
    mixed = wet.copy()
    mixed[:19, :34] = 0
    series = [np.stack([a, b]) for a, b in zip(tile_records(x, wet, 2, 2, NX), tile_records(x, mixed, 2, 2, NX))]
    assert mr.same(cd.combine_monitor_records(series), np.stack([whole_record(x, wet), whole_record(x, mixed)]))
    with pytest.raises(ValueError):
        cd.combine_monitor_records([per_rank[0], per_rank[1][:1]])


def test_combine_integral_records_is_the_correctly_rounded_sum_over_ranks():
    rng = np.random.default_rng(7)
    per_rank = [rng.standard_normal((3, 5)) * 10.0 ** rng.integers(-8, 9, (3, 5)) for _ in range(4)]
    per_rank[0][0, 0], per_rank[1][0, 0], per_rank[2][0, 0], per_rank[3][0, 0] = 1.0, 1e100, 1.0, -1e100   # fsum: 2, a plain sum: 0
    got = cd.combine_integral_records(per_rank)
    assert got.shape == (3, 5) and got[0, 0] == 2.0
    for r in range(3):
        for e in range(5):
            assert got[r, e] == math.fsum(float(p[r, e]) for p in per_rank)
    assert np.array_equal(got, cd.combine_integral_records(per_rank[::-1]))          # the order of the ranks does not enter
    bad = [np.array([np.inf, np.nan, 1.0]), np.array([-np.inf, 1.0, 2.0])]
    out = cd.combine_integral_records(bad)
    assert np.isnan(out[0]) and np.isnan(out[1]) and out[2] == 3.0


def _operators():
    src = SimpleNamespace(size=(NX, NY, 1), longitude=(0.0, 360.0), latitude=(-75.0, 80.0))
    return dict(zonal=regridding.zonal_mean_weights(src, nlat=12), latlon=regridding.conservative_latlon_weights(src, nlon=9, nlat=6))


def _regrid_arrays():
    rng = np.random.default_rng(11)
    fields = [1.0 + rng.random((NY, NX)), rng.standard_normal((NY, NX)) * 300.0]
    wet = (rng.random((NY, NX)) < 0.7).astype(np.uint8)
    wet[:10, :40] = 0            # destination cells with no ocean: NaN rows of the small latitude–longitude operator
    return fields, wet


@pytest.mark.parametrize("name", ["zonal", "latlon"])
@pytest.mark.parametrize("px,py", sc.WORLDS)
def test_restricted_operators_combine_to_the_whole_operators_mean(name, px, py):
    op = _operators()[name]
    fields, wet = _regrid_arrays()
    whole_grid = (NX, NY, 0, 0)
    want_def = rr.definition(*op, fields, wet, whole_grid)
    want, _ = rr.order_model(*op, fields, wet, whole_grid, mode=rr.MEAN)
    assert any(d["D"] == 0 for d in want_def) or name == "zonal"
    numerators, coverages, definitions, seen = [], [], [], []
    for i0, i1, j0, j1 in tiles(px, py):
        row_ptr, col, weight = cd.restrict_operator(op, NX, i0, i1, j0, j1)
        assert row_ptr.dtype == np.int64 and col.dtype == np.int32 and row_ptr.size == op.row_ptr.size and row_ptr[-1] == col.size == weight.size
        assert col.size == 0 or (col.min() >= 0 and col.max() < (i1 - i0) * (j1 - j0))
        nxl = i1 - i0
        back = (col // nxl + j0).astype(np.int64) * NX + (col % nxl + i0)               # the global cell numbers again
        seen.append([(r, int(c), float(w)) for r in range(op.n_rows) for c, w in zip(back[row_ptr[r]:row_ptr[r + 1]], weight[row_ptr[r]:row_ptr[r + 1]])])
        cut = [np.ascontiguousarray(f[j0:j1, i0:i1]) for f in fields]
        grid = (nxl, j1 - j0, 0, 0)
        N, D = rr.order_model(row_ptr, col, weight, cut, wet[j0:j1, i0:i1], grid, mode=rr.SUM)
        numerators.append(N)
        coverages.append(D)
        definitions.append(rr.definition(row_ptr, col, weight, cut, wet[j0:j1, i0:i1], grid))
    # every entry of the whole operator lies in exactly one tile, and each row keeps its order within a tile
    everything = sorted(e for s in seen for e in s)
    assert everything == sorted((r, int(c), float(w)) for r in range(op.n_rows) for c, w in zip(op.col[op.row_ptr[r]:op.row_ptr[r + 1]], op.weight[op.row_ptr[r]:op.row_ptr[r + 1]]))
    got = cd.combine_regridded(numerators, coverages)
    tol = sc.regrid_row_bounds(definitions + [want_def])
    exact = np.array([[rr.expected(d, f, rr.MEAN) for d in want_def] for f in range(len(fields))])
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isnan(got), np.isnan(exact))
    ok = ~np.isnan(exact)
    assert ok.any() and (np.abs(got - want)[ok] <= tol[ok]).all(), np.nanmax(np.abs(got - want) / np.where(tol > 0, tol, np.nan))
    assert (np.abs(got - exact)[ok] <= tol[ok]).all()
    assert (tol[ok] < 1e-12 * np.maximum(np.abs(exact[ok]), 1.0) * 300).all(), "the derived tolerance is a rounding bound, not a loose one"


def test_combine_regridded_gives_nan_where_no_rank_covers_a_row():
    N = [np.array([[1.0, 0.0, 2.0]]), np.array([[3.0, 0.0, 0.0]])]
    D = [np.array([2.0, 0.0, 4.0]), np.array([2.0, 0.0, 0.0])]
    got = cd.combine_regridded(N, D)
    assert got.shape == (1, 3) and got[0, 0] == 1.0 and np.isnan(got[0, 1]) and got[0, 2] == 0.5
    with pytest.raises(ValueError):
        cd.combine_regridded(N, D[:1])


def test_sum_bound_is_the_any_order_bound():
    rng = np.random.default_rng(3)
    t = rng.standard_normal(1000) * 10.0 ** rng.integers(-3, 4, 1000)
    exact, bound = sc.sum_bound(t)
    for order in (t, t[::-1], np.sort(t), rng.permutation(t)):
        s = 0.0
        for v in order:
            s += float(v)
        assert abs(s - exact) <= bound
    assert sc.gamma(0) == 0.0 and sc.sum_bound([5.0]) == (5.0, 0.0)
