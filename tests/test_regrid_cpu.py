"""CPU tests of the sparse surface operator's host side: the operator builders of coflux.regridding on deliberately non-nested
grids, the NumPy model of the device's summation order against the definition (regrid_reference.py), the planted defects the
operator atlas has to catch, and the three hand-kept copies of the ABI.

Tolerances of the builder checks count roundings, u = 2⁻⁵³.  A weight is fl(fl(R² · fl(rad(Δλ))) · fl(Δsin)): Δλ and Δsin are
differences of neighbouring piece boundaries, which telescope exactly over the pieces of a cell (adjacent pieces share the
same float boundary and hence the same sine), so a sum of P pieces differs from the cell's own area by at most 3 roundings
per piece and P − 1 additions — (4P + 4) u relative — plus what the cell's WIDTH loses: a longitude face is
fl(lo + fl(fl(i·Δ)/n)) and may be shifted by a multiple of 360°, 4 roundings of up to u · L each with L = 720° bounding every
longitude that occurs, so the width of a cell is off by up to 8 u L, relative 8 u L / Δλ (the latitude faces and their sines
are the same floats LatitudeLongitudeGrid.cell_areas() uses: nothing is lost there)."""
import ctypes as C
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import regrid_reference as rr
from coflux import abi
from coflux import models as cm
from coflux import regridding as rg
from test_julia_stub import HEADER, STUB, julia_structs, struct_size

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
L_MAX = 720.0
NEW_SYMBOLS = ("cf_regrid_create", "cf_regrid_destroy", "cf_regrid_apply")

SOURCES = {
    "100x37": cm.LatitudeLongitudeGrid(size=(100, 37, 4), halo=(3, 2, 2), longitude=(-180.0, 180.0), latitude=(-63.5, 71.25)),
    "7x5": cm.LatitudeLongitudeGrid(size=(7, 5, 4), halo=(2, 2, 2), longitude=(20.0, 380.0), latitude=(-80.0, 85.0)),
    "1x1": cm.LatitudeLongitudeGrid(size=(1, 1, 4), halo=(1, 1, 1), longitude=(0.0, 360.0), latitude=(-90.0, 90.0)),
}
DESTINATIONS = [(360, 180), (11, 7)]


def interior(a, grid):
    (nx, ny, _), (hx, hy, _) = grid.size, grid.halo
    return a[hy:hy + ny, hx:hx + nx]


def rel_tol(pieces, width):
    return (4 * pieces + 4 + 8 * L_MAX / width) * U


@pytest.fixture(scope="module")
def operators():
    return {(s, d): rg.conservative_latlon_weights(SOURCES[s], nlon=d[0], nlat=d[1]) for s in SOURCES for d in DESTINATIONS}


@pytest.mark.parametrize("dst", DESTINATIONS)
@pytest.mark.parametrize("src", list(SOURCES))
def test_column_and_row_sums_are_the_cell_areas(src, dst, operators):
    grid, op = SOURCES[src], operators[src, dst]
    nx, ny = grid.size[:2]
    nlon, nlat = dst
    assert op.shape == (nlat, nlon) and op.n_rows == nlon * nlat and op.col.dtype == np.int32 and op.row_ptr.dtype == np.int64
    assert (op.weight > 0).all() and op.col.min() >= 0 and op.col.max() < nx * ny
    rows = np.repeat(np.arange(op.n_rows), np.diff(op.row_ptr))
    area = interior(grid.cell_areas(), grid).ravel()
    width_src, width_dst = (grid.longitude[1] - grid.longitude[0]) / nx, 360.0 / nlon
    for c in range(nx * ny):
        w = op.weight[op.col == c]
        assert abs(math.fsum(w.tolist()) - area[c]) <= rel_tol(w.size, width_src) * area[c], (c, w.size)
    # destination cells that lie inside the source's latitude range are fully covered (every source spans the full circle)
    faces = -90.0 + np.arange(nlat + 1) * 180.0 / nlat
    dst_area = cm.EARTH_RADIUS ** 2 * np.deg2rad(width_dst) * np.diff(np.sin(np.deg2rad(faces)))
    covered = 0
    for j in range(nlat):
        full = grid.latitude[0] <= faces[j] and faces[j + 1] <= grid.latitude[1]
        for i in range(nlon):
            w = op.weight[rows == j * nlon + i] if (nlon * nlat <= 100 or i in (0, nlon // 3, nlon - 1)) else None
            if w is None:
                continue
            if full:
                covered += 1
                assert abs(math.fsum(w.tolist()) - dst_area[j]) <= rel_tol(w.size, min(width_dst, width_src)) * dst_area[j], (j, i)
            elif faces[j + 1] <= grid.latitude[0] or faces[j] >= grid.latitude[1]:
                assert w.size == 0, (j, i)
    assert covered > 0


@pytest.mark.parametrize("dst", DESTINATIONS)
@pytest.mark.parametrize("src", list(SOURCES))
def test_conservation_and_constant_fields(src, dst, operators):
    grid, op = SOURCES[src], operators[src, dst]
    (nx, ny, _), (hx, hy, _) = grid.size, grid.halo
    g = (nx, ny, hx, hy)
    rng = np.random.default_rng(nx)
    wet = (rng.random(grid.surface_shape) < 0.7).astype(np.uint8) if nx > 1 else np.ones(grid.surface_shape, np.uint8)
    x = rng.standard_normal(grid.surface_shape) * 20.0 + 3.0
    d = rr.definition(*op, [x, np.full(grid.surface_shape, 3.7)], wet, g)
    # Σ_d N_d = Σ_c A_c x_c m_c
    area, xi, mi = (interior(a, grid).ravel() for a in (grid.cell_areas(), x, wet))
    p, e = rr.two_product(area[mi != 0], xi[mi != 0])
    want, scale = math.fsum(p.tolist() + e.tolist()), math.fsum(np.abs(p).tolist())
    got = math.fsum(r["N"][0] for r in d)
    pieces = max(np.bincount(op.col, minlength=nx * ny))
    assert abs(got - want) <= (rel_tol(pieces, (grid.longitude[1] - grid.longitude[0]) / nx) + 2 * U) * scale
    # a constant maps to the constant wherever there is coverage (N, D and the quotient are each correctly rounded: 1.5 ulp),
    # and to NaN poleward of the source
    nlon, nlat = dst
    faces = -90.0 + np.arange(nlat + 1) * 180.0 / nlat
    seen_nan = 0
    for r, rec in enumerate(d):
        value = rr.expected(rec, 1, rr.MEAN)
        if rec["D"] > 0:
            assert abs(value - 3.7) <= 2 * np.spacing(3.7), (r, value)
        else:
            assert math.isnan(value)
            seen_nan += 1
        j = r // nlon
        if faces[j + 1] <= grid.latitude[0] or faces[j] >= grid.latitude[1]:
            assert rec["n"] == 0 and math.isnan(value), r
    assert seen_nan > 0 or src == "1x1"


@pytest.mark.parametrize("src", list(SOURCES))
def test_zonal_weights_are_the_map_summed_over_destination_longitude(src, operators):
    """… and one MEAN apply of them is the reference's row average of the regridded field, Σ_i N / Σ_i D — in exact rationals"""
    grid = SOURCES[src]
    (nx, ny, _), (hx, hy, _) = grid.size, grid.halo
    nlon, nlat = 11, 7
    op, zonal = operators[src, (nlon, nlat)], rg.zonal_mean_weights(grid, nlat=nlat)
    assert zonal.shape == (nlat,) and zonal.n_rows == nlat
    tol = Fraction(rel_tol(nlon + 2, (grid.longitude[1] - grid.longitude[0]) / nx))
    rows = np.repeat(np.arange(op.n_rows), np.diff(op.row_ptr))
    summed = {}
    for r, c, w in zip(rows, op.col, op.weight):
        summed[(r // nlon, int(c))] = summed.get((r // nlon, int(c)), 0) + Fraction(float(w))
    zrows = np.repeat(np.arange(nlat), np.diff(zonal.row_ptr))
    direct = {(int(b), int(c)): Fraction(float(w)) for b, c, w in zip(zrows, zonal.col, zonal.weight)}
    assert set(direct) == set(summed)
    for key, w in direct.items():
        assert abs(w - summed[key]) <= tol * w, key
    rng = np.random.default_rng(5)
    x = rng.standard_normal(nx * ny) * 10.0 + 2.0
    m = rng.random(nx * ny) < 0.7 if nx > 1 else np.ones(1, bool)
    for b in range(nlat):
        num = {k: sum(w * Fraction(float(x[c])) for (bb, c), w in table.items() if bb == b and m[c]) for k, table in (("z", direct), ("m", summed))}
        den = {k: sum(w for (bb, c), w in table.items() if bb == b and m[c]) for k, table in (("z", direct), ("m", summed))}
        assert (den["z"] == 0) == (den["m"] == 0)
        if den["z"] == 0:
            continue
        scale = sum(w * abs(Fraction(float(x[c]))) for (bb, c), w in direct.items() if bb == b and m[c]) / den["z"]
        assert abs(num["z"] / den["z"] - num["m"] / den["m"]) <= 2 * tol * scale, b


def test_zonal_band_weights_bin_by_centre_latitude():
    grid = SOURCES["100x37"]
    nx, ny = grid.size[:2]
    op = rg.zonal_band_weights(grid, nlat=18)
    assert op.shape == (18,) and op.col.size == nx * ny and sorted(op.col.tolist()) == list(range(nx * ny))
    phi, area = interior(grid.cell_latitudes(), grid).ravel(), interior(grid.cell_areas(), grid).ravel()
    rows = np.repeat(np.arange(18), np.diff(op.row_ptr))
    assert np.array_equal(rows, np.floor((phi[op.col] + 90.0) / 10.0).astype(int)) and np.array_equal(op.weight, area[op.col])
    # a grid that carries centres and areas only
    tri = cm.TripolarGrid(size=(40, 20, 4), halo=(3, 3, 2))
    with pytest.raises(ValueError, match="area"):
        rg.zonal_band_weights(tri)
    a = np.random.default_rng(0).random((20, 40)) + 1.0
    for given in (dict(area=a), dict()):
        t = cm.TripolarGrid(size=(40, 20, 4), halo=(3, 3, 2), **({} if given else dict(area=a)))
        op = rg.zonal_band_weights(t, nlat=30, **given)
        lat = interior(t.cell_latitudes(), t).ravel()
        rows = np.repeat(np.arange(30), np.diff(op.row_ptr))
        assert op.col.size == 800 and np.array_equal(op.weight, a.ravel()[op.col])
        assert np.array_equal(rows, np.minimum(np.floor((lat[op.col] + 90.0) / 6.0), 29).astype(int))
    assert "binning" in rg.zonal_band_weights.__doc__.lower() and "not conservative" in rg.zonal_band_weights.__doc__.lower()


def test_csr_from_triplets_is_a_stable_sort_that_keeps_duplicates():
    rows = [2, 0, 2, 0, 2, 4, 0]
    cols = [5, 9, 1, 9, 5, 0, 3]
    w = [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0]
    op = rg.csr_from_triplets(rows, cols, w, 5)
    assert op.row_ptr.tolist() == [0, 3, 3, 6, 6, 7] and op.shape == (5,)
    assert op.col.tolist() == [3, 9, 9, 1, 5, 5, 0]
    assert op.weight.tolist() == [7.0, 2.0, 4.0, 3.0, 1.0, 5.0, 6.0], "duplicates stay, in the order given"
    row_ptr, col, weight = op
    assert row_ptr is op.row_ptr and col is op.col and weight is op.weight
    for bad in (dict(rows=[5]), dict(rows=[-1]), dict(cols=[-1])):
        args = dict(rows=[0], cols=[0], weights=[1.0])
        args.update(bad)
        with pytest.raises(ValueError):
            rg.csr_from_triplets(args["rows"], args["cols"], args["weights"], 5)


# ---- the order model against the definition --------------------------------------------------------------------------------
ATLAS = rr.build_atlas()
GRID = (rr.ATLAS_NX, rr.ATLAS_NY, 3, 2)
OP = (ATLAS["row_ptr"], ATLAS["col"], ATLAS["weight"])


@pytest.fixture(scope="module")
def atlas_definition():
    fields, wet = rr.atlas_arrays(ATLAS, 3, 2)
    return fields, wet, rr.definition(*OP, fields, wet, GRID)


def failures(dst, cov, definition, mode, fields=(0,)):
    """names of the atlas rows whose value or coverage misses the bound"""
    out = []
    for name, r in ATLAS["names"].items():
        d = definition[r]
        ok = abs(cov[r] - d["D"]) <= rr.coverage_bound(d)
        for f in fields:
            want = rr.expected(d, f, mode)
            ok = ok and (math.isnan(dst[f, r]) if math.isnan(want) else abs(dst[f, r] - want) <= rr.bound(d, f, mode))
        if not ok:
            out.append(name)
    return out


def test_the_atlas_holds_every_case_it_names():
    names, n = ATLAS["names"], np.diff(ATLAS["row_ptr"])
    wet = ATLAS["wet"].ravel() != 0
    for count in (0, 1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1025):
        assert n[names[f"n{count}"]] == count
    cols = lambda name: ATLAS["col"][ATLAS["row_ptr"][names[name]]:ATLAS["row_ptr"][names[name] + 1]]  # noqa: E731
    weights = lambda name: ATLAS["weight"][ATLAS["row_ptr"][names[name]]:ATLAS["row_ptr"][names[name] + 1]]  # noqa: E731
    assert len(set(cols("n257").tolist())) < 257, "columns repeat"
    assert wet[cols("zero_weight")].all() and (weights("zero_weight") == 0).all()
    assert not wet[cols("all_land")].any()
    for name in ("partly_land", "partly_land_long", "same_short_a", "same_long_a"):
        assert wet[cols(name)].any() and not wet[cols(name)].all(), name
    nx, ny = rr.ATLAS_NX, rr.ATLAS_NY
    assert sorted(cols("corners").tolist()) == [0, nx - 1, (ny - 1) * nx, ny * nx - 1] and wet[cols("corners")].all()
    assert sorted(cols("row_ends").tolist()) == sorted([j * nx + i for j in range(ny) for i in (0, nx - 1)])
    assert (np.diff(cols("descending")) <= 0).all()
    for stem in ("same_short", "same_long"):
        a, b, c = (names[f"{stem}_{k}"] for k in "abc")
        assert a == min(a, 1) and c >= len(names) - 2 and a < b < c
        assert np.array_equal(cols(f"{stem}_a"), cols(f"{stem}_b")) and np.array_equal(weights(f"{stem}_a"), weights(f"{stem}_c"))


@pytest.mark.parametrize("mode", [rr.MEAN, rr.SUM])
def test_the_order_model_stays_within_the_bound(mode, atlas_definition):
    fields, wet, definition = atlas_definition
    dst, cov = rr.order_model(*OP, fields, wet, GRID, mode=mode)
    assert failures(dst, cov, definition, mode, fields=range(16)) == []
    names = ATLAS["names"]
    for stem in ("same_short", "same_long"):
        assert rr.same_bits(dst[:, names[f"{stem}_a"]], dst[:, names[f"{stem}_b"]])
        assert rr.same_bits(dst[:, names[f"{stem}_a"]], dst[:, names[f"{stem}_c"]])
    r = names["n0"]
    assert cov[r] == 0.0 and (np.isnan(dst[:, r]).all() if mode == rr.MEAN else (dst[:, r].view(np.int64) == 0).all())
    # the model does not depend on the halo widths
    for hx, hy in ((1, 1), (7, 2)):
        f2, w2 = rr.atlas_arrays(ATLAS, hx, hy)
        d2, c2 = rr.order_model(*OP, f2, w2, (rr.ATLAS_NX, rr.ATLAS_NY, hx, hy), mode=mode)
        assert rr.same_bits(d2, dst) and rr.same_bits(c2, cov)


CAUGHT_BY = {
    "drops_last_partial_segment": ("n65", "n255", "n257", "n1025"),
    "off_by_one_at_64": ("n65",),
    "off_by_one_at_256": ("n257", "n1025"),
    "nx_instead_of_pitch": ("row_ends", "corners", "n1"),
    "land_multiplied_by_zero": ("partly_land", "partly_land_long"),
    "coverage_includes_land": ("partly_land", "all_land"),
}


@pytest.mark.parametrize("defect", rr.DEFECTS)
def test_a_planted_defect_is_caught_at_the_bound_by_its_atlas_entry(defect, atlas_definition):
    fields, wet, definition = atlas_definition
    assert set(CAUGHT_BY) == set(rr.DEFECTS)
    dst, cov = rr.order_model(*OP, fields, wet, GRID, defect=defect)
    missed = failures(dst, cov, definition, rr.MEAN)
    for name in CAUGHT_BY[defect]:
        assert name in missed, (defect, name, missed)
    if defect.startswith("off_by_one"):     # and nowhere else: the boundaries are what the entries are there for
        assert set(missed) == set(CAUGHT_BY[defect]), missed


# ---- header, abi.py and the Julia stub ---------------------------------------------------------------------------------------
def test_the_three_copies_of_the_abi_list_the_new_names():
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    declared = set(re.findall(r"\b(cf_\w+)\s*\(", code))
    called = set(re.findall(r"\(:(cf_\w+), libcoflux\)", STUB))
    lib = abi.load_library()
    for name in NEW_SYMBOLS:
        assert name in declared and name in abi.EXPORTED_SYMBOLS and name in called and hasattr(lib, name), name
    assert re.search(r"#define CF_ABI_VERSION 5\b", HEADER) and abi.ABI_VERSION == 5 and lib.cf_version() == 5
    for macro, value in (("CF_REGRID_MAX_FIELDS", abi.REGRID_MAX_FIELDS), ("CF_REGRID_MEAN", abi.REGRID_MEAN), ("CF_REGRID_SUM", abi.REGRID_SUM)):
        assert re.search(rf"#define {macro} {value}\b", HEADER), macro
        assert re.search(rf"\b{macro}\b", STUB), macro
    assert abi.REGRID_MAX_FIELDS == 16
    for doc in ("INTEGRATION.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, doc)).read()
        for name in NEW_SYMBOLS + ("cf_regrid_desc",):
            assert name in text, (doc, name)
    # the summation order is stated where the issue asks for it
    kernel = open(os.path.join(ROOT, "climaocean.jl_amd", "csrc", "coflux_regrid.hip")).read()
    for text in (HEADER, kernel):
        assert re.search(r"entry count n alone", text, re.I) and "shfl_xor(v, 8), 4, 2, 1" in text


def test_the_struct_twins_agree():
    structs = julia_structs()
    assert "CfRegridDesc" in structs
    assert struct_size("CfRegridDesc", structs)[0] == C.sizeof(abi.RegridDesc) == 64
    assert [f for f, _t in structs["CfRegridDesc"]] == [f for f, *_ in abi.RegridDesc._fields_]
    body = re.search(r"typedef struct cf_regrid_desc \{(.*?)\} cf_regrid_desc;", HEADER, re.S).group(1)
    fields = re.findall(r"(\w+)(?:\[\w+\])?;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [f for f, *_ in abi.RegridDesc._fields_]
    for name, ctype in abi.RegridDesc._fields_:
        assert (ctype is C.c_int64) == (name in ("n_rows", "nnz"))
