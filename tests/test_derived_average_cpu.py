"""CPU tests of the derived averager's host side (include/coflux.h: cf_average_create_derived): the NumPy restatement
(tests/derived_reference.py) is held to the definitions evaluated exactly, planted defects in copies of it are caught by
named cases, and the mirror (abi.py, models.py, the Julia stub) is held to the header."""
import ctypes as C
import re
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import derived_reference as dr
from coflux import abi
from coflux import models as cm
from test_julia_stub import HEADER, julia_structs, struct_size

NX, NY, HX, HY = 7, 5, 2, 3
U = Fraction(1, 2 ** 53)


def fields(seed, n=4):
    rng = np.random.default_rng(seed)
    shape = (NY + 2 * HY, NX + 2 * HX)
    return [rng.standard_normal(shape) * 10.0 ** rng.integers(-2, 3, shape) for _ in range(n)]


def leaves(kind, flags, a0, ax, ay, b0, by, c, s):
    """the exact leaf products of x: x = Σ leaves"""
    F = Fraction
    a0, ax, ay, b0, by, c, s = (F(float(v)) for v in (a0, ax, ay, b0, by, c, s))
    if kind == dr.FIELD:
        return [a0]
    if kind == dr.PRODUCT:
        return [a0 * b0]
    if kind == dr.CENTER_X:
        return [a0 / 2, ax / 2]
    if kind == dr.CENTER_Y:
        return [a0 / 2, ay / 2]
    if kind == dr.CENTER_X_SQUARE:
        return [a0 * a0 / 2, ax * ax / 2]
    if kind == dr.CENTER_Y_SQUARE:
        return [a0 * a0 / 2, ay * ay / 2]
    if kind == dr.KINETIC_ENERGY:
        return [a0 * a0 / 4, ax * ax / 4, b0 * b0 / 4, by * by / 4]
    p = [a0] if flags else [a0 / 2, ax / 2]
    q = [b0] if flags else [b0 / 2, by / 2]
    if kind == dr.EAST:
        return [x * c for x in p] + [-x * s for x in q]
    return [x * s for x in p] + [x * c for x in q]


def worst_excess(model, kind, flags, scale, seed=0):
    """max over the interior of |model − exact| / bound, bound = (k + 2) · 2⁻⁵³ · |scale| · Σ|leaves|"""
    a, b, c, s = fields(seed)
    got = model.sample(kind, flags, a, b, scale, c, s)
    k = dr.ROUNDINGS[kind]
    k = k[1 if flags else 0] if isinstance(k, tuple) else k
    worst = Fraction(0)
    for j in range(NY):
        for i in range(NX):
            J, I = j + HY, i + HX
            L = leaves(kind, flags, a[J, I], a[J, I + 1], a[J + 1, I], b[J, I], b[J + 1, I], c[J, I], s[J, I])
            exact = sum(L) * Fraction(scale)
            bound = (k + 2) * U * abs(Fraction(scale)) * sum(abs(x) for x in L)
            assert bound > 0
            worst = max(worst, abs(Fraction(float(got[j, i])) - exact) / bound)
    return float(worst)


CASES = [(k, 0) for k in range(9)] + [(dr.EAST, dr.AT_CENTERS), (dr.NORTH, dr.AT_CENTERS)]


@pytest.mark.parametrize("kind,flags", CASES)
@pytest.mark.parametrize("scale", [1.0, -1026.0, 1026.0 * 3991.86795711963])
def test_restatement_is_the_definition_within_its_roundings(kind, flags, scale):
    assert worst_excess(dr.DerivedModel(NX, NY, HX, HY), kind, flags, scale, seed=kind) <= 1.0


def test_scale_one_keeps_every_bit():
    m = dr.DerivedModel(NX, NY, HX, HY)
    a = fields(1)[0]
    a[HY, HX], a[HY + 1, HX], a[HY, HX + 1] = -0.0, np.nan, np.inf
    got = m.sample(dr.FIELD, 0, a, None, 1.0)
    assert np.array_equal(got.view(np.int64), m.here(a).view(np.int64))


def test_recurrence_stores_first_and_is_the_weighted_mean():
    rng = np.random.default_rng(5)
    xs, ws = [rng.standard_normal((NY, NX)) for _ in range(4)], [0.5, 2.0, 1.25, 3.0]
    got = dr.recurrence(list(zip(xs, ws)))
    exact = sum(x * w for x, w in zip(xs, ws)) / sum(ws)
    assert np.abs(got - exact).max() <= 1e-14 * max(np.abs(x).max() for x in xs)
    assert np.array_equal(dr.recurrence([(xs[0], 7.0)]).view(np.int64), xs[0].view(np.int64))


# ---- planted defects: each copy of the model is caught by its named case ------------------------------------------------------
class WrongRowPitch(dr.DerivedModel):
    """[i+1] addressed in a flat array whose rows are nx + hx long instead of nx + 2hx"""
    def east(self, a):
        j, i = np.meshgrid(np.arange(self.ny), np.arange(self.nx), indexing="ij")
        return a.ravel()[(j + self.hy) * (self.nx + self.hx) + self.hx + i + 1]


class SouthForNorth(dr.DerivedModel):
    def north(self, a):
        return a[self.hy - 1:self.hy + self.ny - 1, self.hx:self.hx + self.nx]


class SquareOfMean(dr.DerivedModel):
    def center_square(self, lo, hi):
        m = (lo + hi) * dr.HALF
        return m * m


class SwappedSineSign(dr.DerivedModel):
    def rotate_east(self, p, q, c, s):
        return p * c + q * s

    def rotate_north(self, p, q, c, s):
        return q * c - p * s


class ScaleBeforeSum(dr.DerivedModel):
    def sample(self, kind, flags, a, b, scale, cos=None, sin=None):
        if kind not in (dr.EAST, dr.NORTH):
            return super().sample(kind, flags, a, b, scale, cos, sin)
        p, q = self.components(flags, a, b)
        c, s, k = self.here(cos), self.here(sin), np.float64(scale)
        return p * c * k - q * s * k if kind == dr.EAST else p * s * k + q * c * k


class KineticEnergyTwice(dr.DerivedModel):
    def kinetic_energy(self, a, b):
        return self.center_square(self.here(a), self.east(a)) + self.center_square(self.here(b), self.north(b))


DEFECTS = [("i+1 with the wrong row pitch", WrongRowPitch, dr.CENTER_X, 0, 1.0, True),
           ("j+1 taken as j-1", SouthForNorth, dr.CENTER_Y, 0, 1.0, True),
           ("square of the mean for the mean of squares", SquareOfMean, dr.CENTER_X_SQUARE, 0, 1.0, True),
           ("sign of sin swapped between east and north", SwappedSineSign, dr.EAST, 0, 1.0, True),
           ("sign of sin swapped between east and north", SwappedSineSign, dr.NORTH, dr.AT_CENTERS, 1.0, True),
           # a difference of roundings only: inside the bound of the definition, outside the bits of the restatement
           ("scale before the rotation sum", ScaleBeforeSum, dr.EAST, 0, -1026.0, False),
           ("kinetic energy without its outer half", KineticEnergyTwice, dr.KINETIC_ENERGY, 0, 1.0, True)]


@pytest.mark.parametrize("name,defect,kind,flags,scale,gross", DEFECTS, ids=[d[0] + f" ({dr.KIND_NAMES[d[2]]})" for d in DEFECTS])
def test_planted_defect_is_caught(name, defect, kind, flags, scale, gross):
    a, b, c, s = fields(kind)
    good = dr.DerivedModel(NX, NY, HX, HY).sample(kind, flags, a, b, scale, c, s)
    bad = defect(NX, NY, HX, HY).sample(kind, flags, a, b, scale, c, s)
    assert not np.array_equal(good.view(np.int64), bad.view(np.int64)), name
    if gross:
        assert worst_excess(defect(NX, NY, HX, HY), kind, flags, scale, seed=kind) > 1.0, name


# ---- the mirror ----------------------------------------------------------------------------------------------------------------
def test_constants_and_structs_are_the_headers_and_the_stubs():
    for name in ("FIELD", "PRODUCT", "CENTER_X", "CENTER_Y", "CENTER_X_SQUARE", "CENTER_Y_SQUARE", "KINETIC_ENERGY", "EAST", "NORTH",
                 "AT_CENTERS"):
        value = int(re.search(rf"#define CF_TERM_{name}\s+(\d+)", HEADER).group(1))
        assert getattr(abi, "TERM_" + name) == value == getattr(dr, name), name
    assert abi.DERIVED_MAX_SOURCES == int(re.search(r"#define CF_DERIVED_MAX_SOURCES\s+(\d+)", HEADER).group(1))
    assert "cf_average_create_derived" in abi.EXPORTED_SYMBOLS
    structs = julia_structs()
    for name, twin in (("CfAverageTerm", abi.AverageTerm), ("CfAverageDesc", abi.AverageDesc)):
        assert struct_size(name, structs)[0] == C.sizeof(twin), name
        assert [f for f, _t in structs[name]] == [f for f, *_ in twin._fields_], name
    assert C.sizeof(abi.AverageTerm) == 40 and C.sizeof(abi.AverageDesc) == 40
    lib = abi.load_library()
    assert hasattr(lib, "cf_average_create_derived")


class FakeContext:
    """records what SurfaceFluxAverages asks the context for"""
    def __init__(self):
        self.calls = []

    def zeros(self):
        return torch.zeros((NY + 2 * HY, NX + 2 * HX), dtype=torch.float64)

    def average(self, sources, means):
        self.calls.append(("average", sources, means))
        return SimpleNamespace()

    def derived_average(self, terms, cos_rotation=None, sin_rotation=None):
        self.calls.append(("derived_average", terms, cos_rotation, sin_rotation))
        return SimpleNamespace()


def fake_model():
    ctx = FakeContext()
    grid = SimpleNamespace(size=(NX, NY, 1), halo=(HX, HY, 1), longitude=(0.0, 360.0))
    itf = SimpleNamespace(context=ctx, weights={}, _grid_rotation=None, net_fluxes=SimpleNamespace(_ocean_fields={}),
                          atmosphere_ocean_interface=SimpleNamespace(_fields={}))
    return SimpleNamespace(interfaces=itf, ocean=SimpleNamespace(grid=grid)), ctx


def test_expressions_lower_to_the_expected_terms():
    u, v = torch.zeros(3, dtype=torch.float64), torch.ones(3, dtype=torch.float64)
    T = abi
    assert cm.Squared(u).term() == (T.TERM_PRODUCT, 0, u, u, 1.0)
    assert cm.Product(u, v).term() == (T.TERM_PRODUCT, 0, u, v, 1.0)
    assert cm.CenteredX(u).term() == (T.TERM_CENTER_X, 0, u, None, 1.0)
    assert cm.CenteredY(v).term() == (T.TERM_CENTER_Y, 0, v, None, 1.0)
    assert cm.CenteredXSquare(u).term() == (T.TERM_CENTER_X_SQUARE, 0, u, None, 1.0)
    assert cm.CenteredYSquare(v).term() == (T.TERM_CENTER_Y_SQUARE, 0, v, None, 1.0)
    assert cm.KineticEnergy(u, v).term() == (T.TERM_KINETIC_ENERGY, 0, u, v, 1.0)
    assert cm.East(u, v).term() == (T.TERM_EAST, 0, u, v, 1.0)
    assert cm.North(u, v, at_centers=True).term() == (T.TERM_NORTH, T.TERM_AT_CENTERS, u, v, 1.0)
    assert cm.Scaled(cm.East(u, v), -1026.0).term() == (T.TERM_EAST, 0, u, v, -1026.0)
    assert cm.Scaled(cm.Scaled(cm.Squared(u), 2.0), 3.0).term() == (T.TERM_PRODUCT, 0, u, u, 6.0)
    assert cm.Scaled(u, 4.0).term() == (T.TERM_FIELD, 0, u, None, 4.0)
    assert cm.Scaled(cm.North(u, v), 2.0).rotates and not cm.Scaled(u, 2.0).rotates


def test_surface_flux_averages_builds_the_descriptor_and_keeps_plain_fields_on_cf_average_create():
    model, ctx = fake_model()
    a, b = ctx.zeros(), ctx.zeros()
    plain = cm.SurfaceFluxAverages(model, outputs=dict(x=a, y=b))
    assert [c[0] for c in ctx.calls] == ["average"]
    assert [t.data_ptr() for t in ctx.calls[0][1]] == [a.data_ptr(), b.data_ptr()]
    assert [t.data_ptr() for t in ctx.calls[0][2]] == [m.data_ptr() for m in plain.means.values()]
    # derived: kinds, flags, pointers, scales, the means in order; 18 outputs make two launches of 16 and 2 terms
    model, ctx = fake_model()
    outputs = dict(x=a, xx=cm.Squared(a), e=cm.Scaled(cm.East(a, b), -1026.0), n=cm.North(a, b, at_centers=True))
    outputs.update({f"k{k}": cm.KineticEnergy(a, b) for k in range(14)})
    w = cm.SurfaceFluxAverages(model, outputs=outputs)
    assert [c[0] for c in ctx.calls] == ["derived_average"] * 2 and len(w.averagers) == 2
    first, second = ctx.calls[0][1], ctx.calls[1][1]
    assert len(first) == 16 and len(second) == 2
    means = list(w.means.values())
    want = [(abi.TERM_FIELD, a, None, 1.0, 0), (abi.TERM_PRODUCT, a, a, 1.0, 0), (abi.TERM_EAST, a, b, -1026.0, 0),
            (abi.TERM_NORTH, a, b, 1.0, abi.TERM_AT_CENTERS)]
    for k, (kind, ta, tb, scale, flags) in enumerate(want):
        got = first[k]
        assert (got[0], got[3], got[4]) == (kind, scale, flags) and got[1] is ta and got[2] is tb and got[5] is means[k], k
    assert second[1][5] is means[17]
    # identity rotation where the grid has none (LatitudeLongitudeGrid)
    cos, sin = ctx.calls[0][2], ctx.calls[0][3]
    assert torch.equal(cos, torch.ones_like(cos)) and torch.equal(sin, torch.zeros_like(sin))


def test_library_written_fields_get_their_neighbour_halos_filled_before_a_collection():
    """East / North from faces on the net stresses read halo cells that the library never writes: the writer wraps the east
    column (a wall on a grid that does not close in longitude) and zeroes the north wall's row; fields that are not the
    library's (the ocean's own) are left alone."""
    rng = np.random.default_rng(3)
    for lon, periodic in (((0.0, 360.0), True), ((-180.0, 180.0), True), ((0.0, 90.0), False)):
        model, ctx = fake_model()
        model.ocean.grid.longitude = lon
        tu, tv, u, v = (torch.from_numpy(rng.standard_normal((NY + 2 * HY, NX + 2 * HX))) for _ in range(4))
        model.interfaces.net_fluxes._ocean_fields.update(u=tu, v=tv)
        before = [t.clone() for t in (tu, tv, u, v)]
        w = cm.SurfaceFluxAverages(model, outputs=dict(e=cm.Scaled(cm.East(tu, tv), -1026.0), n=cm.North(tu, tv), k=cm.KineticEnergy(u, v),
                                                       c=cm.East(tu, tv, at_centers=True)))
        assert [t.data_ptr() for t in w._east] == [tu.data_ptr()] and [(t.data_ptr(), s) for t, s in w._north] == [(tv.data_ptr(), -1.0)]
        w.fill_halos()
        want_u, want_v = before[0].clone(), before[1].clone()
        want_u[HY:HY + NY, HX + NX] = before[0][HY:HY + NY, HX] if periodic else 0.0
        want_v[HY + NY, HX:HX + NX] = 0.0
        assert torch.equal(tu, want_u) and torch.equal(tv, want_v) and torch.equal(u, before[2]) and torch.equal(v, before[3])
    assert cm.CenteredY(tv, fold_sign=1.0).fold_sign == 1.0 and cm.Scaled(cm.CenteredY(tv, fold_sign=1.0), 2.0).fold_sign == 1.0
    assert cm.Scaled(cm.East(tu, tv), 2.0).neighbours() == ([tu], [tv]) and cm.Squared(tu).neighbours() == ([], [])


def test_variance():
    rng = np.random.default_rng(2)
    x = rng.standard_normal((5, NY, NX)) + 3.0
    got = cm.variance((x * x).mean(0), x.mean(0))
    assert np.abs(got - x.var(0)).max() <= 1e-13 * (x * x).max()
    assert cm.variance(np.float64(4.0), np.float64(2.0)) == 0.0
