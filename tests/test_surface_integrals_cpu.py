"""Host side of the surface integrals (coflux.models: cell_areas, hemisphere_regions, the SurfaceIntegrals writer and its
presets) and the three hand-kept copies of the new ABI (header, abi.py, Julia stub) — no GPU: the writer is driven through a
stand-in context whose integrator restates cf_integrals_collect with numpy sums."""
import ctypes as C
import math
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from coflux import abi
from coflux import models as cm
from test_julia_stub import HEADER, STUB, julia_structs, struct_size

NEW_SYMBOLS = ("cf_integrals_create", "cf_integrals_destroy", "cf_integrals_collect", "cf_integrals_count", "cf_integrals_read",
               "cf_integrals_reset", "cf_attach_integrals")


# ---- the grid's weights ------------------------------------------------------------------------------------------------------
def test_cell_areas_of_the_readme_grid_sum_to_the_area_of_the_band():
    grid = cm.LatitudeLongitudeGrid()      # 1440 × 560, halo 7, 70°S … 70°N
    (nx, ny, _), (hx, hy, _) = grid.size, grid.halo
    A = grid.cell_areas()
    assert A.shape == grid.surface_shape and A.dtype == np.float64 and (A > 0).all()
    total = math.fsum(A[hy:hy + ny, hx:hx + nx].ravel().tolist())
    want = cm.EARTH_RADIUS ** 2 * 2 * math.pi * (math.sin(math.radians(70)) - math.sin(math.radians(-70)))
    assert abs(total - want) <= 1e-12 * want, (total, want)
    # rows of one latitude are equal, the band is symmetric about the equator
    assert (A == A[:, :1]).all() and np.allclose(A[hy:hy + ny, 0], A[hy:hy + ny, 0][::-1], rtol=1e-12)
    # the cell north of the equator: R² Δλ (sin Δφ − sin 0)
    dl, dphi = math.radians(360 / nx), math.radians(140 / ny)
    assert A[hy + ny // 2, hx] == pytest.approx(cm.EARTH_RADIUS ** 2 * dl * math.sin(dphi), rel=1e-12)


def test_hemisphere_regions_are_strict():
    grid = cm.LatitudeLongitudeGrid(size=(8, 23, 1), halo=(2, 3, 1))     # an odd number of rows: row 11 sits at φ = 0 exactly
    (nx, ny, _), (hx, hy, _) = grid.size, grid.halo
    phi = grid.cell_latitudes()
    assert phi.shape == grid.surface_shape and phi[hy + 11, 0] == 0.0
    R = cm.hemisphere_regions(grid)
    assert R.dtype == np.uint8 and R.shape == grid.surface_shape
    assert (R[hy + 11] == 1).all(), "a cell at exactly φ = 0 is in neither hemisphere"
    assert (R[hy + 12:hy + ny] == 1 + 2).all() and (R[hy:hy + 11] == 1 + 4).all()
    assert (R & 1).all()
    even = cm.hemisphere_regions(cm.LatitudeLongitudeGrid(size=(8, 20, 1), halo=(1, 1, 1)))
    assert set(np.unique(even[1:-1])) == {3, 5}


def test_a_tripolar_grid_brings_its_areas_or_the_presets_raise():
    grid = cm.TripolarGrid(size=(16, 8, 1), halo=(2, 2, 1))
    with pytest.raises(ValueError, match="area"):
        grid.cell_areas()
    Az = np.arange(1.0, 16 * 8 + 1).reshape(8, 16)
    grid = cm.TripolarGrid(size=(16, 8, 1), halo=(2, 2, 1), area=Az)
    A = grid.cell_areas()
    assert A.shape == (12, 20) and np.array_equal(A[2:10, 2:18], Az) and A[:2].sum() == 0 and A[:, :2].sum() == 0
    R = cm.hemisphere_regions(grid)
    phi = grid.mesh()[1]
    assert np.array_equal(R[2:10, 2:18], (1 + 2 * (phi > 0) + 4 * (phi < 0)).astype(np.uint8))
    assert (R[:2] == 1).all(), "a halo cell is in neither hemisphere"


# ---- the writer, on a stand-in context -------------------------------------------------------------------------------------
class _Integrator:
    """cf_integrals_* restated on the CPU: plain numpy sums over the whole array (the stand-in fields have no halos to avoid)"""

    def __init__(self, entries, area=None, mask=None, region=None, capacity=1024, max_workgroups=0):
        self.entries, self.area, self.mask, self.region, self.capacity = entries, area, mask, region, capacity
        self.values, self.time, self.collections, self.resets = [], [], 0, 0

    def collect(self, time=0.0):
        assert len(self.values) < self.capacity, "the writer drains a full series before it collects"
        A = self.area.numpy()
        wet = np.ones(A.shape, bool) if self.mask is None else self.mask.numpy() != 0
        reg = np.ones(A.shape, np.uint8) if self.region is None else self.region.numpy()
        rec = []
        for kind, a, b, thr, bit in self.entries:
            x = dict(one=lambda: np.ones_like(A), field=lambda: a.numpy(), product=lambda: a.numpy() * b.numpy(),
                     above=lambda: (a.numpy() > thr) * 1.0)[kind]()
            rec.append(float((A * x)[wet & ((reg >> bit) & 1 != 0)].sum()))
        self.values.append(rec)
        self.time.append(time)
        self.collections += 1

    def count(self):
        return len(self.values)

    def read(self, first=0, n=None):
        n = len(self.values) - first if n is None else n
        return np.array(self.values[first:first + n]).reshape(n, len(self.entries)), np.array(self.time[first:first + n])

    def reset(self):
        self.values, self.time, self.resets = [], [], self.resets + 1

    def close(self):
        pass


def _fake_model(nx=6, ny=4, sea_ice=True):
    shape = (ny, nx)
    f = lambda v=0.0: torch.full(shape, float(v), dtype=torch.float64)  # noqa: E731
    ctx = SimpleNamespace(integrals=_Integrator, to_device=lambda a: torch.as_tensor(np.ascontiguousarray(a)),
                          params=SimpleNamespace(mask_kind=abi.MASK_U8), discard_prefetched_atmosphere_state=lambda: None, sync=lambda: None)
    net = {k: f() for k in ("u", "v", "T", "S")}
    ao = {k: f() for k in ("sensible_heat", "latent_heat")}
    itf = SimpleNamespace(context=ctx, net_fluxes=SimpleNamespace(_ocean_fields=net), atmosphere_ocean_interface=SimpleNamespace(_fields=ao),
                          _exchange_current=0)
    phi = np.broadcast_to(np.linspace(-30, 30, ny)[:, None], shape)
    grid = SimpleNamespace(size=(nx, ny, 1), halo=(0, 0, 0), cell_areas=lambda: np.full(shape, 2.0), cell_latitudes=lambda: phi)
    wet = torch.ones(shape, dtype=torch.uint8)
    wet[0, 0] = 0
    state = dict(T=f(10.0), S=f(35.0))
    ocean = SimpleNamespace(grid=grid, model=SimpleNamespace(wet_mask=wet), surface_state=lambda: state)
    ice = SimpleNamespace(thickness=f(2.0), concentration=f(0.5)) if sea_ice else None
    return SimpleNamespace(interfaces=itf, ocean=ocean, sea_ice=ice, clock=SimpleNamespace(time=0.0, iteration=0)), net, ao


def _stepper(net, ao):
    def fake_step(m, dt):           # every flux field takes the value of the step's iteration
        m.clock.time += dt
        m.clock.iteration += 1
        for t in list(net.values()) + list(ao.values()):
            t.fill_(float(m.clock.iteration))
    return fake_step


def test_the_writer_collects_on_its_iteration_interval_and_drains_a_full_series(monkeypatch):
    model, net, ao = _fake_model()
    monkeypatch.setattr(cm, "time_step", _stepper(net, ao))
    every = cm.surface_global_means(model)
    third = cm.SurfaceIntegrals(model, dict(total=("field", net["T"]), north=("field", net["T"], None, 0.0, 1), cells=("one",),
                                            hot=("above", net["T"], None, 6.0), sq=("product", net["T"], net["T"]),
                                            mean_north=("mean", net["S"], None, 0.0, 1)),
                                schedule=cm.IterationInterval(3), regions=cm.hemisphere_regions(model.ocean.grid), capacity=2)
    assert [e[0] for e in every.entries] == ["one"] + ["field"] * 6 and every.integrator.mask is model.ocean.model.wet_mask
    assert [e[0] for e in third.entries] == ["field", "field", "one", "above", "product", "one", "field"]
    cm.run(cm.Simulation(model, dt=10.0, stop_iteration=10, output_writers=dict(every=every, third=third)))
    assert list(every.times) == [10.0 * k for k in range(1, 11)] and every.integrator.collections == 10
    assert list(third.times) == [30.0, 60.0, 90.0] and third.integrator.collections == 3 and third.integrator.resets >= 1
    s = every.series()
    assert list(s) == ["hfds", "wfo", "hfss", "hfls", "tos", "sos"]
    assert np.array_equal(s["hfds"], np.arange(1.0, 11.0)) and np.array_equal(s["tos"], np.full(10, 10.0))
    t = third.series()
    wet_cells, north_cells = 6 * 4 - 1, 6 * 2
    assert np.array_equal(t["cells"], np.full(3, 2.0 * wet_cells))
    assert np.array_equal(t["total"], 2.0 * wet_cells * np.array([3.0, 6.0, 9.0]))
    assert np.array_equal(t["north"], 2.0 * north_cells * np.array([3.0, 6.0, 9.0]))
    assert np.array_equal(t["hot"], 2.0 * wet_cells * np.array([0.0, 0.0, 1.0])), "6 > 6 is false: strict"
    assert np.array_equal(t["sq"], 2.0 * wet_cells * np.array([9.0, 36.0, 81.0]))
    assert np.array_equal(t["mean_north"], np.array([3.0, 6.0, 9.0]))
    # a second run! goes on with the same series
    sim = cm.Simulation(model, dt=10.0, stop_iteration=12, output_writers=dict(third=third))
    cm.run(sim)
    assert list(third.times) == [30.0, 60.0, 90.0, 120.0]
    assert cm.SurfaceIntegrals(model, dict(x=("one",)), schedule=4).schedule.interval == 4
    for bad in (0, 2.5, -1):
        with pytest.raises(ValueError, match="IterationInterval"):
            cm.IterationInterval(bad)


def test_the_sea_ice_preset_names_the_reference_diagnostics(monkeypatch):
    model, net, ao = _fake_model()
    monkeypatch.setattr(cm, "time_step", _stepper(net, ao))
    w = cm.sea_ice_integrals(model)
    si = model.sea_ice
    assert [(e[0], e[3], e[4]) for e in w.entries] == [("product", 0.0, 1), ("field", 0.0, 1), ("above", 0.15, 1),
                                                        ("product", 0.0, 2), ("field", 0.0, 2), ("above", 0.15, 2)]
    assert all(e[1] is (si.thickness if e[0] == "product" else si.concentration) for e in w.entries)
    assert w.entries[0][2] is si.concentration
    assert np.array_equal(w.regions.numpy(), cm.hemisphere_regions(model.ocean.grid))
    si.concentration[:2] = 0.15          # the southern rows sit at the threshold exactly: no extent
    cm.run(cm.Simulation(model, dt=1.0, stop_iteration=2, output_writers=dict(ice=w)))
    s = w.series()
    assert list(s) == ["arctic_volume", "arctic_area", "arctic_extent", "antarctic_volume", "antarctic_area", "antarctic_extent"]
    assert np.array_equal(s["arctic_volume"], np.full(2, 2.0 * 12 * 2.0 * 0.5)) and np.array_equal(s["arctic_extent"], np.full(2, 24.0))
    assert np.array_equal(s["antarctic_extent"], np.zeros(2)) and np.allclose(s["antarctic_area"], 2.0 * 11 * 0.15, rtol=1e-15)
    ocean_only, _, _ = _fake_model(sea_ice=False)
    with pytest.raises(ValueError, match="no sea ice"):
        cm.sea_ice_integrals(ocean_only)


# ---- header, abi.py and the Julia stub ---------------------------------------------------------------------------------------
def test_the_three_copies_of_the_abi_list_the_new_names():
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    declared = set(re.findall(r"\b(cf_\w+)\s*\(", code))
    called = set(re.findall(r"\(:(cf_\w+), libcoflux\)", STUB))
    for name in NEW_SYMBOLS:
        assert name in declared and name in abi.EXPORTED_SYMBOLS and name in called, name
    assert re.search(r"#define CF_ABI_VERSION 5\b", HEADER) and abi.ABI_VERSION == 5
    for macro, value in (("CF_INTEGRALS_MAX_ENTRIES", abi.INTEGRALS_MAX_ENTRIES), ("CF_INTEGRALS_MAX_FIELDS", abi.INTEGRALS_MAX_FIELDS),
                         ("CF_INTEGRAND_ONE", abi.INTEGRAND_ONE), ("CF_INTEGRAND_FIELD", abi.INTEGRAND_FIELD),
                         ("CF_INTEGRAND_PRODUCT", abi.INTEGRAND_PRODUCT), ("CF_INTEGRAND_ABOVE", abi.INTEGRAND_ABOVE)):
        assert re.search(rf"#define {macro} {value}\b", HEADER), macro
        if macro.startswith("CF_INTEGRAND"):
            assert re.search(rf"\b{macro}\b[^\n]*Int32\(", STUB), macro
    for doc in ("INTEGRATION.md", "DESIGN.md"):
        text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), doc)).read()
        for name in NEW_SYMBOLS:
            assert name in text, (doc, name)


def test_the_julia_twins_of_the_new_structs_have_the_ctypes_layout():
    structs = julia_structs()
    for name, twin in (("CfIntegralEntry", abi.IntegralEntry), ("CfIntegralsDesc", abi.IntegralsDesc)):
        assert name in structs, f"{name} missing from the stub"
        assert struct_size(name, structs)[0] == C.sizeof(twin), (name, struct_size(name, structs)[0], C.sizeof(twin))
        assert [f for f, _t in structs[name]] == [f for f, *_ in twin._fields_], name
    # the header's structs, field by field in the same order
    for struct, twin in (("cf_integral_entry", abi.IntegralEntry), ("cf_integrals_desc", abi.IntegralsDesc)):
        body = re.search(rf"typedef struct {struct} \{{(.*?)\}} {struct};", HEADER, re.S).group(1)
        fields = re.findall(r"(\w+)(?:\[\w+\])?;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
        assert fields == [f for f, *_ in twin._fields_], struct
    assert C.sizeof(abi.IntegralEntry) == 32 and C.sizeof(abi.IntegralsDesc) == 40 + 32 * abi.INTEGRALS_MAX_ENTRIES
