"""CPU checks of the coupled step loop's interface (cf_prepare_coupled_step, cf_time_steps_coupled): the header, abi.py and the
Julia stub agree on the two new structs, both symbols are exported, the ABI version stands, the header states a footprint for
both entry points — and the designed case of tests/coupled_case.py is what its description says (NumPy counts)."""
import ctypes as C
import re

import numpy as np
import pytest

import coupled_case as cc
import test_julia_stub as tj
from coflux import abi

NEW_STRUCTS = {"cf_coupled_prepare": ("CfCoupledPrepare", abi.CoupledPrepare), "cf_coupled_step": ("CfCoupledStep", abi.CoupledStep)}
C_SIZES = {"int32_t": 4, "double": 8, "cf_ocean_surface": C.sizeof(abi.OceanSurface), "cf_interp_weights": C.sizeof(abi.InterpWeights),
           "cf_land_source": C.sizeof(abi.LandSource), "cf_ice_ocean_params": C.sizeof(abi.IceOceanParams),
           "cf_ice_ocean_fluxes": C.sizeof(abi.IceOceanFluxes), "cf_interface_fluxes": C.sizeof(abi.InterfaceFluxes),
           "cf_net_sea_ice_fluxes": C.sizeof(abi.NetSeaIceFluxes)}


def header_struct(name):
    """[(field, C type)] of `typedef struct name { … } name;` in include/coflux.h, comments removed."""
    m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), tj.HEADER, re.S)
    assert m, name
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        mm = re.match(r"(.*?)(\w+)$", decl, re.S)
        out.append((mm.group(2), mm.group(1).strip()))
    return out


@pytest.mark.parametrize("cname", sorted(NEW_STRUCTS))
def test_header_abi_and_julia_stub_agree_on_the_new_structs(cname):
    jname, twin = NEW_STRUCTS[cname]
    structs = tj.julia_structs()
    assert jname in structs, f"{jname} missing from the stub"
    names = [f for f, *_ in twin._fields_]
    assert [f for f, _t in structs[jname]] == names
    assert tj.struct_size(jname, structs)[0] == C.sizeof(twin)
    fields = header_struct(cname)
    assert [f for f, _t in fields] == names
    # the header's layout, computed with natural alignment from its own declarations, is the ctypes twin's
    off = 0
    for (fname, ctype), (_n, ct) in zip(fields, twin._fields_):
        size = 8 if "*" in ctype else C_SIZES[ctype]
        align = 4 if ctype == "int32_t" else 8
        off = (off + align - 1) // align * align
        assert off == getattr(twin, fname).offset, (cname, fname, off, getattr(twin, fname).offset)
        assert size == C.sizeof(ct), (cname, fname)
        off += size
    assert (off + 7) // 8 * 8 == C.sizeof(twin)
    # the embedded structs of the stub are value types: a mutable struct would be a reference as a field
    for _f, t in structs[jname]:
        if t.startswith("Cf"):
            assert not re.search(r"^mutable struct %s\b" % t, tj.STUB, re.M), t


def test_both_entry_points_are_exported_bound_and_the_abi_version_stands():
    lib = abi.load_library()
    for name in ("cf_prepare_coupled_step", "cf_time_steps_coupled"):
        assert name in abi.EXPORTED_SYMBOLS and hasattr(lib, name), name
        assert re.search(r"\(:%s, libcoflux\)" % name, tj.STUB), name
        assert getattr(lib, name).restype is C.c_int
    assert abi.ABI_VERSION == 5 and lib.cf_version() == 5
    assert re.search(r"#define CF_ABI_VERSION 5\b", tj.HEADER)


def test_the_header_states_a_footprint_for_both_entry_points():
    for name in ("cf_prepare_coupled_step", "cf_time_steps_coupled"):
        at = tj.HEADER.index("int %s(" % name)
        before = tj.HEADER[:at]
        comment = before[before.rindex("/*"):]
        assert comment.lstrip("/* ").startswith("Footprint"), (name, comment[:80])
        assert before.rstrip().endswith("*/"), name     # the comment sits right above the declaration


SHAPES = [(70, 23, 3, 2), (64, 2, 2, 2), (131, 37, 4, 3), (257, 5, 2, 3), (192, 48, 4, 4)]


@pytest.mark.parametrize("nx, ny, hx, hy", SHAPES)
def test_the_case_qualifies(nx, ny, hx, hy):
    """At least 8 cells of every class, an aligned run of 64 interior cells with at least four classes, stresses that are
    non-zero in the east halo column and the north halo row, a land source that is non-zero on coastal nodes, and second and
    third ice states that differ in ℵ on the planted cells."""
    case = cc.build(nx, ny, hx, hy)
    for state, ice in ((0, 0), (1, 1), (0, 2)):
        counts, best = cc.census(case, state, ice)
        for k in cc.CLASSES:
            assert counts[k] >= 8, (state, ice, k, counts)
        assert best >= 4, (state, ice, best)
    east = (slice(hy, hy + ny), hx + nx)
    north = (hy + ny, slice(hx, hx + nx))
    for k in ("x_stress", "y_stress"):
        assert np.all(case[k][east] != 0.0) and np.all(case[k][north] != 0.0), k
    inner = (slice(hy, hy + ny), slice(hx, hx + nx))
    planted = np.zeros((ny, nx), bool).reshape(-1)
    for r in cc.planted_runs(nx, ny):
        planted[64 * r:64 * r + 64] = True
    planted = planted.reshape(ny, nx)
    c0, c1, c2 = (c[inner] for c in case["concentrations"])
    assert (c1[planted] != c0[planted]).any() and (c2[planted] != c1[planted]).any() and (c2[planted] != c0[planted]).any()
    # coastal cells draw from non-zero source nodes at every level
    w = case["weights"]
    assert (w["fi"] < 0).any()
    fi = np.broadcast_to(w["fi"][None, :], case["coast"].shape)[case["coast"]]
    fj = np.broadcast_to(w["fj"][:, None], case["coast"].shape)[case["coast"]]
    nsy, nsx = case["land"]["friver"].shape[1:]
    assert case["coast"][inner].sum() >= 8
    for n in range(cc.LAND_CLOCK["n_levels"]):
        assert np.all(case["land"]["friver"][n, np.clip(np.trunc(fj).astype(int), 0, nsy - 1), np.trunc(fi).astype(int) % nsx] > 0)


def test_the_two_clocks_cross_level_boundaries_at_different_steps():
    land, atmos = cc.crossings(cc.LAND_CLOCK), cc.crossings(cc.ATMOS_CLOCK)
    assert land and atmos and not set(land) & set(atmos), (land, atmos)
    assert all(0 < s < cc.N_STEPS for s in land + atmos)
    # … and the 5 + 7 split separates them: a crossing on either side of the call boundary
    assert any(s < 5 for s in land + atmos) and any(s >= 5 for s in land + atmos)


def test_models_clock_rebasing_reproduces_the_host_clock():
    """models.time_steps holds the device loop's clock (fraction + step · increment) to time_step!'s (t / Δt_snapshot): the
    pair device_clock returns gives exactly the wanted level and fraction at its step, for a Δt that is no binary fraction of
    the snapshot interval, from any starting iteration."""
    from coflux import clocks
    dt, interval, n = 1200.0, 10800.0, 7
    inc = dt / interval
    for first in (0, 5, 1000, 26279):
        t = first * dt
        for s in range(first, first + 40):
            t += dt
            x = t / interval
            base = int(np.floor(x))
            want = (base % n, (base + 1) % n, x - base)
            c = clocks.device_clock(want[0], want[2], n, s, inc)
            assert c is not None, (first, s)
            assert clocks.clock_at(c[0], c[1], n, s, inc) == want, (first, s)
