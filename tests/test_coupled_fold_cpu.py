"""CPU tests of the coupled loop's fold plan (coflux/distributed.py: coupled_fold_plan — the host statement of which fields
cf_time_steps_coupled exchanges under CF_HALO_PEER, in which exchanges, and how the tripolar fold maps each on the last rank;
include/coflux.h: "Tripolar slabs"), and of the one convention in it the ocean does not already state: ice velocities at cell
centres fold with sign −1."""
import itertools
import re

import numpy as np

import test_julia_stub as tj
from coflux import abi
from coflux import synthetic as syn
from coflux.distributed import MAX_EXCHANGE_FIELDS, coupled_fold_plan
from coflux.runtime import FluxContext

OCEAN = ("T", "S", "u", "v")
# the order of include/coflux.h; the names of cf_sea_ice_state (its velocities appear in the plan as ice_u, ice_v)
ICE_ORDER = ("concentration", "thickness", "snow_thickness", "u", "v", "albedo")
CALL_ORDER = ("x_stress", "y_stress", "skin_temperature")
NX, NY, H = 360, 180, 5


def test_the_counter_is_declared_exported_and_bound():
    lib = abi.load_library()
    assert "cf_debug_fold_counts" in abi.EXPORTED_SYMBOLS and hasattr(lib, "cf_debug_fold_counts")
    assert re.search(r"int cf_debug_fold_counts\(cf_ctx\* ctx, long long\* fold_launches, long long\* exchanges_with_fold\);", tj.HEADER)
    assert "(:cf_debug_fold_counts, libcoflux)" in tj.STUB and callable(FluxContext.fold_counts)
    assert lib.cf_version() == abi.ABI_VERSION == 5           # additive: no version bump came with it


def test_the_header_states_the_order_the_plan_follows():
    text = re.sub(r"\s*\n \*\s*", " ", tj.HEADER)
    assert "in the order concentration, thickness, snow_thickness, u, v, albedo" in text
    assert "the non-NULL ones of ice->x_stress, ice->y_stress, and skin_temperature" in text
    assert "exchanges of at most 8 fields" in text and MAX_EXCHANGE_FIELDS == 8


def test_the_plan_follows_the_cut_rule_for_every_combination_of_optional_fields():
    """snow, either ice velocity, the albedo and either stress present or not: at most eight fields per exchange, filled in the
    header's order with none left out and none invented; the ocean's conventions are synthetic's; every scalar is (centre, +1),
    every vector component −1, the ice velocities at centres and the stresses on the faces of the ocean velocities."""
    for snow, iu, iv, albedo, tx, ty in itertools.product((False, True), repeat=6):
        ice = [k for k, on in zip(ICE_ORDER, (True, True, snow, iu, iv, albedo)) if on]
        call = [k for k, on in zip(CALL_ORDER, (tx, ty, True)) if on]
        per_call, per_step = coupled_fold_plan(OCEAN, ice, call)
        want_step = list(OCEAN) + [("ice_" + k if k in ("u", "v") else k) for k in ice]
        for exchanges, want in ((per_step, want_step), (per_call, call)):
            assert all(1 <= len(e) <= MAX_EXCHANGE_FIELDS for e in exchanges)
            assert all(len(e) == MAX_EXCHANGE_FIELDS for e in exchanges[:-1])            # cut only where an exchange is full
            assert [name for e in exchanges for name, _l, _s in e] == want
            assert len(exchanges) == -(-len(want) // MAX_EXCHANGE_FIELDS)
        assert len(per_call) == 1 and len(per_step) == (1 if len(want_step) <= 8 else 2)
        triples = {name: (loc, sign) for e in per_call + per_step for name, loc, sign in e}
        for k in OCEAN:
            assert triples[k] == (syn.FOLD_LOCATION[k], syn.FOLD_SIGN[k])
        for name, (loc, sign) in triples.items():
            if name in ("ice_u", "ice_v"):
                assert (loc, sign) == ("center", -1.0)
            elif name in ("x_stress", "y_stress"):
                assert (loc, sign) == triples["u" if name == "x_stress" else "v"]
            elif name not in ("u", "v"):
                assert (loc, sign) == ("center", 1.0), name
    # the defaults: what cf_time_steps_coupled requires (ℵ, hᵢ, the skin temperature) beside the ocean
    per_call, per_step = coupled_fold_plan()
    assert [[n for n, *_ in e] for e in per_step] == [["T", "S", "u", "v", "concentration", "thickness"]]
    assert [[n for n, *_ in e] for e in per_call] == [["skin_temperature"]]


def test_ice_velocities_at_cell_centres_fold_with_sign_minus_one():
    """On synthetic's tripolar mesh a geographic vector field rotated into the grid frame at the cell centres — the halo cells
    beyond the fold included, whose i-axis is the mirror cell's reversed — equals the plan's fold of the grid-frame field:
    both components at centres with sign −1, as tests/test_tripolar.py shows for the ocean's conventions."""
    per_call, per_step = coupled_fold_plan(OCEAN, ICE_ORDER, CALL_ORDER)
    triples = {name: (loc, sign) for e in per_call + per_step for name, loc, sign in e}
    case = syn.tripolar_case(NX, NY, H, H)
    w = case["weights"]
    lam = np.deg2rad(w["fi"] * (360.0 / syn.JRA55_NX))
    phi = np.deg2rad(w["latitude"])
    uE, vN = np.cos(phi) * np.sin(2 * lam), 0.3 * np.sin(phi) + np.cos(lam)           # smooth geographic (E, N) components
    ug, vg = uE * w["cos_rot"] + vN * w["sin_rot"], -uE * w["sin_rot"] + vN * w["cos_rot"]
    assert np.abs(ug[H + NY:H + NY + 2]).max() > 0.1 and np.abs(vg[H + NY:H + NY + 2]).max() > 0.1
    for name, a in (("ice_u", ug), ("ice_v", vg)):
        location, sign = triples[name]
        folded = a.copy()
        folded[H + NY:] = np.nan
        syn.fold_north(folded, NX, NY, H, H, 2, location, sign)
        np.testing.assert_allclose(folded[H + NY:H + NY + 2], a[H + NY:H + NY + 2], atol=1e-12, err_msg=name)
        wrong = a.copy()
        syn.fold_north(wrong, NX, NY, H, H, 2, location, -sign)                         # (the other sign is off by twice the field)
        assert np.abs(wrong[H + NY:H + NY + 2] - a[H + NY:H + NY + 2]).max() > 0.1, name
