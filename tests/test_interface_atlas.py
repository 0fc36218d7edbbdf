"""The atmosphere–sea-ice interface solve (ice_iterate, ice_iterate_lean and the three launches that carry them) on a designed
atlas of ice regimes (tests/interface_atlas.py), held to the reference per entry and to ITSELF by bits.

Before this file the interface solve met one smooth polar state, on which a cell's wave-mates are near copies of it and half
the cells orbit, so that util.compare_ice_fluxes has to accept them as a distribution.  Here every entry is compared on its
own, in a class the reference alone assigns per (preset, scheme):
    fast       ≤ 40 trips, u★ ≥ 1e-8       all nine fields within TOL_ICE = 1e-9 (sea_ice_fixed5: 1e-8), identical trip counts
    slow       41 … 99 trips               1e-6 (sea_ice_ncar under the linearised scheme: 1e-5), identical trip counts
    cap        the reference gave up        finite, and at the cap on the device too
    collapsed  u★ < 1e-8                   1e-6, trip counts within ±1
and every entry of every class — orbits and collapsed cells amplify anything — must give the same BITS in every copy, layout,
mask, call, launch and option that claims not to change the arithmetic.

CPU part (no marker): the entries have the property they are named for (read off the instrumented NumPy restatement,
tests/skin_linearised_reference.py), the layouts have the copies and lanes they promise, the two CPU restatements qualify
each other (C oracle and numpy_oracle.atmosphere_sea_ice_fluxes: identical trip counts, TOL_REFERENCE on fast and slow
entries; the explicit and semi-implicit schemes only — the linearised scheme has ONE restatement, skin_linearised_reference,
which is held to the C oracle on the other two schemes instead), the class tables, the conditions on them, and seeded
defects that the atlas sees and the smooth polar state does not.

Measured on the CPU: trip counts of the C and NumPy restatements differ in 0 entries in all ten (preset, scheme) runs; worst
scaled difference on fast and slow entries 1.75e-13 (sea_ice_fixed5, semi-implicit, latent_heat, wind[-x]).

Non-finite entries.  C's and the kernels' fmin / fmax drop a NaN operand where NumPy's minimum / maximum hand it on, so the
reference for them is the C oracle (the linearised restatement calls fmin / fmax in the same places and agrees with it on
NaN thickness, skin and shortwave).  A NaN humidity is clamped to 0 by the C oracle's phase partition; a NaN or infinite air
temperature leaves u★ finite there (fmax against the profile floor) and the skin at its carried value (the NaN guard).

GPU part: see the docstrings below; DEVICE_KNOWN lists what the device is known to miss, each with its cause."""
import functools

import numpy as np
import pytest

import interface_atlas as ia
import numpy_oracle as npo
import oracle as orc
import regime_atlas as ra
import skin_linearised_reference as slr
import util
from coflux import abi
from coflux import interface_computations as ic
from coflux.runtime import EXCHANGE_NAMES, FLUX_NAMES, FLUX_OPTIONAL, NET_NAMES

gpu = pytest.mark.gpu

H, RING = ia.HALO, ia.RING
TOL_REFERENCE = 1e-12     # what test_oracle.py holds the two restatements to
TOL_ICE = 1e-9            # test_gpu_parity.TOL_ICE
CELL_FIELDS = FLUX_NAMES + FLUX_OPTIONAL
ALL = CELL_FIELDS + ("iterations",)
SCHEMES = {"explicit": abi.SKIN_EXPLICIT, "semi_implicit": abi.SKIN_SEMI_IMPLICIT, "linearised": abi.SKIN_LINEARISED}
CLASSES = ("fast", "slow", "cap", "collapsed")
SLOW = 40


def _corrected_log():
    """sea_ice_corrected with the plain logarithmic profile: constant roughness lengths keep it on the lean body, whose
    non-COARE instantiation no preset reaches."""
    fluxes = ic.corrected_atmosphere_sea_ice_fluxes()
    fluxes.similarity_form = ic.LogarithmicSimilarityProfile()
    return fluxes, ic.RelativeVelocity()


CONFIGS = dict({k: util.ICE_CONFIGS[k] for k in ("sea_ice_corrected", "sea_ice_ncar", "sea_ice_default", "sea_ice_fixed5")},
               sea_ice_corrected_log=_corrected_log)
PRESETS = ("sea_ice_corrected", "sea_ice_ncar", "sea_ice_default", "sea_ice_fixed5")     # the ones the conditions are stated for
RUNS = [(c, s) for c in CONFIGS for s in SCHEMES]


def _formulation(config, maxiter=None):
    fluxes, vd = CONFIGS[config]()
    if maxiter is not None:
        fluxes.solver_stop_criteria = ic.ConvergenceStopCriteria(maxiter=maxiter)
    return fluxes, vd


def _maxiter(config, maxiter=None):
    stop = _formulation(config, maxiter)[0].solver_stop_criteria
    return stop.iterations if isinstance(stop, ic.FixedIterations) else stop.maxiter


def _wind(vd):
    return "wind" if isinstance(vd, ic.WindVelocity) else "relative"


# =============================================================================================
# CPU: the references on the atlas as one row of cells
# =============================================================================================
def _entries(out):
    return {k: v[1, 1:-1] for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def _c_row(config, scheme, maxiter=None):
    fluxes, vd = _formulation(config, maxiter)
    ocean, atmos, ice = ia.row()
    props = ic.SeaIceInterfaceProperties(skin_temperature_scheme=SCHEMES[scheme])
    return _entries(orc.compute_atmosphere_sea_ice_fluxes(orc.make_grid(ia.A, 1, 1, 1, 0), ic.flux_params(fluxes, velocity_difference=vd),
                                                          props.to_params(), ice, ocean, atmos))


@functools.lru_cache(maxsize=None)
def _np_row(config, scheme):
    fluxes, vd = _formulation(config)
    ocean, atmos, ice = ia.row()
    with np.errstate(all="ignore"):
        return _entries(npo.atmosphere_sea_ice_fluxes(
            fluxes, ic.SeaIceInterfaceProperties(skin_temperature_scheme=SCHEMES[scheme]), ice, ocean, atmos, hx=1, hy=1, ring=0,
            thermodynamics=ic.AtmosphereThermodynamicsParameters(), ocean_properties=ic.OceanProperties(),
            velocity_difference=_wind(vd)))


def _restated(config, scheme, state=None, maxiter=None, hx=1, hy=1, ring=0, **kw):
    """tests/skin_linearised_reference.py on the row (or on `state`); kw: trace, defect, orbit_shortcut."""
    fluxes, vd = _formulation(config, maxiter)
    ocean, atmos, ice = ia.row() if state is None else state
    with np.errstate(all="ignore"):
        out = slr.interface_fluxes(fluxes, ic.SeaIceInterfaceProperties(skin_temperature_scheme=SCHEMES[scheme]), ice, ocean, atmos,
                                   hx=hx, hy=hy, ring=ring, scheme=SCHEMES[scheme], velocity_difference=_wind(vd),
                                   thermodynamics=ic.AtmosphereThermodynamicsParameters(), **kw)
    return _entries(out) if state is None else out


@functools.lru_cache(maxsize=None)
def _restated_row(config, scheme, maxiter=None):
    trace = {}
    out = _restated(config, scheme, maxiter=maxiter, trace=trace)
    return out, {k: v[0] for k, v in trace.items()}


@functools.lru_cache(maxsize=None)
def _clamped_row(config, scheme, maxiter=None):
    """The linearised restatement with the C oracle's reading of a NaN humidity (clamped to 0)."""
    ocean, atmos, ice = ia.row()
    atmos = dict(atmos, q=np.where(np.isnan(atmos["q"]), 0.0, atmos["q"]))
    return _entries(_restated(config, scheme, (ocean, atmos, ice), maxiter))


def _reference(config, scheme, maxiter=None):
    """What the device is held to: the C oracle (explicit, semi-implicit); the restatement (linearised), with the C oracle's
    explicit-scheme NaN pattern on the entries whose air temperature is not finite (see the module docstring)."""
    if scheme != "linearised":
        return _c_row(config, scheme, maxiter)
    ref = {k: v.copy() for k, v in _clamped_row(config, scheme, maxiter).items()}
    c = _c_row(config, "explicit", maxiter)
    for name in ("nan_T", "inf_T"):       # (in no class: held to the NaN pattern and the carried skin, not to these values)
        i = ia.INDEX[name]
        for k in ALL:
            ref[k][i] = c[k][i]
    return ref


@functools.lru_cache(maxsize=None)
def _classes(config, scheme, maxiter=None):
    """dict class → bool [A], by the reference alone; non-finite entries are in no class."""
    ref = _reference(config, scheme, maxiter)
    its, us = ref["iterations"], ref["friction_velocity"]
    fixed = isinstance(_formulation(config)[0].solver_stop_criteria, ic.FixedIterations)
    cap = ia.FINITE & (not fixed) & (its >= _maxiter(config, maxiter))
    with np.errstate(invalid="ignore"):
        collapsed = ia.FINITE & ~cap & (us < 1e-8)
    slow = ia.FINITE & ~cap & ~collapsed & (its > SLOW)
    return dict(fast=ia.FINITE & ~cap & ~collapsed & ~slow, slow=slow, cap=cap, collapsed=collapsed)


def _scaled_error(got, ref, fields=util.ICE_FLUX_FIELDS):
    """Per entry, the largest |Δ| / max(|ref|, field scale) over the nine fields; a NaN on one side only is inf."""
    worst = np.zeros(np.shape(ref["sensible_heat"]))
    for k in fields:
        with np.errstate(invalid="ignore"):
            e = np.abs(got[k] - ref[k]) / np.maximum(np.abs(ref[k]), util.FIELD_SCALE[k])
        e = np.where(np.isnan(got[k]) & np.isnan(ref[k]), 0.0, np.where(np.isnan(e), np.inf, e))
        worst = np.maximum(worst, e)
    return worst


def _at(arr, name):
    return arr[ia.INDEX[name]]


ZETA_EDGE = (2.0 ** 34 - 1.0) / 16.0      # coflux_tables.h: ψ is tabulated against x = 1 + 16 |ζ| < 2^34; beyond, closed forms


def _zeta(config, scheme):
    """ζ = h κ b★ / u★² at the reference's answer, per entry (b★ from the answer's scales: g (θ★ / Tₛ + δ q★))."""
    ref = _reference(config, scheme)
    th = npo.Thermo(ic.AtmosphereThermodynamicsParameters())
    with np.errstate(all="ignore"):
        b = 9.81 * (ref["temperature_scale"] / (ref["temperature"] + 273.15) + (th.eps - 1.0) * ref["humidity_scale"])
        return 10.0 * 0.4 * b / ref["friction_velocity"] ** 2


# ---------------------------------------------------------------------------------------------
# the atlas and its layouts
# ---------------------------------------------------------------------------------------------
def test_the_atlas_is_what_the_layouts_need():
    assert ia.A == 1183 and np.gcd(ia.A, 64) == 1 and len(set(ia.NAMES)) == ia.A and len(ia.GRID) == 1152
    assert {k: len(v) for k, v in ia.EDGE_FAMILIES.items()} == {"limiter[": 3, "cap[": 4, "h[": 6, "drift[": 1, "wind[": 4,
                                                                "albedo[": 2, "neutral": 1, "open[": 4, "nonfinite": 6}
    assert len(ia.GRID) + sum(len(v) for v in ia.EDGE_FAMILIES.values()) == ia.A          # (no pad entry was needed)
    assert {k: len(v) for k, v in ia.GROUPS.items()} == {"U=0": 192, "U=30": 192, "Ta=235": 288, "Ta=280": 288, "h=0": 288,
                                                         "h=0.02": 288, "h=3": 288, "Ts=-40": 384, "Ts=0": 384, "sunlit": 576, "dark": 576}
    cols = ia.table()
    for f in ia.FIELDS:
        bad = ~np.isfinite(cols[f])
        assert [ia.NAMES[i] for i in np.flatnonzero(bad)] == [n for n in ia.NONFINITE if n.split("_")[1] == f], f
    assert np.all(np.isfinite(np.stack([ia.table(nonfinite=False)[f] for f in ia.FIELDS])))
    grid = np.array([n in ia.GRID for n in ia.NAMES])
    assert np.all(cols["conc"][grid] == 0.9) and not cols["ui"][grid].any() and not cols["vi"][grid].any()
    for i in np.flatnonzero(~ia.FINITE):                                     # each non-finite entry sits between finite ones
        assert ia.FINITE[i - 1] and ia.FINITE[i + 1]
    nx, ny, ids = ia.layout("cyclic")
    assert (nx, ny) == (131, 37) and ids.shape == (39, 133) and np.array_equal(ids.reshape(-1), np.arange(5187) % ia.A)
    assert np.bincount(ids.reshape(-1), minlength=ia.A).min() == 4           # four or five copies of every entry …
    for e in (0, 700, ia.A - 1):
        lanes = np.flatnonzero(ids.reshape(-1) == e) % 64
        assert len(set(lanes.tolist())) == lanes.size                        # … each in another lane
    nx, ny, ids = ia.layout("blocks")
    flat = ids.reshape(-1)
    assert flat.size >= 64 * ia.A and flat.size - 64 * ia.A < ids.shape[1] and flat.size <= 90000
    assert np.array_equal(flat[:64 * ia.A].reshape(ia.A, 64), np.repeat(np.arange(ia.A)[:, None], 64, axis=1))
    for kind in ("cyclic", "blocks"):                                        # the land variant leaves every entry a wet copy
        wet, mask = ia.land_mask(kind)
        _, _, ids = ia.layout(kind)
        assert 0.45 < wet.mean() < 0.55 and mask.dtype == np.uint8
        assert np.bincount(ids[wet], minlength=ia.A).min() >= 1
        order, starts = ia.copies(ids, wet)
        assert np.array_equal(ids.reshape(-1)[order[starts]], np.arange(ia.A))
    nx, ny, ids, ocean, atmos, ice = ia.fields("cyclic")
    assert atmos["T"].shape == (37 + 2 * H, 131 + 2 * H) and not ocean["u"].any() and "mask" not in ocean
    W = lambda a: util.window(a, H, H, nx, ny, RING)   # noqa: E731
    assert np.array_equal(W(ice["thickness"]), cols["h"][ids], equal_nan=True) and np.array_equal(W(atmos["Qs"]), cols["Qs"][ids], equal_nan=True)
    # the regime atlas' own layouts did not move
    assert ra.layout("cyclic")[2].max() == ra.A - 1 and ra.layout("blocks")[2].max() == ra.A - 1


def test_entries_have_the_property_they_are_named_for():
    """Read off the instrumented restatement (trace): which branch every named entry takes, per scheme where it matters."""
    cols = ia.table()
    for config in PRESETS:
        fixed = config == "sea_ice_fixed5"
        for scheme in SCHEMES:
            out, tr = _restated_row(config, scheme)
            lab = (config, scheme)
            # the limiter: the first trips pinned
            assert _at(tr["first_limiter_trips"], "limiter[up]") >= 5 and _at(tr["first_step"], "limiter[up]") > ia.DT_MAX, lab
            assert _at(tr["first_limiter_trips"], "limiter[down]") >= 5 and _at(tr["first_step"], "limiter[down]") < -ia.DT_MAX, lab
            # the cap
            assert _at(tr["ends_on_the_cap"], "cap[carried]") and _at(out["temperature"], "cap[carried]") == 0.0, lab
            assert _at(tr["left_the_cap"], "cap[touch_and_leave]") and not _at(tr["ends_on_the_cap"], "cap[touch_and_leave]"), lab
            # thickness: h/k against hk_min, and the values either side
            for name in ia.EDGE_FAMILIES["h["]:
                assert _at(tr["hk_is_minimum"], name) == (name != "h[consolidation+ulp]"), (lab, name)
            assert _at(tr["hk_is_minimum"], "grid[U=8,Ta=262,rh=1,h=0.02,Ts=-1,rad=dark]"), lab
            assert not _at(tr["hk_is_minimum"], "grid[U=8,Ta=262,rh=1,h=0.3,Ts=-1,rad=dark]"), lab
            # calm air: the U = 0 grid entries; ice drifting with the wind under RelativeVelocity only
            relative = _wind(_formulation(config)[1]) == "relative"
            assert np.array_equal(tr["calm"], (cols["u"] - (cols["ui"] if relative else 0) == 0) & (cols["v"] - (cols["vi"] if relative else 0) == 0))
            assert _at(tr["calm"], "drift[with_wind]") == relative and tr["calm"].sum() == 192 + relative, lab
            calm = tr["calm"]
            assert not out["x_momentum"][calm].any() and not out["y_momentum"][calm].any(), lab
            for name in ia.EDGE_FAMILIES["wind["]:
                assert abs(np.hypot(_at(cols["u"], name), _at(cols["v"], name)) - 8.0) < 1e-14, name
                same = abs(np.hypot(_at(out["x_momentum"], name), _at(out["y_momentum"], name)) / _at(out["x_momentum"], "wind[-x]") - 1)
                assert same < (1e-6 if not fixed else 1e-3), (lab, name, same)     # (−x started from another skin bit: converged alike)
            assert _at(out["x_momentum"], "wind[-x]") > 0 and _at(out["y_momentum"], "wind[+y]") < 0 < _at(out["y_momentum"], "wind[-y]"), lab
            # zero buoyancy scale on the second trip, after a first trip pinned at +ΔT_max
            assert _at(tr["zero_buoyancy"], "neutral") and _at(tr["first_step"], "neutral") > ia.DT_MAX and tr["zero_buoyancy"].sum() == 1, lab
            # the NaN guard is taken by the entries whose balance is NaN
            for name in ia.NONFINITE:
                assert _at(tr["nan_guard"], name) == (name != "nan_h"), (lab, name)     # (fmax drops a NaN thickness: thin ice)
            assert not tr["nan_guard"][ia.FINITE].any(), lab
            # the floors are reached somewhere
            assert tr["gust_floor"][ia.FINITE].any(), lab
    assert _restated_row("sea_ice_ncar", "linearised")[1]["profile_floor"][ia.FINITE].sum() >= 100
    # albedo 0 and 1: all and none of the shortwave
    for name, factor in (("albedo[0]", 1.0), ("albedo[1]", 0.0)):
        cell = {f: _at(cols[f], name) for f in ia.FIELDS}
        base = dict(cell, Qs=0.0)
        assert ia.first_explicit_step(cell) - ia.first_explicit_step(base) == pytest.approx(0.15 * factor * 300.0, rel=1e-12), name
    # exactly ΔT_max below its balance (explicit scheme, first trip): not limited, and the next skin below is
    out, tr = _restated_row("sea_ice_corrected", "explicit")
    step = _at(tr["first_step"], "limiter[exact]")
    assert 0 <= ia.DT_MAX - step < 1e-12 and _at(tr["first_limiter_trips"], "limiter[exact]") == 0
    cell = {f: _at(cols[f], "limiter[exact]") for f in ia.FIELDS}
    assert ia.first_explicit_step(cell) == step and ia.first_explicit_step(dict(cell, Ts=np.nextafter(cell["Ts"], -100.0))) > ia.DT_MAX
    # the smallest heating that just fails to reach the cap, and its neighbour that reaches it (sea_ice_corrected, linearised)
    out, tr = _restated_row("sea_ice_corrected", "linearised")
    assert np.nextafter(ia.CAP_MISSED_QS, np.inf) == ia.CAP_REACHED_QS
    assert _at(out["temperature"], "cap[just_reached]") == 0.0 and _at(tr["ends_on_the_cap"], "cap[just_reached]")
    assert -1e-12 < _at(out["temperature"], "cap[just_missed]") < 0.0 and not _at(tr["ends_on_the_cap"], "cap[just_missed]")
    # open water: what CF_ICE_FREE_ZERO skips is ℵ == 0 and h == 0, the sign of the zero regardless
    for name, (conc, h) in ia.OPEN_WATER.items():
        assert (_at(cols["conc"], name) == 0.0 and _at(cols["h"], name) == 0.0) == (name in ia.SKIPPED_WHEN_ICE_FREE)
    assert np.signbit(_at(cols["conc"], "open[conc=-0,h=0]")) and np.signbit(_at(cols["h"], "h[-0]"))


# ---------------------------------------------------------------------------------------------
# qualification by the reference alone
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("scheme", ["explicit", "semi_implicit"])
def test_the_restatements_qualify_each_other(config, scheme):
    """C oracle against numpy_oracle.atmosphere_sea_ice_fluxes: identical trip counts on every finite entry, TOL_REFERENCE
    on fast and slow ones; and the restatement that alone states the linearised scheme, run on this scheme, against the C
    oracle: the same, and the same NaN pattern on the non-finite entries whose air temperature is finite."""
    c, n, (r, _) = _c_row(config, scheme), _np_row(config, scheme), _restated_row(config, scheme)
    cls = _classes(config, scheme)
    held = cls["fast"] | cls["slow"]
    for other, label in ((n, "numpy_oracle"), (r, "skin_linearised_reference")):
        assert np.array_equal(c["iterations"][ia.FINITE], other["iterations"][ia.FINITE]), label
        e = _scaled_error(other, c)
        assert e[held].max() <= TOL_REFERENCE, (label, float(e[held].max()), ia.NAMES[int(np.where(held, e, 0).argmax())])
    for name in ("nan_Qs", "nan_h", "nan_Ts"):
        i = ia.INDEX[name]
        for k in CELL_FIELDS:
            assert np.isnan(c[k][i]) == np.isnan(r[k][i]), (name, k)
        assert c["iterations"][i] == r["iterations"][i], name
    for name in ("nan_T", "inf_T"):                 # the skin stays the carried one, u★ stays finite, the heat fluxes are NaN
        i = ia.INDEX[name]
        assert c["temperature"][i] == -10.0 and np.isfinite(c["friction_velocity"][i]) and np.isnan(c["sensible_heat"][i]), name
    assert np.all(np.isfinite([c[k][ia.INDEX["nan_q"]] for k in CELL_FIELDS]))


# fast, slow, cap, collapsed per (preset, scheme), finite entries; measured on the CPU with the references above
CLASS_COUNTS = {
    ("sea_ice_corrected", "explicit"): (611, 33, 533, 0),
    ("sea_ice_corrected", "semi_implicit"): (637, 25, 515, 0),
    ("sea_ice_corrected", "linearised"): (1135, 42, 0, 0),
    ("sea_ice_ncar", "explicit"): (316, 69, 498, 294),
    ("sea_ice_ncar", "semi_implicit"): (322, 81, 480, 294),
    ("sea_ice_ncar", "linearised"): (847, 12, 18, 300),
    ("sea_ice_default", "explicit"): (628, 17, 532, 0),
    ("sea_ice_default", "semi_implicit"): (657, 18, 502, 0),
    ("sea_ice_default", "linearised"): (1136, 41, 0, 0),
    ("sea_ice_fixed5", "explicit"): (1177, 0, 0, 0),
    ("sea_ice_fixed5", "semi_implicit"): (1177, 0, 0, 0),
    ("sea_ice_fixed5", "linearised"): (1177, 0, 0, 0),
    ("sea_ice_corrected_log", "explicit"): (611, 33, 533, 0),
    ("sea_ice_corrected_log", "semi_implicit"): (637, 25, 515, 0),
    ("sea_ice_corrected_log", "linearised"): (1135, 42, 0, 0),
}


def test_class_tables():
    """The class of every entry per run, so that a change to the atlas or to a reference shows."""
    got = {(c, s): tuple(int(_classes(c, s)[k].sum()) for k in CLASSES) for c, s in RUNS}
    assert got == CLASS_COUNTS, got
    for counts in got.values():
        assert sum(counts) == ia.A - len(ia.NONFINITE)


def test_conditions_on_the_classes():
    """By the reference alone: every run keeps ≥ 25 % of the entries fast, every named group ≥ 20 fast entries in every run,
    and every finite edge entry is fast in at least one preset under the linearised scheme."""
    smallest = {}
    for config, scheme in RUNS:
        fast = _classes(config, scheme)["fast"]
        assert fast.sum() >= 0.25 * ia.A, (config, scheme, int(fast.sum()))
        for group, names in ia.GROUPS.items():
            n = int(fast[[ia.INDEX[x] for x in names]].sum())
            assert n >= 20, (config, scheme, group, n)
            smallest[(config, scheme)] = min(smallest.get((config, scheme), (n, group)), (n, group))
    print(smallest)
    for family, names in ia.EDGE_FAMILIES.items():
        for name in names:
            if family != "nonfinite":
                assert any(_at(_classes(config, "linearised")["fast"], name) for config in PRESETS), name
    # the melt cap is a class of its own making: enough fast entries end exactly on it in every run
    for config, scheme in RUNS:
        ref, fast = _reference(config, scheme), _classes(config, scheme)["fast"]
        assert (fast & (ref["temperature"] == 0.0)).sum() >= 100, (config, scheme)


# ---------------------------------------------------------------------------------------------
# seeded defects
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _polar(nx=90, ny=40):
    """The smooth state the interface solve was tested on before: util.build_case + util.polar_atmosphere."""
    case = util.build_case(nx, ny)
    g = orc.make_grid(nx, ny, 3, 3, 1)
    at = util.polar_atmosphere(orc.interpolate_atmosphere_state(g, case["src"], case["weights"], 0, 1, 0.37))
    return dict(case["ice_state"]), case["ocean"], at


def _polar_run(config, scheme, **kw):
    ice, ocean, at = _polar()
    out = _restated(config, scheme, (ocean, at, ice), hx=3, hy=3, ring=1, **kw)
    return {k: util.window(v, 3, 3, 90, 40, 1) for k, v in out.items()}


# defect → (preset, scheme) under which the atlas is asked, whether the smooth polar state sees it too (beyond 1e-9 on a
# cell its reference converges within 40 trips)
DEFECTS = {
    "cap_dropped": ("sea_ice_corrected", "linearised", False),
    "limiter_one_sided": ("sea_ice_corrected", "linearised", True),
    "hk_min_ignored": ("sea_ice_corrected", "linearised", True),
    "nan_guard_dropped": ("sea_ice_corrected", "linearised", False),
    "vaporisation_for_sublimation": ("sea_ice_corrected", "linearised", True),
    "albedo_ignored": ("sea_ice_corrected", "linearised", True),
    "calm_guard_dropped": ("sea_ice_corrected", "linearised", False),
    "gturb_not_carried": ("sea_ice_corrected", "linearised", True),
    "orbit_parity_flipped": ("sea_ice_corrected", "explicit", False),
}


@pytest.mark.parametrize("defect", list(slr.DEFECTS))
def test_seeded_defect_is_seen_by_the_atlas(defect):
    """Each defect, seeded into the NumPy restatement, moves at least one FAST entry beyond 1e-9 (the non-finite entries count
    for the NaN guard: there a defect shows as a NaN skin where the reference keeps the carried one); DEFECTS records which
    of them the smooth polar state sees too.  The point is the ones it does not.

    orbit_parity_flipped is the exception, by construction: the shortcut fires only on a cell that has NOT converged, and then
    sets its trip count to maxiter, so no entry it touches is fast in any run with a convergence criterion; under
    sea_ice_fixed5 no state repeats within five trips.  It is asked of the cap class instead (and on the device of every
    entry, by bits: test_orbit_shortcut_returns_the_bits_of_the_full_iteration)."""
    config, scheme, polar_sees = DEFECTS[defect]
    shortcut = defect == "orbit_parity_flipped"
    clean = _restated(config, scheme, orbit_shortcut=shortcut)
    bad = _restated(config, scheme, defect=defect, orbit_shortcut=shortcut)
    cls = _classes(config, scheme)
    e = _scaled_error(bad, clean)
    if shortcut:
        full, _ = _restated_row(config, scheme)
        assert np.array_equal(_scaled_error(clean, full) == 0, np.ones(ia.A, bool)) and np.array_equal(clean["iterations"], full["iterations"])
        moved = cls["cap"] & (e > 1e-9)
        assert not (e[cls["fast"] | cls["slow"]] > 0).any()
        for c in PRESETS:                                    # (nothing repeats within five trips, nothing fast orbits)
            tr = {}
            _restated(c, scheme, orbit_shortcut=True, trace=tr)
            assert not (tr["orbit"][0] & (_classes(c, scheme)["fast"] if c != "sea_ice_fixed5" else ia.FINITE)).any(), c
    elif defect == "nan_guard_dropped":
        assert not (e[ia.FINITE] > 0).any()
        moved = ~ia.FINITE & (clean["temperature"] == ia.table()["Ts"]) & (bad["temperature"] != clean["temperature"])
    else:
        moved = cls["fast"] & (e > 1e-9)
    print(defect, int(moved.sum()), [ia.NAMES[i] for i in np.flatnonzero(moved)[:8]])
    assert moved.any(), defect
    p_clean = _polar_run(config, scheme, orbit_shortcut=shortcut)
    p_bad = _polar_run(config, scheme, defect=defect, orbit_shortcut=shortcut)
    wet = p_clean["iterations"] > 0
    p_fast = wet & (p_clean["iterations"] <= SLOW) & (p_clean["friction_velocity"] >= 1e-8)
    sees = bool((_scaled_error(p_bad, p_clean)[p_fast] > 1e-9).any())
    assert sees == polar_sees, (defect, sees)


def test_the_smooth_state_misses_defects_the_atlas_sees():
    assert sorted(d for d, (_, _, sees) in DEFECTS.items() if not sees) == ["calm_guard_dropped", "cap_dropped", "nan_guard_dropped",
                                                                            "orbit_parity_flipped"]


# =============================================================================================
# GPU
# =============================================================================================
# name: (CONFIGS key, solver option).  The lean body runs constant roughness lengths with a gustiness floor under
# CF_SOLVER_TABLES; any other solver value sends the same presets to the full ice_iterate, as the existing tests select the
# non-tables ocean solver.  COARE and plain logarithmic profiles are separate instantiations of both bodies.
BODIES = {
    "lean_coare": ("sea_ice_corrected", abi.SOLVER_TABLES),
    "lean_ncar": ("sea_ice_ncar", abi.SOLVER_TABLES),
    "lean_log": ("sea_ice_corrected_log", abi.SOLVER_TABLES),
    "full_log": ("sea_ice_default", abi.SOLVER_TABLES),
    "full_coare": ("sea_ice_corrected", abi.SOLVER_LIBM),
    "full_ncar": ("sea_ice_ncar", abi.SOLVER_LIBM),
    "fixed5": ("sea_ice_fixed5", abi.SOLVER_TABLES),
}
BODY_CASES = [(b, s) for b in BODIES for s in SCHEMES]
NAN_BITS = np.uint64(0x7FF8000000000000)

# Entries a body is known to treat unlike the reference, with the cause read from the kernel code:
# (entry, bodies, schemes, cause).  Such an entry is left out of that run's reference comparison (never out of the bitwise
# checks) and carries a strict xfail of its own, test_entries_the_device_is_known_to_miss.  At most 1 % of a run's fast and
# slow entries, never a whole named group or edge family (test_device_known_is_within_its_caps).
DEVICE_KNOWN = (
    ("inf_T", tuple(BODIES), tuple(SCHEMES),
     "an infinite air temperature.  The C oracle divides: rho = p / (R_m T) = 0, so its stresses are -0.0, and its scales are "
     "theta* = +inf, q* = -inf.  The interface solve's cell set-up in ao_flux_fast_body (coflux_solver.hip) multiplies by a "
     "Newton-refined reciprocal, inv_Ta = frcp(Ta): r = rcp(inf) = 0, then r + r (1 - Ta r) with Ta r = inf * 0 = NaN.  So rho, "
     "q_a's vapour part and with them the stresses and q* are NaN on the device, for both iteration bodies (the set-up is "
     "shared).  The same cause as regime_atlas.DEVICE_KNOWN's inf_T; keeping 1 / inf = 0 means a select on the refined value in "
     "the flagship's path.  The skin stays the carried one on both sides (the NaN guard), and that is still asserted."),
)


def _bits(a):
    """The bit patterns of an array, every NaN the same one."""
    a = np.ascontiguousarray(a)
    if a.dtype != np.float64:
        return a.astype(np.int64)
    b = a.view(np.uint64).copy()
    b[np.isnan(a)] = NAN_BITS
    return b


@functools.lru_cache(maxsize=None)
def _inputs(kind, land=False, nonfinite=True, rounded=False):
    import mask_atlas as ma
    nx, ny, ids, ocean, atmos, ice = ia.fields(kind, nonfinite)
    wet = ia.land_mask(kind)[0] if land else np.ones(ids.shape, bool)
    if rounded:
        atmos = ra.through_float32(atmos)
    ocean = dict(ocean, mask=ma.embed(wet, nx, ny))
    return dict(nx=nx, ny=ny, ids=ids, wet=wet, ocean=ocean, atmos=atmos, ice=ice)


def _sentinels(ctx, names, with_iterations=False):
    import torch
    out = {k: util._fill(torch.empty(ctx.shape, dtype=torch.float64, device=ctx.device), util.SENTINEL64) for k in names}
    if with_iterations:
        out["iterations"] = util._fill(torch.empty(ctx.shape, dtype=torch.int32, device=ctx.device), util.SENTINEL32)
    return out


def _untouched(a):
    if a.dtype == np.int32:
        return a == np.int32(util.SENTINEL32)
    return a.view(np.uint64) == np.uint64(util.SENTINEL64)


def _context(c, config, scheme, solver=abi.SOLVER_TABLES, options=(), maxiter=None):
    from coflux.runtime import FluxContext
    fluxes, vd = _formulation(config, maxiter)
    ctx = FluxContext(c["nx"], c["ny"], H, H, ic.flux_params(), ring=RING)      # (the ocean formulation is independent)
    ctx.set_option(abi.OPT_SOLVER, solver)
    ctx.set_sea_ice_formulation(ic.flux_params(fluxes, velocity_difference=vd),
                                ic.SeaIceInterfaceProperties(skin_temperature_scheme=SCHEMES[scheme]).to_params())
    for opt, val in options:
        ctx.set_option(opt, val)
    dev = ctx.to_device
    d = dict(ocean={k: dev(v) for k, v in c["ocean"].items()}, atmos={k: dev(c["atmos"][k]) for k in EXCHANGE_NAMES},
             ice={k: dev(v) for k, v in c["ice"].items()})
    return ctx, d


def _solve(ctx, d, c, calls=1):
    """`calls` interface solves with identical inputs, each into fresh sentinel-filled outputs; the skin is an input buffer of its
    own (never an output's), and must come back untouched.  Returns the window of every field per call."""
    import torch
    skin = d["ice"]["top_temperature"].clone()
    runs = []
    for _ in range(calls):
        out = _sentinels(ctx, CELL_FIELDS, with_iterations=True)
        ctx.compute_atmosphere_sea_ice_fluxes(d["ice"], d["ocean"], d["atmos"], out)
        ctx.sync()
        torch.cuda.synchronize()
        runs.append({k: util.window(v.cpu().numpy(), H, H, c["nx"], c["ny"], RING) for k, v in out.items()})
    assert torch.equal(skin.view(torch.int64), d["ice"]["top_temperature"].view(torch.int64))
    return runs


def _run(c, config, scheme, solver=abi.SOLVER_TABLES, options=(), maxiter=None, calls=1):
    ctx, d = _context(c, config, scheme, solver, options, maxiter)
    runs = _solve(ctx, d, c, calls)
    ctx.close()
    return runs if calls > 1 else runs[0]


def _names(ids, where):
    found = np.unique(ids[where])
    return [ia.NAMES[i] for i in found[:6]] + (["…"] if found.size > 6 else [])


def _check_written(label, c, got, fixed_trips=0):
    """Every window cell written; land exactly zero — the skin temperature 0 K in the interface's units; no trips, or under
    FixedIterations the fixed count, as in the C oracle."""
    land = ~c["wet"]
    for k in ALL:
        left = _untouched(got[k])
        assert not left.any(), (label, k, "window cells left unwritten", int(left.sum()), _names(c["ids"], left))
        want = -ic.SeaIceInterfaceProperties().temperature_offset if k == "temperature" else 0
        if k == "iterations" and fixed_trips:
            assert np.all(np.isin(got[k][land], (0, fixed_trips))), (label, k, "land")
        else:
            assert np.all(got[k][land] == want), (label, k, "land")


def _canonical(c, got):
    """Per field, the bits of every entry's first wet copy."""
    order, starts = ia.copies(c["ids"], c["wet"])
    return {k: _bits(got[k]).reshape(-1)[order[starts]] for k in ALL}


def _first_copy(c, got):
    order, starts = ia.copies(c["ids"], c["wet"])
    return {k: got[k].reshape(-1)[order[starts]] for k in ALL}


def _check_copies(label, c, got, canon):
    """Position independence: every wet copy of an entry holds the canonical bits, in every field and in the trip count."""
    for k in ALL:
        differ = c["wet"] & (_bits(got[k]) != canon[k][c["ids"]])
        assert not differ.any(), (label, k, "copies of one entry differ", int(differ.sum()), _names(c["ids"], differ))


def _same(label, a, b, where=None):
    for k in ALL:
        differ = _bits(a[k]) != _bits(b[k])
        if where is not None:
            differ &= where
        assert not differ.any(), (label, k, int(differ.sum()))


def _known(body, scheme):
    return tuple(dict.fromkeys(name for name, bodies, schemes, _ in DEVICE_KNOWN if body in bodies and scheme in schemes))


def _tolerances(config, scheme):
    fast = 1e-8 if config == "sea_ice_fixed5" else TOL_ICE          # (test_gpu_parity.py: the ψ tables at |ζ| > 1e3, amplified)
    slow = 1e-5 if (config, scheme) == ("sea_ice_ncar", "linearised") else 1e-6
    return fast, slow


def _check_reference(label, config, scheme, got, *, maxiter=None, skip=(), only=None):
    """One value per entry (`got`: field → [A]) against the reference, by class.  Collects every miss before it fails, and
    returns the worst scaled error per class."""
    ref, cls = _reference(config, scheme, maxiter), _classes(config, scheme, maxiter)
    tol_fast, tol_slow = _tolerances(config, scheme)
    listed = np.isin(np.arange(ia.A), [ia.INDEX[n] for n in (only if only is not None else skip)])
    sel = listed if only is not None else ~listed
    e = _scaled_error(got, ref)
    it_g, it_r = got["iterations"].astype(int), ref["iterations"].astype(int)
    misses = []

    def miss(what, where):
        if where.any():
            i = np.flatnonzero(where)
            misses.append((what, int(i.size), [(ia.NAMES[j], float(e[j]), int(it_g[j]), int(it_r[j])) for j in i[:8]]))

    miss("fast beyond %g" % tol_fast, sel & cls["fast"] & ~(e <= tol_fast))
    miss("slow beyond %g" % tol_slow, sel & cls["slow"] & ~(e <= tol_slow))
    miss("collapsed beyond %g" % tol_slow, sel & cls["collapsed"] & ~(e <= tol_slow))
    miss("trip counts", sel & (cls["fast"] | cls["slow"]) & (it_g != it_r))
    miss("collapsed trip counts", sel & cls["collapsed"] & (np.abs(it_g - it_r) > 1))
    miss("not at the cap", sel & cls["cap"] & (it_g != it_r))
    finite = np.all([np.isfinite(got[k]) for k in CELL_FIELDS], axis=0)
    miss("cap entry not finite", sel & cls["cap"] & ~finite)
    # the melting cap: exactly 0 °C where the reference ends on it
    # (the knife edge apart: cap[just_missed] and cap[just_reached] are neighbouring doubles of shortwave, the first under
    # which the NumPy restatement ends on the cap and the last under which it ends one ulp of 273.15 K below.  Which side a fused
    # multiply-add or a reciprocal in place of a division lands on is rounding — measured: the full body's linearised step
    # ends 5.7e-14 K below under both, every other field within 1.2e-13 — so for these two the skin is 0 or within 1e-12 below)
    edge = np.isin(np.arange(ia.A), [ia.INDEX["cap[just_missed]"], ia.INDEX["cap[just_reached]"]])
    capped = (cls["fast"] | cls["slow"]) & (ref["temperature"] == 0.0) & ~edge
    miss("melt cap not exactly 0.0", sel & capped & ~(_bits(got["temperature"]) == _bits(np.zeros(1))[0]))
    miss("knife edge of the cap", sel & edge & (cls["fast"] | cls["slow"]) & (np.abs(ref["temperature"]) < 1e-12)
         & ~((got["temperature"] <= 0.0) & (got["temperature"] > -1e-12)))
    # calm and co-moving air: exact zeros
    cols = ia.table()
    relative = _wind(_formulation(config)[1]) == "relative"
    calm = ia.FINITE & (cols["u"] - (cols["ui"] if relative else 0) == 0) & (cols["v"] - (cols["vi"] if relative else 0) == 0)
    miss("stress under calm air", sel & calm & ((got["x_momentum"] != 0) | (got["y_momentum"] != 0)))
    # non-finite entries: NaN in the same fields; the skin is the carried input where the reference's is
    for name in ia.NONFINITE:
        i = ia.INDEX[name]
        carried = _at(cols["Ts"], name)
        if (sel[i] or only is None) and ref["temperature"][i] == carried and got["temperature"][i] != carried:
            misses.append(("skin is not the carried input", name, float(got["temperature"][i])))     # (a listed entry too)
        if not sel[i]:
            continue
        for k in CELL_FIELDS:
            if np.isnan(got[k][i]) != np.isnan(ref[k][i]):
                misses.append(("NaN pattern", name, k, float(got[k][i]), float(ref[k][i])))
    worst = {k: float(e[sel & cls[k]].max(initial=0.0)) for k in CLASSES}
    print(label, "worst scaled error per class", {k: "%.2e" % v for k, v in worst.items()},
          "share of cap entries within 1e-9: %.3f" % float((e[sel & cls["cap"]] <= 1e-9).mean() if (sel & cls["cap"]).any() else 1.0))
    assert not misses, (label, misses)
    return worst


def _hints_reorder(ctx, c, first):
    """Whether the trip counts the first call left as hints put some chunk's wet list into another order: the list starts in
    index order and each call sorts it by the hint's bin, longest first (coflux_solver_shared.hpp: one bin per count below
    56).  So the order changes wherever, within a chunk, a cell is followed by one that took more trips.  Cells at the cap
    are left out: under the orbit shortcut their hint is the work done, not the trip count reported."""
    begins, counts, valid = ctx.debug_chunk_table()
    assert valid and len(counts) >= 2
    its, wet = first["iterations"].reshape(-1), c["wet"].reshape(-1)
    changed = 0
    for b, e in zip(begins[:-1], begins[1:]):
        t = its[b:e][wet[b:e] & (its[b:e] < 56)]
        changed += bool(np.any(np.diff(t) > 0))
    return changed, len(counts)


@gpu
@pytest.mark.parametrize("body,scheme", BODY_CASES, ids=[f"{b}-{s}" for b, s in BODY_CASES])
def test_interface_body_on_the_atlas(body, scheme):
    """One body and scheme on the four runs of the atlas — cyclic and blocks, each all-wet and under the checkerboard — from
    sentinel-filled outputs: every window cell written, land zero; the first copy of every entry against the reference by
    class (_check_reference; measured worst errors in DESIGN.md §5.4); every copy within and between the layouts and their
    land variants the same bits; and a second call with identical inputs — by then the first call's trip counts have
    re-sorted every chunk's list, so the same cell has other wave-mates — the same bits again.

    Measured on an MI355X, worst scaled error over the entries held (DEVICE_KNOWN left out), cyclic layout:
        body        scheme         fast      slow      collapsed                  cap entries within 1e-9 (worst)
        lean_coare  explicit       3.95e-11  1.44e-12  –                          97.0 % (5.2e-02)
        lean_coare  semi-implicit  3.95e-11  1.45e-12  –                          96.9 % (5.0e-02)
        lean_coare  linearised     4.92e-11  1.43e-12  –                          no cap entries
        lean_ncar   explicit       5.77e-13  1.35e-13  3.49e-15                   99.0 % (3.3e-06)
        lean_ncar   semi-implicit  6.56e-13  2.87e-13  1.06e-14                   99.0 % (1.8e-05)
        lean_ncar   linearised     6.20e-12  2.27e-13  1.06e-14                   100 %  (2.2e-13)
        lean_log    explicit       3.73e-11  2.38e-12  –                          95.9 % (5.9e-02)
        lean_log    semi-implicit  3.78e-11  2.31e-12  –                          95.0 % (5.8e-02)
        lean_log    linearised     3.77e-10  1.49e-12  –                          no cap entries
        full_log    explicit       7.18e-12  2.34e-12  –                          100 %  (8.1e-10)
        full_log    semi-implicit  7.18e-12  2.84e-13  –                          99.8 % (1.4e-08)
        full_log    linearised     7.18e-12  7.43e-14  –                          no cap entries
        full_coare  explicit       3.95e-11  1.44e-12  –                          97.0 % (5.2e-02)
        full_coare  semi-implicit  3.96e-11  1.44e-12  –                          96.9 % (5.0e-02)
        full_coare  linearised     4.92e-11  1.44e-12  –                          no cap entries
        full_ncar   explicit       5.77e-13  1.34e-13  3.49e-15                   98.8 % (2.0e-06)
        full_ncar   semi-implicit  5.77e-13  2.81e-13  2.12e-14                   99.0 % (1.9e-05)
        full_ncar   linearised     6.25e-12  1.60e-14  1.06e-14                   100 %  (2.0e-13)
        fixed5      explicit       9.13e-10  –         –                          –        (bound 1e-8)
        fixed5      semi-implicit  6.65e-10  –         –                          –
        fixed5      linearised     1.15e-10  –         –                          –
    (all nine fields; beyond the ψ tables both bodies take ψ from closed forms, psi_beyond_tables.)  Trip counts are identical on every fast and slow entry held; every cap entry of the
    reference is at the cap on the device.  The whole file's GPU tests take 18 s."""
    config, solver = BODIES[body]
    canon = None
    for kind, land in (("cyclic", False), ("cyclic", True), ("blocks", False), ("blocks", True)):
        label = (body, scheme, kind, "checkerboard" if land else "all_wet")
        c = _inputs(kind, land)
        ctx, d = _context(c, config, scheme, solver)
        runs = _solve(ctx, d, c, calls=2 if kind == "cyclic" else 1)
        if kind == "cyclic" and not land and config != "sea_ice_fixed5" and ctx.debug_chunk_table()[2]:
            changed, chunks = _hints_reorder(ctx, c, runs[0])
            assert changed >= 1, (label, "the hints left the order alone: the repeat call shows nothing", changed, chunks)
        ctx.close()
        for call, got in enumerate(runs):
            lab = label + (f"call {call}",)
            _check_written(lab, c, got, 5 if config == "sea_ice_fixed5" else 0)
            if canon is None:
                canon = _canonical(c, got)
                _check_reference(lab, config, scheme, _first_copy(c, got), skip=_known(body, scheme))
            _check_copies(lab, c, got, canon)


KNOWN_CASES = [(body, scheme, name, cause) for name, bodies, schemes, cause in DEVICE_KNOWN for body in bodies for scheme in schemes]


@gpu
@pytest.mark.parametrize("body,scheme,name,cause", KNOWN_CASES, ids=[f"{b}-{s}-{n}" for b, s, n, _ in KNOWN_CASES])
def test_entries_the_device_is_known_to_miss(body, scheme, name, cause, request):
    """DEVICE_KNOWN: the reference comparison on nothing but one listed entry, cyclic layout.  Strict: a body that comes to
    agree with the reference must leave the list."""
    request.applymarker(pytest.mark.xfail(strict=True, raises=AssertionError, reason=cause))
    _check_reference((body, scheme, name), BODIES[body][0], scheme, _cyclic_first_copy(body, scheme), only=(name,))


@functools.lru_cache(maxsize=None)
def _cyclic_first_copy(body, scheme):
    config, solver = BODIES[body]
    c = _inputs("cyclic")
    return _first_copy(c, _run(c, config, scheme, solver))


def test_the_atlas_reaches_beyond_the_psi_tables():
    """By the reference alone: fast entries whose |ζ| at the answer lies beyond the ψ tables' edge (2^34 / 16 = 1.07e9) exist in
    the runs over constant roughness lengths — calm air warmer than thick ice in the dark, u★ = 2e-6 … 4e-6 m/s — so the
    closed forms the two iteration bodies use out there (psi_beyond_tables, coflux_fast.hpp) are held to 1e-9 by
    test_interface_body_on_the_atlas.  With ψ evaluated at the tables' edge instead these entries miss by up to 6 % in θ★
    (measured before psi_beyond_tables existed: 12, 12, 6, 6 and 24 entries, and no other fast or slow entry of any run)."""
    want = {("lean_coare", "linearised"): 12, ("full_coare", "linearised"): 12, ("lean_log", "explicit"): 6,
            ("lean_log", "semi_implicit"): 6, ("lean_log", "linearised"): 24}
    for body, (config, _) in BODIES.items():
        for scheme in SCHEMES:
            cls = _classes(config, scheme)
            with np.errstate(invalid="ignore"):
                beyond = (cls["fast"] | cls["slow"]) & (np.abs(_zeta(config, scheme)) > ZETA_EDGE)
            if config != "sea_ice_fixed5":
                assert beyond.sum() == want.get((body, scheme), 0), (body, scheme, int(beyond.sum()))
                assert all(ia.NAMES[i].startswith("grid[U=0,") and ia.NAMES[i].endswith("rad=dark]") for i in np.flatnonzero(beyond))


def test_device_known_is_within_its_caps():
    """At most 1 % of a run's fast and slow entries, never a whole named group or edge family, every entry with a cause."""
    for body, (config, _) in BODIES.items():
        for scheme in SCHEMES:
            names = _known(body, scheme)
            cls = _classes(config, scheme)
            held = cls["fast"] | cls["slow"]
            listed = sum(bool(_at(held, n)) for n in names)
            assert listed <= 0.01 * held.sum(), (body, scheme, listed)
            for group in list(ia.GROUPS.values()) + list(ia.EDGE_FAMILIES.values()):
                assert not set(group) <= set(names), (body, scheme, group[:2])
    for name, bodies, schemes, cause in DEVICE_KNOWN:
        assert name in ia.INDEX and set(bodies) <= set(BODIES) and set(schemes) <= set(SCHEMES) and len(cause) > 80


SHORTCUT_CASES = [(b, s) for b in ("lean_coare", "lean_ncar", "full_log", "full_coare") for s in SCHEMES]


@gpu
@pytest.mark.parametrize("body,scheme", SHORTCUT_CASES, ids=[f"{b}-{s}" for b, s in SHORTCUT_CASES])
def test_orbit_shortcut_returns_the_bits_of_the_full_iteration(body, scheme):
    """CF_OPT_ICE_ORBIT_SHORTCUT 0 against 1 on every entry, with maxiter as the preset sets it and one smaller — both
    parities of (maxiter − it) & 1 — through the preset's own stop criterion.  The shortcut must have fired: the run with
    it off is the one whose cap entries did all their trips."""
    config, solver = BODIES[body]
    c = _inputs("cyclic")
    for maxiter in (100, 99):
        full = _run(c, config, scheme, solver, ((abi.OPT_ICE_ORBIT_SHORTCUT, 0),), maxiter)
        short = _run(c, config, scheme, solver, ((abi.OPT_ICE_ORBIT_SHORTCUT, 1),), maxiter)
        _same((body, scheme, maxiter), full, short)
        assert full["iterations"].max() == maxiter or scheme == "linearised", (body, scheme, maxiter)
        cap = _classes(config, scheme, maxiter)["cap"]
        assert np.array_equal(_first_copy(c, full)["iterations"][cap], np.full(int(cap.sum()), maxiter)), (body, scheme, maxiter)


ICE_FREE_CASES = [(b, s, k) for b, s in (("lean_coare", "linearised"), ("lean_ncar", "explicit"), ("full_log", "semi_implicit"))
                  for k in ("blocks", "cyclic")]


@gpu
@pytest.mark.parametrize("body,scheme,kind", ICE_FREE_CASES, ids=[f"{b}-{s}-{k}" for b, s, k in ICE_FREE_CASES])
def test_ice_free_option_skips_open_water_and_nothing_else(body, scheme, kind):
    """CF_OPT_ICE_FREE_CELLS = CF_ICE_FREE_ZERO against the default: identical bits on every entry that has ice; zero scales
    and fluxes, zero trips and the input skin's bits on (ℵ, h) = (0, 0) and (−0, 0); (0, 0.3) and (0.9, 0) are solved.  In
    `blocks` an open-water entry is a whole wave (the batch skips the solve), in `cyclic` one lane among solving ones."""
    config, solver = BODIES[body]
    c = _inputs(kind)
    base = _run(c, config, scheme, solver)
    zero = _run(c, config, scheme, solver, ((abi.OPT_ICE_FREE_CELLS, abi.ICE_FREE_ZERO),))
    _check_written((body, scheme, kind), c, zero)
    skipped = np.isin(c["ids"], [ia.INDEX[n] for n in ia.SKIPPED_WHEN_ICE_FREE])
    assert skipped.sum() >= (128 if kind == "blocks" else 8)
    _same((body, scheme, kind, "cells with ice"), base, zero, where=~skipped)
    for k in ALL:
        if k == "temperature":
            assert np.array_equal(_bits(zero[k][skipped]), _bits(np.full(int(skipped.sum()), ia._cell()["Ts"]))), k
        else:
            assert not zero[k][skipped].any(), (k, "open water is not zero")
    for name in ("open[conc=0,h=0.3]", "open[conc=0.9,h=0]") + ia.SKIPPED_WHEN_ICE_FREE:
        assert np.all(base["iterations"][c["ids"] == ia.INDEX[name]] > 0), name


CARRY_CASES = [("sea_ice_corrected", "linearised", "default", "cyclic"), ("sea_ice_corrected", "explicit", "ncar", "cyclic"),
               ("sea_ice_ncar", "semi_implicit", "default", "blocks"), ("sea_ice_ncar", "linearised", "ncar", "blocks")]


@gpu
@pytest.mark.parametrize("config,scheme,ocean_config,kind", CARRY_CASES, ids=["-".join(x) for x in CARRY_CASES])
def test_carrying_launches_give_the_same_interface_bits(config, scheme, ocean_config, kind):
    """The interface solve in its own launch, and inside cf_update_state_sea_ice with CF_OPT_MERGED_PREFETCH = 2 — where,
    read from cf_update_state_sea_ice and update_state_impl, the lean ocean formulation (`default`) makes the ocean solve ride
    in the interface solve's launch (ice_ocean_kernel) and the Large–Yeager one (`ncar`) leaves the face stresses to ride in
    its tail (ao_flux_fast_kernel's tail form) — on the checkerboard variant of the atlas, the atmosphere handed out by the
    identity source (float32: the own launch runs on the same rounded fields).  Same interface bits on every wet cell; the
    net sea-ice fluxes of the launch's epilogue are the bits cf_compute_net_sea_ice_fluxes gives afterwards."""
    import torch
    from coflux.runtime import FluxContext
    c = _inputs(kind, True, False, True)
    own = _run(c, config, scheme)
    src, w = ra.identity_source(ia.fields(kind, False)[4])
    fluxes, vd = _formulation(config)
    ofluxes, ovd = util.CONFIGS[ocean_config]()
    ctx = FluxContext(c["nx"], c["ny"], H, H, ic.flux_params(ofluxes, velocity_difference=ovd), ring=RING)
    ctx.set_sea_ice_formulation(ic.flux_params(fluxes, velocity_difference=vd),
                                ic.SeaIceInterfaceProperties(skin_temperature_scheme=SCHEMES[scheme]).to_params())
    ctx.set_option(abi.OPT_MERGED_PREFETCH, 2)
    dev = ctx.to_device
    ocean = {k: dev(v) for k, v in c["ocean"].items()}
    dsrc = {k: dev(v) for k, v in src.items()}
    dw = {k: (dev(v) if isinstance(v, np.ndarray) else v) for k, v in w.items()}
    state = {k: dev(v) for k, v in c["ice"].items()}
    part = dict(concentration=state["concentration"], **{k: ctx.zeros() for k in ("interface_heat", "salt_flux", "x_stress", "y_stress")})
    atmos, fl, net = _sentinels(ctx, EXCHANGE_NAMES), _sentinels(ctx, CELL_FIELDS, with_iterations=True), _sentinels(ctx, NET_NAMES)
    ai, net_ice = _sentinels(ctx, CELL_FIELDS, with_iterations=True), _sentinels(ctx, ("top_heat", "bottom_heat"))
    ctx.update_state_sea_ice(dsrc, dw, ocean, atmos, fl, net, part, state, ai, net_ice, level1=0, level2=1, time_fraction=0.0)
    ctx.sync()
    after = _sentinels(ctx, ("top_heat", "bottom_heat"))
    ctx.compute_net_sea_ice_fluxes(state, ocean, atmos, ai, after)
    ctx.sync()
    torch.cuda.synchronize()
    W = lambda t, r=RING: util.window(t.cpu().numpy(), H, H, c["nx"], c["ny"], r)   # noqa: E731
    label = (config, scheme, ocean_config, kind)
    for k in EXCHANGE_NAMES:      # the identity source handed out the rounded atlas: both forms solved the same cells
        assert np.array_equal(_bits(W(atmos[k])), _bits(util.window(c["atmos"][k], H, H, c["nx"], c["ny"], RING))), (label, "atmos." + k)
    carried = {k: W(v) for k, v in ai.items()}
    _check_written(label, c, carried)
    _same(label, own, carried, where=c["wet"])
    for k in ("top_heat", "bottom_heat"):
        a, b = W(net_ice[k], 0), W(after[k], 0)
        assert not _untouched(a).any() and np.array_equal(_bits(a), _bits(b)), (label, k)
    assert np.any(W(net_ice["top_heat"], 0) != 0)
    ctx.close()
