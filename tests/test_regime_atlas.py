"""Every solver body on an atlas of surface regimes (tests/regime_atlas.py), held to the oracle and to ITSELF.

The suite's claims about the similarity solve — every body within TOL_SOLVER = 1e-9 of the CPU oracle with the oracle's trip
counts, most bodies bitwise equal to one another — were checked on the smooth state of util.build_case, where a cell's
wave-mates are near copies of it.  A result that depends on which cells share a lane's wave, batch or chunk moves a
converged cell by less than the stop tolerance: inside 1e-9, and without contrast on a smooth surface.  Here one cell is
compared with itself under different wave-mates, by bits.

CPU part (no marker): the entries' own properties, the qualification of the reference alone (C and NumPy restatements:
identical trip counts, 1e-12, nothing at the cap), the collapsed cells, seeded defects that the atlas sees and the smooth
case does not.  GPU part: per body and layout the oracle comparison, position independence within and between the
layouts and the land variants, the bitwise claims between forms, the step loop.

Measured on the CPU (both currents, every preset of util.CONFIGS): trip counts of the two restatements differ in 0 entries,
worst scaled difference 2.65e-13 (latent_heat, grid[U=80,dT=-0.001,rh=0.98,sst=15]).  On the full 1320-cell grid seven
presets leave nothing at the cap (trips 4 … 38 of 100) and nothing with u★ < 1e-8; sea_ice_ncar — Large–Yeager stability
functions over constant roughness — collapses or orbits on 204 calm, stable cells (regime_atlas.UNQUALIFIED).  Those are
dropped, eleven of them kept as BITS_ONLY; on the 1153 entries that remain every preset qualifies (trips 4 … 33, sea_ice_ncar 5 … 93) and
COLLAPSED is empty."""
import functools

import numpy as np
import pytest

import numpy_oracle as npo
import oracle as orc
import regime_atlas as ra
import util
from coflux import abi
from coflux import interface_computations as ic
from coflux.runtime import EXCHANGE_NAMES, NET_NAMES
from test_mask_atlas import BODIES, CELL_FIELDS, TOL_SOLVER, _host, _params, _sentinel_fields, _untouched

gpu = pytest.mark.gpu

H, RING = ra.HALO, ra.RING
TOL_REFERENCE = 1e-12     # what test_oracle.py holds the two restatements to
FIVE = ("sensible_heat", "latent_heat", "water_vapor", "x_momentum", "y_momentum")
ATLAS_BODIES = dict(BODIES,
                    corrected_wind=("corrected_wind", "unfused", (), abi.SOLVER_TABLES),
                    shear_aware=("shear_aware", "unfused", (), abi.SOLVER_TABLES))
RUN_CONFIGS = tuple(dict.fromkeys(v[0] for v in ATLAS_BODIES.values()))     # the presets the atlas bodies run


# =============================================================================================
# CPU
# =============================================================================================
def _row(current, nonfinite=True):
    """The atlas as one row of cells (ring 0, halo 1): (grid, ocean, atmos)."""
    cols = ra.table(current, nonfinite)
    shape = (3, ra.A + 2)
    full = {f: np.full(shape, cols[f][0]) for f in ra.FIELDS}
    for f in ra.FIELDS:
        full[f][1, 1:-1] = cols[f]
    uc, vc = ra.CURRENTS[current]
    ocean = dict(T=full["To"], S=full["So"], u=np.full(shape, uc), v=np.full(shape, vc))
    return orc.make_grid(ra.A, 1, 1, 1, 0), ocean, {f: full[f] for f in ra.ATMOS}


def _entries(out):
    return {k: v[1, 1:-1] for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def _c_row(config, current, nonfinite=True):
    g, ocean, atmos = _row(current, nonfinite)
    return _entries(orc.compute_atmosphere_ocean_fluxes(g, _params(config), ocean, atmos))


def _np_fluxes(config, ocean, atmos, h, ring, *, fluxes=None, absolute_wind=False):
    f, vd = util.CONFIGS[config]()
    wind = absolute_wind or isinstance(vd, ic.WindVelocity)
    with np.errstate(all="ignore"):
        return npo.atmosphere_ocean_fluxes(fluxes or f, ocean, atmos, hx=h, hy=h, ring=ring,
                                           thermodynamics=ic.AtmosphereThermodynamicsParameters(), seawater=ic.SeawaterComposition(),
                                           ocean_properties=ic.OceanProperties(), velocity_difference="wind" if wind else "relative")


def _np_row(config, current, nonfinite=True, **kw):
    _, ocean, atmos = _row(current, nonfinite)
    return _entries(_np_fluxes(config, ocean, atmos, 1, 0, **kw))


def _cell_error(got, ref):
    """Per cell, the largest |Δ| / max(|ref|, field scale) over the nine cell-local fields; a NaN on one side only is inf."""
    worst = np.zeros(np.shape(ref["sensible_heat"]))
    for k in CELL_FIELDS:
        with np.errstate(invalid="ignore"):
            e = np.abs(got[k] - ref[k]) / np.maximum(np.abs(ref[k]), util.FIELD_SCALE[k])
        e = np.where(np.isnan(got[k]) & np.isnan(ref[k]), 0.0, np.where(np.isnan(e), np.inf, e))
        worst = np.maximum(worst, e)
    return worst


def test_the_atlas_is_what_the_layouts_need():
    assert ra.A == 1153 and np.gcd(ra.A, 64) == 1 and len(set(ra.NAMES)) == ra.A
    assert {k: len(v) for k, v in ra.GROUPS.items()} == dict(grid=1127, kinematics=10, edges=8, nonfinite=7, pad=1)
    assert len(list(ra.grid_cells())) == 1320 and 1320 - 1127 == 204 - len(ra.BITS_ONLY) and set(ra.BITS_ONLY) <= set(ra.NAMES)
    assert sum(len(v) for v in ra.GROUPS.values()) == ra.A
    for current in ra.CURRENTS:
        cols = ra.table(current)
        for f in ra.FIELDS:
            bad = ~np.isfinite(cols[f])
            assert [ra.NAMES[i] for i in np.flatnonzero(bad)] == [n for n in ra.NONFINITE if n.split("_")[1] == f], f
        assert np.all(np.isfinite(np.stack([ra.table(current, nonfinite=False)[f] for f in ra.FIELDS])))
    nx, ny, ids = ra.layout("cyclic")
    assert ids.shape == (39, 133) and np.array_equal(ids.reshape(-1), np.arange(5187) % ra.A)
    assert np.bincount(ids.reshape(-1), minlength=ra.A).min() == 4          # four or five copies of every entry …
    lanes = [set((np.flatnonzero(ids.reshape(-1) == e) % 64).tolist()) for e in (0, 700, ra.A - 1)]
    assert all(len(s) >= 3 for s in lanes)                                  # … each in another lane
    nx, ny, ids = ra.layout("blocks")
    flat = ids.reshape(-1)
    assert flat.size >= 64 * ra.A and flat.size - 64 * ra.A < ids.shape[1] and flat.size <= 90000
    assert np.array_equal(flat[:64 * ra.A].reshape(ra.A, 64), np.repeat(np.arange(ra.A)[:, None], 64, axis=1))
    for kind in ("cyclic", "blocks"):                                       # the land variant leaves every entry a wet copy
        wet, mask = ra.land_mask(kind)
        _, _, ids = ra.layout(kind)
        assert 0.45 < wet.mean() < 0.55 and mask.dtype == np.uint8
        assert np.bincount(ids[wet], minlength=ra.A).min() >= 1
    ocean, atmos = ra.fields("cyclic", "drift", nonfinite=False)   # (a NaN node poisons its neighbours through 0 · NaN)
    assert np.all(ocean["u"] == 0.25) and np.all(ocean["v"] == -0.15) and atmos["T"].shape == (37 + 2 * H, 131 + 2 * H)
    src, w = ra.identity_source(atmos)
    g = orc.make_grid(131, 37, H, H, RING)
    back = orc.interpolate_atmosphere_state(g, src, w, 0, 1, 0.0)
    want = ra.through_float32(atmos)
    for k in EXCHANGE_NAMES:   # the identity map hands out the float32-rounded atlas
        assert np.array_equal(util.window(back[k], H, H, 131, 37, RING), util.window(want[k], H, H, 131, 37, RING)), k


def test_entries_have_the_property_they_are_named_for():
    rest, drift = _c_row("default", "rest"), _c_row("default", "drift")
    at = lambda out, k, name: out[k][ra.INDEX[name]]   # noqa: E731
    part = lambda name, key: float(name.split(key + "=")[1].split(",")[0])   # noqa: E731
    grid = [(ra.INDEX[name], cell["u"], part(name, "dT"), part(name, "rh"))     # (entry, wind speed, contrast, humidity)
            for name, cell, _ in ra.grid_cells() if name in ra.INDEX]
    assert len(grid) == 1127 and {d for _, _, d, _ in grid} == set(ra.CONTRASTS)
    n_unstable = n_stable = 0
    for config in RUN_CONFIGS:
        out = _c_row(config, "rest")
        for k, s, d, r in grid:
            th, q = out["temperature_scale"][k], out["humidity_scale"][k]
            assert np.isfinite([out[f][k] for f in CELL_FIELDS]).all(), (config, ra.NAMES[k])
            if d <= -1.0 and r <= 0.5:       # colder, drier air: θ★ < 0 and q★ < 0 ⇒ b★ < 0, unstable
                assert th < 0 and q < 0, (config, ra.NAMES[k], th, q)
                n_unstable += 1
            if d >= 1.0 and r == 1.3:        # warmer, super-saturated air: θ★ > 0 and q★ > 0 ⇒ b★ > 0, stable
                assert th > 0 and q > 0, (config, ra.NAMES[k], th, q)
                n_stable += 1
            if abs(d) <= 1e-3:               # Δθ = ΔT + g h / c_p: the 10 m of lapse decide the sign
                assert 0 < th, (config, ra.NAMES[k], th)
            if s == 0.0:                     # calm: exactly zero stress, gustiness keeps the scalar fluxes alive
                assert out["x_momentum"][k] == 0.0 and out["y_momentum"][k] == 0.0 and out["friction_velocity"][k] > 0
            else:
                assert out["x_momentum"][k] < 0.0 and out["y_momentum"][k] == 0.0, (config, ra.NAMES[k])
    assert n_unstable == len(RUN_CONFIGS) * 180 and n_stable == len(RUN_CONFIGS) * sum(1 for _, _, d, r in grid if d >= 1.0 and r == 1.3) > 0
    # kinematics: the stress opposes the wind in every octant, with one magnitude; components on an axis are exact zeros
    mags = []
    for k in range(8):
        name = f"octant{k * 45}"
        u, v = ra.table("rest")["u"][ra.INDEX[name]], ra.table("rest")["v"][ra.INDEX[name]]
        tx, ty = at(rest, "x_momentum", name), at(rest, "y_momentum", name)
        assert np.sign(tx) == -np.sign(u) and np.sign(ty) == -np.sign(v), name
        mags.append(np.hypot(tx, ty))
    assert np.ptp(mags) <= 1e-12 * mags[0]
    for out, current in ((rest, "rest"), (drift, "drift")):
        assert at(out, "x_momentum", "wind_is_current") == 0.0 and at(out, "y_momentum", "wind_is_current") == 0.0, current
        assert at(out, "friction_velocity", "wind_is_current") > 0
    assert ra.table("drift")["u"][ra.INDEX["wind_is_current"]] == 0.25 and ra.table("drift")["v"][ra.INDEX["wind_opposes_current"]] == 0.15
    assert at(rest, "x_momentum", "wind_opposes_current") == 0.0
    assert at(drift, "x_momentum", "wind_opposes_current") > 0.0 > at(drift, "y_momentum", "wind_opposes_current")
    windy = _c_row("corrected_wind", "drift")      # WindVelocity ignores the current
    assert at(windy, "x_momentum", "wind_is_current") < 0.0 < at(windy, "y_momentum", "wind_is_current")
    # composition: fresher water evaporates more; bone-dry air takes vapour whatever the temperature contrast
    assert at(rest, "latent_heat", "S=0") > at(rest, "latent_heat", "octant0") > at(rest, "latent_heat", "S=45") > 0
    assert at(rest, "x_momentum", "p=50000") > at(rest, "x_momentum", "octant0") > at(rest, "x_momentum", "p=108000")   # ρ ∝ p
    for name in ("q=0,dT=-15", "q=0,dT=15"):
        assert at(rest, "humidity_scale", name) < 0 and at(rest, "water_vapor", name) > 0
    for name in ("radiation_zero", "radiation_large"):     # radiation and rain enter the net fluxes only
        for f in CELL_FIELDS + ("iterations",):
            assert at(rest, f, name) == at(rest, f, "octant0"), (name, f)


# Which of the nine cell-local fields of the C oracle are NaN for each non-finite entry — under every preset the atlas
# bodies run and both currents, unless a preset is named.  The issue expected NaN in every flux field; that holds for NaN
# in T or p only.  The oracle (and the kernels, written after it) clamps with fmax / fmin, which return the other operand
# when one is NaN: q = fmin(fmax(q, 0), 1) turns a NaN humidity into bone-dry air with finite fluxes, the roughness
# lengths' fmin(…, ℓ_max) drops a NaN viscosity, Large–Yeager's U = fmax(|Δu|, minimum wind) a NaN wind.  The NumPy
# restatement clamps with np.maximum / np.minimum, which propagate (next test).  The pattern is asserted as it IS, so
# that a change of it — NaN-propagating clamps, in oracle and kernels alike — fails a passing test.
_US, _TS, _QS, _T = "friction_velocity", "temperature_scale", "humidity_scale", "temperature"
NAN_FIELDS = {
    "nan_u": {None: FIVE + (_US,), "ncar": ("x_momentum", "y_momentum")},
    "nan_T": {None: FIVE + (_TS, _QS)},
    "nan_p": {None: FIVE + (_QS,)},
    "nan_q": {None: ()},
    "nan_To": {None: ("sensible_heat", "latent_heat", "water_vapor", _T, _TS, _QS)},
    "nan_So": {None: ("latent_heat", "water_vapor", _QS)},
    "inf_T": {None: ("sensible_heat", "latent_heat", "water_vapor")},
}


@pytest.mark.parametrize("name", ra.NONFINITE)
def test_nonfinite_entries_give_nan_in_exactly_these_fields(name):
    for config in RUN_CONFIGS:
        want = set(NAN_FIELDS[name].get(config, NAN_FIELDS[name][None]))
        for current in ra.CURRENTS:
            out = _c_row(config, current)
            got = {f for f in CELL_FIELDS if np.isnan(out[f][ra.INDEX[name]])}
            assert got == want, (name, config, current, sorted(got ^ want))
    assert {n for n in ra.NONFINITE if set(FIVE) <= set(NAN_FIELDS[n][None])} == {"nan_u", "nan_T", "nan_p"}


def test_nonfinite_entries_poison_the_numpy_restatement_and_nothing_else():
    for config in RUN_CONFIGS:
        c, n = _c_row(config, "rest"), _np_row(config, "rest")
        for name in ra.NONFINITE:
            k = ra.INDEX[name]
            assert all(np.isnan(n[f][k]) for f in FIVE), (config, name)
            if name != "nan_q":
                assert any(np.isnan(c[f][k]) for f in FIVE), (config, name)
        for f in CELL_FIELDS:
            assert np.all(np.isfinite(c[f][ra.FINITE])) and np.all(np.isfinite(n[f][ra.FINITE])), (config, f)


@pytest.mark.parametrize("config", list(util.CONFIGS))
def test_reference_qualifies_on_the_atlas(config):
    """The C and the NumPy restatement alone: identical trip counts on every finite entry, 1e-12, nothing at the cap,
    and the entries with u★ < 1e-8 are the ones the atlas lists."""
    assert set(util.CONFIGS) >= set(RUN_CONFIGS) and "shear_aware" in util.CONFIGS
    assert len(ra.BITS_ONLY) <= 0.01 * ra.A
    held = ra.QUALIFIED
    f, _ = util.CONFIGS[config]()
    sc = getattr(f, "solver_stop_criteria", None)
    cap = None if isinstance(sc, ic.FixedIterations) or isinstance(f, ic.CoefficientBasedFluxes) else sc.maxiter
    for current in ra.CURRENTS:
        c, n = _c_row(config, current), _np_row(config, current)
        differ = [ra.NAMES[i] for i in np.flatnonzero(held & (c["iterations"] != n["iterations"]))]
        assert not differ, (config, current, differ[:5])
        err = _cell_error(n, c)
        worst = int(np.argmax(np.where(held, err, 0.0)))
        print(f"[{config}/{current}] trips {c['iterations'][held].min()} … {c['iterations'][held].max()}, worst {err[worst]:.2e} at {ra.NAMES[worst]}")
        assert err[worst] <= TOL_REFERENCE, (config, current, ra.NAMES[worst], err[worst])
        collapsed = tuple(ra.NAMES[i] for i in np.flatnonzero(held & (c["friction_velocity"] < 1e-8)))
        if cap is not None:
            assert c["iterations"][held].max() < cap, (config, current)
        assert collapsed == tuple(ra.COLLAPSED.get(config, ())), (config, current, collapsed[:5])
    assert sum(len(v) for v in ra.COLLAPSED.values()) <= 0.01 * ra.A


def test_nothing_is_dropped_that_qualifies():
    """regime_atlas.UNQUALIFIED against the oracle: every grid cell that the atlas drops (or keeps as BITS_ONLY) is at the
    cap or collapsed under sea_ice_ncar with the ocean at rest or adrift, and no cell that it keeps is."""
    cells = list(ra.grid_cells())
    shape = (3, len(cells) + 2)
    fails = np.zeros(len(cells), bool)
    for uc, vc in ra.CURRENTS.values():
        full = {f: np.full(shape, cells[0][1][f]) for f in ra.FIELDS}
        for f in ra.FIELDS:
            full[f][1, 1:-1] = [cell[f] for _, cell, _ in cells]
        ocean = dict(T=full["To"], S=full["So"], u=np.full(shape, uc), v=np.full(shape, vc))
        out = _entries(orc.compute_atmosphere_ocean_fluxes(orc.make_grid(len(cells), 1, 1, 1, 0), _params("sea_ice_ncar"), ocean,
                                                           {f: full[f] for f in ra.ATMOS}))
        fails |= (out["iterations"] >= 100) | (out["friction_velocity"] < 1e-8)
    marked = np.array([not qualified for _, _, qualified in cells])
    assert np.array_equal(fails, marked), [cells[i][0] for i in np.flatnonzero(fails != marked)][:5]
    assert marked.sum() == 204 and all(not q for n, _, q in cells if n in ra.BITS_ONLY)


# ---------------------------------------------------------------------------------------------
# seeded defects
# ---------------------------------------------------------------------------------------------
def _no_gustiness_floor(m):
    def scale(fluxes, Jb, dU2, h_bl):
        wstar = fluxes.gustiness_parameter * np.cbrt(np.maximum(Jb, 0.0) * h_bl)
        return np.sqrt(dU2 + wstar * wstar)
    m.setattr(npo, "_wind_speed_scale", scale)


def _stable_psi_at_zero(m):
    psi_m, psi_h = npo.psi_m, npo.psi_h
    m.setattr(npo, "psi_m", lambda name, z: psi_m(name, np.minimum(z, 0.0)))
    m.setattr(npo, "psi_h", lambda name, z: psi_h(name, np.minimum(z, 0.0)))


def _no_calm_guard(m):
    pack = npo._pack_fluxes

    def unguarded(th, A, Ta, Ts, du, dv, us, ts, qq, its, wet, ocean, ocean_properties, W):
        out = pack(th, A, Ta, Ts, du, dv, us, ts, qq, its, wet, ocean, ocean_properties, W)
        us = np.where(wet, us, 0.0)
        with np.errstate(all="ignore"):
            dU = np.sqrt(du * du + dv * dv)
            out["x_momentum"][W], out["y_momentum"][W] = A["rho"] * -us * us * du / dU, A["rho"] * -us * us * dv / dU
        return out
    m.setattr(npo, "_pack_fluxes", unguarded)


def _no_condensate(m):
    m.setattr(npo.Thermo, "partition", lambda self, s: (0.0 * s["T"], 0.0 * s["T"]))


def _no_high_wind_branch(m):
    fluxes = ic.ncar_atmosphere_ocean_fluxes()
    fluxes.transfer_coefficients.high_wind = np.inf
    return dict(fluxes=fluxes)


def _no_charnock_floor(m):
    fluxes = ic.corrected_atmosphere_ocean_fluxes()
    fluxes.momentum_roughness_length.wave_formulation.minimum = -np.inf
    return dict(fluxes=fluxes)


def _absolute_wind(m):
    return dict(absolute_wind=True)


def _keeps_iterating(config, ocean, atmos, h, ring, group=64):
    """A converged cell goes on to the largest trip count among the 64 cells of its group (window order), as a lane would
    that left its loop only on the wave's vote: the restatement's own loop run for that many trips."""
    base = _np_fluxes(config, ocean, atmos, h, ring)
    ny, nx = base["iterations"].shape[0] - 2 * h, base["iterations"].shape[1] - 2 * h
    W = lambda a: util.window(a, h, h, nx, ny, ring)   # noqa: E731 (a view)
    its = W(base["iterations"]).reshape(-1)
    wet = np.ones(its.size, bool) if ocean.get("mask") is None else W(ocean["mask"]).reshape(-1) != 0
    pad = (-its.size) % group
    grouped = np.concatenate([np.where(wet, its, 0), np.zeros(pad, its.dtype)]).reshape(-1, group)
    target = np.repeat(grouped.max(axis=1), group)[:its.size]
    out = {k: v.copy() for k, v in base.items()}
    for n in np.unique(target[wet & (its < target)]):
        fixed = _np_fluxes(config, ocean, atmos, h, ring, fluxes=util._fixed(util.CONFIGS[config]()[0], int(n)))
        sel = (wet & (its < target) & (target == n)).reshape(W(base["iterations"]).shape)
        for k in out:
            W(out[k])[sel] = W(fixed[k])[sel]
    return out


# name: (preset, current, the seeded defect, an entry it moves beyond TOL_SOLVER, whether util.build_case(90, 40) sees it)
DEFECTS = {
    "keeps_iterating_with_its_group": ("default", "rest", None, "grid[U=0.05,dT=0.1,rh=0.5,sst=15]", True),
    "calm_guard_dropped": ("default", "rest", _no_calm_guard, "grid[U=0,dT=-1,rh=0.5,sst=15]", False),
    "condensate_ignored": ("default", "rest", _no_condensate, "grid[U=7,dT=1,rh=1.3,sst=15]", False),
    "high_wind_branch_dropped": ("ncar", "rest", _no_high_wind_branch, "grid[U=80,dT=-1,rh=0.5,sst=15]", False),
    "gustiness_floor_dropped": ("default", "rest", _no_gustiness_floor, "grid[U=1,dT=1,rh=0.5,sst=15]", True),
    "stable_psi_taken_at_zero": ("default", "rest", _stable_psi_at_zero, "grid[U=3,dT=4,rh=0.5,sst=15]", True),
    "absolute_wind_for_relative": ("default", "drift", _absolute_wind, "wind_is_current", True),
    "charnock_floor_removed": ("corrected", "rest", _no_charnock_floor, "grid[U=0.3,dT=-1,rh=0.5,sst=15]", True),
}


@functools.lru_cache(maxsize=None)
def _smooth(config):
    case = util.build_case(90, 40)
    g = orc.make_grid(90, 40, 3, 3, 1)
    at = orc.interpolate_atmosphere_state(g, case["src"], case["weights"], 0, 1, 0.37)
    return case, at, orc.compute_atmosphere_ocean_fluxes(g, _params(config), case["ocean"], at)


@pytest.mark.parametrize("defect", list(DEFECTS))
def test_seeded_defect_moves_a_named_entry(defect, monkeypatch):
    """Each defect, seeded into the NumPy restatement, moves its named entry beyond the GPU bound against the C oracle;
    the ones marked so stay inside the bound on every wet cell of util.build_case(90, 40) — the smooth case cannot see them."""
    config, current, seed, name, smooth_sees = DEFECTS[defect]
    case, at, smooth_ref = _smooth(config)
    W = lambda d: {k: util.window(d[k], 3, 3, 90, 40, 1) for k in CELL_FIELDS}   # noqa: E731
    wet = util.window(case["ocean"]["mask"], 3, 3, 90, 40, 1) != 0
    assert _cell_error(_np_row(config, current, nonfinite=False), _c_row(config, current, False)).max() <= TOL_REFERENCE
    assert _cell_error(W(_np_fluxes(config, case["ocean"], at, 3, 1)), W(smooth_ref))[wet].max() <= TOL_REFERENCE
    with monkeypatch.context() as m:
        if seed is None:
            _, ocean, atmos = _row(current, nonfinite=False)
            on_atlas = _entries(_keeps_iterating(config, ocean, atmos, 1, 0))
            on_smooth = _keeps_iterating(config, case["ocean"], at, 3, 1)
        else:
            kw = seed(m) or {}
            on_atlas = _np_row(config, current, nonfinite=False, **kw)
            on_smooth = _np_fluxes(config, case["ocean"], at, 3, 1, **kw)
    err = _cell_error(on_atlas, _c_row(config, current, False))
    smooth_err = _cell_error(W(on_smooth), W(smooth_ref))[wet].max()
    print(f"[{defect}] atlas: {err[ra.INDEX[name]]:.2e} at {name}, {int((err > TOL_SOLVER).sum())} entries beyond the bound, "
          f"worst {err.max():.2e} at {ra.NAMES[int(err.argmax())]}; build_case(90, 40): {smooth_err:.2e}")
    assert err[ra.INDEX[name]] > TOL_SOLVER, (defect, name, err[ra.INDEX[name]])
    assert (smooth_err > TOL_SOLVER) == smooth_sees, (defect, smooth_err)


def test_at_least_three_defects_are_seen_by_the_atlas_alone():
    assert len(DEFECTS) >= 5 and sum(1 for d in DEFECTS.values() if d[4] is False) >= 3


# =============================================================================================
# GPU
# =============================================================================================
NAN_BITS = np.uint64(0x7FF8000000000000)
RUNS = (("cyclic", "rest", False), ("cyclic", "rest", True), ("blocks", "rest", False), ("blocks", "rest", True),
        ("cyclic", "drift", False))
FROM_SOURCE = ("fused", "certified")     # modes that start from a JRA55 source: the atlas without group (d), through float32
ALL = CELL_FIELDS + ("iterations",)


def _bits(a):
    """The bit patterns of an array, every NaN the same one (NaN compares equal to NaN, everything else by bits)."""
    a = np.ascontiguousarray(a)
    if a.dtype != np.float64:
        return a.astype(np.int64)
    b = a.view(np.uint64).copy()
    b[np.isnan(a)] = NAN_BITS
    return b


def _names(ids, where):
    found = np.unique(ids[where])
    return [ra.NAMES[i] for i in found[:6]] + (["…"] if found.size > 6 else [])


@functools.lru_cache(maxsize=None)
def _inputs(kind, current, land, nonfinite, rounded, shift=0, mask_kind="u8"):
    import mask_atlas as ma
    nx, ny, ids = ra.layout(kind, shift)
    ocean, atmos = ra.fields(kind, current, nonfinite, shift)
    wet = ra.land_mask(kind)[0] if land else np.ones(ids.shape, bool)
    src, w = ra.identity_source(atmos)
    if rounded:
        atmos = ra.through_float32(atmos)
    ocean = dict(ocean, mask=ma.embed(wet, nx, ny, kind=mask_kind, z_surface=ic.flux_params().ocean_surface_z))
    return dict(nx=nx, ny=ny, ids=ids, wet=wet, ocean=ocean, atmos=atmos, src=src, weights=w)


@functools.lru_cache(maxsize=None)
def _oracle(config, kind, current, land, nonfinite, rounded, shift=0):
    """The C oracle on a layout (once per formulation and layout, shared by the bodies and forms)."""
    c = _inputs(kind, current, land, nonfinite, rounded, shift)
    g, params = orc.make_grid(c["nx"], c["ny"], H, H, RING), _params(config)
    fl = orc.compute_atmosphere_ocean_fluxes(g, params, c["ocean"], c["atmos"], nthreads=0)
    net = orc.compute_net_ocean_fluxes(g, params, c["ocean"], c["atmos"], fl, ice=None, weights=c["weights"])
    return dict(fluxes=fl, net=net, atmos=c["atmos"])


def _context(c, params, options=(), solver=abi.SOLVER_TABLES, ring=RING):
    from coflux.runtime import FluxContext
    ctx = FluxContext(c["nx"], c["ny"], H, H, params, ring=ring)
    ctx.set_option(abi.OPT_SOLVER, solver)
    for opt, val in options:
        ctx.set_option(opt, val)
    dev = ctx.to_device
    d = dict(ocean={k: dev(v) for k, v in c["ocean"].items()}, src={k: dev(v) for k, v in c["src"].items()},
             weights={k: (dev(v) if isinstance(v, np.ndarray) else v) for k, v in c["weights"].items()})
    return ctx, d


def _launch(ctx, d, c, mode, calls=1):
    """`calls` runs of one form on fresh sentinel-filled outputs: "fused" / "certified" cf_update_state from the identity
    source, "three" the same in three launches, "unfused" / "hints" solver + net launches on exchange fields set directly."""
    import torch
    runs = []
    for _ in range(calls):
        fl = _sentinel_fields(ctx, CELL_FIELDS, with_iterations=True)
        net = _sentinel_fields(ctx, NET_NAMES)
        if mode in FROM_SOURCE:
            atmos = _sentinel_fields(ctx, EXCHANGE_NAMES)
            ctx.update_state(d["src"], d["weights"], d["ocean"], atmos, fl, net, level1=0, level2=1, time_fraction=0.0)
        else:
            if mode == "three":
                atmos = _sentinel_fields(ctx, EXCHANGE_NAMES)
                ctx.interpolate_atmosphere_state(d["src"], d["weights"], atmos, 0, 1, 0.0)
            else:
                atmos = {k: ctx.to_device(c["atmos"][k]) for k in EXCHANGE_NAMES}
            ctx.compute_atmosphere_ocean_fluxes(d["ocean"], atmos, fl)
            ctx.compute_net_ocean_fluxes(d["ocean"], atmos, fl, net, weights=d["weights"])
        ctx.sync()
        torch.cuda.synchronize()
        runs.append(dict(fluxes=_host(fl), net=_host(net), atmos=_host(atmos)))
    return runs


def _check_source(label, c, got):
    """The interpolation handed out the float32-rounded atlas, bit for bit: the oracle ran on what the solver read."""
    for k in EXCHANGE_NAMES:
        g, r = (util.window(a[k], H, H, c["nx"], c["ny"], RING) for a in (got["atmos"], c["atmos"]))
        assert np.array_equal(_bits(g), _bits(r)), (label, "atmos." + k)


def _known_cells(c, names, ring=RING):
    """(cells, net cells) of the window that carry one of the entries `names`, and the interior cells whose net fluxes
    read one: the face stresses average with the west / south neighbour's ρτ."""
    K = np.isin(c["ids"], [ra.INDEX[n] for n in names])
    east, north = np.zeros_like(K), np.zeros_like(K)
    east[:, 1:], north[1:, :] = K[:, :-1], K[:-1, :]
    cut = (slice(RING - ring, K.shape[0] - (RING - ring)), slice(RING - ring, K.shape[1] - (RING - ring)))
    return K[cut], (K | east | north)[RING:-RING, RING:-RING]


def _check_oracle(label, c, got, ref, *, ring=RING, certified=False, skip=(), only=None):
    """Every window cell written; NaN exactly where the oracle has NaN; land as the oracle's; trip counts the oracle's; wet
    cells of finite entries within TOL_SOLVER; no such cell of the reference at the cap or collapsed (u★ < 1e-8), so no
    looser rule is in use.
    `skip`: entries left out (ra.DEVICE_KNOWN: they have a strict xfail of their own); `only`: nothing but these entries."""
    nx, ny = c["nx"], c["ny"]
    W = lambda a, r=ring: util.window(a, H, H, nx, ny, r)   # noqa: E731
    inner = (slice(RING - ring, c["ids"].shape[0] - (RING - ring)), slice(RING - ring, c["ids"].shape[1] - (RING - ring)))
    ids, wet = c["ids"][inner], c["wet"][inner]
    K, KN = _known_cells(c, only if only is not None else tuple(skip) + ra.BITS_ONLY, ring)
    sel, sel_net = (K, KN) if only is not None else (~K, ~KN)
    # A poisoned cell converges nowhere: the fields that drop its NaN hold whatever the last of 100 trips left, on either
    # side.  Group (d) is held to the oracle's NaN pattern, its trip count and its land — not to those values.
    poisoned, poisoned_net = _known_cells(c, ra.NONFINITE, ring)
    sound, sound_net = ~poisoned, ~poisoned_net
    for k in ALL:
        left = _untouched(W(got["fluxes"][k]))
        assert not left.any(), (label, k, "window cells left unwritten", int(left.sum()), _names(ids, left))
    for k in CELL_FIELDS:
        g, r = W(got["fluxes"][k]), W(ref["fluxes"][k])
        differ = sel & (np.isnan(g) != np.isnan(r))
        assert not differ.any(), (label, k, "NaN where the oracle has none, or the reverse", _names(ids, differ))
        land = sel & ~wet
        assert np.array_equal(g[land], r[land]), (label, k, "land differs from the oracle")
    if not certified:
        it_g, it_r = W(got["fluxes"]["iterations"]), W(ref["fluxes"]["iterations"])
        differ = sel & (it_g != it_r)
        assert not differ.any(), (label, "trip counts", int(differ.sum()), _names(ids, differ),
                                  it_g[differ][:6].tolist(), it_r[differ][:6].tolist())
        held = wet & ra.QUALIFIED[ids]
        assert it_r[held].max() < 100 and W(ref["fluxes"]["friction_velocity"])[held].min() >= 1e-8, label
        for k in CELL_FIELDS:
            g, r = W(got["fluxes"][k]), W(ref["fluxes"][k])
            with np.errstate(invalid="ignore"):
                e = np.abs(g - r) / np.maximum(np.abs(r), util.FIELD_SCALE[k])
            e = np.where(sel & wet & sound & np.isfinite(r), e, 0.0)
            assert e.max() <= TOL_SOLVER, (label, k, float(e.max()), ra.NAMES[ids.reshape(-1)[int(e.argmax())]])
    wet0, ids0 = c["wet"][RING:-RING, RING:-RING], c["ids"][RING:-RING, RING:-RING]
    for k in NET_NAMES:
        g, r = W(got["net"][k], 0), W(ref["net"][k], 0)
        left = _untouched(g)
        assert not left.any(), (label, "net." + k, "interior cells left unwritten", int(left.sum()))
        # NaN on the faces that read a NaN cell's ρτ, as in the oracle; a land cell is exactly zero, also where the oracle's
        # 0 · NaN left a NaN on it
        differ = sel_net & wet0 & (np.isnan(g) != np.isnan(r))
        assert not differ.any(), (label, "net." + k, "NaN where the oracle has none, or the reverse", _names(ids0, differ))
        if certified:
            continue
        with np.errstate(invalid="ignore"):
            e = np.abs(g - r) / np.maximum(np.abs(r), util.FIELD_SCALE[k])
        e = np.where(sel_net & sound_net & np.isfinite(r), e, 0.0)
        assert e.max() <= TOL_SOLVER, (label, "net." + k, float(e.max()), ra.NAMES[ids0.reshape(-1)[int(e.argmax())]])
        if k in ("u", "v", "T", "S"):
            assert not np.any(g[sel_net & ~wet0]), (label, "net." + k, "land takes a flux")


def _canonical(c, fluxes):
    """Per field, the bits of every entry's first wet copy."""
    order, starts = ra.copies(c["ids"], c["wet"])
    return {k: _bits(util.window(fluxes[k], H, H, c["nx"], c["ny"], RING)).reshape(-1)[order[starts]] for k in ALL}


def _check_copies(label, c, fluxes, canon):
    """Position independence: every wet copy of an entry holds the canonical bits, in every cell-local field and in the
    trip count."""
    for k in ALL:
        b = _bits(util.window(fluxes[k], H, H, c["nx"], c["ny"], RING))
        differ = c["wet"] & (b != canon[k][c["ids"]])
        assert not differ.any(), (label, k, "copies of one entry differ", int(differ.sum()), _names(c["ids"], differ))


def _same(label, a, b, groups=("atmos", "fluxes", "net")):
    for grp in groups:
        for k in a[grp]:
            assert np.array_equal(_bits(a[grp][k]), _bits(b[grp][k])), (label, grp + "." + k)


def _known(body, land):
    return tuple(dict.fromkeys(name for name, bodies, lands, _ in ra.DEVICE_KNOWN if body in bodies and land in lands))


@gpu
@pytest.mark.parametrize("body", list(ATLAS_BODIES))
def test_solver_body_on_the_atlas(body):
    """One body on the five runs of the atlas — cyclic and blocks, each all-ocean and under the checkerboard, and cyclic on
    the drifting ocean: the oracle comparison per run (_check_oracle; the certified body keeps compare_certified), then
    position independence within cyclic, between cyclic and blocks, and between the all-ocean runs and their land variants."""
    config, mode, options, solver = ATLAS_BODIES[body]
    source = mode in FROM_SOURCE
    canon = {}
    for kind, current, land in RUNS:
        label = (body, kind, current, "checkerboard" if land else "all_ocean")
        c = _inputs(kind, current, land, not source, source)
        ref = _oracle(config, kind, current, land, not source, source)
        ctx, d = _context(c, _params(config), options, solver)
        runs = _launch(ctx, d, c, mode, calls=3 if mode == "hints" else 1)
        if body == "corrected_line":
            assert ctx.solver_latency_layout(), label
        if mode == "certified":
            assert ctx.solver_iteration_path() == abi.SOLVER_PATH_CERTIFIED
        ctx.close()
        for call, got in enumerate(runs):
            lab = label + (f"call {call}",)
            if source:
                _check_source(lab, c, got)
            _check_oracle(lab, c, got, ref, certified=mode == "certified", skip=_known(body, land))
            if mode == "certified":
                from test_certified import compare_certified
                case = dict(nx=c["nx"], ny=c["ny"], hx=H, hy=H, ocean=c["ocean"])
                compare_certified(case, got, ref, expect_certified=False, max_exact_share=1.0, label=str(lab))
            if call:
                _same(lab, runs[0], got)          # the hints only reorder work
            canon.setdefault(current, _canonical(c, got["fluxes"]))
            _check_copies(lab, c, got["fluxes"], canon[current])


KNOWN_CASES = [(body, name, land, cause) for name, bodies, lands, cause in ra.DEVICE_KNOWN for body in bodies for land in lands]


@gpu
@pytest.mark.parametrize("body,name,land,cause", KNOWN_CASES,
                         ids=[f"{b}-{n}-{'checkerboard' if land else 'all_ocean'}" for b, n, land, _ in KNOWN_CASES])
def test_entries_the_device_is_known_to_miss(body, name, land, cause, request):
    """ra.DEVICE_KNOWN: the oracle comparison on nothing but the cells of one listed entry (and the faces that read its
    stress), cyclic layout, one case per mask.  Strict: a body that comes to agree with the oracle must leave the list."""
    request.applymarker(pytest.mark.xfail(strict=True, raises=AssertionError, reason=cause))
    config, mode, options, solver = ATLAS_BODIES[body]
    assert mode not in FROM_SOURCE and name in ra.NONFINITE
    c = _inputs("cyclic", "rest", land, True, False)
    ctx, d = _context(c, _params(config), options, solver)
    got = _launch(ctx, d, c, mode)[0]
    ctx.close()
    _check_oracle((body, name, land), c, got, _oracle(config, "cyclic", "rest", land, True, False), only=(name,))


FORM_CASES = [(k, land) for k in ("cyclic", "blocks") for land in (False, True)]


@gpu
@pytest.mark.parametrize("kind,land", FORM_CASES, ids=[f"{k}-{'checkerboard' if land else 'all_ocean'}" for k, land in FORM_CASES])
def test_forms_are_bitwise_equal_on_the_atlas(kind, land):
    """The bitwise claims between forms: default_fused == three launches, corrected_line == corrected, the chunk plans
    256 / 512 / 768 == the automatic one, ring 0 == ring 1 on the interior, the bottom-height mask == the byte mask."""
    where = (kind, "checkerboard" if land else "all_ocean")
    # from the source: fused epilogue against three launches, line layout against production
    c = _inputs(kind, "rest", land, False, True)
    for config, forms in (("default", (("fused", ()), ("three", ()))),
                          ("corrected", (("fused", ()), ("fused", ((abi.OPT_LATENCY_LAYOUT, 2),))))):
        ref, outs = _oracle(config, kind, "rest", land, False, True), []
        for mode, options in forms:
            ctx, d = _context(c, _params(config), options)
            outs.append(_launch(ctx, d, c, mode)[0])
            if options:
                assert ctx.solver_latency_layout()
            ctx.close()
        _check_source(where + (config,), c, outs[0])
        _check_oracle(where + (config,), c, outs[0], ref)
        _same(where + (config, forms[1]), outs[0], outs[1])
    # on exchange fields set directly, group (d) included: chunk plans, ring, mask kind
    c = _inputs(kind, "rest", land, True, False)
    ref = _oracle("default", kind, "rest", land, True, False)
    ctx, d = _context(c, _params("default"))
    base = _launch(ctx, d, c, "unfused")[0]
    ctx.close()
    _check_oracle(where + ("automatic plan",), c, base, ref, skip=_known("default", land))
    for chunk in (256, 512, 768):
        ctx, d = _context(c, _params("default"), ((abi.OPT_AO_CHUNK, chunk),))
        _same(where + ("chunk", chunk), base, _launch(ctx, d, c, "unfused")[0], groups=("fluxes", "net"))
        ctx.close()
    ctx, d = _context(c, _params("default"), ring=0)
    ring0 = _launch(ctx, d, c, "unfused")[0]
    ctx.close()
    inner = lambda a: util.window(a, H, H, c["nx"], c["ny"], 0)   # noqa: E731
    for k in ALL:
        assert not _untouched(inner(ring0["fluxes"][k])).any(), (where, "ring 0", k)
        assert np.array_equal(_bits(inner(ring0["fluxes"][k])), _bits(inner(base["fluxes"][k]))), (where, "ring 0", k)
    cz = _inputs(kind, "rest", land, True, False, 0, "bottom_height")
    fluxes, vd = util.CONFIGS["default"]()
    ctx, d = _context(cz, ic.flux_params(fluxes, velocity_difference=vd, mask_kind=abi.MASK_BOTTOM_HEIGHT))
    _same(where + ("bottom height",), base, _launch(ctx, d, cz, "unfused")[0], groups=("fluxes", "net"))
    ctx.close()


STEP_SHIFT = 577       # the second ocean state and the second source level carry the atlas moved on by this many entries
STEP_CASES = [(config, kind, kind == "cyclic") for config in ("default", "ncar") for kind in ("cyclic", "blocks")]


@gpu
@pytest.mark.parametrize("config,kind,land", STEP_CASES, ids=[f"{cfg}-{k}" for cfg, k, _ in STEP_CASES])
def test_time_steps_on_the_atlas_is_the_host_loop_bitwise(config, kind, land):
    """cf_time_steps — plain, pipelined, and with CF_OPT_MERGED_PREFETCH 1 and 2 — == the host loop of cf_update_state
    calls, bit for bit, for the lean body and for ncar.  The clock advances one snapshot per step, so every step interpolates
    at time fraction 0 from the level that goes with its ocean state: even steps carry the atlas, odd steps the atlas moved
    on by STEP_SHIFT entries, and the next step's interpolation rides in this step's launches.  The last step is held to
    the oracle and to position independence like any other run."""
    c, c1 = (_inputs(kind, "rest", land, False, True, shift) for shift in (0, STEP_SHIFT))
    n = 5
    src, _ = ra.identity_source(ra.fields(kind, "rest", False, 0)[1], second=ra.fields(kind, "rest", False, STEP_SHIFT)[1])
    ref = _oracle(config, kind, "rest", land, False, True)
    outs = {}
    for form, (merged, pipeline) in dict(host=(0, None), plain=(0, False), pipelined=(0, True), merged=(1, True), tail=(2, True)).items():
        ctx, d = _context(c, _params(config))
        states = [d["ocean"], dict({k: ctx.to_device(c1["ocean"][k]) for k in ("T", "S", "u", "v")}, mask=d["ocean"]["mask"])]
        dsrc = {k: ctx.to_device(v) for k, v in src.items()}
        fl, net = _sentinel_fields(ctx, CELL_FIELDS, with_iterations=True), _sentinel_fields(ctx, NET_NAMES)
        if pipeline is None:
            last = _sentinel_fields(ctx, EXCHANGE_NAMES)
            for s in range(n):
                ctx.update_state(dsrc, d["weights"], states[s % 2], last, fl, net, level1=s % 2, level2=(s + 1) % 2, time_fraction=0.0)
        else:
            ctx.set_option(abi.OPT_MERGED_PREFETCH, merged)
            sets = [_sentinel_fields(ctx, EXCHANGE_NAMES) for _ in range(2 if pipeline else 1)]
            sched = ctx.make_schedule(states, sets, first_level=0, time_fraction=0.0, time_fraction_increment=1.0, pipeline=pipeline)
            ctx.time_steps(0, 2, sched, dsrc, d["weights"], fl, net)      # in two calls: the step counter carries the clock
            ctx.time_steps(2, n - 2, sched, dsrc, d["weights"], fl, net)
            last = sets[(n - 1) % len(sets)]
        ctx.sync()
        outs[form] = dict(fluxes=_host(fl), net=_host(net), atmos=_host(last))
        ctx.close()
    label = (config, kind, "host loop")
    _check_source(label, c, outs["host"])
    _check_oracle(label, c, outs["host"], ref)
    _check_copies(label, c, outs["host"]["fluxes"], _canonical(c, outs["host"]["fluxes"]))
    for form in ("plain", "pipelined", "merged", "tail"):
        _same((config, kind, form), outs["host"], outs[form])
