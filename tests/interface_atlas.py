"""Designed ice regimes for the atmosphere–sea-ice interface solve: what one cell of cf_compute_atmosphere_sea_ice_fluxes
CARRIES, varied.

The regime atlas (tests/regime_atlas.py) does this for the ocean solves; its sea_ice_* presets are ocean solves with sea-ice
stability functions, not the skin-temperature iteration.  Here every entry is one cell's complete input to ice_iterate /
ice_iterate_lean — atmosphere u, v, T, p, q, Qs, Ql, ocean salinity, and the sea-ice state: thickness, carried skin
temperature, concentration, drift and albedo — and the regime atlas' two layouts (`cyclic`: every entry in four or five
places, each in another lane, among wave-mates of every regime; `blocks`: whole waves of one entry) put copies of it where a
result that depends on a lane's neighbours shows as a difference of BITS.  A plain module of data and layouts: imported by
tests/test_interface_atlas.py.

(a) the grid: wind × air temperature × humidity × thickness × carried skin × radiation, 1152 entries, ice at rest,
    concentration 0.9;
(b) named edge entries, one branch of the iteration each: the ±ΔT_max limiter, the melting cap, the consolidation thickness,
    calm and co-moving air, a zero buoyancy scale, open water, non-finite inputs."""
import math

import numpy as np

import numpy_oracle as npo
import regime_atlas as ra
from coflux import interface_computations as ic
from coflux import synthetic as syn

RING, HALO = ra.RING, ra.HALO
ATMOS = ("u", "v", "T", "p", "q", "Qs", "Ql", "Mp")                    # K, Pa, kg/kg, W/m², kg/m²/s
ICE = ("h", "Ts", "conc", "ui", "vi", "alb")                          # m, °C, –, m/s, m/s, –
FIELDS = ATMOS + ("So",) + ICE
P0, S0, ALBEDO0, CONC0, MP0 = 1e5, 34.0, 0.7, 0.9, 0.0
OCEAN_T = -1.8                                                        # °C: the interface solve does not read it

SPEEDS = (0.0, 0.3, 3.0, 8.0, 15.0, 30.0)                              # m/s, along +x
AIR = (235.0, 262.0, 272.5, 280.0)                                    # K
HUMIDITIES = (0.3, 1.0)                                               # of saturation at the air temperature
THICKNESSES = (0.0, 0.02, 0.3, 3.0)                                   # m: none, below, above and far above consolidation
SKINS = (-40.0, -1.0, 0.0)                                            # °C, carried from the step before
RADIATION = {"dark": (0.0, 150.0), "sunlit": (300.0, 320.0)}          # (Qs, Ql)

_PROPS = ic.SeaIceInterfaceProperties()
DT_MAX, T_MELT, H_MIN = _PROPS.maximum_temperature_change, _PROPS.freshwater_melting_temperature, _PROPS.consolidation_thickness
_TH = npo.Thermo(ic.AtmosphereThermodynamicsParameters())
_G, _HREF, _SIGMA = 9.81, 10.0, 5.67e-8

NONFINITE = ("nan_T", "nan_q", "nan_Qs", "nan_h", "nan_Ts", "inf_T")
# (ℵ, h): only the first two are open water to CF_OPT_ICE_FREE_CELLS = CF_ICE_FREE_ZERO (ℵ == 0 and h == 0); the others are solved
OPEN_WATER = {"open[conc=0,h=0]": (0.0, 0.0), "open[conc=-0,h=0]": (-0.0, 0.0), "open[conc=0,h=0.3]": (0.0, 0.3),
              "open[conc=0.9,h=0]": (0.9, 0.0)}
SKIPPED_WHEN_ICE_FREE = ("open[conc=0,h=0]", "open[conc=-0,h=0]")


def _cell(U=8.0, Ta=262.0, rh=0.8, h=0.3, Ts=-10.0, rad="dark", *, u=None, v=0.0, p=P0, q=None, Qs=None, Ql=None, S=S0,
          conc=CONC0, ui=0.0, vi=0.0, alb=ALBEDO0):
    qs, ql = RADIATION[rad]
    return dict(u=U if u is None else u, v=v, T=Ta, p=p, q=rh * float(syn._qsat_tetens(Ta, p)) if q is None else q,
                Qs=qs if Qs is None else Qs, Ql=ql if Ql is None else Ql, Mp=MP0, So=S, h=h, Ts=Ts, conc=conc, ui=ui, vi=vi,
                alb=alb)


def _air(cell):
    """(ρ, c_p, ℒ_s) of a cell's air, as every restatement forms them."""
    A = _TH.state_pTq(cell["p"], cell["T"], cell["q"])
    return float(A["rho"]), float(_TH.cp_m(A)), _TH.Ls0 + (_TH.cpv - _TH.cpi) * (cell["T"] - _TH.T0)


def first_explicit_step(cell):
    """T★ − Tₛ of the explicit balance on the first trip (the scales still at their start value 1e-4): the same in every preset."""
    rho, cp, Ls = _air(cell)
    Ti = T_MELT - _PROPS.liquidus_slope * cell["So"]
    Ts = cell["Ts"] + _PROPS.temperature_offset
    hk = max(cell["h"], H_MIN) / _PROPS.conductivity
    Q = -rho * 1e-4 * (Ls * 1e-4 + cp * 1e-4) + (-(1 - cell["alb"]) * cell["Qs"] - _PROPS.emissivity * cell["Ql"]) \
        + _PROPS.emissivity * _SIGMA * Ts ** 4
    return Ti - hk * Q - Ts


def _skin_one_limit_below_balance():
    """The carried skin whose first explicit step is ΔT_max, to the last bit bisection can reach."""
    lo, hi = -40.0, 0.0                       # the step falls as the skin warms
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if mid in (lo, hi):
            break
        if first_explicit_step(_cell(h=0.3, Ts=mid)) > DT_MAX:
            lo = mid
        else:
            hi = mid
    return hi                                 # the first skin whose step is NOT limited: T★ − Tₛ ≤ ΔT_max


NEUTRAL_SKIN = 255.0                          # K: what the first, limited trip of `neutral` leaves (250 + ΔT_max)


def _neutral():
    """θ_a = Tₛ and q_a = q_s after the first trip: that trip is pinned at +ΔT_max (250 K → 255 K exactly under every scheme),
    so both differences are exact zeros, the scales θ★ = q★ = 0 and the SECOND trip's buoyancy scale b★ == 0.  (On the first
    trip b★ is formed from the start values 1e-4 and cannot vanish.)"""
    cell = _cell(U=8.0, Ta=254.9, h=3.0, rad="sunlit", q=1e-3)
    carried = float(np.float64(250.0) - _PROPS.temperature_offset)
    while carried + _PROPS.temperature_offset != 250.0:
        carried = math.nextafter(carried, 0.0)
    cell["Ts"] = carried
    for _ in range(50):
        A = _TH.state_pTq(cell["p"], cell["T"], cell["q"])
        rho, cp = float(A["rho"]), float(_TH.cp_m(A))
        q = float(_TH.svp(NEUTRAL_SKIN, _TH.Ls0, _TH.cpv - _TH.cpi) / (rho * _TH.Rv * NEUTRAL_SKIN))
        T = NEUTRAL_SKIN - _G * _HREF / cp
        for _ in range(8):                    # the last bits: θ_a is formed as T + g h / c_p
            r = T + _G * _HREF / cp - NEUTRAL_SKIN
            if r == 0.0:
                break
            T = math.nextafter(T, -math.inf if r > 0 else math.inf)
        if (q, T) == (cell["q"], cell["T"]):
            break
        cell["q"], cell["T"] = q, T
    return cell


def _build():
    out = []
    for U in SPEEDS:
        for Ta in AIR:
            for rh in HUMIDITIES:
                for h in THICKNESSES:
                    for Ts in SKINS:
                        for rad in RADIATION:
                            out.append((f"grid[U={U:g},Ta={Ta:g},rh={rh:g},h={h:g},Ts={Ts:g},rad={rad}]", _cell(U, Ta, rh, h, Ts, rad)))
    edge = []
    # the limiter: thick ice, so that the explicit step is large
    edge.append(("limiter[up]", _cell(Ta=272.5, h=3.0, Ts=-40.0, rad="sunlit")))          # heating: the first trips at +ΔT_max
    edge.append(("limiter[down]", _cell(Ta=235.0, h=3.0, Ts=-1.0, rad="dark")))           # cooling: the first trips at −ΔT_max
    edge.append(("limiter[exact]", _cell(h=0.3, Ts=_skin_one_limit_below_balance())))     # exactly ΔT_max below its balance
    # the melting cap
    edge.append(("cap[carried]", _cell(Ta=280.0, rh=1.0, h=0.3, Ts=0.0, rad="sunlit", Qs=600.0)))   # at 0 °C already, strong heating
    edge.append(("cap[touch_and_leave]", _cell(U=15.0, Ta=250.0, rh=0.3, h=3.0, Ts=-3.0, rad="sunlit", Qs=CAP_TOUCH_QS)))
    edge.append(("cap[just_missed]", _cell(U=3.0, Ta=272.5, rh=1.0, h=0.3, Ts=-1.0, rad="sunlit", Qs=CAP_MISSED_QS)))
    edge.append(("cap[just_reached]", _cell(U=3.0, Ta=272.5, rh=1.0, h=0.3, Ts=-1.0, rad="sunlit", Qs=CAP_REACHED_QS)))
    # thickness about the consolidation thickness (h/k against hk_min)
    for tag, h in (("0", 0.0), ("-0", -0.0), ("tiny_negative", -1e-300), ("consolidation", H_MIN),
                   ("consolidation-ulp", math.nextafter(H_MIN, 0.0)), ("consolidation+ulp", math.nextafter(H_MIN, 1.0))):
        edge.append((f"h[{tag}]", _cell(h=h)))
    # kinematics
    edge.append(("drift[with_wind]", _cell(u=5.0, v=3.0, ui=5.0, vi=3.0)))    # dU = 0 under RelativeVelocity only
    edge.append(("wind[-x]", _cell(u=-8.0)))
    edge.append(("wind[+y]", _cell(u=0.0, v=8.0)))
    edge.append(("wind[-y]", _cell(u=0.0, v=-8.0)))
    edge.append(("wind[diagonal]", _cell(u=8.0 * math.sqrt(0.5), v=-8.0 * math.sqrt(0.5))))
    edge.append(("albedo[0]", _cell(rad="sunlit", alb=0.0)))
    edge.append(("albedo[1]", _cell(rad="sunlit", alb=1.0)))
    edge.append(("neutral", _neutral()))
    for name, (conc, h) in OPEN_WATER.items():
        edge.append((name, _cell(conc=conc, h=h)))
    # non-finite inputs, one field at a time, each between finite entries
    for k, name in enumerate(NONFINITE):
        kind, field = name.split("_")
        cell = _cell()
        cell[field] = math.nan if kind == "nan" else math.inf
        edge.insert(3 * k + 2, (name, cell))
    out += edge
    k = 0
    while math.gcd(len(out), 64) != 1:        # a length coprime to 64: copies land in every lane
        out.append((f"pad{k}", _cell()))
        k += 1
    return out


# Shortwave (W/m², albedo 0.7).  The last two are neighbouring doubles found by bisection on the NumPy restatement
# (sea_ice_corrected, linearised scheme): under the first the skin ends one ulp below 0 °C, under the second on the cap.
# tests/test_interface_atlas.py::test_entries_have_the_property_they_are_named_for holds all three to what their names say.
CAP_TOUCH_QS, CAP_MISSED_QS, CAP_REACHED_QS = 600.0, 45.85665534031542, 45.85665534031543

_ENTRIES = _build()
NAMES = tuple(n for n, _ in _ENTRIES)
INDEX = {n: k for k, n in enumerate(NAMES)}
A = len(NAMES)
FINITE = np.array([n not in NONFINITE for n in NAMES])
EDGE_FAMILIES = {fam: tuple(n for n in NAMES if n.startswith(fam)) for fam in ("limiter[", "cap[", "h[", "drift[", "wind[",
                                                                                 "albedo[", "neutral", "open[")}
EDGE_FAMILIES["nonfinite"] = NONFINITE
GRID = tuple(n for n in NAMES if n.startswith("grid["))
# the groups of grid entries every run must keep some qualified members of
GROUPS = {key: tuple(n for n in GRID if tag in n) for key, tag in (
    ("U=0", "[U=0,"), ("U=30", "[U=30,"), ("Ta=235", ",Ta=235,"), ("Ta=280", ",Ta=280,"), ("h=0", ",h=0,"), ("h=0.02", ",h=0.02,"),
    ("h=3", ",h=3,"), ("Ts=-40", ",Ts=-40,"), ("Ts=0", ",Ts=0,"), ("sunlit", "rad=sunlit"), ("dark", "rad=dark"))}


def table(nonfinite=True):
    """dict field → float64 [A]: every entry's input.  nonfinite=False: the non-finite entries hold the pad cell instead (the
    forms that start from a float32 source), so the atlas keeps its length."""
    cols = {f: np.empty(A) for f in FIELDS}
    for k, (name, cell) in enumerate(_ENTRIES):
        if not nonfinite and name in NONFINITE:
            cell = _cell()
        for f in FIELDS:
            cols[f][k] = cell[f]
    return cols


def layout(kind, shift=0):
    """regime_atlas.layout for this atlas' length."""
    return ra.layout(kind, shift, a=A)


def land_mask(kind, variant="checkerboard"):
    return ra.land_mask(kind, variant, a=A)


def copies(ids, wet=None):
    return ra.copies(ids, wet, a=A)


def state(cols, ids, shape, win):
    """(ocean, atmos, ice_state) halo-inclusive float64 arrays with `cols[ids]` on the window `win` and the pad cell outside;
    the ocean is at rest and has no mask."""
    pad = _cell()
    full = {}
    for f in FIELDS:
        full[f] = np.full(shape, pad[f])
        full[f][win] = cols[f][ids]
    ocean = dict(T=np.full(shape, OCEAN_T), S=full["So"], u=np.zeros(shape), v=np.zeros(shape))
    ice = dict(thickness=full["h"], top_temperature=full["Ts"], concentration=full["conc"], u=full["ui"], v=full["vi"],
               albedo=full["alb"])
    return ocean, {f: full[f] for f in ATMOS}, ice


def fields(kind, nonfinite=True, shift=0):
    """(nx, ny, ids, ocean, atmos, ice_state) of a layout."""
    nx, ny, ids = layout(kind, shift)
    shape = (ny + 2 * HALO, nx + 2 * HALO)
    win = (slice(HALO - RING, HALO + ny + RING), slice(HALO - RING, HALO + nx + RING))
    return (nx, ny, ids) + state(table(nonfinite), ids, shape, win)


def row(nonfinite=True):
    """The atlas as one row of cells (ring 0, halo 1): (ocean, atmos, ice_state); entry k sits at [1, 1 + k]."""
    shape = (3, A + 2)
    return state(table(nonfinite), np.arange(A)[None, :], shape, (slice(1, 2), slice(1, A + 1)))
