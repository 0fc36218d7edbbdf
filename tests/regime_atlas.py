"""Designed surface regimes for the similarity solvers: what one solver cell CARRIES, varied.

The mask atlas varies where the wet cells are, the weight atlas where they read from; on both, every cell holds the smooth
state of util.build_case, where a cell's wave-mates are near copies of it.  Here every entry is one cell's complete input —
atmosphere u, v, T, p, q, Qs, Ql, Mp and ocean T, S — and the two layouts put copies of an entry among wave-mates of every
regime (`cyclic`) or among copies of itself (`blocks`), so that a result which depends on a lane's neighbours shows as a
difference of BITS between copies of one entry.  A plain module: imported by tests/test_regime_atlas.py.

Ocean velocities are face values shared between neighbours, so the current is one uniform vector per run (CURRENTS); the
two `follow` entries take their wind from it."""
import math

import numpy as np

import mask_atlas as ma
from coflux import abi
from coflux import synthetic as syn

RING, HALO = ma.RING, ma.HALO
FIELDS = ("u", "v", "T", "p", "q", "Qs", "Ql", "Mp", "To", "So")   # atmosphere (K, Pa, kg/kg, W/m², kg/m²/s), ocean (°C, psu)
ATMOS = FIELDS[:8]
CURRENTS = {"rest": (0.0, 0.0), "drift": (0.25, -0.15)}

# (a) the regime grid
SPEEDS = (0.0, 1e-9, 0.05, 0.3, 1.0, 3.0, 7.0, 15.0, 30.0, 80.0)                     # m/s, along +x
CONTRASTS = (-15.0, -4.0, -1.0, -0.1, -1e-3, 0.0, 1e-3, 0.1, 1.0, 4.0, 15.0)         # air − sea temperature, K
HUMIDITIES = (0.0, 0.5, 0.98, 1.3)                                                   # of saturation at the air temperature
SSTS = (-1.9, 15.0, 35.0)                                                            # °C
P0, S0, QS0, QL0, MP0 = 101325.0, 35.0, 200.0, 350.0, 3e-5

NONFINITE = ("nan_u", "nan_T", "nan_p", "nan_q", "nan_To", "nan_So", "inf_T")        # (d)

# Grid cells that the reference does not qualify under every preset of util.CONFIGS, per (wind speed, contrast): an `x`
# for each of the twelve (humidity, SST) pairs, humidity-major.  All are calm or weakly windy and stably stratified, and all
# fail under one preset, sea_ice_ncar (Large–Yeager stability functions over constant roughness lengths): there the
# turbulence collapses (u★ < 1e-8, 179 cells at rest and 175 adrift) or the iteration orbits to the cap (16 and 9);
# 204 cells in the union, 15 % of the grid.  Such an entry is dropped from the atlas — except the eleven of BITS_ONLY.
# tests/test_regime_atlas.py::test_nothing_is_dropped_that_qualifies holds this table to the oracle.
UNQUALIFIED = {
    (0.0, -0.001): "..........x.",
    (0.0, 0.0): "..........x.",
    (0.0, 0.001): "..........x.",
    (0.0, 0.1): "........x.xx",
    (0.0, 1.0): "x..xx.xxxxxx",
    (0.0, 4.0): "xx.xxxxxxxxx",
    (0.0, 15.0): "xxxxxxxxxxxx",
    (1e-09, -0.001): "..........x.",
    (1e-09, 0.0): "..........x.",
    (1e-09, 0.001): "..........x.",
    (1e-09, 0.1): "........x.xx",
    (1e-09, 1.0): "x..xx.xxxxxx",
    (1e-09, 4.0): "xx.xxxxxxxxx",
    (1e-09, 15.0): "xxxxxxxxxxxx",
    (0.05, -0.001): "..........x.",
    (0.05, 0.0): "..........x.",
    (0.05, 0.001): "..........x.",
    (0.05, 0.1): "........x.xx",
    (0.05, 1.0): "x..xx.xxxxxx",
    (0.05, 4.0): "xx.xxxxxxxxx",
    (0.05, 15.0): "xxxxxxxxxxxx",
    (0.3, -0.001): "..........x.",
    (0.3, 0.0): "..........x.",
    (0.3, 0.001): "..........x.",
    (0.3, 0.1): "..........xx",
    (0.3, 1.0): "x..xx.xxxxxx",
    (0.3, 4.0): "xx.xxxxxxxxx",
    (0.3, 15.0): "xxxxxxxxxxxx",
    (1.0, 1.0): "x..x..xxxxxx",
    (1.0, 4.0): "xx.xxxxxxxxx",
    (1.0, 15.0): "xxxxxxxxxxxx",
    (3.0, 4.0): "x..x..xxxxxx",
    (3.0, 15.0): "xxxxxxxxxxxx",
    (7.0, 15.0): "........x..x",
}
# Entries the two CPU restatements do not qualify (see above), kept for position independence only: at most 1 % of the
# atlas.  One per regime that the thinning would otherwise remove from the layouts' wave-mates.
BITS_ONLY = ("grid[U=0,dT=0.1,rh=1.3,sst=35]", "grid[U=0,dT=1,rh=0.98,sst=15]", "grid[U=0,dT=15,rh=0.5,sst=15]",
             "grid[U=1e-09,dT=4,rh=0.98,sst=15]", "grid[U=0.05,dT=4,rh=0.5,sst=15]", "grid[U=0.05,dT=15,rh=0.98,sst=15]",
             "grid[U=0.3,dT=1,rh=0.5,sst=15]", "grid[U=0.3,dT=4,rh=0.98,sst=15]", "grid[U=1,dT=4,rh=0.98,sst=-1.9]",
             "grid[U=1,dT=15,rh=0.5,sst=15]", "grid[U=3,dT=15,rh=0.98,sst=15]")
# Entries whose oracle u★ < 1e-8 under some preset (the ψ tables' clamp, util.compare_ice_fluxes' `collapsed` rule), by preset.
COLLAPSED = {}
# Entries a device body is known to treat unlike the oracle, with the cause read from the kernel code:
# (entry, bodies, masks — False all-ocean, True checkerboard —, cause).  Such an entry is left out of that body's oracle
# comparison under those masks (never out of position independence) and carries a strict xfail of its own,
# tests/test_regime_atlas.py::test_entries_the_device_is_known_to_miss.
_DIRECT = ("default", "corrected", "ncar", "constant_roughness", "fixed5", "default_libm", "default_hints", "corrected_wind",
           "shear_aware")
DEVICE_KNOWN = (
    ("inf_T", tuple(b for b in _DIRECT if b != "default_libm"), (False, True),
     "an infinite air temperature.  The oracle divides: rho = p / (R_m T) = 0, so its stress is -0.0 and its q* = -inf.  The "
     "table kernels multiply by a Newton-refined reciprocal in the cell set-up: frcp(Ta) in coflux_fast.hpp / "
     "coflux_solver.hip is r = rcp(inf) = 0, then r + r (1 - Ta r) with Ta r = inf * 0 = NaN; coflux_lean.hpp shares one "
     "reciprocal, frcp1(Ta * Ts), and forms 1 / Ts = rT * Ta = 0 * inf.  So 1 / Ta, rho and with them the stress and q* are "
     "NaN.  The libm kernel divides and agrees with the oracle.  Keeping 1 / inf = 0 means a select on the refined value in "
     "the fast kernel and two reciprocals in place of the shared one in the lean kernel's set-up: the flagship's path."),
)


def _cell(speed=7.0, dT=-1.0, rh=0.8, sst=15.0, *, u=None, v=0.0, p=P0, S=S0, q=None, Qs=QS0, Ql=QL0, Mp=MP0):
    Ta = sst + 273.15 + dT
    return dict(u=speed if u is None else u, v=v, T=Ta, p=p, q=rh * float(syn._qsat_tetens(Ta, p)) if q is None else q,
                Qs=Qs, Ql=Ql, Mp=Mp, To=sst, So=S)


def grid_cells():
    """Yields (name, cell, qualified) over the whole regime grid, dropped cells included."""
    for s in SPEEDS:
        for d in CONTRASTS:
            marks = UNQUALIFIED.get((s, d), "." * 12)
            for i, r in enumerate(HUMIDITIES):
                for j, t in enumerate(SSTS):
                    yield f"grid[U={s:g},dT={d:g},rh={r:g},sst={t:g}]", _cell(s, d, r, t), marks[3 * i + j] == "."


def _build():
    out = [(name, cell, None) for name, cell, qualified in grid_cells() if qualified or name in BITS_ONLY]
    # (b) kinematics: the eight octants at 7 m/s, and the wind tied to the run's current
    tail = []
    for k in range(8):
        c, s = math.cos(k * math.pi / 4), math.sin(k * math.pi / 4)
        c, s = (round(c), round(s)) if k % 2 == 0 else (c, s)     # the axis-aligned directions carry an exact zero
        tail.append((f"octant{k * 45}", _cell(u=7.0 * c, v=7.0 * s), None))
    tail.append(("wind_is_current", _cell(u=0.0, v=0.0), 1.0))
    tail.append(("wind_opposes_current", _cell(u=0.0, v=0.0), -1.0))
    # (c) composition and thermodynamic edges
    for S in (0.0, 45.0):
        tail.append((f"S={S:g}", _cell(S=S), None))
    for p in (50000.0, 108000.0):
        tail.append((f"p={p:g}", _cell(p=p), None))
    for d in (-15.0, 15.0):
        tail.append((f"q=0,dT={d:g}", _cell(dT=d, q=0.0), None))
    tail.append(("radiation_zero", _cell(Qs=0.0, Ql=0.0, Mp=0.0), None))
    tail.append(("radiation_large", _cell(Qs=1200.0, Ql=500.0, Mp=5e-3), None))
    # (d) non-finite inputs, one field at a time — each between two finite entries of (b) and (c), so that in both layouts
    # the faces that read a non-finite cell's stress belong to finite entries, never to another entry of (d)
    for k, name in enumerate(NONFINITE):
        kind, field = name.split("_")
        cell = _cell()
        cell[field] = math.nan if kind == "nan" else math.inf
        tail.insert(3 * k + 2, (name, cell, None))
    out += tail
    k = 0
    while math.gcd(len(out), 64) != 1:                             # a length coprime to 64: copies land in every lane
        out.append((f"pad{k}", _cell(), None))
        k += 1
    return out


_ENTRIES = _build()
NAMES = tuple(n for n, _, _ in _ENTRIES)
INDEX = {n: k for k, n in enumerate(NAMES)}
A = len(NAMES)
GROUPS = dict(grid=tuple(n for n in NAMES if n.startswith("grid[")),
              kinematics=tuple(n for n in NAMES if n.startswith(("octant", "wind_"))),
              edges=tuple(n for n in NAMES if n.startswith(("S=", "p=", "q=0", "radiation_"))),
              nonfinite=NONFINITE, pad=tuple(n for n in NAMES if n.startswith("pad")))
FINITE = np.array([n not in NONFINITE for n in NAMES])
QUALIFIED = FINITE & np.array([n not in BITS_ONLY for n in NAMES])


def table(current="rest", nonfinite=True):
    """dict field → float64 [A]: every entry's input under a run's current.  nonfinite=False: group (d) holds the pad
    cell instead (the forms that start from a float32 source), so the atlas keeps its length."""
    uc, vc = CURRENTS[current]
    cols = {f: np.empty(A) for f in FIELDS}
    for k, (name, cell, follow) in enumerate(_ENTRIES):
        if not nonfinite and name in NONFINITE:
            cell = _cell()
        for f in FIELDS:
            cols[f][k] = cell[f]
        if follow is not None:
            cols["u"][k], cols["v"][k] = follow * uc + 0.0, follow * vc + 0.0
    return cols


def layout(kind, shift=0, a=None):
    """(nx, ny, ids): `ids` an int [wy, wx] array over the ring-inclusive window, row-major = the solver's index order,
    the atlas entry each window cell carries.  "cyclic": cell n carries entry n mod A on the mask atlas' base shape (about
    four copies, each in another lane, batch and chunk).  "blocks": entry (n // 64) mod A — every aligned run of 64 cells,
    a whole wave, is one entry; the window is the smallest 323-wide one that holds 64 · A cells.  `shift` moves every entry
    that many places on (the second state of a stepped run).  `a`: the length of another atlas that shares the layouts
    (tests/interface_atlas.py); this one's by default."""
    a = A if a is None else a
    if kind == "cyclic":
        nx, ny = ma.SHAPES["base"]
    else:
        assert kind == "blocks"
        nx = 321
        ny = -(-64 * a // (nx + 2 * RING)) - 2 * RING
    wx, wy = ma.window_shape(nx, ny, RING)
    n = np.arange(wx * wy).reshape(wy, wx)
    return nx, ny, ((n if kind == "cyclic" else n // 64) + shift) % a


def land_mask(kind, variant="checkerboard", a=None):
    """The window's wet cells of a layout's land variant (a mask atlas mask) and its halo-inclusive uint8 array."""
    nx, ny, ids = layout(kind, a=a)
    (_, wet), = ma.atlas(ids.shape[1], ids.shape[0], only=(variant,))
    return wet, ma.embed(wet, nx, ny)


def fields(kind, current="rest", nonfinite=True, shift=0):
    """(ocean, atmos): halo-inclusive float64 arrays of a layout.  Outside the window every cell is the pad cell; the
    ocean velocity is the run's current on every face."""
    nx, ny, ids = layout(kind, shift)
    cols = table(current, nonfinite)
    shape = (ny + 2 * HALO, nx + 2 * HALO)
    win = (slice(HALO - RING, HALO + ny + RING), slice(HALO - RING, HALO + nx + RING))
    pad = _cell()
    full = {}
    for f in FIELDS:
        full[f] = np.full(shape, pad[f])
        full[f][win] = cols[f][ids]
    uc, vc = CURRENTS[current]
    ocean = dict(T=full["To"], S=full["So"], u=np.full(shape, uc), v=np.full(shape, vc))
    return ocean, {f: full[f] for f in ATMOS}


def identity_source(atmos, second=None):
    """A two-level float32 JRA55 source and the separable weight map (integer fractional indices; the caller passes time
    fraction 0) under which the interpolation hands out `atmos` — as far as float32 holds it.  Level 1 holds `second`, or
    level 0 negated: with time fraction 0 it carries weight exactly 0."""
    ny, nx = atmos["T"].shape
    take = dict(uas="u", vas="v", tas="T", psl="p", huss="q", rsds="Qs", rlds="Ql", prra="Mp")
    src = {}
    for var in abi.JRA55_VARIABLES:
        if var in take:
            first = atmos[take[var]].astype(np.float32)
            other = -first if second is None else second[take[var]].astype(np.float32)
        else:
            first = other = np.zeros((ny, nx), np.float32)
        src[var] = np.ascontiguousarray(np.stack([first, other]))
    w = dict(separable=True, fi=np.arange(nx, dtype=np.float64), fj=np.arange(ny, dtype=np.float64), latitude=np.zeros(ny))
    return src, w


def through_float32(atmos):
    """What the identity source hands out: every exchange field rounded to float32 (rain + snow = Mp + 0)."""
    return {k: v.astype(np.float32).astype(np.float64) for k, v in atmos.items()}


def copies(ids, wet=None, a=None):
    """(order, starts): window cells (flat indices, wet ones only) sorted by the entry they carry, and where each entry's
    run starts — np.split(order, starts[1:]) lists every entry's copies."""
    flat = ids.reshape(-1)
    cells = np.arange(flat.size) if wet is None else np.flatnonzero(wet.reshape(-1))
    order = cells[np.argsort(flat[cells], kind="stable")]
    starts = np.searchsorted(flat[order], np.arange(A if a is None else a))
    return order, starts
