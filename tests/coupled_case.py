"""The designed case of the coupled step loop (cf_prepare_coupled_step, cf_time_steps_coupled).

synthetic.ocean_state has no cell below freezing (T ≥ −1.8 °C while T_f = −0.054 S ≤ −1.69 °C and mostly near −1.9 °C), so on
util.build_case alone the frazil branch and "the exchange sees T_o = T_f" never run.  This case starts from build_case and
plants cells of six classes, cycling through them inside aligned runs of 64 interior cells (a wave of the interior kernels), so
that every class has wave-mates of the others:

    supercooled_ice    wet, T < T_f, ℵ > 0         frazil, then the exchange at T_o = T_f
    supercooled_open   wet, T < T_f, ℵ = 0         frazil alone
    warm_ice           wet, T ≥ T_f, ℵ > 0         the three-equation exchange, no frazil
    open_water         wet, T ≥ T_f, ℵ = 0         zeros from a wet cell
    fresh              wet, S < ocean_minimum_salinity
    land               mask = 0

Both ice–ocean stresses are non-zero everywhere, the east halo column and the north halo row included; the land source is
non-zero on the source nodes the coastal cells interpolate from.  Two ocean states, three ice states (the second and third
differ in ℵ on the planted cells), and two clocks that cross their level boundaries at different steps of the twelve.

NumPy only up to `Device`: tests/test_coupled_steps_cpu.py holds the case to its own description without a GPU."""
import numpy as np

import util
from coflux import synthetic as syn

CLASSES = ("supercooled_ice", "supercooled_open", "warm_ice", "open_water", "fresh", "land")
MIN_SALINITY = 5.0      # ocean_minimum_salinity of the case's flux parameters
LIQUIDUS = 0.054        # cf_default_ice_ocean_params.liquidus_slope
N_STEPS = 12
LAND_CLOCK = dict(first_level=1, n_levels=3, fraction=0.8, increment=1.0 / 9.0)
ATMOS_CLOCK = dict(first_level=0, n_levels=4, fraction=0.0, increment=1.0 / 9.0)
PISTON_VELOCITY = 1.0 / 6.0 / 86400.0
ICE_OCEAN_TIME_STEP = 1200.0


def clock_levels(clock, steps=N_STEPS, first_step=0):
    """(level1, level2, fraction) per step by cf_time_steps' arithmetic: total = fraction + step · increment."""
    out = []
    for s in range(first_step, first_step + steps):
        total = clock["fraction"] + float(s) * clock["increment"]
        whole = np.floor(total)
        l1 = int((clock["first_level"] + int(whole)) % clock["n_levels"])
        out.append((l1, (l1 + 1) % clock["n_levels"], float(total - whole)))
    return out


def crossings(clock, steps=N_STEPS):
    """The steps at which the clock's first level differs from the previous step's."""
    lv = [l[0] for l in clock_levels(clock, steps)]
    return [s for s in range(1, steps) if lv[s] != lv[s - 1]]


def planted_runs(nx, ny):
    """The aligned runs [64 r, 64 r + 64) of interior cells (index j · nx + i) that are planted: every third whole run."""
    whole = (nx * ny) // 64
    return [r for r in range(whole) if r % 3 == 1] or [0]


def _plant(T, S, mask, conc, thickness, nx, ny, hx, hy, variant):
    """Writes the six classes into the planted runs; `variant` 0, 1, 2 moves the planted values a little (the second ocean
    state, the second and third ice state)."""
    for r in planted_runs(nx, ny):
        for n in range(64):
            idx = 64 * r + n
            j, i = divmod(idx, nx)
            c = (j + hy, i + hx)
            cls = n % 6
            jitter = 0.01 * (n % 7) + 0.003 * variant
            if mask is not None:
                mask[c] = 0 if cls == 5 else 1
            salt = 0.5 * MIN_SALINITY if cls == 4 else 34.0 + jitter
            tf = -LIQUIDUS * salt
            if S is not None:
                S[c] = salt
            if T is not None:
                T[c] = (tf - 0.3 - jitter) if cls in (0, 1) else (tf + 0.8 + jitter if cls == 2 else 2.0 + jitter)
            if conc is not None:
                base = {0: 0.6, 1: 0.0, 2: 0.8, 3: 0.0, 4: 0.3, 5: 0.5}[cls]
                if variant == 1:
                    base *= 0.5
                elif variant == 2:   # the open supercooled cells freeze over, the icy ones open
                    base = {0: 0.0, 1: 0.2, 2: 0.4, 3: 0.0, 4: 0.0, 5: 0.5}[cls]
                conc[c] = base
            if thickness is not None and cls in (1, 3):
                thickness[c] = 0.0


def classify(ocean, conc):
    """Boolean halo-inclusive arrays per class, from the fields alone (not from where cells were planted)."""
    wet = ocean["mask"] != 0
    cold = ocean["T"] < -LIQUIDUS * ocean["S"]
    fresh = ocean["S"] < MIN_SALINITY
    return dict(supercooled_ice=wet & cold & (conc > 0) & ~fresh, supercooled_open=wet & cold & (conc == 0) & ~fresh,
                warm_ice=wet & ~cold & (conc > 0) & ~fresh, open_water=wet & ~cold & (conc == 0) & ~fresh, fresh=wet & fresh,
                land=~wet)


def build(nx, ny, hx, hy, weights="latlon"):
    """The case as host arrays: ocean states, ice states, stresses, weights (negative fractional indices present), sources."""
    case = util.build_case(nx, ny, hx, hy, weights=weights, n_levels=ATMOS_CLOCK["n_levels"])
    o0 = {k: np.array(case["ocean"][k]) for k in ("T", "S", "u", "v", "mask")}
    o1 = syn.evolved_ocean_state(case["ocean"], nx, ny, hx, hy, 1)
    o1 = {k: np.array(o1[k]) for k in ("T", "S", "u", "v", "mask")}
    si = {k: np.array(v) for k, v in case["ice_state"].items()}
    conc = [np.array(case["ocean"]["ice_concentration"]) for _ in range(3)]
    conc[1] = np.clip(conc[1] * 0.9, 0.0, 1.0)
    conc[2] = np.clip(conc[2] * 1.05, 0.0, 1.0)
    _plant(o0["T"], o0["S"], o0["mask"], conc[0], si["thickness"], nx, ny, hx, hy, 0)
    _plant(o1["T"], o1["S"], None, conc[1], None, nx, ny, hx, hy, 1)
    _plant(None, None, None, conc[2], None, nx, ny, hx, hy, 2)
    o1["mask"] = o0["mask"]
    i, j = syn.ocean_indices(nx, ny, hx, hy)
    tx = 2e-5 * (syn.normal("txio", i, j) + 0.25)
    ty = 2e-5 * (syn.normal("tyio", i, j) - 0.25)
    w = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in case["weights"].items()}
    # the first interior column lies west of the first source node: negative fractional indices
    w["fi"] = w["fi"] - (0.37 + (w["fi"][hx] if w["separable"] else w["fi"][hy:hy + ny, hx].max()))
    # the land record: synthetic rivers, plus discharge on every source node a coastal cell interpolates from
    land = syn.jra55_land_snapshots(LAND_CLOCK["n_levels"])
    wet = o0["mask"] != 0
    coast = wet & ~(np.roll(wet, 1, 0) & np.roll(wet, -1, 0) & np.roll(wet, 1, 1) & np.roll(wet, -1, 1))
    fi2 = np.broadcast_to(w["fi"][None, :], wet.shape) if w["separable"] else w["fi"]
    fj2 = np.broadcast_to(w["fj"][:, None], wet.shape) if w["separable"] else w["fj"]
    nsy, nsx = land["friver"].shape[1:]
    ci = np.trunc(fi2[coast]).astype(int) % nsx
    cj = np.clip(np.trunc(fj2[coast]).astype(int), 0, nsy - 1)
    for n in range(LAND_CLOCK["n_levels"]):
        land["friver"][n, cj, ci] = np.float32(1e-4 * (1.0 + 0.25 * n)) * (1.0 + 0.001 * (ci % 13)).astype(np.float32)
    target = o0["S"] + 0.1 * syn.normal("So", i, j, 5)
    area = 1.0 + syn.uniform("hi", i, j, 5)
    bottom = np.where(wet, -1000.0, 10.0)
    return dict(nx=nx, ny=ny, hx=hx, hy=hy, oceans=[o0, o1], ice_state=si, concentrations=conc, x_stress=tx, y_stress=ty,
                weights=w, src=case["src"], land=land, target=target, area=area, bottom_height=bottom, coast=coast)


def census(case, state=0, ice=0):
    """{class: number of interior cells} of ocean state `state` under ice state `ice`, and the largest number of classes met
    inside one aligned run of 64 interior cells."""
    nx, ny, hx, hy = case["nx"], case["ny"], case["hx"], case["hy"]
    inner = (slice(hy, hy + ny), slice(hx, hx + nx))
    cls = {k: v[inner].reshape(-1) for k, v in classify(case["oceans"][state], case["concentrations"][ice]).items()}
    counts = {k: int(v.sum()) for k, v in cls.items()}
    best = 0
    for r in range((nx * ny) // 64):
        best = max(best, sum(bool(v[64 * r:64 * r + 64].any()) for v in cls.values()))
    return counts, best
