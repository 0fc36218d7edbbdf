"""A designed atlas of ice states for the pointwise sea-ice and net-flux kernels, a 50-digit reference of each kernel and a
NumPy model of each with defect flags (test infrastructure of tests/test_ice_atlas.py; CPU only, nothing here imports the
library).

The kernels: compute_sea_ice_ocean_fluxes! (three equations + frazil), SeaIceAlbedo (CCSM3), compute_net_sea_ice_fluxes!,
compute_net_ocean_fluxes! (net_cell_local + net_face_stress), the materialised salinity restoring and NormalizeSalinity.
Random fields essentially never land on their branch points (T_o = T_f, ℵ = 0, S_o = S_min, T_s = T_melt − ΔT, h_i = h_ref,
h_s = 0, |τ| = 0, u★ = u★_min); every cell of the atlas is a named state that sits ON one, one ulp beside it, or far from it.

Layout.  The main surface is 67 × 5 with unequal halos (3, 2): 335 cells = two 256-thread workgroups, the second partial, its
last wave partial.  States are laid row-major and tiled; the three-equation cross product (8 temperatures × 5 salinities ×
5 concentrations = 200 states) is laid on three surfaces with different rotations, so that every state meets several face
stresses, both settings of the u★ floor and of the frazil switch.  Halos hold designed values that differ from every interior
value (stresses 4 … 8, ℵ ≈ 2⁻⁶, never a periodic copy): a neighbour read on the wrong side or with the wrong stride moves the
result by orders of magnitude, and the window's first and last column and row each hold wet, ice-covered cells whose halo-side
neighbour differs by more than a factor 10.  Face stresses follow a column / row pattern with exact zeros, −0.0, 1e-12, a
3-4-5 pair (3·2⁻¹², 4·2⁻¹²: |τ| = 5·2⁻¹² without rounding) and jumps of two to five orders between the two faces of a cell.

The reference.  mpmath at 50 digits, one plain function per kernel, written from the definitions in include/coflux.h.  Inputs
are exact doubles; parameters are the doubles of the parameter blocks (1/ρ, 1/c_p, ε·σ are NOT rounded: the device's
reciprocals are part of what is counted).  Every reference also returns M, the largest intermediate term of the cell, in which
the counted bounds are expressed.  One branch is decided by a rounded product: frazil forms where T_o < T_f = −m·S_o, and m =
0.054 is no dyadic number.  CHOSEN HERE: the reference takes the BRANCH from the double product fl(−m·S_o), as the kernel
and both oracles do, and every VALUE (T_f in the frazil heat, the clamped T_o) from the exact product.  The "at freezing"
entries are therefore at T_o = fl(−m·S_o) exactly, which is what "at the branch point" means for the code under test.

NormalizeSalinity's two sums are exact (fractions.Fraction over the dyadic inputs).

The defect model.  `model_*` restate each kernel in NumPy (double precision, the device's order of operations) with one
flag per plausible defect; tests/test_ice_atlas.py asserts that the clean model is within the GPU bound and that every flag is
caught by named entries at that bound.  One flag of the list cannot be caught by any test: `To <= Tf` for `To < Tf` changes no
bit of any output (at equality the frazil heat is ρ c Δz·0/Δt = +0 and T_o := T_f = T_o); it is kept as EQUIVALENT and the
test asserts exactly that.
"""
from fractions import Fraction

import mpmath as mp
import numpy as np

mp.mp.dps = 50
MPF = mp.mpf

NX, NY, HX, HY = 67, 5, 3, 2
SHAPE = (NY + 2 * HY, NX + 2 * HX)
INNER = (slice(HY, HY + NY), slice(HX, HX + NX))
SENTINEL = 7.0e77
U = 2.0 ** -53                       # one rounding to nearest, relative
TINY = 5e-324                        # the smallest denormal


def up(x):
    return float(np.nextafter(x, np.inf))


def down(x):
    return float(np.nextafter(x, -np.inf))


def interior_mask(shape=SHAPE, hx=HX, hy=HY):
    m = np.zeros(shape, bool)
    m[hy:shape[0] - hy, hx:shape[1] - hx] = True
    return m


def ladder(shape, salt, lo=0.0, hi=1.0):
    """Deterministic, pairwise distinct values in [lo, hi): the golden-ratio sequence over the flat index."""
    n = int(np.prod(shape))
    x = ((np.arange(1, n + 1, dtype=np.float64) + 97.0 * salt) * 0.6180339887498949) % 1.0
    return (lo + (hi - lo) * x).reshape(shape)


def with_halo(interior, base, shape=SHAPE, hx=HX, hy=HY, step=2.0 ** -10):
    """Parent array: `interior` inside, base·(1 + step·flat index) in the halo (distinct, none equal to an interior value)."""
    a = base * (1.0 + step * np.arange(int(np.prod(shape)), dtype=np.float64).reshape(shape))
    a[hy:shape[0] - hy, hx:shape[1] - hx] = interior
    return a


def land_pattern(ny=NY, nx=NX):
    """uint8 [ny, nx], 1 = wet: a diagonal lattice of land cells (≈ 6 %), none of them at a corner."""
    j, i = np.mgrid[0:ny, 0:nx]
    return np.where((3 * i + 5 * j) % 17 == 4, 0, 1).astype(np.uint8)


def mask_arrays(wet, z_surface=-150.0):
    """The same wet set as a uint8 mask and as bottom heights (land: z_surface ≤ z_b), parent-shaped, halos dry."""
    m = np.zeros(SHAPE, np.uint8)
    m[INNER] = wet
    zb = np.where(m != 0, -4000.0, z_surface)          # z_b = z_surface exactly is land (the header's `<=`)
    zb[INNER][(wet == 0) & (np.arange(NX)[None, :] % 2 == 0)] = 12.5
    return m, np.ascontiguousarray(zb)


# =============================================================================================
# compute_sea_ice_ocean_fluxes!: three equations + frazil
# =============================================================================================
OCEAN = dict(rho_o=1026.0, c_o=3991.86795711963, rho_f=1000.0, T_offset=273.15)
TE_PARAMS = dict(heat_transfer_coefficient=0.0095, salt_transfer_coefficient=0.0095 / 35.0, minimum_friction_velocity=0.0,
                 ice_density=917.0, latent_heat_of_fusion=334000.0, ice_salinity=4.0, liquidus_slope=0.054,
                 top_cell_thickness=5.0, time_step=1200.0)
TE_TEMPERATURES = ("at", "ulp_above", "ulp_below", "1e-9_above", "0.1_above", "0.1_below", "2_above", "30_above")
TE_SALINITIES = (("0", 0.0), ("S_ice", 4.0), ("above_S_ice", up(4.0)), ("34", 34.0), ("45", 45.0))
TE_CONCENTRATIONS = (("0", 0.0), ("denormal", TINY), ("1e-12", 1e-12), ("0.15", 0.15), ("1", 1.0))
TE_STATES = tuple((t, s, a) for t in TE_TEMPERATURES for s in TE_SALINITIES for a in TE_CONCENTRATIONS)
# (rotation of the state list, u★ floor, Δt): the floor 0.02 lies above |τ|^½ of the zero and 1e-12 stresses and below that of the others
TE_SURFACES = ((0, 0.0, 1200.0), (71, 0.02, 1200.0), (137, 0.0, 0.0))
S345 = 2.0 ** -12
TX_PATTERN = (0.0, 0.0, -0.0, -0.0, 1e-12, 3 * S345, 3 * S345, 0.4)      # along x: cell (i, j) reads tx[i], tx[i + 1]
TY_PATTERN = (0.0, 0.0, 4 * S345, 4 * S345, 1e-5, 0.3)                   # along y: cell (i, j) reads ty[j], ty[j + 1]
TE_OUTPUTS = ("interface_heat", "salt_flux", "frazil_heat", "friction_velocity")
TE_SCALES = dict(interface_heat=1.0, salt_flux=1e-7, frazil_heat=1.0, friction_velocity=1e-3)   # test_sea_ice_physics.py's


def te_temperature(kind, Tf):
    return {"at": Tf, "ulp_above": up(Tf), "ulp_below": down(Tf), "1e-9_above": Tf + 1e-9, "0.1_above": Tf + 0.1,
            "0.1_below": Tf - 0.1, "2_above": Tf + 2.0, "30_above": Tf + 30.0}[kind]


def te_surface(s):
    """Surface s of the three-equation atlas: parent arrays T, S, conc, tx, ty, the two masks, the parameter dict, and per
    interior cell the state (names[j, i] = "T|S|a") it holds."""
    rot, us_min, dt = TE_SURFACES[s]
    Q = dict(TE_PARAMS, minimum_friction_velocity=us_min, time_step=dt)
    m = Q["liquidus_slope"]
    T, S, A = np.zeros((NY, NX)), np.zeros((NY, NX)), np.zeros((NY, NX))
    names = np.empty((NY, NX), dtype=object)
    state = np.zeros((NY, NX), np.int64)
    for n in range(NX * NY):
        j, i = divmod(n, NX)
        k = (n + rot) % len(TE_STATES)
        t, (sn, So), (an, a) = TE_STATES[k]
        Tf = -m * So                                   # the double product: the branch point of the code under test
        T[j, i], S[j, i], A[j, i] = te_temperature(t, Tf), So, a
        names[j, i], state[j, i] = "%s|S=%s|a=%s" % (t, sn, an), k
    jj, ii = np.mgrid[0:NY, 0:NX]
    tx = np.array(TX_PATTERN)[(ii + jj) % len(TX_PATTERN)]
    ty = np.array(TY_PATTERN)[(jj + 2 * ii) % len(TY_PATTERN)]
    wet = land_pattern()
    mask, zb = mask_arrays(wet)
    return dict(T=with_halo(T, 11.0), S=with_halo(S, 20.0), conc=with_halo(A, 2.0 ** -6), tx=with_halo(tx, 4.0),
                ty=with_halo(ty, -5.0), mask=mask, bottom_height=zb, params=Q, names=names, state=state, wet=wet != 0)


def _cells(ny=NY, nx=NX, hx=HX, hy=HY):
    for j in range(ny):
        for i in range(nx):
            yield j, i, j + hy, i + hx


def ref_three_equation(F, use=("conc", "tx", "ty")):
    """The four outputs on the interior (float64 arrays of the correctly rounded 50-digit values).  `use`: which nullable
    inputs are given (an absent concentration is 0, an absent stress component 0)."""
    Q, O = F["params"], OCEAN
    out = {k: np.zeros((NY, NX)) for k in TE_OUTPUTS}
    ah, as_, m = MPF(Q["heat_transfer_coefficient"]), MPF(Q["salt_transfer_coefficient"]), MPF(Q["liquidus_slope"])
    L, Si, dz, dt = MPF(Q["latent_heat_of_fusion"]), MPF(Q["ice_salinity"]), MPF(Q["top_cell_thickness"]), MPF(Q["time_step"])
    rho, c = MPF(O["rho_o"]), MPF(O["c_o"])
    for j, i, J, I in _cells():
        if not F["wet"][j, i]:
            continue
        To, So = MPF(F["T"][J, I]), MPF(F["S"][J, I])
        Tf = -m * So
        if Q["time_step"] > 0.0 and F["T"][J, I] < -Q["liquidus_slope"] * F["S"][J, I]:      # the branch: from the double product
            out["frazil_heat"][j, i] = float(rho * c * dz * (To - Tf) / dt)
            To = Tf
        a = MPF(F["conc"][J, I]) if "conc" in use else MPF(0)
        if a > 0:
            txc = (MPF(F["tx"][J, I]) + MPF(F["tx"][J, I + 1])) / 2 if "tx" in use else MPF(0)
            tyc = (MPF(F["ty"][J, I]) + MPF(F["ty"][J + 1, I])) / 2 if "ty" in use else MPF(0)
            us = max(mp.sqrt(mp.sqrt(txc * txc + tyc * tyc)), MPF(Q["minimum_friction_velocity"]))
            # α_s (S_o − S_b) = (c α_h / ℒ)(T_o + m S_b)(S_b − S_i): the positive root
            g = c * ah / L
            A, B, C = g * m, g * To - g * m * Si + as_, g * To * Si + as_ * So
            Sb = (-B + mp.sqrt(B * B + 4 * A * C)) / (2 * A)
            Tb = -m * Sb
            out["interface_heat"][j, i] = float(a * rho * c * ah * us * (To - Tb))
            out["salt_flux"][j, i] = float(a * as_ * us * (So - Sb))
            out["friction_velocity"][j, i] = float(us)
    return out


TE_FLAGS = ("te_west_south", "te_y_stride", "te_a_ge", "te_negative_root", "te_no_floor", "te_T_before_clamp")
EQUIVALENT_FLAGS = ("te_T_le",)      # changes no bit of any output (module docstring)


def model_three_equation(F, defect=None, use=("conc", "tx", "ty")):
    """The kernel in NumPy doubles, the device's order of operations; `defect`: one of TE_FLAGS / EQUIVALENT_FLAGS."""
    Q, O = F["params"], OCEAN
    rho, c = O["rho_o"], O["c_o"]
    sl = lambda a, dj=0, di=0: a[HY + dj:HY + NY + dj, HX + di:HX + NX + di]      # noqa: E731
    To, So = sl(F["T"]).copy(), sl(F["S"])
    m = Q["liquidus_slope"]
    Tf = -m * So
    T0 = To.copy()
    frz = ((To <= Tf) if defect == "te_T_le" else (To < Tf)) & (Q["time_step"] > 0.0)
    with np.errstate(all="ignore"):
        qfr = np.where(frz, rho * c * Q["top_cell_thickness"] * (To - Tf) / (Q["time_step"] if Q["time_step"] > 0 else 1.0), 0.0)
        To = np.where(frz, Tf, To)
        a = sl(F["conc"]) if "conc" in use else np.zeros((NY, NX))
        side = -1 if defect == "te_west_south" else 1
        txc = 0.5 * (sl(F["tx"]) + sl(F["tx"], 0, side)) if "tx" in use else np.zeros((NY, NX))
        if "ty" in use:
            other = sl(F["ty"], 0, 1) if defect == "te_y_stride" else sl(F["ty"], side, 0)
            tyc = 0.5 * (sl(F["ty"]) + other)
        else:
            tyc = np.zeros((NY, NX))
        us = np.sqrt(np.sqrt(txc * txc + tyc * tyc))
        if defect != "te_no_floor":
            us = np.maximum(us, Q["minimum_friction_velocity"])
        ah, as_, Si = Q["heat_transfer_coefficient"], Q["salt_transfer_coefficient"], Q["ice_salinity"]
        g = c * ah / Q["latent_heat_of_fusion"]
        A, B, C = g * m, g * To - g * m * Si + as_, g * To * Si + as_ * So
        root = np.sqrt(B * B + 4.0 * A * C)
        Sb = (-B - root if defect == "te_negative_root" else -B + root) / (2.0 * A)
        Tb = -m * Sb
        icy = (a >= 0.0) if defect == "te_a_ge" else (a > 0.0)
        Tq = T0 if defect == "te_T_before_clamp" else To
        qio = np.where(icy, a * rho * c * ah * us * (Tq - Tb), 0.0)
        jio = np.where(icy, a * as_ * us * (So - Sb), 0.0)
        us = np.where(icy, us, 0.0)
    wet = F["wet"]
    return dict(interface_heat=np.where(wet, qio, 0.0), salt_flux=np.where(wet, jio, 0.0),
                frazil_heat=np.where(wet, qfr, 0.0), friction_velocity=np.where(wet, us, 0.0))


def scaled_error(got, ref, scale):
    """|Δ| / max(|ref|, scale) per cell (the metric of test_sea_ice_physics.py); NaN counts as infinite."""
    d = np.abs(np.asarray(got, np.float64) - ref) / np.maximum(np.abs(ref), scale)
    return np.where(np.isnan(d), np.inf, d)


# =============================================================================================
# SeaIceAlbedo (CCSM3): every cell of the parent array
# =============================================================================================
ALBEDO_SETS = (
    dict(ice_visible=0.78, ice_near_infrared=0.36, snow_visible=0.98, snow_near_infrared=0.70, ocean_albedo=0.06,
         reference_thickness=0.3, melt_temperature_range=1.0, ice_melt_change=0.075, snow_melt_change_visible=0.10,
         snow_melt_change_near_infrared=0.15, snow_patch_thickness=0.02, visible_fraction=0.5, melting_temperature=0.0),
    # every temperature parameter dyadic (the kinks stay exact), visible fraction ≠ ½, melting point ≠ 0, other h_ref and patch
    dict(ice_visible=0.73, ice_near_infrared=0.33, snow_visible=0.96, snow_near_infrared=0.68, ocean_albedo=0.07,
         reference_thickness=0.5, melt_temperature_range=0.5, ice_melt_change=0.085, snow_melt_change_visible=0.11,
         snow_melt_change_near_infrared=0.16, snow_patch_thickness=0.03125, visible_fraction=0.6875, melting_temperature=-1.75),
)
ALBEDO_TS = ("melt_onset", "melt_onset_ulp_above", "melt_onset_ulp_below", "melting", "melting_ulp_above", "melting_ulp_below",
             "mid_range", "above_melting", "far_below")
ALBEDO_HI = ("0", "tiny", "h_ref", "h_ref_ulp_above", "h_ref_ulp_below", "5m")
ALBEDO_HS = ("0", "-0", "denormal", "patch", "10m")
ALBEDO_STATES = tuple((t, h, s) for t in ALBEDO_TS for h in ALBEDO_HI for s in ALBEDO_HS)       # 270 ≤ 657 parent cells
BOUND_ALBEDO = 24                                     # units of U · 1 (test_ice_atlas.py counts)


def albedo_fields(A):
    """hi, hs, Ts over the WHOLE parent array (the kernel's footprint), tiled states; names parent-shaped."""
    Tm, dT, href, patch = A["melting_temperature"], A["melt_temperature_range"], A["reference_thickness"], A["snow_patch_thickness"]
    onset = Tm - dT
    ts = dict(melt_onset=onset, melt_onset_ulp_above=up(onset), melt_onset_ulp_below=down(onset), melting=Tm,
              melting_ulp_above=up(Tm), melting_ulp_below=down(Tm), mid_range=Tm - 0.5 * dT, above_melting=Tm + 2.0, far_below=Tm - 40.0)
    hi = {"0": 0.0, "tiny": 1e-300, "h_ref": href, "h_ref_ulp_above": up(href), "h_ref_ulp_below": down(href), "5m": 5.0}
    hs = {"0": 0.0, "-0": -0.0, "denormal": TINY, "patch": patch, "10m": 10.0}
    n = int(np.prod(SHAPE))
    out = dict(hi=np.zeros(n), hs=np.zeros(n), Ts=np.zeros(n), names=np.empty(n, dtype=object), state=np.zeros(n, np.int64))
    for k in range(n):
        s = (k * 7 + 3) % len(ALBEDO_STATES)          # 7 is coprime to 270: the first 270 cells hold every state once
        t, h, c = ALBEDO_STATES[s]
        out["hi"][k], out["hs"][k], out["Ts"][k], out["names"][k], out["state"][k] = hi[h], hs[c], ts[t], "Ts=%s|hi=%s|hs=%s" % (t, h, c), s
    return {k: v.reshape(SHAPE) for k, v in out.items()}


def ref_albedo_cell(A, hi, hs, Ts):
    P = {k: MPF(v) for k, v in A.items()}
    hi, hs, Ts = MPF(hi), MPF(hs), MPF(Ts)
    fh = min(mp.atan(4 * hi) / mp.atan(4 * P["reference_thickness"]), MPF(1))
    fT = min((P["melting_temperature"] - Ts) / P["melt_temperature_range"] - 1, MPF(0))      # 0 below T_melt − ΔT, −1 at T_melt
    ocean = P["ocean_albedo"]
    band = []
    for ice, snow, dsnow in ((P["ice_visible"], P["snow_visible"], P["snow_melt_change_visible"]),
                             (P["ice_near_infrared"], P["snow_near_infrared"], P["snow_melt_change_near_infrared"])):
        bare = max(ice * fh + ocean * (1 - fh) + P["ice_melt_change"] * fT, ocean)
        cover = hs / (hs + P["snow_patch_thickness"]) if hs > 0 else MPF(0)
        band.append(bare * (1 - cover) + (snow + dsnow * fT) * cover)
    return P["visible_fraction"] * band[0] + (1 - P["visible_fraction"]) * band[1]


def ref_albedo(A, hi, hs, Ts):
    f = np.frompyfunc(lambda a, b, c: float(ref_albedo_cell(A, a, b, c)), 3, 1)
    return f(hi, np.zeros_like(hi) if hs is None else hs, Ts).astype(np.float64)


ALBEDO_FLAGS = ("alb_fT_unclamped", "alb_fh_unclamped", "alb_snow_at_zero", "alb_bands_swapped")


def model_albedo(A, hi, hs, Ts, defect=None):
    hs = np.zeros_like(hi) if hs is None else hs
    fh = np.arctan(4.0 * hi) / np.arctan(4.0 * A["reference_thickness"])
    if defect != "alb_fh_unclamped":
        fh = np.minimum(fh, 1.0)
    ao = A["ocean_albedo"] * (1.0 - fh)
    fT = (A["melting_temperature"] - Ts) / A["melt_temperature_range"] - 1.0
    if defect != "alb_fT_unclamped":
        fT = np.minimum(fT, 0.0)
    ice_v = np.maximum(A["ice_visible"] * fh + ao + A["ice_melt_change"] * fT, A["ocean_albedo"])
    ice_n = np.maximum(A["ice_near_infrared"] * fh + ao + A["ice_melt_change"] * fT, A["ocean_albedo"])
    snow_v = A["snow_visible"] + A["snow_melt_change_visible"] * fT
    snow_n = A["snow_near_infrared"] + A["snow_melt_change_near_infrared"] * fT
    with np.errstate(all="ignore"):
        cover = np.where(hs > 0.0, hs / (hs + A["snow_patch_thickness"]), 1.0 if defect == "alb_snow_at_zero" else 0.0)
    v, n = ice_v * (1.0 - cover) + snow_v * cover, ice_n * (1.0 - cover) + snow_n * cover
    if defect == "alb_bands_swapped":
        v, n = n, v
    return A["visible_fraction"] * v + (1.0 - A["visible_fraction"]) * n


# =============================================================================================
# compute_net_sea_ice_fluxes!
# =============================================================================================
NSI_PARAMS = dict(albedo=0.7, emissivity=0.97, sigma=5.67e-8, T_offset=273.15)
NSI_CONCENTRATIONS = (("0", 0.0), ("denormal", TINY), ("1", 1.0))
BOUND_NSI_TOP, BOUND_NSI_BOTTOM = 17, 2


def nsi_fields():
    j, i = np.mgrid[0:NY, 0:NX]
    pick = (i + 2 * j) % 3
    conc = np.array([a for _, a in NSI_CONCENTRATIONS])[pick]
    names = np.array([n for n, _ in NSI_CONCENTRATIONS], dtype=object)[pick]
    wet = land_pattern()
    mask, zb = mask_arrays(wet)
    inner = (NY, NX)
    F = dict(conc=with_halo(conc, 2.0 ** -6), albedo=with_halo(ladder(inner, 1, 0.3, 0.9), 0.05),
             Qs=with_halo(ladder(inner, 2, 0.0, 900.0), 4000.0), Ql=with_halo(ladder(inner, 3, 150.0, 450.0), 3000.0),
             Ts=with_halo(ladder(inner, 4, -40.0, 0.0), 25.0), Qc=with_halo(ladder(inner, 5, -200.0, 200.0), 2500.0),
             Qv=with_halo(ladder(inner, 6, -100.0, 150.0), -2200.0), Qf=with_halo(-ladder(inner, 7, 0.0, 80.0), 1700.0),
             Qi=with_halo(ladder(inner, 8, -30.0, 300.0), -1300.0), mask=mask, bottom_height=zb, wet=wet != 0,
             names=np.array(["a=%s" % n for n in names.ravel()], dtype=object).reshape(inner))
    return F


def ref_net_sea_ice(F, K=NSI_PARAMS, albedo_field=True, frazil=True, interface=True):
    """(top, bottom, M_top, M_bottom) on the interior: ΣQt = (Q_d + Q_u + Q_c + Q_v)·[ℵ > 0], ΣQb = Q_frazil + Q_interface."""
    top, bot, Mt, Mb = (np.zeros((NY, NX)) for _ in range(4))
    eps, sig, off = MPF(K["emissivity"]), MPF(K["sigma"]), MPF(K["T_offset"])
    for j, i, J, I in _cells():
        if not F["wet"][j, i]:
            continue
        alb = MPF(F["albedo"][J, I]) if albedo_field else MPF(K["albedo"])
        Qs, Ql, Qc, Qv = (MPF(F[k][J, I]) for k in ("Qs", "Ql", "Qc", "Qv"))
        Qu = eps * sig * (MPF(F["Ts"][J, I]) + off) ** 4
        sw, lw = (1 - alb) * Qs, eps * Ql
        Qd = -sw - lw
        s1 = Qd + Qu
        s2 = s1 + Qc
        s3 = s2 + Qv
        if F["conc"][J, I] > 0.0:
            top[j, i] = float(s3)
        Mt[j, i] = float(max(abs(x) for x in (Qu, sw, lw, Qd, s1, s2, s3, Qc, Qv)))
        Qf = MPF(F["Qf"][J, I]) if frazil else MPF(0)
        Qi = MPF(F["Qi"][J, I]) if interface else MPF(0)
        bot[j, i] = float(Qf + Qi)
        Mb[j, i] = float(max(abs(Qf), abs(Qi)))
    return top, bot, Mt, Mb


NSI_FLAGS = ("nsi_top_ungated", "nsi_no_emissivity")


def model_net_sea_ice(F, K=NSI_PARAMS, defect=None, albedo_field=True, frazil=True, interface=True):
    c = lambda k: F[k][INNER]      # noqa: E731
    alb = c("albedo") if albedo_field else K["albedo"]
    T = c("Ts") + K["T_offset"]
    T2 = T * T
    Qu = (K["emissivity"] * K["sigma"]) * T2 * T2
    Qd = -(1.0 - alb) * c("Qs") - (1.0 if defect == "nsi_no_emissivity" else K["emissivity"]) * c("Ql")
    s = Qd + Qu + c("Qc") + c("Qv")
    top = s if defect == "nsi_top_ungated" else np.where(c("conc") > 0.0, s, 0.0)
    bottom = (c("Qf") if frazil else 0.0) + (c("Qi") if interface else 0.0) + np.zeros((NY, NX))
    return np.where(F["wet"], top, 0.0), np.where(F["wet"], bottom, 0.0)


# =============================================================================================
# compute_net_ocean_fluxes!: net_cell_local + net_face_stress
# =============================================================================================
S_MIN = 31.0
NO_SALINITIES = (("S_min", S_MIN), ("S_min_ulp_above", up(S_MIN)), ("S_min_ulp_below", down(S_MIN)), ("35", 35.0), ("20", 20.0))
NO_FRESHWATER = (("rain", 3e-5, 1e-5, 0.0), ("evaporation", 1e-5, 3e-5, 0.0), ("rain+river", 3e-5, 1e-5, 3e-4),
                 ("evaporation+river", 1e-5, 3e-5, 3e-4))              # (name, M_p, M_v, M_land)
NO_CONCENTRATIONS = (0.0, 0.3, 1.0)
NO_LATITUDES = (-90.0, -45.0, 0.0, 45.0, 90.0)
# name → (albedo kind, penetrating, emissivity, ice fields given, land, latitude storage)
NO_CONFIGS = {
    "constant": dict(albedo=0.06, latitude=None, penetrating=1, emissivity=0.97, ice=("concentration", "interface_heat", "salt_flux", "x_stress", "y_stress"), land=True),
    "latitude_1d": dict(albedo=(0.069, 0.011), latitude="separable", penetrating=0, emissivity=1.0, ice=("concentration", "interface_heat", "salt_flux"), land=False),
    "latitude_2d": dict(albedo=(0.069, 0.011), latitude="general", penetrating=0, emissivity=0.97, ice=("concentration", "interface_heat", "salt_flux", "x_stress", "y_stress"), land=True),
    "no_ice": dict(albedo=0.06, latitude=None, penetrating=1, emissivity=0.97, ice=(), land=False),
}
NO_OUTPUTS = ("u", "v", "T", "S", "shortwave_surface_flux", "upwelling_longwave", "downwelling_longwave", "downwelling_shortwave")
# counted bounds in units of U · M (test_ice_atlas.py)
BOUND_NO = dict(u=10, v=10, T=32, S=12, shortwave_surface_flux=10, upwelling_longwave=10, downwelling_longwave=2, downwelling_shortwave=6)
SIGMA = 5.67e-8


def _draw3(seed=2026):
    """Independent draws from {0, 1, 2} per interior cell (seeded: the same surface every time)."""
    return np.random.default_rng(seed).integers(0, 3, (NY, NX))


def no_surface(config):
    """The net-ocean atlas surface under one of NO_CONFIGS: parent arrays of every input, masks, names."""
    cfg = NO_CONFIGS[config]
    inner = (NY, NX)
    j, i = np.mgrid[0:NY, 0:NX]
    n = j * NX + i
    sal, fw = n % len(NO_SALINITIES), (n // len(NO_SALINITIES)) % len(NO_FRESHWATER)
    S = np.array([v for _, v in NO_SALINITIES])[sal]
    Mp, Mv, Ml = (np.array([f[k] for f in NO_FRESHWATER])[fw] * (1.0 + 0.25 * ladder(inner, 20 + k)) for k in (1, 2, 3))
    conc = np.array(NO_CONCENTRATIONS)[_draw3()]
    wet = land_pattern()
    wet[0, 0] = wet[0, NX - 1] = wet[NY - 1, 0] = wet[NY - 1, NX - 1] = 1
    conc[0, 0], conc[0, NX - 1], conc[NY - 1, 0], conc[NY - 1, NX - 1] = 1.0, 0.3, 0.3, 1.0     # wet ice at every edge of the window
    mask, zb = mask_arrays(wet)
    rtx = np.where(i % 2 == 0, 0.01, 1.0) * (1.0 + ladder(inner, 31))      # two orders between the two cells of a face
    rty = np.where(j % 2 == 0, -0.8, 0.004) * (1.0 + ladder(inner, 32))
    if cfg["latitude"] == "separable":
        lat = np.array((-63.0, 17.0) + NO_LATITUDES + (29.0, -11.0))       # [ny + 2 hy]: one per row, halo rows distinct
    elif cfg["latitude"] == "general":
        lat = with_halo(np.array(NO_LATITUDES)[(i + 2 * j) % 5], 10.0)
    else:
        lat = None
    F = dict(config=config, cfg=cfg, S=with_halo(S, 20.5), conc=with_halo(conc, 2.0 ** -6), Mp=with_halo(Mp, 0.9), Mv=with_halo(Mv, 0.7),
             land=with_halo(Ml, 0.6), Qs=with_halo(ladder(inner, 2, 0.0, 900.0), 4000.0), Ql=with_halo(ladder(inner, 3, 150.0, 450.0), 3000.0),
             Ts=with_halo(ladder(inner, 4, -1.8, 30.0), 55.0), Qc=with_halo(ladder(inner, 5, -200.0, 200.0), 2500.0),
             Qv=with_halo(ladder(inner, 6, -50.0, 300.0), -2200.0), Qio=with_halo(ladder(inner, 9, -20.0, 400.0), 1900.0),
             Jsio=with_halo(ladder(inner, 10, -1e-6, 4e-6), 0.02), txio=with_halo(ladder(inner, 11, -2e-4, 2e-4), 0.3),
             tyio=with_halo(ladder(inner, 12, -2e-4, 2e-4), -0.4), rtx=with_halo(rtx, 30.0), rty=with_halo(rty, -45.0),
             latitude=lat, mask=mask, bottom_height=zb, wet=wet != 0)
    F["names"] = np.array(["S=%s|%s|a=%g,west=%g,south=%g" % (NO_SALINITIES[sal[b, a]][0], NO_FRESHWATER[fw[b, a]][0], F["conc"][b + HY, a + HX],
                                                               F["conc"][b + HY, a + HX - 1], F["conc"][b + HY - 1, a + HX])
                           for b in range(NY) for a in range(NX)], dtype=object).reshape(inner)
    return F


def _no_inputs(F, J, I):
    """Inputs of one cell with the absent ones at their documented defaults (0)."""
    cfg = F["cfg"]
    g = lambda name, key, dj=0, di=0: F[key][J + dj, I + di] if name in cfg["ice"] else 0.0      # noqa: E731
    return dict(a=g("concentration", "conc"), aw=g("concentration", "conc", 0, -1), as_=g("concentration", "conc", -1, 0),
                Qio=g("interface_heat", "Qio"), Jsio=g("salt_flux", "Jsio"), txio=g("x_stress", "txio"), tyio=g("y_stress", "tyio"),
                Ml=F["land"][J, I] if cfg["land"] else 0.0)


def ref_net_ocean(F):
    """{output: (value, M)} on the interior, zero on land.  M = the largest intermediate term of the cell in the output's units."""
    cfg, O = F["cfg"], OCEAN
    out = {k: (np.zeros((NY, NX)), np.zeros((NY, NX))) for k in NO_OUTPUTS}
    eps, rho, c, rf, off = MPF(cfg["emissivity"]), MPF(O["rho_o"]), MPF(O["c_o"]), MPF(O["rho_f"]), MPF(O["T_offset"])
    big = lambda *xs: float(max(abs(x) for x in xs))      # noqa: E731
    for j, i, J, I in _cells():
        if not F["wet"][j, i]:
            continue
        x = {k: MPF(v) for k, v in _no_inputs(F, J, I).items()}
        if cfg["latitude"] is None:
            alb = MPF(cfg["albedo"])
        else:
            phi = F["latitude"][J] if cfg["latitude"] == "separable" else F["latitude"][J, I]
            alb = MPF(cfg["albedo"][0]) - MPF(cfg["albedo"][1]) * mp.cos(2 * MPF(phi) * mp.pi / 180)
        So, Qs, Ql, Qc, Qv, Mp, Mv = (MPF(F[k][J, I]) for k in ("S", "Qs", "Ql", "Qc", "Qv", "Mp", "Mv"))
        Qu = eps * MPF(SIGMA) * (MPF(F["Ts"][J, I]) + off) ** 4
        Qal = -eps * Ql
        Qts = -(1 - alb) * Qs * (1 - x["a"])
        Qss = MPF(0) if cfg["penetrating"] else Qts
        s1 = Qu + Qc
        s2 = s1 + Qv
        s3 = s2 + Qal
        SQ = s3 * (1 - x["a"]) + Qss
        SF = (-Mp + Mv) / rf
        floor = F["S"][J, I] < S_MIN
        SFs = MPF(0) if floor and SF < 0 else SF
        SFl = -x["Ml"] / rf
        SFls = MPF(0) if floor and SFl < 0 else SFl
        roc = 1 / (rho * c)
        put = lambda k, v, M: (out[k][0].__setitem__((j, i), float(v)), out[k][1].__setitem__((j, i), M))      # noqa: E731
        put("T", SQ * roc + x["Qio"] * roc, big(Qu, Qc, Qv, Qal, s1, s2, s3, Qts, SQ, x["Qio"]) * float(roc))
        put("S", (1 - x["a"]) * (-So * SFs) + x["Jsio"] + (-So * SFls), big(So * Mp / rf, So * Mv / rf, So * SFl, x["Jsio"]))
        put("shortwave_surface_flux", Qts * roc, big(Qs * roc))
        put("upwelling_longwave", Qu, big(Qu))
        put("downwelling_longwave", -Qal, big(Qal))
        put("downwelling_shortwave", -Qts, big(Qs))
        for name, key, nb, an, tio in (("u", "rtx", (J, I - 1), x["aw"], x["txio"]), ("v", "rty", (J - 1, I), x["as_"], x["tyio"])):
            ta, tb = MPF(F[key][nb]), MPF(F[key][J, I])
            af = (an + x["a"]) / 2
            put(name, (1 - af) * ((ta + tb) / 2 / rho) + af * tio, big(ta / rho, tb / rho, tio))
    return out


NO_FLAGS = ("no_floor_le", "no_land_ice_masked", "no_land_unfloored", "no_face_ice_cell_only", "no_stress_wrong_side",
            "no_sw_in_JT", "no_lat_wrong_index")


def model_net_ocean(F, defect=None):
    cfg, O = F["cfg"], OCEAN
    sl = lambda a, dj=0, di=0: a[HY + dj:HY + NY + dj, HX + di:HX + NX + di]      # noqa: E731
    z = np.zeros((NY, NX))
    ice = lambda name, key, dj=0, di=0: sl(F[key], dj, di) if name in cfg["ice"] else z      # noqa: E731
    a, aw, as_ = ice("concentration", "conc"), ice("concentration", "conc", 0, -1), ice("concentration", "conc", -1, 0)
    rho_inv, c_inv, rf_inv = 1.0 / O["rho_o"], 1.0 / O["c_o"], 1.0 / O["rho_f"]
    if cfg["latitude"] is None:
        alb = cfg["albedo"]
    else:
        if cfg["latitude"] == "separable" or defect == "no_lat_wrong_index":
            lat = F["latitude"] if F["latitude"].ndim == 1 else F["latitude"].ravel()      # the separable read of a 2-D array: [j + hy]
            phi = np.broadcast_to(lat[HY:HY + NY, None], (NY, NX))
        else:
            phi = sl(F["latitude"])
        alb = cfg["albedo"][0] - cfg["albedo"][1] * np.cos(2.0 * phi * (np.pi / 180.0))
    So = sl(F["S"])
    T = sl(F["Ts"]) + O["T_offset"]
    T2 = T * T
    Qu = cfg["emissivity"] * SIGMA * T2 * T2
    Qal = -cfg["emissivity"] * sl(F["Ql"])
    Qts = -(1.0 - alb) * sl(F["Qs"]) * (1.0 - a)
    Qss = Qts if (not cfg["penetrating"] or defect == "no_sw_in_JT") else 0.0
    SQ = (Qu + sl(F["Qc"]) + sl(F["Qv"]) + Qal) * (1.0 - a) + Qss
    SF = -sl(F["Mp"]) * rf_inv + sl(F["Mv"]) * rf_inv
    below = (So <= S_MIN) if defect == "no_floor_le" else (So < S_MIN)
    SFs = np.where(below & (SF < 0.0), 0.0, SF)
    roc = rho_inv * c_inv
    SFl = -(sl(F["land"]) if cfg["land"] else z) * rf_inv
    SFls = SFl if defect == "no_land_unfloored" else np.where(below & (SFl < 0.0), 0.0, SFl)
    land_term = -So * SFls
    if defect == "no_land_ice_masked":
        land_term = (1.0 - a) * land_term
    res = dict(T=SQ * roc + ice("interface_heat", "Qio") * roc, S=(1.0 - a) * (-So * SFs) + ice("salt_flux", "Jsio") + land_term,
               shortwave_surface_flux=Qts * roc, upwelling_longwave=Qu, downwelling_longwave=-Qal, downwelling_shortwave=-Qts)
    side = 1 if defect == "no_stress_wrong_side" else -1
    for name, key, nb, an, tio in (("u", "rtx", (0, side), aw, ice("x_stress", "txio")), ("v", "rty", (side, 0), as_, ice("y_stress", "tyio"))):
        tao = 0.5 * (sl(F[key], *nb) + sl(F[key])) * rho_inv
        af = a if defect == "no_face_ice_cell_only" else 0.5 * (an + a)
        res[name] = (1.0 - af) * tao + af * tio
    return {k: np.where(F["wet"], v, 0.0) for k, v in res.items()}


# =============================================================================================
# SurfaceFluxRestoring materialised
# =============================================================================================
PISTON = 1.0 / 6.0 / 86400.0
BOUND_RESTORING = 3


def restoring_fields():
    F = no_surface("constant")
    S = F["S"]
    j, i = np.mgrid[0:SHAPE[0], 0:SHAPE[1]]
    target = np.where((i + j) % 3 == 0, S, 34.5 + 0.25 * ((i * 5 + j) % 7))      # S == target on a third of the cells
    return dict(S=S, target=target, mask=F["mask"], bottom_height=F["bottom_height"], wet=F["wet"])


def ref_restoring(R, vp=PISTON):
    out = np.zeros((NY, NX))
    for j, i, J, I in _cells():
        if R["wet"][j, i]:
            out[j, i] = float(MPF(vp) * (MPF(R["S"][J, I]) - MPF(R["target"][J, I])))
    return out


# =============================================================================================
# NormalizeSalinity
# =============================================================================================
NZ_BLOCK, NZ_MAX_BLOCKS = 256, 512      # salinity_partial_sums_kernel's launch: min(512, ⌈n/256⌉) workgroups of 256, grid-stride
NZ_CASES = ("one_cell", "constant", "one_wet_cell", "all_land", "cancelling", "cancelling_bottom_height")


def nz_case(name):
    """dict(nx, ny, hx, hy, ring, flux, additional | None, area | None, mask_kind ("u8" / "bottom_height"), mask, wet)."""
    big = name.startswith("cancelling")
    nx, ny, hx, hy, ring = (1, 1, 1, 1, 0) if name == "one_cell" else (513, 257, 2, 1, 0) if big else (NX, NY, HX, HY, 1)
    shape = (ny + 2 * hy, nx + 2 * hx)
    inner = (slice(hy, hy + ny), slice(hx, hx + nx))
    n = nx * ny
    flat = np.arange(n).reshape(ny, nx)
    flux = with_halo(ladder((ny, nx), 40, -5.0, 5.0), 9.0, shape, hx, hy)                  # land and halos carry large values
    area = 1.0 + (np.arange(int(np.prod(shape))).reshape(shape) % 7) / 8.0                 # dyadic, 1 … 1.75
    additional = None
    wet = np.zeros((ny, nx), bool)
    if name == "one_cell":
        wet[:] = True
        flux[inner] = 3.3e-7
        area[inner] = 4.0                                                                  # a power of two: v·A / A is exact
    elif name == "constant":
        wet = land_pattern() != 0
        flux[inner] = np.where(wet, 2.5e-7, flux[inner])
    elif name == "one_wet_cell":
        wet.ravel()[300] = True                                                            # in the second, partial workgroup
        additional = with_halo(ladder((ny, nx), 41, -1e-6, 1e-6), 3.0, shape, hx, hy)
        area[inner][wet] = 2.0
    elif name == "all_land":
        pass
    else:
        # 769 wet cells in the first trip of the grid-stride loop (+1e-3) and all 769 cells of the second trip (−1e-3 + 2e-12),
        # pairwise with the same areas: the weighted mean is 1e-12, and +1e-3 without the tail
        first = 170 * np.arange(769)
        tail = NZ_MAX_BLOCKS * NZ_BLOCK + np.arange(769)
        assert tail[-1] == n - 1 and first[-1] < NZ_MAX_BLOCKS * NZ_BLOCK
        wet.ravel()[first] = True
        wet.ravel()[tail] = True
        a = 1.0 + (np.arange(769) % 7) / 8.0
        A = area[inner].copy()
        A.ravel()[first], A.ravel()[tail] = a, a
        area[inner] = A
        v = flux[inner].copy()
        v.ravel()[first], v.ravel()[tail] = 1e-3, -1e-3 + 2e-12
        flux[inner] = v
        if name == "cancelling":
            additional = np.zeros(shape)
            additional[inner] = np.where(wet, 2.0 ** -40 * ((flat % 5) - 2), 7.0)          # Σ over the pairs is not zero: it is in the reference
            additional = with_halo(additional[inner], 3.0, shape, hx, hy)
    kind = "bottom_height" if name in ("one_wet_cell", "cancelling_bottom_height") else "u8"
    m8 = np.zeros(shape, np.uint8)
    m8[inner] = wet
    mask = np.where(m8 != 0, -4000.0, -150.0) if kind == "bottom_height" else m8
    use_area = name not in ("cancelling_bottom_height", "all_land")
    return dict(name=name, nx=nx, ny=ny, hx=hx, hy=hy, ring=ring, shape=shape, inner=inner, flux=flux, additional=additional,
                area=np.ascontiguousarray(area) if use_area else None, mask_kind=kind, mask=np.ascontiguousarray(mask), wet=wet)


def nz_exact(c):
    """(exact mean as a Fraction, bound n·2⁻⁵³·Σ|v·A| / ΣA as a float, wet count): the definition, no rounding."""
    inner, wet = c["inner"], c["wet"]
    f = c["flux"][inner][wet]
    add = c["additional"][inner][wet] if c["additional"] is not None else np.zeros(f.shape)
    A = c["area"][inner][wet] if c["area"] is not None else np.ones(f.shape)
    sv = sa = sabs = Fraction(0)
    for x, y, w in zip(f, add, A):
        v = Fraction(float(x)) + Fraction(float(y))
        sv += v * Fraction(float(w))
        sabs += abs(v) * Fraction(float(w))
        sa += Fraction(float(w))
    n = int(wet.sum())
    if sa == 0:
        return Fraction(0), 0.0, 0
    return sv / sa, float(n * Fraction(1, 2 ** 53) * sabs / sa), n


NZ_FLAGS = ("nz_second_trip_dropped", "nz_land_included", "nz_interior_only")


def model_normalize(c, defect=None):
    """(flux after, mean): sums in index order (the device's order differs — the bound covers any order)."""
    inner = c["inner"]
    n = c["nx"] * c["ny"]
    seen = np.ones(n, bool)
    if defect == "nz_second_trip_dropped":
        seen[NZ_MAX_BLOCKS * NZ_BLOCK:] = False
    take = (np.ones(n, bool) if defect == "nz_land_included" else c["wet"].ravel()) & seen
    v = c["flux"][inner].ravel() + (c["additional"][inner].ravel() if c["additional"] is not None else 0.0)
    A = c["area"][inner].ravel() if c["area"] is not None else np.ones(n)
    sj, sa = float(np.sum((v * A)[take])), float(np.sum(A[take]))
    mean = sj / sa if sa > 0.0 else 0.0
    out = c["flux"].copy()
    if defect == "nz_interior_only":
        out[inner] -= mean
    else:
        out -= mean
    return out, mean
