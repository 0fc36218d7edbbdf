"""The pointwise sea-ice and net-flux kernels of csrc/coflux_net.hip (and the same arithmetic inlined into the solver
epilogues) on a designed atlas of ice states (tests/ice_atlas.py), against a 50-digit reference, from sentinel-filled outputs.

Before this file each of these kernels met one smooth random field at one or two shapes, was compared with the C oracle (the
same formula typed again in the same precision) and wrote into zero-filled buffers, where an unwritten land or ice-free cell
looks correct.  Here every cell is a named state on or one ulp beside a branch point, halos hold values that make a wrong
neighbour visible, every output starts as 7.0e77, and NormalizeSalinity's grid-stride loop takes its second trip (513 × 257).

Bounds, in units of U = 2⁻⁵³ times M, the largest intermediate term of the cell (ice_atlas returns it); the reference's own
rounding to double (1 U of the result) is included.  net_cell_local, net_face_stress and net_sea_ice_cell have contraction off;
elsewhere an FMA only removes roundings.
  · Q_u = ((εσ)·T²)·T², T = T_s + 273.15: T 1, T² 2·1 + 1 = 3, εσ 1, product 1 + 3 + 1 = 5, product 5 + 3 + 1 = 9 (relative)
  · net sea ice, top: Q_u 9; (1 − α) 1, ·Q_s 1; ε·Q_ℓ 1; the difference Q_d 1; three sums 3; reference 1       → 17 U·M
    bottom: one sum, reference                                                                                  →  2 U·M
  · net ocean JT: Q_u 9, −εQ_ℓ 1, three sums 3 = 13; (1 − ℵ) 1, product 1 = 15; Q_ss = (1 − α)·Q_s·(1 − ℵ): (1 − α) 2 (the
    latitude-dependent α = α_d − α_dir cos 2φ adds < 1 U of 1: α_dir = 0.011), 2 products, (1 − ℵ) 1 = 5; sum 1 = 21;
    ρ⁻¹c⁻¹: 2 reciprocals + product 3; SQ·roc 1 = 25; Q_io·roc 3 + 1 = 4; sum 1; reference 1 = 31                 → 32 U·M
  · JS: ρ_f⁻¹ 1, two products 2·… ≤ 3 with the sum; −S·SF 1; (1 − ℵ)· 2 = 6; land term 3; two sums 2; reference 1  → 12 U·M
  · shortwave flux: Q_ts 5, roc 3, product 1, reference 1 → 10; upwelling longwave 9 + 1 → 10; downwelling longwave 1 + 1 → 2;
    downwelling shortwave 5 + 1 → 6
  · face stress: (ρτ_a + ρτ_b) 1, ρ⁻¹ 1, product 1 = 3; face ℵ 1; (1 − ℵ) 1 (of 1), product 1 = 6; ℵ·τ_io 1 + 1 = 2; sum 1;
    reference 1                                                                                                   → 10 U·M
  · restoring v_p (S − S★): difference 1, product 1, reference 1                                                   →  3 U·|result|
  · CCSM3 albedo (every term ≤ 1, so M = 1): f_h: two atan at 2 ulp = 4 U each, quotient 1 = 9; 1 − f_h 1; f_T ≤ 5;
    bare ice ≤ 0.78·9 + 1 + 0.06·11 + 0.075·5 + 1 + 2 ≈ 12; snow ≤ 3; cover 2, 1 − cover 3; band ≤ max(12 + 3 + 1, …) + 1 = 17;
    broadband: 1 − f_vis 1, products 1, sum 1 = 20; reference 1 = 21                                              → 24 U
The three-equation solve is conditioned by B² / 4AC, so its bound is measured, as the issue that asked for this file prescribes:
the C oracle's worst error against the reference over the whole atlas in the metric |Δ| / max(|ref|, scale), scales
(1, 1e-7, 1, 1e-3) as in test_sea_ice_physics.py, measured on the CPU (TE_ORACLE_WORST below; asserted there), the device gets
4 × that and never more than 1e-9 (TE_BOUND).  Measured: interface heat 4.11e-11 (at|S=45|a=1 under a halo stress: the exact
answer is −7e-12 W m⁻², ρ c α_h u★ ≈ 1e5 W m⁻² K⁻¹ times an ulp of T_f), salt flux 7.59e-11 (30_above|S=S_ice|a=1: exact answer
0, the root's rounding times α_s u★), frazil heat 3.20e-12 (ulp_below|S=45: ρ c Δz / Δt times the rounding of T_f), friction
velocity 1.41e-16.  Recorded rounded up: 4.2e-11, 7.6e-11, 3.2e-12, 1.5e-16; device bounds 1.68e-10, 3.04e-10, 1.28e-11, 6.0e-16.
NormalizeSalinity: |mean − exact| ≤ n·2⁻⁵³·Σ|v·A| / ΣA with n the wet count; every cell of the parent is fl(flux − mean_device)
bit for bit; repeat calls give the same bits.

Which entries catch which defect of the model (test_each_defect_is_caught asserts one named entry per flag and prints all):
west / south faces, y-face stride — cells at a jump of the stress pattern and the last column / row (halo stresses 4 … 8); a ≥ 0 —
every wet a=0 entry with a non-zero stress or floor (u★); negative root — every a>0 entry; floor dropped — zero-stress cells
of the surface with u★_min = 0.02; T before the clamp — the 0.1_below entries with ice and Δt > 0; albedo f_T — the far_below
entries (f_T = 39 or 79 unclamped), f_h — hi=5m, snow at zero — hs=0 and −0, bands swapped — every entry of the second parameter
set; floor `<=` — S=S_min entries with rain or river; land × (1 − ℵ) — river entries with ℵ > 0; land unfloored — river entries
below S_min; face ℵ — cells whose west / south neighbour holds another ℵ; stress side — every cell (two orders between neighbours);
shortwave in JT — every cell of a penetrating config with ℵ < 1; latitude index — the general-storage config; top ungated — a=0;
emissivity — every a>0 entry; second trip, land included, interior only — the cancelling 513 × 257 cases (and every case for the last).
`To <= Tf` changes no output bit and is asserted to be equivalent instead.

The GPU tests below were written without a device at hand and had not run on one when this file was committed (their Python
side was exercised against a stand-in context backed by the C oracle).
"""
import ctypes as C
import functools
from fractions import Fraction

import numpy as np
import pytest

import ice_atlas as ia
import numpy_oracle as npo
import oracle as orc
from coflux import abi
from coflux import interface_computations as ic
from coflux import synthetic as syn

gpu = pytest.mark.gpu
U = ia.U
NX, NY, HX, HY, INNER = ia.NX, ia.NY, ia.HX, ia.HY, ia.INNER

# the C oracle's worst error against the reference over the three surfaces (measured on the CPU, rounded up; asserted below)
TE_ORACLE_WORST = dict(interface_heat=4.2e-11, salt_flux=7.6e-11, frazil_heat=3.2e-12, friction_velocity=1.5e-16)
TE_BOUND = {k: min(4.0 * v, 1e-9) for k, v in TE_ORACLE_WORST.items()}
TE_NULLABLE = (("conc", "tx", "ty"), ("tx", "ty"), ("conc", "ty"), ("conc", "tx"))     # all given, then each input absent in turn


# ---------------------------------------------------------------------------------------------
# shared, computed once
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def te(s):
    return ia.te_surface(s)


@functools.lru_cache(maxsize=None)
def te_ref(s, use=TE_NULLABLE[0]):
    return ia.ref_three_equation(te(s), use)


@functools.lru_cache(maxsize=None)
def alb(s):
    F = ia.albedo_fields(ia.ALBEDO_SETS[s])
    return F, ia.ref_albedo(ia.ALBEDO_SETS[s], F["hi"], F["hs"], F["Ts"]), ia.ref_albedo(ia.ALBEDO_SETS[s], F["hi"], None, F["Ts"])


@functools.lru_cache(maxsize=None)
def nsi():
    return ia.nsi_fields()


NSI_VARIANTS = ((True, True, True), (False, True, True), (True, False, True), (True, True, False), (False, False, False))


@functools.lru_cache(maxsize=None)
def nsi_ref(variant=NSI_VARIANTS[0]):
    return ia.ref_net_sea_ice(nsi(), ia.NSI_PARAMS, *variant)


@functools.lru_cache(maxsize=None)
def no(config):
    F = ia.no_surface(config)
    return F, ia.ref_net_ocean(F)


@functools.lru_cache(maxsize=None)
def restoring():
    R = ia.restoring_fields()
    return R, ia.ref_restoring(R)


@functools.lru_cache(maxsize=None)
def nz(name):
    c = ia.nz_case(name)
    return c, ia.nz_exact(c)


def _excess(got, ref, bound):
    """The largest |got − ref| / bound over ALL cells (0 / 0 = 0: where the bound is zero the result must be the reference's bits)."""
    d = np.abs(np.asarray(got, dtype=np.float64) - ref)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(bound > 0, d / bound, np.where(d == 0, 0.0, np.inf))
    r = np.where(np.isnan(d), np.inf, r)
    return r


def _within(got, ref, bound, label):
    r = _excess(got, ref, bound)
    print("%-60s worst |Δ| / bound = %.3g" % (label, r.max(initial=0.0)))
    assert r.max(initial=0.0) <= 1.0, (label, "|Δ| / bound", float(r.max()), "at", np.unravel_index(np.argmax(r), r.shape))


def _te_within(got, ref, label, bound=TE_BOUND):
    for k in ia.TE_OUTPUTS:
        e = ia.scaled_error(got[k], ref[k], ia.TE_SCALES[k])
        print("%-60s %-18s worst scaled error %.3g (bound %.3g)" % (label, k, e.max(), bound[k]))
        assert e.max() <= bound[k], (label, k, float(e.max()), np.unravel_index(np.argmax(e), e.shape))


def _flux_params(cfg=None, mask_kind=abi.MASK_U8, fluxes=None):
    cfg = cfg or ia.NO_CONFIGS["constant"]
    albedo = cfg["albedo"] if cfg["latitude"] is None else ic.LatitudeDependentAlbedo(*cfg["albedo"])
    return ic.flux_params(fluxes, ocean_surface=ic.SurfaceRadiationProperties(albedo=albedo, emissivity=cfg["emissivity"]),
                          ocean_minimum_salinity=ia.S_MIN, mask_kind=mask_kind, penetrating_shortwave=bool(cfg["penetrating"]))


def _struct(cls, default, values):
    p = cls()
    assert default(C.byref(p)) == 0
    for k, v in values.items():
        setattr(p, k, v)
    return p


def _ice_ocean_params(Q):
    return _struct(abi.IceOceanParams, abi.load_library().cf_default_ice_ocean_params, Q)


def _albedo_params(A):
    return _struct(abi.SeaIceAlbedoParams, abi.load_library().cf_default_sea_ice_albedo_params, A)


def _sea_ice_params():
    K = ia.NSI_PARAMS
    return ic.SeaIceInterfaceProperties(albedo=K["albedo"], emissivity=K["emissivity"], temperature_offset=K["T_offset"]).to_params()


def _mask(F, kind):
    return {abi.MASK_NONE: None, abi.MASK_U8: F["mask"], abi.MASK_BOTTOM_HEIGHT: F["bottom_height"]}[kind]


def _no_host_inputs(F):
    """(ocean, atmos, fluxes, ice, weights, land) dicts of parent arrays as the entry point takes them."""
    cfg = F["cfg"]
    z = np.zeros(ia.SHAPE)
    ocean = dict(T=z, S=F["S"], u=z, v=z, mask=F["mask"])
    atmos = dict(u=z, v=z, T=z, p=z, q=z, Qs=F["Qs"], Ql=F["Ql"], Mp=F["Mp"])
    fluxes = dict(sensible_heat=F["Qc"], latent_heat=F["Qv"], water_vapor=F["Mv"], x_momentum=F["rtx"], y_momentum=F["rty"], temperature=F["Ts"])
    names = dict(concentration="conc", interface_heat="Qio", salt_flux="Jsio", x_stress="txio", y_stress="tyio")
    ice = {k: F[names[k]] for k in cfg["ice"]} or None
    weights = None if cfg["latitude"] is None else dict(separable=cfg["latitude"] == "separable", latitude=F["latitude"])
    return ocean, atmos, fluxes, ice, weights, (F["land"] if cfg["land"] else None)


# =============================================================================================
# CPU: the atlas
# =============================================================================================
def test_atlas_entries_have_the_property_they_are_named_for():
    m = ia.TE_PARAMS["liquidus_slope"]
    seen = set()
    for s in range(len(ia.TE_SURFACES)):
        F = te(s)
        T, S, a = F["T"][INNER], F["S"][INNER], F["conc"][INNER]
        for j in range(NY):
            for i in range(NX):
                t, (sn, So), (an, conc) = ia.TE_STATES[F["state"][j, i]]
                Tf = -m * S[j, i]                                        # the double product the kernel branches on
                assert S[j, i] == So and a[j, i] == conc and F["names"][j, i] == "%s|S=%s|a=%s" % (t, sn, an)
                d = T[j, i] - Tf
                if t == "at":
                    assert T[j, i] == Tf and not T[j, i] < Tf
                elif t == "ulp_above":
                    assert T[j, i] > Tf and np.nextafter(T[j, i], -np.inf) == Tf
                elif t == "ulp_below":
                    assert T[j, i] < Tf and np.nextafter(T[j, i], np.inf) == Tf
                else:
                    want = {"1e-9_above": 1e-9, "0.1_above": 0.1, "0.1_below": -0.1, "2_above": 2.0, "30_above": 30.0}[t]
                    assert abs(d - want) <= 2e-14 + 1e-6 * abs(want) * (t == "1e-9_above")
                if F["wet"][j, i]:
                    seen.add(int(F["state"][j, i]))
        assert S.min() == 0.0 and (S == 4.0).any() and (S == ia.up(4.0)).any() and S.max() == 45.0
        assert set(np.unique(a)) == {0.0, ia.TINY, 1e-12, 0.15, 1.0}
    assert seen == set(range(len(ia.TE_STATES))), "every three-equation state is wet on some surface"
    # the face stresses: exact zeros, −0.0, 1e-12, a 3-4-5 pair whose |τ| is exact, faces that differ by orders of magnitude
    F = te(0)
    tx, ty = F["tx"], F["ty"]
    txc = 0.5 * (tx[INNER] + tx[HY:HY + NY, HX + 1:HX + NX + 1])
    tyc = 0.5 * (ty[INNER] + ty[HY + 1:HY + NY + 1, HX:HX + NX])
    assert ((txc == 0) & (tyc == 0)).any() and (np.signbit(tx[INNER]) & (tx[INNER] == 0)).any() and (tx[INNER] == 1e-12).any()
    pyth = (txc == 3 * ia.S345) & (tyc == 4 * ia.S345)
    assert pyth.any() and Fraction(3 * ia.S345) ** 2 + Fraction(4 * ia.S345) ** 2 == Fraction(5 * ia.S345) ** 2
    east, west = tx[HY:HY + NY, HX + 1:HX + NX + 1], tx[INNER]
    north, south = ty[HY + 1:HY + NY + 1, HX:HX + NX], ty[INNER]
    assert (np.abs(east) > 100 * np.abs(west)).any() and (np.abs(west) > 100 * np.abs(east)).any()
    assert (np.abs(north) > 100 * np.abs(south)).any() and (np.abs(south) > 100 * np.abs(north)).any()
    floors = [ia.TE_SURFACES[s][1] for s in range(3)]
    us = np.sqrt(np.sqrt(txc ** 2 + tyc ** 2))
    assert 0.0 in floors and any(f > 0 and (us < f).any() and (us > f).any() for f in floors), "u★ floor below and above |τ|^½"
    assert {ia.TE_SURFACES[s][2] > 0 for s in range(3)} == {True, False}, "frazil on and off"
    # CCSM3: exact kinks (every temperature parameter is dyadic), hi and hs at their branch points; one set is non-default
    for A in ia.ALBEDO_SETS:
        F = ia.albedo_fields(A)
        fr = lambda x: Fraction(float(x))      # noqa: E731
        for k in range(F["hi"].size):
            t, h, c = ia.ALBEDO_STATES[F["state"].ravel()[k]]
            fT = (fr(A["melting_temperature"]) - fr(F["Ts"].ravel()[k])) / fr(A["melt_temperature_range"]) - 1
            assert {"melt_onset": fT == 0, "melt_onset_ulp_above": -1e-15 < fT < 0, "melt_onset_ulp_below": 0 < fT < 1e-15, "melting": fT == -1,
                    "melting_ulp_above": -1 - 1e-15 < fT < -1, "melting_ulp_below": -1 < fT < -1 + 1e-15, "mid_range": fT == Fraction(-1, 2),
                    "above_melting": fT < -1, "far_below": fT > 10}[t], (t, float(fT))
            hi, hs = F["hi"].ravel()[k], F["hs"].ravel()[k]
            href = A["reference_thickness"]
            assert {"0": hi == 0, "tiny": 0 < hi < 1e-200, "h_ref": hi == href, "h_ref_ulp_above": hi == ia.up(href),
                    "h_ref_ulp_below": hi == ia.down(href), "5m": hi == 5.0}[h]
            assert {"0": hs == 0 and not np.signbit(hs), "-0": hs == 0 and np.signbit(hs), "denormal": hs == ia.TINY,
                    "patch": hs == A["snow_patch_thickness"], "10m": hs == 10.0}[c]
        assert set(F["state"].ravel()) == set(range(len(ia.ALBEDO_STATES))), "every state, halos included in the tiling"
    assert ia.ALBEDO_SETS[1]["visible_fraction"] != 0.5 and ia.ALBEDO_SETS[1]["melting_temperature"] != 0.0
    # net sea ice: ℵ ∈ {0, denormal, 1} each on wet cells, and land
    F = nsi()
    for name, a in ia.NSI_CONCENTRATIONS:
        hit = (F["conc"][INNER] == a) & F["wet"]
        assert hit.any() and all(n == "a=" + name for n in F["names"][hit])
    assert (~F["wet"]).any() and ia.NSI_PARAMS["emissivity"] != 1.0
    # net ocean: the 27 combinations of (ℵ, ℵ west, ℵ south) away from the halo, both arms of both floors, the three salinities at S_min
    F, _ = no("constant")
    a = F["conc"]
    combos = {(a[j, i], a[j, i - 1], a[j - 1, i]) for j in range(HY + 1, HY + NY) for i in range(HX + 1, HX + NX) if F["wet"][j - HY, i - HX]}
    assert len(combos) == 27, len(combos)
    S, Mp, Mv, Ml, wet = F["S"][INNER], F["Mp"][INNER], F["Mv"][INNER], F["land"][INNER], F["wet"]
    for So in (ia.S_MIN, ia.up(ia.S_MIN), ia.down(ia.S_MIN)):
        for rain in (True, False):
            for river in (True, False):
                assert (wet & (S == So) & ((Mp > Mv) == rain) & ((Ml > 0) == river)).any(), (So, rain, river)
    assert (wet & (S < ia.S_MIN) & (Mp < Mv) & (Ml > 0)).any(), "rain arm open, land arm floored"
    assert {c["penetrating"] for c in ia.NO_CONFIGS.values()} == {0, 1}
    assert {c["latitude"] for c in ia.NO_CONFIGS.values()} == {None, "separable", "general"}
    assert any(c["emissivity"] != 1.0 for c in ia.NO_CONFIGS.values())
    assert any("x_stress" in c["ice"] for c in ia.NO_CONFIGS.values()) and any(c["ice"] and "x_stress" not in c["ice"] for c in ia.NO_CONFIGS.values())
    assert {c["land"] for c in ia.NO_CONFIGS.values()} == {True, False}
    for config in ("latitude_1d", "latitude_2d"):
        lat = no(config)[0]["latitude"]
        inner = lat[HY:HY + NY] if lat.ndim == 1 else lat[INNER]
        assert set(np.unique(inner)) == set(ia.NO_LATITUDES)
    # restoring: exact zeros where S == target
    R, ref = restoring()
    same = (R["S"][INNER] == R["target"][INNER]) & R["wet"]
    assert same.any() and np.all(ref[same] == 0.0) and (ref != 0).any()
    # NormalizeSalinity: the cases are what they are named for
    c, (mean, bound, n) = nz("cancelling")
    assert c["nx"] * c["ny"] == 131841 > ia.NZ_MAX_BLOCKS * ia.NZ_BLOCK and n == 2 * 769
    tail = c["wet"].ravel()[ia.NZ_MAX_BLOCKS * ia.NZ_BLOCK:]
    assert tail.all() and tail.size == 769 and 0 < float(mean) < 3e-12 and np.abs(c["flux"][c["inner"]][c["wet"]]).min() > 9e-4
    c, (mean, bound, n) = nz("constant")
    assert mean == Fraction(2.5e-7) and n > 300 and c["area"] is not None
    c, (mean, bound, n) = nz("one_wet_cell")
    assert n == 1 and c["mask_kind"] == "bottom_height" and c["additional"] is not None
    c, (mean, bound, n) = nz("all_land")
    assert n == 0 and mean == 0
    assert nz("one_cell")[0]["shape"] == (3, 3) and nz("cancelling_bottom_height")[0]["area"] is None


def test_layout_puts_wet_ice_at_every_edge_next_to_a_halo_that_differs():
    assert NX * NY == 335 and 256 < NX * NY < 512 and (NX * NY - 256) % 64 != 0 and HX != HY
    inner = ia.interior_mask()
    for F, fields, stress in [(te(s), ("T", "S", "conc", "tx", "ty"), ("tx", "ty")) for s in range(3)] + \
                             [(no("constant")[0], ("S", "conc", "rtx", "rty", "Qs", "Ql", "Ts", "Qc", "Qv", "Mp", "Mv", "land", "Qio", "Jsio", "txio", "tyio"), ("rtx", "rty"))]:
        for k in fields:
            halo = F[k][~inner]
            assert np.unique(halo).size == halo.size and not np.isin(halo, F[k][inner]).any(), k      # designed, no periodic copies
        icy = F["wet"] & (F["conc"][INNER] > 0)
        edges = dict(west=(slice(None), 0, (0, -1)), east=(slice(None), NX - 1, (0, 1)), south=(0, slice(None), (-1, 0)), north=(NY - 1, slice(None), (1, 0)))
        for edge, (jj, ii, (dj, di)) in edges.items():
            ok = np.zeros((NY, NX), bool)
            ok[jj, ii] = True
            ok &= icy
            for k in ("conc",) + stress:
                here, there = F[k][INNER], F[k][HY + dj:HY + NY + dj, HX + di:HX + NX + di]
                ok &= (np.abs(there) >= 10 * np.abs(here)) | (np.abs(here) >= 10 * np.abs(there))
            assert ok.any(), (edge, "no wet ice-covered cell whose halo neighbour differs by a factor 10 in ℵ and τ")


def test_reference_equals_hand_worked_cells():
    # three equations: at S_o = S_i the root is S_b = S_i whatever T_o is: no salt flux, Q = ℵ ρ c α_h u★ (T_o + m S_i)
    Q, O = ia.TE_PARAMS, ia.OCEAN
    one = dict(T=np.full(ia.SHAPE, 1.0), S=np.full(ia.SHAPE, 4.0), conc=np.full(ia.SHAPE, 0.5), tx=np.full(ia.SHAPE, 3 * ia.S345),
               ty=np.full(ia.SHAPE, 4 * ia.S345), wet=np.ones((NY, NX), bool), params=Q)
    r = ia.ref_three_equation(one)
    us = (5 * ia.S345) ** 0.5
    want = 0.5 * O["rho_o"] * O["c_o"] * 0.0095 * us * (1.0 + 0.054 * 4.0)
    assert abs(r["interface_heat"][2, 5] - want) < 1e-13 * want and abs(r["salt_flux"][2, 5]) < 1e-40 and abs(r["friction_velocity"][2, 5] - us) < 1e-17
    # … water 0.1 K below freezing: ρ c Δz (−0.1)/Δt of frazil heat and then no exchange (T_o = T_f ⇒ S_b = S_o)
    one.update(S=np.full(ia.SHAPE, 34.0), T=np.full(ia.SHAPE, -0.054 * 34.0 - 0.1))
    r = ia.ref_three_equation(one)
    want = O["rho_o"] * O["c_o"] * 5.0 * (-0.1) / 1200.0
    assert abs(r["frazil_heat"][0, 0] - want) < 1e-12 * abs(want) and abs(r["interface_heat"][0, 0]) < 1e-10 and abs(r["salt_flux"][0, 0]) < 1e-18
    # CCSM3 (Briegleb et al. 2004): thick cold bare ice, the melting point, vanishing ice, deep cold snow, half way through the range
    A = ia.ALBEDO_SETS[0]
    cell = lambda hi, hs, Ts: float(ia.ref_albedo_cell(A, hi, hs, Ts))      # noqa: E731
    assert abs(cell(2.0, 0.0, -20.0) - 0.57) < 2e-16 and abs(cell(2.0, 0.0, 0.0) - (0.57 - 0.075)) < 2e-16
    assert abs(cell(0.0, 0.0, -20.0) - 0.06) < 1e-17 and abs(cell(2.0, 0.0, -0.5) - (0.57 - 0.0375)) < 2e-16
    assert abs(cell(2.0, 10.0, -20.0) - (0.84 * 10 / 10.02 + 0.57 * 0.02 / 10.02)) < 2e-16
    assert abs(cell(2.0, 0.0, 1.0) - (0.57 - 0.15)) < 2e-16                  # f_T goes on below −1 above the melting point (as defined)
    # net sea ice, ℵ = 1: −(1 − α) Q_s − ε Q_ℓ + ε σ T⁴ + Q_c + Q_v; ℵ = 0: top 0, bottom Q_f + Q_i
    F = nsi()
    top, bot, Mt, Mb = nsi_ref()
    K = ia.NSI_PARAMS
    for (j, i) in ((0, 0), (0, 1), (0, 2), (3, 40)):
        J, I = j + HY, i + HX
        if not F["wet"][j, i]:
            assert top[j, i] == 0 and bot[j, i] == 0
            continue
        want = (-(1 - F["albedo"][J, I]) * F["Qs"][J, I] - K["emissivity"] * F["Ql"][J, I] + K["emissivity"] * K["sigma"] * (F["Ts"][J, I] + 273.15) ** 4
                + F["Qc"][J, I] + F["Qv"][J, I])
        assert (abs(top[j, i] - want) < 1e-12 * Mt[j, i]) if F["conc"][J, I] > 0 else top[j, i] == 0.0
        assert abs(bot[j, i] - (F["Qf"][J, I] + F["Qi"][J, I])) < 1e-13 * Mb[j, i]
    # net ocean without ice or land: JT = (εσT⁴ + Q_c + Q_v − εQ_ℓ)/(ρ c), JS = −S (M_v − M_p)/ρ_f (0 below S_min in rain), τ = ½(ρτ_w + ρτ)/ρ
    F, ref = no("no_ice")
    O = ia.OCEAN
    for (j, i) in ((0, 0), (1, 7), (4, 66), (2, 33)):
        J, I = j + HY, i + HX
        assert F["wet"][j, i]
        JT = (0.97 * ia.SIGMA * (F["Ts"][J, I] + 273.15) ** 4 + F["Qc"][J, I] + F["Qv"][J, I] - 0.97 * F["Ql"][J, I]) / (O["rho_o"] * O["c_o"])
        assert abs(ref["T"][0][j, i] - JT) < 1e-13 * ref["T"][1][j, i]
        SF = (F["Mv"][J, I] - F["Mp"][J, I]) / O["rho_f"]
        JS = 0.0 if (F["S"][J, I] < ia.S_MIN and SF < 0) else -F["S"][J, I] * SF
        assert abs(ref["S"][0][j, i] - JS) < 1e-13 * ref["S"][1][j, i]
        assert abs(ref["u"][0][j, i] - 0.5 * (F["rtx"][J, I - 1] + F["rtx"][J, I]) / O["rho_o"]) < 1e-13 * ref["u"][1][j, i]
        assert abs(ref["v"][0][j, i] - 0.5 * (F["rty"][J - 1, I] + F["rty"][J, I]) / O["rho_o"]) < 1e-13 * ref["v"][1][j, i]
        assert abs(ref["downwelling_shortwave"][0][j, i] - 0.94 * F["Qs"][J, I]) < 1e-13 * F["Qs"][J, I]
    # latitude-dependent albedo at the poles, 45° and the equator: α_d + α_dir, α_d, α_d − α_dir
    F, ref = no("latitude_1d")
    for j, alb_want in enumerate((0.08, 0.069, 0.058, 0.069, 0.08)):
        i = int(np.argmax(F["wet"][j] & (F["conc"][j + HY, HX:HX + NX] == 0)))
        assert abs(ref["downwelling_shortwave"][0][j, i] - (1 - alb_want) * F["Qs"][j + HY, i + HX]) < 1e-13 * F["Qs"][j + HY, i + HX]
    # NormalizeSalinity: the constant's mean is the constant, the cancelling field's is 1e-12 to its last digit's neighbourhood
    assert nz("constant")[1][0] == Fraction(2.5e-7)
    assert abs(float(nz("cancelling_bottom_height")[1][0]) - 1e-12) < 1e-18


def test_oracles_are_within_the_bounds_on_the_whole_atlas():
    g = orc.make_grid(NX, NY, HX, HY, 1)
    c = INNER
    E, N = (slice(HY, HY + NY), slice(HX + 1, HX + NX + 1)), (slice(HY + 1, HY + NY + 1), slice(HX, HX + NX))
    worst = {k: 0.0 for k in ia.TE_OUTPUTS}
    for s in range(len(ia.TE_SURFACES)):
        F, Q = te(s), te(s)["params"]
        oc = dict(T=F["T"], S=F["S"], u=F["T"], v=F["T"], mask=F["mask"])
        for use in TE_NULLABLE if s == 0 else TE_NULLABLE[:1]:
            ref = te_ref(s, use)
            arg = lambda k: F[k] if k in use else None      # noqa: E731
            got = orc.sea_ice_ocean_fluxes(g, _flux_params(), _ice_ocean_params(Q), oc, arg("conc"), arg("tx"), arg("ty"))
            for k in ia.TE_OUTPUTS:
                worst[k] = max(worst[k], float(ia.scaled_error(got[k][c], ref[k], ia.TE_SCALES[k]).max()))
            zero = np.zeros((NY, NX))
            conc = F["conc"][c] if "conc" in use else zero
            Qio, Js, Qfr, us, _ = npo.sea_ice_ocean_fluxes(F["T"][c], F["S"][c], conc, 0.5 * (F["tx"][c] + F["tx"][E]) if "tx" in use else zero,
                                                          0.5 * (F["ty"][c] + F["ty"][N]) if "ty" in use else zero, us_min=Q["minimum_friction_velocity"],
                                                          dz=Q["top_cell_thickness"], dt=Q["time_step"])
            wet = F["wet"]
            _te_within({k: np.where(wet, v, 0.0) for k, v in zip(ia.TE_OUTPUTS, (Qio, Js, Qfr, us))}, ref, "numpy oracle, surface %d %s" % (s, use))
    print("C oracle, three equations, worst scaled errors:", worst)
    for k in ia.TE_OUTPUTS:
        assert worst[k] <= TE_ORACLE_WORST[k], (k, worst[k])
        assert worst[k] >= 0.9 * TE_ORACLE_WORST[k], ("the recorded figure is stale: the device's bound is 4 × the measured one", k, worst[k])
    for s, A in enumerate(ia.ALBEDO_SETS):
        F, ref, ref_bare = alb(s)
        _within(orc.sea_ice_albedo(_albedo_params(A), F["hi"], F["hs"], F["Ts"]), ref, ia.BOUND_ALBEDO * U, "C oracle albedo %d" % s)
        _within(orc.sea_ice_albedo(_albedo_params(A), F["hi"], None, F["Ts"]), ref_bare, ia.BOUND_ALBEDO * U, "C oracle albedo %d, no snow" % s)
        kw = dict(ice=(A["ice_visible"], A["ice_near_infrared"]), snow=(A["snow_visible"], A["snow_near_infrared"]), ocean=A["ocean_albedo"],
                  h_ref=A["reference_thickness"], dT=A["melt_temperature_range"], d_ice=A["ice_melt_change"],
                  d_snow=(A["snow_melt_change_visible"], A["snow_melt_change_near_infrared"]), patch=A["snow_patch_thickness"],
                  visible_fraction=A["visible_fraction"], T_melt=A["melting_temperature"])
        with np.errstate(all="ignore"):
            _within(npo.sea_ice_albedo(F["hi"], F["hs"], F["Ts"], **kw), ref, ia.BOUND_ALBEDO * U, "numpy oracle albedo %d" % s)
    F = nsi()
    z = np.zeros(ia.SHAPE)
    oc = dict(T=z, S=z, u=z, v=z, mask=F["mask"])
    at = dict(u=z, v=z, T=z, p=z, q=z, Qs=F["Qs"], Ql=F["Ql"], Mp=z)
    fl = dict(sensible_heat=F["Qc"], latent_heat=F["Qv"], temperature=F["Ts"])
    for variant in NSI_VARIANTS:
        top, bot, Mt, Mb = nsi_ref(variant)
        got = orc.compute_net_sea_ice_fluxes(g, _flux_params(), _sea_ice_params(), dict(concentration=F["conc"], albedo=F["albedo"] if variant[0] else None),
                                             oc, at, fl, F["Qf"] if variant[1] else None, F["Qi"] if variant[2] else None)
        _within(got["top_heat"][c], top, ia.BOUND_NSI_TOP * U * Mt, "C oracle net sea ice top %s" % (variant,))
        _within(got["bottom_heat"][c], bot, ia.BOUND_NSI_BOTTOM * U * Mb, "C oracle net sea ice bottom %s" % (variant,))
    for config in ia.NO_CONFIGS:
        F, ref = no(config)
        ocean, atmos, fluxes, ice, weights, land = _no_host_inputs(F)
        got = orc.compute_net_ocean_fluxes(g, _flux_params(F["cfg"]), ocean, atmos, fluxes, ice=ice, weights=weights, land=land)
        for k in ia.NO_OUTPUTS:
            _within(got[k][c], ref[k][0], ia.BOUND_NO[k] * U * ref[k][1], "C oracle net ocean %s %s" % (config, k))
        cfg = F["cfg"]
        full = None
        if ice is not None:
            full = {k: ice.get(k, z) for k in ("concentration", "interface_heat", "salt_flux", "x_stress", "y_stress")}
        lat2d = None if cfg["latitude"] is None else (np.broadcast_to(F["latitude"][:, None], ia.SHAPE) if cfg["latitude"] == "separable" else F["latitude"])
        albedo = cfg["albedo"] if cfg["latitude"] is None else ic.LatitudeDependentAlbedo(*cfg["albedo"])
        got = npo.net_ocean_fluxes(ocean, atmos, fluxes, hx=HX, hy=HY, ocean_properties=ic.OceanProperties(), albedo=albedo, emissivity=cfg["emissivity"],
                                   min_salinity=ia.S_MIN, penetrating=bool(cfg["penetrating"]), ice=full, latitude2d=lat2d, land=land)
        for k in ia.NO_OUTPUTS:
            _within(got[k][c], ref[k][0], ia.BOUND_NO[k] * U * ref[k][1], "numpy oracle net ocean %s %s" % (config, k))
    for name in ia.NZ_CASES:
        case, (mean, bound, n) = nz(name)
        P = _flux_params(mask_kind=abi.MASK_BOTTOM_HEIGHT if case["mask_kind"] == "bottom_height" else abi.MASK_U8)
        after, got = orc.normalize_salinity_flux(orc.make_grid(case["nx"], case["ny"], case["hx"], case["hy"], case["ring"]), P, case["flux"], case["mask"],
                                                additional=case["additional"], area=case["area"])
        assert abs(Fraction(got) - mean) <= Fraction(bound), (name, got, float(mean), bound)
        np.testing.assert_array_equal(after, case["flux"] - got)


def _caught(bad, names):
    return sorted(set(names[bad])) if bad.any() else []


def test_each_defect_is_caught_by_named_entries_at_the_gpu_bounds():
    """The clean model is within every bound; each flag puts named entries outside it (printed: which entries catch which flag)."""
    found = {}
    # three equations
    for s in range(3):
        F = te(s)
        for use in TE_NULLABLE if s == 0 else TE_NULLABLE[:1]:
            _te_within(ia.model_three_equation(F, None, use), te_ref(s, use), "clean model, surface %d %s" % (s, use))
        clean = ia.model_three_equation(F)
        for flag in ia.TE_FLAGS:
            got = ia.model_three_equation(F, flag)
            bad = np.zeros((NY, NX), bool)
            for k in ia.TE_OUTPUTS:
                bad |= ia.scaled_error(got[k], te_ref(s)[k], ia.TE_SCALES[k]) > TE_BOUND[k]
            found.setdefault(flag, []).extend(_caught(bad, F["names"]))
        for flag in ia.EQUIVALENT_FLAGS:
            got = ia.model_three_equation(F, flag)
            for k in ia.TE_OUTPUTS:
                assert np.array_equal(got[k].view(np.int64), clean[k].view(np.int64)), (flag, k, "was declared output-equivalent")
    # albedo
    for s, A in enumerate(ia.ALBEDO_SETS):
        F, ref, ref_bare = alb(s)
        with np.errstate(all="ignore"):
            _within(ia.model_albedo(A, F["hi"], F["hs"], F["Ts"]), ref, ia.BOUND_ALBEDO * U, "clean albedo model %d" % s)
            _within(ia.model_albedo(A, F["hi"], None, F["Ts"]), ref_bare, ia.BOUND_ALBEDO * U, "clean albedo model %d, no snow" % s)
            for flag in ia.ALBEDO_FLAGS:
                bad = _excess(ia.model_albedo(A, F["hi"], F["hs"], F["Ts"], flag), ref, ia.BOUND_ALBEDO * U) > 1
                found.setdefault(flag, []).extend(_caught(bad, F["names"]))
    # net sea ice
    F = nsi()
    for variant in NSI_VARIANTS:
        top, bot, Mt, Mb = nsi_ref(variant)
        t, b = ia.model_net_sea_ice(F, ia.NSI_PARAMS, None, *variant)
        _within(t, top, ia.BOUND_NSI_TOP * U * Mt, "clean net sea ice model, top %s" % (variant,))
        _within(b, bot, ia.BOUND_NSI_BOTTOM * U * Mb, "clean net sea ice model, bottom %s" % (variant,))
    top, bot, Mt, Mb = nsi_ref()
    for flag in ia.NSI_FLAGS:
        t, b = ia.model_net_sea_ice(F, ia.NSI_PARAMS, flag)
        bad = (_excess(t, top, ia.BOUND_NSI_TOP * U * Mt) > 1) | (_excess(b, bot, ia.BOUND_NSI_BOTTOM * U * Mb) > 1)
        found.setdefault(flag, []).extend(_caught(bad, F["names"]))
    # net ocean
    for config in ia.NO_CONFIGS:
        F, ref = no(config)
        got = ia.model_net_ocean(F)
        for k in ia.NO_OUTPUTS:
            _within(got[k], ref[k][0], ia.BOUND_NO[k] * U * ref[k][1], "clean net ocean model %s %s" % (config, k))
        for flag in ia.NO_FLAGS:
            got = ia.model_net_ocean(F, flag)
            bad = np.zeros((NY, NX), bool)
            for k in ia.NO_OUTPUTS:
                bad |= _excess(got[k], ref[k][0], ia.BOUND_NO[k] * U * ref[k][1]) > 1
            found.setdefault(flag, []).extend("%s:%s" % (config, n) for n in _caught(bad, F["names"]))
    # NormalizeSalinity
    for name in ia.NZ_CASES:
        case, (mean, bound, n) = nz(name)
        after, got = ia.model_normalize(case)
        assert abs(Fraction(got) - mean) <= Fraction(bound), (name, got, float(mean))
        for flag in ia.NZ_FLAGS:
            after, got = ia.model_normalize(case, flag)
            if abs(Fraction(got) - mean) > Fraction(bound) or not np.array_equal(after, case["flux"] - got):
                found.setdefault(flag, []).append(name)
    for flag, names in sorted(found.items()):
        print("%-24s caught by %d entries, e.g. %s" % (flag, len(set(names)), sorted(set(names))[:6]))
    has = lambda flag, *parts: any(all(p in n for p in parts) for n in found.get(flag, ()))      # noqa: E731
    assert has("te_west_south", "a=1") and has("te_y_stride", "a=0.15")
    assert has("te_a_ge", "|a=0") and all(n.endswith("|a=0") for n in found["te_a_ge"])
    assert has("te_negative_root", "30_above", "a=1") and has("te_no_floor", "a=1") and has("te_T_before_clamp", "0.1_below", "a=1")
    assert all(n.startswith("0.1_below") or n.startswith("ulp_below") for n in found["te_T_before_clamp"])
    assert has("alb_fT_unclamped", "Ts=far_below") and all("far_below" in n for n in found["alb_fT_unclamped"])
    assert has("alb_fh_unclamped", "hi=5m") and all("hi=5m" in n for n in found["alb_fh_unclamped"])
    assert has("alb_snow_at_zero", "hs=0") and has("alb_snow_at_zero", "hs=-0") and all(n.endswith("hs=0") or n.endswith("hs=-0") for n in found["alb_snow_at_zero"])
    assert has("alb_bands_swapped", "Ts=far_below")
    assert has("nsi_top_ungated", "a=0") and set(found["nsi_top_ungated"]) == {"a=0"} and has("nsi_no_emissivity", "a=1")
    assert has("no_floor_le", "S=S_min|") and all("S=S_min|" in n for n in found["no_floor_le"])
    assert has("no_land_ice_masked", "river") and all("river" in n for n in found["no_land_ice_masked"])
    assert has("no_land_unfloored", "S=20|", "river") and all("river" in n and ("S=20|" in n or "S=S_min_ulp_below|" in n) for n in found["no_land_unfloored"])
    assert has("no_face_ice_cell_only", "a=1,west=0") and has("no_stress_wrong_side", "constant:") and has("no_sw_in_JT", "constant:", "a=0,")
    assert has("no_lat_wrong_index", "latitude_2d:") and all(n.startswith("latitude_2d:") for n in found["no_lat_wrong_index"])
    assert "cancelling" in found["nz_second_trip_dropped"] and "cancelling_bottom_height" in found["nz_second_trip_dropped"]
    assert "cancelling" in found["nz_land_included"] and "constant" in found["nz_land_included"]
    assert set(found["nz_interior_only"]) >= {"cancelling", "constant", "one_wet_cell", "one_cell"}
    assert set(found) == set(ia.TE_FLAGS + ia.ALBEDO_FLAGS + ia.NSI_FLAGS + ia.NO_FLAGS + ia.NZ_FLAGS)


# =============================================================================================
# GPU
# =============================================================================================
def _context(P, ring=1, shape=(NX, NY, HX, HY)):
    from coflux.runtime import FluxContext
    return FluxContext(*shape, P, ring=ring)


def _sentinels(ctx, names):
    import torch
    return {k: torch.full(ctx.shape, ia.SENTINEL, dtype=torch.float64, device=ctx.device) for k in names}


def _footprint(t, written, label):
    """Every cell the entry point is documented to write holds a result, every other cell still the sentinel."""
    a = t.cpu().numpy()
    assert not (a[written] == ia.SENTINEL).any(), (label, "a sentinel survived inside the footprint", np.argwhere((a == ia.SENTINEL) & written)[:4])
    assert np.isfinite(a[written]).all(), label
    assert (a[~written] == ia.SENTINEL).all(), (label, "written outside the footprint", np.argwhere((a != ia.SENTINEL) & ~written)[:4])
    return a


def _dev(ctx, d):
    return None if d is None else {k: (ctx.to_device(v) if isinstance(v, np.ndarray) else v) for k, v in d.items() if v is not None}


def _run_three_equation(ctx, F, use=TE_NULLABLE[0], mask_kind=abi.MASK_U8, outputs=ia.TE_OUTPUTS):
    oc = dict(T=ctx.to_device(F["T"]), S=ctx.to_device(F["S"]), u=None, v=None)
    m = _mask(F, mask_kind)
    oc["mask"] = None if m is None else ctx.to_device(m)
    out = _sentinels(ctx, outputs)
    arg = lambda k: ctx.to_device(F[k]) if k in use else None      # noqa: E731
    ctx.compute_sea_ice_ocean_fluxes(_ice_ocean_params(F["params"]), oc, arg("conc"), arg("tx"), arg("ty"), out)
    ctx.sync()
    inner = ia.interior_mask()
    return {k: _footprint(out[k], inner, "three equations " + k)[INNER] for k in outputs}


@gpu
@pytest.mark.parametrize("s", range(len(ia.TE_SURFACES)))
def test_gpu_three_equation_fluxes_on_the_atlas(s):
    ctx = _context(_flux_params())
    F = te(s)
    full = None
    for use in TE_NULLABLE if s == 0 else TE_NULLABLE[:1]:
        got = _run_three_equation(ctx, F, use)
        full = full or got
        _te_within(got, te_ref(s, use), "device, surface %d, inputs %s" % (s, use))
        for k in ia.TE_OUTPUTS:
            assert np.all(got[k][~F["wet"]] == 0.0), ("land", k)
    if s == 0:      # each optional OUTPUT absent in turn: the others keep their bits
        for absent in ("frazil_heat", "friction_velocity"):
            rest = tuple(k for k in ia.TE_OUTPUTS if k != absent)
            part = _run_three_equation(ctx, F, outputs=rest)
            for k in rest:
                assert np.array_equal(part[k].view(np.int64), full[k].view(np.int64)), (absent, k)
    ctx.close()


@gpu
@pytest.mark.parametrize("s", range(len(ia.ALBEDO_SETS)))
def test_gpu_ccsm3_albedo_on_the_atlas_over_the_whole_parent(s):
    ctx = _context(_flux_params())
    F, ref, ref_bare = alb(s)
    everywhere = np.ones(ia.SHAPE, bool)
    for hs, want, label in ((F["hs"], ref, "snow"), (None, ref_bare, "no snow field")):
        out = _sentinels(ctx, ("albedo",))["albedo"]
        ctx.compute_sea_ice_albedo(_albedo_params(ia.ALBEDO_SETS[s]), ctx.to_device(F["hi"]), None if hs is None else ctx.to_device(hs), ctx.to_device(F["Ts"]), out)
        ctx.sync()
        _within(_footprint(out, everywhere, "albedo"), want, ia.BOUND_ALBEDO * U, "device albedo, set %d, %s" % (s, label))
    ctx.close()


def _nsi_device_inputs(ctx, F, mask_kind=abi.MASK_U8):
    import torch
    z = torch.zeros(ctx.shape, dtype=torch.float64, device=ctx.device)
    m = _mask(F, mask_kind)
    oc = dict(T=z, S=z, u=z, v=z, mask=None if m is None else ctx.to_device(m))
    at = dict(u=z, v=z, T=z, p=z, q=z, Qs=ctx.to_device(F["Qs"]), Ql=ctx.to_device(F["Ql"]), Mp=z)
    fl = dict(sensible_heat=ctx.to_device(F["Qc"]), latent_heat=ctx.to_device(F["Qv"]), water_vapor=z, x_momentum=z, y_momentum=z,
              temperature=ctx.to_device(F["Ts"]))
    return oc, at, fl


@gpu
def test_gpu_net_sea_ice_fluxes_on_the_atlas():
    F = nsi()
    inner = ia.interior_mask()
    for mask_kind in (abi.MASK_U8, abi.MASK_BOTTOM_HEIGHT):
        ctx = _context(_flux_params(mask_kind=mask_kind))
        ctx.set_sea_ice_formulation(_flux_params(mask_kind=mask_kind, fluxes=ic.corrected_atmosphere_sea_ice_fluxes()), _sea_ice_params())
        oc, at, fl = _nsi_device_inputs(ctx, F, mask_kind)
        for variant in NSI_VARIANTS:
            top, bot, Mt, Mb = nsi_ref(variant)
            state = dict(concentration=ctx.to_device(F["conc"]), albedo=ctx.to_device(F["albedo"]) if variant[0] else None)
            out = _sentinels(ctx, ("top_heat", "bottom_heat"))
            ctx.compute_net_sea_ice_fluxes(state, oc, at, fl, out, frazil_heat=ctx.to_device(F["Qf"]) if variant[1] else None,
                                           interface_heat=ctx.to_device(F["Qi"]) if variant[2] else None)
            ctx.sync()
            t, b = (_footprint(out[k], inner, "net sea ice " + k)[INNER] for k in ("top_heat", "bottom_heat"))
            _within(t, top, ia.BOUND_NSI_TOP * U * Mt, "device net sea ice top, mask %d, %s" % (mask_kind, variant))
            _within(b, bot, ia.BOUND_NSI_BOTTOM * U * Mb, "device net sea ice bottom, mask %d, %s" % (mask_kind, variant))
            assert np.all(t[~F["wet"]] == 0) and np.all(b[~F["wet"]] == 0) and np.all(t[F["wet"] & (F["conc"][INNER] == 0)] == 0)
        ctx.close()


def _run_net_ocean(ctx, F, mask_kind=abi.MASK_U8):
    ocean, atmos, fluxes, ice, weights, land = _no_host_inputs(F)
    ocean = dict(ocean, mask=_mask(F, mask_kind))
    d_land = None if land is None else ctx.to_device(land)
    ctx.set_land_freshwater(d_land)
    net = _sentinels(ctx, ia.NO_OUTPUTS)
    ctx.compute_net_ocean_fluxes(_dev(ctx, ocean), _dev(ctx, atmos), _dev(ctx, fluxes), net, ice=_dev(ctx, ice), weights=_dev(ctx, weights))
    ctx.sync()
    ctx.set_land_freshwater(None)
    inner = ia.interior_mask()
    return {k: _footprint(net[k], inner, "net ocean " + k)[INNER] for k in ia.NO_OUTPUTS}


@gpu
@pytest.mark.parametrize("config", tuple(ia.NO_CONFIGS))
def test_gpu_net_ocean_fluxes_on_the_atlas(config):
    F, ref = no(config)
    ctx = _context(_flux_params(F["cfg"]))
    got = _run_net_ocean(ctx, F)
    for k in ia.NO_OUTPUTS:
        _within(got[k], ref[k][0], ia.BOUND_NO[k] * U * ref[k][1], "device net ocean %s %s" % (config, k))
        assert np.all(got[k][~F["wet"]] == 0.0), ("land", k)
    ctx.close()


@gpu
def test_gpu_salinity_restoring_on_the_atlas():
    R, ref = restoring()
    ctx = _context(_flux_params())
    oc = dict(T=None, S=ctx.to_device(R["S"]), u=None, v=None, mask=ctx.to_device(R["mask"]))
    out = _sentinels(ctx, ("J",))["J"]
    ctx.materialize_salinity_restoring(ia.PISTON, ctx.to_device(R["target"]), oc, out)
    ctx.sync()
    got = _footprint(out, ia.interior_mask(), "restoring")[INNER]          # halo cells untouched
    _within(got, ref, ia.BOUND_RESTORING * U * np.abs(ref), "device salinity restoring")
    assert np.all(got[~R["wet"]] == 0.0) and np.all(got[(R["S"][INNER] == R["target"][INNER])] == 0.0)
    ctx.close()


@gpu
@pytest.mark.parametrize("name", ia.NZ_CASES)
def test_gpu_normalize_salinity_on_the_atlas(name):
    import torch
    case, (mean, bound, n) = nz(name)
    P = _flux_params(mask_kind=abi.MASK_BOTTOM_HEIGHT if case["mask_kind"] == "bottom_height" else abi.MASK_U8)
    ctx = _context(P, ring=case["ring"], shape=(case["nx"], case["ny"], case["hx"], case["hy"]))
    runs = []
    for repeat in range(2):
        flux = ctx.to_device(case["flux"])
        mean_out = torch.full((1,), ia.SENTINEL, dtype=torch.float64, device=ctx.device)
        ctx.normalize_salinity_flux(flux, ctx.to_device(case["mask"]), additional=None if case["additional"] is None else ctx.to_device(case["additional"]),
                                    area=None if case["area"] is None else ctx.to_device(case["area"]), mean_out=mean_out)
        ctx.sync()
        runs.append((flux.cpu().numpy(), float(mean_out.cpu()[0])))
    after, got = runs[0]
    print("%s: device mean %.17g, exact %.17g, |Δ| %.3g, bound %.3g" % (name, got, float(mean), abs(float(Fraction(got) - mean)), bound))
    assert abs(Fraction(got) - mean) <= Fraction(bound), (name, got, float(mean), bound)
    want = case["flux"] - got                                               # fl(flux − mean_device), every cell of the parent
    assert np.array_equal(after.view(np.int64), want.view(np.int64)), (name, np.argwhere(after != want)[:4])
    if n == 0:
        assert got == 0.0 and np.array_equal(after.view(np.int64), case["flux"].view(np.int64)), "all land: the flux keeps its bits"
    assert runs[1][1] == got and np.array_equal(runs[0][0].view(np.int64), runs[1][0].view(np.int64)), "repeat calls are bitwise equal"
    ctx.close()


# ---------------------------------------------------------------------------------------------
# b. one arithmetic, several launches: bitwise, from sentinel-filled outputs
# ---------------------------------------------------------------------------------------------
def _step_inputs(ctx, F):
    """A whole step's inputs on the atlas surface: synthetic atmosphere and ocean T, u, v; the atlas's S, mask, ℵ and ice fluxes."""
    o = syn.ocean_state(NX, NY, HX, HY)
    ocean = dict(T=o["T"], S=F["S"], u=o["u"], v=o["v"], mask=F["mask"])
    src = {k: ctx.to_device(v) for k, v in syn.jra55_snapshots(2).items()}
    fi, fj, phi = syn.latlon_fractional_indices(NX, NY, HX, HY)
    w = dict(separable=True, fi=ctx.to_device(fi), fj=ctx.to_device(fj), latitude=ctx.to_device(phi))
    ice = dict(concentration=F["conc"], interface_heat=F["Qio"], salt_flux=F["Jsio"], x_stress=F["txio"], y_stress=F["tyio"])
    return _dev(ctx, ocean), src, w, _dev(ctx, ice)


def _bitwise_interior(a, b, label):
    x, y = a.cpu().numpy()[INNER], b.cpu().numpy()[INNER]
    assert not (x == ia.SENTINEL).any() and not (y == ia.SENTINEL).any(), (label, "a sentinel survived on the interior")
    assert np.array_equal(x.view(np.int64), y.view(np.int64)), (label, np.argwhere(x != y)[:4])


@gpu
@pytest.mark.parametrize("mode", (abi.ICE_FREE_ITERATE, abi.ICE_FREE_ZERO))
def test_gpu_fused_epilogue_and_separate_net_ocean_kernel_agree_bitwise_from_sentinels(mode):
    from coflux.runtime import EXCHANGE_NAMES, FLUX_NAMES
    F, _ = no("constant")
    assert (~F["wet"]).any() and (F["wet"] & (F["conc"][INNER] == 0)).any()
    ctx = _context(_flux_params(F["cfg"]))
    ctx.set_option(abi.OPT_ICE_FREE_CELLS, mode)
    ctx.set_option(abi.OPT_FUSED_NET, 1)
    assert ctx.solver_path()[1] >= 1, "the net fluxes are not in the solver's epilogue"
    ocean, src, w, ice = _step_inputs(ctx, F)
    land = ctx.to_device(F["land"])
    ctx.set_land_freshwater(land)
    atmos, fl, fused = _sentinels(ctx, EXCHANGE_NAMES), _sentinels(ctx, FLUX_NAMES), _sentinels(ctx, ia.NO_OUTPUTS)
    ctx.update_state(src, w, ocean, atmos, fl, fused, ice=ice, time_fraction=0.37)
    separate = _sentinels(ctx, ia.NO_OUTPUTS)
    ctx.compute_net_ocean_fluxes(ocean, atmos, fl, separate, ice=ice, weights=w)
    ctx.sync()
    for k in ia.NO_OUTPUTS:
        _bitwise_interior(fused[k], separate[k], "net." + k)
        _footprint(fused[k], ia.interior_mask(), "fused net." + k)
        assert np.all(fused[k].cpu().numpy()[INNER][~F["wet"]] == 0.0), ("land", k)
    ctx.set_land_freshwater(None)
    ctx.close()


@gpu
@pytest.mark.parametrize("mode", (abi.ICE_FREE_ITERATE, abi.ICE_FREE_ZERO))
def test_gpu_interface_epilogue_and_separate_net_sea_ice_kernel_agree_bitwise_from_sentinels(mode):
    from coflux.runtime import EXCHANGE_NAMES, FLUX_NAMES
    F, _ = no("constant")
    N = nsi()
    ctx = _context(_flux_params(F["cfg"]))
    ctx.set_sea_ice_formulation(_flux_params(fluxes=ic.corrected_atmosphere_sea_ice_fluxes()), _sea_ice_params())
    ctx.set_option(abi.OPT_ICE_FREE_CELLS, mode)
    ctx.set_option(abi.OPT_MERGED_PREFETCH, 2)                             # the net sea-ice fluxes ride in the interface solve's epilogue
    ocean, src, w, ice = _step_inputs(ctx, F)
    si = syn.sea_ice_state(NX, NY, HX, HY)
    conc = F["conc"]
    state = _dev(ctx, dict(concentration=conc, thickness=np.where(conc > 0, si["thickness"], 0.0), top_temperature=si["top_temperature"],
                           u=si["u"], v=si["v"], albedo=N["albedo"]))
    frazil, interface = ctx.to_device(N["Qf"]), ctx.to_device(N["Qi"])
    atmos, fl, net, ai = _sentinels(ctx, EXCHANGE_NAMES), _sentinels(ctx, FLUX_NAMES), _sentinels(ctx, ia.NO_OUTPUTS), _sentinels(ctx, FLUX_NAMES)
    in_step = _sentinels(ctx, ("top_heat", "bottom_heat"))
    ctx.update_state_sea_ice(src, w, ocean, atmos, fl, net, ice, state, ai, in_step, frazil_heat=frazil, interface_heat=interface, time_fraction=0.37)
    separate = _sentinels(ctx, ("top_heat", "bottom_heat"))
    ctx.compute_net_sea_ice_fluxes(state, ocean, atmos, ai, separate, frazil_heat=frazil, interface_heat=interface)
    ctx.sync()
    for k in ("top_heat", "bottom_heat"):
        _bitwise_interior(in_step[k], separate[k], k)
        a = _footprint(in_step[k], ia.interior_mask(), "in-step " + k)[INNER]
        assert np.all(a[~F["wet"]] == 0.0), ("land", k)
    assert np.all(in_step["top_heat"].cpu().numpy()[INNER][F["wet"] & (conc[INNER] == 0)] == 0.0)
    for k in ia.NO_OUTPUTS:
        _footprint(net[k], ia.interior_mask(), "net." + k)
    ctx.close()


# ---------------------------------------------------------------------------------------------
# c. rings 0 and 1, mask kinds none / u8 / bottom height: land exactly zero, wet cells the same bits as (a)
# ---------------------------------------------------------------------------------------------
@gpu
def test_gpu_rings_and_mask_kinds_give_the_same_bits_on_wet_cells():
    F, _ = no("constant")
    T = te(0)
    base_no = base_te = None
    for ring in (1, 0):
        for mask_kind in (abi.MASK_U8, abi.MASK_BOTTOM_HEIGHT, abi.MASK_NONE):
            ctx = _context(_flux_params(F["cfg"], mask_kind=mask_kind), ring=ring)
            got_no, got_te = _run_net_ocean(ctx, F, mask_kind), _run_three_equation(ctx, T, mask_kind=mask_kind)
            ctx.close()
            if base_no is None:
                base_no, base_te = got_no, got_te                           # ring 1, u8: what (a) compared with the reference
            for got, base, wet in ((got_no, base_no, F["wet"]), (got_te, base_te, T["wet"])):
                for k in got:
                    assert np.array_equal(got[k][wet].view(np.int64), base[k][wet].view(np.int64)), (ring, mask_kind, k)
                    if mask_kind != abi.MASK_NONE:
                        assert np.all(got[k][~wet] == 0.0), (ring, mask_kind, k, "land")
                    assert np.isfinite(got[k]).all(), (ring, mask_kind, k)
