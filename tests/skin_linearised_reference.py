"""NumPy restatement of the atmosphere–sea-ice interface iteration with the linearised skin-temperature scheme
(CF_SKIN_LINEARISED, include/coflux.h): the reference the tests of that scheme hold the HIP kernels to.

The loop is typed again here rather than patched into oracle/numpy_oracle.py; only the oracle's thermodynamics, ψ functions,
roughness lengths and wind-speed scale are imported.  `scheme` also takes CF_SKIN_EXPLICIT and CF_SKIN_SEMI_IMPLICIT, so
that one loop can be compared with itself across schemes.

Each iteration takes one Newton step on the surface energy balance  k (Tᵢ − Tₛ)/h = Q(Tₛ)  about the previous skin
temperature, with the previous iterate's u★ and profile factors χ = κ/D held fixed:
    Q(Tₛ)  = −ρ u★ (ℒ_s q★ + c_p θ★) + Q_d + εσTₛ⁴
    Q'(Tₛ) = 4εσTₛ³ + ρ c_p u★ χ_θ + ρ ℒ_s u★ χ_q · dq_s/dT(Tₛ),   dq_s/dT = q_s ((a_i − 1)/Tₛ + b_i/Tₛ²)
    T★     = (Tᵢ − (h/k)(Q − Q' Tₛ)) / (1 + (h/k) Q')
then the NaN guard, the ±ΔT_max limiter, the cap at the melting point and the similarity step, as in every scheme.

For tests/test_interface_atlas.py the loop can also report which of its branches a cell took (`trace`), run with one of
the DEFECTS seeded, and end an exact period-2 orbit early as the kernels do (`orbit_shortcut`); none of the three is on by
default and the default path computes what it always did."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.join(os.path.dirname(HERE), "oracle"), os.path.join(os.path.dirname(HERE), "climaocean.jl_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy_oracle as npo  # noqa: E402

SKIN_EXPLICIT, SKIN_SEMI_IMPLICIT, SKIN_LINEARISED = 0, 1, 2
# what `defect` takes: one branch of the iteration broken on purpose
DEFECTS = ("cap_dropped", "limiter_one_sided", "hk_min_ignored", "nan_guard_dropped", "vaporisation_for_sublimation",
           "albedo_ignored", "calm_guard_dropped", "gturb_not_carried", "orbit_parity_flipped")


def interface_fluxes(fluxes, iprops, ice, ocean, atmos, *, hx, hy, ring, thermodynamics, scheme=SKIN_LINEARISED,
                     velocity_difference="relative", h=10.0, h_bl=600.0, g=9.81, sigma=5.67e-8, trace=None, defect=None,
                     orbit_shortcut=False):
    """Fluxes, skin temperature and trip counts on the window of `ring` halo cells around the interior (the shape of the
    oracle's outputs: full arrays, zero outside the window).  `fluxes` is a coflux.interface_computations formulation.
    `trace`: a dict that receives, per window cell, which branches were taken (see the end of the loop).  `defect`: one of
    DEFECTS.  `orbit_shortcut`: a cell whose state repeats the one two trips ago bit for bit, unconverged, stops there with
    the iterate that trip `maxiter` would have reached (the kernels' CF_OPT_ICE_ORBIT_SHORTCUT)."""
    assert defect is None or defect in DEFECTS, defect
    from coflux import interface_computations as ic
    th = npo.Thermo(thermodynamics)
    ny, nx = ocean["T"].shape[0] - 2 * hy, ocean["T"].shape[1] - 2 * hx
    W = (slice(hy - ring, hy + ny + ring), slice(hx - ring, hx + nx + ring))
    Ti = iprops.freshwater_melting_temperature - iprops.liquidus_slope * ocean["S"][W]
    wet = ocean["mask"][W] != 0 if ocean.get("mask") is not None else np.ones(Ti.shape, bool)
    ua, va, Ta, pa, qa, Qsw, Qlw = (atmos[k][W] for k in ("u", "v", "T", "p", "q", "Qs", "Ql"))
    ui = ice["u"][W] if ice.get("u") is not None else 0.0
    vi = ice["v"][W] if ice.get("v") is not None else 0.0
    alb = ice["albedo"][W] if ice.get("albedo") is not None else iprops.albedo
    if defect == "albedo_ignored":
        alb = 0.0
    Ts = ice["top_temperature"][W] + iprops.temperature_offset
    air = th.state_pTq(pa, Ta, qa)
    rho, cp, qav = air["rho"], th.cp_m(air), th.q_vapor(air)
    Ls = th.Lv(Ta) if defect == "vaporisation_for_sublimation" else th.Ls0 + (th.cpv - th.cpi) * (Ta - th.T0)
    Qd = -(1 - alb) * Qsw - iprops.emissivity * Qlw
    es = iprops.emissivity * sigma
    # (fmax, fmin: what C and the kernels call — a NaN operand is ignored, not handed on; the same on finite values)
    hk = np.fmax(ice["thickness"][W], iprops.consolidation_thickness) / iprops.conductivity
    if defect == "hk_min_ignored":
        hk = ice["thickness"][W] / iprops.conductivity
    a_i = (th.cpv - th.cpi) / th.Rv
    b_i = (th.Ls0 - (th.cpv - th.cpi) * th.T0) / th.Rv
    if velocity_difference == "relative":
        du, dv = ua - ui, va - vi
    else:
        du, dv = ua + 0 * Ti, va + 0 * Ti
    dU = np.sqrt(du * du + dv * dv)
    delta, kap = th.eps - 1.0, fluxes.von_karman_constant
    stab = fluxes.stability_functions.name
    coare = isinstance(fluxes.similarity_form, ic.COARELogarithmicSimilarityProfile)
    stop = fluxes.solver_stop_criteria
    fixed = isinstance(stop, ic.FixedIterations)
    maxit = stop.iterations if fixed else stop.maxiter

    us = np.full(Ti.shape, 1e-4)
    ts, qq = us.copy(), us.copy()
    gturb = np.zeros(Ti.shape)        # ρ u★ (c_p χ_θ + ℒ_s χ_q dq_s/dT) of the last similarity step; 0 before the first
    its = np.zeros(Ti.shape, np.int32)
    active = np.ones(Ti.shape, bool) if fixed else wet.copy()
    dTm, Tm = iprops.maximum_temperature_change, iprops.freshwater_melting_temperature
    tr = {k: np.zeros(Ti.shape, bool) for k in ("limited_up", "limited_down", "capped", "left_the_cap", "nan_guard",
                                                "zero_buoyancy", "profile_floor", "gust_floor", "orbit")}
    tr["first_limiter_trips"] = np.zeros(Ti.shape, np.int32)     # how many trips from the first on were limited
    tr["first_step"] = np.full(Ti.shape, np.nan)                 # T★ − Tₛ of the first trip, before the limiter
    prev, prev2 = None, None                                     # the states one and two trips ago
    it = 0
    while active.any() and it < maxit:
        Q = -rho * us * (Ls * qq + cp * ts) + Qd + es * Ts ** 4
        if scheme == SKIN_LINEARISED:
            dQ = 4.0 * es * Ts ** 3 + gturb
            Tstar = (Ti - hk * (Q - dQ * Ts)) / (1.0 + hk * dQ)
        elif scheme == SKIN_SEMI_IMPLICIT:
            Tstar = (Ti - hk * (Q - es * Ts ** 4)) / (1.0 + hk * es * Ts ** 3)
        else:
            Tstar = Ti - hk * Q
        tr["nan_guard"] |= active & np.isnan(Tstar)
        if defect != "nan_guard_dropped":
            Tstar = np.where(np.isnan(Tstar), Ts, Tstar)
        step = Tstar - Ts
        if it == 0:
            tr["first_step"] = step
        with np.errstate(invalid="ignore"):
            up, down = active & (step > dTm), active & (step < -dTm)
            dT = np.fmin(step, dTm) if defect == "limiter_one_sided" else np.fmin(np.fmax(step, -dTm), dTm)
            Tn = Ts + dT if defect == "cap_dropped" else np.fmin(Ts + dT, Tm)
        tr["limited_up"] |= up
        tr["limited_down"] |= down
        tr["first_limiter_trips"] += ((up | down) & (tr["first_limiter_trips"] == it))
        tr["left_the_cap"] |= active & (Ts == Tm) & (Tn < Tm)
        tr["capped"] |= active & (Ts + dT >= Tm)
        qs = th.svp(Tn, th.Ls0, th.cpv - th.cpi) / (rho * th.Rv * Tn)
        dq, dth = qav - qs, Ta + g * h / cp - Tn
        surf = th.state_pTq(pa, Tn, qs)
        Tv, qv = th.T_virtual(surf), th.q_vapor(surf)
        b = g / Tv * (ts * (1 + delta * qv) + delta * Tv * qq)
        U = npo._wind_speed_scale(fluxes, -us * b, du * du + dv * dv, h_bl)
        tr["zero_buoyancy"] |= active & (b == 0)
        tr["gust_floor"] |= active & (fluxes.gustiness_parameter * np.cbrt(np.maximum(-us * b, 0.0) * h_bl) <= fluxes.minimum_gustiness)
        lu = npo.momentum_length(fluxes.momentum_roughness_length, g, us, dU, Tn)
        lq = npo.scalar_length(fluxes.water_vapor_roughness_length, lu, us, Tn)
        lt = npo.scalar_length(fluxes.temperature_roughness_length, lu, us, Tn)
        with np.errstate(divide="ignore", invalid="ignore"):
            L = np.where(b == 0, np.inf, us * us / (kap * b))

            def profile(psi, length):
                r = np.log(h / length) - psi(stab, h / L)
                r = r if coare else r + psi(stab, length / L)
                tr["profile_floor"] |= active & (r < fluxes.similarity_profile_floor)
                return np.fmax(r, fluxes.similarity_profile_floor)

            chi_t, chi_q = kap / profile(npo.psi_h, lt), kap / profile(npo.psi_h, lq)
            nus = kap / profile(npo.psi_m, lu) * U
        nts, nqs = chi_t * dth, chi_q * dq
        dqs = qs * ((a_i - 1.0) / Tn + b_i / (Tn * Tn))
        ngturb = rho * nus * (cp * chi_t + Ls * chi_q * dqs)
        if defect == "gturb_not_carried":
            ngturb = 0.0 * ngturb
        drift = np.abs(nus - us) + np.abs(nts - ts) + np.abs(nqs - qq)
        us, ts, qq, Ts, gturb = (np.where(active, n_, o_) for n_, o_ in
                                 ((nus, us), (nts, ts), (nqs, qq), (Tn, Ts), (ngturb, gturb)))
        its += active
        it += 1
        if orbit_shortcut:
            # exact period 2, not converged: trip `maxit` would hold this state again if an even number of trips is left, the one
            # before it otherwise
            now = (us, ts, qq, Ts, gturb)
            with np.errstate(invalid="ignore"):
                repeats = active & ~(drift < (0.0 if fixed else stop.tolerance))
                if prev2 is not None:
                    for n_, o_ in zip(now, prev2):
                        repeats = repeats & (n_ == o_)
                else:
                    repeats = repeats & False
            odd = bool((maxit - it) & 1) != (defect == "orbit_parity_flipped")
            if odd and repeats.any():
                us, ts, qq, Ts, gturb = (np.where(repeats, p_, n_) for n_, p_ in zip(now, prev))
            its = np.where(repeats, maxit, its).astype(np.int32)
            tr["orbit"] |= repeats
            active = active & ~repeats
            prev2, prev = prev, now
        if not fixed:
            active = active & ~(drift < stop.tolerance)

    zero = ~wet
    us, ts, qq = (np.where(zero, 0.0, a) for a in (us, ts, qq))
    with np.errstate(divide="ignore", invalid="ignore"):
        calm = (dU == 0) & (defect != "calm_guard_dropped")
        tx = np.where(calm, 0.0, -us * us * du / dU)
        ty = np.where(calm, 0.0, -us * us * dv / dU)
    if trace is not None:
        trace.update(tr, calm=dU == 0, hk_is_minimum=hk == iprops.consolidation_thickness / iprops.conductivity,
                     ends_on_the_cap=Ts == Tm)
    with np.errstate(invalid="ignore"):
        res = dict(sensible_heat=-rho * cp * us * ts, latent_heat=-rho * us * qq * Ls, water_vapor=-rho * us * qq,
                   x_momentum=rho * tx, y_momentum=rho * ty,
                   temperature=np.where(zero, 0.0, Ts) - iprops.temperature_offset,
                   friction_velocity=us, temperature_scale=ts, humidity_scale=qq,
                   # the surface energy balance at the answer: k (Tᵢ − Tₛ)/h − Q(Tₛ) with the final scales, W m⁻²
                   balance_residual=np.where(zero, 0.0, (Ti - Ts) / hk - (-rho * us * (Ls * qq + cp * ts) + Qd + es * Ts ** 4)))
    out = {}
    for k, a in res.items():
        full = np.zeros(ocean["T"].shape)
        full[W] = np.where(a == 0, 0.0, a)
        out[k] = full
    full = np.zeros(ocean["T"].shape, np.int32)
    full[W] = its
    out["iterations"] = full
    return out


def balance_residual(fluxes_out, iprops, ice, ocean, atmos, *, hx, hy, ring, thermodynamics, sigma=5.67e-8):
    """k (Tᵢ − Tₛ)/h − Q(Tₛ) of any scheme's answer (fluxes of `interface_fluxes` or of the oracle), from its skin temperature
    and its sensible and latent heat fluxes; on the window, W m⁻²."""
    th = npo.Thermo(thermodynamics)
    ny, nx = ocean["T"].shape[0] - 2 * hy, ocean["T"].shape[1] - 2 * hx
    W = (slice(hy - ring, hy + ny + ring), slice(hx - ring, hx + nx + ring))
    Ti = iprops.freshwater_melting_temperature - iprops.liquidus_slope * ocean["S"][W]
    alb = ice["albedo"][W] if ice.get("albedo") is not None else iprops.albedo
    Qd = -(1 - alb) * atmos["Qs"][W] - iprops.emissivity * atmos["Ql"][W]
    hk = np.maximum(ice["thickness"][W], iprops.consolidation_thickness) / iprops.conductivity
    Ts = fluxes_out["temperature"][W] + iprops.temperature_offset
    Q = fluxes_out["sensible_heat"][W] + fluxes_out["latent_heat"][W] + Qd + iprops.emissivity * sigma * Ts ** 4
    return (Ti - Ts) / hk - Q
