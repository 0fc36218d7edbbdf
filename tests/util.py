"""Shared builders for the parity tests: seeded synthetic inputs (coflux.synthetic), the oracle
run on them, and the comparison metric  |Δ| ≤ tol · max(|ref|, field scale)  (SURVEY.md §7 H4:
a pure relative error blows up where a flux crosses zero)."""
import atexit
import os
import shutil
import tempfile

import numpy as np

from coflux import interface_computations as ic
from coflux import synthetic as syn

# field scales used as the floor of the relative-error denominator
FIELD_SCALE = dict(sensible_heat=1.0, latent_heat=1.0, water_vapor=1e-6, x_momentum=1e-3, y_momentum=1e-3,
                   temperature=1.0, friction_velocity=1e-3, temperature_scale=1e-3, humidity_scale=1e-6,
                   u=1e-6, v=1e-6, T=1e-6, S=1e-7, shortwave_surface_flux=1e-6, upwelling_longwave=1.0,
                   downwelling_longwave=1.0, downwelling_shortwave=1.0,
                   p=1.0, q=1e-4, Qs=1.0, Ql=1.0, Mp=1e-6)
ATMOS_SCALE = dict(u=1.0, v=1.0, T=1.0, p=1.0, q=1e-4, Qs=1.0, Ql=1.0, Mp=1e-6)


def rendezvous():
    """init_method for the ranks of one multi-process test: torch.distributed's store in a fresh file.  A TCP port found
    free with bind(0) and closed again can be taken by another process before rank 0 listens on it (EADDRINUSE)."""
    d = tempfile.mkdtemp(prefix="coflux_rdzv_")
    atexit.register(shutil.rmtree, d, True)
    return "file://" + os.path.join(d, "store")

CONFIGS = {
    "default": lambda: (ic.SimilarityTheoryFluxes(), None),
    "corrected": lambda: (ic.corrected_atmosphere_ocean_fluxes(), ic.RelativeVelocity()),
    "corrected_wind": lambda: (ic.corrected_atmosphere_ocean_fluxes(), ic.WindVelocity()),
    "sea_ice_corrected": lambda: (ic.corrected_atmosphere_sea_ice_fluxes(), None),
    "sea_ice_ncar": lambda: (ic.ncar_atmosphere_sea_ice_fluxes(), None),
    "ncar": lambda: (ic.ncar_atmosphere_ocean_fluxes(), None),
    "fixed5": lambda: (ic.SimilarityTheoryFluxes(solver_stop_criteria=ic.FixedIterations(5)), None),
    # launch.sh:67-72,350: `:corrected` with the shear-aware gustiness U_G² = (β w★)² + (0.04 |Δu|)² + U_G,0²
    "shear_aware": lambda: (ic.shear_aware_atmosphere_ocean_fluxes(), ic.RelativeVelocity()),
}


def _with_shear(fluxes, c=0.04):
    fluxes.shear_gustiness_coefficient = c
    return fluxes


# the same gustiness form through the other solver bodies: README defaults (log profile, constant Charnock), constant
# roughness lengths (the generic / sea-ice-type body), Large–Yeager stability functions
SHEAR_CONFIGS = {
    "default_shear": lambda: (_with_shear(ic.SimilarityTheoryFluxes()), None),
    "constant_roughness_shear": lambda: (_with_shear(ic.corrected_atmosphere_sea_ice_fluxes(), 0.08), ic.WindVelocity()),
    "no_convective_gust_shear": lambda: (_with_shear(ic.ncar_atmosphere_sea_ice_fluxes()), None),
}


def _fixed(fluxes, n):
    fluxes.solver_stop_criteria = ic.FixedIterations(n)
    return fluxes


ICE_CONFIGS = {
    "sea_ice_corrected": lambda: (ic.corrected_atmosphere_sea_ice_fluxes(), ic.RelativeVelocity()),
    "sea_ice_ncar": lambda: (ic.ncar_atmosphere_sea_ice_fluxes(), ic.WindVelocity()),
    "sea_ice_default": lambda: (ic.SimilarityTheoryFluxes(), None),
    "sea_ice_fixed5": lambda: (_fixed(ic.corrected_atmosphere_sea_ice_fluxes(), 5), None),
    "sea_ice_shear": lambda: (_with_shear(ic.corrected_atmosphere_sea_ice_fluxes()), ic.RelativeVelocity()),
}


def build_case(nx, ny, hx=3, hy=3, *, weights="latlon", land=True, n_levels=2, ny_global=None, j_offset=0):
    ocean = syn.ocean_state(nx, ny, hx, hy, ny_global=ny_global, j_offset=j_offset, land_fraction=land)
    src = syn.jra55_snapshots(n_levels)
    if weights == "latlon":
        fi, fj, phi = syn.latlon_fractional_indices(nx, ny, hx, hy, ny_global=ny_global, j_offset=j_offset)
        w = dict(separable=True, fi=fi, fj=fj, latitude=phi)
    else:
        fi, fj, c, s, phi = syn.tripolar_like_weights(nx, ny, hx, hy, ny_global=ny_global, j_offset=j_offset)
        w = dict(separable=False, fi=fi, fj=fj, cos_rot=c, sin_rot=s, latitude=phi)
    ice = dict(concentration=ocean["ice_concentration"], interface_heat=ocean["ice_interface_heat"],
               salt_flux=ocean["ice_salt_flux"], x_stress=ocean["ice_x_stress"], y_stress=ocean["ice_y_stress"])
    ice_state = syn.sea_ice_state(nx, ny, hx, hy, ny_global=ny_global, j_offset=j_offset)
    ice_state["concentration"] = ocean["ice_concentration"]
    return dict(nx=nx, ny=ny, hx=hx, hy=hy, ocean=ocean, src=src, weights=w, ice=ice, ice_state=ice_state)


def polar_atmosphere(at):
    """Turn the interpolated (mostly warm) synthetic atmosphere into a polar one so that the sea-ice
    skin temperature sits below the melting point on most cells: T 252–267 K, q at 80 % of
    saturation, weak shortwave, 200 W/m² longwave."""
    out = {k: np.array(v, dtype=np.float64, copy=True) for k, v in at.items()}
    out["T"] = 253.0 + 0.5 * (at["T"] - 273.15)
    out["q"] = 0.8 * syn._qsat_tetens(out["T"], out["p"]) * (0.9 + 0.1 * at["q"] / np.max(at["q"]))
    out["Qs"] = 0.3 * at["Qs"]
    out["Ql"] = 200.0 + 0.5 * (at["Ql"] - 350.0)
    return out


def window(a, hx, hy, nx, ny, ring):
    return a[hy - ring:hy + ny + ring, hx - ring:hx + nx + ring]


def rel_err(got, ref, scale):
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), scale)))


ICE_FLUX_FIELDS = ("sensible_heat", "latent_heat", "water_vapor", "x_momentum", "y_momentum", "temperature",
                   "friction_velocity", "temperature_scale", "humidity_scale")


def compare_ice_fluxes(got, ref, tol_converged, tol_unconverged=None, maxiter=100, tol_slow=1e-6, slow=40,
                       orbit_shares=((1e-9, 0.97), (1e-6, 0.995), (1e-3, 0.999)), sum_bias_tol=1e-6):
    """Sea-ice interface comparison, same-shape windows.  The recalled skin-temperature balance does not contract for
    thick ice in wind (gain ≈ (h/k)·∂Q/∂T > 1, explicit and semi-implicit form alike): such cells orbit under the ±ΔTmax
    limiter until `maxiter`.  Most of those orbits are attracting cycles both sides land on — measured on the GPU
    (scratch/orbit_cells.py): 98.9–99.6 % of the abandoned cells agree with the oracle to 1e-9, ≥ 99.8 % to 1e-6 — and a
    few per ten thousand amplify rounding without bound (errors up to O(1)).  So the cells the reference leaves at
    `maxiter` ARE compared in value, as a distribution: at least `orbit_shares` of them within each
    tolerance, every one finite, both sides must abandon the same cells, and the abandoned cells' SUMMED sensible and latent
    heat fluxes agree to `sum_bias_tol` of the surface total (a systematic error on thick ice cannot pass as outliers).  A wrong Q_d, albedo or ℒ_s on thick ice
    moves every one of them and fails the first share.  Cells that converge but need more than `slow` iterations (a
    weakly contracting orbit, ≈ 1.3× amplification per iteration) are held to the north star's `tol_slow` = 1e-6, every
    other cell to `tol_converged`; trip counts must be identical on all converged cells."""
    unconv = np.asarray(ref["iterations"]) >= maxiter
    # collapsed turbulence (u★ → 1e-11 on the −5ζ branch): ζ leaves the ψ tables' range |ζ| ≤ 4.3e9, where the
    # device clamps ψ; u★ then differs by ≈4e-11 m/s in absolute terms, all fluxes are < 1e-9 of their scale
    collapsed = np.asarray(ref["friction_velocity"]) < 1e-8
    slowc = ((np.asarray(ref["iterations"]) > slow) | collapsed) & ~unconv
    fast = ~unconv & ~slowc
    strict = ~unconv & ~collapsed
    assert np.array_equal(np.asarray(got["iterations"])[strict], np.asarray(ref["iterations"])[strict])
    # collapsed cells: u★ differs by ≈ 4e-11 in absolute terms (ψ clamp), which can move the 1e-8 drift test by one iteration
    loose = ~unconv & collapsed
    assert np.all(np.abs(np.asarray(got["iterations"])[loose].astype(int) - np.asarray(ref["iterations"])[loose].astype(int)) <= 1)
    worst = {}
    for k in ICE_FLUX_FIELDS:
        g, r = np.asarray(got[k], dtype=np.float64), np.asarray(ref[k], dtype=np.float64)
        err = np.abs(g - r) / np.maximum(np.abs(r), FIELD_SCALE[k])
        worst[k] = (float(err[fast].max(initial=0.0)), float(err[slowc].max(initial=0.0)),
                    float(err[unconv].max(initial=0.0)))
        assert worst[k][0] <= tol_converged, (k, worst[k])
        assert worst[k][1] <= max(tol_slow, tol_converged), (k, worst[k])
        if tol_unconverged is not None:
            assert worst[k][2] <= tol_unconverged, (k, worst[k])
        assert np.all(np.isfinite(g[unconv])), k
    if tol_unconverged is None:   # both sides must have given up on the same cells, and the bulk of them agrees in value
        assert np.array_equal(np.asarray(got["iterations"])[unconv], np.asarray(ref["iterations"])[unconv])
        n = int(unconv.sum())
        if n >= 50:
            e = np.zeros(unconv.shape)
            for k in ICE_FLUX_FIELDS:
                g, r = np.asarray(got[k], dtype=np.float64), np.asarray(ref[k], dtype=np.float64)
                e = np.maximum(e, np.abs(g - r) / np.maximum(np.abs(r), FIELD_SCALE[k]))
            for tol, share in orbit_shares:
                have = float((e[unconv] <= tol).mean())
                assert have >= share, ("abandoned cells within", tol, have, "needed", share, n)
                worst["abandoned<=%g" % tol] = have
            # ... and what the shares could hide: a systematic error on the abandoned cells would show in their SUMS (the
            # rounding-amplifying orbits scatter both ways).  The summed heat fluxes of the abandoned cells must agree to
            # 1e-6 of the summed magnitudes over the whole surface (uniform cell weights: a relative statement), and the
            # count of cells beyond 1e-6 is reported per field
            # (summed over the abandoned cells that agree to 1e-3: the ≤ 0.1 % the last share lets through are the
            # rounding-amplifying orbits — errors up to O(1) in single cells, which on a small surface would swamp any
            # sum; their count and their largest absolute error are reported)
            calm = unconv & (e <= 1e-3)
            for k in ("sensible_heat", "latent_heat"):
                g, r = np.asarray(got[k], dtype=np.float64), np.asarray(ref[k], dtype=np.float64)
                total = float(np.abs(r).sum())
                bias = abs(float((g[calm] - r[calm]).sum()))
                worst["abandoned_sum_bias." + k] = bias / max(total, 1e-300)
                worst["abandoned_outlier_max_abs." + k] = float(np.abs(g - r)[unconv & ~calm].max(initial=0.0))
                assert bias <= sum_bias_tol * total, ("summed difference over the abandoned cells", k, bias, total)
            worst["abandoned_outliers"] = int((unconv & ~calm).sum())
            for k in ICE_FLUX_FIELDS:
                g, r = np.asarray(got[k], dtype=np.float64), np.asarray(ref[k], dtype=np.float64)
                err = np.abs(g - r) / np.maximum(np.abs(r), FIELD_SCALE[k])
                worst["abandoned_beyond_1e-6." + k] = int((err[unconv] > 1e-6).sum())
            print("[sea-ice abandoned cells] n = %d; beyond 1e-6 per field: %s; summed-heat-flux bias / surface total: %s; %d beyond 1e-3, largest |Δ| %s W/m²" % (
                n, {k.split(".")[1]: v for k, v in worst.items() if str(k).startswith("abandoned_beyond")},
                {k.split(".")[1]: "%.1e" % v for k, v in worst.items() if str(k).startswith("abandoned_sum_bias")}, worst["abandoned_outliers"],
                {k.split(".")[1]: "%.2g" % v for k, v in worst.items() if str(k).startswith("abandoned_outlier_max_abs")}))
    return worst


# ---------------------------------------------------------------------------------------------
# Memory the way a caller lays it out: views that start at odd offsets inside larger buffers, and the k = top level slab
# of a 3-D array (tests/test_layout_footprint.py).  Both are contiguous, so the runtime's is_contiguous() checks pass them.
# ---------------------------------------------------------------------------------------------
SENTINEL64 = 0x7FF8DEADBEEF5A5A   # a quiet NaN with a payload: what an untouched f64 output cell must still hold
SENTINEL32 = 0x7EADBEEF           # the same for the int32 `iterations`

_BITS = {"float64": "int64", "float32": "int32", "int32": "int32", "uint8": "uint8"}


def bits_dtype(dtype):
    """The integer dtype that reads the bits of a `dtype` tensor (torch dtypes)."""
    import torch
    return getattr(torch, _BITS[str(dtype).replace("torch.", "")])


def _fill(t, fill):
    """fill a tensor with a value, or (an int for a floating-point tensor) with that bit pattern."""
    if t.dtype.is_floating_point and isinstance(fill, (int, np.integer)) and not isinstance(fill, bool):
        signed = np.array([fill], dtype=np.uint64 if t.element_size() == 8 else np.uint32).view(np.int64 if t.element_size() == 8 else np.int32)
        t.view(bits_dtype(t.dtype)).fill_(int(signed[0]))
    else:
        t.fill_(fill)
    return t


def guarded(shape, dtype, *, offset, guard, fill, device="cuda"):
    """A contiguous device view of `shape` that starts `offset + guard` elements into a fresh buffer: `offset` shifts its
    alignment (1 double = 8 bytes off the allocation's 256-byte alignment, 1–3 bytes for uint8), and at least `guard`
    elements of `fill` lie before and after it (buffer_of(view) gives the whole buffer)."""
    import torch
    n = int(np.prod(shape))
    buf = _fill(torch.empty(offset + guard + n + guard, dtype=dtype, device=device), fill)
    return buf[offset + guard:offset + guard + n].view(shape)


def top_slab(nx, ny, hx, hy, *, nz, hz, dtype, fill, device="cuda"):
    """The k = Nz level of a (Nz + 2Hz, Ny + 2Hy, Nx + 2Hx) array, as models.OceanSimulation hands a 3-D field's surface to
    the library: its first element sits (Hz + Nz − 1) slabs into the allocation, so with an odd slab size and an odd level
    the pointer is 8- but not 16-byte aligned.  Every other level is the guard."""
    import torch
    full = _fill(torch.empty((nz + 2 * hz, ny + 2 * hy, nx + 2 * hx), dtype=dtype, device=device), fill)
    return full[hz + nz - 1]


def buffer_of(view):
    """(flat buffer, first element of `view` in it) of a view made by guarded() or top_slab()."""
    base = view._base if view._base is not None else view
    return base.reshape(-1), view.storage_offset() - base.storage_offset()

