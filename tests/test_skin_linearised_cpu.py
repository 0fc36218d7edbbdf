"""CF_SKIN_LINEARISED on the CPU: the constant in every binding, and the scheme itself (tests/skin_linearised_reference.py)
on the committed polar tile, where the explicit scheme leaves ≈ 3/4 of the cells in a period-2 orbit at maxiter."""
import os
import re

import numpy as np
import pytest

import numpy_oracle as npo
import skin_linearised_reference as slr
import test_upstream_pin as tup
from coflux import abi
from coflux import interface_computations as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAXITER = 100
FORMULATIONS = {"corrected": ic.corrected_atmosphere_sea_ice_fluxes, "ncar": ic.ncar_atmosphere_sea_ice_fluxes}


def test_linearised_scheme_is_value_2_in_every_binding():
    header = open(os.path.join(ROOT, "include", "coflux.h")).read()
    assert re.search(r"^#define CF_SKIN_LINEARISED 2\b", header, re.M)
    assert re.search(r"^#define CF_ABI_VERSION 5\b", header, re.M)
    assert abi.SKIN_LINEARISED == 2 and abi.ABI_VERSION == 5
    stub = open(os.path.join(ROOT, "climaocean.jl_amd", "julia", "CoFluxMI355X.jl")).read()
    assert re.search(r"^const CF_SKIN_LINEARISED = Int32\(2\)", stub, re.M)
    assert "CF_SKIN_LINEARISED" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    p = ic.SeaIceInterfaceProperties(skin_temperature_scheme=abi.SKIN_LINEARISED).to_params()
    assert p.skin_temperature_scheme == 2


def _tile(name, scheme):
    nx, ny, h, ring, ocean, atmos, ice = tup._polar_case()
    props = ic.SeaIceInterfaceProperties()
    kw = dict(hx=h, hy=h, ring=ring, thermodynamics=ic.AtmosphereThermodynamicsParameters())
    with np.errstate(all="ignore"):
        if scheme == abi.SKIN_LINEARISED:
            out = slr.interface_fluxes(FORMULATIONS[name](), props, ice, ocean, atmos, scheme=scheme, **kw)
        else:
            out = npo.atmosphere_sea_ice_fluxes(FORMULATIONS[name](), props, ice, ocean, atmos, ocean_properties=ic.OceanProperties(),
                                                **kw)
        resid = slr.balance_residual(out, props, ice, ocean, atmos, **kw)
    inner = (slice(h, h + ny), slice(h, h + nx))
    win = (slice(ring, ring + ny), slice(ring, ring + nx))
    return out["iterations"][inner], out["temperature"][inner], resid[win], props


@pytest.mark.parametrize("name", list(FORMULATIONS))
def test_linearised_scheme_converges_on_the_polar_tile(name):
    its, _, _, _ = _tile(name, abi.SKIN_LINEARISED)
    share = float((its >= MAXITER).mean())
    its_e, _, _, _ = _tile(name, abi.SKIN_EXPLICIT)
    print(f"{name}: linearised {100 * share:.1f} % at maxiter (median {int(np.median(its))} trips), "
          f"explicit {100 * (its_e >= MAXITER).mean():.1f} % (median {int(np.median(its_e))})")
    assert share <= 0.01
    assert (its_e >= MAXITER).mean() > 0.5     # (the finding it answers: the explicit scheme orbits on this tile)


@pytest.mark.parametrize("name", list(FORMULATIONS))
def test_linearised_answer_satisfies_the_surface_energy_balance(name):
    its, T, resid, props = _tile(name, abi.SKIN_LINEARISED)
    ok = (its < MAXITER) & (T + props.temperature_offset < props.freshwater_melting_temperature)
    assert ok.sum() > 0.9 * ok.size
    assert np.max(np.abs(resid[ok])) <= 1e-3, np.max(np.abs(resid[ok]))


@pytest.mark.parametrize("name", list(FORMULATIONS))
def test_linearised_and_explicit_agree_where_the_explicit_scheme_truly_converged(name):
    its, T, resid, props = _tile(name, abi.SKIN_LINEARISED)
    its_e, T_e, resid_e, _ = _tile(name, abi.SKIN_EXPLICIT)
    both = (its < MAXITER) & (its_e < MAXITER) & (np.abs(resid_e) <= 1e-3)
    assert both.sum() >= 20, both.sum()
    assert np.max(np.abs(T[both] - T_e[both])) <= 1e-5
