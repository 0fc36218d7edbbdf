"""NumPy restatement of the budget averager (include/coflux.h: cf_average_create_budget): every kind, the land select, the
scale and the designed case the tests share — one IEEE operation per NumPy operation in the order the header writes them,
so that the device is held to it bit for bit.  `BudgetModel` keeps each step in a method of its own: tests plant defects by
overriding one.  `exact_parts` evaluates the same definitions in rational arithmetic (fractions.Fraction: no rounding at
all), and `exact_sum` adds computed parts exactly for the closure bounds.

Roundings of the closure bounds, counted from the formulas (shared operands — Qu, Qal, Qts, om, roc, Fe, Fp — are the same
floats on both sides and count as given):
  heat   every part (Q · om) · roc carries 2 roundings of its own (the shortwave Qts · roc: 1), so the exact sum of the
         computed parts is within 2 · u · Σ|parts| of the exact Σ Q om roc; JTao = ((((Qu + Qc) + Qv) + Qal) · om + Qss) · roc
         puts 3 additions, the product with om, the addition of Qss and the product with roc behind a part: 6.  n_T = 2 + 6 = 8.
  salt   evaporation and precipitation om · ((−Sₒ) · F) carry 2 each; SALT_ATMOSPHERE_OCEAN = om · ((−Sₒ) · (Fp + Fe)) carries 3.
         n_S = 2 + 3 = 5.
(first order in u = 2⁻⁵³; the second-order terms are 2⁻⁵³ of the bound.)

Inputs are interior arrays (ny, nx) in a dict: S, temperature (°C, as cf_interface_fluxes has it), Mp, Qs, Ql, Qc, Qv, Mv,
aice, Qio, Jsio, land, frazil, wet (bool) and alb (the albedo per cell); a missing entry is the library's NULL pointer: 0.0."""
from fractions import Fraction
from types import SimpleNamespace

import numpy as np

KIND_NAMES = ("heat_shortwave", "heat_longwave_up", "heat_longwave_down", "heat_sensible", "heat_latent", "heat_atmosphere_ocean",
              "heat_ice_ocean", "heat_frazil", "heat_net", "salt_evaporation", "salt_precipitation", "salt_atmosphere_ocean",
              "salt_ice_ocean", "salt_land", "salt_net")
(HEAT_SHORTWAVE, HEAT_LONGWAVE_UP, HEAT_LONGWAVE_DOWN, HEAT_SENSIBLE, HEAT_LATENT, HEAT_ATMOSPHERE_OCEAN, HEAT_ICE_OCEAN, HEAT_FRAZIL,
 HEAT_NET, SALT_EVAPORATION, SALT_PRECIPITATION, SALT_ATMOSPHERE_OCEAN, SALT_ICE_OCEAN, SALT_LAND, SALT_NET) = range(15)
HEAT_PARTS = (HEAT_SHORTWAVE, HEAT_LONGWAVE_UP, HEAT_LONGWAVE_DOWN, HEAT_SENSIBLE, HEAT_LATENT)
N_T, N_S = 8, 5
U = Fraction(1, 2 ** 53)
# the reference's six, by its names (omip_diagnostics.jl:84-89)
REFERENCE_SIX = dict(JTao=HEAT_ATMOSPHERE_OCEAN, JTio=HEAT_ICE_OCEAN, JTf=HEAT_FRAZIL, JTn=HEAT_NET, JSn=SALT_NET, JSio=SALT_ICE_OCEAN)
# the inputs each kind reads (the header's "reads" column); "alb" stands for the albedo (and the latitude where it depends on it)
_HEAT_AO = {"Qs", "temperature", "Ql", "Qc", "Qv", "aice", "alb"}
_SALT_AO = {"S", "Mv", "Mp", "aice"}
READS = {HEAT_SHORTWAVE: {"Qs", "aice", "alb"}, HEAT_LONGWAVE_UP: {"temperature", "aice"}, HEAT_LONGWAVE_DOWN: {"Ql", "aice"},
         HEAT_SENSIBLE: {"Qc", "aice"}, HEAT_LATENT: {"Qv", "aice"}, HEAT_ATMOSPHERE_OCEAN: _HEAT_AO, HEAT_ICE_OCEAN: {"Qio"},
         HEAT_FRAZIL: {"frazil"}, HEAT_NET: _HEAT_AO | {"Qio"}, SALT_EVAPORATION: _SALT_AO, SALT_PRECIPITATION: _SALT_AO,
         SALT_ATMOSPHERE_OCEAN: _SALT_AO, SALT_ICE_OCEAN: {"Jsio"}, SALT_LAND: {"S", "land"},
         SALT_NET: _SALT_AO | {"Jsio", "S", "land"}}
INPUT_NAMES = ("S", "temperature", "Mp", "Qs", "Ql", "Qc", "Qv", "Mv", "aice", "Qio", "Jsio", "land", "frazil")

ZERO, ONE = np.float64(0.0), np.float64(1.0)


def fma(a, b, c):
    """round(a · b + c), once"""
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def constants(params):
    """what the library derives from cf_flux_params on the host, in double"""
    f = np.float64
    return SimpleNamespace(emissivity=f(params.ocean_emissivity), sigma=f(params.stefan_boltzmann),
                           rho_o_inv=ONE / f(params.ocean_reference_density), c_o_inv=ONE / f(params.ocean_heat_capacity),
                           rho_f_inv=ONE / f(params.ocean_freshwater_density), T_offset=f(params.ocean_temperature_offset),
                           S_min=f(params.ocean_minimum_salinity), albedo=f(params.ocean_albedo),
                           albedo_diffuse=f(params.ocean_albedo_diffuse), albedo_direct=f(params.ocean_albedo_direct),
                           latitude_dependent=int(params.ocean_albedo_kind) == 1, penetrating=bool(params.penetrating_shortwave))


def albedo_of(params, latitude):
    """the albedo per cell: the constant, or a_diffuse − a_direct · cos(2φ · (π / 180)) with the product and the difference
    contracted into one rounding, as the device function shared with the net-flux kernel is compiled"""
    P = constants(params)
    latitude = np.asarray(latitude, dtype=np.float64)
    if not P.latitude_dependent:
        return np.full(latitude.shape, P.albedo)
    c = np.cos(np.float64(2.0) * latitude * (np.float64(np.pi) / np.float64(180.0)))
    return np.array([fma(-P.albedo_direct, x, P.albedo_diffuse) for x in c.ravel()]).reshape(latitude.shape)


class BudgetModel:
    def __init__(self, params):
        self.P = constants(params)

    # -- the intermediates of compute_net_ocean_fluxes!, written as the library writes them ---------------------------------
    def get(self, I, name):
        v = I.get(name)
        shape = np.shape(I["wet"])
        return np.zeros(shape) if v is None else np.asarray(v, dtype=np.float64)

    def om(self, I):
        return ONE - self.get(I, "aice")

    def roc(self):
        return self.P.rho_o_inv * self.P.c_o_inv

    def Qu(self, I):
        T = self.get(I, "temperature") + self.P.T_offset
        T2 = T * T
        return self.P.emissivity * self.P.sigma * T2 * T2

    def Qal(self, I):
        return -self.P.emissivity * self.get(I, "Ql")

    def Qts(self, I):
        return -(ONE - self.get(I, "alb")) * self.get(I, "Qs") * (ONE - self.get(I, "aice"))

    def Qss(self, I):
        return np.zeros_like(self.Qts(I)) if self.P.penetrating else self.Qts(I)

    def SQao(self, I):
        return (self.Qu(I) + self.get(I, "Qc") + self.get(I, "Qv") + self.Qal(I)) * (ONE - self.get(I, "aice")) + self.Qss(I)

    def Fp(self, I):
        return -self.get(I, "Mp") * self.P.rho_f_inv

    def Fe(self, I):
        return self.get(I, "Mv") * self.P.rho_f_inv

    def SFao(self, I):
        return self.Fp(I) + self.Fe(I)

    def floor_gate(self, I):
        return (self.get(I, "S") < self.P.S_min) & (self.SFao(I) < ZERO)

    def part_gate(self, I, F):
        """whether the floor zeroes a part's freshwater flux F: the SUM decides"""
        return self.floor_gate(I)

    def SFs(self, I):
        return np.where(self.floor_gate(I), ZERO, self.SFao(I))

    def SFls(self, I):
        SFl = -self.get(I, "land") * self.P.rho_f_inv
        return np.where((self.get(I, "S") < self.P.S_min) & (SFl < ZERO), ZERO, SFl)

    # -- the kinds --------------------------------------------------------------------------------------------------------
    def masked_heat(self, Q, I):
        return (Q * self.om(I)) * self.roc()

    def heat_shortwave(self, I):
        return self.Qts(I) * self.roc()

    def heat_longwave_up(self, I):
        return self.masked_heat(self.Qu(I), I)

    def heat_longwave_down(self, I):
        return self.masked_heat(self.Qal(I), I)

    def heat_sensible(self, I):
        return self.masked_heat(self.get(I, "Qc"), I)

    def heat_latent(self, I):
        return self.masked_heat(self.get(I, "Qv"), I)

    def heat_atmosphere_ocean(self, I):
        return self.SQao(I) * self.roc()

    def heat_ice_ocean(self, I):
        return self.get(I, "Qio") * self.roc()

    def heat_frazil(self, I):
        return self.get(I, "frazil") * self.roc()

    def heat_net(self, I):
        return self.SQao(I) * self.roc() + self.get(I, "Qio") * self.roc()

    def salt_part(self, F, I):
        return self.om(I) * (-self.get(I, "S") * np.where(self.part_gate(I, F), ZERO, F))

    def salt_evaporation(self, I):
        return self.salt_part(self.Fe(I), I)

    def salt_precipitation(self, I):
        return self.salt_part(self.Fp(I), I)

    def salt_atmosphere_ocean(self, I):
        return self.om(I) * (-self.get(I, "S") * self.SFs(I))

    def salt_ice_ocean(self, I):
        return self.get(I, "Jsio").copy()

    def salt_land(self, I):
        return -self.get(I, "S") * self.SFls(I)

    def salt_net(self, I):
        So = self.get(I, "S")
        return (ONE - self.get(I, "aice")) * (-So * self.SFs(I)) + self.get(I, "Jsio") + (-So * self.SFls(I))

    def value(self, kind, I):
        with np.errstate(all="ignore"):
            return getattr(self, KIND_NAMES[kind])(I)

    def sample(self, kind, I, scale=1.0):
        """the interior array that enters the recurrence: land is a select on x, the scale is always multiplied"""
        x = np.where(I["wet"], self.value(kind, I), ZERO)
        with np.errstate(all="ignore"):
            return x * np.float64(scale)


def only(I, kinds):
    """the inputs the kinds read (the others absent: the library never loads them)"""
    keep = set().union(*(READS[k] for k in kinds)) | {"wet"}
    return {k: v for k, v in I.items() if k in keep}


# ---- exact evaluation -------------------------------------------------------------------------------------------------------
def exact_parts(params, cell):
    """{kind: (x, Σ|leaves|)} of one WET cell in rational arithmetic from the same double inputs and host constants: no
    operation is rounded.  `cell`: name → float (missing: 0)."""
    P = constants(params)
    F = lambda v: Fraction(float(v))  # noqa: E731
    g = lambda n: F(cell.get(n, 0.0) or 0.0)  # noqa: E731
    eps, sigma, rfi, roc = F(P.emissivity), F(P.sigma), F(P.rho_f_inv), F(P.rho_o_inv) * F(P.c_o_inv)
    om, So, T = 1 - g("aice"), g("S"), g("temperature") + F(P.T_offset)
    Qu, Qal, Qts = eps * sigma * T ** 4, -eps * g("Ql"), -(1 - g("alb")) * g("Qs") * om
    heat = {HEAT_SHORTWAVE: Qts * roc, HEAT_LONGWAVE_UP: Qu * om * roc, HEAT_LONGWAVE_DOWN: Qal * om * roc,
            HEAT_SENSIBLE: g("Qc") * om * roc, HEAT_LATENT: g("Qv") * om * roc}
    in_sum = [k for k in HEAT_PARTS if not (k == HEAT_SHORTWAVE and P.penetrating)]
    Fe, Fp = g("Mv") * rfi, -g("Mp") * rfi
    gate = So < F(P.S_min) and Fe + Fp < 0
    Fe, Fp = (0, 0) if gate else (Fe, Fp)
    SFl = -g("land") * rfi
    SFl = 0 if (So < F(P.S_min) and SFl < 0) else SFl
    out = {k: (v, abs(v)) for k, v in heat.items()}
    out[HEAT_ATMOSPHERE_OCEAN] = (sum(heat[k] for k in in_sum), sum(abs(heat[k]) for k in in_sum))
    out[HEAT_ICE_OCEAN] = (g("Qio") * roc, abs(g("Qio") * roc))
    out[HEAT_FRAZIL] = (g("frazil") * roc, abs(g("frazil") * roc))
    out[HEAT_NET] = (out[HEAT_ATMOSPHERE_OCEAN][0] + out[HEAT_ICE_OCEAN][0], out[HEAT_ATMOSPHERE_OCEAN][1] + out[HEAT_ICE_OCEAN][1])
    e, p, land = om * -So * Fe, om * -So * Fp, -So * SFl
    out[SALT_EVAPORATION], out[SALT_PRECIPITATION] = (e, abs(e)), (p, abs(p))
    out[SALT_ATMOSPHERE_OCEAN] = (e + p, abs(e) + abs(p))
    out[SALT_ICE_OCEAN] = (g("Jsio"), abs(g("Jsio")))
    out[SALT_LAND] = (land, abs(land))
    out[SALT_NET] = (e + p + g("Jsio") + land, abs(e) + abs(p) + abs(g("Jsio")) + abs(land))
    return out


def exact_sum(values):
    """Σ of doubles, exactly"""
    return sum((Fraction(float(v)) for v in values), Fraction(0))


# ---- the designed case ------------------------------------------------------------------------------------------------------
# named cells, all in the first wave (row 0, columns 0 … 8) of the 67 × 5 interior
CELLS = dict(land=0, open_water=1, full_ice=2, partial_ice=3, floor_freshening=4, floor_evaporation=5, floor_land=6, frazil=7, dark=8)
S_MIN = 5.0


def designed_case(nx=67, ny=5, seed=0):
    """Interior inputs of the designed case: a seeded random background (partial ice on about half the cells, land on about
    a seventh, land freshwater on a third) with the named cells of CELLS planted in row 0.  Use with
    ocean_minimum_salinity = S_MIN.  The 1 × 1 case is the open-water cell alone."""
    rng = np.random.default_rng([seed, nx, ny])
    sh = (ny, nx)
    I = dict(S=rng.uniform(30.0, 37.0, sh), temperature=rng.uniform(-1.8, 29.0, sh), Mp=rng.uniform(0.0, 2e-4, sh),
             Qs=rng.uniform(0.0, 900.0, sh), Ql=rng.uniform(150.0, 450.0, sh), Qc=rng.uniform(-80.0, 40.0, sh),
             Qv=rng.uniform(-300.0, 20.0, sh), Mv=rng.uniform(-1e-5, 1.2e-4, sh),
             aice=np.where(rng.random(sh) < 0.5, rng.uniform(0.0, 1.0, sh), 0.0), Qio=rng.uniform(-30.0, 30.0, sh),
             Jsio=rng.uniform(-1e-6, 1e-6, sh), land=np.where(rng.random(sh) < 0.33, rng.uniform(0.0, 3e-4, sh), 0.0),
             frazil=np.where(rng.random(sh) < 0.2, rng.uniform(0.0, 50.0, sh), 0.0), wet=rng.random(sh) >= 1.0 / 7.0)
    if nx * ny == 1:
        I["wet"][:] = True
        I["aice"][:] = 0.0
        return I
    assert nx > max(CELLS.values())
    c = CELLS
    I["wet"][0, :len(c)] = True
    I["wet"][0, c["land"]] = False
    for name in ("S", "temperature", "Qs", "Ql", "Qc", "Qv"):       # land holds what nobody should read
        I[name][0, c["land"]] = np.nan
    I["aice"][0, c["open_water"]], I["land"][0, c["open_water"]], I["Qs"][0, c["open_water"]] = 0.0, 0.0, 612.5
    I["aice"][0, c["full_ice"]] = 1.0
    I["aice"][0, c["partial_ice"]], I["land"][0, c["partial_ice"]] = 0.37, 2.5e-4
    # below the floor: precipitation beats evaporation (the sum freshens) / evaporation beats precipitation (it does not)
    for name, Mp, Mv in (("floor_freshening", 1.5e-4, 4e-5), ("floor_evaporation", 2e-5, 9e-5)):
        I["S"][0, c[name]], I["Mp"][0, c[name]], I["Mv"][0, c[name]], I["land"][0, c[name]] = 3.25, Mp, Mv, 0.0
        I["aice"][0, c[name]] = 0.25
    I["S"][0, c["floor_land"]], I["land"][0, c["floor_land"]], I["Mp"][0, c["floor_land"]], I["Mv"][0, c["floor_land"]] = 2.0, 3e-4, 1e-5, 8e-5
    I["temperature"][0, c["frazil"]], I["frazil"][0, c["frazil"]], I["aice"][0, c["frazil"]] = -1.95, 41.25, 0.0
    I["Qs"][0, c["dark"]], I["aice"][0, c["dark"]] = 0.0, 0.0
    return I


def halo_layout(a, hx, hy, fill=np.nan):
    """an interior array in the halo layout (ny + 2hy, nx + 2hx), halos filled with `fill`"""
    a = np.asarray(a)
    out = np.full((a.shape[0] + 2 * hy, a.shape[1] + 2 * hx), fill, dtype=a.dtype)
    out[hy:hy + a.shape[0], hx:hx + a.shape[1]] = a
    return out
