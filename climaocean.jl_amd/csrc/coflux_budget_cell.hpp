// coflux_budget_cell.hpp — the parts of compute_net_ocean_fluxes!'s two sums, per cell (include/coflux.h:
// cf_average_create_budget has the table).  net_cell_local (coflux_kernel_types.hpp) forms them and keeps JT and JS;
// budget_cell forms them again and keeps every part.  Its intermediates — Qu, Qal, Qts, Qss, SQao, SFao, SFs, roc, SFl,
// SFls — are written exactly as net_cell_local writes them, with contraction off, so HEAT_NET, SALT_NET and HEAT_SHORTWAVE
// are bit for bit what the library stores in net T, S and shortwave_surface_flux.
#pragma once
#include "coflux_kernel_types.hpp"

namespace coflux {

// x of every kind, indexed by CF_BUDGET_* (16 wide: a register vector that a term indexes with its uniform kind)
typedef double BudgetParts __attribute__((ext_vector_type(16)));
static_assert(CF_BUDGET_KINDS <= 16, "a kind indexes BudgetParts");

__device__ __forceinline__ BudgetParts budget_cell(const DevParams& P, double alb, double aice, double So, double Ts_kelvin,
                                                   double Mp, double Qs, double Ql, double Qc, double Qv, double Mv,
                                                   double Qio, double Jsio, double Mland, double Qfr) {
#pragma clang fp contract(off)
    const double T2 = Ts_kelvin * Ts_kelvin;
    const double Qu = P.emissivity * P.sigma * T2 * T2;
    const double Qal = -P.emissivity * Ql;
    const double Qts = -(1.0 - alb) * Qs * (1.0 - aice);
    const double Qss = P.penetrating_sw ? 0.0 : Qts;
    const double SQao = (Qu + Qc + Qv + Qal) * (1.0 - aice) + Qss;
    const double SFao = -Mp * P.rho_f_inv + Mv * P.rho_f_inv;
    const double SFs = (So < P.S_min && SFao < 0.0) ? 0.0 : SFao;
    const double roc = P.rho_o_inv * P.c_o_inv;
    const double SFl = -Mland * P.rho_f_inv;                       // land freshwater (rivers, calving): not ice-masked
    const double SFls = (So < P.S_min && SFl < 0.0) ? 0.0 : SFl;
    // the parts: om is net_cell_local's (1.0 − aice); the floor gate is the SUM's, applied to each part's freshwater flux
    const double om = 1.0 - aice;
    const bool floor_gate = So < P.S_min && SFao < 0.0;
    const double Fe = floor_gate ? 0.0 : Mv * P.rho_f_inv;
    const double Fp = floor_gate ? 0.0 : -Mp * P.rho_f_inv;
    BudgetParts X = 0.0;
    X[CF_BUDGET_HEAT_SHORTWAVE] = Qts * roc;
    X[CF_BUDGET_HEAT_LONGWAVE_UP] = (Qu * om) * roc;
    X[CF_BUDGET_HEAT_LONGWAVE_DOWN] = (Qal * om) * roc;
    X[CF_BUDGET_HEAT_SENSIBLE] = (Qc * om) * roc;
    X[CF_BUDGET_HEAT_LATENT] = (Qv * om) * roc;
    X[CF_BUDGET_HEAT_ATMOSPHERE_OCEAN] = SQao * roc;
    X[CF_BUDGET_HEAT_ICE_OCEAN] = Qio * roc;
    X[CF_BUDGET_HEAT_FRAZIL] = Qfr * roc;
    X[CF_BUDGET_HEAT_NET] = SQao * roc + Qio * roc;
    X[CF_BUDGET_SALT_EVAPORATION] = om * (-So * Fe);
    X[CF_BUDGET_SALT_PRECIPITATION] = om * (-So * Fp);
    X[CF_BUDGET_SALT_ATMOSPHERE_OCEAN] = om * (-So * SFs);
    X[CF_BUDGET_SALT_ICE_OCEAN] = Jsio;
    X[CF_BUDGET_SALT_LAND] = -So * SFls;
    X[CF_BUDGET_SALT_NET] = (1.0 - aice) * (-So * SFs) + Jsio + (-So * SFls);
    return X;
}

}  // namespace coflux
