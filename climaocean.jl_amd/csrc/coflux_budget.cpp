// coflux_budget.cpp — cf_average_create_budget (include/coflux.h): checks a table of budget kinds, turns the kinds' "reads"
// column into the load mask of the kernel (a NULL input pointer: not read) and hands back a cf_average whose collections
// go to the kernel of coflux_budget.hip (cf_average::collect, coflux_average.cpp, chooses the launch).  Nothing is allocated
// on the device.
#include "coflux_ctx.hpp"

namespace {

constexpr uint32_t bit(int input) { return 1u << input; }
constexpr uint32_t ALBEDO = 1u << BUDGET_INPUTS;   // the kind reads Qts: the albedo, and the latitude where it depends on it
constexpr uint32_t HEAT_AO = bit(BUDGET_IN_QS) | bit(BUDGET_IN_TS) | bit(BUDGET_IN_QL) | bit(BUDGET_IN_QC) | bit(BUDGET_IN_QV) |
                             bit(BUDGET_IN_ICE) | ALBEDO;
constexpr uint32_t SALT_AO = bit(BUDGET_IN_S) | bit(BUDGET_IN_MV) | bit(BUDGET_IN_MP) | bit(BUDGET_IN_ICE);
constexpr uint32_t SALT_LAND = bit(BUDGET_IN_S) | bit(BUDGET_IN_LAND);
// the "reads" column of the header's table, by kind
constexpr uint32_t READS[CF_BUDGET_KINDS] = {
    bit(BUDGET_IN_QS) | bit(BUDGET_IN_ICE) | ALBEDO,   // HEAT_SHORTWAVE
    bit(BUDGET_IN_TS) | bit(BUDGET_IN_ICE),            // HEAT_LONGWAVE_UP
    bit(BUDGET_IN_QL) | bit(BUDGET_IN_ICE),            // HEAT_LONGWAVE_DOWN
    bit(BUDGET_IN_QC) | bit(BUDGET_IN_ICE),            // HEAT_SENSIBLE
    bit(BUDGET_IN_QV) | bit(BUDGET_IN_ICE),            // HEAT_LATENT
    HEAT_AO,                                           // HEAT_ATMOSPHERE_OCEAN
    bit(BUDGET_IN_QIO),                                // HEAT_ICE_OCEAN
    bit(BUDGET_IN_FRAZIL),                             // HEAT_FRAZIL
    HEAT_AO | bit(BUDGET_IN_QIO),                      // HEAT_NET
    SALT_AO,                                           // SALT_EVAPORATION
    SALT_AO,                                           // SALT_PRECIPITATION
    SALT_AO,                                           // SALT_ATMOSPHERE_OCEAN
    bit(BUDGET_IN_JSIO),                               // SALT_ICE_OCEAN
    SALT_LAND,                                         // SALT_LAND
    SALT_AO | bit(BUDGET_IN_JSIO) | SALT_LAND,         // SALT_NET
};
// ℵ, Qio, Jsio, Mland and the frazil heat are 0.0 without their pointer; every other input a kind reads must be there
constexpr uint32_t OPTIONAL = bit(BUDGET_IN_ICE) | bit(BUDGET_IN_QIO) | bit(BUDGET_IN_JSIO) | bit(BUDGET_IN_LAND) | bit(BUDGET_IN_FRAZIL);
const char* const INPUT_NAME[BUDGET_INPUTS] = {"ocean->S", "fluxes->temperature", "exchange->Mp", "exchange->Qs", "exchange->Ql",
                                               "fluxes->sensible_heat", "fluxes->latent_heat", "fluxes->water_vapor",
                                               "ice->concentration", "ice->interface_heat", "ice->salt_flux", "land_freshwater",
                                               "frazil_heat"};

}  // namespace

extern "C" int cf_average_create_budget(cf_ctx* ctx, const cf_budget_desc* desc, cf_average** out) {
    if (!ctx) return fail(nullptr, CF_ERR_INVALID, "ctx is NULL");
    if (!out || !desc) return fail(ctx, CF_ERR_INVALID, "cf_average_create_budget: NULL argument");
    *out = nullptr;
    if (desc->struct_size != (int32_t)sizeof(cf_budget_desc))
        return fail(ctx, CF_ERR_INVALID, "cf_average_create_budget: struct_size %d (expected %d)", desc->struct_size,
                    (int)sizeof(cf_budget_desc));
    if (desc->max_workgroups < 0 || desc->reserved != 0)
        return fail(ctx, CF_ERR_INVALID, "cf_average_create_budget: max_workgroups %d (≥ 0), reserved %d (0)", desc->max_workgroups,
                    desc->reserved);
    const int n = desc->n_terms;
    if (n < 1 || n > CF_AVERAGE_MAX_FIELDS || !desc->terms)
        return fail(ctx, CF_ERR_INVALID, "cf_average_create_budget: %d terms (1…%d, a host array)", n, CF_AVERAGE_MAX_FIELDS);
    const GridDesc& G = ctx->grid;
    const cf_ocean_surface* o = desc->ocean;
    const cf_exchange_fields* e = desc->exchange;
    const cf_interface_fluxes* f = desc->fluxes;
    const cf_sea_ice_fields* ice = desc->ice;
    const double* given[BUDGET_INPUTS] = {o ? o->S : nullptr,
                                          f ? f->temperature : nullptr,
                                          e ? e->Mp : nullptr,
                                          e ? e->Qs : nullptr,
                                          e ? e->Ql : nullptr,
                                          f ? f->sensible_heat : nullptr,
                                          f ? f->latent_heat : nullptr,
                                          f ? f->water_vapor : nullptr,
                                          ice ? ice->concentration : nullptr,
                                          ice ? ice->interface_heat : nullptr,
                                          ice ? ice->salt_flux : nullptr,
                                          desc->land_freshwater,
                                          desc->frazil_heat};
    BudgetArgs A{};
    A.n_terms = n;
    A.max_blocks = desc->max_workgroups;
    uint32_t reads = 0;
    for (int t = 0; t < n; ++t) {
        const cf_budget_term& T = desc->terms[t];
        if (T.kind < 0 || T.kind >= CF_BUDGET_KINDS || T.reserved != 0)
            return fail(ctx, CF_ERR_INVALID, "cf_average_create_budget: term %d has the unknown kind %d (reserved %d)", t, T.kind, T.reserved);
        if (!T.mean) return fail(ctx, CF_ERR_INVALID, "cf_average_create_budget: term %d (kind %d) has a NULL mean", t, T.kind);
        if (!std::isfinite(T.scale)) return fail(ctx, CF_ERR_INVALID, "cf_average_create_budget: term %d has the scale %g", t, T.scale);
        for (int s = 0; s < BUDGET_INPUTS; ++s)
            if ((READS[T.kind] & ~OPTIONAL & bit(s)) && !given[s])
                return fail(ctx, CF_ERR_INVALID, "cf_average_create_budget: term %d (kind %d) reads %s, which is NULL", t, T.kind, INPUT_NAME[s]);
        reads |= READS[T.kind];
        A.kind[t] = (uint8_t)T.kind;
        A.scale[t] = T.scale;
        A.mean[t] = T.mean;
    }
    for (int s = 0; s < BUDGET_INPUTS; ++s) A.in[s] = (reads & bit(s)) ? given[s] : nullptr;
    A.mask = o ? o->mask : nullptr;
    A.reads_albedo = (reads & ALBEDO) ? 1 : 0;
    if (A.reads_albedo && desc->weights) {
        A.latitude = desc->weights->latitude;
        A.separable = desc->weights->separable;
    }
    if (A.reads_albedo && ctx->dev.albedo_kind == CF_ALBEDO_LATITUDE_DEPENDENT && !A.latitude)
        return fail(ctx, CF_ERR_INVALID, "cf_average_create_budget: the latitude-dependent albedo needs weights->latitude");
    for (int t = 0; t < n; ++t) {
        for (int s = 0; s < BUDGET_INPUTS; ++s)
            if (A.in[s] && fields_overlap(G, A.mean[t], A.in[s]))
                return fail(ctx, CF_ERR_INVALID, "cf_average_create_budget: mean %d overlaps the input %s", t, INPUT_NAME[s]);
        // the mask's own bytes: a uint8 mask is an eighth of a parent array of doubles, and a mean right behind it is legal
        const uintptr_t parent_bytes = (uintptr_t)G.sj * (uintptr_t)(G.ny + 2 * G.hy) * sizeof(double);
        if (A.mask && ranges_overlap(A.mean[t], parent_bytes, A.mask, ctx->dev.mask_kind == CF_MASK_U8 ? parent_bytes / sizeof(double) : parent_bytes))
            return fail(ctx, CF_ERR_INVALID, "cf_average_create_budget: mean %d overlaps the mask", t);
        for (int u = 0; u < t; ++u)
            if (fields_overlap(G, A.mean[t], A.mean[u]))
                return fail(ctx, CF_ERR_INVALID, "cf_average_create_budget: means %d and %d overlap", u, t);
    }
    cf_average* a = new cf_average();
    a->args = A;
    child_adopt(ctx, a);
    *out = a;
    return CF_OK;
}
