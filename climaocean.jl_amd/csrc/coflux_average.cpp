// coflux_average.cpp — time averages of surface fields accumulated on the device (include/coflux.h: cf_average_*,
// cf_attach_average, cf_attach_average_slot; the kernel is coflux_average.hip).  The host keeps each window's total weight and turns a collection
// of weight w into the two coefficients of the running mean; the device does one launch per collection.
#include "coflux_ctx.hpp"

int average_collect(cf_average* a, double weight) {
    cf_ctx* ctx = a->ctx;
    const double total = a->total + weight;
    const bool store = a->samples == 0;
    const double c_prev = store ? 0.0 : a->total / total;
    const double c_new = store ? 1.0 : weight / total;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (a->budget) {
        // the parameters are read at each collection: a latitude-dependent albedo set after the averager was made needs the latitude
        if (a->budget_terms.reads_albedo && ctx->dev.albedo_kind == CF_ALBEDO_LATITUDE_DEPENDENT && !a->budget_terms.latitude)
            return fail(ctx, CF_ERR_INVALID, "cf_average_collect: the latitude-dependent albedo needs the budget averager's weights->latitude");
        HIP_TRY(ctx, launch_budget_average(ctx->stream, ctx->dev, a->budget_terms, ctx->grid, store, c_prev, c_new));
    } else if (a->derived)
        HIP_TRY(ctx, launch_derived_average(ctx->stream, a->terms, ctx->grid, store, c_prev, c_new));
    else
        HIP_TRY(ctx, launch_average(ctx->stream, a->fields, a->nfields, ctx->grid, store, c_prev, c_new));
    a->total = total;
    ++a->samples;
    return CF_OK;
}

extern "C" {

int cf_average_create(cf_ctx* ctx, int nfields, const double* const* d_sources, double* const* d_means, cf_average** out) {
    if (!ctx) return fail(nullptr, CF_ERR_INVALID, "ctx is NULL");
    if (!out || !d_sources || !d_means) return fail(ctx, CF_ERR_INVALID, "cf_average_create: NULL argument");
    *out = nullptr;
    if (nfields < 1 || nfields > CF_AVERAGE_MAX_FIELDS)
        return fail(ctx, CF_ERR_INVALID, "cf_average_create: %d fields (1…%d)", nfields, CF_AVERAGE_MAX_FIELDS);
    const GridDesc& G = ctx->grid;
    auto overlap = [&](const void* p, const void* q) { return fields_overlap(G, p, q); };
    for (int f = 0; f < nfields; ++f)
        if (!d_sources[f] || !d_means[f]) return fail(ctx, CF_ERR_INVALID, "cf_average_create: field %d has a NULL pointer", f);
    for (int f = 0; f < nfields; ++f)
        for (int g = 0; g < nfields; ++g) {
            if (overlap(d_means[f], d_sources[g]))
                return fail(ctx, CF_ERR_INVALID, "cf_average_create: mean %d overlaps source %d", f, g);
            if (g != f && overlap(d_means[f], d_means[g]))
                return fail(ctx, CF_ERR_INVALID, "cf_average_create: means %d and %d overlap", f, g);
        }
    cf_average* a = new cf_average();
    a->nfields = nfields;
    for (int f = 0; f < nfields; ++f) {
        a->fields.src[f] = d_sources[f];
        a->fields.mean[f] = d_means[f];
    }
    child_adopt(ctx, a);
    *out = a;
    return CF_OK;
}

int cf_average_destroy(cf_average* a) {
    if (!a) return CF_OK;
    if (a->ctx)
        for (auto& slot : a->ctx->averages)
            if (slot.handle == a) slot.handle = nullptr;
    child_leave(a);
    delete a;
    return CF_OK;
}

int cf_average_reset(cf_average* a) {
    CHECK(live(a, "cf_average_reset", "averager"));
    a->total = 0.0;
    a->samples = 0;
    return CF_OK;
}

int cf_average_collect(cf_average* a, double weight) {
    CHECK(live(a, "cf_average_collect", "averager"));
    if (!(weight > 0.0) || !std::isfinite(weight) || !std::isfinite(a->total + weight))
        return fail(a->ctx, CF_ERR_INVALID, "cf_average_collect: weight %g (> 0 and finite)", weight);
    return average_collect(a, weight);
}

int cf_average_weight(cf_average* a, double* total, int64_t* samples) {
    CHECK(live(a, "cf_average_weight", "averager"));
    if (total) *total = a->total;
    if (samples) *samples = a->samples;
    return CF_OK;
}

// one slot of ctx->averages; `fn` names the entry point in the error text
static int attach_average_slot(cf_ctx* ctx, const char* fn, int32_t slot, cf_average* a, int32_t stride, double step_weight) {
    if (!a) {
        ctx->averages[slot].handle = nullptr;
        return CF_OK;
    }
    if (a->ctx != ctx) return fail(ctx, CF_ERR_INVALID, "%s: the averager belongs to another context", fn);
    if (stride < 1 || !(step_weight > 0.0) || !std::isfinite(step_weight * stride))
        return fail(ctx, CF_ERR_INVALID, "%s: stride %d (≥ 1), step weight %g (> 0 and finite)", fn, stride, step_weight);
    for (int32_t s = 0; s < CF_ATTACHED_AVERAGES_MAX; ++s)
        if (s != slot && ctx->averages[s].handle == a)
            return fail(ctx, CF_ERR_INVALID, "%s: the averager is already attached to slot %d", fn, s);
    ctx->averages[slot] = cf_ctx::AverageSlot{a, stride, step_weight};
    return CF_OK;
}

int cf_attach_average(cf_ctx* ctx, cf_average* a, int32_t stride, double step_weight) {
    if (!ctx) return fail(nullptr, CF_ERR_INVALID, "ctx is NULL");
    return attach_average_slot(ctx, "cf_attach_average", 0, a, stride, step_weight);
}

int cf_attach_average_slot(cf_ctx* ctx, int32_t slot, cf_average* a, int32_t stride, double step_weight) {
    if (!ctx) return fail(nullptr, CF_ERR_INVALID, "ctx is NULL");
    if (slot < 0 || slot >= CF_ATTACHED_AVERAGES_MAX)
        return fail(ctx, CF_ERR_INVALID, "cf_attach_average_slot: slot %d (0…%d)", slot, CF_ATTACHED_AVERAGES_MAX - 1);
    return attach_average_slot(ctx, "cf_attach_average_slot", slot, a, stride, step_weight);
}

}  // extern "C"
