// coflux_average.cpp — time averages of surface fields accumulated on the device (include/coflux.h: cf_average_*,
// cf_attach_average, cf_attach_average_slot; the kernel is coflux_average.hip).  The host keeps each window's total weight and turns a collection
// of weight w into the two coefficients of the running mean (RunningWeight, coflux_collect.hpp); the device does one launch per collection.
#include "coflux_ctx.hpp"

int cf_average::collect(double w) {
    const RunningWeight::Blend c = weight.next(w);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (const BudgetArgs* budget = std::get_if<BudgetArgs>(&args)) {
        // the parameters are read at each collection: a latitude-dependent albedo set after the averager was made needs the latitude
        if (budget->reads_albedo && ctx->dev.albedo_kind == CF_ALBEDO_LATITUDE_DEPENDENT && !budget->latitude)
            return fail(ctx, CF_ERR_INVALID, "cf_average_collect: the latitude-dependent albedo needs the budget averager's weights->latitude");
        HIP_TRY(ctx, launch_budget_average(ctx->stream, ctx->dev, *budget, ctx->grid, c.store, c.c_prev, c.c_new));
    } else if (const DerivedArgs* derived = std::get_if<DerivedArgs>(&args)) {
        HIP_TRY(ctx, launch_derived_average(ctx->stream, *derived, ctx->grid, c.store, c.c_prev, c.c_new));
    } else {
        const PlainAverageArgs& plain = std::get<PlainAverageArgs>(args);
        HIP_TRY(ctx, launch_average(ctx->stream, plain.fields, plain.nfields, ctx->grid, c.store, c.c_prev, c.c_new));
    }
    weight.add(w);
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
    PlainAverageArgs A{};
    A.nfields = nfields;
    for (int f = 0; f < nfields; ++f) {
        A.fields.src[f] = d_sources[f];
        A.fields.mean[f] = d_means[f];
    }
    cf_average* a = new cf_average();
    a->args = A;
    child_adopt(ctx, a);
    *out = a;
    return CF_OK;
}

int cf_average_destroy(cf_average* a) {
    if (!a) return CF_OK;
    child_leave(a);
    delete a;
    return CF_OK;
}

int cf_average_reset(cf_average* a) {
    CHECK(live(a, "cf_average_reset", "averager"));
    a->weight.reset();
    return CF_OK;
}

int cf_average_collect(cf_average* a, double weight) {
    CHECK(live(a, "cf_average_collect", "averager"));
    if (!a->weight.accepts(weight)) return fail(a->ctx, CF_ERR_INVALID, "cf_average_collect: weight %g (> 0 and finite)", weight);
    return a->collect(weight);
}

int cf_average_weight(cf_average* a, double* total, int64_t* samples) {
    CHECK(live(a, "cf_average_weight", "averager"));
    if (total) *total = a->weight.total;
    if (samples) *samples = a->weight.samples;
    return CF_OK;
}

// one averager slot of ctx->attached; `fn` names the entry point in the error text
static int attach_average_slot(cf_ctx* ctx, const char* fn, int32_t slot, cf_average* a, int32_t stride, double step_weight) {
    if (!a) {
        ctx->attached[slot] = Attachment{};
        return CF_OK;
    }
    if (a->ctx != ctx) return fail(ctx, CF_ERR_INVALID, "%s: the averager belongs to another context", fn);
    if (stride < 1 || !(step_weight > 0.0) || !std::isfinite(step_weight * stride))
        return fail(ctx, CF_ERR_INVALID, "%s: stride %d (≥ 1), step weight %g (> 0 and finite)", fn, stride, step_weight);
    for (int32_t s = 0; s < CF_ATTACHED_AVERAGES_MAX; ++s)
        if (s != slot && ctx->attached[s].handle == a)
            return fail(ctx, CF_ERR_INVALID, "%s: the averager is already attached to slot %d", fn, s);
    ctx->attached[slot] = Attachment{a, StepSchedule{stride}, step_weight};
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
