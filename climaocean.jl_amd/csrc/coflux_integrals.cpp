// coflux_integrals.cpp — area-weighted surface integrals and their time series (include/coflux.h: cf_integrals_*,
// cf_attach_integrals; the kernels are coflux_integrals.hip).  The host numbers the distinct arrays of the entries, owns the
// series' device buffer and the per-tile partial sums, keeps the records' times and counts the records; the device does one
// pass and one combination launch per collection.
#include "coflux_ctx.hpp"

int integrals_collect(cf_integrals* q, double time) {
    cf_ctx* ctx = q->ctx;
    if (q->count >= q->capacity)
        return fail(ctx, CF_ERR_INVALID, "cf_integrals_collect: the series is full (%lld records)", (long long)q->capacity);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_integrals(ctx->stream, q->args, ctx->grid, q->d_series.get() + (size_t)q->count * (size_t)q->args.n_entries,
                                  q->max_blocks));
    q->times[(size_t)q->count] = time;
    ++q->count;
    return CF_OK;
}

int integrals_room(cf_ctx* ctx, int64_t first_step, int nsteps) {
    const cf_integrals* q = ctx->integrals;
    if (!q || nsteps <= 0) return CF_OK;
    const int64_t stride = ctx->integrals_stride;
    const int64_t collections = (first_step + nsteps) / stride - first_step / stride;   // steps s with (s + 1) % stride == 0
    if (q->count + collections > q->capacity)
        return fail(ctx, CF_ERR_INVALID, "cf_time_steps: the attached integrator's series holds %lld of %lld records and this call "
                    "would add %lld", (long long)q->count, (long long)q->capacity, (long long)collections);
    return CF_OK;
}

extern "C" {

int cf_integrals_create(cf_ctx* ctx, const cf_integrals_desc* desc, int32_t capacity, cf_integrals** out) {
    if (!ctx) return fail(nullptr, CF_ERR_INVALID, "ctx is NULL");
    if (!out || !desc) return fail(ctx, CF_ERR_INVALID, "cf_integrals_create: NULL argument");
    *out = nullptr;
    if (desc->struct_size != (int32_t)sizeof(cf_integrals_desc))
        return fail(ctx, CF_ERR_INVALID, "cf_integrals_desc.struct_size = %d, library expects %zu", desc->struct_size,
                    sizeof(cf_integrals_desc));
    if (desc->n_entries < 1 || desc->n_entries > CF_INTEGRALS_MAX_ENTRIES)
        return fail(ctx, CF_ERR_INVALID, "cf_integrals_create: %d entries (1…%d)", desc->n_entries, CF_INTEGRALS_MAX_ENTRIES);
    if (capacity < 1) return fail(ctx, CF_ERR_INVALID, "cf_integrals_create: capacity %d (≥ 1)", capacity);
    if (desc->max_workgroups < 0) return fail(ctx, CF_ERR_INVALID, "cf_integrals_create: max_workgroups %d (≥ 0)", desc->max_workgroups);
    IntegralArgs K{};
    uint32_t entry[CF_INTEGRALS_MAX_ENTRIES] = {};
    double threshold[CF_INTEGRALS_MAX_ENTRIES] = {};
    auto slot = [&](const double* p) {
        for (int f = 0; f < K.n_fields; ++f)
            if (K.field[f] == p) return f;
        if (K.n_fields == CF_INTEGRALS_MAX_FIELDS) return -1;
        K.field[K.n_fields] = p;
        return K.n_fields++;
    };
    for (int e = 0; e < desc->n_entries; ++e) {
        const cf_integral_entry& E = desc->entries[e];
        if (E.kind < CF_INTEGRAND_ONE || E.kind > CF_INTEGRAND_ABOVE)
            return fail(ctx, CF_ERR_INVALID, "cf_integrals_create: entry %d has the unknown kind %d", e, E.kind);
        if (E.region_bit < 0 || E.region_bit > 7)
            return fail(ctx, CF_ERR_INVALID, "cf_integrals_create: entry %d names region bit %d (0…7)", e, E.region_bit);
        if (E.kind != CF_INTEGRAND_ONE && !E.a) return fail(ctx, CF_ERR_INVALID, "cf_integrals_create: entry %d has a NULL a", e);
        if (E.kind == CF_INTEGRAND_PRODUCT && !E.b) return fail(ctx, CF_ERR_INVALID, "cf_integrals_create: entry %d (a product) has a NULL b", e);
        if (E.kind == CF_INTEGRAND_ABOVE && !std::isfinite(E.threshold))
            return fail(ctx, CF_ERR_INVALID, "cf_integrals_create: entry %d has the non-finite threshold %g", e, E.threshold);
        int sa = 0, sb = 0;
        if (E.kind != CF_INTEGRAND_ONE) sa = sb = slot(E.a);
        if (E.kind == CF_INTEGRAND_PRODUCT && sa >= 0) sb = slot(E.b);
        if (sa < 0 || sb < 0)
            return fail(ctx, CF_ERR_INVALID, "cf_integrals_create: more than %d distinct arrays", CF_INTEGRALS_MAX_FIELDS);
        entry[e] = (uint32_t)E.kind | (uint32_t)sa << 8 | (uint32_t)sb << 16 | (uint32_t)1 << (24 + E.region_bit);
        threshold[e] = E.kind == CF_INTEGRAND_ABOVE ? E.threshold : 0.0;
    }
    K.n_entries = desc->n_entries;
    K.area = desc->area;
    K.mask_kind = desc->mask ? ctx->dev.mask_kind : CF_MASK_NONE;
    K.mask = K.mask_kind == CF_MASK_NONE ? nullptr : desc->mask;
    K.z_surface = ctx->dev.z_surface;
    K.region = desc->region;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // one allocation: [capacity][n_entries] series | [tiles][bucket] partial sums | thresholds | entry descriptors
    const size_t n_series = (size_t)capacity * (size_t)K.n_entries;
    const size_t n_partial = (size_t)integrals_tiles(ctx->grid) * (size_t)integrals_bucket(K.n_entries);
    cf::DeviceBuffer<double> series;
    HIP_TRY(ctx, series.create((n_series + n_partial + CF_INTEGRALS_MAX_ENTRIES) * sizeof(double) + sizeof(entry)));
    K.partial = series.get() + n_series;
    double* d_threshold = series.get() + n_series + n_partial;
    K.threshold = d_threshold;
    K.entry = reinterpret_cast<const uint32_t*>(d_threshold + CF_INTEGRALS_MAX_ENTRIES);
    HIP_TRY(ctx, hipMemcpy(d_threshold, threshold, sizeof(threshold), hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(d_threshold + CF_INTEGRALS_MAX_ENTRIES, entry, sizeof(entry), hipMemcpyHostToDevice));
    cf_integrals* q = new cf_integrals();
    q->args = K;
    q->max_blocks = desc->max_workgroups;
    q->capacity = capacity;
    q->times.assign((size_t)capacity, 0.0);
    q->d_series = std::move(series);
    child_adopt(ctx, q);
    *out = q;
    return CF_OK;
}

int cf_integrals_destroy(cf_integrals* q) {
    if (!q) return CF_OK;
    if (q->ctx && q->ctx->integrals == q) q->ctx->integrals = nullptr;
    child_leave(q);
    // hipFree (in the delete; it needs no current device) waits for the buffer's device: a collection still in flight has finished before its buffers go
    (void)hipSetDevice(q->device);
    delete q;
    return CF_OK;
}

int cf_integrals_collect(cf_integrals* q, double time) {
    CHECK(live(q, "cf_integrals_collect", "integrator"));
    return integrals_collect(q, time);
}

int cf_integrals_count(cf_integrals* q, int64_t* records) {
    CHECK(live(q, "cf_integrals_count", "integrator"));
    if (records) *records = q->count;
    return CF_OK;
}

int cf_integrals_read(cf_integrals* q, int64_t first, int64_t n, double* h_values, double* h_times) {
    CHECK(live(q, "cf_integrals_read", "integrator"));
    cf_ctx* ctx = q->ctx;
    if (first < 0 || n < 0 || first + n > q->count || (n > 0 && !h_values))
        return fail(ctx, CF_ERR_INVALID, "cf_integrals_read: records %lld … %lld of %lld", (long long)first, (long long)(first + n),
                    (long long)q->count);
    if (n == 0) return CF_OK;
    const size_t ne = (size_t)q->args.n_entries;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpyAsync(h_values, q->d_series.get() + (size_t)first * ne, (size_t)n * ne * sizeof(double), hipMemcpyDeviceToHost,
                                ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (h_times) std::copy(q->times.begin() + first, q->times.begin() + first + n, h_times);
    return CF_OK;
}

int cf_integrals_reset(cf_integrals* q) {
    CHECK(live(q, "cf_integrals_reset", "integrator"));
    q->count = 0;
    return CF_OK;
}

int cf_attach_integrals(cf_ctx* ctx, cf_integrals* q, int32_t stride, double time_origin, double step_seconds) {
    if (!ctx) return fail(nullptr, CF_ERR_INVALID, "ctx is NULL");
    if (!q) {
        ctx->integrals = nullptr;
        return CF_OK;
    }
    if (q->ctx != ctx) return fail(ctx, CF_ERR_INVALID, "cf_attach_integrals: the integrator belongs to another context");
    if (stride < 1 || !std::isfinite(time_origin) || !std::isfinite(step_seconds))
        return fail(ctx, CF_ERR_INVALID, "cf_attach_integrals: stride %d (≥ 1), time origin %g and step %g (finite)", stride, time_origin,
                    step_seconds);
    ctx->integrals = q;
    ctx->integrals_stride = stride;
    ctx->integrals_time_origin = time_origin;
    ctx->integrals_step_seconds = step_seconds;
    return CF_OK;
}

}  // extern "C"
