// coflux_integrals.cpp — area-weighted surface integrals and their time series (include/coflux.h: cf_integrals_*,
// cf_attach_integrals; the kernels are coflux_integrals.hip).  The host numbers the distinct arrays of the entries, owns the
// series' device buffer and the per-tile partial sums, keeps the records' times and counts the records; the device does one
// pass and one combination launch per collection.
#include "coflux_series.hpp"

int cf_integrals::collect(double time) {
    return series_collect(this, time, "cf_integrals_collect", [this](double* record) {
        return launch_integrals(ctx->stream, args, ctx->grid, record, max_blocks);
    });
}

extern "C" {

int cf_integrals_create(cf_ctx* ctx, const cf_integrals_desc* desc, int32_t capacity, cf_integrals** out) {
    CHECK(series_check_create(ctx, desc, capacity, out, CF_INTEGRALS_MAX_ENTRIES, "cf_integrals"));
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
    cf::Layout L;
    L.add((size_t)capacity * (size_t)K.n_entries * sizeof(double));   // the series starts the allocation
    const size_t at_partial = L.add((size_t)integrals_tiles(ctx->grid) * (size_t)integrals_bucket(K.n_entries) * sizeof(double));
    const size_t at_threshold = L.add(sizeof(threshold)), at_entry = L.add(sizeof(entry));
    cf::DeviceBuffer<double> series;
    HIP_TRY(ctx, series.create(L.bytes));
    K.partial = cf::Layout::at<double>(series.get(), at_partial);
    double* d_threshold = cf::Layout::at<double>(series.get(), at_threshold);
    uint32_t* d_entry = cf::Layout::at<uint32_t>(series.get(), at_entry);
    K.threshold = d_threshold;
    K.entry = d_entry;
    HIP_TRY(ctx, hipMemcpy(d_threshold, threshold, sizeof(threshold), hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(d_entry, entry, sizeof(entry), hipMemcpyHostToDevice));
    cf_integrals* q = new cf_integrals();
    q->args = K;
    series_adopt(ctx, q, K.n_entries, desc->max_workgroups, capacity, std::move(series));
    *out = q;
    return CF_OK;
}

int cf_integrals_destroy(cf_integrals* q) { return series_destroy(q); }

int cf_integrals_collect(cf_integrals* q, double time) {
    CHECK(live(q, "cf_integrals_collect", "integrator"));
    return q->collect(time);
}

int cf_integrals_count(cf_integrals* q, int64_t* records) { return series_count(q, records, "cf_integrals_count", "integrator"); }

int cf_integrals_read(cf_integrals* q, int64_t first, int64_t n, double* h_values, double* h_times) {
    return series_read(q, first, n, h_values, h_times, "cf_integrals_read", "integrator");
}

int cf_integrals_reset(cf_integrals* q) {
    CHECK(live(q, "cf_integrals_reset", "integrator"));
    q->count = 0;
    return CF_OK;
}

int cf_attach_integrals(cf_ctx* ctx, cf_integrals* q, int32_t stride, double time_origin, double step_seconds) {
    return series_attach(ctx, cf_ctx::AT_INTEGRALS, q, stride, time_origin, step_seconds, "cf_attach_integrals", "integrator");
}

}  // extern "C"
