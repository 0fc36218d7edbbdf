// coflux_monitor.cpp — surface extrema, non-finite counts and state hashes and their time series (include/coflux.h:
// cf_monitor_*, cf_attach_monitor; the kernels are coflux_monitor.hip).  The host owns the series' device buffer with the
// partials, the entries' device copies and the status behind it, keeps the records' times and counts the records; the device
// does one pass and one combination launch per collection.
#include "coflux_series.hpp"

int cf_monitor::collect(double time) {
    return series_collect(this, time, "cf_monitor_collect", [this](cf_monitor_value* record) {
        return launch_monitor(ctx->stream, args, ctx->grid, record, count, max_blocks);
    });
}

extern "C" {

int cf_monitor_create(cf_ctx* ctx, const cf_monitor_desc* desc, int32_t capacity, cf_monitor** out) {
    CHECK(series_check_create(ctx, desc, capacity, out, CF_MONITOR_MAX_ENTRIES, "cf_monitor"));
    MonitorEntry entry[CF_MONITOR_MAX_ENTRIES] = {};
    for (int e = 0; e < desc->n_entries; ++e) {
        const cf_monitor_entry& E = desc->entries[e];
        if (E.kind != CF_MONITOR_VALUE && E.kind != CF_MONITOR_ABS)
            return fail(ctx, CF_ERR_INVALID, "cf_monitor_create: entry %d has the unknown kind %d", e, E.kind);
        if (!E.a) return fail(ctx, CF_ERR_INVALID, "cf_monitor_create: entry %d has a NULL a", e);
        entry[e] = MonitorEntry{E.a, E.kind, 0};
    }
    if (desc->row_length < 0 || (desc->row_length > 0 && desc->row_length < ctx->grid.nx))
        return fail(ctx, CF_ERR_INVALID, "cf_monitor_create: row_length %d (0: nx, or ≥ nx = %d)", desc->row_length, ctx->grid.nx);
    MonitorArgs K{};
    K.n_entries = desc->n_entries;
    K.mask_kind = desc->mask ? ctx->dev.mask_kind : CF_MASK_NONE;
    K.mask = K.mask_kind == CF_MASK_NONE ? nullptr : desc->mask;
    K.z_surface = ctx->dev.z_surface;
    K.first_cell = desc->first_cell;
    K.row_length = desc->row_length > 0 ? desc->row_length : ctx->grid.nx;
    K.slices = monitor_slices(ctx->grid, K.n_entries);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // one allocation: [capacity][n_entries] series | [n_entries][slices] partials | entries | status
    cf::Layout L;
    L.add((size_t)capacity * (size_t)K.n_entries * sizeof(cf_monitor_value));   // the series starts the allocation
    const size_t at_partial = L.add((size_t)K.n_entries * (size_t)K.slices * sizeof(MonitorPartial));
    const size_t at_entry = L.add(sizeof(entry)), at_status = L.add(sizeof(MonitorStatus));
    // (records and partials are 64 bytes, an entry 16: every piece is whole 16-byte units, so each lies where it lay without Layout)
    static_assert(sizeof(cf_monitor_value) % 16 == 0 && sizeof(MonitorPartial) % 16 == 0 && sizeof(entry) % 16 == 0, "a piece would move");
    cf::DeviceBuffer<cf_monitor_value> series;
    HIP_TRY(ctx, series.create(L.bytes));
    K.partial = cf::Layout::at<MonitorPartial>(series.get(), at_partial);
    MonitorEntry* d_entry = cf::Layout::at<MonitorEntry>(series.get(), at_entry);
    K.entry = d_entry;
    K.status = cf::Layout::at<MonitorStatus>(series.get(), at_status);
    const MonitorStatus clean{};
    HIP_TRY(ctx, hipMemcpy(d_entry, entry, sizeof(entry), hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(K.status, &clean, sizeof(clean), hipMemcpyHostToDevice));
    cf_monitor* m = new cf_monitor();
    m->args = K;
    series_adopt(ctx, m, K.n_entries, desc->max_workgroups, capacity, std::move(series));
    *out = m;
    return CF_OK;
}

int cf_monitor_destroy(cf_monitor* m) { return series_destroy(m); }

int cf_monitor_collect(cf_monitor* m, double time) {
    CHECK(live(m, "cf_monitor_collect", "monitor"));
    return m->collect(time);
}

int cf_monitor_count(cf_monitor* m, int64_t* records) { return series_count(m, records, "cf_monitor_count", "monitor"); }

int cf_monitor_read(cf_monitor* m, int64_t first, int64_t n, cf_monitor_value* h_values, double* h_times) {
    return series_read(m, first, n, h_values, h_times, "cf_monitor_read", "monitor");
}

int cf_monitor_status(cf_monitor* m, int64_t* first_bad_record, uint32_t* bad_entries) {
    CHECK(live(m, "cf_monitor_status", "monitor"));
    cf_ctx* ctx = m->ctx;
    MonitorStatus s{};
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpyAsync(&s, m->args.status, sizeof(s), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (first_bad_record) *first_bad_record = s.first_bad_plus_one - 1;
    if (bad_entries) *bad_entries = s.first_bad_plus_one > 0 ? s.bad_entries : 0u;
    return CF_OK;
}

int cf_monitor_reset(cf_monitor* m) {
    CHECK(live(m, "cf_monitor_reset", "monitor"));
    cf_ctx* ctx = m->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemsetAsync(m->args.status, 0, sizeof(MonitorStatus), ctx->stream));   // behind every collection already queued
    m->count = 0;
    return CF_OK;
}

int cf_attach_monitor(cf_ctx* ctx, cf_monitor* m, int32_t stride, double time_origin, double step_seconds) {
    return series_attach(ctx, cf_ctx::AT_MONITOR, m, stride, time_origin, step_seconds, "cf_attach_monitor", "monitor");
}

}  // extern "C"
