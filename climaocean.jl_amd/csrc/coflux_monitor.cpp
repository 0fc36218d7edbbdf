// coflux_monitor.cpp — surface extrema, non-finite counts and state hashes and their time series (include/coflux.h:
// cf_monitor_*, cf_attach_monitor; the kernels are coflux_monitor.hip).  The host owns the series' device buffer with the
// partials, the entries' device copies and the status behind it, keeps the records' times and counts the records; the device
// does one pass and one combination launch per collection.
#include "coflux_ctx.hpp"

int monitor_collect(cf_monitor* m, double time) {
    cf_ctx* ctx = m->ctx;
    if (m->count >= m->capacity)
        return fail(ctx, CF_ERR_INVALID, "cf_monitor_collect: the series is full (%lld records)", (long long)m->capacity);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_monitor(ctx->stream, m->args, ctx->grid, m->d_series.get() + (size_t)m->count * (size_t)m->args.n_entries, m->count,
                                m->max_blocks));
    m->times[(size_t)m->count] = time;
    ++m->count;
    return CF_OK;
}

int monitor_room(cf_ctx* ctx, int64_t first_step, int nsteps) {
    const cf_monitor* m = ctx->monitor;
    if (!m || nsteps <= 0) return CF_OK;
    const int64_t stride = ctx->monitor_stride;
    const int64_t collections = (first_step + nsteps) / stride - first_step / stride;   // steps s with (s + 1) % stride == 0
    if (m->count + collections > m->capacity)
        return fail(ctx, CF_ERR_INVALID, "cf_time_steps: the attached monitor's series holds %lld of %lld records and this call "
                    "would add %lld", (long long)m->count, (long long)m->capacity, (long long)collections);
    return CF_OK;
}

extern "C" {

int cf_monitor_create(cf_ctx* ctx, const cf_monitor_desc* desc, int32_t capacity, cf_monitor** out) {
    if (!ctx) return fail(nullptr, CF_ERR_INVALID, "ctx is NULL");
    if (!out || !desc) return fail(ctx, CF_ERR_INVALID, "cf_monitor_create: NULL argument");
    *out = nullptr;
    if (desc->struct_size != (int32_t)sizeof(cf_monitor_desc))
        return fail(ctx, CF_ERR_INVALID, "cf_monitor_desc.struct_size = %d, library expects %zu", desc->struct_size, sizeof(cf_monitor_desc));
    if (desc->n_entries < 1 || desc->n_entries > CF_MONITOR_MAX_ENTRIES)
        return fail(ctx, CF_ERR_INVALID, "cf_monitor_create: %d entries (1…%d)", desc->n_entries, CF_MONITOR_MAX_ENTRIES);
    if (capacity < 1) return fail(ctx, CF_ERR_INVALID, "cf_monitor_create: capacity %d (≥ 1)", capacity);
    if (desc->max_workgroups < 0) return fail(ctx, CF_ERR_INVALID, "cf_monitor_create: max_workgroups %d (≥ 0)", desc->max_workgroups);
    MonitorEntry entry[CF_MONITOR_MAX_ENTRIES] = {};
    for (int e = 0; e < desc->n_entries; ++e) {
        const cf_monitor_entry& E = desc->entries[e];
        if (E.kind != CF_MONITOR_VALUE && E.kind != CF_MONITOR_ABS)
            return fail(ctx, CF_ERR_INVALID, "cf_monitor_create: entry %d has the unknown kind %d", e, E.kind);
        if (!E.a) return fail(ctx, CF_ERR_INVALID, "cf_monitor_create: entry %d has a NULL a", e);
        entry[e] = MonitorEntry{E.a, E.kind, 0};
    }
    MonitorArgs K{};
    K.n_entries = desc->n_entries;
    K.mask_kind = desc->mask ? ctx->dev.mask_kind : CF_MASK_NONE;
    K.mask = K.mask_kind == CF_MASK_NONE ? nullptr : desc->mask;
    K.z_surface = ctx->dev.z_surface;
    K.first_cell = desc->first_cell;
    K.slices = monitor_slices(ctx->grid, K.n_entries);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // one allocation: [capacity][n_entries] series | [n_entries][slices] partials | entries | status
    const size_t n_series = (size_t)capacity * (size_t)K.n_entries, n_partial = (size_t)K.n_entries * (size_t)K.slices;
    cf::DeviceBuffer<cf_monitor_value> series;
    HIP_TRY(ctx, series.create(n_series * sizeof(cf_monitor_value) + n_partial * sizeof(MonitorPartial) + sizeof(entry) + sizeof(MonitorStatus)));
    K.partial = reinterpret_cast<MonitorPartial*>(series.get() + n_series);
    MonitorEntry* d_entry = reinterpret_cast<MonitorEntry*>(K.partial + n_partial);
    K.entry = d_entry;
    K.status = reinterpret_cast<MonitorStatus*>(d_entry + CF_MONITOR_MAX_ENTRIES);
    const MonitorStatus clean{};
    HIP_TRY(ctx, hipMemcpy(d_entry, entry, sizeof(entry), hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(K.status, &clean, sizeof(clean), hipMemcpyHostToDevice));
    cf_monitor* m = new cf_monitor();
    m->args = K;
    m->max_blocks = desc->max_workgroups;
    m->capacity = capacity;
    m->times.assign((size_t)capacity, 0.0);
    m->d_series = std::move(series);
    child_adopt(ctx, m);
    *out = m;
    return CF_OK;
}

int cf_monitor_destroy(cf_monitor* m) {
    if (!m) return CF_OK;
    if (m->ctx && m->ctx->monitor == m) m->ctx->monitor = nullptr;
    child_leave(m);
    // hipFree (in the delete; it needs no current device) waits for the buffer's device: a collection still in flight has finished before its buffers go
    (void)hipSetDevice(m->device);
    delete m;
    return CF_OK;
}

int cf_monitor_collect(cf_monitor* m, double time) {
    CHECK(live(m, "cf_monitor_collect", "monitor"));
    return monitor_collect(m, time);
}

int cf_monitor_count(cf_monitor* m, int64_t* records) {
    CHECK(live(m, "cf_monitor_count", "monitor"));
    if (records) *records = m->count;
    return CF_OK;
}

int cf_monitor_read(cf_monitor* m, int64_t first, int64_t n, cf_monitor_value* h_values, double* h_times) {
    CHECK(live(m, "cf_monitor_read", "monitor"));
    cf_ctx* ctx = m->ctx;
    if (first < 0 || n < 0 || first + n > m->count || (n > 0 && !h_values))
        return fail(ctx, CF_ERR_INVALID, "cf_monitor_read: records %lld … %lld of %lld", (long long)first, (long long)(first + n),
                    (long long)m->count);
    if (n == 0) return CF_OK;
    const size_t ne = (size_t)m->args.n_entries;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpyAsync(h_values, m->d_series.get() + (size_t)first * ne, (size_t)n * ne * sizeof(cf_monitor_value),
                                hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (h_times) std::copy(m->times.begin() + first, m->times.begin() + first + n, h_times);
    return CF_OK;
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
    if (!ctx) return fail(nullptr, CF_ERR_INVALID, "ctx is NULL");
    if (!m) {
        ctx->monitor = nullptr;
        return CF_OK;
    }
    if (m->ctx != ctx) return fail(ctx, CF_ERR_INVALID, "cf_attach_monitor: the monitor belongs to another context");
    if (stride < 1 || !std::isfinite(time_origin) || !std::isfinite(step_seconds))
        return fail(ctx, CF_ERR_INVALID, "cf_attach_monitor: stride %d (≥ 1), time origin %g and step %g (finite)", stride, time_origin,
                    step_seconds);
    ctx->monitor = m;
    ctx->monitor_stride = stride;
    ctx->monitor_time_origin = time_origin;
    ctx->monitor_step_seconds = step_seconds;
    return CF_OK;
}

}  // extern "C"
