// coflux_series.hpp — the series recorder behind the integrators and the monitors (coflux_integrals.cpp, coflux_monitor.cpp;
// cf_time_steps in coflux_steps.cpp collects the attached ones).  A handle owns one device allocation that starts with
// [capacity][n_entries] records, keeps the records' times on the host and counts the records.  What the two families share
// is here and takes the calling function's name and the handle's noun ("integrator" / "monitor") for its messages; the
// entry tables and the launches stay in their own files.
#pragma once
#include "coflux_ctx.hpp"

template <class Record>
struct cf_series : cf_child {
    int n_entries = 0, max_blocks = 0;
    int64_t capacity = 0, count = 0;
    std::vector<double> times;          // of the records, host side
    cf::DeviceBuffer<Record> d_series;  // [capacity][n_entries]; what the family's kernels need besides lies behind it
    Record* record(int64_t r) const { return d_series.get() + (size_t)r * (size_t)n_entries; }
};

struct cf_integrals : cf_series<double> {
    IntegralArgs args{};   // the partial sums, the thresholds and the entries' descriptors lie behind the series
};

struct cf_monitor : cf_series<cf_monitor_value> {
    MonitorArgs args{};    // the partials, the entries' device copies and the status lie behind the series
};

// The head of cf_<family>_create: the argument and descriptor checks every family makes (`family`: "cf_integrals")
template <class Desc, class Handle>
int series_check_create(cf_ctx* ctx, const Desc* desc, int32_t capacity, Handle** out, int max_entries, const char* family) {
    if (!ctx) return fail(nullptr, CF_ERR_INVALID, "ctx is NULL");
    if (!out || !desc) return fail(ctx, CF_ERR_INVALID, "%s_create: NULL argument", family);
    *out = nullptr;
    if (desc->struct_size != (int32_t)sizeof(Desc))
        return fail(ctx, CF_ERR_INVALID, "%s_desc.struct_size = %d, library expects %zu", family, desc->struct_size, sizeof(Desc));
    if (desc->n_entries < 1 || desc->n_entries > max_entries)
        return fail(ctx, CF_ERR_INVALID, "%s_create: %d entries (1…%d)", family, desc->n_entries, max_entries);
    if (capacity < 1) return fail(ctx, CF_ERR_INVALID, "%s_create: capacity %d (≥ 1)", family, capacity);
    if (desc->max_workgroups < 0) return fail(ctx, CF_ERR_INVALID, "%s_create: max_workgroups %d (≥ 0)", family, desc->max_workgroups);
    return CF_OK;
}

// The tail of cf_<family>_create: `s` takes the allocation that starts with its series and joins the context
template <class Record>
void series_adopt(cf_ctx* ctx, cf_series<Record>* s, int n_entries, int max_blocks, int32_t capacity, cf::DeviceBuffer<Record>&& block) {
    s->n_entries = n_entries;
    s->max_blocks = max_blocks;
    s->capacity = capacity;
    s->times.assign((size_t)capacity, 0.0);
    s->d_series = std::move(block);
    child_adopt(ctx, s);
}

// cf_<family>_collect: `launch(record)` is the family's launch into the next record of `s`
template <class Record, class Launch>
int series_collect(cf_series<Record>* s, double time, const char* fn, const char* noun, Launch launch) {
    CHECK(live(s, fn, noun));
    cf_ctx* ctx = s->ctx;
    if (s->count >= s->capacity) return fail(ctx, CF_ERR_INVALID, "%s: the series is full (%lld records)", fn, (long long)s->capacity);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch(s->record(s->count)));
    s->times[(size_t)s->count] = time;
    ++s->count;
    return CF_OK;
}

// CF_ERR_INVALID unless the attached handle's series has room for what cf_time_steps(first_step, nsteps) collects
template <class Handle>
int series_room(cf_ctx* ctx, const SeriesAttachment<Handle>& at, int64_t first_step, int nsteps, const char* noun) {
    if (!at.handle || nsteps <= 0) return CF_OK;
    const int64_t collections = at.collections(first_step, nsteps);
    if (at.handle->count + collections > at.handle->capacity)
        return fail(ctx, CF_ERR_INVALID, "cf_time_steps: the attached %s's series holds %lld of %lld records and this call "
                    "would add %lld", noun, (long long)at.handle->count, (long long)at.handle->capacity, (long long)collections);
    return CF_OK;
}

template <class Record>
int series_count(cf_series<Record>* s, int64_t* records, const char* fn, const char* noun) {
    CHECK(live(s, fn, noun));
    if (records) *records = s->count;
    return CF_OK;
}

template <class Record>
int series_read(cf_series<Record>* s, int64_t first, int64_t n, Record* h_values, double* h_times, const char* fn, const char* noun) {
    CHECK(live(s, fn, noun));
    cf_ctx* ctx = s->ctx;
    if (first < 0 || n < 0 || first + n > s->count || (n > 0 && !h_values))
        return fail(ctx, CF_ERR_INVALID, "%s: records %lld … %lld of %lld", fn, (long long)first, (long long)(first + n), (long long)s->count);
    if (n == 0) return CF_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpyAsync(h_values, s->record(first), (size_t)n * (size_t)s->n_entries * sizeof(Record), hipMemcpyDeviceToHost,
                                ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (h_times) std::copy(s->times.begin() + first, s->times.begin() + first + n, h_times);
    return CF_OK;
}

// `slot`: where a context keeps its attached handle of this family (&cf_ctx::integrals, &cf_ctx::monitor)
template <class Handle>
int series_destroy(Handle* s, SeriesAttachment<Handle> cf_ctx::*slot) {
    if (!s) return CF_OK;
    if (s->ctx && (s->ctx->*slot).handle == s) (s->ctx->*slot).detach();
    child_leave(s);
    // hipFree (in the delete; it needs no current device) waits for the buffer's device: a collection still in flight has finished before its buffers go
    (void)hipSetDevice(s->device);
    delete s;
    return CF_OK;
}

template <class Handle>
int series_attach(cf_ctx* ctx, SeriesAttachment<Handle> cf_ctx::*slot, Handle* s, int32_t stride, double time_origin, double step_seconds,
                  const char* fn, const char* noun) {
    if (!ctx) return fail(nullptr, CF_ERR_INVALID, "ctx is NULL");
    if (!s) {
        (ctx->*slot).detach();
        return CF_OK;
    }
    if (s->ctx != ctx) return fail(ctx, CF_ERR_INVALID, "%s: the %s belongs to another context", fn, noun);
    if (stride < 1 || !std::isfinite(time_origin) || !std::isfinite(step_seconds))
        return fail(ctx, CF_ERR_INVALID, "%s: stride %d (≥ 1), time origin %g and step %g (finite)", fn, stride, time_origin, step_seconds);
    ctx->*slot = SeriesAttachment<Handle>{s, stride, time_origin, step_seconds};
    return CF_OK;
}
