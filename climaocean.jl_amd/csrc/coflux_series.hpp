// coflux_series.hpp — the series recorder behind the integrators and the monitors (coflux_integrals.cpp, coflux_monitor.cpp;
// cf_time_steps in coflux_steps.cpp collects the attached ones).  A handle owns one device allocation that starts with
// [capacity][n_entries] records, keeps the records' times on the host and counts the records.  What the two families share
// is here and takes the calling function's name and the handle's noun ("integrator" / "monitor") for its messages; the
// entry tables and the launches stay in their own files.  A series' checkpoint section (cf_child) is [status] | records on the
// device and, padded to 16 bytes, the records' times on the host; only the monitor has a status.
#pragma once
#include "coflux_ctx.hpp"

template <class Record>
struct cf_series : cf_child {
    int n_entries = 0, max_blocks = 0;
    int64_t capacity = 0, count = 0;
    std::vector<double> times;          // of the records, host side
    cf::DeviceBuffer<Record> d_series;  // [capacity][n_entries]; what the family's kernels need besides lies behind it
    Record* record(int64_t r) const { return d_series.get() + (size_t)r * (size_t)n_entries; }
    virtual int collect(double time) = 0;   // the next record (cf_<family>_collect on a live handle)
    virtual const char* noun() const = 0;
    virtual unsigned char* status() const { return nullptr; }   // cfck::MONITOR_STATUS_BYTES on the device in front of a section's records

    // attached: the series has room for what cf_time_steps(first_step, nsteps) collects; one record per due step
    int admit(const Attachment& at, const char*, int64_t first_step, int nsteps) const override {
        const int64_t collections = nsteps > 0 ? at.when.collections(first_step, nsteps) : 0;
        if (count + collections > capacity)
            return fail(ctx, CF_ERR_INVALID, "cf_time_steps: the attached %s's series holds %lld of %lld records and this call "
                        "would add %lld", noun(), (long long)count, (long long)capacity, (long long)collections);
        return CF_OK;
    }
    int collect_step(const Attachment& at, int64_t step) override { return collect(at.when.stamp(step)); }

    // of `n` records: the payload's bytes on the device and the padding between them and the times
    uint64_t device_bytes(int64_t n) const { return (status() ? cfck::MONITOR_STATUS_BYTES : 0) + (uint64_t)n * (uint64_t)n_entries * sizeof(Record); }
    uint64_t section_room() const override { return cfck::round_up(device_bytes(capacity)) + 8 * (uint64_t)capacity; }
    void plan_section(const SectionPlan& P, const int64_t* image_count) const override {
        const int64_t n = image_count ? *image_count : count;
        const uint64_t head = device_bytes(0), pad = cfck::round_up(device_bytes(n)) - device_bytes(n);
        P.entry.n_entries = (uint32_t)n_entries;
        P.entry.count = n;
        P.device_bytes = device_bytes(n);
        P.entry.bytes = P.device_bytes + pad + 8 * (uint64_t)n;
        if (head) P.segments.push_back(CheckpointSegment{status(), P.offset, head, 0, P.section, 0});
        if (n) P.segments.push_back(CheckpointSegment{reinterpret_cast<unsigned char*>(d_series.get()), P.offset + head, P.device_bytes - head, head / 8, P.section, 0});
        if (image_count) return;
        P.tail.assign((size_t)pad + 8 * (size_t)n, 0);
        for (int64_t r = 0; r < n; ++r) cfck::put_f64(P.tail.data() + pad + 8 * (size_t)r, times[(size_t)r]);
    }
    int check_entry(const cfck::Entry& E, const char* fn) const override {
        const char* kind = cfck::kind_name(section_kind());
        if ((int)E.n_entries != n_entries)
            return fail(ctx, CF_ERR_INVALID, "%s: section \"%s\" has %u entries in the image, the %s has %d", fn, E.name, E.n_entries, kind, n_entries);
        if (E.count > capacity)
            return fail(ctx, CF_ERR_INVALID, "%s: section \"%s\" holds %lld records, the %s's series has room for %lld", fn, E.name, (long long)E.count, kind, (long long)capacity);
        return CF_OK;
    }
    void load_tail(const std::vector<unsigned char>& tail, int64_t n) override {
        const unsigned char* at = tail.data() + (tail.size() - 8 * (size_t)n);
        for (int64_t r = 0; r < n; ++r) times[(size_t)r] = cfck::get_f64(at + 8 * (size_t)r);
        count = n;
    }
};

struct cf_integrals final : cf_series<double> {
    IntegralArgs args{};   // the partial sums, the thresholds and the entries' descriptors lie behind the series
    int collect(double time) override;
    const char* noun() const override { return "integrator"; }
    uint32_t section_kind() const override { return cfck::KIND_INTEGRALS; }
};

struct cf_monitor final : cf_series<cf_monitor_value> {
    MonitorArgs args{};    // the partials, the entries' device copies and the status lie behind the series
    int collect(double time) override;
    const char* noun() const override { return "monitor"; }
    uint32_t section_kind() const override { return cfck::KIND_MONITOR; }
    unsigned char* status() const override { return reinterpret_cast<unsigned char*>(args.status); }
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

// <family>::collect: `launch(record)` is the family's launch into the next record of `s` (alive); `fn`: cf_<family>_collect
template <class Record, class Launch>
int series_collect(cf_series<Record>* s, double time, const char* fn, Launch launch) {
    cf_ctx* ctx = s->ctx;
    if (s->count >= s->capacity) return fail(ctx, CF_ERR_INVALID, "%s: the series is full (%lld records)", fn, (long long)s->capacity);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch(s->record(s->count)));
    s->times[(size_t)s->count] = time;
    ++s->count;
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

template <class Handle>
int series_destroy(Handle* s) {
    if (!s) return CF_OK;
    child_leave(s);
    // hipFree (in the delete; it needs no current device) waits for the buffer's device: a collection still in flight has finished before its buffers go
    (void)hipSetDevice(s->device);
    delete s;
    return CF_OK;
}

// `slot`: where a context keeps its attached handle of this family (cf_ctx::AT_INTEGRALS, cf_ctx::AT_MONITOR)
inline int series_attach(cf_ctx* ctx, int slot, cf_child* s, int32_t stride, double time_origin, double step_seconds, const char* fn,
                         const char* noun) {
    if (!ctx) return fail(nullptr, CF_ERR_INVALID, "ctx is NULL");
    if (!s) {
        ctx->attached[slot] = Attachment{};
        return CF_OK;
    }
    if (s->ctx != ctx) return fail(ctx, CF_ERR_INVALID, "%s: the %s belongs to another context", fn, noun);
    if (stride < 1 || !std::isfinite(time_origin) || !std::isfinite(step_seconds))
        return fail(ctx, CF_ERR_INVALID, "%s: stride %d (≥ 1), time origin %g and step %g (finite)", fn, stride, time_origin, step_seconds);
    ctx->attached[slot] = Attachment{s, StepSchedule{stride, time_origin, step_seconds}};
    return CF_OK;
}
