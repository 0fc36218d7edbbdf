// coflux_window.cpp — the JRA55 snapshot window in HBM (cf_window_*, include/coflux.h):
// device slots, pinned staging mirrors, a copy stream, and the events that order it against the context's
// compute stream in both directions.
#include "coflux_ctx.hpp"

// JRA55 snapshot window (cf_window_*): n_slots snapshots × nine variables in HBM + pinned staging mirrors.
struct cf_window : cf_child {
    int ns_x = 0, ns_y = 0, n_slots = 0;
    size_t plane = 0;                       // floats per (slot, variable)
    cf::DeviceBuffer<float> d_data[CF_JRA55_NVARS];   // device, each [n_slots][ns_y][ns_x]
    cf::PinnedBuffer<float> h_data[CF_JRA55_NVARS];   // pinned host mirror, same layout
    cf::Stream copy_stream;
    cf::Event ev_compute;                   // "everything queued on the compute stream so far"
    std::vector<cf::Event> ev_uploaded;     // per slot: its H2D copies have landed
    std::vector<int64_t> time_index;        // per slot: snapshot it holds, or INT64_MIN
    std::vector<char> in_flight;            // per slot: an upload was started and not yet waited for by the host
    std::vector<char> ordered;              // per slot: `ordered_on` already waits for the slot's latest upload
    hipStream_t ordered_on = nullptr;       // the compute stream those waits were queued on
};

extern "C" {

// ---------------------------------------------------------------------------------------------
// JRA55 snapshot window
// ---------------------------------------------------------------------------------------------
int cf_window_create(cf_ctx* ctx, int32_t ns_x, int32_t ns_y, int32_t n_slots, cf_window** out) {
    if (!ctx || !out) return fail(ctx, CF_ERR_INVALID, "cf_window_create: NULL argument");
    *out = nullptr;
    if (ns_x < 2 || ns_y < 2 || n_slots < 2)
        return fail(ctx, CF_ERR_INVALID, "cf_window_create: source grid %dx%d with %d slots (need >= 2 each)", ns_x, ns_y, n_slots);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    cf_window* w = new cf_window;
    w->ns_x = ns_x;
    w->ns_y = ns_y;
    w->n_slots = n_slots;
    w->plane = (size_t)ns_x * ns_y;
    w->time_index.assign(n_slots, INT64_MIN);
    w->in_flight.assign(n_slots, 0);
    w->ordered.assign(n_slots, 0);
    w->ev_uploaded.resize(n_slots);
    const size_t bytes = w->plane * n_slots * sizeof(float);
    bool ok = w->copy_stream.create() == hipSuccess && w->ev_compute.create(hipEventDisableTiming) == hipSuccess;
    for (int s = 0; ok && s < n_slots; ++s) ok = w->ev_uploaded[s].create(hipEventDisableTiming) == hipSuccess;
    for (int v = 0; ok && v < CF_JRA55_NVARS; ++v)
        ok = w->d_data[v].create(bytes) == hipSuccess && w->h_data[v].create(bytes) == hipSuccess;
    if (!ok) {
        delete w;   // (nothing is queued on what it holds)
        return fail(ctx, CF_ERR_HIP, "cf_window_create: allocating %d slots of %dx%d failed", n_slots, ns_x, ns_y);
    }
    child_adopt(ctx, w);
    *out = w;
    return CF_OK;
}

int cf_window_destroy(cf_window* w) {
    if (!w) return CF_OK;
    child_leave(w);
    (void)hipSetDevice(w->device);
    (void)hipStreamSynchronize(w->copy_stream.get());   // an upload still in flight has landed before its buffers go
    delete w;
    return CF_OK;
}

float* cf_window_host_buffer(cf_window* w, int32_t slot, int32_t variable) {
    if (!w || slot < 0 || slot >= w->n_slots || variable < 0 || variable >= CF_JRA55_NVARS) return nullptr;
    return w->h_data[variable].get() + (size_t)slot * w->plane;
}

int cf_window_wait_slot(cf_window* w, int32_t slot) {
    CHECK(live(w, "cf_window_wait_slot", "window"));
    if (slot < 0 || slot >= w->n_slots) return fail(w->ctx, CF_ERR_INVALID, "slot %d outside [0, %d)", slot, w->n_slots);
    if (w->in_flight[slot]) {
        HIP_TRY(w->ctx, hipSetDevice(w->device));  // a reader thread calls this: its current device may differ
        HIP_TRY(w->ctx, hipEventSynchronize(w->ev_uploaded[slot].get()));
        w->in_flight[slot] = 0;
    }
    return CF_OK;
}

int cf_window_commit(cf_window* w, int32_t slot, int64_t time_index) {
    CHECK(live(w, "cf_window_commit", "window"));
    cf_ctx* ctx = w->ctx;
    if (slot < 0 || slot >= w->n_slots) return fail(ctx, CF_ERR_INVALID, "slot %d outside [0, %d)", slot, w->n_slots);
    HIP_TRY(ctx, hipSetDevice(ctx->device));  // one process may drive several contexts / devices
    // An interpolation requested AHEAD that reads this slot (cf_prefetch_atmosphere_state, cf_time_steps with
    // CF_PIPELINE_CONTINUING) was computed — or would be — from the snapshot this commit replaces: it is void.  The step it
    // was meant for then interpolates again, from the window's current contents.
    // One that left on the auxiliary stream: its writes must not race the redo.
    const AheadLedger::Work voided = ctx->ahead.commit_slot(slot);
    CHECK(cf_ahead_perform(ctx, &voided));
    // the device copy of this slot may only be overwritten once every interpolation already queued has read it
    HIP_TRY(ctx, hipEventRecord(w->ev_compute.get(), ctx->stream));
    HIP_TRY(ctx, hipStreamWaitEvent(w->copy_stream.get(), w->ev_compute.get(), 0));
    const size_t off = (size_t)slot * w->plane, bytes = w->plane * sizeof(float);
    for (int v = 0; v < CF_JRA55_NVARS; ++v)
        HIP_TRY(ctx, hipMemcpyAsync(w->d_data[v].get() + off, w->h_data[v].get() + off, bytes, hipMemcpyHostToDevice, w->copy_stream.get()));
    HIP_TRY(ctx, hipEventRecord(w->ev_uploaded[slot].get(), w->copy_stream.get()));
    w->time_index[slot] = time_index;
    w->in_flight[slot] = 1;
    w->ordered[slot] = 0;
    return CF_OK;
}

int cf_window_upload(cf_window* w, int64_t time_index, const float* const* host_vars) {
    if (!w || !host_vars) return fail(w ? w->ctx : nullptr, CF_ERR_INVALID, "cf_window_upload: NULL argument");
    CHECK(live(w, "cf_window_upload", "window"));
    const int slot = (int)(((time_index % w->n_slots) + w->n_slots) % w->n_slots);
    CHECK(cf_window_wait_slot(w, slot));
    for (int v = 0; v < CF_JRA55_NVARS; ++v) {
        if (!host_vars[v]) return fail(w->ctx, CF_ERR_INVALID, "cf_window_upload: variable %d is NULL", v);
        std::memcpy(w->h_data[v].get() + (size_t)slot * w->plane, host_vars[v], w->plane * sizeof(float));
    }
    return cf_window_commit(w, slot, time_index);
}

int cf_window_find(cf_window* w, int64_t time_index) {
    if (!w) return -1;
    const int slot = (int)(((time_index % w->n_slots) + w->n_slots) % w->n_slots);
    return w->time_index[slot] == time_index ? slot : -1;
}

int cf_window_source(cf_window* w, int64_t n1, int64_t n2, double time_fraction, cf_atmos_source* out) {
    if (!w || !out) return fail(w ? w->ctx : nullptr, CF_ERR_INVALID, "cf_window_source: NULL argument");
    CHECK(live(w, "cf_window_source", "window"));
    cf_ctx* ctx = w->ctx;
    const int s1 = cf_window_find(w, n1), s2 = cf_window_find(w, n2);
    if (s1 < 0 || s2 < 0)
        return fail(ctx, CF_ERR_INVALID, "snapshot %lld is not in the window (time_indices_in_memory = %d)",
                    (long long)(s1 < 0 ? n1 : n2), w->n_slots);
    if (!(time_fraction >= 0.0 && time_fraction <= 1.0))
        return fail(ctx, CF_ERR_INVALID, "time fraction %g outside [0, 1]", time_fraction);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // One wait per upload and stream: stream order carries it to everything queued behind (a wait on an event that has
    // long fired still costs the queue a barrier packet — with two descriptors per step, +24 µs on an 86 µs step, measured)
    if (w->ordered_on != ctx->stream) {
        std::fill(w->ordered.begin(), w->ordered.end(), 0);
        w->ordered_on = ctx->stream;
    }
    for (const int s : {s1, s2})
        if (!w->ordered[s]) {
            HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, w->ev_uploaded[s].get(), 0));
            w->ordered[s] = 1;
        }
    for (int v = 0; v < CF_JRA55_NVARS; ++v) out->data[v] = w->d_data[v].get();
    out->ns_x = w->ns_x;
    out->ns_y = w->ns_y;
    out->n_levels = w->n_slots;
    out->level1 = s1;
    out->level2 = s2;
    out->time_fraction = time_fraction;
    return CF_OK;
}

}  // extern "C"
