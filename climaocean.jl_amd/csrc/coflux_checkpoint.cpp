// coflux_checkpoint.cpp — checkpoint and pickup (include/coflux.h: cf_checkpoint_*; the kernel is coflux_checkpoint.hip, the
// image's parser coflux_checkpoint_image.cpp).  A handle keeps the caller's registration — device arrays and the averagers,
// climatologies, integrators and monitors whose private state goes along — and owns a drain stream, two events, the device
// staging image, the pinned host image and the kernel's tables.  A capture lays the image out from the handles' state at the
// call (the plan), copies what the host keeps, issues one launch for every device byte and drains behind an event;
// cf_checkpoint_wait writes the header, the directory and the host-kept bytes into the drained image.  A restore refuses
// before it touches anything, then runs the plan backwards.  What a handle's section holds is the handle's to say (cf_child,
// coflux_ctx.hpp): this file lays out arrays and walks the registration.
#include "coflux_series.hpp"

struct cf_checkpoint : cf_child {
    int flags = 0, max_blocks = 0;
    bool streaming_stores = false;   // the pack launch writes the staging image with streaming (nt) stores
    struct Section {
        std::string name;
        uint32_t kind = cfck::KIND_ARRAY;
        unsigned char* ptr = nullptr;   // an array's bytes …
        size_t bytes = 0;
        cf_child* child = nullptr;      // … or the handle whose private state goes along
    };
    std::vector<Section> sections;
    std::vector<unsigned char> blob;
    // one image laid out: the directory's entries, each section's host-kept bytes (they follow its device bytes) and the runs
    // of device bytes the kernel moves
    struct Plan {
        std::vector<cfck::Entry> entries;
        std::vector<uint64_t> device_bytes;               // per section, from the start of its payload
        std::vector<std::vector<unsigned char>> tail;     // per section: payload bytes [device_bytes, bytes)
        std::vector<CheckpointSegment> segments;
        uint64_t sections_end = 0, blob_offset = 0, total = 0;
    } plan;
    cf::Stream drain;
    cf::Event ev_packed, ev_done, ev_uploaded;
    bool uploaded = false;                       // ev_uploaded has been recorded: the pinned tables and image were read by an H2D copy
    cf::DeviceBuffer<unsigned char> d_image;     // the staging image (not with CF_CHECKPOINT_DIRECT)
    cf::PinnedBuffer<unsigned char> h_image;
    size_t d_image_bytes = 0, h_image_bytes = 0;
    cf::DeviceBuffer<unsigned char> d_tables;    // segments | tile table | hash words
    cf::PinnedBuffer<unsigned char> h_tables;
    size_t tables_bytes = 0;
    cf::PinnedBuffer<unsigned long long> h_hash; // the hash words as the device formed them
    bool capturing = false, restoring = false, have_image = false;
    std::vector<uint64_t> expected;              // after a restore: what the device's hash words must be
};

namespace {

// the parser states the monitor's sizes on its own (it includes no library header): a change to either struct stops the build here
static_assert(sizeof(cf_monitor_value) == cfck::MONITOR_RECORD_BYTES && sizeof(MonitorStatus) == cfck::MONITOR_STATUS_BYTES,
              "coflux_checkpoint_image.hpp states other sizes than the monitor has");
static_assert(CF_CHECKPOINT_MAX_SECTIONS == cfck::MAX_SECTIONS && CF_MONITOR_MAX_ENTRIES <= cfck::MAX_ENTRIES && CF_INTEGRALS_MAX_ENTRIES <= cfck::MAX_ENTRIES &&
              CF_CLIMATOLOGY_MAX_BINS <= cfck::MAX_ENTRIES, "coflux_checkpoint_image.hpp states other limits than include/coflux.h");

// Which stores write the staging image: streaming stores, the form of coflux_solver_shared.hpp::gstore_final — the image is read
// next by the copy engine, not by a kernel.  They measured no worse than plain stores on either surface.
constexpr bool STREAMING_STORES_DEFAULT = true;
constexpr unsigned char SENTINEL = 0xA5;   // fresh staging and pinned buffers are filled with it: a byte nobody wrote shows

int check_name(cf_checkpoint* cp, const char* fn, const char* name) {
    cf_ctx* ctx = cp->ctx;
    if (!name || !name[0]) return fail(ctx, CF_ERR_INVALID, "%s: the name is NULL or empty", fn);
    if (std::strlen(name) >= cfck::NAME_BYTES) return fail(ctx, CF_ERR_INVALID, "%s: the name \"%s\" has more than %zu bytes", fn, name, cfck::NAME_BYTES - 1);
    if (cp->sections.size() >= CF_CHECKPOINT_MAX_SECTIONS) return fail(ctx, CF_ERR_INVALID, "%s: \"%s\" would be section %zu (at most %d)", fn, name, cp->sections.size() + 1, CF_CHECKPOINT_MAX_SECTIONS);
    for (const auto& s : cp->sections)
        if (s.name == name) return fail(ctx, CF_ERR_INVALID, "%s: a section named \"%s\" is registered already", fn, name);
    if (cp->capturing) return fail(ctx, CF_ERR_INVALID, "%s: a capture is in flight (cf_checkpoint_wait first)", fn);
    return CF_OK;
}

int add_handle(cf_checkpoint* cp, const char* fn, const char* name, cf_child* h, uint32_t kind) {
    CHECK(live(cp, fn, "checkpoint"));
    CHECK(check_name(cp, fn, name));
    if (!h || h->ctx != cp->ctx) return fail(cp->ctx, CF_ERR_INVALID, "%s: section \"%s\": the %s is NULL or belongs to another context", fn, name, cfck::kind_name(kind));
    for (const auto& s : cp->sections)
        if (s.child == h) return fail(cp->ctx, CF_ERR_INVALID, "%s: section \"%s\": this %s is registered already as \"%s\"", fn, name, cfck::kind_name(kind), s.name.c_str());
    cf_checkpoint::Section s;
    s.name = name;
    s.kind = h->section_kind();
    s.child = h;
    cp->sections.push_back(std::move(s));
    return CF_OK;
}

// Lays the image out.  `counts`: per section the records of a series (NULL: what the handles hold now).  With `image` the
// host-kept bytes are the image's, else the handles'.
void make_plan(cf_checkpoint* cp, const int64_t* counts, const unsigned char* image) {
    cf_checkpoint::Plan& P = cp->plan;
    const size_t n = cp->sections.size();
    P.entries.assign(n, cfck::Entry{});
    P.device_bytes.assign(n, 0);
    P.tail.assign(n, {});
    P.segments.clear();
    uint64_t cursor = cfck::HEADER_BYTES + cfck::ENTRY_BYTES * n;
    for (size_t k = 0; k < n; ++k) {
        const cf_checkpoint::Section& S = cp->sections[k];
        cfck::Entry& E = P.entries[k];
        std::snprintf(E.name, sizeof E.name, "%s", S.name.c_str());
        E.kind = S.kind;
        E.offset = cursor;
        if (S.child) {
            S.child->plan_section(SectionPlan{(uint32_t)k, cursor, E, P.device_bytes[k], P.tail[k], P.segments}, counts ? &counts[k] : nullptr);
        } else {
            E.bytes = S.bytes;
            P.device_bytes[k] = S.bytes;
            if (S.bytes) P.segments.push_back(CheckpointSegment{S.ptr, cursor, S.bytes, 0, (uint32_t)k, 0});
        }
        if (image) P.tail[k].assign(image + cursor + P.device_bytes[k], image + cursor + E.bytes);
        cursor += cfck::round_up(E.bytes);
    }
    P.sections_end = P.blob_offset = cursor;
    P.total = cursor + cfck::round_up(cp->blob.size());
}

// the hash of section k's host-kept bytes: the words behind the device's
uint64_t tail_hash(const cf_checkpoint::Plan& P, size_t k) {
    return cfck::hash_bytes(P.tail[k].data(), P.tail[k].size(), (P.device_bytes[k] + 7) / 8);
}

// What the image grows to while the registration stands: every series at its capacity, and some room for the caller's blob
// (JSON whose numbers change their length).  The buffers are sized for this, so that a series that fills from capture to
// capture never makes a capture allocate — an allocation or a release waits for the device.
uint64_t image_room(const cf_checkpoint* cp) {
    const cf_checkpoint::Plan& P = cp->plan;
    uint64_t room = P.total + 4096;
    for (size_t k = 0; k < cp->sections.size(); ++k) {
        if (!cp->sections[k].child) continue;
        const uint64_t full = cfck::round_up(cp->sections[k].child->section_room()), now = cfck::round_up(P.entries[k].bytes);
        if (full > now) room += full - now;
    }
    return room;
}

// The buffers of an image of plan.total bytes and the tables of the plan's segments: sized on first use for image_room, regrown
// only when an image outgrows that (another blob, a restore of a larger image).  The host writes the tables here; the caller
// uploads them.
int ensure_buffers(cf_checkpoint* cp, bool staging, uint32_t* n_tiles, CheckpointSegment** d_segments, uint32_t** d_tile_first, unsigned long long** d_hash) {
    cf_ctx* ctx = cp->ctx;
    const cf_checkpoint::Plan& P = cp->plan;
    if (cp->uploaded) HIP_TRY(ctx, hipEventSynchronize(cp->ev_uploaded.get()));   // long complete but right behind a restore
    const size_t room = (size_t)image_room(cp);
    if (cp->h_image_bytes < P.total) {
        HIP_TRY(ctx, cp->h_image.create(room));
        cp->h_image_bytes = room;
        std::memset(cp->h_image.get(), SENTINEL, cp->h_image_bytes);
        cp->have_image = false;
    }
    if (staging && cp->d_image_bytes < P.total) {
        HIP_TRY(ctx, cp->d_image.create(room));
        cp->d_image_bytes = room;
        HIP_TRY(ctx, hipMemsetAsync(cp->d_image.get(), SENTINEL, cp->d_image_bytes, ctx->stream));
    }
    if (!cp->h_hash) HIP_TRY(ctx, cp->h_hash.create(sizeof(unsigned long long) * CF_CHECKPOINT_MAX_SECTIONS));
    *n_tiles = (uint32_t)((P.sections_end + CHECKPOINT_TILE_BYTES - 1) / CHECKPOINT_TILE_BYTES);
    cf::Layout L;
    const size_t at_segments = L.add(sizeof(CheckpointSegment) * std::max<size_t>(P.segments.size(), 1));
    const size_t at_tiles = L.add(sizeof(uint32_t) * (size_t)*n_tiles), at_hash = L.add(sizeof(unsigned long long) * CF_CHECKPOINT_MAX_SECTIONS);
    if (cp->tables_bytes < L.bytes) {   // for the image's room as well: two segments per section at the most, a tile entry per tile of the room
        cf::Layout R;
        R.add(sizeof(CheckpointSegment) * 2 * CF_CHECKPOINT_MAX_SECTIONS);
        R.add(sizeof(uint32_t) * (room / CHECKPOINT_TILE_BYTES + 1));
        R.add(sizeof(unsigned long long) * CF_CHECKPOINT_MAX_SECTIONS);
        const size_t bytes = std::max(R.bytes, L.bytes);
        HIP_TRY(ctx, cp->d_tables.create(bytes));
        HIP_TRY(ctx, cp->h_tables.create(bytes));
        cp->tables_bytes = bytes;
    }
    CheckpointSegment* seg = cf::Layout::at<CheckpointSegment>(cp->h_tables.get(), at_segments);
    std::copy(P.segments.begin(), P.segments.end(), seg);
    uint32_t* first = cf::Layout::at<uint32_t>(cp->h_tables.get(), at_tiles);
    uint32_t s = 0;
    for (uint32_t t = 0; t < *n_tiles; ++t) {   // the first segment that ends behind the tile's start
        const uint64_t lo = (uint64_t)t * CHECKPOINT_TILE_BYTES;
        while (s < P.segments.size() && P.segments[s].image_offset + cfck::round_up(P.segments[s].bytes) <= lo) ++s;
        first[t] = s;
    }
    std::memset(cf::Layout::at<unsigned char>(cp->h_tables.get(), at_hash), 0, sizeof(unsigned long long) * CF_CHECKPOINT_MAX_SECTIONS);
    *d_segments = cf::Layout::at<CheckpointSegment>(cp->d_tables.get(), at_segments);
    *d_tile_first = cf::Layout::at<uint32_t>(cp->d_tables.get(), at_tiles);
    *d_hash = cf::Layout::at<unsigned long long>(cp->d_tables.get(), at_hash);
    // one copy brings the tables and the zeroed hash words: stream ordered in front of the launch
    HIP_TRY(ctx, hipMemcpyAsync(cp->d_tables.get(), cp->h_tables.get(), L.bytes, hipMemcpyHostToDevice, ctx->stream));
    return CF_OK;
}

int mark_uploaded(cf_checkpoint* cp) {
    cf_ctx* ctx = cp->ctx;
    HIP_TRY(ctx, hipEventRecord(cp->ev_uploaded.get(), ctx->stream));
    cp->uploaded = true;
    return CF_OK;
}

// after a restore: the device's hash words against the image's (the stream has reached ev_done)
int settle_restore(cf_checkpoint* cp) {
    cf_ctx* ctx = cp->ctx;
    HIP_TRY(ctx, hipEventSynchronize(cp->ev_done.get()));
    cp->restoring = false;
    for (size_t k = 0; k < cp->expected.size(); ++k)
        if (cp->h_hash.get()[k] != cp->expected[k])
            return fail(ctx, CF_ERR_HIP, "cf_checkpoint_restore: section \"%s\": the bytes written to the device hash to %016llx, the image's to %016llx",
                        cp->sections[k].name.c_str(), (unsigned long long)cp->h_hash.get()[k], (unsigned long long)cp->expected[k]);
    return CF_OK;
}

}  // namespace

int checkpoint_settle_restores(cf_ctx* ctx) {
    for (cf_checkpoint* cp : ctx->checkpoints)
        if (cp->restoring) CHECK(settle_restore(cp));
    return CF_OK;
}

extern "C" {

int cf_checkpoint_create(cf_ctx* ctx, const cf_checkpoint_desc* desc, cf_checkpoint** out) {
    if (!ctx) return fail(nullptr, CF_ERR_INVALID, "ctx is NULL");
    if (!out || !desc) return fail(ctx, CF_ERR_INVALID, "cf_checkpoint_create: NULL argument");
    *out = nullptr;
    if (desc->struct_size != (int32_t)sizeof(cf_checkpoint_desc))
        return fail(ctx, CF_ERR_INVALID, "cf_checkpoint_desc.struct_size = %d, library expects %zu", desc->struct_size, sizeof(cf_checkpoint_desc));
    if (desc->flags & ~CF_CHECKPOINT_DIRECT) return fail(ctx, CF_ERR_INVALID, "cf_checkpoint_create: unknown flags 0x%x", desc->flags);
    if (desc->max_workgroups < 0) return fail(ctx, CF_ERR_INVALID, "cf_checkpoint_create: max_workgroups %d (≥ 0)", desc->max_workgroups);
    if (desc->reserved != 0) return fail(ctx, CF_ERR_INVALID, "cf_checkpoint_create: reserved is not 0");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    cf::Stream drain;
    cf::Event ev_packed, ev_done, ev_uploaded;
    HIP_TRY(ctx, drain.create());
    HIP_TRY(ctx, ev_packed.create(hipEventDisableTiming));
    HIP_TRY(ctx, ev_done.create(hipEventDisableTiming));
    HIP_TRY(ctx, ev_uploaded.create(hipEventDisableTiming));
    cf_checkpoint* cp = new cf_checkpoint();
    cp->flags = desc->flags;
    cp->streaming_stores = STREAMING_STORES_DEFAULT;
    if (experiments_enabled())   // a measurement aid (tools/checkpoint_probe.py), read when the handle is made: same bytes either way
        if (const char* e = std::getenv("COFLUX_CHECKPOINT_STORES")) cp->streaming_stores = std::strcmp(e, "streaming") == 0 ? true : (std::strcmp(e, "plain") == 0 ? false : cp->streaming_stores);
    cp->max_blocks = desc->max_workgroups;
    cp->drain = std::move(drain);
    cp->ev_packed = std::move(ev_packed);
    cp->ev_done = std::move(ev_done);
    cp->ev_uploaded = std::move(ev_uploaded);
    child_adopt(ctx, cp);
    ctx->checkpoints.push_back(cp);
    *out = cp;
    return CF_OK;
}

int cf_checkpoint_destroy(cf_checkpoint* cp) {
    if (!cp) return CF_OK;
    if (cf_ctx* ctx = cp->ctx) ctx->checkpoints.erase(std::remove(ctx->checkpoints.begin(), ctx->checkpoints.end(), cp), ctx->checkpoints.end());
    child_leave(cp);
    (void)hipSetDevice(cp->device);
    if (cp->drain) (void)hipStreamSynchronize(cp->drain.get());   // a drain in flight ends before its buffers go
    if (cp->capturing || cp->restoring || cp->uploaded) (void)hipEventSynchronize(cp->ev_done.get());
    if (cp->uploaded) (void)hipEventSynchronize(cp->ev_uploaded.get());
    delete cp;
    return CF_OK;
}

int cf_checkpoint_add_array(cf_checkpoint* cp, const char* name, void* d_ptr, size_t bytes) {
    const char* fn = "cf_checkpoint_add_array";
    CHECK(live(cp, fn, "checkpoint"));
    CHECK(check_name(cp, fn, name));
    cf_ctx* ctx = cp->ctx;
    if (!d_ptr && bytes) return fail(ctx, CF_ERR_INVALID, "%s: section \"%s\": %zu bytes at NULL", fn, name, bytes);
    if ((uintptr_t)d_ptr & 7u) return fail(ctx, CF_ERR_INVALID, "%s: section \"%s\": the array's base %p is not 8-byte aligned", fn, name, d_ptr);
    if (bytes > ((size_t)1 << 46)) return fail(ctx, CF_ERR_INVALID, "%s: section \"%s\": %zu bytes", fn, name, bytes);
    for (const auto& s : cp->sections)
        if (s.kind == cfck::KIND_ARRAY && s.bytes && bytes && ranges_overlap(d_ptr, bytes, s.ptr, s.bytes))
            return fail(ctx, CF_ERR_INVALID, "%s: section \"%s\" overlaps section \"%s\"", fn, name, s.name.c_str());
    cf_checkpoint::Section s;
    s.name = name;
    s.kind = cfck::KIND_ARRAY;
    s.ptr = static_cast<unsigned char*>(d_ptr);
    s.bytes = bytes;
    cp->sections.push_back(std::move(s));
    return CF_OK;
}

int cf_checkpoint_add_average(cf_checkpoint* cp, const char* name, cf_average* a) {
    return add_handle(cp, "cf_checkpoint_add_average", name, a, cfck::KIND_AVERAGE);
}
int cf_checkpoint_add_climatology(cf_checkpoint* cp, const char* name, cf_climatology* c) {
    return add_handle(cp, "cf_checkpoint_add_climatology", name, c, cfck::KIND_CLIMATOLOGY);
}
int cf_checkpoint_add_integrals(cf_checkpoint* cp, const char* name, cf_integrals* q) {
    return add_handle(cp, "cf_checkpoint_add_integrals", name, q, cfck::KIND_INTEGRALS);
}
int cf_checkpoint_add_monitor(cf_checkpoint* cp, const char* name, cf_monitor* m) {
    return add_handle(cp, "cf_checkpoint_add_monitor", name, m, cfck::KIND_MONITOR);
}

int cf_checkpoint_set_host_blob(cf_checkpoint* cp, const void* h_blob, size_t bytes) {
    CHECK(live(cp, "cf_checkpoint_set_host_blob", "checkpoint"));
    if (bytes && !h_blob) return fail(cp->ctx, CF_ERR_INVALID, "cf_checkpoint_set_host_blob: %zu bytes at NULL", bytes);
    if (bytes > ((size_t)1 << 30)) return fail(cp->ctx, CF_ERR_INVALID, "cf_checkpoint_set_host_blob: %zu bytes (at most 2^30)", bytes);
    if (cp->capturing) return fail(cp->ctx, CF_ERR_INVALID, "cf_checkpoint_set_host_blob: a capture is in flight (cf_checkpoint_wait first)");
    const unsigned char* p = static_cast<const unsigned char*>(h_blob);
    cp->blob.assign(p, p + bytes);
    return CF_OK;
}

int cf_checkpoint_capture(cf_checkpoint* cp) {
    const char* fn = "cf_checkpoint_capture";
    CHECK(live(cp, fn, "checkpoint"));
    cf_ctx* ctx = cp->ctx;
    if (cp->capturing) return fail(ctx, CF_ERR_INVALID, "%s: a capture is in flight (cf_checkpoint_wait first)", fn);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (cp->restoring) CHECK(settle_restore(cp));   // its hash words are about to be reused
    const bool direct = (cp->flags & CF_CHECKPOINT_DIRECT) != 0;
    make_plan(cp, nullptr, nullptr);
    const cf_checkpoint::Plan& P = cp->plan;
    uint32_t n_tiles = 0;
    CheckpointSegment* d_segments = nullptr;
    uint32_t* d_tile_first = nullptr;
    unsigned long long* d_hash = nullptr;
    CHECK(ensure_buffers(cp, !direct, &n_tiles, &d_segments, &d_tile_first, &d_hash));
    CHECK(mark_uploaded(cp));
    cp->have_image = false;
    const uint32_t n_segments = (uint32_t)P.segments.size();
    const size_t dir_end = cfck::HEADER_BYTES + cfck::ENTRY_BYTES * cp->sections.size();
    const size_t hash_bytes = sizeof(unsigned long long) * std::max<size_t>(cp->sections.size(), 1);
    if (direct) {
        HIP_TRY(ctx, launch_checkpoint(ctx->stream, CHECKPOINT_HASH_ONLY, false, d_segments, n_segments, d_tile_first, n_tiles, nullptr, d_hash, cp->max_blocks));
        for (const CheckpointSegment& S : P.segments)
            HIP_TRY(ctx, hipMemcpyAsync(cp->h_image.get() + S.image_offset, S.ptr, (size_t)S.bytes, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(cp->h_hash.get(), d_hash, hash_bytes, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipEventRecord(cp->ev_done.get(), ctx->stream));
    } else {
        HIP_TRY(ctx, launch_checkpoint(ctx->stream, CHECKPOINT_PACK, cp->streaming_stores, d_segments, n_segments, d_tile_first, n_tiles,
                                       cp->d_image.get(), d_hash, cp->max_blocks));
        HIP_TRY(ctx, hipEventRecord(cp->ev_packed.get(), ctx->stream));
        HIP_TRY(ctx, hipStreamWaitEvent(cp->drain.get(), cp->ev_packed.get(), 0));
        if (P.sections_end > dir_end)
            HIP_TRY(ctx, hipMemcpyAsync(cp->h_image.get() + dir_end, cp->d_image.get() + dir_end, (size_t)P.sections_end - dir_end, hipMemcpyDeviceToHost, cp->drain.get()));
        HIP_TRY(ctx, hipMemcpyAsync(cp->h_hash.get(), d_hash, hash_bytes, hipMemcpyDeviceToHost, cp->drain.get()));
        HIP_TRY(ctx, hipEventRecord(cp->ev_done.get(), cp->drain.get()));
    }
    cp->capturing = true;
    return CF_OK;
}

int cf_checkpoint_wait(cf_checkpoint* cp, const void** h_image, size_t* bytes) {
    const char* fn = "cf_checkpoint_wait";
    CHECK(live(cp, fn, "checkpoint"));
    cf_ctx* ctx = cp->ctx;
    if (h_image) *h_image = nullptr;
    if (bytes) *bytes = 0;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (cp->restoring) CHECK(settle_restore(cp));
    if (cp->capturing) {
        HIP_TRY(ctx, hipEventSynchronize(cp->ev_done.get()));
        cp->capturing = false;
        const cf_checkpoint::Plan& P = cp->plan;
        const bool direct = (cp->flags & CF_CHECKPOINT_DIRECT) != 0;
        unsigned char* image = cp->h_image.get();
        const size_t n = cp->sections.size();
        // the host-kept bytes behind each section's device bytes, and the padding the kernel does not own (all of it without staging)
        for (size_t k = 0; k < n; ++k) {
            const cfck::Entry& E = P.entries[k];
            if (!P.tail[k].empty()) std::memcpy(image + E.offset + P.device_bytes[k], P.tail[k].data(), P.tail[k].size());
            if (direct || !P.tail[k].empty()) std::memset(image + E.offset + E.bytes, 0, (size_t)(cfck::round_up(E.bytes) - E.bytes));
        }
        if (direct)
            for (const CheckpointSegment& S : P.segments) std::memset(image + S.image_offset + S.bytes, 0, (size_t)(cfck::round_up(S.bytes) - S.bytes));
        for (size_t k = 0; k < n; ++k) {
            cfck::Entry E = P.entries[k];
            E.hash = (uint64_t)cp->h_hash.get()[k] + tail_hash(P, k);
            cfck::write_entry(image + cfck::HEADER_BYTES + cfck::ENTRY_BYTES * k, E);
        }
        if (!cp->blob.empty()) std::memcpy(image + P.blob_offset, cp->blob.data(), cp->blob.size());
        std::memset(image + P.blob_offset + cp->blob.size(), 0, (size_t)(P.total - P.blob_offset - cp->blob.size()));
        std::memset(image, 0, cfck::HEADER_BYTES);
        cfck::put64(image + cfck::H_MAGIC, cfck::MAGIC);
        cfck::put32(image + cfck::H_VERSION, cfck::VERSION);
        cfck::put32(image + cfck::H_SECTIONS, (uint32_t)n);
        cfck::put64(image + cfck::H_TOTAL, P.total);
        cfck::put32(image + cfck::H_NX, (uint32_t)ctx->grid.nx);
        cfck::put32(image + cfck::H_NY, (uint32_t)ctx->grid.ny);
        cfck::put32(image + cfck::H_HX, (uint32_t)ctx->grid.hx);
        cfck::put32(image + cfck::H_HY, (uint32_t)ctx->grid.hy);
        cfck::put64(image + cfck::H_DIR_HASH, cfck::hash_bytes(image + cfck::HEADER_BYTES, cfck::ENTRY_BYTES * n));
        cfck::put64(image + cfck::H_BLOB_BYTES, cp->blob.size());
        cfck::put64(image + cfck::H_BLOB_OFFSET, P.blob_offset);
        cfck::put64(image + cfck::H_BLOB_HASH, cfck::hash_bytes(cp->blob.data(), cp->blob.size()));
        cfck::put64(image + cfck::H_HASH, cfck::hash_bytes(image, cfck::H_HASH));
        cp->have_image = true;
    }
    if (!cp->have_image) return CF_OK;   // (a wait behind a restore: only its check)
    if (h_image) *h_image = cp->h_image.get();
    if (bytes) *bytes = (size_t)cp->plan.total;
    return CF_OK;
}

int cf_checkpoint_verify(const void* h_image, size_t bytes) {
    char msg[512];
    if (cfck::verify(h_image, bytes, nullptr, msg, sizeof msg) != 0) return fail(nullptr, CF_ERR_INVALID, "cf_checkpoint_verify: %s", msg);
    return CF_OK;
}

int cf_checkpoint_hash(const void* h_bytes, size_t n, uint64_t* out) {
    if (!out || (n && !h_bytes)) return fail(nullptr, CF_ERR_INVALID, "cf_checkpoint_hash: NULL argument");
    *out = cfck::hash_bytes(h_bytes, n);
    return CF_OK;
}

int cf_checkpoint_host_blob(const void* h_image, size_t bytes, const void** h_blob, size_t* blob_bytes) {
    char msg[512];
    cfck::Header H{};
    if (!h_blob || !blob_bytes) return fail(nullptr, CF_ERR_INVALID, "cf_checkpoint_host_blob: NULL argument");
    if (cfck::verify(h_image, bytes, &H, msg, sizeof msg) != 0) return fail(nullptr, CF_ERR_INVALID, "cf_checkpoint_host_blob: %s", msg);
    *h_blob = static_cast<const unsigned char*>(h_image) + H.blob_offset;
    *blob_bytes = (size_t)H.blob_bytes;
    return CF_OK;
}

int cf_checkpoint_restore(cf_checkpoint* cp, const void* h_image, size_t bytes) {
    const char* fn = "cf_checkpoint_restore";
    CHECK(live(cp, fn, "checkpoint"));
    cf_ctx* ctx = cp->ctx;
    if (cp->capturing) return fail(ctx, CF_ERR_INVALID, "%s: a capture is in flight (cf_checkpoint_wait first)", fn);
    char msg[512];
    cfck::Header H{};
    if (cfck::verify(h_image, bytes, &H, msg, sizeof msg) != 0) return fail(ctx, CF_ERR_INVALID, "%s: %s", fn, msg);
    const unsigned char* image = static_cast<const unsigned char*>(h_image);
    const GridDesc& G = ctx->grid;
    if (H.nx != G.nx || H.ny != G.ny || H.hx != G.hx || H.hy != G.hy)
        return fail(ctx, CF_ERR_INVALID, "%s: the image's grid is %d × %d with halos %d, %d; the context's is %d × %d with %d, %d", fn, H.nx, H.ny, H.hx, H.hy,
                    G.nx, G.ny, G.hx, G.hy);
    const size_t n = cp->sections.size();
    if (H.n_sections != n) return fail(ctx, CF_ERR_INVALID, "%s: the image has %u sections, %zu are registered", fn, H.n_sections, n);
    std::vector<int64_t> counts(n, 0);
    for (size_t k = 0; k < n; ++k) {
        const cf_checkpoint::Section& S = cp->sections[k];
        cfck::Entry E;
        cfck::read_entry(image + cfck::HEADER_BYTES + cfck::ENTRY_BYTES * k, &E);
        if (S.name != E.name) return fail(ctx, CF_ERR_INVALID, "%s: section %zu is \"%s\" in the image and \"%s\" in the registration", fn, k, E.name, S.name.c_str());
        if (S.kind != E.kind)
            return fail(ctx, CF_ERR_INVALID, "%s: section \"%s\" is of kind %s in the image and %s in the registration", fn, E.name, cfck::kind_name(E.kind), cfck::kind_name(S.kind));
        counts[k] = E.count;
        if (S.child) CHECK(S.child->check_entry(E, fn));
        else if (E.bytes != S.bytes)
            return fail(ctx, CF_ERR_INVALID, "%s: section \"%s\" has %llu bytes in the image and %zu in the registration", fn, E.name, (unsigned long long)E.bytes, S.bytes);
    }
    // nothing has been written or launched up to here
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (cp->restoring) CHECK(settle_restore(cp));
    const std::vector<unsigned char> keep_blob = std::move(cp->blob);
    cp->blob.assign(image + H.blob_offset, image + H.blob_offset + H.blob_bytes);   // the plan's total is the image's
    make_plan(cp, counts.data(), image);
    cp->blob = keep_blob;
    const cf_checkpoint::Plan& P = cp->plan;
    const bool direct = (cp->flags & CF_CHECKPOINT_DIRECT) != 0;
    uint32_t n_tiles = 0;
    CheckpointSegment* d_segments = nullptr;
    uint32_t* d_tile_first = nullptr;
    unsigned long long* d_hash = nullptr;
    CHECK(ensure_buffers(cp, !direct, &n_tiles, &d_segments, &d_tile_first, &d_hash));
    const uint32_t n_segments = (uint32_t)P.segments.size();
    const size_t dir_end = cfck::HEADER_BYTES + cfck::ENTRY_BYTES * n;
    // the copies read the handle's pinned image, not the caller's memory: the call returns while they are queued
    if (image != cp->h_image.get()) std::memcpy(cp->h_image.get() + dir_end, image + dir_end, (size_t)P.sections_end - dir_end);
    cp->have_image = false;
    if (direct) {
        for (const CheckpointSegment& S : P.segments)
            HIP_TRY(ctx, hipMemcpyAsync(S.ptr, cp->h_image.get() + S.image_offset, (size_t)S.bytes, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, launch_checkpoint(ctx->stream, CHECKPOINT_HASH_ONLY, false, d_segments, n_segments, d_tile_first, n_tiles, nullptr, d_hash, cp->max_blocks));
    } else {
        if (P.sections_end > dir_end)
            HIP_TRY(ctx, hipMemcpyAsync(cp->d_image.get() + dir_end, cp->h_image.get() + dir_end, (size_t)P.sections_end - dir_end, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, launch_checkpoint(ctx->stream, CHECKPOINT_UNPACK, false, d_segments, n_segments, d_tile_first, n_tiles, cp->d_image.get(), d_hash, cp->max_blocks));
    }
    CHECK(mark_uploaded(cp));
    HIP_TRY(ctx, hipMemcpyAsync(cp->h_hash.get(), d_hash, sizeof(unsigned long long) * std::max<size_t>(n, 1), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(cp->ev_done.get(), ctx->stream));
    cp->expected.assign(n, 0);
    for (size_t k = 0; k < n; ++k) {
        cfck::Entry E;
        cfck::read_entry(image + cfck::HEADER_BYTES + cfck::ENTRY_BYTES * k, &E);
        cp->expected[k] = E.hash - tail_hash(P, k);
    }
    cp->restoring = true;
    // the handles' host state, at once
    for (size_t k = 0; k < n; ++k)
        if (cp->sections[k].child) cp->sections[k].child->load_tail(P.tail[k], counts[k]);
    return CF_OK;
}

}  // extern "C"
