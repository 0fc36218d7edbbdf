// coflux_steps.cpp — what surrounds update_state! in a multi-step, multi-GPU run (include/coflux.h):
//   * cf_prefetch_atmosphere_state: the next step's interpolation on an auxiliary stream,
//   * cf_peer_halo_*: latitude-slab halo rows through HIP-IPC-mapped mailboxes (coflux_halo.hip),
//   * cf_peer_reduce_*: the reduction world of the exact sums, every rank's mailbox mapped by every other (coflux_exact_sum.hip),
//   * cf_fold_north_halo: the tripolar fold on the last slab,
//   * cf_time_steps: run!(simulation) of a prescribed-ocean coupled model without returning to the host language.
#include <map>
#include <optional>

#include "coflux_series.hpp"

// Mailboxes exported by contexts of THIS process: a handle that comes back to the process that made it cannot be
// opened through HIP IPC (and need not be): the pointer is used as is.  Several slabs per process happen in tests
// and in single-process multi-GPU drivers.
static std::mutex g_peer_mutex;
static std::map<std::string, std::pair<char*, int>> g_peer_local;  // handle bytes → (mailbox, device)

// What a mailbox was exported for, carried by the mailbox itself: in the spare bytes of its first flag line (a flag line uses
// 8 of its 64 bytes, and the kernels touch only those 8), written once at export and read back with a device-to-host copy by
// cf_peer_halo_connect — of an IPC-mapped mailbox and of one of the same process alike.  A rank addresses its NEIGHBOUR's
// mailbox with its OWN slot size max_fields · max_rows · sj, so the two must have been exported for one shape on one width.
struct PeerShapeNote {
    unsigned long long magic;
    int max_fields, max_rows, sj, pad;
};
constexpr unsigned long long PEER_SHAPE_MAGIC = 0x636f666c75786d62ull;  // "cofluxmb"
constexpr size_t PEER_SHAPE_OFFSET = 16;                                // inside flag line 0, clear of its 8-byte flag
static_assert(PEER_SHAPE_OFFSET >= 8 && PEER_SHAPE_OFFSET + sizeof(PeerShapeNote) <= 64, "the note stays inside the first flag line");

static int ensure_aux_stream(cf_ctx* ctx) {
    if (ctx->aux.stream) return CF_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    cf_ctx::AuxLane lane;
    HIP_TRY(ctx, lane.stream.create());
    HIP_TRY(ctx, lane.ev_gate.create(hipEventDisableTiming));
    for (cf::Event& e : lane.done) HIP_TRY(ctx, e.create(hipEventDisableTiming));
    ctx->aux = std::move(lane);
    return CF_OK;
}

// Queues what a transition of the ledger answered with, in Work's order.  A request that leaves on the auxiliary stream is
// gated on the lane's gate event (recorded on the main stream at the point after which its set is free to be overwritten).
int cf_ahead_perform(cf_ctx* ctx, const AheadLedger::Work* work) {
    if (const int k = work->launch_aux; k >= 0) {
        const AheadLedger::Record& r = work->launched;
        if (work->gate_late) HIP_TRY(ctx, hipEventRecord(ctx->aux.ev_gate.get(), ctx->stream));
        HIP_TRY(ctx, hipStreamWaitEvent(ctx->aux.stream.get(), ctx->aux.ev_gate.get(), 0));
        // the LDS-free gather kernel (≤ 56 VGPRs, no LDS): it is resident BESIDE the solver's workgroups, which fill
        // the CU's LDS and 456 of 512 registers per SIMD; the tiled kernel would wait for them to retire
        HIP_TRY(ctx, launch_interpolate_background(ctx->aux.stream.get(), ctx->grid, &r.src, &r.w, &r.out));
        HIP_TRY(ctx, hipEventRecord(ctx->aux.done[k].get(), ctx->aux.stream.get()));
    }
    for (int k = 0; k < 2; ++k)
        if (work->wait_done >> k & 1) HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->aux.done[k].get(), 0));
    if (work->gate_now) HIP_TRY(ctx, hipEventRecord(ctx->aux.ev_gate.get(), ctx->stream));
    return CF_OK;
}

// Books a request and queues what that implies; *rec: its record.  defer: it waits for the next solver launch
static int book_request(cf_ctx* ctx, const cf_atmos_source* src, const cf_interp_weights* w, const cf_exchange_fields* out, bool defer,
                        const AheadLedger::Record** rec = nullptr) {
    const AheadLedger::Booked B = ctx->ahead.request(*src, *w, *out, ctx->merged_prefetch, defer);
    CHECK(cf_ahead_perform(ctx, &B.work));
    if (!B.rec) return fail(ctx, CF_ERR_INVALID, "two prefetched atmosphere states are already pending");
    if (rec) *rec = B.rec;
    return CF_OK;
}

// cf_prefetch_atmosphere_state (defer) and a request that leaves on the auxiliary stream at once
static int request_prefetch(cf_ctx* ctx, const cf_atmos_source* src, const cf_interp_weights* w,
                            const cf_exchange_fields* out, bool defer) {
    if (!ctx) return fail(nullptr, CF_ERR_INVALID, "ctx is NULL");
    if (!src || !w || !w->fi || !w->fj || !out || !out->u || !out->v || !out->T || !out->p || !out->q || !out->Qs ||
        !out->Ql || !out->Mp)
        return fail(ctx, CF_ERR_INVALID, "cf_prefetch_atmosphere_state: NULL argument");
    for (int v = 0; v < CF_JRA55_NVARS; ++v)
        if (!src->data[v]) return fail(ctx, CF_ERR_INVALID, "atmosphere source variable %d is NULL", v);
    if (src->level1 < 0 || src->level1 >= src->n_levels || src->level2 < 0 || src->level2 >= src->n_levels)
        return fail(ctx, CF_ERR_INVALID, "time levels (%d,%d) outside the %d levels in memory", src->level1, src->level2,
                    src->n_levels);
    CHECK(ensure_aux_stream(ctx));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    CHECK(book_request(ctx, src, w, out, defer));
    if (defer) return CF_OK;
    const AheadLedger::Work now = ctx->ahead.leave_aux();
    return cf_ahead_perform(ctx, &now);
}

extern "C" {

int cf_prefetch_atmosphere_state(cf_ctx* ctx, const cf_atmos_source* src, const cf_interp_weights* w,
                                 const cf_exchange_fields* out) {
    return request_prefetch(ctx, src, w, out, true);
}

}  // extern "C"

// cf_destroy: the mailbox of a context that goes away must not be handed to a later cf_peer_halo_connect of this process
void cf_peer_forget_local(const char* mailbox) {
    std::lock_guard<std::mutex> lock(g_peer_mutex);
    for (auto it = g_peer_local.begin(); it != g_peer_local.end();)
        it = it->second.first == mailbox ? g_peer_local.erase(it) : std::next(it);
}

// cf_peer_tile_export (coflux_tiles.cpp): a mailbox of this process, found again by cf_peer_map_mailbox
void cf_peer_remember_local(const void* handle, char* mailbox, int device) {
    std::lock_guard<std::mutex> lock(g_peer_mutex);
    g_peer_local[std::string((const char*)handle, CF_PEER_HANDLE_BYTES)] = {mailbox, device};
}

extern "C" {

// ---- peer-direct halo rows --------------------------------------------------------------------
int cf_peer_halo_export(cf_ctx* ctx, int max_fields, int max_rows, void* handle_out) {
    if (!ctx || !handle_out) return fail(ctx, CF_ERR_INVALID, "cf_peer_halo_export: NULL argument");
    if (max_fields < 1 || max_fields > PEER_MAX_FIELDS || max_rows < 1 || max_rows > ctx->grid.hy)
        return fail(ctx, CF_ERR_INVALID, "cf_peer_halo_export: %d fields (1…%d), %d rows (1…hy = %d)", max_fields,
                    PEER_MAX_FIELDS, max_rows, ctx->grid.hy);
    static_assert(sizeof(hipIpcMemHandle_t) <= CF_PEER_HANDLE_BYTES, "HIP IPC handle does not fit the ABI blob");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (ctx->peer_mine) return fail(ctx, CF_ERR_INVALID, "cf_peer_halo_export: this context already has a mailbox");
    const size_t slot = (size_t)max_fields * max_rows * ctx->grid.sj;
    const size_t bytes = PEER_FLAG_BYTES + 4 * slot * sizeof(double);
    cf::DeviceBuffer<char> mailbox;
    cf::DeviceBuffer<int> status;
    // fine-grained: stores arriving over xGMI and the owner's polling loads must meet in memory, not in a cache.
    // Mandatory: on coarse-grained memory the flag poll can spin to its timeout and — worse — the rows read
    // behind the flag can come from stale L2 lines, a silently wrong halo.  The caller falls back to the RCCL exchange.
    hipError_t e = mailbox.create_fine_grained(bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(ctx, CF_ERR_COMM, "cf_peer_halo_export: no fine-grained device memory for the halo mailbox (%s); use cf_halo_exchange_rows (RCCL)",
                    hipGetErrorString(e));
    }
    HIP_TRY(ctx, hipMemset(mailbox.get(), 0, bytes));
    const PeerShapeNote note{PEER_SHAPE_MAGIC, max_fields, max_rows, ctx->grid.sj, 0};
    HIP_TRY(ctx, hipMemcpy(mailbox.get() + PEER_SHAPE_OFFSET, &note, sizeof note, hipMemcpyHostToDevice));
    if (!ctx->d_peer_status) {
        HIP_TRY(ctx, status.create(sizeof(int)));
        HIP_TRY(ctx, hipMemset(status.get(), 0, sizeof(int)));
    }
    HIP_TRY(ctx, hipDeviceSynchronize());
    hipIpcMemHandle_t h;
    std::memset(&h, 0, sizeof h);
    e = hipIpcGetMemHandle(&h, mailbox.get());
    if (e != hipSuccess) return fail(ctx, CF_ERR_HIP, "hipIpcGetMemHandle on the halo mailbox: %s", hipGetErrorString(e));
    // everything succeeded: the context takes the mailbox (and a status word it did not have yet)
    if (status) ctx->d_peer_status = std::move(status);
    ctx->peer_mine = std::move(mailbox);
    ctx->peer.mine = ctx->peer_mine.get();
    ctx->peer.data_offset = PEER_FLAG_BYTES;
    ctx->peer.slot_doubles = slot;
    ctx->peer_max_fields = max_fields;
    ctx->peer_max_rows = max_rows;
    std::memset(handle_out, 0, CF_PEER_HANDLE_BYTES);
    std::memcpy(handle_out, &h, sizeof h);
    {
        std::lock_guard<std::mutex> lock(g_peer_mutex);
        g_peer_local[std::string((const char*)handle_out, CF_PEER_HANDLE_BYTES)] = {ctx->peer.mine, ctx->device};
    }
    return CF_OK;
}

// `*out`: the neighbour's mailbox behind `handle` (NULL without one); `*mapping` owns it where HIP IPC had to open it
int cf_peer_map_mailbox(cf_ctx* ctx, const void* handle, char** out, cf::IpcMapping* mapping) {
    *out = nullptr;
    mapping->reset();
    if (!handle) return CF_OK;
    {
        std::lock_guard<std::mutex> lock(g_peer_mutex);
        auto it = g_peer_local.find(std::string((const char*)handle, CF_PEER_HANDLE_BYTES));
        if (it != g_peer_local.end()) {  // exported by this very process
            const int dev = it->second.second;
            if (dev != ctx->device) {
                int can = 0;
                HIP_TRY(ctx, hipDeviceCanAccessPeer(&can, ctx->device, dev));
                if (!can) return fail(ctx, CF_ERR_COMM, "device %d cannot access its neighbour's device %d", ctx->device, dev);
                hipError_t e = hipDeviceEnablePeerAccess(dev, 0);
                if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled)
                    return fail(ctx, CF_ERR_HIP, "hipDeviceEnablePeerAccess(%d): %s", dev, hipGetErrorString(e));
                (void)hipGetLastError();
            }
            *out = it->second.first;
            return CF_OK;
        }
    }
    hipIpcMemHandle_t h;
    std::memcpy(&h, handle, sizeof h);
    hipError_t e = mapping->create(h);
    if (e != hipSuccess) return fail(ctx, CF_ERR_COMM, "hipIpcOpenMemHandle on a neighbour's halo mailbox: %s", hipGetErrorString(e));
    *out = (char*)mapping->get();
    return CF_OK;
}

// the neighbour's mailbox was exported for this context's shape on this context's row length (launches nothing: one copy)
static int check_mailbox_shape(cf_ctx* ctx, const char* mailbox, const char* which) {
    if (!mailbox) return CF_OK;
    PeerShapeNote theirs{};
    HIP_TRY(ctx, hipMemcpy(&theirs, mailbox + PEER_SHAPE_OFFSET, sizeof theirs, hipMemcpyDeviceToHost));
    if (theirs.magic != PEER_SHAPE_MAGIC)
        return fail(ctx, CF_ERR_INVALID, "cf_peer_halo_connect: the %s handle is not a mailbox of cf_peer_halo_export", which);
    if (theirs.max_fields != ctx->peer_max_fields || theirs.max_rows != ctx->peer_max_rows || theirs.sj != ctx->grid.sj)
        return fail(ctx, CF_ERR_INVALID,
                    "cf_peer_halo_connect: the %s neighbour's mailbox is (max_fields, max_rows, nx + 2hx) = (%d, %d, %d), this rank's "
                    "is (%d, %d, %d): all ranks export one shape on one grid width",
                    which, theirs.max_fields, theirs.max_rows, theirs.sj, ctx->peer_max_fields, ctx->peer_max_rows, ctx->grid.sj);
    return CF_OK;
}

// cf_peer_halo_connect that did not succeed leaves the context without neighbours, whatever it had before
static void disconnect_peers(cf_ctx* ctx) {
    ctx->peer_connected = false;
    ctx->peer.south = ctx->peer.north = nullptr;
    ctx->peer_south_map.reset();
    ctx->peer_north_map.reset();
}

int cf_peer_halo_connect(cf_ctx* ctx, const void* south_handle, const void* north_handle, int rank, int nranks) {
    if (!ctx || nranks <= 0 || rank < 0 || rank >= nranks) return fail(ctx, CF_ERR_INVALID, "cf_peer_halo_connect: bad arguments");
    if (!ctx->peer_mine) return fail(ctx, CF_ERR_INVALID, "cf_peer_halo_connect: call cf_peer_halo_export first");
    if (ctx->tile.connected)
        return fail(ctx, CF_ERR_INVALID, "cf_peer_halo_connect: this context is connected to a tile world (cf_peer_tile_connect): slabs or tiles");
    if ((rank > 0) != (south_handle != nullptr) || (rank < nranks - 1) != (north_handle != nullptr))
        return fail(ctx, CF_ERR_INVALID, "cf_peer_halo_connect: rank %d of %d needs %s south and %s north handle", rank, nranks,
                    rank > 0 ? "a" : "no", rank < nranks - 1 ? "a" : "no");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = cf_peer_map_mailbox(ctx, south_handle, &ctx->peer.south, &ctx->peer_south_map);
    if (rc == CF_OK) rc = cf_peer_map_mailbox(ctx, north_handle, &ctx->peer.north, &ctx->peer_north_map);
    if (rc == CF_OK) rc = check_mailbox_shape(ctx, ctx->peer.south, "south");
    if (rc == CF_OK) rc = check_mailbox_shape(ctx, ctx->peer.north, "north");
    if (rc != CF_OK) {
        disconnect_peers(ctx);
        return rc;
    }
    ctx->rank = rank;
    ctx->nranks = nranks;
    ctx->peer_connected = true;
    return CF_OK;
}

// what a peer-direct exchange of `nfields` × `rows` needs of the context (cf_halo_exchange_rows_peer, and cf_time_steps for all
// of its steps before the first of them)
static int check_peer_rows(cf_ctx* ctx, int nfields, int rows) {
    if (!ctx->peer_connected) return fail(ctx, CF_ERR_COMM, "cf_peer_halo_connect has not been called");
    if (nfields > ctx->peer_max_fields || rows < 1 || rows > ctx->peer_max_rows || rows > ctx->grid.ny)
        return fail(ctx, CF_ERR_INVALID, "cf_halo_exchange_rows_peer: %d fields / %d rows exceed the mailbox (%d / %d) or ny = %d",
                    nfields, rows, ctx->peer_max_fields, ctx->peer_max_rows, ctx->grid.ny);
    return CF_OK;
}

int cf_halo_exchange_rows_peer(cf_ctx* ctx, double* const* d_fields, int nfields, int rows) {
    if (!ctx || !d_fields || nfields <= 0) return fail(ctx, CF_ERR_INVALID, "cf_halo_exchange_rows_peer: bad arguments");
    CHECK(check_peer_rows(ctx, nfields, rows));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    PeerFields F{};
    F.n = nfields;
    for (int f = 0; f < nfields; ++f) {
        if (!d_fields[f]) return fail(ctx, CF_ERR_INVALID, "cf_halo_exchange_rows_peer: field %d is NULL", f);
        F.ptr[f] = d_fields[f];
    }
    return cf_peer_halo_launch_now(ctx, &F, rows);
}

int cf_peer_halo_launch_now(cf_ctx* ctx, const PeerFields* F, int rows) {
    // every rank counts its exchanges: the same number names the same step everywhere — counted once the kernel is queued (a
    // launch that failed is no exchange: this rank's sequence and mailbox parity would run ahead of its neighbours')
    HIP_TRY(ctx, launch_peer_halo(ctx->stream, ctx->peer, *F, ctx->grid, rows, ctx->peer_seq + 1, ctx->d_peer_status.get()));
    ++ctx->peer_seq;
    return CF_OK;
}

int cf_peer_halo_stats(cf_ctx* ctx, unsigned long long* exchanges, unsigned long long* in_solver_launch) {
    if (!ctx) return fail(nullptr, CF_ERR_INVALID, "ctx is NULL");
    if (exchanges) *exchanges = ctx->peer_seq;
    if (in_solver_launch) *in_solver_launch = ctx->halo_in_launch_count;
    return CF_OK;
}

// ---- the reduction world of the exact sums ------------------------------------------------------
constexpr unsigned long long REDUCE_MAGIC = 0x636f666c75787264ull;  // "cofluxrd"

int cf_peer_reduce_export(cf_ctx* ctx, void* handle_out) {
    if (!ctx || !handle_out) return fail(ctx, CF_ERR_INVALID, "cf_peer_reduce_export: NULL argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (ctx->reduce_mine) return fail(ctx, CF_ERR_INVALID, "cf_peer_reduce_export: this context already has a reduce mailbox");
    cf::DeviceBuffer<char> mailbox;
    cf::DeviceBuffer<int> status;
    // fine-grained, for the reason of the halo mailbox: the other ranks' stores and this rank's polling loads meet in memory
    hipError_t e = mailbox.create_fine_grained(REDUCE_MAILBOX_BYTES);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(ctx, CF_ERR_COMM, "cf_peer_reduce_export: no fine-grained device memory for the reduce mailbox (%s)", hipGetErrorString(e));
    }
    HIP_TRY(ctx, hipMemset(mailbox.get(), 0, REDUCE_MAILBOX_BYTES));
    const ReduceNote note{REDUCE_MAGIC, REDUCE_LAYOUT_VERSION, (unsigned)REDUCE_MAX_RANKS, (unsigned)REDUCE_SLOT_WORDS, 0, REDUCE_MAILBOX_BYTES};
    HIP_TRY(ctx, hipMemcpy(mailbox.get(), &note, sizeof note, hipMemcpyHostToDevice));
    if (!ctx->d_peer_status) {
        HIP_TRY(ctx, status.create(sizeof(int)));
        HIP_TRY(ctx, hipMemset(status.get(), 0, sizeof(int)));
    }
    HIP_TRY(ctx, hipDeviceSynchronize());
    hipIpcMemHandle_t h;
    std::memset(&h, 0, sizeof h);
    e = hipIpcGetMemHandle(&h, mailbox.get());
    if (e != hipSuccess) return fail(ctx, CF_ERR_HIP, "hipIpcGetMemHandle on the reduce mailbox: %s", hipGetErrorString(e));
    if (status) ctx->d_peer_status = std::move(status);
    ctx->reduce_mine = std::move(mailbox);
    std::memset(handle_out, 0, CF_PEER_HANDLE_BYTES);
    std::memcpy(handle_out, &h, sizeof h);
    {
        std::lock_guard<std::mutex> lock(g_peer_mutex);
        g_peer_local[std::string((const char*)handle_out, CF_PEER_HANDLE_BYTES)] = {ctx->reduce_mine.get(), ctx->device};
    }
    return CF_OK;
}

// cf_peer_reduce_connect that did not succeed leaves the context without a world, whatever it had before
static void disconnect_reduce_world(cf_ctx* ctx) {
    ctx->reduce_connected = false;
    ctx->reduce = ReduceWorld{nullptr, nullptr, 0, 1};
    for (cf::IpcMapping& m : ctx->reduce_maps) m.reset();
}

int cf_peer_reduce_connect(cf_ctx* ctx, const void* handles, int rank, int nranks) {
    if (!ctx) return fail(nullptr, CF_ERR_INVALID, "ctx is NULL");
    if (!ctx->reduce_mine) return fail(ctx, CF_ERR_INVALID, "cf_peer_reduce_connect: call cf_peer_reduce_export first");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // (a kernel of an earlier world may still be queued: it reads the table this call rewrites)
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    disconnect_reduce_world(ctx);
    if (nranks < 1 || nranks > CF_PEER_REDUCE_MAX_RANKS || rank < 0 || rank >= nranks || (nranks > 1 && !handles))
        return fail(ctx, CF_ERR_INVALID, "cf_peer_reduce_connect: rank %d of nranks = %d (1…%d), handles %s", rank, nranks,
                    CF_PEER_REDUCE_MAX_RANKS, handles ? "given" : "NULL");
    if (ctx->reduce_seq)   // the sequence numbers of a world start together
        return fail(ctx, CF_ERR_INVALID, "cf_peer_reduce_connect: this context has already reduced over a world (%llu reductions)", ctx->reduce_seq);
    char* table[REDUCE_MAX_RANKS] = {};
    int rc = CF_OK;
    for (int r = 0; r < nranks && rc == CF_OK; ++r) {
        if (r == rank) {
            table[r] = ctx->reduce_mine.get();
            continue;
        }
        rc = cf_peer_map_mailbox(ctx, (const char*)handles + (size_t)r * CF_PEER_HANDLE_BYTES, &table[r], &ctx->reduce_maps[r]);
        if (rc != CF_OK) break;
        ReduceNote theirs{};
        hipError_t e = hipMemcpy(&theirs, table[r], sizeof theirs, hipMemcpyDeviceToHost);
        if (e != hipSuccess)
            rc = fail(ctx, CF_ERR_HIP, "cf_peer_reduce_connect: reading rank %d's mailbox: %s", r, hipGetErrorString(e));
        else if (theirs.magic != REDUCE_MAGIC)
            rc = fail(ctx, CF_ERR_INVALID, "cf_peer_reduce_connect: the handle of rank %d is not a mailbox of cf_peer_reduce_export", r);
        else if (theirs.version != REDUCE_LAYOUT_VERSION || theirs.max_ranks != (unsigned)REDUCE_MAX_RANKS ||
                 theirs.slot_words != (unsigned)REDUCE_SLOT_WORDS || theirs.bytes != REDUCE_MAILBOX_BYTES)
            rc = fail(ctx, CF_ERR_INVALID, "cf_peer_reduce_connect: rank %d's mailbox has layout version %u, %u ranks, %u words per slot, %llu "
                      "bytes; this library's is %u, %d, %d, %zu", r, theirs.version, theirs.max_ranks, theirs.slot_words, theirs.bytes,
                      REDUCE_LAYOUT_VERSION, REDUCE_MAX_RANKS, REDUCE_SLOT_WORDS, REDUCE_MAILBOX_BYTES);
    }
    if (rc == CF_OK && !ctx->d_reduce_peers) {
        hipError_t e = ctx->d_reduce_peers.create(sizeof table);
        if (e != hipSuccess) rc = fail(ctx, CF_ERR_HIP, "cf_peer_reduce_connect: the table of mailboxes: %s", hipGetErrorString(e));
    }
    if (rc == CF_OK) {
        hipError_t e = hipMemcpy(ctx->d_reduce_peers.get(), table, sizeof table, hipMemcpyHostToDevice);
        if (e != hipSuccess) rc = fail(ctx, CF_ERR_HIP, "cf_peer_reduce_connect: the table of mailboxes: %s", hipGetErrorString(e));
    }
    if (rc != CF_OK) {
        disconnect_reduce_world(ctx);
        return rc;
    }
    ctx->reduce = ReduceWorld{ctx->reduce_mine.get(), ctx->d_reduce_peers.get(), rank, nranks};
    ctx->reduce_connected = true;
    return CF_OK;
}

// what the fold of `rows` rows needs of the grid (cf_fold_north_halo, and cf_time_steps with fold_north before its first step)
int check_fold_geometry(cf_ctx* ctx, int rows) {
    const GridDesc& G = ctx->grid;
    if (rows < 1 || rows > G.hy || rows + 1 > G.ny)
        return fail(ctx, CF_ERR_INVALID, "cf_fold_north_halo: rows = %d outside [1, min(hy, ny − 1)]", rows);
    if (G.nx % 2) return fail(ctx, CF_ERR_INVALID, "cf_fold_north_halo: a tripolar grid has an even number of columns (nx = %d)", G.nx);
    return CF_OK;
}

int cf_fold_north_halo(cf_ctx* ctx, double* const* d_fields, const int* locations, const double* signs, int nfields,
                       int rows) {
    if (!ctx || !d_fields || !locations || !signs || nfields <= 0 || nfields > PEER_MAX_FIELDS)
        return fail(ctx, CF_ERR_INVALID, "cf_fold_north_halo: bad arguments (1…%d fields)", PEER_MAX_FIELDS);
    const GridDesc& G = ctx->grid;
    CHECK(check_fold_geometry(ctx, rows));
    FoldFields F{};
    F.n = nfields;
    for (int f = 0; f < nfields; ++f) {
        if (!d_fields[f] || locations[f] < CF_FOLD_CENTER || locations[f] > CF_FOLD_Y_FACE)
            return fail(ctx, CF_ERR_INVALID, "cf_fold_north_halo: field %d is NULL or has an unknown location", f);
        F.ptr[f] = d_fields[f];
        F.location[f] = locations[f];
        F.sign[f] = signs[f];
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_fold_north(ctx->stream, F, G, rows));
    ++ctx->fold_launch_count;
    return CF_OK;
}

int cf_debug_fold_counts(cf_ctx* ctx, long long* fold_launches, long long* exchanges_with_fold) {
    if (!ctx) return fail(nullptr, CF_ERR_INVALID, "ctx is NULL");
    if (fold_launches) *fold_launches = ctx->fold_launch_count;
    if (exchanges_with_fold) *exchanges_with_fold = ctx->fold_exchange_count;
    return CF_OK;
}

int cf_discard_prefetched_atmosphere_state(cf_ctx* ctx) {
    if (!ctx) return fail(nullptr, CF_ERR_INVALID, "ctx is NULL");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // requested, not launched: never will be.  Launched on the auxiliary stream: whatever the caller does to that exchange set
    // next is ordered behind it
    const AheadLedger::Work W = ctx->ahead.discard();
    return cf_ahead_perform(ctx, &W);
}

// ---- run!(simulation) -------------------------------------------------------------------------
// cf_time_steps_coupled under CF_HALO_PEER: which rows cross a slab boundary, as exchanges of at most PEER_MAX_FIELDS fields.
// The split depends only on which optional fields are non-NULL (the same on every rank: the caller's contract, coflux.h).
// Every field carries how the tripolar fold maps it (location, sign): on the rank that owns the fold the exchange's north side
// folds the very fields it exchanges (coflux/distributed.py: coupled_fold_plan is the host statement of these two tables).
constexpr int COUPLED_MAX_EXCHANGES = 2;
struct RowField {
    const double* p;
    int location;
    double sign;
};
static int split_rows(const RowField* fields, int n, FoldFields* F) {
    int present = 0, sets = 0;
    for (int k = 0; k < n; ++k) {
        if (!fields[k].p) continue;
        if (present % PEER_MAX_FIELDS == 0) F[sets++] = FoldFields{};
        FoldFields& X = F[sets - 1];
        X.ptr[X.n] = const_cast<double*>(fields[k].p);
        X.location[X.n] = fields[k].location;
        X.sign[X.n] = fields[k].sign;
        ++X.n;
        ++present;
    }
    return sets;
}
// per step: the four ocean fields, as cf_time_steps exchanges and folds them, then the non-NULL fields of the step's ice state
// (scalars at cell centres; the ice velocities, which cf_sea_ice_state documents at cell centres, change sign across the fold)
static int coupled_step_rows(const cf_ocean_surface* o, const cf_sea_ice_state* is, FoldFields* F) {
    const RowField fields[10] = {{o->T, CF_FOLD_CENTER, 1.0},
                                 {o->S, CF_FOLD_CENTER, 1.0},
                                 {o->u, CF_FOLD_X_FACE, -1.0},
                                 {o->v, CF_FOLD_Y_FACE, -1.0},
                                 {is->concentration, CF_FOLD_CENTER, 1.0},
                                 {is->thickness, CF_FOLD_CENTER, 1.0},
                                 {is->snow_thickness, CF_FOLD_CENTER, 1.0},
                                 {is->u, CF_FOLD_CENTER, -1.0},
                                 {is->v, CF_FOLD_CENTER, -1.0},
                                 {is->albedo, CF_FOLD_CENTER, 1.0}};
    static_assert(10 <= COUPLED_MAX_EXCHANGES * PEER_MAX_FIELDS, "a step's rows fit its exchanges");
    return split_rows(fields, 10, F);
}
// once per call: the ice–ocean stresses (read at j + 1) and the carried skin temperature (first guess on the ring window)
static int coupled_call_rows(const cf_sea_ice_fields* ice, const cf_coupled_step* K, FoldFields* F) {
    const RowField fields[3] = {{ice ? ice->x_stress : nullptr, CF_FOLD_X_FACE, -1.0},
                                {ice ? ice->y_stress : nullptr, CF_FOLD_Y_FACE, -1.0},
                                {K->skin_temperature, CF_FOLD_CENTER, 1.0}};
    return split_rows(fields, 3, F);
}
// one exchange of the coupled loop: the exchange kernel, or on the rank that owns the fold the form whose north side folds
static int coupled_exchange(cf_ctx* ctx, const FoldFields* F, int rows, bool fold) {
    if (!fold) {
        PeerFields P{};
        P.n = F->n;
        for (int f = 0; f < F->n; ++f) P.ptr[f] = F->ptr[f];
        return cf_peer_halo_launch_now(ctx, &P, rows);
    }
    // counted like every exchange, once the kernel is queued: the sequence number names the same step on every rank
    HIP_TRY(ctx, launch_peer_halo_fold(ctx->stream, ctx->peer, *F, ctx->grid, rows, ctx->peer_seq + 1, ctx->d_peer_status.get()));
    ++ctx->peer_seq;
    ++ctx->fold_exchange_count;
    return CF_OK;
}

// cf_time_steps_coupled: what the block itself must satisfy (the schedule's scalars are checked already).  Every message names
// the field.
static int check_coupled_block(cf_ctx* ctx, const cf_run_schedule* S, const cf_atmos_source* src, const cf_interp_weights* w,
                               const cf_interface_fluxes* fluxes, const cf_sea_ice_fields* ice, const cf_net_ocean_fluxes* net,
                               const cf_coupled_step* K) {
    const char* fn = "cf_time_steps_coupled";
    if (K->struct_size != (int32_t)sizeof(cf_coupled_step))
        return fail(ctx, CF_ERR_INVALID, "cf_coupled_step.struct_size = %d, library expects %zu", K->struct_size, sizeof(cf_coupled_step));
    if (!ctx->ice_ready) return fail(ctx, CF_ERR_INVALID, "%s: cf_set_sea_ice_formulation has not been called", fn);
    if (S->halo_backend != CF_HALO_NONE && S->halo_backend != CF_HALO_PEER)
        return fail(ctx, CF_ERR_INVALID, "%s: halo_backend = %d, but nothing has exercised the ice rows or the global mean over RCCL: "
                    "CF_HALO_NONE or CF_HALO_PEER", fn, S->halo_backend);
    if (K->normalize_salinity < 0 || K->normalize_salinity > CF_NORMALIZE_EXACT)
        return fail(ctx, CF_ERR_INVALID, "%s: normalize_salinity = %d outside 0…%d", fn, K->normalize_salinity, CF_NORMALIZE_EXACT);
    if (K->n_ice_states < 1 || !K->ice_states) return fail(ctx, CF_ERR_INVALID, "%s: n_ice_states = %d (at least 1) or ice_states is NULL", fn, K->n_ice_states);
    for (int n = 0; n < K->n_ice_states; ++n) {
        if (!K->ice_states[n].concentration || !K->ice_states[n].thickness)
            return fail(ctx, CF_ERR_INVALID, "%s: ice_states[%d].concentration or .thickness is NULL", fn, n);
        // the partition reads ℵ of the step's ice state: a fixed pointer in `ice` can only be that of every state
        if (ice && ice->concentration && ice->concentration != K->ice_states[n].concentration)
            return fail(ctx, CF_ERR_INVALID, "%s: ice->concentration is not ice_states[%d].concentration: the partition and the interface "
                        "solve would read different ice (pass NULL: every step takes its ice state's)", fn, n);
    }
    if (!K->skin_temperature) return fail(ctx, CF_ERR_INVALID, "%s: skin_temperature is NULL", fn);
    if (S->fold_north) CHECK(check_fold_geometry(ctx, ctx->grid.ring + 1));   // (its messages name cf_fold_north_halo)
    if (S->halo_backend == CF_HALO_PEER) {
        if (!ctx->peer_connected)
            return fail(ctx, CF_ERR_INVALID, "%s: halo_backend = CF_HALO_PEER, but cf_peer_halo_connect has not been called", fn);
        int most = 0;   // the largest exchange of the call: the once-per-call set, and every ice state's split
        FoldFields F[COUPLED_MAX_EXCHANGES];
        for (int n = -1; n < K->n_ice_states; ++n) {
            const int sets = n < 0 ? coupled_call_rows(ice, K, F) : coupled_step_rows(&S->ocean_states[0], &K->ice_states[n], F);
            for (int e = 0; e < sets; ++e) most = std::max(most, F[e].n);
        }
        if (most > ctx->peer_max_fields || S->halo_rows > ctx->peer_max_rows || S->halo_rows > ctx->grid.ny)
            return fail(ctx, CF_ERR_INVALID, "%s: halo_backend = CF_HALO_PEER: exchanges of up to %d fields × %d rows exceed the halo mailbox "
                        "(%d fields × %d rows) or ny = %d", fn, most, S->halo_rows, ctx->peer_max_fields, ctx->peer_max_rows, ctx->grid.ny);
        if (S->fold_north && ctx->peer.north)
            return fail(ctx, CF_ERR_INVALID, "%s: fold_north with CF_HALO_PEER on a rank with a north neighbour (rank %d of %d): the fold "
                        "is the north side of the LAST rank's exchanges", fn, ctx->rank, ctx->nranks);
        if (K->normalize_salinity == 1)
            return fail(ctx, CF_ERR_INVALID, "%s: normalize_salinity = 1 under CF_HALO_PEER: its summation order depends on the slab; "
                        "CF_NORMALIZE_EXACT (2) gives the single domain's mean", fn);
        if (K->normalize_salinity == CF_NORMALIZE_EXACT && !ctx->reduce_connected)
            return fail(ctx, CF_ERR_INVALID, "%s: normalize_salinity = CF_NORMALIZE_EXACT under CF_HALO_PEER, but cf_peer_reduce_connect has not "
                        "been called", fn);
    }
    if (K->ai_fluxes.temperature && K->ai_fluxes.temperature != K->skin_temperature)
        return fail(ctx, CF_ERR_INVALID, "%s: ai_fluxes.temperature is neither NULL nor skin_temperature", fn);
    if (!K->net_ice.top_heat || !K->net_ice.bottom_heat) return fail(ctx, CF_ERR_INVALID, "%s: net_ice.top_heat or .bottom_heat is NULL", fn);
    if (K->land.friver) {
        if (!K->land_freshwater) return fail(ctx, CF_ERR_INVALID, "%s: land_freshwater is NULL", fn);
        if (K->land.ns_x <= 0 || K->land.ns_y <= 0 || K->land.n_levels <= 0 || K->land_first_level < 0 || K->land_first_level >= K->land.n_levels)
            return fail(ctx, CF_ERR_INVALID, "%s: land shape %dx%d, land_first_level = %d of %d levels", fn, K->land.ns_x, K->land.ns_y,
                        K->land_first_level, K->land.n_levels);
        if (!(K->land_time_fraction >= 0.0) || !(K->land_time_fraction_increment >= 0.0) || !std::isfinite(K->land_time_fraction) ||
            !std::isfinite(K->land_time_fraction_increment))
            return fail(ctx, CF_ERR_INVALID, "%s: land_time_fraction = %g, land_time_fraction_increment = %g", fn, K->land_time_fraction,
                        K->land_time_fraction_increment);
    }
    if (K->compute_ice_ocean && (!K->ice_ocean_fluxes.interface_heat || !K->ice_ocean_fluxes.salt_flux))
        return fail(ctx, CF_ERR_INVALID, "%s: ice_ocean_fluxes.interface_heat or .salt_flux is NULL", fn);
    cf_interface_fluxes ai = K->ai_fluxes;
    ai.temperature = K->skin_temperature;
    CHECK(check_coupled_update(ctx, src, w, S, fluxes, net, &ai));
    if (K->mean_out) {   // one double: it may not lie inside any ocean-grid array of the call (the normalisation would race with it)
        std::vector<const void*> arrays;
        auto add = [&](const void* p) {
            if (p) arrays.push_back(p);
        };
        auto add_fluxes = [&](const cf_interface_fluxes& f) {
            for (const void* p : {(const void*)f.sensible_heat, (const void*)f.latent_heat, (const void*)f.water_vapor, (const void*)f.x_momentum,
                                  (const void*)f.y_momentum, (const void*)f.temperature, (const void*)f.friction_velocity,
                                  (const void*)f.temperature_scale, (const void*)f.humidity_scale})
                add(p);
        };
        for (int n = 0; n < S->n_ocean_states; ++n) {
            const cf_ocean_surface& o = S->ocean_states[n];
            for (const void* p : {(const void*)o.T, (const void*)o.S, (const void*)o.u, (const void*)o.v}) add(p);
        }
        for (int n = 0; n < S->n_atmos_sets; ++n) {
            const cf_exchange_fields& e = S->atmos[n];
            for (const void* p : {(const void*)e.u, (const void*)e.v, (const void*)e.T, (const void*)e.p, (const void*)e.q, (const void*)e.Qs,
                                  (const void*)e.Ql, (const void*)e.Mp})
                add(p);
        }
        for (int n = 0; n < K->n_ice_states; ++n) {
            const cf_sea_ice_state& st = K->ice_states[n];
            for (const void* p : {(const void*)st.concentration, (const void*)st.thickness, (const void*)st.u, (const void*)st.v,
                                  (const void*)st.albedo, (const void*)st.snow_thickness})
                add(p);
        }
        add_fluxes(*fluxes);
        add_fluxes(ai);
        for (const void* p : {(const void*)net->u, (const void*)net->v, (const void*)net->T, (const void*)net->S,
                              (const void*)net->shortwave_surface_flux, (const void*)net->upwelling_longwave,
                              (const void*)net->downwelling_longwave, (const void*)net->downwelling_shortwave})
            add(p);
        if (ice) {
            add(ice->x_stress);
            add(ice->y_stress);
        }
        for (const void* p : {(const void*)K->net_ice.top_heat, (const void*)K->net_ice.bottom_heat, (const void*)K->land_freshwater,
                              (const void*)K->ice_ocean_fluxes.interface_heat, (const void*)K->ice_ocean_fluxes.salt_flux,
                              (const void*)K->ice_ocean_fluxes.frazil_heat, (const void*)K->ice_ocean_fluxes.friction_velocity,
                              (const void*)K->target_salinity, (const void*)K->restoring_buffer, (const void*)K->area})
            add(p);
        const uintptr_t bytes = (uintptr_t)ctx->grid.sj * (uintptr_t)(ctx->grid.ny + 2 * ctx->grid.hy) * sizeof(double);
        const uintptr_t m = (uintptr_t)K->mean_out;
        for (const void* p : arrays)
            if (m + sizeof(double) > (uintptr_t)p && m < (uintptr_t)p + bytes)
                return fail(ctx, CF_ERR_INVALID, "%s: mean_out lies inside another array of the call", fn);
    }
    return CF_OK;
}

// The one step loop behind cf_time_steps (K = NULL: per step cf_update_state) and cf_time_steps_coupled (K: the coupled block —
// per step the preamble, cf_update_state_sea_ice and the normalisation).  `name`: the entry point, for the messages.
static int time_steps_loop(cf_ctx* ctx, const char* name, int64_t first_step, int nsteps, const cf_run_schedule* S,
                           const cf_atmos_source* src, const cf_interp_weights* w, const cf_interface_fluxes* fluxes,
                           const cf_sea_ice_fields* ice, const cf_net_ocean_fluxes* net, const cf_coupled_step* K) {
    if (!ctx || !S || !src || !w) return fail(ctx, CF_ERR_INVALID, "%s: NULL argument", name);
    if (S->struct_size != (int32_t)sizeof(cf_run_schedule))
        return fail(ctx, CF_ERR_INVALID, "cf_run_schedule.struct_size = %d, library expects %zu", S->struct_size, sizeof(cf_run_schedule));
    if (nsteps < 0 || first_step < 0 || S->n_ocean_states < 1 || !S->ocean_states || !S->atmos)
        return fail(ctx, CF_ERR_INVALID, "%s: bad schedule", name);
    if (S->pipeline < 0 || S->pipeline > CF_PIPELINE_CONTINUING) return fail(ctx, CF_ERR_INVALID, "%s: pipeline = %d", name, S->pipeline);
    if (S->n_atmos_sets < 1 || S->n_atmos_sets > 2 || (S->pipeline && S->n_atmos_sets != 2))
        return fail(ctx, CF_ERR_INVALID, "%s: %d exchange-field sets (pipelining needs 2)", name, S->n_atmos_sets);
    if (!(S->time_fraction >= 0.0) || !(S->time_fraction_increment >= 0.0) || S->first_level < 0 || S->first_level >= src->n_levels)
        return fail(ctx, CF_ERR_INVALID, "%s: bad clock (fraction %g, increment %g, level %d of %d)", name, S->time_fraction,
                    S->time_fraction_increment, S->first_level, src->n_levels);
    if (S->halo_backend != CF_HALO_NONE && S->halo_rows != ctx->grid.ring + 1)
        return fail(ctx, CF_ERR_INVALID, "%s: halo_rows = %d, but the ring row reads v[j+1]: rows must be ring + 1 = %d", name,
                    S->halo_rows, ctx->grid.ring + 1);
    auto source_at = [&](int64_t step) {
        cf_atmos_source s = *src;
        const double total = S->time_fraction + (double)step * S->time_fraction_increment;
        const double whole = std::floor(total);
        s.level1 = (int)((S->first_level + (int64_t)whole) % src->n_levels);
        s.level2 = (s.level1 + 1) % src->n_levels;
        s.time_fraction = total - whole;
        return s;
    };
    // the dataset the coupled block's restoring job follows, if one is attached and the block has the job: step s restores toward
    // S★ at time_origin + s · step_seconds, the time of the ocean state it reads (checked for every step before the first launch)
    const cf_dataset* dataset = K && K->restoring_buffer ? static_cast<const cf_dataset*>(ctx->restoring_dataset.handle) : nullptr;
    auto target_at = [&](int64_t step) {
        DatasetTarget T{};
        const StepSchedule& when = ctx->restoring_dataset.when;
        (void)dataset_target_at(dataset, name, when.time_origin + (double)step * when.step_seconds, &T);
        return T;
    };
    // the coupled block's preamble for step `step`: the land clock runs by source_at's arithmetic on the block's own fields
    auto prepare_at =[&](int64_t step, const cf_ocean_surface* o, const cf_sea_ice_state* is) {
        cf_coupled_prepare P{};
        P.struct_size = (int32_t)sizeof(cf_coupled_prepare);
        P.ocean = *o;
        if (K->land.friver) {
            P.weights = *w;
            P.land = K->land;
            const double total = K->land_time_fraction + (double)step * K->land_time_fraction_increment;
            const double whole = std::floor(total);
            P.land.level1 = (int)((K->land_first_level + (int64_t)whole) % K->land.n_levels);
            P.land.level2 = (P.land.level1 + 1) % K->land.n_levels;
            P.land.time_fraction = total - whole;
            P.land_freshwater = K->land_freshwater;
        }
        if (K->compute_ice_ocean) {
            P.ice_ocean = K->ice_ocean;
            P.concentration = is->concentration;
            P.x_stress = ice ? ice->x_stress : nullptr;
            P.y_stress = ice ? ice->y_stress : nullptr;
            P.ice_ocean_fluxes = K->ice_ocean_fluxes;
        }
        if (K->restoring_buffer) {
            P.piston_velocity = K->piston_velocity;
            P.target_salinity = dataset ? target_at(step).level1 : K->target_salinity;
            P.restoring_buffer = K->restoring_buffer;
        }
        return P;
    };
    if (K) {   // everything the steps' own entry points would refuse, before the first launch: the outputs stay untouched
        if (ctx->tile.connected && ctx->tile.place.px > 1)
            return fail(ctx, CF_ERR_INVALID, "%s: this context is connected to a tile world with px = %d: the ice rows and the stresses do not cross "
                        "x yet; cf_time_steps steps a tile world, the coupled loop latitude slabs (px = 1, cf_peer_halo_connect)", name, ctx->tile.place.px);
        CHECK(check_coupled_block(ctx, S, src, w, fluxes, ice, net, K));
        if (dataset) {
            if (K->target_salinity)
                return fail(ctx, CF_ERR_INVALID, "%s: target_salinity is given and a restoring dataset is attached (one of the two)", name);
            DatasetTarget T{};
            for (int64_t step = first_step; step < first_step + nsteps; ++step)
                CHECK(dataset_target_at(dataset, name, ctx->restoring_dataset.when.time_origin +
                                                           (double)step * ctx->restoring_dataset.when.step_seconds, &T));
        }
        for (int n = 0; n < S->n_ocean_states; ++n) {
            const cf_coupled_prepare P = prepare_at(first_step, &S->ocean_states[n], &K->ice_states[0]);
            CHECK(check_coupled_prepare(ctx, &P));
        }
    }
    // what is attached says whether the call may run — a series that would overflow, a calendar table that does not cover a step
    // it would collect: nothing is launched.  (The series are asked first: which refusal a call with two gets is part of the ABI.)
    for (int k : {cf_ctx::AT_INTEGRALS, cf_ctx::AT_MONITOR, cf_ctx::AT_CLIMATOLOGY})
        if (const Attachment& at = ctx->attached[k]; at.handle) CHECK(at.handle->admit(at, name, first_step, nsteps));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    for (int n = 0; n < S->n_ocean_states; ++n) {
        if (ctx->dev.mask_kind != CF_MASK_NONE && !S->ocean_states[n].mask) return fail(ctx, CF_ERR_INVALID, "ocean state %d has no mask", n);
        // one static wet mask per schedule: another mask pointer would make cf_update_state rebuild the solver's schedule
        // INSIDE the step loop (a stream synchronisation behind a queued peer-direct halo kernel that waits for its
        // neighbour, and a rebuild per step when states alternate: ADVICE r2)
        if (S->ocean_states[n].mask != S->ocean_states[0].mask)
            return fail(ctx, CF_ERR_INVALID, "%s: ocean state %d carries a different mask pointer than state 0; the states of a "
                        "schedule share one wet mask", name, n);
    }
    // cf_time_steps: everything one of its steps would refuse, at whichever step, is refused here — before the first launch and
    // before anything of the context changes (the chunk table, the ledger of requested states, the halo request, the land-zero
    // scope), as check_coupled_block does for the coupled form.  Behind the attachments: which refusal a call with two gets …
    // A tile-connected context (cf_peer_tile_connect): CF_HALO_PEER is the tile exchange of the four ocean fields, whose check
    // covers the mailbox, the geometry and whether fold_north agrees with the rank's place in the world.
    const bool tile_peer = ctx->tile.connected && S->halo_backend == CF_HALO_PEER;
    if (!K) {
        CHECK(check_step_arguments(ctx, src, w, S, fluxes, net));
        if (ctx->tile.connected && S->halo_backend == CF_HALO_RCCL)
            return fail(ctx, CF_ERR_INVALID, "%s: halo_backend = CF_HALO_RCCL on a context connected to a tile world: CF_HALO_PEER", name);
        if (tile_peer) CHECK(check_tile_exchange(ctx, name, 4, S->halo_rows, S->fold_north));
        else if (S->fold_north) CHECK(check_fold_geometry(ctx, ctx->grid.ring + 1));
        if (S->halo_backend == CF_HALO_PEER && !tile_peer) CHECK(check_peer_rows(ctx, 4, S->halo_rows));
    }
    CHECK(cf_ensure_chunk_table(ctx, S->ocean_states[0].mask));
    // CF_OPT_HALO_IN_SOLVER_LAUNCH: a step's request lives from its arming below to the cf_update_state of the same iteration;
    // by whatever way this function returns, none stays armed for a later cf_update_state of the host
    HaloRequestScope halo_request_scope(ctx);
    static const int fold_loc[4] = {CF_FOLD_CENTER, CF_FOLD_CENTER, CF_FOLD_X_FACE, CF_FOLD_Y_FACE};
    static const double fold_sign[4] = {1.0, 1.0, -1.0, -1.0};
    const bool coupled_peer = K && S->halo_backend == CF_HALO_PEER;
    // on the rank that owns the fold every exchange of the coupled loop folds its own fields as its north side (the four ocean
    // fields ride in the step's first exchange): the same number of launches per step on every rank, and no fold launch of its own
    const bool fold_in_exchange = coupled_peer && S->fold_north;
    if (coupled_peer && nsteps > 0) {   // once per call: afterwards both neighbours recompute the skin temperature's ring rows
        FoldFields F[COUPLED_MAX_EXCHANGES];   // (and beyond the fold the solve recomputes its north ring row from folded inputs)
        const int sets = coupled_call_rows(ice, K, F);
        for (int e = 0; e < sets; ++e) CHECK(coupled_exchange(ctx, &F[e], S->halo_rows, fold_in_exchange));
    }
    if (S->pipeline && nsteps > 0) {  // the first step's atmosphere, unless a previous call already started it
        const cf_atmos_source s0 = source_at(first_step);
        const cf_exchange_fields* a0 = &S->atmos[first_step % 2];
        const AheadLedger::FirstStep F = ctx->ahead.first_step_of_call(a0->u, s0, *w);
        CHECK(cf_ahead_perform(ctx, &F.work));
        if (F.needed && ctx->merged_prefetch != 0) {
            // the merged forms keep everything on the context's stream: so does the first step's interpolation.  (A state of
            // this set that is not the one this step asks for may have left on the auxiliary stream — under
            // CF_OPT_MERGED_PREFETCH = 0 before a switch, or sent off by this very request: the launch is ordered behind it)
            const AheadLedger::Record* rec;
            CHECK(book_request(ctx, &s0, w, a0, true, &rec));
            HIP_TRY(ctx, launch_interpolate(ctx->stream, ctx->launch, ctx->grid, &s0, w, a0));
            ctx->ahead.leave_main(rec, AheadLedger::OWN);
        } else if (F.needed) {
            CHECK(request_prefetch(ctx, &s0, w, a0, false));
        }
    }
    // CF_OPT_LAND_ZEROS: the steps below are one loop over fixed outputs, one mask pointer and one chunk table (checked above) —
    // cf_update_state may leave the land cells to the first of them.  Closed on every way out of this function.
    // (the coupled form does not open one: it writes the land at every step, as the host loop of its entry points does)
    std::optional<LandZeroScope> land_zero_scope;
    if (!K) land_zero_scope.emplace(ctx);
    for (int64_t step = first_step; step < first_step + nsteps; ++step) {
        const cf_ocean_surface* o = &S->ocean_states[step % S->n_ocean_states];
        double* rows[4] = {const_cast<double*>(o->T), const_cast<double*>(o->S), const_cast<double*>(o->u),
                           const_cast<double*>(o->v)};
        if (S->halo_backend == CF_HALO_RCCL)
            CHECK(cf_halo_exchange_rows(ctx, rows, 4, S->halo_rows));
        else if (coupled_peer) {
            // (CF_OPT_HALO_IN_SOLVER_LAUNCH arms no request here: the coupled step's solver launch is not the one that carries riders)
            FoldFields F[COUPLED_MAX_EXCHANGES];
            const int sets = coupled_step_rows(o, &K->ice_states[step % K->n_ice_states], F);
            for (int e = 0; e < sets; ++e) CHECK(coupled_exchange(ctx, &F[e], S->halo_rows, fold_in_exchange));
        } else if (tile_peer) {
            // (CF_OPT_HALO_IN_SOLVER_LAUNCH arms no request on a tile world: the exchange kernels run.  On a world one tile wide
            // the exchange ends with the local fold's launch)
            FoldFields F{};
            F.n = 4;
            for (int f = 0; f < 4; ++f) {
                F.ptr[f] = rows[f];
                F.location[f] = fold_loc[f];
                F.sign[f] = fold_sign[f];
            }
            CHECK(tile_exchange_launch(ctx, &F, S->halo_rows, S->fold_north));
        } else if (S->halo_backend == CF_HALO_PEER) {
            if (ctx->halo_in_launch) {   // (the mailbox takes 4 fields × halo_rows: check_peer_rows above)
                // CF_OPT_HALO_IN_SOLVER_LAUNCH: left as a request — this step's solver launch carries the exchange as rider
                // workgroups where it can, cf_update_state issues the exchange kernel in front of the solver where it cannot
                ctx->halo_request.F = PeerFields{};
                ctx->halo_request.F.n = 4;
                for (int f = 0; f < 4; ++f) ctx->halo_request.F.ptr[f] = rows[f];
                ctx->halo_request.rows = S->halo_rows;
                ctx->halo_request.valid = true;
            } else {
                CHECK(cf_halo_exchange_rows_peer(ctx, rows, 4, S->halo_rows));
            }
        }
        if (S->fold_north && !fold_in_exchange && !tile_peer) CHECK(cf_fold_north_halo(ctx, rows, fold_loc, fold_sign, 4, ctx->grid.ring + 1));
        const cf_sea_ice_state* is = K ? &K->ice_states[step % K->n_ice_states] : nullptr;
        if (K) {
            const cf_coupled_prepare P = prepare_at(step, o, is);
            if (dataset) {
                const DatasetTarget T = target_at(step);
                CHECK(prepare_coupled_step_levels(ctx, &P, T.level2, T.fraction));
            } else {
                CHECK(cf_prepare_coupled_step(ctx, &P));
            }
            if (K->land.friver) ctx->d_land_freshwater = K->land_freshwater;   // cf_set_land_freshwater
        }
        const cf_atmos_source s = source_at(step);
        const cf_exchange_fields* a = &S->atmos[S->n_atmos_sets == 2 ? step % 2 : 0];
        // CF_PIPELINE_WITHIN_CALL: nothing beyond this call's steps is read or written.  CF_PIPELINE_CONTINUING: the last
        // step also requests step first_step + nsteps (the loop goes on in the next call, which finds that state pending
        // by its key; the caller promises the source levels of that step are resident and final, and that the other
        // exchange set is not read after this call's last step: coflux.h).
        // queued BEFORE this step's kernels: the set it overwrites was last read by the previous step's net fluxes
        if (S->pipeline && (step + 1 < first_step + nsteps || S->pipeline == CF_PIPELINE_CONTINUING)) {
            const cf_atmos_source sn = source_at(step + 1);
            CHECK(cf_prefetch_atmosphere_state(ctx, &sn, w, &S->atmos[(step + 1) % 2]));
        }
        if (K) {
            cf_sea_ice_fields partition{};   // ℵ of this step's ice state, the caller's stresses, the block's ice–ocean fluxes
            if (ice) partition = *ice;
            partition.concentration = is->concentration;
            partition.interface_heat = K->ice_ocean_fluxes.interface_heat;
            partition.salt_flux = K->ice_ocean_fluxes.salt_flux;
            cf_sea_ice_state state = *is;    // the skin temperature is carried: first guess and result in one buffer
            state.top_temperature = K->skin_temperature;
            cf_interface_fluxes ai = K->ai_fluxes;
            ai.temperature = K->skin_temperature;
            CHECK(cf_update_state_sea_ice(ctx, &s, w, o, a, fluxes, &partition, net, &state, &ai, K->ice_ocean_fluxes.frazil_heat,
                                          K->ice_ocean_fluxes.interface_heat, &K->net_ice));
            if (K->normalize_salinity == CF_NORMALIZE_EXACT)
                CHECK(cf_normalize_salinity_flux_exact(ctx, net->S, K->restoring_buffer, K->area, o->mask, K->mean_out));
            else if (K->normalize_salinity)
                CHECK(cf_normalize_salinity_flux(ctx, net->S, K->restoring_buffer, K->area, o->mask, K->mean_out));
        } else {
            CHECK(cf_update_state(ctx, &s, w, o, a, fluxes, ice, net));
        }
        // what is attached collects where its schedule says the step is due, in the order of cf_ctx::attached: the averagers in
        // slot order, the climatology, the integrator, the monitor.  Queued behind every launch of the step — the
        // face stresses of the merged and tail forms included
        for (const Attachment& at : ctx->attached)
            if (at.collects(step)) CHECK(at.handle->collect_step(at, step));
    }
    return CF_OK;
}

int cf_time_steps(cf_ctx* ctx, int64_t first_step, int nsteps, const cf_run_schedule* S, const cf_atmos_source* src,
                  const cf_interp_weights* w, const cf_interface_fluxes* fluxes, const cf_sea_ice_fields* ice,
                  const cf_net_ocean_fluxes* net) {
    return time_steps_loop(ctx, "cf_time_steps", first_step, nsteps, S, src, w, fluxes, ice, net, nullptr);
}

int cf_time_steps_coupled(cf_ctx* ctx, int64_t first_step, int nsteps, const cf_run_schedule* S, const cf_atmos_source* src,
                          const cf_interp_weights* w, const cf_interface_fluxes* fluxes, const cf_sea_ice_fields* ice,
                          const cf_net_ocean_fluxes* net, const cf_coupled_step* coupled) {
    if (ctx && !coupled) return fail(ctx, CF_ERR_INVALID, "cf_time_steps_coupled: the coupled block is NULL");
    return time_steps_loop(ctx, "cf_time_steps_coupled", first_step, nsteps, S, src, w, fluxes, ice, net, coupled);
}

}  // extern "C"
