// coflux_tiles.cpp — the tile world (include/coflux.h: cf_peer_tile_*): a px × py partition of the surface whose ranks exchange
// x-halo columns, y-halo rows and, on the top row of a tripolar world, the fold with the partner tile (px − 1 − p, py − 1).
// The arithmetic of the world is coflux_tile_geometry.hpp's (plain C++), the device side coflux_halo_device.hpp's
// (tile_halo_x_side, tile_halo_y_side); here are the mailbox, the connection and the two launches of an exchange.
#include "coflux_ctx.hpp"

// cf_peer_tile_connect that did not succeed leaves the context unconnected, whatever it had before
static void disconnect_tiles(cf_ctx* ctx) {
    cf_ctx::TileWorld& W = ctx->tile;
    W.connected = false;
    W.tripolar = false;
    W.place = TilePlace{};
    for (int s = 0; s < 4; ++s) {
        W.M.remote[s] = nullptr;
        W.M.remote_slot[s] = nullptr;
    }
    for (cf::IpcMapping& m : W.maps) m.reset();
}

// how many columns a rank's x-phase fills west and east, and whether its north side sends a fold to a partner
struct TileCall {
    int wcols, ecols;
    bool sends_fold, local_fold;
};
static TileCall tile_call(const cf_ctx* ctx, int fold_north) {
    TileCall C{};
    C.sends_fold = fold_north && ctx->tile.place.partner_north;
    C.local_fold = fold_north && !ctx->tile.place.partner_north;   // px = 1: the partner is this rank
    tile_phase_columns(ctx->grid.ring, C.sends_fold, &C.wcols, &C.ecols);
    return C;
}

int check_tile_exchange(cf_ctx* ctx, const char* fn, int nfields, int rows, int fold_north) {
    const cf_ctx::TileWorld& W = ctx->tile;
    const GridDesc& G = ctx->grid;
    if (!W.connected) return fail(ctx, CF_ERR_COMM, "%s: cf_peer_tile_connect has not been called", fn);
    const bool top_fold = W.tripolar && W.place.top_row;
    if ((fold_north != 0) != top_fold)
        return fail(ctx, CF_ERR_INVALID, "%s: fold_north = %d on rank (p, q) = (%d, %d) of a %d x %d %s world: fold_north is 1 on every rank "
                    "of the top row of a tripolar world and 0 everywhere else", fn, fold_north, W.place.p, W.place.q, W.place.px, W.place.py,
                    W.tripolar ? "tripolar" : "latitude-longitude");
    const TileCall C = tile_call(ctx, fold_north);
    if (nfields < 1 || nfields > W.note.max_fields || rows < 1 || rows > W.note.max_rows || rows > G.ny || rows > G.hy ||
        (W.place.px > 1 && C.ecols > W.note.max_cols))
        return fail(ctx, CF_ERR_INVALID, "%s: the tile mailbox (%d fields x %d rows x %d columns) does not take %d fields x %d rows x %d columns "
                    "(ring + 1%s), or rows exceeds ny = %d or hy = %d", fn, W.note.max_fields, W.note.max_rows, W.note.max_cols, nfields, rows,
                    W.place.px > 1 ? C.ecols : 0, C.sends_fold ? ", and one more east column under the fold" : "", G.ny, G.hy);
    if (W.place.px > 1 && (G.nx < C.ecols || G.hx < C.ecols))
        return fail(ctx, CF_ERR_INVALID, "%s: nx = %d, hx = %d, but the x-phase moves %d columns", fn, G.nx, G.hx, C.ecols);
    if (C.local_fold) CHECK(check_fold_geometry(ctx, rows));
    if (C.sends_fold && rows + 1 > G.ny)
        return fail(ctx, CF_ERR_INVALID, "%s: fold_north with rows = %d on a tile of ny = %d rows: the fold reads rows ny - 1 - rows ... ny - 1", fn,
                    rows, G.ny);
    return CF_OK;
}

int tile_exchange_launch(cf_ctx* ctx, const FoldFields* F, int rows, int fold_north) {
    cf_ctx::TileWorld& W = ctx->tile;
    const TileCall C = tile_call(ctx, fold_north);
    const unsigned long long seq = W.seq + 1;   // one number per exchange, the same on every rank: both phases carry it
    PeerFields P{};
    P.n = F->n;
    for (int f = 0; f < F->n; ++f) P.ptr[f] = F->ptr[f];
    const bool columns = W.place.px > 1;
    if (columns) HIP_TRY(ctx, launch_tile_halo_x(ctx->stream, W.M, P, ctx->grid, C.wcols, C.ecols, seq, ctx->d_peer_status.get()));
    TileFold fold{};
    if (C.sends_fold) {
        fold.cols = ctx->grid.ring + 1;
        fold.g0 = (W.place.px - 1 - W.place.p) * ctx->grid.nx;   // the partner's first global column
        fold.Nx = W.place.px * ctx->grid.nx;
    }
    if (W.M.remote[TILE_S] || W.M.remote[TILE_N])
        HIP_TRY(ctx, launch_tile_halo_y(ctx->stream, W.M, *F, ctx->grid, rows, fold, seq, ctx->d_peer_status.get()));
    if (C.local_fold) {
        HIP_TRY(ctx, launch_fold_north(ctx->stream, *F, ctx->grid, rows));
        ++ctx->fold_launch_count;
    }
    // counted once everything is queued, as the slabs count theirs
    ++W.seq;
    if (columns) ++W.column_launches;
    if (C.sends_fold) ++W.folds_sent;
    return CF_OK;
}

extern "C" {

int cf_peer_tile_export(cf_ctx* ctx, int max_fields, int max_rows, int max_cols, void* handle_out) {
    if (!ctx || !handle_out) return fail(ctx, CF_ERR_INVALID, "cf_peer_tile_export: NULL argument");
    const GridDesc& G = ctx->grid;
    if (max_fields < 1 || max_fields > PEER_MAX_FIELDS || max_rows < 1 || max_rows > G.hy || max_cols < 1 || max_cols > G.hx)
        return fail(ctx, CF_ERR_INVALID, "cf_peer_tile_export: %d fields (1…%d), %d rows (1…hy = %d), %d columns (1…hx = %d)", max_fields,
                    PEER_MAX_FIELDS, max_rows, G.hy, max_cols, G.hx);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (ctx->tile.mine) return fail(ctx, CF_ERR_INVALID, "cf_peer_tile_export: this context already has a tile mailbox");
    const TileNote note{TILE_MAGIC, max_fields, max_rows, max_cols, G.sj, G.ny, G.hx, G.hy, 0};
    const size_t bytes = tile_mailbox_bytes(note);
    cf::DeviceBuffer<char> mailbox;
    cf::DeviceBuffer<int> status;
    // fine-grained, for the reason of the slabs' mailbox: the neighbours' stores and this rank's polling loads meet in memory
    hipError_t e = mailbox.create_fine_grained(bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(ctx, CF_ERR_COMM, "cf_peer_tile_export: no fine-grained device memory for the tile mailbox (%s)", hipGetErrorString(e));
    }
    HIP_TRY(ctx, hipMemset(mailbox.get(), 0, bytes));
    HIP_TRY(ctx, hipMemcpy(mailbox.get() + TILE_NOTE_OFFSET, &note, sizeof note, hipMemcpyHostToDevice));
    if (!ctx->d_peer_status) {
        HIP_TRY(ctx, status.create(sizeof(int)));
        HIP_TRY(ctx, hipMemset(status.get(), 0, sizeof(int)));
    }
    HIP_TRY(ctx, hipDeviceSynchronize());
    hipIpcMemHandle_t h;
    std::memset(&h, 0, sizeof h);
    e = hipIpcGetMemHandle(&h, mailbox.get());
    if (e != hipSuccess) return fail(ctx, CF_ERR_HIP, "hipIpcGetMemHandle on the tile mailbox: %s", hipGetErrorString(e));
    if (status) ctx->d_peer_status = std::move(status);
    cf_ctx::TileWorld& W = ctx->tile;
    W.mine = std::move(mailbox);
    W.note = note;
    W.M = TileMailbox{};
    W.M.mine = W.mine.get();
    W.M.x_slot = tile_x_slot(note);
    W.M.y_slot = tile_y_slot(note);
    for (int s = 0; s < 4; ++s) W.M.my_slot[s] = reinterpret_cast<double*>(W.M.mine + tile_slot_offset(note, s));
    std::memset(handle_out, 0, CF_PEER_HANDLE_BYTES);
    std::memcpy(handle_out, &h, sizeof h);
    cf_peer_remember_local(handle_out, W.M.mine, ctx->device);
    return CF_OK;
}

int cf_peer_tile_connect(cf_ctx* ctx, const void* handles, int px, int py, int rank, int tripolar) {
    if (!ctx) return fail(nullptr, CF_ERR_INVALID, "ctx is NULL");
    cf_ctx::TileWorld& W = ctx->tile;
    if (!W.mine) return fail(ctx, CF_ERR_INVALID, "cf_peer_tile_connect: call cf_peer_tile_export first");
    if (ctx->peer_connected)
        return fail(ctx, CF_ERR_INVALID, "cf_peer_tile_connect: this context is connected to latitude slabs (cf_peer_halo_connect): slabs or tiles");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // (a kernel of an earlier world may still be queued: it reads the mappings this call replaces)
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    disconnect_tiles(ctx);
    char why[200];
    if (tile_world_refusal(px, py, rank, tripolar, ctx->grid.nx, why, sizeof why)) return fail(ctx, CF_ERR_INVALID, "cf_peer_tile_connect: %s", why);
    const TilePlace T = tile_place(px, py, rank, tripolar != 0);
    if (px * py > 1 && !handles) return fail(ctx, CF_ERR_INVALID, "cf_peer_tile_connect: handles is NULL in a world of %d ranks", px * py);
    static const char* const side_name[4] = {"west", "east", "south", "north"};
    char* base[TILE_MAX_RANKS] = {};
    int rc = CF_OK;
    for (int s = 0; s < 4 && rc == CF_OK; ++s) {
        const int r = T.neighbour[s];
        if (r < 0) continue;
        const char* which = s == TILE_N && T.partner_north ? "fold partner" : side_name[s];
        if (!base[r]) rc = cf_peer_map_mailbox(ctx, (const char*)handles + (size_t)r * CF_PEER_HANDLE_BYTES, &base[r], &W.maps[r]);
        if (rc != CF_OK) break;
        TileNote theirs{};
        hipError_t e = hipMemcpy(&theirs, base[r] + TILE_NOTE_OFFSET, sizeof theirs, hipMemcpyDeviceToHost);
        if (e != hipSuccess) {
            rc = fail(ctx, CF_ERR_HIP, "cf_peer_tile_connect: reading rank %d's mailbox: %s", r, hipGetErrorString(e));
        } else if (theirs.magic != TILE_MAGIC) {
            rc = fail(ctx, CF_ERR_INVALID, "cf_peer_tile_connect: the handle of rank %d (%s) is not a mailbox of cf_peer_tile_export", r, which);
        } else if (!tile_notes_agree(W.note, theirs, s)) {
            char a[160], b[160];
            tile_note_text(theirs, a, sizeof a);
            tile_note_text(W.note, b, sizeof b);
            rc = fail(ctx, CF_ERR_INVALID, "cf_peer_tile_connect: the %s mailbox (rank %d) was exported for %s, this rank's for %s: %s", which, r, a, b,
                      s < TILE_S ? "the ranks of one row share ny, hy and what the mailboxes take" :
                                   "the ranks of one column, and fold partners, share nx + 2hx, hx and what the mailboxes take");
        } else {
            W.M.remote[s] = base[r];
            W.M.remote_side[s] = T.remote_side[s];
            W.M.remote_slot[s] = reinterpret_cast<double*>(base[r] + tile_slot_offset(theirs, T.remote_side[s]));
        }
    }
    if (rc != CF_OK) {
        disconnect_tiles(ctx);
        return rc;
    }
    W.place = T;
    W.tripolar = tripolar != 0;
    W.connected = true;
    ctx->rank = rank;
    ctx->nranks = px * py;
    return CF_OK;
}

int cf_halo_exchange_tile_peer(cf_ctx* ctx, double* const* d_fields, const int* locations, const double* signs, int nfields, int rows,
                               int fold_north) {
    const char* fn = "cf_halo_exchange_tile_peer";
    if (!ctx || !d_fields || nfields <= 0 || nfields > PEER_MAX_FIELDS) return fail(ctx, CF_ERR_INVALID, "%s: bad arguments (1…%d fields)", fn, PEER_MAX_FIELDS);
    if (fold_north && (!locations || !signs)) return fail(ctx, CF_ERR_INVALID, "%s: fold_north without locations or signs", fn);
    CHECK(check_tile_exchange(ctx, fn, nfields, rows, fold_north));
    FoldFields F{};
    F.n = nfields;
    for (int f = 0; f < nfields; ++f) {
        if (!d_fields[f]) return fail(ctx, CF_ERR_INVALID, "%s: field %d is NULL", fn, f);
        F.ptr[f] = d_fields[f];
        if (fold_north) {
            if (locations[f] < CF_FOLD_CENTER || locations[f] > CF_FOLD_Y_FACE) return fail(ctx, CF_ERR_INVALID, "%s: field %d has an unknown location", fn, f);
            F.location[f] = locations[f];
            F.sign[f] = signs[f];
        }
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return tile_exchange_launch(ctx, &F, rows, fold_north);
}

int cf_peer_tile_stats(cf_ctx* ctx, unsigned long long* exchanges, unsigned long long* column_launches, unsigned long long* folds_sent) {
    if (!ctx) return fail(nullptr, CF_ERR_INVALID, "ctx is NULL");
    if (exchanges) *exchanges = ctx->tile.seq;
    if (column_launches) *column_launches = ctx->tile.column_launches;
    if (folds_sent) *folds_sent = ctx->tile.folds_sent;
    return CF_OK;
}

}  // extern "C"
