// coflux_tile_geometry.hpp — the host arithmetic of the tile world (include/coflux.h: cf_peer_tile_*), plain C++ without a HIP
// call: the rank's place in the px × py world, its neighbours and fold partner, what a tile mailbox was exported for and where
// its slots lie.  coflux_tiles.cpp builds the exchange from these; tests/tile_geometry_driver.cpp runs them alone under the
// sanitizers.
//
// The world: rank = p + px · q, x fastest.  Rank (p, q) owns columns [p · nxl, (p + 1) · nxl) and one block of rows.  x is
// periodic, y is not.  On the top row (q = py − 1) of a tripolar world the north side is the fold partner (px − 1 − p, py − 1).
#pragma once
#include <cstddef>
#include <cstdio>

namespace coflux {

constexpr int TILE_W = 0, TILE_E = 1, TILE_S = 2, TILE_N = 3;
constexpr int TILE_MAX_RANKS = 8;                      // CF_PEER_REDUCE_MAX_RANKS: the worlds the exact mean takes
constexpr size_t TILE_NOTE_OFFSET = 8 * 64;            // behind the eight flag lines [side][parity]
constexpr size_t TILE_DATA_OFFSET = TILE_NOTE_OFFSET + 64;
constexpr unsigned long long TILE_MAGIC = 0x636f666c7578746cull;  // "cofluxtl"

// what a tile mailbox was exported for; it lies in the mailbox, on a line of its own
struct TileNote {
    unsigned long long magic;
    int max_fields, max_rows, max_cols, sj, ny, hx, hy, pad;
};
static_assert(sizeof(TileNote) <= 64, "the note stays inside its own line");

// doubles per (side, parity) slot: the columns of W and E cover the interior rows, the rows of S and N the full width
inline size_t tile_x_slot(const TileNote& n) { return (size_t)n.max_fields * (size_t)n.max_cols * (size_t)n.ny; }
inline size_t tile_y_slot(const TileNote& n) { return (size_t)n.max_fields * (size_t)n.max_rows * (size_t)n.sj; }
inline size_t tile_mailbox_bytes(const TileNote& n) { return TILE_DATA_OFFSET + 4 * (tile_x_slot(n) + tile_y_slot(n)) * sizeof(double); }
// bytes from the mailbox base to parity 0 of `side`'s slot: [W][E] pairs of x slots, then [S][N] pairs of y slots
inline size_t tile_slot_offset(const TileNote& n, int side) {
    const size_t doubles = side < TILE_S ? (size_t)side * 2 * tile_x_slot(n) : 4 * tile_x_slot(n) + (size_t)(side - TILE_S) * 2 * tile_y_slot(n);
    return TILE_DATA_OFFSET + doubles * sizeof(double);
}

struct TilePlace {
    int px, py, p, q;
    int neighbour[4];    // rank on each side, −1: nobody (the ends of y; every x side when px = 1: the x-halos stay the caller's)
    int remote_side[4];  // the side of that rank's mailbox this rank's side writes
    bool top_row;        // q = py − 1
    bool partner_north;  // the north side is the fold partner (top row of a tripolar world, px > 1)
};

// "" when (px, py, rank, tripolar) on tiles `nxl` columns wide is a world this library steps, else why not
inline bool tile_world_refusal(int px, int py, int rank, int tripolar, int nxl, char* why, size_t n) {
    why[0] = 0;
    if (px < 1 || py < 1 || (long long)px * py > TILE_MAX_RANKS)
        std::snprintf(why, n, "px = %d, py = %d: a world of 1 … %d ranks", px, py, TILE_MAX_RANKS);
    else if (rank < 0 || rank >= px * py)
        std::snprintf(why, n, "rank = %d outside the %d x %d world", rank, px, py);
    else if (px > 1 && px % 2)
        std::snprintf(why, n, "px = %d: 1 or even (with an odd px the middle rank would be its own fold partner for half a tile)", px);
    else if (tripolar && ((long long)px * nxl) % 2)
        std::snprintf(why, n, "tripolar with an odd global Nx = px · nx = %d · %d", px, nxl);
    return why[0] != 0;
}

inline TilePlace tile_place(int px, int py, int rank, int tripolar) {
    TilePlace T{};
    T.px = px;
    T.py = py;
    T.p = rank % px;
    T.q = rank / px;
    T.top_row = T.q == py - 1;
    T.partner_north = T.top_row && tripolar && px > 1;
    T.neighbour[TILE_W] = px > 1 ? (T.p + px - 1) % px + px * T.q : -1;
    T.neighbour[TILE_E] = px > 1 ? (T.p + 1) % px + px * T.q : -1;
    T.neighbour[TILE_S] = T.q > 0 ? T.p + px * (T.q - 1) : -1;
    T.neighbour[TILE_N] = T.partner_north ? (px - 1 - T.p) + px * T.q : T.top_row ? -1 : T.p + px * (T.q + 1);
    T.remote_side[TILE_W] = TILE_E;
    T.remote_side[TILE_E] = TILE_W;
    T.remote_side[TILE_S] = TILE_N;
    T.remote_side[TILE_N] = T.partner_north ? TILE_N : TILE_S;   // partners write each other's north slots
    return T;
}

// W and E neighbours share this rank's rows, S, N and the partner its columns; all share what the mailboxes take
inline bool tile_notes_agree(const TileNote& mine, const TileNote& theirs, int side) {
    if (theirs.max_fields != mine.max_fields || theirs.max_rows != mine.max_rows || theirs.max_cols != mine.max_cols) return false;
    return side < TILE_S ? theirs.ny == mine.ny && theirs.hy == mine.hy : theirs.sj == mine.sj && theirs.hx == mine.hx;
}

inline void tile_note_text(const TileNote& n, char* out, size_t len) {
    std::snprintf(out, len, "(max_fields, max_rows, max_cols, nx + 2hx, ny, hx, hy) = (%d, %d, %d, %d, %d, %d, %d)", n.max_fields, n.max_rows,
                  n.max_cols, n.sj, n.ny, n.hx, n.hy);
}

// columns the x-phase fills: `west` in the west halo, `east` in the east halo.  Where the north side sends a fold the x-face map
// reads sender column nx − i for receiver columns i ≥ −(ring + 1): one east column more than the step's kernels read themselves.
inline void tile_phase_columns(int ring, bool sends_fold, int* west, int* east) {
    *west = ring + 1;
    *east = ring + 1 + (sends_fold ? 1 : 0);
}

}  // namespace coflux
