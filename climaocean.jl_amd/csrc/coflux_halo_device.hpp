// coflux_halo_device.hpp — the device side of the peer-direct halo rows (include/coflux.h: cf_peer_halo_*), shared by the
// stand-alone exchange kernels (coflux_halo.hip) and by the rider workgroups of the solver launch (coflux_lean_kernel.hpp, HALO),
// and the tripolar fold's per-element map, shared by the fold's own kernel and by the exchange whose north side folds.
#pragma once
#include <hip/hip_runtime.h>

#include "coflux_kernel_types.hpp"

namespace coflux {

// the waiting lane gives up after this many polls (s_sleep 8 ≈ 512 clocks + the load ≈ 1.3 µs each): ≈ 5 s
constexpr unsigned long long PEER_SPIN_LIMIT = 4ull * 1000 * 1000;

__device__ __forceinline__ double* mailbox_rows(const PeerMailbox& M, char* base, int side, int parity) {
    return reinterpret_cast<double*>(base + M.data_offset) + ((size_t)(side * 2 + parity)) * M.slot_doubles;
}
__device__ __forceinline__ unsigned long long* mailbox_flag(char* base, int side, int parity) {
    return reinterpret_cast<unsigned long long*>(base) + (side * 2 + parity) * 8;  // one flag per 64-byte line
}

// Steps (ii) and (iii) of one side of an exchange (below), and the acquire in front of (iv), run by the whole workgroup: true when
// the neighbour's rows of step `seq` have arrived.  A wait that exceeds its bound sets the sticky status to `code`, which names
// the side (cf_sync: 1 south, 2 north; of a tile world also 4 west, 5 east, 6 the fold partner).
__device__ __forceinline__ bool peer_publish_and_wait(unsigned long long* remote_flag, unsigned long long* my_flag, unsigned long long seq,
                                                      int* __restrict__ status, int code, int* lds_ok) {
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) {
        __hip_atomic_store(remote_flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        unsigned long long spins = 0;
        int good = 1;
        while (__hip_atomic_load(my_flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) < seq) {
            __builtin_amdgcn_s_sleep(8);
            if (++spins > PEER_SPIN_LIMIT) {
                good = 0;
                break;
            }
        }
        *lds_ok = good;
        if (!good) atomicExch(status, code);  // sticky: reported by the next cf_sync
    }
    __syncthreads();
    if (!*lds_ok) return false;
    __atomic_thread_fence(__ATOMIC_ACQUIRE);  // system scope: nothing cached of the mailbox survives the flag
    return true;
}

// One direction of the stand-alone exchange, run by ONE workgroup of PEER_BLOCK lanes (coflux_halo.hip: peer_halo_kernel's two
// workgroups, and workgroup 0 of peer_halo_fold_kernel): dir 0 exchanges with the south neighbour, 1 with the north.
//   (i)   my boundary rows of every field → the neighbour's mailbox; seen from THERE they arrive from the opposite side;
//   (ii)  publish the step's sequence number: every lane's stores are visible system-wide before the flag is;
//   (iii) wait for the neighbour's rows of the same step (one lane polls, bounded, sleeping between polls);
//   (iv)  mailbox → my halo rows.  A wait that exceeds its bound sets the sticky status and copies nothing.
__device__ __forceinline__ void peer_halo_side(const PeerMailbox& M, double* const* fields, int nfields, const GridDesc& G, int rows,
                                               unsigned long long seq, int* __restrict__ status, int dir, int* lds_ok) {
    char* remote = dir == 0 ? M.south : M.north;
    if (!remote) return;  // end of the slab ring (or a fold): nothing to exchange in this direction
    const int parity = (int)(seq & 1ull);
    const size_t row_doubles = (size_t)G.sj, per_field = (size_t)rows * row_doubles;
    {
        double* dst = mailbox_rows(M, remote, 1 - dir, parity);
        const size_t first_row = dir == 0 ? (size_t)G.hy : (size_t)(G.hy + G.ny - rows);
        for (int f = 0; f < nfields; ++f) {
            const double* src = fields[f] + first_row * row_doubles;
            for (size_t n = threadIdx.x; n < per_field; n += PEER_BLOCK) dst[(size_t)f * per_field + n] = src[n];
        }
    }
    if (!peer_publish_and_wait(mailbox_flag(remote, 1 - dir, parity), mailbox_flag(M.mine, dir, parity), seq, status, 1 + dir, lds_ok)) return;
    {
        const double* src = mailbox_rows(M, M.mine, dir, parity);
        const size_t first_row = dir == 0 ? (size_t)(G.hy - rows) : (size_t)(G.hy + G.ny);
        for (int f = 0; f < nfields; ++f) {
            double* dst = fields[f] + first_row * row_doubles;
            for (size_t n = threadIdx.x; n < per_field; n += PEER_BLOCK) dst[n] = src[(size_t)f * per_field + n];
        }
    }
}

// The tripolar fold's per-element map (include/coflux.h: cf_fold_north_halo), the one device statement of it: where the value of
// north halo row ny − 1 + r (r ≥ 1) at column i comes from, for a field at `location` with `sign`, on a mirror `nx` columns wide.
// `on_axis`: the column's global periodic image is 0 — the x-face on the fold axis maps onto itself and keeps |sign|.  Columns
// are relative to whoever holds the source: the single domain passes a periodic image and wraps the answer (fold_north_value),
// a tile passes its partner's column and reads its own halo columns where the answer leaves its interior (tile_halo_y_side).
struct FoldSource {
    int is, js;
    double sign;
};
__device__ __forceinline__ FoldSource fold_north_source(int nx, int ny, int location, double sign, int i, bool on_axis, int r) {
    if (location == CF_FOLD_X_FACE) return FoldSource{nx - i, ny - 1 - r, on_axis ? fabs(sign) : sign};
    if (location == CF_FOLD_Y_FACE) return FoldSource{nx - 1 - i, ny - r, sign};
    return FoldSource{nx - 1 - i, ny - 1 - r, sign};
}

// The fold on one rank's own rows: `ip` is the column's periodic image inside [0, nx).  The product sign · value is formed as
// written: −1 · 0.0 stays −0.0.
__device__ __forceinline__ double fold_north_value(const double* p, const GridDesc& G, int location, double sign, int ip, int r) {
    FoldSource S = fold_north_source(G.nx, G.ny, location, sign, ip, ip == 0, r);
    if (S.is >= G.nx) S.is -= G.nx;  // the face on the fold axis
    return S.sign * p[cell_index(G, S.is, S.js)];
}

// One north halo row of one field, full width nx + 2hx, by one workgroup: the lanes stride over the written columns in ascending
// order (the stores of a wave are one contiguous run; its loads are one contiguous run too, walked downwards — the same cache lines
// as an ascending wave touches, each once).  The periodic image comes from at most a few additions per column, not a division.
__device__ __forceinline__ void fold_north_row(double* p, const GridDesc& G, int location, double sign, int r, int nthreads) {
    const int width = G.nx + 2 * G.hx;
    for (int c = (int)threadIdx.x; c < width; c += nthreads) {
        const int i = c - G.hx;  // interior-relative column, x-halos included
        int ip = i;
        while (ip < 0) ip += G.nx;
        while (ip >= G.nx) ip -= G.nx;
        p[cell_index(G, i, G.ny - 1 + r)] = fold_north_value(p, G, location, sign, ip, r);
    }
}

// ---- the tile world (include/coflux.h: cf_peer_tile_*) ----------------------------------------------------------------------

// One side of the x-phase, run by ONE workgroup of PEER_BLOCK lanes: side TILE_W exchanges with the west neighbour, TILE_E with
// the east.  peer_halo_side's protocol with columns for rows: my boundary columns of every field, interior rows 0 … ny − 1, go
// into the neighbour's slot as [field][column][row] — consecutive lanes take consecutive rows of one column, so a wave's remote
// stores are one contiguous run and the stride sj is paid by its local loads —, publish, wait, and the received columns go
// into my x-halo columns.  The west halo takes `wcols` columns, the east halo `ecols` (coflux_tile_geometry.hpp).
__device__ __forceinline__ void tile_halo_x_side(const TileMailbox& M, double* const* fields, int nfields, const GridDesc& G, int wcols,
                                                 int ecols, unsigned long long seq, int* __restrict__ status, int side, int* lds_ok) {
    char* remote = M.remote[side];
    if (!remote) return;
    const int parity = (int)(seq & 1ull);
    const int send_cols = side == TILE_W ? ecols : wcols, recv_cols = side == TILE_W ? wcols : ecols;   // my west columns fill an EAST halo
    const int first_send = side == TILE_W ? 0 : G.nx - send_cols, first_recv = side == TILE_W ? -recv_cols : G.nx;
    {
        double* dst = M.remote_slot[side] + (size_t)parity * M.x_slot;
        const int per_field = send_cols * G.ny;
        for (int f = 0; f < nfields; ++f) {
            const double* src = fields[f];
            for (int n = (int)threadIdx.x; n < per_field; n += PEER_BLOCK) {
                const int c = n / G.ny, j = n - c * G.ny;
                dst[(size_t)f * per_field + n] = src[cell_index(G, first_send + c, j)];
            }
        }
    }
    if (!peer_publish_and_wait(mailbox_flag(remote, M.remote_side[side], parity), mailbox_flag(M.mine, side, parity), seq, status, 4 + side, lds_ok))
        return;
    {
        const double* src = M.my_slot[side] + (size_t)parity * M.x_slot;
        const int per_field = recv_cols * G.ny;
        for (int f = 0; f < nfields; ++f) {
            double* dst = fields[f];
            for (int n = (int)threadIdx.x; n < per_field; n += PEER_BLOCK) {
                const int c = n / G.ny, j = n - c * G.ny;
                dst[cell_index(G, first_recv + c, j)] = src[(size_t)f * per_field + n];
            }
        }
    }
}

// One side of the y-phase, by one workgroup: side TILE_S or TILE_N.  The rows travel full width nx + 2hx exactly as in
// peer_halo_side — the x-phase has filled the sender's x-halos, so the corners arrive without a diagonal message.  Where the north
// side is the fold partner (fold.cols > 0) the SENDER writes the partner's north halo rows already mirrored and signed, over the
// partner's columns −cols … nx − 1 + cols, and both copy in exactly those columns: fold_north_source with the partner's column
// as the mirror's argument — sender column nx − 1 − i (centres, y-faces) or nx − i (x-faces: up to this rank's east halo column
// nx + cols, which is why the x-phase comes first and fills one more east column here).
__device__ __forceinline__ void tile_halo_y_side(const TileMailbox& M, const FoldFields& F, const GridDesc& G, int rows, const TileFold& fold,
                                                 unsigned long long seq, int* __restrict__ status, int side, int* lds_ok) {
    char* remote = M.remote[side];
    if (!remote) return;
    const int parity = (int)(seq & 1ull), dir = side - TILE_S;   // 0: south, 1: north
    const bool folds = dir == 1 && fold.cols > 0;
    const size_t row_doubles = (size_t)G.sj, per_field = (size_t)rows * row_doubles;
    const int width = G.nx + 2 * fold.cols, folded = rows * width;
    {
        double* dst = M.remote_slot[side] + (size_t)parity * M.y_slot;
        const size_t first_row = dir == 0 ? (size_t)G.hy : (size_t)(G.hy + G.ny - rows);
        for (int f = 0; f < F.n; ++f) {
            if (folds) {
                const double* p = F.ptr[f];
                for (int n = (int)threadIdx.x; n < folded; n += PEER_BLOCK) {
                    const int r = n / width + 1, i = n - (r - 1) * width - fold.cols;   // the partner's halo row ny − 1 + r, its column i
                    const int g = fold.g0 + i;
                    const FoldSource S = fold_north_source(G.nx, G.ny, F.location[f], F.sign[f], i, g == 0 || g == fold.Nx, r);
                    dst[(size_t)f * per_field + (size_t)(r - 1) * row_doubles + (size_t)(i + G.hx)] = S.sign * p[cell_index(G, S.is, S.js)];
                }
            } else {
                const double* src = F.ptr[f] + first_row * row_doubles;
                for (size_t n = threadIdx.x; n < per_field; n += PEER_BLOCK) dst[(size_t)f * per_field + n] = src[n];
            }
        }
    }
    if (!peer_publish_and_wait(mailbox_flag(remote, M.remote_side[side], parity), mailbox_flag(M.mine, side, parity), seq, status,
                               folds ? 6 : 1 + dir, lds_ok))
        return;
    {
        const double* src = M.my_slot[side] + (size_t)parity * M.y_slot;
        const size_t first_row = dir == 0 ? (size_t)(G.hy - rows) : (size_t)(G.hy + G.ny);
        for (int f = 0; f < F.n; ++f) {
            double* dst = F.ptr[f] + first_row * row_doubles;
            if (folds) {
                for (int n = (int)threadIdx.x; n < folded; n += PEER_BLOCK) {
                    const int r = n / width, c = n - r * width - fold.cols + G.hx;
                    dst[(size_t)r * row_doubles + c] = src[(size_t)f * per_field + (size_t)r * row_doubles + c];
                }
            } else {
                for (size_t n = threadIdx.x; n < per_field; n += PEER_BLOCK) dst[n] = src[(size_t)f * per_field + n];
            }
        }
    }
}

// One rider workgroup of a solver launch: direction dir = h / F.n (0: south neighbour, 1: north), field f = h mod F.n.
//   (i)   my boundary rows of field f → the neighbour's mailbox (plain stores over xGMI), system-scope fence;
//   (ii)  count myself into counters[dir]; the workgroup that completes the direction's count publishes the step's sequence
//         number in the neighbour's mailbox (system-scope release: every field's rows are visible before the flag);
//   (iii) wait (one lane, bounded, sleeping) for the neighbour's number in my own mailbox;
//   (iv)  its rows of field f → my halo rows; agent-scope release of counters[2 + dir], which the solver workgroups that read
//         those rows wait for (ao_lean_body).  On a timeout the sticky status is set and the counter is released all the same:
//         the launch ends, the next cf_sync reports CF_ERR_COMM.
// Same mailbox protocol, same data movement as peer_halo_kernel — the rows that arrive are the same bits.
// (The rider's arguments arrive as scalars: the caller reads them from the kernel-argument block with uniform indices — a
// by-value HaloRider indexed by `f` would live in scratch.)
__device__ __forceinline__ void peer_halo_rider(const PeerMailbox& M, double* field, int f, int dir, int rows, unsigned long long seq,
                                                unsigned long long* counters, unsigned long long expect_sent, int* status,
                                                const GridDesc& G, int nthreads, int* lds_ok) {
    char* remote = dir == 0 ? M.south : M.north;
    if (!remote) return;  // end of the slab ring (or the fold): nothing to exchange, nobody waits
    const int parity = (int)(seq & 1ull), tid = (int)threadIdx.x;
    const size_t row_doubles = (size_t)G.sj, per_field = (size_t)rows * row_doubles;
    {
        double* dst = mailbox_rows(M, remote, 1 - dir, parity) + (size_t)f * per_field;
        const size_t first_row = dir == 0 ? (size_t)G.hy : (size_t)(G.hy + G.ny - rows);
        const double* src = field + first_row * row_doubles;
        for (size_t n = tid; n < per_field; n += nthreads) dst[n] = src[n];
    }
    __threadfence_system();
    __syncthreads();
    if (tid == 0) {
        const unsigned long long before = __hip_atomic_fetch_add(&counters[dir], 1ull, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (before + 1ull == expect_sent)
            __hip_atomic_store(mailbox_flag(remote, 1 - dir, parity), seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        unsigned long long* flag = mailbox_flag(M.mine, dir, parity);
        unsigned long long spins = 0;
        int good = 1;
        while (__hip_atomic_load(flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) < seq) {
            __builtin_amdgcn_s_sleep(8);
            if (++spins > PEER_SPIN_LIMIT) {
                good = 0;
                break;
            }
        }
        *lds_ok = good;
        if (!good) atomicExch(status, 1 + dir);  // sticky: reported by the next cf_sync
    }
    __syncthreads();
    if (*lds_ok) {
        __atomic_thread_fence(__ATOMIC_ACQUIRE);  // system scope: nothing cached of the mailbox survives the flag
        const double* src = mailbox_rows(M, M.mine, dir, parity) + (size_t)f * per_field;
        const size_t first_row = dir == 0 ? (size_t)(G.hy - rows) : (size_t)(G.hy + G.ny);
        double* dst = field + first_row * row_doubles;
        for (size_t n = tid; n < per_field; n += nthreads) dst[n] = src[n];
    }
    __threadfence();
    __syncthreads();
    if (tid == 0) __hip_atomic_fetch_add(&counters[2 + dir], 1ull, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}

// A solver workgroup whose cells read halo rows waits here (every wave; lane 0 polls, the wave re-converges behind it) until the
// riders have copied them in.  Bounded like the riders' own wait, plus their bound: a rider that timed out still releases.
__device__ __forceinline__ void peer_halo_wait(const unsigned long long* counter, unsigned long long expect) {
    if ((threadIdx.x & 63) == 0) {
        unsigned long long spins = 0;
        while (__hip_atomic_load(counter, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) < expect) {
            __builtin_amdgcn_s_sleep(4);
            if (++spins > 4ull * PEER_SPIN_LIMIT) break;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");  // (every lane: the rows the riders wrote, not what this CU may have cached of them)
}

}  // namespace coflux
