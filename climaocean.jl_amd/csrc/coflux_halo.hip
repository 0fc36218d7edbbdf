// coflux_halo.hip — halo rows of the latitude-slab decomposition without a collective library, and the
// tripolar fold (include/coflux.h: cf_peer_halo_*, cf_fold_north_halo).
//
// Peer-direct exchange.  At ≤ 93 KB per neighbour and step the exchange is pure latency, so it is ONE launch:
// two workgroups (one per direction) each (i) store this rank's boundary rows straight into the neighbour's
// mailbox — fine-grained device memory mapped through HIP IPC, i.e. plain stores that travel over xGMI —,
// (ii) publish the step's sequence number with a system-scope release, (iii) wait for the neighbour's number in
// the own mailbox (one lane polls, bounded, sleeping between polls) and (iv) copy the received rows into the halo
// rows.  No host round trip, no second launch, nothing for the solver to wait on except stream order.  The steps themselves are
// peer_halo_side (coflux_halo_device.hpp).  On the rank that owns the tripolar fold the coupled loop launches the form whose north
// side folds the exchange's own fields instead (peer_halo_fold_kernel).
#include <hip/hip_runtime.h>

#include "coflux_halo_device.hpp"
#include "coflux_kernel_types.hpp"
#include "coflux_kernels.h"

namespace coflux {

__global__ __launch_bounds__(PEER_BLOCK) void peer_halo_kernel(PeerMailbox M, PeerFields F, GridDesc G, int rows,
                                                               unsigned long long seq, int* __restrict__ status) {
    __shared__ int ok;
    peer_halo_side(M, F.ptr, F.n, G, rows, seq, status, (int)blockIdx.x, &ok);  // workgroup 0: south neighbour, 1: north neighbour
}

// The exchange launch of the rank that owns the tripolar fold (cf_time_steps_coupled under CF_HALO_PEER with fold_north): that
// rank has no north neighbour, and the north halo rows of the exchange's own fields are the fold of its own interior rows.
// Workgroup 0 is the south exchange, the protocol of peer_halo_kernel unchanged; workgroup 1 + f · rows + (r − 1) folds north
// halo row ny − 1 + r of field f with the field's own location and sign — cf_fold_north_halo's arithmetic, bit for bit.
// The two sides need no ordering: check_fold_geometry admits rows ≤ ny − 1, so the fold reads only the interior rows
// ny − 1 − rows … ny − 1 and writes only north halo rows, while the south side reads the interior rows 0 … rows − 1 and writes
// only south halo rows; no cell one side writes is touched by the other, and neither side writes a cell the fold reads.
__global__ __launch_bounds__(PEER_BLOCK) void peer_halo_fold_kernel(PeerMailbox M, FoldFields F, GridDesc G, int rows,
                                                                    unsigned long long seq, int* __restrict__ status) {
    __shared__ int ok;
    if (blockIdx.x == 0) {
        peer_halo_side(M, F.ptr, F.n, G, rows, seq, status, 0, &ok);
        return;
    }
    const int h = (int)blockIdx.x - 1, f = h / rows, r = h - f * rows + 1;  // (uniform: the field's entry is read with scalar loads)
    fold_north_row(F.ptr[f], G, F.location[f], F.sign[f], r, PEER_BLOCK);
}

hipError_t launch_peer_halo(hipStream_t st, const PeerMailbox& M, const PeerFields& F, const GridDesc& G, int rows,
                            unsigned long long seq, int* d_status) {
    hipLaunchKernelGGL(peer_halo_kernel, dim3(2), dim3(PEER_BLOCK), 0, st, M, F, G, rows, seq, d_status);
    return hipGetLastError();
}

hipError_t launch_peer_halo_fold(hipStream_t st, const PeerMailbox& M, const FoldFields& F, const GridDesc& G, int rows,
                                 unsigned long long seq, int* d_status) {
    hipLaunchKernelGGL(peer_halo_fold_kernel, dim3(1 + F.n * rows), dim3(PEER_BLOCK), 0, st, M, F, G, rows, seq, d_status);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// The tile world (include/coflux.h: cf_peer_tile_*): two launches per exchange on the context's stream, the columns first.  The
// y-phase sends its rows full width, x-halos included, and the fold a north side sends reads this rank's east halo column:
// both need the columns the x-phase delivers, and stream order is all that orders them.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PEER_BLOCK) void tile_halo_x_kernel(TileMailbox M, PeerFields F, GridDesc G, int wcols, int ecols,
                                                                 unsigned long long seq, int* __restrict__ status) {
    __shared__ int ok;
    tile_halo_x_side(M, F.ptr, F.n, G, wcols, ecols, seq, status, TILE_W + (int)blockIdx.x, &ok);  // workgroup 0: west, 1: east
}

__global__ __launch_bounds__(PEER_BLOCK) void tile_halo_y_kernel(TileMailbox M, FoldFields F, GridDesc G, int rows, TileFold fold,
                                                                 unsigned long long seq, int* __restrict__ status) {
    __shared__ int ok;
    tile_halo_y_side(M, F, G, rows, fold, seq, status, TILE_S + (int)blockIdx.x, &ok);  // workgroup 0: south, 1: north or the fold partner
}

hipError_t launch_tile_halo_x(hipStream_t st, const TileMailbox& M, const PeerFields& F, const GridDesc& G, int wcols, int ecols,
                              unsigned long long seq, int* d_status) {
    hipLaunchKernelGGL(tile_halo_x_kernel, dim3(2), dim3(PEER_BLOCK), 0, st, M, F, G, wcols, ecols, seq, d_status);
    return hipGetLastError();
}

hipError_t launch_tile_halo_y(hipStream_t st, const TileMailbox& M, const FoldFields& F, const GridDesc& G, int rows, const TileFold& fold,
                              unsigned long long seq, int* d_status) {
    hipLaunchKernelGGL(tile_halo_y_kernel, dim3(2), dim3(PEER_BLOCK), 0, st, M, F, G, rows, fold, seq, d_status);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Tripolar fold: the north halo rows of the last slab from its own mirrored interior rows
// (include/coflux.h: cf_fold_north_halo; Oceananigans zipper boundary condition, UPSTREAM-RECALL).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fold_north_kernel(FoldFields F, GridDesc G, int rows) {
    const int f = (int)blockIdx.y;
    const int width = G.nx + 2 * G.hx;
    const int n = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (n >= width * rows) return;
    const int r = n / width + 1;        // halo row ny − 1 + r
    const int i = n - (r - 1) * width - G.hx;  // interior-relative column, x-halos included
    int ip = i % G.nx;                  // periodic image inside [0, nx)
    if (ip < 0) ip += G.nx;
    double* p = F.ptr[f];
    p[cell_index(G, i, G.ny - 1 + r)] = fold_north_value(p, G, F.location[f], F.sign[f], ip, r);
}

hipError_t launch_fold_north(hipStream_t st, const FoldFields& F, const GridDesc& G, int rows) {
    const int n = (G.nx + 2 * G.hx) * rows;
    hipLaunchKernelGGL(fold_north_kernel, dim3((n + 255) / 256, F.n), dim3(256), 0, st, F, G, rows);
    return hipGetLastError();
}

}  // namespace coflux
