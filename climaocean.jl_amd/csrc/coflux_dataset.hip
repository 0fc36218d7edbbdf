// coflux_dataset.hip — a dataset staged on the device and followed in time (cf_dataset_*, include/coflux.h; the host glue is
// coflux_dataset.cpp, the host rules coflux_dataset_rules.hpp): a plane of the dataset's own latitude–longitude grid is
// converted to f64, land-inpainted by nearest-neighbour sweeps and interpolated bilinearly onto one level of ocean-grid
// arrays; S★ at a time is one level or the linear blend of two.
//
// Inpainting [UPSTREAM-RECALL inpaint_mask!, NearestNeighborInpainting].  One sweep reads plane p and writes plane q: a cell
// that is not NaN is copied; a NaN cell takes the mean of its donors that are not NaN in p, added in the fixed order W, S, E, N
// starting from the first valid one and divided by their count (inpaint_cell: additions and one division, contraction off).
// The host knows the number of sweeps before the first launch, so nothing is counted or tested on the device.
//   Form one: one sweep per launch, one thread per cell, grid-strided.
//   Form two: h ≤ INPAINT_MAX_SWEEPS sweeps per launch on overlapped LDS tiles.  A workgroup holds INPAINT_LX × INPAINT_LY
//     cells twice; the tile's core, (LX − 2h) × (LY − 2h), is surrounded by h cells on each side, wrapped (periodic x) or cut
//     (absent cells: they never become donors) at the plane's edges.  The cells at the tile's rim lack the neighbours outside
//     the tile, so after sweep s the cells nearer than s to the rim are wrong and every other cell holds the plane's bits of
//     that sweep: after h sweeps the core is exact, and only the core is written back.  Launches are cut where the whole plane
//     has to meet (every h sweeps): p is read-only in a launch, q is written once per cell.
// Both forms call inpaint_cell with the same five values, so they give the same bits.
#include <algorithm>

#include "coflux_coupled_cells.hpp"
#include "coflux_kernel_types.hpp"
#include "coflux_kernels.h"

namespace coflux {

namespace {

constexpr int DATASET_BLOCK = 256;
constexpr int DATASET_MAX_BLOCKS = 2048;   // memory-bound passes: cap the grid and stride the rest
constexpr int INPAINT_LX = 64, INPAINT_LY = 32;
static_assert(INPAINT_LX - 2 * INPAINT_MAX_SWEEPS >= 16 && INPAINT_LY - 2 * INPAINT_MAX_SWEEPS >= 8, "a tile keeps a core");

__device__ __forceinline__ double inpaint_cell(double self, double w, double s, double e, double n) {
#pragma clang fp contract(off)
    if (!isnan(self)) return self;
    double sum = 0.0;
    int c = 0;
    if (!isnan(w)) {
        sum = w;
        c = 1;
    }
    if (!isnan(s)) {
        sum = c ? sum + s : s;
        ++c;
    }
    if (!isnan(e)) {
        sum = c ? sum + e : e;
        ++c;
    }
    if (!isnan(n)) {
        sum = c ? sum + n : n;
        ++c;
    }
    return c ? sum / (double)c : self;
}

__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

__global__ __launch_bounds__(DATASET_BLOCK) void dataset_convert_kernel(const float* __restrict__ in, double* __restrict__ out, unsigned n) {
    for (unsigned c = blockIdx.x * DATASET_BLOCK + threadIdx.x; c < n; c += gridDim.x * DATASET_BLOCK) out[c] = (double)in[c];
}

__global__ __launch_bounds__(DATASET_BLOCK) void dataset_default_kernel(double* __restrict__ plane, unsigned n, double fill) {
    for (unsigned c = blockIdx.x * DATASET_BLOCK + threadIdx.x; c < n; c += gridDim.x * DATASET_BLOCK)
        if (isnan(plane[c])) plane[c] = fill;
}

// form one
__global__ __launch_bounds__(DATASET_BLOCK) void inpaint_sweep_kernel(const double* __restrict__ p, double* __restrict__ q, int ns_x, int ns_y,
                                                                      int periodic) {
    const unsigned n = (unsigned)ns_x * (unsigned)ns_y;
    for (unsigned c = blockIdx.x * DATASET_BLOCK + threadIdx.x; c < n; c += gridDim.x * DATASET_BLOCK) {
        const int j = (int)(c / (unsigned)ns_x), i = (int)(c - (unsigned)j * (unsigned)ns_x);
        const double self = p[c];
        double out = self;
        if (isnan(self)) {
            const double nan = quiet_nan();
            const double w = i > 0 ? p[c - 1] : (periodic ? p[c + (unsigned)(ns_x - 1)] : nan);
            const double e = i + 1 < ns_x ? p[c + 1] : (periodic ? p[c - (unsigned)(ns_x - 1)] : nan);
            const double s = j > 0 ? p[c - (unsigned)ns_x] : nan;
            const double nn = j + 1 < ns_y ? p[c + (unsigned)ns_x] : nan;
            out = inpaint_cell(self, w, s, e, nn);
        }
        q[c] = out;
    }
}

// form two: h sweeps on tiles whose cores are cx × cy = (LX − 2h) × (LY − 2h); tiles are grid-strided
__global__ __launch_bounds__(DATASET_BLOCK) void inpaint_tiled_kernel(const double* __restrict__ p, double* __restrict__ q, int ns_x, int ns_y,
                                                                      int periodic, int h, int tiles_x, int tiles) {
    __shared__ double tile[2][INPAINT_LY][INPAINT_LX];
    constexpr int CELLS = INPAINT_LX * INPAINT_LY;
    const int cx = INPAINT_LX - 2 * h, cy = INPAINT_LY - 2 * h;
    const double nan = quiet_nan();
    for (int t = (int)blockIdx.x; t < tiles; t += (int)gridDim.x) {
        const int ty = t / tiles_x, tx = t - ty * tiles_x;
        const int x0 = tx * cx - h, y0 = ty * cy - h;   // plane coordinates of the tile's cell (0, 0)
        // load: a cell of the tile is a cell of the plane (x wrapped when periodic) or absent (NaN, and it stays NaN)
        for (int l = (int)threadIdx.x; l < CELLS; l += DATASET_BLOCK) {
            const int ly = l / INPAINT_LX, lx = l - ly * INPAINT_LX;
            int gx = x0 + lx;
            const int gy = y0 + ly;
            if (periodic) gx = wrap_index(gx, ns_x);
            const bool exists = gx >= 0 && gx < ns_x && gy >= 0 && gy < ns_y;
            tile[0][ly][lx] = exists ? p[(size_t)gy * (size_t)ns_x + (size_t)gx] : nan;
        }
        __syncthreads();
        int cur = 0;
        for (int s = 0; s < h; ++s) {
            for (int l = (int)threadIdx.x; l < CELLS; l += DATASET_BLOCK) {
                const int ly = l / INPAINT_LX, lx = l - ly * INPAINT_LX;
                const double self = tile[cur][ly][lx];
                double out = self;
                if (isnan(self)) {
                    const int gx = x0 + lx, gy = y0 + ly;
                    const bool exists = (periodic || (gx >= 0 && gx < ns_x)) && gy >= 0 && gy < ns_y;
                    if (exists) {
                        const double w = lx > 0 ? tile[cur][ly][lx - 1] : nan;
                        const double e = lx + 1 < INPAINT_LX ? tile[cur][ly][lx + 1] : nan;
                        const double so = ly > 0 ? tile[cur][ly - 1][lx] : nan;
                        const double no = ly + 1 < INPAINT_LY ? tile[cur][ly + 1][lx] : nan;
                        out = inpaint_cell(self, w, so, e, no);
                    }
                }
                tile[cur ^ 1][ly][lx] = out;
            }
            __syncthreads();
            cur ^= 1;
        }
        // the core goes back
        for (int l = (int)threadIdx.x; l < cx * cy; l += DATASET_BLOCK) {
            const int yy = l / cx, xx = l - yy * cx;
            const int gx = x0 + h + xx, gy = y0 + h + yy;
            if (gx < ns_x && gy < ns_y) q[(size_t)gy * (size_t)ns_x + (size_t)gx] = tile[cur][h + yy][h + xx];
        }
        __syncthreads();   // the next tile's load overwrites tile[0]
    }
}

// bilinear interpolation of the inpainted plane at cell (i, j) of the ring window: the index arithmetic of
// land_freshwater_cell (coflux_coupled_cells.hpp: periodic x, clamped y) on one f64 plane, no time blend
__device__ __forceinline__ double dataset_regrid_cell(const double* __restrict__ plane, int ns_x, int ns_y, const WeightDesc& Wt,
                                                      const GridDesc& G, int i, int j, size_t k) {
    const double fi = Wt.separable ? Wt.fi[i + G.hx] : Wt.fi[k];
    const double fj = Wt.separable ? Wt.fj[j + G.hy] : Wt.fj[k];
    const double xi = fi - floor(fi), eta = fj - floor(fj);
    const int i0 = (int)trunc(fi), ja = (int)trunc(fj);
    const int is0 = wrap_index(i0, ns_x), is1 = wrap_index(i0 + (fi > 0.0 ? 1 : (fi < 0.0 ? -1 : 0)), ns_x);
    const int j0 = min(max(ja, 0), ns_y - 1), j1 = min(max(ja + (fj > 0.0 ? 1 : (fj < 0.0 ? -1 : 0)), 0), ns_y - 1);
    const size_t g00 = (size_t)j0 * ns_x + is0, g10 = (size_t)j0 * ns_x + is1, g01 = (size_t)j1 * ns_x + is0, g11 = (size_t)j1 * ns_x + is1;
    const double w00 = (1.0 - xi) * (1.0 - eta), w01 = (1.0 - xi) * eta, w10 = xi * (1.0 - eta), w11 = xi * eta;
    return bilinear(w00, w01, w10, w11, plane[g00], plane[g01], plane[g10], plane[g11]);
}

__global__ __launch_bounds__(DATASET_BLOCK) void dataset_regrid_kernel(const double* __restrict__ plane, int ns_x, int ns_y, WeightDesc Wt,
                                                                       GridDesc G, double* __restrict__ out) {
    const int wx = G.nx + 2 * G.ring, wy = G.ny + 2 * G.ring;
    for (int idx = (int)(blockIdx.x * DATASET_BLOCK + threadIdx.x); idx < wx * wy; idx += (int)(gridDim.x * DATASET_BLOCK)) {
        const int jj = idx / wx;
        const int i = idx - jj * wx - G.ring, j = jj - G.ring;
        const size_t k = cell_index(G, i, j);
        out[k] = dataset_regrid_cell(plane, ns_x, ns_y, Wt, G, i, j, k);
    }
}

// S★ on the ring window W
__global__ __launch_bounds__(DATASET_BLOCK) void dataset_evaluate_kernel(const double* __restrict__ level1, const double* __restrict__ level2,
                                                                         double fraction, GridDesc G, double* __restrict__ out) {
    const int wx = G.nx + 2 * G.ring, wy = G.ny + 2 * G.ring;
    for (int idx = (int)(blockIdx.x * DATASET_BLOCK + threadIdx.x); idx < wx * wy; idx += (int)(gridDim.x * DATASET_BLOCK)) {
        const int jj = idx / wx;
        const size_t k = cell_index(G, idx - jj * wx - G.ring, jj - G.ring);
        const double target = dataset_target_cell(level1, level2, fraction, k);
        out[k] = target;
    }
}

// cf_materialize_dataset_restoring: salinity_restoring_kernel (coflux_net.hip) with S★ formed per cell from the two levels
__global__ __launch_bounds__(DATASET_BLOCK) void dataset_restoring_kernel(DevParams P, GridDesc G, const void* mask, double vp,
                                                                          const double* __restrict__ level1, const double* __restrict__ level2,
                                                                          double fraction, const double* __restrict__ S, double* __restrict__ out) {
    const int idx = (int)blockIdx.x * DATASET_BLOCK + (int)threadIdx.x;
    if (idx >= G.nx * G.ny) return;
    const int j = idx / G.nx;
    const size_t k = cell_index(G, idx - j * G.nx, j);
    const bool wet = cell_is_wet(P, mask, k);
    out[k] = salinity_restoring_cell(wet, vp, wet ? S[k] : 0.0, level1, level2, fraction, k);
}

int capped_blocks(size_t items, int max_blocks) {
    const size_t want = (items + DATASET_BLOCK - 1) / DATASET_BLOCK;
    const size_t cap = (size_t)(max_blocks > 0 ? max_blocks : DATASET_MAX_BLOCKS);
    return (int)std::max<size_t>(1, std::min(want, cap));
}

}  // namespace

hipError_t launch_dataset_convert(hipStream_t st, const float* in, double* out, size_t n, int max_blocks) {
    hipLaunchKernelGGL(dataset_convert_kernel, dim3(capped_blocks(n, max_blocks)), dim3(DATASET_BLOCK), 0, st, in, out, (unsigned)n);
    return hipGetLastError();
}

hipError_t launch_dataset_default(hipStream_t st, double* plane, size_t n, double fill, int max_blocks) {
    hipLaunchKernelGGL(dataset_default_kernel, dim3(capped_blocks(n, max_blocks)), dim3(DATASET_BLOCK), 0, st, plane, (unsigned)n, fill);
    return hipGetLastError();
}

hipError_t launch_dataset_inpaint(hipStream_t st, const double* p, double* q, int ns_x, int ns_y, bool periodic, int sweeps, int max_blocks) {
    if (sweeps < 1 || sweeps > INPAINT_MAX_SWEEPS) return hipErrorInvalidValue;
    if (sweeps == 1) {
        hipLaunchKernelGGL(inpaint_sweep_kernel, dim3(capped_blocks((size_t)ns_x * (size_t)ns_y, max_blocks)), dim3(DATASET_BLOCK), 0, st, p, q,
                           ns_x, ns_y, periodic ? 1 : 0);
        return hipGetLastError();
    }
    const int cx = INPAINT_LX - 2 * sweeps, cy = INPAINT_LY - 2 * sweeps;
    const int tiles_x = (ns_x + cx - 1) / cx, tiles = tiles_x * ((ns_y + cy - 1) / cy);
    const int blocks = std::max(1, std::min(tiles, max_blocks > 0 ? max_blocks : DATASET_MAX_BLOCKS));
    hipLaunchKernelGGL(inpaint_tiled_kernel, dim3(blocks), dim3(DATASET_BLOCK), 0, st, p, q, ns_x, ns_y, periodic ? 1 : 0, sweeps, tiles_x, tiles);
    return hipGetLastError();
}

hipError_t launch_dataset_regrid(hipStream_t st, const double* plane, int ns_x, int ns_y, const cf_interp_weights* w, const GridDesc& G,
                                 double* out, int max_blocks) {
    const size_t n = (size_t)(G.nx + 2 * G.ring) * (size_t)(G.ny + 2 * G.ring);
    hipLaunchKernelGGL(dataset_regrid_kernel, dim3(capped_blocks(n, max_blocks)), dim3(DATASET_BLOCK), 0, st, plane, ns_x, ns_y, make_weights(w), G, out);
    return hipGetLastError();
}

hipError_t launch_dataset_evaluate(hipStream_t st, const double* level1, const double* level2, double fraction, const GridDesc& G, double* out,
                                   int max_blocks) {
    const size_t n = (size_t)(G.nx + 2 * G.ring) * (size_t)(G.ny + 2 * G.ring);
    hipLaunchKernelGGL(dataset_evaluate_kernel, dim3(capped_blocks(n, max_blocks)), dim3(DATASET_BLOCK), 0, st, level1, level2, fraction, G, out);
    return hipGetLastError();
}

hipError_t launch_dataset_restoring(hipStream_t st, const DevParams& P, const GridDesc& G, const void* mask, double vp, const double* level1,
                                    const double* level2, double fraction, const double* S, double* out) {
    const int ncells = G.nx * G.ny;
    hipLaunchKernelGGL(dataset_restoring_kernel, dim3((ncells + DATASET_BLOCK - 1) / DATASET_BLOCK), dim3(DATASET_BLOCK), 0, st, P, G, mask, vp,
                       level1, level2, fraction, S, out);
    return hipGetLastError();
}

}  // namespace coflux
