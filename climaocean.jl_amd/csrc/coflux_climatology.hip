// coflux_climatology.hip — calendar-binned means of surface fields accumulated on the device and their per-cell extremes
// over the bins (cf_climatology_*, include/coflux.h; the host glue is coflux_climatology.cpp).
//
// Collection.  One launch per collection and the geometry of average_kernel (coflux_average.hip): blockIdx.y is the field, x
// grid-strides over (row j, slot s) of the interior, CLIMATOLOGY_UNROLL slots per thread and trip.  The source of a cell is
// loaded once and enters two running means, the total's and one bin's, each by `blend` of coflux_surface_cells.hpp (two
// products and a sum, each rounded) with its own coefficients, or stored without reading where that destination sees its first
// sample.  Store or accumulate is a template parameter per destination: four instantiations, nothing decided per cell.  A
// field without a total (its pointer is NULL) skips that destination: uniform per workgroup.
// Slot s of row j covers the elements e = 2s − h, e + 1, h = 1 when the BIN's row starts 8 but not 16 bytes into a 16-byte
// line: the bin is accessed 16 bytes at a time wherever the pair lies inside the interior, the source and the total are where
// their row shares that offset, and by 8-byte accesses otherwise (the peel at either end of a row, an array of the other
// alignment).  Every cell's arithmetic is the same on either path, so the bits do not depend on it.  All loads of a trip are
// issued before its first store.  No LDS, no scratch.
//
// Extremes.  One thread per interior cell and trip, grid-strided; the non-empty bins are listed by value in ascending order
// and their loads are independent: EXTREMES_UNROLL of them are issued before the first comparison.  The comparison is
// Julia's min / max written out: a NaN wins and stays (the first one), −0.0 < +0.0, a later equal value does not replace an
// earlier one — so the index is the smallest bin that attains the result, or the first NaN bin.
#include <algorithm>

#include "coflux_kernel_types.hpp"
#include "coflux_kernels.h"
#include "coflux_surface_cells.hpp"

namespace coflux {

namespace {

constexpr int CLIMATOLOGY_BLOCK = 256;
constexpr int CLIMATOLOGY_MAX_BLOCKS = 2048;   // memory-bound: cap the grid and stride the rest
constexpr int CLIMATOLOGY_UNROLL = 2;          // slots per thread per trip, all loaded before any is stored
constexpr int EXTREMES_UNROLL = 4;             // bins in flight per cell

// one array's pair of a slot: one 16-byte access where `vec` (a native vector type: the access stays whole through the
// optimiser), else the elements that exist
typedef double pair_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ pair_t load_pair(const double* p, bool vec, bool lo, bool hi) {
    pair_t v = {0.0, 0.0};
    if (vec) {
        v = *reinterpret_cast<const pair_t*>(p);
    } else {
        if (lo) v.x = p[0];
        if (hi) v.y = p[1];
    }
    return v;
}
__device__ __forceinline__ void store_pair(double* p, pair_t v, bool vec, bool lo, bool hi) {
    if (vec) {
        *reinterpret_cast<pair_t*>(p) = v;
    } else {
        if (lo) p[0] = v.x;
        if (hi) p[1] = v.y;
    }
}

template <bool STORE_TOTAL, bool STORE_BIN>
__global__ __launch_bounds__(CLIMATOLOGY_BLOCK) void climatology_kernel(ClimatologyFields F, GridDesc G, unsigned slots,
                                                                          ClimatologyBlend C) {
    const int f = blockIdx.y;
    const double* __restrict__ src = F.src[f];
    double* __restrict__ tot = F.total[f];
    double* __restrict__ bin = F.bin[f];
    const bool has_total = tot != nullptr;
    const unsigned total = (unsigned)G.ny * slots;
    const unsigned stride = gridDim.x * CLIMATOLOGY_BLOCK;
    for (unsigned t0 = blockIdx.x * CLIMATOLOGY_BLOCK + threadIdx.x; t0 < total; t0 += CLIMATOLOGY_UNROLL * stride) {
        pair_t fv[CLIMATOLOGY_UNROLL], tv[CLIMATOLOGY_UNROLL], bv[CLIMATOLOGY_UNROLL];
        ptrdiff_t at[CLIMATOLOGY_UNROLL];                                    // element offset of the slot's first element
        bool lo[CLIMATOLOGY_UNROLL], hi[CLIMATOLOGY_UNROLL];                 // element e / e + 1 exists
        bool vb[CLIMATOLOGY_UNROLL], vs[CLIMATOLOGY_UNROLL], vt[CLIMATOLOGY_UNROLL];   // the pair as one access: bin / source / total
#pragma unroll
        for (int u = 0; u < CLIMATOLOGY_UNROLL; ++u) {
            const unsigned t = t0 + u * stride;
            lo[u] = hi[u] = vb[u] = vs[u] = vt[u] = false;
            fv[u] = tv[u] = bv[u] = pair_t{0.0, 0.0};
            at[u] = 0;
            if (t >= total) continue;
            const unsigned j = t / slots, s = t - j * slots;
            const size_t row = (size_t)(j + G.hy) * (size_t)G.sj + (size_t)G.hx;
            const int h = (int)(((uintptr_t)(bin + row) >> 3) & 1);
            const int e = 2 * (int)s - h;
            lo[u] = e >= 0 && e < G.nx;
            hi[u] = e + 1 < G.nx;
            // (e = −1 with lo false: `at` then names the element before the row, which is never accessed — only at + 1 is)
            at[u] = (ptrdiff_t)row + e;
            vb[u] = lo[u] && hi[u];
            vs[u] = vb[u] && (int)(((uintptr_t)(src + row) >> 3) & 1) == h;
            vt[u] = vb[u] && has_total && (int)(((uintptr_t)(tot + row) >> 3) & 1) == h;
            fv[u] = load_pair(src + at[u], vs[u], lo[u], hi[u]);
            if (!STORE_TOTAL && has_total) tv[u] = load_pair(tot + at[u], vt[u], lo[u], hi[u]);
            if (!STORE_BIN) bv[u] = load_pair(bin + at[u], vb[u], lo[u], hi[u]);
        }
        // no load of the trip sinks below this point and no store rises above it (no instruction: a compiler fence)
        asm volatile("" ::: "memory");
#pragma unroll
        for (int u = 0; u < CLIMATOLOGY_UNROLL; ++u) {
            if (has_total) {
                pair_t out = fv[u];
                if (!STORE_TOTAL) {
                    out.x = blend(tv[u].x, fv[u].x, C.total_prev, C.total_new);
                    out.y = blend(tv[u].y, fv[u].y, C.total_prev, C.total_new);
                }
                store_pair(tot + at[u], out, vt[u], lo[u], hi[u]);
            }
            pair_t out = fv[u];
            if (!STORE_BIN) {
                out.x = blend(bv[u].x, fv[u].x, C.bin_prev, C.bin_new);
                out.y = blend(bv[u].y, fv[u].y, C.bin_prev, C.bin_new);
            }
            store_pair(bin + at[u], out, vb[u], lo[u], hi[u]);
        }
    }
}

// Julia's isless-free min / max on doubles: min(x, y) = NaN if either is NaN, −0.0 below +0.0.  `better` says whether the
// candidate v replaces the held value m (never on a tie: the earlier bin keeps the index; never once m is NaN).
__device__ __forceinline__ bool is_nan(double x) { return x != x; }
__device__ __forceinline__ bool negative(double x) { return __builtin_signbit(x) != 0; }
__device__ __forceinline__ bool better_min(double v, double m) {
    if (is_nan(m)) return false;
    if (is_nan(v)) return true;
    return v < m || (v == m && negative(v) && !negative(m));
}
__device__ __forceinline__ bool better_max(double v, double m) {
    if (is_nan(m)) return false;
    if (is_nan(v)) return true;
    return v > m || (v == m && !negative(v) && negative(m));
}

__global__ __launch_bounds__(CLIMATOLOGY_BLOCK) void climatology_extremes_kernel(const double* __restrict__ bins, size_t parent,
                                                                                   ClimatologyBinList L, GridDesc G,
                                                                                   double* __restrict__ d_min, double* __restrict__ d_max,
                                                                                   int32_t* __restrict__ d_argmin,
                                                                                   int32_t* __restrict__ d_argmax) {
    const unsigned cells = (unsigned)G.nx * (unsigned)G.ny;
    const unsigned stride = gridDim.x * CLIMATOLOGY_BLOCK;
    for (unsigned c = blockIdx.x * CLIMATOLOGY_BLOCK + threadIdx.x; c < cells; c += stride) {
        const unsigned j = c / (unsigned)G.nx, i = c - j * (unsigned)G.nx;
        const size_t k = (size_t)(j + G.hy) * (size_t)G.sj + (size_t)(i + G.hx);
        const double first = bins[(size_t)L.bin[0] * parent + k];
        double mn = first, mx = first;
        int32_t imin = L.bin[0], imax = L.bin[0];
        for (int b0 = 1; b0 < L.n; b0 += EXTREMES_UNROLL) {
            double v[EXTREMES_UNROLL];
#pragma unroll
            for (int u = 0; u < EXTREMES_UNROLL; ++u)
                v[u] = b0 + u < L.n ? bins[(size_t)L.bin[b0 + u] * parent + k] : 0.0;
#pragma unroll
            for (int u = 0; u < EXTREMES_UNROLL; ++u) {
                if (b0 + u >= L.n) continue;
                const int32_t b = L.bin[b0 + u];
                if (better_min(v[u], mn)) {
                    mn = v[u];
                    imin = b;
                }
                if (better_max(v[u], mx)) {
                    mx = v[u];
                    imax = b;
                }
            }
        }
        if (d_min) d_min[k] = mn;
        if (d_max) d_max[k] = mx;
        if (d_argmin) d_argmin[k] = imin;
        if (d_argmax) d_argmax[k] = imax;
    }
}

}  // namespace

hipError_t launch_climatology(hipStream_t st, const ClimatologyFields& F, int nfields, const GridDesc& G, bool store_total,
                              bool store_bin, const ClimatologyBlend& C, int max_blocks) {
    const unsigned slots = (unsigned)(G.nx / 2 + 1);
    const unsigned long long work = (unsigned long long)G.ny * slots;
    const int cap = max_blocks > 0 ? std::min(max_blocks, CLIMATOLOGY_MAX_BLOCKS) : CLIMATOLOGY_MAX_BLOCKS;
    const int per_field = std::max(1, cap / nfields);
    const int bx = (int)std::min<unsigned long long>((work + CLIMATOLOGY_BLOCK - 1) / CLIMATOLOGY_BLOCK, (unsigned long long)per_field);
    const dim3 grid(bx, nfields), block(CLIMATOLOGY_BLOCK);
    if (store_total && store_bin)
        hipLaunchKernelGGL((climatology_kernel<true, true>), grid, block, 0, st, F, G, slots, C);
    else if (store_total)
        hipLaunchKernelGGL((climatology_kernel<true, false>), grid, block, 0, st, F, G, slots, C);
    else if (store_bin)
        hipLaunchKernelGGL((climatology_kernel<false, true>), grid, block, 0, st, F, G, slots, C);
    else
        hipLaunchKernelGGL((climatology_kernel<false, false>), grid, block, 0, st, F, G, slots, C);
    return hipGetLastError();
}

hipError_t launch_climatology_extremes(hipStream_t st, const double* bins, size_t parent, const ClimatologyBinList& L, const GridDesc& G,
                                       double* d_min, double* d_max, int32_t* d_argmin, int32_t* d_argmax, int max_blocks) {
    const unsigned long long cells = (unsigned long long)G.nx * (unsigned long long)G.ny;
    const int cap = max_blocks > 0 ? std::min(max_blocks, CLIMATOLOGY_MAX_BLOCKS) : CLIMATOLOGY_MAX_BLOCKS;
    const int bx = (int)std::min<unsigned long long>((cells + CLIMATOLOGY_BLOCK - 1) / CLIMATOLOGY_BLOCK, (unsigned long long)cap);
    hipLaunchKernelGGL(climatology_extremes_kernel, dim3(bx), dim3(CLIMATOLOGY_BLOCK), 0, st, bins, parent, L, G, d_min, d_max, d_argmin,
                       d_argmax);
    return hipGetLastError();
}

}  // namespace coflux
