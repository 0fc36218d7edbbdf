// coflux_average.hip — time averages of surface fields accumulated on the device (cf_average_*, include/coflux.h).
//
// The running-mean form of Oceananigans' WindowedTimeAverage / integrate_average! [UPSTREAM-RECALL]: after a collection of
// weight w the buffer holds Σ w f / Σ w,
//     m ← (m · c_prev) + (f · c_new),   c_prev = T_prev / T_cur,  c_new = w / T_cur,  T_cur = T_prev + w,
// two products and one sum, each rounded (contraction off: numpy restates it bit for bit); the first collection of a window
// stores m ← f without reading m (a fresh buffer may hold NaNs).  The host computes c_prev and c_new in double.  The three
// operations are `blend` of coflux_surface_cells.hpp, which coflux_derived.hip applies to its samples as well.
//
// One launch covers every field of an averager: blockIdx.y is the field, x grid-strides over (row j, slot s) of the interior,
// AVERAGE_UNROLL slots per thread and trip.
// Slot s of row j covers the elements e = 2s − h, e + 1 (h = 1 when the mean's row starts 8 but not 16 bytes into a 16-byte
// line, so that a pair starts on a 16-byte boundary): one 16-byte access per array where both rows share that offset and
// the pair lies inside the interior, 8-byte accesses otherwise (the peel at either end of a row, or a source and a mean of
// different alignment).  Pointers need only 8-byte alignment.
#include <algorithm>

#include "coflux_kernel_types.hpp"
#include "coflux_kernels.h"
#include "coflux_surface_cells.hpp"

namespace coflux {

namespace {

constexpr int AVERAGE_BLOCK = 256;
constexpr int AVERAGE_MAX_BLOCKS = 2048;   // memory-bound: cap the grid and stride the rest

// slots per thread per trip of the grid-stride loop, all loaded before any is stored (bytes in flight; A/B builds may set it)
#ifndef COFLUX_AVERAGE_UNROLL
#define COFLUX_AVERAGE_UNROLL 2
#endif
constexpr int AVERAGE_UNROLL = COFLUX_AVERAGE_UNROLL;

template <bool STORE>
__global__ __launch_bounds__(AVERAGE_BLOCK) void average_kernel(AverageFields F, GridDesc G, unsigned slots, double c_prev,
                                                                  double c_new) {
    const int f = blockIdx.y;
    const double* __restrict__ src = F.src[f];
    double* __restrict__ mean = F.mean[f];
    const unsigned total = (unsigned)G.ny * slots;
    const unsigned stride = gridDim.x * AVERAGE_BLOCK;
    for (unsigned t0 = blockIdx.x * AVERAGE_BLOCK + threadIdx.x; t0 < total; t0 += AVERAGE_UNROLL * stride) {
        double2 fv[AVERAGE_UNROLL], mv[AVERAGE_UNROLL];
        double* m[AVERAGE_UNROLL];
        bool vec[AVERAGE_UNROLL], lo[AVERAGE_UNROLL], hi[AVERAGE_UNROLL];   // the pair as one access / element e / element e + 1
#pragma unroll
        for (int u = 0; u < AVERAGE_UNROLL; ++u) {
            const unsigned t = t0 + u * stride;
            vec[u] = lo[u] = hi[u] = false;
            fv[u] = mv[u] = double2{0.0, 0.0};
            m[u] = nullptr;
            if (t >= total) continue;
            const unsigned j = t / slots, s = t - j * slots;
            const size_t row = (size_t)(j + G.hy) * (size_t)G.sj + (size_t)G.hx;
            const int h = (int)(((uintptr_t)(mean + row) >> 3) & 1);
            const int e = 2 * (int)s - h;
            const double* a = src + row + e;
            m[u] = mean + row + e;
            lo[u] = e >= 0 && e < G.nx;
            hi[u] = e + 1 < G.nx;
            vec[u] = lo[u] && hi[u] && (int)(((uintptr_t)(src + row) >> 3) & 1) == h;
            if (vec[u]) {
                fv[u] = *reinterpret_cast<const double2*>(a);
                if (!STORE) mv[u] = *reinterpret_cast<const double2*>(m[u]);
            } else {
                if (lo[u]) {
                    fv[u].x = a[0];
                    if (!STORE) mv[u].x = m[u][0];
                }
                if (hi[u]) {
                    fv[u].y = a[1];
                    if (!STORE) mv[u].y = m[u][1];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < AVERAGE_UNROLL; ++u) {
            double2 out = fv[u];
            if (!STORE) {
                out.x = blend(mv[u].x, fv[u].x, c_prev, c_new);
                out.y = blend(mv[u].y, fv[u].y, c_prev, c_new);
            }
            if (vec[u]) {
                *reinterpret_cast<double2*>(m[u]) = out;
            } else {
                if (lo[u]) m[u][0] = out.x;
                if (hi[u]) m[u][1] = out.y;
            }
        }
    }
}

}  // namespace

hipError_t launch_average(hipStream_t st, const AverageFields& F, int nfields, const GridDesc& G, bool store, double c_prev,
                          double c_new) {
    const unsigned slots = (unsigned)(G.nx / 2 + 1);
    const unsigned long long work = (unsigned long long)G.ny * slots;
    const int per_field = std::max(1, AVERAGE_MAX_BLOCKS / nfields);
    const int bx = (int)std::min<unsigned long long>((work + AVERAGE_BLOCK - 1) / AVERAGE_BLOCK, (unsigned long long)per_field);
    const dim3 grid(bx, nfields);
    if (store)
        hipLaunchKernelGGL(average_kernel<true>, grid, dim3(AVERAGE_BLOCK), 0, st, F, G, slots, c_prev, c_new);
    else
        hipLaunchKernelGGL(average_kernel<false>, grid, dim3(AVERAGE_BLOCK), 0, st, F, G, slots, c_prev, c_new);
    return hipGetLastError();
}

}  // namespace coflux
