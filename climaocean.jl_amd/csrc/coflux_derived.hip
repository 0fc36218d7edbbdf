// coflux_derived.hip — derived surface quantities averaged in the collection launch (cf_average_create_derived,
// include/coflux.h has the kinds, their order of operations and the footprint).
//
// One launch per collection covers every term.  A work item is (band b, column i): the thread walks the DERIVED_ROWS rows
// j = b · DERIVED_ROWS … of its band from south to north, consecutive lanes hold consecutive i of one band.
//   * Each distinct source array (slot) is loaded ONCE per cell, whatever number of terms names it; the terms then pick
//     their operands out of registers.
//   * [i+1] is handed over by the neighbouring lane (__shfl_down: the LDS crossbar, no LDS memory); lane 63 of a wave and
//     the last cell of a row load their own — the row's last cell reads halo column nx.
//   * [j+1] is loaded as the row above and carried in registers into the thread's next row, so a band of R rows reads
//     R + 1 rows of such a slot instead of 2R; the band's top row is read again by the band above (row ny: the halo row).
//   * The term table is uniform per launch: it lives in the kernel arguments (SGPRs) and is dispatched on scalars.  The
//     slot and term loops are unrolled over the bucket K (4 / 8 / 16 ≥ slots and terms), so pointers, scales and means have
//     static indices; the per-cell values sit in K-wide register vectors that a term indexes with its (uniform) slot
//     number — register-relative moves, no scratch, no LDS.
// Every operation of a sample is rounded on its own (contraction off) so that NumPy restates it bit for bit; the sample
// enters the mean through `blend` of coflux_surface_cells.hpp.
#include <algorithm>

#include "coflux_kernel_types.hpp"
#include "coflux_kernels.h"
#include "coflux_surface_cells.hpp"

namespace coflux {

namespace {

constexpr int DERIVED_BLOCK = 256;
constexpr int DERIVED_MAX_BLOCKS = 2048;   // memory-bound: cap the grid and stride the rest
#ifndef COFLUX_DERIVED_ROWS
#define COFLUX_DERIVED_ROWS 4              // rows per band (scheduling only, never results; A/B builds may set it)
#endif
constexpr int DERIVED_ROWS = COFLUX_DERIVED_ROWS;

struct Operands {   // what a term may read at its cell
    double a0, ax, ay, b0, by, c, s;
};

__device__ __forceinline__ double center(double lo, double hi) {
#pragma clang fp contract(off)
    return (lo + hi) * 0.5;
}
__device__ __forceinline__ double center_square(double lo, double hi) {
#pragma clang fp contract(off)
    return (lo * lo + hi * hi) * 0.5;
}

__device__ __forceinline__ double term_value(int kind, int flags, const Operands& o) {
#pragma clang fp contract(off)
    switch (kind) {
        case CF_TERM_FIELD: return o.a0;
        case CF_TERM_PRODUCT: return o.a0 * o.b0;
        case CF_TERM_CENTER_X: return center(o.a0, o.ax);
        case CF_TERM_CENTER_Y: return center(o.a0, o.ay);
        case CF_TERM_CENTER_X_SQUARE: return center_square(o.a0, o.ax);
        case CF_TERM_CENTER_Y_SQUARE: return center_square(o.a0, o.ay);
        case CF_TERM_KINETIC_ENERGY: return (center_square(o.a0, o.ax) + center_square(o.b0, o.by)) * 0.5;
        default: {
            const bool centers = (flags & CF_TERM_AT_CENTERS) != 0;
            const double p = centers ? o.a0 : center(o.a0, o.ax);
            const double q = centers ? o.b0 : center(o.b0, o.by);
            return kind == CF_TERM_EAST ? p * o.c - q * o.s : p * o.s + q * o.c;
        }
    }
}

template <int K, bool STORE>
__global__ __launch_bounds__(DERIVED_BLOCK) void derived_average_kernel(DerivedArgs A, GridDesc G, unsigned items, double c_prev,
                                                                          double c_new) {
    typedef double vec __attribute__((ext_vector_type(K)));
    const unsigned lane = threadIdx.x & 63u;
    const unsigned stride = gridDim.x * DERIVED_BLOCK;
    const unsigned nx = (unsigned)G.nx;
    for (unsigned base = blockIdx.x * DERIVED_BLOCK; base < items; base += stride) {   // uniform per workgroup
        const unsigned q = base + threadIdx.x;
        const bool live = q < items;
        const unsigned band = live ? q / nx : 0u, i = live ? q - band * nx : 0u;
        const bool own = lane == 63u || i + 1u == nx;   // nobody hands this lane its [i+1]
        vec v0 = 0.0, vx = 0.0, vy = 0.0, mv = 0.0;
        for (int r = 0; r < DERIVED_ROWS; ++r) {
            const int j = (int)band * DERIVED_ROWS + r;
            const bool on = live && j < G.ny;
            const size_t k = (size_t)(j + G.hy) * (size_t)G.sj + (size_t)G.hx + (size_t)i;
            // every load of the row goes out before anything waits for one
#pragma unroll
            for (int s = 0; s < K; ++s) {
                if (s < A.n_src) {
                    const double* p = A.src[s];
                    const bool x = (A.need_x >> s) & 1u, y = (A.need_y >> s) & 1u;
                    if (r > 0 && y) {
                        v0[s] = vy[s];   // the row above of the previous trip
                    } else {
                        double t = 0.0;
                        if (on) t = p[k];
                        v0[s] = t;
                    }
                    if (x) {
                        double t = 0.0;
                        if (on && own) t = p[k + 1];
                        vx[s] = t;
                    }
                    if (y) {
                        double t = 0.0;
                        if (on) t = p[k + (size_t)G.sj];
                        vy[s] = t;
                    }
                }
            }
            if (!STORE) {
#pragma unroll
                for (int t = 0; t < K; ++t) {
                    if (t < A.n_terms) {
                        double m = 0.0;
                        if (on) m = A.mean[t][k];
                        mv[t] = m;
                    }
                }
            }
            // [i+1] from the lane to the east (all lanes of the wave are here: the conditions above are uniform)
#pragma unroll
            for (int s = 0; s < K; ++s) {
                if (s < A.n_src && ((A.need_x >> s) & 1u)) {
                    const double east = __shfl_down(v0[s], 1);
                    vx[s] = own ? vx[s] : east;
                }
            }
            Operands o{};
            if (A.cos_slot >= 0) {
                o.c = v0[A.cos_slot];
                o.s = v0[A.sin_slot];
            }
#pragma unroll
            for (int t = 0; t < K; ++t) {
                if (t < A.n_terms) {
                    const int a = A.a[t], b = A.b[t];
                    o.a0 = v0[a];
                    o.ax = vx[a];
                    o.ay = vy[a];
                    o.b0 = v0[b];
                    o.by = vy[b];
                    double sample;
                    {
#pragma clang fp contract(off)
                        sample = term_value(A.kind[t], A.flags[t], o) * A.scale[t];
                    }
                    const double out = STORE ? sample : blend(mv[t], sample, c_prev, c_new);
                    if (on) A.mean[t][k] = out;
                }
            }
        }
    }
}

template <int K>
void launch_bucket(hipStream_t st, int blocks, const DerivedArgs& A, const GridDesc& G, unsigned items, bool store, double c_prev,
                   double c_new) {
    if (store)
        hipLaunchKernelGGL((derived_average_kernel<K, true>), dim3(blocks), dim3(DERIVED_BLOCK), 0, st, A, G, items, c_prev, c_new);
    else
        hipLaunchKernelGGL((derived_average_kernel<K, false>), dim3(blocks), dim3(DERIVED_BLOCK), 0, st, A, G, items, c_prev, c_new);
}

}  // namespace

hipError_t launch_derived_average(hipStream_t st, const DerivedArgs& A, const GridDesc& G, bool store, double c_prev, double c_new) {
    const unsigned long long bands = ((unsigned long long)G.ny + DERIVED_ROWS - 1) / DERIVED_ROWS;
    const unsigned long long items = bands * (unsigned long long)G.nx;
    if (G.nx < 1 || G.ny < 1 || items + (unsigned long long)DERIVED_MAX_BLOCKS * DERIVED_BLOCK >= (1ull << 32)) return hipErrorInvalidValue;
    const int cap = A.max_blocks > 0 ? std::min(A.max_blocks, DERIVED_MAX_BLOCKS) : DERIVED_MAX_BLOCKS;
    const int blocks = (int)std::min<unsigned long long>((items + DERIVED_BLOCK - 1) / DERIVED_BLOCK, (unsigned long long)cap);
    const int widest = std::max(A.n_src, A.n_terms);
    if (widest <= 4)
        launch_bucket<4>(st, blocks, A, G, (unsigned)items, store, c_prev, c_new);
    else if (widest <= 8)
        launch_bucket<8>(st, blocks, A, G, (unsigned)items, store, c_prev, c_new);
    else
        launch_bucket<16>(st, blocks, A, G, (unsigned)items, store, c_prev, c_new);
    return hipGetLastError();
}

}  // namespace coflux
