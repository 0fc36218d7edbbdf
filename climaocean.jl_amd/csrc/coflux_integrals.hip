// coflux_integrals.hip — area-weighted, masked, regional surface integrals (cf_integrals_*, include/coflux.h).
//
// One collection turns up to CF_INTEGRALS_MAX_ENTRIES entries (kind, a, b, threshold, region bit) into one record
//     value[e] = Σ A·x_e  over the interior cells that are wet and carry the entry's region bit,
// x = 1 | a | a·b | [a > threshold].  Excluded cells are selected away, never multiplied by zero: their field and area values
// may be NaN.
//
// Summation order — a function of (nx, ny) alone, so a record's bits do not depend on the halo widths, on where the arrays
// start in memory, on the number of workgroups launched or on the run:
//   1. the interior is numbered row by row, c = j·nx + i, and cut into tiles of INTEGRALS_TILE = 1024 consecutive cells;
//   2. thread t of a tile owns the cells c₀ + 2t, c₀ + 2t + 1, c₀ + 512 + 2t, c₀ + 512 + 2t + 1 and adds their terms in that
//      order to a zero accumulator;
//   3. the 64 lanes of a wave are combined by the butterfly v += shfl_xor(v, 32), 16, 8, 4, 2, 1 (every lane ends with the
//      same bits: IEEE addition commutes);
//   4. the four waves are added in wave order through LDS: ((w0 + w1) + w2) + w3 → partial[tile][e];
//   5. a second launch (one workgroup per entry) combines the tiles: thread t adds the partials of tiles t, t + 256, … in that
//      order, then steps 3 and 4 again → the record.
// No floating-point atomics.  A tile loop that strides by gridDim keeps step 1 independent of the grid that was launched.
// Alignment only chooses the width of the loads (one 16-byte access where a thread's two cells lie in one row and the
// array's address there is 16-byte aligned, two 8-byte accesses otherwise), never the cells a thread owns.
//
// Every distinct array is loaded once per cell: the host numbers the distinct `a` / `b` pointers (slots), a thread parks
// its two values of slot f in LDS at [f][t] — its own cell of LDS, so no barrier — and each entry reads the slots it names
// from there.  The entry loop is unrolled over the compile-time bucket NE (8 / 16 / 32), so the accumulators are registers
// with static indices and the slot index only ever addresses LDS: no scratch.  The entries' descriptors live in LDS as well
// (as kernel arguments they took a hundred scalar registers): one broadcast read and a uniform branch on the kind per entry.
// Contraction is off throughout: a·b is one rounded product, ·A another, the sum a third, in every instantiation.
// The pair of cells, its loads, its wet test and the butterfly (wave_sum) are coflux_surface_cells.hpp's.
#include <algorithm>

#include "coflux_kernel_types.hpp"
#include "coflux_kernels.h"
#include "coflux_surface_cells.hpp"

namespace coflux {

namespace {

constexpr int INTEGRALS_BLOCK = 256;
constexpr int INTEGRALS_PAIRS = INTEGRALS_TILE / (2 * INTEGRALS_BLOCK);   // pairs of cells per thread and tile
static_assert(INTEGRALS_PAIRS * 2 * INTEGRALS_BLOCK == INTEGRALS_TILE, "a tile is a whole number of pairs per thread");
constexpr int INTEGRALS_WAVES = INTEGRALS_BLOCK / 64;

template <int NE>
__global__ __launch_bounds__(INTEGRALS_BLOCK) void integrals_tile_kernel(IntegralArgs K, GridDesc G, unsigned n_cells,
                                                                         unsigned n_tiles) {
#pragma clang fp contract(off)
    extern __shared__ double2 stage[];                 // [max(n_fields, 1)][INTEGRALS_BLOCK]
    __shared__ double wsum[INTEGRALS_WAVES][NE];
    // the entries' descriptors live in LDS, not in 100 scalar registers: one broadcast read per entry and tile
    __shared__ unsigned ent[NE];
    __shared__ double thr[NE];
    const unsigned t = threadIdx.x;
    if ((int)t < K.n_entries) {
        ent[t] = K.entry[t];
        thr[t] = K.threshold[t];
    }
    __syncthreads();
    for (unsigned tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        double acc[NE];
#pragma unroll
        for (int e = 0; e < NE; ++e) acc[e] = 0.0;
#pragma unroll
        for (int u = 0; u < INTEGRALS_PAIRS; ++u) {
            const unsigned c0 = tile * (unsigned)INTEGRALS_TILE + 2u * (t + (unsigned)(u * INTEGRALS_BLOCK));
            const CellPair C = cell_pair<true>(c0, n_cells, G);
            const bool v0 = C.v0, v1 = C.v1;
            const size_t k0 = C.k0, k1 = C.k1;
            const PairWet wet = pair_wet(K.mask, K.mask_kind, K.z_surface, C);
            unsigned r0 = v0 ? 1u : 0u, r1 = v1 ? 1u : 0u;  // region bits
            if (K.region != nullptr) {
                r0 = v0 ? K.region[k0] : 0u;
                r1 = v1 ? K.region[k1] : 0u;
            }
            double2 A{1.0, 1.0};
            if (K.area != nullptr) A = load_pair(K.area, C);
#pragma unroll 4
            for (int f = 0; f < K.n_fields; ++f) stage[f * INTEGRALS_BLOCK + t] = load_pair(K.field[f], C);

#pragma unroll
            for (int e = 0; e < NE; ++e) {
                if (e < K.n_entries) {
                    const unsigned d = __builtin_amdgcn_readfirstlane(ent[e]);   // kind | slot of a << 8 | slot of b << 16 | region mask << 24
                    const unsigned kind = d & 0xffu;
                    double2 x{1.0, 1.0};
                    if (kind != CF_INTEGRAND_ONE) {
                        const double2 a = stage[((d >> 8) & 0xffu) * INTEGRALS_BLOCK + t];
                        if (kind == CF_INTEGRAND_FIELD) {
                            x = a;
                        } else if (kind == CF_INTEGRAND_PRODUCT) {
                            const double2 b = stage[((d >> 16) & 0xffu) * INTEGRALS_BLOCK + t];
                            x.x = a.x * b.x;
                            x.y = a.y * b.y;
                        } else {
                            const double th = thr[e];
                            x.x = a.x > th ? 1.0 : 0.0;
                            x.y = a.y > th ? 1.0 : 0.0;
                        }
                    }
                    const unsigned bits = d >> 24;
                    const double term0 = (wet.s0 && (r0 & bits) != 0u) ? x.x * A.x : 0.0;
                    const double term1 = (wet.s1 && (r1 & bits) != 0u) ? x.y * A.y : 0.0;
                    acc[e] = (acc[e] + term0) + term1;
                }
            }
        }
#pragma unroll
        for (int e = 0; e < NE; ++e)
            if (e < K.n_entries) {
                const double v = wave_sum(acc[e]);
                if ((t & 63u) == 0u) wsum[t >> 6][e] = v;
            }
        __syncthreads();
        if ((int)t < K.n_entries) {
            double s = wsum[0][t];
#pragma unroll
            for (int w = 1; w < INTEGRALS_WAVES; ++w) s = s + wsum[w][t];
            K.partial[(size_t)tile * NE + t] = s;
        }
        __syncthreads();
    }
}

// record[e] = the partials of entry e = blockIdx.x over all tiles, in the order of the header's step 5
__global__ __launch_bounds__(INTEGRALS_BLOCK) void integrals_combine_kernel(const double* __restrict__ partial, int stride,
                                                                            unsigned n_tiles, double* __restrict__ record) {
#pragma clang fp contract(off)
    __shared__ double wsum[INTEGRALS_WAVES];
    const unsigned t = threadIdx.x, e = blockIdx.x;
    double s = 0.0;
    for (unsigned tile = t; tile < n_tiles; tile += INTEGRALS_BLOCK) s = s + partial[(size_t)tile * stride + e];
    s = wave_sum(s);
    if ((t & 63u) == 0u) wsum[t >> 6] = s;
    __syncthreads();
    if (t == 0) {
        double r = wsum[0];
#pragma unroll
        for (int w = 1; w < INTEGRALS_WAVES; ++w) r = r + wsum[w];
        record[e] = r;
    }
}

template <int NE>
hipError_t launch_tiles(hipStream_t st, const IntegralArgs& K, const GridDesc& G, unsigned n_cells, unsigned n_tiles, unsigned blocks) {
    const size_t lds = (size_t)std::max(K.n_fields, 1) * INTEGRALS_BLOCK * sizeof(double2);
    if (lds > 48 * 1024) {   // beyond the default dynamic LDS limit of a launch (gfx950 has 160 KiB per workgroup)
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&integrals_tile_kernel<NE>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)((size_t)CF_INTEGRALS_MAX_FIELDS * INTEGRALS_BLOCK * sizeof(double2)));
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(integrals_tile_kernel<NE>, dim3(blocks), dim3(INTEGRALS_BLOCK), lds, st, K, G, n_cells, n_tiles);
    return hipGetLastError();
}

}  // namespace

int integrals_bucket(int n_entries) { return n_entries <= 8 ? 8 : (n_entries <= 16 ? 16 : 32); }

unsigned integrals_tiles(const GridDesc& G) {
    const unsigned long long cells = (unsigned long long)G.nx * (unsigned long long)G.ny;
    return (unsigned)((cells + INTEGRALS_TILE - 1) / INTEGRALS_TILE);
}

hipError_t launch_integrals(hipStream_t st, const IntegralArgs& K, const GridDesc& G, double* record, int max_blocks) {
    const unsigned n_cells = (unsigned)G.nx * (unsigned)G.ny, n_tiles = integrals_tiles(G);
    const unsigned blocks = max_blocks > 0 ? std::min(n_tiles, (unsigned)max_blocks) : n_tiles;
    const int NE = integrals_bucket(K.n_entries);
    hipError_t e = NE == 8    ? launch_tiles<8>(st, K, G, n_cells, n_tiles, blocks)
                   : NE == 16 ? launch_tiles<16>(st, K, G, n_cells, n_tiles, blocks)
                              : launch_tiles<32>(st, K, G, n_cells, n_tiles, blocks);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(integrals_combine_kernel, dim3(K.n_entries), dim3(INTEGRALS_BLOCK), 0, st, K.partial, NE, n_tiles, record);
    return hipGetLastError();
}

}  // namespace coflux
