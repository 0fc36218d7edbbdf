// coflux_regrid.hip — a fixed sparse surface operator applied to masked ocean-grid fields (cf_regrid_*, include/coflux.h):
// conservative maps onto a latitude–longitude grid, zonal means, any regridder built elsewhere.
//
// Per destination row r, with W(r) the entries of the row whose source cell is wet,
//     D = Σ_{k∈W} weight[k],   N_f = Σ_{k∈W} weight[k] · src_f[col[k]],   dst_f[r] = N_f / D (MEAN; NaN where D == 0) | N_f (SUM),
// for up to CF_REGRID_MAX_FIELDS fields in one pass: the entry's offset, its weight and its mask byte are loaded once for
// all fields, each field costs one 8-byte gather per entry.  Excluded entries are selected away, never multiplied by zero:
// a land cell may hold NaN or Inf.  weight·x, every addition and the division are rounded separately (contraction is off).
//
// Summation order — a function of the row's entry count n alone (land entries keep their place and add a selected +0.0), so
// the bits of dst_f[r] depend only on the row's (col, weight) in the order given, the mask and the interior values — not on
// the row's index or its neighbours in the operator, the halo widths, where the arrays start, the number of workgroups,
// n_fields, the other fields, or the run:
//   n ≤ 64   the row belongs to a group of 16 lanes (four rows per wave).  Lane g adds the terms of entries g, g + 16, g + 32,
//            g + 48, in that order, to +0.0 (an absent entry adds +0.0 as well); the group is combined by the butterfly
//            v += shfl_xor(v, 8), 4, 2, 1 (every lane ends with the same bits: IEEE addition commutes).
//   n > 64   the row is cut into segments of 256 consecutive entries, one wave per segment.  Lane l adds the terms of the
//            segment's entries l, l + 64, l + 128, l + 192 to +0.0, then the butterfly 32, 16, 8, 4, 2, 1.  A row of one
//            segment is finished there; otherwise the segment partials p₀, p₁, … are added in segment order,
//            ((p₀ + p₁) + p₂) + …, by a second small launch (one thread per such row), which also divides.
// D is summed in exactly the same order as every N_f.  No floating-point atomics.  The host builds the unit tables at create
// (coflux_regrid.cpp); the kernel strides over wave units by the launched grid, which therefore never reaches a bit.
//
// The field loop is unrolled over the compile-time bucket KB (1 / 4 / 8 / 16), so the accumulators and the field pointers
// have static indices: no scratch.  No LDS, no barrier: a wave never waits for another.
// The butterfly is coflux_surface_cells.hpp's butterfly_sum<W>.
#include <algorithm>
#include <cmath>

#include "coflux_kernel_types.hpp"
#include "coflux_kernels.h"
#include "coflux_surface_cells.hpp"

namespace coflux {

namespace {

constexpr int REGRID_BLOCK = 256;
constexpr int REGRID_WAVES = REGRID_BLOCK / 64;
constexpr int REGRID_TERMS = 4;          // entries per lane of a group (16 lanes · 4 = REGRID_SHORT) or segment (64 · 4)
static_assert(16 * REGRID_TERMS == REGRID_SHORT && 64 * REGRID_TERMS == REGRID_SEGMENT, "a lane owns four entries");

// Lane g of W adds its four entries of [start, start + count) — count ≤ 4 W — and the group is combined: N[f], D.
template <int KB, int W>
__device__ __forceinline__ void regrid_span(const RegridTables& T, const RegridFields& F, uint32_t start, uint32_t count, uint32_t g,
                                            double (&N)[KB], double& D) {
#pragma clang fp contract(off)
    uint32_t off[REGRID_TERMS];
    double w[REGRID_TERMS];
    bool wet[REGRID_TERMS];
#pragma unroll
    for (int u = 0; u < REGRID_TERMS; ++u) {
        const uint32_t e = g + (uint32_t)(u * W);
        const bool in = e < count;
        off[u] = in ? T.offset[start + e] : 0u;
        w[u] = in ? T.weight[start + e] : 0.0;
        wet[u] = in;
        if (in && T.mask_kind == CF_MASK_U8) wet[u] = ((const uint8_t*)T.mask)[off[u]] != 0;
        if (in && T.mask_kind == CF_MASK_BOTTOM_HEIGHT) wet[u] = !(T.z_surface <= ((const double*)T.mask)[off[u]]);
    }
    double d = 0.0;
#pragma unroll
    for (int u = 0; u < REGRID_TERMS; ++u) d = d + (wet[u] ? w[u] : 0.0);
    D = butterfly_sum<W>(d);
#pragma unroll
    for (int f = 0; f < KB; ++f) {
        N[f] = 0.0;
        if (f < F.n_fields) {
            const double* __restrict__ x = F.src[f];
            double t[REGRID_TERMS];
#pragma unroll
            for (int u = 0; u < REGRID_TERMS; ++u) t[u] = wet[u] ? x[off[u]] : 0.0;
            double a = 0.0;
#pragma unroll
            for (int u = 0; u < REGRID_TERMS; ++u) a = a + (wet[u] ? w[u] * t[u] : 0.0);
            N[f] = butterfly_sum<W>(a);
        }
    }
}

__device__ __forceinline__ double regrid_value(int mode, double N, double D) {
#pragma clang fp contract(off)
    if (mode == CF_REGRID_SUM) return N;
    return D == 0.0 ? __builtin_nan("") : N / D;
}

template <int KB>
__device__ __forceinline__ void regrid_finish(const RegridTables& T, const RegridFields& F, uint32_t row, const double (&N)[KB],
                                              double D) {
    if (F.coverage != nullptr) F.coverage[row] = D;
#pragma unroll
    for (int f = 0; f < KB; ++f)
        if (f < F.n_fields) F.dst[f][row] = regrid_value(T.mode, N[f], D);
}

template <int KB>
__global__ __launch_bounds__(REGRID_BLOCK) void regrid_rows_kernel(RegridTables T, RegridFields F) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t units = T.n_segments + T.n_short_units;
    // wave-uniform: every lane of a wave takes every trip and every shuffle
    for (uint32_t unit = blockIdx.x * REGRID_WAVES + wave; unit < units; unit += gridDim.x * REGRID_WAVES) {
        double N[KB], D;
        if (unit < T.n_segments) {
            const RegridSegment S = T.segments[unit];
            regrid_span<KB, 64>(T, F, S.start, S.count, lane, N, D);
            if (lane == 0) {
                if (S.slot == REGRID_NONE) {
                    regrid_finish<KB>(T, F, S.row, N, D);
                } else {
                    double* p = T.partial + (size_t)S.slot * REGRID_PARTIAL;
#pragma unroll
                    for (int f = 0; f < KB; ++f)
                        if (f < F.n_fields) p[f] = N[f];
                    p[CF_REGRID_MAX_FIELDS] = D;
                }
            }
        } else {
            const uint32_t row = T.short_rows[(size_t)(unit - T.n_segments) * 4u + (lane >> 4)];
            uint32_t start = 0u, count = 0u;
            if (row != REGRID_NONE) {
                start = T.row_start[row];
                count = T.row_start[row + 1u] - start;
            }
            regrid_span<KB, 16>(T, F, start, count, lane & 15u, N, D);
            if (row != REGRID_NONE && (lane & 15u) == 0u) regrid_finish<KB>(T, F, row, N, D);
        }
    }
}

// the rows of several segments: partials in segment order, then the division (one thread per row)
template <int KB>
__global__ __launch_bounds__(64) void regrid_combine_kernel(RegridTables T, RegridFields F) {
#pragma clang fp contract(off)
    const uint32_t r = blockIdx.x * 64u + threadIdx.x;
    if (r >= T.n_long_rows) return;
    const RegridLongRow R = T.long_rows[r];
    const double* p = T.partial + (size_t)R.first_slot * REGRID_PARTIAL;
    double N[KB], D = p[CF_REGRID_MAX_FIELDS];
#pragma unroll
    for (int f = 0; f < KB; ++f) N[f] = f < F.n_fields ? p[f] : 0.0;
    for (uint32_t s = 1; s < R.n_segments; ++s) {
        p += REGRID_PARTIAL;
        D = D + p[CF_REGRID_MAX_FIELDS];
#pragma unroll
        for (int f = 0; f < KB; ++f)
            if (f < F.n_fields) N[f] = N[f] + p[f];
    }
    regrid_finish<KB>(T, F, R.row, N, D);
}

template <int KB>
hipError_t launch_bucket(hipStream_t st, const RegridTables& T, const RegridFields& F, unsigned blocks) {
    hipLaunchKernelGGL(regrid_rows_kernel<KB>, dim3(blocks), dim3(REGRID_BLOCK), 0, st, T, F);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || T.n_long_rows == 0) return e;
    hipLaunchKernelGGL(regrid_combine_kernel<KB>, dim3((T.n_long_rows + 63u) / 64u), dim3(64), 0, st, T, F);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_regrid(hipStream_t st, const RegridTables& T, const RegridFields& F, int max_blocks, int cu_count) {
    const unsigned long long units = (unsigned long long)T.n_segments + T.n_short_units;
    if (units == 0) return hipSuccess;
    const unsigned long long want = (units + REGRID_WAVES - 1) / REGRID_WAVES;
    const unsigned long long cap = max_blocks > 0 ? (unsigned long long)max_blocks : 8ull * (unsigned long long)std::max(cu_count, 1);
    const unsigned blocks = (unsigned)std::min(want, cap);
    if (F.n_fields <= 1) return launch_bucket<1>(st, T, F, blocks);
    if (F.n_fields <= 4) return launch_bucket<4>(st, T, F, blocks);
    if (F.n_fields <= 8) return launch_bucket<8>(st, T, F, blocks);
    return launch_bucket<16>(st, T, F, blocks);
}

}  // namespace coflux
