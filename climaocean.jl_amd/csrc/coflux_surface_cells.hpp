// coflux_surface_cells.hpp — what the surface-diagnostic kernels share (coflux_average.hip, coflux_derived.hip,
// coflux_integrals.hip, coflux_monitor.hip, coflux_regrid.hip): the walk over the interior in pairs of cells, the wet test
// of a pair, the butterfly sum and the running-mean blend.  Device code only; each kernel's own file states its summation
// order and names the pieces it takes from here.
#pragma once
#include "coflux_kernel_types.hpp"

namespace coflux {

// v += shfl_xor(v, W/2), …, 2, 1 within groups of W lanes: every lane of a group ends with the same bits (IEEE addition commutes)
template <int W>
__device__ __forceinline__ double butterfly_sum(double v) {
#pragma clang fp contract(off)
#pragma unroll
    for (int off = W / 2; off >= 1; off >>= 1) v = v + __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ double wave_sum(double v) { return butterfly_sum<64>(v); }

// the running mean after a collection (coflux_average.hip has the coefficients): two products and one sum, each rounded
__device__ __forceinline__ double blend(double m, double f, double c_prev, double c_new) {
#pragma clang fp contract(off)
    return m * c_prev + f * c_new;
}

// The interior is numbered row by row, c = j·nx + i; a thread takes the cells c0 (even) and c0 + 1.  k0 / k1: their element
// offsets in a halo-layout array, v0 / v1: whether they exist (a cell that does not is never loaded), pair: both in one row.
// (i0, j0): the first cell's column and row; wrap: it ends its row, so the second cell is (0, j0 + 1).
struct CellPair {
    size_t k0, k1;
    unsigned i0, j0;
    bool v0, v1, pair, wrap;
};

// GUARD = false: the caller knows c0 < n_cells
template <bool GUARD>
__device__ __forceinline__ CellPair cell_pair(unsigned c0, unsigned n_cells, const GridDesc& G) {
    const bool v0 = !GUARD || c0 < n_cells, v1 = c0 + 1u < n_cells;
    const unsigned j0 = v0 ? c0 / (unsigned)G.nx : 0u, i0 = v0 ? c0 - j0 * (unsigned)G.nx : 0u;
    const bool wrap = i0 + 1u == (unsigned)G.nx;
    const unsigned j1 = wrap ? j0 + 1u : j0, i1 = wrap ? 0u : i0 + 1u;
    const size_t k0 = (size_t)(j0 + G.hy) * (size_t)G.sj + (size_t)(i0 + G.hx);
    const size_t k1 = v1 ? (size_t)(j1 + G.hy) * (size_t)G.sj + (size_t)(i1 + G.hx) : k0;
    return CellPair{k0, k1, i0, j0, v0, v1, v1 && !wrap, wrap};
}

// The pair's two values of one array as raw bits, zero for a cell that does not exist.  Alignment only chooses the width of
// the loads: one 16-byte access where the two cells lie in one row and the array's address there is 16-byte aligned, two
// 8-byte accesses otherwise.
template <class Pair, class T>
__device__ __forceinline__ Pair load_pair_as(const T* __restrict__ q, const CellPair& C) {
    if (C.pair && (((uintptr_t)(q + C.k0)) & 15u) == 0) return *reinterpret_cast<const Pair*>(q + C.k0);
    Pair r{0, 0};
    if (C.v0) r.x = q[C.k0];
    if (C.v1) r.y = q[C.k1];
    return r;
}
__device__ __forceinline__ double2 load_pair(const double* __restrict__ p, const CellPair& C) { return load_pair_as<double2>(p, C); }
__device__ __forceinline__ ulonglong2 load_pair_bits(const double* __restrict__ p, const CellPair& C) {
    return load_pair_as<ulonglong2>(reinterpret_cast<const unsigned long long*>(p), C);
}

// Whether the pair's cells exist and are wet.  A bottom height that is NaN is wet: !(z_surface <= zb).
struct PairWet {
    bool s0, s1;
};
__device__ __forceinline__ PairWet pair_wet(const void* mask, int mask_kind, double z_surface, const CellPair& C) {
    bool s0 = C.v0, s1 = C.v1;
    if (mask != nullptr && mask_kind == CF_MASK_U8) {
        const uint8_t* m = (const uint8_t*)mask;
        if (C.v0) s0 = m[C.k0] != 0;
        if (C.v1) s1 = m[C.k1] != 0;
    } else if (mask != nullptr && mask_kind == CF_MASK_BOTTOM_HEIGHT) {
        const double2 zb = load_pair((const double*)mask, C);
        s0 = C.v0 && !(z_surface <= zb.x);
        s1 = C.v1 && !(z_surface <= zb.y);
    }
    return PairWet{s0, s1};
}

}  // namespace coflux
