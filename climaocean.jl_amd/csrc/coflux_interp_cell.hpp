// coflux_interp_cell.hpp — the arithmetic every copy of interpolate_atmosphere_state! shares (the gather kernels of
// coflux_interp.hip, the tiled routine of coflux_interp_tiles.hpp and its fallback), so that every path produces the same
// bits: a source node's two time levels are blended first, the four blended corners are interpolated second (the
// reference interpolates each level and blends last; the two orders differ by rounding, ≈ 1e-16 relative).
#pragma once
#include "coflux_kernel_types.hpp"

namespace coflux {

__device__ __forceinline__ int wrap_index(int i, int n) {
    int r = i % n;
    return r < 0 ? r + n : r;
}

__device__ __forceinline__ double blend_levels(float a, float b, double tf) { return (double)b * tf + (double)a * (1.0 - tf); }
__device__ __forceinline__ double bilinear(double w00, double w01, double w10, double w11, double c00, double c01, double c10,
                                           double c11) {
    return w00 * c00 + w01 * c01 + w10 * c10 + w11 * c11;
}

}  // namespace coflux
