// coflux_coupled_cells.hpp — the per-cell bodies of the three pointwise passes that precede a coupled step's solve: the land
// freshwater (interpolate_land_kernel), the ice–ocean exchange with frazil (sea_ice_ocean_flux_kernel) and the salinity
// restoring buffer (salinity_restoring_kernel).  Each kernel of its own and the one launch that does all three
// (prepare_coupled_step_kernel, coflux_net.hip) call the same function, so every path produces the same bits: the build
// contracts within a source expression only, and the expressions below are the kernels' own, unsplit.
#pragma once
#include "coflux_interp_cell.hpp"
#include "coflux_kernel_types.hpp"
#include "coflux_kernels.h"

namespace coflux {

// JRA55PrescribedLand at cell (i, j) of the ring window, k = cell_index(G, i, j): friver + licalvf, same weights and time
// blend as the atmosphere, gather form
__device__ __forceinline__ double land_freshwater_cell(const float* __restrict__ friver, const float* __restrict__ licalvf, int ns_x,
                                                       int ns_y, int level1, int level2, double tf, const WeightDesc& Wt,
                                                       const GridDesc& G, int i, int j, size_t k) {
    const double fi = Wt.separable ? Wt.fi[i + G.hx] : Wt.fi[k];
    const double fj = Wt.separable ? Wt.fj[j + G.hy] : Wt.fj[k];
    const double xi = fi - floor(fi), eta = fj - floor(fj);
    const int i0 = (int)trunc(fi), ja = (int)trunc(fj);
    const int is0 = wrap_index(i0, ns_x), is1 = wrap_index(i0 + (fi > 0.0 ? 1 : (fi < 0.0 ? -1 : 0)), ns_x);
    const int j0 = min(max(ja, 0), ns_y - 1), j1 = min(max(ja + (fj > 0.0 ? 1 : (fj < 0.0 ? -1 : 0)), 0), ns_y - 1);
    const size_t g00 = (size_t)j0 * ns_x + is0, g10 = (size_t)j0 * ns_x + is1, g01 = (size_t)j1 * ns_x + is0, g11 = (size_t)j1 * ns_x + is1;
    const size_t plane = (size_t)ns_x * ns_y;
    const double w00 = (1.0 - xi) * (1.0 - eta), w01 = (1.0 - xi) * eta, w10 = xi * (1.0 - eta), w11 = xi * eta;
    auto value = [&](const float* d) {
        const float* a = d + (size_t)level1 * plane;
        const float* b = d + (size_t)level2 * plane;
        return bilinear(w00, w01, w10, w11, blend_levels(a[g00], b[g00], tf), blend_levels(a[g01], b[g01], tf),
                        blend_levels(a[g10], b[g10], tf), blend_levels(a[g11], b[g11], tf));
    };
    return value(friver) + (licalvf ? value(licalvf) : 0.0);
}

// ThreeEquationHeatFlux with momentum-based friction velocity + frazil at interior cell k; `wet` and `So` (read where wet)
// are the caller's, so that a launch with several interior jobs reads the mask and S once
struct IceOceanCell {
    double q_io, j_io, q_fr, us;
};
__device__ __forceinline__ IceOceanCell sea_ice_ocean_cell(const DevParams& P, const cf_ice_ocean_params& Q, const GridDesc& G, bool wet,
                                                           double So, const double* __restrict__ T, const double* __restrict__ conc,
                                                           const double* __restrict__ tx, const double* __restrict__ ty, size_t k) {
    double q_io = 0.0, j_io = 0.0, q_fr = 0.0, us = 0.0;
    if (wet) {
        const double rho_o = 1.0 / P.rho_o_inv, c_o = 1.0 / P.c_o_inv;
        double To = T[k];
        const double Tf = -Q.liquidus_slope * So;
        if (Q.time_step > 0.0 && To < Tf) {  // frazil: the deficit below freezing is handed to the ice model
            q_fr = rho_o * c_o * Q.top_cell_thickness * (To - Tf) / Q.time_step;
            To = Tf;
        }
        const double a = conc ? conc[k] : 0.0;
        if (a > 0.0) {
            const double txc = tx ? 0.5 * (tx[k] + tx[k + 1]) : 0.0, tyc = ty ? 0.5 * (ty[k] + ty[k + (size_t)G.sj]) : 0.0;
            us = fmax(sqrt(sqrt(txc * txc + tyc * tyc)), Q.minimum_friction_velocity);
            // α_s (S_o − S_b) = (c_o α_h / ℒ)(T_o + m S_b)(S_b − S_i): the positive root of A S_b² + B S_b − C = 0
            const double ah = Q.heat_transfer_coefficient, as = Q.salt_transfer_coefficient, m = Q.liquidus_slope;
            const double g = c_o * ah / Q.latent_heat_of_fusion;
            const double A = g * m, B = g * To - g * m * Q.ice_salinity + as, C = g * To * Q.ice_salinity + as * So;
            const double Sb = (-B + sqrt(B * B + 4.0 * A * C)) / (2.0 * A);
            const double Tb = -m * Sb;
            q_io = a * rho_o * c_o * ah * us * (To - Tb);
            j_io = a * as * us * (So - Sb);
        }
    }
    return IceOceanCell{q_io, j_io, q_fr, us};
}

// SurfaceFluxRestoring materialised at interior cell k: J_add = v_p (Sₒ − S★) where wet, 0 elsewhere
__device__ __forceinline__ double salinity_restoring_cell(bool wet, double vp, double So, const double* __restrict__ target, size_t k) {
    return wet ? vp * (So - target[k]) : 0.0;
}

// S★ of a staged dataset (cf_dataset_*) between two of its levels: blend_levels' expression on doubles.  Every reader of a
// blended S★ calls this one function and holds the result in a named variable before using it, so that the expression is
// rounded the same way whatever follows it.
__device__ __forceinline__ double dataset_blend(double a, double b, double f) { return b * f + a * (1.0 - f); }

// S★ at element k: level1's value when the fraction is 0.0 (level2 is not read), else the blend
__device__ __forceinline__ double dataset_target_cell(const double* __restrict__ level1, const double* __restrict__ level2, double fraction,
                                                      size_t k) {
    if (fraction == 0.0) return level1[k];
    const double target = dataset_blend(level1[k], level2[k], fraction);
    return target;
}

// the two-level form of the restoring cell: S★ formed from a dataset's two levels (fraction 0.0: the one-level form on level1)
__device__ __forceinline__ double salinity_restoring_cell(bool wet, double vp, double So, const double* __restrict__ level1,
                                                          const double* __restrict__ level2, double fraction, size_t k) {
    if (fraction == 0.0) return salinity_restoring_cell(wet, vp, So, level1, k);
    if (!wet) return 0.0;
    const double target = dataset_blend(level1[k], level2[k], fraction);
    return vp * (So - target);
}

}  // namespace coflux
