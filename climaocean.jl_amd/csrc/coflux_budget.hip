// coflux_budget.hip — the net heat and salt flux budget averaged in the collection launch (cf_average_create_budget,
// include/coflux.h has the kinds, their order of operations and the footprint).
//
// One launch per collection covers every term; the geometry is coflux_derived.hip's without its neighbours: a work item is
// an interior cell c = j · nx + i, consecutive lanes hold consecutive cells, the grid is capped and the rest is strided.
//   * The inputs of compute_net_ocean_fluxes!'s cell have a fixed numbering (BudgetInput); the host leaves a NULL where no
//     requested kind reads an input, so a cell loads exactly the arrays the table's "reads" column names, each ONCE, and
//     sees 0.0 for the others.  Pointers, scales, kinds and means live in the kernel arguments (SGPRs); the input and term
//     loops are unrolled, so they have static indices.
//   * Every load of the cell — inputs, mask, latitude, means — is issued before anything waits for one.
//   * budget_cell (coflux_budget_cell.hpp) evaluates every part in registers; a term picks its part out of the 16-wide
//     register vector with its (uniform) kind — register-relative moves, no scratch, no LDS.
//   * Land (cell_is_wet, both mask kinds) is a select on the part: the sample is 0.0 · scale, as net_flux_kernel stores 0.0.
// Every operation of a sample is rounded on its own (contraction off) so that NumPy restates it bit for bit; the sample
// enters the mean through `blend` of coflux_surface_cells.hpp.  STORE: the first collection of a window never reads the mean.
#include <algorithm>

#include "coflux_budget_cell.hpp"
#include "coflux_kernel_types.hpp"
#include "coflux_kernels.h"
#include "coflux_surface_cells.hpp"

namespace coflux {

namespace {

constexpr int BUDGET_BLOCK = 256;
#ifndef COFLUX_BUDGET_MAX_BLOCKS
#define COFLUX_BUDGET_MAX_BLOCKS 2048        // memory-bound: cap the grid and stride the rest (scheduling only; A/B builds may set it)
#endif
constexpr int BUDGET_MAX_BLOCKS = COFLUX_BUDGET_MAX_BLOCKS;

template <int K, bool STORE>
__global__ __launch_bounds__(BUDGET_BLOCK) void budget_average_kernel(DevParams P, GridDesc G, BudgetArgs A, unsigned cells, double c_prev,
                                                                       double c_new) {
    typedef double vec __attribute__((ext_vector_type(K)));
    const unsigned stride = gridDim.x * BUDGET_BLOCK;
    const unsigned nx = (unsigned)G.nx;
    WeightDesc Wt{};
    Wt.latitude = A.latitude;
    Wt.separable = A.separable;
    for (unsigned base = blockIdx.x * BUDGET_BLOCK; base < cells; base += stride) {   // uniform per workgroup
        const unsigned q = base + threadIdx.x;
        const bool on = q < cells;
        const unsigned j = on ? q / nx : 0u, i = on ? q - j * nx : 0u;
        const size_t k = (size_t)(j + (unsigned)G.hy) * (size_t)G.sj + (size_t)G.hx + (size_t)i;
        // every load of the cell goes out before anything waits for one
        double v[BUDGET_INPUTS];
#pragma unroll
        for (int s = 0; s < BUDGET_INPUTS; ++s) {
            double t = 0.0;
            if (A.in[s] != nullptr && on) t = A.in[s][k];
            v[s] = t;
        }
        double phi = 0.0;
        if (A.reads_albedo && on) phi = ocean_latitude_cell(P, Wt, G, (int)j, k);
        vec mv = 0.0;
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
        // the mask's load is the last one out: cell_is_wet compares as soon as it has it
        const bool wet = on ? cell_is_wet(P, A.mask, k) : false;
        // (an empty statement that holds the latitude: without it the compiler sinks the albedo's first products into the
        // block of the latitude's load and waits there, in front of the means' loads)
        asm volatile("" : "+v"(phi));
        double alb = 0.0;
        if (A.reads_albedo) alb = ocean_albedo_cell(P, phi);
        const BudgetParts X = budget_cell(P, alb, v[BUDGET_IN_ICE], v[BUDGET_IN_S], v[BUDGET_IN_TS] + P.T_offset, v[BUDGET_IN_MP],
                                          v[BUDGET_IN_QS], v[BUDGET_IN_QL], v[BUDGET_IN_QC], v[BUDGET_IN_QV], v[BUDGET_IN_MV],
                                          v[BUDGET_IN_QIO], v[BUDGET_IN_JSIO], v[BUDGET_IN_LAND], v[BUDGET_IN_FRAZIL]);
#pragma unroll
        for (int t = 0; t < K; ++t) {
            if (t < A.n_terms) {
                const double x = wet ? X[A.kind[t]] : 0.0;
                double sample;
                {
#pragma clang fp contract(off)
                    sample = x * A.scale[t];
                }
                const double out = STORE ? sample : blend(mv[t], sample, c_prev, c_new);
                if (on) A.mean[t][k] = out;
            }
        }
    }
}

template <int K>
void launch_bucket(hipStream_t st, int blocks, const DevParams& P, const BudgetArgs& A, const GridDesc& G, unsigned cells, bool store,
                   double c_prev, double c_new) {
    if (store)
        hipLaunchKernelGGL((budget_average_kernel<K, true>), dim3(blocks), dim3(BUDGET_BLOCK), 0, st, P, G, A, cells, c_prev, c_new);
    else
        hipLaunchKernelGGL((budget_average_kernel<K, false>), dim3(blocks), dim3(BUDGET_BLOCK), 0, st, P, G, A, cells, c_prev, c_new);
}

}  // namespace

hipError_t launch_budget_average(hipStream_t st, const DevParams& P, const BudgetArgs& A, const GridDesc& G, bool store, double c_prev,
                                 double c_new) {
    const unsigned long long cells = (unsigned long long)G.nx * (unsigned long long)G.ny;
    if (G.nx < 1 || G.ny < 1 || cells + (unsigned long long)BUDGET_MAX_BLOCKS * BUDGET_BLOCK >= (1ull << 32)) return hipErrorInvalidValue;
    const int cap = A.max_blocks > 0 ? std::min(A.max_blocks, BUDGET_MAX_BLOCKS) : BUDGET_MAX_BLOCKS;
    const int blocks = (int)std::min<unsigned long long>((cells + BUDGET_BLOCK - 1) / BUDGET_BLOCK, (unsigned long long)cap);
    if (A.n_terms <= 4)
        launch_bucket<4>(st, blocks, P, A, G, (unsigned)cells, store, c_prev, c_new);
    else if (A.n_terms <= 8)
        launch_bucket<8>(st, blocks, P, A, G, (unsigned)cells, store, c_prev, c_new);
    else
        launch_bucket<16>(st, blocks, P, A, G, (unsigned)cells, store, c_prev, c_new);
    return hipGetLastError();
}

}  // namespace coflux
