// coflux_exact_sum.hip — NormalizeSalinity's two sums, exact (include/coflux.h: cf_normalize_salinity_flux_exact; the format and
// the rounding: coflux_exact_sum.hpp).  Σ t and Σ a over the wet interior, t = fl(fl(flux + additional) · a), are integer sums of
// 32-bit pieces: their bits depend on no workgroup, no slab and no order of arrival.
//
//   exact_sums_kernel    one pass over the interior.  A wave splits its 64 terms into pieces and adds up, per distinct first
//                        digit among them (the terms of a real field cluster in two or three), the pieces of the lanes that share
//                        it — integer shuffles —; one lane then adds the three totals to the workgroup's digits in LDS (64-bit
//                        integer LDS atomics).  At its end the workgroup adds its non-zero digits to the context's accumulator
//                        pair (64-bit integer global atomics).  No floating-point atomic anywhere.
//   exact_finish_kernel  one workgroup: takes the accumulator pair (and zeroes it for the next call), sends it to every other
//                        rank of the reduction world and adds theirs (HIP-IPC mailboxes, the protocol of the halo rows:
//                        coflux_halo_device.hpp), carries and rounds once: sums[0] = fl(Σ t), sums[1] = fl(Σ a).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "coflux_exact_sum.hpp"
#include "coflux_halo_device.hpp"
#include "coflux_kernel_types.hpp"
#include "coflux_kernels.h"

// t = fl(fl(flux + additional) · a): two roundings, never a fused multiply-add
#pragma clang fp contract(off)

namespace coflux {

constexpr int XS_BLOCK = 256;
constexpr int XS_NO_TERM = 1 << 20;   // a lane without a term (land, beyond the interior, a zero)

__device__ __forceinline__ long long wave_sum(long long x) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m);
    return x;
}

// the wave's terms `x` (of the lanes with `active`) into the accumulator `acc` (XS_WORDS words of LDS).  Called by whole waves.
__device__ __forceinline__ void wave_accumulate(unsigned long long* acc, bool active, double x) {
    const XsTerm T = xs_split(x);
    const int lane = (int)(threadIdx.x & 63);
    int first = active ? T.first : XS_NO_TERM;
    if (first >= 0 && (T.piece[0] | T.piece[1] | T.piece[2]) == 0) first = XS_NO_TERM;
    unsigned long long todo = __ballot(first != XS_NO_TERM);
    while (todo) {   // (wave-uniform: one round per distinct first digit, or kind of non-number, among the lanes)
        const int f = __shfl(first, __ffsll((long long)todo) - 1);
        const bool mine = first == f;
        const unsigned long long who = __ballot(mine);
        if (f < 0) {
            if (lane == 0)
                __hip_atomic_fetch_add(&acc[XS_DIGITS + (-1 - f)], (unsigned long long)__popcll(who), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        } else {
            // 64 pieces below 2³² each: the totals stay below 2³⁸
            const long long p0 = wave_sum(mine ? (long long)T.piece[0] : 0ll);
            const long long p1 = wave_sum(mine ? (long long)T.piece[1] : 0ll);
            const long long p2 = wave_sum(mine ? (long long)T.piece[2] : 0ll);
            if (lane == 0) {   // f + 2 ≤ 66 (xs_add)
                if (p0) __hip_atomic_fetch_add(&acc[f], (unsigned long long)p0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (p1) __hip_atomic_fetch_add(&acc[f + 1], (unsigned long long)p1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (p2) __hip_atomic_fetch_add(&acc[f + 2], (unsigned long long)p2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
        todo &= ~who;
    }
}

__global__ __launch_bounds__(XS_BLOCK) void exact_sums_kernel(DevParams P, GridDesc G, const double* __restrict__ flux,
                                                              const double* __restrict__ additional, const double* __restrict__ area,
                                                              const void* mask, unsigned long long* __restrict__ accumulator) {
    __shared__ unsigned long long digits[REDUCE_SLOT_WORDS];   // the pair: Σ t, then Σ a
    const int tid = (int)threadIdx.x;
    if (tid < REDUCE_SLOT_WORDS) digits[tid] = 0;
    __syncthreads();
    const long long ncells = (long long)G.nx * G.ny, stride = (long long)gridDim.x * XS_BLOCK;
    for (long long base = (long long)blockIdx.x * XS_BLOCK; base < ncells; base += stride) {   // (uniform: whole waves go round)
        const long long idx = base + tid;
        bool wet = false;
        double t = 0.0, a = 0.0;
        if (idx < ncells) {
            const int j = (int)(idx / G.nx), i = (int)(idx - (long long)j * G.nx);
            const size_t k = cell_index(G, i, j);
            wet = cell_is_wet(P, mask, k);
            if (wet) {   // land and halo cells are selected away, never multiplied: they may hold NaN
                a = area ? area[k] : 1.0;
                const double v = additional ? flux[k] + additional[k] : flux[k];
                t = v * a;
            }
        }
        wave_accumulate(digits, wet, t);
        wave_accumulate(digits + XS_WORDS, wet, a);
    }
    __syncthreads();
    if (tid < REDUCE_SLOT_WORDS) {
        const unsigned long long d = digits[tid];
        if (d) __hip_atomic_fetch_add(&accumulator[tid], d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__device__ __forceinline__ unsigned long long* reduce_flag(char* base, int parity, int rank) {
    return reinterpret_cast<unsigned long long*>(base + REDUCE_FLAG_OFFSET) + (parity * REDUCE_MAX_RANKS + rank) * 8;   // a 64-byte line each
}
__device__ __forceinline__ unsigned long long* reduce_slot(char* base, int parity, int rank) {
    return reinterpret_cast<unsigned long long*>(base + REDUCE_SLOT_OFFSET) + (size_t)(parity * REDUCE_MAX_RANKS + rank) * REDUCE_SLOT_WORDS;
}

// One workgroup.  With W.nranks > 1, reduction number `seq` of this context (every rank issues the same number of them):
//   (i)   my pair → slot [parity][my rank] of every other rank's mailbox, system-scope fence;
//   (ii)  lane r publishes seq in rank r's flag [parity][my rank] (system-scope release) and then
//   (iii) waits (bounded, sleeping) for rank r's number in my own mailbox;
//   (iv)  the others' slots are added to mine digit-wise.  A rank publishes seq + 1 only after it has read every slot of seq, and
//         it writes a slot of seq + 2 only after it has seen every flag of seq + 1: two parities are enough.
// On a timeout the sticky status is set (the next cf_sync reports CF_ERR_COMM) and the kernel ends with this rank's own sums.
__global__ __launch_bounds__(XS_BLOCK) void exact_finish_kernel(unsigned long long* __restrict__ accumulator, ReduceWorld W,
                                                                unsigned long long seq, int* __restrict__ status,
                                                                double* __restrict__ sums, unsigned long long* __restrict__ nonfinite) {
    __shared__ unsigned long long digits[REDUCE_SLOT_WORDS];
    __shared__ int ok;
    const int tid = (int)threadIdx.x;
    if (tid < REDUCE_SLOT_WORDS) {
        digits[tid] = accumulator[tid];
        accumulator[tid] = 0;
    }
    if (tid == 0) ok = 1;
    __syncthreads();
    if (W.nranks > 1) {
        const int parity = (int)(seq & 1ull);
        if (tid < REDUCE_SLOT_WORDS)
            for (int r = 0; r < W.nranks; ++r)
                if (r != W.rank) reduce_slot(W.peers[r], parity, W.rank)[tid] = digits[tid];
        __threadfence_system();
        __syncthreads();
        if (tid < W.nranks && tid != W.rank) {
            __hip_atomic_store(reduce_flag(W.peers[tid], parity, W.rank), seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            unsigned long long* flag = reduce_flag(W.mine, parity, tid);
            unsigned long long spins = 0;
            while (__hip_atomic_load(flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) < seq) {
                __builtin_amdgcn_s_sleep(8);
                if (++spins > PEER_SPIN_LIMIT) {
                    atomicExch(&ok, 0);
                    atomicExch(status, 3);   // sticky: reported by the next cf_sync
                    break;
                }
            }
        }
        __syncthreads();
        if (ok) {
            __atomic_thread_fence(__ATOMIC_ACQUIRE);  // system scope: nothing cached of the mailbox survives the flags
            if (tid < REDUCE_SLOT_WORDS) {
                unsigned long long d = digits[tid];
                for (int r = 0; r < W.nranks; ++r)
                    if (r != W.rank) d += reduce_slot(W.mine, parity, r)[tid];
                digits[tid] = d;
            }
        }
        __syncthreads();
    }
    if (nonfinite && tid < XS_COUNTERS) nonfinite[tid] = digits[XS_DIGITS + tid];
    if (tid == 0 || tid == 64) {   // one lane of two waves: Σ t and Σ a are carried and rounded side by side
        unsigned long long* A = digits + (tid ? XS_WORDS : 0);
        sums[tid ? 1 : 0] = xs_round_digits(reinterpret_cast<int64_t*>(A), reinterpret_cast<const uint64_t*>(A + XS_DIGITS));
    }
}

hipError_t launch_exact_sums(hipStream_t st, const DevParams& P, const GridDesc& G, const double* flux, const double* additional,
                             const double* area, const void* mask, unsigned long long* accumulator) {
    const long long ncells = (long long)G.nx * G.ny;
    const int nblocks = (int)std::max(1ll, std::min((long long)EXACT_SUM_BLOCKS, (ncells + XS_BLOCK - 1) / XS_BLOCK));
    hipLaunchKernelGGL(exact_sums_kernel, dim3(nblocks), dim3(XS_BLOCK), 0, st, P, G, flux, additional, area, mask, accumulator);
    return hipGetLastError();
}

hipError_t launch_exact_finish(hipStream_t st, unsigned long long* accumulator, const ReduceWorld& W, unsigned long long seq, int* d_status,
                               double* sums, unsigned long long* nonfinite) {
    hipLaunchKernelGGL(exact_finish_kernel, dim3(1), dim3(XS_BLOCK), 0, st, accumulator, W, seq, d_status, sums, nonfinite);
    return hipGetLastError();
}

}  // namespace coflux
