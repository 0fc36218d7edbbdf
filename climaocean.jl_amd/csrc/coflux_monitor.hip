// coflux_monitor.hip — surface extrema, non-finite counts and state hashes (cf_monitor_*, include/coflux.h).
//
// One collection turns up to CF_MONITOR_MAX_ENTRIES entries (field x, kind) into one record of cf_monitor_value: minimum and
// maximum of y = x | |x| over the wet interior cells whose x is not NaN with the smallest cell index that holds each, the
// counts of NaN and ±Inf wet cells with the smallest index of either, and the hash of the raw bits of ALL interior cells.
//
// Every one of the eight quantities is an exact, associative and commutative reduction — a minimum / maximum of the
// order-preserving integer key of the bits with the cell index as tie-break, integer sums, a minimum of indices, a wrapping
// 64-bit sum — so the partition of the cells is free and is chosen for bandwidth: no fixed summation order, no
// floating-point comparison (v_min_f64 / v_max_f64 treat NaN and ±0 by a mode), no floating-point or other atomics.
//   1. the interior is walked row by row, local cell j·nx + i, and cut into pairs (2p, 2p + 1); the record holds the global
//      number c = first_cell + j·row_length + i of a cell (row_length = nx unless the context is a tile of a wider surface);
//   2. the work is (entry, slice): slice s of `slices` owns the pairs p ≡ s·256 + t (mod slices·256), thread t keeps the
//      entry's eight running values in registers over that stride;
//   3. the 64 lanes of a wave are merged by a butterfly, the four waves through LDS → partial[entry][slice] (64 bytes);
//   4. a second, single-workgroup launch merges an entry's partials (one wave per entry, four entries at a time), turns the
//      keys back into doubles, writes the record, and its thread 0 — alone, after a barrier — updates the status.
// A workgroup loops over the (entry, slice) items with a stride of gridDim, so a capped launch computes the same partials.
// Alignment only chooses the width of the loads (one 16-byte access where a thread's two cells lie in one row and the
// array's address there is 16-byte aligned, two 8-byte accesses otherwise), never the cells a thread owns.
// Traffic: 8 bytes per cell and entry, each field cell loaded once per collection; the mask is read once per ENTRY, not once
// per cell (n_entries · (1 | 8) bytes per cell: the price of one entry per workgroup, which keeps the running values at 16
// registers).  Excluded cells are selected away: only the hash reads them.
// The pair of cells, its loads and its wet test are coflux_surface_cells.hpp's.
#include <algorithm>

#include "coflux_kernel_types.hpp"
#include "coflux_kernels.h"
#include "coflux_surface_cells.hpp"

namespace coflux {

namespace {

constexpr int MONITOR_BLOCK = 256;
constexpr int MONITOR_WAVES = MONITOR_BLOCK / 64;
constexpr int MONITOR_TARGET_BLOCKS = 2048;      // workgroups of an uncapped launch: eight waves per SIMD on 256 compute units
constexpr uint64_t SIGN_BIT = 0x8000000000000000ull, EXPONENT = 0x7FF0000000000000ull, HASH_K = 0x9E3779B97F4A7C15ull;
constexpr int64_t NO_CELL = INT64_MAX;

__device__ __forceinline__ uint64_t mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// the IEEE total order of the non-NaN doubles as an unsigned order: negative values flip all bits, the others the sign bit
__device__ __forceinline__ uint64_t order_key(uint64_t bits) { return bits ^ ((uint64_t)((int64_t)bits >> 63) | SIGN_BIT); }
__device__ __forceinline__ uint64_t key_bits(uint64_t key) { return key ^ ((key & SIGN_BIT) ? SIGN_BIT : ~0ull); }

__device__ __forceinline__ MonitorPartial empty_partial() {
    return MonitorPartial{~0ull, 0ull, NO_CELL, NO_CELL, 0, 0, NO_CELL, 0ull};
}

// (by value: a conditional between two members is a conditional between two addresses, which keeps the aggregate in memory)
template <class T>
__device__ __forceinline__ T pick(bool c, T a, T b) {
    return c ? a : b;
}

__device__ __forceinline__ void merge(MonitorPartial& A, const MonitorPartial B) {
    const bool lower = B.key_min < A.key_min || (B.key_min == A.key_min && B.argmin < A.argmin);
    A.key_min = pick(lower, B.key_min, A.key_min);
    A.argmin = pick(lower, B.argmin, A.argmin);
    const bool higher = B.key_max > A.key_max || (B.key_max == A.key_max && B.argmax < A.argmax);
    A.key_max = pick(higher, B.key_max, A.key_max);
    A.argmax = pick(higher, B.argmax, A.argmax);
    A.nan_count += B.nan_count;
    A.inf_count += B.inf_count;
    A.first_nonfinite = pick(B.first_nonfinite < A.first_nonfinite, B.first_nonfinite, A.first_nonfinite);
    A.hash += B.hash;
}

// one interior cell: `bits` of x, global index c, `counted`: inside the interior and wet
__device__ __forceinline__ void take(MonitorPartial& R, uint64_t bits, int64_t c, bool counted, bool absolute) {
    const uint64_t magnitude = bits & ~SIGN_BIT;
    const bool nan = magnitude > EXPONENT, inf = magnitude == EXPONENT;
    R.nan_count += (counted && nan) ? 1 : 0;
    R.inf_count += (counted && inf) ? 1 : 0;
    R.first_nonfinite = pick((counted && (nan || inf) && c < R.first_nonfinite), c, R.first_nonfinite);
    const uint64_t key = order_key(absolute ? magnitude : bits);
    const bool ordered = counted && !nan;
    const bool lower = ordered && (key < R.key_min || (key == R.key_min && c < R.argmin));
    R.key_min = pick(lower, key, R.key_min);
    R.argmin = pick(lower, c, R.argmin);
    const bool higher = ordered && (key > R.key_max || (key == R.key_max && c < R.argmax));
    R.key_max = pick(higher, key, R.key_max);
    R.argmax = pick(higher, c, R.argmax);
}

// 64-bit values cross the lanes as two 32-bit halves, and partials cross memory word by word: no aggregate ever has its address
// taken, so the running values stay in registers (no scratch)
__device__ __forceinline__ uint64_t shfl_xor64(uint64_t v, int off) {
    const unsigned lo = __shfl_xor((unsigned)v, off, 64), hi = __shfl_xor((unsigned)(v >> 32), off, 64);
    return (uint64_t)hi << 32 | lo;
}

__device__ __forceinline__ MonitorPartial wave_merge(MonitorPartial R) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        MonitorPartial O;
        O.key_min = shfl_xor64(R.key_min, off);
        O.key_max = shfl_xor64(R.key_max, off);
        O.argmin = (int64_t)shfl_xor64((uint64_t)R.argmin, off);
        O.argmax = (int64_t)shfl_xor64((uint64_t)R.argmax, off);
        O.nan_count = (int64_t)shfl_xor64((uint64_t)R.nan_count, off);
        O.inf_count = (int64_t)shfl_xor64((uint64_t)R.inf_count, off);
        O.first_nonfinite = (int64_t)shfl_xor64((uint64_t)R.first_nonfinite, off);
        O.hash = shfl_xor64(R.hash, off);
        merge(R, O);
    }
    return R;
}

__device__ __forceinline__ MonitorPartial get_partial(const MonitorPartial* p) {
    const uint64_t* w = reinterpret_cast<const uint64_t*>(p);
    return MonitorPartial{w[0], w[1], (int64_t)w[2], (int64_t)w[3], (int64_t)w[4], (int64_t)w[5], (int64_t)w[6], w[7]};
}
__device__ __forceinline__ void put_partial(MonitorPartial* p, const MonitorPartial& R) {
    uint64_t* w = reinterpret_cast<uint64_t*>(p);
    w[0] = R.key_min, w[1] = R.key_max, w[2] = (uint64_t)R.argmin, w[3] = (uint64_t)R.argmax;
    w[4] = (uint64_t)R.nan_count, w[5] = (uint64_t)R.inf_count, w[6] = (uint64_t)R.first_nonfinite, w[7] = R.hash;
}

__global__ __launch_bounds__(MONITOR_BLOCK) void monitor_pass_kernel(MonitorArgs K, GridDesc G, unsigned n_cells, unsigned n_pairs) {
    __shared__ MonitorPartial wave_part[MONITOR_WAVES];
    const unsigned t = threadIdx.x;
    const unsigned slices = (unsigned)K.slices, items = (unsigned)K.n_entries * slices;
    for (unsigned item = blockIdx.x; item < items; item += gridDim.x) {
        const unsigned e = item / slices, slice = item - e * slices;
        const MonitorEntry E = K.entry[e];                  // uniform: scalar loads
        const bool absolute = E.kind == CF_MONITOR_ABS;
        MonitorPartial R = empty_partial();
        for (unsigned p = slice * (unsigned)MONITOR_BLOCK + t; p < n_pairs; p += slices * (unsigned)MONITOR_BLOCK) {
            const unsigned c0 = 2u * p;                      // p < n_pairs: c0 < n_cells
            const CellPair C = cell_pair<false>(c0, n_cells, G);
            const bool v1 = C.v1;
            const ulonglong2 x = load_pair_bits(E.a, C);
            const PairWet wet = pair_wet(K.mask, K.mask_kind, K.z_surface, C);
            // each cell is numbered from its own (i, j): the pair that wraps starts row j + 1 of the global numbering
            const int64_t row = K.first_cell + (int64_t)C.j0 * (int64_t)K.row_length;
            const int64_t c = row + (int64_t)C.i0, c1 = C.wrap ? row + (int64_t)K.row_length : c + 1;
            R.hash += mix64(x.x ^ (HASH_K * (uint64_t)(c + 1)));
            take(R, x.x, c, wet.s0, absolute);
            if (v1) R.hash += mix64(x.y ^ (HASH_K * (uint64_t)(c1 + 1)));
            take(R, x.y, c1, wet.s1, absolute);
        }
        R = wave_merge(R);
        if ((t & 63u) == 0u) put_partial(&wave_part[t >> 6], R);
        __syncthreads();
        if (t == 0) {
            MonitorPartial S = get_partial(&wave_part[0]);
#pragma unroll
            for (int w = 1; w < MONITOR_WAVES; ++w) merge(S, get_partial(&wave_part[w]));
            put_partial(&K.partial[item], S);
        }
        __syncthreads();
    }
}

// record[e] from the partials of entry e (one wave per entry), then the status by thread 0 alone
__global__ __launch_bounds__(MONITOR_BLOCK) void monitor_combine_kernel(MonitorArgs K, cf_monitor_value* __restrict__ record,
                                                                        long long record_index) {
    __shared__ unsigned bad[CF_MONITOR_MAX_ENTRIES];
    const unsigned t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    if (t < CF_MONITOR_MAX_ENTRIES) bad[t] = 0u;
    __syncthreads();
    for (unsigned e = wave; e < (unsigned)K.n_entries; e += MONITOR_WAVES) {
        MonitorPartial R = empty_partial();
        for (unsigned s = lane; s < (unsigned)K.slices; s += 64u) merge(R, get_partial(&K.partial[(size_t)e * (size_t)K.slices + s]));
        R = wave_merge(R);
        if (lane == 0u) {
            cf_monitor_value V;
            const bool none_min = R.argmin == NO_CELL, none_max = R.argmax == NO_CELL;
            V.minimum = __longlong_as_double((long long)(none_min ? EXPONENT : key_bits(R.key_min)));               // +Inf
            V.maximum = __longlong_as_double((long long)(none_max ? (EXPONENT | SIGN_BIT) : key_bits(R.key_max)));  // −Inf
            V.argmin = none_min ? -1 : R.argmin;
            V.argmax = none_max ? -1 : R.argmax;
            V.nan_count = R.nan_count;
            V.inf_count = R.inf_count;
            V.first_nonfinite = R.first_nonfinite == NO_CELL ? -1 : R.first_nonfinite;
            V.hash = R.hash;
            record[e] = V;
            bad[e] = (R.nan_count + R.inf_count) > 0 ? 1u : 0u;
        }
    }
    __syncthreads();
    if (t == 0) {
        unsigned entries = 0u;
        for (int e = 0; e < K.n_entries; ++e) entries |= bad[e] << e;
        if (entries != 0u && K.status->first_bad_plus_one == 0) {
            K.status->first_bad_plus_one = record_index + 1;
            K.status->bad_entries = entries;
        }
    }
}

}  // namespace

int monitor_slices(const GridDesc& G, int n_entries) {
    const unsigned long long cells = (unsigned long long)G.nx * (unsigned long long)G.ny, pairs = (cells + 1) / 2;
    const unsigned long long whole = (pairs + MONITOR_BLOCK - 1) / MONITOR_BLOCK;          // one pair per thread
    const unsigned long long share = (unsigned long long)std::max(1, MONITOR_TARGET_BLOCKS / std::max(n_entries, 1));
    return (int)std::max(1ull, std::min(whole, share));
}

hipError_t launch_monitor(hipStream_t st, const MonitorArgs& K, const GridDesc& G, cf_monitor_value* record, int64_t record_index,
                          int max_blocks) {
    const unsigned n_cells = (unsigned)G.nx * (unsigned)G.ny, n_pairs = (n_cells + 1u) / 2u;
    const unsigned items = (unsigned)K.n_entries * (unsigned)K.slices;
    const unsigned blocks = max_blocks > 0 ? std::min(items, (unsigned)max_blocks) : items;
    hipLaunchKernelGGL(monitor_pass_kernel, dim3(blocks), dim3(MONITOR_BLOCK), 0, st, K, G, n_cells, n_pairs);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(monitor_combine_kernel, dim3(1), dim3(MONITOR_BLOCK), 0, st, K, record, (long long)record_index);
    return hipGetLastError();
}

}  // namespace coflux
