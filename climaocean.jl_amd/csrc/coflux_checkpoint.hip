// coflux_checkpoint.hip — the pack kernel of the checkpoint (cf_checkpoint_capture / _restore, include/coflux.h).
//
// One launch moves every device section of a checkpoint between its own array and the packed image, and forms every section's
// hash on the way.  The image is cut into tiles of CHECKPOINT_TILE_BYTES; workgroups take tiles with a stride of gridDim, so a
// capped launch does the same work.  A tile looks up the first segment that meets it (the host's table) and walks the segments
// until one starts behind its end; of each it takes the 16-byte chunks that lie inside the tile, one chunk per thread and turn.
//   body   a chunk wholly inside the segment: one 16-byte access on the image side (always 16-byte aligned), and on the section
//          side one 16-byte access where the section's base is 16-byte aligned, two 8-byte accesses where it is only 8-byte
//          aligned (the k-th slab of a 3-D field with an odd plane size);
//   tail   the segment's last chunk when its length is no multiple of 16: the section side byte by byte, never beyond its
//          last byte; the image side whole, the padding written as zeros.
// Hash: every 8-byte word w at index k of its section adds mix64(w XOR K·(k + 1)) — the surface monitor's mixer — to the lane's
// wrapping sum; the lanes of a wave are summed by a butterfly, the four waves through LDS, and thread 0 adds the workgroup's
// sum to the section's hash word with ONE 64-bit integer atomic.  A wrapping integer sum is exact, associative and commutative:
// the hash depends on the bytes alone — not on the tile size, the launched grid, the CU count or the form that ran.  No
// floating-point atomics.
// One body, three forms (template argument): PACK section → image, HASH_ONLY section → nothing, UNPACK image → section (the hash
// is then of what was written).  PACK's image stores come in two forms (`NT`): streaming stores as in
// coflux_solver_shared.hpp::gstore_final, the default — the image is read next by the copy engine, not by a kernel — and plain
// stores, which measured the same within the rounds' spread (the host picks the form, the bytes are the same).
#include <algorithm>

#include "coflux_checkpoint.hpp"

namespace coflux {

namespace {

constexpr int CK_BLOCK = 256;
constexpr int CK_WAVES = CK_BLOCK / 64;
constexpr int CK_TARGET_BLOCKS = 2048;   // workgroups of an uncapped launch: eight waves per SIMD on 256 compute units
constexpr uint64_t CK_HASH_K = 0x9E3779B97F4A7C15ull;

typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
#define CK_GLOBAL __attribute__((address_space(1)))

__device__ __forceinline__ uint64_t ck_mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__device__ __forceinline__ uint64_t ck_shfl_xor64(uint64_t v, int off) {
    const unsigned lo = __shfl_xor((unsigned)v, off, 64), hi = __shfl_xor((unsigned)(v >> 32), off, 64);
    return (uint64_t)hi << 32 | lo;
}

// 16 bytes of a section at an 8-byte aligned address: one access where `wide` (the address is 16-byte aligned), else two
__device__ __forceinline__ u64x2 section_load(const unsigned char* p, bool wide) {
    if (wide) return *(const CK_GLOBAL u64x2*)p;
    const CK_GLOBAL unsigned long long* q = (const CK_GLOBAL unsigned long long*)p;
    u64x2 v;
    v.x = q[0];
    v.y = q[1];
    return v;
}
__device__ __forceinline__ void section_store(unsigned char* p, bool wide, u64x2 v) {
    if (wide) {
        *(CK_GLOBAL u64x2*)p = v;
    } else {
        CK_GLOBAL unsigned long long* q = (CK_GLOBAL unsigned long long*)p;
        q[0] = v.x;
        q[1] = v.y;
    }
}

template <int FORM, bool NT>
__global__ __launch_bounds__(CK_BLOCK) void checkpoint_pack_kernel(const CheckpointSegment* __restrict__ segments, uint32_t n_segments,
                                                                   const uint32_t* __restrict__ tile_first, uint32_t n_tiles,
                                                                   unsigned char* __restrict__ image, unsigned long long* __restrict__ hash) {
    __shared__ unsigned long long wave_sum[CK_WAVES];
    const unsigned t = threadIdx.x;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t tile_lo = (uint64_t)tile * CHECKPOINT_TILE_BYTES, tile_hi = tile_lo + CHECKPOINT_TILE_BYTES;
        for (uint32_t s = tile_first[tile]; s < n_segments; ++s) {
            const CheckpointSegment S = segments[s];   // uniform: scalar loads
            if (S.image_offset >= tile_hi) break;
            const uint64_t end = S.image_offset + ((S.bytes + 15ull) & ~15ull);
            const uint64_t lo = S.image_offset > tile_lo ? S.image_offset : tile_lo, hi = end < tile_hi ? end : tile_hi;
            const unsigned chunks = hi > lo ? (unsigned)((hi - lo) >> 4) : 0u;   // ≤ CHECKPOINT_TILE_BYTES / 16
            const uint64_t p0 = lo - S.image_offset;                             // of the first chunk, within the segment
            const bool wide = ((uintptr_t)S.ptr & 15u) == 0u;
            uint64_t sum = 0;
            for (unsigned c = t; c < chunks; c += CK_BLOCK) {
                const uint64_t p = p0 + 16ull * c;       // a multiple of 16 below round16(bytes): p < bytes
                const uint64_t left = S.bytes - p;       // bytes of the section from p on: ≥ 1
                unsigned char* sec = S.ptr + p;
                unsigned char* img = FORM == CHECKPOINT_HASH_ONLY ? nullptr : image + (lo + 16ull * c);
                u64x2 v;
                if (left >= 16) {
                    if (FORM == CHECKPOINT_UNPACK) {
                        v = *(const CK_GLOBAL u64x2*)img;
                        section_store(sec, wide, v);
                    } else {
                        v = section_load(sec, wide);
                    }
                } else if (FORM == CHECKPOINT_UNPACK) {
                    v = *(const CK_GLOBAL u64x2*)img;
                    // (the padding of a verified image is zero; the hash is of the bytes written)
                    const unsigned bits_x = left >= 8 ? 64u : 8u * (unsigned)left, bits_y = left > 8 ? 8u * (unsigned)(left - 8) : 0u;
                    v.x = bits_x == 64u ? v.x : v.x & ((1ull << bits_x) - 1ull);
                    v.y = bits_y == 0u ? 0ull : v.y & ((1ull << bits_y) - 1ull);
#pragma unroll
                    for (unsigned b = 0; b < 15; ++b)
                        if (b < left) ((CK_GLOBAL unsigned char*)sec)[b] = (unsigned char)((b < 8 ? v.x : v.y) >> (8u * (b & 7u)));
                } else {
                    v.x = 0ull;
                    v.y = 0ull;
#pragma unroll
                    for (unsigned b = 0; b < 15; ++b)
                        if (b < left) {
                            const unsigned long long byte = ((const CK_GLOBAL unsigned char*)sec)[b];
                            if (b < 8) v.x |= byte << (8u * b);
                            else v.y |= byte << (8u * (b - 8u));
                        }
                }
                if (FORM == CHECKPOINT_PACK) {
                    if (NT) __builtin_nontemporal_store(v, (CK_GLOBAL u64x2*)img);
                    else *(CK_GLOBAL u64x2*)img = v;
                }
                const uint64_t k = S.first_word + (p >> 3);
                sum += ck_mix64(v.x ^ (CK_HASH_K * (k + 1)));
                if (left > 8) sum += ck_mix64(v.y ^ (CK_HASH_K * (k + 2)));
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) sum += ck_shfl_xor64(sum, off);
            if ((t & 63u) == 0u) wave_sum[t >> 6] = sum;
            __syncthreads();
            if (t == 0) {
                unsigned long long total = wave_sum[0];
#pragma unroll
                for (int w = 1; w < CK_WAVES; ++w) total += wave_sum[w];
                atomicAdd(&hash[S.section], total);
            }
            __syncthreads();
        }
    }
}

template <int FORM, bool NT>
hipError_t launch_form(hipStream_t st, unsigned blocks, const CheckpointSegment* d_segments, uint32_t n_segments, const uint32_t* d_tile_first,
                       uint32_t n_tiles, unsigned char* image, unsigned long long* d_hash) {
    hipLaunchKernelGGL((checkpoint_pack_kernel<FORM, NT>), dim3(blocks), dim3(CK_BLOCK), 0, st, d_segments, n_segments, d_tile_first, n_tiles, image,
                       d_hash);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_checkpoint(hipStream_t st, CheckpointForm form, bool streaming_stores, const CheckpointSegment* d_segments, uint32_t n_segments,
                             const uint32_t* d_tile_first, uint32_t n_tiles, unsigned char* image, unsigned long long* d_hash, int max_blocks) {
    if (n_tiles == 0 || n_segments == 0) return hipSuccess;
    unsigned blocks = std::min<unsigned>(n_tiles, CK_TARGET_BLOCKS);
    if (max_blocks > 0) blocks = std::min<unsigned>(blocks, (unsigned)max_blocks);
    switch (form) {
        case CHECKPOINT_PACK:
            return streaming_stores ? launch_form<CHECKPOINT_PACK, true>(st, blocks, d_segments, n_segments, d_tile_first, n_tiles, image, d_hash)
                                    : launch_form<CHECKPOINT_PACK, false>(st, blocks, d_segments, n_segments, d_tile_first, n_tiles, image, d_hash);
        case CHECKPOINT_HASH_ONLY:
            return launch_form<CHECKPOINT_HASH_ONLY, false>(st, blocks, d_segments, n_segments, d_tile_first, n_tiles, nullptr, d_hash);
        default:
            return launch_form<CHECKPOINT_UNPACK, false>(st, blocks, d_segments, n_segments, d_tile_first, n_tiles, image, d_hash);
    }
}

}  // namespace coflux
