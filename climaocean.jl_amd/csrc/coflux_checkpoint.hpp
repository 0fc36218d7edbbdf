// coflux_checkpoint.hpp — what coflux_checkpoint.cpp (the host side of cf_checkpoint_*) and coflux_checkpoint.hip (the pack
// kernel) share.  Internal: nothing here crosses the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace coflux {

constexpr unsigned CHECKPOINT_TILE_BYTES = 16384;   // the image is cut into tiles of this many bytes, one workgroup at a time

// One run of device bytes of a section and where it lies in the image.  `image_offset` is a multiple of 16; the run owns the
// image bytes [image_offset, image_offset + round16(bytes)) and no other run meets them; `ptr` is 8-byte aligned.
struct CheckpointSegment {
    unsigned char* ptr;      // the section's device bytes (read by pack and hash-only, written by unpack)
    uint64_t image_offset;
    uint64_t bytes;          // > 0
    uint64_t first_word;     // index, within its section, of the 8-byte word the run starts with
    uint32_t section;        // whose hash word receives the run's sum
    uint32_t reserved;
};

enum CheckpointForm { CHECKPOINT_PACK = 0, CHECKPOINT_HASH_ONLY = 1, CHECKPOINT_UNPACK = 2 };

// One launch over tiles [0, n_tiles): d_tile_first[t] is the first segment (ascending image_offset) that ends behind the start
// of tile t.  `image` is the device staging image (NULL for CHECKPOINT_HASH_ONLY), `d_hash` one zeroed word per section.
hipError_t launch_checkpoint(hipStream_t st, CheckpointForm form, bool streaming_stores, const CheckpointSegment* d_segments, uint32_t n_segments,
                             const uint32_t* d_tile_first, uint32_t n_tiles, unsigned char* image, unsigned long long* d_hash, int max_blocks);

}  // namespace coflux
