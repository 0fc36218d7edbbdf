// coflux_checkpoint_image.hpp — the checkpoint image as bytes: its layout, the section hash and the parser behind
// cf_checkpoint_verify (include/coflux.h states the format).  Plain C++: no HIP header, no context, so that
// coflux_checkpoint_image.cpp builds and runs alone (tests/checkpoint_image_driver.cpp links nothing else).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace cfck {

constexpr uint64_t MAGIC = 0x54504B43584C4643ull;   // "CFLXCKPT", little endian
constexpr uint32_t VERSION = 1;
constexpr size_t HEADER_BYTES = 96, ENTRY_BYTES = 96, NAME_BYTES = 48, ALIGN = 16;
constexpr uint32_t MAX_SECTIONS = 256;
constexpr uint32_t KIND_ARRAY = 0, KIND_AVERAGE = 1, KIND_CLIMATOLOGY = 2, KIND_INTEGRALS = 3, KIND_MONITOR = 4, KINDS = 5;
inline const char* kind_name(uint32_t kind) {
    constexpr const char* names[KINDS] = {"array", "average", "climatology", "integrals", "monitor"};
    return kind < KINDS ? names[kind] : "unknown";
}
constexpr size_t MONITOR_STATUS_BYTES = 16, MONITOR_RECORD_BYTES = 64;
constexpr uint64_t MAX_COUNT = 1ull << 31, MAX_ENTRIES = 32;   // what a series can hold: keeps every size below 2⁴⁸

// header, little endian (byte offsets)
constexpr size_t H_MAGIC = 0, H_VERSION = 8, H_SECTIONS = 12, H_TOTAL = 16, H_NX = 24, H_NY = 28, H_HX = 32, H_HY = 36, H_DIR_HASH = 40,
                 H_BLOB_BYTES = 48, H_BLOB_OFFSET = 56, H_BLOB_HASH = 64, H_RESERVED = 72, H_HASH = 88;
// directory entry
constexpr size_t E_NAME = 0, E_KIND = 48, E_ENTRIES = 52, E_BYTES = 56, E_OFFSET = 64, E_HASH = 72, E_COUNT = 80, E_RESERVED = 88;

struct Entry {
    char name[NAME_BYTES];   // NUL terminated
    uint32_t kind, n_entries;
    uint64_t bytes, offset, hash;
    int64_t count;
};

struct Header {
    uint32_t n_sections;
    uint64_t total;
    int32_t nx, ny, hx, hy;
    uint64_t blob_bytes, blob_offset;
};

inline uint64_t round_up(uint64_t n) { return (n + (ALIGN - 1)) & ~(uint64_t)(ALIGN - 1); }

inline uint64_t mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
constexpr uint64_t HASH_K = 0x9E3779B97F4A7C15ull;

// Σ mix64(w_k XOR K·(k + 1)) over the 8-byte little-endian words k = first_word … of `n` bytes at p, the last one zero padded
uint64_t hash_bytes(const void* p, size_t n, uint64_t first_word = 0);

// the payload of a library-kept section: what the kind, n_entries and count of its entry imply (false: not a valid combination)
bool payload_bytes(uint32_t kind, uint32_t n_entries, int64_t count, uint64_t* bytes);
// of a series section: the bytes the device holds (status and records, from the start of the payload) and where the times begin
inline uint64_t series_device_bytes(uint32_t kind, uint32_t n_entries, int64_t count) {
    return kind == KIND_MONITOR ? MONITOR_STATUS_BYTES + MONITOR_RECORD_BYTES * (uint64_t)n_entries * (uint64_t)count
                                : 8 * (uint64_t)n_entries * (uint64_t)count;
}

// little endian; a double travels as its bits
inline uint32_t get32(const unsigned char* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
inline uint64_t get64(const unsigned char* p) { return (uint64_t)get32(p) | (uint64_t)get32(p + 4) << 32; }
inline void put32(unsigned char* p, uint32_t v) {
    for (int b = 0; b < 4; ++b) p[b] = (unsigned char)(v >> (8 * b));
}
inline void put64(unsigned char* p, uint64_t v) {
    put32(p, (uint32_t)v);
    put32(p + 4, (uint32_t)(v >> 32));
}
inline double get_f64(const unsigned char* p) {
    const uint64_t bits = get64(p);
    double v;
    std::memcpy(&v, &bits, 8);
    return v;
}
inline void put_f64(unsigned char* p, double v) {
    uint64_t bits;
    std::memcpy(&bits, &v, 8);
    put64(p, bits);
}
void write_entry(unsigned char* at, const Entry& e);
void read_entry(const unsigned char* at, Entry* e);

// Checks everything cf_checkpoint_verify promises; 0, or −1 with a message that names the field or the section in `msg`.
// On success *header (may be NULL) is filled; entries are read with read_entry at HEADER_BYTES + k · ENTRY_BYTES.
int verify(const void* image, size_t bytes, Header* header, char* msg, size_t msg_bytes);

}  // namespace cfck
