// coflux_checkpoint_image.cpp — the checkpoint image's parser and the section hash on the host (coflux_checkpoint_image.hpp;
// the format is stated in include/coflux.h).  No HIP header and no context: this file builds and runs alone.  Every offset
// and length is checked against the image size before it is used, with sums that cannot wrap.
#include "coflux_checkpoint_image.hpp"

#include <cstdarg>
#include <cstdio>
#include <cstring>

namespace cfck {

uint64_t hash_bytes(const void* data, size_t n, uint64_t first_word) {
    const unsigned char* p = static_cast<const unsigned char*>(data);
    uint64_t h = 0, k = first_word;
    size_t at = 0;
    for (; at + 8 <= n; at += 8, ++k) h += mix64(get64(p + at) ^ (HASH_K * (k + 1)));
    if (at < n) {
        uint64_t w = 0;
        for (size_t b = 0; at + b < n; ++b) w |= (uint64_t)p[at + b] << (8 * b);
        h += mix64(w ^ (HASH_K * (k + 1)));
    }
    return h;
}

bool payload_bytes(uint32_t kind, uint32_t n_entries, int64_t count, uint64_t* bytes) {
    const uint64_t n = n_entries, c = (uint64_t)count;
    switch (kind) {
        case KIND_AVERAGE:
            *bytes = 16;
            return n_entries == 0 && count == 0;
        case KIND_CLIMATOLOGY:
            *bytes = 16 + 16 * n;
            return n >= 1 && n <= MAX_ENTRIES && count == 0;
        case KIND_INTEGRALS:
        case KIND_MONITOR:
            if (n < 1 || n > MAX_ENTRIES || count < 0 || c > MAX_COUNT) return false;
            *bytes = round_up(series_device_bytes(kind, n_entries, count)) + 8 * c;
            return true;
        default:
            return false;
    }
}

void write_entry(unsigned char* at, const Entry& e) {
    std::memset(at, 0, ENTRY_BYTES);
    std::memcpy(at + E_NAME, e.name, strnlen(e.name, NAME_BYTES - 1));
    put32(at + E_KIND, e.kind);
    put32(at + E_ENTRIES, e.n_entries);
    put64(at + E_BYTES, e.bytes);
    put64(at + E_OFFSET, e.offset);
    put64(at + E_HASH, e.hash);
    put64(at + E_COUNT, (uint64_t)e.count);
}

void read_entry(const unsigned char* at, Entry* e) {
    std::memcpy(e->name, at + E_NAME, NAME_BYTES);
    e->name[NAME_BYTES - 1] = 0;
    e->kind = get32(at + E_KIND);
    e->n_entries = get32(at + E_ENTRIES);
    e->bytes = get64(at + E_BYTES);
    e->offset = get64(at + E_OFFSET);
    e->hash = get64(at + E_HASH);
    e->count = (int64_t)get64(at + E_COUNT);
}

namespace {

int refuse(char* msg, size_t msg_bytes, const char* fmt, ...) {
    if (msg && msg_bytes) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(msg, msg_bytes, fmt, ap);
        va_end(ap);
    }
    return -1;
}

bool all_zero(const unsigned char* p, uint64_t n) {
    for (uint64_t b = 0; b < n; ++b)
        if (p[b]) return false;
    return true;
}

}  // namespace

int verify(const void* image, size_t bytes, Header* header, char* msg, size_t n) {
    if (!image) return refuse(msg, n, "the image is NULL");
    const unsigned char* p = static_cast<const unsigned char*>(image);
    if (bytes < HEADER_BYTES) return refuse(msg, n, "header: the image has %zu bytes, a header has %zu", bytes, HEADER_BYTES);
    if (get64(p + H_MAGIC) != MAGIC) return refuse(msg, n, "header field magic: not a checkpoint image");
    if (get32(p + H_VERSION) != VERSION)
        return refuse(msg, n, "header field version: %u, this library reads version %u", get32(p + H_VERSION), VERSION);
    if (get64(p + H_HASH) != hash_bytes(p, H_HASH)) return refuse(msg, n, "header field header_hash: the header is damaged");
    if (!all_zero(p + H_RESERVED, H_HASH - H_RESERVED)) return refuse(msg, n, "header field reserved: not zero");
    const uint64_t total = get64(p + H_TOTAL);
    if (total != (uint64_t)bytes)
        return refuse(msg, n, "header field total_bytes: %llu, the image has %zu bytes", (unsigned long long)total, bytes);
    const uint32_t sections = get32(p + H_SECTIONS);
    if (sections > MAX_SECTIONS) return refuse(msg, n, "header field n_sections: %u (at most %u)", sections, MAX_SECTIONS);
    const uint64_t dir_end = HEADER_BYTES + ENTRY_BYTES * (uint64_t)sections;   // ≤ 96 · 257
    if (dir_end > total) return refuse(msg, n, "directory: %u entries end at byte %llu of %llu", sections, (unsigned long long)dir_end, (unsigned long long)total);
    if (get64(p + H_DIR_HASH) != hash_bytes(p + HEADER_BYTES, (size_t)(dir_end - HEADER_BYTES)))
        return refuse(msg, n, "header field directory_hash: the directory is damaged");
    uint64_t cursor = dir_end;   // where the next payload starts: a multiple of 16, never above total
    for (uint32_t k = 0; k < sections; ++k) {
        const unsigned char* at = p + HEADER_BYTES + ENTRY_BYTES * (size_t)k;
        if (at[E_NAME] == 0) return refuse(msg, n, "section %u: the name is empty", k);
        if (std::memchr(at + E_NAME, 0, NAME_BYTES) == nullptr) return refuse(msg, n, "section %u: the name is not terminated", k);
        Entry e;
        read_entry(at, &e);
        const size_t len = std::strlen(e.name);
        if (!all_zero(at + E_NAME + len, NAME_BYTES - len)) return refuse(msg, n, "section \"%s\": bytes behind the name", e.name);
        if (!all_zero(at + E_RESERVED, ENTRY_BYTES - E_RESERVED)) return refuse(msg, n, "section \"%s\": reserved is not zero", e.name);
        for (uint32_t j = 0; j < k; ++j)
            if (std::memcmp(at + E_NAME, p + HEADER_BYTES + ENTRY_BYTES * (size_t)j + E_NAME, NAME_BYTES) == 0)
                return refuse(msg, n, "section \"%s\": sections %u and %u have the same name", e.name, j, k);
        if (e.kind >= KINDS) return refuse(msg, n, "section \"%s\": unknown kind %u", e.name, e.kind);
        if (e.kind == KIND_ARRAY) {
            if (e.n_entries != 0 || e.count != 0) return refuse(msg, n, "section \"%s\": an array with n_entries or count", e.name);
        } else {
            uint64_t want = 0;
            if (!payload_bytes(e.kind, e.n_entries, e.count, &want))
                return refuse(msg, n, "section \"%s\": n_entries %u and count %lld do not fit kind %u", e.name, e.n_entries, (long long)e.count, e.kind);
            if (want != e.bytes)
                return refuse(msg, n, "section \"%s\": %llu payload bytes, its kind, n_entries and count give %llu", e.name,
                              (unsigned long long)e.bytes, (unsigned long long)want);
        }
        if (e.offset != cursor)
            return refuse(msg, n, "section \"%s\": offset %llu, its payload belongs at %llu of %llu", e.name, (unsigned long long)e.offset,
                          (unsigned long long)cursor, (unsigned long long)total);
        if (e.bytes > total - cursor)   // (cursor ≤ total: no wrap)
            return refuse(msg, n, "section \"%s\": %llu bytes at offset %llu end beyond the image's %llu", e.name, (unsigned long long)e.bytes,
                          (unsigned long long)e.offset, (unsigned long long)total);
        const uint64_t padded = round_up(e.bytes);   // e.bytes ≤ total ≤ SIZE_MAX: a wrap gives 0 < e.bytes
        if (padded < e.bytes || padded > total - cursor) return refuse(msg, n, "section \"%s\": its padding ends beyond the image", e.name);
        if (!all_zero(p + cursor + e.bytes, padded - e.bytes)) return refuse(msg, n, "section \"%s\": the padding is not zero", e.name);
        if (e.kind == KIND_INTEGRALS) {   // the records' own padding in front of the times
            const uint64_t dev = series_device_bytes(e.kind, e.n_entries, e.count);
            if (!all_zero(p + cursor + dev, round_up(dev) - dev)) return refuse(msg, n, "section \"%s\": the padding behind the records is not zero", e.name);
        }
        if (hash_bytes(p + cursor, (size_t)e.bytes) != e.hash) return refuse(msg, n, "section \"%s\": the payload does not have its hash", e.name);
        cursor += padded;
    }
    const uint64_t blob = get64(p + H_BLOB_BYTES);
    if (get64(p + H_BLOB_OFFSET) != cursor)
        return refuse(msg, n, "header field blob_offset: %llu, the host blob belongs at %llu", (unsigned long long)get64(p + H_BLOB_OFFSET), (unsigned long long)cursor);
    if (blob > total - cursor) return refuse(msg, n, "header field blob_bytes: %llu bytes at %llu end beyond the image's %llu", (unsigned long long)blob,
                                             (unsigned long long)cursor, (unsigned long long)total);
    const uint64_t padded = round_up(blob);
    if (padded < blob || padded != total - cursor) return refuse(msg, n, "header field total_bytes: the image does not end with the host blob");
    if (!all_zero(p + cursor + blob, padded - blob)) return refuse(msg, n, "host blob: the padding is not zero");
    if (hash_bytes(p + cursor, (size_t)blob) != get64(p + H_BLOB_HASH)) return refuse(msg, n, "host blob: the bytes do not have their hash (header field blob_hash)");
    if (header) {
        header->n_sections = sections;
        header->total = total;
        header->nx = (int32_t)get32(p + H_NX);
        header->ny = (int32_t)get32(p + H_NY);
        header->hx = (int32_t)get32(p + H_HX);
        header->hy = (int32_t)get32(p + H_HY);
        header->blob_bytes = blob;
        header->blob_offset = cursor;
    }
    return 0;
}

}  // namespace cfck
