"""The checkpoint image restated in plain Python (include/coflux.h, "Checkpoint and pickup"): the section hash, a writer
that lays an image out from payloads, and a reader.  Nothing here calls the library; the tests hold the library to it."""
import struct

import numpy as np

MAGIC = b"CFLXCKPT"
VERSION = 1
HEADER_BYTES = ENTRY_BYTES = 96
NAME_BYTES = 48
KIND_ARRAY, KIND_AVERAGE, KIND_CLIMATOLOGY, KIND_INTEGRALS, KIND_MONITOR = range(5)
TILE_BYTES = 16384
M64 = (1 << 64) - 1
HASH_K = 0x9E3779B97F4A7C15


def mix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def hash_bytes_plain(data):
    """Σ_k mix64(w_k XOR K·(k + 1)) mod 2⁶⁴ with Python integers, word by word."""
    data = bytes(data)
    h = 0
    for k in range((len(data) + 7) // 8):
        w = int.from_bytes(data[8 * k:8 * k + 8], "little")   # a short last word is zero padded
        h = (h + mix64(w ^ ((HASH_K * (k + 1)) & M64))) & M64
    return h


def hash_bytes(data):
    """The same with numpy's wrapping uint64 arithmetic (images of megabytes)."""
    data = bytes(data)
    n = (len(data) + 7) // 8
    if n == 0:
        return 0
    w = np.frombuffer(data + b"\0" * (8 * n - len(data)), dtype="<u8").copy()
    with np.errstate(over="ignore"):
        z = w ^ (np.uint64(HASH_K) * np.arange(1, n + 1, dtype=np.uint64))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
        return int(z.sum(dtype=np.uint64))


def round16(n):
    return (n + 15) & ~15


def average_payload(total, samples):
    return struct.pack("<dq", total, samples)


def climatology_payload(weight, samples, bin_weight, bin_samples):
    n = len(bin_weight)
    return struct.pack("<dq", weight, samples) + struct.pack(f"<{n}d", *bin_weight) + struct.pack(f"<{n}q", *bin_samples)


def integrals_payload(records, times):
    """records: float64 [count, n_entries]; the records are zero padded to 16 bytes in front of the times"""
    r = np.ascontiguousarray(records, dtype="<f8").tobytes()
    return r + b"\0" * (round16(len(r)) - len(r)) + np.ascontiguousarray(times, dtype="<f8").tobytes()


def monitor_payload(status, records, times):
    """status: the 16 bytes (first_bad_plus_one i64, bad_entries u32, 0); records: bytes of [count, n_entries] × 64"""
    assert len(status) == 16 and len(records) % 64 == 0
    return bytes(status) + bytes(records) + np.ascontiguousarray(times, dtype="<f8").tobytes()


def monitor_status(first_bad_record, bad_entries):
    return struct.pack("<qII", first_bad_record + 1, bad_entries if first_bad_record >= 0 else 0, 0)


def section(name, payload, kind=KIND_ARRAY, n_entries=0, count=0):
    return dict(name=name, payload=bytes(payload), kind=kind, n_entries=n_entries, count=count)


def write_entry(name, kind, n_entries, nbytes, offset, h, count):
    raw = name.encode() if isinstance(name, str) else bytes(name)
    assert len(raw) < NAME_BYTES
    return raw + b"\0" * (NAME_BYTES - len(raw)) + struct.pack("<IIQQQqQ", kind, n_entries, nbytes & M64, offset & M64, h, count, 0)


def write_header(n_sections, total, grid, dir_hash, blob_bytes, blob_offset, blob_hash):
    head = MAGIC + struct.pack("<IIQ4iQQQQ", VERSION, n_sections, total & M64, *grid, dir_hash, blob_bytes & M64, blob_offset & M64, blob_hash) + b"\0" * 16
    assert len(head) == 88
    return head + struct.pack("<Q", hash_bytes_plain(head))


def build_image(sections, grid, blob=b"", mutate_entry=None):
    """The one encoding of (sections, grid, blob).  `mutate_entry(k, fields)` may change a directory entry's fields before the
    directory and the header are hashed: how the tests make images that are wrong in one designed place only."""
    cursor = HEADER_BYTES + ENTRY_BYTES * len(sections)
    directory, payloads = [], b""
    for k, s in enumerate(sections):
        p = s["payload"]
        fields = dict(name=s["name"], kind=s["kind"], n_entries=s["n_entries"], nbytes=len(p), offset=cursor, h=hash_bytes(p), count=s["count"])
        if mutate_entry:
            mutate_entry(k, fields)
        directory.append(write_entry(**fields))
        payloads += p + b"\0" * (round16(len(p)) - len(p))
        cursor += round16(len(p))
    directory = b"".join(directory)
    total = cursor + round16(len(blob))
    head = write_header(len(sections), total, grid, hash_bytes_plain(directory), len(blob), cursor, hash_bytes(blob))
    return head + directory + payloads + bytes(blob) + b"\0" * (round16(len(blob)) - len(blob))


def rehash(image):
    """`image` (bytes) with its directory hash and header hash recomputed: a change to a directory entry that the hashes do
    not give away."""
    image = bytearray(image)
    n = struct.unpack_from("<I", image, 12)[0]
    struct.pack_into("<Q", image, 40, hash_bytes_plain(bytes(image[HEADER_BYTES:HEADER_BYTES + ENTRY_BYTES * n])))
    struct.pack_into("<Q", image, 88, hash_bytes_plain(bytes(image[:88])))
    return bytes(image)


def read_image(image):
    """(header dict, [entry dicts with their payload], blob) of an image that is taken on trust"""
    image = bytes(image)
    version, n, total, nx, ny, hx, hy, dir_hash, blob_bytes, blob_offset, blob_hash = struct.unpack_from("<IIQ4iQQQQ", image, 8)
    entries = []
    for k in range(n):
        at = HEADER_BYTES + ENTRY_BYTES * k
        kind, n_entries, nbytes, offset, h, count, _ = struct.unpack_from("<IIQQQqQ", image, at + NAME_BYTES)
        entries.append(dict(name=image[at:at + NAME_BYTES].split(b"\0")[0].decode(), kind=kind, n_entries=n_entries, nbytes=nbytes, offset=offset,
                            h=h, count=count, payload=image[offset:offset + nbytes]))
    header = dict(version=version, n_sections=n, total=total, grid=(nx, ny, hx, hy), dir_hash=dir_hash, blob_hash=blob_hash,
                  header_hash=struct.unpack_from("<Q", image, 88)[0])
    return header, entries, image[blob_offset:blob_offset + blob_bytes]
