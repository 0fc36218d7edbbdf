"""CPU-side checks of checkpoint and pickup (include/coflux.h, "Checkpoint and pickup"): the new entry points are declared,
exported and bound in the header, abi.py and the Julia stub; cf_checkpoint_hash against a plain-Python restatement;
cf_checkpoint_verify on images written by tests/checkpoint_reference.py, whole and damaged in one designed place each; the
same images replayed through a stand-alone sanitizer build of the parser; and the mirror's file handling and schedules."""
import ctypes as C
import os
import random
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import checkpoint_reference as ref
from coflux import abi, runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "climaocean.jl_amd", "csrc")
NEW_SYMBOLS = ("cf_checkpoint_create", "cf_checkpoint_destroy", "cf_checkpoint_add_array", "cf_checkpoint_add_average",
               "cf_checkpoint_add_climatology", "cf_checkpoint_add_integrals", "cf_checkpoint_add_monitor", "cf_checkpoint_set_host_blob",
               "cf_checkpoint_capture", "cf_checkpoint_wait", "cf_checkpoint_restore", "cf_checkpoint_verify", "cf_checkpoint_hash",
               "cf_checkpoint_host_blob")
GRID = (70, 23, 3, 2)

KNOWN_ANSWERS = [
    (struct.pack("<6Q", 0, 0x8000000000000000, 0x3FF0000000000000, 0x7FF8000000000000, 0x7FF0000000000000, 0xBFF8000000000000), 0xbc9733db8e1747df),
    (struct.pack("<d", 0.0), 0xe220a8397b1dcdaf),
    (b"", 0),
    (bytes(range(1, 12)), 0x21e51a3dd06edc89),
    (b"\x01", 0xe4d971771b652c20),
]


def test_symbols_are_declared_exported_and_bound_and_the_abi_is_still_5():
    header = open(os.path.join(ROOT, "include", "coflux.h")).read()
    stub = open(os.path.join(ROOT, "climaocean.jl_amd", "julia", "CoFluxMI355X.jl")).read()
    lib = abi.load_library()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in abi.EXPORTED_SYMBOLS and hasattr(lib, name), name
        assert f"(:{name}, libcoflux)" in stub, name
    assert lib.cf_version() == abi.ABI_VERSION == 5 and "#define CF_ABI_VERSION 5" in header
    # the descriptor has one size in its three copies
    m = re.search(r"typedef struct cf_checkpoint_desc \{(.*?)\} cf_checkpoint_desc;", header, re.S)
    c_fields = re.findall(r"\bint32_t\s+(\w+);", m.group(1))
    assert c_fields == [f for f, _ in abi.CheckpointDesc._fields_] and C.sizeof(abi.CheckpointDesc) == 4 * len(c_fields) == 16
    m = re.search(r"struct CfCheckpointDesc\n(.*?)\nend", stub, re.S)
    assert re.findall(r"(\w+)::Int32", m.group(1)) == c_fields
    assert (abi.CHECKPOINT_MAX_SECTIONS, abi.CHECKPOINT_DIRECT) == (256, 1)
    assert "#define CF_CHECKPOINT_MAX_SECTIONS 256" in header and "#define CF_CHECKPOINT_DIRECT 1" in header


def test_hash_known_answers():
    for data, want in KNOWN_ANSWERS:
        assert ref.hash_bytes_plain(data) == want, data
        assert ref.hash_bytes(data) == want, data
        assert runtime.checkpoint_hash(data) == want, data


def test_hash_equals_the_plain_restatement_at_every_length_class():
    rng = random.Random(11)
    pool = bytes(rng.getrandbits(8) for _ in range(16384 + 16))
    for n in list(range(0, 41)) + [16384 + d for d in (0, 1, 7, 8, 9, -1, -7, -8, -9)]:
        assert runtime.checkpoint_hash(pool[:n]) == ref.hash_bytes_plain(pool[:n]) == ref.hash_bytes(pool[:n]), n
    big = np.random.default_rng(5).integers(0, 256, 100 * 1024, dtype=np.uint8).tobytes()
    assert runtime.checkpoint_hash(big) == ref.hash_bytes_plain(big) == ref.hash_bytes(big)
    # bytes-like objects of every kind the mirror hands in
    assert runtime.checkpoint_hash(bytearray(big[:99])) == runtime.checkpoint_hash(memoryview(big)[:99]) == ref.hash_bytes_plain(big[:99])
    # a single changed byte always changes the hash (mix64 is a bijection of the word)
    flipped = bytearray(big[:64])
    flipped[17] ^= 0x20
    assert runtime.checkpoint_hash(flipped) != runtime.checkpoint_hash(big[:64])


def designed_sections():
    """One section of every kind, payload lengths in every class mod 16, an empty one, a series that is empty and one whose
    records need padding in front of the times."""
    rng = np.random.default_rng(3)
    raw = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()  # noqa: E731
    return [
        ref.section("T", raw(8 * 29 * 76)),
        ref.section("one_byte", raw(1)),
        ref.section("empty", b""),
        ref.section("eleven", raw(11)),
        ref.section("averages", ref.average_payload(3600.0, 3), ref.KIND_AVERAGE),
        ref.section("climatology", ref.climatology_payload(7200.0, 6, [3600.0, 0.0, 3600.0], [3, 0, 3]), ref.KIND_CLIMATOLOGY, n_entries=3),
        ref.section("integrals", ref.integrals_payload(rng.normal(size=(3, 5)), [1.0, 2.0, 3.0]), ref.KIND_INTEGRALS, n_entries=5, count=3),
        ref.section("integrals_empty", ref.integrals_payload(np.zeros((0, 4)), []), ref.KIND_INTEGRALS, n_entries=4, count=0),
        ref.section("monitor", ref.monitor_payload(ref.monitor_status(1, 0b101), raw(64 * 3 * 2), [10.0, 20.0]), ref.KIND_MONITOR, n_entries=3, count=2),
        ref.section("mask", raw(29 * 76 + 3)),
    ]


BLOB = b'{"clock": {"time": 6000.0, "iteration": 5}}'


def corrupt_images():
    """{label: (image, words the refusal must contain)}: each image is wrong in one designed place."""
    sections = designed_sections()
    good = ref.build_image(sections, GRID, BLOB)
    _, entries, _ = ref.read_image(good)
    n = len(sections)
    out = {}
    # truncation: inside the header, at every directory boundary, in the middle of a payload, one byte short
    out["truncated_header"] = (good[:50], ["header"])
    for k in range(n + 1):
        out[f"truncated_directory_{k}"] = (good[:ref.HEADER_BYTES + ref.ENTRY_BYTES * k], ["total_bytes"])
    out["truncated_payload"] = (good[:entries[0]["offset"] + 1000], ["total_bytes"])
    out["truncated_last_byte"] = (good[:-1], ["total_bytes"])

    def flip(at, bit=0):
        b = bytearray(good)
        b[at] ^= 1 << bit
        return bytes(b)
    # one flipped bit in the header: magic, version, n_sections, total, grid, the hashes, the reserved bytes
    for name, at, words in (("magic", 3, ["magic"]), ("version", 8, ["version"]), ("n_sections", 12, ["header"]), ("total", 17, ["header"]),
                            ("nx", 24, ["header"]), ("hy", 37, ["header"]), ("directory_hash", 41, ["header"]), ("blob_bytes", 48, ["header"]),
                            ("reserved", 75, ["header"]), ("header_hash", 90, ["header_hash"])):
        out[f"header_bit_{name}"] = (flip(at, 3), words)
    # one flipped bit in a directory entry (name, kind, bytes, offset, hash, count of several sections)
    for k, field_at in ((0, 0), (3, 48), (4, 56), (6, 64), (8, 72), (6, 80), (9, 90)):
        out[f"directory_bit_{k}_{field_at}"] = (flip(ref.HEADER_BYTES + ref.ENTRY_BYTES * k + field_at), ["directory_hash"])
    # … and in a payload, in a series' host-kept times, in the padding behind a section, in the blob and in its padding
    out["payload_bit"] = (flip(entries[0]["offset"] + 777, 6), ['"T"'])
    out["times_bit"] = (flip(entries[8]["offset"] + entries[8]["nbytes"] - 3), ['"monitor"'])
    out["padding_bit"] = (flip(entries[3]["offset"] + 11 + 2), ['"eleven"', "padding"])
    out["records_padding_bit"] = (flip(entries[6]["offset"] + 8 * 15 + 1), ['"integrals"'])
    blob_at = len(good) - ref.round16(len(BLOB))
    out["blob_bit"] = (flip(blob_at + 5), ["blob"])
    out["blob_padding_bit"] = (flip(len(good) - 1), ["blob", "padding"])

    # entries that are wrong but whose directory and header hash as they should
    def mutated(k, **changes):
        def mutate(j, fields):
            if j == k:
                fields.update(changes)
        return ref.build_image(sections, GRID, BLOB, mutate_entry=mutate)
    out["offset_beyond_image"] = (mutated(9, offset=len(good) + 4096), ['"mask"', "offset"])
    out["offset_into_directory"] = (mutated(0, offset=96), ['"T"', "offset"])
    out["offset_unaligned"] = (mutated(1, offset=entries[1]["offset"] + 8), ['"one_byte"', "offset"])
    out["length_overflows"] = (mutated(9, nbytes=(1 << 64) - 8), ['"mask"'])
    out["length_overflows_sum"] = (mutated(0, nbytes=(1 << 64) - entries[0]["offset"] + 16), ['"T"'])
    out["length_beyond_image"] = (mutated(9, nbytes=entries[9]["nbytes"] + 64), ['"mask"'])
    out["same_name"] = (mutated(3, name="T"), ['"T"', "same name"])
    out["unknown_kind"] = (mutated(2, kind=9), ['"empty"', "kind"])
    out["series_count_lies"] = (mutated(6, count=4), ['"integrals"'])
    out["series_count_negative"] = (mutated(8, count=-1), ['"monitor"'])
    out["series_count_huge"] = (mutated(8, count=1 << 62), ['"monitor"'])
    out["bins_lie"] = (mutated(5, n_entries=4), ['"climatology"'])
    out["array_with_count"] = (mutated(0, count=1), ['"T"'])
    out["wrong_hash"] = (mutated(4, h=entries[4]["h"] ^ 1), ['"averages"', "hash"])
    out["too_many_sections"] = (ref.rehash(good[:12] + struct.pack("<I", 257) + good[16:]), ["n_sections"])
    out["sections_beyond_image"] = (ref.rehash(good[:12] + struct.pack("<I", 256) + good[16:]), [])
    return good, out


def test_reference_images_verify_and_carry_their_blob():
    good, _ = corrupt_images()
    runtime.checkpoint_verify(good)
    assert runtime.checkpoint_host_blob(good) == BLOB
    for sections, blob in (([], b""), ([], b"x"), (designed_sections()[:1], b""), ([ref.section(f"s{k}", bytes(k % 19)) for k in range(256)], BLOB)):
        image = ref.build_image(sections, GRID, blob)
        runtime.checkpoint_verify(image)
        runtime.checkpoint_verify(bytearray(image))
        assert runtime.checkpoint_host_blob(image) == blob
    header, entries, blob = ref.read_image(good)
    assert header["grid"] == GRID and [e["name"] for e in entries] == [s["name"] for s in designed_sections()] and blob == BLOB
    assert all(e["offset"] % 16 == 0 for e in entries)


def test_every_designed_damage_is_refused_with_a_message_that_names_the_place():
    _, images = corrupt_images()
    assert len(images) > 50
    for label, (image, words) in images.items():
        with pytest.raises(ValueError) as e:
            runtime.checkpoint_verify(image)
        for word in words:
            assert word in str(e.value), (label, str(e.value))
        with pytest.raises(ValueError):
            runtime.checkpoint_host_blob(image)
    for junk in (b"", b"\0" * 95, b"\0" * 96, os.urandom(4096)):
        with pytest.raises(ValueError):
            runtime.checkpoint_verify(junk)


def test_a_sanitizer_build_of_the_parser_alone_replays_the_images(tmp_path):
    """tests/checkpoint_image_driver.cpp + csrc/coflux_checkpoint_image.cpp and nothing else, compiled with
    -fsanitize=address,undefined, run as a subprocess over the reference images and every damaged one: the same verdicts, and
    no report from either sanitizer (each image sits in a heap block of exactly its size).  The sanitizer runtimes are linked
    into the program statically: nothing is preloaded and the environment is left as it is."""
    compiler = shutil.which("g++") or shutil.which("clang++")
    if compiler is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "checkpoint_image_driver")
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(compiler) == "g++" else ["-static-libsan"]
    build = subprocess.run([compiler, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static, "-I", CSRC,
                            os.path.join(ROOT, "tests", "checkpoint_image_driver.cpp"), os.path.join(CSRC, "coflux_checkpoint_image.cpp"), "-o", exe],
                           capture_output=True, text=True)
    if build.returncode != 0 and re.search(r"cannot find.*(asan|ubsan|clang_rt)|libasan|libubsan|asan_preinit|static-lib", build.stderr):
        pytest.skip("the sanitizer runtime does not link here: " + build.stderr.strip().splitlines()[-1])
    assert build.returncode == 0, build.stderr
    good, images = corrupt_images()
    paths, want = [], []
    for label, image in [("good", good), ("empty_registration", ref.build_image([], GRID, b""))] + [(k, v[0]) for k, v in images.items()]:
        p = tmp_path / (label + ".cfck")
        p.write_bytes(image)
        paths.append(str(p))
        want.append(label in ("good", "empty_registration"))
    run = subprocess.run([exe] + paths, capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    lines = run.stdout.strip().splitlines()
    assert len(lines) == len(paths)
    for path, ok, line in zip(paths, want, lines):
        got_path, verdict = line.split("\t")[:2]
        assert got_path == path and verdict == ("OK" if ok else "REFUSED"), line
    assert lines[0].split("\t")[2] == "%016x" % ref.hash_bytes(good)
    # the library gives the same message for the same image
    for (label, (image, _)), line in zip(images.items(), lines[2:]):
        with pytest.raises(ValueError) as e:
            runtime.checkpoint_verify(image)
        assert line.split("\t")[2] in str(e.value), label


# ---------------------------------------------------------------------------------------------
# the mirror's host side: schedules and files (the library call faked)
# ---------------------------------------------------------------------------------------------
class FakeCheckpoint:
    """What Checkpointer needs of a runtime.Checkpoint, without a device: the image is the blob behind a tag."""

    def __init__(self):
        self.blob, self.captures, self.waits = b"", [], 0

    def set_host_blob(self, data):
        self.blob = bytes(data)

    def capture(self):
        self.captures.append(self.blob)

    def wait(self, copy=True):
        self.waits += 1
        return memoryview(b"IMAGE:" + self.captures[-1])

    def close(self):
        pass


def fake_checkpointer(tmp_path, **kw):
    from types import SimpleNamespace

    from coflux import models as cm
    model = SimpleNamespace(clock=SimpleNamespace(time=0.0, iteration=0), ocean=SimpleNamespace(model=SimpleNamespace(clock=SimpleNamespace(time=0.0, iteration=0))))
    w = cm.Checkpointer(model, dir=str(tmp_path), **kw)
    w.checkpoint = FakeCheckpoint()
    return w, model


def step(w, model, dt=1200.0):
    model.clock.time += dt
    model.clock.iteration += 1
    w.write(model.clock)


def test_time_interval_actuates_when_the_clock_reaches_k_intervals():
    from coflux import models as cm
    s = cm.TimeInterval(3600.0)
    s.initialize(0.0, 1200.0)
    assert [s.actuate(1200.0 * k) for k in range(1, 10)] == [False, False, True] * 3
    # a clock that is a repeated sum arrives a rounding error early or late: within 1e-6 Δt counts as reached, once
    s = cm.TimeInterval(1.0)
    s.initialize(0.0, 0.1)
    t, hits = 0.0, []
    for k in range(1, 31):
        t += 0.1
        if s.actuate(t):
            hits.append(k)
    assert hits == [10, 20, 30]
    # initialised in the middle of a run (after a pickup): the next multiple, not the one just reached
    s = cm.TimeInterval(3600.0)
    s.initialize(3600.0, 1200.0)
    assert [s.actuate(3600.0 + 1200.0 * k) for k in range(1, 4)] == [False, False, True]
    s.initialize(4000.0, 1200.0)
    assert not s.actuate(5200.0) and s.actuate(7200.0)
    # a step that jumps over several multiples actuates once
    s = cm.TimeInterval(10.0)
    s.initialize(0.0, 35.0)
    assert s.actuate(35.0) and not s.actuate(39.0) and s.actuate(40.0)
    with pytest.raises(ValueError):
        cm.TimeInterval(0.0)


def test_checkpointer_names_files_by_iteration_and_writes_them_one_write_late(tmp_path):
    from coflux import models as cm
    w, model = fake_checkpointer(tmp_path / "out", schedule=cm.IterationInterval(3), prefix="omip")
    for _ in range(3):
        step(w, model)
    # the capture of iteration 3 is in flight: no file yet, no wait yet
    assert w.checkpoint.captures and w.checkpoint.waits == 0 and w.iterations() == []
    step(w, model)
    assert w.iterations() == [3] and os.path.basename(w.latest()) == "omip_iteration3.cfck"
    blob = open(w.path(3), "rb").read()
    assert blob.startswith(b"IMAGE:") and b'"iteration": 3' in blob and b'"time": 3600.0' in blob
    for _ in range(5):
        step(w, model)
    assert w.iterations() == [3, 6]           # iteration 9 is still in flight
    w.close()
    assert w.iterations() == [3, 6, 9] and w.latest() == w.path(9)
    assert sorted(os.listdir(tmp_path / "out")) == ["omip_iteration3.cfck", "omip_iteration6.cfck", "omip_iteration9.cfck"]
    # "latest" is the highest NUMBER, not the last name in the alphabet; other prefixes and suffixes are not this writer's
    for name in ("omip_iteration10.cfck", "omip_iteration10.cfck.tmp", "other_iteration99.cfck", "omip_iteration11.jld2", "omip_iterationX.cfck"):
        (tmp_path / "out" / name).write_bytes(b"")
    assert w.iterations() == [3, 6, 9, 10] and w.latest() == w.path(10)
    assert cm.Checkpointer(model, dir=str(tmp_path / "nowhere")).latest() is None


def test_checkpointer_time_schedule_and_cleanup(tmp_path):
    from coflux import models as cm
    w, model = fake_checkpointer(tmp_path, schedule=cm.TimeInterval(3600.0), cleanup=True)
    w.schedule.initialize(0.0, 1200.0)
    for _ in range(10):
        step(w, model)
        assert len(w.iterations()) <= 1       # the previous file goes once the next one is whole
    assert w.iterations() == [9] and w.checkpoint.waits == 3   # captured at 3, 6 and 9; the write of iteration 10 wrote 9's file
    w.flush()                                 # nothing in flight: nothing to do
    assert w.iterations() == [9] and w.checkpoint.waits == 3
    step(w, model)
    step(w, model)                            # iteration 12 is captured and in flight
    assert w.iterations() == [9] and len(w.checkpoint.captures) == 4
    w.flush()
    assert w.iterations() == [12] and w.checkpoint.waits == 4


def test_checkpointer_renames_a_whole_temporary_file_into_place(tmp_path, monkeypatch):
    from coflux import models as cm
    w, model = fake_checkpointer(tmp_path, schedule=cm.IterationInterval(1))
    seen = []
    real = os.replace

    def watched(src, dst):
        # at the rename the temporary file holds the whole image and the final name does not exist yet
        seen.append((os.path.basename(src), os.path.basename(dst), open(src, "rb").read(), os.path.exists(dst)))
        real(src, dst)
    monkeypatch.setattr(os, "replace", watched)
    step(w, model)
    w.flush()
    assert len(seen) == 1
    src, dst, content, existed = seen[0]
    assert (src, dst, existed) == ("checkpoint_iteration1.cfck.tmp", "checkpoint_iteration1.cfck", False)
    assert content == open(w.path(1), "rb").read() and content.startswith(b"IMAGE:")
    assert os.listdir(tmp_path) == ["checkpoint_iteration1.cfck"]
    # a write that fails half way leaves no file under the final name
    monkeypatch.setattr(os, "replace", lambda src, dst: (_ for _ in ()).throw(OSError("disk full")))
    step(w, model)
    with pytest.raises(OSError):
        w.flush()
    assert w.iterations() == [1]
