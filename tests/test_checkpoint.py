"""GPU tests of checkpoint and pickup (include/coflux.h, "Checkpoint and pickup"): the packed image against the plain-Python
writer of tests/checkpoint_reference.py on designed section sets, in both forms and under capped launches; the unpack into
guarded sentinel-filled arrays of another alignment and every refusal; the private state of an averager, a climatology, an
integrator and a monitor across the destruction of their context; and the coupled step loop split by capture → restore."""
import struct

import numpy as np
import pytest
import torch

import checkpoint_reference as ref
import coupled_case as cc
import test_coupled_steps as tcs
import util
from coflux import abi
from coflux import interface_computations as ic
from coflux.runtime import Checkpoint, CofluxError, FluxContext, checkpoint_host_blob, checkpoint_verify

pytestmark = pytest.mark.gpu

GUARD = 96
TILE = ref.TILE_BYTES
SPECIALS = [0x0000000000000000, 0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000, 0x7FF8000000000000, 0x7FF8DEADBEEF0001,
            0xFFF4000000000123, 0x0000000000000001, 0x3FF0000000000000, 0xBFF8000000000000]
CONFIGS = [(direct, cap) for direct in (False, True) for cap in (0, 1, 3)]


def device_bytes(t):
    """A d2h copy of a tensor's bytes."""
    return t.contiguous().view(torch.uint8).cpu().numpy().tobytes() if t.numel() else b""


def f64(n, seed, offset=0):
    """n doubles of designed bits (NaN payloads, −0.0, ±Inf and a subnormal among ordinary values) in a fresh buffer whose first
    element lies `offset` doubles behind the allocation's start."""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 1 << 63, n, dtype=np.uint64) ^ (rng.integers(0, 2, n, dtype=np.uint64) << np.uint64(63))
    bits[::7] = np.array(SPECIALS, dtype=np.uint64)[np.arange(len(bits[::7])) % len(SPECIALS)]
    buf = torch.empty(offset + n, dtype=torch.float64, device="cuda")
    view = buf[offset:]
    view.view(torch.int64).copy_(torch.from_numpy(bits.view(np.int64)))
    return view


def u8(n, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)).cuda()


def section_sets():
    """{set: [(name, tensor)]}: the smallest shapes at which the pack kernel takes another path."""
    sets = {}
    sets["small"] = [("one_byte", u8(1, 1)), ("empty", torch.empty(0, dtype=torch.float64, device="cuda")), ("eleven", u8(11, 2)),
                     ("specials", f64(23, 3)), ("int32_odd", torch.arange(-3, 4, dtype=torch.int32, device="cuda")), ("fifteen", u8(15, 4)),
                     ("seventeen", u8(17, 5)), ("misaligned", f64(5, 6, offset=1))]
    sets["tiles"] = [("tile", f64(TILE // 8, 7)), ("tile_plus_8", f64(TILE // 8 + 1, 8, offset=1)), ("tile_minus_8", f64(TILE // 8 - 1, 9)),
                     ("five_tiles", f64(5 * TILE // 8 + 3, 10)), ("five_tiles_misaligned", f64(5 * TILE // 8 - 5, 11, offset=1)),
                     ("bytes_across_a_tile", u8(TILE + 13, 12))]
    sets["64_in_a_tile"] = [(f"s{k}", u8(1 + (k * 37) % 250, 100 + k) if k % 3 else f64(1 + k % 9, 100 + k, offset=k % 2)) for k in range(64)]
    assert 96 * 65 + sum(ref.round16(t.numel() * t.element_size()) for _, t in sets["64_in_a_tile"]) < TILE   # header, directory and all
    sets["256_sections"] = [(f"section_{k:03d}", u8((k * 131) % 1900, 400 + k) if k % 2 else f64((k * 29) % 300, 400 + k, offset=(k // 2) % 2))
                            for k in range(256)]
    cube = f64(3 * 13 * 21, 13).view(3, 13, 21)   # an odd plane: slab 1 is 8- but not 16-byte aligned
    assert cube[1].data_ptr() % 16 == 8 and cube[0].data_ptr() % 16 == 0
    sets["slabs"] = [("k0", cube[0]), ("k1", cube[1]), ("k2", cube[2]), ("mask", u8(13 * 21, 14))]
    return sets


def reference_image(named, grid, blob=b""):
    return ref.build_image([ref.section(name, device_bytes(t)) for name, t in named], grid, blob)


@pytest.fixture(scope="module")
def small_ctx():
    ctx = FluxContext(16, 8, 2, 3, ic.flux_params())
    yield ctx
    ctx.close()


@pytest.mark.parametrize("which", ["small", "tiles", "64_in_a_tile", "256_sections", "slabs"])
def test_pack_is_the_definition(small_ctx, which):
    """capture + wait gives exactly the bytes checkpoint_reference.py lays out from d2h copies of the sections — header,
    directory, hashes, payloads and zero padding (fresh staging and pinned buffers hold a sentinel) — with the staging image and
    without it, uncapped and capped at 1 and 3 workgroups, twice in a row from the same handle."""
    ctx = small_ctx
    named = section_sets()[which]
    blob = b'{"iteration": 5}' if which != "tiles" else b""
    want = reference_image(named, (16, 8, 2, 3), blob)
    checkpoint_verify(want)
    for direct, cap in CONFIGS:
        cp = Checkpoint(ctx, direct=direct, max_workgroups=cap)
        for name, t in named:
            cp.add_array(name, t)
        cp.set_host_blob(blob)
        for again in range(2):
            cp.capture()
            got = cp.wait()
            assert len(got) == len(want), (direct, cap, again)
            if got != want:
                at = next(k for k in range(len(want)) if got[k] != want[k])
                raise AssertionError(f"direct={direct} cap={cap} capture {again}: first difference at byte {at} of {len(want)}")
        checkpoint_verify(got)
        assert checkpoint_host_blob(got) == blob
        cp.close()


def test_registration_and_capture_errors(small_ctx):
    ctx = small_ctx
    a, b = f64(64, 1), f64(64, 2)
    cp = Checkpoint(ctx)
    cp.add_array("a", a)
    for name, t, words in (("a", b, "registered already"), ("x" * 48, b, "47"), ("", b, "empty"), ("overlap", a[8:24], '"a"'),
                           ("odd", u8(32, 1)[4:], "aligned")):
        with pytest.raises(CofluxError, match=words):
            cp.add_array(name, t)
    cp.add_array("x" * 47, b)
    cp.add_array("nothing", a[:0])         # an empty section overlaps nothing
    assert cp.wait() is None                # nothing captured yet
    cp.capture()
    with pytest.raises(CofluxError, match="in flight"):
        cp.capture()
    with pytest.raises(CofluxError, match="in flight"):
        cp.restore(reference_image([("a", a)], (16, 8, 2, 3)))
    image = cp.wait()
    assert image == reference_image([("a", a), ("x" * 47, b), ("nothing", a[:0])], (16, 8, 2, 3))
    other = FluxContext(16, 8, 2, 3, ic.flux_params())
    avg = other.average([other.zeros()], [other.zeros()])
    with pytest.raises(CofluxError, match="another context"):
        cp.add("avg", avg)
    many = Checkpoint(ctx)
    for k in range(256):
        many.add_array(f"s{k}", a[:0])
    with pytest.raises(CofluxError, match="256"):
        many.add_array("one_too_many", a[:0])
    avg.close()
    other.close()
    cp.close()
    many.close()


def bits_of(t):
    """The tensor's elements as integers: sentinels are NaNs, which compare unequal as floats."""
    return t.view(util.bits_dtype(t.dtype))


def guarded_like(t, offset):
    """A sentinel-filled guarded array of t's shape and dtype, `offset` elements off the allocation's alignment."""
    fill = util.SENTINEL64 if t.dtype == torch.float64 else (0x5A if t.dtype == torch.uint8 else util.SENTINEL32)
    return util.guarded(tuple(t.shape), t.dtype, offset=offset, guard=GUARD, fill=fill)


@pytest.mark.parametrize("which", ["small", "tiles", "64_in_a_tile", "slabs"])
def test_unpack_writes_every_section_and_nothing_else(small_ctx, which):
    """restore into sentinel-filled guarded arrays of another allocation whose alignment is the OTHER one (16 ↔ 8 bytes): every
    section comes back bit for bit, every byte around it keeps the sentinel; both forms, capped and uncapped."""
    ctx = small_ctx
    named = section_sets()[which]
    image = reference_image(named, (16, 8, 2, 3), b"blob")
    for direct, cap in CONFIGS:
        cp = Checkpoint(ctx, direct=direct, max_workgroups=cap)
        targets = []
        for name, t in named:
            flat = t.reshape(-1)
            if t.dtype == torch.float64:      # GUARD doubles are a multiple of 16 bytes: one double more flips the alignment
                d = guarded_like(flat, 1 if flat.data_ptr() % 16 == 0 else 2)
            else:                             # uint8 and int32 bases stay 8-byte aligned
                d = guarded_like(flat, 0 if t.dtype == torch.uint8 else 2)
            assert d.data_ptr() % 8 == 0
            if t.dtype == torch.float64 and flat.numel():
                assert d.data_ptr() % 16 != flat.data_ptr() % 16
            before = bits_of(util.buffer_of(d)[0]).clone()
            cp.add_array(name, d)
            targets.append((name, t, d, before))
        cp.restore(image)
        ctx.sync()
        assert cp.wait() is None
        for name, t, d, before in targets:
            buf, first = util.buffer_of(d)
            buf, n = bits_of(buf), d.numel()
            assert device_bytes(d) == device_bytes(t), (direct, cap, name)
            assert torch.equal(buf[:first], before[:first]) and torch.equal(buf[first + n:], before[first + n:]), (direct, cap, name)
        cp.close()


# ---------------------------------------------------------------------------------------------
# the handles' private state
# ---------------------------------------------------------------------------------------------
N_COLLECT = 10
BINS = [0, 2, 0, -1, 1, 2, 2, 0, 1, -1]
SHAPE = (131, 37, 4, 3)


class HandleRig:
    """An averager, a climatology, an integrator and a monitor on the coupled case's surface, their output arrays in guarded
    sentinel-filled buffers, and a checkpoint handle over all of it.  collect(i) is sample i of a designed sequence: the
    sources are the case's T, S, u scaled by 1 + i / 32, with an Inf planted at sample 3 and a NaN at sample 7."""

    def __init__(self, capacity=N_COLLECT, n_bins=3, n_integrals=4, direct=False, max_workgroups=0, offset=1, monitor_capacity=None,
                 handles_first=False):
        nx, ny, hx, hy = SHAPE
        case = tcs.host_case(nx, ny, hx, hy)
        self.ctx = ctx = FluxContext(nx, ny, hx, hy, ic.flux_params(ocean_minimum_salinity=cc.MIN_SALINITY, mask_kind=abi.MASK_U8))
        ocean = case["oceans"][0]
        self.base = [ctx.to_device(ocean[k]) for k in ("T", "S", "u")]
        self.src = [torch.empty_like(b) for b in self.base]
        self.mask, self.area = ctx.to_device(ocean["mask"]), ctx.to_device(case["area"])
        wet = np.argwhere(ocean["mask"][hy:hy + ny, hx:hx + nx] != 0)
        self.cells = [(int(j) + hy, int(i) + hx) for j, i in wet[[3, 40]]]
        f = lambda *lead: util.guarded(tuple(lead) + ctx.shape, torch.float64, offset=offset, guard=GUARD, fill=util.SENTINEL64)  # noqa: E731
        self.means = [f() for _ in range(3)]
        self.totals, self.bins = [f() for _ in range(2)], [f(n_bins) for _ in range(2)]
        self.average = ctx.average(self.src, self.means)
        self.climatology = ctx.climatology(self.src[:2], self.totals, self.bins, n_bins)
        entries = [("field", self.src[0]), ("product", self.src[1], self.src[2]), ("above", self.src[0], None, 1.0), ("one",)][:n_integrals]
        self.integrals = ctx.integrals(entries, area=self.area, mask=self.mask, capacity=capacity)
        self.monitor = ctx.monitor([self.src[0], (self.src[2], "abs")], mask=self.mask, capacity=monitor_capacity or capacity)
        self.cp = cp = ctx.checkpoint(direct=direct, max_workgroups=max_workgroups)
        if handles_first:    # the handles in front of the arrays they write into: a handle's own refusal is then the first one met
            cp.add("climatology", self.climatology)
            cp.add("monitor", self.monitor)
            cp.add("integrals", self.integrals)
            cp.add("average", self.average)
            for k, t in enumerate(self.arrays()):
                cp.add_array(f"array{k}", t)
            return
        for k, t in enumerate(self.means):
            cp.add_array(f"mean{k}", t)
        cp.add("average", self.average)
        for k in range(2):
            cp.add_array(f"total{k}", self.totals[k])
            cp.add_array(f"bins{k}", self.bins[k])
        cp.add("climatology", self.climatology)
        cp.add("integrals", self.integrals)
        cp.add("monitor", self.monitor)

    def collect(self, i):
        for b, s in zip(self.base, self.src):
            torch.mul(b, 1.0 + i / 32.0, out=s)
        if i == 3:
            self.src[0][self.cells[0]] = float("inf")
        if i == 7:
            self.src[2][self.cells[1]] = float("nan")
        w = 600.0 * (1 + i % 3)
        self.average.collect(w)
        self.climatology.collect(BINS[i], w)
        self.integrals.collect(1000.0 + 7.5 * i)
        self.monitor.collect(2000.0 + 0.1 * i)

    def arrays(self):
        return self.means + self.totals + self.bins

    def record(self):
        iv, it = self.integrals.read()
        mv, mt = self.monitor.read()
        total, samples, bw, bs = self.climatology.weights()
        return dict(arrays=[tcs.raw_bits(t) for t in self.arrays()], weight=self.average.weight(), clim=(total, samples, bw.tobytes(), bs.tobytes()),
                    integrals=iv.tobytes(), integral_times=it.tobytes(), monitor=mv.tobytes(), monitor_times=mt.tobytes(),
                    counts=(self.integrals.count(), self.monitor.count()), status=self.monitor.status())

    def close(self):
        for h in (self.cp, self.average, self.climatology, self.integrals, self.monitor):
            h.close()
        self.ctx.close()


def assert_same_record(got, want, what):
    assert got.keys() == want.keys()
    for k in want:
        if k == "arrays":
            for n, (g, w) in enumerate(zip(got[k], want[k])):
                assert torch.equal(g, w), f"{what}: array {n} differs in {int((g != w).sum())} words"
        else:
            assert got[k] == want[k], f"{what}: {k}"


@pytest.fixture(scope="module")
def uninterrupted():
    rig = HandleRig()
    for i in range(N_COLLECT):
        rig.collect(i)
    rec = rig.record()
    rig.close()
    assert rec["status"] == (3, 0b01) and rec["counts"] == (N_COLLECT, N_COLLECT)
    return rec


@pytest.mark.parametrize("direct", [False, True], ids=["packed", "direct"])
@pytest.mark.parametrize("split", [0, 5, N_COLLECT], ids=["empty_series", "half", "full_series"])
def test_handle_state_survives_the_destruction_of_its_context(uninterrupted, split, direct):
    """Collect `split` samples, capture, destroy every handle and the context, rebuild, restore, collect the rest: means,
    totals, bins (whole guarded buffers), cf_average_weight, cf_climatology_weights, both series with their times and counts
    and the monitor's status equal the uninterrupted run's, bit for bit — also when the series is empty or full at the capture.
    The image is the plain-Python writer's of the same state."""
    first = HandleRig(direct=direct)
    for i in range(split):
        first.collect(i)
    first.cp.set_host_blob(b"clock")
    first.cp.capture()
    image = first.cp.wait()
    checkpoint_verify(image)
    # the image against the definition, from what the public entry points give
    iv, it = first.integrals.read()
    mv, mt = first.monitor.read()
    total, samples, bw, bs = first.climatology.weights()
    status = first.monitor.status()
    by_name = {f"mean{k}": ref.section(f"mean{k}", device_bytes(t)) for k, t in enumerate(first.means)}
    for k in range(2):
        by_name[f"total{k}"] = ref.section(f"total{k}", device_bytes(first.totals[k]))
        by_name[f"bins{k}"] = ref.section(f"bins{k}", device_bytes(first.bins[k]))
    by_name["average"] = ref.section("average", ref.average_payload(*first.average.weight()), ref.KIND_AVERAGE)
    by_name["climatology"] = ref.section("climatology", ref.climatology_payload(total, samples, list(bw), [int(x) for x in bs]), ref.KIND_CLIMATOLOGY, n_entries=3)
    by_name["integrals"] = ref.section("integrals", ref.integrals_payload(iv, it), ref.KIND_INTEGRALS, n_entries=4, count=split)
    by_name["monitor"] = ref.section("monitor", ref.monitor_payload(ref.monitor_status(*status), mv.tobytes(), mt), ref.KIND_MONITOR, n_entries=2, count=split)
    assert image == ref.build_image([by_name[n] for n in first.cp.names], SHAPE, b"clock")
    first.close()
    del first
    second = HandleRig(direct=direct)
    second.cp.restore(image)
    second.ctx.sync()
    assert second.average.weight() == struct.unpack("<dq", by_name["average"]["payload"])
    assert (second.integrals.count(), second.monitor.count()) == (split, split)
    for i in range(split, N_COLLECT):
        second.collect(i)
    if split == N_COLLECT:
        with pytest.raises(CofluxError, match="full"):
            second.integrals.collect(0.0)
    assert_same_record(second.record(), uninterrupted, f"split at {split}")
    second.close()


def test_a_filling_series_does_not_make_a_capture_allocate():
    """The buffers are sized by the first capture for every series at its capacity: while the integrator's and the monitor's
    series fill from empty to full the pinned image stays where it is (an allocation inside a capture would wait for the
    device), and every image verifies."""
    rig = HandleRig()
    where, sizes = set(), []
    for i in range(N_COLLECT + 1):
        rig.cp.capture()
        view = rig.cp.wait(copy=False)
        where.add(np.frombuffer(view, dtype=np.uint8).ctypes.data)
        sizes.append(len(view))
        checkpoint_verify(view)
        if i < N_COLLECT:
            rig.collect(i)
    assert len(where) == 1 and sizes == sorted(sizes) and sizes[-1] > sizes[0]
    rig.close()


def test_every_refusal_leaves_arrays_and_handles_as_they_were():
    """An image that fails the verification, another grid, a directory that differs from the registration in name, order, kind
    or byte count, a series with more records than the capacity or other n_entries, a climatology with other n_bins: refused
    with a message that names the section; the arrays keep every bit and the handles their counts and weights."""
    first = HandleRig()
    for i in range(5):
        first.collect(i)
    first.cp.capture()
    image = first.cp.wait()
    first.close()
    header, entries, blob = ref.read_image(image)
    sections = [ref.section(e["name"], e["payload"], e["kind"], e["n_entries"], e["count"]) for e in entries]
    assert ref.build_image(sections, SHAPE, blob) == image

    def rebuilt(change):
        s = [dict(x) for x in sections]
        change(s)
        return ref.build_image(s, SHAPE, blob)

    def rename(s):
        s[1]["name"] = "mean_1"

    def swap(s):
        s[0], s[1] = s[1], s[0]

    def as_array(s):
        s[3].update(kind=ref.KIND_ARRAY)

    def shorter(s):
        s[4]["payload"] = s[4]["payload"][:-16]

    flipped = bytearray(image)
    flipped[entries[2]["offset"] + 100] ^= 4
    cases = [("payload_bit", bytes(flipped), {}, '"mean2"'), ("truncated", image[:-16], {}, "total_bytes"),
             ("grid", ref.build_image(sections, (131, 37, 4, 4), blob), {}, "grid"), ("renamed", rebuilt(rename), {}, '"mean_1"'),
             ("order", rebuilt(swap), {}, '"mean1"'), ("kind", rebuilt(as_array), {}, '"average"'), ("bytes", rebuilt(shorter), {}, '"total0"'),
             ("fewer_sections", ref.build_image(sections[:-1], SHAPE, blob), {}, "sections"),
             ("capacity", image, dict(capacity=4), '"integrals"'), ("n_entries", image, dict(n_integrals=3), '"integrals"'),
             ("n_bins", image, dict(n_bins=4), '"bins0"')]
    # the same image with the handles registered in front of their arrays: what a handle itself refuses is reached
    first = HandleRig(handles_first=True)
    for i in range(5):
        first.collect(i)
    first.cp.capture()
    handles_image = first.cp.wait()
    first.close()
    assert [e["name"] for e in ref.read_image(handles_image)[1]][:4] == ["climatology", "monitor", "integrals", "average"]
    cases += [("climatology_n_bins", handles_image, dict(handles_first=True, n_bins=4), '"climatology".* 3 bins .* 4'),
              ("monitor_capacity", handles_image, dict(handles_first=True, monitor_capacity=4), '"monitor".* 5 records'),
              ("integrals_capacity", handles_image, dict(handles_first=True, capacity=4, monitor_capacity=N_COLLECT), '"integrals".* 5 records'),
              ("integrals_n_entries", handles_image, dict(handles_first=True, n_integrals=3), '"integrals".* 4 entries')]
    rig, rig_kw = None, None
    for label, bad, kw, words in cases:
        if rig is None or kw != rig_kw:
            if rig is not None:
                rig.close()
            rig, rig_kw = HandleRig(**kw), kw
            for i in range(2):
                rig.collect(i)
        before = rig.record()
        with pytest.raises(CofluxError, match=words) as e:
            rig.cp.restore(bad)
        assert "cf_checkpoint_restore" in str(e.value), label
        rig.ctx.sync()
        assert_same_record(rig.record(), before, label)     # (cf_climatology_weights, cf_average_weight, both counts and the status among it)
    rig.close()
    # … and with nothing wrong the same rig order restores
    rig = HandleRig(handles_first=True)
    rig.cp.restore(handles_image)
    rig.ctx.sync()
    assert rig.climatology.weights()[1] == 4 and rig.monitor.count() == 5     # (sample 3 went to bin −1: four collected)
    rig.close()


# ---------------------------------------------------------------------------------------------
# the coupled step loop
# ---------------------------------------------------------------------------------------------
class LoopRun:
    """The designed coupled case with an averager, an integrator, a monitor (tests/test_coupled_steps.py's Collectors) and a
    climatology attached to the loop, and a checkpoint over every array the loop writes and every handle."""
    TABLE = (np.array([0.0, 100.0 + 4 * 1200.0, 100.0 + 9 * 1200.0, 1e6]), np.array([0, 1, 2], dtype=np.int32))

    def __init__(self, direct=False):
        self.rig = rig = tcs.Rig(tcs.host_case(131, 37, 4, 3), merged=2)
        ctx = rig.ctx
        self.out = out = tcs.Outputs(rig)
        self.col = col = tcs.Collectors(rig, out)
        self.totals, self.bins = [tcs.sentinel_field(ctx.shape)], [tcs.sentinel_field((3,) + ctx.shape)]
        self.climatology = ctx.climatology([out.net["T"]], self.totals, self.bins, 3)
        col.attach(ctx)
        ctx.attach_climatology(self.climatology, self.TABLE, stride=1, step_weight=1200.0, time_origin=100.0, step_seconds=1200.0)
        self.cp = cp = ctx.checkpoint(direct=direct)
        for name, t in sorted(out.views().items()):
            cp.add_array(name, t)
        for k, m in enumerate(col.means):
            cp.add_array(f"mean{k}", m)
        cp.add_array("clim.total", self.totals[0])
        cp.add_array("clim.bins", self.bins[0])
        cp.add("average", col.average)
        cp.add("climatology", self.climatology)
        cp.add("integrals", col.integrals)
        cp.add("monitor", col.monitor)

    def steps(self, first, n):
        sch, block = tcs.coupled_arguments(self.rig, self.out)
        self.rig.ctx.time_steps_coupled(first, n, sch, self.rig.src, self.rig.w, self.out.fl, self.out.net, self.rig.stresses, block)

    def record(self):
        self.rig.ctx.sync()
        rec = self.col.record()
        total, samples, bw, bs = self.climatology.weights()
        rec.update(out=self.out.bits(), clim=(total, samples, bw.tobytes(), bs.tobytes()), clim_arrays=[tcs.raw_bits(self.totals[0]), tcs.raw_bits(self.bins[0])],
                   status=self.col.monitor.status())
        return rec

    def close(self):
        self.cp.close()
        self.climatology.close()
        self.col.close()
        self.rig.close()


def assert_same_loop(got, want, what):
    assert got.keys() == want.keys()
    for k in want:
        if k == "out":
            tcs.assert_same_bits(got[k], want[k], what)
        elif k in ("means", "clim_arrays"):
            assert all(torch.equal(g, w) for g, w in zip(got[k], want[k])), f"{what}: {k}"
        elif isinstance(want[k], np.ndarray):
            assert np.array_equal(got[k], want[k]), f"{what}: {k}"
        else:
            assert got[k] == want[k], f"{what}: {k}"


@pytest.fixture(scope="module")
def twelve_steps():
    run = LoopRun()
    run.steps(0, cc.N_STEPS)
    rec = run.record()
    run.close()
    assert rec["counts"] == (6, 3) and rec["clim"][1] == 12
    return rec


@pytest.mark.parametrize("direct", [False, True], ids=["packed", "direct"])
def test_loop_split_by_a_checkpoint_is_the_unsplit_loop(twelve_steps, direct):
    """cf_time_steps_coupled for 12 steps == 5 steps, capture, restore into a new context, 7 steps: every output field, the
    carried skin temperature, every mean, bin, weight and record.  The image captured at step 5 while steps 6 … 12 run behind it
    is the image of a run that stops and synchronises at step 5."""
    a = LoopRun(direct=direct)
    a.steps(0, 5)
    a.cp.capture()
    a.steps(5, 7)          # issued between capture and wait: must not reach the image
    in_flight = a.cp.wait()
    assert_same_loop(a.record(), twelve_steps, "capture in the middle of a run")
    a.close()
    b = LoopRun(direct=direct)
    b.steps(0, 5)
    b.rig.ctx.sync()
    b.cp.capture()
    settled = b.cp.wait()
    b.close()
    assert in_flight == settled
    c = LoopRun(direct=direct)
    c.cp.restore(settled)
    c.rig.ctx.discard_prefetched_atmosphere_state()
    c.steps(5, 7)
    assert_same_loop(c.record(), twelve_steps, "5 + restore + 7")
    c.close()


def test_loop_restored_at_every_step_is_the_unsplit_loop(twelve_steps):
    """One capture per step, each restored into a new context that takes the next step."""
    image = None
    for s in range(cc.N_STEPS):
        run = LoopRun()
        if image is not None:
            run.cp.restore(image)
        run.steps(s, 1)
        if s + 1 < cc.N_STEPS:
            run.cp.capture()
            image = run.cp.wait()
        else:
            assert_same_loop(run.record(), twelve_steps, "restored at every step")
        run.close()


# ---------------------------------------------------------------------------------------------
# the mirror: run!(simulation; pickup = true)
# ---------------------------------------------------------------------------------------------
MIRROR_DTS = (1350.0, 1200.0)   # 3 h / 8 (a binary fraction of the snapshot interval) and 20 min


@pytest.fixture(scope="module")
def picked_up(tmp_path_factory):
    """For both time steps: run! to iteration 5 here with a Checkpointer(IterationInterval(5)), then ONE fresh child process that
    builds a new model and a new simulation for each and runs them with pickup = true to iteration 12."""
    import os
    import subprocess
    import sys

    import checkpoint_mirror as mirror
    from coflux import models as cm
    root = tmp_path_factory.mktemp("pickup")
    first = {}
    for dt in MIRROR_DTS:
        sim, normalize = mirror.simulation(dt, str(root / repr(dt)), mirror.SPLIT)
        cm.run(sim)
        assert sim.model.clock.iteration == mirror.SPLIT and sim.output_writers["checkpoint"].iterations() == [mirror.SPLIT]
        first[dt] = [t_k for t_k, _ in sim.output_writers["surface"].windows], {f"window.{t_k!r}.{k}": a.view(np.int64) for t_k, arrays in sim.output_writers["surface"].windows for k, a in arrays.items()}
        sim.output_writers["checkpoint"].close()
    out = root / "second.npz"
    child = subprocess.run([sys.executable, os.path.abspath(mirror.__file__), str(root), str(out)] + [repr(dt) for dt in MIRROR_DTS],
                           capture_output=True, text=True, timeout=300)
    assert child.returncode == 0, child.stdout[-2000:] + child.stderr[-4000:]
    return first, dict(np.load(out))


@pytest.mark.parametrize("dt", MIRROR_DTS, ids=["binary_fraction", "twenty_minutes"])
def test_mirror_pickup_in_a_fresh_process_is_the_unsplit_run(picked_up, dt):
    """run!(simulation) for 12 iterations == run! to 5 with a Checkpointer, then a new model and simulation in a fresh child
    process run with pickup = true to 12: the same fields, clocks, averaged windows (the window that ends at iteration 8
    straddles the split), series with their times, monitor status and climatology (the month turns after the split)."""
    import checkpoint_mirror as mirror
    from coflux import models as cm
    sim, normalize = mirror.simulation(dt, None, mirror.N_ITERATIONS)
    del sim.output_writers["checkpoint"]
    cm.run(sim)
    want = mirror.results(sim, normalize)
    first, second = picked_up
    ends, early_windows = first[dt]
    assert ends == [4 * dt]
    got = {k[len(repr(dt)) + 1:]: v for k, v in second.items() if k.startswith(repr(dt) + "/")}
    got.update(early_windows)     # the window delivered before the split belongs to the first process
    assert sorted(got) == sorted(want)
    assert sum(k.startswith("window.") for k in want) == 3 * 6 and want["monthly.weights"][1] == 12
    bins = want["monthly.weights"][2:14]
    assert bins[0] > 0 and bins[1] > 0     # January and February both received samples
    for k in want:
        assert got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), k


def test_mirror_pickup_without_a_file_warns_and_with_a_missing_iteration_raises(tmp_path):
    import checkpoint_mirror as mirror
    from coflux import models as cm
    sim, normalize = mirror.simulation(1350.0, str(tmp_path / "empty"), 2)
    with pytest.warns(UserWarning, match="starting from scratch"):
        cm.run(sim, pickup=True)
    assert sim.model.clock.iteration == 2
    with pytest.raises(FileNotFoundError):
        cm.run(sim, pickup=7)
    with pytest.raises(FileNotFoundError):
        cm.run(sim, pickup=str(tmp_path / "nowhere.cfck"))
    sim.output_writers["checkpoint"].close()
