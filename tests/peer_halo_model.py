"""The peer-direct halo rows (include/coflux.h: cf_peer_halo_*) as a protocol model, a world and a sequence, in plain NumPy.

THE MODEL restates the mailbox protocol as the header and csrc/coflux_halo_device.hpp state it.  Every rank owns a mailbox:
four sequence numbers [side][parity] and, behind them, four slots [side][parity] of max_fields · max_rows · sj doubles (side 0:
what the south neighbour sent, side 1: the north neighbour; parity: the exchange's sequence number mod 2).  An exchange of
`fields` × `rows` lays its rows out at the head of the slot as [field][row][sj] WITH THE CALL'S OWN `rows`; the tail of the
slot keeps whatever an earlier exchange left there.  send() stores this rank's boundary rows into the neighbour's slot and
then the sequence number; receive() finds the number (a number that is not there is a wait that would run into its bound:
ModelTimeout) and copies the rows into the halo rows.  Both are slice assignments on reshaped views of the slot, not loops
over lanes: the model is the definition under test, not a copy of the kernel.

THE WORLD: nx = 13, hx = 2, hy = 3 — sj = 17 is odd, so every per-field and per-row offset is an odd multiple of 8 bytes, and
hx != hy; three ranks of 3, 5 and 4 rows (rank 0: ny == hy, so rows == ny occurs; the middle rank sends and receives on both
sides) or two ranks of 3 and 4 rows; every mailbox exported for 8 fields × 3 rows.

THE SEQUENCE: eleven exchanges that one connected world runs from first to last, so that sequence numbers and parities
carry over; shapes shrink and grow inside every (side, parity) slot, and the first fills the whole mailbox.

CONTENT: every element of every field of every call is a bit pattern of its own that names (rank, call, field, row, column)
— decode() reads it back, so a wrong element says where it came from — in the number classes a copy could mistreat: NaNs of
both signs with payloads, subnormals of both signs, normal numbers, and in the boundary rows −0.0 and ±Inf (those three are
what they are and name nothing; they sit in columns that move with field, row and call).  The halo rows hold such patterns
too, marked as sentinels.  THE EXPECTATION is a plain slice copy between the ranks' arrays; everything is compared as uint64.

run() plays the sequence in the order a legal run can take: the even ranks run one send ahead — rank r sends exchange s + 1
as soon as it has received exchange s, before its neighbours have drained exchange s from their own mailboxes.  That is what
the two parity slots are for, and the only schedule under which a model without them is wrong."""
import numpy as np

NX, HX, HY = 13, 2, 3
SJ = NX + 2 * HX
HEIGHTS = {3: (3, 5, 4), 2: (3, 4)}
MAX_FIELDS, MAX_ROWS = 8, 3
HELD = 8                        # every rank holds eight fields, whether a call passes them or not
SEQUENCE = ((8, 3), (1, 1), (1, 1), (3, 2), (8, 1), (5, 3), (4, 2), (4, 2), (4, 2), (2, 3), (7, 2))
SOUTH, NORTH = 0, 1

# Each flag makes the model wrong in one way (tests/test_peer_halo_atlas.py seeds them one at a time)
DEFECTS = (
    "field_stride_max_rows",     # the sender places field f at f · max_rows · sj instead of f · rows · sj
    "row_length_nx",             # a row is nx doubles long, not sj: the exchange moves nx of the sj columns
    "row_length_nx_plus_hx",     # … nx + hx doubles
    "parity_stuck",              # the parity does not alternate: one slot per side
    "side_swapped_on_send",      # the sender stores into the neighbour's slot of its OWN direction, not the opposite one
    "north_send_first_row",      # the rows sent north start one row too far south
    "south_receive_first_row",   # the rows received from the south land one row too far north
    "receive_max_rows",          # the receiver copies max_rows rows per field whatever the call says
    "send_skips_field_4_up",     # the sender stores fields 0…3 only
)


class ModelTimeout(Exception):
    """receive() before the neighbour's send(): on the device, a wait that runs into its bound"""


# ---------------------------------------------------------------------------------------------
# content: one bit pattern per element
# ---------------------------------------------------------------------------------------------
_MARK = 0x3C3C3                  # low 20 bits of every pattern (never zero: a NaN stays a NaN, a subnormal stays one)
_CLASS_BITS = (0x7FF8 << 48, 0xFFF8 << 48, 0x0000 << 48, 0x8000 << 48, 0x3FF0 << 48, 0xC010 << 48, 0x4340 << 48)
_CLASS_NAMES = ("+NaN", "-NaN", "+subnormal", "-subnormal", "normal", "normal", "normal")
_LITERALS = {0x8000000000000000: "-0.0", 0x7FF0000000000000: "+Inf", 0xFFF0000000000000: "-Inf"}
GUARD_BITS = 0x7FF8DEADBEEF5A5A   # (util.SENTINEL64: what the guard space around a device view holds)


def _code(rank, call, field, row, col, halo):
    return (((((halo * 4 + rank) * 16 + call) * 8 + field) * 16 + row) * 32 + col)


def fill(heights, call):
    """[rank] → (HELD, ny + 2hy, sj) uint64: what the fields of every rank hold before exchange `call` (1-based)"""
    out = []
    for rank, ny in enumerate(heights):
        f, j, i = np.meshgrid(np.arange(HELD), np.arange(ny + 2 * HY), np.arange(SJ), indexing="ij")
        halo = ((j < HY) | (j >= HY + ny)).astype(np.int64)
        code = _code(rank, call, f, j, i, halo).astype(np.uint64)
        cls = (i + 2 * j + 3 * f + call) % len(_CLASS_BITS)
        a = np.array(_CLASS_BITS, dtype=np.uint64)[cls] | (code << np.uint64(20)) | np.uint64(_MARK)
        boundary = (halo == 0) & ((j < HY + MAX_ROWS) | (j >= HY + ny - MAX_ROWS))
        where = (i + f + 2 * j + call) % SJ
        for k, literal in enumerate(_LITERALS):
            a[boundary & (where == k)] = np.uint64(literal)
        out.append(a)
    return out


def decode(bits):
    """what a bit pattern is: the (rank, call, field, row, column) it was made for, or what else"""
    bits = int(bits)
    if bits in _LITERALS:
        return _LITERALS[bits] + " (a boundary row's literal)"
    if bits == 0:
        return "0 (a mailbox as exported)"
    if bits == GUARD_BITS:
        return "the guard sentinel"
    if bits & 0xFFFFF != _MARK or (bits & ((1 << 48) - 1)) >> 39:      # (the code is 19 bits: 20 … 38)
        return "no pattern of this atlas: %#018x" % bits
    code = (bits >> 20) & ((1 << 19) - 1)
    top = bits & (0xFFFF << 48)
    if top not in _CLASS_BITS:
        return "no pattern of this atlas: %#018x" % bits
    col, row, field, call, rank, halo = code % 32, code // 32 % 16, code // 512 % 8, code // 4096 % 16, code // 65536 % 4, code // 262144
    return dict(rank=rank, call=call, field=field, row=row, column=col, kind="halo sentinel" if halo else "interior",
                number=_CLASS_NAMES[_CLASS_BITS.index(top)])


def expectation(heights, before, fields, rows):
    """[rank] → arrays after an exchange of `fields` × `rows`: a slice copy between the ranks' arrays, nothing else"""
    after = [a.copy() for a in before]
    for r, ny in enumerate(heights):
        if r > 0:
            south_ny = heights[r - 1]
            after[r][:fields, HY - rows:HY, :] = before[r - 1][:fields, HY + south_ny - rows:HY + south_ny, :]
        if r < len(heights) - 1:
            after[r][:fields, HY + ny:HY + ny + rows, :] = before[r + 1][:fields, HY:HY + rows, :]
    return after


# ---------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------
class Mailboxes:
    """The mailboxes of one world.  send() and receive() work on `arrays`: the (fields, ny + 2hy, sj) uint64 fields a rank
    passes to one call; receive() writes into them."""

    def __init__(self, heights, max_fields=MAX_FIELDS, max_rows=MAX_ROWS, defect=None):
        assert defect is None or defect in DEFECTS, defect
        self.heights, self.world = tuple(heights), len(heights)
        self.max_fields, self.max_rows, self.defect = max_fields, max_rows, defect
        self.slot = max_fields * max_rows * SJ
        self.number = [np.zeros((2, 2), np.uint64) for _ in heights]          # [rank][side, parity]
        self.data = [np.zeros((2, 2, self.slot), np.uint64) for _ in heights]  # [rank][side, parity, field · row · sj]

    def _neighbour(self, rank, direction):
        n = rank - 1 if direction == SOUTH else rank + 1
        return n if 0 <= n < self.world else None

    def _parity(self, seq):
        return 0 if self.defect == "parity_stuck" else seq & 1

    def _row_length(self):
        return {"row_length_nx": NX, "row_length_nx_plus_hx": NX + HX}.get(self.defect, SJ)

    def send(self, rank, direction, arrays, rows, seq):
        to = self._neighbour(rank, direction)
        if to is None:
            return
        fields, ny, length = len(arrays), self.heights[rank], self._row_length()
        first = HY if direction == SOUTH else HY + ny - rows
        if self.defect == "north_send_first_row" and direction == NORTH:
            first -= 1
        side = direction if self.defect == "side_swapped_on_send" else 1 - direction   # seen from there, the opposite side
        slot = self.data[to][side, self._parity(seq)]
        mine = arrays[:, first:first + rows, :length]
        if self.defect == "send_skips_field_4_up":
            fields = min(fields, 4)
            mine = mine[:fields]
        if self.defect == "field_stride_max_rows":
            slot[:fields * self.max_rows * SJ].reshape(fields, self.max_rows, SJ)[:, :rows, :] = mine
        else:
            slot[:fields * rows * length].reshape(fields, rows, length)[...] = mine
        self.number[to][side, self._parity(seq)] = seq     # behind the rows: a release

    def receive(self, rank, direction, arrays, rows, seq):
        if self._neighbour(rank, direction) is None:
            return
        parity = self._parity(seq)
        if self.number[rank][direction, parity] < seq:
            raise ModelTimeout(f"rank {rank} waits for exchange {seq} from the {'south' if direction == SOUTH else 'north'}: "
                               f"its mailbox holds {int(self.number[rank][direction, parity])}")
        fields, ny, length = len(arrays), self.heights[rank], self._row_length()
        if self.defect == "receive_max_rows":
            rows = self.max_rows
        first = HY - rows if direction == SOUTH else HY + ny
        if self.defect == "south_receive_first_row" and direction == SOUTH:
            first += 1
        slot = self.data[rank][direction, parity]
        arrays[:, first:first + rows, :length] = slot[:fields * rows * length].reshape(fields, rows, length)


def run(heights, sequence, contents, max_fields=MAX_FIELDS, max_rows=MAX_ROWS, defect=None):
    """The model's world plays `sequence` ((fields, rows) per exchange); contents(call) → what the ranks' fields hold before
    exchange `call`.  Returns [exchange][rank] → the (HELD, ny + 2hy, sj) arrays afterwards, or None from the exchange on at
    which a rank's wait found nothing (that rank stops there, as a worker does).  Even ranks run one send ahead (module text)."""
    world = len(heights)
    boxes = Mailboxes(heights, max_fields, max_rows, defect)
    held = {s: contents(s) for s in range(1, len(sequence) + 1)}
    evens, odds = range(0, world, 2), range(1, world, 2)

    def send(r, s):
        fields, rows = sequence[s - 1]
        for direction in (SOUTH, NORTH):
            boxes.send(r, direction, held[s][r][:fields], rows, s)

    def receive(r, s):
        fields, rows = sequence[s - 1]
        for direction in (SOUTH, NORTH):
            boxes.receive(r, direction, held[s][r][:fields], rows, s)

    results = []
    try:
        for r in evens:
            send(r, 1)
        for s in range(1, len(sequence) + 1):
            for r in odds:
                send(r, s)
            for r in evens:
                receive(r, s)
            if s < len(sequence):
                for r in evens:
                    send(r, s + 1)       # … before the odd ranks have drained exchange s
            for r in odds:
                receive(r, s)
            results.append(held[s])
    except ModelTimeout:
        results += [None] * (len(sequence) - len(results))
    return results
