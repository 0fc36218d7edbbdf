"""Designed wet masks for the solver's index machinery, and the NumPy statement of the chunk table.

The flux solver never sees (i, j): it sees the ring-inclusive WINDOW as one row-major run of cells, idx = jj · wx + ii
(wx = nx + 2 · ring), cut into chunks by a cost-balanced table (csrc/coflux_solver.hip: a wet cell costs `unit`, a land
cell 1).  Every mask here puts wet cells where that machinery can go wrong — on a chunk or batch edge, behind a land run
longer than the strips a workgroup requests up front, in the last cell, only in the ring — and `reference_partition`
says where the table's cuts must then fall.  A plain module: imported by tests/test_mask_atlas.py."""
import numpy as np

from coflux import synthetic as syn

RING, HALO = 1, 3
LAND_RUN = 3000        # longer than the 8 × 256 cells a workgroup's start phase requests up front
K256, K64 = 3, 5       # first_256k*: 256 · 3 cells; first_64k_plus1: 64 · 5 + 1

# the smallest shapes that reach each mechanism (nx, ny); halo 3, ring 1
SHAPES = {
    "base": (131, 37),       # 133 × 39 = 5187 window cells, about 21 chunks of 256: ordinary chunking
    "narrow": (2, 700),      # wx = 4: the row arithmetic with a tiny divisor
    "split": (300, 222),     # 67 648 cells: more than 64 builder blocks, more than 256 × 256 wet cells
    "layered": (640, 322),   # 208 008 cells: more than 3 × 256 × 256 wet cells, the 768 / 512 arrival layers
}

U8_WET_BYTES = np.array([1, 2, 255], dtype=np.uint8)   # kernel and oracle both test != 0


def window_shape(nx, ny, ring=RING):
    return nx + 2 * ring, ny + 2 * ring


def blob_window(wx, wy, ring=RING, halo=HALO):
    """Today's synthetic mask (coflux.synthetic: about 30 % land in blobs, 2 % specks) on the window."""
    nx, ny = wx - 2 * ring, wy - 2 * ring
    mask = syn.ocean_state(nx, ny, halo, halo)["mask"] != 0
    return np.ascontiguousarray(mask[halo - ring:halo + ny + ring, halo - ring:halo + nx + ring])


def atlas(wx, wy, ring=RING, halo=HALO, only=None):
    """Yields (name, wet): `wet` a boolean (wy, wx) array over the ring-inclusive window, row-major = the solver's index
    order.  `only`: names to keep (the rest is not built)."""
    n = wx * wy
    idx = np.arange(n).reshape(wy, wx)
    jj, ii = np.divmod(idx, wx)

    def first(m):
        return idx < m

    frame = (ii < ring) | (ii >= wx - ring) | (jj < ring) | (jj >= wy - ring)
    corners = ((ii == 0) | (ii == wx - 1)) & ((jj == 0) | (jj == wy - 1))
    entries = (
        ("single_first", lambda: idx == 0),
        ("single_last", lambda: idx == n - 1),
        ("four_corners", lambda: corners),
        ("checkerboard", lambda: (ii + jj) % 2 == 0),
        ("odd_columns", lambda: ii % 2 == 1),
        ("odd_rows", lambda: jj % 2 == 1),
        ("one_row", lambda: jj == wy // 2),
        ("one_column", lambda: ii == wx // 2),
        ("ring_only", lambda: frame),
        ("interior_only", lambda: ~frame),
        ("first_256k", lambda: first(256 * K256)),
        ("first_256k_plus1", lambda: first(256 * K256 + 1)),
        ("first_256k_minus1", lambda: first(256 * K256 - 1)),
        ("first_64k_plus1", lambda: first(64 * K64 + 1)),
        ("land_run_then_wet", lambda: idx >= LAND_RUN),
        ("wet_then_land_run", lambda: idx < n - LAND_RUN),
        ("every_97th", lambda: idx % 97 == 0),
        ("blob", lambda: blob_window(wx, wy, ring, halo)),
    )
    for name, make in entries:
        if only is None or name in only:
            yield name, np.ascontiguousarray(np.broadcast_to(make(), (wy, wx)).astype(bool))


ATLAS_NAMES = tuple(name for name, _ in atlas(8, 8))


def embed(wet, nx, ny, hx=HALO, hy=HALO, ring=RING, kind="u8", z_surface=0.0):
    """The halo-inclusive mask array of a window `wet`, land outside the window.  kind "u8": wet bytes drawn from
    {1, 2, 255} by index, land 0.  kind "bottom_height": float64 bottom heights, wet −3000.0, land alternately +10.0 and
    exactly `z_surface` (equality is land: a cell is wet only where NOT z_surface <= bottom height)."""
    wx, wy = window_shape(nx, ny, ring)
    assert wet.shape == (wy, wx) and wet.dtype == bool
    idx = np.arange(wx * wy).reshape(wy, wx)
    win = (slice(hy - ring, hy + ny + ring), slice(hx - ring, hx + nx + ring))
    if kind == "u8":
        out = np.zeros((ny + 2 * hy, nx + 2 * hx), dtype=np.uint8)
        out[win] = np.where(wet, U8_WET_BYTES[idx % 3], 0)
    else:
        assert kind == "bottom_height"
        out = np.full((ny + 2 * hy, nx + 2 * hx), 10.0)
        out[win] = np.where(wet, -3000.0, np.where(idx % 2 == 0, 10.0, float(z_surface)))
    return out


def reference_partition(wet, rounds, unit, with_sizes=False):
    """The chunk table in NumPy.  `rounds`: the (wet cells per chunk, number of chunks) list of cf_debug_chunk_plan, `unit`
    its return value.  A cell costs `unit` when wet, else 1; `prefix` is the exclusive cumulative cost; a cell's chunk id is
    first_r + (prefix − base_r) // (w_r · unit), base_r and first_r accumulated over the rounds, the last round open-ended;
    the begins are the indices where the id changes, led by 0 and closed by the cell count.
    → (begins [n + 1], wet cells per chunk [n]) and, with_sizes, each chunk's round size w_r."""
    flat = np.asarray(wet, dtype=bool).reshape(-1)
    cost = np.where(flat, int(unit), 1).astype(np.int64)
    prefix = np.cumsum(cost) - cost
    ids = np.empty(flat.size, dtype=np.int64)
    size_of = np.empty(flat.size, dtype=np.int64)
    base, first_id = 0, 0
    for r, (w, count) in enumerate(rounds):
        last = r == len(rounds) - 1
        end = None if last else base + count * w * unit
        sel = prefix >= base if last else (prefix >= base) & (prefix < end)
        ids[sel] = first_id + (prefix[sel] - base) // (w * unit)
        size_of[sel] = w
        if not last:
            base, first_id = end, first_id + count
    change = np.flatnonzero(ids[1:] != ids[:-1]) + 1
    begins = np.concatenate(([0], change, [flat.size])).astype(np.int64)
    counts = np.add.reduceat(flat.astype(np.int64), begins[:-1])
    if with_sizes:
        return begins, counts, size_of[begins[:-1]]
    return begins, counts
