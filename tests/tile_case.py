"""The worlds, shapes and stamped fields of the tile-world tests (tests/test_tile_world_cpu.py, tests/test_tile_halo.py): a global
halo-inclusive array per field — periodic in x, the tripolar fold beyond the top row by coflux.synthetic.fold_north — whose
every interior element is a bit pattern naming its field, global column and global row; the tiles cut from it with every
halo cell a neighbour, a partner or the fold must deliver overwritten by a pattern naming rank, field and local cell; and the
cells an exchange DEFINES (include/coflux.h: cf_halo_exchange_tile_peer, footprint), which are compared with the global array."""
import numpy as np

from coflux import synthetic as syn
from coflux.distributed import tile_bounds, tile_coords

HX, HY, RING = 4, 3, 1
ROWS = COLS = RING + 1

# (location, sign) of the eight fields an exchange carries at most: every location with either sign; field 6 holds ±0.0 on the
# rows the fold reads and on global column 0 (the |sign| rule on the fold axis, and −1 · 0.0 = −0.0)
FIELDS = (("center", 1.0), ("x_face", -1.0), ("y_face", -1.0), ("center", -1.0), ("x_face", 1.0), ("y_face", 1.0), ("x_face", -1.0), ("center", 1.0))
ZEROS_FIELD = 6


def shapes(py):
    """(tile width nxl, global ny): 3 × 3 tiles, the least the geometry admits (nxl ≥ ring + 2 where a fold is sent, ny ≥ ring + 2
    under the fold); 32 × 12 tiles; 34 columns on unequal row blocks of a global ny that is no multiple of py (7 where py = 1)"""
    return [(3, 3 * py), (32, 12 * py), (34, 6 * py + 1)]


def stamp(f, gcol, grow):
    """an exact double < 2^44 that names (field, global column, global row)"""
    return ((f + 1) * 2.0 ** 40 + gcol * 2.0 ** 20 + (grow + 1)).astype(np.float64)


def poison(rank, f, shape):
    """exact doubles ≥ 2^52 that name (rank, field, local row, local column): no stamp, no product ±1 · stamp equals one"""
    lj, li = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), indexing="ij")
    return 2.0 ** 52 + rank * 2.0 ** 44 + f * 2.0 ** 40 + lj * 2.0 ** 20 + li


def global_fields(nxg, nyg, nfields, tripolar, call=0):
    """[field] → (nyg + 2HY, nxg + 2HX): stamped interior (`call` moves the rows' stamps: two exchanges carry different bits),
    x-halos the periodic image, y-halos NaN — nobody defines them — but the fold's rows on a tripolar world"""
    out = []
    cols = np.arange(-HX, nxg + HX) % nxg
    for f in range(nfields):
        gcol, grow = np.meshgrid(np.arange(nxg), np.arange(nyg))
        interior = stamp(f, gcol, grow + 1000 * call)
        if f == ZEROS_FIELD:
            zero = np.where((gcol + grow) % 2 == 0, 0.0, -0.0)
            interior = np.where((grow >= nyg - 1 - ROWS) | (gcol == 0), zero, interior)
        g = np.full((nyg + 2 * HY, nxg + 2 * HX), np.nan)
        g[HY:HY + nyg] = interior[:, cols]
        if tripolar:
            syn.fold_north(g, nxg, nyg, HX, HY, ROWS, *FIELDS[f])
        out.append(g)
    return out


def cut_tiles(fields, nxg, nyg, px, py):
    """[rank][field] → the tile's halo-inclusive array with its halos poisoned.  With px = 1 the x-halo columns of the interior
    rows keep the global's values: they stay the caller's, who wraps them."""
    tiles = []
    for rank in range(px * py):
        i0, i1, j0, j1 = tile_bounds(nxg, nyg, rank, px, py)
        mine = []
        for f, g in enumerate(fields):
            t = poison(rank, f, (j1 - j0 + 2 * HY, i1 - i0 + 2 * HX))
            keep = slice(HX, HX + i1 - i0) if px > 1 else slice(None)
            t[HY:HY + j1 - j0, keep] = g[HY + j0:HY + j1, i0:i1 + 2 * HX][:, keep]
            mine.append(t)
        tiles.append(mine)
    return tiles


def defined_window(rank, px, py, ny, tripolar):
    """(rows, columns) of the tile's array an exchange defines: within ring + 1 of the interior, corners included, except beyond
    the world's south edge and, without a fold, beyond its north edge"""
    _p, q = tile_coords(rank, px)
    lo = HY - (ROWS if q > 0 else 0)
    hi = HY + ny + (ROWS if q < py - 1 or tripolar else 0)
    return slice(lo, hi), slice(HX - COLS, None if COLS == HX else -(HX - COLS))


def same_bits(a, b):
    return np.asarray(a, np.float64).view(np.int64) == np.asarray(b, np.float64).view(np.int64)
