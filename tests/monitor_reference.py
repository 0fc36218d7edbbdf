"""NumPy restatement of the surface monitor (include/coflux.h: cf_monitor_*): the hash, the order keys, the counts and the
indices of one cf_monitor_value, from the definitions alone.  Everything is integer arithmetic on the bits of the doubles:
the tests compare with equality, never with a tolerance."""
import numpy as np

from coflux import abi

K = np.uint64(0x9E3779B97F4A7C15)
M1, M2 = np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)
SIGN, EXPONENT = np.uint64(1 << 63), np.uint64(0x7FF0000000000000)
ALL = np.uint64(0xFFFFFFFFFFFFFFFF)
DTYPE = abi.MONITOR_VALUE_DTYPE


def bits(x):
    """the raw bits of float64 values as uint64 (same shape)"""
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def from_bits(b):
    return np.ascontiguousarray(b, dtype=np.uint64).view(np.float64)


def mix64(z):
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * M1
        z = (z ^ (z >> np.uint64(27))) * M2
    return z ^ (z >> np.uint64(31))


def cell_numbers(x, first_cell=0, row_length=0):
    """c of every cell of `x`, flattened (int64).  row_length = 0: first_cell + position in the flattened array (any shape);
    row_length > 0: `x` is (ny, nx) with nx ≤ row_length and c = first_cell + j·row_length + i."""
    if row_length == 0:
        return first_cell + np.arange(np.size(x), dtype=np.int64)
    ny, nx = np.shape(x)
    assert row_length >= nx, (row_length, nx)
    return (first_cell + np.arange(ny, dtype=np.int64)[:, None] * row_length + np.arange(nx, dtype=np.int64)[None, :]).ravel()


def cell_hashes(x, first_cell=0, row_length=0):
    """mix64(bits(x_c) XOR K·(c + 1)) per cell, c of cell_numbers"""
    b = bits(x).ravel()
    with np.errstate(over="ignore"):
        c1 = (cell_numbers(x, first_cell, row_length) + 1).astype(np.uint64) * K      # (a negative c + 1 wraps mod 2⁶⁴)
    return mix64(b ^ c1)


def state_hash(x, first_cell=0, row_length=0):
    """Σ_c mix64(bits(x_c) XOR K·(c + 1)) mod 2⁶⁴ as a Python int"""
    return int(np.add.reduce(cell_hashes(x, first_cell, row_length), dtype=np.uint64)) if np.size(x) else 0      # (uint64 sums wrap)


def order_key(b):
    """the IEEE total order of the non-NaN doubles as an unsigned order of their bits"""
    b = np.asarray(b, dtype=np.uint64)
    return np.where(b >> np.uint64(63) != 0, b ^ ALL, b ^ SIGN)


def key_value(k):
    k = np.asarray(k, dtype=np.uint64)
    return from_bits(np.where(k >> np.uint64(63) != 0, k ^ SIGN, k ^ ALL))


def monitor_value(x, wet=None, kind="value", first_cell=0, row_length=0):
    """One cf_monitor_value (a numpy record of abi.MONITOR_VALUE_DTYPE) of the interior array `x` (any shape, row-major cell
    numbering; (ny, nx) with row_length > 0: cell_numbers) under the boolean / uint8 array `wet` (None: all wet)."""
    b = bits(x).ravel()
    c = cell_numbers(x, first_cell, row_length)
    w = np.ones(b.size, bool) if wet is None else np.asarray(wet).ravel() != 0
    mag = b & ~SIGN
    nan, inf = mag > EXPONENT, mag == EXPONENT
    out = np.zeros((), dtype=DTYPE)
    out["nan_count"], out["inf_count"] = int((w & nan).sum()), int((w & inf).sum())
    bad = np.flatnonzero(w & (nan | inf))
    out["first_nonfinite"] = int(c[bad[0]]) if bad.size else -1
    keys = order_key(mag if kind in ("abs", abi.MONITOR_ABS) else b)
    sel = np.flatnonzero(w & ~nan)
    if sel.size:
        k = keys[sel]
        lo, hi = k.min(), k.max()
        out["minimum"], out["maximum"] = key_value(lo), key_value(hi)
        out["argmin"] = int(c[sel[np.flatnonzero(k == lo)[0]]])      # the smallest c that holds it (c grows with the position)
        out["argmax"] = int(c[sel[np.flatnonzero(k == hi)[0]]])
    else:
        out["minimum"], out["maximum"], out["argmin"], out["argmax"] = np.inf, -np.inf, -1, -1
    out["hash"] = state_hash(x, first_cell, row_length)
    return out


def combine(a, b):
    """the host's combination of two slabs' values (the header's `Slabs`)"""
    out = np.zeros((), dtype=DTYPE)
    key = lambda v: int(order_key(bits(v).ravel()[0]))  # noqa: E731
    ka, kb = key(a["minimum"]), key(b["minimum"])
    lo = min((x for x in ((ka, int(a["argmin"]), a), (kb, int(b["argmin"]), b)) if x[1] >= 0), key=lambda x: x[:2], default=None)
    ka, kb = key(a["maximum"]), key(b["maximum"])
    hi = min((x for x in ((-ka, int(a["argmax"]), a), (-kb, int(b["argmax"]), b)) if x[1] >= 0), key=lambda x: x[:2], default=None)
    out["minimum"], out["argmin"] = (lo[2]["minimum"], lo[1]) if lo else (np.inf, -1)
    out["maximum"], out["argmax"] = (hi[2]["maximum"], hi[1]) if hi else (-np.inf, -1)
    out["nan_count"], out["inf_count"] = a["nan_count"] + b["nan_count"], a["inf_count"] + b["inf_count"]
    first = [int(v["first_nonfinite"]) for v in (a, b) if v["first_nonfinite"] >= 0]
    out["first_nonfinite"] = min(first) if first else -1
    out["hash"] = (int(a["hash"]) + int(b["hash"])) % (1 << 64)
    return out


def same(a, b):
    """bitwise equality of two values / arrays of values (NaN-safe: compares the bytes)"""
    a, b = np.ascontiguousarray(a, dtype=DTYPE), np.ascontiguousarray(b, dtype=DTYPE)
    return a.shape == b.shape and a.tobytes() == b.tobytes()
