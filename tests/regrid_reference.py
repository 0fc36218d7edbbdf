"""References for the sparse surface operator (include/coflux.h: cf_regrid_*), shared by test_regrid_cpu.py and test_regrid.py.

definition()    the definition per row: with W the entries of the row whose source cell is wet, N_f = Σ_{k∈W} w_k · x_f[col_k]
                and D = Σ_{k∈W} w_k as math.fsum of EXACT terms (every product w · x is split into its rounded value and its
                rounding error by Dekker's two-product, so fsum returns the correctly rounded exact sum), and Σ|w · x| for
                the bound.
bound()         (2n + 4) · 2⁻⁵³ · Σ|w·x| / D for the mean of a row of n wet entries: n rounded products and n − 1 rounded
                additions in the numerator, n − 1 additions in the denominator, one division — to first order
                2n · 2⁻⁵³ · Σ|w·x| / D; the + 4 covers the second-order terms (and the reference's own final rounding).
                Without the division (SUM mode, and the coverage with x ≡ 1) the same count times Σ|w·x|.
order_model()   a NumPy model of the summation order stated in csrc/coflux_regrid.hip, one IEEE operation per NumPy
                operation: it reproduces the device's bits.  `defect` plants one of DEFECTS, for the tests that show the
                atlas catches each of them.
"""
import math

import numpy as np

EPS = 2.0 ** -53
SHORT, SEGMENT = 64, 256
MEAN, SUM = 0, 1
DEFECTS = ("drops_last_partial_segment", "off_by_one_at_64", "off_by_one_at_256", "nx_instead_of_pitch",
           "land_multiplied_by_zero", "coverage_includes_land")


def two_product(a, b):
    """p, e with p = fl(a · b) and p + e = a · b exactly (Veltkamp / Dekker; no overflow or underflow in the tests' ranges)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    p = a * b
    split = 134217729.0   # 2^27 + 1
    ca, cb = split * a, split * b
    ah, bh = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


def offsets(col, grid, pitch=None):
    """halo-layout element offsets of interior cell numbers c = j · nx + i"""
    nx, ny, hx, hy = grid
    col = np.asarray(col, dtype=np.int64)
    j, i = col // nx, col % nx
    return (j + hy) * (nx + 2 * hx if pitch is None else pitch) + (i + hx)


def definition(row_ptr, col, weight, fields, wet, grid, rows=None):
    """Per row r (all rows, or `rows`): dict(N=[per field], D, abs=[Σ|w·x| per field], n=wet entries).  fields: halo-layout
    2-D arrays; wet: halo-layout boolean array or None (all wet)."""
    flat = [np.asarray(f, dtype=np.float64).ravel() for f in fields]
    wet_flat = None if wet is None else np.asarray(wet).ravel() != 0
    weight = np.asarray(weight, dtype=np.float64)
    out = []
    for r in (range(len(row_ptr) - 1) if rows is None else rows):
        k = slice(int(row_ptr[r]), int(row_ptr[r + 1]))
        off, w = offsets(col[k], grid), weight[k]
        if wet_flat is not None:
            keep = wet_flat[off]
            off, w = off[keep], w[keep]
        N, A = [], []
        for x in flat:
            p, e = two_product(w, x[off])
            N.append(math.fsum(p.tolist() + e.tolist()))
            A.append(math.fsum(np.abs(p).tolist()))
        out.append(dict(N=N, D=math.fsum(w.tolist()), abs=A, n=int(w.size)))
    return out


def expected(d, f, mode):
    """the definition's value of field f for the row record d"""
    if mode == SUM:
        return d["N"][f]
    return d["N"][f] / d["D"] if d["D"] > 0 else float("nan")


def bound(d, f, mode):
    n, D = d["n"], d["D"]
    if mode == SUM or D == 0:
        return (2 * n + 4) * EPS * d["abs"][f]
    return (2 * n + 4) * EPS * d["abs"][f] / D


def coverage_bound(d):
    return (2 * d["n"] + 4) * EPS * d["D"]


def _butterfly(v, width):
    off = width // 2
    idx = np.arange(width)
    while off >= 1:
        v = v + v[idx ^ off]
        off //= 2
    return v[0]


def _span(terms, width):
    """`width` lanes, lane g adds terms g, g + width, g + 2·width, g + 3·width to +0.0 (absent: +0.0), then the butterfly"""
    t = np.zeros(4 * width)
    t[:terms.size] = terms
    t = t.reshape(4, width)
    acc = np.zeros(width)
    for u in range(4):
        acc = acc + t[u]
    return _butterfly(acc, width)


def _row_sum(terms, defect=None):
    """Σ terms in the stated order of a row of terms.size entries (excluded entries are +0.0 terms)"""
    n = terms.size
    if n <= (SHORT + 1 if defect == "off_by_one_at_64" else SHORT):    # the defect: a row of 65 goes to 16 lanes · 4 entries
        return _span(terms[:SHORT], 16)
    n_segments = (n + SEGMENT - 1) // SEGMENT
    if defect == "off_by_one_at_256":                                  # ceil((n − 1) / 256): a row of 257 gets one segment
        n_segments = (n - 1 + SEGMENT - 1) // SEGMENT
    if defect == "drops_last_partial_segment":
        n_segments = n // SEGMENT
    total = None
    for s in range(n_segments):
        p = _span(terms[s * SEGMENT:(s + 1) * SEGMENT], 64)
        total = p if total is None else total + p
    return 0.0 if total is None else total


def order_model(row_ptr, col, weight, fields, wet, grid, mode=MEAN, defect=None, rows=None):
    """(dst[f][r], coverage[r]) with the bits the device produces.  Same arguments as definition()."""
    nx, ny, hx, hy = grid
    flat = [np.asarray(f, dtype=np.float64).ravel() for f in fields]
    wet_flat = None if wet is None else np.asarray(wet).ravel() != 0
    weight = np.asarray(weight, dtype=np.float64)
    rows = list(range(len(row_ptr) - 1) if rows is None else rows)
    dst, cov = np.zeros((len(flat), len(rows))), np.zeros(len(rows))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for q, r in enumerate(rows):
            k = slice(int(row_ptr[r]), int(row_ptr[r + 1]))
            off, w = offsets(col[k], grid, pitch=nx if defect == "nx_instead_of_pitch" else None), weight[k]
            keep = np.ones(w.size, dtype=bool) if wet_flat is None else wet_flat[off]
            D = _row_sum(w if defect == "coverage_includes_land" else np.where(keep, w, 0.0), defect)
            cov[q] = D
            for f, x in enumerate(flat):
                terms = (w * x[off]) * keep if defect == "land_multiplied_by_zero" else np.where(keep, w * x[off], 0.0)
                N = _row_sum(terms, defect)
                dst[f, q] = N if mode == SUM else (N / D if D != 0 else np.nan)
    return dst, cov


def same_bits(a, b):
    """bit for bit, every NaN standing for every other (the payload of a propagated NaN is the hardware's)"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.int64), b[~nan].view(np.int64))


# ---- the operator atlas: a 67 × 5 source, every row a named case ------------------------------------------------------------
ATLAS_NX, ATLAS_NY = 67, 5
ATLAS_COUNTS = (0, 1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1025)
POISON = (float("nan"), 7.0e77)


def build_atlas(seed=20261018, n_fields=16):
    """dict(row_ptr, col, weight, names {name: row}, wet (ny, nx) uint8, fields [n_fields × (ny, nx)], zb (ny, nx)).
    Rows of ATLAS_COUNTS entries over wet cells with repeated columns ("n<count>"); wet entries of weight 0 ("zero_weight");
    "all_land"; "partly_land" (short) and "partly_land_long"; "corners" (the four interior corners) and "row_ends" (both ends
    of every interior row); "descending" columns; one short and one long partly-land row stored three times each
    ("same_short_a/b/c", "same_long_a/b/c") at the start, in the middle and at the end of the operator.  Field 0 is positive
    (a lost entry cannot hide in cancellation), the others are signed; weights are positive areas of order 1e9."""
    rng = np.random.default_rng(seed)
    nx, ny = ATLAS_NX, ATLAS_NY
    wet = (rng.random((ny, nx)) < 0.7).astype(np.uint8)
    wet[:, 0] = wet[:, -1] = 1
    wet_cells, land_cells = np.flatnonzero(wet.ravel()), np.flatnonzero(wet.ravel() == 0)
    fields = [1.0 + rng.random((ny, nx))] + [rng.standard_normal((ny, nx)) * 10.0 ** rng.integers(-2, 3) for _ in range(n_fields - 1)]
    zb = np.where(wet != 0, -4000.0 * (0.05 + rng.random((ny, nx))), 10.0 * rng.random((ny, nx)))   # land: at or above the surface

    def weights(n):
        return (0.5 + rng.random(n)) * 1.0e9

    def mixed(n):
        c = np.concatenate([rng.choice(wet_cells, n - n // 3), rng.choice(land_cells, n // 3)])
        return rng.permutation(c), weights(n)

    same_short, same_long = mixed(37), mixed(300)
    rows = [("same_short_a", *same_short), ("same_long_a", *same_long)]
    for n in ATLAS_COUNTS:
        rows.append((f"n{n}", rng.choice(wet_cells, n), weights(n)))
    rows.append(("zero_weight", rng.choice(wet_cells, 20), np.zeros(20)))
    rows.append(("all_land", rng.choice(land_cells, 12), weights(12)))
    rows.append(("partly_land", *mixed(40)))
    rows.append(("same_short_b", *same_short))
    rows.append(("same_long_b", *same_long))
    rows.append(("partly_land_long", *mixed(700)))
    rows.append(("corners", np.array([0, nx - 1, (ny - 1) * nx, ny * nx - 1]), weights(4)))
    ends = np.array([[j * nx, j * nx + nx - 1] for j in range(ny)]).ravel()
    rows.append(("row_ends", ends, weights(ends.size)))
    rows.append(("descending", np.sort(rng.choice(wet_cells, 30))[::-1], weights(30)))
    rows.append(("same_short_c", *same_short))
    rows.append(("same_long_c", *same_long))
    row_ptr = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum([len(c) for _, c, _ in rows], out=row_ptr[1:])
    return dict(row_ptr=row_ptr, col=np.concatenate([np.asarray(c, dtype=np.int64) for _, c, _ in rows]).astype(np.int32),
                weight=np.concatenate([w for _, _, w in rows]), names={name: r for r, (name, _, _) in enumerate(rows)},
                wet=wet, fields=fields, zb=zb)


def embed(a, hx, hy, fill):
    ny, nx = a.shape
    g = np.full((ny + 2 * hy, nx + 2 * hx), fill, dtype=a.dtype)
    g[hy:hy + ny, hx:hx + nx] = a
    return g


def atlas_arrays(atlas, hx, hy, n_fields=None):
    """(fields, wet) in the halo layout: every halo cell and every land cell of field f holds POISON[f % 2]; the mask's halo is
    1 (nothing may read it)."""
    wet = atlas["wet"]
    fields = [embed(np.where(wet != 0, x, POISON[f % 2]), hx, hy, POISON[f % 2]) for f, x in enumerate(atlas["fields"][:n_fields])]
    return fields, embed(wet, hx, hy, 1)
