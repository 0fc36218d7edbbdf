"""A designed atlas of interpolation weight maps, an exact reference and a NumPy model of the tiled kernel's footprint
(test infrastructure of tests/test_weight_atlas.py; CPU only, nothing here imports the library).

interpolate_atmosphere_state! exists in three hand-written copies on the device (interpolate_tiles<ROWS>,
interpolate_gather_kernel, interpolate_land_kernel), the tiled one in three instantiations and four launches.  Geographic
weight maps leave most of their index logic untouched: no latitude clamp, hardly a negative index, one fold.  The atlas
holds maps that each FORCE one situation (a seam inside a staged tile, a tile that sees the whole circle, exact nodes, signed
zeros, …); `tile_model` says — per tile — what the header's comments promise the kernel does with them, so that the
situation is asserted, not assumed; `exact_interpolate` is the definition in exact arithmetic.

The exact reference.  Oceananigans' `interpolator`: i⁻ = trunc(f), i⁺ = i⁻ + sign(f), ξ = f − floor(f); periodic in
longitude, clamped in latitude; every level interpolated, the two results blended in time (the reference's order, not the
kernel's); rain + snow summed; winds rotated by the given cos / sin.  Every float32 / float64 input is a dyadic rational, so
the whole formula is evaluated WITHOUT rounding: `exact_cell` does it with fractions.Fraction, one cell at a time (the
definition, as plainly as it can be written), and `exact_interpolate` does the same arithmetic on whole windows with Python
integers over a common power-of-two denominator (a Fraction whose denominator never needs a gcd: ≈ 30× faster, which is what
lets the atlas be compared cell by cell).  test_weight_atlas.py holds the two against each other.  Only the final result
is rounded to double (Python's int / int is correctly rounded).

Besides the value the reference returns, per cell and source variable, M = the largest |node value| among the four corners
at both levels: the error bound of a result is taken against ITS OWN corners, not against a global field scale.
"""
from fractions import Fraction

import numpy as np

VARIABLES = ("tas", "huss", "psl", "uas", "vas", "rlds", "rsds", "prra", "prsn")   # abi.JRA55_VARIABLES
SCALAR_FIELDS = dict(T="tas", p="psl", q="huss", Qs="rsds", Ql="rlds")             # exchange field → source variable
EXCHANGE_NAMES = ("u", "v", "T", "p", "q", "Qs", "Ql", "Mp")

SOURCE_GRIDS = ((16, 8), (17, 9), (64, 12), (5, 3), (2, 2), (1, 1))                # ns_x × ns_y (17: odd half; 1 × 1: degenerate)
# (nx, ny, hx, hy, ring): wx = 64 exactly (the library wants hx ≥ ring + 1: the GPU tests assert that it refuses this one);
# wx = 65 and wy = 7 (a one-lane tile, a partial last row group, unequal halos); three tiles across, ring 0; one cell; and
# the first window again with the smallest halo the library accepts
WINDOWS = ((62, 3, 1, 1, 1), (63, 5, 2, 7, 1), (130, 9, 8, 3, 0), (1, 1, 1, 1, 0), (62, 3, 2, 2, 1))
ROWS = (1, 2, 4)
CAPS = (16, 128, 224)
TIME_FRACTIONS = (0.0, 1.0, 0.37, 2.0 ** -60)
LEVEL_PAIRS = ((0, 1), (2, 0), (1, 1))
BLENDS = tuple((l1, l2, tf) for (l1, l2) in LEVEL_PAIRS for tf in TIME_FRACTIONS)
N_LEVELS = 3

U = 2.0 ** -53          # one rounding to nearest, relative
BOUND_SCALAR, BOUND_MP, BOUND_ROTATED = 16, 20, 24     # the accepted bounds in units of U · M (test_weight_atlas.py counts)


def window_shape(win):
    nx, ny, hx, hy, ring = win
    return ny + 2 * ring, nx + 2 * ring


def parent_shape(win):
    nx, ny, hx, hy, ring = win
    return ny + 2 * hy, nx + 2 * hx


def cut(a, win):
    """The ring window of a parent-shaped array."""
    nx, ny, hx, hy, ring = win
    return a[hy - ring:hy + ny + ring, hx - ring:hx + nx + ring]


# ---------------------------------------------------------------------------------------------
# node values
# ---------------------------------------------------------------------------------------------
_MAGNITUDE = dict(tas=(245.0, 60.0), huss=(1e-3, 2e-2), psl=(9.6e4, 8e3), uas=(-12.0, 24.0), vas=(-9.0, 18.0),
                  rlds=(150.0, 300.0), rsds=(0.0, 900.0), prra=(0.0, 6e-5), prsn=(0.0, 2e-5))   # (offset, span), as in JRA55
_LAND_MAGNITUDE = dict(friver=(0.0, 4e-4), licalvf=(0.0, 4e-5))


def node_values(nsx, nsy, kind="jra", seed=11):
    """float32 [3, ns_y, ns_x] per variable, seeded, distinct per node and level within every variable.  "jra": every variable at its JRA55
    magnitude (psl ≈ 1e5 … precipitation ≈ 1e-5).  "wide": the same with a few nodes per variable near the float32 maximum and
    in the float32 subnormals (both signs): a precision loss that a field scale would hide shows against the local M."""
    rng = np.random.default_rng([seed, nsx, nsy, 0 if kind == "jra" else 1])
    out = {}
    for name, (a, span) in {**_MAGNITUDE, **_LAND_MAGNITUDE}.items():
        n_nodes = N_LEVELS * nsy * nsx       # a shuffled ladder with jitter inside each rung: no two nodes of a variable are equal
        rung = (rng.permutation(n_nodes) + rng.uniform(0.2, 0.8, n_nodes)) / n_nodes
        v = (a + span * (0.02 + 0.96 * rung)).astype(np.float32).reshape(N_LEVELS, nsy, nsx)
        if kind == "wide":
            flat = v.reshape(-1)
            k = rng.permutation(flat.size)
            n = max(1, flat.size // 6)
            flat[k[:n]] = (rng.choice([-1.0, 1.0], n) * rng.uniform(0.5, 1.0, n) * 3.4e38).astype(np.float32)
            sub = (rng.choice([-1, 1], n) * rng.integers(1, 1 << 22, n)).astype(np.float64) * 2.0 ** -149
            flat[k[n:2 * n]] = sub.astype(np.float32)
        out[name] = v
    return out


# ---------------------------------------------------------------------------------------------
# the exact reference
# ---------------------------------------------------------------------------------------------
def _dyadic(a):
    """float array → (object array of Python ints n, S) with a == n / 2**S exactly."""
    flat = [float(x).as_integer_ratio() for x in np.asarray(a, dtype=np.float64).ravel()]
    S = max(d.bit_length() - 1 for _, d in flat)
    ints = np.empty(len(flat), dtype=object)
    for k, (n, d) in enumerate(flat):
        ints[k] = n << (S - (d.bit_length() - 1))
    return ints.reshape(np.shape(a)), S


_ROUND = np.frompyfunc(lambda n, d: n / d, 2, 1)      # int / int: correctly rounded


def _to_double(ints, scale_bits):
    return _ROUND(ints, 1 << scale_bits).astype(np.float64)


def corners(fi, fj, nsx, nsy):
    """(i⁻, i⁺, j⁻, j⁺) of the definition: trunc, + sign, periodic in longitude, clamped in latitude (integer arrays)."""
    fi, fj = np.asarray(fi, dtype=np.float64), np.asarray(fj, dtype=np.float64)
    im, jm = np.trunc(fi).astype(np.int64), np.trunc(fj).astype(np.int64)
    ip, jp = im + np.sign(fi).astype(np.int64), jm + np.sign(fj).astype(np.int64)
    return np.mod(im, nsx), np.mod(ip, nsx), np.clip(jm, 0, nsy - 1), np.clip(jp, 0, nsy - 1)


class ExactMap:
    """The blend-independent part of the exact reference on one window: the four weights as integers over 4**S and every
    (level, variable) plane interpolated exactly.  `values`: dict name → float32 [levels, ns_y, ns_x]."""

    def __init__(self, values, fi, fj):
        first = next(iter(values.values()))
        self.nsy, self.nsx = first.shape[1:]
        self.values = values
        self.im, self.ip, self.jm, self.jp = corners(fi, fj, self.nsx, self.nsy)
        F, Sx = _dyadic(fi)
        G, Sy = _dyadic(fj)
        S = max(Sx, Sy)
        one = 1 << S
        xi = (F * (1 << (S - Sx))) % one          # ξ = f − floor(f): Python's % is the floored one
        eta = (G * (1 << (S - Sy))) % one
        self.w = ((one - xi) * (one - eta), (one - xi) * eta, xi * (one - eta), xi * eta)   # (−,−) (−,+) (+,−) (+,+)
        self.wbits = 2 * S
        self._planes, self._blended, self._rounded, self._magnitude = {}, {}, {}, {}

    NODE_BITS = 149                                   # float32: every value is an integer multiple of 2**-149

    def plane(self, name, level):
        """Σ w · node of one (variable, level), integers over 2**(wbits + 149)."""
        key = (name, level)
        if key not in self._planes:
            d, S = _dyadic(self.values[name][level])
            d = d * (1 << (self.NODE_BITS - S))
            w00, w01, w10, w11 = self.w
            self._planes[key] = (w00 * d[self.jm, self.im] + w01 * d[self.jp, self.im] + w10 * d[self.jm, self.ip]
                                 + w11 * d[self.jp, self.ip])
        return self._planes[key]

    def blended(self, name, l1, l2, tf):
        """(integers, scale bits) of  level2 · tf + level1 · (1 − tf)  of the two interpolated levels (kept: the twelve blends
        of the atlas have seven distinct exact results — tf = 0, tf = 1 and level1 = level2 are single levels)."""
        if l1 == l2 or tf == 0.0:
            l1, l2, tf = l1, l1, 0.0
        elif tf == 1.0:
            l1, l2, tf = l2, l2, 0.0
        key = (name, l1, l2, tf)
        if key not in self._blended:
            n, d = float(tf).as_integer_ratio()
            self._blended[key] = (self.plane(name, l2) * n + self.plane(name, l1) * (d - n), self.wbits + self.NODE_BITS + d.bit_length() - 1)
        return self._blended[key]

    def rounded(self, name, l1, l2, tf):
        """The exact blend of one variable rounded to double, once."""
        v, bits = self.blended(name, l1, l2, tf)
        key = id(v)
        if key not in self._rounded:
            self._rounded[key] = (_to_double(v, bits), v)
        return self._rounded[key][0]

    def magnitude(self, name, l1, l2):
        """M: the largest |node| among the four corners at both levels (float64, exact)."""
        key = (name, min(l1, l2), max(l1, l2))
        if key in self._magnitude:
            return self._magnitude[key]
        m = self._magnitude[key] = np.zeros(self.im.shape)
        for lv in (l1, l2):
            d = np.abs(self.values[name][lv].astype(np.float64))
            for jj, ii in ((self.jm, self.im), (self.jp, self.im), (self.jm, self.ip), (self.jp, self.ip)):
                np.maximum(m, d[jj, ii], out=m)
        return m


def exact_interpolate(values, fi, fj, l1, l2, tf, cos_rot=None, sin_rot=None, cache=None):
    """The eight exchange fields on a window (fi, fj, cos_rot, sin_rot: window-shaped), each the exact result rounded once,
    and their bounds' magnitudes: returns (fields, M) with M[field] = M for a scalar, M_rain + M_snow for Mp, M_u + M_v for
    rotated winds.  `cache`: a dict that keeps the ExactMap of a (values, map) pair across blends."""
    key = (id(values), np.asarray(fi).tobytes(), np.asarray(fj).tobytes())
    em = cache.get(key) if cache is not None else None
    if em is None:
        em = ExactMap(values, fi, fj)
        if cache is not None:
            cache[key] = em
    out, M = {}, {}
    for field, name in SCALAR_FIELDS.items():
        out[field], M[field] = em.rounded(name, l1, l2, tf), em.magnitude(name, l1, l2)
    rain, bits = em.blended("prra", l1, l2, tf)
    snow, _ = em.blended("prsn", l1, l2, tf)
    out["Mp"], M["Mp"] = _to_double(rain + snow, bits), em.magnitude("prra", l1, l2) + em.magnitude("prsn", l1, l2)
    ua, bits = em.blended("uas", l1, l2, tf)
    va, _ = em.blended("vas", l1, l2, tf)
    Mu, Mv = em.magnitude("uas", l1, l2), em.magnitude("vas", l1, l2)
    if cos_rot is None:
        out["u"], out["v"], M["u"], M["v"] = em.rounded("uas", l1, l2, tf), em.rounded("vas", l1, l2, tf), Mu, Mv
    else:
        c, Sc = _dyadic(cos_rot)
        s, Ss = _dyadic(sin_rot)
        R = max(Sc, Ss)
        c, s = c * (1 << (R - Sc)), s * (1 << (R - Ss))
        out["u"], out["v"] = _to_double(ua * c + va * s, bits + R), _to_double(va * c - ua * s, bits + R)
        M["u"] = M["v"] = Mu + Mv
    return out, M


def exact_land(values, fi, fj, l1, l2, tf, calving=True, cache=None):
    """JRA55PrescribedLand: friver (+ licalvf) → (field, M_friver + M_licalvf)."""
    key = (id(values), np.asarray(fi).tobytes(), np.asarray(fj).tobytes())
    em = cache.get(key) if cache is not None else None
    if em is None:
        em = ExactMap(values, fi, fj)
        if cache is not None:
            cache[key] = em
    v, bits = em.blended("friver", l1, l2, tf)
    M = em.magnitude("friver", l1, l2)
    if calving:
        v = v + em.blended("licalvf", l1, l2, tf)[0]
        M = M + em.magnitude("licalvf", l1, l2)
    return _to_double(v, bits), M


def exact_cell(values, name, fi, fj, l1, l2, tf):
    """One variable at one cell, from the definition, in fractions.Fraction (the check of exact_interpolate's integers)."""
    import math
    nsy, nsx = values[name].shape[1:]
    f, g = Fraction(float(fi)), Fraction(float(fj))
    xi, eta = f - math.floor(f), g - math.floor(g)
    im, jm = math.trunc(f), math.trunc(g)
    ip, jp = im + (f > 0) - (f < 0), jm + (g > 0) - (g < 0)
    im, ip = im % nsx, ip % nsx
    jm, jp = min(max(jm, 0), nsy - 1), min(max(jp, 0), nsy - 1)
    level = []
    for lv in (l1, l2):
        d = values[name][lv]
        n = lambda j, i: Fraction(float(d[j, i]))
        level.append((1 - xi) * (1 - eta) * n(jm, im) + (1 - xi) * eta * n(jp, im) + xi * (1 - eta) * n(jm, ip)
                     + xi * eta * n(jp, ip))
    t = Fraction(float(tf))
    return level[1] * t + level[0] * (1 - t)


def bounds(M, rotated):
    """The accepted |Δ| per exchange field, from the magnitudes exact_interpolate returned."""
    b = {k: BOUND_SCALAR * U * M[k] for k in SCALAR_FIELDS}
    b["Mp"] = BOUND_MP * U * M["Mp"]
    for k in ("u", "v"):
        b[k] = (BOUND_ROTATED if rotated else BOUND_SCALAR) * U * M[k]
    return b


# ---------------------------------------------------------------------------------------------
# the tile model
# ---------------------------------------------------------------------------------------------
DEFECTS = ("xi_from_trunc", "plus_is_always_east", "w01_w10_swapped", "tf_swapped", "rotation_sign", "snow_dropped",
           "row0_clamp")


def tile_model(fi, fj, nsx, nsy, rows, cap, defects=()):
    """What interpolate_tiles<rows> does with a window's maps (fi, fj: window-shaped), per tile of 64 lanes × `rows` rows, as
    coflux_interp_tiles.hpp describes it: out-of-window lanes shadow the last column and rows beyond the window the last row;
    the reference column is lane 0's i⁻ in the tile's first row; every column is re-centred on it into [−half, ns_x − half);
    the footprint lo…hi × jlo…jhi covers both corners of every lane and row; it is staged when W · H ≤ cap and W ≤ ns_x.
    Returns a dict of (tiles_y, tiles_x) arrays ref, lo, hi, jlo, jhi, W, H, fits, and the per-lane arrays (tiles_y, tiles_x,
    rows, 64) the values are read with: d0, di, j0, j1, xi, eta, the source node (row, column) of each of the four corners as
    the staged offsets (or, without `fits`, the fallback's wrapped indices) address it, and `inside` (the lane stores).
    `defects`: names from DEFECTS that change the index logic; every index stays in range under each of them."""
    fi, fj = np.asarray(fi, dtype=np.float64), np.asarray(fj, dtype=np.float64)
    wy, wx = fi.shape
    tiles_x, tiles_y = (wx + 63) // 64, (wy + rows - 1) // rows
    half = nsx // 2
    col = np.arange(tiles_x)[None, :, None, None] * 64 + np.arange(64)[None, None, None, :]
    row = np.arange(tiles_y)[:, None, None, None] * rows + np.arange(rows)[None, None, :, None]
    inside = (col < wx) & (row < wy)
    cc = np.minimum(col, wx - 1) + 0 * row
    rc = np.minimum(row, wy - 1) + 0 * col
    if "row0_clamp" in defects:      # the row clamp taken from the tile's first row for every row
        rc = np.minimum(row[:, :, :1, :], wy - 1) + 0 * row + 0 * col
    f, g = fi[rc, cc], fj[rc, cc]
    i0, ja = np.trunc(f).astype(np.int64), np.trunc(g).astype(np.int64)
    xi, eta = f - np.floor(f), g - np.floor(g)
    if "xi_from_trunc" in defects:
        xi, eta = f - np.trunc(f), g - np.trunc(g)
    di, dj = np.sign(f).astype(np.int64), np.sign(g).astype(np.int64)
    if "plus_is_always_east" in defects:
        di, dj = np.ones_like(di), np.ones_like(dj)
    j0, j1 = np.clip(ja, 0, nsy - 1), np.clip(ja + dj, 0, nsy - 1)
    ref = i0[:, :, :1, :1]
    d0 = np.mod(i0 - ref + half, nsx) - half
    lo = np.minimum(d0, d0 + di).min(axis=(2, 3), keepdims=True)
    hi = np.maximum(d0, d0 + di).max(axis=(2, 3), keepdims=True)
    jlo = np.minimum(j0, j1).min(axis=(2, 3), keepdims=True)
    jhi = np.maximum(j0, j1).max(axis=(2, 3), keepdims=True)
    W, H = hi - lo + 1, jhi - jlo + 1
    fits = (W * H <= cap) & (W <= nsx)
    # staged: tile[y][x] = node(jlo + y, wrap(ref + lo + x)); a corner is read at offset (j − jlo) · W + (d − lo) [+ di]
    o00, o01 = (j0 - jlo) * W + (d0 - lo), (j1 - jlo) * W + (d0 - lo)

    def staged(o):
        assert np.all((o >= 0) & (o < W * H) | ~fits), "a staged offset outside the tile"
        y, x = o // W, o % W
        return jlo + y, np.mod(ref + lo + x, nsx)

    def pick(o, jf, i_f):
        js, is_ = staged(o)
        return np.where(fits, js, jf), np.where(fits, is_, i_f)

    is0, is1 = np.mod(ref + d0, nsx), np.mod(ref + d0 + di, nsx)
    c00, c01 = pick(o00, j0, is0), pick(o01, j1, is0)
    c10, c11 = pick(o00 + di, j0, is1), pick(o01 + di, j1, is1)
    sq = lambda a: a[:, :, 0, 0]
    return dict(ref=sq(ref), lo=sq(lo), hi=sq(hi), jlo=sq(jlo), jhi=sq(jhi), W=sq(W), H=sq(H), fits=sq(fits), f=f, g=g, d0=d0, di=di,
                j0=j0, j1=j1, xi=xi, eta=eta, corners=(c00, c01, c10, c11), inside=inside, col=cc, row=rc,
                full=sq(np.all(col < wx, axis=3, keepdims=True) & (row[:, :, :1, :] < wy)), shape=(wy, wx))


def model_values(model, values, l1, l2, tf, cos_rot=None, sin_rot=None, defects=()):
    """The eight exchange fields as the tile model reads them (double arithmetic in the kernel's order: the two levels of a
    node blended, then the four corners combined left to right), window-shaped."""
    wy, wx = model["shape"]
    xi, eta = model["xi"], model["eta"]
    w00, w01, w10, w11 = (1.0 - xi) * (1.0 - eta), (1.0 - xi) * eta, xi * (1.0 - eta), xi * eta
    if "w01_w10_swapped" in defects:
        w01, w10 = w10, w01
    if "tf_swapped" in defects:
        tf = 1.0 - tf
    (a, b), (c, d), (e, f), (g, h) = model["corners"]
    m = model["inside"]
    rr, cc = (model["row"] + 0 * model["col"])[m], (model["col"] + 0 * model["row"])[m]
    if "row0_clamp" in defects:     # the store goes to the lane's own row; only the indices came from row 0
        tiles_y, tiles_x, rows, _ = m.shape
        own = np.arange(tiles_y)[:, None, None, None] * rows + np.arange(rows)[None, None, :, None] + 0 * model["col"]
        rr = own[m]

    def one(name):
        node = values[name][l2].astype(np.float64) * tf + values[name][l1].astype(np.float64) * (1.0 - tf)
        val = w00 * node[a, b] + w01 * node[c, d] + w10 * node[e, f] + w11 * node[g, h]
        out = np.full((wy, wx), np.nan)
        out[rr, cc] = val[m]
        return out

    out = {field: one(name) for field, name in SCALAR_FIELDS.items()}
    out["Mp"] = one("prra") if "snow_dropped" in defects else one("prra") + one("prsn")
    ua, va = one("uas"), one("vas")
    if cos_rot is not None:
        sn = -sin_rot if "rotation_sign" in defects else sin_rot
        ua, va = ua * cos_rot + va * sn, -ua * sn + va * cos_rot
    out["u"], out["v"] = ua, va
    return out


# ---------------------------------------------------------------------------------------------
# the atlas
# ---------------------------------------------------------------------------------------------
def _tri(p):
    """Triangle wave of period 1: 0 at p = 0, +1 at 1/4, −1 at 3/4."""
    p = np.mod(p, 1.0)
    return np.where(p < 0.25, 4 * p, np.where(p < 0.75, 2 - 4 * p, 4 * p - 4))


def _angles(C, R):
    return 0.7 * np.sin(0.37 * C + 0.11) + 1.9 * np.cos(0.53 * R) + 0.0 * C


def _seam_east(C, R, nsx, nsy, wx, wy):
    start = 4.0 if wx > 128 else 0.0            # three tiles across: the crossing sits in the middle one
    return nsx - 2.3 - start + C / 16.0, 1.3 + 0.1 * R


def _seam_west(C, R, nsx, nsy, wx, wy):
    return -0.3 - C / 16.0 - 0.01 * R, 1.45 + 0.1 * R - 0.001 * C


def _south_clamp(C, R, nsx, nsy, wx, wy):
    return 0.37 * C + 0.2, -1.9 + 0.75 * R


def _north_clamp(C, R, nsx, nsy, wx, wy):
    return nsx - 0.21 * C, nsy - 1 - 0.4 + 0.6 * R


def _exact_nodes(C, R, nsx, nsy, wx, wy):
    return np.floor(C / 4.0) - 5.0, R - 2.0


def _zeros(C, R, nsx, nsy, wx, wy):
    return np.where(C % 2 == 0, 0.0, -0.0), np.where(R % 3 == 0, -0.0, np.where(R % 3 == 1, 0.0, 0.5 * R))


def _more_than_circle(C, R, nsx, nsy, wx, wy):
    return 1.5 * C + 0.25, np.full(R.shape, 0.25)


def _exactly_circle(C, R, nsx, nsy, wx, wy):
    # a triangle wave around the middle of the circle: lane 0 of every tile sits mid-range, the extremes 0.25 and ns_x − 1.25
    # fall on lanes 48 and 16 — i⁻ takes every column but the last, i⁺ adds that one: W = ns_x, not ns_x + 1
    mid, amp = (nsx - 1.0) / 2.0, (nsx - 1.5) / 2.0
    return mid + amp * _tri(C / 64.0), np.full(R.shape, 0.25)


def _fold(C, R, nsx, nsy, wx, wy, rows_that_jump=None):
    # the second half of the window's first tile lies beyond a fold: half a circle further, and (as across a real fold)
    # some rows away
    jump = (C >= 32) & (C < 64) & (True if rows_that_jump is None else rows_that_jump(R))
    fi = 2.2 + C / 16.0 + 0.01 * R + np.where(jump, nsx // 2, 0)
    fj = 1.3 + 0.1 * R + 0.001 * C + np.where(jump, min(6, max(nsy - 3, 0)), 0)
    return fi, fj


def _multi_row_fold(C, R, nsx, nsy, wx, wy):
    return _fold(C, R, nsx, nsy, wx, wy, rows_that_jump=lambda R: R % 2 == 1)


def _one_node(C, R, nsx, nsy, wx, wy):
    return np.full(C.shape, -0.0), np.full(R.shape, nsy + 1.5)


def _tiny(C, R, nsx, nsy, wx, wy):
    # |f| so small that ξ = f − floor(f) itself rounds (to 1.0 for a tiny negative f), beside indices one ulp off a node
    k = ((C + 3 * R) % 6).astype(np.int64)
    fi = np.choose(k, [-2.0 ** -60, 2.0 ** -60, -1.5 * 2.0 ** -40, 3.0 - 2.0 ** -51, -2.0 + 2.0 ** -52, 1.0 + 2.0 ** -52])
    k = ((2 * C + R) % 5).astype(np.int64)
    fj = np.choose(k, [-2.0 ** -55, 1.5 * 2.0 ** -70, 2.0 - 2.0 ** -52, -(2.0 ** -30), 1.0 + 2.0 ** -50])
    return fi, fj


def _random(C, R, nsx, nsy, wx, wy):
    rng = np.random.default_rng([7, nsx, nsy, C.shape[0], C.shape[1]])
    return rng.uniform(-nsx, 2 * nsx, size=C.shape), rng.uniform(-3, nsy + 2, size=C.shape)


# name → (map, separable storage, rotation).  A separable entry is also run in general storage with a rotation ("name/2d": the
# same indices through the other addressing, and rotated winds), so every map is held in the storage(s) it allows.
ENTRIES = {
    "seam_east": (_seam_east, True, False),
    "seam_west": (_seam_west, False, True),
    "south_clamp": (_south_clamp, True, False),
    "north_clamp": (_north_clamp, True, False),
    "exact_nodes": (_exact_nodes, True, False),
    "zeros": (_zeros, True, False),
    "more_than_circle": (_more_than_circle, True, False),
    "exactly_circle": (_exactly_circle, True, False),
    "fold": (_fold, False, True),
    "multi_row_fold": (_multi_row_fold, False, False),
    "one_node": (_one_node, True, False),
    "tiny": (_tiny, False, True),
    "random": (_random, False, True),
    "latlon": (None, True, False),
    "tripolar": (None, False, True),
}
NAMES = tuple(n for name, (_, sep, _r) in ENTRIES.items() for n in ((name, name + "/2d") if sep else (name,)))


def weight_map(name, grid, win):
    """dict(separable, fi, fj[, cos_rot, sin_rot]) in the library's storage for the parent arrays of `win`: separable maps as
    fi[nx + 2 hx], fj[ny + 2 hy], general ones (and the rotation) as parent-shaped arrays.  The maps are functions of the window
    column and row (0 at the ring window's first cell), so a window's tiles see the same indices whatever the halo."""
    nsx, nsy = grid
    nx, ny, hx, hy, ring = win
    base, general_twin = (name[:-3], True) if name.endswith("/2d") else (name, False)
    fn, separable, rotated = ENTRIES[base]
    shape = parent_shape(win)
    C = np.broadcast_to((np.arange(-hx, nx + hx) + ring)[None, :].astype(np.float64), shape).copy()
    R = np.broadcast_to((np.arange(-hy, ny + hy) + ring)[:, None].astype(np.float64), shape).copy()
    wy, wx = window_shape(win)
    if fn is not None:
        fi, fj = fn(C, R, nsx, nsy, wx, wy)
        fi, fj = np.array(fi, dtype=np.float64), np.array(fj, dtype=np.float64)     # (no arithmetic here: −0.0 keeps its sign)
        assert fi.shape == shape and fj.shape == shape, name
        theta = _angles(C, R)
        cs, sn = np.cos(theta), np.sin(theta)
    else:
        from coflux import synthetic as syn
        if base == "latlon":
            f1, g1, _ = syn.latlon_fractional_indices(nx, ny, hx, hy, nsx=nsx, nsy=max(nsy, 2))
            fi, fj = np.broadcast_to(f1[None, :], shape).copy(), np.broadcast_to(g1[:, None], shape).copy()
            theta = _angles(C, R)
            cs, sn = np.cos(theta), np.sin(theta)
        else:
            fi, fj, cs, sn, _ = syn.tripolar_like_weights(nx, ny, hx, hy, nsx=nsx, nsy=max(nsy, 2))
        if nsy < 2:
            fj = np.zeros(shape)
    fi, fj = np.ascontiguousarray(fi), np.ascontiguousarray(fj)
    if separable and not general_twin:
        assert np.array_equal(fi, np.broadcast_to(fi[:1], shape)) and np.array_equal(fj, np.broadcast_to(fj[:, :1], shape)), name
        return dict(separable=True, fi=np.ascontiguousarray(fi[0]), fj=np.ascontiguousarray(fj[:, 0]))
    w = dict(separable=False, fi=fi, fj=fj)
    if rotated or general_twin:
        w.update(cos_rot=np.ascontiguousarray(cs), sin_rot=np.ascontiguousarray(sn))
    return w


def window_maps(w, win):
    """(fi, fj, cos, sin) of a weight_map on the ring window, 2-D (cos, sin None without a rotation)."""
    nx, ny, hx, hy, ring = win
    if w["separable"]:
        shape = parent_shape(win)
        fi, fj = np.broadcast_to(w["fi"][None, :], shape), np.broadcast_to(w["fj"][:, None], shape)
    else:
        fi, fj = w["fi"], w["fj"]
    cs = cut(w["cos_rot"], win) if w.get("cos_rot") is not None else None
    sn = cut(w["sin_rot"], win) if w.get("sin_rot") is not None else None
    return np.ascontiguousarray(cut(fi, win)), np.ascontiguousarray(cut(fj, win)), cs, sn


# ---------------------------------------------------------------------------------------------
# the property every entry must have, as a predicate on the tile model
# ---------------------------------------------------------------------------------------------
def _staged_crosses_seam(m, nsx):
    """tiles that stage a footprint whose columns run over ns_x − 1 → 0"""
    first = np.mod(m["ref"] + m["lo"], nsx)
    return m["fits"] & (first + m["W"] - 1 >= nsx)


def _row_width(m):
    lo = np.minimum(m["d0"], m["d0"] + m["di"]).min(axis=3)
    hi = np.maximum(m["d0"], m["d0"] + m["di"]).max(axis=3)
    return hi - lo + 1      # (tiles_y, tiles_x, rows)


def has_property(name, m, grid, rows, cap):
    """Whether the map of entry `name` shows, in tile model `m`, the situation it is in the atlas for."""
    nsx, nsy = grid
    base = name[:-3] if name.endswith("/2d") else name
    ins = m["inside"]
    if base == "seam_east":
        return bool(np.any(_staged_crosses_seam(m, nsx) & m["full"]))
    if base == "seam_west":
        lane0 = m["f"][:, :, 0, 0]
        return bool(np.any(_staged_crosses_seam(m, nsx) & (lane0 < 0) & (m["f"].min(axis=(2, 3)) < -1.0)))
    if base in ("south_clamp", "north_clamp"):
        beyond = (m["g"] < 0) if base == "south_clamp" else (m["g"] > nsy - 1)
        edge = 0 if base == "south_clamp" else nsy - 1
        degenerate = beyond & (m["j0"] == edge) & (m["j1"] == edge) & ins
        mixed = np.any(degenerate, axis=(2, 3)) & np.any(~beyond & ins & (m["j0"] != m["j1"]), axis=(2, 3))
        return bool(np.any(degenerate) and np.all(m["j0"][beyond] == m["j1"][beyond]) and (rows == 1 or np.any(mixed)))
    if base == "exact_nodes":
        f = m["f"][ins]
        return bool(np.all(f == np.trunc(f)) and np.all(m["xi"][ins] == 0.0) and np.any(m["di"][ins] == 1) and np.any(m["di"][ins] == -1)
                    and np.any(f > 0) and np.any(f < 0))
    if base == "zeros":
        f, g = m["f"][ins], m["g"][ins]
        return bool(np.all(f == 0.0) and np.any(np.signbit(f)) and np.any(~np.signbit(f)) and np.all(m["di"][ins] == 0) and np.all(m["W"] == 1)
                    and np.any((g == 0.0) & np.signbit(g)) and np.any((g == 0.0) & ~np.signbit(g)))
    if base == "more_than_circle":      # W > ns_x decides: the footprint's area alone would still fit
        return bool(np.any((m["W"] > nsx) & (m["W"] * m["H"] <= cap) & ~m["fits"] & m["full"]))
    if base == "exactly_circle":
        return bool(np.any(m["fits"] & (m["W"] == nsx) & m["full"]))
    if base == "fold":
        wide = _row_width(m).max(axis=2) > nsx // 2
        return bool(np.any(m["fits"]) and np.any(~m["fits"] & wide))
    if base == "multi_row_fold":
        rw = _row_width(m)
        if rows == 1:
            return bool(np.any(m["fits"]) and np.any(~m["fits"]))
        return bool(np.any((rw.max(axis=2) > nsx // 2) & (rw.min(axis=2) <= nsx // 4 + 2)))
    if base == "one_node":
        return bool(np.all(m["W"] * m["H"] == 1) and np.all(m["fits"]))
    if base == "tiny":
        f = m["f"][ins]
        return bool(np.any((f < 0) & (m["xi"][ins] == 1.0)) and np.any((f > 0) & (f < 2.0 ** -50)))
    if base == "random":
        f, g = m["f"][ins], m["g"][ins]
        return bool(f.min() >= -nsx and f.max() < 2 * nsx and g.min() >= -3 and g.max() < nsy + 2 and (f.size < 64 or (np.any(f < 0) and np.any(f > nsx)
                    and np.any(g < 0) and np.any(g > nsy - 1))))
    if base in ("latlon", "tripolar"):
        return True
    raise KeyError(name)
