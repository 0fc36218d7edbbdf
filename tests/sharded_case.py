"""What tests/test_sharded_diagnostics_cpu.py and tests/test_sharded_diagnostics.py share: the designed monitor array on the
68 × 37 surface, its cuts, and the derived error bounds of the integrals and of the combined regridding.  NumPy only.

The designed array (monitor_fixture) is made so that numbering a tile's cells with the tile's own nx cannot pass, on the worlds
(2,2) — tiles 34 wide, row blocks 19 + 18 — and (4,1) — tiles 17 wide:

    maximum   3.0 at (j, i) = (4, 40), c = 312, and at (5, 3), c = 343: rank 1 | 2 holds the smaller global index, rank 0 the
              other.  With c = first_cell + j·nx_local + i the two are 176 | 108 and 173 | 88: on (2,2) the tie goes to the
              wrong tile, on both worlds to a wrong number.
    zeros     +0.0 at (1, 60), c = 128 (rank 1 | 3) and −0.0 at (30, 10), c = 2050 (rank 2 | 0): with the non-finite cells dry
              the minimum is −0.0 at 2050 although a +0.0 has the smaller index (the total order, not ==); under "abs" both are
              +0.0 and the tie goes to 128.
    NaN, Inf  NaN at (20, 50), c = 1410 (rank 3 | 2) and −Inf at (25, 5), c = 1705 (rank 2 | 0): first_nonfinite is the NaN's,
              held by the higher rank.  (−Inf, so that the maximum stays the doubled 3.0; it is the minimum while it is wet.)
    the rest  distinct values in (1, 2).
"""
import math

import numpy as np

NX, NY = 68, 37
WORLDS = ((2, 2), (4, 1))
MAXIMUM = 3.0
CELLS = dict(max_first=(4, 40), max_second=(5, 3), plus_zero=(1, 60), minus_zero=(30, 10), nan=(20, 50), inf=(25, 5))
U = 2.0 ** -53


def cell_number(name, row_length=NX):
    j, i = CELLS[name]
    return j * row_length + i


def monitor_fixture():
    """(x, wet_finite): the designed (NY, NX) array and the uint8 mask that is dry at its NaN and its −Inf and wet elsewhere"""
    rng = np.random.default_rng(20261021)
    x = 1.0 + rng.permutation(NX * NY).reshape(NY, NX) / float(NX * NY)      # distinct, in [1, 2)
    x[CELLS["max_first"]] = x[CELLS["max_second"]] = MAXIMUM
    x[CELLS["plus_zero"]], x[CELLS["minus_zero"]] = 0.0, -0.0
    x[CELLS["nan"]], x[CELLS["inf"]] = np.nan, -np.inf
    wet = np.ones((NY, NX), dtype=np.uint8)
    wet[CELLS["nan"]] = wet[CELLS["inf"]] = 0
    return x, wet


def gamma(n):
    """γ(n) = n·u / (1 − n·u), u = 2⁻⁵³: the relative error bound of a sum of n + 1 terms in ANY order (Higham, Accuracy and
    Stability of Numerical Algorithms, §4.2)"""
    n = max(int(n), 0)
    return n * U / (1.0 - n * U)


def sum_bound(terms):
    """(exact, bound): math.fsum of `terms` and γ(n − 1) · Σ|t_k|, within which every floating-point sum of them lies"""
    t = np.asarray(terms, dtype=np.float64).ravel()
    return math.fsum(t.tolist()), gamma(t.size - 1) * math.fsum(np.abs(t).tolist())


def regrid_row_bounds(definitions):
    """Per destination row the tolerance of  combine_regridded(ranks' CF_REGRID_SUM)  against the single domain's CF_REGRID_MEAN,
    per field: `definitions` = [per rank] + [whole], each regrid_reference.definition() of that operator (rows of dict N, D, abs, n).

    Form.  The per-row counts are written in regrid_reference's linearised form, (2n + 4)·u for a row of n entries, not as
    γ(2n) = 2n·u / (1 − 2n·u): the two agree to first order and the + 4 exceeds γ(2n) − 2n·u = (2n·u)² / (1 − 2n·u) for every row
    of fewer than 2²⁶ entries ((2n·u)² < 4u; the rows here have a few hundred), so the linearised count is the larger of the two
    here; the ranks' additions use γ itself.

    Derivation.  A device row sum of n rounded products lies within (2n + 4)·u·Σ|w·x| of the exact N (regrid_reference.bound:
    n products, n − 1 additions in any order, second-order terms), the coverage within (2n + 4)·u·D.  Adding R ranks' sums takes
    R − 1 more additions of partial sums that are each at most Σ|w·x| (resp. D) in size: (R − 1)·u·(1 + small)·Σ|w·x|, taken as
    γ(R − 1)·(1 + γ(2n + 4)).  So  δN ≤ Σ_r (2n_r + 4)·u·A_r + γ(R − 1)·(1 + γ(2n + 4))·A  and the same for δD with D for A
    (A = Σ_r A_r, D = Σ_r D_r exactly: every entry lies in one tile).  The quotient N̂ / D̂, rounded once, is within
    (δN + |N / D|·δD) / (D − δD) + u·|N̂ / D̂| of N / D; |N / D| ≤ A / D.  The single domain's mean is within (2n + 4)·u·A / D of
    N / D (regrid_reference.bound).  The tolerance is the sum of the two, with u·|N̂ / D̂| ≤ u·(1 + small)·A / D taken as 2u·A / D."""
    *ranks, whole = definitions
    n_rows, n_fields = len(whole), len(whole[0]["N"])
    tol = np.zeros((n_fields, n_rows))
    for r in range(n_rows):
        w = whole[r]
        if w["D"] == 0:
            continue                                   # a NaN row on both sides: compared as such, not by a tolerance
        n, R = w["n"], len(ranks)
        extra = gamma(R - 1) * (1.0 + gamma(2 * n + 4))
        dD = sum((2 * d[r]["n"] + 4) * U * d[r]["D"] for d in ranks) + extra * w["D"]
        for f in range(n_fields):
            A = w["abs"][f]
            dN = sum((2 * d[r]["n"] + 4) * U * d[r]["abs"][f] for d in ranks) + extra * A
            combined = (dN + A / w["D"] * dD) / (w["D"] - dD) + 2 * U * A / w["D"]
            tol[f, r] = combined + (2 * n + 4) * U * A / w["D"]
    return tol
