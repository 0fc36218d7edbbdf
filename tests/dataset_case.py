"""Designed planes and weight maps for the staged dataset (tests/test_dataset_cpu.py, tests/test_dataset.py).

SMALL (24 × 12 source) carries, in one plane:
  a one-cell island at (j 2, i 4) whose four donors are all valid;
  a continent over columns 22, 23, 0 (rows 4 … 8) that crosses the x seam: periodic and non-periodic staging differ on it;
  land on the first row (i 3 … 5; the cell (0, 4) has N as its only valid donor) and on the last row (i 2 … 3);
  the corners (0, 0) and (11, 23): two donors each when x does not wrap, three when it does;
  a 10 × 10 block (rows 1 … 10, columns 9 … 18): five sweeps;
  +Inf at (10, 3), the S donor of the land cell (11, 3).
LARGE (80 × 40 source) carries a continent of 60 × 28 cells over columns 70 … 79, 0 … 49 and rows 6 … 33 — wider than one LDS
tile of the tiled inpainting at any sweeps_per_launch, fourteen sweeps deep (more than eight sweeps per launch), across tile
seams and the x seam — and a few islands."""
import math

import numpy as np


def _base(ns_x, ns_y):
    i, j = np.meshgrid(np.arange(ns_x, dtype=np.float64), np.arange(ns_y, dtype=np.float64))
    return (34.0 + 2.0 * np.sin(0.37 * i + 0.011 * j * j) + 0.013 * i * j / (1.0 + 0.1 * j)).astype(np.float32)


def small_plane():
    p = _base(24, 12)
    p[2, 4] = np.nan
    p[4:9, [22, 23, 0]] = np.nan
    p[0, 3:6] = np.nan
    p[11, 2:4] = np.nan
    p[0, 0] = np.nan
    p[11, 23] = np.nan
    p[1:11, 9:19] = np.nan
    p[10, 3] = np.inf
    return p


def large_plane():
    p = _base(80, 40)
    p[6:34, 70:] = np.nan
    p[6:34, :50] = np.nan
    for j, i in ((1, 7), (2, 60), (37, 33), (38, 79), (0, 0), (39, 41), (20, 58), (20, 59), (21, 59)):
        p[j, i] = np.nan
    return p


def full_plane():
    return _base(24, 12)


def empty_plane():
    return np.full((12, 24), np.nan, dtype=np.float32)


# name → (plane, periodic_x, max_sweeps)
def staging_cases():
    s, l = small_plane(), large_plane()
    return {
        "small_periodic": (s, True, -1),
        "small_cut": (s, False, -1),
        "small_no_sweep": (s, True, 0),
        "small_two_sweeps": (s, False, 2),
        "no_nan": (full_plane(), True, -1),
        "all_nan": (empty_plane(), True, -1),
        "all_nan_limited": (empty_plane(), False, 2),
        "large_periodic": (l, True, -1),
        "large_cut": (l, False, -1),
        "large_nine_sweeps": (l, True, 9),
    }


FILL_VALUE = -7.5

# ocean grids of the regridding checks: (nx, ny) → the halo widths it is staged under
OCEAN_GRIDS = {(17, 9): ((2, 3), (4, 2)), (77, 23): ((7, 2), (3, 5))}


def fractional_indices(nx, ny, hx, hy, ns_x, ns_y):
    """(fi [nx + 2hx], fj [ny + 2hy]) of a lat-lon ocean grid on the dataset's grid, as functions of the interior index (so that
    they are the same numbers under any halo width): fi runs below 0 and beyond ns_x − 1 (periodic x: negative indices step
    west, the last interval wraps), fj below 0 and beyond ns_y − 1 (clamped)."""
    i = np.arange(-hx, nx + hx, dtype=np.float64)
    j = np.arange(-hy, ny + hy, dtype=np.float64)
    fi = (i + 0.5) * (ns_x / nx) - 0.5 + 0.03125 * np.sin(1.0 + i)
    fj = (j + 0.5) * ((ns_y + 1.5) / ny) - 1.25 + 0.0625 * np.cos(j)
    fi[hx + nx // 2] = float(math.floor(fi[hx + nx // 2]))   # an exact node: ξ = 0
    return fi, fj


def weights_2d(fi, fj):
    return np.ascontiguousarray(np.broadcast_to(fi[None, :], (fj.size, fi.size))), np.ascontiguousarray(np.broadcast_to(fj[:, None], (fj.size, fi.size)))
