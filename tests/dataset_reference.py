"""The definition of a staged dataset (include/coflux.h: cf_dataset_*) in NumPy and plain Python: the nearest-neighbour
inpainting sweep and its loop, the depth by breadth-first search, the bilinear regridding with periodic x and clamped y, the
clock and the blend.  Every number is a Python float or a float64 array: IEEE double, no contraction."""
import bisect
import math
from collections import deque

import numpy as np


def sweep(p, periodic_x):
    """One sweep: q from p.  A cell that is not NaN is copied; a NaN cell takes (donors that are not NaN in p, added in the
    order W, S, E, N starting from the first valid one) / count, or stays NaN without any."""
    ny, nx = p.shape
    q = p.copy()
    for j, i in zip(*np.nonzero(np.isnan(p))):
        donors = []
        if i > 0 or periodic_x:
            donors.append(p[j, (i - 1) % nx])
        if j > 0:
            donors.append(p[j - 1, i])
        if i + 1 < nx or periodic_x:
            donors.append(p[j, (i + 1) % nx])
        if j + 1 < ny:
            donors.append(p[j + 1, i])
        valid = [float(d) for d in donors if not math.isnan(d)]
        if valid:
            total = valid[0]
            for d in valid[1:]:
                total = total + d
            with np.errstate(all="ignore"):
                q[j, i] = np.float64(total) / np.float64(len(valid))
    return q


def sweeps_needed(plane, periodic_x):
    """How many sweeps the loop `while any NaN: sweep` runs before nothing changes any more (0 for a plane without NaN or
    without a valid cell)."""
    p = np.asarray(plane, dtype=np.float64)
    n = 0
    while np.isnan(p).any():
        q = sweep(p, periodic_x)
        if np.array_equal(np.isnan(q), np.isnan(p)):
            break
        p, n = q, n + 1
    return n


def distances(plane, periodic_x):
    """4-connected distance of every cell from the nearest cell that is not NaN (x wraps when periodic); −1: unreachable."""
    nan = np.isnan(np.asarray(plane, dtype=np.float64))
    ny, nx = nan.shape
    dist = np.where(nan, -1, 0).astype(np.int64)
    queue = deque((j, i) for j in range(ny) for i in range(nx) if not nan[j, i])
    while queue:
        j, i = queue.popleft()
        for jj, ii in ((j, i - 1), (j, i + 1), (j - 1, i), (j + 1, i)):
            if periodic_x:
                ii %= nx
            if 0 <= ii < nx and 0 <= jj < ny and dist[jj, ii] < 0:
                dist[jj, ii] = dist[j, i] + 1
                queue.append((jj, ii))
    return dist


def depth(plane, periodic_x):
    return int(max(distances(plane, periodic_x).max(), 0))


def inpaint(plane, periodic_x, max_sweeps, fill_value):
    """(the staged f64 plane, sweeps, cells filled by a sweep, cells given fill_value) of a float32 plane."""
    p = np.asarray(plane, dtype=np.float32).astype(np.float64)
    missing = int(np.isnan(p).sum())
    d = depth(p, periodic_x)
    n = d if max_sweeps < 0 else min(max_sweeps, d)
    for _ in range(n):
        p = sweep(p, periodic_x)
    left = np.isnan(p)
    p[left] = fill_value
    return p, n, missing - int(left.sum()), int(left.sum())


def stencil(fi, fj, ns_x, ns_y):
    """The four source nodes and weights of fractional indices (fi, fj): periodic x, clamped y (land_freshwater_cell)."""
    xi, eta = fi - math.floor(fi), fj - math.floor(fj)
    i0, ja = int(math.trunc(fi)), int(math.trunc(fj))
    sx = 1 if fi > 0.0 else (-1 if fi < 0.0 else 0)
    sy = 1 if fj > 0.0 else (-1 if fj < 0.0 else 0)
    is0, is1 = i0 % ns_x, (i0 + sx) % ns_x
    j0, j1 = min(max(ja, 0), ns_y - 1), min(max(ja + sy, 0), ns_y - 1)
    w = ((1.0 - xi) * (1.0 - eta), (1.0 - xi) * eta, xi * (1.0 - eta), xi * eta)
    return ((j0, is0), (j1, is0), (j0, is1), (j1, is1)), w


def regrid(plane, fi2d, fj2d, nx, ny, hx, hy, ring):
    """(level, bound): the ocean-grid array [ny + 2hy, nx + 2hx] — bilinear on the ring window, zero elsewhere — and per cell
    max |corner| (the tolerance of a comparison is 8 · 2⁻⁵³ · bound: four products and three additions of weights in [0, 1])."""
    ns_y, ns_x = plane.shape
    out = np.zeros((ny + 2 * hy, nx + 2 * hx))
    bound = np.zeros_like(out)
    for j in range(-ring, ny + ring):
        for i in range(-ring, nx + ring):
            nodes, w = stencil(float(fi2d[j + hy, i + hx]), float(fj2d[j + hy, i + hx]), ns_x, ns_y)
            c = [float(plane[n]) for n in nodes]
            out[j + hy, i + hx] = w[0] * c[0] + w[1] * c[1] + w[2] * c[2] + w[3] * c[3]
            bound[j + hy, i + hx] = max(abs(v) for v in c)
    return out, bound


def time_index(times, period, time):
    """(level1, level2, fraction) of cf_dataset_time_index on a good table; ValueError for a time that is not finite."""
    if not math.isfinite(time):
        raise ValueError("time is not finite")
    n = len(times)
    if n == 1:
        return 0, 0, 0.0
    tau = time
    if period > 0.0:
        r = math.fmod(time - times[0], period)
        if r < 0.0:
            r += period
        tau = times[0] + r
        if tau >= times[-1]:
            return n - 1, 0, (tau - times[-1]) / (times[0] + period - times[-1])
    else:
        if tau < times[0]:
            return 0, 0, 0.0
        if tau >= times[-1]:
            return n - 1, n - 1, 0.0
    k = bisect.bisect_right(times, tau) - 1
    return k, k + 1, (tau - times[k]) / (times[k + 1] - times[k])


def times_ok(times, period):
    if len(times) < 1 or not all(math.isfinite(t) for t in times) or any(b <= a for a, b in zip(times, times[1:])):
        return False
    if not math.isfinite(period) or period < 0.0:
        return False
    return period == 0.0 or period > times[-1] - times[0]


def blend(a, b, f):
    """S★ between two levels: level a when f is 0.0, else b·f + a·(1 − f) (each operation rounded; a build that contracts
    differs by one rounding)."""
    return a.copy() if f == 0.0 else b * f + a * (1.0 - f)
