"""Sparse surface operators for FluxContext.regridder (cf_regrid_*): builders of the CSR arrays on the host (NumPy only) and
the writer that applies them to the window means of SurfaceFluxAverages on the device.

What a reference run derives from the surface for its figures (experiments/OMIPSimulations/scripts/visualize/cache.jl):
regrid_surface_to_latlon (:983-1011) conservatively regrids field · mask and mask onto a shared 360 × 180 latitude–longitude
grid and divides, NaN where a destination cell has no ocean; compute_zonal_mean (:918-937) sums the regridded field · mask · A
and mask · A per latitude row and divides.  Both are one sparse matrix with a masked normalisation — what cf_regrid_apply
computes; the matrix is what this module builds.  An operator is CSR over DESTINATION rows; a column is the interior cell
number c = j·nx + i of the source grid.

    conservative_latlon_weights   latitude–longitude source → latitude–longitude destination, exact overlap areas
    zonal_mean_weights            the same operator summed over the destination longitudes: one row per latitude band
    zonal_band_weights            any grid with cell-centre latitudes and areas: BINNING by centre latitude, not conservative
    csr_from_triplets             the way in for an operator built elsewhere (ConservativeRegridding.jl's matrix of a tripolar grid)
"""
from dataclasses import dataclass

import numpy as np

from . import abi
from .grids import EARTH_RADIUS


@dataclass
class SurfaceOperator:
    """CSR over destination rows: row r owns entries row_ptr[r] … row_ptr[r + 1] − 1; `shape` is the destination's, (nlat, nlon)
    for a map (row = j_dst · nlon + i_dst) or (nlat,) for bands."""
    row_ptr: np.ndarray   # int64, n_rows + 1
    col: np.ndarray       # int32, interior cell numbers of the source grid
    weight: np.ndarray    # float64, ≥ 0
    shape: tuple

    @property
    def n_rows(self):
        return self.row_ptr.size - 1

    def __iter__(self):   # row_ptr, col, weight = operator
        return iter((self.row_ptr, self.col, self.weight))


def csr_from_triplets(rows, cols, weights, n_rows, shape=None):
    """(row, col, weight) triplets in any order → SurfaceOperator, by a STABLE sort on (row, col): duplicates are kept, in the
    order they were given (the device adds a row's entries in a fixed order of their positions, so the order is part of the
    result's bits).  Rows without a triplet are empty rows."""
    rows = np.asarray(rows, dtype=np.int64).ravel()
    cols = np.asarray(cols, dtype=np.int64).ravel()
    weights = np.asarray(weights, dtype=np.float64).ravel()
    if not (rows.size == cols.size == weights.size):
        raise ValueError(f"csr_from_triplets: {rows.size} rows, {cols.size} cols, {weights.size} weights")
    if n_rows < 1 or (rows.size and (rows.min() < 0 or rows.max() >= n_rows)):
        raise ValueError(f"csr_from_triplets: rows outside 0 … {n_rows - 1}")
    if cols.size and (cols.min() < 0 or cols.max() >= 2 ** 31):
        raise ValueError("csr_from_triplets: columns outside 0 … 2^31 − 1")
    order = np.lexsort((cols, rows))   # stable: the last key is the primary one
    row_ptr = np.zeros(n_rows + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n_rows), out=row_ptr[1:])
    return SurfaceOperator(row_ptr, cols[order].astype(np.int32), weights[order].copy(), tuple(shape) if shape is not None else (n_rows,))


def _faces(lo, hi, n):
    """The n + 1 cell faces [deg] of a uniform axis — the expression LatitudeLongitudeGrid.cell_areas() uses, so that the sines
    of a source grid's faces are the same bits here and there."""
    return lo + np.arange(0, n + 1) * (hi - lo) / n


def _overlaps(src_faces, dst_faces, period=None):
    """Every (i_dst, i_src, lo, hi) [deg] with hi > lo: the overlap of source cell i_src with destination cell i_dst on one
    axis.  With `period` the source cells are taken modulo it into the destination's range (a cell that straddles the seam
    gives two pieces)."""
    d0, nd = dst_faces[0], dst_faces.size - 1
    width = (dst_faces[-1] - d0) / nd
    out = []
    for i in range(src_faces.size - 1):
        a, b = float(src_faces[i]), float(src_faces[i + 1])
        pieces = [(a, b)]
        if period is not None:
            shift = np.floor((a - d0) / period) * period
            a, b = a - shift, b - shift
            pieces = [(a, min(b, d0 + period))] + ([(d0, b - period)] if b > d0 + period else [])
        for lo, hi in pieces:
            first = max(int(np.floor((lo - d0) / width)) - 1, 0)
            last = min(int(np.ceil((hi - d0) / width)) + 1, nd)
            for k in range(first, last):
                o_lo, o_hi = max(lo, float(dst_faces[k])), min(hi, float(dst_faces[k + 1]))
                if o_hi > o_lo:
                    out.append((k, i, o_lo, o_hi))
    return out


def _latlon_source(src):
    nx, ny = src.size[0], src.size[1]
    return nx, ny, _faces(src.longitude[0], src.longitude[1], nx), _faces(src.latitude[0], src.latitude[1], ny)


def conservative_latlon_weights(src, nlon=360, nlat=180, longitude=(0.0, 360.0), latitude=(-90.0, 90.0)):
    """The conservative map of a LatitudeLongitudeGrid onto an nlon × nlat latitude–longitude grid:
    weight = R² · Δλ_overlap · (sin φ_hi − sin φ_lo), the exact area of the overlap of a source and a destination cell on the
    sphere, for every pair that overlaps.  Separable (a longitude overlap times a latitude overlap); longitudes are taken
    modulo 360°, so a source that starts at −180° or at 20° meets a destination on (0, 360).  Row j_dst · nlon + i_dst."""
    nx, ny, lam_s, phi_s = _latlon_source(src)
    lon = _overlaps(lam_s, _faces(longitude[0], longitude[1], nlon), period=360.0)
    lat = _overlaps(phi_s, _faces(latitude[0], latitude[1], nlat))
    i_dst, i_src = (np.array([p[k] for p in lon], dtype=np.int64) for k in (0, 1))
    j_dst, j_src = (np.array([p[k] for p in lat], dtype=np.int64) for k in (0, 1))
    dlam = np.deg2rad(np.array([p[3] - p[2] for p in lon]))
    dsin = np.array([np.sin(np.deg2rad(p[3])) - np.sin(np.deg2rad(p[2])) for p in lat])
    rows = (j_dst[:, None] * nlon + i_dst[None, :]).ravel()
    cols = (j_src[:, None] * nx + i_src[None, :]).ravel()
    weights = ((EARTH_RADIUS ** 2 * dlam)[None, :] * dsin[:, None]).ravel()
    return csr_from_triplets(rows, cols, weights, nlon * nlat, shape=(nlat, nlon))


def zonal_mean_weights(src, nlat=180, latitude=(-90.0, 90.0)):
    """One row per latitude band: row b holds, for every source cell that reaches into band b, the area of the part inside,
    R² · Δλ_cell · (sin φ_hi − sin φ_lo) — conservative_latlon_weights summed over the destination longitudes (of a destination
    that spans the full circle).  In "mean" mode one apply gives Σ_i N / Σ_i D of the regridded row, which is the reference's
    compute_zonal_mean of the regridded field."""
    nx, ny, lam_s, phi_s = _latlon_source(src)
    lat = _overlaps(phi_s, _faces(latitude[0], latitude[1], nlat))
    j_dst, j_src = (np.array([p[k] for p in lat], dtype=np.int64) for k in (0, 1))
    dsin = np.array([np.sin(np.deg2rad(p[3])) - np.sin(np.deg2rad(p[2])) for p in lat])
    dlam = np.deg2rad(np.diff(lam_s))
    rows = np.repeat(j_dst, nx)
    cols = (j_src[:, None] * nx + np.arange(nx)[None, :]).ravel()
    weights = ((EARTH_RADIUS ** 2 * dlam)[None, :] * dsin[:, None]).ravel()
    return csr_from_triplets(rows, cols, weights, nlat, shape=(nlat,))


def zonal_band_weights(grid, nlat=180, area=None, latitude=(-90.0, 90.0)):
    """Latitude bands for ANY grid with cell_latitudes() and cell areas (TripolarGrid(area=…) included): every cell goes, whole,
    into the band that holds its CENTRE latitude, with weight = its area.  This is binning, NOT conservative regridding: the
    grid carries cell centres and no vertices, so the overlap polygon of a tripolar cell with a band cannot be formed here (an
    operator that does it, built elsewhere, comes in through csr_from_triplets).  `area`: (ny, nx) interior areas or a
    halo-layout array; default grid.cell_areas().  Cells with a NaN latitude or outside `latitude` are left out."""
    (nx, ny, _), (hx, hy, _) = grid.size, grid.halo
    phi = np.asarray(grid.cell_latitudes(), dtype=np.float64)[hy:hy + ny, hx:hx + nx]
    A = np.asarray(grid.cell_areas() if area is None else area, dtype=np.float64)
    if A.shape != (ny, nx):
        A = A[hy:hy + ny, hx:hx + nx]
    width = (latitude[1] - latitude[0]) / nlat
    with np.errstate(invalid="ignore"):
        inside = (phi >= latitude[0]) & (phi <= latitude[1])
    band = np.zeros(phi.shape, dtype=np.int64)
    band[inside] = np.minimum(np.floor((phi[inside] - latitude[0]) / width).astype(np.int64), nlat - 1)
    cells = np.arange(nx * ny, dtype=np.int64).reshape(ny, nx)
    return csr_from_triplets(band[inside], cells[inside], A[inside], nlat, shape=(nlat,))


class RegriddedSurfaceMeans:
    """RegriddedSurfaceMeans(model, averages, regridder, zonal=None, on_window=None): when a window of `averages` (a
    SurfaceFluxAverages) closes, its means — still in device memory — go through the operator(s) on the device, one apply per
    operator for up to abi.REGRID_MAX_FIELDS outputs, and the result is appended to `windows` as (t_k, maps, zonal, coverage)
    and handed to on_window(t_k, maps, zonal, coverage): maps[name] (nlat, nlon) and zonal[name] (nlat,) NumPy arrays, NaN
    where the destination has no ocean; coverage = dict(map=(nlat, nlon), zonal=(nlat,)), the regridded wet mask (Σ of the wet
    weights).  `regridder` / `zonal`: a SurfaceOperator (made into a "mean" regridder on the model's context with the ocean's
    wet mask) or a SurfaceRegridder already made; either may be None.  It hooks into averages.on_window — a hook that was
    there is still called first — and SurfaceFluxAverages itself is unchanged."""

    def __init__(self, model, averages, regridder, zonal=None, on_window=None):
        ctx = self.ctx = model.interfaces.context
        self.model, self.averages, self.on_window = model, averages, on_window
        mask = model.ocean.model.wet_mask if ctx.params.mask_kind == abi.MASK_U8 else None

        self._made = []

        def made(op):
            if not isinstance(op, SurfaceOperator):   # None, or a SurfaceRegridder of the caller's (which the caller closes)
                return op, None
            self._made.append(ctx.regridder(op.row_ptr, op.col, op.weight, mask=mask, mode="mean"))
            return self._made[-1], op.shape

        (self.regridder, self.map_shape), (self.zonal, self.zonal_shape) = made(regridder), made(zonal)
        self.windows = []
        self._previous_hook = averages.on_window
        averages.on_window = self._window

    def _apply(self, rg, shape, names, fields):
        out, coverage = {}, None
        shape = shape if shape is not None else (rg.n_rows,)
        for first in range(0, len(fields), abi.REGRID_MAX_FIELDS):
            chunk = slice(first, first + abi.REGRID_MAX_FIELDS)
            for name, t in zip(names[chunk], rg.apply(fields[chunk])):
                out[name] = t.to("cpu").numpy().reshape(shape)
            coverage = rg.coverage.to("cpu").numpy().reshape(shape)
        return out, coverage

    def _window(self, t_k, arrays):
        if self._previous_hook is not None:
            self._previous_hook(t_k, arrays)
        names, fields = list(self.averages.means), list(self.averages.means.values())
        maps, zonal, coverage = {}, {}, {}
        if self.regridder is not None:
            maps, coverage["map"] = self._apply(self.regridder, self.map_shape, names, fields)
        if self.zonal is not None:
            zonal, coverage["zonal"] = self._apply(self.zonal, self.zonal_shape, names, fields)
        self.windows.append((t_k, maps, zonal, coverage))
        if self.on_window is not None:
            self.on_window(t_k, maps, zonal, coverage)

    def close(self):
        self.averages.on_window = self._previous_hook
        for rg in self._made:
            rg.close()
