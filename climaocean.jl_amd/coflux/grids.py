"""The ocean grids of the surface path: only the metadata that interpolation, folding and area weights need."""
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import synthetic

EARTH_RADIUS = 6.371e6   # m (Oceananigans' R_Earth)


@dataclass
class LatitudeLongitudeGrid:
    """README.md:56-61 (only the metadata the surface path needs)."""
    size: tuple = (1440, 560, 10)
    halo: tuple = (7, 7, 7)
    longitude: tuple = (0.0, 360.0)
    latitude: tuple = (-70.0, 70.0)
    z: tuple = (-3000.0, 0.0)
    device: int = 0

    @property
    def surface_shape(self):
        (nx, ny, _), (hx, hy, _) = self.size, self.halo
        return (ny + 2 * hy, nx + 2 * hx)

    @property
    def surface_z(self):
        nz = self.size[2]
        dz = (self.z[1] - self.z[0]) / nz
        return self.z[1] - 0.5 * dz  # centre of the top cell (uniform spacing)

    def fractional_indices(self, nsx=synthetic.JRA55_NX, nsy=synthetic.JRA55_NY):
        nx, ny, _ = self.size
        hx, hy, _ = self.halo
        return synthetic.latlon_fractional_indices(nx, ny, hx, hy, latitude=self.latitude, nsx=nsx, nsy=nsy)

    fold_north = False

    def interpolation_weights(self, to_device, nsx=synthetic.JRA55_NX, nsy=synthetic.JRA55_NY):
        """cf_interp_weights for this grid: separable fractional indices into the JRA55 grid (no rotation)."""
        fi, fj, phi = self.fractional_indices(nsx, nsy)
        return dict(separable=True, fi=to_device(fi), fj=to_device(fj), latitude=to_device(phi))

    def cell_latitudes(self):
        """φ [deg] of the cell centres in the halo layout (ny + 2hy, nx + 2hx)."""
        (nx, ny, _), (hx, hy, _) = self.size, self.halo
        phi = self.latitude[0] + (np.arange(-hy, ny + hy) + 0.5) * (self.latitude[1] - self.latitude[0]) / ny
        return np.ascontiguousarray(np.broadcast_to(phi[:, None], self.surface_shape))

    def cell_areas(self):
        """Az = R² Δλ (sin φ_f[j+1] − sin φ_f[j]) [m²] in the halo layout (the formula runs on through the halo rows)."""
        (nx, ny, _), (hx, hy, _) = self.size, self.halo
        dlam = np.deg2rad((self.longitude[1] - self.longitude[0]) / nx)
        faces = np.deg2rad(self.latitude[0] + np.arange(-hy, ny + hy + 1) * (self.latitude[1] - self.latitude[0]) / ny)
        rows = EARTH_RADIUS ** 2 * dlam * np.diff(np.sin(faces))
        return np.ascontiguousarray(np.broadcast_to(rows[:, None], self.surface_shape))


@dataclass
class TripolarGrid:
    """TripolarGrid(arch; size = (360, 180, Nz), halo = (5, 5, 4), z, …) — OceanConfigurations/one_degree_tripolar.jl:32,48-51
    (1°), half_degree_tripolar.jl:48-51 (720×360), sixth_degree_tripolar.jl:33-36 (2160×1080, halo 7), tenth_degree… (3600×1800).
    Only what the surface path needs: cell-centre positions → general (2-D) fractional indices into the JRA55 grid, the
    rotation of the grid's i-axis against geographic east (visualize/cache.jl:406-427: the winds are rotated into the
    grid frame) and the north fold (the last row of tracer points is its own mirror image; Oceananigans' zipper
    boundary).  The mesh itself comes from `synthetic.tripolar_mesh` (a bipolar cap with the real fold topology) unless
    `longitude` / `latitude` / rotation arrays of the real grid are handed in."""
    size: tuple = (360, 180, 10)
    halo: tuple = (5, 5, 4)
    z: tuple = (-3000.0, 0.0)
    southernmost_latitude: float = -80.0
    first_pole_longitude: float = 75.0
    north_poles_latitude: float = 55.0
    device: int = 0
    longitude: Optional[np.ndarray] = None     # (ny, nx) cell-centre λ [deg] of a real grid (else synthetic)
    latitude: Optional[np.ndarray] = None      # (ny, nx) cell-centre φ [deg]
    cos_rotation: Optional[np.ndarray] = None
    sin_rotation: Optional[np.ndarray] = None
    area: Optional[np.ndarray] = None          # (ny, nx) cell areas Az [m²] of a real grid (nothing is guessed without them)

    fold_north = True

    def _halo_layout(self, a, fill):
        (nx, ny, _), (hx, hy, _) = self.size, self.halo
        g = np.full(self.surface_shape, fill, dtype=np.asarray(a).dtype)
        g[hy:hy + ny, hx:hx + nx] = a
        return g

    def cell_latitudes(self):
        """φ [deg] of the cell centres in the halo layout; the halos hold NaN (no cell there belongs to a hemisphere)."""
        return self._halo_layout(np.asarray(self.mesh()[1], dtype=np.float64), np.nan)

    def cell_areas(self):
        """The `area` array of the real grid in the halo layout (halos 0)."""
        if self.area is None:
            raise ValueError("TripolarGrid: cell areas are not derived from the synthetic mesh; pass TripolarGrid(area=Az) "
                             "(ny × nx, m²) or hand an area array to the integrals")
        return self._halo_layout(np.asarray(self.area, dtype=np.float64), 0.0)

    @property
    def surface_shape(self):
        (nx, ny, _), (hx, hy, _) = self.size, self.halo
        return (ny + 2 * hy, nx + 2 * hx)

    @property
    def surface_z(self):
        nz = self.size[2]
        dz = (self.z[1] - self.z[0]) / nz
        return self.z[1] - 0.5 * dz

    def mesh(self):
        nx, ny, _ = self.size
        if self.longitude is not None:
            if self.latitude is None or self.cos_rotation is None or self.sin_rotation is None:
                raise ValueError("TripolarGrid: longitude, latitude, cos_rotation and sin_rotation come together")
            return self.longitude, self.latitude, self.cos_rotation, self.sin_rotation
        return synthetic.tripolar_mesh(nx, ny, southernmost_latitude=self.southernmost_latitude,
                                       cap_latitude=self.north_poles_latitude, pole_longitude=self.first_pole_longitude)

    def interpolation_weights(self, to_device, nsx=synthetic.JRA55_NX, nsy=synthetic.JRA55_NY, rows=2):
        """General weights + rotation, halo-inclusive: periodic in x, the north halo rows are the fold images of the
        interior rows (their i-axis points the other way: rotation reversed), as synthetic.tripolar_case builds them."""
        (nx, ny, _), (hx, hy, _) = self.size, self.halo
        lam, phi, cos_t, sin_t = self.mesh()

        def halo2d(a):
            g = np.empty((ny + 2 * hy, nx + 2 * hx))
            g[hy:hy + ny, hx:hx + nx] = a
            g[:hy] = g[hy:hy + 1]
            g[hy + ny:] = g[hy + ny - 1:hy + ny]
            g[:, :hx], g[:, hx + nx:] = g[:, nx:nx + hx], g[:, hx:2 * hx]
            return g
        LAM, PHI, COS, SIN = (halo2d(a) for a in (lam, phi, cos_t, sin_t))
        r = min(rows, hy)
        for a in (LAM, PHI, COS, SIN):
            synthetic.fold_north(a, nx, ny, hx, hy, r, "center", 1)
        COS[hy + ny:hy + ny + r] *= -1.0
        SIN[hy + ny:hy + ny + r] *= -1.0
        fi = LAM / (360.0 / nsx)
        fj = (PHI - synthetic.JRA55_LAT0) / (2 * 89.57 / (nsy - 1))
        c = np.ascontiguousarray
        return dict(separable=False, fi=to_device(c(fi)), fj=to_device(c(fj)), cos_rot=to_device(c(COS)), sin_rot=to_device(c(SIN)),
                    latitude=to_device(c(PHI)))
