"""NumPy restatement of the derived averager (include/coflux.h: cf_average_create_derived): every kind, the scale and the
running-mean recurrence, one IEEE operation per NumPy operation in the order the header writes them, so that the device
is held to it bit for bit.  `DerivedModel` keeps each step in a method of its own: tests plant defects by overriding one.

Arrays are float64 in the halo layout (ny + 2hy, nx + 2hx); results are interior arrays (ny, nx)."""
import numpy as np

(FIELD, PRODUCT, CENTER_X, CENTER_Y, CENTER_X_SQUARE, CENTER_Y_SQUARE, KINETIC_ENERGY, EAST, NORTH) = range(9)
AT_CENTERS = 1
KIND_NAMES = ("field", "product", "center_x", "center_y", "center_x_square", "center_y_square", "kinetic_energy", "east", "north")
# roundings of x per kind (the · 0.5 is exact); EAST / NORTH: from faces, at centres
ROUNDINGS = {FIELD: 0, PRODUCT: 1, CENTER_X: 1, CENTER_Y: 1, CENTER_X_SQUARE: 3, CENTER_Y_SQUARE: 3, KINETIC_ENERGY: 7,
             EAST: (5, 3), NORTH: (5, 3)}
HALF = np.float64(0.5)


def reads_b(kind):
    return kind in (PRODUCT, KINETIC_ENERGY, EAST, NORTH)


def reads_east(kind, flags=0):
    """the kind reads `a` at [i+1]"""
    return kind in (CENTER_X, CENTER_X_SQUARE, KINETIC_ENERGY) or (kind in (EAST, NORTH) and not flags & AT_CENTERS)


def reads_north(kind, flags=0):
    """(a is read at [j+1], b is read at [j+1])"""
    return kind in (CENTER_Y, CENTER_Y_SQUARE), kind == KINETIC_ENERGY or (kind in (EAST, NORTH) and not flags & AT_CENTERS)


class DerivedModel:
    def __init__(self, nx, ny, hx, hy):
        self.nx, self.ny, self.hx, self.hy = nx, ny, hx, hy

    # -- addressing ------------------------------------------------------------------------------
    def here(self, a):
        return a[self.hy:self.hy + self.ny, self.hx:self.hx + self.nx]

    def east(self, a):
        return a[self.hy:self.hy + self.ny, self.hx + 1:self.hx + self.nx + 1]

    def north(self, a):
        return a[self.hy + 1:self.hy + self.ny + 1, self.hx:self.hx + self.nx]

    # -- arithmetic, one rounding per operation ------------------------------------------------------
    def center(self, lo, hi):
        return (lo + hi) * HALF

    def center_square(self, lo, hi):
        return (lo * lo + hi * hi) * HALF

    def kinetic_energy(self, a, b):
        return (self.center_square(self.here(a), self.east(a)) + self.center_square(self.here(b), self.north(b))) * HALF

    def components(self, flags, a, b):
        if flags & AT_CENTERS:
            return self.here(a), self.here(b)
        return self.center(self.here(a), self.east(a)), self.center(self.here(b), self.north(b))

    def rotate_east(self, p, q, c, s):
        return p * c - q * s

    def rotate_north(self, p, q, c, s):
        return p * s + q * c

    def scaled(self, x, scale):
        return x * np.float64(scale)

    def sample(self, kind, flags, a, b, scale, cos=None, sin=None):
        """the interior array that enters the recurrence"""
        if kind in (EAST, NORTH):
            p, q = self.components(flags, a, b)
            rotate = self.rotate_east if kind == EAST else self.rotate_north
            return self.scaled(rotate(p, q, self.here(cos), self.here(sin)), scale)
        return self.scaled(self.value(kind, a, b), scale)

    def value(self, kind, a, b):
        if kind == FIELD:
            return self.here(a)
        if kind == PRODUCT:
            return self.here(a) * self.here(b)
        if kind == CENTER_X:
            return self.center(self.here(a), self.east(a))
        if kind == CENTER_Y:
            return self.center(self.here(a), self.north(a))
        if kind == CENTER_X_SQUARE:
            return self.center_square(self.here(a), self.east(a))
        if kind == CENTER_Y_SQUARE:
            return self.center_square(self.here(a), self.north(a))
        if kind == KINETIC_ENERGY:
            return self.kinetic_energy(a, b)
        raise ValueError(kind)


def recurrence(samples):
    """[(sample, weight)] → mean: the first collection stores, each later one m = (m · c_prev) + (sample · c_new) with
    c_prev = T_prev / T_cur, c_new = w / T_cur computed in double as the host does."""
    m, total = None, 0.0
    with np.errstate(all="ignore"):
        for x, w in samples:
            cur = total + w
            m = np.array(x, dtype=np.float64) if m is None else m * np.float64(total / cur) + x * np.float64(w / cur)
            total = cur
    return m
