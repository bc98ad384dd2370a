"""The planning of one surface for ONE wavefront, in scalars: the yardstick for ``paos_amd.run._plan_surface`` and the
rules of ``_SurfaceApertures``.  It restates the reference's formulas (paos/core/run.py:81-122: the coordinate break, the
aperture geometry with ``math.sqrt``, ``make_aperture`` and the bounding-box test) and, per aperture object, what the walk
derives from one: the live rows and columns behind a clear aperture, and whether it may ride on a pass as line records."""
import math

import numpy as np

from paos_amd import _lib
from paos_amd.aperture import EllipticalAperture, bbox_misses_grid, make_aperture
from paos_amd.coordinate_break import coordinate_break

MASK_RUN = 192  # kMaskW of csrc/frugal_pass.h


class Ray:
    """The two paraxial rays of one field point (run.py:64-65)."""

    def __init__(self, field):
        self.vt, self.vs = np.array([0.0, field["ut"]]), np.array([0.0, field["us"]])

    @property
    def still(self):
        return not (np.any(self.vt) or np.any(self.vs))

    def advance(self, abcd_t, abcd_s):
        self.vt, self.vs = abcd_t() @ self.vt, abcd_s() @ self.vs


def plan_aperture(ray, item, n, dx, dy):
    """run.py:81-122 for one wavefront: the coordinate break moves ``ray``; returns (aperture object, obscuration) or None
    where the item has no aperture or its radii are not both finite.  ``TypeError`` when the box misses the grid."""
    if item["type"] == "Coordinate Break":
        ray.vt, ray.vs = coordinate_break(ray.vt, ray.vs, item["xdec"], item["ydec"], item["xrot"], item["yrot"], 0.0)
    ap = item.get("aperture")
    if ap is None:
        return None
    xdec = ap["xc"] if math.isfinite(ap["xc"]) else ray.vs[0]
    ydec = ap["yc"] if math.isfinite(ap["yc"]) else ray.vt[0]
    xrad, yrad = ap["xrad"], ap["yrad"]
    xrad *= math.sqrt(1 / (ray.vs[1] ** 2 + 1))
    yrad *= math.sqrt(1 / (ray.vt[1] ** 2 + 1))
    xaper, yaper = xdec - ray.vs[0], ydec - ray.vt[0]
    if not (math.isfinite(xrad) and math.isfinite(yrad)):
        return None
    handle = make_aperture(n, dx, dy, xaper, yaper, hx=xrad, hy=yrad, shape=ap["shape"])
    if bbox_misses_grid(handle, n):
        raise TypeError("aperture does not overlap the grid (mask is None in the reference)")
    return handle, ap["type"] != "aperture"


def block_of(ap):
    """The parameter block of paos_aperture for what ``plan_aperture`` returned: all zero for None."""
    return [0.0] * _lib.APERTURE_STRIDE if ap is None else ap[0].block(obscuration=ap[1])


def fits_line_records(handle, obscuration, n, precision):
    if n < (1024 if precision == "fp64" else 2048) or handle.theta != 0.0:
        return False
    if isinstance(handle, EllipticalAperture):
        a, b = handle.a, handle.b
        if not (a >= 2.0 and b >= 2.0):
            return False
        return (2.0 * a * math.sqrt(3.0 / b) + 8.0 <= MASK_RUN and
                2.0 * b * math.sqrt(3.0 / a) + 8.0 <= MASK_RUN)
    return not obscuration and handle.w > 0.0 and handle.h > 0.0


def all_fit_line_records(aps, n, precision):
    """Over the items that carry an aperture; False when none does."""
    aps = [ap for ap in aps if ap is not None]
    return bool(aps) and all(fits_line_records(h, o, n, precision) for h, o in aps)


def _clear_extent(ap, axis, n):
    """[lo, hi) along ``axis`` (0: columns, 1: rows) outside which a clear untilted aperture leaves exact zeros (photutils'
    bounding box widened by a pixel), or None."""
    if ap is None or ap[1] or ap[0].theta != 0.0:
        return None
    h = ap[0]
    if isinstance(h, EllipticalAperture):
        ext = (h.a, h.b)[axis]
    else:
        ext = (h.w, h.h)[axis] / 2.0
    c = h._xy[axis]
    if not (math.isfinite(c) and math.isfinite(ext) and ext > 0.0):
        return None
    lo = max(0, int(math.floor(c - ext + 0.5)) - 1)
    hi = min(n, int(math.ceil(c + ext + 0.5)) + 1)
    return None if lo >= hi else [lo, hi]


def live_rows_after(aps, live, n):
    """Rows that may be non-zero after the apertures ``aps`` (one per item: ``plan_aperture``'s results) were applied;
    ``live`` is updated in place, one [lo, hi) per item."""
    for ap, r in zip(aps, live):
        box = _clear_extent(ap, 1, n)
        if box is None:
            continue
        r[0], r[1] = max(r[0], box[0]), min(r[1], box[1])
        if r[0] >= r[1]:  # disjoint boxes: everything is zero; keep a token range
            r[0], r[1] = 0, 0


def live_cols_of(aps, n):
    """Per item the columns [lo, hi) outside which a clear aperture leaves exact zeros, or None when some item has no
    such aperture."""
    out = [_clear_extent(ap, 0, n) for ap in aps]
    return None if any(box is None for box in out) else out


def start_shape(aps):
    """The one shape code when every item carries an aperture and all share a shape, else None."""
    if any(ap is None for ap in aps) or len({isinstance(ap[0], EllipticalAperture) for ap in aps}) != 1:
        return None
    return _lib.SHAPE_ELLIPSE if isinstance(aps[0][0], EllipticalAperture) else _lib.SHAPE_RECT
