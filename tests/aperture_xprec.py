"""Arbitrary-precision aperture weights: what every device path that produces or consumes a mask is measured against
(tests/test_aperture_xprec_reference.py on the CPU, tests/test_gpu_aperture_xprec.py on the GPU).

Ellipse -- ``ellipse_weights``: area(pixel INTERSECT ellipse) by closed-form strip integrals in mpmath at 50 digits.  With the
conic  A x^2 + 2 B x y + C y^2 = 1  (x, y relative to the centre; A C - B^2 = 1 / (a b)^2) a column x meets the ellipse
in  y-(x) .. y+(x),  y+-(x) = (-B x +- sqrt(C - x^2 / (a b)^2)) / C,  |x| <= xe = a b sqrt(C), and

    area = integral over [x0, x1] of  max(0, min(y+, y1) - max(y-, y0)) dx,

cut at the points where y+- meets a pixel edge (the roots of A x^2 + 2 B Y x + C Y^2 - 1 for Y = y0, y1), with
integral of y+- = -B x^2 / (2 C) +- a b S(x / xe),  S(X) = (X sqrt(1 - X^2) + asin X) / 2.  The differences cancel like
a b against a result <= 1, which costs log10(a b) of the 50 digits and nothing else.  This is different mathematics
from the kernel's edge-wise Green's theorem (oracle/aperture_np.py restates that one in fp64), and the reference test
checks it against direct quadrature of the strip integrand.  Only pixels the boundary may cross are evaluated in
mpmath; a float64 pre-filter with a margin of 1e-6 (in the conic's value, whose float64 error is ~1e-13 at the
largest case) sets the others to exactly 0 or 1.

Rectangle -- ``rectangle_weights``: the sub-sample rule itself, vectorised over pixels, with the sample positions
accumulated by the same double additions in the same order as the kernel (pointwise.h: subpixel_count_1d, rect_pixel).

Bound -- ``bound(a, b) = C_AP 2^-53 max(a, b, 1)``, absolute, on a weight: the four edge terms of the Green's-theorem
sum are each ~1/a in unit-disk coordinates and cancel to ~1/(a b); that is multiplied by a b.  The constant comes
from what the fp64 restatement of the reference (oracle/aperture_np.py, not the code under test) reaches over every
ellipse case of the two test modules -- see YARDSTICK below."""
import functools
import math

import numpy as np

DPS = 50
U64 = 2.0 ** -53
MARGIN_PX = 1e-9  # "surely 0" / "surely 1": farther than this from the boundary

# Largest |oracle/aperture_np.py - reference| / (2^-53 max(a, b, 1)) per ellipse case of
# tests/test_aperture_xprec_reference.py (which holds every ellipse of tests/test_gpu_aperture_xprec.py), as printed by
# test_oracle_against_the_reference, which asserts that none exceeds YARDSTICK_WORST:
#   the sizes the project runs   128: 40.7 x 25.2  1.96     1200: 512 x 512 at 600.3 / 599.1  2.54, at 600.5 / 600.5  1.82
#                                2400: 1100 x 40  2.83 (the worst)    400: 75 x 2  1.40    64: 0.4 x 0.3  0.11
#                                4096: 512 x 512 centred  2.00
#   ELLIPSES at n = 256          between 0.001 (sub-pixel on a corner) and 2.74 (straddles one edge); the Pythagorean
#                                circles 1.55 / 2.00 / 2.67; 1100 x 40 cut by the grid 0.23
#   TILTED                       2.01 / 1.75 / 0.32
#   frugal_ellipses(1024, 0 / 1) between 1.16 and 2.16
# In units of eps = 2^-52 the worst is 1.42.  C_AP = the next power of two at or above twice the worst.
YARDSTICK_WORST = 2.84
C_AP = 8.0


def require_mpmath():
    """The reference is mpmath's or nothing: a missing mpmath fails the tests that need it, it never skips them."""
    try:
        import mpmath
    except ImportError as exc:  # pragma: no cover
        raise AssertionError("mpmath is not installed: no arbitrary-precision aperture reference") from exc
    return mpmath


def bound(a, b):
    return C_AP * U64 * max(a, b, 1.0)


def yardstick_unit(a, b):
    """What errors are quoted in: 2^-53 max(a, b, 1)."""
    return U64 * max(a, b, 1.0)


# ---- ellipse ---------------------------------------------------------------------------------------------------------
class _Conic:
    """The ellipse's conic in the number type ``num`` (float or mpmath.mpf), centre at the origin."""

    def __init__(self, a, b, theta, num, cos, sin, sqrt):
        a, b, theta = num(a), num(b), num(theta)
        ct, st = cos(theta), sin(theta)
        self.a, self.b = a, b
        self.A = ct * ct / (a * a) + st * st / (b * b)
        self.B = ct * st * (1 / (a * a) - 1 / (b * b))
        self.C = st * st / (a * a) + ct * ct / (b * b)
        self.ab = a * b
        self.xe = sqrt(a * a * ct * ct + b * b * st * st)
        self.ye = sqrt(a * a * st * st + b * b * ct * ct)

    def q(self, x, y):
        return self.A * x * x + 2 * self.B * x * y + self.C * y * y


def _qmin(g, x0, x1, y0, y1, clamp, minimum, where):
    """min of the conic's value over the pixel [x0, x1] x [y0, y1] (0 where it holds the centre): the minimum of a
    convex quadratic over a rectangle that does not hold its minimiser lies on an edge."""
    best = None
    for x in (x0, x1):
        y = clamp(-g.B * x / g.C, y0, y1)
        v = g.q(x, y)
        best = v if best is None else minimum(best, v)
    for y in (y0, y1):
        x = clamp(-g.B * y / g.A, x0, x1)
        best = minimum(best, g.q(x, y))
    return where((x0 <= 0) & (x1 >= 0) & (y0 <= 0) & (y1 >= 0), 0 * best, best)


def _strip_area(mp, g, x0, x1, y0, y1):
    """area(pixel INTERSECT ellipse), the pixel's edges relative to the centre, all mpf."""
    lo, hi = max(x0, -g.xe), min(x1, g.xe)
    if not lo < hi:
        return mp.mpf(0)
    pts = {lo, hi}
    for Y in (y0, y1):
        disc = (g.B * Y) ** 2 - g.A * (g.C * Y * Y - 1)
        s = mp.sqrt(disc) if disc > 0 else 0
        # (the abscissa between the two roots as well: where the edge is tangent to the ellipse, or within rounding of
        # it, the curve touches Y there and nowhere else, and no interval may have that point as the midpoint that
        # decides which of curve and edge bounds it)
        for r in ((-g.B * Y - s) / g.A, -g.B * Y / g.A, (-g.B * Y + s) / g.A):
            if lo < r < hi:
                pts.add(r)
    pts = sorted(pts)

    def S(x):
        X = min(max(x / g.xe, -1), 1)
        return (X * mp.sqrt(1 - X * X) + mp.asin(X)) / 2

    curve = [g.ab * S(x) for x in pts]
    line = [-g.B * x * x / (2 * g.C) for x in pts]
    area = mp.mpf(0)
    for i in range(len(pts) - 1):
        p, r = pts[i], pts[i + 1]
        m = (p + r) / 2
        root = mp.sqrt(max(g.C - m * m / (g.ab * g.ab), 0))
        yp, ym = (-g.B * m + root) / g.C, (-g.B * m - root) / g.C
        if min(yp, y1) <= max(ym, y0):
            continue
        dl, dc = line[i + 1] - line[i], curve[i + 1] - curve[i]
        area += (dl + dc) if yp < y1 else y1 * (r - p)
        area -= (dl - dc) if ym > y0 else y0 * (r - p)
    return area


@functools.lru_cache(maxsize=None)
def ellipse_weights(n, xc, yc, a, b, theta=0.0):
    """(w, lo, surely0, surely1) on an n x n grid: the exact pixel INTERSECT ellipse area is w + lo (w the nearest
    float64, lo the rest, so that (got - w) - lo is a kernel's error without the reference's own rounding); surely0 /
    surely1: pixels farther than MARGIN_PX outside / inside the boundary.  Cached per geometry; treat as read-only."""
    mp = require_mpmath()
    w = np.zeros((n, n))
    lo = np.zeros((n, n))
    sure0 = np.ones((n, n), dtype=bool)
    sure1 = np.zeros((n, n), dtype=bool)
    gf = _Conic(a, b, theta, float, math.cos, math.sin, math.sqrt)
    jx0, jx1 = max(int(math.floor(xc - gf.xe)) - 2, 0), min(int(math.ceil(xc + gf.xe)) + 3, n)
    jy0, jy1 = max(int(math.floor(yc - gf.ye)) - 2, 0), min(int(math.ceil(yc + gf.ye)) + 3, n)
    if jx0 >= jx1 or jy0 >= jy1:
        return w, lo, sure0, sure1
    kx, ky = np.arange(jx0, jx1, dtype=np.float64)[None, :], np.arange(jy0, jy1, dtype=np.float64)[:, None]
    x0, x1, y0, y1 = (kx - 0.5) - xc, (kx + 0.5) - xc, (ky - 0.5) - yc, (ky + 0.5) - yc
    qmax = np.maximum(np.maximum(gf.q(x0, y0), gf.q(x1, y0)), np.maximum(gf.q(x1, y1), gf.q(x0, y1)))
    qmin = _qmin(gf, x0 + 0 * y0, x1 + 0 * y0, y0 + 0 * x0, y1 + 0 * x0, np.clip, np.minimum, np.where)
    inside, outside = qmax < 1.0 - 1e-6, qmin > 1.0 + 1e-6
    sub_w, sub_lo = np.where(inside, 1.0, 0.0), np.zeros(inside.shape)
    sub0, sub1 = outside.copy(), inside.copy()
    with mp.workdps(DPS):
        g = _Conic(a, b, theta, mp.mpf, mp.cos, mp.sin, mp.sqrt)
        far = mp.mpf(MARGIN_PX) / min(g.a, g.b)  # sqrt(q) is Lipschitz with 1 / min(a, b) in pixels
        q_in, q_out = (1 - far) ** 2, (1 + far) ** 2
        cxm, cym = mp.mpf(xc), mp.mpf(yc)

        def clamp(v, l, h):
            return min(max(v, l), h)

        for r, c in zip(*np.nonzero(~inside & ~outside)):
            px, py = mp.mpf(int(jx0 + c)), mp.mpf(int(jy0 + r))
            e = ((px - 0.5) - cxm, (px + 0.5) - cxm, (py - 0.5) - cym, (py + 0.5) - cym)
            area = _strip_area(mp, g, *e)
            sub_w[r, c] = float(area)
            sub_lo[r, c] = float(area - mp.mpf(sub_w[r, c]))
            holds = e[0] <= 0 <= e[1] and e[2] <= 0 <= e[3]
            sub1[r, c] = max(g.q(e[0], e[2]), g.q(e[1], e[2]), g.q(e[1], e[3]), g.q(e[0], e[3])) <= q_in
            sub0[r, c] = (not holds) and _qmin(g, *e, clamp, min, lambda cond, x, y: y) >= q_out
            if sub1[r, c]:
                sub_w[r, c], sub_lo[r, c] = 1.0, 0.0
            if sub0[r, c]:
                sub_w[r, c], sub_lo[r, c] = 0.0, 0.0
    w[jy0:jy1, jx0:jx1], lo[jy0:jy1, jx0:jx1] = sub_w, sub_lo
    sure0[jy0:jy1, jx0:jx1], sure1[jy0:jy1, jx0:jx1] = sub0, sub1
    for arr in (w, lo, sure0, sure1):
        arr.setflags(write=False)
    return w, lo, sure0, sure1


def ellipse_errors(got, n, xc, yc, a, b, theta=0.0):
    """|got - exact area| per pixel, in float64, free of the reference's own rounding to float64."""
    w, lo, _, _ = ellipse_weights(n, xc, yc, a, b, theta)
    return np.abs((np.asarray(got, dtype=np.float64) - w) - lo)


def partial_pixels(n, xc, yc, a, b, theta=0.0):
    """(rows, cols) of the pixels the reference evaluated in mpmath and found strictly between 0 and 1."""
    w = ellipse_weights(n, xc, yc, a, b, theta)[0]
    return np.nonzero((w > 0.0) & (w < 1.0))


def strip_area(xc, yc, a, b, theta, kx, ky):
    """The strip-integral area of pixel (kx, ky) alone, as an mpf (what ellipse_weights stores, unrounded)."""
    mp = require_mpmath()
    with mp.workdps(DPS):
        g = _Conic(a, b, theta, mp.mpf, mp.cos, mp.sin, mp.sqrt)
        cxm, cym, px, py = mp.mpf(xc), mp.mpf(yc), mp.mpf(int(kx)), mp.mpf(int(ky))
        return _strip_area(mp, g, (px - 0.5) - cxm, (px + 0.5) - cxm, (py - 0.5) - cym, (py + 0.5) - cym)


def quad_area(xc, yc, a, b, theta, kx, ky):
    """The same area by mpmath.quad of the strip integrand max(0, min(y+, y1) - max(y-, y0)) over the pixel's columns,
    split at the integrand's kinks (found here by solving for them, independently of _strip_area's antiderivatives)."""
    mp = require_mpmath()
    with mp.workdps(DPS):
        g = _Conic(a, b, theta, mp.mpf, mp.cos, mp.sin, mp.sqrt)
        cxm, cym, px, py = mp.mpf(xc), mp.mpf(yc), mp.mpf(int(kx)), mp.mpf(int(ky))
        x0, x1, y0, y1 = (px - 0.5) - cxm, (px + 0.5) - cxm, (py - 0.5) - cym, (py + 0.5) - cym
        lo, hi = max(x0, -g.xe), min(x1, g.xe)
        if not lo < hi:
            return mp.mpf(0)

        def height(x):
            root = mp.sqrt(max(g.C - x * x / (g.ab * g.ab), 0))
            return max(min((-g.B * x + root) / g.C, y1) - max((-g.B * x - root) / g.C, y0), 0)

        pts = [lo, hi]
        for Y in (y0, y1):
            disc = (g.B * Y) ** 2 - g.A * (g.C * Y * Y - 1)
            s = mp.sqrt(disc) if disc > 0 else 0
            pts += [r for r in ((-g.B * Y - s) / g.A, -g.B * Y / g.A, (-g.B * Y + s) / g.A) if lo < r < hi]
        with mp.workdps(DPS + 10):
            return mp.quad(height, sorted(pts))


# ---- rectangle -------------------------------------------------------------------------------------------------------
def _samples_1d(k, centre, subpixels):
    """[subpixels][len(k)]: x = (k - 0.5 - c) - 0.5 step, then x += step, the kernel's additions in the kernel's order."""
    step = 1.0 / subpixels
    x = ((k - 0.5) - centre) - 0.5 * step
    out = np.empty((subpixels, k.size))
    for s in range(subpixels):
        x = x + step
        out[s] = x
    return out


@functools.lru_cache(maxsize=None)
def rectangle_weights(n, xc, yc, w, h, theta=0.0, S=32):
    """(weights, margin): count / S^2 of the sub-samples with |x_rot| < w/2 and |y_rot| < h/2 (strict), and the smallest
    distance of any sample to an edge of the rectangle (inf at theta = 0, where the count involves no device function
    and is exact).  A tilted case is exact for a kernel whose sin / cos differ from the host's by a few ulps as long as
    ``margin`` stays far above |sample| ulp: tests assert margin >= 1e-9."""
    hw, hh = w / 2.0, h / 2.0
    k = np.arange(n, dtype=np.float64)
    xs, ys = _samples_1d(k, xc, S), _samples_1d(k, yc, S)
    if theta == 0.0:
        cx = np.sum(np.abs(xs) < hw, axis=0)
        cy = np.sum(np.abs(ys) < hh, axis=0)
        out = (cy[:, None] * cx[None, :]) / float(S * S)
        out.setflags(write=False)
        return out, math.inf
    ct, st = math.cos(theta), math.sin(theta)
    ext = math.hypot(hw, hh) + 2.0
    cols = np.nonzero(np.abs(k - xc) < ext)[0]
    rows = np.nonzero(np.abs(k - yc) < ext)[0]
    cnt = np.zeros((rows.size, cols.size), dtype=np.int64)
    margin = math.inf
    for i in range(S):
        x = xs[i][cols][None, :]
        for j in range(S):
            y = ys[j][rows][:, None]
            xt, yt = np.abs(y * st + x * ct), np.abs(y * ct - x * st)
            cnt += (xt < hw) & (yt < hh)
            dx, dy = np.abs(xt - hw), np.abs(yt - hh)
            near = np.where(yt < hh + 1e-6, dx, np.inf), np.where(xt < hw + 1e-6, dy, np.inf)
            margin = min(margin, float(near[0].min()), float(near[1].min()))
    out = np.zeros((n, n))
    if rows.size and cols.size:
        out[np.ix_(rows, cols)] = cnt / float(S * S)
    out.setflags(write=False)
    return out, margin


# ---- the geometries both test modules use ----------------------------------------------------------------------------
N_TABLE = 256
# (xc, yc, a, b) in pixels of an N_TABLE grid, theta = 0
ELLIPSES = {
    "centred n/8 circle": (128.0, 128.0, 32.0, 32.0),
    "half-integer centre": (127.5, 128.5, 40.7, 25.2),
    "extents on pixel boundaries": (128.0, 127.0, 30.5, 20.5),
    "pythagorean r=5": (127.5, 127.5, 5.0, 5.0),        # pixel corners ON the circle: `<= 1.0` decides
    "pythagorean r=25": (100.5, 90.5, 25.0, 25.0),
    "pythagorean r=65": (127.5, 128.5, 65.0, 65.0),
    "generic decentred": (120.3, 131.1, 40.7, 25.2),
    "straddles one edge": (30.2, 131.4, 40.7, 25.2),
    "straddles a corner": (3.0, 252.5, 9.0, 7.0),
    "centre on -0.5": (-0.5, 100.0, 4.0, 8.0),
    "box overlaps column 0 only": (-2.6, 120.0, 3.0, 3.0),
    "sub-pixel inside one pixel": (100.2, 99.7, 0.4, 0.3),
    "sub-pixel across a boundary": (100.5, 100.0, 0.45, 0.2),
    "sub-pixel on a corner": (100.5, 100.5, 0.3, 0.25),
    "below 1 px but wider than a pixel": (100.0, 100.0, 0.9, 0.6),
    "1100 x 40 flat": (128.3, 127.6, 1100.0, 40.0),
}
# the cases that also run as obscurations.  The render path returns the mask alone, so an obscuration never reaches (a): its weight
# is 1 - mask, formed on the host with the kernels' one rounding, and enters in (b), where weights are applied.
OBSCURED = ("generic decentred", "pythagorean r=25", "straddles one edge", "sub-pixel across a boundary")
# (xc, yc, a, b, theta)
TILTED = {
    "tilted 0.6": (120.3, 131.1, 40.7, 25.2, 0.6),
    "quarter turn on a half-integer centre": (127.5, 128.5, 40.0, 15.0, math.pi / 2),
    "tilted sub-pixel": (100.2, 99.7, 0.4, 0.3, 1.1),
}
# n, xc, yc, a, b: the sizes the project runs (CPU module; the last one is the GPU module's production case too)
PRODUCTION = {
    "128: 40.7 x 25.2": (128, 64.3, 63.1, 40.7, 25.2),
    "1200: 512 x 512 at 600.3 / 599.1": (1200, 600.3, 599.1, 512.0, 512.0),
    "1200: 512 x 512 at 600.5 / 600.5": (1200, 600.5, 600.5, 512.0, 512.0),
    "2400: 1100 x 40": (2400, 1200.3, 1199.1, 1100.0, 40.0),
    "400: 75 x 2": (400, 200.3, 199.1, 75.0, 2.0),
    "64: 0.4 x 0.3": (64, 32.2, 31.7, 0.4, 0.3),
    "4096: 512 x 512 centred": (4096, 2048.0, 2048.0, 512.0, 512.0),
}


def frugal_ellipses(n, axis):
    """(xc, yc, a, b, obscuration) for an aperture riding on a pass of the production kernels along ``axis`` (0: rows), chosen
    for the record consumer's index arithmetic (frugal_pass.h: frugal_slot): flat ellipses at the riding limit
    2 along sqrt(3 / across) + 8 <= 192 (tip lines with partial runs of ~150 pixels and no interior, p1 == p2), centres
    shifted along the line by 0, 0.5, 17.3, 31.9 and 63.5 so that the runs start at every alignment to the 64-lane and
    thread strides, an ellipse cut by the grid edge, and an obscuration."""
    h = n / 2.0
    along_first = [
        (h, h, 75.0, 2.0, 0.0),
        (h + 0.5, h + 17.3, 83.9, 2.5, 0.0),
        (h + 17.3, h + 0.5, 159.0, 9.0, 0.0),
        (h + 31.9, h - 63.5, 100.0, 30.0, 0.0),
        (h + 63.5, h + 31.9, 30.0, 30.0, 0.0),
        (10.3, h - 100.2, 75.0, 2.0, 0.0),          # cut by the grid edge at the start of its lines
        (n - 20.5, h + 100.0, 83.0, 2.5, 0.0),      # ... and at their end
        (h - 0.5, h + 1.0, 60.0, 20.0, 1.0),        # obscuration
    ]
    if axis == 0:
        return along_first
    return [(yc, xc, b, a, o) for xc, yc, a, b, o in along_first]
