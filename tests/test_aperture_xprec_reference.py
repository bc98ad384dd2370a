"""CPU checks of tests/aperture_xprec.py, the arbitrary-precision aperture weights the GPU tests of
tests/test_gpu_aperture_xprec.py measure against: the strip-integral reference against direct quadrature, the fp64
restatement of the reference's rule (oracle/aperture_np.py) against it at the sizes the project runs -- which is what sets
the constant of the bound --, and the rectangle restatement against both oracles.  oracle/aperture_alt.py, the "second
restatement" of tests/test_aperture_restatements.py, is measured here as well: it arbitrates small apertures only."""
import numpy as np
import pytest

import aperture_xprec as ax
from oracle.aperture_alt import ellipse_mask_alt, rectangle_mask_alt
from oracle.aperture_np import ellipse_mask, rectangle_mask
from test_aperture_restatements import RECTS


def setup_module():
    ax.require_mpmath()


def _table_cases():
    out = {k: (ax.N_TABLE, *v, 0.0) for k, v in ax.ELLIPSES.items()}
    out.update({k: (ax.N_TABLE, *v) for k, v in ax.TILTED.items()})
    return out


QUAD_CASES = {
    "40.7 x 25.2": (128, 64.3, 63.1, 40.7, 25.2, 0.0),
    "512 circle": (1200, 600.3, 599.1, 512.0, 512.0, 0.0),
    "75 x 2": (400, 200.3, 199.1, 75.0, 2.0, 0.0),
    "pythagorean": (ax.N_TABLE, *ax.ELLIPSES["pythagorean r=25"], 0.0),
    "sub-pixel inside one pixel": (64, 32.2, 31.7, 0.4, 0.3, 0.0),
    "sub-pixel across a boundary": (ax.N_TABLE, *ax.ELLIPSES["sub-pixel across a boundary"], 0.0),
    **{k: (ax.N_TABLE, *v) for k, v in ax.TILTED.items()},
}


@pytest.mark.parametrize("name", list(QUAD_CASES))
def test_reference_against_quadrature(name):
    """The closed-form strip integrals against mpmath.quad of the strip integrand on a seeded sample of partial pixels."""
    import mpmath

    case = QUAD_CASES[name]
    rows, cols = ax.partial_pixels(*case)
    assert rows.size > 0
    rng = np.random.default_rng(rows.size)
    pick = rng.choice(rows.size, min(16, rows.size), replace=False)
    worst = mpmath.mpf(0)
    for i in pick:
        worst = max(worst, abs(ax.strip_area(*case[1:], cols[i], rows[i]) - ax.quad_area(*case[1:], cols[i], rows[i])))
    print(f"{name}: {pick.size} partial pixels, strip integrals against quadrature {mpmath.nstr(worst, 3)}")
    assert worst < mpmath.mpf("1e-30"), mpmath.nstr(worst, 5)


def test_reference_area_is_the_ellipse():
    """sum of the weights = pi a b where the ellipse lies on the grid (the partial pixels' float64 roundings add up to
    ~sqrt(count) 1e-16, the mpmath values themselves are good to 1e-45)."""
    for case in (QUAD_CASES["40.7 x 25.2"], (ax.N_TABLE, *ax.TILTED["tilted 0.6"]), QUAD_CASES["sub-pixel inside one pixel"]):
        w, lo, _, _ = ax.ellipse_weights(*case)
        exact = np.pi * case[3] * case[4]
        got = float(np.sum(w.astype(np.longdouble)) + np.sum(lo.astype(np.longdouble)))
        assert abs(got - exact) <= 4e-16 * max(exact, 1.0), (case, got - exact)


def _frugal_cases():
    return {f"riding, axis {axis}, #{i}": (1024, xc, yc, a, b, 0.0)
            for axis in (0, 1) for i, (xc, yc, a, b, _) in enumerate(ax.frugal_ellipses(1024, axis))}


YARD_CASES = {**{k: (*v, 0.0) for k, v in ax.PRODUCTION.items()}, **_table_cases(), **_frugal_cases()}


@pytest.mark.parametrize("name", list(YARD_CASES))
def test_oracle_against_the_reference(name):
    """oracle/aperture_np.py (fp64, the Green's-theorem algorithm the kernels mirror) against the exact areas: this is the
    yardstick.  Its error, in units of 2^-53 max(a, b, 1), stays at or below aperture_xprec.YARDSTICK_WORST -- so that the
    bound, C_AP = the next power of two at or above twice that, leaves every case a factor two --, "surely 0" pixels are
    exactly 0 and "surely 1" pixels exactly 1."""
    n, xc, yc, a, b, th = YARD_CASES[name]
    got = ellipse_mask((n, n), xc, yc, a, b, th)
    assert got is not None
    w, _, sure0, sure1 = ax.ellipse_weights(n, xc, yc, a, b, th)
    err = float(ax.ellipse_errors(got, n, xc, yc, a, b, th).max())
    ratio = err / ax.yardstick_unit(a, b)
    print(f"yardstick {name}: {ratio:.3f} x 2^-53 max(a, b, 1)  ({int((~sure0 & ~sure1).sum())} boundary pixels)")
    assert np.all(got[sure0] == 0.0) and np.all(got[sure1] == 1.0)
    assert got.min() >= 0.0 and got.max() <= 1.0
    assert ratio <= ax.YARDSTICK_WORST, (name, ratio)
    assert ax.bound(a, b) >= 2.0 * err


def test_c_ap_follows_from_the_yardstick():
    worst2 = 2.0 * ax.YARDSTICK_WORST
    assert ax.C_AP == 2.0 ** np.ceil(np.log2(worst2))


def test_what_the_second_restatement_can_arbitrate():
    """oracle/aperture_alt.py's closed-form strip integrals in fp64 cancel like eps a b: fine at the a <= 12 of
    tests/test_aperture_restatements.py (2e-14 there), ~1e-12 at 40.7 x 25.2, and blind in the ninth digit at the 512-pixel
    entrance pupil of the headline configuration -- where the Green's-theorem restatement keeps its 1e-13.  The 512
    circle is measured on a 64 x 64 window over its rightmost boundary pixels (centre far off the grid): aperture_alt
    evaluates every pixel in plain Python, so the whole mask would take it minutes."""
    n, xc, yc, a, b = ax.PRODUCTION["128: 40.7 x 25.2"]
    e_alt = float(ax.ellipse_errors(ellipse_mask_alt((n, n), xc, yc, a, b, 0.0), n, xc, yc, a, b).max())
    e_np = float(ax.ellipse_errors(ellipse_mask((n, n), xc, yc, a, b, 0.0), n, xc, yc, a, b).max())
    print(f"40.7 x 25.2: aperture_np {e_np:.3g}, aperture_alt {e_alt:.3g}")
    assert e_np < 2e-14 and 1e-14 < e_alt < 1e-11
    n, xc, yc, a, b = 64, 32.3 - 512.0, 31.1, 512.0, 512.0
    e_alt = float(ax.ellipse_errors(ellipse_mask_alt((n, n), xc, yc, a, b, 0.0), n, xc, yc, a, b).max())
    e_np = float(ax.ellipse_errors(ellipse_mask((n, n), xc, yc, a, b, 0.0), n, xc, yc, a, b).max())
    print(f"512 circle, rightmost pixels: aperture_np {e_np:.3g}, aperture_alt {e_alt:.3g}")
    assert e_np < 4e-13 and e_alt > 1e-11


@pytest.mark.parametrize("n,xc,yc,w,h,th", RECTS)
def test_rectangle_restatement_equals_the_oracles(n, xc, yc, w, h, th):
    """rectangle_weights is the oracle's mask exactly on the RECTS table, and at theta = 0 the literal per-pixel loops of
    oracle/aperture_alt.py as well; tilted cases keep every sample 1e-9 px from an edge."""
    got, margin = ax.rectangle_weights(n, xc, yc, w, h, th, 32)
    assert np.array_equal(got, rectangle_mask((n, n), xc, yc, w, h, th, 32))
    if th == 0.0:
        assert margin == np.inf and np.array_equal(got, rectangle_mask_alt((n, n), xc, yc, w, h, th, 32))
    else:
        print(f"rectangle theta {th:.3g}: smallest sample-to-edge distance {margin:.3g}")
        assert margin >= 1e-9


@pytest.mark.parametrize("S", [1, 4])
def test_rectangle_restatement_other_subpixels(S):
    for n, xc, yc, w, h, th in RECTS[:5]:
        assert np.array_equal(ax.rectangle_weights(n, xc, yc, w, h, th, S)[0], rectangle_mask((n, n), xc, yc, w, h, th, S))
