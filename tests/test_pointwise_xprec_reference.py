"""CPU checks of tests/pointwise_xprec.py, the long-double yardstick of the Zernike, Gram and PSF-metric kernels: against
mpmath (the polynomials themselves), against the fp64 NumPy restatement of the reference (oracle/zernike_np.py, np.sum),
which must stay within the bounds with a factor 2 to spare, and against tests/fakes.py:ModelDevice, the NumPy model of
the kernels."""
import numpy as np
import pytest

import pointwise_xprec as px
from fakes import ModelDevice
from paos_amd.planner import gram_polynomials, jacobi_recurrence, zernike_block
from paos_amd.zernike import zernike_tables

mpmath = pytest.importorskip("mpmath")

ORDERINGS = ("ansi", "noll", "fringe", "standard")
OFFSETS = (0.0, 30.0, -90.0, 370.0)


def setup_module():
    px.require_long_double()


def _count(nmax, ordering):
    """Number of terms of an ordering whose radial orders reach nmax (fringe: whole squares)."""
    return (nmax // 2 + 1) ** 2 if ordering == "fringe" else (nmax + 1) * (nmax + 2) // 2


def _mp_term(mj, nj, normalize, rho, phi_mp):
    am, k = abs(mj), (nj - abs(mj)) // 2
    rad = (-1) ** k * mpmath.mpf(rho) ** am * mpmath.jacobi(k, am, 0, 1 - 2 * mpmath.mpf(rho) ** 2)
    az = 1 if mj == 0 else (mpmath.cos(am * phi_mp) if mj > 0 else mpmath.sin(am * phi_mp))
    nrm = (mpmath.sqrt(nj + 1) if mj == 0 else mpmath.sqrt(2 * (nj + 1))) if normalize else 1
    return nrm * rad * az


@pytest.mark.parametrize("ordering", ORDERINGS)
def test_zernike_terms_against_mpmath(ordering):
    """Single polynomials, n up to 40, at rho = 0, 1, 1 - 2^-52, small and random rho, both origins and four offsets:
    long double within (nmax + 1) 16 eps_ld of the polynomial's envelope (eps_ld ~ 1.1e-19)."""
    mpmath.mp.dps = 40
    nmax = 40
    count = _count(nmax, ordering)
    m, n, _ = zernike_tables(count, ordering, True)
    rng = np.random.default_rng(7)
    terms = np.unique(np.concatenate([np.arange(6), count - 1 - np.arange(6), rng.integers(0, count, 12)]))
    eps_ld = float(np.finfo(np.longdouble).eps)
    worst = 0.0
    npts = 0
    for origin in ("x", "y"):
        for off in OFFSETS:
            # (x, y) pairs with rho = rr / radius hitting the special values; radius 1
            rhos = np.array([0.0, 1.0, 1.0 - 2.0**-52, 1e-9, 1e-3, 0.25, 0.7071, 0.999])
            ang = rng.uniform(-np.pi, np.pi, rhos.size)
            xs, ys = rhos * np.cos(ang), rhos * np.sin(ang)
            xs[1], ys[1] = 1.0, 0.0  # exactly on the rim, on the x axis
            xs[2], ys[2] = 0.0, -(1.0 - 2.0**-52)
            rho = np.sqrt(xs * xs + ys * ys)
            a, b = (ys, xs) if origin == "x" else (xs, ys)
            phi = np.arctan2(a.astype(px.LD), b.astype(px.LD))
            vals, envs = px.zernike_terms(m[terms], n[terms], True, rho, phi, off)
            for p in range(rho.size):
                phi_mp = mpmath.atan2(mpmath.mpf(float(a[p])), mpmath.mpf(float(b[p]))) + mpmath.mpf(off) * mpmath.pi / 180
                npts += 1
                for t, j in enumerate(terms):
                    want = _mp_term(int(m[j]), int(n[j]), True, float(rho[p]), phi_mp)
                    v = vals[t][p]
                    hi = float(v)
                    err = abs(mpmath.mpf(hi) + mpmath.mpf(float(v - px.LD(hi))) - want)  # (long double exactly)
                    scale = max(float(envs[t][p]), 1e-300)
                    worst = max(worst, float(err) / scale)
    assert npts * terms.size >= 300
    # the argument m phi carries |m phi| eps_ld (|phi| < 8.5 rad with the 370 degree offset), the recurrence a few eps_ld
    # per step: (nmax + 1) 16 eps_ld ~ 7e-17 -- 250 times below the map bound at this order
    tol = (nmax + 1) * 16 * eps_ld
    assert worst <= tol, f"{ordering}: long-double Zernike term error {worst:.3g} x envelope (> {tol:.3g})"


def _map_case(nmax, ordering, normalize, npix, dx, dy, radius, seed=0):
    count = _count(nmax, ordering)
    m, n, norm = zernike_tables(count, ordering, normalize)
    rng = np.random.default_rng(seed + nmax)
    z = rng.standard_normal(count) * 1e-7 / np.sqrt(count)
    rows, cols = px.sample_pixels(npix, dx, dy, radius, extra=256, seed=seed)
    return m, n, norm, z, rows, cols


@pytest.mark.parametrize("nmax,ordering", [(8, "ansi"), (9, "noll"), (20, "fringe"), (40, "standard")])
def test_numpy_restatement_and_model_within_map_bound(nmax, ordering):
    """The fp64 oracle (scipy's Jacobi polynomials, cos(m phi)) stays below half of bound_map, and the NumPy model of the
    kernel (fakes.ModelDevice.zernike: the same recurrences) within it -- offsets, origin y and an anamorphic grid
    included; the mask is the same decision bit for bit."""
    npix, dx, dy, radius = 256, 1e-3, 1.3e-3, 0.11
    m, n, norm, z, rows, cols = _map_case(nmax, ordering, True, npix, dx, dy, radius)
    nm = int(n.max())
    for off in OFFSETS:
        for origin in ("x", "y"):
            ref, scale, masked = px.zernike_map(z, m, n, True, rows, cols, npix, dx, dy, radius, off, origin)
            b = float(px.C_MAP * (nm + 1) * px.U64)
            yard, same = px.map_errors(px.zernike_map_np(z, m, n, True, rows, cols, npix, dx, dy, radius, off, origin),
                                       ref, scale, masked)
            assert same, "oracle mask differs"
            dev = ModelDevice(npix, 1)
            dev.fill(1.0)
            blk, nmx, kdim = zernike_block(m, n, norm, z, dx, dy, radius, 1e-6, origin=origin, offset_deg=off)
            wfe = dev.zernike(nmx, kdim, jacobi_recurrence(nmx), [blk], want_wfe=True)
            got, same = px.map_errors(wfe[rows, cols], ref, scale, masked)
            msg = (f"nmax {nm} {ordering} offset {off} origin {origin}: model {got:.3g}, NumPy fp64 {yard:.3g}, "
                   f"bound {b:.3g} (x E(p))")
            assert same, "model mask differs -- " + msg
            assert b >= 2 * yard, "bound tighter than twice the yardstick -- " + msg
            assert got <= b, msg


@pytest.mark.parametrize("pupil", [False, True])
def test_gram_sums_numpy_and_model_within_bound(pupil):
    """Gram sums at 128^2, K = 21 (n <= 5), origin y and an offset, with and without a pupil: the fp64 restatement
    below half of bound_gram, the model within it, and the pixel count exact."""
    npix, dx, dy, radius, off = 128, 1e-3, 0.9e-3, 0.05, 30.0
    m, n, norm = zernike_tables(21, "ansi", True)
    nm = int(n.max())
    pw = None
    if pupil:
        yy, xx = np.mgrid[0:npix, 0:npix]
        pw = (((xx - 60.3) / 40.0) ** 2 + ((yy - 66.1) / 30.0) ** 2 <= 1.0).astype(np.float64)
    ref, absum, count = px.gram_sums(m, n, True, npix, dx, dy, radius, off, "y", pupil=pw)
    b = px.bound_gram(nm, absum, count)
    yard = px.gram_sums_np(m, n, True, npix, dx, dy, radius, off, "y", pupil=pw)
    dev = ModelDevice(npix, 1)
    blk, nmx, kdim = zernike_block(m, n, norm, np.zeros(len(m)), dx, dy, radius, 1e-6, origin="y", offset_deg=off)
    if pupil:
        dev.pupil_upload(0, pw)
    sums, counts = dev.zernike_gram(nmx, kdim, jacobi_recurrence(nmx), [blk], gram_polynomials(m, n, norm), pupil=pupil)
    ey = np.abs(yard.astype(px.LD) - ref).astype(np.float64)
    em = np.abs(sums[0].astype(px.LD) - ref).astype(np.float64)
    msg = f"model {np.max(em / b):.3g}, NumPy {np.max(ey / b):.3g} of the bound"
    assert counts[0] == count
    assert np.all(b >= 2 * ey), "bound tighter than twice the yardstick -- " + msg
    assert np.all(em <= b), msg


def test_psf_metrics_numpy_and_model_within_bound():
    """PSF metrics at 512^2, a fractional non-symmetric centre, radii equal to some pixel's distance: np.sum below half
    of bound_metric, the model within it; the peak exact."""
    npix = 512
    rng = np.random.default_rng(3)
    yy, xx = np.mgrid[0:npix, 0:npix]
    u = np.exp(-((xx - 200.3) ** 2 + (yy - 301.7) ** 2) / 900.0) * (1 + 0.1 * rng.standard_normal((npix, npix))) + 0j
    centre = (203.25, 297.625)
    radii = [0.0, 1.0, np.hypot(3 - 0.25, 5 + 0.375), 10.5, 40.0, 150.0, 700.0]
    ref, scales = px.psf_metrics(u, radii, centre)
    b = px.bound_metric(npix * npix, scales)
    yard = px.psf_metrics_np(u, radii, centre)
    dev = ModelDevice(npix, 1)
    dev.upload(0, u)
    got = dev.psf_metrics(radii, centre)[0]
    mod = np.array([got["power"], got["centroid"][0] * got["power"], got["centroid"][1] * got["power"], got["peak"],
                    *got["encircled"]])
    ey = np.abs(yard.astype(px.LD) - ref).astype(np.float64)
    em = np.abs(mod.astype(px.LD) - ref).astype(np.float64)
    assert yard[3] == ref[3] and mod[3] == ref[3]
    keep = np.arange(ref.size) != 3
    assert np.all(b[keep] >= 2 * ey[keep]), f"bound tighter than twice the yardstick: {ey} vs {b}"
    # (the model's centroid is a quotient, multiplied back: one more rounding each way)
    assert np.all(em[keep] <= b[keep] + 4 * px.U64 * np.abs(mod[keep])), f"model {em} vs bound {b}"
