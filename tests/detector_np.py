"""NumPy restatement of the detector definition (README.md, "Detector images"; include/paos_hip.h, paos_detector_*).

Written from the definition, with overlaps taken as clipped interval lengths.  Lengths are measured in grid pixels of
the item: grid column j spans [j, j + 1] there, which is the definition's [(j - N/2 - 1/2) dx, (j - N/2 + 1/2) dx]
divided by dx, and a detector edge at x metres sits at x / dx + N/2 + 1/2.  The overlap length in those units is the
definition's fraction fx(j, m) itself.  An edge is formed as ``(centre + (m - nd/2) pitch) / d + (N/2 + 1/2)``, one
rounding per operation; the device forms it the same way.
"""
import numpy as np


def edges(nd, pitch, centre, d, n):
    """Detector edges 0 .. nd in grid-pixel units of an item with pitch ``d`` on an ``n``-point grid."""
    t = np.arange(nd + 1, dtype=np.float64) - 0.5 * nd
    return (centre + t * pitch) / d + (0.5 * n + 0.5)


def fractions(nd, pitch, centre, d, n):
    """f[j, m]: the length of grid line j's overlap with detector line m, over d.  Shape (n, nd)."""
    e = edges(nd, pitch, centre, d, n)
    j = np.arange(n, dtype=np.float64)[:, None]
    return np.clip(np.minimum(j + 1.0, e[None, 1:]) - np.maximum(j, e[None, :-1]), 0.0, None)


def rebin(psf, det, dx, dy):
    """A[n, m] = sum_k sum_j psf[k, j] fy(k, n) fx(j, m), (ny, nx) float64."""
    n = psf.shape[0]
    fx = fractions(det.nx, det.pitch_x, det.xc, dx, n)
    fy = fractions(det.ny, det.pitch_y, det.yc, dy, n)
    cols = np.flatnonzero(fx.any(axis=1))
    rows = np.flatnonzero(fy.any(axis=1))
    if cols.size == 0 or rows.size == 0:
        return np.zeros((det.ny, det.nx))
    j0, j1, k0, k1 = cols[0], cols[-1] + 1, rows[0], rows[-1] + 1
    return fy[k0:k1].T @ (np.asarray(psf, dtype=np.float64)[k0:k1, j0:j1] @ fx[j0:j1])


def accumulate(images, weights, image=None):
    """image <- image + w_i A_i, item after item (one rounding per product and per sum)."""
    out = np.zeros_like(images[0]) if image is None else image.copy()
    for a, w in zip(images, weights):
        out = out + np.float64(w) * a
    return out
