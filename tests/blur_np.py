"""Blurred PSFs without the library (README.md, "Blurred PSFs"; include/paos_hip.h, paos_blur_*).

* ``table_longdouble`` / ``table``: ``t[m] = exp(-2 pi^2 sigma^2 f_m^2) sinc(p f_m)``, ``f_m = m / (N d)``, evaluated in
  ``np.longdouble`` and rounded to double once -- what paos_blur_table computes.
* ``transfer``: ``T[ky][kx] = ty[min(ky, N - ky)] tx[min(kx, N - kx)]`` in unshifted indices, any dtype.
* ``blur``: the NumPy restatement ``P' = ifft2(T fft2(P))`` in fp64 (``precision="fp32"``: in complex64 with ``T``
  rounded to float32, what an fp32 context does).
* ``blur_longdouble``: the same definition by direct DFT matrices in long double (small N): the yardstick of ``blur``.
* ``blur_reference`` / ``blur_reference_lines``: ``P'`` in long double by ``np.fft`` on long doubles, whole or on
  sampled image rows and columns (the convolution along the other axis is a direct long-double contraction).
* ``errors`` / ``bound`` / ``check``: the measures and the gate of tests/test_gpu_blur.py.
* ``BlurModelDevice``: the OTF model device (tests/otf_np.py) with ``blur_apply`` by its documented semantics, so the
  host logic of ``run_batch(psf_blur=...)`` runs on a CPU.
Test infrastructure only.
"""
import numpy as np

import detector_np
import otf_np
import xprec_np as xp
from paos_amd import _lib

LDR = np.longdouble
LD = xp.LD
PI = np.arctan2(LDR(0), LDR(-1))  # pi in long double


def table_longdouble(n, d, sigma, pixel=0.0):
    """t[0 .. n/2] in long double, the operations of the definition in its order."""
    m = np.arange(n // 2 + 1, dtype=np.int64).astype(LDR)
    f = m / (LDR(n) * LDR(d))
    x = PI * (LDR(pixel) * f)
    safe = np.where(x == 0, LDR(1), x)
    sinc = np.where(x == 0, LDR(1), np.sin(safe) / safe)
    return np.exp(-2 * PI * PI * (LDR(sigma) * LDR(sigma)) * (f * f)) * sinc


def table(n, d, sigma, pixel=0.0):
    return table_longdouble(n, d, sigma, pixel).astype(np.float64)


def fold(n):
    """min(k, N - k) for k < N: the table entry of an unshifted frequency index."""
    k = np.arange(n)
    return np.minimum(k, n - k)


def transfer(tx, ty, dtype=np.float64):
    """T[ky][kx] from the two tables (N/2 + 1 values each), the product formed in ``dtype``."""
    n = 2 * (len(tx) - 1)
    idx = fold(n)
    return np.asarray(ty, dtype=dtype)[idx][:, None] * np.asarray(tx, dtype=dtype)[idx][None, :]


def tables_of(n, dx, dy, sigma_x, sigma_y, pixel_x=0.0, pixel_y=0.0):
    return table(n, dx, sigma_x, pixel_x), table(n, dy, sigma_y, pixel_y)


def blur(psf, tx, ty, precision="fp64"):
    """The restatement: ifft2(T fft2(P)) by np.fft's real-input pair (rfft2 / irfft2 on the half spectrum), float64 out.
    fp32: PSF and T rounded to float32, complex64 transforms."""
    p = np.asarray(psf, dtype=np.float64)
    n = p.shape[0]
    t = transfer(tx, ty)[:, : n // 2 + 1]  # g = fl64(tx ty); P is real: the half spectrum (rfft2) carries everything
    if precision == "fp32":
        s = np.fft.rfft2(p.astype(np.float32))
        assert s.dtype == np.complex64
        out = np.fft.irfft2(s * t.astype(np.float32), s=p.shape)
        assert out.dtype == np.float32
        return out.astype(np.float64)
    return np.fft.irfft2(np.fft.rfft2(p) * t, s=p.shape)


def _dft_longdouble(n, sign):
    k = np.arange(n, dtype=np.int64)
    a = 2 * PI * np.mod(np.outer(k, k), n).astype(LDR) / LDR(n)
    return np.cos(a) + sign * 1j * np.sin(a)


def blur_longdouble(psf, tx, ty):
    """The definition by direct DFT matrices in long double: W* (T . (W P W^T)) W*^T / N^2 (small N)."""
    xp.require_long_double()
    p = np.asarray(psf, dtype=np.float64).astype(LD)
    n = p.shape[0]
    w, wi = _dft_longdouble(n, -1), _dft_longdouble(n, +1)
    s = (w @ p @ w.T) * transfer(tx, ty, LDR)
    return ((wi @ s @ wi.T) / (LDR(n) * LDR(n))).real


def blur_reference(psf, tx, ty):
    """P' in long double by np.fft on long doubles, (N, N) np.longdouble."""
    xp.require_long_double()
    s = np.fft.fft2(np.asarray(psf, dtype=np.float64).astype(LD))
    assert s.dtype == LD
    out = np.fft.ifft2(s * transfer(tx, ty, LDR))
    assert out.dtype == LD
    return out.real


def _kernel_rows(t, rows):
    """K[r][k] = kappa[(r - k) mod N] for the image lines ``rows``: the circular convolution kernel of one axis,
    kappa = ifft(t folded out to N values), real and even, in long double."""
    n = 2 * (len(t) - 1)
    kappa = np.fft.ifft(np.asarray(t, dtype=np.float64).astype(LD)[fold(n)])
    assert kappa.dtype == LD
    kappa = kappa.real
    return kappa[np.mod(np.asarray(rows)[:, None] - np.arange(n)[None, :], n)]


def blur_reference_lines(psf, tx, ty, idx, rows=True):
    """The image rows ``idx`` of ``blur_reference`` without the whole transform, shape (len(idx), N): the convolution
    along y as a direct long-double contraction onto those rows, the one along x by long-double transforms of them.
    ``rows=False``: the image COLUMNS ``idx`` by the same routine on P^T, returned as (N, len(idx))."""
    xp.require_long_double()
    p = np.asarray(psf, dtype=np.float64)
    if not rows:
        return blur_reference_lines(p.T, ty, tx, idx).T
    # (P^T K^T)^T: the long-double product walks P^T and the small K^T along their rows
    a = (np.ascontiguousarray(p.T).astype(LDR) @ np.ascontiguousarray(_kernel_rows(ty, idx).T)).T
    n = p.shape[0]
    out = np.fft.ifft(np.fft.fft(a.astype(LD), axis=1) * np.asarray(tx, dtype=np.float64).astype(LDR)[fold(n)][None, :], axis=1)
    assert out.dtype == LD
    return out.real


def sample_indices(n):
    """Image rows / columns of the sampled check: the first block of four, both sides of N/2 (the self-mirror column of
    the column launch and the first mirror written) and the last line."""
    return np.array(sorted({0, 1, 2, 3, n // 2 - 1, n // 2, n // 2 + 1, n - 1}), dtype=np.int64)


def errors(got, ref, norm, count):
    """(L2, element) errors of ``got`` against ``ref`` on the elements evaluated, relative to the WHOLE reference image:
    ``norm`` its L2 norm, ``count`` its number of elements.  L2: the rms error over the elements evaluated over the rms
    of the image (= ||got - ref|| / ||ref|| when all of it is evaluated; for sampled lines the share of the whole-image
    error that falls on them, scaled up).  Element: the largest error over ``norm`` -- the error of an element of a 2-D
    transform scales with the norm of the image, not with the content of its row."""
    d = np.abs(np.asarray(got).astype(LDR) - np.asarray(ref).astype(LDR))
    rms = np.sqrt(np.sum(d * d) / d.size)
    return float(rms / (LDR(norm) / np.sqrt(LDR(count)))), float(np.max(d) / LDR(norm))


def bound(n, precision):
    """Four line transforms and one factor per element: ``xprec_np.bound(n, 4, 1, precision)``."""
    return xp.bound(n, 4, 1, precision)


def check(got, ref, yard, norm, n, precision, what):
    """``xprec_np.check`` semantics with ``errors``: the kernel within the bound, the restatement within half of it."""
    b_l2, b_el = bound(n, precision)
    g_l2, g_el = errors(got, ref, norm, n * n)
    y_l2, y_el = errors(yard, ref, norm, n * n)
    msg = (f"{what}: kernel L2 {g_l2:.3g} / element {g_el:.3g}; NumPy {precision} restatement L2 {y_l2:.3g} / element "
           f"{y_el:.3g}; bound L2 {b_l2:.3g} / element {b_el:.3g}")
    assert b_l2 >= 2 * y_l2 and b_el >= 2 * y_el, "bound tighter than twice the restatement -- " + msg
    assert g_l2 <= b_l2 and g_el <= b_el, msg
    return msg


def gaussian(n, sigma_x, sigma_y, x0=None, y0=None):
    """A separable sampled Gaussian of unit peak about (x0, y0) (default: the grid centre), sigmas in pixels."""
    j = np.arange(n, dtype=np.float64)
    x0 = n / 2 if x0 is None else x0
    y0 = n / 2 if y0 is None else y0
    return np.exp(-((j - y0) ** 2) / (2.0 * sigma_y**2))[:, None] * np.exp(-((j - x0) ** 2) / (2.0 * sigma_x**2))[None, :]


class BlurModelDevice(otf_np.OtfModelDevice):
    """OtfModelDevice with paos_blur_apply by the restatement: the PSFs become P', the transfer functions those of P'
    (they stay valid), a second call compounds.  ``detector_add`` / ``detector_fetch`` by tests/detector_np.py."""

    def blur_apply(self, dxs, dys, sigma_x, sigma_y, pixel_x=0.0, pixel_y=0.0):
        self._otf_ready("paos_blur_apply")
        cols = [np.broadcast_to(np.asarray(c, dtype=np.float64), (self.batch,)) for c in (dxs, dys, sigma_x, sigma_y, pixel_x, pixel_y)]
        per_item = np.stack(cols, axis=1)
        if not np.all(np.isfinite(per_item)) or np.any(per_item[:, :2] <= 0.0) or np.any(per_item[:, 2:] < 0.0):
            raise _lib.PaosHipError("paos_blur_apply failed (1): a parameter paos_blur_table refuses")
        self.log.append(("blur_apply", None))
        psf = np.array(self.psf, dtype=np.float64)
        for i, (dx, dy, sx, sy, px, py) in enumerate(per_item):
            psf[i] = blur(psf[i], *tables_of(self.n, dx, dy, sx, sy, px, py))
        self.psf = psf
        self._otf = np.stack([otf_np.otf(p) for p in self.psf])

    def detector_add(self, dxs, dys, weights, origins=None):
        images = self.detector_images(dxs, dys, origins)
        self.image = detector_np.accumulate(images, np.asarray(weights, dtype=np.float64), self.image)

    def detector_fetch(self):
        return self.image.copy()
