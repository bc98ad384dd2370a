"""Zoomed PSF windows without the library (README.md, "Zoomed PSFs"; include/paos_hip.h, paos_zoom_*).

* ``phase_table``: the weights of one axis for a fractional centre, by the definition, in long double.
* ``weight_matrix``: the dense (M, N) weight matrix of one axis, long double rounded to double once.
* ``window``: the restatement, ``Wy @ u @ Wx.T`` on a fetched field.
* ``window_by_spectrum``: an independent evaluation -- the trigonometric polynomial built from ``np.fft.fft2(u)`` with
  the Nyquist term split evenly, evaluated at the window's sample positions.
* ``ZoomModelDevice``: the NumPy model of the device (tests/focus_np.py) with ``zoom_compute / zoom_fetch`` by their
  documented semantics, so the host logic of ``run_batch(psf_zoom=...)`` runs on a CPU.
"""
import numpy as np

from focus_np import FocusModelDevice
from paos_amd import _lib

LD = np.longdouble
PI = LD("3.141592653589793238462643383279502884")


def phase_table(n, s, frac):
    """(w[s][n] long double, carry[s]): w[b][m mod n] for m in [-n/2, n/2) -- the layout of paos_zoom_weights."""
    w = np.zeros((s, n), dtype=LD)
    carry = np.zeros(s, dtype=np.int64)
    m = np.arange(-n // 2, n // 2)
    for b in range(s):
        phi = LD(frac) + LD(b) / LD(s)
        if phi >= 1:
            phi -= LD(1)
            carry[b] = 1
        if phi == 0:
            w[b, 0] = 1
            continue
        v = np.sin(PI * phi) / (LD(n) * np.tan(PI * (m.astype(LD) + phi) / LD(n)))
        w[b, m % n] = np.where(m % 2 == 1, -v, v)
    return w, carry


def weight_matrix(n, m, s, c):
    """W[q][j], the weight of grid pixel j in fine sample q of a window of m samples about pixel position c."""
    ci = int(np.floor(c))
    tab, carry = phase_table(n, s, c - ci)
    out = np.empty((m, n), dtype=np.float64)
    j = np.arange(n)
    for q in range(m):
        a, b = divmod(q - m // 2, s)
        a += int(carry[b])
        out[q] = tab[b, (ci + a - j) % n].astype(np.float64)
    return out


def window(u, m, s, cx=None, cy=None):
    """The complex window U = Wy u Wx^T of the definition (``|U|^2`` is ``psf_zoom``); ``u`` row-major [y][x]."""
    n = u.shape[0]
    wy = weight_matrix(n, m, s, n // 2 if cy is None else cy)
    wx = weight_matrix(n, m, s, n // 2 if cx is None else cx)
    u = np.asarray(u, dtype=np.complex128)
    re, im = np.ascontiguousarray(u.real), np.ascontiguousarray(u.imag)  # (strided views would miss the BLAS path)
    tr, ti = wy @ re, wy @ im
    return tr @ wx.T + 1j * (ti @ wx.T)


def psf(U):
    return U.real * U.real + U.imag * U.imag


def positions(n, m, s, c):
    """The sample positions of one axis, in pixels (long double)."""
    return LD(n // 2 if c is None else c) + (np.arange(m) - m // 2).astype(LD) / LD(s)


def window_by_spectrum(u, m, s, cx=None, cy=None):
    """(1 / N^2) sum S[ky][kx] e_ky(y) e_kx(x) with S = fft2(u), e_k(t) = exp(2 pi i k t / N) for signed k in
    (-N/2, N/2) and cos(pi t) for k = N/2."""
    n = u.shape[0]
    spec = np.fft.fft2(np.asarray(u, dtype=np.complex128))
    k = np.fft.fftfreq(n, 1.0 / n)  # signed integers; index n/2 is -n/2: the Nyquist term

    def basis(c):
        t = positions(n, m, s, c)
        arg = (2 * PI * t[:, None] * k[None, :].astype(LD) / LD(n))
        e = (np.cos(arg) + 1j * np.sin(arg)).astype(np.complex128)
        e[:, n // 2] = np.cos(PI * t).astype(np.float64)
        return e

    return basis(cy) @ spec @ basis(cx).T / (n * n)


class ZoomModelDevice(FocusModelDevice):
    """FocusModelDevice with the paos_zoom_* entry points by the restatement."""

    def zoom_compute(self, size, oversample, centres=None, field=False):
        ctr = None if centres is None else _lib.zoom_centres(centres, self.batch, self.n)
        _lib.zoom_check(size, oversample, self.n)
        self.log.append(("zoom_compute", (int(size), int(oversample), None if ctr is None else ctr.copy(), bool(field))))
        before = self.u.copy()
        self._zoom = [window(self.u[i], int(size), int(oversample), *(ctr[i] if ctr is not None else (None, None)))
                      for i in range(self.batch)]
        self._zoom_field = bool(field)
        assert np.array_equal(before, self.u, equal_nan=True)

    def zoom_fetch(self, item=0, what="psf"):
        if what not in ("psf", "field"):
            raise ValueError(what)
        if getattr(self, "_zoom", None) is None:
            raise _lib.PaosHipError("paos_zoom_fetch failed (1): no window computed")
        if what == "field":
            if not self._zoom_field:
                raise _lib.PaosHipError("paos_zoom_fetch failed (1): the complex window was not asked for")
            return self._zoom[item].copy()
        return psf(self._zoom[item])
