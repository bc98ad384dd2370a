"""Transfer functions without the library (README.md, "Transfer functions"; include/paos_hip.h, paos_otf_*).

* ``otf`` / ``mtf`` / ``cuts`` / ``freqs``: the definition on a fetched PSF with plain ``np.fft`` and the shifts,
  ``fftshift(fft2(ifftshift(P)))`` over its zero-frequency value, zero frequency at pixel [N/2][N/2].
* ``otf_longdouble``: the defining double sum evaluated directly in long double (small N): the yardstick of ``otf``.
* ``phase_ramp``: the exact OTF of a single bright pixel.
* ``diffraction_mtf``: the analytic MTF of a clear circular pupil.
* ``OtfModelDevice``: the NumPy model of the device (tests/fakes.py, tests/focus_np.py) with ``otf_compute / otf_fetch /
  otf_cuts`` by their documented semantics, staleness included, so the host logic of ``run_batch(outputs=("mtf", ...),
  mtf_cuts=True)`` runs on a CPU.
Test infrastructure only.
"""
import numpy as np

from focus_np import FocusModelDevice
from paos_amd import _lib


def otf(psf):
    """OTF[ky][kx] of the definition, complex128 (N, N); zeros for a PSF whose sum is zero."""
    p = np.asarray(psf, dtype=np.float64)
    s = np.fft.fftshift(np.fft.fft2(np.fft.ifftshift(p)))
    n = p.shape[0]
    dc = s[n // 2, n // 2].real
    out = s * (1.0 / dc if dc != 0.0 else 0.0)
    out[n // 2, n // 2] = 1.0 if dc != 0.0 else 0.0  # by definition (dc times the rounded 1 / dc need not be 1)
    return out


def mtf(psf):
    return np.abs(otf(psf))


def cuts_of(full):
    """(along +fx, along +fy) of a centred (N, N) array: N/2 + 1 values from zero frequency to Nyquist.  Nyquist is pixel 0
    (the frequency -1/(2 d), which the point symmetry maps onto +1/(2 d))."""
    n = full.shape[0]
    h = n // 2
    return np.append(full[h, h:], full[h, 0]), np.append(full[h:, h], full[0, h])


def freqs(n, d):
    """The frequency axis of a cut, cycles per metre: m / (N d), m = 0 .. N/2."""
    return np.arange(n // 2 + 1, dtype=np.float64) / (n * d)


def _kernel_longdouble(n):
    """exp(-2 pi i (a - N/2)(b - N/2) / N) for a, b < N in long double; the integer product is reduced mod N exactly."""
    g = np.arange(n, dtype=np.int64) - n // 2
    m = np.mod(np.outer(g, g), n).astype(np.longdouble)
    two_pi = 2 * np.arctan2(np.longdouble(0), np.longdouble(-1))
    a = two_pi * m / np.longdouble(n)
    return np.cos(a) - 1j * np.sin(a)


def otf_longdouble(psf):
    """The defining double sum, S[ky][kx] = sum_k sum_j P[k][j] W[ky][k] W[kx][j], and its normalisation in long double."""
    if float(np.finfo(np.longdouble).eps) > 1e-18:
        raise AssertionError("np.longdouble is no wider than fp64 on this platform: no extended-precision reference")
    p = np.asarray(psf, dtype=np.longdouble)
    n = p.shape[0]
    w = _kernel_longdouble(n)
    s = w @ p.astype(np.clongdouble) @ w.T
    dc = s[n // 2, n // 2].real
    return s * (1 / dc if dc != 0 else np.longdouble(0))


def phase_ramp(n, k0, j0):
    """The OTF of a PSF that is one bright pixel at row k0, column j0: exp(-2 pi i ((j0 - N/2)(kx - N/2) + (k0 - N/2)(ky -
    N/2)) / N), with the integer phase reduced mod N before it is multiplied by 2 pi / N; correctly rounded complex128."""
    g = np.arange(n, dtype=np.int64) - n // 2
    m = np.mod((j0 - n // 2) * g[None, :] + (k0 - n // 2) * g[:, None], n).astype(np.longdouble)
    a = 2 * np.arctan2(np.longdouble(0), np.longdouble(-1)) * m / np.longdouble(n)
    return (np.cos(a) - 1j * np.sin(a)).astype(np.complex128)  # evaluated in long double, rounded once


def diffraction_mtf(f, wl, fratio):
    """(2 / pi)(acos s - s sqrt(1 - s^2)), s = f wl F#, zero beyond the cut-off s = 1."""
    s = np.asarray(f, dtype=np.float64) * wl * fratio
    sc = np.clip(s, 0.0, 1.0)
    return np.where(s < 1.0, (2.0 / np.pi) * (np.arccos(sc) - sc * np.sqrt(1.0 - sc * sc)), 0.0)


class OtfModelDevice(FocusModelDevice):
    """FocusModelDevice with the paos_otf_* entry points by the restatement.  Whatever stores PSFs makes a computed
    result stale, as in the library."""

    def psf_keep(self):
        super().psf_keep()
        self._otf_valid = False

    def run_passes(self, passes, blocks, live_rows=None, rows_stale=False, final_intensity=False, live_cols=None):
        ticket = super().run_passes(passes, blocks, live_rows=live_rows, rows_stale=rows_stale,
                                    final_intensity=final_intensity, live_cols=live_cols)
        if final_intensity and final_intensity != 2:
            self._otf_valid = False
        return ticket

    def otf_compute(self):
        if not hasattr(self, "psf"):
            raise _lib.PaosHipError("paos_otf_compute failed (1): no PSF kept (paos_psf_keep)")
        self.log.append(("otf_compute", None))
        self._otf = np.stack([otf(p) for p in self.psf])
        self._otf_valid = True

    def _otf_ready(self, who):
        if getattr(self, "_otf", None) is None:
            raise _lib.PaosHipError(f"{who} failed (1): no transfer functions computed (paos_otf_compute)")
        if not self._otf_valid:
            raise _lib.PaosHipError(f"{who} failed (1): the transfer functions are stale")

    def otf_fetch(self, item=0, what="mtf"):
        if what not in ("mtf", "otf"):
            raise ValueError(f"what must be 'mtf' or 'otf', got {what!r}")
        self._otf_ready("paos_otf_fetch")
        if not 0 <= int(item) < self.batch:
            raise _lib.PaosHipError("paos_otf_fetch failed (1): bad item")
        self.log.append(("otf_fetch", what))
        return np.abs(self._otf[item]) if what == "mtf" else self._otf[item].copy()

    def otf_cuts(self):
        self._otf_ready("paos_otf_cuts")
        self.log.append(("otf_cuts", None))
        return np.stack([np.stack(cuts_of(np.abs(o))) for o in self._otf])
