"""Through-focus stacks without the library (README.md, "Through-focus stacks"; include/paos_hip.h, paos_focus_*).

* ``plane``: the definition on a fetched field, ``ifft2(exp(-i pi wl dz (fx^2 + fy^2)) fft2(u))`` with
  ``fx, fy = np.fft.fftfreq(N, dx), np.fft.fftfreq(N, dy)``.
* ``FocusModelDevice``: the NumPy model of the device (tests/fakes.py) with ``focus_begin / focus_plane / focus_end``
  by their documented semantics (and the detector entry points by tests/detector_np.py), so the host logic of
  ``run_batch(focus_planes=...)`` runs on a CPU.
* ``oracle_end_state``: the oracle's wavefront object as its propagation loop leaves it -- the field and the pilot-beam
  state (z, zw0, zr, C) behind everything the last surface does -- without touching anything under oracle/.
* ``refocused_chain``: the chain with its last surface given a thickness and one more saved surface appended.
"""
import copy

import numpy as np

import detector_np
from fakes import ModelDevice
from paos_amd import _lib
from paos_amd.abcd import ABCD


def plane(u, wl, dx, dy, dz):
    """u(dz) of the definition; ``u`` row-major [y][x] as ``download`` returns it."""
    n = u.shape[0]
    fx, fy = np.fft.fftfreq(n, d=dx), np.fft.fftfreq(n, d=dy)
    fxx, fyy = np.meshgrid(fx, fy)
    return np.fft.ifft2(np.exp(-1.0j * (np.pi * wl * dz) * (fxx**2 + fyy**2)) * np.fft.fft2(u, norm="ortho"), norm="ortho")


class FocusModelDevice(ModelDevice):
    """ModelDevice with the paos_focus_* entry points (and paos_detector_* by the restatement)."""

    def focus_begin(self):
        if getattr(self, "_spectrum", None) is not None:
            raise _lib.PaosHipError("paos_focus_begin failed (1): a focus stack is already open")
        self.log.append(("focus_begin", None))
        before = self.u.copy()
        self._spectrum = np.fft.fft2(self.u, axes=(1, 2), norm="ortho")
        assert np.array_equal(before, self.u, equal_nan=True)

    def focus_plane(self, blocks):
        if getattr(self, "_spectrum", None) is None:
            raise _lib.PaosHipError("paos_focus_plane failed (1): no focus stack is open")
        b = np.asarray(blocks, dtype=np.float64)
        assert b.shape == (self.batch, _lib.PHASE_STRIDE)
        if not np.all(np.isfinite(b)):
            raise _lib.PaosHipError("paos_focus_plane failed (1): non-finite parameter")
        self.log.append(("focus_plane", None))
        i = np.arange(self.n)
        g = np.where(i < self.n // 2, i, i - self.n).astype(np.float64)
        for k, (enable, sx, sy, coef, sgn) in enumerate(b):
            spec = self._spectrum[k]
            if enable:
                xx, yy = np.meshgrid(g * sx, g * sy)
                q = coef * (xx**2 + yy**2)
                spec = spec * (np.cos(q) + 1j * sgn * np.sin(q))
            self.u[k] = np.fft.ifft2(spec, norm="ortho")

    def focus_end(self):
        if getattr(self, "_spectrum", None) is None:
            raise _lib.PaosHipError("paos_focus_end failed (1): no focus stack is open")
        self.log.append(("focus_end", None))
        self._spectrum = None

    # -- detector (tests/detector_np.py; origins: the image-plane position of each item's grid centre) ------------------
    def detector_begin(self, det):
        self.detector = det
        self.image = np.zeros((det.ny, det.nx))

    def detector_images(self, dxs, dys, origins=None):
        if not hasattr(self, "psf"):
            raise _lib.PaosHipError("no PSF kept (paos_psf_keep)")
        dxs = np.broadcast_to(np.asarray(dxs, dtype=np.float64), (self.batch,))
        dys = np.broadcast_to(np.asarray(dys, dtype=np.float64), (self.batch,))
        assert origins is None
        return np.stack([detector_np.rebin(self.psf[i], self.detector, dxs[i], dys[i]) for i in range(self.batch)])


def oracle_end_state(pupil_diameter, wavelength, gridsize, zoom, field, opt_chain):
    """(saved records, the oracle's RefWFO behind the last surface) of ``oracle.run_np.run``."""
    from oracle import run_np

    made = []

    class Recording(run_np.RefWFO):
        def __init__(self, *args, **kwargs):
            super().__init__(*args, **kwargs)
            made.append(self)

    original = run_np.RefWFO
    run_np.RefWFO = Recording
    try:
        out = run_np.run(pupil_diameter, wavelength, gridsize, zoom, field, opt_chain, light=True)
    finally:
        run_np.RefWFO = original
    assert len(made) == 1
    return out, made[0]


def refocused_chain(opt_chain, dz):
    """The chain with its last surface's thickness replaced by ``dz`` and one more saved, inert surface appended.  The
    last surface must be one whose matrices do nothing else (no power, unit magnification, same medium)."""
    keys = list(opt_chain.keys())
    out = {k: opt_chain[k] for k in keys}
    last = copy.copy(opt_chain[keys[-1]])
    t = last["ABCDt"]
    assert t.power == 0 and t.M == 1.0 and last["ABCDs"].M == 1.0 and abs(t.n1n2) == 1.0 and t.thickness == 0.0
    last["ABCDt"], last["ABCDs"] = ABCD(thickness=dz), ABCD(thickness=dz)
    out[keys[-1]] = last
    num = max(int(opt_chain[k]["num"]) for k in keys) + 1
    key = num if isinstance(keys[-1], (int, np.integer)) else f"focus_{num}"
    out[key] = {"num": num, "type": "Standard", "name": "FOCUS", "is_stop": False, "save": True,
                "ABCDt": ABCD(), "ABCDs": ABCD()}
    return out, num
