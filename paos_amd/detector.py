"""Broadband PSFs on a detector pixel grid, integrated on the GPU.

The reference's user guide puts multi-wavelength runs first (docs/source/user/montecarlo/index.rst, "Multi-wavelength
simulations"); the product of such a run is one image on the instrument's pixels.  Each wavelength's PSF comes out on
its own sampling (``dx`` and ``dy`` at the image plane scale with the wavelength), so the PSFs are rebinned onto a common
detector grid before they are added.  The rebinning runs on the device, from the PSFs the walk keeps in HBM
(``keep_psf``), into an accumulator that stays there across the batches of a sweep (include/paos_hip.h,
``paos_detector_*``).

Definition (README.md, "Detector images"):

* Grid column ``j`` of item ``i`` spans ``[(j - N/2 - 1/2) dx_i, (j - N/2 + 1/2) dx_i]`` (the pixel-centre convention of
  wfo.py:236-237 and run.py:443); row ``k`` likewise with ``dy_i``.
* Detector column ``m`` spans ``[xc + (m - nx/2) pitch_x, xc + (m + 1 - nx/2) pitch_x]``; row ``n`` likewise with ``yc``
  and ``pitch_y``.  Images are ``(ny, nx)`` float64 arrays, rows along ``y`` (as ``download`` and ``psf_fetch``).
* ``fx_i(j, m)`` is the length of the overlap of grid column ``j`` and detector column ``m`` divided by ``dx_i``;
  ``fy_i(k, n)`` likewise along ``y``.
* ``A_i[n, m] = sum_k sum_j PSF_i[k, j] fy_i(k, n) fx_i(j, m)``: exact, flux-conserving rebinning of a PSF that is
  constant within each grid pixel.  Energy outside the detector is dropped; detector area outside the grid receives
  nothing.
* The broadband image is updated once per item, in ascending item order, in fp64: ``image <- image + w_i A_i``.  No
  float atomics: splitting a sweep into batches differently changes no bit, provided the PSFs are bit-identical.
"""
import math
from dataclasses import dataclass
from numbers import Integral, Real

import numpy as np

MAX_PIXELS = 4096  # per axis (paos_detector_begin)


@dataclass(frozen=True)
class Detector:
    """A detector pixel grid in the image plane: ``ny`` rows and ``nx`` columns of ``pitch_x`` x ``pitch_y`` metres
    (``pitch_y`` defaults to ``pitch_x``), centred on ``(xc, yc)`` metres."""

    nx: int
    ny: int
    pitch_x: float
    pitch_y: float = None
    xc: float = 0.0
    yc: float = 0.0

    def __post_init__(self):
        for name in ("nx", "ny"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, Integral) or not 1 <= int(v) <= MAX_PIXELS:
                raise ValueError(f"{name} must be an integer in 1..{MAX_PIXELS}, got {v!r}")
            object.__setattr__(self, name, int(v))
        if self.pitch_y is None:
            object.__setattr__(self, "pitch_y", self.pitch_x)
        for name in ("pitch_x", "pitch_y", "xc", "yc"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, Real) or not math.isfinite(float(v)):
                raise ValueError(f"{name} must be a finite number, got {v!r}")
            object.__setattr__(self, name, float(v))
        if self.pitch_x <= 0.0 or self.pitch_y <= 0.0:
            raise ValueError("detector pitches must be positive")

    def geometry(self):
        """The parameter block of ``paos_detector_begin``: nx, ny, pitch_x, pitch_y, xc, yc."""
        return np.array([self.nx, self.ny, self.pitch_x, self.pitch_y, self.xc, self.yc], dtype=np.float64)


def run_broadband(pupil_diameter, wavelengths, weights, gridsize, zoom, field, opt_chains, detector, batch=32,
                  precision="fp64", device=0, detector_origin=None, psf_blur=None):
    """The broadband image of a wavelength sweep on ``detector``: ``sum_i w_i A_i`` over ``wavelengths[i]`` /
    ``weights[i]`` (``opt_chains``: one chain per wavelength, or one chain for all; their last surface must be saved).
    ``field``: one field point for all, or one per wavelength (the items are then (wavelength, field, weight) triples:
    a field-of-view study lists every wavelength once per field point).  ``detector_origin`` as for ``run_batch``: None,
    ``"chief_ray"``, or an (items, 2) array of grid-centre positions.  ``psf_blur`` (a :class:`paos_amd.PsfBlur`, per-item
    values one per wavelength) is passed on to ``run_batch``: every item's PSF is blurred before it is rebinned (README.md,
    "Blurred PSFs"; blocks with a blur are issued with ``sync=True``, as ``run_batch`` asks).

    The sweep is walked in blocks of ``batch`` on one device context, each block issued as ``bench.measure`` issues a
    step (``run_batch`` with ``outputs=()``, the lean walk, ``keep_psf``, no synchronisation) and followed by
    ``detector_add``.  A last block that is short is filled up with its last wavelength at weight 0, which adds exact
    zeros.  Returns ``{"image": (ny, nx) float64, "power": sum_i w_i P_i (P_i: sum |u|^2 at the last surface),
    "wavelengths", "weights"}``; the image crosses to the host once, at the end.  ``run_broadband_series`` is the same
    sweep with the time series of a moving line of sight beside the image."""
    return _broadband(pupil_diameter, wavelengths, weights, gridsize, zoom, field, opt_chains, detector, batch, precision, device,
                      detector_origin, psf_blur, None, None)


def run_broadband_series(pupil_diameter, wavelengths, weights, gridsize, zoom, field, opt_chains, detector, pointing,
                         pointing_weights=None, batch=32, precision="fp64", device=0, detector_origin=None, psf_blur=None):
    """``run_broadband`` with the broadband series of the sweep (README.md, "Broadband series"): every other argument, the
    block walk and ``"image"`` / ``"power"`` are ``run_broadband``'s, bit for bit.  ``pointing`` (a
    :class:`paos_amd.PointingSeries`; per-wavelength offsets (nw, T, 2) and origins (nw, 2) are sliced per block): every
    block's frames are added into a sum that stays on the device, ``S[t] += w[i][t] F_i[t]``, with ``pointing_weights``
    ((nw,) or (nw, T); None: the spectral ``weights``); the padded tail has weight 0 and is not read.  Blocks stay
    unsynchronised unless a blur forces it.  The result gains ``"series_flux"`` (T, A) -- the flux of ``S g`` inside the
    series' apertures, ``g`` its response --, ``"series_offsets"`` and, with ``frames=True``, ``"series_frames"``
    (T, ny, nx) = ``S g`` (the product formed with NumPy).  The series' detector is its own and need not be ``detector``.
    ``ValueError`` before a device context is made: a ``pointing`` that is not a ``PointingSeries``; per-item offsets or
    origins for another number of wavelengths; weights of a wrong shape or not finite; ``psf_blur`` with a ``pixel``
    aperture."""
    from .pointing import PointingSeries

    if not isinstance(pointing, PointingSeries):
        raise ValueError(f"pointing must be a paos_amd.PointingSeries, got {pointing!r}")
    return _broadband(pupil_diameter, wavelengths, weights, gridsize, zoom, field, opt_chains, detector, batch, precision, device,
                      detector_origin, psf_blur, pointing, pointing_weights)


def _broadband(pupil_diameter, wavelengths, weights, gridsize, zoom, field, opt_chains, detector, batch, precision, device,
               detector_origin, psf_blur, pointing, pointing_weights):
    """The sweep of ``run_broadband`` (``pointing`` None) and ``run_broadband_series``."""
    from . import _lib
    from .run import run_batch

    if not isinstance(detector, Detector):
        raise TypeError("detector must be a paos_amd.detector.Detector")
    wls = [float(w) for w in wavelengths]
    nw = len(wls)
    w = np.asarray(weights, dtype=np.float64).reshape(-1)
    if nw == 0 or w.size != nw:
        raise ValueError("one weight per wavelength is required (and at least one wavelength)")
    if not np.all(np.isfinite(w)):
        raise ValueError("weights must be finite")
    chains = [opt_chains] * nw if isinstance(opt_chains, dict) else list(opt_chains)
    if len(chains) != nw:
        raise ValueError("one chain per wavelength (or a single chain) is required")
    if int(batch) < 1:
        raise ValueError("batch must be >= 1")
    from .run import _fields_of

    fields = _fields_of(field, nw)
    origins = None
    if detector_origin is not None and not isinstance(detector_origin, str):
        origins = np.array(detector_origin, dtype=np.float64)
        if origins.shape != (nw, 2):
            raise ValueError(f"detector_origin must have shape ({nw}, 2), got {origins.shape}")
    if psf_blur is not None:
        from .blur import PsfBlur

        if not isinstance(psf_blur, PsfBlur):
            raise ValueError(f"psf_blur must be a paos_amd.PsfBlur, got {psf_blur!r}")
        psf_blur.check(nw)
    if pointing is not None:
        pointing.check(nw, int(gridsize))
        pw = pointing.weights_for(w if pointing_weights is None else pointing_weights, nw)
        if psf_blur is not None and psf_blur.pixel is not None:
            raise ValueError("psf_blur with a pixel aperture and a pointing series: the rebinning already integrates over the pixel")
    nb = min(int(batch), nw)
    dev = _lib.DeviceFields(int(gridsize), nb, precision, device)
    try:
        dev.detector_begin(detector)
        pending = []  # (the powers of a block's last surface, or their handle; that block's weights)
        power = 0.0

        def settle(entry):
            p, wb = entry
            p = p.fetch() if hasattr(p, "fetch") else p
            return sum(float(wb[i]) * float(p[i]) for i in range(len(wb)))

        for b0 in range(0, nw, nb):
            idx = list(range(b0, min(b0 + nb, nw)))
            pad = nb - len(idx)
            wl_blk = [wls[i] for i in idx] + [wls[idx[-1]]] * pad
            ch_blk = [chains[i] for i in idx] + [chains[idx[-1]]] * pad
            f_blk = field if isinstance(field, dict) else [fields[i] for i in idx] + [fields[idx[-1]]] * pad
            o_blk = detector_origin if origins is None else origins[idx + [idx[-1]] * pad]
            w_blk = np.concatenate([w[idx], np.zeros(pad)])
            blur = {} if psf_blur is None else {"psf_blur": psf_blur.take(idx + [idx[-1]] * pad)}
            if pointing is not None:
                blur["pointing"] = pointing.take(idx + [idx[-1]] * pad)
                blur["pointing_weights"] = np.concatenate([pw[idx], np.zeros((pad,) + pw.shape[1:])])
            res = run_batch(pupil_diameter, wl_blk, gridsize, zoom, f_blk, ch_blk, precision=precision, device=device,
                            outputs=(), dev=dev, sync=psf_blur is not None, keep_psf=True, detector=detector,
                            detector_weights=w_blk, detector_origin=o_blk, **blur)
            num = _last_num(ch_blk[0])
            handle = res[0][num].get("power_ticket")
            # every other reduction of the block is given back unread (as bench.measure does)
            others = {id(t._red): t for r in res for rec in r.values() for t in [rec.get("power_ticket")] if t is not None}
            for t in others.values():
                if handle is None or t._red is not handle._red:
                    t.release()
            pending.append((handle if handle is not None else [r[num]["power"] for r in res], w_blk))
            if len(pending) >= _lib.NORM_SLOTS // 2:  # a long sweep: keep the library's ticket ring from filling
                power += settle(pending.pop(0))
        image = dev.detector_fetch()
        for entry in pending:
            power += settle(entry)
        series = {}
        if pointing is not None:
            nframes = pointing.offsets.shape[-2]
            series["series_flux"] = (dev.series_sum_flux(pointing.apertures, pointing.response) if pointing.apertures
                                     else np.zeros((nframes, 0)))
            series["series_offsets"] = pointing.offsets.copy()
            if pointing.frames:
                frames = dev.series_sum_fetch()
                series["series_frames"] = frames if pointing.response is None else frames * pointing.response
    finally:
        dev.close()
    return {"image": image, "power": power, "wavelengths": np.asarray(wls), "weights": w.copy(), **series}


def _last_num(chain):
    return chain[list(chain.keys())[-1]]["num"]
