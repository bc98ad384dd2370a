"""Pointing series: what ``run_batch(..., pointing=PointingSeries(...))`` asks for (README.md, "Pointing series")."""
import copy
from numbers import Integral

import numpy as np

MAX_FRAMES = 65536  # paos_series_compute
MAX_BOXES = 16


class PointingSeries:
    """The time series of a line of sight that moves over a detector: for every offset ``(ox_t, oy_t)`` (metres at the
    image plane; ``offsets`` of shape (T, 2) for every item alike, or (B, T, 2) per item) the last surface's kept PSF of
    each item is rebinned onto ``detector`` with its grid centre at ``origin + offset``, multiplied pixel by pixel by
    ``response`` ((ny, nx) gains; None: ones) and summed inside each of up to 16 ``apertures`` -- half-open boxes
    ``(m0, m1, n0, n1)`` of detector pixels, columns ``m0 .. m1-1`` and rows ``n0 .. n1-1``.  ``origin``: None (every grid
    centre at the image-plane origin), ``"chief_ray"`` or a (B, 2) array, as ``detector_origin`` of ``run_batch``.
    ``frames=True`` hands out the frames as well.  The series carries its own detector: the accumulator of
    ``detector_weights`` and the context's detector are left alone.
    """

    reads_psf = True

    def __init__(self, detector, offsets, apertures=(), response=None, origin=None, frames=False):
        from .detector import Detector

        if not isinstance(detector, Detector):
            raise ValueError(f"detector must be a paos_amd.Detector, got {detector!r}")
        try:
            offsets = np.array(offsets, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"offsets must be a (T, 2) or (B, T, 2) array of metres, got {offsets!r}") from None
        if offsets.ndim not in (2, 3) or offsets.shape[-1] != 2 or not 1 <= offsets.shape[-2] <= MAX_FRAMES or offsets.shape[0] < 1:
            raise ValueError(f"offsets must have shape (T, 2) or (B, T, 2) with 1 <= T <= {MAX_FRAMES}, got {offsets.shape}")
        if not np.all(np.isfinite(offsets)):
            raise ValueError("offsets must be finite")
        try:
            boxes = [tuple(box) for box in apertures]
        except TypeError:
            raise ValueError(f"apertures must be a sequence of (m0, m1, n0, n1) boxes, got {apertures!r}") from None
        if len(boxes) > MAX_BOXES:
            raise ValueError(f"at most {MAX_BOXES} apertures, got {len(boxes)}")
        for box in boxes:
            if len(box) != 4 or any(isinstance(v, bool) or not isinstance(v, Integral) for v in box):
                raise ValueError(f"an aperture is four integers (m0, m1, n0, n1), got {box!r}")
            m0, m1, n0, n1 = (int(v) for v in box)
            if not (0 <= m0 < m1 <= detector.nx and 0 <= n0 < n1 <= detector.ny):
                raise ValueError(f"aperture {box!r} must satisfy 0 <= m0 < m1 <= {detector.nx} and 0 <= n0 < n1 <= {detector.ny}")
        if response is not None:
            try:
                response = np.array(response, dtype=np.float64)
            except (TypeError, ValueError):
                raise ValueError(f"response must be a ({detector.ny}, {detector.nx}) array of pixel gains") from None
            if response.shape != (detector.ny, detector.nx):
                raise ValueError(f"response must have shape ({detector.ny}, {detector.nx}), got {response.shape}")
            if not np.all(np.isfinite(response)):
                raise ValueError("response must be finite")
        origins = None
        if origin is None or isinstance(origin, str):
            if origin not in (None, "chief_ray"):
                raise ValueError(f"origin must be None, 'chief_ray' or a (B, 2) array, got {origin!r}")
        else:
            try:
                origins = np.array(origin, dtype=np.float64)
            except (TypeError, ValueError):
                raise ValueError(f"origin must be None, 'chief_ray' or a (B, 2) array, got {origin!r}") from None
            if origins.ndim != 2 or origins.shape[1] != 2:
                raise ValueError(f"origin must be None, 'chief_ray' or a (B, 2) array, got shape {origins.shape}")
            if not np.all(np.isfinite(origins)):
                raise ValueError("origin must be finite")
        if not boxes and not frames:
            raise ValueError("no apertures and frames=False: nothing to compute")
        self.detector, self.offsets, self.response = detector, offsets, response
        self.apertures = [tuple(int(v) for v in box) for box in boxes]
        self.frames = bool(frames)
        # what run_batch resolves as it resolves detector_origin: ``chief`` -- the chief rays at the last surface, which the
        # walk fills into ``origins`` there
        self.origin, self.chief, self.origins = origin, isinstance(origin, str), origins

    def check(self, batch, n):
        """Everything that depends on the batch -- ``ValueError``, before anything is launched."""
        if self.offsets.ndim == 3 and self.offsets.shape[0] != batch:
            raise ValueError(f"per-item offsets must have shape ({batch}, T, 2), got {self.offsets.shape}")
        if not self.chief and self.origins is not None and self.origins.shape != (batch, 2):
            raise ValueError(f"origin must have shape ({batch}, 2), got {self.origins.shape}")

    def take(self, idx):
        """The series of the items ``idx`` of the batch this one was written for (a block of a longer sweep): per-item
        offsets and origins are sliced, everything else is shared."""
        pick = np.asarray(idx, dtype=np.int64)
        part = copy.copy(self)
        if self.offsets.ndim == 3:
            part.offsets = self.offsets[pick]
        if not self.chief and self.origins is not None:
            part.origins = self.origins[pick]
        return part

    def weights_for(self, weights, batch, what="pointing_weights"):
        """``weights`` of a broadband sum as a float64 array of shape (batch,) or (batch, T) -- ``ValueError`` otherwise."""
        try:
            w = np.array(weights, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"{what} must be an array of shape ({batch},) or ({batch}, T), got {weights!r}") from None
        nframes = self.offsets.shape[-2]
        if w.shape not in ((batch,), (batch, nframes)):
            raise ValueError(f"{what} must have shape ({batch},) or ({batch}, {nframes}), got {w.shape}")
        if not np.all(np.isfinite(w)):
            raise ValueError(f"{what} must be finite")
        return w

    def add_to_sum(self, dev, weights, dxs, dys):
        """Add every item's frames, weighted, into the broadband sum of ``dev`` (README.md, "Broadband series"), which is
        opened first when ``dev`` has none for this detector and number of frames.  Enqueues only; no record is touched."""
        self.check(dev.batch, dev.n)
        nframes = self.offsets.shape[-2]
        if getattr(dev, "series_sum", None) != (self.detector, nframes):
            dev.series_sum_begin(self.detector, nframes)
        dev.series_sum_add(dxs, dys, weights, self.offsets, origins=self.origins)

    def attach(self, dev, recs, dxs, dys):
        """``recs[i]`` gets item i's entries, from the PSFs ``dev`` keeps right now.  Synchronises (one copy of the fluxes,
        and of every frame with ``frames=True``)."""
        self.check(dev.batch, dev.n)
        frames = dev.series_compute(self.detector, dxs, dys, self.offsets, self.apertures, response=self.response,
                                    origins=self.origins, frames=self.frames)
        nframes = self.offsets.shape[-2]
        flux = dev.series_fetch() if self.apertures else np.zeros((dev.batch, nframes, 0))
        for i, rec in enumerate(recs):
            rec["series_flux"] = flux[i].copy()
            if self.frames:
                rec["series_frames"] = frames[i].copy()
            rec["series_offsets"] = (self.offsets[i] if self.offsets.ndim == 3 else self.offsets).copy()
