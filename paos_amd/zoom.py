"""Zoomed PSF windows: what ``run_batch(..., psf_zoom=PsfWindow(...))`` asks for (README.md, "Zoomed PSFs")."""
import math

import numpy as np

from . import _lib


class PsfWindow:
    """A ``size`` x ``size`` window of the last surface's field at ``1 / oversample`` of the grid pitch, interpolated
    exactly (the field is band-limited on its own grid) on the GPU.

    ``size``: a multiple of 16 in 16 .. 1024, at most ``oversample * gridsize``; ``oversample``: an integer in 1 .. 64.
    ``centre``: None -- the grid centre (pixel N/2, N/2); a (B, 2) array of pixel positions ``(x, y)`` in ``[0, N)``,
    fractional ones included; ``"centroid"`` -- per item (and per focus plane) the pixel nearest to the intensity
    centroid, the grid centre when the power is zero.  ``field``: also hand out the complex window (``'wfo_zoom'``).
    """

    reads_psf = False  # (``attach`` reads the field, not the kept PSFs: run._attach_products)

    def __init__(self, size, oversample, centre=None, field=False):
        _lib.zoom_check(size, oversample, 1 << 30)  # (the rule that needs the grid is checked by run_batch)
        if isinstance(centre, str):
            if centre != "centroid":
                raise ValueError(f"centre must be None, 'centroid' or a (B, 2) array, got {centre!r}")
        elif centre is not None:
            try:
                centre = np.array(centre, dtype=np.float64)
            except (TypeError, ValueError):
                raise ValueError("centre must be None, 'centroid' or a (B, 2) array of pixel positions (x, y)") from None
            if centre.ndim != 2 or centre.shape[1] != 2:
                raise ValueError(f"centre must have shape (B, 2), got {centre.shape}")
        self.size, self.oversample, self.centre, self.field = int(size), int(oversample), centre, bool(field)

    def check(self, batch, n):
        """Everything that depends on the batch and the grid -- ``ValueError``, before anything is launched."""
        _lib.zoom_check(self.size, self.oversample, n)
        if self.centre is not None and not isinstance(self.centre, str):
            _lib.zoom_centres(self.centre, batch, n)

    def attach(self, dev, recs, dxs, dys):
        """``recs[i]`` gets item i's window of the field ``dev`` holds right now.  Synchronises."""
        n, s = dev.n, self.oversample
        if self.centre is None:
            ctr = np.full((dev.batch, 2), float(n // 2))
        elif isinstance(self.centre, str):
            ctr = np.full((dev.batch, 2), float(n // 2))
            for i, met in enumerate(dev.psf_metrics(())):
                cxy = met["centroid"]
                if met["power"] > 0 and all(math.isfinite(v) for v in cxy):
                    ctr[i] = [float(math.floor(v + 0.5) % n) for v in cxy]
        else:
            ctr = _lib.zoom_centres(self.centre, dev.batch, n)
        dev.zoom_compute(self.size, s, None if self.centre is None else ctr, field=self.field)
        for i, rec in enumerate(recs):
            rec["psf_zoom"] = dev.zoom_fetch(i, "psf")
            if self.field:
                rec["wfo_zoom"] = dev.zoom_fetch(i, "field")
            rec["zoom_dx"], rec["zoom_dy"] = dxs[i] / s, dys[i] / s
            rec["zoom_centre"] = (float(ctr[i, 0]), float(ctr[i, 1]))
