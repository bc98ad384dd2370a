"""NumPy restatement of placed detector images (README.md, "Detector images"; include/paos_hip.h,
paos_detector_*_placed) and a model device that has a detector.  TEST INFRASTRUCTURE ONLY.

An item whose grid centre lies at (x0, y0) in the image plane is rebinned as an item at the origin on a detector whose
centre is moved by (-x0, -y0): grid column j spans [x0 + (j - N/2 - 1/2) dx, x0 + (j - N/2 + 1/2) dx], so its overlap
with detector column m is the overlap of [(j - N/2 - 1/2) dx, (j - N/2 + 1/2) dx] with the detector column moved by
-x0.  The moved centre is formed once, ``xc - x0`` (one rounding), and then used as ``tests/detector_np.py`` uses ``xc``;
zero offsets give that restatement bit for bit.
"""
import dataclasses

import numpy as np

import detector_np
from fakes import ModelDevice


def moved(det, x0, y0):
    """The detector as item (x0, y0) sees it: centre (xc - x0, yc - y0), rounded once."""
    return dataclasses.replace(det, xc=float(np.float64(det.xc) - np.float64(x0)),
                               yc=float(np.float64(det.yc) - np.float64(y0)))


def rebin_placed(psf, det, dx, dy, x0, y0):
    """A[n, m] of an item whose grid centre lies at (x0, y0), (ny, nx) float64."""
    return detector_np.rebin(psf, moved(det, x0, y0), dx, dy)


def supersampled(psf, det, dx, dy, x0, y0, s):
    """Brute force: every grid pixel split into s x s equal parts, each put whole into the detector pixel that holds its
    centre.  Exact when every detector edge falls on a boundary of the parts (the tests choose such geometries)."""
    n = psf.shape[0]
    sub = (np.arange(n * s) + 0.5) / s  # part centres in grid-pixel units, column j spans [j, j + 1]
    x = x0 + (sub - 0.5 - n / 2) * dx
    y = y0 + (sub - 0.5 - n / 2) * dy
    mx = np.floor((x - det.xc) / det.pitch_x + det.nx / 2).astype(int)
    my = np.floor((y - det.yc) / det.pitch_y + det.ny / 2).astype(int)
    img = np.zeros((det.ny, det.nx))
    part = np.kron(np.asarray(psf, dtype=np.float64), np.ones((s, s))) / (s * s)
    okx, oky = (mx >= 0) & (mx < det.nx), (my >= 0) & (my < det.ny)
    for k in np.flatnonzero(oky):
        np.add.at(img[my[k]], mx[okx], part[k, okx])
    return img


class DetectorModelDevice(ModelDevice):
    """``fakes.ModelDevice`` with the detector calls of ``_lib.DeviceFields`` (restated in NumPy).  ``origins_seen``
    records the origins of every placed call."""

    def __init__(self, n, batch=1, precision="fp64", device=0):
        super().__init__(n, batch, precision, device)
        self.detector, self.image = None, None
        self.origins_seen = []

    def detector_begin(self, det):
        self.detector, self.image = det, np.zeros((det.ny, det.nx))

    def _images(self, dxs, dys, origins):
        o = np.zeros((self.batch, 2)) if origins is None else np.broadcast_to(np.asarray(origins, dtype=np.float64),
                                                                              (self.batch, 2))
        if origins is not None:
            self.origins_seen.append(np.array(o))
        dxs = np.broadcast_to(np.asarray(dxs, dtype=np.float64), (self.batch,))
        dys = np.broadcast_to(np.asarray(dys, dtype=np.float64), (self.batch,))
        return np.array([rebin_placed(self.psf_fetch(i), self.detector, dxs[i], dys[i], o[i, 0], o[i, 1])
                         for i in range(self.batch)])

    def detector_add(self, dxs, dys, weights, origins=None):
        self.image = detector_np.accumulate(self._images(dxs, dys, origins), weights, self.image)

    def detector_images(self, dxs, dys, origins=None):
        return self._images(dxs, dys, origins)

    def detector_fetch(self):
        return self.image.copy()
