"""Pointing series without the library (README.md, "Pointing series"; include/paos_hip.h, paos_series_*).

* ``placed``: where the item's grid centre lies in a frame, ``fl(x0 + ox)``.
* ``frame_loop``: a frame in the very order of the definition -- per pixel, rows ``k`` ascending, within a row columns
  ``j`` ascending, ``r = r + P[k][j] fx`` and ``a = a + r fy``, every operation an IEEE double operation -- as a plain
  Python loop (the shapes of the tests are small).  ``frame_rebin``: the same frame by ``detector_placed_np.rebin_placed``
  (matrix products: another summation order, for the tolerance comparison).
* ``flux_tree``: the flux of a box in the lane-and-tree order; ``flux_longdouble``: the same sum in long double, with the
  number of pixels and ``sum |F'|`` (what the bound needs).
* ``SeriesModelDevice``: the detector and energy model devices with ``series_compute`` / ``series_fetch`` by their
  documented semantics, so that the host logic of ``run_batch(pointing=...)`` runs on a CPU.
Test infrastructure only.
"""
import math

import numpy as np

import detector_placed_np
import energy_np
from paos_amd import _lib

LDR = np.longdouble
LANES = 64


def placed(x0, ox):
    """fl(x0 + ox)"""
    return float(np.float64(x0) + np.float64(ox))


def _edge(m, nd, pitch, centre, d, n):
    t = float(m) - 0.5 * float(nd)
    pos = centre + t * pitch
    return pos / d + (0.5 * float(n) + 0.5)


def _lines(nd, pitch, centre, d, n):
    """per detector line: [(grid line, overlap fraction)] with a fraction > 0, grid lines ascending (det_edge, det_lo,
    det_hi of csrc/detector_pass.h written out)"""
    out = []
    for m in range(nd):
        e0, e1 = _edge(m, nd, pitch, centre, d, n), _edge(m + 1, nd, pitch, centre, d, n)
        lo = int(min(max(math.floor(e0), 0.0), float(n)))
        hi = int(min(max(math.ceil(e1), 0.0), float(n)))
        pairs = []
        for j in range(lo, hi):
            f = min(float(j + 1), e1) - max(float(j), e0)
            if f > 0.0:
                pairs.append((j, f))
        out.append(pairs)
    return out


def frame_loop(psf, det, dx, dy, gx, gy, response=None):
    """F[n][m] (F' with a response) of an item whose grid centre lies at (gx, gy), in the order of the definition."""
    p = np.asarray(psf, dtype=np.float64)
    n = p.shape[0]
    rows = p.tolist()
    xc = float(np.float64(det.xc) - np.float64(gx))
    yc = float(np.float64(det.yc) - np.float64(gy))
    cols = _lines(det.nx, det.pitch_x, xc, float(dx), n)
    lines = _lines(det.ny, det.pitch_y, yc, float(dy), n)
    out = np.zeros((det.ny, det.nx))
    for row, ks in enumerate(lines):
        for m, js in enumerate(cols):
            a = 0.0
            for k, fy in ks:
                line = rows[k]
                r = 0.0
                for j, fx in js:
                    r = r + line[j] * fx
                a = a + r * fy
            out[row, m] = a
    return out if response is None else out * np.asarray(response, dtype=np.float64)


def frame_rebin(psf, det, dx, dy, gx, gy):
    return detector_placed_np.rebin_placed(psf, det, dx, dy, gx, gy)


def flux_tree(frame, box):
    """Lane l adds the box's pixels q = l, l + 64, ... (row-major) in ascending order from +0.0; then the tree
    p[l] = p[l] + p[l + s], s = 32 .. 1; p[0]."""
    m0, m1, n0, n1 = box
    v = np.asarray(frame, dtype=np.float64)[n0:n1, m0:m1].reshape(-1)
    pad = (-v.size) % LANES
    v = np.concatenate([v, np.zeros(pad)]).reshape(-1, LANES)  # (a lane's sum is never -0.0: adding +0.0 changes nothing)
    p = np.zeros(LANES)
    for line in v:
        p = p + line
    s = LANES // 2
    while s >= 1:
        p[:s] = p[:s] + p[s:2 * s]
        s //= 2
    return float(p[0])


def flux_longdouble(frame, box):
    """(the sum in long double, the number of pixels, sum |F'|)"""
    m0, m1, n0, n1 = box
    v = np.asarray(frame, dtype=np.float64)[n0:n1, m0:m1].astype(LDR)
    return np.sum(v), v.size, float(np.sum(np.abs(v)))


def series(psfs, det, dxs, dys, offsets, boxes, response=None, origins=None, frame=frame_loop):
    """(frames (B, T, ny, nx), flux (B, T, A)) of a batch by the restatement."""
    nb = len(psfs)
    off = np.asarray(offsets, dtype=np.float64)
    org = np.zeros((nb, 2)) if origins is None else np.broadcast_to(np.asarray(origins, dtype=np.float64), (nb, 2))
    dxs = np.broadcast_to(np.asarray(dxs, dtype=np.float64), (nb,))
    dys = np.broadcast_to(np.asarray(dys, dtype=np.float64), (nb,))
    nt = off.shape[-2]
    frames = np.empty((nb, nt, det.ny, det.nx))
    flux = np.empty((nb, nt, len(boxes)))
    for i in range(nb):
        o = off[i] if off.ndim == 3 else off
        for t in range(nt):
            f = frame(psfs[i], det, dxs[i], dys[i], placed(org[i, 0], o[t, 0]), placed(org[i, 1], o[t, 1]))
            frames[i, t] = f if response is None else f * np.asarray(response, dtype=np.float64)
            for a, box in enumerate(boxes):
                flux[i, t, a] = flux_tree(frames[i, t], box)
    return frames, flux


class SeriesModelDevice(detector_placed_np.DetectorModelDevice, energy_np.EnergyModelDevice):
    """The detector model device (placed images; with the blur and energy calls of ``EnergyModelDevice``) with the
    paos_series_* entry points by the restatement.  ``series_seen`` records the origins of every series call."""

    def __init__(self, n, batch=1, precision="fp64", device=0):
        super().__init__(n, batch, precision, device)
        self.series_seen = []
        self._series = None

    def series_compute(self, det, dxs, dys, offsets, boxes=(), response=None, origins=None, frames=False):
        if not hasattr(self, "psf"):
            raise _lib.PaosHipError("paos_series_compute failed (1): no PSF kept (paos_psf_keep)")
        off = np.asarray(offsets, dtype=np.float64)
        boxes = [tuple(int(v) for v in b) for b in boxes]
        ok = off.ndim in (2, 3) and off.shape[-1] == 2 and 1 <= off.shape[-2] <= _lib.SERIES_MAX_FRAMES and np.all(np.isfinite(off))
        ok = ok and len(boxes) <= _lib.SERIES_MAX_BOXES and (boxes or frames)
        ok = ok and all(0 <= m0 < m1 <= det.nx and 0 <= n0 < n1 <= det.ny for m0, m1, n0, n1 in boxes)
        ok = ok and (response is None or bool(np.all(np.isfinite(response))))
        if not ok:
            raise _lib.PaosHipError("paos_series_compute failed (1): offsets, boxes or response")
        self.log.append(("series_compute", (off.shape[-2], len(boxes), bool(frames))))
        self.series_seen.append(None if origins is None else np.array(origins, dtype=np.float64))
        got, flux = series(np.asarray(self.psf, dtype=np.float64), det, dxs, dys, off, boxes, response, origins)
        self._series = flux if boxes else None
        return got if frames else None

    def series_fetch(self):
        if self._series is None:
            raise _lib.PaosHipError("paos_series_fetch failed (1): no series with boxes computed (paos_series_compute)")
        self.log.append(("series_fetch", None))
        return self._series.copy()
