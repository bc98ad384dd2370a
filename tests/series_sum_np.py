"""Broadband series without the library (README.md, "Broadband series"; include/paos_hip.h, paos_series_sum_*).

* ``weights_bt``: weights of shape (B,) or (B, T) as (B, T).
* ``fold``: one add in the very order of the definition over frames that are given -- per frame, items ascending, an item
  whose weight is 0.0 skipped unread, ``a = a + fl(w F)``, every operation an IEEE double operation on whole frames (NumPy
  rounds a product and a sum of doubles once each).
* ``add``: ``fold`` over the frames of ``series_np.frame_loop`` (or of ``frame_rebin``, for the tolerance comparison); only
  the frames of items with a non-zero weight are formed.
* ``sum_longdouble``: ``sum_i w_i F_i`` in long double with ``sum_i |w_i F_i|`` per pixel (what the bound needs).
* ``SeriesSumModelDevice``: ``series_np.SeriesModelDevice`` with the four calls by their documented semantics, so that the
  host logic of ``run_batch(pointing_weights=...)`` and ``run_broadband_series(pointing=...)`` runs on a CPU.
Test infrastructure only.
"""
import numpy as np

import series_np as snp
from paos_amd import _lib

LDR = np.longdouble


def weights_bt(weights, nb, nt):
    w = np.asarray(weights, dtype=np.float64)
    return np.broadcast_to(w[:, None], (nb, nt)) if w.ndim == 1 else w


def fold(acc, frames, weights):
    """``acc`` (T, ny, nx) after one add of ``frames`` (B, T, ny, nx; ``frames[i]`` may be None where every weight of item
    i is 0) with ``weights`` (B,) or (B, T).  Returns a new array."""
    out = np.array(acc, dtype=np.float64)
    nb, nt = len(frames), out.shape[0]
    w = weights_bt(weights, nb, nt)
    for t in range(nt):
        a = out[t]
        for i in range(nb):
            if w[i, t] == 0.0:
                continue
            a = a + np.float64(w[i, t]) * frames[i][t]
        out[t] = a
    return out


def item_frames(psf, det, dx, dy, offsets, origin=(0.0, 0.0), frame=snp.frame_loop):
    """(T, ny, nx): the frames of one item without a response."""
    return np.array([frame(psf, det, dx, dy, snp.placed(origin[0], o[0]), snp.placed(origin[1], o[1])) for o in offsets])


def add(acc, psfs, det, dxs, dys, weights, offsets, origins=None, frame=snp.frame_loop):
    """``acc`` after one add of the batch ``psfs`` by the restatement."""
    nb = len(psfs)
    off = np.asarray(offsets, dtype=np.float64)
    nt = off.shape[-2]
    org = np.zeros((nb, 2)) if origins is None else np.broadcast_to(np.asarray(origins, dtype=np.float64), (nb, 2))
    dxs = np.broadcast_to(np.asarray(dxs, dtype=np.float64), (nb,))
    dys = np.broadcast_to(np.asarray(dys, dtype=np.float64), (nb,))
    w = weights_bt(weights, nb, nt)
    frames = [item_frames(psfs[i], det, dxs[i], dys[i], off[i] if off.ndim == 3 else off, org[i], frame) if np.any(w[i] != 0.0) else None
              for i in range(nb)]
    return fold(acc, frames, w)


def sum_longdouble(frames, weights):
    """(sum_i w_i F_i, sum_i |w_i F_i|) per pixel in long double, items with weight 0 left out; frames (B, T, ny, nx)."""
    nb, nt = len(frames), np.asarray(frames[0]).shape[0]
    w = weights_bt(weights, nb, nt)
    total = np.zeros(np.asarray(frames[0]).shape, dtype=LDR)
    sabs = np.zeros_like(total)
    for i in range(nb):
        for t in range(nt):
            if w[i, t] != 0.0:
                term = LDR(w[i, t]) * np.asarray(frames[i][t], dtype=LDR)
                total[t] += term
                sabs[t] += np.abs(term)
    return total, sabs


class SeriesSumModelDevice(snp.SeriesModelDevice):
    """The series model device with the paos_series_sum_* entry points by the restatement.  ``sum_seen`` records the
    origins of every add."""

    def __init__(self, n, batch=1, precision="fp64", device=0):
        super().__init__(n, batch, precision, device)
        self.series_sum, self._sum = None, None
        self.sum_seen = []

    def series_sum_begin(self, det, frames):
        frames = int(frames)
        if not 1 <= frames <= _lib.SERIES_MAX_FRAMES or frames * det.nx * det.ny > _lib.SERIES_SUM_MAX_DOUBLES:
            raise _lib.PaosHipError("paos_series_sum_begin failed (1): frames or the size rule")
        self.log.append(("series_sum_begin", (frames,)))
        self.series_sum, self._sum = (det, frames), np.zeros((frames, det.ny, det.nx))

    def _open(self, call):
        if self.series_sum is None:
            raise _lib.PaosHipError(f"{call} failed (1): no sum open (paos_series_sum_begin)")
        return self.series_sum

    def series_sum_add(self, dxs, dys, weights, offsets, origins=None):
        det, nframes = self._open("paos_series_sum_add")
        if not hasattr(self, "psf"):
            raise _lib.PaosHipError("paos_series_sum_add failed (1): no PSF kept (paos_psf_keep)")
        off = np.asarray(offsets, dtype=np.float64)
        w = np.asarray(weights, dtype=np.float64)
        if off.shape not in ((nframes, 2), (self.batch, nframes, 2)) or w.shape not in ((self.batch,), (self.batch, nframes)):
            raise ValueError("offsets or weights: shape")
        if not (np.all(np.isfinite(off)) and np.all(np.isfinite(w))):
            raise _lib.PaosHipError("paos_series_sum_add failed (1): offsets or weights")
        self.log.append(("series_sum_add", (nframes, w.ndim)))
        self.sum_seen.append(None if origins is None else np.array(origins, dtype=np.float64))
        self._sum = add(self._sum, np.asarray(self.psf, dtype=np.float64), det, dxs, dys, w, off, origins)

    def series_sum_flux(self, boxes, response=None):
        det, nframes = self._open("paos_series_sum_flux")
        boxes = [tuple(int(v) for v in b) for b in boxes]
        ok = 1 <= len(boxes) <= _lib.SERIES_MAX_BOXES and all(0 <= m0 < m1 <= det.nx and 0 <= n0 < n1 <= det.ny for m0, m1, n0, n1 in boxes)
        if not ok or (response is not None and not np.all(np.isfinite(response))):
            raise _lib.PaosHipError("paos_series_sum_flux failed (1): boxes or response")
        self.log.append(("series_sum_flux", None))
        seen = self._sum if response is None else self._sum * np.asarray(response, dtype=np.float64)
        return np.array([[snp.flux_tree(seen[t], box) for box in boxes] for t in range(nframes)]).reshape(nframes, len(boxes))

    def series_sum_fetch(self):
        self._open("paos_series_sum_fetch")
        self.log.append(("series_sum_fetch", None))
        return self._sum.copy()
