"""Encircled energy without the library (README.md, "Encircled energy"; include/paos_hip.h, paos_ee_*).

* ``summary``: S, Sx, Sy in long double, the peak and its first position in row-major order, and the centre by the rule
  of the definition (the centroid from the long-double sums, rounded once).
* ``geometry`` / ``ring_indices``: membership exactly as defined -- ``x = j - cx``, ``y = (k - cy) a``, ``d2 = x x + y y``,
  ``r_b = (b + 1) D``, ``t_b = r_b r_b`` in fp64, each operation rounded once -- as the smallest ``b`` with
  ``d2 <= t_b`` (``fmax(|x|, |y|) <= r_b`` for the squares) of every pixel.
* ``curves``: the sums of the members in long double, with the number of members and ``sum |P|`` over them per radius
  (what the bound needs).  ``curves_brute``: the same by a loop over pixels and radii, for small N.
* ``ree``: the radii at the requested fractions.  ``bound``: the project's bound for metric sums.
* ``EnergyModelDevice``: the blur model device (tests/blur_np.py) with ``energy_compute`` / ``energy_fetch`` by their
  documented semantics, staleness included, so the host logic of ``run_batch(psf_energy=...)`` runs on a CPU.
Test infrastructure only.
"""
import numpy as np

import blur_np
import pointwise_xprec as px
from paos_amd import _lib

LDR = np.longdouble
GIVEN, CENTROID, PEAK = _lib.EE_GIVEN, _lib.EE_CENTROID, _lib.EE_PEAK


def summary(psf, mode=GIVEN, given=None):
    """dict(S, Sx, Sy as long doubles; peak, peak_col, peak_row; cx, cy, fallback) of one PSF."""
    p = np.asarray(psf, dtype=np.float64)
    n = p.shape[0]
    pl = p.astype(LDR)
    idx = np.arange(n, dtype=np.float64).astype(LDR)
    s, sx, sy = np.sum(pl), np.sum(np.sum(pl, axis=0) * idx), np.sum(np.sum(pl, axis=1) * idx)
    at = int(np.argmax(p))  # (the first occurrence in row-major order)
    out = dict(S=s, Sx=sx, Sy=sy, peak=float(p.reshape(-1)[at]), peak_col=at % n, peak_row=at // n, fallback=False)
    if mode == GIVEN:
        cx, cy = (n / 2, n / 2) if given is None else (float(given[0]), float(given[1]))
    elif mode == PEAK:
        cx, cy = float(out["peak_col"]), float(out["peak_row"])
    else:
        with np.errstate(divide="ignore", invalid="ignore"):
            cx, cy = float(sx / s), float(sy / s)
        if not s > 0 or not 0.0 <= cx < n or not 0.0 <= cy < n:
            cx, cy, out["fallback"] = n / 2, n / 2, True
    out["cx"], out["cy"] = cx, cy
    return out


def sum_scales(psf):
    """sum |P|, sum |P j|, sum |P k| (float): what the bounds of S, Sx, Sy are relative to."""
    a = np.abs(np.asarray(psf, dtype=np.float64)).astype(LDR)
    idx = np.arange(a.shape[0], dtype=np.float64).astype(LDR)
    return float(np.sum(a)), float(np.sum(np.sum(a, axis=0) * idx)), float(np.sum(np.sum(a, axis=1) * idx))


def radii(bins, delta):
    """(r_b, t_b) in fp64: r_b = (double)(b + 1) D, t_b = r_b r_b."""
    r = (np.arange(bins, dtype=np.float64) + 1.0) * np.float64(delta)
    return r, r * r


def geometry(n, cx, cy, aspect):
    """(d2, max(|x|, |y|)) of every pixel, (n, n) float64, each operation rounded once."""
    j = np.arange(n, dtype=np.float64)
    x = (j - np.float64(cx))[None, :]
    y = ((j - np.float64(cy)) * np.float64(aspect))[:, None]
    return x * x + y * y, np.maximum(np.abs(x), np.abs(y))


def ring_indices(n, cx, cy, delta, aspect, bins, square=False):
    """The smallest b with d2 <= t_b (square: with max(|x|, |y|) <= r_b) of every pixel, ``bins`` where there is none.
    (np.searchsorted(t, v, 'left') is the number of t_b < v: exactly these comparisons on the same doubles.)"""
    d2, m = geometry(n, cx, cy, aspect)
    r, t = radii(bins, delta)
    return np.searchsorted(r, m, side="left") if square else np.searchsorted(t, d2, side="left")


def curves(psf, cx, cy, delta, aspect, bins, square=False):
    """(ee as long doubles, members per radius, sum |P| over the members per radius): ring by ring pairwise sums in long
    double, then the running sum over the rings."""
    p = np.asarray(psf, dtype=np.float64)
    n = p.shape[0]
    idx = ring_indices(n, cx, cy, delta, aspect, bins, square).reshape(-1)
    order = np.argsort(idx, kind="stable")
    vals = p.reshape(-1)[order].astype(LDR)
    ends = np.searchsorted(idx[order], np.arange(bins), side="right")
    ee, sabs = np.zeros(bins, dtype=LDR), np.zeros(bins, dtype=LDR)
    lo, run, run_abs = 0, LDR(0), LDR(0)
    for b in range(bins):
        hi = int(ends[b])
        if hi > lo:
            run = run + np.sum(vals[lo:hi])
            run_abs = run_abs + np.sum(np.abs(vals[lo:hi]))
        ee[b], sabs[b], lo = run, run_abs, hi
    return ee, ends.astype(np.int64), sabs.astype(np.float64)


def curves_brute(psf, cx, cy, delta, aspect, bins, square=False):
    """The definition by a loop over pixels and radii in Python floats (IEEE doubles, every operation rounded once)."""
    p = np.asarray(psf, dtype=np.float64)
    n = p.shape[0]
    cx, cy, delta, aspect = float(cx), float(cy), float(delta), float(aspect)
    ee, count = [LDR(0)] * bins, [0] * bins
    for k in range(n):
        y = (float(k) - cy) * aspect
        for j in range(n):
            x = float(j) - cx
            d2 = x * x + y * y
            for b in range(bins):
                r = float(b + 1) * delta
                inside = max(abs(x), abs(y)) <= r if square else d2 <= r * r
                if inside:
                    ee[b] = ee[b] + LDR(p[k, j])
                    count[b] += 1
    return np.array(ee, dtype=LDR), np.array(count, dtype=np.int64)


def lattice_count(r, aspect):
    """Points (i, k) of the integer lattice with i^2 + (aspect k)^2 <= r^2, for radii and aspects exact in binary."""
    total, reach = 0, int(r / aspect) + 1
    for k in range(-reach, reach + 1):
        for i in range(-int(r) - 1, int(r) + 2):
            total += i * i + (aspect * k) ** 2 <= r * r
    return total


def ree(ee, total, step, fractions):
    """b* step + step (f S - lo) / (ee[b*] - lo) with b* the first ring that reaches f S; NaN where none does or S > 0 is false."""
    out = []
    for f in fractions:
        target = f * total
        radius = float("nan")
        if total > 0.0:
            for b in range(len(ee)):
                if ee[b] >= target:
                    lo = float(ee[b - 1]) if b else 0.0
                    radius = b * step + step * (target - lo) / (float(ee[b]) - lo)
                    break
        out.append(radius)
    return np.array(out, dtype=np.float64)


def bound(count, sum_abs):
    """The project's bound for a metric sum of ``count`` terms whose magnitudes add up to ``sum_abs``:
    C_METRIC log2(max(2, count)) 2^-53 sum_abs.  (bound_metric wants the four leading values of a metrics record and
    zeroes the peak's: the sum goes first.)"""
    return float(px.bound_metric(int(count), [float(sum_abs), 0.0, 0.0, 0.0])[0])


def check_curve(got, psf, cx, cy, delta, aspect, square=False, what=""):
    """``got`` (bins doubles from the device) against the long-double curve about the same centre, radius by radius within
    ``bound``.  Returns the largest error as a multiple of its bound (0 where the bound is 0 and the curve exact)."""
    got = np.asarray(got, dtype=np.float64)
    want, count, sabs = curves(psf, cx, cy, delta, aspect, got.size, square)
    err = np.abs(got.astype(LDR) - want).astype(np.float64)
    lim = np.array([bound(c, s) for c, s in zip(count, sabs)])
    worst = 0.0
    for b in range(got.size):
        assert err[b] <= lim[b], f"{what}: radius {b}: |got - ref| = {err[b]:.3g} > bound {lim[b]:.3g} ({count[b]} members)"
        if lim[b] > 0.0:
            worst = max(worst, err[b] / lim[b])
    return worst


class EnergyModelDevice(blur_np.BlurModelDevice):
    """BlurModelDevice with the paos_ee_* entry points by the restatement (rounded to double).  Whatever stores PSFs,
    ``blur_apply`` included, makes the curves of an earlier compute stale, as in the library."""

    def psf_keep(self):
        super().psf_keep()
        self._ee_valid = False

    def run_passes(self, passes, blocks, live_rows=None, rows_stale=False, final_intensity=False, live_cols=None):
        ticket = super().run_passes(passes, blocks, live_rows=live_rows, rows_stale=rows_stale,
                                    final_intensity=final_intensity, live_cols=live_cols)
        if final_intensity and final_intensity != 2:
            self._ee_valid = False
        return ticket

    def blur_apply(self, *args, **kwargs):
        super().blur_apply(*args, **kwargs)
        self._ee_valid = False

    def energy_compute(self, bins, deltas, aspects, centre_mode, centres=None, square=False):
        n, nb = self.n, self.batch
        if not hasattr(self, "psf"):
            raise _lib.PaosHipError("paos_ee_compute failed (1): no PSF kept (paos_psf_keep)")
        if not 1 <= int(bins) <= _lib.EE_MAX_BINS or centre_mode not in (GIVEN, CENTROID, PEAK):
            raise _lib.PaosHipError("paos_ee_compute failed (1): bins or centre mode")
        d = np.broadcast_to(np.asarray(deltas, dtype=np.float64), (nb,))
        a = np.broadcast_to(np.asarray(aspects, dtype=np.float64), (nb,))
        ctr = np.full((nb, 2), n / 2) if centres is None else np.broadcast_to(np.asarray(centres, dtype=np.float64), (nb, 2))
        ok = np.all(np.isfinite(d)) and np.all(d > 0) and np.all(np.isfinite(a)) and np.all(a > 0)
        if not ok or np.any(bins * d > n / 2) or np.any(bins * d / a > n / 2):
            raise _lib.PaosHipError("paos_ee_compute failed (1): ring width, aspect or the size rule")
        if centre_mode == GIVEN and not (np.all(np.isfinite(ctr)) and np.all(ctr >= 0) and np.all(ctr < n)):
            raise _lib.PaosHipError("paos_ee_compute failed (1): the centre must be finite and inside [0, n)")
        self.log.append(("energy_compute", (int(bins), int(centre_mode), bool(square))))
        self._ee_summary = np.empty((nb, _lib.EE_SUMMARY))
        self._ee_curves = np.empty((nb, 2 if square else 1, int(bins)))
        for i, p in enumerate(np.asarray(self.psf, dtype=np.float64)):
            s = summary(p, centre_mode, ctr[i])
            self._ee_summary[i] = [float(s["S"]), float(s["Sx"]), float(s["Sy"]), s["peak"], s["peak_col"], s["peak_row"],
                                   s["cx"], s["cy"], float(s["fallback"])]
            for q in range(2 if square else 1):
                self._ee_curves[i, q] = curves(p, s["cx"], s["cy"], d[i], a[i], int(bins), square=bool(q))[0].astype(np.float64)
        self._ee_valid = True

    def energy_fetch(self, curves=True):
        if getattr(self, "_ee_summary", None) is None:
            raise _lib.PaosHipError("paos_ee_fetch failed (1): no energy profiles computed (paos_ee_compute)")
        if curves and not self._ee_valid:
            raise _lib.PaosHipError("paos_ee_fetch failed (1): the curves are stale")
        self.log.append(("energy_fetch", None))
        return self._ee_summary.copy(), self._ee_curves.copy() if curves else None
