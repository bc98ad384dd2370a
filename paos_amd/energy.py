"""Encircled energy: what ``run_batch(..., psf_energy=EnergyProfile(...))`` asks for (README.md, "Encircled energy")."""
import numpy as np

MAX_BINS = 1024  # paos_ee_compute


class EnergyProfile:
    """Encircled-energy curves of the last surface's kept PSFs, each about the item's own centre, on the GPU: ``bins``
    radii ``(b + 1) * step``, in metres at the image plane (``unit="m"``: circles on the detector, whatever ``dx`` and
    ``dy`` are) or in pixels (``unit="px"``: the circles of ``paos_psf_metrics``).  ``centre``: None -- the grid centre
    ``(N/2, N/2)``; ``"centroid"`` or ``"peak"`` -- formed on the device from the PSF itself, without a host round trip;
    or a (B, 2) array of pixel positions ``(x, y)`` in ``[0, N)``.  ``square=True`` adds the ensquared energy (squares of
    half-width ``(b + 1) * step``).  ``fractions`` in ``(0, 1]``: the radii at which the encircled energy reaches that
    share of the PSF's total power, interpolated linearly within a ring (``ree``).
    """

    reads_psf = True

    def __init__(self, bins, step, unit="m", centre=None, fractions=(), square=False):
        if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)) or not 1 <= bins <= MAX_BINS:
            raise ValueError(f"bins must be an integer in 1 .. {MAX_BINS}, got {bins!r}")
        try:
            step = float(step)
        except (TypeError, ValueError):
            raise ValueError(f"step must be a finite number > 0, got {step!r}") from None
        if not np.isfinite(step) or not step > 0.0:
            raise ValueError(f"step must be a finite number > 0, got {step!r}")
        if unit not in ("m", "px"):
            raise ValueError(f"unit must be 'm' or 'px', got {unit!r}")
        if centre is None or isinstance(centre, str):
            if centre not in (None, "centroid", "peak"):
                raise ValueError(f"centre must be None, 'centroid', 'peak' or a (B, 2) array, got {centre!r}")
        else:
            try:
                centre = np.array(centre, dtype=np.float64)
            except (TypeError, ValueError):
                raise ValueError(f"centre must be None, 'centroid', 'peak' or a (B, 2) array, got {centre!r}") from None
            if centre.ndim != 2 or centre.shape[1] != 2:
                raise ValueError(f"centre must be None, 'centroid', 'peak' or a (B, 2) array, got shape {centre.shape}")
            if not np.all(np.isfinite(centre)):
                raise ValueError("centres must be finite")
        try:
            fractions = np.array(fractions, dtype=np.float64).reshape(-1)
        except (TypeError, ValueError):
            raise ValueError(f"fractions must be numbers in (0, 1], got {fractions!r}") from None
        if not np.all((fractions > 0.0) & (fractions <= 1.0)):  # (a NaN fails both)
            raise ValueError(f"fractions must lie in (0, 1], got {fractions.tolist()!r}")
        self.bins, self.step, self.unit, self.centre = int(bins), step, unit, centre
        self.fractions, self.square = fractions, bool(square)

    def check(self, batch, n):
        """Everything that depends on the batch and the grid -- ``ValueError``, before anything is launched."""
        if isinstance(self.centre, np.ndarray):
            if self.centre.shape != (batch, 2):
                raise ValueError(f"centres must have shape ({batch}, 2), got {self.centre.shape}")
            if np.any(self.centre < 0.0) or np.any(self.centre >= n):
                raise ValueError(f"centres must lie inside [0, {n})")

    def rings(self, n, dxs, dys):
        """(ring widths in units of dx_i, aspects dy_i / dx_i) on the samplings given, one division each; ``ValueError``
        naming the first item whose largest circle would be wider or taller than the n-pixel grid."""
        dxs, dys = np.asarray(dxs, dtype=np.float64), np.asarray(dys, dtype=np.float64)
        if self.unit == "m":
            deltas, aspects = self.step / dxs, dys / dxs
        else:
            deltas, aspects = np.full(dxs.shape, self.step), np.ones(dxs.shape)
        for i, (d, a) in enumerate(zip(deltas.tolist(), aspects.tolist())):
            reach = float(self.bins) * d
            if not (np.isfinite(d) and d > 0.0 and np.isfinite(a) and a > 0.0):
                raise ValueError(f"psf_energy: item {i}: the sampling (dx = {dxs[i]!r}, dy = {dys[i]!r}) gives no ring width")
            if reach > n / 2 or reach / a > n / 2:
                raise ValueError(f"psf_energy: item {i}: {self.bins} rings of {self.step!r} {self.unit} reach {reach!r} x "
                                 f"{reach / a!r} pixels, more than half the {n}-pixel grid")
        return deltas, aspects

    def ree(self, ee, total):
        """The radii at which the curve ``ee`` reaches ``fractions * total``: with ``b*`` the first ring with ``ee[b*] >=
        target`` and ``lo = ee[b* - 1]`` (0 for ``b* = 0``), ``b* step + step (target - lo) / (ee[b*] - lo)``.  NaN where
        the curve never gets there or ``total > 0`` is false."""
        ee = np.asarray(ee, dtype=np.float64)
        out = np.full(self.fractions.shape, np.nan)
        if not total > 0.0:
            return out
        for q, f in enumerate(self.fractions.tolist()):
            target = f * total
            hit = np.flatnonzero(ee >= target)
            if hit.size:
                b = int(hit[0])
                lo = float(ee[b - 1]) if b > 0 else 0.0
                out[q] = b * self.step + self.step * (target - lo) / (float(ee[b]) - lo)
        return out

    def attach(self, dev, recs, dxs, dys):
        """``recs[i]`` gets item i's entries, from the PSFs ``dev`` keeps right now.  Synchronises (one small copy)."""
        from . import _lib

        deltas, aspects = self.rings(dev.n, dxs, dys)
        self.check(dev.batch, dev.n)
        given = isinstance(self.centre, np.ndarray)
        mode = _lib.EE_GIVEN if given or self.centre is None else {"centroid": _lib.EE_CENTROID, "peak": _lib.EE_PEAK}[self.centre]
        centres = self.centre if given else None
        dev.energy_compute(self.bins, deltas, aspects, mode, centres=centres, square=self.square)
        summary, curves = dev.energy_fetch()
        radius = (np.arange(self.bins, dtype=np.float64) + 1.0) * self.step
        for i, rec in enumerate(recs):
            s = summary[i]
            rec["ee_radius"] = radius.copy()
            rec["ee"] = curves[i, 0].copy()
            if self.square:
                rec["ensq"] = curves[i, 1].copy()
            rec["ee_total"] = float(s[0])
            rec["ee_centre"] = (float(s[6]), float(s[7]))
            rec["ee_peak"] = (float(s[3]), (int(s[4]), int(s[5])))
            rec["ee_fallback"] = bool(s[8] != 0.0)
            rec["ree"] = self.ree(curves[i, 0], float(s[0]))
