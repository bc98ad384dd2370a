"""Wavefront fits: what ``run_batch(..., wavefront=WavefrontFit(...))`` and ``WFO.fit_zernikes`` ask for, and the host
algebra that turns the device's sums into coefficients and OPD statistics (README.md, "Wavefront fits")."""
import numpy as np

from .planner import gram_polynomials, jacobi_recurrence, zernike_block
from .zernike import ORDERINGS, zernike_tables

MAX_TERMS = 63  # paos_wavefront_fit: K + 1 <= 64 columns
WEIGHTS = {"uniform": 0, "intensity": 1}  # PAOS_WF_UNIFORM, PAOS_WF_INTENSITY
TWO_PI = 2.0 * np.pi
# the summary of paos_wavefront_fetch
S_COUNT, S_RE, S_IM, S_SQRT_I, S_I, S_PHI_MIN, S_PHI_MAX, S_FALLBACK, S_W, S_WPHI = range(10)


def _numbers(value, what, positive=False):
    """A finite scalar, or a 1-D array of them (one per item); ``ValueError`` otherwise."""
    try:
        arr = np.array(value, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be a finite number or one per item, got {value!r}") from None
    if arr.ndim > 1 or not np.all(np.isfinite(arr)) or isinstance(value, (bool, str)):
        raise ValueError(f"{what} must be a finite number or one per item, got {value!r}")
    if positive and not np.all(arr > 0.0):
        raise ValueError(f"{what} must be > 0, got {value!r}")
    return arr


def fit_from_sums(summary, sums, terms, wl):
    """The ``wf_*`` entries of one item from its row of the device's summary and of its sums (the Gram matrix of
    ``[Z_0 .. Z_{K-1}, phi]`` under the weights, upper triangle row by row), fp64:

    ``c = solve(G, b)``; ``wf_coeff = c lambda / 2 pi`` (metres, positive where a positive coefficient of ``WFO.zernikes``
    would have put it; the piston is relative to the direction of the reference phasor r); ``wf_rms`` the weighted
    standard deviation of phi, ``wf_residual_rms`` what the fit leaves, ``wf_pv``, ``wf_strehl = |r|^2 / (sum sqrt I)^2``.
    An empty support or a singular G gives NaN coefficients and RMS values (``wf_singular``); nothing is raised."""
    k = int(terms)
    s = np.asarray(summary, dtype=np.float64)
    a = np.zeros((k + 1, k + 1), dtype=np.float64)
    iu = np.triu_indices(k + 1)
    a[iu] = np.asarray(sums, dtype=np.float64)
    a.T[iu] = a[iu]
    g, b, phi2 = a[:k, :k], a[:k, k], a[k, k]
    count, sw, swphi = int(s[S_COUNT]), float(s[S_W]), float(s[S_WPHI])
    scale = wl / TWO_PI
    coeff = np.full(k, np.nan)
    rms = residual = pv = strehl = np.nan
    singular = False
    if count > 0:
        try:
            # (solve raises for an exactly singular matrix only: a G of deficient rank -- more terms than pixels -- is one too)
            if not np.all(np.isfinite(g)) or np.linalg.matrix_rank(g, hermitian=True) < k:
                raise np.linalg.LinAlgError("singular")
            c = np.linalg.solve(g, b)
            if not np.all(np.isfinite(c)):
                raise np.linalg.LinAlgError("singular")
            coeff = c * scale
        except np.linalg.LinAlgError:
            singular = True
        if sw > 0.0 and not singular:
            residual = scale * np.sqrt(max(0.0, (phi2 - float(b @ c)) / sw))
            rms = scale * np.sqrt(max(0.0, phi2 / sw - (swphi / sw) ** 2))
        pv = scale * (s[S_PHI_MAX] - s[S_PHI_MIN])
        if s[S_SQRT_I] > 0.0:
            strehl = (s[S_RE] * s[S_RE] + s[S_IM] * s[S_IM]) / (s[S_SQRT_I] * s[S_SQRT_I])
    return {
        "wf_coeff": coeff, "wf_rms": float(rms), "wf_residual_rms": float(residual), "wf_pv": float(pv),
        "wf_strehl": float(strehl), "wf_pixels": count, "wf_phase_absmax": float(max(abs(s[S_PHI_MIN]), abs(s[S_PHI_MAX]))),
        "wf_fallback": bool(s[S_FALLBACK] != 0.0), "wf_singular": singular,
    }


class WavefrontFit:
    """The Zernike content and the OPD statistics of the field at saved surfaces, summed on the GPU: the first ``terms``
    polynomials (1 .. 63) of ``ordering`` / ``normalize`` on the disk of ``radius`` metres about the grid centre, with
    ``origin`` and ``offset`` (degrees) as ``WFO.zernikes`` takes them; ``weight`` ``"uniform"`` or ``"intensity"``; pixels
    with ``|u|^2 <= min_intensity`` are left out.  ``radius`` and ``min_intensity`` are scalars or one value per item.
    ``surfaces``: the surface numbers (the ``num`` keys of the results) to fit at; None -- every saved surface.

    The phase is taken relative to the field's own sum over the disk and is not unwrapped: the fit is valid while the OPD
    stays within half a wavelength of the amplitude-weighted mean (``wf_phase_absmax`` tells how close to pi it came)."""

    def __init__(self, terms, radius, ordering="standard", normalize=True, origin="x", offset=0.0, weight="uniform",
                 min_intensity=0.0, surfaces=None):
        if isinstance(terms, bool) or not isinstance(terms, (int, np.integer)) or not 1 <= terms <= MAX_TERMS:
            raise ValueError(f"terms must be an integer in 1 .. {MAX_TERMS}, got {terms!r}")
        if ordering not in ORDERINGS:
            raise ValueError(f"ordering must be one of {ORDERINGS}, got {ordering!r}")
        if origin not in ("x", "y"):
            raise ValueError(f"origin must be 'x' or 'y', got {origin!r}")
        if weight not in WEIGHTS:
            raise ValueError(f"weight must be 'uniform' or 'intensity', got {weight!r}")
        self.radius = _numbers(radius, "radius", positive=True)
        self.min_intensity = _numbers(min_intensity, "min_intensity")
        if np.any(self.min_intensity < 0.0):
            raise ValueError(f"min_intensity must be >= 0, got {min_intensity!r}")
        off = _numbers(offset, "offset")
        if off.ndim:
            raise ValueError(f"offset must be one finite number, got {offset!r}")
        self.terms, self.ordering, self.normalize, self.origin = int(terms), ordering, normalize, origin
        self.offset, self.weight = float(off), weight
        if surfaces is not None:
            try:
                surfaces = tuple(surfaces)
            except TypeError:
                raise ValueError(f"surfaces must be None or an iterable of surface numbers, got {surfaces!r}") from None
        self.surfaces = surfaces

    def check(self, batch):
        """Everything that depends on the batch -- ``ValueError``, before anything is launched."""
        for name, arr in (("radius", self.radius), ("min_intensity", self.min_intensity)):
            if arr.ndim and arr.shape != (batch,):
                raise ValueError(f"wavefront: {name} must be a scalar or have one value per item ({batch}), got {arr.size}")

    def request(self, dxs, dys, wls):
        """(nmax, kdim, table, blocks, poly) of ``DeviceFields.wavefront_fit`` on the samplings given: the header of a
        ``planner.zernike_block`` per item (its coefficient planes are not read)."""
        m, n, norm = zernike_tables(self.terms, self.ordering, bool(self.normalize))
        nmax = int(n.max())
        radii = np.broadcast_to(self.radius, (len(dxs),))
        zeros = np.zeros(self.terms)
        blocks = [zernike_block(m, n, norm, zeros, dx, dy, r, wl, origin=self.origin, offset_deg=self.offset, nmax=nmax)[0][:8]
                  for dx, dy, r, wl in zip(dxs, dys, radii.tolist(), wls)]
        return nmax, nmax // 2 + 1, jacobi_recurrence(nmax), np.array(blocks), gram_polynomials(m, n, norm)

    def fit(self, dev, dxs, dys, wls):
        """One dict of ``wf_*`` entries per item, from the fields ``dev`` holds right now.  Synchronises (one small copy)."""
        self.check(dev.batch)
        nmax, kdim, table, blocks, poly = self.request(dxs, dys, wls)
        floors = np.broadcast_to(self.min_intensity, (dev.batch,))
        dev.wavefront_fit(nmax, kdim, table, blocks, poly, weight=WEIGHTS[self.weight], min_intensity=floors)
        summary, sums = dev.wavefront_fetch()
        return [fit_from_sums(summary[i], sums[i], self.terms, wl) for i, wl in enumerate(wls)]
