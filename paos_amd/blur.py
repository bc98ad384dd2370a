"""Blurred PSFs: what ``run_batch(..., psf_blur=PsfBlur(...))`` asks for (README.md, "Blurred PSFs")."""
import numpy as np


def _per_item(value, what):
    """A scalar or a 1-D sequence of finite, non-negative doubles (``ValueError`` otherwise)."""
    try:
        arr = np.array(value, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be a number or one number per item, got {value!r}") from None
    if arr.ndim > 1:
        raise ValueError(f"{what} must be a number or one number per item, got an array of shape {arr.shape}")
    if not np.all(np.isfinite(arr)) or np.any(arr < 0.0):
        raise ValueError(f"{what} must be finite and >= 0, got {value!r}")
    return arr


class PsfBlur:
    """The last surface's PSFs convolved, on the GPU, with what the instrument adds to the optics: a Gaussian of 1-sigma
    widths ``sigma_x`` / ``sigma_y`` in metres at the image plane (line-of-sight jitter and charge diffusion add in
    quadrature: pass their root sum of squares; ``sigma_y`` defaults to ``sigma_x``) and, with ``pixel=(px, py)`` in
    metres, the pixel aperture -- the sampled "effective PSF".  The sigmas are scalars or one value per item.

    The blur is one multiplication on the spectrum of the kept PSF, ``exp(-2 pi^2 (sigma_x^2 fx^2 + sigma_y^2 fy^2))
    sinc(px fx) sinc(py fy)``, and a packed real-output inverse transform back into the PSF buffer (``paos_blur_apply``):
    the convolution is circular, the sum is kept, nothing is clamped.  ``array=True`` also hands out the blurred PSF
    itself (``'psf_blur'``).
    """

    reads_psf = True  # (``attach`` rewrites the kept PSFs: run._attach_products runs it before every other reader)

    def __init__(self, sigma_x, sigma_y=None, pixel=None, array=False):
        self.sigma_x = _per_item(sigma_x, "sigma_x")
        self.sigma_y = self.sigma_x.copy() if sigma_y is None else _per_item(sigma_y, "sigma_y")
        if pixel is None:
            self.pixel = None
        else:
            try:
                px, py = pixel
            except (TypeError, ValueError):
                raise ValueError(f"pixel must be None or (px, py), got {pixel!r}") from None
            self.pixel = (_per_item(px, "pixel[0]"), _per_item(py, "pixel[1]"))
        self.array = bool(array)

    def _columns(self):
        px, py = self.pixel if self.pixel is not None else (np.float64(0.0), np.float64(0.0))
        return (("sigma_x", self.sigma_x), ("sigma_y", self.sigma_y), ("pixel[0]", px), ("pixel[1]", py))

    def check(self, batch):
        """Everything that depends on the batch -- ``ValueError``, before anything is launched."""
        for what, arr in self._columns():
            if np.ndim(arr) == 1 and np.shape(arr)[0] != batch:
                raise ValueError(f"{what} must be a number or one number per item ({batch}), got {np.shape(arr)[0]} values")

    def take(self, idx):
        """The blur of the items ``idx`` of the batch this one was written for (a block of a longer sweep)."""
        pick = lambda arr: arr if np.ndim(arr) == 0 else arr[np.asarray(idx, dtype=np.int64)]  # noqa: E731
        pixel = None if self.pixel is None else (pick(self.pixel[0]), pick(self.pixel[1]))
        return PsfBlur(pick(self.sigma_x), pick(self.sigma_y), pixel, self.array)

    def attach(self, dev, recs, dxs, dys):
        """Blur the PSFs ``dev`` keeps right now, in place; ``recs[i]`` gets item i's entries.  The spectra ``dev`` holds
        afterwards are the system transfer functions.  Enqueues only, unless the arrays are asked for."""
        nb = dev.batch
        sx, sy, px, py = (np.broadcast_to(arr, (nb,)) for _, arr in self._columns())
        dev.otf_compute()
        dev.blur_apply(dxs, dys, sx, sy, px, py)
        for i, rec in enumerate(recs):
            rec["blur_sigma"] = (float(sx[i]), float(sy[i]))
            if self.array:
                rec["psf_blur"] = dev.psf_fetch(i)
