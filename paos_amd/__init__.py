"""paos_amd -- MI355X-native Fresnel propagation core behind the PAOS API.

Drop-in for the wavefront-propagation hot path of arielmission-space/PAOS
(``paos.core.run.run`` driving ``paos.classes.wfo.WFO``): the same
``paos_amd.run.run(pupil_diameter, wavelength, gridsize, zoom, field, opt_chain)`` and
``WFO(beam_diameter, wl, grid_size, zoom)`` surfaces, with the N x N complex
field living in HBM and every field operator a hand-written HIP kernel for
gfx950 reached through a ctypes C-ABI (``libpaoship.so``, include/paos_hip.h).

Importing the package does not need a GPU; creating a ``WFO`` or calling
``run`` loads the HIP library and fails loudly when it (or a GPU) is missing --
there is no CPU fallback in the product path.

``run_batch(..., focus_planes=[dz, ...])`` adds a through-focus stack behind the last surface: K defocus planes
(``WFO.ptp(dz)`` of the last-surface field, on the image plane's sampling) from one chain walk and one forward
transform, each with its power, arrays, metrics and detector image (README.md, "Through-focus stacks").

``run_batch(..., outputs=("mtf", "otf"), mtf_cuts=True)`` hands out the transfer functions of the last surface's PSFs,
computed on the GPU by a packed real-input 2-D transform (README.md, "Transfer functions").

``run_batch(..., psf_zoom=PsfWindow(size, oversample))`` adds a window of the last surface's PSF on a finer grid: the
exact band-limited interpolant of the field, two fp64 matrix-instruction contractions (README.md, "Zoomed PSFs").

``run_batch(..., psf_blur=PsfBlur(sigma_x, sigma_y, pixel=...))`` blurs the last surface's kept PSFs by pointing jitter,
charge diffusion and the pixel aperture: one multiplication on their spectra and a packed real-output inverse transform
on the GPU; detector images and transfer functions are then the system ones (README.md, "Blurred PSFs").

``run_batch(..., psf_energy=EnergyProfile(bins, step, centre="centroid", fractions=(0.9,)))`` adds the encircled (and
ensquared) energy of the last surface's kept PSFs on up to 1024 radii in metres, each about the item's own centroid, peak
or given centre, with the radii that enclose the requested fractions -- summed, centred and binned on the GPU, on the lean
walk and behind a blur (README.md, "Encircled energy").

``run_batch(..., wavefront=WavefrontFit(terms, radius, surfaces=(num,)))`` answers the pupil-side questions: the Zernike
coefficients, RMS and peak-to-valley OPD and the Strehl ratio of the field at saved surfaces, from sums formed on the GPU
(README.md, "Wavefront fits"); ``WFO.fit_zernikes`` does the same for the drop-in class.

``run_batch(..., pointing=PointingSeries(det, offsets, apertures=[(m0, m1, n0, n1)], response=gains))`` gives the time
series of a moving line of sight: the flux of every frame inside boxes of detector pixels whose gains differ (and, with
``frames=True``, the frames), made on the GPU from the kept PSFs; only the fluxes cross to the host (README.md, "Pointing
series").  With ``pointing_weights`` the frames are instead added, weighted, into a sum that the caller's device context
keeps in HBM across the blocks of a sweep, and ``run_broadband_series(..., pointing)`` returns the broadband series: what a
detector records over its passband while the line of sight moves (README.md, "Broadband series").
"""
from .abcd import ABCD
from .coordinate_break import coordinate_break
from .parse_config import parse_config
from .zernike import Zernike

from .raytrace import raytrace

__all__ = ["ABCD", "Detector", "EnergyProfile", "PointingSeries", "PsfBlur", "PsfWindow", "WFO", "WavefrontFit", "Zernike", "coordinate_break", "parse_config", "raytrace",
           "run_batch", "run_broadband", "run_broadband_series", "run_sharded"]
__version__ = "0.1.0"


def __getattr__(name):
    # device-backed entry points are imported on first use so that host-only helpers (parser,
    # ABCD, chain builders) work on machines without a GPU.  ``paos_amd.run`` is the MODULE
    # (like paos.core.run); its function is ``paos_amd.run.run``.
    import importlib

    if name == "WFO":
        return importlib.import_module(".wfo", __name__).WFO
    if name == "run_batch":
        return importlib.import_module(".run", __name__).run_batch
    if name in ("Detector", "run_broadband", "run_broadband_series"):
        return getattr(importlib.import_module(".detector", __name__), name)
    if name == "PsfBlur":
        return importlib.import_module(".blur", __name__).PsfBlur
    if name == "EnergyProfile":
        return importlib.import_module(".energy", __name__).EnergyProfile
    if name == "PointingSeries":
        return importlib.import_module(".pointing", __name__).PointingSeries
    if name == "WavefrontFit":
        return importlib.import_module(".wavefront", __name__).WavefrontFit
    if name == "PsfWindow":
        return importlib.import_module(".zoom", __name__).PsfWindow
    if name == "run_sharded":
        return importlib.import_module(".dist", __name__).run_sharded
    raise AttributeError(name)
