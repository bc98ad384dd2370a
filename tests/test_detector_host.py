"""Detector images without a GPU: the NumPy restatement of the definition (tests/detector_np.py) against brute force
and aligned cases, the Detector's validation, and run_batch(detector=...) / run_broadband on the NumPy model of the
device (tests/fakes.py) against the oracle's PSFs rebinned."""
import numpy as np
import pytest

import detector_np
from conftest import l2_rel_err, rel_err
from fakes import ModelDevice
from oracle.run_np import run as oracle_run
from paos_amd import _lib
from paos_amd.chains import syn20_chain, syn20_wavelength
from paos_amd.detector import Detector, run_broadband
from paos_amd.run import run_batch

FIELD = {"us": 0.0, "ut": 0.0}
PSF_TOL = 1.0e-10


class DetectorModelDevice(ModelDevice):
    """ModelDevice with the restatement as its paos_detector_* entry points."""

    def detector_begin(self, det):
        self.detector = det
        self.image = np.zeros((det.ny, det.nx))

    def _images(self, dxs, dys):
        if not hasattr(self, "psf"):
            raise _lib.PaosHipError("no PSF kept (paos_psf_keep)")
        dxs = np.broadcast_to(np.asarray(dxs, dtype=np.float64), (self.batch,))
        dys = np.broadcast_to(np.asarray(dys, dtype=np.float64), (self.batch,))
        return [detector_np.rebin(self.psf[i], self.detector, dxs[i], dys[i]) for i in range(self.batch)]

    def detector_add(self, dxs, dys, weights):
        w = np.broadcast_to(np.asarray(weights, dtype=np.float64), (self.batch,))
        self.image = detector_np.accumulate(self._images(dxs, dys), w, self.image)

    def detector_images(self, dxs, dys):
        return np.stack(self._images(dxs, dys))

    def detector_fetch(self):
        return self.image.copy()


def brute_fractions(nd, pitch, centre, d, n, sub=1000):
    """Overlap fractions by counting sub-samples: ``sub`` per grid pixel, on a lattice whose points lie half a step away
    from every edge the geometries below place (their edges are multiples of 1 / sub in grid pixels)."""
    u = (np.arange(n * sub) + 0.5) / sub           # grid-pixel coordinate of each sub-sample
    x = (u - (0.5 * n + 0.5)) * d                   # the same point in metres
    j = np.floor(u).astype(int)
    m = np.floor((x - (centre - 0.5 * nd * pitch)) / pitch).astype(int)
    f = np.zeros((n, nd))
    ok = (m >= 0) & (m < nd)
    np.add.at(f, (j[ok], m[ok]), 1.0 / sub)
    return f


@pytest.mark.parametrize("ratio", [0.37, 1.0, 1.7, 2.0, 3.7])
@pytest.mark.parametrize("shift", [0.0, 0.123, -5.871])
def test_fractions_agree_with_supersampling(ratio, shift):
    n, d = 32, 2.0e-6
    for nd in (5, 13):
        got = detector_np.fractions(nd, ratio * d, shift * d, d, n)
        want = brute_fractions(nd, ratio * d, shift * d, d, n)
        assert np.max(np.abs(got - want)) < 1e-9, (nd, ratio, shift)


def test_aligned_cases_are_exact():
    rng = np.random.default_rng(5)
    n = 16
    psf = rng.random((n, n))
    for dx in (2.0**-20, 1.3e-6):
        det = Detector(n, n, dx, xc=-dx / 2, yc=-dx / 2)
        a = detector_np.rebin(psf, det, dx, dx)
        if dx == 2.0**-20:
            assert np.array_equal(a, psf)
        assert np.max(np.abs(a - psf)) <= 1e-13 * psf.max()
    dx = 2.0**-20
    det = Detector(n // 2, n // 2, 2 * dx, xc=-dx / 2, yc=-dx / 2)
    want = psf.reshape(n // 2, 2, n // 2, 2).sum(axis=(1, 3))
    assert np.allclose(detector_np.rebin(psf, det, dx, dx), want, rtol=1e-15, atol=0)
    # a detector that covers the grid keeps every photon; one off the grid gets none
    det = Detector(7, 9, 3.7 * dx, xc=0.3 * dx, yc=-0.2 * dx)
    assert abs(detector_np.rebin(psf, det, dx, dx).sum() - psf.sum()) < 1e-13 * psf.sum()
    assert not detector_np.rebin(psf, Detector(4, 4, dx, xc=100 * dx), dx, dx).any()


@pytest.mark.parametrize("kw", [dict(nx=0), dict(nx=4097), dict(nx=2.5), dict(nx=True), dict(ny=-3),
                                dict(pitch_x=0.0), dict(pitch_x=-1e-6), dict(pitch_x=float("nan")),
                                dict(pitch_y=float("inf")), dict(pitch_y=0.0), dict(xc=float("nan")),
                                dict(yc=float("-inf")), dict(pitch_x="1e-6")])
def test_detector_rejects_bad_inputs(kw):
    args = dict(nx=16, ny=8, pitch_x=1e-6)
    args.update(kw)
    with pytest.raises(ValueError):
        Detector(**args)


def test_detector_defaults():
    det = Detector(16, 8, 1e-6)
    assert det.pitch_y == 1e-6 and det.xc == 0.0 and det.yc == 0.0
    assert det.geometry().tolist() == [16, 8, 1e-6, 1e-6, 0.0, 0.0]
    assert Detector(np.int64(16), 8, 1e-6) == det


def _oracle_images(n, wls, det):
    out, powers = [], []
    for wl in wls:
        ref = oracle_run(1.0, wl, n, 4, FIELD, syn20_chain(), light=True)[20]
        psf = ref["amplitude"] ** 2
        out.append(detector_np.rebin(psf, det, ref["dx"], ref["dy"]))
        powers.append(psf.sum())
    return out, powers


@pytest.mark.parametrize("n", [64, 128])
def test_run_batch_and_run_broadband_on_the_model_device(n, monkeypatch):
    wls = [syn20_wavelength(k) for k in (0, 200, 511)]
    chains = [syn20_chain() for _ in wls]
    mid = oracle_run(1.0, wls[1], n, 4, FIELD, syn20_chain(), light=True)[20]
    det = Detector(21, 17, 1.7 * mid["dx"], 2.3 * mid["dy"], xc=0.31 * mid["dx"], yc=-0.62 * mid["dy"])
    want, powers = _oracle_images(n, wls, det)
    scale = max(a.max() for a in want)
    # per-item images on the record of the last surface
    res = run_batch(1.0, wls, n, 4, FIELD, chains, outputs=(), dev=DetectorModelDevice(n, len(wls)), detector=det)
    for i in range(len(wls)):
        got = res[i][20]["detector"]
        assert got.shape == (det.ny, det.nx)
        assert np.max(np.abs(got - want[i])) < PSF_TOL * scale and l2_rel_err(got, want[i]) < PSF_TOL
        assert 1 not in res[i] or "detector" not in res[i][1]
    # weighted accumulation into the context
    w = np.array([0.7, 0.0, 2.5])
    dev = DetectorModelDevice(n, len(wls))
    run_batch(1.0, wls, n, 4, FIELD, chains, outputs=(), dev=dev, sync=False, keep_psf=False, detector=det,
              detector_weights=w)
    ref_image = detector_np.accumulate(want, w)
    assert rel_err(dev.detector_fetch(), ref_image) < PSF_TOL
    # run_broadband: one block, and blocks of two (the second one padded), bit for bit
    monkeypatch.setattr(_lib, "DeviceFields", DetectorModelDevice)
    one = run_broadband(1.0, wls, w, n, 4, FIELD, chains, det, batch=3)
    two = run_broadband(1.0, wls, w, n, 4, FIELD, syn20_chain(), det, batch=2)
    assert np.array_equal(one["image"], two["image"])
    assert rel_err(one["image"], ref_image) < PSF_TOL and l2_rel_err(one["image"], ref_image) < PSF_TOL
    want_power = sum(wi * p for wi, p in zip(w, powers))
    assert abs(one["power"] - want_power) < 1e-12 * want_power and abs(two["power"] - one["power"]) < 1e-14 * want_power
    assert one["wavelengths"].tolist() == wls and one["weights"].tolist() == w.tolist()


def test_detector_needs_a_saved_last_surface():
    chain = syn20_chain()
    chain[20] = dict(chain[20], save=False)
    det = Detector(8, 8, 1e-6)
    with pytest.raises(ValueError):
        run_batch(1.0, [syn20_wavelength(0)], 64, 4, FIELD, [chain], outputs=(), dev=DetectorModelDevice(64, 1),
                  detector=det)
    with pytest.raises(ValueError):  # weights accumulate into a context the caller keeps
        run_batch(1.0, [syn20_wavelength(0)], 64, 4, FIELD, [syn20_chain()], outputs=(), detector=det,
                  detector_weights=[1.0])
