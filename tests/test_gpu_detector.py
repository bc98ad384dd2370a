"""Detector images on the GPU (include/paos_hip.h, paos_detector_*): the kernels against the NumPy restatement of the
definition (tests/detector_np.py), the accumulator's order and determinism, and run_broadband end to end against the
oracle.  Everything goes through the C ABI of libpaoship.so."""
import os

import numpy as np
import pytest

import detector_np
from conftest import l2_rel_err, rel_err

pytestmark = pytest.mark.gpu

ON_AXIS = {"us": 0.0, "ut": 0.0}
TOL = 1.0e-13
LENS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "data", "lens")
DX0 = 1.0e-6


def _random_psfs(dev, seed):
    rng = np.random.default_rng(seed)
    for i in range(dev.batch):
        dev.upload(i, rng.standard_normal((dev.n, dev.n)) + 1j * rng.standard_normal((dev.n, dev.n)))
    dev.psf_keep()
    return [dev.psf_fetch(i) for i in range(dev.batch)]


def _geometries(n):
    from paos_amd.detector import Detector

    out = []
    for r in (0.37, 1.0, 1.7, 2.0, 3.7):  # pitch / dx, non-integer centres, pitch_x != pitch_y, nx != ny
        out.append(Detector(37, 29, r * DX0, 1.13 * r * DX0, xc=0.31 * DX0, yc=-0.77 * DX0))
    # hanging off the right and the bottom grid edges
    out.append(Detector(45, 61, 1.7 * DX0, 1.3 * DX0, xc=0.5 * n * DX0 + 0.3 * DX0, yc=-0.5 * n * DX0 - 2.6 * DX0))
    return out


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("n", [256, 1024, 4096])
def test_detector_images_match_the_restatement(n, precision):
    from paos_amd import _lib

    dev = _lib.DeviceFields(n, 3, precision)
    try:
        psfs = _random_psfs(dev, n)
        dxs = DX0 * np.array([1.0, 1.37, 1.9])  # the items' pitches span a factor 1.9
        dys = 1.1 * dxs
        for det in _geometries(n):
            dev.detector_begin(det)
            got = dev.detector_images(dxs, dys)
            for i in range(3):
                want = detector_np.rebin(psfs[i], det, dxs[i], dys[i])
                assert want.any()
                e, e2 = rel_err(got[i], want), l2_rel_err(got[i], want)
                assert e < TOL and e2 < TOL, (det, i, e, e2)
    finally:
        dev.close()


def test_flux_is_kept_and_empty_detectors_are_zero():
    from paos_amd import _lib
    from paos_amd.detector import Detector

    n = 1024
    dev = _lib.DeviceFields(n, 3)
    try:
        psfs = _random_psfs(dev, 11)
        dxs = DX0 * np.array([1.0, 1.5, 1.9])
        dev.detector_begin(Detector(1000, 1001, 1.9 * DX0 * 1.05, 1.9 * DX0 * 1.04, xc=0.4 * DX0, yc=-0.3 * DX0))
        got = dev.detector_images(dxs, dxs)
        for i in range(3):
            assert abs(got[i].sum() - psfs[i].sum()) <= TOL * psfs[i].sum(), i
        dev.detector_begin(Detector(64, 32, 2 * DX0, xc=n * 2 * DX0, yc=0.0))
        assert not dev.detector_images(dxs, dxs).any()
        dev.detector_add(dxs, dxs, [1.0, 2.0, 3.0])
        assert not dev.detector_fetch().any()
    finally:
        dev.close()


def test_accumulation_order_and_determinism():
    from paos_amd import _lib
    from paos_amd.detector import Detector

    n = 256
    w = np.array([0.3, 0.0, 1.7, 2.2, 0.0, 0.9, 1.1, 0.05])
    dxs = DX0 * np.linspace(1.0, 1.9, 8)
    dys = 1.2 * dxs
    det = Detector(53, 47, 1.7 * DX0, 2.1 * DX0, xc=0.37 * DX0, yc=0.11 * DX0)
    dev = _lib.DeviceFields(n, 8)
    half = _lib.DeviceFields(n, 4)
    try:
        rng = np.random.default_rng(3)
        fields = [rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)) for _ in range(8)]
        for i, f in enumerate(fields):
            dev.upload(i, f)
        dev.psf_keep()
        psfs = [dev.psf_fetch(i) for i in range(8)]
        dev.detector_begin(det)
        dev.detector_add(dxs, dys, w)
        image = dev.detector_fetch()
        want = detector_np.accumulate([detector_np.rebin(p, det, a, b) for p, a, b in zip(psfs, dxs, dys)], w)
        assert rel_err(image, want) < TOL and l2_rel_err(image, want) < TOL
        # the same run again: bit for bit
        dev.detector_begin(det)
        dev.detector_add(dxs, dys, w)
        assert np.array_equal(dev.detector_fetch(), image)
        # the same 8 PSFs fed as two halves of 4
        half.detector_begin(det)
        for h in (0, 1):
            for i in range(4):
                half.upload(i, fields[4 * h + i])
            half.psf_keep()
            assert all(np.array_equal(half.psf_fetch(i), psfs[4 * h + i]) for i in range(4))
            half.detector_add(dxs[4 * h:4 * h + 4], dys[4 * h:4 * h + 4], w[4 * h:4 * h + 4])
        assert np.array_equal(half.detector_fetch(), image)
    finally:
        dev.close()
        half.close()


def _airs():
    from paos_amd.parse_config import parse_config

    pup, par, wls, fields, chains = parse_config(os.path.join(LENS, "Ariel_AIRS-CH0.ini"))
    return pup, par, wls, fields, chains


def test_run_broadband_airs_ch0_vs_oracle():
    from oracle.run_np import run as oracle_run
    from paos_amd.detector import Detector, run_broadband

    pup, par, wls_um, fields, chains = _airs()
    n, zoom = int(par["grid_size"]), par["zoom"]
    assert n == 512 and len(wls_um) == 4
    wls = [1.0e-6 * x for x in wls_um]  # the lens file lists micrometres
    last = list(chains[0].keys())[-1]
    refs = [oracle_run(pup, wl, n, zoom, fields[0], ch, light=True)[last] for wl, ch in zip(wls, chains)]
    assert max(r["dx"] for r in refs) / min(r["dx"] for r in refs) > 2.0
    mid = refs[1]
    det = Detector(96, 80, 2.0 * mid["dx"], 1.6 * mid["dy"], xc=0.27 * mid["dx"], yc=-0.41 * mid["dy"])
    w = np.array([1.0, 0.35, 2.0, 0.8])
    want = detector_np.accumulate([detector_np.rebin(r["amplitude"] ** 2, det, r["dx"], r["dy"]) for r in refs], w)
    assert want.max() > 0.0
    got = run_broadband(pup, wls, w, n, zoom, fields[0], chains, det, batch=2)
    e, e2 = rel_err(got["image"], want), l2_rel_err(got["image"], want)
    assert e < 1e-10 and e2 < 1e-10, (e, e2)
    want_power = sum(wi * (r["amplitude"] ** 2).sum() for wi, r in zip(w, refs))
    assert abs(got["power"] - want_power) < 1e-10 * want_power
    # fp32 contexts: the same image within the fp32 gate
    got32 = run_broadband(pup, wls, w, n, zoom, fields[0], chains, det, batch=2, precision="fp32")
    assert rel_err(got32["image"], got["image"]) < 2e-5 and l2_rel_err(got32["image"], got["image"]) < 2e-5


def test_lean_and_ordinary_walk_at_the_headline_shape():
    """SYN20 at 4096^2 x 32, two walked steps as bench.measure issues them, the second with a 256^2 detector at twice the
    pitch of the first step's middle wavelength.  The surface-1 save is switched off in both walks, so the ordinary walk
    (outputs=("psf",)) copies back one PSF per item, not two."""
    import hashlib

    from paos_amd import _lib
    from paos_amd.chains import syn20_chain, syn20_wavelength
    from paos_amd.detector import Detector
    from paos_amd.run import run_batch

    n, nb = 4096, 32
    chain = syn20_chain()
    chain[1] = dict(chain[1], save=False)
    chains = [chain] * nb
    w = np.linspace(0.5, 1.5, nb)
    w[5] = 0.0
    det = None
    images, digests = {}, {}
    for outputs in ((), ("psf",)):
        dev = _lib.DeviceFields(n, nb)
        try:
            res = None
            for g in (0, 1):
                if res is not None:
                    for t in {rec["power_ticket"] for r in res for rec in r.values() if "power_ticket" in rec}:
                        dev.norm2_release(t)
                    if det is None:
                        mid = res[nb // 2][20]
                        det = Detector(256, 256, 2.0 * mid["dx"], 2.0 * mid["dy"], xc=0.3 * mid["dx"], yc=-0.2 * mid["dy"])
                    res = None
                wls = [syn20_wavelength((g * nb + i) % 512) for i in range(nb)]
                kw = dict(detector=det, detector_weights=w) if g == 1 else {}
                res = run_batch(1.0, wls, n, 4, ON_AXIS, chains, outputs=outputs, dev=dev, sync=False, keep_psf=True, **kw)
            images[outputs] = dev.detector_fetch()
            want = np.zeros((det.ny, det.nx))
            digests[outputs] = []
            for i in range(nb):
                psf = dev.psf_fetch(i)
                if outputs:
                    assert np.array_equal(psf, res[i][20]["psf"])
                    del res[i][20]["psf"]
                digests[outputs].append(hashlib.sha256(psf.tobytes()).hexdigest())
                want = want + w[i] * detector_np.rebin(psf, det, res[i][20]["dx"], res[i][20]["dy"])
                del psf
            e, e2 = rel_err(images[outputs], want), l2_rel_err(images[outputs], want)
            assert e < TOL and e2 < TOL, (outputs, e, e2)
            res = None
        finally:
            dev.close()
    lean, plain = images[()], images[("psf",)]
    assert lean.max() > 0.0
    assert rel_err(lean, plain) < TOL and l2_rel_err(lean, plain) < TOL
    same = digests[()] == digests[("psf",)]
    print(f"lean and ordinary walks: kept PSFs bit-identical: {same}")
    if same:
        assert np.array_equal(lean, plain)


def test_errors():
    from paos_amd import _lib
    from paos_amd.chains import syn20_chain, syn20_wavelength
    from paos_amd.detector import Detector
    from paos_amd.run import run_batch

    dev = _lib.DeviceFields(64, 2)
    try:
        dev.detector_begin(Detector(8, 8, 1e-6))
        with pytest.raises(_lib.PaosHipError):
            dev.detector_add([1e-6, 1e-6], [1e-6, 1e-6], [1.0, 1.0])
        chain = syn20_chain()
        chain[20] = dict(chain[20], save=False)
        with pytest.raises(ValueError):
            run_batch(1.0, [syn20_wavelength(0)] * 2, 64, 4, ON_AXIS, [chain] * 2, outputs=(), dev=dev,
                      detector=Detector(8, 8, 1e-6))
        dev.psf_keep()
        for bad in ([0.0, 1e-6], [float("nan"), 1e-6], [-1e-6, 1e-6]):
            with pytest.raises(_lib.PaosHipError):
                dev.detector_add(bad, [1e-6, 1e-6], [1.0, 1.0])
        with pytest.raises(_lib.PaosHipError):
            dev.detector_add([1e-6, 1e-6], [1e-6, 1e-6], [1.0, float("inf")])
    finally:
        dev.close()
