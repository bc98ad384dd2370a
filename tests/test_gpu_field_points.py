"""Several field points per batch on the GPU, and detector images placed at each item's chief ray
(paos_detector_*_placed).  Off-axis items in production batches (FGS1 at 1024^2 and 4096^2, periscope with its
coordinate breaks) run through the geometry-dependent fast paths -- 2-D box pruning, record windows, the start box, twins,
one-line workgroups -- that on-axis batches alone never leave centred: every item is compared with the oracle at its own
field point, and with the same item in a batch of its own field point, bit for bit."""
import os

import numpy as np
import pytest

import detector_np
import detector_placed_np
from conftest import l2_rel_err, rel_err

pytestmark = pytest.mark.gpu

LENS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "data", "lens")
SYNTH = {"us": 3.0e-4, "ut": -5.0e-4}
PSF_TOL = 1e-10
DET_TOL = 1e-13


def _lens(name):
    from paos_amd.parse_config import parse_config

    return parse_config(os.path.join(LENS, name + ".ini"))


def _key(f):
    return (float(f["us"]), float(f["ut"]))


def _walk(pup, zoom, n, wls, fl, chains, lean):
    """PSFs at the last surface of one batch, (ordinary: the returned arrays; lean: the kept buffer)."""
    from paos_amd import _lib
    from paos_amd.run import run_batch

    last = list(chains[0].keys())[-1]
    dev = _lib.DeviceFields(n, len(wls))
    try:
        if lean:
            res = run_batch(pup, wls, n, zoom, fl, chains, outputs=(), dev=dev, keep_psf=True)
            psfs = [dev.psf_fetch(i) for i in range(len(wls))]
        else:
            res = run_batch(pup, wls, n, zoom, fl, chains, outputs=("psf",), dev=dev)
            psfs = [r[last]["psf"] for r in res]
    finally:
        dev.close()
    return res, psfs, last


def _mixed_batch_checks(name, n, fl, wl_idx, lean, oracle_items):
    """One batch with per-item fields: every item equals the same item in a batch of its field point alone (bit for bit)
    and, for the items named, the oracle at its field point (the parity gate)."""
    from oracle.run_np import run as oracle_run

    pup, par, wls, fields, chains = _lens(name)
    zoom = par["zoom"]
    wl = [1e-6 * wls[k] for k in wl_idx]
    ch = [chains[k] for k in wl_idx]
    res, psfs, last = _walk(pup, zoom, n, wl, fl, ch, lean)
    for f in {_key(f) for f in fl}:
        idx = [i for i in range(len(fl)) if _key(fl[i]) == f]
        _, alone, _ = _walk(pup, zoom, n, [wl[i] for i in idx], {"us": f[0], "ut": f[1]}, [ch[i] for i in idx], lean)
        for j, i in enumerate(idx):
            assert np.array_equal(psfs[i], alone[j]), (name, n, lean, i, f)
        del alone
    for i in oracle_items:
        ref = oracle_run(pup, wl[i], n, zoom, fl[i], ch[i], light=True)[last]
        want = np.abs(ref["wfo"]) ** 2
        e, e2 = rel_err(psfs[i], want), l2_rel_err(psfs[i], want)
        assert e < PSF_TOL and e2 < PSF_TOL, (name, n, lean, i, e, e2)
        assert res[i][last]["dx"] == ref["dx"] and res[i][last]["dy"] == ref["dy"]
    return psfs


@pytest.mark.parametrize("lean", [False, True], ids=["ordinary", "lean"])
def test_fgs1_1024_eight_items_three_field_points(lean):
    _, _, wls, fields, _ = _lens("Ariel_FGS-FGS1")
    fl = [fields[0], fields[1], SYNTH, fields[1], fields[0], SYNTH, fields[1], fields[0]]
    wl_idx = [k % len(wls) for k in range(8)]
    _mixed_batch_checks("Ariel_FGS-FGS1", 1024, fl, wl_idx, lean, range(8))


def test_fgs1_4096_32_items_two_field_points():
    """16 f1 + 16 f2 at the headline shape (lean walk, kept PSFs): bit equality for every item; the oracle for one item
    per field point (about 47 s per wavefront)."""
    _, _, wls, fields, _ = _lens("Ariel_FGS-FGS1")
    fl = [fields[i % 2] for i in range(32)]
    wl_idx = [(i // 2) % len(wls) for i in range(32)]
    _mixed_batch_checks("Ariel_FGS-FGS1", 4096, fl, wl_idx, True, [0, 1])


def test_periscope_1024_two_field_points():
    _, _, wls, fields, _ = _lens("periscope")
    fl = [fields[0], fields[1], fields[1], fields[0]]
    _mixed_batch_checks("periscope", 1024, fl, [0, 0, 1, 1], False, range(4))


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("n", [256, 1024, 4096])
def test_placed_detector_kernels_match_the_restatement(n, precision):
    from paos_amd import _lib
    from test_gpu_detector import DX0, _geometries, _random_psfs

    dev = _lib.DeviceFields(n, 3, precision)
    try:
        psfs = _random_psfs(dev, n + 1)
        dxs = DX0 * np.array([1.0, 1.37, 1.9])
        dys = 1.1 * dxs
        zero = np.zeros((3, 2))
        for det in _geometries(n):
            dev.detector_begin(det)
            # zero offsets: the unplaced kernels, bit for bit
            assert np.array_equal(dev.detector_images(dxs, dys, origins=zero), dev.detector_images(dxs, dys))
            for org in (np.array([[0.3, -0.3], [-0.3, 0.3], [0.3, 0.3]]) * np.stack([dxs, dys], 1),  # +-0.3 grid pixel
                        np.array([[3.0, -2.0], [-5.0, 4.0], [7.0, 1.0]]) * [det.pitch_x, det.pitch_y]):  # detector pixels
                got = dev.detector_images(dxs, dys, origins=org)
                for i in range(3):
                    want = detector_placed_np.rebin_placed(psfs[i], det, dxs[i], dys[i], *org[i])
                    if not want.any():
                        assert not got[i].any()
                        continue
                    e, e2 = rel_err(got[i], want), l2_rel_err(got[i], want)
                    assert e < DET_TOL and e2 < DET_TOL, (det, i, e, e2)
        # accumulation: one add, or the items added one call at a time, or with zero offsets vs unplaced: the same bits
        det = _geometries(n)[1]
        org = np.array([[0.3, -0.3], [-2.0, 1.0], [0.0, 5.0]]) * np.stack([dxs, dys], 1)
        w = np.array([0.5, 1.25, 2.0])
        dev.detector_begin(det)
        dev.detector_add(dxs, dys, w, origins=org)
        whole = dev.detector_fetch()
        dev.detector_begin(det)
        for i in range(3):
            dev.detector_add(dxs, dys, np.where(np.arange(3) == i, w, 0.0), origins=org)
        assert np.array_equal(dev.detector_fetch(), whole)
        want = detector_np.accumulate([detector_placed_np.rebin_placed(psfs[i], det, dxs[i], dys[i], *org[i])
                                       for i in range(3)], w)
        assert rel_err(whole, want) < DET_TOL
        dev.detector_begin(det)
        dev.detector_add(dxs, dys, w, origins=np.zeros((3, 2)))
        a = dev.detector_fetch()
        dev.detector_begin(det)
        dev.detector_add(dxs, dys, w)
        assert np.array_equal(a, dev.detector_fetch())
        # a footprint that misses the detector adds exact zeros; a non-finite origin is refused
        far = np.array([[1.0, 0.0]] * 3) * (4 * n * DX0 + 2 * det.nx * det.pitch_x)
        assert not dev.detector_images(dxs, dys, origins=far).any()
        for bad in (float("nan"), float("inf")):
            with pytest.raises(_lib.PaosHipError):
                dev.detector_add(dxs, dys, w, origins=np.array([[0.0, 0.0], [bad, 0.0], [0.0, 0.0]]))
            with pytest.raises(_lib.PaosHipError):
                dev.detector_images(dxs, dys, origins=np.array([[0.0, bad]] * 3))
    finally:
        dev.close()


def test_airs_ch0_broadband_at_the_chief_rays_against_the_oracle():
    """AIRS-CH0, f1 and f2 over its four wavelengths, run_broadband(..., detector_origin="chief_ray") end to end: the
    oracle's PSFs placed at the raytrace's chief rays through the placed restatement."""
    from oracle.run_np import run as oracle_run
    from paos_amd.detector import Detector, run_broadband
    from paos_amd.raytrace import trace

    pup, par, wls, fields, chains = _lens("Ariel_AIRS-CH0")
    n, zoom = 512, par["zoom"]
    fl = [fields[0]] * len(wls) + [fields[1]] * len(wls)
    wl = [1e-6 * w for w in wls] * 2
    ch = list(chains) * 2
    weights = np.linspace(0.5, 1.5, len(wl))
    last = list(ch[0].keys())[-1]
    refs = [oracle_run(pup, wl[i], n, zoom, fl[i], ch[i], light=True)[last] for i in range(len(wl))]
    org = np.array([[float(r[3][0]), float(r[2][0])] for r in (list(trace(f, c))[-2] for f, c in zip(fl, ch))])
    mid = 0.5 * (org[0] + org[-1])
    dxm = refs[len(wls) // 2]["dx"]
    det = Detector(96, 96, 2.0 * dxm, 2.0 * dxm, xc=float(mid[0]) + 0.3 * dxm, yc=float(mid[1]) - 0.2 * dxm)
    got = run_broadband(pup, wl, weights, n, zoom, fl, ch, det, batch=3, detector_origin="chief_ray")
    want = detector_np.accumulate([detector_placed_np.rebin_placed(np.abs(r["wfo"]) ** 2, det, r["dx"], r["dy"], *org[i])
                                   for i, r in enumerate(refs)], weights)
    assert want.max() > 0.0
    e, e2 = rel_err(got["image"], want), l2_rel_err(got["image"], want)
    assert e < PSF_TOL and e2 < PSF_TOL, (e, e2)
