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


def _partly_on_chains():
    """Stop, lens, a slit at its focus, lens, image plane, for three items whose slits differ: an ellipse, an aperture with
    a NaN radius (the reference applies none), a rectangle.  The slit is saved and a propagation follows it; the pass that
    brings the field to the focus is still open there, so the slits ride on it as its last operator."""
    from paos_amd.abcd import ABCD

    def surface(num, kind, name, thickness=0.0, curvature=0.0, **extra):
        item = {"num": num, "type": kind, "name": name, "is_stop": False, "save": False,
                "ABCDt": ABCD(thickness=thickness, curvature=curvature), "ABCDs": ABCD(thickness=thickness, curvature=curvature)}
        item.update(extra)
        return item

    def aperture(**geo):
        return dict({"shape": "elliptical", "type": "aperture", "xc": 0.0, "yc": 0.0}, **geo)

    slits = [aperture(xrad=3.0e-4, yrad=2.0e-4), aperture(xrad=float("nan"), yrad=2.0e-4),
             aperture(shape="rectangular", xrad=5.0e-4, yrad=3.0e-4)]
    return [{1: surface(1, "Standard", "STOP", is_stop=True, save=True, aperture=aperture(xrad=0.5, yrad=0.5)),
             2: surface(2, "Paraxial Lens", "L1", thickness=10.0, curvature=0.1),
             3: surface(3, "Standard", "SLIT", thickness=10.0, save=True, aperture=slit),
             4: surface(4, "Paraxial Lens", "L2", thickness=10.0, curvature=0.1),
             5: surface(5, "Standard", "IMAGE_PLANE", save=True)} for slit in slits]


def test_one_surface_with_an_ellipse_no_aperture_and_a_rectangle():
    """1024^2 fp64 is the smallest grid at which apertures ride on a pass as line records.  Three items whose apertures at
    one surface are an ellipse, none (a NaN radius) and a rectangle share every launch: each item's fields equal those of
    the same item run alone, bit for bit, and the lean walk reports the ordinary walk's powers -- both are fp64 sums of
    the same 2^20 non-negative terms, associated differently by the two reductions (trees of depth ~20: a few 1e-15
    relative each), so 1e-13 relative, the bound the lean walk has been held to since it exists (test_gpu_r3.py)."""
    from paos_amd import _lib
    from paos_amd.run import run_batch

    n, on_axis = 1024, {"us": 0.0, "ut": 0.0}
    chains = _partly_on_chains()
    wls = [1.0e-6, 1.1e-6, 1.2e-6]
    stats = {}
    whole = run_batch(1.0, wls, n, 4, on_axis, chains, outputs=("wfo",), stats=stats)
    for i in range(3):
        own = {}
        alone = run_batch(1.0, [wls[i]], n, 4, on_axis, [chains[i]], outputs=("wfo",), stats=own)[0]
        assert sorted(alone) == sorted(whole[i]) == [1, 3, 5] and own == stats
        for k in alone:
            assert np.array_equal(alone[k]["wfo"], whole[i][k]["wfo"]), (i, k)
            assert alone[k]["power"] == whole[i][k]["power"], (i, k)
        assert np.abs(whole[i][5]["wfo"]).max() > 0.0
    # the three slits did three different things: the one that is off passes everything
    passed = [whole[i][3]["power"] / whole[i][1]["power"] for i in range(3)]
    assert passed[0] < 0.999 and passed[2] < 0.999 and passed[0] != passed[2] and abs(passed[1] - 1.0) < 1e-12
    dev = _lib.DeviceFields(n, 3)
    try:
        lean = run_batch(1.0, wls, n, 4, on_axis, chains, outputs=(), dev=dev, keep_psf=True)
        for i in range(3):
            for k in (1, 3, 5):
                print(f"item {i} surface {k}: lean power {lean[i][k]['power']!r}, ordinary {whole[i][k]['power']!r}")
                assert abs(lean[i][k]["power"] - whole[i][k]["power"]) <= 1e-13 * whole[i][k]["power"], (i, k)
    finally:
        dev.close()
