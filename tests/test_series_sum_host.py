"""Broadband series without a GPU (README.md, "Broadband series"): the fold of the definition (tests/series_sum_np.py)
against the long-double weighted sum of matrix-product frames, its consequences bit for bit (a single item, batch splits,
per-frame weights, a NaN item of weight 0), ``run_batch(pointing_weights=...)`` and ``run_broadband_series(pointing=...)`` on the
NumPy model of the device against the fold over the oracle's PSFs -- plus every refusal."""
import os

import numpy as np
import pytest

import series_np as snp
import series_sum_np as ssnp
from oracle.run_np import run as oracle_run
from paos_amd import _lib
from paos_amd.chains import syn20_chain, syn20_wavelength
from paos_amd.detector import Detector, run_broadband, run_broadband_series
from paos_amd.parse_config import parse_config
from paos_amd.run import run_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENS = os.path.join(ROOT, "data", "lens")
FIELD = {"us": 0.0, "ut": 0.0}
TOL = 1.0e-13  # tests/test_series_host.py: frame_loop against frame_rebin, max-norm relative to max |frame_rebin|
PSF_TOL = 1.0e-10  # tests/test_series_host.py: a frame of run_batch's PSF against the oracle's, relative to the PSF's power
EPS = 2.0**-53
DX0 = 1.0e-6


def _last_num(chain):
    return chain[list(chain.keys())[-1]]["num"]


def _random_psf(n, seed):
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    return u.real**2 + u.imag**2


@pytest.fixture(scope="module")
def five():
    """5 items at N = 32 on a 9 x 7 detector, T = 3, per-item offsets and origins: (psfs, det, dxs, dys, off, org, frames)"""
    n, nb = 32, 5
    psfs = [_random_psf(n, 40 + i) for i in range(nb)]
    det = Detector(9, 7, 2.3 * DX0, 1.9 * DX0, xc=0.2 * DX0, yc=-0.4 * DX0)
    dxs = DX0 * np.linspace(1.0, 1.6, nb)
    dys = 1.1 * dxs
    one = np.array([[0.0, 0.0], [0.7 * DX0, -1.3 * DX0], [det.pitch_x, -det.pitch_y]])
    off = np.stack([(1.0 + 0.3 * i) * one for i in range(nb)])
    org = DX0 * np.array([[0.3 * i, -0.2 * i] for i in range(nb)])
    frames = np.array([ssnp.item_frames(psfs[i], det, dxs[i], dys[i], off[i], org[i]) for i in range(nb)])
    return psfs, det, dxs, dys, off, org, frames


W5 = np.array([0.7, -1.3, 2.5, 0.4, -0.05])


def _zero(det, nt=3):
    return np.zeros((nt, det.ny, det.nx))


# ---- the definition ---------------------------------------------------------------------------------------------------
def test_fold_against_the_long_double_sum_of_matrix_product_frames(five):
    psfs, det, dxs, dys, off, org, frames = five
    nb = len(psfs)
    got = ssnp.add(_zero(det), psfs, det, dxs, dys, W5, off, org)
    assert np.array_equal(got, ssnp.fold(_zero(det), frames, W5))
    rebin = np.array([ssnp.item_frames(psfs[i], det, dxs[i], dys[i], off[i], org[i], frame=snp.frame_rebin) for i in range(nb)])
    want, _ = ssnp.sum_longdouble(rebin, W5)
    _, sabs = ssnp.sum_longdouble(frames, W5)
    # B products and B sums, each rounded once: (B + 1) 2^-53 sum_i |w_i F_i| to first order; and every F_i may differ from
    # its matrix-product restatement by TOL max |F_i| (tests/test_series_host.py), which enters weighted by |w_i|
    orders = sum(abs(W5[i]) * TOL * np.max(np.abs(rebin[i]), axis=(1, 2)) for i in range(nb))  # (T,)
    lim = (nb + 1) * EPS * sabs.astype(np.float64) + orders[:, None, None]
    err = np.abs(got.astype(ssnp.LDR) - want).astype(np.float64)
    assert want.any() and np.all(err <= lim), float(np.max(err / lim))


def test_a_single_item_of_weight_one_is_the_per_item_series(five):
    psfs, det, dxs, dys, off, org, frames = five
    for i in (0, 3):
        got = ssnp.add(_zero(det), [psfs[i]], det, dxs[i], dys[i], [1.0], off[i], org[i:i + 1])
        per_item, _ = snp.series([psfs[i]], det, [dxs[i]], [dys[i]], off[i], [(0, 9, 0, 7)], origins=org[i:i + 1])
        assert np.array_equal(got, per_item[0])


def test_splitting_a_sweep_into_adds_changes_no_bit(five):
    psfs, det, dxs, dys, off, org, frames = five
    whole = ssnp.add(_zero(det), psfs, det, dxs, dys, W5, off, org)
    for cuts in ([(0, 2), (2, 4), (4, 5)], [(i, i + 1) for i in range(5)]):
        acc = _zero(det)
        for a, b in cuts:
            acc = ssnp.add(acc, psfs[a:b], det, dxs[a:b], dys[a:b], W5[a:b], off[a:b], org[a:b])
        assert np.array_equal(acc, whole), cuts
    # the weight-0 padding of a short last block adds nothing: its last item again, at weight 0
    acc = ssnp.add(_zero(det), psfs[:3], det, dxs[:3], dys[:3], W5[:3], off[:3], org[:3])
    pad = [3, 4, 4]
    acc = ssnp.add(acc, [psfs[i] for i in pad], det, dxs[pad], dys[pad], [W5[3], W5[4], 0.0], off[pad], org[pad])
    assert np.array_equal(acc, whole)


def test_per_frame_weights_are_separate_sums_per_frame(five):
    psfs, det, dxs, dys, off, org, frames = five
    wbt = np.random.default_rng(8).standard_normal((5, 3))
    wbt[1, 2] = 0.0
    got = ssnp.add(_zero(det), psfs, det, dxs, dys, wbt, off, org)
    for t in range(3):
        alone = ssnp.add(_zero(det), psfs, det, dxs, dys, wbt[:, t], off, org)
        assert np.array_equal(got[t], alone[t]), t


def test_a_nan_item_of_weight_zero_leaves_the_sum_finite(five):
    psfs, det, dxs, dys, off, org, frames = five
    bad = [p.copy() for p in psfs]
    bad[2][:] = np.nan
    w = W5.copy()
    w[2] = 0.0
    got = ssnp.add(_zero(det), bad, det, dxs, dys, w, off, org)
    keep = [0, 1, 3, 4]
    want = ssnp.add(_zero(det), [psfs[i] for i in keep], det, dxs[keep], dys[keep], w[keep], off[keep], org[keep])
    assert np.all(np.isfinite(got)) and np.array_equal(got, want)
    # one frame's weight only
    wbt = np.repeat(W5[:, None], 3, axis=1)
    wbt[2, 1] = 0.0
    part = ssnp.add(_zero(det), bad, det, dxs, dys, wbt, off, org)
    assert np.all(np.isfinite(part[1])) and np.array_equal(part[1], want[1]) and np.all(np.isnan(part[0]))


# ---- PointingSeries.take --------------------------------------------------------------------------------------------------
def test_take_slices_what_is_per_item():
    from paos_amd import PointingSeries

    det = Detector(9, 7, 2.0e-6)
    off = np.arange(5 * 3 * 2, dtype=np.float64).reshape(5, 3, 2) * 1e-7
    org = np.arange(10, dtype=np.float64).reshape(5, 2) * 1e-7
    ps = PointingSeries(det, off, apertures=[(0, 9, 0, 7)], origin=org, response=np.ones((7, 9)))
    part = ps.take([3, 4, 4])
    assert np.array_equal(part.offsets, off[[3, 4, 4]]) and np.array_equal(part.origins, org[[3, 4, 4]])
    assert part.detector is det and part.apertures == ps.apertures and part.response is ps.response
    assert ps.offsets.shape == (5, 3, 2) and ps.origins.shape == (5, 2)  # the series itself is as it was
    part.check(3, 64)
    shared = PointingSeries(det, off[0], frames=True, origin="chief_ray").take([1, 2])
    assert shared.offsets.shape == (3, 2) and shared.chief and shared.origins is None


# ---- run_batch and run_broadband_series on the model device --------------------------------------------------------------------
def _case(name):
    """(pupil diameter, zoom, field, wavelengths [m], chain)"""
    if name == "SYN20":
        return 1.0, 4, FIELD, [syn20_wavelength(k) for k in (0, 100, 200, 350, 511)], syn20_chain()
    pup, par, wls, fields, chains = parse_config(os.path.join(LENS, "Hubble_simple.ini"))
    return pup, par["zoom"], fields[0], [s * 1e-6 * wls[0] for s in (1.0, 1.1, 1.2, 1.3, 1.4)], chains[0]


class _Kept(ssnp.SeriesSumModelDevice):
    """records every device that a sweep makes"""

    made = []

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        _Kept.made.append(self)


@pytest.mark.parametrize("name", ["Hubble_simple", "SYN20"])
def test_run_batch_and_run_broadband_series_against_the_fold_over_the_oracle_psfs(name, monkeypatch):
    from paos_amd import PointingSeries

    n = 64
    pup, zoom, field, wls, chain = _case(name)
    nw = len(wls)
    num = _last_num(chain)
    refs = [oracle_run(pup, wl, n, zoom, field, chain)[num] for wl in wls]
    psfs = [ref["amplitude"] ** 2 for ref in refs]
    totals = np.array([float(p.sum()) for p in psfs])
    dx, dy = refs[0]["dx"], refs[0]["dy"]
    det = Detector(9, 7, 2.3 * dx, 1.9 * dy, xc=0.2 * dx, yc=-0.4 * dy)
    shared = np.array([[0.0, 0.0], [0.7 * dx, -1.3 * dy], [det.pitch_x, det.pitch_y]])
    per_item = np.stack([(1.0 + 0.5 * i) * shared for i in range(nw)])
    origins = np.array([[0.3 * dx * i, -0.2 * dy * i] for i in range(nw)])
    boxes = [(0, 9, 0, 7), (3, 6, 2, 5), (8, 9, 6, 7)]
    gains = 1.0 + 0.05 * np.random.default_rng(1).standard_normal((7, 9))
    w = np.array([0.7, -1.3, 2.5, 0.4, 0.9])
    wbt = w[:, None] * np.array([1.0, 0.5, -2.0])[None, :]
    dxs, dys = [r["dx"] for r in refs], [r["dy"] for r in refs]

    # run_batch: one add into the caller's device, no record touched, nothing synchronised
    plain = run_batch(pup, wls, n, zoom, field, [chain] * nw, outputs=(), dev=ssnp.SeriesSumModelDevice(n, nw))
    for off, org, ww in ((shared, None, w), (per_item, origins, wbt)):
        ps = PointingSeries(det, off, apertures=boxes, response=gains, origin=org, frames=True)
        dev = ssnp.SeriesSumModelDevice(n, nw)
        res = run_batch(pup, wls, n, zoom, field, [chain] * nw, outputs=(), dev=dev, sync=False, pointing=ps, pointing_weights=ww)
        calls = [what for what, _ in dev.log]
        assert "download" not in calls and calls.count("series_sum_begin") == 1 and calls.count("series_sum_add") == 1
        assert "series_compute" not in calls and "series_fetch" not in calls and dev.detector is None
        assert dev.series_sum == (det, 3)
        for i in range(nw):
            # no record is touched (an unsynchronised call hands out a power ticket in place of the power)
            assert set(res[i][num]) - {"power", "power_ticket"} == set(plain[i][num]) - {"power", "power_ticket"}
        want = ssnp.add(np.zeros((3, 7, 9)), psfs, det, dxs, dys, ww, off, org)
        got = dev.series_sum_fetch()
        # every item's frame may differ by PSF_TOL of its power (tests/test_series_host.py); it enters weighted by |w|
        lim = PSF_TOL * float(np.sum(np.max(np.abs(ssnp.weights_bt(ww, nw, 3)), axis=1) * totals))
        assert want.any() and np.max(np.abs(got - want)) <= lim
        flux = dev.series_sum_flux(boxes, gains)
        for t in range(3):
            for a, box in enumerate(boxes):
                assert flux[t, a] == snp.flux_tree(got[t] * gains, box)
        # a second call on the same device adds into the same sum
        run_batch(pup, wls, n, zoom, field, [chain] * nw, outputs=(), dev=dev, sync=False, pointing=ps, pointing_weights=ww)
        assert [what for what, _ in dev.log].count("series_sum_begin") == 1
        assert np.array_equal(dev.series_sum_fetch(), ssnp.fold(got, _frames_of(dev, det, dxs, dys, off, org), ww))

    # run_broadband_series: blocks of 2 (the last one padded) and of 5 -- equal bits; "image" and "power" as without a series
    monkeypatch.setattr(_lib, "DeviceFields", _Kept)
    for off, org, pw in ((shared, None, None), (per_item, origins, wbt)):
        ps = PointingSeries(det, off, apertures=boxes, response=gains, origin=org, frames=True)
        kw = dict(pointing=ps) if pw is None else dict(pointing=ps, pointing_weights=pw)
        _Kept.made = []
        two = run_broadband_series(pup, wls, w, n, zoom, field, chain, det, batch=2, **kw)
        blocks = [what for what, _ in _Kept.made[0].log]
        assert blocks.count("series_sum_add") == 3 and blocks.count("series_sum_begin") == 1 and "series_compute" not in blocks
        five_ = run_broadband_series(pup, wls, w, n, zoom, field, chain, det, batch=5, **kw)
        bare = run_broadband(pup, wls, w, n, zoom, field, chain, det, batch=2)
        assert set(two) == set(bare) | {"series_flux", "series_frames", "series_offsets"}
        for key in ("series_flux", "series_frames", "series_offsets"):
            assert np.array_equal(two[key], five_[key]), key
        assert np.array_equal(two["image"], bare["image"]) and two["power"] == bare["power"]
        assert np.array_equal(five_["image"], bare["image"])
        assert two["series_flux"].shape == (3, 3) and two["series_frames"].shape == (3, 7, 9)
        assert np.array_equal(two["series_offsets"], off)
        ww = w if pw is None else pw
        want = ssnp.add(np.zeros((3, 7, 9)), psfs, det, dxs, dys, ww, off, org) * gains
        lim = PSF_TOL * float(np.sum(np.max(np.abs(ssnp.weights_bt(ww, nw, 3)), axis=1) * totals)) * float(np.max(np.abs(gains)))
        assert np.max(np.abs(two["series_frames"] - want)) <= lim
        for t in range(3):
            for a, box in enumerate(boxes):
                assert two["series_flux"][t, a] == snp.flux_tree(two["series_frames"][t], box)
    # without frames and without a response; without apertures
    lean = run_broadband_series(pup, wls, w, n, zoom, field, chain, det, batch=2, pointing=PointingSeries(det, shared, apertures=boxes))
    assert "series_frames" not in lean and lean["series_flux"].shape == (3, 3)
    only = run_broadband_series(pup, wls, w, n, zoom, field, chain, det, batch=2, pointing=PointingSeries(det, shared, frames=True))
    assert only["series_flux"].shape == (3, 0)
    for t in range(3):
        for a, box in enumerate(boxes):
            assert lean["series_flux"][t, a] == snp.flux_tree(only["series_frames"][t], box)


def _frames_of(dev, det, dxs, dys, off, org):
    """the frames of the PSFs the model device keeps right now"""
    psf = np.asarray(dev.psf, dtype=np.float64)
    o = np.zeros((dev.batch, 2)) if org is None else org
    return [ssnp.item_frames(psf[i], det, dxs[i], dys[i], off[i] if off.ndim == 3 else off, o[i]) for i in range(dev.batch)]


def test_behind_a_blur_and_at_the_chief_rays():
    from paos_amd import PointingSeries, PsfBlur
    from paos_amd.raytrace import trace

    n, wls = 64, [syn20_wavelength(k) for k in (0, 300)]
    chains = [syn20_chain() for _ in wls]
    ref = oracle_run(1.0, wls[0], n, 4, FIELD, syn20_chain(), light=True)[20]
    dx, dy = ref["dx"], ref["dy"]
    det = Detector(9, 7, 2.3 * dx, 1.9 * dy)
    off = np.array([[0.0, 0.0], [0.7 * dx, -1.3 * dy]])
    ps = PointingSeries(det, off, frames=True)
    w = [0.5, 2.0]
    dev = ssnp.SeriesSumModelDevice(n, 2)
    res = run_batch(1.0, wls, n, 4, FIELD, chains, outputs=(), dev=dev, psf_blur=PsfBlur(2.0 * dx, 1.2 * dy, array=True), pointing=ps,
                    pointing_weights=w)
    calls = [what for what, _ in dev.log]
    assert calls.index("blur_apply") < calls.index("series_sum_add")
    blurred = [res[i][20]["psf_blur"] for i in range(2)]
    want = ssnp.add(np.zeros((2, 7, 9)), blurred, det, [res[i][20]["dx"] for i in range(2)], [res[i][20]["dy"] for i in range(2)], w, off)
    assert np.array_equal(dev.series_sum_fetch(), want)  # (the model adds the very arrays it hands out)
    # origin="chief_ray": resolved where the detector's origins are
    pup, par, fwls, fields, fchains = parse_config(os.path.join(LENS, "Ariel_FGS-FGS1.ini"))
    fl = [fields[0], fields[1], {"us": 3.0e-4, "ut": -5.0e-4}]
    chain = fchains[0]
    det = Detector(16, 12, 1e-6)
    ps = PointingSeries(det, np.array([[0.0, 0.0], [0.5e-6, -0.25e-6]]), frames=True, origin="chief_ray")
    dev = ssnp.SeriesSumModelDevice(n, 3)
    run_batch(pup, [1e-6 * fwls[0]] * 3, n, par["zoom"], fl, [chain] * 3, outputs=(), dev=dev, sync=False, pointing=ps,
              pointing_weights=[1.0, 1.0, 1.0], detector=det, detector_origin="chief_ray")
    origins = dev.sum_seen[-1]
    assert np.array_equal(origins, dev.origins_seen[-1]) and origins[1].any()
    for i, f in enumerate(fl):
        _, _, vt, vs = list(trace(f, chain))[-2]
        assert origins[i].tolist() == [float(vs[0]), float(vt[0])], i


# ---- refusals ---------------------------------------------------------------------------------------------------------
def _refused(**kw):
    n = 64
    dev = kw.pop("dev", ssnp.SeriesSumModelDevice(n, 2))
    with pytest.raises(ValueError) as err:
        run_batch(1.0, [1.0e-6, 1.2e-6], n, 4, FIELD, [syn20_chain(), syn20_chain()], dev=dev, **kw)
    if dev is not None:
        assert dev.log == [] and not dev.u.any(), "something was launched before the refusal"
    return str(err.value)


def test_run_batch_refusals_come_before_any_launch():
    from paos_amd import PointingSeries, PsfBlur

    det = Detector(9, 7, 2.0e-6)
    ps = PointingSeries(det, np.zeros((3, 2)), apertures=[(0, 9, 0, 7)])
    assert "without pointing" in _refused(pointing_weights=[1.0, 1.0])
    assert "dev" in _refused(dev=None, pointing=ps, pointing_weights=[1.0, 1.0])
    for bad in ([1.0], [1.0, 1.0, 1.0], np.ones((2, 2)), np.ones((3, 2)), np.ones((2, 3, 1)), 1.0, "heavy"):
        assert "pointing_weights" in _refused(pointing=ps, pointing_weights=bad)
    for bad in ([1.0, float("nan")], [float("inf"), 1.0], np.where(np.eye(2, 3) > 0, np.nan, 1.0)):
        assert "finite" in _refused(pointing=ps, pointing_weights=bad)
    assert "focus_planes" in _refused(pointing=ps, pointing_weights=[1.0, 1.0], focus_planes=[0.0, 1.0e-4], outputs=("psf",))
    assert "pixel" in _refused(pointing=ps, pointing_weights=[1.0, 1.0], psf_blur=PsfBlur(1.0e-6, 1.0e-6, pixel=(2.0e-6, 2.0e-6)))
    assert "offsets" in _refused(pointing=PointingSeries(det, np.zeros((3, 4, 2)), frames=True), pointing_weights=[1.0, 1.0])
    assert "sync" in _refused(sync=False, pointing=ps)  # (without weights the series still synchronises)
    # what is allowed: sync=False with weights, both weight shapes
    dev = ssnp.SeriesSumModelDevice(64, 2)
    run_batch(1.0, [1.0e-6, 1.2e-6], 64, 4, FIELD, [syn20_chain(), syn20_chain()], dev=dev, outputs=(), sync=False, pointing=ps,
              pointing_weights=np.ones((2, 3)))
    assert dev.series_sum_fetch().any()


def test_run_broadband_series_refusals(monkeypatch):
    from paos_amd import PointingSeries, PsfBlur

    monkeypatch.setattr(_lib, "DeviceFields", _Kept)
    _Kept.made = []
    det = Detector(9, 7, 2.0e-6)
    wls, w = [1.0e-6, 1.1e-6, 1.2e-6], [1.0, 2.0, 3.0]
    ps = PointingSeries(det, np.zeros((4, 2)), apertures=[(0, 9, 0, 7)])
    for kw in (dict(pointing=det), dict(pointing=None, pointing_weights=w), dict(pointing=ps, pointing_weights=[1.0, 2.0]),
               dict(pointing=ps, pointing_weights=np.ones((3, 3))), dict(pointing=ps, pointing_weights=[1.0, 2.0, float("nan")]),
               dict(pointing=PointingSeries(det, np.zeros((2, 4, 2)), frames=True)),
               dict(pointing=PointingSeries(det, np.zeros((4, 2)), frames=True, origin=np.zeros((2, 2)))),
               dict(pointing=ps, psf_blur=PsfBlur(1.0e-6, 1.0e-6, pixel=(2.0e-6, 2.0e-6)))):
        with pytest.raises(ValueError):
            run_broadband_series(1.0, wls, w, 64, 4, FIELD, syn20_chain(), det, batch=2, **kw)
    assert _Kept.made == []  # before a device context is made


def test_the_model_device_refuses_what_the_library_refuses():
    n = 64
    det = Detector(9, 7, 2.0e-6)
    dev = ssnp.SeriesSumModelDevice(n, 2)
    for call in (lambda: dev.series_sum_add(DX0, DX0, [1.0, 1.0], np.zeros((2, 2))), lambda: dev.series_sum_flux([(0, 9, 0, 7)]),
                 dev.series_sum_fetch, lambda: dev.series_sum_begin(det, 0), lambda: dev.series_sum_begin(det, 65537),
                 lambda: dev.series_sum_begin(Detector(64, 64, 2.0e-6), 65536)):
        with pytest.raises(_lib.PaosHipError):
            call()
    assert dev.series_sum is None
    dev.series_sum_begin(det, 2)
    with pytest.raises(_lib.PaosHipError):  # before a PSF is kept
        dev.series_sum_add(DX0, DX0, [1.0, 1.0], np.zeros((2, 2)))
    dev.u[:] = np.sqrt(_random_psf(n, 3))
    dev.psf_keep()
    for kw in (dict(weights=[1.0, np.nan]), dict(offsets=np.full((2, 2), np.inf))):
        call = dict(weights=[1.0, 1.0], offsets=np.zeros((2, 2)))
        call.update(kw)
        with pytest.raises(_lib.PaosHipError):
            dev.series_sum_add(DX0, DX0, **call)
    for boxes, resp in (([], None), ([(0, 1, 0, 1)] * 17, None), ([(0, 10, 0, 7)], None), ([(2, 2, 0, 7)], None),
                        ([(0, 9, 0, 7)], np.full((7, 9), np.inf))):
        with pytest.raises(_lib.PaosHipError):
            dev.series_sum_flux(boxes, resp)
    assert not dev.series_sum_fetch().any()
    dev.series_sum_add(DX0, DX0, [1.0, 1.0], np.zeros((2, 2)))
    assert dev.series_sum_flux([(0, 9, 0, 7)]).shape == (2, 1) and dev.series_sum_fetch().shape == (2, 7, 9)


def test_the_c_calls_refuse_null_contexts():
    lib = _lib.load()
    geom = np.array([9.0, 7.0, 2.0e-6, 2.0e-6, 0.0, 0.0])
    items = np.array([[1.0e-6, 1.0e-6, 0.0, 0.0]])
    off, w = np.zeros((1, 2)), np.ones(1)
    host = np.zeros((1, 7, 9))
    boxes = np.array([[0, 9, 0, 7]], dtype=np.int32)
    p = _lib._dbl_p
    import ctypes

    assert lib.paos_series_sum_begin(None, geom.ctypes.data_as(p), 1) == 1
    assert lib.paos_last_error(None).decode().startswith("paos_series_sum_begin: ")
    assert lib.paos_series_sum_add(None, items.ctypes.data_as(p), off.ctypes.data_as(p), 0, w.ctypes.data_as(p), 0) == 1
    assert lib.paos_last_error(None).decode().startswith("paos_series_sum_add: ")
    assert lib.paos_series_sum_flux(None, boxes.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), 1, None, host.ctypes.data_as(p)) == 1
    assert lib.paos_last_error(None).decode().startswith("paos_series_sum_flux: ")
    assert lib.paos_series_sum_fetch(None, host.ctypes.data_as(p)) == 1
    assert lib.paos_last_error(None).decode().startswith("paos_series_sum_fetch: ")
