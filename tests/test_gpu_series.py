"""Pointing series on the GPU (include/paos_hip.h, paos_series_*): every frame against ``detector_images`` placed where
the frame's grid centre lies, bit for bit, and against the NumPy restatement of the definition within the tolerance of
tests/test_gpu_detector.py; every flux against the lane-and-tree restatement on the fetched frames, bit for bit, and
against the long-double sum within the project's bound for metric sums; chunking, repetition, batch independence, the
context's own detector state, ``run_batch`` end to end and every refusal of the C calls.

Shapes: N = 64 with a batch of 3 in an fp64 and an fp32 context, and one fp64 context at N = 1024.  The blocked layout of
fp32 fields changes its block height at N = 2048 only (csrc/host.h, block_rows), so there is no further fp32 context."""
import ctypes
import os

import numpy as np
import pytest

import energy_np
import series_np as snp
from conftest import l2_rel_err, rel_err

pytestmark = pytest.mark.gpu

TOL = 1.0e-13  # tests/test_gpu_detector.py
DX0 = 1.0e-6
LENS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "data", "lens")
# in a 37 x 29 detector: 1 pixel in the top left corner, 63, 64 and 65 pixels, the whole detector, the right and the bottom edge
BOXES = [(0, 1, 0, 1), (0, 9, 0, 7), (1, 17, 2, 6), (3, 16, 4, 9), (0, 37, 0, 29), (36, 37, 0, 29), (0, 37, 28, 29)]
assert [(b[1] - b[0]) * (b[3] - b[2]) for b in BOXES[:4]] == [1, 63, 64, 65]


def _random_psfs(dev, seed):  # (as tests/test_gpu_detector.py makes them)
    rng = np.random.default_rng(seed)
    for i in range(dev.batch):
        dev.upload(i, rng.standard_normal((dev.n, dev.n)) + 1j * rng.standard_normal((dev.n, dev.n)))
    dev.psf_keep()
    return [dev.psf_fetch(i) for i in range(dev.batch)]


@pytest.fixture(scope="module", params=[(64, "fp64"), (64, "fp32"), (1024, "fp64")], ids=lambda p: f"{p[0]}-{p[1]}")
def ctx(request):
    from paos_amd import _lib

    n, precision = request.param
    dev = _lib.DeviceFields(n, 3, precision)
    psfs = _random_psfs(dev, 25 + n)
    yield dev, psfs
    dev.close()


@pytest.fixture(scope="module")
def small():
    from paos_amd import _lib

    dev = _lib.DeviceFields(64, 3)
    psfs = _random_psfs(dev, 7)
    yield dev, psfs
    dev.close()


def _detector(ratio, nx=37, ny=29):
    from paos_amd.detector import Detector

    return Detector(nx, ny, ratio * DX0, 1.13 * ratio * DX0, xc=0.31 * DX0, yc=-0.77 * DX0)


def _offsets(n, det, per_item):
    """T = 7: none, a fraction of a grid pixel, one detector pitch, a few grid pixels, half off the grid, wholly off the
    grid, and back"""
    span = n * DX0 * 1.9 + det.nx * det.pitch_x + det.ny * det.pitch_y
    one = np.array([[0.0, 0.0], [0.3 * DX0, -0.7 * DX0], [det.pitch_x, 0.0], [-2.5 * DX0, 1.25 * DX0],
                    [0.5 * n * DX0, -0.25 * n * DX0], [span, -span], [-0.11 * DX0, 0.05 * DX0]])
    if not per_item:
        return one
    return np.stack([one, 1.37 * one, -0.61 * one[::-1]])


def _check(dev, psfs, det, dxs, dys, offsets, boxes, response=None, origins=None):
    """one series, every property; returns (frames, flux)"""
    frames = dev.series_compute(det, dxs, dys, offsets, boxes, response=response, origins=origins, frames=True)
    flux = dev.series_fetch()
    nb, nt = dev.batch, offsets.shape[-2]
    assert frames.shape == (nb, nt, det.ny, det.nx) and flux.shape == (nb, nt, len(boxes))
    org = np.zeros((nb, 2)) if origins is None else np.asarray(origins, dtype=np.float64)
    g = 1.0 if response is None else response
    dev.detector_begin(det)
    worst = 0.0
    for t in range(nt):
        o = offsets[:, t] if offsets.ndim == 3 else np.broadcast_to(offsets[t], (nb, 2))
        at = np.array([[snp.placed(org[i, 0], o[i, 0]), snp.placed(org[i, 1], o[i, 1])] for i in range(nb)])
        images = dev.detector_images(dxs, dys, origins=at)
        for i in range(nb):
            assert np.array_equal(frames[i, t], images[i] * g), (t, i)
            want = snp.frame_rebin(psfs[i], det, dxs[i], dys[i], *at[i]) * g
            if want.any():
                e, e2 = rel_err(frames[i, t], want), l2_rel_err(frames[i, t], want)
                assert e < TOL and e2 < TOL, (t, i, e, e2)
            else:
                assert not frames[i, t].any(), (t, i)
            for a, box in enumerate(boxes):
                assert flux[i, t, a] == snp.flux_tree(frames[i, t], box), (t, i, box)
                ref, count, sabs = snp.flux_longdouble(frames[i, t], box)
                err, lim = abs(float(np.longdouble(flux[i, t, a]) - ref)), energy_np.bound(count, sabs)
                assert err <= lim, (t, i, box, err, lim)
                worst = max(worst, err / lim if lim > 0.0 else 0.0)
    print(f"series: n={dev.n} {dev.precision} {det.nx}x{det.ny} T={nt}: worst flux error {worst:.3g} of its bound")
    return frames, flux


@pytest.mark.parametrize("ratio", [0.37, 1.0, 3.7])
def test_frames_and_flux_match_the_definition(ctx, ratio):
    dev, psfs = ctx
    n = dev.n
    det = _detector(ratio)
    dxs = DX0 * np.array([1.0, 1.37, 1.9])
    dys = 1.1 * dxs  # dx != dy
    rng = np.random.default_rng(3)
    gains = 1.0 + 0.1 * rng.standard_normal((det.ny, det.nx))
    origins = DX0 * np.array([[0.0, 0.0], [1.5, -2.25], [-0.4, 0.9]])
    frames, _ = _check(dev, psfs, det, dxs, dys, _offsets(n, det, per_item=True), BOXES, response=gains, origins=origins)
    assert not frames[0, 5].any() and not frames[1, 5].any() and not frames[2, 1].any()  # wholly off the grid: exact zeros
    assert frames[0, 4].any() and not frames[0, 4].all()  # half off the grid
    if dev.n == 1024:  # (the large grid runs the per-item series only)
        return
    # shared offsets, no response, no origins
    _check(dev, psfs, det, dxs, dys, _offsets(n, det, per_item=False), BOXES)
    # T = 1 with a zero offset: the unplaced images
    frames = dev.series_compute(det, dxs, dys, np.zeros((1, 2)), BOXES[:1], frames=True)
    dev.detector_begin(det)
    assert np.array_equal(frames[:, 0], dev.detector_images(dxs, dys))


def test_a_one_pixel_detector(ctx):
    from paos_amd.detector import Detector

    dev, psfs = ctx
    det = Detector(1, 1, 5.3 * DX0, 2.9 * DX0, xc=0.2 * DX0, yc=0.1 * DX0)
    dxs = DX0 * np.array([1.0, 1.37, 1.9])
    frames, flux = _check(dev, psfs, det, dxs, 1.1 * dxs, _offsets(dev.n, det, per_item=False), [(0, 1, 0, 1)])
    assert np.array_equal(flux[:, :, 0], frames[:, :, 0, 0])  # one pixel: the flux is the pixel (+0.0 + x)


def test_chunks_repeats_and_frames_off(small, monkeypatch):
    dev, psfs = small
    det = _detector(1.7)
    dxs = DX0 * np.array([1.0, 1.37, 1.9])
    dys = 1.1 * dxs
    off = _offsets(dev.n, det, per_item=True)
    rng = np.random.default_rng(5)
    gains = 1.0 + 0.1 * rng.standard_normal((det.ny, det.nx))
    monkeypatch.delenv("PAOS_SERIES_SCRATCH_BYTES", raising=False)
    frames, flux = _check(dev, psfs, det, dxs, dys, off, BOXES, response=gains)
    # the same call again
    again = dev.series_compute(det, dxs, dys, off, BOXES, response=gains, frames=True)
    assert np.array_equal(again, frames) and np.array_equal(dev.series_fetch(), flux)
    # flux without frames: enqueued only, one copy
    assert dev.series_compute(det, dxs, dys, off, BOXES, response=gains) is None
    assert np.array_equal(dev.series_fetch(), flux)
    # T = 7 in chunks of 1, 2 and 3 frames of every item (the last chunk uneven), and -- where a frame of every item does
    # not fit -- in chunks of one frame of 1 and of 2 items
    one = det.nx * det.ny * 8
    for cap in (3 * one, 2 * 3 * one, 3 * 3 * one + 8, one, 2 * one, 1):
        monkeypatch.setenv("PAOS_SERIES_SCRATCH_BYTES", str(cap))
        got = dev.series_compute(det, dxs, dys, off, BOXES, response=gains, frames=True)
        assert np.array_equal(got, frames), cap
        assert np.array_equal(dev.series_fetch(), flux), cap
        assert dev.series_compute(det, dxs, dys, off, BOXES, response=gains) is None
        assert np.array_equal(dev.series_fetch(), flux), cap
    monkeypatch.delenv("PAOS_SERIES_SCRATCH_BYTES")


def test_an_item_does_not_depend_on_its_batch(small):
    from paos_amd import _lib

    dev, psfs = small
    det = _detector(1.7)
    dxs = DX0 * np.array([1.0, 1.37, 1.9])
    dys = 1.1 * dxs
    off = _offsets(dev.n, det, per_item=True)
    frames = dev.series_compute(det, dxs, dys, off, BOXES, frames=True)
    flux = dev.series_fetch()
    single = _lib.DeviceFields(dev.n, 1)
    try:
        rng = np.random.default_rng(7)  # (the fields of the fixture, in its order)
        for i in range(3):
            single.upload(0, rng.standard_normal((dev.n, dev.n)) + 1j * rng.standard_normal((dev.n, dev.n)))
            single.psf_keep()
            assert np.array_equal(single.psf_fetch(0), psfs[i])
            # alone, with only the box it shares with nobody, and its own offsets
            got = single.series_compute(det, dxs[i], dys[i], off[i:i + 1], BOXES[3:4], frames=True)
            assert np.array_equal(got[0], frames[i]), i
            assert np.array_equal(single.series_fetch()[0, :, 0], flux[i, :, 3]), i
    finally:
        single.close()


def test_the_contexts_detector_is_left_alone(small):
    from paos_amd.detector import Detector

    dev, psfs = small
    mine = Detector(21, 17, 1.9 * DX0, xc=0.2 * DX0)
    dxs = DX0 * np.array([1.0, 1.37, 1.9])
    dev.detector_begin(mine)
    dev.detector_add(dxs, dxs, [0.5, 1.5, 2.5])
    before, images = dev.detector_fetch(), dev.detector_images(dxs, dxs)
    assert before.any()
    det = _detector(3.7)
    dev.series_compute(det, dxs, 1.1 * dxs, _offsets(dev.n, det, per_item=False), BOXES, frames=True)
    dev.series_fetch()
    assert dev.detector is mine
    assert np.array_equal(dev.detector_fetch(), before) and np.array_equal(dev.detector_images(dxs, dxs), images)
    dev.detector_add(dxs, dxs, [0.0, 0.0, 0.0])  # the accumulator is still the one that was begun
    assert np.array_equal(dev.detector_fetch(), before)


def test_run_batch_end_to_end():
    from paos_amd import Detector, PointingSeries, _lib, run_batch
    from paos_amd.parse_config import parse_config

    n = 64
    pup, par, wls, fields, chains = parse_config(os.path.join(LENS, "Hubble_simple.ini"))
    wl = [1e-6 * wls[0], 1.3e-6 * wls[0]]
    chain = chains[0]
    last = chain[list(chain.keys())[-1]]["num"]
    dev = _lib.DeviceFields(n, 2)
    try:
        plain = run_batch(pup, wl, n, par["zoom"], fields[0], [chain, chain], outputs=(), dev=dev, keep_psf=True)
        dx, dy = plain[0][last]["dx"], plain[0][last]["dy"]
        det = Detector(9, 7, 2.3 * dx, 1.9 * dy, xc=0.2 * dx, yc=-0.4 * dy)
        off = np.array([[0.0, 0.0], [0.7 * dx, -1.3 * dy], [det.pitch_x, det.pitch_y]])
        boxes = [(0, 9, 0, 7), (3, 6, 2, 5)]
        gains = 1.0 + 0.05 * np.random.default_rng(1).standard_normal((7, 9))
        ps = PointingSeries(det, off, apertures=boxes, response=gains, frames=True)
        res = run_batch(pup, wl, n, par["zoom"], fields[0], [chain, chain], outputs=(), dev=dev, pointing=ps)
        for i in range(2):
            rec, psf = res[i][last], dev.psf_fetch(i)
            assert sorted(set(rec) - {"series_flux", "series_frames", "series_offsets"}) == sorted(plain[i][last])
            assert rec["power"] == plain[i][last]["power"]
            assert rec["series_frames"].shape == (3, 7, 9) and rec["series_flux"].shape == (3, 2)
            assert np.array_equal(rec["series_offsets"], off)
            for t in range(3):
                want = snp.frame_loop(psf, det, rec["dx"], rec["dy"], off[t, 0], off[t, 1], gains)
                assert want.any() and np.array_equal(rec["series_frames"][t], want), (i, t)
                for a, box in enumerate(boxes):
                    assert rec["series_flux"][t, a] == snp.flux_tree(want, box)
    finally:
        dev.close()


def _raw(dev, geom, per_item, offsets, frames, per_item_offsets, boxes, nboxes, response, host):
    from paos_amd import _lib

    def dbl(a):
        return None if a is None else a.ctypes.data_as(_lib._dbl_p)

    ints = None if boxes is None else boxes.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    return dev._lib.paos_series_compute(dev._ctx, dbl(geom), dbl(per_item), dbl(offsets), frames, per_item_offsets, ints,
                                        nboxes, dbl(response), dbl(host))


def test_the_c_calls_refuse_misuse_and_the_context_stays_usable():
    from paos_amd import _lib

    n, inf, nan = 64, float("inf"), float("nan")
    dev = _lib.DeviceFields(n, 2)
    try:
        geom = np.array([9.0, 7.0, 2.0 * DX0, 2.0 * DX0, 0.0, 0.0])
        items = np.array([[DX0, DX0, 0.0, 0.0], [1.5 * DX0, DX0, DX0, -DX0]])
        off = np.array([[0.0, 0.0], [DX0, -DX0]])
        boxes = np.array([[0, 9, 0, 7], [2, 3, 4, 5]], dtype=np.int32)
        host = np.full((2, 2, 7, 9), -1.0)
        flux = np.full((2, 2, 2), -1.0)
        good = dict(geom=geom, per_item=items, offsets=off, frames=2, per_item_offsets=0, boxes=boxes, nboxes=2, response=None,
                    host=host)
        assert _raw(dev, **good) == 1 and "no PSF kept" in dev._lib.paos_last_error(dev._ctx).decode()  # before a PSF is kept
        assert dev._lib.paos_series_fetch(dev._ctx, flux.ctypes.data_as(_lib._dbl_p)) == 1  # before a compute
        psfs = _random_psfs(dev, 1)

        def changed(name, index, value):
            a = good[name].copy()
            a[index] = value
            return {name: a}

        bad = [dict(geom=None), dict(per_item=None), dict(offsets=None),
               changed("geom", 0, 0.0), changed("geom", 0, 4097.0), changed("geom", 1, 2.5), changed("geom", 2, 0.0),
               changed("geom", 3, -1.0), changed("geom", 3, inf), changed("geom", 4, nan), changed("geom", 5, inf),
               changed("per_item", (0, 0), 0.0), changed("per_item", (1, 1), -DX0), changed("per_item", (1, 0), nan),
               changed("per_item", (0, 1), inf), changed("per_item", (1, 2), inf), changed("per_item", (0, 3), nan),
               changed("offsets", (1, 0), nan), changed("offsets", (0, 1), -inf),
               dict(**changed("per_item", (1, 2), 1.7e308), **changed("offsets", (1, 0), 1.7e308)),  # x0 + ox overflows
               dict(**changed("geom", 4, -1.7e308), **changed("per_item", (0, 2), 1.7e308)),  # xc - X overflows
               dict(frames=0), dict(frames=65537), dict(frames=-1), dict(nboxes=-1), dict(nboxes=17),
               dict(nboxes=0, host=None), dict(boxes=None),
               changed("boxes", (1, 1), 2), changed("boxes", (0, 1), 10), changed("boxes", (0, 0), -1), changed("boxes", (1, 3), 8),
               changed("boxes", (1, 2), 5), dict(response=np.full((7, 9), nan)), dict(response=np.where(np.eye(7, 9) > 0, inf, 1.0))]
        for kw in bad:
            call = dict(good)
            call.update(kw)
            assert _raw(dev, **call) == 1, kw
            assert dev._lib.paos_last_error(dev._ctx).decode().startswith("paos_series_compute: "), kw
            assert np.all(host == -1.0), kw  # nothing touched
        assert dev._lib.paos_series_fetch(dev._ctx, flux.ctypes.data_as(_lib._dbl_p)) == 1  # still before any compute
        # the context is still usable
        assert _raw(dev, **good) == 0
        assert dev._lib.paos_series_fetch(dev._ctx, None) == 1
        assert dev._lib.paos_series_fetch(dev._ctx, flux.ctypes.data_as(_lib._dbl_p)) == 0
        from paos_amd.detector import Detector

        det = Detector(9, 7, 2.0 * DX0)
        for i in range(2):
            for t in range(2):
                want = snp.frame_loop(psfs[i], det, items[i, 0], items[i, 1], snp.placed(items[i, 2], off[t, 0]),
                                      snp.placed(items[i, 3], off[t, 1]))
                assert np.array_equal(host[i, t], want)
                assert flux[i, t, 0] == snp.flux_tree(want, (0, 9, 0, 7)) and flux[i, t, 1] == want[4, 2]
        # a refused call leaves the last result fetchable; frames without boxes leave nothing to fetch
        assert _raw(dev, **dict(good, frames=0)) == 1
        again = np.empty_like(flux)
        assert dev._lib.paos_series_fetch(dev._ctx, again.ctypes.data_as(_lib._dbl_p)) == 0 and np.array_equal(again, flux)
        assert _raw(dev, **dict(good, boxes=None, nboxes=0)) == 0
        assert dev._lib.paos_series_fetch(dev._ctx, again.ctypes.data_as(_lib._dbl_p)) == 1
        assert "no boxes" in dev._lib.paos_last_error(dev._ctx).decode()
        with pytest.raises(_lib.PaosHipError):
            dev.series_fetch()
    finally:
        dev.close()
