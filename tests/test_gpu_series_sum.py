"""Broadband series on the GPU (include/paos_hip.h, paos_series_sum_*): the accumulator against the NumPy fold of the
device's own per-item frames, bit for bit, against the fold of the loop-order restatement, bit for bit, and against the fold
of the matrix-product restatement within the tolerance of tests/test_gpu_series.py; every flux against the lane-and-tree
restatement on ``S g``, bit for bit, and against the long-double sum within the project's bound for metric sums; batch
splits, zero weights and NaN items, small shapes, both frame ranges of T = 65536, the independence of the sum from the
detector and the per-item series, repetition, ``run_broadband_series`` end to end and every refusal of the C calls.

Shapes: N = 64 with a batch of 3 in an fp64 and an fp32 context, and one fp64 context at N = 1024 with a batch of 2 (the
block layout of the PSF buffer differs by grid size)."""
import ctypes
import os

import numpy as np
import pytest

import energy_np
import series_np as snp
import series_sum_np as ssnp
from conftest import l2_rel_err, rel_err

pytestmark = pytest.mark.gpu

TOL = 1.0e-13  # tests/test_gpu_series.py
DX0 = 1.0e-6
LENS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "data", "lens")
BOXES = [(0, 1, 0, 1), (0, 9, 0, 7), (1, 17, 2, 6), (3, 16, 4, 9), (0, 37, 0, 29), (36, 37, 0, 29), (0, 37, 28, 29)]


def _fields(n, count, seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)) for _ in range(count)]


def _keep(dev, fields):  # (random PSFs as tests/test_gpu_series.py makes them)
    for i, u in enumerate(fields):
        dev.upload(i, u)
    dev.psf_keep()
    return [dev.psf_fetch(i) for i in range(dev.batch)]


@pytest.fixture(scope="module", params=[(64, "fp64", 3), (64, "fp32", 3), (1024, "fp64", 2)], ids=lambda p: f"{p[0]}-{p[1]}")
def ctx(request):
    from paos_amd import _lib

    n, precision, batch = request.param
    dev = _lib.DeviceFields(n, batch, precision)
    psfs = _keep(dev, _fields(n, batch, 26 + n))
    yield dev, psfs
    dev.close()


@pytest.fixture(scope="module")
def small():
    from paos_amd import _lib

    dev = _lib.DeviceFields(64, 3)
    psfs = _keep(dev, _fields(64, 3, 9))
    yield dev, psfs
    dev.close()


def _detector(ratio, nx=37, ny=29):
    from paos_amd.detector import Detector

    return Detector(nx, ny, ratio * DX0, 1.13 * ratio * DX0, xc=0.31 * DX0, yc=-0.77 * DX0)


def _offsets(n, det, nb):
    """T = 5 per item: none, a fraction of a grid pixel, one detector pitch, half off the grid, a few grid pixels"""
    one = np.array([[0.0, 0.0], [0.3 * DX0, -0.7 * DX0], [det.pitch_x, 0.0], [0.5 * n * DX0, -0.25 * n * DX0], [-2.5 * DX0, 1.25 * DX0]])
    return np.stack([one, 1.37 * one, -0.61 * one[::-1]][:nb])


def _check(dev, psfs, det, dxs, dys, off, org, weights, boxes, gains):
    """one add on a fresh sum, every property; returns (S, flux)"""
    nb, nt = dev.batch, off.shape[-2]
    per_item = dev.series_compute(det, dxs, dys, off, boxes[:1], origins=org, frames=True)  # no response
    dev.series_sum_begin(det, nt)
    dev.series_sum_add(dxs, dys, weights, off, origins=org)
    got = dev.series_sum_fetch()
    zero = np.zeros((nt, det.ny, det.nx))
    assert got.shape == zero.shape and got.any()
    assert np.array_equal(got, ssnp.fold(zero, per_item, weights))  # the device's own frames, folded by NumPy
    assert np.array_equal(got, ssnp.add(zero, psfs, det, dxs, dys, weights, off, org))  # the loop-order restatement
    want = ssnp.add(zero, psfs, det, dxs, dys, weights, off, org, frame=snp.frame_rebin)
    for t in range(nt):
        e, e2 = rel_err(got[t], want[t]), l2_rel_err(got[t], want[t])
        assert want[t].any() and e < TOL and e2 < TOL, (t, e, e2)
    flux = dev.series_sum_flux(boxes, gains)
    assert flux.shape == (nt, len(boxes))
    seen = got if gains is None else got * gains
    worst = 0.0
    for t in range(nt):
        for a, box in enumerate(boxes):
            assert flux[t, a] == snp.flux_tree(seen[t], box), (t, box)
            ref, count, sabs = snp.flux_longdouble(seen[t], box)
            err, lim = abs(float(np.longdouble(flux[t, a]) - ref)), energy_np.bound(count, sabs)
            assert err <= lim, (t, box, err, lim)
            worst = max(worst, err / lim if lim > 0.0 else 0.0)
    print(f"series sum: n={dev.n} {dev.precision} {det.nx}x{det.ny} T={nt}: worst flux error {worst:.3g} of its bound")
    return got, flux


def test_the_sum_and_its_flux_match_the_definition(ctx):
    dev, psfs = ctx
    nb = dev.batch
    big = dev.n == 1024
    det = _detector(3.7, 64, 64) if big else _detector(1.7)  # 37 x 29 = 1073 pixels: a partial last workgroup
    boxes = [(0, 1, 0, 1), (24, 40, 24, 40), (0, 64, 0, 64), (63, 64, 0, 64)] if big else BOXES
    dxs = DX0 * np.array([1.0, 1.37, 1.9])[:nb]
    dys = 1.1 * dxs  # dx != dy
    off = _offsets(dev.n, det, nb)[:, :3] if big else _offsets(dev.n, det, nb)
    org = DX0 * np.array([[0.0, 0.0], [1.5, -2.25], [-0.4, 0.9]])[:nb]
    gains = 1.0 + 0.1 * np.random.default_rng(3).standard_normal((det.ny, det.nx))
    weights = np.array([0.7, -1.3, 2.5])[:nb]  # mixed signs
    _check(dev, psfs, det, dxs, dys, off, org, weights, boxes, gains)
    if big:
        return
    # per-frame weights with zeros among them, shared offsets, no origins, no response
    wbt = np.random.default_rng(4).standard_normal((nb, 5))
    wbt[1, 2] = wbt[0, 4] = wbt[2, 4] = 0.0
    got, _ = _check(dev, psfs, det, dxs, dys, off[0], None, wbt, boxes, None)
    for t in range(5):  # (B, T) weights: T separate sums of (B,) weights
        dev.series_sum_begin(det, 5)
        dev.series_sum_add(dxs, dys, wbt[:, t].copy(), off[0])
        assert np.array_equal(dev.series_sum_fetch()[t], got[t]), t
    # a single item of weight 1 on a fresh sum: the per-item series
    per_item = dev.series_compute(det, dxs, dys, off, boxes[:1], origins=org, frames=True)
    for i in range(nb):
        dev.series_sum_begin(det, 5)
        dev.series_sum_add(dxs, dys, np.eye(nb)[i], off, origins=org)
        assert np.array_equal(dev.series_sum_fetch(), per_item[i]), i


def test_splitting_a_sweep_into_adds_changes_no_bit():
    from paos_amd import _lib

    n = 64
    fields = _fields(n, 4, 11)
    det = _detector(1.7)
    dxs = DX0 * np.array([1.0, 1.37, 1.9, 1.2])
    dys = 1.1 * dxs
    one = _offsets(n, det, 3)
    off = np.stack([one[0], one[1], one[2], 0.5 * one[1]])
    org = DX0 * np.array([[0.0, 0.0], [1.5, -2.25], [-0.4, 0.9], [0.1, 0.2]])
    w = np.array([0.7, -1.3, 2.5, 0.4])
    whole = _lib.DeviceFields(n, 4)
    try:
        psfs = _keep(whole, fields)
        whole.series_sum_begin(det, 5)
        whole.series_sum_add(dxs, dys, w, off, origins=org)
        want = whole.series_sum_fetch()
        assert np.array_equal(want, ssnp.add(np.zeros((5, 29, 37)), psfs, det, dxs, dys, w, off, org))
    finally:
        whole.close()
    for batch in (2, 1):
        dev = _lib.DeviceFields(n, batch)
        try:
            dev.series_sum_begin(det, 5)
            for b0 in range(0, 4, batch):
                part = slice(b0, b0 + batch)
                assert all(np.array_equal(a, b) for a, b in zip(_keep(dev, fields[part]), psfs[part]))
                dev.series_sum_add(dxs[part], dys[part], w[part], off[part], origins=org[part])  # (enqueued only)
            assert np.array_equal(dev.series_sum_fetch(), want), batch
        finally:
            dev.close()


def test_a_nan_item_of_weight_zero_and_the_padding():
    from paos_amd import _lib

    n = 64
    fields = _fields(n, 3, 12)
    det = _detector(1.7)
    dxs = DX0 * np.array([1.0, 1.37, 1.9])
    off = _offsets(n, det, 3)
    w = np.array([0.7, 0.0, 2.5])
    dev = _lib.DeviceFields(n, 3)
    try:
        _keep(dev, fields)
        dev.series_sum_begin(det, 5)
        dev.series_sum_add(dxs, dxs, w, off)
        clean = dev.series_sum_fetch()
        per_item = dev.series_compute(det, dxs, dxs, off, BOXES[:1], frames=True)
        assert np.array_equal(clean, ssnp.fold(np.zeros_like(clean), [per_item[0], None, per_item[2]], w))  # without that item
        psfs = _keep(dev, [fields[0], np.full((n, n), np.nan + 0j), fields[2]])
        assert np.all(np.isnan(psfs[1]))
        dev.series_sum_begin(det, 5)
        dev.series_sum_add(dxs, dxs, w, off)
        got = dev.series_sum_fetch()
        assert np.all(np.isfinite(got)) and np.array_equal(got, clean)
        # (B, T) weights: the NaN item has weight 0 in frames 1 and 3 only
        wbt = np.repeat(w[:, None], 5, axis=1)
        wbt[1] = [1.0, 0.0, 1.0, 0.0, -1.0]
        dev.series_sum_begin(det, 5)
        dev.series_sum_add(dxs, dxs, wbt, off)
        got = dev.series_sum_fetch()
        assert np.array_equal(got[[1, 3]], clean[[1, 3]]) and np.all(np.isnan(got[[0, 2]]))
        # the padding of a short last block: the last item again at weight 0 adds nothing, and -0.0 is a zero
        _keep(dev, [fields[0], fields[2], fields[2]])
        dev.series_sum_begin(det, 5)
        dev.series_sum_add(dxs[[0, 2, 2]], dxs[[0, 2, 2]], np.array([0.7, 2.5, -0.0]), off[[0, 2, 2]])
        assert np.array_equal(dev.series_sum_fetch(), clean)
    finally:
        dev.close()


def test_small_shapes(small):
    from paos_amd.detector import Detector

    dev, psfs = small
    dxs = DX0 * np.array([1.0, 1.37, 1.9])
    w = np.array([0.7, -1.3, 2.5])
    # a one-pixel detector
    det = Detector(1, 1, 5.3 * DX0, 2.9 * DX0, xc=0.2 * DX0, yc=0.1 * DX0)
    off = _offsets(dev.n, det, 3)
    got, flux = _check(dev, psfs, det, dxs, 1.1 * dxs, off, None, w, [(0, 1, 0, 1)], np.array([[1.25]]))
    assert np.array_equal(flux[:, 0], got[:, 0, 0] * 1.25)  # one pixel: the flux is the pixel (+0.0 + x)
    # a footprint that misses the grid: exact +0.0
    det = _detector(1.7)
    span = dev.n * DX0 * 1.9 + det.nx * det.pitch_x + det.ny * det.pitch_y
    dev.series_sum_begin(det, 2)
    dev.series_sum_add(dxs, dxs, w, np.array([[span, -span], [-span, 0.0]]))
    got = dev.series_sum_fetch()
    assert not got.any() and not np.signbit(got).any()
    assert not dev.series_sum_flux(BOXES).any()


def test_both_frame_ranges_of_the_longest_series():
    from paos_amd import _lib
    from paos_amd.detector import Detector

    n, nt = 64, 65536
    det = Detector(2, 2, 3.1 * DX0, 2.7 * DX0, xc=0.2 * DX0)
    off = 4.0 * DX0 * np.random.default_rng(13).standard_normal((nt, 2))
    dev = _lib.DeviceFields(n, 1)
    try:
        _keep(dev, _fields(n, 1, 13))
        per_item = dev.series_compute(det, DX0, 1.1 * DX0, off, [(0, 2, 0, 2)], frames=True)
        dev.series_sum_begin(det, nt)
        dev.series_sum_add(DX0, 1.1 * DX0, [1.0], off)
        got = dev.series_sum_fetch()
        for t in (0, 32767, 32768, 65535):
            assert got[t].any() and np.array_equal(got[t], per_item[0, t]), t
        assert np.array_equal(got, per_item[0])
        flux = dev.series_sum_flux([(0, 2, 0, 2)])
        assert np.array_equal(flux, dev.series_fetch()[0])  # (the per-item flux of the same frames, no response)
    finally:
        dev.close()


def test_the_sum_the_detector_and_the_per_item_series_leave_each_other_alone(small):
    from paos_amd.detector import Detector

    dev, psfs = small
    mine = Detector(21, 17, 1.9 * DX0, xc=0.2 * DX0)
    dxs = DX0 * np.array([1.0, 1.37, 1.9])
    w = np.array([0.7, -1.3, 2.5])
    dev.detector_begin(mine)
    dev.detector_add(dxs, dxs, [0.5, 1.5, 2.5])
    image = dev.detector_fetch()
    other = _detector(3.7)
    off = _offsets(dev.n, other, 3)
    dev.series_compute(other, dxs, 1.1 * dxs, off, BOXES)
    series = dev.series_fetch()
    assert image.any() and series.any()
    det = _detector(1.7, 19, 23)
    dev.series_sum_begin(det, 5)
    dev.series_sum_add(dxs, dxs, w, off)
    flux = dev.series_sum_flux([(0, 19, 0, 23), (3, 5, 7, 11)], np.full((23, 19), 1.5))
    assert dev.detector is mine and np.array_equal(dev.detector_fetch(), image)
    assert np.array_equal(dev.series_fetch(), series)
    dev.detector_add(dxs, dxs, [0.0, 0.0, 0.0])  # the accumulator is still the one that was begun
    assert np.array_equal(dev.detector_fetch(), image)
    # the reverse: a per-item series and a detector image in between leave S alone
    before = dev.series_sum_fetch()
    dev.series_compute(other, dxs, 1.1 * dxs, off, BOXES, frames=True)
    dev.detector_images(dxs, dxs)
    assert np.array_equal(dev.series_sum_fetch(), before)
    assert np.array_equal(dev.series_sum_flux([(0, 19, 0, 23), (3, 5, 7, 11)], np.full((23, 19), 1.5)), flux)
    # begin again and the same adds: the same bits; two adds stack in order
    dev.series_sum_begin(det, 5)
    assert not dev.series_sum_fetch().any()
    dev.series_sum_add(dxs, dxs, w, off)
    assert np.array_equal(dev.series_sum_fetch(), before)
    dev.series_sum_add(dxs, dxs, -0.5 * w, off)
    per_item = dev.series_compute(det, dxs, dxs, off, frames=True)
    assert np.array_equal(dev.series_sum_fetch(), ssnp.fold(before, per_item, -0.5 * w))


def test_run_broadband_series_end_to_end():
    from paos_amd import Detector, PointingSeries, _lib, run_batch, run_broadband, run_broadband_series
    from paos_amd.parse_config import parse_config

    n = 64
    pup, par, wls0, fields, chains = parse_config(os.path.join(LENS, "Hubble_simple.ini"))
    wls = [s * 1e-6 * wls0[0] for s in (1.0, 1.1, 1.2, 1.3, 1.4)]
    chain = chains[0]
    last = chain[list(chain.keys())[-1]]["num"]
    w = np.array([0.7, 1.3, 2.5, 0.4, 0.9])
    dev = _lib.DeviceFields(n, 2)
    try:
        first = run_batch(pup, wls[:2], n, par["zoom"], fields[0], [chain, chain], outputs=(), dev=dev)
        dx, dy = first[0][last]["dx"], first[0][last]["dy"]
        det = Detector(9, 7, 2.3 * dx, 1.9 * dy, xc=0.2 * dx, yc=-0.4 * dy)
        shared = np.array([[0.0, 0.0], [0.7 * dx, -1.3 * dy], [det.pitch_x, det.pitch_y]])
        off = np.stack([(1.0 + 0.25 * i) * shared for i in range(5)])
        org = np.array([[0.3 * dx * i, -0.2 * dy * i] for i in range(5)])
        boxes = [(0, 9, 0, 7), (3, 6, 2, 5)]
        gains = 1.0 + 0.05 * np.random.default_rng(1).standard_normal((7, 9))
        ps = PointingSeries(det, off, apertures=boxes, response=gains, origin=org, frames=True)
        got = run_broadband_series(pup, wls, w, n, par["zoom"], fields[0], chain, det, batch=2, pointing=ps)
        bare = run_broadband(pup, wls, w, n, par["zoom"], fields[0], chain, det, batch=2)
        assert np.array_equal(got["image"], bare["image"]) and got["power"] == bare["power"]
        # the per-item frames of run_batch(pointing=...) over the same blocks, folded by NumPy
        acc = np.zeros((3, 7, 9))
        for idx in ([0, 1], [2, 3], [4, 4]):
            one = PointingSeries(det, off[idx], origin=org[idx], frames=True)
            res = run_batch(pup, [wls[i] for i in idx], n, par["zoom"], fields[0], [chain, chain], outputs=(), dev=dev, pointing=one)
            wb = w[idx] if idx != [4, 4] else np.array([w[4], 0.0])
            acc = ssnp.fold(acc, [res[k][last]["series_frames"] for k in range(2)], wb)
        assert acc.any() and np.array_equal(got["series_frames"], acc * gains)
        assert np.array_equal(got["series_offsets"], off)
        for t in range(3):
            for a, box in enumerate(boxes):
                assert got["series_flux"][t, a] == snp.flux_tree(acc[t] * gains, box)
    finally:
        dev.close()


def _dbl(a):
    from paos_amd import _lib

    return None if a is None else a.ctypes.data_as(_lib._dbl_p)


def _ints(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


def test_the_c_calls_refuse_misuse_and_the_context_stays_usable():
    from paos_amd import _lib
    from paos_amd.detector import Detector

    n, inf, nan = 64, float("inf"), float("nan")
    dev = _lib.DeviceFields(n, 2)
    lib, c = dev._lib, dev._ctx
    try:
        geom = np.array([9.0, 7.0, 2.0 * DX0, 2.0 * DX0, 0.0, 0.0])
        items = np.array([[DX0, DX0, 0.0, 0.0], [1.5 * DX0, DX0, DX0, -DX0]])
        off = np.array([[0.0, 0.0], [DX0, -DX0]])
        w = np.array([0.7, -1.3])
        boxes = np.array([[0, 9, 0, 7], [2, 3, 4, 5]], dtype=np.int32)
        host = np.full((2, 7, 9), -1.0)
        flux = np.full((2, 2), -1.0)

        def last(entry):
            return lib.paos_last_error(c).decode().startswith(f"paos_series_sum_{entry}: ")

        def add(per_item=items, offsets=off, per_item_offsets=0, weights=w, per_frame=0):
            return lib.paos_series_sum_add(c, _dbl(per_item), _dbl(offsets), per_item_offsets, _dbl(weights), per_frame)

        def flux_of(bx=boxes, nboxes=2, response=None, out=flux):
            return lib.paos_series_sum_flux(c, _ints(bx), nboxes, _dbl(response), _dbl(out))

        def changed(a, index, value):
            a = a.copy()
            a[index] = value
            return a

        # before begin
        assert add() == 1 and last("add") and flux_of() == 1 and last("flux")
        assert lib.paos_series_sum_fetch(c, _dbl(host)) == 1 and last("fetch")
        # begin: null, a geometry paos_detector_begin refuses, frames, the size rule (nothing is allocated)
        assert lib.paos_series_sum_begin(c, None, 2) == 1 and last("begin")
        for index, value in ((0, 0.0), (0, 4097.0), (1, 2.5), (2, 0.0), (3, -1.0), (3, inf), (4, nan), (5, inf)):
            assert lib.paos_series_sum_begin(c, _dbl(changed(geom, index, value)), 2) == 1 and last("begin"), (index, value)
        for frames in (0, -1, 65537):
            assert lib.paos_series_sum_begin(c, _dbl(geom), frames) == 1 and last("begin"), frames
        assert lib.paos_series_sum_begin(c, _dbl(np.array([64.0, 64.0, DX0, DX0, 0.0, 0.0])), 65536) == 1 and last("begin")
        assert "2^27" in lib.paos_last_error(c).decode()
        assert lib.paos_series_sum_fetch(c, _dbl(host)) == 1  # a refused begin opens nothing
        assert lib.paos_series_sum_begin(c, _dbl(geom), 2) == 0
        # add before a PSF is kept
        assert add() == 1 and "no PSF kept" in lib.paos_last_error(c).decode()
        psfs = _keep(dev, _fields(n, 2, 1))
        bad = [dict(per_item=None), dict(offsets=None), dict(weights=None),
               dict(per_item=changed(items, (0, 0), 0.0)), dict(per_item=changed(items, (1, 1), -DX0)),
               dict(per_item=changed(items, (1, 0), nan)), dict(per_item=changed(items, (0, 1), inf)),
               dict(per_item=changed(items, (1, 2), inf)), dict(per_item=changed(items, (0, 3), nan)),
               dict(offsets=changed(off, (1, 0), nan)), dict(offsets=changed(off, (0, 1), -inf)),
               dict(per_item=changed(items, (1, 2), 1.7e308), offsets=changed(off, (1, 0), 1.7e308)),  # x0 + ox overflows
               dict(weights=changed(w, 1, nan)), dict(weights=changed(w, 0, inf)),
               dict(weights=np.array([[1.0, 1.0], [1.0, nan]]), per_frame=1)]
        for kw in bad:
            assert add(**kw) == 1 and last("add"), kw
        assert lib.paos_series_sum_begin(c, _dbl(changed(geom, 4, -1.7e308)), 2) == 0  # xc - X overflows
        assert add(per_item=changed(items, (0, 2), 1.7e308)) == 1 and last("add")
        assert lib.paos_series_sum_begin(c, _dbl(geom), 2) == 0
        # flux and fetch
        for kw in (dict(bx=None), dict(out=None), dict(nboxes=0), dict(nboxes=-1), dict(nboxes=17),
                   dict(bx=changed(boxes, (1, 1), 2)), dict(bx=changed(boxes, (0, 1), 10)), dict(bx=changed(boxes, (0, 0), -1)),
                   dict(bx=changed(boxes, (1, 3), 8)), dict(bx=changed(boxes, (1, 2), 5)), dict(response=np.full((7, 9), nan)),
                   dict(response=np.where(np.eye(7, 9) > 0, inf, 1.0))):
            assert flux_of(**kw) == 1 and last("flux"), kw
            assert np.all(flux == -1.0), kw  # nothing touched
        assert lib.paos_series_sum_fetch(c, None) == 1 and last("fetch")
        # nothing was added by a refused call, and the context is still usable
        assert lib.paos_series_sum_fetch(c, _dbl(host)) == 0 and not host.any()
        assert add() == 0 and flux_of() == 0 and lib.paos_series_sum_fetch(c, _dbl(host)) == 0
        det = Detector(9, 7, 2.0 * DX0)
        want = ssnp.add(np.zeros((2, 7, 9)), psfs, det, items[:, 0], items[:, 1], w, off, items[:, 2:])
        assert np.array_equal(host, want)
        for t in range(2):
            assert flux[t, 0] == snp.flux_tree(want[t], (0, 9, 0, 7)) and flux[t, 1] == want[t, 4, 2]
    finally:
        dev.close()
