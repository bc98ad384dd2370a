"""Encircled energy on the GPU (paos_ee_compute / paos_ee_fetch, run_batch(psf_energy=...); csrc/energy_pass.h): sums,
centres and curves against the long-double restatement of tests/energy_np.py on the fetched PSF, at the project's bound
for metric sums; the exact cases, the bit-for-bit invariants, staleness, the run_batch paths and misuse of the C calls.
``pytest -s`` prints the measured errors as multiples of the bound (XPREC lines: profiles/r20_energy_xprec.md)."""
import math

import numpy as np
import pytest

import energy_np as enp
import xprec_np as xp

pytestmark = pytest.mark.gpu

FIELD = {"us": 0.0, "ut": 0.0}
LDR = np.longdouble
GIVEN, CENTROID, PEAK = enp.GIVEN, enp.CENTROID, enp.PEAK


def _field(n, seed, x0=None, y0=None, width=None):
    """A speckled blob: complex Gaussian noise under a separable Gaussian envelope about (x0, y0) -- a PSF with a core, wings
    that fall off, and a centroid that is neither the grid centre nor the peak."""
    rng = np.random.default_rng(202000 + 7 * n + seed)
    j = np.arange(n, dtype=np.float64)
    x0 = n / 2 + 0.37 * (seed + 1) if x0 is None else x0
    y0 = n / 2 - 0.81 * (seed + 1) if y0 is None else y0
    w = n / 10 if width is None else width
    env = np.exp(-((j - y0) ** 2) / (4 * w * w))[:, None] * np.exp(-((j - x0) ** 2) / (4 * w * w))[None, :]
    u = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    u *= env
    return u


def _device(n, precision, fields):
    from paos_amd import _lib

    dev = _lib.DeviceFields(n, len(fields), precision)
    for i, u in enumerate(fields):
        dev.upload(i, u)
    dev.psf_keep()
    return dev


def _check_summary(row, psf, mode, given, what):
    """One item's fetched summary against the long-double sums: S, Sx, Sy within bound_metric over N^2 terms; the peak, its
    position and the fallback flag exact; a centroid within what its two sums and one division allow:
    |Sx'/S' - Sx/S| <= (bound(Sx) + |cx| bound(S)) / S to first order (a factor 1 + 1e-6 for the second), plus one rounding
    of the quotient.  Returns the errors of the three sums as multiples of their bounds."""
    n = psf.shape[0]
    ref = enp.summary(psf, mode, given)
    scales = enp.sum_scales(psf)
    mult = []
    lims = []
    for k, key in enumerate(("S", "Sx", "Sy")):
        lim = enp.bound(n * n, scales[k])
        err = float(abs(LDR(row[k]) - ref[key]))
        assert err <= lim, f"{what}: {key}: |got - ref| = {err:.3g} > bound {lim:.3g}"
        mult.append(err / lim if lim > 0 else 0.0)
        lims.append(lim)
    assert row[3] == ref["peak"] and (int(row[4]), int(row[5])) == (ref["peak_col"], ref["peak_row"]), what
    assert bool(row[8]) == ref["fallback"], what
    if mode == CENTROID and not ref["fallback"]:
        s = float(ref["S"])
        for got, want, lim in ((row[6], ref["Sx"] / ref["S"], lims[1]), (row[7], ref["Sy"] / ref["S"], lims[2])):
            tol = (lim + abs(float(want)) * lims[0]) / s * (1.0 + 1.0e-6) + 2.0**-52 * abs(float(want))
            assert float(abs(LDR(got) - want)) <= tol, f"{what}: centroid {got!r} against {float(want)!r} (tolerance {tol:.3g})"
    else:
        assert (row[6], row[7]) == (ref["cx"], ref["cy"]), what
    return mult


def _check(dev, psfs, bins, deltas, aspects, mode, centres=None, square=False, what=""):
    """compute + fetch, every item against the restatement about the device's own fetched centre.  Returns (summary, curves)."""
    nb = len(psfs)
    deltas = np.broadcast_to(np.asarray(deltas, dtype=np.float64), (nb,))
    aspects = np.broadcast_to(np.asarray(aspects, dtype=np.float64), (nb,))
    dev.energy_compute(bins, deltas, aspects, mode, centres=centres, square=square)
    summary, curves = dev.energy_fetch()
    assert summary.shape == (nb, 9) and curves.shape == (nb, 2 if square else 1, bins)
    for i, psf in enumerate(psfs):
        tag = f"{what} item {i}"
        sums = _check_summary(summary[i], psf, mode, None if centres is None else centres[i], tag)
        cx, cy = summary[i, 6], summary[i, 7]
        worst = [enp.check_curve(curves[i, q], psf, cx, cy, deltas[i], aspects[i], square=bool(q), what=f"{tag} curve {q}")
                 for q in range(curves.shape[1])]
        print(f"XPREC energy {tag}: S {sums[0]:.3f} Sx {sums[1]:.3f} Sy {sums[2]:.3f} ee {worst[0]:.3f}"
              + (f" ensq {worst[1]:.3f}" if square else "") + " of the bound")
    return summary, curves


# ---- against the long-double restatement --------------------------------------------------------------------------------
def test_64_fp64_batch_3():
    """The general case, a single ring, rings mostly empty, centres in corner pixels and on a half pixel."""
    xp.require_long_double()
    n = 64
    fields = [_field(n, s) for s in range(3)]
    dev = _device(n, "fp64", fields)
    try:
        psfs = [dev.psf_fetch(i) for i in range(3)]
        for mode in (CENTROID, PEAK, GIVEN):
            _check(dev, psfs, 20, [1.5, 1.1, 0.7], 1.0, mode, square=True, what=f"64^2 fp64 mode {mode}")
        _check(dev, psfs, 1, 2.7, 1.0, PEAK, what="64^2 one ring")
        _check(dev, psfs, 1, 0.3, 1.0, CENTROID, square=True, what="64^2 one ring of 0.3 px")
        half = np.array([[31.5, 32.5], [32.5, 31.5], [0.5, 62.5]])
        _check(dev, psfs, 100, 0.3, 1.0, GIVEN, centres=half, square=True, what="64^2 rings of 0.3 px, half-pixel centres")
        corner = np.array([[0.0, 0.0], [63.0, 63.0], [0.0, 63.0]])
        _check(dev, psfs, 16, 2.0, 1.0, GIVEN, centres=corner, square=True, what="64^2 corner pixels, bins D = N/2")
    finally:
        dev.close()


@pytest.mark.parametrize("aspect,bins,delta", [(0.5, 16, 2.0), (2.0, 32, 2.0), (0.5, 7, 1.3), (2.0, 9, 3.1)])
def test_128_fp64_anamorphic(aspect, bins, delta):
    xp.require_long_double()
    n = 128
    fields = [_field(n, 0), _field(n, 1, x0=40.2, y0=90.6)]
    dev = _device(n, "fp64", fields)
    try:
        psfs = [dev.psf_fetch(i) for i in range(2)]
        _check(dev, psfs, bins, delta, aspect, CENTROID, square=True, what=f"128^2 fp64 a = {aspect}")
        _check(dev, psfs, bins, delta, [aspect, 1.0], GIVEN, centres=np.array([[17.25, 100.5], [64.0, 64.0]]),
               what=f"128^2 fp64 a = {aspect}, 1")
    finally:
        dev.close()


def test_2048_fp32_batch_2():
    """The only place the 8-row block layout occurs."""
    xp.require_long_double()
    n = 2048
    fields = [_field(n, 0, width=60.0), _field(n, 1, x0=700.3, y0=1500.7, width=35.0)]
    dev = _device(n, "fp32", fields)
    try:
        psfs = [dev.psf_fetch(i) for i in range(2)]
        _check(dev, psfs, 256, [1.7, 0.9], [1.0, 1.3], CENTROID, square=True, what="2048^2 fp32")
    finally:
        dev.close()


def test_4096_fp64_every_row():
    """bins D = N/2 with 1024 rings: every row is reached, which pins the grid of the binning launch and its scratch."""
    xp.require_long_double()
    n = 4096
    dev = _device(n, "fp64", [_field(n, 0, width=300.0)])
    try:
        psfs = [dev.psf_fetch(0)]
        _check(dev, psfs, 1024, 2.0, 1.0, CENTROID, what="4096^2 fp64 1024 rings of 2 px")
    finally:
        dev.close()


# ---- exact cases --------------------------------------------------------------------------------------------------------
def test_all_ones_gives_integers():
    n, bins, delta = 64, 12, 1.25
    from paos_amd import _lib

    dev = _lib.DeviceFields(n, 2, "fp64")
    try:
        dev.fill(1.0 + 0.0j)
        dev.psf_keep()
        for aspect in (1.0, 0.5, 2.0):
            dev.energy_compute(bins, delta, aspect, GIVEN, square=True)
            summary, curves = dev.energy_fetch()
            for i in range(2):
                assert summary[i, 0] == n * n and summary[i, 1] == n * n * (n - 1) / 2 and summary[i, 2] == summary[i, 1]
                assert (summary[i, 3], summary[i, 4], summary[i, 5], summary[i, 8]) == (1.0, 0.0, 0.0, 0.0)
                assert curves[i, 0].tolist() == [float(enp.lattice_count((b + 1) * delta, aspect)) for b in range(bins)]
                want = [(2 * math.floor((b + 1) * delta) + 1) * (2 * math.floor((b + 1) * delta / aspect) + 1) for b in range(bins)]
                assert curves[i, 1].tolist() == [float(v) for v in want]
        # the centroid of all ones is (N - 1) / 2 exactly: a half-pixel centre, formed on the device
        dev.energy_compute(bins, delta, 1.0, CENTROID)
        summary, curves = dev.energy_fetch()
        assert (summary[0, 6], summary[0, 7]) == ((n - 1) / 2, (n - 1) / 2)
        want = enp.curves(np.ones((n, n)), (n - 1) / 2, (n - 1) / 2, delta, 1.0, bins)[0]
        assert curves[0, 0].tolist() == [float(v) for v in want]
    finally:
        dev.close()


def test_single_pixel_zero_item_and_peak_tie():
    from paos_amd import EnergyProfile

    n = 64
    spike = np.zeros((n, n), dtype=np.complex128)
    spike[40, 21] = 2.0  # |u|^2 = 4 at row 40, column 21
    tie = np.zeros((n, n), dtype=np.complex128)
    tie[50, 3] = tie[17, 30] = tie[17, 44] = 1.5j
    tie[20, 20] = 1.0
    dev = _device(n, "fp64", [spike, np.zeros((n, n), dtype=np.complex128), tie])
    try:
        # about the grid centre the spike sits at x = -11, y = 8: d2 = 185, inside the circles of radius >= 13.60..
        dev.energy_compute(16, 1.0, 1.0, GIVEN, square=True)
        summary, curves = dev.energy_fetch()
        assert curves[0, 0].tolist() == [0.0] * 13 + [4.0] * 3 and curves[0, 1].tolist() == [0.0] * 10 + [4.0] * 6
        assert summary[0].tolist() == [4.0, 84.0, 160.0, 4.0, 21.0, 40.0, 32.0, 32.0, 0.0]
        prof = EnergyProfile(16, 1.0, unit="px", fractions=(0.5, 1.0))
        assert prof.ree(curves[0, 0], summary[0, 0]).tolist() == [13.5, 14.0]
        # the all-zero item among them: zero curves, no fallback for a given centre
        assert not curves[1].any() and summary[1].tolist() == [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 32.0, 32.0, 0.0]
        # centroid: the spike's own pixel; the all-zero item falls back to the grid centre; NaN ree
        dev.energy_compute(4, 0.5, 1.0, CENTROID)
        summary, curves = dev.energy_fetch()
        assert (summary[0, 6], summary[0, 7], summary[0, 8]) == (21.0, 40.0, 0.0) and curves[0, 0].tolist() == [4.0] * 4
        assert (summary[1, 6], summary[1, 7], summary[1, 8]) == (32.0, 32.0, 1.0) and not curves[1].any()
        assert np.all(np.isnan(prof.ree(curves[1, 0], summary[1, 0])))
        # peak: a tie goes to the first in row-major order; the zero item's peak is its first pixel
        dev.energy_compute(4, 0.5, 1.0, PEAK)
        summary, curves = dev.energy_fetch()
        assert summary[2, 3:9].tolist() == [2.25, 30.0, 17.0, 30.0, 17.0, 0.0] and curves[2, 0].tolist() == [2.25] * 4
        assert summary[1, 3:9].tolist() == [0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
        _check(dev, [dev.psf_fetch(i) for i in range(3)], 30, 1.0, 1.0, PEAK, square=True, what="64^2 spikes")
    finally:
        dev.close()


# ---- bit for bit --------------------------------------------------------------------------------------------------------
def test_repeatable_and_independent_of_the_batch():
    n = 64
    fields = [_field(n, s) for s in range(3)]
    dev = _device(n, "fp64", fields)
    one = _device(n, "fp64", fields[2:])
    try:
        args = (24, [1.3, 0.9, 1.1], [1.0, 0.8, 1.25], CENTROID)
        dev.energy_compute(*args, square=True)
        first = dev.energy_fetch()
        dev.energy_compute(8, 1.0, 1.0, PEAK)  # (another request in between)
        dev.energy_compute(*args, square=True)
        again = dev.energy_fetch()
        assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
        one.energy_compute(24, 1.1, 1.25, CENTROID, square=True)
        alone = one.energy_fetch()
        assert np.array_equal(alone[0][0], first[0][2]) and np.array_equal(alone[1][0], first[1][2])
        # ... nor on what the other items ask for (the grid of the binning launch follows the largest request)
        dev.energy_compute(24, [0.2, 0.2, 1.1], [4.0, 4.0, 1.25], CENTROID, square=True)
        assert np.array_equal(dev.energy_fetch()[1][2], first[1][2])
    finally:
        dev.close()
        one.close()


def test_against_psf_metrics():
    """unit="px", the grid centre, step 1: the 16 circles of paos_psf_metrics on the field behind the same psf_keep.  Both
    are held to the long-double sums, so they agree within the sum of the two bounds."""
    xp.require_long_double()
    n = 64
    dev = _device(n, "fp64", [_field(n, 0), _field(n, 1)])
    try:
        radii = np.arange(1, 17, dtype=np.float64)
        met = dev.psf_metrics(radii)
        dev.energy_compute(16, 1.0, 1.0, GIVEN)
        summary, curves = dev.energy_fetch()
        for i in range(2):
            psf = dev.psf_fetch(i)
            _, count, sabs = enp.curves(psf, n / 2, n / 2, 1.0, 1.0, 16)
            for b in range(16):
                assert abs(curves[i, 0, b] - met[i]["encircled"][b]) <= 2 * enp.bound(count[b], sabs[b])
            assert abs(summary[i, 0] - met[i]["power"]) <= 2 * enp.bound(n * n, enp.sum_scales(psf)[0])
            assert summary[i, 3] == met[i]["peak"]
    finally:
        dev.close()


def test_behind_a_pixel_blur_and_staleness():
    """A pixel aperture rings: negative values in P'.  paos_blur_apply makes earlier curves stale, like paos_psf_keep."""
    xp.require_long_double()
    from paos_amd import _lib

    n = 64
    dev = _device(n, "fp64", [_field(n, 0, width=1.2), _field(n, 1, width=2.0)])
    try:
        dev.energy_compute(8, 1.0, 1.0, CENTROID)
        before = dev.energy_fetch()
        dev.otf_compute()
        dev.blur_apply(1.0e-5, 1.3e-5, 0.0, 0.0, 3.0e-5, 2.6e-5)
        with pytest.raises(_lib.PaosHipError, match="stale"):
            dev.energy_fetch()
        assert np.array_equal(dev.energy_fetch(curves=False)[0], before[0])  # (the summary is still served)
        psfs = [dev.psf_fetch(i) for i in range(2)]
        assert min(p.min() for p in psfs) < 0.0
        _check(dev, psfs, 24, 1.3, 1.3, CENTROID, square=True, what="64^2 behind a pixel blur")
        _check(dev, psfs, 32, 1.0, 1.0, PEAK, what="64^2 behind a pixel blur, peak")
        served = dev.energy_fetch()
        dev.psf_keep()
        with pytest.raises(_lib.PaosHipError, match="stale"):
            dev.energy_fetch()
        dev.energy_compute(32, 1.0, 1.0, PEAK)
        fresh = dev.energy_fetch()
        assert fresh[1].shape == served[1].shape and not np.array_equal(fresh[1], served[1])
    finally:
        dev.close()


# ---- run_batch ------------------------------------------------------------------------------------------------------------
def test_run_batch_end_to_end():
    """Hubble_simple at 256^2 x 2 with outputs=(): the lean walk (no array in the records, the curves of the ordinary walk
    bit for bit, as tests/test_gpu_otf.py holds the cuts), the curves against the restatement of the PSFs the device keeps,
    and the same through focus."""
    xp.require_long_double()
    import os

    from paos_amd import EnergyProfile, _lib
    from paos_amd.parse_config import parse_config
    from paos_amd.run import run_batch

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pup, par, wls, fields, chains = parse_config(os.path.join(root, "data", "lens", "Hubble_simple.ini"))
    wls = [1e-6 * wls[0], 1.3e-6 * wls[0]]
    chains = [chains[0], chains[0]]
    n = 256
    num = chains[0][list(chains[0].keys())[-1]]["num"]
    dev = _lib.DeviceFields(n, 2, "fp64")
    try:
        probe = run_batch(pup, wls, n, par["zoom"], fields[0], chains, outputs=(), dev=dev)
        step = 1.5 * probe[0][num]["dx"]
        bins = int((n / 2) * min(min(r[num]["dx"], r[num]["dy"]) for r in probe) / step)
        prof = EnergyProfile(bins, step, centre="centroid", fractions=(0.5, 0.9), square=True)
        lean = run_batch(pup, wls, n, par["zoom"], fields[0], chains, outputs=(), dev=dev, psf_energy=prof)
        psfs = [dev.psf_fetch(i) for i in range(2)]
        full = run_batch(pup, wls, n, par["zoom"], fields[0], chains, outputs=("psf",), psf_energy=prof)
        for i in range(2):
            rec = lean[i][num]
            assert "psf" not in rec and not any(isinstance(v, np.ndarray) and v.ndim == 2 for v in rec.values())
            for key in ("ee", "ensq", "ee_radius", "ree"):
                assert np.array_equal(rec[key], full[i][num][key], equal_nan=True), key
            assert rec["ee_centre"] == full[i][num]["ee_centre"] and rec["ee_peak"] == full[i][num]["ee_peak"]
            delta, aspect = step / rec["dx"], rec["dy"] / rec["dx"]
            cx, cy = rec["ee_centre"]
            _check_summary([rec["ee_total"], np.sum(psfs[i].astype(LDR) * np.arange(n)[None, :]),
                            np.sum(psfs[i].astype(LDR) * np.arange(n)[:, None]), rec["ee_peak"][0], *rec["ee_peak"][1], cx, cy,
                            rec["ee_fallback"]], psfs[i], CENTROID, None, f"run_batch item {i}")
            worst = [enp.check_curve(rec[key], psfs[i], cx, cy, delta, aspect, square=sq, what=f"run_batch item {i} {key}")
                     for key, sq in (("ee", False), ("ensq", True))]
            print(f"XPREC energy run_batch lean 256^2 item {i}: ee {worst[0]:.3f} ensq {worst[1]:.3f} of the bound")
            assert np.array_equal(rec["ree"], enp.ree(rec["ee"], rec["ee_total"], step, (0.5, 0.9)), equal_nan=True)
            assert np.all(np.isfinite(rec["ree"])) and rec["ree"][0] < rec["ree"][1]
        dz = 2.0e-4
        stack = run_batch(pup, wls, n, par["zoom"], fields[0], chains, outputs=("psf",), focus_planes=[-dz, 0.0, dz], psf_energy=prof)
        for i in range(2):
            rec = stack[i][num]
            for key in ("ee", "ensq"):
                assert np.array_equal(rec[key], full[i][num][key]), key
            for p in rec["focus"]:
                if p["dz"] == 0.0:
                    for key in ("ee", "ensq", "ree", "ee_radius"):
                        assert np.array_equal(p[key], rec[key], equal_nan=True), key
                    assert (p["ee_total"], p["ee_centre"], p["ee_peak"], p["ee_fallback"]) == \
                        (rec["ee_total"], rec["ee_centre"], rec["ee_peak"], rec["ee_fallback"])
                else:
                    # the plane's 'psf' is |u|^2 of the field the kept PSF was made from
                    cx, cy = p["ee_centre"]
                    enp.check_curve(p["ee"], p["psf"], cx, cy, step / rec["dx"], rec["dy"] / rec["dx"], what=f"plane {p['dz']}")
                    assert not np.array_equal(p["ee"], rec["ee"])
    finally:
        dev.close()


# ---- misuse of the C calls ------------------------------------------------------------------------------------------------
def test_misuse_of_the_c_calls():
    from paos_amd import _lib

    n = 64
    lib = _lib.load()
    dev = _lib.DeviceFields(n, 2, "fp64")
    ptr = lambda a: a.ctypes.data_as(_lib._dbl_p)  # noqa: E731
    good = np.array([[1.0, 1.0, 32.0, 32.0], [2.0, 2.0, 0.0, 63.5]])
    summary, curves = np.zeros((2, 9)), np.zeros((2, 2, 16))

    def refused(call, *args):
        assert call(dev._ctx, *args) == 1, args  # PAOS_EINVAL
        return lib.paos_last_error(dev._ctx).decode()

    try:
        assert "no PSF kept" in refused(lib.paos_ee_compute, 8, 0, CENTROID, ptr(good))
        assert "no energy profiles" in refused(lib.paos_ee_fetch, ptr(summary), None)
        for i, u in enumerate((_field(n, 0), _field(n, 1))):
            dev.upload(i, u)
        dev.psf_keep()
        assert "no energy profiles" in refused(lib.paos_ee_fetch, ptr(summary), ptr(curves))
        dev.energy_compute(16, good[:, 0], good[:, 1], GIVEN, centres=good[:, 2:], square=True)
        kept = dev.energy_fetch()
        assert "null" in refused(lib.paos_ee_compute, 8, 0, CENTROID, None)
        assert "null" in refused(lib.paos_ee_fetch, None, None)
        for bins in (0, -3, 1025):
            assert "bins" in refused(lib.paos_ee_compute, bins, 0, CENTROID, ptr(good))
        for mode in (-1, 3):
            assert "centre mode" in refused(lib.paos_ee_compute, 8, 0, mode, ptr(good))
        for col in (0, 1):
            for bad in (0.0, -1.0, float("nan"), float("inf")):
                rec = good.copy()
                rec[1, col] = bad
                assert "item 1" in refused(lib.paos_ee_compute, 8, 0, CENTROID, ptr(rec))
        assert "item 0" in refused(lib.paos_ee_compute, 33, 0, CENTROID, ptr(good))  # 33 x 1 px > N/2
        tall = good.copy()
        tall[1, 1] = 0.5
        assert "item 1" in refused(lib.paos_ee_compute, 9, 0, CENTROID, ptr(tall))   # 9 x 2 / 0.5 = 36 rows > N/2
        for bad in ((64.0, 1.0), (-0.25, 1.0), (1.0, 64.0), (1.0, float("nan")), (float("inf"), 1.0)):
            rec = good.copy()
            rec[0, 2:] = bad
            assert "centre" in refused(lib.paos_ee_compute, 8, 0, GIVEN, ptr(rec))
            assert lib.paos_ee_compute(dev._ctx, 8, 0, CENTROID, ptr(rec)) == 0  # (read for PAOS_EE_GIVEN only)
            dev.energy_compute(16, good[:, 0], good[:, 1], GIVEN, centres=good[:, 2:], square=True)
        # nothing was touched by the refusals, and the context is usable
        again = dev.energy_fetch()
        assert np.array_equal(kept[0], again[0]) and np.array_equal(kept[1], again[1])
        assert lib.paos_ee_fetch(dev._ctx, None, ptr(curves)) == 0 and np.array_equal(curves, kept[1])
        assert lib.paos_ee_fetch(dev._ctx, ptr(summary), None) == 0 and np.array_equal(summary, kept[0])
    finally:
        dev.close()
