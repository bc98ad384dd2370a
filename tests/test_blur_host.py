"""Blurred PSFs without a GPU (README.md, "Blurred PSFs"): the NumPy restatement (tests/blur_np.py) against the analytic
answer for Gaussians and against the definition evaluated by direct DFT in long double, paos_blur_table (host only)
against the long-double tables, and ``run_batch(psf_blur=...)`` / ``run_broadband`` on the NumPy model of the device
against the restatement applied to the oracle's PSF -- plus every refusal, which must come before anything is launched."""
import os

import numpy as np
import pytest

import blur_np
import detector_np
import otf_np
from oracle.run_np import run as oracle_run
from paos_amd import _lib
from paos_amd.chains import syn20_chain, syn20_wavelength
from paos_amd.detector import Detector, run_broadband
from paos_amd.parse_config import parse_config
from paos_amd.run import run_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENS = os.path.join(ROOT, "data", "lens")
FIELD = {"us": 0.0, "ut": 0.0}
TOL = 1.0e-10  # the project's fp64 parity gate, relative to the peak of the PSF / image

# Separable sampled Gaussian, sigma = (3, 2.5) px at 128^2, blurred by sigma = (4, 1.5) px: the Gaussian whose variances
# are the sums.  The restatement agrees to 2.2e-16 of the peak (measured; a few units of fp64 rounding); gated at:
ANALYTIC_TOL = 1.0e-13
# np.fft in fp64 against the direct DFT in long double, 16^2 and 32^2, seeded random PSFs (values of order 1): measured
# 3.1e-16 of the peak at most; ten times that:
RESTATEMENT_TOL = 3.1e-15


def _last_num(chain):
    return chain[list(chain.keys())[-1]]["num"]


def _random_psf(n, seed=606):
    rng = np.random.default_rng(seed + n)
    u = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    return u.real**2 + u.imag**2


def _case(name):
    """(pupil diameter, zoom, field, wavelengths [m], chains), 64^2"""
    if name == "SYN20":
        wls = [syn20_wavelength(k) for k in (0, 200, 511)]
        return 1.0, 4, FIELD, wls, [syn20_chain() for _ in wls]
    pup, par, wls, fields, chains = parse_config(os.path.join(LENS, "Hubble_simple.ini"))
    wls = [1e-6 * wls[0], 1.3e-6 * wls[0]]
    return pup, par["zoom"], fields[0], wls, [chains[0], chains[0]]


# ---- the definition ---------------------------------------------------------------------------------------------------
def test_gaussian_blurred_by_a_gaussian_adds_the_variances():
    n = 128
    p = blur_np.gaussian(n, 3.0, 2.5)
    got = blur_np.blur(p, *blur_np.tables_of(n, 1.0, 1.0, 4.0, 1.5))
    sx, sy = np.hypot(3.0, 4.0), np.hypot(2.5, 1.5)
    want = blur_np.gaussian(n, sx, sy) * (3.0 * 2.5) / (sx * sy)
    err = float(np.max(np.abs(got - want)) / want.max())
    print(f"Gaussian (3, 2.5) px blurred by (4, 1.5) px at 128^2: max |restatement - analytic| / peak = {err:.2e}")
    assert err <= ANALYTIC_TOL
    # the axes are not interchangeable: a transposed table pair would show
    swapped = blur_np.blur(p, *blur_np.tables_of(n, 1.0, 1.0, 1.5, 4.0))
    assert np.max(np.abs(swapped - want)) / want.max() > 1e-2


@pytest.mark.parametrize("n", [16, 32])
def test_restatement_against_the_direct_dft_in_long_double(n):
    psf = _random_psf(n)
    worst = 0.0
    for dx, dy, sx, sy, px, py in ((1.0, 1.0, 1.2, 0.7, 0.0, 0.0), (2.0e-6, 3.0e-6, 1.1e-6, 4.0e-6, 5.0e-6, 2.5e-6)):
        tx, ty = blur_np.tables_of(n, dx, dy, sx, sy, px, py)
        want = blur_np.blur_longdouble(psf, tx, ty)
        for got in (blur_np.blur(psf, tx, ty), blur_np.blur_reference(psf, tx, ty)):
            worst = max(worst, float(np.max(np.abs(got.astype(np.longdouble) - want)) / np.max(np.abs(want))))
        rows = np.array([0, 1, n // 2, n - 1])
        lines = blur_np.blur_reference_lines(psf, tx, ty, rows)
        assert float(np.max(np.abs(lines - want[rows]))) <= 1e-17 * float(np.max(np.abs(want)))
        cols = blur_np.blur_reference_lines(psf, tx, ty, rows, rows=False)
        assert float(np.max(np.abs(cols - want[:, rows]))) <= 1e-17 * float(np.max(np.abs(want)))
    print(f"restatement vs direct DFT in long double, {n}^2: max |dP'| / peak = {worst:.2e} (tolerance {RESTATEMENT_TOL:.1e})")
    assert worst <= RESTATEMENT_TOL


def test_sum_is_kept_and_no_blur_is_the_identity():
    n = 64
    psf = _random_psf(n)
    ones = blur_np.tables_of(n, 1.0e-5, 1.0e-5, 0.0, 0.0)
    assert all(np.array_equal(t, np.ones(n // 2 + 1)) for t in ones)
    assert np.max(np.abs(blur_np.blur(psf, *ones) - psf)) <= 1e-14 * psf.max()
    for args in ((1.0e-5, 1.3e-5, 2.0e-5, 0.7e-5), (1.0e-5, 1.3e-5, 0.0, 1.0e-5, 3.0e-5, 2.0e-5)):
        out = blur_np.blur(psf, *blur_np.tables_of(n, *args))
        assert abs(out.sum() - psf.sum()) <= 1e-13 * psf.sum()
    # a pixel factor rings: the band-limited box under a single bright pixel goes negative, and nothing is clamped
    spike = np.zeros((n, n))
    spike[20, 41] = 1.0
    assert blur_np.blur(spike, *blur_np.tables_of(n, 1.0, 1.0, 0.0, 0.0, 3.0, 3.0)).min() < -1e-3


# ---- paos_blur_table --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,sigma,pixel", [(64, 1.0, 1.5, 0.0), (64, 1.0, 0.0, 2.0), (256, 1.3e-5, 2.1e-5, 1.8e-5),
                                              (4096, 4.0e-6, 9.0e-6, 1.0e-5), (2, 1.0, 0.3, 0.5), (128, 1.0, 0.0, 0.0)])
def test_blur_table_against_the_long_double_restatement(n, d, sigma, pixel):
    got = _lib.blur_table(n, d, sigma, pixel)
    want = blur_np.table_longdouble(n, d, sigma, pixel)
    assert got.shape == (n // 2 + 1,) and got.dtype == np.float64 and got[0] == 1.0
    # to 1 ulp: two long-double evaluations (libm here, NumPy's there) may straddle a rounding boundary of the double
    ulp = np.spacing(np.abs(want.astype(np.float64)))
    assert np.all(np.abs(got.astype(np.longdouble) - want) <= ulp), float(np.max(np.abs(got - want) / ulp))
    if sigma == 0.0 and pixel == 0.0:
        assert np.array_equal(got, np.ones(n // 2 + 1))
    if pixel == 2.0 and sigma == 0.0:  # sinc(2 m / 64) changes sign at m = 32: Nyquist of a 2-pixel box is its first zero
        assert abs(got[-1]) < 1e-16 and got[-2] > 0.0


@pytest.mark.parametrize("args", [(3, 1.0, 1.0, 0.0), (0, 1.0, 1.0, 0.0), ((1 << 20) + 2, 1.0, 1.0, 0.0), (-4, 1.0, 1.0, 0.0),
                                  (64, 0.0, 1.0, 0.0), (64, -1.0, 1.0, 0.0), (64, float("nan"), 1.0, 0.0),
                                  (64, float("inf"), 1.0, 0.0), (64, 1.0, -1.0, 0.0), (64, 1.0, float("nan"), 0.0),
                                  (64, 1.0, float("inf"), 0.0), (64, 1.0, 1.0, -2.0), (64, 1.0, 1.0, float("nan")),
                                  (64, 1.0, 1.0, float("inf"))])
def test_blur_table_refusals(args):
    lib = _lib.load()
    out = np.full(1 << 19, 7.0)
    assert lib.paos_blur_table(*args, out.ctypes.data_as(_lib._dbl_p)) == 1  # PAOS_EINVAL
    assert lib.paos_last_error(None).decode().startswith("paos_blur_table: ")
    assert np.all(out == 7.0)


def test_blur_table_refuses_a_null_pointer():
    lib = _lib.load()
    assert lib.paos_blur_table(64, 1.0, 1.0, 0.0, None) == 1
    assert lib.paos_last_error(None).decode() == "paos_blur_table: null argument"
    assert lib.paos_blur_apply(None, None) == 1


# ---- PsfBlur ----------------------------------------------------------------------------------------------------------
def test_psf_blur_is_exported_and_validates():
    import paos_amd

    assert "PsfBlur" in paos_amd.__all__
    PsfBlur = paos_amd.PsfBlur
    b = PsfBlur(1.0e-6)
    assert b.sigma_y == b.sigma_x and b.pixel is None and b.array is False and b.reads_psf
    b = PsfBlur([1.0e-6, 2.0e-6], 3.0e-6, pixel=(1.0e-5, 2.0e-5), array=True)
    b.check(2)
    with pytest.raises(ValueError):
        b.check(3)
    sub = b.take([1, 1])
    assert sub.sigma_x.tolist() == [2.0e-6, 2.0e-6] and float(sub.sigma_y) == 3.0e-6 and sub.array
    for bad in (dict(sigma_x=-1.0), dict(sigma_x=float("nan")), dict(sigma_x=1.0, sigma_y=float("inf")),
                dict(sigma_x=[1.0, -2.0]), dict(sigma_x=1.0, pixel=(1.0, -1.0)), dict(sigma_x=1.0, pixel=(float("nan"), 1.0)),
                dict(sigma_x=1.0, pixel=3.0), dict(sigma_x=1.0, pixel=(1.0, 2.0, 3.0)), dict(sigma_x="wide"),
                dict(sigma_x=[[1.0, 2.0]])):
        with pytest.raises(ValueError):
            PsfBlur(**bad)


# ---- run_batch on the model device ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["Hubble_simple", "SYN20"])
def test_run_batch_against_the_restatement_of_the_oracle_psf(name):
    from paos_amd import PsfBlur

    n = 64
    pup, zoom, field, wls, chains = _case(name)
    nb = len(wls)
    num = _last_num(chains[0])
    refs = [oracle_run(pup, wl, n, zoom, field, chain)[num] for wl, chain in zip(wls, chains)]
    sx = [(1.5 + 0.8 * i) * refs[i]["dx"] for i in range(nb)]
    sy = [(0.6 + 1.1 * i) * refs[i]["dy"] for i in range(nb)]
    det = Detector(21, 17, 1.7 * refs[0]["dx"], 2.3 * refs[0]["dy"], xc=0.31 * refs[0]["dx"], yc=-0.62 * refs[0]["dy"])
    dev = blur_np.BlurModelDevice(n, nb)
    res = run_batch(pup, wls, n, zoom, field, chains, outputs=("psf", "mtf"), mtf_cuts=True, dev=dev, detector=det,
                    metrics_radii_px=(3.0,), psf_blur=PsfBlur(sx, sy, array=True))
    plain = run_batch(pup, wls, n, zoom, field, chains, outputs=("psf",), metrics_radii_px=(3.0,),
                      dev=blur_np.BlurModelDevice(n, nb))
    calls = [what for what, _ in dev.log]
    assert calls.count("otf_compute") == 1 and calls.count("blur_apply") == 1
    assert calls.index("otf_compute") < calls.index("blur_apply")
    for i, ref in enumerate(refs):
        rec = res[i][num]
        psf = ref["amplitude"] ** 2
        want = blur_np.blur(psf, *blur_np.tables_of(n, ref["dx"], ref["dy"], sx[i], sy[i]))
        assert rec["blur_sigma"] == (sx[i], sy[i])
        assert rec["psf_blur"].shape == (n, n) and rec["psf_blur"].dtype == np.float64
        assert np.max(np.abs(rec["psf_blur"] - want)) < TOL * psf.max()
        image = detector_np.rebin(want, det, ref["dx"], ref["dy"])
        assert np.max(np.abs(rec["detector"] - image)) < TOL * image.max()
        sharp = detector_np.rebin(psf, det, ref["dx"], ref["dy"])
        assert np.max(np.abs(rec["detector"] - sharp)) > 1e-3 * sharp.max()  # (the blur does change the image)
        # the system MTF: the optical one times the table, and what the restatement gives for P'
        for axis, table in (("x", blur_np.table(n, ref["dx"], sx[i])), ("y", blur_np.table(n, ref["dy"], sy[i]))):
            optical = otf_np.cuts_of(otf_np.mtf(psf))[axis == "y"]
            assert np.max(np.abs(rec["mtf_" + axis] - optical * table)) < TOL
            assert np.max(np.abs(rec["mtf_" + axis] - otf_np.cuts_of(otf_np.mtf(want))[axis == "y"])) < TOL
        assert np.array_equal(rec["mtf_x"][: n // 2], rec["mtf"][n // 2, n // 2:])
        # what is read from the field stays optical, and only the last surface's record carries the new keys
        new = {"blur_sigma", "psf_blur", "detector", "mtf", "mtf_x", "mtf_y", "freq_x", "freq_y"}
        for key, other in res[i].items():
            assert sorted(set(other) - new) == sorted(plain[i][key])
            if key != num:
                assert not new & set(other)
        assert np.array_equal(rec["psf"], plain[i][num]["psf"]) and rec["power"] == plain[i][num]["power"]
        assert rec["metrics"] == plain[i][num]["metrics"]


def test_the_lean_walk_the_accumulator_and_the_focus_planes():
    from paos_amd import PsfBlur

    n, wls = 64, [syn20_wavelength(k) for k in (0, 300)]
    chains = [syn20_chain() for _ in wls]
    refs = [oracle_run(1.0, wl, n, 4, FIELD, syn20_chain())[20] for wl in wls]
    blur = PsfBlur(2.0 * refs[0]["dx"], 1.2 * refs[0]["dy"])
    det = Detector(16, 16, 2.0 * refs[0]["dx"])
    # lean: nothing is downloaded, the PSF comes out of the last pass, and the cuts are the ordinary walk's
    dev = blur_np.BlurModelDevice(n, 2)
    lean = run_batch(1.0, wls, n, 4, FIELD, chains, outputs=(), mtf_cuts=True, dev=dev, psf_blur=blur)
    calls = [what for what, _ in dev.log]
    assert "download" not in calls and "otf_fetch" not in calls and calls.count("otf_compute") == 1
    full = run_batch(1.0, wls, n, 4, FIELD, chains, outputs=("psf",), mtf_cuts=True, dev=blur_np.BlurModelDevice(n, 2), psf_blur=blur)
    for i in range(2):
        assert "psf" not in lean[i][20] and lean[i][20]["blur_sigma"] == full[i][20]["blur_sigma"]
        for key in ("mtf_x", "mtf_y"):
            assert np.max(np.abs(lean[i][20][key] - full[i][20][key])) < TOL
    # the accumulator of detector_weights is made from P'
    w = np.array([0.7, 2.5])
    dev = blur_np.BlurModelDevice(n, 2)
    run_batch(1.0, wls, n, 4, FIELD, chains, outputs=(), dev=dev, detector=det, detector_weights=w, psf_blur=blur)
    images = [detector_np.rebin(blur_np.blur(r["amplitude"] ** 2, *blur_np.tables_of(n, r["dx"], r["dy"], blur.sigma_x, blur.sigma_y)),
                                det, r["dx"], r["dy"]) for r in refs]
    want = detector_np.accumulate(images, w)
    assert np.max(np.abs(dev.detector_fetch() - want)) < TOL * want.max()
    # every plane of a focus stack is treated alike; the nominal plane equals the nominal record
    planes = [1.0e-4, 0.0]
    blur_a = PsfBlur(2.0 * refs[0]["dx"], 1.2 * refs[0]["dy"], pixel=(3.0 * refs[0]["dx"], 2.0 * refs[0]["dy"]), array=True)
    stack = run_batch(1.0, wls, n, 4, FIELD, chains, outputs=("psf",), mtf_cuts=True, focus_planes=planes,
                      dev=blur_np.BlurModelDevice(n, 2), psf_blur=blur_a)
    for i, r in enumerate(refs):
        rec = stack[i][20]
        tabs = blur_np.tables_of(n, r["dx"], r["dy"], blur_a.sigma_x, blur_a.sigma_y, *blur_a.pixel)
        for p in rec["focus"]:
            assert {"blur_sigma", "psf_blur", "mtf_x", "mtf_y"} <= set(p)
            assert np.max(np.abs(p["psf_blur"] - blur_np.blur(p["psf"], *tabs))) < TOL * p["psf"].max()
            if p["dz"] == 0.0:
                for key in ("psf_blur", "mtf_x", "mtf_y", "blur_sigma"):
                    assert np.array_equal(p[key], rec[key]), key


def _refused(**kw):
    n = 64
    chains = kw.pop("chains", [syn20_chain(), syn20_chain()])
    dev = blur_np.BlurModelDevice(n, 2)
    with pytest.raises(ValueError) as err:
        run_batch(1.0, [1.0e-6, 1.2e-6], n, 4, FIELD, chains, dev=dev, **kw)
    assert dev.log == [] and not dev.u.any(), "something was launched before the refusal"
    return str(err.value)


def test_refusals_come_before_any_launch():
    from paos_amd import PsfBlur

    unsaved = syn20_chain()
    unsaved[20] = dict(unsaved[20], save=False)
    blur = PsfBlur(1.0e-6)
    assert "PsfBlur" in _refused(psf_blur=(1.0e-6, 1.0e-6))
    assert "PsfBlur" in _refused(psf_blur=1.0e-6)
    assert "saved" in _refused(chains=[unsaved, unsaved], psf_blur=blur)
    assert "sync" in _refused(sync=False, psf_blur=blur)
    assert "per item" in _refused(psf_blur=PsfBlur([1.0e-6, 2.0e-6, 3.0e-6]))
    assert "per item" in _refused(psf_blur=PsfBlur(1.0e-6, pixel=([1.0e-6], 1.0e-6)))
    assert "pixel" in _refused(psf_blur=PsfBlur(1.0e-6, pixel=(1.0e-5, 1.0e-5)), detector=Detector(8, 8, 1.0e-5))
    with pytest.raises(ValueError):  # (values that are not finite or are negative never make it into a PsfBlur)
        PsfBlur(1.0e-6, -1.0e-6)


def test_run_sharded_and_pipeline_do_not_take_the_keyword():
    import inspect

    from paos_amd.dist import run_sharded

    assert "psf_blur" not in inspect.signature(run_sharded).parameters
    with pytest.raises(TypeError):
        run_sharded(1.0, [1.0e-6], 64, 4, FIELD, [syn20_chain()], batch=1, psf_blur=None)


def test_run_broadband_passes_the_keyword_through(monkeypatch):
    from paos_amd import PsfBlur

    n = 64
    wls = [syn20_wavelength(k) for k in (0, 200, 511)]
    w = np.array([0.7, 0.4, 2.5])
    refs = [oracle_run(1.0, wl, n, 4, FIELD, syn20_chain(), light=True)[20] for wl in wls]
    det = Detector(21, 17, 1.7 * refs[1]["dx"], 2.3 * refs[1]["dy"])
    sx = [(1.0 + i) * refs[1]["dx"] for i in range(3)]
    sy = 0.8 * refs[1]["dy"]
    images = [detector_np.rebin(blur_np.blur(r["amplitude"] ** 2, *blur_np.tables_of(n, r["dx"], r["dy"], sx[i], sy)), det, r["dx"], r["dy"])
              for i, r in enumerate(refs)]
    want = detector_np.accumulate(images, w)
    monkeypatch.setattr(_lib, "DeviceFields", blur_np.BlurModelDevice)
    one = run_broadband(1.0, wls, w, n, 4, FIELD, syn20_chain(), det, batch=3, psf_blur=PsfBlur(sx, sy))
    two = run_broadband(1.0, wls, w, n, 4, FIELD, syn20_chain(), det, batch=2, psf_blur=PsfBlur(sx, sy))  # (a padded block)
    assert np.array_equal(one["image"], two["image"])
    assert np.max(np.abs(one["image"] - want)) < TOL * want.max()
    sharp = run_broadband(1.0, wls, w, n, 4, FIELD, syn20_chain(), det, batch=3)
    assert np.max(np.abs(sharp["image"] - want)) > 1e-3 * want.max()
    assert abs(one["power"] - sharp["power"]) <= 1e-14 * sharp["power"]  # the power stays the optical one
    with pytest.raises(ValueError):
        run_broadband(1.0, wls, w, n, 4, FIELD, syn20_chain(), det, psf_blur=PsfBlur([1.0e-6, 2.0e-6]))
    with pytest.raises(ValueError):
        run_broadband(1.0, wls, w, n, 4, FIELD, syn20_chain(), det, psf_blur=1.0e-6)


def test_the_model_device_refuses_what_the_library_refuses():
    dev = blur_np.BlurModelDevice(64, 2)
    dev.u[:] = np.sqrt(_random_psf(64))
    dev.psf_keep()
    with pytest.raises(_lib.PaosHipError):  # before any otf_compute
        dev.blur_apply(1.0, 1.0, 1.0, 1.0)
    dev.otf_compute()
    dev.psf_keep()
    with pytest.raises(_lib.PaosHipError):  # stale
        dev.blur_apply(1.0, 1.0, 1.0, 1.0)
    dev.otf_compute()
    with pytest.raises(_lib.PaosHipError):
        dev.blur_apply(1.0, 1.0, -1.0, 1.0)
    before = dev.psf_fetch(0)
    dev.blur_apply(1.0, 1.0, [1.0, 2.0], 0.5)
    once = dev.psf_fetch(1)
    assert not np.array_equal(dev.psf_fetch(0), before)
    dev.blur_apply(1.0, 1.0, [1.0, 2.0], 0.5)  # a second call compounds: T2 T1
    want = blur_np.blur(once, *blur_np.tables_of(64, 1.0, 1.0, 2.0, 0.5))
    assert np.max(np.abs(dev.psf_fetch(1) - want)) < 1e-13 * want.max()
    assert abs(dev.otf_fetch(1, "otf")[32, 32] - 1.0) == 0.0
