"""Zoomed PSF windows without a GPU: the restatement (tests/zoom_np.py) against an independent evaluation of the same
interpolant, its exactness properties, the library's host-side weight tables, and run_batch(psf_zoom=...) on the NumPy
model of the device against the restatement applied to the oracle's last-surface field -- plus every refusal, which must
come before anything is launched."""
import ctypes
import os

import numpy as np
import pytest

import focus_np
import zoom_np
from conftest import l2_rel_err, rel_err
from paos_amd import PsfWindow, _lib
from paos_amd.chains import syn20_chain, syn20_wavelength
from paos_amd.parse_config import parse_config
from paos_amd.run import run_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENS = os.path.join(ROOT, "data", "lens")
FIELD = {"us": 0.0, "ut": 0.0}
TOL = 1.0e-10  # the project's fp64 parity gate (max-norm and L2-relative)


def _random_field(n, seed=7):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))


# (window size, oversampling, cx, cy): integer and fractional centres, every oversampling, windows that wrap
CASES = [(32, 1, None, None), (48, 3, 131.0, 120.0), (64, 4, None, None), (64, 8, 100.0, 77.0),
         (48, 3, 128.25, 127.5), (32, 4, 17.375, 200.8125), (64, 8, 90.7, 33.3), (16, 1, 12.5, 250.25),
         (64, 4, 3.0, 254.0), (48, 3, 255.6, 0.2), (96, 1, 250.0, 10.0)]


@pytest.mark.parametrize("m,s,cx,cy", CASES)
def test_restatement_against_the_spectrum(m, s, cx, cy):
    """Wy u Wx^T with the long-double weights is the trigonometric polynomial of fft2(u) with the Nyquist term split:
    two evaluations that share nothing but the field (they agree to about 2e-15 of max|u| at N = 256)."""
    n = 256
    u = _random_field(n)
    got = zoom_np.window(u, m, s, cx, cy)
    want = zoom_np.window_by_spectrum(u, m, s, cx, cy)
    err = np.max(np.abs(got - want)) / np.max(np.abs(u))
    print(f"zoom restatement vs spectrum M={m} s={s} centre=({cx}, {cy}): {err:.2e} of max|u|")
    assert err < TOL
    assert l2_rel_err(got, want) < TOL


def test_a_wrapping_window_is_the_window_of_the_rolled_field():
    n, m, s = 256, 64, 4
    u = _random_field(n, 11)
    wrapped = zoom_np.window(u, m, s, 2.25, 253.5)
    rolled = zoom_np.window(np.roll(u, (100, 40), axis=(0, 1)), m, s, 42.25, 97.5)  # (253.5 + 100) mod 256, 2.25 + 40
    # the same weights on the same samples, summed in another order: equal to rounding (N eps times the weights' 1-norm)
    assert np.max(np.abs(wrapped - rolled)) < 1.0e-12 * np.max(np.abs(u))


@pytest.mark.parametrize("a,b", [(3, -5), (-100, 127), (0, 64), (-127, -1)])
def test_plane_wave_comes_back_analytic(a, b):
    n, m, s = 256, 48, 3
    j = np.arange(n)
    u = np.exp(2j * np.pi * ((a * j[None, :] + b * j[:, None]) % n) / n)
    cx, cy = 100.4, 31.75
    got = zoom_np.window(u, m, s, cx, cy)
    x = np.asarray(zoom_np.positions(n, m, s, cx), dtype=np.float64)
    y = np.asarray(zoom_np.positions(n, m, s, cy), dtype=np.float64)
    want = np.exp(2j * np.pi * (a * x[None, :] + b * y[:, None]) / n)
    assert np.max(np.abs(got - want)) < TOL
    assert np.max(np.abs(zoom_np.psf(got) - 1.0)) < TOL


@pytest.mark.parametrize("m,s,cx,cy", [(32, 1, 40.0, 200.0), (48, 3, 131.0, 120.0), (64, 4, 128.0, 128.0),
                                        (64, 8, 5.0, 251.0)])
def test_grid_aligned_samples_are_the_field(m, s, cx, cy):
    """Integer centre: fine samples with (p - M/2) % s == 0 have unit-vector weight rows -- copies, bit for bit."""
    n = 256
    u = _random_field(n, 3)
    got = zoom_np.window(u, m, s, cx, cy)
    idx = np.arange(m)
    on = idx[(idx - m // 2) % s == 0]
    rows = (int(cy) + (on - m // 2) // s) % n
    cols = (int(cx) + (on - m // 2) // s) % n
    assert on.size >= m // s
    assert np.array_equal(got[np.ix_(on, on)], u[np.ix_(rows, cols)])
    assert np.array_equal(zoom_np.psf(got)[np.ix_(on, on)], (u.real**2 + u.imag**2)[np.ix_(rows, cols)])


def _library_table(n, s, frac):
    lib = _lib.load()
    w = np.full((s, n), np.nan)
    carry = np.full(s, -1, dtype=np.intc)
    rc = lib.paos_zoom_weights(n, s, frac, w.ctypes.data_as(_lib._dbl_p), carry.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
    return rc, w, carry


@pytest.mark.parametrize("n,s,frac", [(64, 1, 0.0), (64, 4, 0.0), (256, 3, 0.0), (256, 4, 0.25), (256, 8, 0.7),
                                      (128, 3, 0.5), (4096, 4, 0.8125), (1024, 64, 0.999), (256, 5, 1.0 / 3.0)])
def test_library_weight_tables(n, s, frac):
    """paos_zoom_weights against the restatement's tables: within 1 ulp of double (two long-double evaluations can
    straddle one rounding boundary); unit-vector rows and the carries exact."""
    rc, w, carry = _library_table(n, s, frac)
    assert rc == 0
    want, want_carry = zoom_np.phase_table(n, s, frac)
    assert np.array_equal(carry, want_carry)
    ref = want.astype(np.float64)
    assert np.all(np.abs(w - ref) <= np.spacing(np.abs(ref)))
    units = 0
    for b in range(s):
        phi = np.longdouble(frac) + np.longdouble(b) / np.longdouble(s)
        if phi == 0 or phi == 1:
            units += 1
            assert np.array_equal(w[b], np.eye(1, n, 0)[0])
    assert units == sum(1 for b in range(s) if (frac * s + b) % s == 0)  # (the fractions used are exact in binary or never hit)
    # a row sums to 1 (the interpolant of a constant is the constant)
    assert np.max(np.abs(w.sum(axis=1) - 1.0)) < 1e-12


def test_library_weight_tables_refuse_bad_arguments():
    lib = _lib.load()
    w = np.zeros((4, 64))
    carry = np.zeros(4, dtype=np.intc)
    wp, cp = w.ctypes.data_as(_lib._dbl_p), carry.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    assert lib.paos_zoom_weights(64, 4, 0.5, wp, cp) == 0
    for n, s, frac in [(63, 4, 0.5), (0, 4, 0.5), (-64, 4, 0.5), (64, 0, 0.5), (64, 65, 0.5), (64, 4, 1.0),
                       (64, 4, -0.25), (64, 4, float("nan")), (64, 4, float("inf"))]:
        assert lib.paos_zoom_weights(n, s, frac, wp, cp) == 1, (n, s, frac)
    assert lib.paos_zoom_weights(64, 4, 0.5, None, cp) == 1
    assert lib.paos_zoom_weights(64, 4, 0.5, wp, None) == 1


def _case(name):
    """(pupil diameter, zoom, field, wavelengths [m], chains, grid)"""
    if name == "SYN20":
        wls = [syn20_wavelength(k) for k in (0, 200, 511)]
        return 1.0, 4, FIELD, wls, [syn20_chain() for _ in wls], 64
    pup, par, wls, fields, chains = parse_config(os.path.join(LENS, "Hubble_simple.ini"))
    wls = [1e-6 * wls[0], 1.3e-6 * wls[0]]
    return pup, par["zoom"], fields[0], wls, [chains[0], chains[0]], 128


@pytest.mark.parametrize("name", ["Hubble_simple", "SYN20"])
def test_run_batch_against_the_oracle(name):
    pup, zoom, field, wls, chains, n = _case(name)
    num = chains[0][list(chains[0].keys())[-1]]["num"]
    oracle = [focus_np.oracle_end_state(pup, wl, n, zoom, field, ch) for wl, ch in zip(wls, chains)]
    centres = np.array([[n / 2 + 0.25 * i, n / 2 - 1.5 + 0.125 * i] for i in range(len(wls))])
    plain = run_batch(pup, wls, n, zoom, field, chains, outputs=("wfo", "psf"), dev=zoom_np.ZoomModelDevice(n, len(wls)))
    for window, ctr in ((PsfWindow(32, 4), None), (PsfWindow(48, 3, centre=centres, field=True), centres)):
        dev = zoom_np.ZoomModelDevice(n, len(wls))
        res = run_batch(pup, wls, n, zoom, field, chains, outputs=("wfo", "psf"), dev=dev, psf_zoom=window)
        assert [k for k, _ in dev.log].count("zoom_compute") == 1
        for i, (saved, end) in enumerate(oracle):
            # the nominal records are what they are without the keyword
            assert sorted(res[i]) == sorted(plain[i])
            for key, rec in plain[i].items():
                for k, v in rec.items():
                    if isinstance(v, np.ndarray):
                        assert np.array_equal(res[i][key][k], v), (key, k)
                assert ("psf_zoom" in res[i][key]) == (key == num)
            rec = res[i][num]
            cxy = (n / 2, n / 2) if ctr is None else tuple(ctr[i])
            want = zoom_np.window(saved[num]["wfo"], window.size, window.oversample, *cxy)
            assert rec["psf_zoom"].shape == (window.size, window.size) and rec["psf_zoom"].dtype == np.float64
            assert rel_err(rec["psf_zoom"], zoom_np.psf(want)) < TOL and l2_rel_err(rec["psf_zoom"], zoom_np.psf(want)) < TOL
            assert rec["zoom_dx"] == end.dx / window.oversample and rec["zoom_dy"] == end.dy / window.oversample
            assert rec["zoom_centre"] == cxy
            assert ("wfo_zoom" in rec) == window.field
            if window.field:
                assert rel_err(rec["wfo_zoom"], want) < TOL and l2_rel_err(rec["wfo_zoom"], want) < TOL


def test_focus_planes_and_centroid():
    """Every plane's dict gets the window of that plane; "centroid" puts it at the pixel nearest to the plane's own
    intensity centroid."""
    import copy

    n, wls = 64, [syn20_wavelength(k) for k in (0, 511)]
    chains = [syn20_chain() for _ in wls]
    ends = [focus_np.oracle_end_state(1.0, wl, n, 4, FIELD, ch)[1] for wl, ch in zip(wls, chains)]
    planes = [1.0e-4, 0.0, -0.5e-4]
    dev = zoom_np.ZoomModelDevice(n, len(wls))
    window = PsfWindow(32, 4, centre="centroid", field=True)
    res = run_batch(1.0, wls, n, 4, FIELD, chains, outputs=("psf",), dev=dev, focus_planes=planes, psf_zoom=window)
    assert [k for k, _ in dev.log].count("zoom_compute") == 1 + len(planes)
    for i, end in enumerate(ends):
        rec = res[i][20]
        for p in rec["focus"]:
            ref = copy.deepcopy(end)
            ref.ptp(p["dz"])
            I = np.abs(ref._wfo) ** 2
            yy, xx = np.mgrid[0:n, 0:n]
            want_ctr = (float(np.floor((I * xx).sum() / I.sum() + 0.5)), float(np.floor((I * yy).sum() / I.sum() + 0.5)))
            assert p["zoom_centre"] == want_ctr
            want = zoom_np.window(ref._wfo, 32, 4, *want_ctr)
            assert rel_err(p["wfo_zoom"], want) < TOL and rel_err(p["psf_zoom"], zoom_np.psf(want)) < TOL
            assert p["zoom_dx"] == end.dx / 4 and p["zoom_dy"] == end.dy / 4
        nominal = rec["focus"][1]
        assert np.array_equal(nominal["psf_zoom"], rec["psf_zoom"]) and np.array_equal(nominal["wfo_zoom"], rec["wfo_zoom"])
        assert nominal["zoom_centre"] == rec["zoom_centre"]
    # zero power: the grid centre
    dark = zoom_np.ZoomModelDevice(n, 1)
    recs = [{}]
    with np.errstate(all="ignore"):
        window.attach(dark, recs, [1.0], [2.0])
    assert recs[0]["zoom_centre"] == (n / 2, n / 2) and not recs[0]["psf_zoom"].any()
    assert recs[0]["zoom_dx"] == 0.25 and recs[0]["zoom_dy"] == 0.5


def _refused(**kw):
    """run_batch must raise ValueError and launch nothing."""
    n = kw.pop("n", 64)
    chains = kw.pop("chains", None) or [syn20_chain(), syn20_chain()]
    dev = zoom_np.ZoomModelDevice(n, len(chains))
    with pytest.raises(ValueError) as err:
        run_batch(1.0, [1.0e-6, 1.5e-6], n, 4, FIELD, chains, outputs=(), dev=dev, **kw)
    assert dev.log == [] and not dev.u.any(), "something was launched before the refusal"
    return str(err.value)


def test_refusals_come_before_any_launch():
    unsaved = syn20_chain()
    unsaved[20] = dict(unsaved[20], save=False)
    assert "saved" in _refused(psf_zoom=PsfWindow(32, 4), chains=[unsaved, unsaved])
    assert "sync" in _refused(psf_zoom=PsfWindow(32, 4), sync=False)
    _refused(psf_zoom=(32, 4))  # not a PsfWindow
    # m > s n
    assert "wider" in _refused(psf_zoom=PsfWindow(128, 1))
    _refused(psf_zoom=PsfWindow(1024, 8))
    # centres: one per item, finite, inside [0, n)
    _refused(psf_zoom=PsfWindow(32, 4, centre=[[32.0, 32.0]]))
    _refused(psf_zoom=PsfWindow(32, 4, centre=[[32.0, 32.0], [64.0, 1.0]]))
    _refused(psf_zoom=PsfWindow(32, 4, centre=[[32.0, 32.0], [-0.5, 1.0]]))
    _refused(psf_zoom=PsfWindow(32, 4, centre=[[32.0, float("nan")], [3.0, 1.0]]))
    _refused(psf_zoom=PsfWindow(32, 4, centre=[[32.0, float("inf")], [3.0, 1.0]]))
    # what the constructor itself refuses (the C rules for the size and the oversampling)
    for size, s in [(8, 4), (40, 4), (1040, 64), (0, 4), (-16, 4), (32, 0), (32, 65), (32.0, 4), (32, 2.5), (True, 4)]:
        with pytest.raises(ValueError):
            PsfWindow(size, s)
    for centre in ("peak", [1.0, 2.0], [[1.0, 2.0, 3.0]], [["a", "b"]]):
        with pytest.raises(ValueError):
            PsfWindow(32, 4, centre=centre)
    # the device entry point applies the same rules before it calls the library
    dev = zoom_np.ZoomModelDevice(64, 2)
    for size, s, ctr in [(24, 4, None), (128, 1, None), (32, 65, None), (32, 4, [[1.0, 2.0]]), (32, 4, [[1.0, 2.0], [64.0, 0.0]])]:
        with pytest.raises(ValueError):
            dev.zoom_compute(size, s, ctr)
        with pytest.raises(ValueError):
            _lib.zoom_check(size, s, 64)
            if ctr is not None:
                _lib.zoom_centres(ctr, 2, 64)
    assert dev.log == []
    with pytest.raises(_lib.PaosHipError):
        dev.zoom_fetch(0)
    dev.zoom_compute(32, 4)
    with pytest.raises(_lib.PaosHipError):
        dev.zoom_fetch(0, "field")


def test_run_sharded_refuses_the_keyword():
    from paos_amd.dist import run_sharded

    with pytest.raises(ValueError):
        run_sharded(1.0, [1.0e-6], 64, 4, FIELD, [syn20_chain()], psf_zoom=PsfWindow(32, 4),
                    make_device=lambda n, b: zoom_np.ZoomModelDevice(n, b))


def test_without_the_keyword_nothing_changes():
    dev = zoom_np.ZoomModelDevice(64, 1)
    res = run_batch(1.0, [1.0e-6], 64, 4, FIELD, [syn20_chain()], outputs=("psf",), dev=dev)
    assert not any(k.startswith("zoom") for rec in res[0].values() for k in rec)
    assert not any(name.startswith("zoom") for name, _ in dev.log)


# ---- the launch plan (paos_zoom_tiles) and what the long-double cases reach of it ----------------------------------------
def test_launch_plan_query():
    """paos_zoom_tiles is the rule paos_zoom_compute launches by: the largest of 8, 4, 2, 1 tiles per wave that still
    leaves 1024 waves and is no more than the window has tiles."""
    assert _lib.zoom_tiles(64, 1, 16) == (1, 1)
    assert _lib.zoom_tiles(4096, 1, 64) == (1, 1)  # 256 x 4 waves at one tile: exactly 1024
    assert _lib.zoom_tiles(4096, 2, 64) == (2, 1)
    assert _lib.zoom_tiles(4096, 32, 1024) == (8, 8)
    assert _lib.zoom_tiles(1024, 2, 256) == (2, 1)  # (what tests/test_gpu_zoom.py reaches)
    lib = _lib.load()
    a, b = ctypes.c_int(-1), ctypes.c_int(-1)
    for n, batch, m in [(256, 1, 24), (256, 1, 8), (256, 1, 0), (256, 1, 1040), (256, 0, 16), (256, -3, 16), (250, 1, 16),
                        (0, 1, 16), (-256, 1, 16)]:
        assert lib.paos_zoom_tiles(n, batch, m, ctypes.byref(a), ctypes.byref(b)) == 1, (n, batch, m)
    assert lib.paos_zoom_tiles(256, 1, 16, None, ctypes.byref(b)) == 1
    assert lib.paos_zoom_tiles(256, 1, 16, ctypes.byref(a), None) == 1
    assert (a.value, b.value) == (-1, -1)
    with pytest.raises(ValueError):
        _lib.zoom_tiles(256, 1, 24)


def test_the_long_double_cases_reach_every_build():
    """tests/test_gpu_products_xprec.py runs products_xprec.ZOOM_CASES and, for the bit-for-bit check, each of them in a
    batch-1 context.  From the library's own rule: together they launch zoom_kernel<T, STAGE, PT> for both stages at
    every PT, each stage with a partial last group at some PT > 1, and the batch-1 companions at PT 1 for both stages.
    A changed rule that leaves a build unreached fails here."""
    import products_xprec as px

    table = {(1024, 16, 128, 4): (8, 1), (1024, 11, 192, 4): (8, 1), (1024, 7, 160, 3): (4, 1), (2048, 4, 128, 4): (4, 1),
             (256, 16, 256, 2): (4, 4), (512, 8, 320, 3): (4, 2), (256, 10, 240, 2): (2, 2), (256, 9, 496, 4): (4, 8),
             (256, 8, 512, 4): (4, 8)}
    assert sorted(px.ZOOM_CASES) == sorted(table)
    reached, partial = set(), set()
    for n, batch, m, s in px.ZOOM_CASES:
        _lib.zoom_check(m, s, n)
        pt = _lib.zoom_tiles(n, batch, m)
        assert pt == table[(n, batch, m, s)], ((n, batch, m, s), pt)
        assert _lib.zoom_tiles(n, 1, m) == (1, 1), (n, m)
        for stage, p in zip("YX", pt):
            reached.update({(stage, p), (stage, 1)})  # (the case itself and its batch-1 companion)
            if p > 1 and (m // 16) % p:
                partial.add(stage)
    assert reached == {(stage, p) for stage in "YX" for p in (1, 2, 4, 8)}, sorted(reached)
    assert partial == {"Y", "X"}, partial
    # a partial group at PT 8 and at PT 4 in stage Y, at PT 2 and PT 8 in stage X (the table of the cases)
    assert _lib.zoom_tiles(1024, 11, 192) == (8, 1) and 12 % 8 and _lib.zoom_tiles(1024, 7, 160)[0] == 4 and 10 % 4
    assert _lib.zoom_tiles(256, 10, 240) == (2, 2) and 15 % 2 and _lib.zoom_tiles(256, 9, 496)[1] == 8 and 31 % 8
