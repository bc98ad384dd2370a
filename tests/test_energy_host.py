"""Encircled energy without a GPU (README.md, "Encircled energy"): the NumPy restatement (tests/energy_np.py) against a
brute-force loop over pixels and against exact lattice-point counts, ``EnergyProfile.ree`` against the formula, and
``run_batch(psf_energy=...)`` on the NumPy model of the device against the restatement applied to the oracle's PSF -- plus
every refusal."""
import math
import os

import numpy as np
import pytest

import blur_np
import energy_np as enp
from oracle.run_np import run as oracle_run
from paos_amd import _lib
from paos_amd.chains import syn20_chain, syn20_wavelength
from paos_amd.parse_config import parse_config
from paos_amd.run import run_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENS = os.path.join(ROOT, "data", "lens")
FIELD = {"us": 0.0, "ut": 0.0}
LDR = np.longdouble
# The model device sums the oracle's PSF in long double; run_batch's PSF on the model agrees with the oracle's to the
# project's fp64 parity gate, relative to the PSF's total power:
TOL = 1.0e-10


def _last_num(chain):
    return chain[list(chain.keys())[-1]]["num"]


def _random_psf(n, seed=2020):
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
@pytest.mark.parametrize("n", [16, 32])
@pytest.mark.parametrize("centre", ["pixel", "half", "corner"])
def test_restatement_against_brute_force(n, centre):
    psf = _random_psf(n)
    cx, cy = {"pixel": (n / 2, n / 2 - 1.0), "half": (n / 2 - 0.5, n / 2 + 0.5), "corner": (0.0, float(n - 1))}[centre]
    for delta, aspect, bins in ((1.0, 1.0, n // 2), (0.5, 1.0, n), (0.75, 0.5, 5), (1.5, 2.0, 4)):
        for square in (False, True):
            got, count, _ = enp.curves(psf, cx, cy, delta, aspect, bins, square)
            want, wcount = enp.curves_brute(psf, cx, cy, delta, aspect, bins, square)
            assert np.array_equal(count, wcount), (delta, aspect, square)
            assert np.max(np.abs(got - want)) <= 1e-17 * float(np.sum(psf)), (delta, aspect, square)
    # a half-pixel centre puts pixels exactly on a radius, on both sides: d2 == t_b counts as inside
    if centre == "half":
        idx = enp.ring_indices(n, cx, cy, 0.5, 1.0, 4)
        k, j = int(cy + 0.5), int(cx + 1.5)  # x = 1.5, y = 0.5: d2 = 2.5 > 1.5^2 = 2.25, <= 2^2
        assert idx[k, j] == 3 and idx[k, int(cx - 1.5)] == 3
        assert idx[int(cy + 0.5), int(cx + 0.5)] == 1 and idx[int(cy - 0.5), int(cx - 0.5)] == 1  # d2 = 0.5 <= 1.0^2


@pytest.mark.parametrize("aspect", [1.0, 0.5, 2.0])
def test_all_ones_counts_lattice_points(aspect):
    n, bins, delta = 64, 12, 1.25
    assert bins * delta <= n / 2 and bins * delta / aspect <= n / 2
    ones = np.ones((n, n))
    ee, count, sabs = enp.curves(ones, n / 2, n / 2, delta, aspect, bins)
    for b in range(bins):
        want = enp.lattice_count((b + 1) * delta, aspect)
        assert ee[b] == want and count[b] == want and sabs[b] == want
    if aspect == 1.0:
        sq, _, _ = enp.curves(ones, n / 2, n / 2, delta, aspect, bins, square=True)
        assert [int(v) for v in sq] == [(2 * math.floor((b + 1) * delta) + 1) ** 2 for b in range(bins)]
    else:  # the squares are rectangles on the pixel lattice: half-widths r along x, r / a along y
        sq, _, _ = enp.curves(ones, n / 2, n / 2, delta, aspect, bins, square=True)
        want = [(2 * math.floor((b + 1) * delta) + 1) * (2 * math.floor((b + 1) * delta / aspect) + 1) for b in range(bins)]
        assert [int(v) for v in sq] == want


def test_a_single_bright_pixel_is_an_exact_step():
    from paos_amd import EnergyProfile

    n = 32
    psf = np.zeros((n, n))
    psf[20, 11] = 3.5
    s = enp.summary(psf, enp.GIVEN)
    assert (s["peak"], s["peak_col"], s["peak_row"]) == (3.5, 11, 20) and s["S"] == 3.5
    assert enp.summary(psf, enp.CENTROID)["cx"] == 11.0 and enp.summary(psf, enp.CENTROID)["cy"] == 20.0
    # about the grid centre the pixel sits at x = -5, y = 4: d2 = 41, inside the circles of radius >= sqrt(41) = 6.40..
    ee, count, _ = enp.curves(psf, n / 2, n / 2, 1.0, 1.0, 10)
    assert [float(v) for v in ee] == [0.0] * 6 + [3.5] * 4 and count[6] == 149  # (lattice points within radius 7)
    prof = EnergyProfile(10, 1.0, unit="px", fractions=(0.5, 1.0))
    # the whole rise happens in ring 6: b* = 6, lo = 0 -> 6 step + step f
    assert prof.ree(ee.astype(np.float64), 3.5).tolist() == [6.5, 7.0]
    assert np.array_equal(prof.ree(ee.astype(np.float64), 3.5), enp.ree(ee, 3.5, 1.0, (0.5, 1.0)))
    # about the pixel itself everything is inside the first circle
    ee0, _, _ = enp.curves(psf, 11.0, 20.0, 0.3, 1.0, 4)
    assert [float(v) for v in ee0] == [3.5] * 4


def test_ree_edge_cases():
    from paos_amd import EnergyProfile

    prof = EnergyProfile(4, 2.0e-6, fractions=(0.25, 0.5, 1.0))
    ee = np.array([1.0, 2.0, 3.0, 4.0])
    got = prof.ree(ee, 4.0)
    assert got.tolist() == [2.0e-6, 2 * 2.0e-6, 3 * 2.0e-6 + 2.0e-6 * (4.0 - 3.0) / (4.0 - 3.0)]
    assert np.array_equal(got, enp.ree(ee, 4.0, 2.0e-6, (0.25, 0.5, 1.0)))
    # not reached: the curve stops short of the total
    short = prof.ree(ee, 8.0)
    assert short[0] == 2 * 2.0e-6 and short[1] == 4 * 2.0e-6 and math.isnan(short[2])
    assert np.array_equal(np.isnan(short), np.isnan(enp.ree(ee, 8.0, 2.0e-6, (0.25, 0.5, 1.0))))
    # S = 0, S < 0 and S = NaN: NaN throughout
    for total in (0.0, -1.0, float("nan")):
        assert np.all(np.isnan(prof.ree(np.zeros(4), total))) and np.all(np.isnan(enp.ree(np.zeros(4), total, 2.0e-6, (0.5,))))
    # interpolation inside a ring, and a curve that is not monotone (negative ringing): the FIRST ring that reaches it
    assert EnergyProfile(3, 1.0, unit="px", fractions=(0.5,)).ree(np.array([1.0, 3.0, 2.5]), 3.0).tolist() == [1.25]
    assert EnergyProfile(3, 1.0, unit="px", fractions=()).ree(ee[:3], 3.0).shape == (0,)


def test_centroid_fallback():
    n = 16
    assert enp.summary(np.zeros((n, n)), enp.CENTROID)["fallback"] and enp.summary(np.zeros((n, n)), enp.CENTROID)["cx"] == n / 2
    neg = np.zeros((n, n))
    neg[3, 3], neg[3, 12] = 1.0, -0.9  # S > 0, but the centroid lands outside the grid: (3 - 10.8) / 0.1 < 0
    s = enp.summary(neg, enp.CENTROID)
    assert s["fallback"] and (s["cx"], s["cy"]) == (n / 2, n / 2)
    assert not enp.summary(neg, enp.PEAK)["fallback"] and not enp.summary(neg, enp.GIVEN, (1.0, 2.0))["fallback"]
    tie = np.zeros((n, n))
    tie[9, 2] = tie[4, 7] = tie[4, 11] = 2.0  # a tie goes to the first in row-major order
    s = enp.summary(tie, enp.PEAK)
    assert (s["peak_col"], s["peak_row"], s["cx"], s["cy"]) == (7, 4, 7.0, 4.0)


# ---- EnergyProfile ----------------------------------------------------------------------------------------------------
def test_energy_profile_is_exported_and_validates():
    import paos_amd

    assert "EnergyProfile" in paos_amd.__all__
    EnergyProfile = paos_amd.EnergyProfile
    e = EnergyProfile(256, 2.0e-6)
    assert (e.bins, e.step, e.unit, e.centre, e.square, e.reads_psf) == (256, 2.0e-6, "m", None, False, True) and e.fractions.size == 0
    e = EnergyProfile(bins=8, step=1.5, unit="px", centre=[[3.0, 4.0], [5.0, 63.5]], fractions=(0.5, 1.0), square=True)
    e.check(2, 64)
    with pytest.raises(ValueError):
        e.check(3, 64)  # the shape against the batch
    with pytest.raises(ValueError):
        e.check(2, 32)  # 63.5 is outside [0, 32)
    with pytest.raises(ValueError):
        EnergyProfile(8, 1.0, centre=[[-1.0, 4.0]]).check(1, 64)
    for bad in (dict(bins=0), dict(bins=1025), dict(bins=8.0), dict(bins=True), dict(bins="many"),
                dict(step=0.0), dict(step=-1.0), dict(step=float("nan")), dict(step=float("inf")), dict(step="wide"),
                dict(unit="mm"), dict(unit=None),
                dict(centre="middle"), dict(centre=[1.0, 2.0]), dict(centre=[[1.0, 2.0, 3.0]]), dict(centre=[[float("nan"), 1.0]]),
                dict(centre=[[float("inf"), 1.0]]), dict(centre=[["a", "b"]]),
                dict(fractions=(0.0,)), dict(fractions=(1.5,)), dict(fractions=(-0.1, 0.5)), dict(fractions=(float("nan"),)),
                dict(fractions="half")):
        kw = dict(bins=8, step=1.0)
        kw.update(bad)
        with pytest.raises(ValueError):
            EnergyProfile(**kw)


def test_rings_per_item_and_the_size_rule():
    from paos_amd import EnergyProfile

    n = 64
    d, a = EnergyProfile(8, 2.0e-6).rings(n, [1.0e-6, 3.0e-6], [2.0e-6, 1.5e-6])
    assert d.tolist() == [2.0e-6 / 1.0e-6, 2.0e-6 / 3.0e-6] and a.tolist() == [2.0e-6 / 1.0e-6, 1.5e-6 / 3.0e-6]
    d, a = EnergyProfile(8, 2.5, unit="px").rings(n, [1.0e-6, 3.0e-6], [2.0e-6, 1.5e-6])
    assert d.tolist() == [2.5, 2.5] and a.tolist() == [1.0, 1.0]
    EnergyProfile(32, 1.0, unit="px").rings(n, [1.0], [1.0])  # bins D = N/2 exactly is allowed
    with pytest.raises(ValueError, match="item 1"):  # too wide: 8 x 5 px = 40 > 32
        EnergyProfile(8, 5.0e-6).rings(n, [2.0e-6, 1.0e-6], [2.0e-6, 1.0e-6])
    with pytest.raises(ValueError, match="item 0"):  # too tall: 8 x 2 / 0.4 = 40 rows
        EnergyProfile(8, 2.0e-6).rings(n, [1.0e-6, 1.0e-6], [0.4e-6, 1.0e-6])


# ---- run_batch on the model device ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["Hubble_simple", "SYN20"])
def test_run_batch_against_the_restatement_of_the_oracle_psf(name):
    from paos_amd import EnergyProfile, PsfBlur

    n = 64
    pup, zoom, field, wls, chains = _case(name)
    nb = len(wls)
    num = _last_num(chains[0])
    refs = [oracle_run(pup, wl, n, zoom, field, chain)[num] for wl, chain in zip(wls, chains)]
    step = 1.5 * refs[0]["dx"]
    bins = int((n / 2) * min(min(r["dx"], r["dy"]) for r in refs) / step)
    given = np.array([[n / 2 + 0.5 * i, n / 2 - 1.0] for i in range(nb)])
    for centre, mode in ((None, enp.GIVEN), ("centroid", enp.CENTROID), ("peak", enp.PEAK), (given, enp.GIVEN)):
        prof = EnergyProfile(bins, step, centre=centre, fractions=(0.5, 0.8), square=True)
        # the lean walk: nothing is downloaded, the PSFs come out of the last pass
        dev = enp.EnergyModelDevice(n, nb)
        res = run_batch(pup, wls, n, zoom, field, chains, outputs=(), dev=dev, psf_energy=prof)
        calls = [what for what, _ in dev.log]
        assert "download" not in calls and calls.count("energy_compute") == 1 and calls.count("energy_fetch") == 1
        plain = run_batch(pup, wls, n, zoom, field, chains, outputs=(), dev=enp.EnergyModelDevice(n, nb))
        new = {"ee_radius", "ee", "ensq", "ee_total", "ee_centre", "ee_peak", "ee_fallback", "ree"}
        for i, ref in enumerate(refs):
            rec = res[i][num]
            for key, other in res[i].items():
                assert sorted(set(other) - new) == sorted(plain[i][key])
                assert key == num or not new & set(other)
            psf = ref["amplitude"] ** 2
            total = float(psf.sum())
            s = enp.summary(psf, mode, given[i] if centre is given else None)
            assert abs(rec["ee_total"] - total) <= TOL * total
            assert np.array_equal(rec["ee_radius"], (np.arange(bins) + 1.0) * step)
            assert rec["ee_peak"][1] == (s["peak_col"], s["peak_row"]) and abs(rec["ee_peak"][0] - s["peak"]) <= TOL * s["peak"]
            assert rec["ee_fallback"] is False
            assert abs(rec["ee_centre"][0] - s["cx"]) <= 1e-8 and abs(rec["ee_centre"][1] - s["cy"]) <= 1e-8
            # about the centre the run found, so that membership is shared
            cx, cy = rec["ee_centre"]
            delta, aspect = step / ref["dx"], ref["dy"] / ref["dx"]
            for key, square in (("ee", False), ("ensq", True)):
                want = enp.curves(psf, cx, cy, delta, aspect, bins, square)[0].astype(np.float64)
                assert rec[key].shape == (bins,) and np.max(np.abs(rec[key] - want)) <= TOL * total, key
            assert np.array_equal(rec["ree"], enp.ree(rec["ee"], rec["ee_total"], step, (0.5, 0.8)), equal_nan=True)
            assert np.all(rec["ree"][np.isfinite(rec["ree"])] <= bins * step)
    # unit="px" with dx = dy gives what unit="m" gives with step = step_px dx
    if name == "SYN20":
        assert all(r["dx"] == r["dy"] for r in refs)
        one = [syn20_wavelength(0)]
        a = run_batch(1.0, one, n, 4, FIELD, [syn20_chain()], outputs=(), dev=enp.EnergyModelDevice(n, 1),
                      psf_energy=EnergyProfile(16, 2.0, unit="px", centre="centroid", fractions=(0.5,)))
        b = run_batch(1.0, one, n, 4, FIELD, [syn20_chain()], outputs=(), dev=enp.EnergyModelDevice(n, 1),
                      psf_energy=EnergyProfile(16, 2.0 * refs[0]["dx"], unit="m", centre="centroid", fractions=(0.5,)))
        assert (2.0 * refs[0]["dx"]) / refs[0]["dx"] == 2.0
        assert np.array_equal(a[0][20]["ee"], b[0][20]["ee"]) and a[0][20]["ee_centre"] == b[0][20]["ee_centre"]
        assert np.array_equal(b[0][20]["ee_radius"], a[0][20]["ee_radius"] * refs[0]["dx"])
        assert abs(b[0][20]["ree"][0] - a[0][20]["ree"][0] * refs[0]["dx"]) <= 1e-15 * b[0][20]["ree"][0]


def test_behind_a_blur_and_through_focus():
    from paos_amd import EnergyProfile, PsfBlur

    n, wls = 64, [syn20_wavelength(k) for k in (0, 300)]
    chains = [syn20_chain() for _ in wls]
    refs = [oracle_run(1.0, wl, n, 4, FIELD, syn20_chain())[20] for wl in wls]
    prof = EnergyProfile(12, 2.0 * refs[0]["dx"], centre="centroid", fractions=(0.9,), square=True)
    blur = PsfBlur(2.0 * refs[0]["dx"], 1.2 * refs[0]["dy"], pixel=(3.0 * refs[0]["dx"], 2.0 * refs[0]["dy"]), array=True)
    # behind a blur the curves are those of P': the blur is attached first, on the lean walk too
    dev = enp.EnergyModelDevice(n, 2)
    res = run_batch(1.0, wls, n, 4, FIELD, chains, outputs=(), dev=dev, psf_blur=blur, psf_energy=prof)
    calls = [what for what, _ in dev.log]
    assert "download" not in calls and calls.index("blur_apply") < calls.index("energy_compute")
    sharp = run_batch(1.0, wls, n, 4, FIELD, chains, outputs=(), dev=enp.EnergyModelDevice(n, 2), psf_energy=prof)
    for i, r in enumerate(refs):
        rec = res[i][20]
        total = float(rec["psf_blur"].sum())
        cx, cy = rec["ee_centre"]
        for key, square in (("ee", False), ("ensq", True)):
            want = enp.curves(rec["psf_blur"], cx, cy, prof.step / r["dx"], r["dy"] / r["dx"], 12, square)[0].astype(np.float64)
            assert np.array_equal(rec[key], want), key  # (the model sums the very array it hands out)
        assert np.max(np.abs(rec["ee"] - sharp[i][20]["ee"])) > 1e-3 * total  # (the blur does change the curve)
        assert rec["ee"][0] < sharp[i][20]["ee"][0]  # (it takes power out of the core)
    # every plane of a focus stack gets the keys, each about its own centre; the nominal plane equals the nominal record
    delta = 2.0e-4
    stack = run_batch(1.0, wls, n, 4, FIELD, chains, outputs=("psf",), focus_planes=[-delta, 0.0, delta],
                      dev=enp.EnergyModelDevice(n, 2), psf_energy=prof)
    keys = ("ee_radius", "ee", "ensq", "ee_total", "ee_centre", "ee_peak", "ee_fallback", "ree")
    for i, r in enumerate(refs):
        rec = stack[i][20]
        for p in rec["focus"]:
            assert set(keys) <= set(p)
            s = enp.summary(p["psf"], enp.CENTROID)
            assert abs(p["ee_centre"][0] - s["cx"]) <= 1e-12 and abs(p["ee_centre"][1] - s["cy"]) <= 1e-12
            want = enp.curves(p["psf"], *p["ee_centre"], prof.step / r["dx"], r["dy"] / r["dx"], 12)[0].astype(np.float64)
            assert np.array_equal(p["ee"], want)
            if p["dz"] == 0.0:
                for key in keys:
                    same = (np.array_equal(p[key], rec[key], equal_nan=(key == "ree")) if isinstance(rec[key], np.ndarray)
                            else p[key] == rec[key])
                    assert same, key
            else:
                assert not np.array_equal(p["ee"], rec["ee"])


# ---- refusals ---------------------------------------------------------------------------------------------------------
def _refused(**kw):
    n = 64
    chains = kw.pop("chains", [syn20_chain(), syn20_chain()])
    dev = enp.EnergyModelDevice(n, 2)
    with pytest.raises(ValueError) as err:
        run_batch(1.0, [1.0e-6, 1.2e-6], n, 4, FIELD, chains, dev=dev, **kw)
    assert dev.log == [] and not dev.u.any(), "something was launched before the refusal"
    return str(err.value)


def test_refusals_come_before_any_launch():
    from paos_amd import EnergyProfile

    unsaved = syn20_chain()
    unsaved[20] = dict(unsaved[20], save=False)
    prof = EnergyProfile(8, 2.0e-6)
    assert "EnergyProfile" in _refused(psf_energy=(8, 2.0e-6))
    assert "EnergyProfile" in _refused(psf_energy=8)
    assert "saved" in _refused(chains=[unsaved, unsaved], psf_energy=prof)
    assert "sync" in _refused(sync=False, psf_energy=prof)
    assert "shape" in _refused(psf_energy=EnergyProfile(8, 2.0e-6, centre=[[1.0, 2.0]]))
    assert "inside" in _refused(psf_energy=EnergyProfile(8, 2.0e-6, centre=[[1.0, 2.0], [64.0, 2.0]]))


def test_the_size_rule_names_the_item():
    from paos_amd import EnergyProfile

    n, wls = 64, [syn20_wavelength(0), syn20_wavelength(511)]
    refs = [oracle_run(1.0, wl, n, 4, FIELD, syn20_chain())[20] for wl in wls]
    assert refs[0]["dx"] < refs[1]["dx"]
    # 32 rings of dx_1 each: exactly half the grid for item 1, more than that for item 0
    dev = enp.EnergyModelDevice(n, 2)
    with pytest.raises(ValueError, match="item 0"):
        run_batch(1.0, wls, n, 4, FIELD, [syn20_chain(), syn20_chain()], outputs=(), dev=dev,
                  psf_energy=EnergyProfile(32, refs[1]["dx"]))
    assert "energy_compute" not in [what for what, _ in dev.log]


def test_run_sharded_does_not_take_the_keyword():
    import inspect

    from paos_amd.dist import run_sharded

    assert "psf_energy" not in inspect.signature(run_sharded).parameters
    with pytest.raises(TypeError):
        run_sharded(1.0, [1.0e-6], 64, 4, FIELD, [syn20_chain()], batch=1, psf_energy=None)


def test_the_model_device_refuses_what_the_library_refuses():
    n = 64
    dev = enp.EnergyModelDevice(n, 2)
    with pytest.raises(_lib.PaosHipError):  # before any PSF is kept
        dev.energy_compute(8, 1.0, 1.0, enp.CENTROID)
    with pytest.raises(_lib.PaosHipError):  # before a compute
        dev.energy_fetch()
    dev.u[:] = np.sqrt(_random_psf(n))
    dev.psf_keep()
    for args in ((0, 1.0, 1.0, enp.PEAK), (1025, 0.01, 1.0, enp.PEAK), (8, 1.0, 1.0, 3), (8, 0.0, 1.0, enp.PEAK),
                 (8, float("nan"), 1.0, enp.PEAK), (8, 1.0, -1.0, enp.PEAK), (8, 1.0, float("inf"), enp.PEAK),
                 (8, 4.5, 1.0, enp.PEAK), (8, 4.0, 0.9, enp.PEAK)):
        with pytest.raises(_lib.PaosHipError):
            dev.energy_compute(*args)
    for ctr in ([[1.0, 2.0], [64.0, 1.0]], [[-0.5, 2.0], [1.0, 1.0]], [[1.0, float("nan")], [1.0, 1.0]]):
        with pytest.raises(_lib.PaosHipError):
            dev.energy_compute(8, 1.0, 1.0, enp.GIVEN, centres=ctr)
    dev.energy_compute(8, 4.0, 1.0, enp.GIVEN, centres=[[63.5, 0.0], [0.0, 63.0]], square=True)  # bins D = N/2: allowed
    summary, curves = dev.energy_fetch()
    assert summary.shape == (2, 9) and curves.shape == (2, 2, 8)
    dev.psf_keep()
    with pytest.raises(_lib.PaosHipError):  # stale
        dev.energy_fetch()
    assert dev.energy_fetch(curves=False)[1] is None  # (the summary is still served)
    dev.energy_compute(8, 4.0, 1.0, enp.PEAK)
    assert dev.energy_fetch()[1].shape == (2, 1, 8)
    dev.otf_compute()
    dev.blur_apply(1.0, 1.0, 1.0, 1.0)
    with pytest.raises(_lib.PaosHipError):  # a blur rewrites the PSFs
        dev.energy_fetch()


def test_the_c_calls_refuse_null_contexts():
    lib = _lib.load()
    per_item = np.array([[1.0, 1.0, 32.0, 32.0]])
    assert lib.paos_ee_compute(None, 8, 0, 1, per_item.ctypes.data_as(_lib._dbl_p)) == 1
    assert lib.paos_last_error(None).decode().startswith("paos_ee_compute: ")
    out = np.zeros(9)
    assert lib.paos_ee_fetch(None, out.ctypes.data_as(_lib._dbl_p), None) == 1
    assert lib.paos_last_error(None).decode().startswith("paos_ee_fetch: ")
