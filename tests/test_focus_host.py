"""Through-focus stacks without a GPU: run_batch(focus_planes=...) on the NumPy model of the device (tests/focus_np.py)
against the oracle -- ``RefWFO.ptp`` applied to the oracle's field behind the last surface, and, for planes within
2 zr of the waist (zr from the oracle's own pilot beam), the oracle's ``run`` on the chain with the last surface given
that thickness and one more saved surface appended -- plus every refusal, which must come before anything is launched."""
import copy
import os

import numpy as np
import pytest

import focus_np
from conftest import l2_rel_err, rel_err
from oracle.run_np import run as oracle_run
from paos_amd.chains import parse_config_variant, syn20_chain, syn20_wavelength
from paos_amd.detector import Detector
from paos_amd.parse_config import parse_config
from paos_amd.run import run_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENS = os.path.join(ROOT, "data", "lens")
FIELD = {"us": 0.0, "ut": 0.0}
TOL = 1.0e-10  # the project's fp64 parity gate (max-norm and L2-relative)


def _case(name):
    """(pupil diameter, zoom, field, wavelengths [m], chains, grid)"""
    if name == "SYN20":
        wls = [syn20_wavelength(k) for k in (0, 200, 511)]
        return 1.0, 4, FIELD, wls, [syn20_chain() for _ in wls], 64
    if name == "Hubble_simple":
        pup, par, wls, fields, chains = parse_config(os.path.join(LENS, "Hubble_simple.ini"))
        wls = [1e-6 * wls[0], 1.3e-6 * wls[0]]
        return pup, par["zoom"], fields[0], wls, [chains[0], chains[0]], 128
    pup, par, wls, fields, chains = parse_config_variant(os.path.join(LENS, "Ariel_AIRS-CH0.ini"), [1.95, 3.0, 3.9])
    return pup, par["zoom"], fields[0], [1e-6 * w for w in wls], chains, 64


def _planes(ends, n):
    """Defocus values for a batch, from the oracle's pilot beams: three inside 2 zr of every item's waist, the nominal
    plane, and one beyond 2 zr of the first item's; all within every item's sampling limit N d^2 / wl."""
    limit = min(n * min(w.dx, w.dy) ** 2 / w.wl for w in ends)
    zr = min(w.zr for w in ends)
    gap = max(abs(w.z - w.zw0) for w in ends)
    step = min(0.45 * (2.0 * zr - gap), 0.3 * limit)
    assert step > 0.0
    far = -np.sign(ends[0].zw0 - ends[0].z or 1.0) * min(0.95 * limit, 2.6 * ends[0].zr)
    return [step, -2.0 * step, 0.0, far, 0.5 * step]


@pytest.mark.parametrize("name", ["Hubble_simple", "SYN20", "Ariel_AIRS-CH0"])
def test_planes_against_the_oracle(name):
    pup, zoom, field, wls, chains, n = _case(name)
    last = list(chains[0].keys())[-1]
    num = chains[0][last]["num"]
    oracle = [focus_np.oracle_end_state(pup, wl, n, zoom, field, ch) for wl, ch in zip(wls, chains)]
    ends = [w for _, w in oracle]
    if name == "Ariel_AIRS-CH0":
        assert all(w.dx != w.dy for w in ends)  # anamorphic
    planes = _planes(ends, n)
    dev = focus_np.FocusModelDevice(n, len(wls))
    res = run_batch(pup, wls, n, zoom, field, chains, outputs=("wfo", "psf"), dev=dev, focus_planes=planes)
    plain = run_batch(pup, wls, n, zoom, field, chains, outputs=("wfo", "psf"), dev=focus_np.FocusModelDevice(n, len(wls)))
    assert [name for name, _ in dev.log].count("focus_begin") == 1  # one forward transform for the whole stack
    assert [name for name, _ in dev.log].count("focus_plane") == len(planes) - 1
    inside = 0
    for i, (wl, chain) in enumerate(zip(wls, chains)):
        # the nominal records are what they are without the keyword
        assert sorted(res[i]) == sorted(plain[i])
        for key, rec in plain[i].items():
            for k, v in rec.items():
                if isinstance(v, np.ndarray):
                    assert np.array_equal(res[i][key][k], v), (key, k)
                elif k not in ("ABCDt", "ABCDs", "aperture"):
                    assert res[i][key][k] == v, (key, k)
            assert ("focus" in res[i][key]) == (key == num)
        stack = res[i][num]["focus"]
        assert [p["dz"] for p in stack] == planes
        saved, end = oracle[i]
        assert rel_err(res[i][num]["wfo"], saved[num]["wfo"]) < TOL
        for p in stack:
            dz = p["dz"]
            if dz == 0.0:  # the nominal arrays, bit for bit
                assert np.array_equal(p["wfo"], res[i][num]["wfo"]) and np.array_equal(p["psf"], res[i][num]["psf"])
                assert p["z"] == end.z and p["wz"] == res[i][num]["wz"]
                continue
            ref = copy.deepcopy(end)
            ref.ptp(dz)
            assert rel_err(p["wfo"], ref._wfo) < TOL and l2_rel_err(p["wfo"], ref._wfo) < TOL, (i, dz)
            assert rel_err(focus_np.plane(res[i][num]["wfo"], end.wl, end.dx, end.dy, dz), ref._wfo) < TOL
            want_power = np.sum(np.abs(ref._wfo) ** 2)
            assert abs(p["power"] - want_power) < TOL * want_power
            assert p["z"] == ref.z and p["wz"] == ref.wz and p["distancetofocus"] == ref.distancetofocus
            if abs(end.z + dz - end.zw0) < 2.0 * end.zr:
                # the reference's propagate takes ptp here: the plane is the oracle's run to a surface dz further on
                inside += 1
                longer, extra = focus_np.refocused_chain(chain, dz)
                far = oracle_run(pup, wl, n, zoom, field, longer, light=True)[extra]
                assert far["propagator"] == "II"
                assert rel_err(p["wfo"], far["wfo"]) < TOL and l2_rel_err(p["wfo"], far["wfo"]) < TOL, (i, dz)
                assert p["wz"] == far["wz"] and p["distancetofocus"] == far["distancetofocus"]
                assert far["dx"] == end.dx and far["dy"] == end.dy
    assert inside >= 3 * len(wls)


def test_metrics_and_detector_per_plane():
    import detector_np

    n, wls = 64, [syn20_wavelength(k) for k in (0, 511)]
    chains = [syn20_chain() for _ in wls]
    ends = [focus_np.oracle_end_state(1.0, wl, n, 4, FIELD, ch)[1] for wl, ch in zip(wls, chains)]
    det = Detector(9, 7, 1.7 * ends[0].dx, 2.3 * ends[0].dy, xc=0.31 * ends[0].dx, yc=-0.62 * ends[0].dy)
    planes = [1.0e-4, 0.0, -0.5e-4]
    radii = [1.5, 4.0]
    dev = focus_np.FocusModelDevice(n, len(wls))
    res = run_batch(1.0, wls, n, 4, FIELD, chains, outputs=("psf",), dev=dev, focus_planes=planes, detector=det,
                    metrics_radii_px=radii)
    for i, end in enumerate(ends):
        rec = res[i][20]
        for p in rec["focus"]:
            ref = copy.deepcopy(end)
            ref.ptp(p["dz"])
            psf = np.abs(ref._wfo) ** 2
            assert rel_err(p["psf"], psf) < TOL
            want = detector_np.rebin(psf, det, end.dx, end.dy)
            assert p["detector"].shape == (det.ny, det.nx) and rel_err(p["detector"], want) < TOL
            assert abs(p["metrics"]["power"] - psf.sum()) < TOL * psf.sum()
            assert abs(p["metrics"]["peak"] - psf.max()) < TOL * psf.max()
        nominal = rec["focus"][1]
        assert np.array_equal(nominal["detector"], rec["detector"]) and np.array_equal(nominal["psf"], rec["psf"])


def _refused(**kw):
    """run_batch must raise ValueError and launch nothing."""
    n = kw.pop("n", 64)
    chains = kw.pop("chains", None) or [syn20_chain(), syn20_chain()]
    wls = kw.pop("wls", [1.0e-6, 1.5e-6])
    dev = focus_np.FocusModelDevice(n, len(wls))
    with pytest.raises(ValueError) as err:
        run_batch(1.0, wls, n, 4, FIELD, chains, outputs=(), dev=dev, **kw)
    assert dev.log == [] and not dev.u.any(), "something was launched before the refusal"
    return str(err.value)


def test_refusals_come_before_any_launch():
    _refused(focus_planes=[1e-4, float("nan")])
    _refused(focus_planes=[float("inf")])
    _refused(focus_planes=[1e-4, 0.0, 1e-4])  # not distinct
    _refused(focus_planes=3.0e-5)  # not a sequence
    # the reference would skip 0 < |dz| < wl / 1000 -- for the longer wavelength only
    assert "item 1" in _refused(focus_planes=[1.2e-9])
    _refused(focus_planes=[-0.5e-9])
    # beyond N d^2 / wl (SYN20 at 64^2: 4.0e-4 m at 1 um, 6.0e-4 m at 1.5 um) the plane is aliased
    msg = _refused(focus_planes=[1e-4, 4.1e-4])
    assert "item 0" in msg and "aliased" in msg
    _refused(focus_planes=[-4.1e-4])
    assert "item 1" in _refused(focus_planes=[5.0e-4], wls=[1.5e-6, 1.2e-6])
    # the last surface must be saved
    unsaved = syn20_chain()
    unsaved[20] = dict(unsaved[20], save=False)
    _refused(focus_planes=[1e-4], chains=[unsaved, unsaved])
    # accumulating detector weights across planes is ambiguous
    _refused(focus_planes=[1e-4], detector=Detector(8, 8, 1e-6), detector_weights=[1.0, 1.0])
    # a chain that ends away from its waist: the wavefront is not planar (C != 0), the reference's ptp would raise
    short = {k: v for k, v in syn20_chain().items() if k <= 4}
    short[4] = dict(short[4], save=True)
    msg = _refused(focus_planes=[1e-4], chains=[short, short])
    assert "item 0" in msg and "planar" in msg


def test_without_the_keyword_nothing_changes():
    n, wls = 64, [1.0e-6]
    dev = focus_np.FocusModelDevice(n, 1)
    res = run_batch(1.0, wls, n, 4, FIELD, [syn20_chain()], outputs=("psf",), dev=dev)
    assert "focus" not in res[0][20] and not any(name.startswith("focus") for name, _ in dev.log)
    # a stack of the nominal plane alone needs no spectrum
    dev = focus_np.FocusModelDevice(n, 1)
    res = run_batch(1.0, wls, n, 4, FIELD, [syn20_chain()], outputs=("psf",), dev=dev, focus_planes=[0.0])
    assert not any(name.startswith("focus") for name, _ in dev.log)
    assert np.array_equal(res[0][20]["focus"][0]["psf"], res[0][20]["psf"])
