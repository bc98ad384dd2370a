"""Transfer functions without a GPU (README.md, "Transfer functions"): the NumPy restatement (tests/otf_np.py) against a
direct long-double evaluation of the definition, against the exact answers for a single bright pixel and for a clear
circular pupil, and ``run_batch(outputs=("mtf", "otf"), mtf_cuts=True)`` on the NumPy model of the device against the
restatement applied to the oracle's PSF -- plus every refusal, which must come before anything is launched."""
import copy
import os

import numpy as np
import pytest

import otf_np
from oracle.run_np import run as oracle_run
from paos_amd.chains import parse_config_variant, syn20_chain, syn20_wavelength
from paos_amd.parse_config import parse_config
from paos_amd.run import run_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENS = os.path.join(ROOT, "data", "lens")
FIELD = {"us": 0.0, "ut": 0.0}
TOL = 1.0e-10  # the project's fp64 parity gate, max-abs on the DC-normalised result (|OTF| <= 1)

# Worst |restatement - long double| over the OTF of a seeded random 64^2 PSF, measured: 5.8e-17 (the restatement is
# np.fft in fp64; the values are <= 1).  Ten times that:
RESTATEMENT_TOL = 5.8e-16
# Clear circular pupil (Hubble_simple without its obscurations), 256^2 at zoom 4 -- a 64-pixel pupil: worst |cut - formula|
# of the restatement applied to the oracle's PSF, measured 9.2e-3 along x and along y (at the lowest frequencies: the
# discretised pupil edge and the PSF wings the finite grid cuts off).  Twice that:
CIRCLE_TOL = 1.9e-2
# ... and the largest value of those cuts beyond the cut-off (from s = 1 + 2/64 on: the partly covered edge pixels widen
# the pupil by up to a pixel), measured 5.4e-7 -- not the 1e-16 of rounding: the chain propagates between two mirrors
# on a finite grid, so its PSF is not strictly band-limited.  Twice that:
CIRCLE_ZERO_TOL = 1.1e-6


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


def _last_num(chain):
    return chain[list(chain.keys())[-1]]["num"]


def _random_psf(n, seed=808):
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    return u.real**2 + u.imag**2


def test_restatement_against_long_double():
    """np.fft with the shifts against the defining double sum in long double, 64^2, seeded random PSF: worst deviation
    measured 5.8e-17; asserted at RESTATEMENT_TOL = 5.8e-16 (10x).  The same for a PSF that sums to zero: zeros."""
    psf = _random_psf(64)
    want = otf_np.otf_longdouble(psf)
    got = otf_np.otf(psf)
    err = float(np.max(np.abs(got - want)))
    print(f"restatement vs long double, 64^2: max |dOTF| = {err:.2e} (tolerance {RESTATEMENT_TOL:.1e})")
    assert err <= RESTATEMENT_TOL
    assert got[32, 32] == 1.0 + 0.0j
    assert abs(float(np.max(np.abs(want))) - 1.0) < 1e-18
    assert not otf_np.otf(np.zeros((64, 64))).any() and not otf_np.otf_longdouble(np.zeros((64, 64))).any()


@pytest.mark.parametrize("n,k0,j0", [(64, 21, 40), (128, 70, 3)])
def test_single_pixel_gives_the_phase_ramp(n, k0, j0):
    """One bright pixel off centre, asymmetric: MTF == 1 everywhere and the OTF is the exact phase ramp, the sign of
    both axes included."""
    psf = np.zeros((n, n))
    psf[k0, j0] = 3.7
    got = otf_np.otf(psf)
    assert np.max(np.abs(np.abs(got) - 1.0)) <= RESTATEMENT_TOL
    assert np.max(np.abs(got - otf_np.phase_ramp(n, k0, j0))) <= RESTATEMENT_TOL
    # the ramp is not symmetric in its axes: a transposed or mirrored restatement would show
    assert np.max(np.abs(got - otf_np.phase_ramp(n, j0, k0))) > 0.5
    assert np.max(np.abs(got - np.conj(otf_np.phase_ramp(n, k0, j0)))) > 0.5


def _clear_hubble():
    """Hubble_simple without its obscurations (pads, secondary, vanes): a clear circular pupil."""
    pup, par, wls, fields, chains = parse_config(os.path.join(LENS, "Hubble_simple.ini"))
    chain = {}
    for key, item in chains[0].items():
        item = copy.copy(item)
        ap = item.get("aperture")
        if ap is not None and ap["type"] == "obscuration":
            del item["aperture"]
        chain[key] = item
    return pup, 1e-6 * wls[0], fields[0], chain


def test_clear_circular_pupil_against_the_diffraction_mtf():
    """run_batch on the model device, Hubble_simple without its obscurations at 256^2, zoom 4: both cuts against
    (2 / pi)(acos s - s sqrt(1 - s^2)), s = f wl F#.  Measured with the restatement on the oracle's PSF: worst deviation
    9.2e-3 on either cut (asserted at CIRCLE_TOL = 1.9e-2, 2x), largest value beyond the cut-off 5.4e-7 (asserted at
    CIRCLE_ZERO_TOL = 1.1e-6, 2x)."""
    n, zoom = 256, 4
    pup, wl, field, chain = _clear_hubble()
    num = _last_num(chain)
    ref = oracle_run(pup, wl, n, zoom, field, chain)[num]
    rx, ry = otf_np.cuts_of(otf_np.mtf(ref["amplitude"] ** 2))
    rec = run_batch(pup, [wl], n, zoom, field, [chain], outputs=(), mtf_cuts=True, dev=otf_np.OtfModelDevice(n, 1))[0][num]
    assert rec["dx"] == ref["dx"] and rec["fratio"] == ref["fratio"]
    for name, cut, restated, f in (("x", rec["mtf_x"], rx, rec["freq_x"]), ("y", rec["mtf_y"], ry, rec["freq_y"])):
        s = f * wl * rec["fratio"]
        want = otf_np.diffraction_mtf(f, wl, rec["fratio"])
        assert s[-1] > 1.5 and np.sum(s < 1.0) > 30, "the cut-off must lie well inside the cut"
        inside, beyond = s < 1.0, s >= 1.0 + 2.0 / np.sum(s < 1.0)  # (one sample of slack for the pupil's edge pixels)
        print(f"clear pupil, cut along {name}: restatement-of-oracle max |MTF - formula| = {np.max(np.abs(restated - want)):.2e}, "
              f"beyond the cut-off max {np.max(restated[beyond]):.2e}; model device {np.max(np.abs(cut - want)):.2e}, "
              f"{np.max(cut[beyond]):.2e}")
        assert np.max(np.abs(cut - want)) <= CIRCLE_TOL
        assert np.max(np.abs(cut[inside] - want[inside])) <= CIRCLE_TOL
        assert np.max(cut[beyond]) <= CIRCLE_ZERO_TOL


@pytest.mark.parametrize("name", ["Hubble_simple", "SYN20", "Ariel_AIRS-CH0"])
def test_run_batch_against_the_restatement_of_the_oracle_psf(name):
    pup, zoom, field, wls, chains, n = _case(name)
    num = _last_num(chains[0])
    dev = otf_np.OtfModelDevice(n, len(wls))
    res = run_batch(pup, wls, n, zoom, field, chains, outputs=("psf", "mtf", "otf"), mtf_cuts=True, dev=dev)
    plain = run_batch(pup, wls, n, zoom, field, chains, outputs=("psf",), dev=otf_np.OtfModelDevice(n, len(wls)))
    assert [what for what, _ in dev.log].count("otf_compute") == 1 and [what for what, _ in dev.log].count("otf_cuts") == 1
    h = n // 2
    for i, (wl, chain) in enumerate(zip(wls, chains)):
        ref = oracle_run(pup, wl, n, zoom, field, chain)[num]
        want = otf_np.otf(ref["amplitude"] ** 2)
        rec = res[i][num]
        assert rec["mtf"].shape == (n, n) and rec["mtf"].dtype == np.float64
        assert rec["otf"].shape == (n, n) and rec["otf"].dtype == np.complex128
        assert np.max(np.abs(rec["otf"] - want)) < TOL and np.max(np.abs(rec["mtf"] - np.abs(want))) < TOL
        assert rec["otf"][h, h] == 1.0 + 0.0j and rec["mtf"][h, h] == 1.0
        # the cuts are row N/2 and column N/2 of the full array from the centre outwards, Nyquist by the point symmetry
        assert np.array_equal(rec["mtf_x"][:h], rec["mtf"][h, h:]) and rec["mtf_x"][h] == rec["mtf"][h, 0]
        assert np.array_equal(rec["mtf_y"][:h], rec["mtf"][h:, h]) and rec["mtf_y"][h] == rec["mtf"][0, h]
        for axis, d in (("x", rec["dx"]), ("y", rec["dy"])):
            f = rec["freq_" + axis]
            assert f.shape == (h + 1,) and f[0] == 0.0 and f[-1] == 1.0 / (2.0 * d)
            assert np.array_equal(f, otf_np.freqs(n, d))
        # only the last surface's record carries them, and nothing else changed
        for key, other in res[i].items():
            assert sorted(set(other) - {"mtf", "otf", "mtf_x", "mtf_y", "freq_x", "freq_y"}) == sorted(plain[i][key])
            if key != num:
                assert not {"mtf", "otf", "mtf_x", "mtf_y", "freq_x", "freq_y"} & set(other)
            for k, v in plain[i][key].items():
                if isinstance(v, np.ndarray):
                    assert np.array_equal(other[k], v), (key, k)
                elif k not in ("ABCDt", "ABCDs", "aperture"):
                    assert other[k] == v, (key, k)


def test_the_lean_walk_and_the_focus_planes():
    """outputs=() with mtf_cuts runs on the lean walk (the PSF comes out of the last pass) and gives the ordinary walk's
    cuts; every plane of a focus stack gets the same keys, the nominal plane the nominal record's arrays."""
    n, wls = 64, [syn20_wavelength(k) for k in (0, 300)]
    chains = [syn20_chain() for _ in wls]
    dev = otf_np.OtfModelDevice(n, len(wls))
    lean = run_batch(1.0, wls, n, 4, FIELD, chains, outputs=(), mtf_cuts=True, dev=dev)
    assert not any(what in ("otf_fetch", "download") for what, _ in dev.log) and [w for w, _ in dev.log].count("otf_cuts") == 1
    full = run_batch(1.0, wls, n, 4, FIELD, chains, outputs=("psf", "mtf"), mtf_cuts=True, dev=otf_np.OtfModelDevice(n, len(wls)))
    planes = [1.0e-4, 0.0, -6.0e-5]
    stack = run_batch(1.0, wls, n, 4, FIELD, chains, outputs=("psf", "mtf", "otf"), mtf_cuts=True, focus_planes=planes,
                      dev=otf_np.OtfModelDevice(n, len(wls)))
    for i in range(len(wls)):
        assert "psf" not in lean[i][20] and "mtf" not in lean[i][20]
        for key in ("mtf_x", "mtf_y"):
            assert np.max(np.abs(lean[i][20][key] - full[i][20][key])) < TOL
        for key in ("freq_x", "freq_y"):
            assert np.array_equal(lean[i][20][key], full[i][20][key])
        rec = stack[i][20]
        assert np.array_equal(rec["mtf"], full[i][20]["mtf"])
        for p in rec["focus"]:
            assert {"mtf", "otf", "mtf_x", "mtf_y", "freq_x", "freq_y"} <= set(p)
            assert np.max(np.abs(p["otf"] - otf_np.otf(p["psf"]))) < TOL
            if p["dz"] == 0.0:
                for key in ("mtf", "otf", "mtf_x", "mtf_y", "freq_x", "freq_y"):
                    assert np.array_equal(p[key], rec[key]), key
            else:
                assert np.max(np.abs(p["mtf"] - rec["mtf"])) > 1e-6  # defocus does change the MTF


def _refused(**kw):
    n = 64
    chains = kw.pop("chains", [syn20_chain(), syn20_chain()])
    dev = otf_np.OtfModelDevice(n, 2)
    with pytest.raises(ValueError) as err:
        run_batch(1.0, [1.0e-6, 1.2e-6], n, 4, FIELD, chains, dev=dev, **kw)
    assert dev.log == [] and not dev.u.any(), "something was launched before the refusal"
    return str(err.value)


def test_refusals_come_before_any_launch():
    unsaved = syn20_chain()
    unsaved[20] = dict(unsaved[20], save=False)
    for kw in (dict(outputs=("mtf",)), dict(outputs=("psf", "otf")), dict(outputs=(), mtf_cuts=True)):
        assert "saved" in _refused(chains=[unsaved, unsaved], **kw)
        assert "sync" in _refused(sync=False, **kw)
    _refused(outputs=("mtf", "ctf"))  # still an unknown output


def test_run_sharded_does_not_take_them():
    from paos_amd.dist import run_sharded

    made = []

    def make(n, nb):
        made.append(otf_np.OtfModelDevice(n, nb))
        return made[-1]

    for outputs in (("mtf",), ("psf", "otf")):
        with pytest.raises(ValueError):
            run_sharded(1.0, [1.0e-6], 64, 4, FIELD, [syn20_chain()], batch=1, outputs=outputs, make_device=make)
    assert not made


def test_the_model_device_refuses_what_the_library_refuses():
    """compute before a PSF is kept; fetch and cuts before a compute; both after a newer psf_keep; a bad item or `what`."""
    from paos_amd import _lib

    dev = otf_np.OtfModelDevice(64, 2)
    dev.u[:] = np.sqrt(_random_psf(64))
    with pytest.raises(_lib.PaosHipError):
        dev.otf_compute()
    dev.psf_keep()
    for call in (dev.otf_fetch, dev.otf_cuts):
        with pytest.raises(_lib.PaosHipError):
            call()
    dev.otf_compute()
    first = dev.otf_fetch(1, "otf")
    with pytest.raises(_lib.PaosHipError):
        dev.otf_fetch(2)
    with pytest.raises(ValueError):
        dev.otf_fetch(0, "ptf")
    dev.psf_keep()
    for call in (dev.otf_fetch, dev.otf_cuts):
        with pytest.raises(_lib.PaosHipError):
            call()
    dev.otf_compute()
    assert np.array_equal(dev.otf_fetch(1, "otf"), first)
