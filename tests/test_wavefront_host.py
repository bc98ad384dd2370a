"""Wavefront fits on the host: the fp64 restatement against the long-double reference, the exact cases of the definition,
the round trip of an injected aberration, ``run_batch(wavefront=...)`` on the NumPy model of the device against the
restatement applied to the oracle's field -- SYN20's wfe variants and the lens file periscope.ini --, ``WFO.fit_zernikes``
and every refusal."""
import numpy as np
import pytest

import wavefront_np as wnp
from oracle.run_np import run as oracle_run
from paos_amd.chains import syn20_chain, syn20_coefficients, syn20_wavelength
from paos_amd.run import run_batch
from paos_amd.wavefront import MAX_TERMS, WavefrontFit, fit_from_sums
from paos_amd.zernike import Zernike

FIELD = {"us": 0.0, "ut": 0.0}
WL = 1.0e-6
DX = 1.0e-3


def _fit(u, terms, radius, wl=WL, dx=DX, dy=DX, ordering="standard", normalize=True, **kw):
    m, n = Zernike.j2mn(terms, ordering)
    summary, sums = wnp.fit_sums_np(u, m, n, normalize, dx, dy, radius, **kw)
    return fit_from_sums(summary, sums, terms, wl), summary, sums


def _aberrated(npix, terms, radius_px, seed, peak=2.0, wl=WL, ordering="standard"):
    """(field, injected coefficients [m]): a seeded wfe of ``terms`` coefficients scaled so that the phase reaches
    ``peak`` rad, under a non-uniform amplitude."""
    rng = np.random.default_rng(seed)
    m, n = Zernike.j2mn(terms, ordering)
    coeffs = rng.normal(0.0, 1.0, terms) / (1.0 + np.arange(terms))
    coeffs[0] = 0.0
    yy, xx = np.mgrid[0:npix, 0:npix] - npix // 2
    amp = 0.5 + np.exp(-((xx - 3.0) ** 2 + (yy + 2.0) ** 2) / (2.0 * (0.8 * radius_px) ** 2))
    unit = wnp.aberrated_field(npix, m, n, True, coeffs, 1.0, DX, DX, radius_px * DX)
    coeffs *= peak / np.max(np.abs(np.angle(unit))) * wl / (2.0 * np.pi) if terms > 1 else 0.0
    return wnp.aberrated_field(npix, m, n, True, coeffs, wl, DX, DX, radius_px * DX, amplitude=amp), coeffs


# ---- the restatement against the long-double reference -------------------------------------------------------------
@pytest.mark.parametrize("weight", ["uniform", "intensity"])
def test_restatement_against_the_long_double_reference(weight):
    wnp.px.require_long_double()
    u, _ = _aberrated(64, 15, 24.5, seed=1)
    m, n = Zernike.j2mn(15, "standard")
    kw = dict(offset_deg=12.0, origin="y", weight=weight, min_intensity=0.3)
    summary, sums = wnp.fit_sums_np(u, m, n, True, DX, 1.1 * DX, 24.5 * DX, **kw)
    vals, bounds = wnp.moments_ld(u, DX, 1.1 * DX, 24.5 * DX, min_intensity=0.3)
    assert summary[0] == float(vals[0]) and summary[0] > 100
    assert np.all(np.abs(summary[1:5] - vals[1:]) <= bounds[1:])
    ref = wnp.fit_sums_ld(u, m, n, True, DX, 1.1 * DX, 24.5 * DX, (summary[1], summary[2]), **kw)
    assert ref["count"] == summary[0]
    assert np.all(np.abs(sums - ref["sums"]) <= ref["sums_bound"])
    assert abs(summary[8] - ref["sw"]) <= ref["sw_bound"] and abs(summary[9] - ref["swphi"]) <= ref["swphi_bound"]
    assert abs(summary[5] - ref["phi_min"]) <= ref["e_phi"] and abs(summary[6] - ref["phi_max"]) <= ref["e_phi"]


# ---- exact cases ------------------------------------------------------------------------------------------------------
def test_a_constant_field_is_flat_exactly():
    """3 - 4i: a constant whose modulus, 5, and whose sums over the disk are integers, so that |r|^2 and (sum sqrt I)^2 are
    the same number exactly (with an inexact square root the two differ in the last bits)."""
    u = np.full((64, 64), 3.0 - 4.0j)
    for weight in ("uniform", "intensity"):
        fit, summary, _ = _fit(u, 10, 20.0 * DX, weight=weight)
        assert summary[5] == 0.0 and summary[6] == 0.0
        assert np.all(fit["wf_coeff"] == 0.0) and fit["wf_rms"] == 0.0 and fit["wf_residual_rms"] == 0.0 and fit["wf_pv"] == 0.0
        assert fit["wf_strehl"] == 1.0 and not fit["wf_fallback"] and not fit["wf_singular"]
        assert fit["wf_pixels"] == summary[0] > 1000


@pytest.mark.parametrize("zero", [0.0, -0.0])
def test_a_pixel_opposite_to_r_reads_plus_or_minus_pi(zero):
    u = np.full((64, 64), complex(1.0, zero))
    u[32, 35] = complex(-1.0, zero)
    # about r = 300 + zero i (a sum of zeros loses the sign, so r is given): im' = fl(uy rx) - fl(ux ry) = zero + zero
    fit, summary, _ = _fit(u, 3, 10.0 * DX, r=(300.0, zero))
    rp, ip = wnp.turned(-1.0, zero, 300.0, zero)
    want = np.arctan2(ip, rp)
    assert want == (-np.pi if np.signbit(zero) else np.pi)
    assert (summary[5] if want < 0 else summary[6]) == want and (summary[6] if want < 0 else summary[5]) == 0.0
    assert fit["wf_phase_absmax"] == np.pi and fit["wf_pv"] == pytest.approx(WL / 2, rel=1e-15)


# ---- round trip -------------------------------------------------------------------------------------------------------
ROUND_TRIPS = [(15, 64, 24.5), (36, 64, 24.5), (15, 64, 8.0), (36, 64, 8.0), (36, 128, 50.3), (63, 256, 100.2)]


@pytest.mark.parametrize("terms, npix, radius_px", ROUND_TRIPS)
@pytest.mark.parametrize("weight", ["uniform", "intensity"])
def test_round_trip_recovers_the_injected_coefficients(terms, npix, radius_px, weight):
    """Stated condition: the inputs keep max |phi| <= 3.0 (nothing wraps).  Coefficients j >= 1 come back to 1e-12 of the
    largest one (measured on the CPU: 4-8e-16; cond(G) <= 3.4)."""
    u, coeffs = _aberrated(npix, terms, radius_px, seed=terms + npix)
    fit, summary, _ = _fit(u, terms, radius_px * DX, weight=weight)
    assert fit["wf_phase_absmax"] <= 3.0
    err = np.max(np.abs(fit["wf_coeff"][1:] - coeffs[1:])) / np.max(np.abs(coeffs))
    print(f"round trip K={terms} N={npix} r={radius_px}px {weight}: {err:.2e} of the largest coefficient, "
          f"max|phi| {fit['wf_phase_absmax']:.3f}")
    assert err <= 1.0e-12
    assert fit["wf_residual_rms"] <= 1.0e-7 * fit["wf_rms"]  # (the square root of a difference of sums that cancel to ~1e-16)
    assert fit["wf_pixels"] == summary[0]


def test_strehl_against_the_marechal_approximation():
    """Uniform amplitude, small aberration: |<exp(i phi)>|^2 = exp(-var phi) up to O(var^2)."""
    m, n = Zernike.j2mn(15, "standard")
    coeffs = np.zeros(15)
    coeffs[4], coeffs[7], coeffs[12] = 12.0e-9, -8.0e-9, 5.0e-9
    u = wnp.aberrated_field(128, m, n, True, coeffs, WL, DX, DX, 50.3 * DX)
    fit, _, _ = _fit(u, 15, 50.3 * DX)
    var = (2.0 * np.pi * fit["wf_rms"] / WL) ** 2
    assert 0.005 < var < 0.02
    assert abs(fit["wf_strehl"] - np.exp(-var)) <= var * var
    assert abs(fit["wf_rms"] - np.sqrt(np.sum(coeffs**2))) <= 0.02 * fit["wf_rms"]  # orthonormal up to the sampling of the disk


def test_the_fallback_when_the_field_sums_to_zero():
    u = np.ones((64, 64), dtype=np.complex128)
    u[:, 32:] = -1.0  # x >= 0 against x < 0 ...
    u[:, 32] = 0.0    # ... without the centre column, which has no partner: the sum over the disk is exactly zero
    fit, summary, _ = _fit(u, 3, 20.0 * DX, min_intensity=0.5)
    assert summary[1] == 0.0 and summary[2] == 0.0 and summary[7] == 1.0
    assert fit["wf_fallback"] and fit["wf_strehl"] == 0.0
    assert summary[5] == 0.0 and summary[6] == np.pi  # phi about 1 + 0i: 0 on the left, atan2(+0, -1) on the right


def test_an_empty_support_and_a_singular_matrix_are_reported():
    u = np.ones((64, 64), dtype=np.complex128)
    fit, summary, sums = _fit(u, 6, 20.0 * DX, min_intensity=2.0)  # no pixel is bright enough
    assert summary[0] == 0 and not sums.any()
    assert fit["wf_pixels"] == 0 and np.all(np.isnan(fit["wf_coeff"])) and np.isnan(fit["wf_rms"]) and np.isnan(fit["wf_residual_rms"])
    assert not fit["wf_singular"]
    fit, summary, _ = _fit(u, 10, 1.2 * DX)  # five pixels, ten terms
    assert summary[0] == 5
    assert fit["wf_singular"] and np.all(np.isnan(fit["wf_coeff"])) and np.isnan(fit["wf_rms"]) and fit["wf_pixels"] == 5


# ---- run_batch on the model device ---------------------------------------------------------------------------------
def _syn20_variants(nb):
    """SYN20 with the Zernike surface saved and a different seeded wfe per item: the chain's own draw, then draws of
    8 nm per term -- the stated condition is that the phase stays inside +-3 rad (the 20 nm draw of seed 2021 wraps)."""
    chains, coeffs = [], []
    for k in range(nb):
        c = syn20_coefficients() if k == 0 else syn20_coefficients(rng_seed=2021 + k, sigma=8.0e-9)
        chain = syn20_chain(c)
        chain[2]["save"] = True
        chains.append(chain)
        coeffs.append(c)
    return chains, coeffs


@pytest.fixture(scope="module")
def syn20_run():
    n, nb = 64, 2
    wls = [syn20_wavelength(0), syn20_wavelength(300)]
    chains, coeffs = _syn20_variants(nb)
    at_z = WavefrontFit(36, 0.5, surfaces=(2,))
    at_image = WavefrontFit(6, np.array([2.0e-3, 2.5e-3]), weight="intensity", min_intensity=1e-9, surfaces=[20])
    dev = wnp.WavefrontModelDevice(n, nb)
    res = run_batch(1.0, wls, n, 4, FIELD, chains, outputs=("wfo",), dev=dev, wavefront=[at_z, at_image])
    return n, wls, chains, coeffs, res, dev


def test_run_batch_recovers_the_injected_coefficients_at_the_zernike_surface(syn20_run):
    n, wls, chains, coeffs, res, _ = syn20_run
    for i, c in enumerate(coeffs):
        rec = res[i][2]
        assert rec["wf_phase_absmax"] <= 3.0 and not rec["wf_fallback"] and not rec["wf_singular"]
        err = np.max(np.abs(rec["wf_coeff"][1:] - c[1:])) / np.max(np.abs(c))
        print(f"SYN20 item {i}: injected coefficients recovered to {err:.2e} of the largest")
        assert err <= 1.0e-12
        assert "wf_coeff" not in res[i][1]


def test_run_batch_equals_the_restatement_on_the_oracle_field(syn20_run):
    n, wls, chains, coeffs, res, dev = syn20_run
    assert [name for name, _ in dev.log].count("wavefront_fit") == 2  # one fit per named surface, whole batch
    m, nn = Zernike.j2mn(6, "standard")
    for i, (wl, radius) in enumerate(zip(wls, (2.0e-3, 2.5e-3))):
        ref = oracle_run(1.0, wl, n, 4, FIELD, chains[i])[20]
        rec = res[i][20]
        summary, sums = wnp.fit_sums_np(ref["wfo"], m, nn, True, ref["dx"], ref["dy"], radius, weight="intensity", min_intensity=1e-9)
        want = fit_from_sums(summary, sums, 6, wl)
        assert rec["wf_pixels"] == want["wf_pixels"] > 6
        # the model's field agrees with the oracle's to the project's parity gate (1e-10 of its peak)
        assert np.allclose(rec["wf_coeff"], want["wf_coeff"], rtol=0, atol=1e-7 * wl)
        assert abs(rec["wf_strehl"] - want["wf_strehl"]) <= 1e-8 and abs(rec["wf_rms"] - want["wf_rms"]) <= 1e-7 * wl


def test_run_batch_on_a_lens_file_with_a_zernike_surface():
    """data/lens/periscope.ini: surface 7 is a saved Zernike surface with one coefficient, 0.05 waves at 3 um = 1.5e-7 m of
    the fourth polynomial, not normalised, on the beam radius 0.05 m; the phase stays within 0.7 rad at both wavelengths.
    The beam has travelled from the stop over two mirrors, so its phase in front of the surface is not flat.  Three
    checks: every wf_* entry against the restatement on the oracle's field; the coefficients against those of the same
    file with the surface's coefficients set to zero -- the fit is linear in the phase and the support does not move, so
    the difference is the injection, to the round trip's 1e-12 of the largest coefficient; and the coefficients as they
    come out against the injection, within what diffraction puts in front of the surface.  That tolerance is stated, not
    fitted: the Fresnel ripple of a 0.05 m beam after about a metre has a phase amplitude of a few hundredths of a
    radian, of which a low-order polynomial picks up a fraction -- 2 % of the injected 0.31 / 0.94 rad is taken, and the
    flat file's own coefficients, which are that contribution, are held to it as well."""
    import os

    from paos_amd.parse_config import parse_config

    lens = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "data", "lens", "periscope.ini")
    pup, par, wls_um, fields, chains = parse_config(lens)
    n, num, terms = 128, 7, 6
    wls = [1.0e-6 * w for w in wls_um]
    z = chains[0][num]
    assert z["type"] == "Zernike" and z["save"] and not z["Znormalize"] and z["Zordering"] == "standard"
    injected = np.asarray(z["Z"], dtype=np.float64)
    flat = []
    for chain in chains:
        twin = dict(chain)
        twin[num] = dict(chain[num], Z=np.zeros_like(injected))
        flat.append(twin)
    refs = [oracle_run(pup, wl, n, par["zoom"], fields[0], chain)[num] for wl, chain in zip(wls, chains)]
    floors = [0.25 * np.max(np.abs(ref["wfo"]) ** 2) for ref in refs]  # the lit part of the beam
    # the file leaves Zradius empty: the surface then takes the beam radius there, 0.05 m but for its last digits, and a
    # radius that differs by 2e-10 of itself shows in the defocus term at twice that
    radii = [ref["wz"] for ref in refs]
    assert all(abs(r - 0.05) < 1e-9 for r in radii)
    wf = WavefrontFit(terms, radii, normalize=False, min_intensity=floors, surfaces=(num,))
    got = run_batch(pup, wls, n, par["zoom"], fields[0], chains, outputs=(), dev=wnp.WavefrontModelDevice(n, 2), wavefront=wf)
    base = run_batch(pup, wls, n, par["zoom"], fields[0], flat, outputs=(), dev=wnp.WavefrontModelDevice(n, 2), wavefront=wf)
    m, nn = Zernike.j2mn(terms, "standard")
    for i, (wl, ref) in enumerate(zip(wls, refs)):
        rec, zero = got[i][num], base[i][num]
        assert rec["wf_phase_absmax"] <= 0.7 and not rec["wf_fallback"] and not rec["wf_singular"]
        want = fit_from_sums(*wnp.fit_sums_np(ref["wfo"], m, nn, False, ref["dx"], ref["dy"], radii[i], min_intensity=floors[i]), terms, wl)
        assert rec["wf_pixels"] == want["wf_pixels"] == zero["wf_pixels"] > 300
        # (the model's field agrees with the oracle's to the project's parity gate, as at SYN20's image plane)
        assert np.allclose(rec["wf_coeff"], want["wf_coeff"], rtol=0, atol=1e-7 * wl)
        assert abs(rec["wf_strehl"] - want["wf_strehl"]) <= 1e-8 and abs(rec["wf_rms"] - want["wf_rms"]) <= 1e-7 * wl
        assert abs(rec["wf_pv"] - want["wf_pv"]) <= 1e-7 * wl and rec["wf_phase_absmax"] == pytest.approx(want["wf_phase_absmax"], abs=1e-7)
        largest = np.max(np.abs(injected))
        step = rec["wf_coeff"] - zero["wf_coeff"]
        err = np.max(np.abs(step[1:] - injected[1:])) / largest
        direct = np.max(np.abs(rec["wf_coeff"][1:] - injected[1:])) / largest
        print(f"periscope item {i}: injection recovered to {err:.2e} of it against the flat file, {direct:.2e} as it comes out")
        assert err <= 1.0e-12
        assert direct <= 0.02 and np.max(np.abs(zero["wf_coeff"][1:])) <= 0.02 * largest


def test_focus_planes_get_nothing():
    import focus_np

    class Device(wnp.WavefrontModelDevice, focus_np.FocusModelDevice):
        pass

    n, wls = 64, [syn20_wavelength(0), syn20_wavelength(300)]
    chains = [syn20_chain(), syn20_chain()]
    res = run_batch(1.0, wls, n, 4, FIELD, chains, outputs=(), dev=Device(n, 2), focus_planes=[-2.0e-4, 0.0, 2.0e-4],
                    wavefront=WavefrontFit(6, 2.0e-3, weight="intensity", min_intensity=1e-9, surfaces=(20,)))
    for item in res:
        assert "wf_coeff" in item[20] and len(item[20]["focus"]) == 3
        assert not any(key.startswith("wf_") for plane in item[20]["focus"] for key in plane)


def test_surfaces_none_fits_every_saved_surface():
    chains, _ = _syn20_variants(1)
    res = run_batch(1.0, [1.0e-6], 64, 4, FIELD, chains, outputs=(), dev=wnp.WavefrontModelDevice(64, 1),
                    wavefront=WavefrontFit(3, 0.5))
    assert all("wf_coeff" in res[0][num] for num in (1, 2, 20))
    assert res[0][1]["wf_rms"] == 0.0 and res[0][1]["wf_strehl"] == pytest.approx(1.0, abs=1e-12)


def test_wfo_fit_zernikes(monkeypatch):
    from paos_amd import wfo as wfo_mod

    monkeypatch.setattr(wfo_mod._lib, "DeviceFields", wnp.WavefrontModelDevice)
    w = wfo_mod.WFO(1.0, WL, 64, 4)
    w.aperture(0.0, 0.0, hx=0.5, hy=0.5, shape="elliptical")
    coeffs = np.array([0.0, 30e-9, -20e-9, 50e-9, 10e-9, -15e-9])
    w.zernikes(np.arange(6), coeffs, "standard", True, 0.5, offset=7.0, origin="y")
    fit = w.fit_zernikes(6, 0.5, offset=7.0, origin="y", min_intensity=0.5)
    assert set(fit) == {"wf_coeff", "wf_rms", "wf_residual_rms", "wf_pv", "wf_strehl", "wf_pixels", "wf_phase_absmax",
                        "wf_fallback", "wf_singular"}
    assert np.max(np.abs(fit["wf_coeff"][1:] - coeffs[1:])) <= 1e-12 * 50e-9


# ---- refusals ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [
    dict(terms=0), dict(terms=MAX_TERMS + 1), dict(terms=3.0), dict(terms=True), dict(ordering="zemax"), dict(origin="z"),
    dict(weight="amplitude"), dict(radius=0.0), dict(radius=-1.0), dict(radius=np.nan), dict(radius=[0.5, np.inf]),
    dict(radius="wide"), dict(offset=np.inf), dict(offset=[1.0, 2.0]), dict(min_intensity=-1.0), dict(min_intensity=np.nan),
    dict(surfaces=5),
])
def test_the_request_refuses_on_its_own(kw):
    args = dict(terms=6, radius=0.5)
    args.update(kw)
    with pytest.raises(ValueError):
        WavefrontFit(**args)


def test_the_request_is_exported():
    import paos_amd

    assert paos_amd.WavefrontFit is WavefrontFit and "WavefrontFit" in paos_amd.__all__


def _refused(match, wavefront, chains=None, **kw):
    chains = chains or [syn20_chain(), syn20_chain()]
    dev = wnp.WavefrontModelDevice(64, 2)
    with pytest.raises(ValueError, match=match):
        run_batch(1.0, [1.0e-6, 1.2e-6], 64, 4, FIELD, chains, dev=dev, wavefront=wavefront, **kw)
    assert not dev.log, "refused before anything was launched"


def test_run_batch_refuses_before_any_launch():
    ok = WavefrontFit(6, 0.5, surfaces=(20,))
    _refused("WavefrontFit", "zernike")
    _refused("WavefrontFit", [ok, 36])
    _refused("WavefrontFit", 36)
    _refused("sync=False", ok, sync=False)
    _refused("not a saved surface", WavefrontFit(6, 0.5, surfaces=(2,)))   # exists, not saved
    _refused("not a saved surface", WavefrontFit(6, 0.5, surfaces=(99,)))  # does not exist
    half = [syn20_chain(), syn20_chain()]
    half[1][20]["save"] = False
    _refused("not a saved surface", ok, chains=half)
    _refused("two requests", [ok, WavefrontFit(3, 0.4, surfaces=(1, 20))])
    _refused("two requests", [ok, WavefrontFit(3, 0.4)])
    _refused("one value per item", WavefrontFit(6, [0.5, 0.4, 0.3], surfaces=(20,)))
    _refused("one value per item", WavefrontFit(6, 0.5, min_intensity=[0.0, 0.0, 0.0], surfaces=(20,)))


@pytest.mark.parametrize("entry", ["run_sharded", "run_broadband", "pipeline"])
def test_the_other_entry_points_do_not_take_the_keyword(entry):
    import inspect

    if entry == "pipeline":
        from paos_amd.pipeline import pipeline as fn
    elif entry == "run_sharded":
        from paos_amd.dist import run_sharded as fn
    else:
        from paos_amd.detector import run_broadband as fn
    params = inspect.signature(fn).parameters
    assert "wavefront" not in params and not any(p.kind is p.VAR_KEYWORD for p in params.values())
