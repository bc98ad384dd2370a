"""Wavefront fits on the GPU (paos_wavefront_fit / paos_wavefront_fetch, run_batch(wavefront=...); csrc/wavefront_pass.h):
the summary and the sums against the long-double reference of tests/wavefront_np.py on the downloaded field, at bounds
built from the project's constants; the exact cases, the fallback, the bit-for-bit invariants, a fit behind a deferred
stop, the run_batch path and misuse of the C calls.  ``pytest -s`` prints the largest observed fraction of each bound
(XPREC lines: profiles/r22_wavefront_xprec.md)."""
import numpy as np
import pytest

import wavefront_np as wnp
from paos_amd.planner import gram_polynomials, jacobi_recurrence, zernike_block
from paos_amd.zernike import Zernike, norm_factors

pytestmark = pytest.mark.gpu

FIELD = {"us": 0.0, "ut": 0.0}
WL = 1.0e-6
OBSERVED = {}  # bound name -> largest |got - ref| / bound seen by the tests of this module


def _note(name, err, bound):
    frac = float(err) / float(bound) if bound > 0 else (0.0 if err == 0 else np.inf)
    OBSERVED[name] = max(OBSERVED.get(name, 0.0), frac)
    return frac


def _field(n, seed, radius_px, dark=False):
    """An aberrated beam: a smooth phase that stays within +-2.6 rad of its mean over the disk, a little seeded phase
    noise, under a decentred Gaussian amplitude; ``dark``: a seeded tenth of the pixels at a hundredth of the amplitude."""
    rng = np.random.default_rng(220000 + 13 * n + seed)
    j = (np.arange(n) - n // 2) / float(radius_px)
    x, y = j[None, :], j[:, None]
    phase = (0.7 - 0.1 * seed) * x - 0.5 * y + 0.8 * (x * x - y * y) + 0.5 * x * y * y + 0.05 * rng.standard_normal((n, n))
    amp = 0.3 + np.exp(-((x - 0.2) ** 2 + (y + 0.1) ** 2))
    if dark:
        amp = np.where(rng.random((n, n)) < 0.1, 0.01 * amp, amp)
    return amp * np.exp(1j * phase)


def _item(dx, radius_px, dy=None, offset=0.0, origin="x", enable=True):
    return dict(dx=dx, dy=dx if dy is None else dy, radius=radius_px * dx, offset=offset, origin=origin, enable=enable)


def _request(items, terms, ordering="standard", normalize=True):
    m, nn = Zernike.j2mn(terms, ordering)
    norm = norm_factors(m, nn, normalize)
    nmax = int(nn.max())
    blocks = []
    for it in items:
        b = zernike_block(m, nn, norm, np.zeros(terms), it["dx"], it["dy"], it["radius"], WL, origin=it["origin"],
                          offset_deg=it["offset"], nmax=nmax)[0]
        b[0] = 1.0 if it["enable"] else 0.0
        blocks.append(b[:8])
    return (nmax, nmax // 2 + 1, jacobi_recurrence(nmax), np.array(blocks), gram_polynomials(m, nn, norm)), m, nn


def _device(n, precision, fields):
    from paos_amd import _lib

    dev = _lib.DeviceFields(n, len(fields), precision)
    for i, u in enumerate(fields):
        dev.upload(i, u)
    return dev


def _check(dev, items, terms, weight="uniform", floors=None, pupils=None, normalize=True, what=""):
    """fit + fetch; every item against the long-double reference on the field the device holds: first the moments (count
    exact, r / sum sqrt I / sum I at the metric bound), then the phase sums about the DEVICE's r.  Returns (summary, sums)."""
    req, m, nn = _request(items, terms, normalize=normalize)
    nb = len(items)
    fl = np.zeros(nb) if floors is None else np.broadcast_to(np.asarray(floors, dtype=np.float64), (nb,))
    dev.wavefront_fit(*req, weight=1 if weight == "intensity" else 0, min_intensity=floors, pupil=pupils is not None)
    summary, sums = dev.wavefront_fetch()
    assert summary.shape == (nb, 10) and sums.shape == (nb, (terms + 1) * (terms + 2) // 2)
    for i, it in enumerate(items):
        tag = f"{what} item {i}"
        if not it["enable"]:
            assert not summary[i].any() and not sums[i].any(), tag
            continue
        u = dev.download(i)
        geo = dict(dx=it["dx"], dy=it["dy"], radius=it["radius"], min_intensity=float(fl[i]),
                   pupil=None if pupils is None else pupils[i])
        vals, bounds = wnp.moments_ld(u, **geo)
        assert summary[i, 0] == float(vals[0]), f"{tag}: count {summary[i, 0]} against {float(vals[0])}"
        for k, name in ((1, "r_re"), (2, "r_im"), (3, "sum_sqrt_I"), (4, "sum_I")):
            err = abs(np.longdouble(summary[i, k]) - vals[k])
            assert err <= bounds[k], f"{tag}: {name}: |got - ref| = {float(err):.3g} > bound {bounds[k]:.3g}"
            _note("moments", err, bounds[k])
        assert bool(summary[i, 7]) == wnp.used_phasor(summary[i, 1], summary[i, 2])[2], tag
        ref = wnp.fit_sums_ld(u, m, nn, normalize, r=(summary[i, 1], summary[i, 2]), offset_deg=it["offset"], origin=it["origin"],
                              weight=weight, **geo)
        err = np.abs(sums[i].astype(np.longdouble) - ref["sums"])
        worst = int(np.argmax(err - ref["sums_bound"]))
        assert np.all(err <= ref["sums_bound"]), (f"{tag}: sum {worst}: |got - ref| = {float(err[worst]):.3g} > bound "
                                                  f"{ref['sums_bound'][worst]:.3g}")
        q = 0
        for p in range(terms + 1):
            for s in range(p, terms + 1):
                if ref["sums_bound"][q] > 0:
                    _note("gram ZZ" if s < terms else ("gram Z phi" if p < terms else "gram phi phi"), err[q], ref["sums_bound"][q])
                q += 1
        for k, name in ((8, "sw"), (9, "swphi")):
            e = abs(np.longdouble(summary[i, k]) - ref[name])
            assert e <= ref[name + "_bound"], f"{tag}: {name}: |got - ref| = {float(e):.3g} > bound {ref[name + '_bound']:.3g}"
            if ref[name + "_bound"] > 0:
                _note("sum w, sum w phi", e, ref[name + "_bound"])
        for k, name in ((5, "phi_min"), (6, "phi_max")):
            e = abs(summary[i, k] - ref[name])
            assert e <= ref["e_phi"], f"{tag}: {name}: {summary[i, k]!r} against {ref[name]!r}"
            _note("phi_min, phi_max", e, ref["e_phi"])
    return summary, sums


# ---- against the long-double reference ------------------------------------------------------------------------------
@pytest.mark.parametrize("weight", ["uniform", "intensity"])
@pytest.mark.parametrize("terms", [1, 15, 63])
def test_a_small_batch_with_a_request_per_item(terms, weight):
    n, dx = 64, 1.0e-3
    items = [_item(dx, 24.5), _item(dx, 17.0, offset=33.0, origin="y", enable=False), _item(2 * dx, 28.3, offset=-12.5, origin="y")]
    dev = _device(n, "fp64", [_field(n, s, 24.0) for s in range(3)])
    try:
        summary, _ = _check(dev, items, terms, weight, what=f"64^2 K={terms} {weight}")
        assert summary[0, 0] > 1500 and summary[2, 0] > 2000
    finally:
        dev.close()


GRIDS = {
    "128 dx != dy": (128, "fp64", 15, [dict(dx=1.0e-3, dy=1.3e-3, radius=50.3e-3, offset=20.0, origin="x", enable=True)] * 2, 50.0),
    "256 fp32": (256, "fp32", 15, [_item(1.0e-3, 100.2), _item(1.0e-3, 61.0, origin="y")], 100.0),
    "1024 fp64 K=36": (1024, "fp64", 36, [_item(1.0e-4, 90.4)], 90.0),
    "2048 fp32": (2048, "fp32", 15, [_item(1.0e-4, 40.3)], 40.0),
}


@pytest.mark.parametrize("weight", ["uniform", "intensity"])
@pytest.mark.parametrize("name", list(GRIDS))
def test_grids_layouts_and_precisions(name, weight):
    """128^2 with dx != dy; 256^2 fp32; 1024^2 (more than one workgroup per item in both sweeps); 2048^2 fp32: the layout
    with blocks of eight rows, under a disk small enough for a cheap reference."""
    n, precision, terms, items, scale = GRIDS[name]
    dev = _device(n, precision, [_field(n, s, scale) for s in range(len(items))])
    try:
        _check(dev, items, terms, weight, what=f"{name} {weight}")
    finally:
        dev.close()


def test_the_floor_cuts_pixels():
    n, dx = 64, 1.0e-3
    items = [_item(dx, 24.5)] * 3
    fields = [_field(n, 5, 24.0, dark=True)] * 3
    dev = _device(n, "fp64", fields)
    try:
        for weight in ("uniform", "intensity"):
            summary, _ = _check(dev, items, 10, weight, floors=[0.0, 1.0e-3, 0.5], what=f"floor {weight}")
            assert summary[0, 0] > summary[1, 0] > summary[2, 0] > 100  # the dark tenth goes first, then the wings
    finally:
        dev.close()


def test_the_pupil_restricts_the_support():
    n, dx = 64, 1.0e-3
    rng = np.random.default_rng(7)
    pupils = [(rng.random((n, n)) < 0.8).astype(np.float64) * (1.0 + rng.random((n, n))) for _ in range(2)]
    items = [_item(dx, 24.5), _item(dx, 20.0, origin="y")]
    dev = _device(n, "fp64", [_field(n, s, 24.0) for s in range(2)])
    try:
        for i, w in enumerate(pupils):
            dev.pupil_upload(i, w)
        with_pupil, _ = _check(dev, items, 10, "intensity", pupils=pupils, what="pupil")
        without, _ = _check(dev, items, 10, "intensity", what="no pupil")
        assert np.all(with_pupil[:, 0] < 0.9 * without[:, 0])
    finally:
        dev.close()


def test_a_disk_larger_than_the_grid():
    n, dx = 64, 1.0e-3
    dev = _device(n, "fp64", [_field(n, 3, 40.0)])
    try:
        summary, _ = _check(dev, [_item(dx, 100.0)], 6, what="disk > grid")
        assert summary[0, 0] == n * n
    finally:
        dev.close()


# ---- exact cases ------------------------------------------------------------------------------------------------------
def test_a_constant_field_is_flat_exactly():
    """3 - 4i: a constant whose modulus, 5, and whose sums over the disk are integers, so that |r|^2 and (sum sqrt I)^2 are
    the same number exactly (with an inexact square root the two differ in the last bits)."""
    from paos_amd.wavefront import fit_from_sums

    n, dx = 64, 1.0e-3
    dev = _device(n, "fp64", [np.full((n, n), 3.0 - 4.0j)])
    try:
        for weight in (0, 1):
            dev.wavefront_fit(*_request([_item(dx, 20.0)], 10)[0], weight=weight)
            summary, sums = dev.wavefront_fetch()
            fit = fit_from_sums(summary[0], sums[0], 10, WL)
            assert summary[0, 5] == 0.0 and summary[0, 6] == 0.0 and summary[0, 0] > 1000
            assert np.all(fit["wf_coeff"] == 0.0) and fit["wf_rms"] == 0.0 and fit["wf_pv"] == 0.0 and fit["wf_strehl"] == 1.0
    finally:
        dev.close()


@pytest.mark.parametrize("zero", [0.0, -0.0])
def test_a_pixel_opposite_to_r_reads_what_arctan2_reads(zero):
    n, dx = 64, 1.0e-3
    u = np.full((n, n), complex(1.0, zero))
    u[32, 35] = complex(-1.0, zero)
    dev = _device(n, "fp64", [u])
    try:
        dev.wavefront_fit(*_request([_item(dx, 10.0)], 3)[0])
        summary, _ = dev.wavefront_fetch()
        rp, ip = wnp.turned(-1.0, zero, summary[0, 1], summary[0, 2])  # about the device's own r
        want = np.arctan2(ip, rp)
        assert abs(want) == np.pi
        assert (summary[0, 5] if want < 0 else summary[0, 6]) == want and (summary[0, 6] if want < 0 else summary[0, 5]) == 0.0
    finally:
        dev.close()


def test_the_fallback_when_the_field_sums_to_zero():
    n, dx = 64, 1.0e-3
    u = np.ones((n, n), dtype=np.complex128)
    u[:, 32:] = -1.0
    u[:, 32] = 0.0
    dev = _device(n, "fp64", [u, np.ones((n, n))])
    try:
        summary, _ = _check(dev, [_item(dx, 20.0)] * 2, 3, floors=0.5, what="fallback")
        assert summary[0, 1] == 0.0 and summary[0, 2] == 0.0 and summary[0, 7] == 1.0 and summary[1, 7] == 0.0
        assert summary[0, 5] == 0.0 and summary[0, 6] == np.pi
    finally:
        dev.close()


# ---- bit for bit ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, precision, scale", [(64, "fp64", 24.0), (256, "fp32", 100.0)])
def test_repeats_batch_size_place_and_neighbours_change_no_bit(n, precision, scale):
    dx = 1.0e-3
    fields = [_field(n, s, scale) for s in range(3)]
    items = [_item(dx, scale + 0.5), _item(dx, 0.7 * scale, offset=33.0, origin="y"), _item(1.5 * dx, 0.6 * scale, offset=-12.5)]
    floors = [0.0, 0.05, 0.2]
    req = _request(items, 15)[0]
    dev = _device(n, precision, fields)
    try:
        dev.wavefront_fit(*req, weight=1, min_intensity=floors)
        first = dev.wavefront_fetch()
        dev.wavefront_fit(*req, weight=1, min_intensity=floors)
        again = dev.wavefront_fetch()
        assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    finally:
        dev.close()
    # every item alone in a batch-1 context
    for i in range(3):
        one = _device(n, precision, [fields[i]])
        try:
            one.wavefront_fit(*_request([items[i]], 15)[0], weight=1, min_intensity=[floors[i]])
            s1, g1 = one.wavefront_fetch()
            assert np.array_equal(s1[0], first[0][i]) and np.array_equal(g1[0], first[1][i]), i
        finally:
            one.close()
    # another place in the batch, beside a neighbour that is switched off
    order = [2, 0, 1]
    dev = _device(n, precision, [fields[k] for k in order])
    try:
        moved = [dict(items[k]) for k in order]
        moved[1]["enable"] = False
        dev.wavefront_fit(*_request(moved, 15)[0], weight=1, min_intensity=[floors[k] for k in order])
        s2, g2 = dev.wavefront_fetch()
        for place, k in enumerate(order):
            if place != 1:
                assert np.array_equal(s2[place], first[0][k]) and np.array_equal(g2[place], first[1][k]), (place, k)
    finally:
        dev.close()


def test_a_deferred_stop_factor_is_applied_first():
    """The fit reads the field every other reader sees: behind paos_stop_defer_last_power the sums are those of the SCALED
    field, the one a download afterwards returns."""
    from paos_amd.passes import PassCompiler

    n, dx = 1024, 1.0e-5
    dev = _device(n, "fp64", [_field(n, s, 90.0) for s in range(2)])
    try:
        before = dev.norm2()
        comp = PassCompiler(2, n)
        comp.ptp([[1.0, 1.0 / (n * dx), 1.0 / (n * dx), np.pi * 1.0e-6 * 2.0e-4, -1.0]] * 2)
        done, ticket = comp.flush(dev, final_intensity=2)
        assert done and ticket is not None
        dev.make_stop(power_known=True, defer=True)
        summary, _ = _check(dev, [_item(dx, 60.2)] * 2, 6, "intensity", what="deferred stop")
        dev.norm2_release(ticket)
        assert np.all(before > 1.0e4) and np.all(summary[:, 4] < 1.0) and np.all(summary[:, 4] > 1.0e-3)
    finally:
        dev.close()


# ---- run_batch ----------------------------------------------------------------------------------------------------------
def test_run_batch_end_to_end():
    """SYN20 with a wfe variant per item at 256^2: the injected coefficients come back at the Zernike surface (the issue's
    bound: 1e-12 of the largest) and equal the host algebra on the restatement of the field the GPU holds there; at the image
    plane the device's sums are held to the long-double reference at the bounds and the record is the host algebra on
    them, bit for bit; both surfaces agree with the model device's run to the project's parity gate (the two fields differ
    by that much)."""
    from paos_amd.chains import syn20_chain, syn20_coefficients, syn20_wavelength
    from paos_amd.run import run_batch
    from paos_amd.wavefront import WavefrontFit, fit_from_sums

    n, wls = 256, [syn20_wavelength(0), syn20_wavelength(300)]
    # (8 nm per term: the chain's own 20 nm draw reaches 3.12 rad at the rim of a 256^2 grid, past the stated +-3.0)
    coeffs = [syn20_coefficients(sigma=8.0e-9), syn20_coefficients(rng_seed=2022, sigma=8.0e-9)]
    chains = [syn20_chain(c) for c in coeffs]
    for chain in chains:
        chain[2]["save"] = True
    requests = [WavefrontFit(36, 0.5, surfaces=(2,)), WavefrontFit(6, [2.0e-3, 2.5e-3], weight="intensity", min_intensity=1e-9, surfaces=(20,))]
    from paos_amd import _lib

    dev = _lib.DeviceFields(n, 2, "fp64")
    try:
        res = run_batch(1.0, wls, n, 4, FIELD, chains, outputs=("wfo",), dev=dev, wavefront=requests)
        # The image plane, intensity weights and a radius per item: the context still holds that surface's field, so the
        # sums of the same request are held to the long-double reference at the bounds, and the record must be the host
        # algebra on exactly those sums (a repeated fit gives the same bits).
        last = [res[i][20] for i in range(2)]
        assert all(np.array_equal(dev.download(i), last[i]["wfo"]) for i in range(2))
        items = [dict(dx=rec["dx"], dy=rec["dy"], radius=r, offset=0.0, origin="x", enable=True) for rec, r in zip(last, (2.0e-3, 2.5e-3))]
        summary, sums = _check(dev, items, 6, "intensity", floors=[1e-9, 1e-9], what="run_batch image plane")
    finally:
        dev.close()
    for i, rec in enumerate(last):
        again = fit_from_sums(summary[i], sums[i], 6, wls[i])
        assert rec["wf_pixels"] > 6 and np.array_equal(rec["wf_coeff"], again["wf_coeff"])
        assert all(rec[key] == again[key] for key in again if key != "wf_coeff")
    model = run_batch(1.0, wls, n, 4, FIELD, chains, outputs=(), dev=wnp.WavefrontModelDevice(n, 2), wavefront=requests)
    m36, n36 = Zernike.j2mn(36, "standard")
    for i, c in enumerate(coeffs):
        rec = res[i][2]
        assert rec["wf_phase_absmax"] <= 3.0 and not rec["wf_fallback"] and not rec["wf_singular"]
        err = np.max(np.abs(rec["wf_coeff"][1:] - c[1:])) / np.max(np.abs(c))
        print(f"XPREC run_batch 256^2 item {i}: injected coefficients recovered to {err:.2e} of the largest")
        assert err <= 1.0e-12
        want = fit_from_sums(*wnp.fit_sums_np(rec["wfo"], m36, n36, True, rec["dx"], rec["dy"], 0.5), 36, wls[i])
        assert rec["wf_pixels"] == want["wf_pixels"]
        assert np.max(np.abs(rec["wf_coeff"] - want["wf_coeff"])) <= 1.0e-12 * np.max(np.abs(c))
        for num in (2, 20):
            got, mod = res[i][num], model[i][num]
            assert got["wf_pixels"] == mod["wf_pixels"]
            assert np.allclose(got["wf_coeff"], mod["wf_coeff"], rtol=0, atol=1e-7 * wls[i])
            assert abs(got["wf_strehl"] - mod["wf_strehl"]) <= 1e-8 and abs(got["wf_rms"] - mod["wf_rms"]) <= 1e-7 * wls[i]
        assert "wf_coeff" not in res[i][1]


# ---- misuse -----------------------------------------------------------------------------------------------------------
def test_misuse_of_the_c_calls():
    from paos_amd import _lib

    n, dx = 64, 1.0e-3
    lib = _lib.load()
    fields = [_field(n, 0, 24.0), _field(n, 1, 24.0)]
    dev = _device(n, "fp64", fields)
    ptr = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(_lib._dbl_p)  # noqa: E731
    (nmax, kdim, table, blocks, poly), _, _ = _request([_item(dx, 24.5), _item(dx, 20.0)], 6)
    table = np.ascontiguousarray(table).reshape(-1)
    summary, sums = np.zeros((2, 10)), np.zeros((2, 28))

    def call(**kw):
        a = dict(nmax=nmax, kdim=kdim, table=table, params=blocks, stride=blocks.shape[1], K=6, poly=poly, mode=0, pupil=0, floors=None)
        a.update(kw)
        keep = [np.ascontiguousarray(a[k], dtype=np.float64) if a[k] is not None else None for k in ("table", "params", "poly", "floors")]
        rc = lib.paos_wavefront_fit(dev._ctx, a["nmax"], a["kdim"], ptr(keep[0]), ptr(keep[1]), a["stride"], a["K"], ptr(keep[2]),
                                    a["mode"], a["pupil"], ptr(keep[3]))
        return rc, lib.paos_last_error(dev._ctx).decode()

    def with_header(col, value):
        b = blocks.copy()
        b[1, col] = value
        return b

    try:
        rc = lib.paos_wavefront_fetch(dev._ctx, ptr(summary), ptr(sums))
        assert rc == 1 and "no wavefront fit" in lib.paos_last_error(dev._ctx).decode()
        assert call()[0] == 0  # the arguments are good: every refusal below is about the one argument that is changed
        dev.wavefront_fit(nmax, kdim, table, blocks, poly)
        good = dev.wavefront_fetch()
        for kw in (dict(table=None), dict(params=None), dict(poly=None)):
            rc, msg = call(**kw)
            assert rc == 1 and "null" in msg, kw
        for kw in (dict(nmax=-1), dict(kdim=1), dict(stride=7)):
            rc, msg = call(**kw)
            assert rc == 1 and "dimensions" in msg, kw
        for bad in (0.0, -1.0, float("nan")):
            rc, msg = call(params=with_header(3, bad))
            assert rc == 1 and "radius" in msg, bad
        for col in (1, 2, 5, 7):
            rc, msg = call(params=with_header(col, float("inf")))
            assert rc == 1 and "non-finite" in msg, col
        outside = poly.copy()
        outside[2, 0] = nmax + 1
        assert call(poly=outside)[0] == 1 and "outside" in call(poly=outside)[1]
        twice = poly.copy()
        twice[3] = twice[2]
        assert call(poly=twice)[0] == 1 and "twice" in call(poly=twice)[1]
        for mode in (-1, 2):
            assert call(mode=mode)[0] == 1 and "weight mode" in call(mode=mode)[1]
        for bad in (-1.0e-30, float("nan"), float("inf")):
            rc, msg = call(floors=[0.0, bad])
            assert rc == 1 and "min_intensity" in msg, bad
        assert call(pupil=1)[0] == 1 and "no pupil" in call(pupil=1)[1]
        for k in (0, 64):
            assert call(K=k)[0] == 3  # PAOS_EUNSUPPORTED
        assert lib.paos_wavefront_fetch(dev._ctx, None, None) == 1
        assert lib.paos_wavefront_fit(None, nmax, kdim, ptr(table), ptr(blocks), 8, 6, ptr(poly), 0, 0, None) == 1
        assert lib.paos_wavefront_fetch(None, ptr(summary), ptr(sums)) == 1
        # nothing was touched, and the context is usable: the earlier results are still there, a new fit gives them again
        after = dev.wavefront_fetch()
        assert np.array_equal(after[0], good[0]) and np.array_equal(after[1], good[1])
        assert lib.paos_wavefront_fetch(dev._ctx, ptr(summary), None) == 0 and np.array_equal(summary, good[0])
        assert lib.paos_wavefront_fetch(dev._ctx, None, ptr(sums)) == 0 and np.array_equal(sums, good[1])
        again, _ = _check(dev, [_item(dx, 24.5), _item(dx, 20.0)], 6, what="after the refusals")
        assert np.array_equal(again, good[0])
        # a larger request grows the scratch
        _check(dev, [_item(dx, 24.5), _item(dx, 20.0)], 28, what="grown scratch")
    finally:
        dev.close()


def test_zz_the_largest_fraction_of_each_bound():
    """Last in the module: what the tests above reached of every bound (the record is profiles/r22_wavefront_xprec.md)."""
    assert OBSERVED, "run the whole module"
    for name, frac in sorted(OBSERVED.items()):
        print(f"XPREC wavefront {name}: largest observed {frac:.3f} of its bound")
        assert frac <= 1.0
