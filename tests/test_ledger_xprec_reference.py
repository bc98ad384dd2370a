"""tests/ledger_xprec.py kept honest without a device: the long-double restatements against the host path, the golden
vectors of the reference project and brute force; every fp64 yardstick inside half of the bound its kernel is held to
(tests/test_gpu_ledger_xprec.py) -- no bound is tighter than correct fp64 arithmetic achieves."""
import numpy as np
import pytest

import ledger_xprec as lx
import xprec_np as xp
from conftest import load_golden


def setup_module(module):
    xp.require_long_double()


# ---- the PSD screen -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 128])
@pytest.mark.parametrize("name", list(lx.PSD_CASES))
def test_psd_reference_against_the_host_path(name, n):
    noise, rough, (dx, dy), kw, params = lx.psd_case(name, n)
    ref, keep = lx.psd_reference(noise, rough, params)
    yard = lx.psd_np(noise, rough, (n, n), dx, dy, **kw)
    b_l2, b_el = lx.psd_bound(n)
    e_l2, e_el = lx.psd_errors(yard, ref)
    print(f"\nXPREC psd {name} {n}^2: host path L2 {e_l2 / xp.U64:.2f} u element {e_el / xp.U64:.2f} u; bound {b_l2 / xp.U64:.0f} u / "
          f"{b_el / xp.U64:.0f} u; {int(keep.sum())} bins kept")
    assert 0 < keep.sum() < n * n and np.max(np.abs(ref)) > 0
    assert e_l2 <= 0.5 * b_l2 and e_el <= 0.5 * b_el, (name, n, e_l2, e_el, b_l2, b_el)


@pytest.mark.parametrize("key", list(lx.PSD_GOLDEN))
def test_psd_reference_against_the_golden_vectors(key):
    """The reference project's own output (seed 1234, a 64^2 grid): inside the bound."""
    name, anam = lx.PSD_GOLDEN[key]
    g = load_golden("r2_phase_maps.npz")
    noise, rough, _, _, params = lx.psd_case(name, 64, anamorphic=anam)
    ref, _ = lx.psd_reference(noise, rough, params)
    b_l2, b_el = lx.psd_bound(64)
    e_l2, e_el = lx.psd_errors(g[key], ref)
    assert e_l2 <= b_l2 and e_el <= b_el, (key, e_l2, e_el, b_l2, b_el)


@pytest.mark.parametrize("n", [64, 128])
def test_psd_edge_band_keeps_the_bins_on_both_edges(n):
    noise, rough, _, kw, params = lx.psd_case("edge_band", n)
    fx, fmin, fmax = params[0], params[6], params[7]
    assert fx == 0.25 and fmin == 0.75 and fmax == 3.25 and kw["fmin"] == fmin and kw["fmax"] == fmax
    ref, keep = lx.psd_reference(noise, rough, params)
    rho = lx.psd_rho(n, params[0], params[1])
    kept, on_min, on_max = lx.edge_band_counts(n)
    assert (on_min, on_max) == (4, 12)
    assert int(keep.sum()) == kept
    assert int((rho == fmin).sum()) == on_min and keep[rho == fmin].all()
    assert int((rho == fmax).sum()) == on_max and keep[rho == fmax].all() and keep[5, 12] and keep[0, 13 - n] and keep[3, 0]
    b_l2, b_el = lx.psd_bound(n)
    for flip in (dict(strict_min=True), dict(strict_max=True)):
        other, keep2 = lx.psd_reference(noise, rough, params, **flip)
        assert int(keep2.sum()) == kept - (on_min if "strict_min" in flip else on_max)
        d_l2, d_el = lx.psd_errors(other, ref)
        assert d_l2 > 100 * b_l2 and d_el > 100 * b_el, (flip, d_l2, d_el)


# ---- power, windows, stops ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("n", [64, 128, 1024])
def test_power_and_stop_yardsticks_inside_half_of_their_bounds(n, precision):
    for scale in (1.0, 1e-150, 1e150):
        u = lx.stored(lx.field(n, 3), precision) * scale
        p = lx.power(u)
        assert abs(float((lx.power_np(u) - p) / p)) <= 0.5 * lx.power_bound_rel(n)
        assert lx.power_bound(n, float(p)) == pytest.approx(lx.power_bound_rel(n) * float(p), rel=1e-15)
    u = lx.stored(lx.field(n, 4), precision)
    ref, p = lx.stop_reference(u)
    yard = lx.stop_np(u)
    e = lx.relative_element_error(yard, ref)
    assert e <= 0.5 * lx.stop_bound(n, "fp64"), (e, lx.stop_bound(n, "fp64"))
    assert abs(float(lx.power(yard)) - 1.0) <= lx.power_bound_rel(n) + 2 * lx.stop_bound(n, "fp64")
    with np.errstate(all="ignore"):
        assert np.isnan(lx.stop_reference(np.zeros((8, 8), dtype=complex))[0]).all()


@pytest.mark.parametrize("br", [4, 8])
def test_window_round_against_brute_force(br):
    n = 64
    for lo in range(n + 1):
        for hi in range(lo, n + 1):
            blocks = [b for b in range(n // br) if any(lo <= r < hi for r in range(b * br, b * br + br))]
            got = lx.window_round(lo, hi, br, n)
            if blocks:
                assert got == (blocks[0] * br, blocks[-1] * br + br), (lo, hi)
            else:  # an empty window: whatever it rounds to holds no row of the nominal window
                assert lo == hi and got[0] <= lo <= got[1] and got[1] - got[0] in (0, br)


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_poison_and_window_field(precision):
    n, br = 64, 4
    u = lx.stored(lx.field(n, 5), precision)
    rows, cols = (5, n - 3), (3, n - 5)
    p = lx.stored(lx.poison(u, rows, cols, br, precision), precision)
    w = lx.window_field(u, rows, cols, br)
    inside = np.zeros((n, n), dtype=bool)
    inside[4:n, 0:n - 4] = True
    assert np.array_equal(p[inside], w[inside]) and not np.isfinite(lx.power_np(p[~inside]))
    assert np.isnan(p[~inside]).any() and (np.abs(p[~inside].real) >= 3e38).any() and not np.isinf(p.real).any()
    assert np.array_equal(w[5:n - 3, 3:n - 5], u[5:n - 3, 3:n - 5]) and int((w != 0).sum()) == (n - 8) * (n - 8)
    assert (w[4] == 0).all() and (w[:, n - 5] == 0).all() and w[5, 3] == u[5, 3]
    assert (lx.window_field(u, (8, 8), None, br) == 0).all()


# ---- phase screens ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 128])
def test_phase_map_yardstick_and_argument_coverage(n):
    w = lx.phase_map_inputs(n)
    arg = lx.phase_map_argument(w, lx.PHASE_WL)
    assert (arg == 0).any() and np.abs(arg).max() > 0.99e12 and np.abs(arg).max() < 1.01e12
    assert ((np.abs(arg) > 0) & (np.abs(arg) < 1e-299)).any()
    for t in (1.0, 1e3, 1e6, 1e12):
        assert ((arg > 0.5 * t) & (arg < 1.5 * t)).any() and ((arg < -0.5 * t) & (arg > -1.5 * t)).any()
    for k in (1, 2, 3, 4, 5, 7):  # both sides of the multiple of pi / 2, within a few ulp
        m = np.float64(k) * (np.pi / 2)
        near = arg[np.abs(arg - m) <= 4 * np.spacing(m)]
        assert (near < m).any() and (near > m).any(), k
    u = lx.field(n, 6)
    ref = lx.phase_map_reference(u, w, lx.PHASE_WL)
    b_l2, b_el = lx.phase_map_bound(n, "fp64")
    e_l2, e_el = xp.line_errors(lx.phase_map_np(u, w, lx.PHASE_WL), ref, 0)
    assert e_l2 <= 0.5 * b_l2 and e_el <= 0.5 * b_el, (e_l2, e_el)
    u32 = lx.stored(u, "fp32")
    yard32 = lx.stored(lx.phase_map_np(u32, w, lx.PHASE_WL), "fp32")
    _, e = lx.phase_map_errors(yard32, lx.phase_map_reference(u32, w, lx.PHASE_WL), u32, "fp32")
    assert e <= lx.phase_map_bound(n, "fp32")[1], e
    # the arguments the host must refuse: finite map values whose fp64 argument is not
    with np.errstate(over="ignore"):
        assert np.isinf(lx.phase_map_argument(1e308, 1e-6)) and np.isinf(lx.phase_map_argument(1.0, 1e-310))


# ---- exports ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_export_inputs_and_run_time_bounds(precision):
    n = 64
    u, pixels = lx.export_inputs(n, precision)
    s = lx.stored(u, precision)
    vals = lx.export_edge_values(precision)
    seen = set()
    for (name, (re, im)), (rows, cols) in zip(vals, pixels):
        got = s[rows, cols]
        assert set(zip(rows % 8, cols % 2)) == {(a, b) for a in range(8) for b in range(2)}, name
        assert not seen & set(zip(rows, cols))
        seen |= set(zip(rows, cols))
        want = np.complex128(complex(re, im)) if precision == "fp64" else np.complex128(np.complex64(complex(re, im)))
        assert np.array_equal(got.real, np.full(16, want.real)) and np.array_equal(np.signbit(got.real), np.full(16, np.signbit(want.real)))
        assert np.array_equal(got.imag, np.full(16, want.imag)) and np.array_equal(np.signbit(got.imag), np.full(16, np.signbit(want.imag)))
        if "denormal" in name or "huge" in name:  # still there after the cast: neither flushed to zero nor overflowed
            assert np.isfinite(got.real).all() and np.isfinite(got.imag).all() and (np.abs(got.real) + np.abs(got.imag) > 0).all(), name
    b_amp, b_ph, y_amp, y_ph = lx.export_bounds(s)
    assert np.isfinite([b_amp, b_ph]).all() and 2 * xp.U64 <= b_amp <= 16 * xp.U64 and 2 * xp.U64 * np.pi <= b_ph <= 16 * xp.U64 * np.pi, \
        (b_amp, b_ph, y_amp, y_ph)
    amp = lx.amplitude_reference(s)
    assert np.isinf(amp.astype(np.float64)).sum() == (16 if precision == "fp64" else 0)
    k = [name for name, _ in vals].index("huge 1e200" if precision == "fp64" else "huge 1e30")
    assert np.isfinite(amp[pixels[k]].astype(np.float64)).all()
    ph = np.arctan2(s.imag, s.real)
    rows, cols = pixels[1]
    assert (ph[rows, cols] == 0).all() and np.signbit(ph[rows, cols]).all()   # atan2(-0, +0) = -0
    rows, cols = pixels[5]
    assert (ph[rows, cols] == -np.pi).all()                                   # atan2(-0, -1) = -pi
