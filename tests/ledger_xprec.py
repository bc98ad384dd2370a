"""Extended-precision references, yardsticks, bounds and inputs of the layer that decides how much light there is and
what the caller gets back: the power ledger (csrc/pointwise.h: norm2_partial_kernel + norm2_final_kernel with their row,
column and same_as windows, intensity_kernel, intensity_power_kernel, stop_scale_kernel; csrc/paos_hip.hip: the deferred
stop), the tabulated phase screens (phase_map_kernel, phase_map_items_kernel), the PSD screen built on the device
(psd_load_kernel, psd_filter_kernel, psd_finish_kernel around four generic passes) and the exports (export_kernel,
import_kernel, psf_unblock_kernel, zero_outside_box_kernel).  It imports no device code;
tests/test_ledger_xprec_reference.py keeps it honest without a device, tests/test_gpu_ledger_xprec.py holds the kernels
to it.

What is formed in fp64, one rounding per operation as the kernels promise, so that every decision is shared bit for bit:
the intensity re^2 + im^2 (pointwise_xprec.intensity), the phase-map argument fl(fl(2 pi w) / wl), the radial frequency
rho of the PSD filter and so the band membership.  What runs in long double: every summation, the stop's 1 / sqrt(P), cos
and sin of the argument and the complex product, the PSD gain, both 2-D transforms and the finish.

Test infrastructure only.
"""
import numpy as np

import pointwise_xprec as px
import xprec_np as xp
from xprec_np import LD, TWO_PI, U32, U64, require_long_double  # noqa: F401

LDR = np.longdouble
DT = {"fp64": np.complex128, "fp32": np.complex64}
TINY = float(np.finfo(np.float64).tiny)


def block_rows(n, precision):
    """Rows of a layout block: 4, or 8 for complex64 fields from 2048^2 up (csrc/host.h: block_rows)."""
    return 8 if (precision == "fp32" and n >= 2048) else 4


def stored(f, precision):
    """What the context holds after upload (import_kernel): complex64 contexts round each component once."""
    with np.errstate(over="ignore"):
        return np.asarray(f, dtype=np.complex128).astype(DT[precision]).astype(np.complex128)


def field(n, seed):
    rng = np.random.default_rng(900000 + 131 * n + seed)
    return rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))


# ---- power sums ---------------------------------------------------------------------------------------------------------
def power(u):
    """Long-double sum of the fp64 intensities: the kernels promise those roundings (__dmul_rn / __dadd_rn); only the
    summation is extended."""
    return np.sum(px.intensity(u).astype(LDR))


def power_np(u):
    """The fp64 yardstick: np.sum (pairwise) of the same intensities."""
    return np.sum(px.intensity(u))


def power_bound_rel(n):
    """2 log2(n^2) u: bound_metric's multiple for a sum of n^2 non-negative terms (psf_metrics_kernel's power meets it with
    the same reduction shape, observed there at 0.43 log2 u)."""
    return px.C_METRIC * np.log2(max(2, n * n)) * U64


def power_bound(n, total=1.0):
    """The same as an absolute bound of a sum ``total`` (= px.bound_metric(n * n, [total, ...])[0])."""
    return float(px.bound_metric(n * n, [float(total), 0.0, 0.0, 0.0])[0])


def window_round(lo, hi, br, n):
    """[lo, hi) rounded outward to whole multiples of ``br``, clipped to n: what check_rows + the kernels' row windows and
    rounded_cols make of a window."""
    lo, hi = int(lo), int(hi)
    return (lo // br) * br, min(n, ((hi + br - 1) // br) * br)


def _box(shape, rows, cols, br):
    n = shape[0]
    r0, r1 = window_round(rows[0], rows[1], br, n)
    c0, c1 = (0, n) if cols is None else window_round(cols[0], cols[1], br, n)
    inside = np.zeros(shape, dtype=bool)
    inside[r0:r1, c0:c1] = True
    return inside


def nominal_box(shape, rows, cols):
    inside = np.zeros(shape, dtype=bool)
    c0, c1 = (0, shape[1]) if cols is None else (int(cols[0]), int(cols[1]))
    inside[int(rows[0]):int(rows[1]), c0:c1] = True
    return inside


def window_field(u, rows, cols, br):
    """The zero-filled field the windowed sums promise to equal the full sum of: ``u`` inside the nominal window, real
    zeros between it and the outward-rounded window and everywhere else."""
    return np.where(nominal_box(u.shape, rows, cols), u, 0.0 + 0.0j)


def poison(u, rows, cols, br, precision="fp64"):
    """``u`` inside the nominal window, real zeros between the nominal and the outward-rounded window, and NaN and +-huge
    (1e300; 3e38 for complex64 contexts) everywhere outside the rounded window: data that a sum must not read."""
    big = 1.0e300 if precision == "fp64" else 3.0e38
    out = window_field(u, rows, cols, br)
    outside = ~_box(u.shape, rows, cols, br)
    r, c = np.indices(u.shape)
    pattern = np.where((r + c) % 3 == 0, complex(np.nan, np.nan), np.where((r + c) % 3 == 1, complex(big, -big), complex(-big, big)))
    return np.where(outside, pattern, out)


# ---- stops ------------------------------------------------------------------------------------------------------------------
def stop_reference(u):
    """(u / sqrt(P) in long double, P): make_stop of one item, P the long-double power of the stored field."""
    p = power(u)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.asarray(u).astype(LD) / np.sqrt(p), p


def stop_np(u):
    """The fp64 yardstick with NumPy's own operations: u * (1 / sqrt(sum))."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.asarray(u, dtype=np.complex128) * (1.0 / np.sqrt(power_np(u)))


def stop_bound(n, precision):
    """Per element, as a fraction of |u| / sqrt(P): half the power's relative bound (the square root halves it) plus four
    roundings -- sqrt, reciprocal and the two products -- plus one rounding to complex64 for fp32 stores."""
    return 0.5 * power_bound_rel(n) + 4 * U64 + (U32 if precision == "fp32" else 0.0)


def relative_element_error(got, ref):
    """max |got - ref| / |ref| over the elements with ref != 0 (the others must be exact zeros: inf otherwise)."""
    g, r = np.asarray(got).astype(LD), np.asarray(ref).astype(LD)
    d, a = np.abs(g - r).astype(LDR), np.abs(r).astype(LDR)
    if np.any(d[a == 0] != 0):
        return float("inf")
    return float(np.max(d[a > 0] / a[a > 0])) if np.any(a > 0) else 0.0


# ---- tabulated phase screens ------------------------------------------------------------------------------------------------
def phase_map_argument(w, wl):
    """fl(fl(2 pi w) / wl) in fp64: the kernels' (and NumPy's) argument."""
    return (TWO_PI * np.asarray(w, dtype=np.float64)) / np.float64(wl)


def phase_map_reference(u, w, wl):
    a = phase_map_argument(w, wl).astype(LDR)
    return np.asarray(u).astype(LD) * (np.cos(a) + 1j * np.sin(a)).astype(LD)


def phase_map_np(u, w, wl):
    return np.exp(1j * phase_map_argument(w, wl)) * np.asarray(u, dtype=np.complex128)


def phase_map_bound(n, precision):
    """fp64: xp.bound(n, 0, 1) -- 4 u per-line L2, 8 u per element of the line's max.  fp32 contexts: the factor is fp64 and
    the product is rounded to complex64 once: per element |err| <= (U32 + 8 U64) |u| (returned as (None, that))."""
    if precision == "fp64":
        return xp.bound(n, 0, 1, "fp64")
    return None, U32 + 8 * U64


PHASE_WL = 1.0e-6
PHASE_WLS = (1.3e-6, 0.7e-6)


def phase_map_args():
    """The arguments the maps are built around: 0, +-1e-300, multiples of pi/2 and their fp64 neighbours, and about 1, 1e3,
    1e6, 1e12 rad with both signs."""
    a = [0.0, 1e-300, -1e-300]
    for k in (1, 2, 3, 4, 5, 7, 100, 12345):
        m = np.float64(k) * (np.pi / 2)
        for s in (1.0, -1.0):
            a += [s * m, s * np.nextafter(m, np.inf), s * np.nextafter(m, -np.inf)]
    for t in (1.0, 1e3, 1e6, 1e12):
        a += [t, -t, 0.999 * t, -1.001 * t, t / 3.0, -t / 7.0]
    return np.array(a, dtype=np.float64)


def phase_map_inputs(n, wl=PHASE_WL, seed=0):
    """An n x n map in metres whose fp64 argument at ``wl`` covers phase_map_args (each within an ulp or two: w is the
    fp64 value nearest arg wl / 2 pi and its two neighbours, so multiples of pi/2 are straddled) in the upper half of the
    grid -- laid out flat, so every layout block position meets them -- and seeded arguments up to 1e3 rad below."""
    rng = np.random.default_rng(77000 + n + seed)
    w = rng.uniform(-1e3, 1e3, (n, n)) * wl / TWO_PI
    a = phase_map_args()
    base = a * wl / TWO_PI
    specials = np.concatenate([base, np.nextafter(base, np.inf), np.nextafter(base, -np.inf)])
    flat = w.reshape(-1)
    reps = (n * n // 2) // specials.size
    flat[:reps * specials.size] = np.tile(specials, reps)
    return w


def phase_map_errors(got, ref, u, precision):
    """(L2 per line, element of the line's max) for fp64; (None, max |err| / |u| per element) for fp32 contexts."""
    if precision == "fp64":
        return xp.line_errors(got, ref, 0)
    d = np.abs(np.asarray(got).astype(LD) - ref).astype(LDR)
    a = np.abs(np.asarray(u).astype(LD)).astype(LDR)
    return None, float(np.max(d[a > 0] / a[a > 0]))


# ---- the PSD screen -------------------------------------------------------------------------------------------------------
def psd_rho(n, fx, fy):
    """rho in fp64 as psd_filter_kernel forms it: k fx, k fy (k the signed FFT index), squares, sum, sqrt, one rounding
    each; rho == 0 -> 1e-100."""
    k = np.arange(n)
    k = np.where(k < n // 2, k, k - n).astype(np.float64)
    gx, gy = k * np.float64(fx), k * np.float64(fy)
    rho = np.sqrt((gx * gx)[None, :] + (gy * gy)[:, None])
    rho[rho == 0.0] = 1e-100
    return rho


def psd_reference(noise, rough, params12, strict_min=False, strict_max=False):
    """(map, kept-bin mask) of paos_psd_screen: rho and the band membership in fp64 as the kernel decides them (a bin with
    rho == fmin or rho == fmax is KEPT: the reference zeroes rho < fmin or rho > fmax); the gain
    sqrt(A / (B + (rho / fknee)^C) / (2 pi rho) * cell) * gain, fft2, ifft2 and (Re + SR rough) 2 unit in long double.
    ``strict_min`` / ``strict_max``: the wrong comparison (<=, >=), for tests that must see the difference."""
    fx, fy, A, B, C, fknee, fmin, fmax, cell, gain, SR, unit = (float(v) for v in params12)
    noise = np.asarray(noise, dtype=np.float64)
    n = noise.shape[0]
    rho = psd_rho(n, fx, fy)
    below = rho <= fmin if strict_min else rho < fmin
    above = rho >= fmax if strict_max else rho > fmax
    keep = ~(below | above)
    r = rho.astype(LDR)
    with np.errstate(over="ignore", divide="ignore"):
        d = LDR(A) / (LDR(B) + (r / LDR(fknee)) ** LDR(C)) / (LDR(TWO_PI) * r) * LDR(cell)
        g = np.where(keep, np.sqrt(d) * LDR(gain), LDR(0))
    spec = np.fft.fft2(noise.astype(LD)) * g
    screen = np.fft.ifft2(spec).real.astype(LDR)
    if rough is not None and SR != 0.0:
        screen = screen + LDR(SR) * np.asarray(rough, dtype=np.float64).astype(LDR)
    return screen * LDR(2) * LDR(unit), keep


def psd_np(noise, rough, shape, dx, dy, **kw):
    """The fp64 yardstick: the host path (paos_amd/phase_maps.py: psd_map_from_draws)."""
    from paos_amd import phase_maps

    return np.ma.filled(phase_maps.psd_map_from_draws(noise, rough, shape, dx, dy, **kw), 0.0)


def psd_bound(n):
    """(L2 over the map relative to its L2, element relative to max |map|): xp.bound(n, 4, 2, "fp64") -- an element sees four
    line transforms; the 8 u are the filter gain's allowance."""
    return xp.bound(n, 4, 2, "fp64")


def psd_errors(got, ref):
    g, r = np.asarray(got).astype(LDR), np.asarray(ref).astype(LDR)
    d = g - r
    return float(np.sqrt(np.sum(d * d) / np.sum(r * r))), float(np.max(np.abs(d)) / np.max(np.abs(r)))


def psd_grid(n, anamorphic=False):
    """(dx, dy): a 1 m pupil at zoom 4 (the golden vectors' grid), stretched to (1.25, 0.8) x that when anamorphic --
    "golden": the other way round, (0.8, 1.25), the grid of the golden vectors' anamorphic beam."""
    if anamorphic == "golden":
        return 0.8 * 4.0 / n, 1.25 * 4.0 / n
    return (1.25 * 4.0 / n, 0.8 * 4.0 / n) if anamorphic else (4.0 / n, 4.0 / n)


def _edge_band(n):
    fx = 1.0 / (n * (4.0 / n))  # 0.25, exact: k fx and np.fft.fftfreq agree bit for bit, and rho(5, 12) = 13 fx = 3.25 exactly
    rho = psd_rho(n, fx, fx)
    return float(np.float64(3.0) * np.float64(fx)), float(rho[5, 12])


# name -> (anamorphic grid?, keyword arguments of the PSD call; fmin / fmax may be callables of n)
PSD_CASES = {
    "powerlaw": (False, dict(A=7.0, B=0.0, C=1.5, fknee=1.0, fmin=None, fmax=None, SR=0.0, units="nm")),
    "knee_sr_anam": (True, dict(A=12.0, B=1.0, C=2.2, fknee=3.0, fmin=0.5, fmax=6.0, SR=2.0, units="nm")),
    "c_zero": (False, dict(A=5.0, B=0.5, C=0.0, fknee=2.0, fmin=None, fmax=None, SR=0.0, units="nm")),
    "edge_band": (False, dict(A=7.0, B=0.0, C=1.5, fknee=1.0, fmin=lambda n: _edge_band(n)[0],
                              fmax=lambda n: _edge_band(n)[1], SR=0.0, units="nm")),
}
# the golden vectors (tests/golden/r2_phase_maps.npz, seed 1234, n = 64) of the first two parameter sets on both grids
PSD_GOLDEN = {"psd_powerlaw_wfe": ("powerlaw", False), "psd_powerlaw_anam_wfe": ("powerlaw", "golden"),
              "psd_knee_sr_wfe": ("knee_sr_anam", False), "psd_knee_sr_anam_wfe": ("knee_sr_anam", "golden")}


def psd_case(name, n, anamorphic=None, seed=1234):
    """(noise, rough or None, (dx, dy), kwargs, params12) of a case at n: the draws are NumPy's legacy generator's, in the
    reference's order, from ``seed`` (the global generator's state is put back)."""
    from paos_amd import phase_maps

    anam, kw = PSD_CASES[name]
    anam = anam if anamorphic is None else anamorphic
    kw = {k: (v(n) if callable(v) else v) for k, v in kw.items()}
    dx, dy = psd_grid(n, anam)
    state = np.random.get_state()
    try:
        np.random.seed(seed)
        noise, rough = phase_maps.psd_draws((n, n))
    finally:
        np.random.set_state(state)
    rough = rough if kw["SR"] != 0.0 else None
    return noise, rough, (dx, dy), kw, phase_maps.psd_device_params((n, n), dx, dy, **kw)


def edge_band_counts(n=64):
    """(kept bins, bins on the lower edge, bins on the upper edge) of the edge-band case by integer arithmetic: bin (i, j)
    has rho = fx sqrt(i^2 + j^2); the band is 3 fx .. 13 fx."""
    k = np.arange(-(n // 2), n // 2)
    s = (k * k)[None, :] + (k * k)[:, None]
    return int(np.sum((s >= 9) & (s <= 169))), int(np.sum(s == 9)), int(np.sum(s == 169))


# ---- exports ---------------------------------------------------------------------------------------------------------------
def export_edge_values(precision):
    """The edge block: (name, value) pairs.  The first eight are the signed-zero and negative-real-axis pixels whose phase
    must match np.arctan2 bit for bit, sign of zero included."""
    pz, nz = 0.0, -0.0
    v = [("zero++", (pz, pz)), ("zero+-", (pz, nz)), ("zero-+", (nz, pz)), ("zero--", (nz, nz)),
         ("neg axis +0", (-1.0, pz)), ("neg axis -0", (-1.0, nz)), ("neg axis 2.5 +0", (-2.5, pz)), ("neg axis 2.5 -0", (-2.5, nz)),
         ("imag +", (pz, 1.0)), ("imag -", (pz, -1.0)), ("imag -0", (nz, 2.0)), ("imag -0 -", (nz, -2.0)),
         ("tiny imag", (1.0, 1e-17)), ("tiny real", (-1e-17, 1.0)),
         ("equal", (3.0, 3.0)), ("equal -+", (-3.0, 3.0)), ("equal --", (-0.7, -0.7))]
    if precision == "fp64":
        v += [("denormal", (5e-324, pz)), ("denormal pair", (5e-324, -5e-324)), ("denormal 1e-310", (1e-310, -1e-310)),
              ("denormal imag", (nz, 1e-310)), ("denormal mixed", (1e-310, 1.0)),
              ("huge 1e200", (1e200, 1e200)), ("huge 1e200 -", (-1e200, 3e199)), ("huge 1.2e308", (1.2e308, 1.2e308)),
              ("huge mixed", (1.2e308, -1.0)), ("overflow", (1.7e308, -1.0e308))]
    else:
        v += [("denormal", (1e-40, pz)), ("denormal pair", (1e-40, -1e-40)), ("denormal imag", (nz, 1e-40)),
              ("denormal mixed", (1e-40, 1.0)),
              ("huge 1e30", (1e30, 1e30)), ("huge 1e30 -", (-1e30, 3e29)), ("huge 3e38", (3e38, 3e38)), ("huge mixed", (3e38, -1.0))]
    return v


EXPORT_EXACT = 8  # the first eight edge values: phase bit for bit


def export_inputs(n, precision):
    """(field, pixels): a seeded random field with the edge block written once at every position (row mod 8, column mod 2)
    of the 4 x 2 and 8 x 2 layout blocks; pixels[k] = (rows[16], cols[16]) of edge value k."""
    u = field(n, 41).copy()
    vals = export_edge_values(precision)
    assert len(vals) <= 32 and n >= 64
    pixels = []
    for k, (_, (re, im)) in enumerate(vals):
        rows, cols = [], []
        for pos in range(16):
            r, c = 8 * (k % 4 + 1) + pos // 2, 2 * (3 + k // 4) + pos % 2
            u[r, c] = complex(re, im)
            rows.append(r)
            cols.append(c)
        pixels.append((np.array(rows), np.array(cols)))
    return u, pixels


def amplitude_reference(u):
    with np.errstate(over="ignore"):
        return np.hypot(np.asarray(u).real.astype(LDR), np.asarray(u).imag.astype(LDR))


def phase_reference(u):
    return np.arctan2(np.asarray(u).imag.astype(LDR), np.asarray(u).real.astype(LDR))


def amplitude_error(got, ref):
    """Largest |got - ref| / max(ref, smallest normal double) over the elements whose reference is finite in fp64 -- a
    denormal result is held to the format's absolute spacing there, 2 u of the smallest normal -- and whether the others
    (the reference overflows fp64) are inf exactly where it does."""
    got = np.asarray(got, dtype=np.float64)
    with np.errstate(over="ignore"):
        finite = np.isfinite(ref.astype(np.float64))
    same_inf = bool(np.array_equal(np.isinf(got), ~finite))
    d = np.abs(got[finite].astype(LDR) - ref[finite]) / np.maximum(ref[finite], LDR(TINY))
    return float(np.max(d)), same_inf


def phase_error(got, ref):
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64).astype(LDR) - ref)))


def export_bounds(u):
    """(amplitude bound, phase bound, yardstick amplitude error, yardstick phase error) taken from the reference at run
    time: 4 x the largest error of np.hypot (relative) / np.arctan2 (absolute) against long double on the same inputs, floored at
    2 u and 2 u pi.  No bound of the device's hypot / atan2 exists in the project; what the device reaches never enters."""
    u = np.asarray(u, dtype=np.complex128)
    with np.errstate(over="ignore"):
        ya, _ = amplitude_error(np.hypot(u.real, u.imag), amplitude_reference(u))
    yp = phase_error(np.arctan2(u.imag, u.real), phase_reference(u))
    return max(4.0 * ya, 2 * U64), max(4.0 * yp, 2 * U64 * np.pi), ya, yp
