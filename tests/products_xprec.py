"""Extended-precision references and bounds of the four products read out behind the pass kernels -- zoomed windows
(csrc/zoom_pass.h), transfer functions (csrc/otf_pass.h), through-focus planes (csrc/focus_pass.h) -- and the geometry
of the detector's chunk loop (csrc/detector.hip).  It extends tests/xprec_np.py (the long-double restatement of a pass
program, ``line_errors``, ``bound``, ``check``); tests/test_products_xprec_reference.py keeps what is here honest without
a device, tests/test_gpu_products_xprec.py holds the kernels to it.

Zoom.  ``zoom_reference`` is ``Wy u Wx^T`` with the weights of the definition (``zoom_np.phase_table``) kept in long double;
``zoom_yardstick`` is the same two contractions in fp64 with the double-rounded weights, a plain loop over k (no BLAS, no
pairwise summation): what a k-ordered chain of n multiply-adds achieves.  The project's error model has no per-element
figure for such a chain, so the gate is 4 x the yardstick's own error against the same reference on the same rows (the
kernel rounds once per term where the yardstick rounds twice, and may associate the four k of one matrix instruction
differently: another draw from the same distribution), plus the rigorous componentwise bound ``zoom_rigorous_bound``.

OTF.  ``otf_reference`` / ``otf_reference_lines`` are ``fft2(ifftshift(P))`` over its zero-frequency value in long double,
whole or on sampled frequency columns; errors are measured per line with the zero-frequency element left out, each element
against the larger of the two lines through it and the L2 norm along frequency rows (``otf_line_errors``, which says why),
not relative to DC = 1.

Focus.  ``focus_passes`` is the program csrc/focus_pass.h names, for ``xprec_np.run_item``; with sy = 0 (sx = 0) the plane
is a row-wise (column-wise) 1-D operation in exact arithmetic and ``focus_passes_1d`` restates it on sampled lines.

Test infrastructure only.
"""
import numpy as np

import xprec_np as xp
import zoom_np
from paos_amd import _lib

LDR = np.longdouble
LD = xp.LD
DT = {"fp64": np.complex128, "fp32": np.complex64}
SIZES = (64, 128, 256, 512, 1024, 2048, 4096)


# ---- zoomed windows ---------------------------------------------------------------------------------------------------
# (n, batch, m, s): with paos_zoom_tiles these reach stage Y at PT 8, 8 partial, 4 partial, 4 (fp32: 8-row blocks), 4, 4,
# 2 partial, 4 partial, 4 and stage X at PT 1, 1, 1, 1, 4, 2, 2 partial, 8 partial, 8 (tests/test_zoom_host.py asserts it)
ZOOM_CASES = [(1024, 16, 128, 4), (1024, 11, 192, 4), (1024, 7, 160, 3), (2048, 4, 128, 4), (256, 16, 256, 2),
              (512, 8, 320, 3), (256, 10, 240, 2), (256, 9, 496, 4), (256, 8, 512, 4)]
ZOOM_SAMPLED_FROM = 1024  # grids from here on: the long-double reference runs on sampled window rows
ZOOM_FACTOR = 4.0


def zoom_fields(n, batch, seed=0):
    """Seeded complex normals, one field per item."""
    rng = np.random.default_rng(424200 + 17 * n + batch + seed)
    return [rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)) for _ in range(batch)]


def zoom_centres(n, batch, m, s):
    """(batch, 2) centres (x, y): non-integer and different per item; item 0's window wraps in both axes, item 1 sits on
    an integer centre, the others lie wherever a window fits without wrapping (or anywhere, when none does)."""
    rng = np.random.default_rng(7000 + n + 31 * batch + m)
    half = 0.5 * m / s + 1.0
    lo, hi = (half, n - half) if n - 2.0 * half > 2.0 else (0.0, float(n) - 1.0)
    ctr = rng.uniform(lo, hi, size=(batch, 2))
    ctr[0] = [1.37, n - 2.62]
    ctr[1] = [n // 2 + 3.0, n // 2 - 5.0]
    assert np.unique(ctr, axis=0).shape[0] == batch
    return ctr


def zoom_sample_rows(m, pt, limit=32):
    """Window rows for the long-double check of a stage-Y launch with ``pt`` tiles of 16 rows per wave: the first and
    last rows, both sides of every 16-row tile boundary inside the first and the last PT group, both sides of every
    PT-group boundary, and rows inside the last group when it is partial."""
    tiles, group = m // 16, 16 * pt
    ngroups = -(-tiles // pt)
    last0 = (ngroups - 1) * group
    rows = {0, m - 1}
    for g in range(1, ngroups):
        rows.update((g * group - 1, g * group))
    for start, stop in ((0, min(group, m)), (last0, m)):
        for b in range(start + 16, stop, 16):
            rows.update((b - 1, b))
    if tiles % pt:
        rows.update((last0 + 5, m - 7))
    rows = np.array(sorted(r for r in rows if 0 <= r < m), dtype=np.int64)
    assert rows.size <= limit, (m, pt, rows.size)
    return rows


def zoom_weights(n, m, s, c):
    """W[q][j] of one axis in long double, NOT rounded to double: ``zoom_np.weight_matrix`` without its last step."""
    ci = int(np.floor(c))
    tab, carry = zoom_np.phase_table(n, s, c - ci)
    out = np.empty((m, n), dtype=LDR)
    j = np.arange(n)
    for q in range(m):
        a, b = divmod(q - m // 2, s)
        out[q] = tab[b, (ci + a + int(carry[b]) - j) % n]
    return out


def _rows_of(w, rows):
    return w if rows is None else w[np.asarray(rows)]


def zoom_reference(u, m, s, cx, cy, rows=None):
    """U[rows] = (Wy u Wx^T)[rows] in long double (all rows when None): stage Y on those rows, the full stage X."""
    n = u.shape[0]
    wy = _rows_of(zoom_weights(n, m, s, cy), rows)
    wxt = np.ascontiguousarray(zoom_weights(n, m, s, cx).T)
    u = np.asarray(u)
    out = np.empty((wy.shape[0], m), dtype=LD)
    out.real = (wy @ np.ascontiguousarray(u.real).astype(LDR)) @ wxt
    out.imag = (wy @ np.ascontiguousarray(u.imag).astype(LDR)) @ wxt
    return out


def zoom_yardstick(u, m, s, cx, cy, rows=None):
    """The same two contractions in fp64 with the double-rounded weights, summed over k in order by a plain loop."""
    n = u.shape[0]
    wy = _rows_of(zoom_weights(n, m, s, cy).astype(np.float64), rows)
    wx = zoom_weights(n, m, s, cx).astype(np.float64)
    d = np.asarray(u, dtype=np.complex128)
    t = np.zeros((wy.shape[0], n), dtype=np.complex128)
    for k in range(n):
        t += wy[:, k, None] * d[k, None, :]
    out = np.zeros((wy.shape[0], m), dtype=np.complex128)
    for k in range(n):
        out += t[:, k, None] * wx[None, :, k]
    return out


def zoom_rigorous_bound(u, m, s, cx, cy, rows=None):
    """(2 n + 4) 2^-53 (|Wy| |u| |Wx|^T)[rows], per element: two chains of n multiply-adds, each rounded once per term
    (gamma_n each), and four roundings for the two weights of a term, rounded to double from long double by two
    evaluations that may straddle a rounding boundary.  The absolute-value product itself is formed in fp64 (its own
    rounding, 1e-13 of it, does not matter to a worst-case bound that random data stays sqrt(n) below)."""
    n = u.shape[0]
    wy = np.abs(_rows_of(zoom_weights(n, m, s, cy), rows)).astype(np.float64)
    wx = np.abs(zoom_weights(n, m, s, cx)).astype(np.float64)
    return (2 * n + 4) * xp.U64 * ((wy @ np.abs(np.asarray(u, dtype=np.complex128))) @ wx.T)


def zoom_errors(got, ref):
    """(L2-relative error over the rows given, largest element error relative to the peak of the reference there)."""
    r = np.asarray(ref).astype(LD)
    d = np.abs(np.asarray(got).astype(LD) - r).astype(LDR)
    ra = np.abs(r).astype(LDR)
    return float(np.sqrt(np.sum(d * d) / np.sum(ra * ra))), float(np.max(d) / np.max(ra))


def zoom_check(got, ref, yard, rigorous, what):
    """Hold ``got`` to ZOOM_FACTOR x the sequential fp64 yardstick's own error (L2-relative and largest element over the
    peak) and, like the yardstick, to the rigorous bound per element.  Returns (message, kernel / yardstick ratios)."""
    g_l2, g_el = zoom_errors(got, ref)
    y_l2, y_el = zoom_errors(yard, ref)
    worst = []
    for name, arr in (("yardstick", yard), ("kernel", got)):
        d = np.abs(np.asarray(arr).astype(LD) - ref).astype(np.float64)
        over = d > rigorous
        worst.append(float(np.max(d / np.where(rigorous > 0, rigorous, 1.0))))
        assert not over.any(), f"{what}: the {name} exceeds the rigorous bound at {np.argwhere(over)[:4].tolist()}"
    ratio = (g_l2 / y_l2, g_el / y_el)
    msg = (f"{what}: kernel L2 {g_l2:.3g} / peak {g_el:.3g}; sequential fp64 yardstick L2 {y_l2:.3g} / peak {y_el:.3g}; "
           f"kernel / yardstick {ratio[0]:.2f} / {ratio[1]:.2f} (gate {ZOOM_FACTOR:g}); share of the rigorous bound: "
           f"yardstick {worst[0]:.3g}, kernel {worst[1]:.3g}")
    assert g_l2 <= ZOOM_FACTOR * y_l2 and g_el <= ZOOM_FACTOR * y_el, msg
    return msg, ratio


# ---- transfer functions -------------------------------------------------------------------------------------------------
OTF_COLS_PER_WORKGROUP = 2  # csrc/focus_otf.hip: the OTF column pass at 4096 (tile_pass) runs COL_LINES x COL_TILES = 2 x 1 columns per workgroup


def otf_random_field(n):
    """Item 0: the seeded random field of tests/test_gpu_otf.py (its PSF is |u|^2)."""
    rng = np.random.default_rng(8080 + n)
    return rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))


def otf_structured_psf(n):
    """Item 1, aimed at the row packing and the self-mirror columns: a compact blob (FWHM ~6 px) off centre by a
    non-integer number of pixels in both axes, plus content on even rows only in the left half and on odd rows only in
    the right half, plus a nonzero column 0 and a nonzero column N/2."""
    rng = np.random.default_rng(9090 + n)
    y, x = np.mgrid[0:n, 0:n].astype(np.float64)
    sigma = 6.0 / 2.3548200450309493
    p = np.exp(-((x - (n / 2 + 3.37)) ** 2 + (y - (n / 2 - 5.81)) ** 2) / (2.0 * sigma * sigma))
    h = n // 2
    p[0::2, :h] += 0.05 * rng.random((h, h))
    p[1::2, h:] += 0.05 * rng.random((h, h))
    p[:, 0] += 0.02 + 0.03 * rng.random(n)
    p[:, h] += 0.02 + 0.03 * rng.random(n)
    return p


def otf_fields(n):
    """The batch of two fields whose kept PSFs are the inputs (the structured one is real: u = sqrt(P))."""
    return [otf_random_field(n), np.sqrt(otf_structured_psf(n)).astype(np.complex128)]


def otf_sample_indices(n):
    """Unshifted frequency indices for the sampled check: 0, 1, N/2 - 1 and N/2 (0 and N/2 mirror onto themselves), N/2 + 1
    and N - 1 (served by conjugation in otf_value), both sides of the first workgroup boundary of the column launch, and
    one column in between.  At most 16."""
    w = OTF_COLS_PER_WORKGROUP
    s = {0, 1, w - 1, w, n // 2 - 1, n // 2, n // 2 + 1, n - 1, 3 * n // 8 + 1}
    out = np.array(sorted(s), dtype=np.int64)
    assert out.size <= 16
    return out


def otf_reference(psf):
    """fft2(ifftshift(P)) over its zero-frequency value, in long double, UNSHIFTED indices [ky][kx]."""
    p = np.fft.ifftshift(np.asarray(psf, dtype=np.float64)).astype(LD)
    s = np.fft.fft2(p)
    assert s.dtype == LD
    return s / s[0, 0].real


def otf_reference_lines(psf, idx, rows=False):
    """The columns ``idx`` (unshifted kx) of ``otf_reference`` without the whole transform, shape (N, len(idx)):
    S[:, kx] = FFT_y(P' e^{-2 pi i j kx / N}) with P' = ifftshift(P) and the integer phase reduced mod N before it is
    scaled.  ``rows``: the same routine on P^T -- the frequency ROWS ``idx``, returned transposed (line l is [:, l])."""
    p = np.fft.ifftshift(np.asarray(psf, dtype=np.float64))
    if rows:
        p = p.T
    p = np.ascontiguousarray(p).astype(LDR)
    n = p.shape[0]
    idx = np.asarray(idx, dtype=np.int64)
    two_pi = 2 * np.arctan2(LDR(0), LDR(-1))
    a = two_pi * np.mod(np.outer(np.arange(n, dtype=np.int64), idx), n).astype(LDR) / LDR(n)
    part = np.empty((n, idx.size), dtype=LD)
    part.real = p @ np.cos(a)
    part.imag = -(p @ np.sin(a))
    s = np.fft.fft(part, axis=0)
    assert s.dtype == LD
    return s / np.sum(p)


def otf_yardstick(psf, precision):
    """NumPy's own fft2 in the context's precision on the same PSF, unshifted, scaled by the rounded reciprocal of its
    zero-frequency value as the kernels do; an fp32 context's otf_row_kernel rounds the PSF to float32 when it loads it."""
    p = np.fft.ifftshift(np.asarray(psf, dtype=np.float64))
    if precision == "fp32":
        s = np.fft.fft2(p.astype(np.float32).astype(np.complex64))
        assert s.dtype == np.complex64
        s = s.astype(np.complex128)
    else:
        s = np.fft.fft2(p)
    return s * (1.0 / s[0, 0].real)


def otf_unshifted(centred):
    """The unshifted view of a fetched (centred) OTF or MTF."""
    return np.fft.ifftshift(np.asarray(centred))


def otf_scales(spectrum):
    """What an element's error is measured against: per unshifted row ky and column kx the largest value and the L2 norm
    of that line of ``spectrum`` (any fp64 evaluation of the normalised spectrum: scales need no extended precision).
    The zero-frequency element counts for the row and the column it lies on, which it dominates."""
    a = np.abs(np.asarray(spectrum)).astype(np.float64)
    return {"rowmax": a.max(axis=1), "colmax": a.max(axis=0), "rownorm": np.sqrt((a * a).sum(axis=1)),
            "colnorm": np.sqrt((a * a).sum(axis=0))}


def otf_line_errors(got, ref, kys, kxs, axis, scales):
    """Per-line errors of the block [kys][kxs] (unshifted indices; None: all) of an OTF, lines along ``axis`` as in
    ``xprec_np.line_errors`` (0: rows, 1: columns), the zero-frequency element left out.  What differs from
    ``xprec_np.line_errors`` is the scale of an element: the LARGER of the two lines through it, row ky and column kx.
    The model of one line transform (error relative to the line's own content) is wrong for the elements of a 2-D
    transform whose lines differ in size: the row pass leaves an error relative to the content of the rows, its
    systematic part adds up coherently at the frequencies ky where the rows share structure (ky = 0 and N/2 for content
    that alternates between even and odd rows), and it arrives in every column, however little that column holds
    itself.  NumPy's own fp64 fft2 shows it: against the line's own content the structured input of
    ``otf_structured_psf`` reaches 150 u at 1024^2, the elements on the zero-frequency row and column (which the
    zero-frequency value dominates) 230 u.  For a spectrum whose lines are alike the two measures agree.

    The L2 measure is taken along frequency ROWS only (``axis`` 0; along columns it is returned as 0.0 and the element
    measure alone holds the line).  A PSF is non-negative, so every row's own DC is its largest bin by far, and a
    Cooley-Tukey row transform forms some bins kx from partial sums that are large and cancel: kx = odd N / 2^j from 2^j
    sums of row-DC / 2^j each, and for a half-empty row the neighbours of those bins as well (the first sidelobes of the
    sub-transforms' DC).  The rounding of the partial sums lands in those bins of EVERY row, so along such a column it adds
    up in L2, while along a frequency row it is a few elements among N.  NumPy's fp64 fft2 once more: against the
    column's own content the per-column L2 error of the 4096^2 random PSF is 3 u at ordinary columns but 33 u at N/2, 23 u
    at N/4 and 16 u at N/8 (0.51, 0.36, 0.25 u of column 0's norm: 2^(-j/2)), and 38 u at N/2 - 1 for the structured PSF
    (half the bound is 26 u) -- while no frequency row of either exceeds 4 u and no element 31 u of its scale.

    Returns (the largest per-line L2 error, the largest element error), each relative to its scale."""
    n = scales["rowmax"].size
    kys = np.arange(n) if kys is None else np.asarray(kys)
    kxs = np.arange(n) if kxs is None else np.asarray(kxs)
    d = np.abs(np.asarray(got).astype(LD) - np.asarray(ref).astype(LD)).astype(np.float64)
    assert d.shape == (kys.size, kxs.size) and (kys.size if axis == 1 else kxs.size) == n, "whole lines along the axis"
    d[np.ix_(kys == 0, kxs == 0)] = 0.0
    smax = np.maximum(scales["rowmax"][kys][:, None], scales["colmax"][kxs][None, :])
    if axis == 1:
        return 0.0, float(np.max(d / smax))
    q = d / np.maximum(scales["rownorm"][kys][:, None], scales["colnorm"][kxs][None, :])
    return float(np.max(np.sqrt((q * q).sum(axis=1)))), float(np.max(d / smax))


def otf_bound(n, precision, mtf=False):
    """Two line transforms per element and four roundings (the untangling add, the exact halving, the scale by 1 / dc):
    ``xprec_np.bound(n, 2, 1, precision)``; |OTF| pays one more rounding, in doubles in either kind of context."""
    l2, el = xp.bound(n, 2, 1, precision)
    return (l2 + xp.U64, el + 2 * xp.U64) if mtf else (l2, el)


def otf_check(got, ref, yard, kys, kxs, axis, scales, precision, what, mtf=False):
    """``xprec_np.check`` semantics with ``otf_line_errors``: the kernel within the bound, the yardstick within half."""
    n = scales["rowmax"].size
    b_l2, b_el = otf_bound(n, precision, mtf)
    g_l2, g_el = otf_line_errors(got, ref, kys, kxs, axis, scales)
    y_l2, y_el = otf_line_errors(yard, ref, kys, kxs, axis, scales)
    msg = (f"{what}: kernel L2 {g_l2:.3g} / element {g_el:.3g}; NumPy {precision} yardstick L2 {y_l2:.3g} / element "
           f"{y_el:.3g}; bound L2 {b_l2:.3g} / element {b_el:.3g}")
    assert b_l2 >= 2 * y_l2 and b_el >= 2 * y_el, "bound tighter than twice the yardstick -- " + msg
    assert g_l2 <= b_l2 and g_el <= b_el, msg
    return msg


# ---- through-focus planes -------------------------------------------------------------------------------------------------
FOCUS_SX, FOCUS_SY = 0.9, 1.3
FOCUS_TARGETS = (1.0e2, 1.0e6)  # the phase argument at the grid corner of the two planes, rad


def focus_field(n, item):
    rng = np.random.default_rng(515100 + 3 * n + item)
    return rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))


def corner_coef(target, n, sx, sy):
    """coef so that the argument of a natural-order quadratic phase at the grid corner (g = -n/2) is ``target``."""
    return target / ((0.5 * n * sx) ** 2 + (0.5 * n * sy) ** 2)


def focus_plane_blocks(n, target, full2d=False):
    """[3][5] blocks of one plane: item 0 with sy = 0, item 1 with sx = 0, item 2 disabled -- or, ``full2d``, with a
    full 2-D H (sx != sy, both nonzero)."""
    b = np.zeros((3, 5))
    b[0] = [1.0, FOCUS_SX, 0.0, corner_coef(target, n, FOCUS_SX, 0.0), -1.0]
    b[1] = [1.0, 0.0, FOCUS_SY, corner_coef(0.7 * target, n, 0.0, FOCUS_SY), -1.0]
    b[2] = [0.0, FOCUS_SX, FOCUS_SY, corner_coef(target, n, FOCUS_SX, FOCUS_SY), -1.0]
    if full2d:
        b[2, 0] = 1.0
    return b


def focus_blocks(n, plane):
    """The block table of ``focus_passes`` / ``focus_passes_1d``: forward, inverse, 1/N, H of ``plane`` ([batch][5])."""
    plane = np.asarray(plane, dtype=np.float64)
    blocks = np.zeros((4, plane.shape[0], 5))
    blocks[0, :] = [1.0, 0.0, 0.0, 0.0, 0.0]
    blocks[1, :] = [1.0, 1.0, 0.0, 0.0, 0.0]
    blocks[2, :] = [1.0, 0.0, 0.0, 1.0 / n, 0.0]
    blocks[3] = plane
    return blocks


def focus_passes():
    """rows[FFT], cols[FFT | mid H, 1/N | IFFT], rows[IFFT | mid 1/N] (csrc/focus_pass.h), H = PW_QPHASE_NATURAL."""
    h, sc = (_lib.PW_QPHASE_NATURAL, 0, 3), (_lib.PW_SCALE, 0, 2)
    return [{"axis": 0, "fft1": 0}, {"axis": 1, "fft1": 0, "fft2": 1, "mid": [h, sc]}, {"axis": 0, "fft1": 1, "mid": [sc]}]


def focus_passes_1d(axis):
    """What ``focus_passes`` is in exact arithmetic when H does not vary across the lines of ``axis`` (0: rows, sy = 0;
    1: columns, sx = 0), or is 1: IFFT(H FFT(line)) / N line by line."""
    return [{"axis": axis, "fft1": 0, "fft2": 1, "mid": [(_lib.PW_QPHASE_NATURAL, 0, 3)], "post": [(_lib.PW_SCALE, 0, 2)]}]


def focus_restate(u, n, plane, item, lines=None, dtype=LD):
    """One item of a plane: items 0 / 1 on the sampled rows / columns ``lines`` (``u`` holds just those), a disabled
    item on sampled rows (the round trip), ``lines`` None: the whole-field program."""
    blocks = focus_blocks(n, plane)
    if lines is None:
        return xp.run_item(u, focus_passes(), blocks, item, n, dtype=dtype)
    p = np.asarray(plane)[item]
    axis = 1 if (p[0] != 0.0 and p[1] == 0.0) else 0
    assert p[0] == 0.0 or (p[2] == 0.0 if axis == 0 else p[1] == 0.0), "H varies across the lines"
    sel = {"rows": lines} if axis == 0 else {"cols": lines}
    return xp.run_item(u, focus_passes_1d(axis), blocks, item, n, dtype=dtype, **sel)


def focus_check(got, ref, yard, axis, n, k_phase, precision, what):
    """Four line transforms and ``k_phase`` phase factors per element: ``xprec_np.check`` in fp64; an fp32 context pays
    the generic family's factor bound per phase factor on top of the transforms' rounding (as tests/test_gpu_xprec.py)."""
    if precision == "fp64":
        return xp.check(got, ref, yard, axis, n, 4, k_phase, precision, what)[4]
    b_l2, b_el = xp.bound(n, 4, 0, precision)
    extra = k_phase * xp.FP32_FACTOR_BOUND["generic"]
    g_l2, g_el = xp.line_errors(got, ref, axis)
    y_l2, y_el = xp.line_errors(yard, ref, axis)
    msg = (f"{what}: kernel L2 {g_l2:.3g} / element {g_el:.3g}; NumPy fp32 yardstick L2 {y_l2:.3g} / element {y_el:.3g}; "
           f"bound L2 {b_l2 + extra:.3g} / element {b_el + extra:.3g}")
    assert b_l2 + extra >= 2 * y_l2 and b_el + extra >= 2 * y_el, "bound tighter than twice the yardstick -- " + msg
    assert g_l2 <= b_l2 + extra and g_el <= b_el + extra, msg
    return msg


# ---- detector: the chunk loop ---------------------------------------------------------------------------------------------
def _detector_scratch_bytes():
    """PAOS_DETECTOR_SCRATCH_MIB as include/paos_hip.h declares it now: a changed cap changes the chunks computed here."""
    import os
    import re

    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "paos_hip.h")
    with open(header) as fh:
        found = re.search(r"PAOS_DETECTOR_SCRATCH_MIB\s*=\s*(\d+)", fh.read())
    assert found, "include/paos_hip.h no longer declares PAOS_DETECTOR_SCRATCH_MIB"
    return int(found.group(1)) << 20


DETECTOR_SCRATCH_BYTES = _detector_scratch_bytes()


def detector_footprint_rows(ny, py, yc, dy, n):
    """[k0, k1): the grid rows under detector rows 0 .. ny - 1 (csrc/detector.hip, from det_edge's formula)."""
    e = (yc + (np.array([0.0, float(ny)]) - 0.5 * ny) * py) / dy + (0.5 * n + 0.5)
    k0 = int(min(max(np.floor(e[0]), 0.0), n))
    k1 = int(min(max(np.ceil(e[1]), 0.0), n))
    return k0, max(k0, k1)


def detector_chunks(rows_bytes, image_bytes=None, cap=DETECTOR_SCRATCH_BYTES):
    """The chunks [start, end) of detector_run's loop for items with ``rows_bytes`` of row scratch each; ``image_bytes``
    (the images form): a chunk's images must fit the cap as well."""
    out, start = [], 0
    while start < len(rows_bytes):
        used, end = 0, start
        while end < len(rows_bytes):
            fits = used + rows_bytes[end] <= cap and (image_bytes is None or (end - start + 1) * image_bytes <= cap)
            if end > start and not fits:
                break
            used += rows_bytes[end]
            end += 1
        out.append((start, end))
        start = end
    return out
