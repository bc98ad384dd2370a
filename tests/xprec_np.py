"""Extended-precision restatement of one pass program (include/paos_hip.h: paos_run_passes) -- the yardstick the pass
kernels are held to at the 1e-16 level (tests/test_gpu_xprec.py).

The semantics are those of ``tests/fakes.py:ModelDevice.run_passes``; what differs is the precision:

* the field is carried as ``np.clongdouble`` (x87 80-bit, eps ~1.1e-19) and the transforms are ``np.fft`` in long double;
* each phase ARGUMENT is formed in fp64, rounded once per operation as the reference and the kernels define it
  (x = g sx, y = g sy, s = x^2 + y^2, q = coef s, [2 pi q]) -- the kernels promise that rounding, so the error budget
  below covers the function evaluation and the FFT, not argument conditioning (~1e-4 rad at 1e12) -- and then
  exp(i sgn q) is evaluated in long double;
* aperture weights (PW_MASK) are an input (``masks``): the GPU tests pass the library's own rendered mask, which keeps
  these checks about pass arithmetic.

``dtype`` = complex128 / complex64 gives the NumPy restatement of the same case in that precision: the "yardstick", what
a correct FFT in that precision achieves.

Every pass transforms lines independently, so a program whose passes all run along one axis can be restated on a subset
of its lines (``rows`` / ``cols``: the grid indices of the lines carried, see ``sample_lines``).  Test infrastructure only.
"""
import numpy as np

from paos_amd import _lib

LD = np.clongdouble
U64 = 2.0**-53
U32 = 2.0**-24
TWO_PI = 6.283185307179586  # the fp64 constant of the reference (2 * np.pi) and the kernels
# fp32 phase factors (slot_factor32: hardware v_sin_f32 / v_cos_f32 on a fraction of a turn; the generic kernels:
# sincos_fast, then one rounding to fp32): largest error observed on an MI355X, per family, and the bound pinned at twice
# that -- never above 16 u32 per factor.  generic: max |factor - exp(i q)| of the stand-alone passes (0.7 u32).  frugal:
# the slots' factors cannot be read without a transform, so this is the largest per-line L2 error of a frugal32 case of
# test_phases_riding_on_transforms, two 4096-point transforms included (8.6 u32): an upper bound on the factor's share.
FP32_OBSERVED = {"generic": 4.21e-8, "frugal": 5.12e-7}
FP32_FACTOR_BOUND = {k: min(2.0 * v, 16 * U32) for k, v in FP32_OBSERVED.items()}


def require_long_double():
    """The reference is only worth something with a wider type than fp64: fail loudly otherwise."""
    eps = float(np.finfo(np.longdouble).eps)
    if eps > 1e-18:
        raise AssertionError(f"np.longdouble has eps {eps:.3g} on this platform: no extended-precision reference")
    got = np.fft.fft(np.ones(8, dtype=LD)).dtype
    if got != LD:
        raise AssertionError(f"np.fft returns {got} for clongdouble input: no extended-precision transforms")


def grid_coords(kind, idx, n):
    """Signed pixel indices g of grid indices ``idx``: centred (idx - n/2) or natural order (FFT order)."""
    idx = np.asarray(idx, dtype=np.int64)
    g = idx - n // 2 if kind == _lib.PW_QPHASE_CENTRED else np.where(idx < n // 2, idx, idx - n)
    return g.astype(np.float64)


def phase_argument(kind, flags, p, n, rows, cols):
    """q[rows][cols] in fp64, one rounding per operation: x = g sx, y = g sy, s = x^2 + y^2, q = coef s, [2 pi q]."""
    x = grid_coords(kind, cols, n) * p[1]
    y = grid_coords(kind, rows, n) * p[2]
    s = (x * x)[None, :] + (y * y)[:, None]
    q = p[3] * s
    if flags & _lib.PWF_MUL2PI:
        q = TWO_PI * q
    return q


def phase_factor(kind, flags, p, n, rows, cols, dtype=LD):
    """cos(q) + i sgn sin(q) of the fp64 argument, evaluated in the precision of ``dtype`` (long double: exact to ~1e-20)."""
    q = phase_argument(kind, flags, p, n, rows, cols)
    real = np.longdouble if dtype == LD else np.float64
    qa = q.astype(real)
    f = (np.cos(qa) + 1j * real(p[4]) * np.sin(qa))
    return f.astype(dtype)


def _apply(u, op, p, n, rows, cols, dtype, mask):
    kind, flags, _ = op
    if kind == _lib.PW_SIGN:
        r = np.asarray(rows)[:, None] & 1
        c = np.asarray(cols)[None, :] & 1
        par = c if flags & _lib.PWF_X_ONLY else (r if flags & _lib.PWF_Y_ONLY else (r + c))
        return np.where(par & 1, -u, u)
    if kind == _lib.PW_SCALE:
        real = np.longdouble if dtype == LD else (np.float32 if dtype == np.complex64 else np.float64)
        return u * real(p[3])
    if kind == _lib.PW_MASK:
        if mask is None:
            raise AssertionError("a PW_MASK operator needs its weights (masks=)")
        return u * np.asarray(mask)[np.ix_(rows, cols)].astype(dtype)
    return u * phase_factor(kind, flags, p, n, rows, cols, LD if dtype == LD else np.complex128).astype(dtype)


def run_item(u, passes, blocks, item, n, rows=None, cols=None, masks=None, dtype=LD):
    """Run a pass program on one batch item.  ``u``: the field on rows x cols (all rows / columns when None), converted
    to ``dtype``; ``blocks``: [n_blocks][batch][5]; ``masks``: {block index: [batch] weight maps (n x n)}.  A pass along
    rows (axis 0) needs every column, a pass along columns every row."""
    rows = np.arange(n) if rows is None else np.asarray(rows)
    cols = np.arange(n) if cols is None else np.asarray(cols)
    u = np.asarray(u).astype(dtype)
    assert u.shape == (rows.size, cols.size)
    blocks = np.asarray(blocks, dtype=np.float64)
    for ps in passes:
        for slot, ctl in (("pre", ps.get("fft1", -1)), ("mid", ps.get("fft2", -1)), ("post", -1)):
            for op in ps.get(slot, ()):
                p = blocks[op[2], item]
                if p[0] == 0.0:
                    continue
                mask = masks[op[2]][item] if (masks is not None and op[0] == _lib.PW_MASK) else None
                u = _apply(u, op, p, n, rows, cols, dtype, mask)
            if ctl is not None and ctl >= 0 and blocks[ctl, item, 0] != 0.0:
                ax = 1 if ps["axis"] == 0 else 0  # "along rows" = NumPy axis 1
                assert (cols if ax == 1 else rows).size == n, "a transform needs whole lines"
                u = np.fft.ifft(u, axis=ax) * n if blocks[ctl, item, 1] else np.fft.fft(u, axis=ax)
                u = u.astype(dtype)
    return u


def sample_lines(n, br=8, group=64):
    """Lines for the long-double checks: the first and last 8; both sides of every boundary of ``group`` lines (the
    tiles and workgroup groups of the layouts); every block-row (``br``) boundary inside the first, middle and last
    ``group`` lines; and a stride of ~1/16 of the rest."""
    s = set(range(min(8, n))) | set(range(max(0, n - 8), n))
    for b in range(0, n, group):
        s.update((b - 1, b))
    for start in (0, n // 2 - group // 2, n - group):
        for b in range(start, start + group + 1, br):
            s.update((b - 1, b))
    s.update(range(3, n, max(1, n // 16)))
    return np.array(sorted(x for x in s if 0 <= x < n), dtype=np.int64)


def line_errors(got, ref, axis):
    """Per-line errors of ``got`` against ``ref`` (lines along ``axis``: 0 = rows, 1 = columns): L2-relative, and the
    largest element error relative to the line's max.  A line whose reference is zero counts its absolute error."""
    g = np.asarray(got).astype(LD)
    r = np.asarray(ref).astype(LD)
    if axis == 1:
        g, r = g.T, r.T
    d = np.abs(g - r).astype(np.longdouble)
    ra = np.abs(r).astype(np.longdouble)
    num = np.sqrt(np.sum(d * d, axis=1))
    den = np.sqrt(np.sum(ra * ra, axis=1))
    l2 = np.where(den > 0, num / np.where(den > 0, den, 1), num)
    mx = np.max(ra, axis=1)
    el = np.where(mx > 0, np.max(d, axis=1) / np.where(mx > 0, mx, 1), np.max(d, axis=1))
    return float(np.max(l2)), float(np.max(el))


def bound(n, n_fft, k_phase, precision):
    """(per-line L2-relative bound, per-element bound relative to the line's max) of a case: (2 n_fft log2 N + 4 K) u and
    twice that; u = 2^-53 (fp64) or 2^-24 (fp32), K = phase factors applied to a point."""
    u = U64 if precision == "fp64" else U32
    l2 = (2 * n_fft * int(np.log2(n)) + 4 * k_phase) * u
    return l2, 2 * l2


def check(got, ref, yard, axis, n, n_fft, k_phase, precision, what):
    """Hold ``got`` (the kernel) to the bound of its case against ``ref`` (long double); ``yard`` (the NumPy restatement in
    the kernel's precision) must stay below half the bound -- no bound is tighter than a correct FFT achieves.  Returns
    the errors (kernel L2, kernel element, yardstick L2, yardstick element) for reports."""
    b_l2, b_el = bound(n, n_fft, k_phase, precision)
    g_l2, g_el = line_errors(got, ref, axis)
    y_l2, y_el = line_errors(yard, ref, axis)
    msg = (f"{what}: kernel L2 {g_l2:.3g} / element {g_el:.3g}; NumPy {precision} yardstick L2 {y_l2:.3g} / element "
           f"{y_el:.3g}; bound L2 {b_l2:.3g} / element {b_el:.3g}")
    assert b_l2 >= 2 * y_l2 and b_el >= 2 * y_el, "bound tighter than twice the yardstick -- " + msg
    assert g_l2 <= b_l2 and g_el <= b_el, msg
    return g_l2, g_el, y_l2, y_el, msg
