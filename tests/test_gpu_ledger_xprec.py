"""The layer that decides how much light there is and what the caller gets back -- power sums and their windows, kept
intensities, stops (swept, from a known power, deferred), tabulated phase screens, the PSD screen built on the device,
exports and import -- against the long-double references and the bounds of tests/ledger_xprec.py, where tests/test_gpu_r3.py,
test_gpu_r5.py and test_gpu_parity.py compare path against path or against fp64 NumPy at 1e-12 .. 1e-15.  Shapes are the
smallest at which each code path exists: 64^2 and 128^2 (fp64), 64^2 (fp32, 4-row blocks), 2048^2 (fp32, 8-row blocks), and
1024^2 fp64 / 2048^2 fp32 where a frugal pass is needed.  Every assertion message carries the kernel's error, the bound and
the yardstick's error; ``pytest -s`` prints them as XPREC lines (profiles/r14_ledger_xprec.md).  Everything goes through
``DeviceFields``."""
import numpy as np
import pytest

import ledger_xprec as lx
import pointwise_xprec as px
import xprec_np as xp

pytestmark = pytest.mark.gpu

LAYOUTS = [(64, "fp64"), (128, "fp64"), (64, "fp32"), (2048, "fp32")]
FRUGAL = [(1024, "fp64"), (2048, "fp32")]
IDS = lambda v: v if isinstance(v, str) else str(v)  # noqa: E731

# The largest device error of each family as a fraction of its bound, on an MI355X (profiles/r14_ledger_xprec.md).  In
# complex64 contexts the one rounding of the store, U32, is nearly the whole bound.  hypot_u, atan2_u and psd_l2_u are the
# device's own figures in u (2^-53): recorded, never fed back into a bound.
OBSERVED_MI355X = {"power": 0.109, "stop_fp64": 0.131, "stop_fp32": 0.998, "ride_fp64": 0.0683, "ride_fp32": 0.147,
                   "phase_map_fp64": 0.247, "phase_map_fp32": 0.996, "psd": 0.0754, "amplitude": 0.407, "phase": 0.353,
                   "hypot_u": 1.64, "atan2_u": 4.22, "psd_l2_u": 4.82}
OBSERVED = dict.fromkeys(OBSERVED_MI355X)


def _lib():
    from paos_amd import _lib as lib

    return lib


def _note(kind, value):
    OBSERVED[kind] = value if OBSERVED[kind] is None else max(OBSERVED[kind], value)


def _batch(n, want):
    return min(want, 2) if n >= 2048 else want


def _bits(a):
    """The bit patterns of a float64 / complex128 array: equality that tells -0 from +0 and one NaN from another."""
    a = np.ascontiguousarray(a)
    return a.view(np.float64).view(np.uint64)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _ctx(lib, n, batch, precision, fields=None):
    dev = lib.DeviceFields(n, batch, precision)
    if fields is not None:
        for i, f in enumerate(fields):
            dev.upload(i, f)
    return dev


def _rows(lines, n):
    return slice(None) if n < 2048 else lines


# ---- a) intensities, f) the import / export pair ------------------------------------------------------------------------------
@pytest.mark.parametrize("n,precision", LAYOUTS, ids=IDS)
def test_intensities_and_field_round_trip_bit_for_bit(n, precision):
    """psf_keep + psf_fetch, psf_keep_power + psf_fetch and download(INTENSITY) equal re^2 + im^2 of the stored field bit
    for bit, every pixel of every item; psf_keep_power's ticket equals norm2_enqueue's bit for bit (one reduction shape);
    download(FIELD) returns the stored field bit for bit, signed zeros, denormals and huge values included -- the one direct
    check that layout_unmap and the import / export pair are inverse at every block position."""
    lib = _lib()
    b = _batch(n, 3)
    fields = [lx.export_inputs(n, precision)[0]] + [lx.field(n, 10 + i) * s for i, s in zip(range(b - 1), (1.0, 1e-3))]
    dev = _ctx(lib, n, b, precision, fields)
    try:
        want = [px.intensity(lx.stored(f, precision)) for f in fields]
        for i in range(b):
            assert _same_bits(dev.download(i), lx.stored(fields[i], precision)), f"item {i}: download(FIELD) is not what was stored"
        dev.psf_keep()
        for i in range(b):
            assert _same_bits(dev.psf_fetch(i), want[i]), f"psf_keep item {i}"
        t0 = dev.norm2_enqueue()
        t1 = dev.psf_keep_power()
        p0, p1 = dev.norm2_fetch(t0), dev.norm2_fetch(t1)
        assert _same_bits(p0, p1), f"psf_keep_power's ticket {p1} differs from norm2_enqueue's {p0}"
        for i in range(b):
            assert _same_bits(dev.psf_fetch(i), want[i]), f"psf_keep_power item {i}"
            assert _same_bits(dev.download(i, lib.WHAT_INTENSITY), want[i]), f"download(INTENSITY) item {i}"
    finally:
        dev.close()


# ---- b) power sums ------------------------------------------------------------------------------------------------------------
def _power_check(got, want, yard, n, what):
    bound = lx.power_bound(n, float(want))
    err, yerr = abs(float(got - want)), abs(float(yard - want))
    msg = (f"{what}: kernel {err / float(want):.3g} relative; NumPy fp64 yardstick {yerr / float(want):.3g}; bound "
           f"{lx.power_bound_rel(n):.3g}")
    assert 2 * yerr <= bound, "bound tighter than twice the yardstick -- " + msg
    assert err <= bound, msg
    _note("power", err / bound)
    return msg


@pytest.mark.parametrize("n,precision", LAYOUTS, ids=IDS)
def test_power_sums_against_long_double(n, precision):
    """norm2, norm2_enqueue and the psf_keep_power ticket of distinct fields, one scaled down and one up as far as the
    squares stay finite (1e-150 / 1e+150; complex64 contexts: 1e-18 / 1e+18, where a float accumulator overflows): each
    inside power_bound of the long-double sum of the fp64 intensities."""
    lib = _lib()
    b = _batch(n, 4)
    small, big = (1e-150, 1e150) if precision == "fp64" else (1e-18, 1e18)
    fields = [lx.field(n, 20 + i) * s for i, s in zip(range(b), (small, big, 1.0, 0.37))]
    dev = _ctx(lib, n, b, precision, fields)
    report = []
    try:
        held = [lx.stored(f, precision) for f in fields]
        want, yard = [lx.power(u) for u in held], [lx.power_np(u) for u in held]
        got = {"norm2": dev.norm2(), "norm2_enqueue": dev.norm2_fetch(dev.norm2_enqueue()),
               "psf_keep_power": dev.norm2_fetch(dev.psf_keep_power())}
        assert _same_bits(got["norm2"], got["norm2_enqueue"]) and _same_bits(got["norm2"], got["psf_keep_power"])
        for name, p in got.items():
            for i in range(b):
                report.append(_power_check(p[i], want[i], yard[i], n, f"{name} {precision} {n}^2 item {i}"))
    finally:
        dev.close()
        print("\nXPREC " + "\nXPREC ".join(report[:b]))


@pytest.mark.parametrize("n,precision", [(64, "fp64"), (64, "fp32")] + FRUGAL, ids=IDS)
def test_power_on_store_against_long_double(n, precision):
    """run_passes(final_intensity=2): the fused path at 1024^2 fp64 / 2048^2 fp32, the fallback at 64^2.  The ticket is
    inside power_bound of the long-double sum of the field the program stored (downloaded), and -- Parseval, one sign and
    one forward transform along rows -- of N sum |u|^2 once the transform's own error is allowed for: a line's L2-relative
    error e moves its power by 2 e, so that allowance is 2 xprec_np.bound(n, 1, 0)[0]."""
    lib = _lib()
    b = _batch(n, 3)
    fields = [lx.field(n, 30 + i) for i in range(b)]
    blocks = np.zeros((2, b, 5))
    blocks[:, :, 0] = 1.0
    passes = [{"axis": 0, "fft1": 1, "pre": [(lib.PW_SIGN, 0, 0)]}]
    dev = _ctx(lib, n, b, precision, fields)
    report = []
    try:
        got = dev.norm2_fetch(dev.run_passes(passes, blocks, final_intensity=2))
        for i in range(b):
            out = dev.download(i)
            report.append(_power_check(got[i], lx.power(out), lx.power_np(out), n, f"power on store {precision} {n}^2 item {i}"))
            exact = n * lx.power(lx.stored(fields[i], precision))
            perr = abs(float((got[i] - exact) / exact))
            allow = lx.power_bound_rel(n) + 2 * xp.bound(n, 1, 0, precision)[0]
            assert perr <= allow, f"item {i}: Parseval off by {perr:.3g} relative (> {allow:.3g})"
    finally:
        dev.close()
        print("\nXPREC " + "\nXPREC ".join(report))


def _windows(n, b, br):
    """name -> ([batch] row windows, [batch] column windows or None, same_as or None)"""
    w = {"rows": ([(5, n - 3)] * b, None, None),
         "box": ([(5, n - 3)] * b, [(3, n - 5)] * b, None),
         "per item": ([(5 + 3 * i, n - 3 - 2 * i) for i in range(b)], [(3 + 9 * i, n - 5 - 3 * i) for i in range(b)], None),
         "same_as": ([(5, n - 3)] * b, [(3, n - 5)] * b, [0, 0, 2, 2][:b])}
    if n < 2048:
        w.update({"same_as rows": ([(6, n - 9)] * b, None, [0, 0, 2, 2][:b]),
                  "one block": ([(br, 2 * br)] * b, [(2 * br, 3 * br)] * b, None),
                  "full": ([(0, n)] * b, [(0, n)] * b, None),
                  "empty": ([(5, 5)] + [(2 * br, 2 * br)] * (b - 1), [(3, n - 5)] * b, None),
                  "empty columns": ([(5, n - 3)] * b, [(7, 7)] + [(br, br)] * (b - 1), None)})
    return w


@pytest.mark.parametrize("n,precision", LAYOUTS, ids=IDS)
def test_windowed_sums_equal_the_full_sum_of_the_zero_filled_field(n, precision):
    """include/paos_hip.h: "bit-identical to the full sum of the zero-filled field".  The context holds NaN and +-huge
    everywhere outside the outward-rounded window (ledger_xprec.poison) and real zeros between the nominal and the rounded
    window; norm2_enqueue(live_rows), (live_rows, live_cols) and (..., same_as) must equal, bit for bit, norm2_enqueue() of a
    second context holding the zero-filled field, and lie inside power_bound of its long-double sum.  Windows that are no
    block multiple, per-item windows, one block, the full grid, an empty window (exactly 0.0).  In the same_as cases the
    followers' fields are entirely poison: they are never read and receive their leader's sum."""
    lib = _lib()
    b = _batch(n, 4)
    br = lx.block_rows(n, precision)
    base = [lx.stored(lx.field(n, 40 + i), precision) for i in range(b)]
    a, z = _ctx(lib, n, b, precision), _ctx(lib, n, b, precision)
    report = []
    try:
        for name, (rows, cols, same) in _windows(n, b, br).items():
            filled = []
            for i in range(b):
                ci = None if cols is None else cols[i]
                lead = i if same is None else same[i]
                filled.append(lx.window_field(base[lead], rows[i], ci, br))
                a.upload(i, lx.poison(base[i], rows[i], ci, br, precision) if lead == i
                         else lx.poison(base[i], (0, 0), None, br, precision))
                z.upload(i, filled[i])
            kw = {} if cols is None else {"live_cols": np.array(cols, dtype=np.float64)}
            if same is not None:
                kw["same_as"] = same
            got = a.norm2_fetch(a.norm2_enqueue(np.array(rows, dtype=np.float64), **kw))
            want = z.norm2_fetch(z.norm2_enqueue())
            assert _same_bits(got, want), f"{name} {precision} {n}^2: windowed {got} != full sum of the zero-filled field {want}"
            for i in range(b):
                exact = lx.power(filled[i])
                if exact == 0:
                    assert got[i] == 0.0 and not np.signbit(got[i]), (name, i, got[i])
                else:
                    report.append(_power_check(got[i], exact, lx.power_np(filled[i]), n, f"window '{name}' {precision} {n}^2 item {i}"))
            if "empty" in name:
                assert got[0] == 0.0, (name, got)
    finally:
        a.close()
        z.close()
        print("\nXPREC " + "\nXPREC ".join(report[:4]))


@pytest.mark.parametrize("cols_of", [lambda n: (3, n - 5), lambda n: (9, n - 11)], ids=["cols 3..n-5", "cols 9..n-11"])
@pytest.mark.parametrize("n,precision", LAYOUTS, ids=IDS)
def test_start_sum_and_zeroing_share_one_window(n, precision, cols_of):
    """rounded_cols' promise ("ONE window"): start(..., write_rows, write_cols) on a sentinel-filled context writes exactly
    the outward-rounded box (rows and columns to whole blocks of the context's block height: the first column window tells
    that from rounding to the two-column block when blocks are 4 rows high, the second when they are 8); the norm2_enqueue
    box ticket sums exactly that box; zero_outside_rows(rows, cols) leaves exactly that box, unchanged inside; and norm2()
    of the zeroed field equals the ticket taken before, bit for bit."""
    lib = _lib()
    br = lx.block_rows(n, precision)
    rows, cols = (5, n - 3), cols_of(n)
    r0, r1 = lx.window_round(*rows, br, n)
    c0, c1 = lx.window_round(*cols, br, n)
    box = np.zeros((n, n), dtype=bool)
    box[r0:r1, c0:c1] = True
    two = np.zeros((n, n), dtype=bool)  # what rounding the columns to the layout's two-column blocks would have given
    two[r0:r1, (cols[0] // 2) * 2:((cols[1] + 1) // 2) * 2] = True
    assert not np.array_equal(box, two)
    sentinel = 7.0 - 3.0j
    lr, lc = np.array([rows] * 2, dtype=np.float64), np.array([cols] * 2, dtype=np.float64)
    dev = _ctx(lib, n, 2, precision)
    try:
        dev.fill(sentinel)
        dev.start(1.0, lib.SHAPE_ELLIPSE, np.zeros((2, 8)), None, write_rows=lr, write_cols=lc)
        ticket = dev.norm2_enqueue(lr, live_cols=lc)
        before = [dev.download(i) for i in range(2)]
        power = dev.norm2_fetch(ticket)
        for i in range(2):
            changed = before[i] != sentinel
            assert np.array_equal(changed, box), (f"item {i}: start wrote {int(changed.sum())} pixels, the rounded box has "
                                                  f"{int(box.sum())}; first differences {np.argwhere(changed != box)[:4].tolist()}")
            assert (before[i][box] == 1.0).all()
            assert power[i] == float(box.sum()), (i, power[i], int(box.sum()))
        dev.zero_outside_rows(lr, lc)
        after = [dev.download(i) for i in range(2)]
        total = dev.norm2()
        for i in range(2):
            assert _same_bits(after[i][box], before[i][box]), f"item {i}: zeroing changed the box"
            assert (after[i][~box] == 0).all(), f"item {i}: {int((after[i][~box] != 0).sum())} pixels outside the box survive"
        assert _same_bits(total, power), (total, power)
    finally:
        dev.close()


# ---- c) stops -----------------------------------------------------------------------------------------------------------------
def _stop_check(got, u, n, precision, what, bound=None):
    ref, p = lx.stop_reference(u)
    bound = lx.stop_bound(n, precision) if bound is None else bound
    err = lx.relative_element_error(got, ref)
    yerr = lx.relative_element_error(lx.stop_np(u), ref)
    msg = f"{what}: kernel {err:.3g} of |u| / sqrt(P) per element; NumPy fp64 yardstick {yerr:.3g}; bound {bound:.3g}"
    assert 2 * yerr <= lx.stop_bound(n, "fp64"), "bound tighter than twice the yardstick -- " + msg
    assert err <= bound, msg
    _note("stop_" + precision, err / bound)
    return msg


@pytest.mark.parametrize("n,precision", LAYOUTS, ids=IDS)
def test_make_stop_against_long_double(n, precision):
    """make_stop(enable = [1, 0, 1]): enabled items inside stop_bound of u / sqrt(P_ld) per element, the disabled item bit
    for bit untouched, norm2() afterwards within power_bound + 2 stop_bound of 1.  An all-zero item: the reference computes
    0 * (1 / sqrt(0)) = 0 * inf and yields NaN in every element -- parity with NumPy's u /= sqrt(sum |u|^2)."""
    lib = _lib()
    b = _batch(n, 3)
    enable = [1.0, 0.0, 1.0][:b]
    fields = [lx.field(n, 50 + i) * s for i, s in zip(range(b), (3.0, 1.0, 1e-3))]
    dev = _ctx(lib, n, b, precision, fields)
    report = []
    try:
        held = [lx.stored(f, precision) for f in fields]
        dev.make_stop(enable)
        total = dev.norm2()
        for i in range(b):
            got = dev.download(i)
            if enable[i] == 0.0:
                assert _same_bits(got, held[i]), "the disabled item changed"
                continue
            report.append(_stop_check(got, held[i], n, precision, f"make_stop {precision} {n}^2 item {i}"))
            allow = lx.power_bound_rel(n) + 2 * lx.stop_bound(n, precision)
            assert abs(total[i] - 1.0) <= allow, f"item {i}: power {total[i]!r} after the stop, more than {allow:.3g} from 1"
        dev.upload(0, np.zeros((n, n), dtype=complex))
        dev.make_stop(enable)
        assert np.isnan(dev.download(0).real).all() and np.isnan(dev.download(0).imag).all(), "an all-zero item must become NaN (0 / 0)"
    finally:
        dev.close()
        print("\nXPREC " + "\nXPREC ".join(report))


def _programs(lib, n, b):
    """(first, second, second with item 1 sitting out, pair, blocks): ``first`` -- a sign and a forward transform along rows
    -- ends with final_intensity = 2; ``second`` is one pass along columns with a phase in front of a forward transform that
    every item takes part in; ``pair`` a forward / inverse pair along columns with the 1 / n scale."""
    blocks = np.zeros((8, b, 5))
    blocks[0, :, 0] = 1.0                                  # sign
    blocks[1, :, 0] = 1.0                                  # forward
    for i in range(b):                                     # a phase along columns, about 1e3 rad at the edge
        blocks[2, i] = [1.0, 0.0, 0.8 + 0.1 * i, 1e3 / ((0.5 * n * (0.8 + 0.1 * i)) ** 2 * xp.TWO_PI), -1.0]
    blocks[3], blocks[4] = blocks[1], blocks[2]            # the same with item 1 switched off
    if b > 1:
        blocks[3, 1, 0] = blocks[4, 1, 0] = 0.0
    blocks[5, :, :2] = [1.0, 1.0]                          # inverse
    blocks[6, :, 0], blocks[6, :, 3] = 1.0, 1.0 / n        # scale 1 / n
    first = [{"axis": 0, "fft1": 1, "pre": [(lib.PW_SIGN, 0, 0)]}]
    second = [{"axis": 1, "fft1": 1, "pre": [(lib.PW_QPHASE_CENTRED, lib.PWF_MUL2PI, 2)]}]
    second_out = [{"axis": 1, "fft1": 3, "pre": [(lib.PW_QPHASE_CENTRED, lib.PWF_MUL2PI, 4)]}]
    pair = [{"axis": 1, "fft1": 1, "fft2": 5, "mid": [(lib.PW_SCALE, 0, 6)]}]
    return first, second, second_out, pair, blocks


@pytest.mark.parametrize("n,precision", [(64, "fp64"), (64, "fp32")] + FRUGAL, ids=IDS)
def test_stop_from_a_known_power_swept_deferred_and_riding(n, precision):
    """Behind a program that ended with final_intensity = 2:

    * make_stop(power_known=True) meets make_stop's bounds and equals make_stop on a twin context to 2 stop_bound;
    * defer=True, then a download: bit-identical to that sweep, and paos_deferred_stop_stats says "settled";
    * defer=True, then a program whose first pass is a frugal pass every item takes part in (1024^2 fp64, 2048^2 fp32): the
      counter says "rode"; the result is inside xprec_np.bound(n, 1, 1) plus stop_bound (relative errors add; fp32: plus
      the frugal family's factor bound) of the long-double program run on the long-double stop; and the next program on
      that context equals the same program on a fresh context holding the same field, bit for bit (dyn_scale is ones again);
    * defer=True, then a program whose first pass cannot take the factor (item 1 sits it out; at 64^2 the generic kernel):
      "settled", and bit-identical to the sweep followed by the same program."""
    lib = _lib()
    b = _batch(n, 3)
    frugal = (n, precision) in FRUGAL
    enable = [1.0, 0.0, 1.0][:b]
    fields = [lx.field(n, 60 + i) for i in range(b)]
    first, second, second_out, pair, blocks = _programs(lib, n, b)
    names = ("plain", "twin", "sweep", "settle", "ride", "out", "sweep_out")
    ctx = {k: _ctx(lib, n, b, precision, fields) for k in names}
    report = []
    try:
        for k in names:
            t = ctx[k].run_passes(first, blocks, final_intensity=0 if k == "twin" else 2)
            if t is not None:
                ctx[k].norm2_fetch(t)
        v0 = [ctx["plain"].download(i) for i in range(b)]
        # the sweep from the known power, and make_stop itself on a twin
        ctx["sweep"].make_stop(enable, power_known=True)
        ctx["twin"].make_stop(enable)
        swept = [ctx["sweep"].download(i) for i in range(b)]
        for i in range(b):
            if enable[i] == 0.0:
                assert _same_bits(swept[i], v0[i])
                continue
            report.append(_stop_check(swept[i], v0[i], n, precision, f"stop from the known power {precision} {n}^2 item {i}"))
            e = lx.relative_element_error(ctx["twin"].download(i), swept[i])
            assert e <= 2 * lx.stop_bound(n, precision), f"item {i}: power_known differs from make_stop by {e:.3g}"
        assert ctx["sweep"].deferred_stop_stats() == (0, 0)
        # deferred, then read: settled by the same sweep
        ctx["settle"].make_stop(enable, power_known=True, defer=True)
        assert ctx["settle"].deferred_stop_stats() == (0, 0)
        for i in range(b):
            assert _same_bits(ctx["settle"].download(i), swept[i]), f"item {i}: a deferred stop read back differs from the sweep"
        assert ctx["settle"].deferred_stop_stats() == (0, 1)
        # deferred, then a first pass that cannot take the factor: settled, and the sweep's bits
        ctx["out"].make_stop(enable, power_known=True, defer=True)
        ctx["sweep_out"].make_stop(enable, power_known=True)
        prog = second_out if (frugal and b > 1) else second
        ctx["out"].run_passes(prog, blocks)
        ctx["sweep_out"].run_passes(prog, blocks)
        assert ctx["out"].deferred_stop_stats() == ((0, 1) if (not frugal or b > 1) else (1, 0))
        if not frugal or b > 1:
            for i in range(b):
                assert _same_bits(ctx["out"].download(i), ctx["sweep_out"].download(i)), f"item {i}: settled in front of a program"
        # deferred, then a first pass that takes it along
        ctx["ride"].make_stop(enable, power_known=True, defer=True)
        ctx["ride"].run_passes(second, blocks)
        stats = ctx["ride"].deferred_stop_stats()
        assert stats == ((1, 0) if frugal else (0, 1)), f"{precision} {n}^2: the deferred stop (rode, settled) = {stats}"
        lines = xp.sample_lines(n, lx.block_rows(n, precision))
        rode = [ctx["ride"].download(i) for i in range(b)]
        for i in range(b):
            start = lx.stop_reference(v0[i])[0] if enable[i] else v0[i].astype(xp.LD)
            ref = xp.run_item(start[:, lines], second, blocks, i, n, cols=lines)
            yard_in = (lx.stop_np(v0[i]) if enable[i] else v0[i])[:, lines].astype(lx.DT[precision])
            yard = xp.run_item(yard_in, second, blocks, i, n, cols=lines, dtype=lx.DT[precision])
            b_l2, b_el = xp.bound(n, 1, 1 if precision == "fp64" else 0, precision)
            extra = lx.stop_bound(n, precision) + (xp.FP32_FACTOR_BOUND["frugal" if frugal else "generic"] if precision == "fp32" else 0.0)
            g_l2, g_el = xp.line_errors(rode[i][:, lines], ref, 1)
            y_l2, y_el = xp.line_errors(yard, ref, 1)
            msg = (f"stop riding on a pass {precision} {n}^2 item {i} ({'rode' if frugal else 'settled'}): kernel L2 {g_l2:.3g} / element "
                   f"{g_el:.3g}; NumPy {precision} yardstick L2 {y_l2:.3g} / element {y_el:.3g}; bound L2 {b_l2 + extra:.3g} / element "
                   f"{b_el + extra:.3g}")
            assert g_l2 <= b_l2 + extra and g_el <= b_el + extra, msg
            _note("ride_" + precision, max(g_l2 / (b_l2 + extra), g_el / (b_el + extra)))
            report.append(msg)
        # the next program on the context that rode: the factor is gone
        fresh = _ctx(lib, n, b, precision, rode)
        try:
            ctx["ride"].run_passes(pair, blocks)
            fresh.run_passes(pair, blocks)
            for i in range(b):
                assert _same_bits(ctx["ride"].download(i), fresh.download(i)), f"item {i}: the program behind the ride still scales"
            assert ctx["ride"].deferred_stop_stats() == stats
        finally:
            fresh.close()
    finally:
        for d in ctx.values():
            d.close()
        print("\nXPREC " + "\nXPREC ".join(report))


# ---- d) tabulated phase screens ---------------------------------------------------------------------------------------------------
def _phase_check(got, u, w, wl, n, precision, lines, what):
    sel = _rows(lines, n)
    ref = lx.phase_map_reference(u[sel], w[sel], wl)
    yard = lx.stored(lx.phase_map_np(u[sel], w[sel], wl), precision)
    b_l2, b_el = lx.phase_map_bound(n, precision)
    g_l2, g_el = lx.phase_map_errors(got[sel], ref, u[sel], precision)
    y_l2, y_el = lx.phase_map_errors(yard, ref, u[sel], precision)
    msg = (f"{what}: kernel L2 {g_l2} / element {g_el:.3g}; NumPy yardstick L2 {y_l2} / element {y_el:.3g}; bound L2 {b_l2} / "
           f"element {b_el:.3g}; largest argument {np.abs(lx.phase_map_argument(w, wl)).max():.3g} rad")
    if precision == "fp64":
        assert 2 * y_l2 <= b_l2 and 2 * y_el <= b_el, "bound tighter than twice the yardstick -- " + msg
        assert g_l2 <= b_l2, msg
        _note("phase_map_fp64", max(g_l2 / b_l2, g_el / b_el))
    else:
        assert y_el <= b_el, "bound tighter than the yardstick -- " + msg
        _note("phase_map_fp32", g_el / b_el)
    assert g_el <= b_el, msg
    return msg


@pytest.mark.parametrize("n,precision", LAYOUTS, ids=IDS)
def test_phase_maps_against_long_double(n, precision):
    """Maps whose fp64 argument covers 0, +-1e-300, both sides of multiples of pi / 2 and 1 .. 1e12 rad with both signs
    (ledger_xprec.phase_map_inputs): phase_map_items(w, [last, 0], [wl_a, wl_b]) inside the bounds of ledger_xprec, the
    unlisted item bit for bit untouched, and equal bit for bit to phase_map(item, w, wl) on a twin context -- the two kernels
    share their expressions."""
    lib = _lib()
    b = _batch(n, 3)
    fields = [lx.field(n, 70 + i) for i in range(b)]
    w = lx.phase_map_inputs(n)
    items, wls = [b - 1, 0], [lx.PHASE_WL, 0.7e-6]
    lines = xp.sample_lines(n, lx.block_rows(n, precision))
    a, t = _ctx(lib, n, b, precision, fields), _ctx(lib, n, b, precision, fields)
    report = []
    try:
        held = [lx.stored(f, precision) for f in fields]
        a.phase_map_items(w, items, wls)
        for i, wl in zip(items, wls):
            t.phase_map(i, w, wl)
        for i in range(b):
            got = a.download(i)
            assert _same_bits(got, t.download(i)), f"item {i}: phase_map_items differs from phase_map"
            if i not in items:
                assert _same_bits(got, held[i]), "the unlisted item changed"
                continue
            report.append(_phase_check(got, held[i], w, wls[items.index(i)], n, precision, lines, f"phase map {precision} {n}^2 item {i}"))
    finally:
        a.close()
        t.close()
        print("\nXPREC " + "\nXPREC ".join(report))


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_phase_map_host_refusals_leave_the_field_untouched(precision):
    """An item listed twice (two slices of one launch would update one field in no order) and a finite map whose argument
    fl(fl(2 pi w) / wl) overflows -- w = 1e308, or w = 1 over wl = 1e-310, also when the map is kept under a key and a later
    call brings the smaller wavelength: PaosHipError, and every item is bit for bit what it was."""
    lib = _lib()
    n, b = 64, 3
    fields = [lx.field(n, 80 + i) for i in range(b)]
    ok = np.ones((n, n))
    huge = np.zeros((n, n))
    huge[17, 5] = -1e308
    dev = _ctx(lib, n, b, precision, fields)
    try:
        held = [lx.stored(f, precision) for f in fields]

        def untouched(what):
            for i in range(b):
                assert _same_bits(dev.download(i), held[i]), f"{what}: item {i} changed"

        with pytest.raises(lib.PaosHipError, match="twice"):
            dev.phase_map_items(ok * 1e-7, [2, 0, 2], [1e-6, 1.1e-6, 1.2e-6])
        untouched("duplicate item")
        for what, call in (("phase_map w = 1e308", lambda: dev.phase_map(1, huge, 1e-6)),
                           ("phase_map wl = 1e-310", lambda: dev.phase_map(1, ok, 1e-310)),
                           ("phase_map_items w = 1e308", lambda: dev.phase_map_items(huge, [0, 1], [1e-6, 2e-6])),
                           ("phase_map_items wl = 1e-310", lambda: dev.phase_map_items(ok, [0, 1], [1e-6, 1e-310], key=5))):
            with pytest.raises(lib.PaosHipError, match="not finite"):
                call()
            untouched(what)
        # the cached-key path: the map is kept under key 5 with a wavelength that passes; the smaller one is still refused,
        # with and without the host buffer
        dev.phase_map_items(ok, [1], [1e-6], key=5)
        held[1] = dev.download(1)
        with pytest.raises(lib.PaosHipError, match="not finite"):
            dev.phase_map_items(None, [0, 2], [1e-6, 1e-310], key=5)
        with pytest.raises(lib.PaosHipError, match="not finite"):
            dev.phase_map_items(ok, [0, 2], [1e-310, 1e-6], key=5)
        untouched("cached key, smaller wavelength")
    finally:
        dev.close()


# ---- e) the PSD screen ----------------------------------------------------------------------------------------------------------
def _psd_cases():
    out = [(name, n) for name in lx.PSD_CASES for n in (64, 128)]
    return out + [("knee_sr_anam", 1024)]


@pytest.mark.parametrize("name,n", _psd_cases(), ids=IDS)
def test_psd_screen_against_long_double(name, n):
    """psd_screen(noise, rough, params, key, want_map=True) inside xprec_np.bound(n, 4, 2) of ledger_xprec.psd_reference (L2
    over the map, and the largest element against max |map|), the host path inside half of it.  The edge-band case places
    fmin and fmax on bins: the device's map must differ from either strict-comparison variant's reference by more than
    100 x the bound -- it made the inclusive choice.  1024^2 is the size production builds on the device
    (phase_maps.PSD_ON_DEVICE_FROM).  Then phase_map_items(None, ..., key) applies the kept map: inside
    xprec_np.bound(n, 0, 1) of the phase reference of the map psd_screen returned."""
    from paos_amd import phase_maps

    lib = _lib()
    assert n < phase_maps.PSD_ON_DEVICE_FROM or n == 1024
    noise, rough, (dx, dy), kw, params = lx.psd_case(name, n)
    ref, keep = lx.psd_reference(noise, rough, params)
    yard = lx.psd_np(noise, rough, (n, n), dx, dy, **kw)
    b_l2, b_el = lx.psd_bound(n)
    u = lx.field(n, 90)
    dev = _ctx(lib, n, 1, "fp64", [u])
    try:
        got = dev.psd_screen(noise, rough, params, key=77, want_map=True)
        g_l2, g_el = lx.psd_errors(got, ref)
        y_l2, y_el = lx.psd_errors(yard, ref)
        msg = (f"psd {name} {n}^2 ({int(keep.sum())} bins): kernel L2 {g_l2 / xp.U64:.2f} u / element {g_el / xp.U64:.2f} u; host path "
               f"L2 {y_l2 / xp.U64:.2f} u / element {y_el / xp.U64:.2f} u; bound {b_l2 / xp.U64:.0f} u / {b_el / xp.U64:.0f} u")
        print("\nXPREC " + msg)
        assert 2 * y_l2 <= b_l2 and 2 * y_el <= b_el, "bound tighter than twice the yardstick -- " + msg
        assert g_l2 <= b_l2 and g_el <= b_el, msg
        _note("psd", max(g_l2 / b_l2, g_el / b_el))
        _note("psd_l2_u", g_l2 / xp.U64)
        if name == "edge_band":
            for flip in (dict(strict_min=True), dict(strict_max=True)):
                d_l2, d_el = lx.psd_errors(got, lx.psd_reference(noise, rough, params, **flip)[0])
                assert d_l2 > 100 * b_l2 and d_el > 100 * b_el, f"{flip}: the device's map is {d_l2:.3g} from the strict variant"
        if n <= 128:
            dev.phase_map_items(None, [0], [lx.PHASE_WL * 1e-3], key=77)  # (nanometre maps: arguments of a few radians)
            lines = xp.sample_lines(n)
            print("XPREC " + _phase_check(dev.download(0), u, got, lx.PHASE_WL * 1e-3, n, "fp64", lines, f"kept psd map {name} {n}^2"))
    finally:
        dev.close()


# ---- f) exports -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,precision", LAYOUTS, ids=IDS)
def test_amplitude_and_phase_exports_against_long_double(n, precision):
    """download(AMPLITUDE) and download(PHASE) of a field with the edge block of ledger_xprec.export_inputs at every block
    position -- signed zeros, the negative real axis with +0 and -0, pure imaginary values, (1, 1e-17), equal components,
    denormals, values whose squares overflow -- against long-double hypot and arctan2.  No bound of the device's hypot /
    atan2 exists in the project: it is 4 x the largest error of np.hypot (relative) / np.arctan2 (absolute) on the same
    inputs, floored at 2 u / 2 u pi (ledger_xprec.export_bounds).  The signed-zero and negative-axis pixels must equal
    np.arctan2 bit for bit; the amplitude is inf exactly where the reference overflows fp64."""
    lib = _lib()
    u, pixels = lx.export_inputs(n, precision)
    dev = _ctx(lib, n, 1, precision, [u])
    try:
        s = lx.stored(u, precision)
        b_amp, b_ph, y_amp, y_ph = lx.export_bounds(s)
        amp, ph = dev.download(0, lib.WHAT_AMPLITUDE), dev.download(0, lib.WHAT_PHASE)
        g_amp, same_inf = lx.amplitude_error(amp, lx.amplitude_reference(s))
        g_ph = lx.phase_error(ph, lx.phase_reference(s))
        msg = (f"exports {precision} {n}^2: hypot {g_amp / xp.U64:.2f} u relative (np.hypot {y_amp / xp.U64:.2f} u, bound {b_amp / xp.U64:.2f} u); "
               f"atan2 {g_ph / xp.U64:.2f} u absolute (np.arctan2 {y_ph / xp.U64:.2f} u, bound {b_ph / xp.U64:.2f} u)")
        print("\nXPREC " + msg)
        _note("hypot_u", g_amp / xp.U64)
        _note("atan2_u", g_ph / xp.U64)
        _note("amplitude", g_amp / b_amp)
        _note("phase", g_ph / b_ph)
        want_ph = np.arctan2(s.imag, s.real)
        names = [name for name, _ in lx.export_edge_values(precision)]
        for k in range(lx.EXPORT_EXACT):
            rows, cols = pixels[k]
            assert _same_bits(ph[rows, cols], want_ph[rows, cols]), \
                f"phase of '{names[k]}': {ph[rows, cols][:2]} (sign bit {np.signbit(ph[rows, cols])[:2]}), np.arctan2 gives {want_ph[rows, cols][0]!r}"
            assert (amp[rows, cols] == np.hypot(s.real, s.imag)[rows, cols]).all(), names[k]
        assert same_inf, "the amplitude is inf where the reference is finite in fp64, or finite where it overflows: " + msg
        k = names.index("huge 1e200" if precision == "fp64" else "huge 1e30")
        assert np.isfinite(amp[pixels[k]]).all()
        assert g_amp <= b_amp and g_ph <= b_ph, msg
    finally:
        dev.close()


def test_zzz_report_observed():
    """(last in the module) the largest errors seen, as fractions of their bounds (``*_u``: in units of u = 2^-53)."""
    print("\nXPREC ledger observed:", {k: (None if v is None else float(f"{v:.3g}")) for k, v in OBSERVED.items()})
