"""The pass kernels against the long-double restatement of tests/xprec_np.py, at the 1e-16 level their source comments
claim (fft_core.h: sincos_fast; frugal_pass.h: sincos_tab, slot_factor, slot_factor32, phase_table_kernel; the radix
stages and their twiddles).  The other GPU tests compare against fp64 NumPy at 1e-11 .. 1e-13 of max|u|, three to five
orders of magnitude above these claims, and none pushes phase arguments towards the 1e12 rad the host accepts.

Every case runs a batch of 2 or 3 items with different parameters; where a third item is present every operator of
it is disabled and it must come back bit for bit.  Long-double checks run on sampled lines (xprec_np.sample_lines:
edges, block-row and tile boundaries, a stride); the bound of a case is xprec_np.bound, and every assertion message
carries the kernel's error next to NumPy's in the same precision.  Everything goes through the C ABI of libpaoship.so."""
import numpy as np
import pytest

import xprec_np as xp
from conftest import rel_err

pytestmark = pytest.mark.gpu

TARGETS = (1.0, 1e3, 1e6, 1e9, 0.99e12)  # phase argument at the grid corner, rad
# the runs of one phase case: two targets per run, the third item disabled
RUNS = ((1.0, 1e3), (1e6, 1e9), (0.99e12, 1.0))
DT = {"fp64": np.complex128, "fp32": np.complex64}
FP32_FACTOR_BOUND = xp.FP32_FACTOR_BOUND  # (tests/xprec_np.py: one value for every module that prices fp32 phase factors)

_FIELDS = {}


def _lib():
    from paos_amd import _lib as lib

    return lib


def _field(n, seed):
    """Seeded complex normals (cached: the 4096^2 ones are reused across cases)."""
    key = (n, seed)
    if key not in _FIELDS:
        if len(_FIELDS) > 6:
            _FIELDS.clear()
        rng = np.random.default_rng(1000 * n + seed)
        _FIELDS[key] = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    return _FIELDS[key]


def _structured(u, axis):
    """Lines where the exact answer is known ride along: an impulse at the last index, a tone at the Nyquist bin and a
    constant (lines 0, 1, 2 along the pass axis)."""
    u = u.copy()
    n = u.shape[0]
    lines = np.zeros((3, n), dtype=complex)
    lines[0, n - 1] = 1.0
    lines[1] = np.where(np.arange(n) & 1, -1.0, 1.0) * (0.5 - 0.25j)
    lines[2] = 1.5 + 0.5j
    if axis == 1:
        u[:, :3] = lines.T
    else:
        u[:3] = lines
    return u


def _corner_coef(target, n, sx, sy, mul2pi):
    """coef so that the argument at the grid corner (g = -n/2 on both axes) is ``target``."""
    h2 = (0.5 * n * sx) ** 2 + (0.5 * n * sy) ** 2
    return target / (h2 * (xp.TWO_PI if mul2pi else 1.0))


def _run(lib, n, precision, fields, passes, blocks, **kw):
    """Upload, run, download (every item); returns (outputs, launch tags, power ticket value or None)."""
    dev = lib.DeviceFields(n, len(fields), precision)
    try:
        for i, f in enumerate(fields):
            dev.upload(i, f)
        dev.profile_begin(lib.KERNEL_PASS_ANY, max_launches=64)
        ticket = dev.run_passes(passes, blocks, **kw)
        power = None if ticket is None else dev.norm2_fetch(ticket)
        _, tags = dev.profile_end_launches()
        if kw.get("final_intensity") == 1:
            out = [dev.psf_fetch(i) for i in range(len(fields))]
        else:
            out = [dev.download(i) for i in range(len(fields))]
        return out, tags, power
    finally:
        dev.close()


def _as_input(f, precision):
    """What the context holds after upload: complex64 contexts round the field."""
    return f.astype(DT[precision]).astype(np.complex128)


def _untouched(got, f, precision, what):
    assert np.array_equal(got, _as_input(f, precision), equal_nan=True), f"{what}: the disabled item changed"


# ---- a) phase factors alone ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("kind,mul2pi", [("centred", True), ("centred", False), ("natural", True), ("natural", False)])
def test_phase_factor_alone_at_corner_arguments_up_to_1e12(precision, kind, mul2pi):
    """A stand-alone pass (axis = -1) of one PW_QPHASE_* on a field of ones returns the factor itself: fp64 within 4 u
    (4.4e-16) absolute of exp(i sgn q), every element, for corner arguments from 1 to 0.99e12 rad (sincos_fast)."""
    lib = _lib()
    n = 512
    op = lib.PW_QPHASE_CENTRED if kind == "centred" else lib.PW_QPHASE_NATURAL
    flags = lib.PWF_MUL2PI if mul2pi else 0
    bound = 4 * xp.U64 if precision == "fp64" else FP32_FACTOR_BOUND["generic"]
    other = _field(n, 1)
    worst = 0.0
    for ta, tb in RUNS:
        blocks = np.zeros((1, 3, 5))
        # different sampling and sign per item, sx != sy
        blocks[0, 0] = [1.0, 1.0, 0.7, _corner_coef(ta, n, 1.0, 0.7, mul2pi), -1.0]
        blocks[0, 1] = [1.0, 0.3, 1.1, _corner_coef(tb, n, 0.3, 1.1, mul2pi), 1.0]
        blocks[0, 2] = [0.0, 2.0, 2.0, 1e3, 1.0]
        ones = np.ones((n, n), dtype=complex)
        out, _, _ = _run(lib, n, precision, [ones, ones, other], [{"axis": -1, "pre": [(op, flags, 0)]}], blocks)
        for i in range(2):
            ref = xp.phase_factor(op, flags, blocks[0, i], n, np.arange(n), np.arange(n))
            err = float(np.max(np.abs(out[i].astype(xp.LD) - ref)))
            q = xp.phase_argument(op, flags, blocks[0, i], n, np.arange(n), np.arange(n))
            worst = max(worst, err)
            assert err <= bound, (f"{precision} {kind} mul2pi={mul2pi} item {i}: max |factor - exp(i q)| = {err:.3g} "
                                  f"> {bound:.3g} (max |q| {np.max(np.abs(q)):.3g} rad)")
        _untouched(out[2], other, precision, "phase alone")
    print(f"\nXPREC phase-alone {precision} {kind} mul2pi={mul2pi}: max abs error {worst:.3g} (bound {bound:.3g})")


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_host_refuses_phase_arguments_at_1e12_and_nan(precision):
    lib = _lib()
    n = 256
    dev = lib.DeviceFields(n, 2, precision)
    try:
        dev.fill(1.0)
        passes = [{"axis": -1, "pre": [(lib.PW_QPHASE_CENTRED, lib.PWF_MUL2PI, 0)]}]
        for coef in (_corner_coef(1.0e12, n, 1.0, 1.0, True) * (1 + 1e-12), _corner_coef(5e12, n, 1.0, 1.0, True),
                     float("nan"), float("inf")):
            blocks = np.zeros((1, 2, 5))
            blocks[0, 0] = [1.0, 1.0, 1.0, 1e-9, 1.0]
            blocks[0, 1] = [1.0, 1.0, 1.0, coef, -1.0]
            with pytest.raises(lib.PaosHipError):
                dev.run_passes(passes, blocks)
        # the same argument on a DISABLED item is not looked at
        blocks[0, 1, 0] = 0.0
        dev.run_passes(passes, blocks)
    finally:
        dev.close()


# ---- b) phase factors riding on transforms ------------------------------------------------------------------------
# (family, precision, n, K, where): the builds that evaluate phases (pass_program.h: lower_frugal; passes.hip: phases_along_lines,
# can_fuse_pair, pick_build)
#   generic   fp64 N <= 512, fp32 N <= 1024; at any N a pass with a post operator ("post") or a phase with |sgn| != 1
#   frugal    fp64 N >= 1024, phases across the lines: sincos_tab; K = 2 in one slot: merged (slot_factor<2>); K = 3 sits in
#             the middle slot (kFrugalMaxPre = 2), in front of it the empty slot (PLAIN)
#   table     phases along the lines only, two passes of a chain in one launch (tag bit 4): phase_table_kernel + reads;
#             "single": one pass over half of the lines (live_rows), whose tables also come from phase_table_kernel
#   frugal32  fp32 N >= 2048: slot_factor32, K = 1 and merged K = 2
PHASE_CASES = [
    ("generic", "fp64", 512, 1, "pre"),
    ("generic", "fp32", 1024, 1, "pre"),
    ("generic", "fp64", 4096, 1, "post"),
    ("generic", "fp64", 2048, 1, "sgn"),
    ("frugal", "fp64", 1024, 1, "pre"),
    ("frugal", "fp64", 1024, 2, "pre"),
    ("frugal", "fp64", 1024, 3, "mid"),
    ("frugal", "fp64", 2048, 2, "pre"),
    ("frugal", "fp64", 4096, 3, "mid"),
    ("table", "fp64", 1024, 1, "fused"),
    ("table", "fp64", 4096, 1, "fused"),
    ("table", "fp64", 2048, 1, "single"),
    ("frugal32", "fp32", 2048, 1, "pre"),
    ("frugal32", "fp32", 2048, 2, "pre"),
    ("frugal32", "fp32", 4096, 2, "pre"),
]


def _phase_program(lib, family, n, k, where, axis, targets, case_no):
    """pre phases -> fft forward -> mid scale 1/N -> fft inverse (the phased field), or with the phases in the middle
    slot (the phases act on the spectrum).  Returns passes, blocks, K per point, transforms per line."""
    nb = 4 + 2 * k
    blocks = np.zeros((nb, 3, 5))
    blocks[0, :2] = [1.0, 0.0, 0.0, 0.0, 0.0]  # forward
    blocks[1, :2] = [1.0, 1.0, 0.0, 0.0, 0.0]  # inverse
    blocks[2, :2] = [1.0, 0.0, 0.0, 1.0 / n, 0.0]  # scale
    blocks[3, :2] = [1.0, 0.0, 0.0, 1.0, 0.0]  # scale by one (a post operator)
    along_only = family == "table"
    ops = []
    for j in range(k):
        kind = lib.PW_QPHASE_CENTRED if (j + case_no) % 2 == 0 else lib.PW_QPHASE_NATURAL
        flags = lib.PWF_MUL2PI if (j + case_no + axis) % 2 == 0 else 0
        ops.append((kind, flags, 4 + j))
        for i, t in enumerate(targets):
            s_along, s_across = (0.9, 0.0) if along_only else ((1.0, 0.6) if i == 0 else (0.45, 1.3))
            sx, sy = (s_along, s_across) if axis == 0 else (s_across, s_along)
            sgn = (0.5 if i == 0 else -0.75) if where == "sgn" else (-1.0 if i == 0 else 1.0)
            # K phases share the target: each gets 1/K of it
            blocks[4 + j, i] = [1.0, sx, sy, _corner_coef(t / k, n, sx, sy, flags != 0), sgn]
    blocks[4:, 2] = [0.0, 0.5, 0.5, 1e-3, 1.0]
    p = {"axis": axis, "fft1": 0, "fft2": 1, "pre": ops, "mid": [(lib.PW_SCALE, 0, 2)]}
    if where == "mid":
        p = {"axis": axis, "fft1": 0, "fft2": 1, "pre": [], "mid": [(lib.PW_SCALE, 0, 2)] + ops}
    if where == "post":
        p["post"] = [(lib.PW_SCALE, 0, 3)]
    passes = [p]
    if where == "fused":
        # the second pass of the chain: the same phases once more (its own blocks would do as well)
        passes = [p, dict(p)]
        return passes, blocks, 2 * k, 4
    return passes, blocks, k, 2


# (a column pass has no row window to halve: the column side of the table slots is the fused case)
PHASE_RUNS = [(c, a) for c in range(len(PHASE_CASES)) for a in (0, 1) if not (PHASE_CASES[c][4] == "single" and a == 1)]


@pytest.mark.parametrize("case_no,axis", PHASE_RUNS, ids=["-".join(map(str, PHASE_CASES[c])) + f"-{a}" for c, a in PHASE_RUNS])
def test_phases_riding_on_transforms(case_no, axis):
    """Every build that evaluates phase factors, at the corner arguments 1 .. 0.99e12 rad, on both axes, against the
    long-double restatement of the same program (the phased field after one round trip)."""
    lib = _lib()
    family, precision, n, k, where = PHASE_CASES[case_no]
    lines = xp.sample_lines(n)
    report = []
    for r, targets in enumerate(RUNS):
        passes, blocks, kk, nfft = _phase_program(lib, family, n, k, where, axis, targets, case_no + r)
        fields = [_structured(_field(n, r), axis), _structured(_field(n, r + 1), axis), _field(n, r + 2)]
        kw = {}
        if where == "single":
            # one pass over the rows [n/4, 3n/4) -- the others are zero in memory: at most half of the lines, so its
            # phase factors come from the tables (passes.hip: stage_groups)
            lo, hi = n // 4, 3 * n // 4
            for f in fields[:2]:
                f[:lo] = 0
                f[hi:] = 0
            kw = {"live_rows": np.array([[lo, hi], [lo, hi], [0, n]], dtype=np.float64)}
        out, tags, _ = _run(lib, n, precision, fields, passes, blocks, **kw)
        if where == "fused":
            assert tags.size == 1 and tags[0] & 16, f"the chain was not fused into one launch: tags {tags}"
        elif n >= 1024 and family != "generic":
            assert not np.any(tags & 48), tags
        _untouched(out[2], fields[2], precision, f"{family} {n}")
        for i in range(2):
            sel = {"rows": lines} if axis == 0 else {"cols": lines}
            fin = _as_input(fields[i], precision)
            part = fin[lines] if axis == 0 else fin[:, lines]
            ref = xp.run_item(part, passes, blocks, i, n, **sel)
            yard = xp.run_item(part.astype(DT[precision]), passes, blocks, i, n, dtype=DT[precision], **sel)
            got = out[i][lines] if axis == 0 else out[i][:, lines]
            what = f"{family} {precision} {n}^2 K={k} {where} axis {axis} corner {targets[i]:.3g} rad"
            if precision == "fp32":
                # each factor may carry the fp32 factor bound on top of the transforms' rounding
                fam = "frugal" if family == "frugal32" else "generic"
                b_l2, b_el = xp.bound(n, nfft, 0, precision)
                extra = kk * FP32_FACTOR_BOUND[fam]
                g_l2, g_el = xp.line_errors(got, ref, axis)
                y_l2, y_el = xp.line_errors(yard, ref, axis)
                msg = (f"{what}: kernel L2 {g_l2:.3g} / element {g_el:.3g}; NumPy yardstick {y_l2:.3g} / {y_el:.3g}; "
                       f"bound {b_l2 + extra:.3g} / {b_el + extra:.3g}")
                report.append(msg)
                assert g_l2 <= b_l2 + extra and g_el <= b_el + extra, msg
            else:
                report.append(xp.check(got, ref, yard, axis, n, nfft, kk, precision, what)[4])
    print("\nXPREC " + "\nXPREC ".join(report))


# ---- c) transforms --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nfft", [1, 2])
@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("n", [64, 128, 256, 512, 1024, 2048, 4096])
def test_transforms_against_long_double(n, precision, axis, nfft):
    """A checkerboard sign in front of one or two transforms, forward on item 0 and inverse on item 1 (item 2 sits it
    out): sampled lines against the long-double restatement at the bound, every line against the fp64 NumPy
    restatement at the existing gate (1e-13 of max|u| fp64, 2e-5 fp32).  Reaches every family: the generic kernels,
    d1024 / d2048 / d4096 and f2048 / f4096."""
    lib = _lib()
    blocks = np.zeros((3, 3, 5))
    blocks[0, :2, 0] = 1.0  # sign
    blocks[1, 0] = [1.0, 0.0, 0.0, 0.0, 0.0]  # item 0 forward
    blocks[1, 1] = [1.0, 1.0, 0.0, 0.0, 0.0]  # item 1 inverse
    blocks[2, :2] = blocks[1, :2]
    passes = [{"axis": axis, "fft1": 1, "fft2": 2 if nfft == 2 else -1, "pre": [(lib.PW_SIGN, 0, 0)]}]
    fields = [_structured(_field(n, 0), axis), _structured(_field(n, 1), axis), _field(n, 2)]
    out, tags, _ = _run(lib, n, precision, fields, passes, blocks)
    _untouched(out[2], fields[2], precision, "transform")
    lines = xp.sample_lines(n)
    gate = 1e-13 if precision == "fp64" else 2e-5
    msgs = []
    for i in range(2):
        fin = _as_input(fields[i], precision)
        sel = {"rows": lines} if axis == 0 else {"cols": lines}
        part = fin[lines] if axis == 0 else fin[:, lines]
        ref = xp.run_item(part, passes, blocks, i, n, **sel)
        yard = xp.run_item(part.astype(DT[precision]), passes, blocks, i, n, dtype=DT[precision], **sel)
        got = out[i][lines] if axis == 0 else out[i][:, lines]
        msgs.append(xp.check(got, ref, yard, axis, n, nfft, 0, precision,
                             f"{precision} {n}^2 axis {axis} nfft {nfft} {'inverse' if i else 'forward'}")[4])
        whole = xp.run_item(fin, passes, blocks, i, n, dtype=np.complex128)
        err = rel_err(out[i], whole)
        assert err < gate, (i, err)
        del whole
    print("\nXPREC " + "\nXPREC ".join(msgs))


# ---- d) fused, storing and pruned launches ---------------------------------------------------------------------------
def _chain(lib, n, axis, count, across=False):
    """``count`` passes of one row / column chain: along-line phase, forward, scale 1/N (+ a phase), inverse."""
    blocks = np.zeros((4 + 2 * count, 3, 5))
    blocks[0, :2] = [1.0, 0.0, 0.0, 0.0, 0.0]
    blocks[1, :2] = [1.0, 1.0, 0.0, 0.0, 0.0]
    blocks[2, :2] = [1.0, 0.0, 0.0, 1.0 / n, 0.0]
    blocks[3, :2] = [1.0, 0.0, 0.0, 0.0, 0.0]
    passes = []
    for q in range(count):
        for i, (t, sg) in enumerate(((3e4, -1.0), (7e8, 1.0))):
            for j, s in enumerate((0.8, 1.3)):
                sxy = (s, 0.4 if (across and q == 1 and j == 0) else 0.0)
                sx, sy = sxy if axis == 0 else sxy[::-1]
                blocks[4 + 2 * q + j, i] = [1.0, sx, sy, _corner_coef(t * (q + 1), n, sx, sy, j == 0), sg]
        passes.append({"axis": axis, "fft1": 0, "fft2": 1, "pre": [(lib.PW_QPHASE_CENTRED, lib.PWF_MUL2PI, 4 + 2 * q)],
                       "mid": [(lib.PW_SCALE, 0, 2), (lib.PW_QPHASE_NATURAL, 0, 5 + 2 * q)]})
    return passes, blocks


@pytest.mark.parametrize("n,precision", [(1024, "fp64"), (2048, "fp64"), (2048, "fp32")])
@pytest.mark.parametrize("axis", [0, 1])
def test_fused_chains_against_long_double(n, precision, axis):
    """Two and three passes of one chain in one launch (can_fuse_pair: tag bit 4 / 5) and, for contrast, a chain the
    library must not fuse (a phase that varies across the lines in the second pass: tags & 48 == 0) -- each against
    the long-double restatement on sampled lines."""
    lib = _lib()
    lines = xp.sample_lines(n)
    for count, across, want in ((2, False, 16), (3, False, 32), (2, True, 0)):
        passes, blocks = _chain(lib, n, axis, count, across)
        fields = [_field(n, 3), _field(n, 4), _field(n, 5)]
        out, tags, _ = _run(lib, n, precision, fields, passes, blocks)
        if want:
            assert tags.size == 1 and tags[0] & want, (count, tags)
        else:
            assert tags.size == count and not np.any(tags & 48), tags
        _untouched(out[2], fields[2], precision, "chain")
        for i in range(2):
            sel = {"rows": lines} if axis == 0 else {"cols": lines}
            fin = _as_input(fields[i], precision)
            part = fin[lines] if axis == 0 else fin[:, lines]
            ref = xp.run_item(part, passes, blocks, i, n, **sel)
            yard = xp.run_item(part.astype(DT[precision]), passes, blocks, i, n, dtype=DT[precision], **sel)
            got = out[i][lines] if axis == 0 else out[i][:, lines]
            what = f"chain of {count}{' (not fused)' if not want else ''} {precision} {n}^2 axis {axis} item {i}"
            if precision == "fp32":
                b_l2, b_el = xp.bound(n, 2 * count, 0, precision)
                extra = 2 * count * FP32_FACTOR_BOUND["frugal"]
                g_l2, g_el = xp.line_errors(got, ref, axis)
                assert g_l2 <= b_l2 + extra and g_el <= b_el + extra, (what, g_l2, g_el)
                print(f"\nXPREC {what}: L2 {g_l2:.3g} element {g_el:.3g}")
            else:
                print("\nXPREC " + xp.check(got, ref, yard, axis, n, 2 * count, 2 * count, precision, what)[4])


@pytest.mark.parametrize("n,precision", [(4096, "fp64"), (2048, "fp32")])
def test_storing_builds_psf_and_power(n, precision):
    """final_intensity = 1 stores the PSF (tag bit 3) -- checked against |U_ld|^2 on sampled rows; = 2 stores the field
    and its power.  The power matches the long-double sum (Parseval: N sum |u|^2 for a sign, a phase and one forward
    transform) to 1e-14 relative (fp64).  Both items take part: a storing build needs every item in the last pass."""
    lib = _lib()
    blocks = np.zeros((3, 2, 5))
    blocks[0, :, 0] = 1.0
    blocks[1] = [[1.0, 0.0, 0.0, 0.0, 0.0], [1.0, 1.0, 0.0, 0.0, 0.0]]
    blocks[2, 0] = [1.0, 0.9, 0.0, _corner_coef(2e5, n, 0.9, 0.0, True), -1.0]
    blocks[2, 1] = [1.0, 0.5, 0.0, _corner_coef(9e10, n, 0.5, 0.0, True), 1.0]
    passes = [{"axis": 0, "fft1": 1, "pre": [(lib.PW_SIGN, 0, 0), (lib.PW_QPHASE_CENTRED, lib.PWF_MUL2PI, 2)]}]
    fields = [_field(n, 6), _field(n, 7)]
    lines = xp.sample_lines(n)
    exact = [n * np.sum(np.abs(_as_input(f, precision).astype(xp.LD)) ** 2) for f in fields]
    ptol = 1e-14 if precision == "fp64" else 1e-6
    for mode in (1, 2):
        out, tags, power = _run(lib, n, precision, fields, passes, blocks, final_intensity=mode)
        if mode == 1:
            assert tags.size == 1 and tags[0] & 8, tags
        for i in range(2):
            ref = xp.run_item(_as_input(fields[i], precision)[lines], passes, blocks, i, n, rows=lines)
            yard = xp.run_item(_as_input(fields[i], precision)[lines].astype(DT[precision]), passes, blocks, i, n,
                               rows=lines, dtype=DT[precision])
            perr = abs(float(power[i] - exact[i]) / float(exact[i]))
            assert perr <= ptol, f"final_intensity={mode} item {i}: power off by {perr:.3g} relative (> {ptol:g})"
            if mode == 1:
                psf_ref = (ref.real ** 2 + ref.imag ** 2)
                psf_yard = (np.abs(yard) ** 2)
                b_l2, b_el = xp.bound(n, 1, 1, precision)
                if precision == "fp32":
                    b_l2, b_el = (b + FP32_FACTOR_BOUND["frugal"] for b in xp.bound(n, 1, 0, precision))
                g_l2, g_el = xp.line_errors(out[i][lines], psf_ref, 0)
                y_l2, _ = xp.line_errors(psf_yard, psf_ref, 0)
                msg = (f"PSF {precision} {n}^2 item {i}: L2 {g_l2:.3g} element {g_el:.3g}; NumPy {y_l2:.3g}; "
                       f"bound {2 * b_l2:.3g} / {2 * b_el:.3g}; power {perr:.3g}")
                assert g_l2 <= 2 * b_l2 and g_el <= 2 * b_el, msg
                print("\nXPREC " + msg)
            elif precision == "fp32":
                b_l2, b_el = xp.bound(n, 1, 0, precision)
                extra = FP32_FACTOR_BOUND["frugal"]
                g_l2, g_el = xp.line_errors(out[i][lines], ref, 0)
                msg = f"field + power fp32 {n}^2 item {i}: L2 {g_l2:.3g} element {g_el:.3g} (power {perr:.3g})"
                assert g_l2 <= b_l2 + extra and g_el <= b_el + extra, msg
                print("\nXPREC " + msg)
            else:
                print("\nXPREC " + xp.check(out[i][lines], ref, yard, 0, n, 1, 1, precision,
                                            f"field + power {precision} {n}^2 item {i} (power {perr:.3g})")[4])


def _poison(f, n, lo, hi, br=8):
    """rows outside [lo, hi) stand for zeros: real zeros up to the block boundary, NaN beyond it."""
    f = f.copy()
    f[:lo] = 0
    f[hi:] = 0
    f[:(lo // br) * br] = np.nan
    f[-(-hi // br) * br:] = np.nan
    return f


def _two_axis_program(lib, n, generic=False):
    """row pass: sign, a phase across the lines, forward; column pass: a phase, inverse, scale (+ a post operator)."""
    blocks = np.zeros((6, 2, 5))
    blocks[0, :, 0] = 1.0
    blocks[1, :] = [1.0, 0.0, 0.0, 0.0, 0.0]
    blocks[2, :] = [1.0, 1.0, 0.0, 0.0, 0.0]
    blocks[3, :] = [1.0, 0.0, 0.0, 1.0 / n, 0.0]
    blocks[4, 0] = [1.0, 0.7, 0.3, _corner_coef(4e7, n, 0.7, 0.3, True), -1.0]
    blocks[4, 1] = [1.0, 0.2, 1.0, _corner_coef(2e3, n, 0.2, 1.0, True), 1.0]
    blocks[5, 0] = [1.0, 1.0, 0.5, _corner_coef(6e9, n, 1.0, 0.5, False), 1.0]
    blocks[5, 1] = [1.0, 0.4, 0.9, _corner_coef(50.0, n, 0.4, 0.9, False), -1.0]
    p1 = {"axis": 0, "fft1": 1, "pre": [(lib.PW_SIGN, 0, 0), (lib.PW_QPHASE_CENTRED, lib.PWF_MUL2PI, 4)]}
    p2 = {"axis": 1, "fft1": 2, "pre": [(lib.PW_QPHASE_NATURAL, 0, 5)], "mid": [(lib.PW_SCALE, 0, 3)]}
    if generic:
        p1 = dict(p1, post=[(lib.PW_SIGN, lib.PWF_X_ONLY, 0)])
    return [p1, p2], blocks


@pytest.mark.parametrize("generic", [False, True])
def test_pruned_windows_on_stale_rows(generic):
    """Line windows off the block-row / tile boundaries ([3, 1021) rows, [5, 517) columns), and an empty one, over a
    buffer poisoned with NaN outside (rows_stale): the stale lines are zeros to the reference.  generic=True mixes in a
    pass with a post operator: the library plans no windows then and must write the zeros itself."""
    lib = _lib()
    n, precision = 1024, "fp64"
    passes, blocks = _two_axis_program(lib, n, generic)
    for rows, cols in (([[3, 1021], [512, 512]], None), ([[3, 1021], [40, 300]], [[5, 517], [0, 1024]])):
        fields = []
        for i, (lo, hi) in enumerate(rows):
            f = _poison(_field(n, 8 + i), n, lo, hi)
            if cols is not None:
                cl, ch = cols[i]
                f[:, :(cl // 8) * 8] = np.nan
                f[:, -(-ch // 8) * 8:] = np.nan
                f[:, (cl // 8) * 8:cl] = np.where(np.isnan(f[:, (cl // 8) * 8:cl]), np.nan, 0)
                f[:, ch:-(-ch // 8) * 8] = np.where(np.isnan(f[:, ch:-(-ch // 8) * 8]), np.nan, 0)
            fields.append(f)
        kw = {"live_rows": np.array(rows, dtype=np.float64), "rows_stale": True}
        if cols is not None:
            kw["live_cols"] = np.array(cols, dtype=np.float64)
        out, tags, _ = _run(lib, n, precision, fields, passes, blocks, **kw)
        for i in range(2):
            fin = np.nan_to_num(fields[i], nan=0.0)
            ref = xp.run_item(fin, passes, blocks, i, n)
            yard = xp.run_item(fin, passes, blocks, i, n, dtype=np.complex128)
            assert np.isfinite(out[i]).all(), f"rows {rows[i]} cols {cols and cols[i]}: stale data reached the output"
            print("\nXPREC " + xp.check(out[i], ref, yard, 0, n, 2, 2, precision,
                                        f"pruned generic={generic} rows {rows[i]} cols {cols and cols[i]} item {i}")[4])


@pytest.mark.parametrize("n", [2048, 4096])
def test_single_table_pass_on_one_line_workgroups(n):
    """A single table pass whose items load AND store at most half of their positions runs on one-line workgroups
    (passes.hip: pick_build, `one_line`; frugal_launch.h: FrugalGeometry, ONE).  How this program gets there: the entry box
    (rows_stale with live_rows and live_cols, a quarter of the grid each way) makes the first pass -- along columns, its
    phases along the columns only -- work on a quarter of the lines (few enough for tables) and load a quarter of its
    positions; the second pass, along rows, carries an aperture whose bounding box spans a quarter of the rows, so the
    first pass stores only those rows.  The column pass therefore skips loads and stores (tag bits 1 and 2) and is not
    fused (different axes)."""
    lib = _lib()
    precision = "fp64"
    lo, hi, cl, ch = 3 * n // 8, 5 * n // 8, n // 4 + 3, n // 2 + 3
    blocks = np.zeros((8, 2, 5))
    blocks[0, :] = [1.0, 0.0, 0.0, 0.0, 0.0]
    blocks[1, :] = [1.0, 1.0, 0.0, 0.0, 0.0]
    blocks[2, :] = [1.0, 0.0, 0.0, 1.0 / n, 0.0]
    blocks[3, 0] = [1.0, 0.0, 0.8, _corner_coef(3e6, n, 0.0, 0.8, True), -1.0]
    blocks[3, 1] = [1.0, 0.0, 1.7, _corner_coef(5e10, n, 0.0, 1.7, True), 1.0]
    ap = [[1.0, n / 2 + 0.3, n / 2 - 0.2, n / 10, n / 9], [1.0, n / 2 - 5.5, n / 2 + 7.25, n / 7, n / 10]]
    for i in range(2):
        blocks[4, i] = ap[i][:5]
        blocks[5, i] = [0.0, 0.0, 32.0, lib.SHAPE_ELLIPSE, 0.0]
    passes = [{"axis": 1, "fft1": 0, "fft2": 1, "pre": [(lib.PW_QPHASE_CENTRED, lib.PWF_MUL2PI, 3)],
               "mid": [(lib.PW_SCALE, 0, 2)]},
              {"axis": 0, "fft1": 0, "pre": [(lib.PW_MASK, 0, 4)]}]
    fields = []
    for i in range(2):
        f = _poison(_field(n, 10 + i), n, lo, hi)
        f[lo:hi, (cl // 8) * 8:cl] = 0  # (inside the window's blocks: read, so real zeros)
        f[lo:hi, ch:-(-ch // 8) * 8] = 0
        f[:, :(cl // 8) * 8] = np.nan
        f[:, -(-ch // 8) * 8:] = np.nan
        fields.append(f)
    dev = lib.DeviceFields(n, 2, precision)
    try:
        masks = {4: [dev.aperture_mask(lib.SHAPE_ELLIPSE, ap[i] + [0.0, 0.0, 32.0]) for i in range(2)]}
    finally:
        dev.close()
    out, tags, _ = _run(lib, n, precision, fields, passes, blocks, live_rows=np.array([[lo, hi]] * 2, dtype=np.float64),
                        rows_stale=True, live_cols=np.array([[cl, ch]] * 2, dtype=np.float64))
    assert tags.size == 2 and (tags[0] & 6) == 6 and not np.any(tags & 48), tags
    del fields
    for i in range(2):
        fin = np.nan_to_num(_poison(_field(n, 10 + i), n, lo, hi), nan=0.0)
        fin[:, :cl] = 0
        fin[:, ch:] = 0
        # the column pass on the live columns, then the row pass on the rows the aperture leaves non-zero
        live = np.arange((cl // 8) * 8, -(-ch // 8) * 8)
        mid = xp.run_item(fin[:, live], passes[:1], blocks, i, n, cols=live)
        rws = np.nonzero(masks[4][i].any(axis=1))[0]
        u = np.zeros((rws.size, n), dtype=xp.LD)
        u[:, live] = mid[rws]
        ref = xp.run_item(u, passes[1:], blocks, i, n, rows=rws, masks=masks)
        umid = np.zeros((rws.size, n), dtype=np.complex128)
        umid[:, live] = xp.run_item(fin[:, live], passes[:1], blocks, i, n, cols=live, dtype=np.complex128)[rws]
        yard = xp.run_item(umid, passes[1:], blocks, i, n, rows=rws, masks=masks, dtype=np.complex128)
        others = np.setdiff1d(np.arange(n), rws)
        assert not np.any(out[i][others]), "rows the aperture zeroes"
        print("\nXPREC " + xp.check(out[i][rws], ref, yard, 0, n, 3, 1, precision, f"one-line table pass {n}^2 item {i}")[4])
