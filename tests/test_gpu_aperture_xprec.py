"""Aperture weights on every device path against exact pixel areas (tests/aperture_xprec.py: mpmath at 50 digits).

(a) Truth enters at the render path: ``DeviceFields.aperture_mask`` (aperture_kernel's render form) against the
    arbitrary-precision areas under ``bound(a, b) = C_AP 2^-53 max(a, b, 1)``, pixels farther than 1e-9 px from the
    boundary exactly 0 or 1; rectangles against the restated sub-sample count, exactly.
(b) Every other path hands out the render path's weights bit for bit: paos_aperture, the four start paths, the generic
    pass's PAOS_PW_MASK in its three slots, and the line records of the production (frugal) pass kernels -- five shape
    families, both axes, mask in front of the transform, behind a disabled one, behind a running one, and in the second
    pass of a fused launch; every record renderer; pruning on and off.  Weights are read out exactly with the field
    1 + 0.5j (w + 0.5 w j without rounding; in fp32 contexts float32(w), whichever of product and weight is rounded),
    and one random field per precision checks the exact host expectation of each path: T(double(u) w) for the
    stand-alone and the generic kernels, float32(u) float32(w) for the fp32 record consumer.

Behind a running transform the field is the unit impulse: the same program with the mask operator disabled must store
the constant 1 + 0.5j bit for bit (asserted), so the masked store is the weights again, in the consumer's
post-transform position order.

Obscurations: the render path returns the mask alone, so (a) never sees one; an obscuration's weight is 1 - mask, formed
here with the kernels' one rounding (ApertureEval::weight), and enters in (b).  Pruning off is switched through the
context (``DeviceFields.set_pruning``), not with PAOS_NO_PRUNE=1, which the library reads once per process: a pass
program prunes when both allow it (passes.hip: ``use_pruning() && c->prune``), so the effect is the same.

Every assertion message of (a) carries the kernel's error, the bound and what the fp64 NumPy restatement of the
reference's rule (oracle/aperture_np.py) reaches on the same case.  Everything goes through the C ABI."""
import os

import numpy as np
import pytest

import aperture_mask_worker
import aperture_xprec as ax
from test_aperture_restatements import RECTS

pytestmark = pytest.mark.gpu

# Largest kernel error observed on an MI355X over this module, as a fraction of the bound of its case (C_AP = 8): the
# render path over every ellipse, and the field of a start with stop (bound + 4 2^-53 relative).
# test_zzz_report_observed prints this run's values.
OBSERVED_MI355X = {"render": 0.343, "start_with_stop": 0.341}
OBSERVED = {"render": None, "start_with_stop": None}

N = ax.N_TABLE
VALUE = 1.0 + 0.5j
SENTINEL = 7.0 + 9.0j  # what a start that writes a box only must leave alone
DT = {"fp64": np.complex128, "fp32": np.complex64}
_W = {}


def setup_module():
    ax.require_mpmath()


def _lib():
    from paos_amd import _lib as lib

    return lib


def _note(kind, ratio):
    OBSERVED[kind] = ratio if OBSERVED[kind] is None else max(OBSERVED[kind], ratio)


def _ell(xc, yc, a, b, theta=0.0, obsc=0.0, enable=1.0):
    return [enable, xc, yc, a, b, theta, obsc, 0.0]


def _rect(xc, yc, w, h, theta=0.0, obsc=0.0, subpix=32, enable=1.0):
    return [enable, xc, yc, w, h, theta, obsc, float(subpix)]


def _weights(dev, shape, block):
    """The render path's weight map of an 8-double aperture record: the mask, or 1 - mask for an obscuration (one
    rounding, the kernels': ApertureEval::weight).  Kept per (n, record)."""
    key = (dev.n, shape, tuple(block[1:]))
    if key not in _W:
        if len(_W) > 24:
            _W.clear()
        m = dev.aperture_mask(shape, [1.0] + list(block[1:]))
        _W[key] = (1.0 - m) if block[6] != 0.0 else m
    return _W[key]


def _times(u, w, precision):
    """T(double(u) w): what the stand-alone and the generic kernels store for a field value u already of type T."""
    u = np.asarray(u, dtype=np.complex128)
    out = u.real * w + 1j * (u.imag * w)
    return out.astype(DT[precision]).astype(np.complex128)


def _times_frugal(u, w, precision):
    """What the record consumer stores (frugal_pass.h: frugal_slot): fl(u w) in fp64, float32(u) float32(w) in fp32."""
    if precision == "fp64":
        return _times(u, w, precision)
    u = np.asarray(u, dtype=np.complex128)
    wf = np.asarray(w, dtype=np.float64).astype(np.float32)
    re, im = u.real.astype(np.float32) * wf, u.imag.astype(np.float32) * wf
    return re.astype(np.float64) + 1j * im.astype(np.float64)


def _stored(u, precision):
    return np.asarray(u).astype(DT[precision]).astype(np.complex128)


def _same(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        r, c = bad[0]
        raise AssertionError(f"{what}: {len(bad)} pixels differ, first at row {r} column {c}: got {got[r, c]!r}, want {want[r, c]!r}")


# ---- (a) the render path against exact areas --------------------------------------------------------------------------
def _check_render(got, n, xc, yc, a, b, th, what):
    from oracle.aperture_np import ellipse_mask

    _, _, sure0, sure1 = ax.ellipse_weights(n, xc, yc, a, b, th)
    err = float(ax.ellipse_errors(got, n, xc, yc, a, b, th).max())
    oracle = ellipse_mask((n, n), xc, yc, a, b, th)
    yard = float(ax.ellipse_errors(oracle, n, xc, yc, a, b, th).max())
    bnd = ax.bound(a, b)
    msg = f"{what}: weight error {err:.3g}, bound {bnd:.3g}, fp64 NumPy restatement {yard:.3g}"
    assert bnd >= 2.0 * yard, "bound tighter than twice the yardstick -- " + msg
    assert np.all(got[sure0] == 0.0), "a pixel 1e-9 px outside the ellipse is not exactly 0 -- " + msg
    assert np.all(got[sure1] == 1.0), "a pixel 1e-9 px inside the ellipse is not exactly 1 -- " + msg
    assert got.min() >= 0.0 and got.max() <= 1.0, "a weight outside [0, 1] -- " + msg
    if th == 0.0:
        # A pixel whose four corners pass x^2 + y^2 <= 1.0 -- in the kernel's own roundings; cos 0 = 1 and sin 0 = 0, so no
        # device function is involved -- is exactly 1: the rule's definition of an interior pixel.  The Pythagorean circles
        # put pixel corners ON the boundary: there a `<` for the `<=` turns 16 (r = 25) and 20 (r = 65) of these pixels into
        # 1 - 2e-15, far inside the bound.  (Which boundary pixels come out as exactly 0 or are clamped to 1 depends on
        # atan2's last bit and is not asserted: r = 65 has eight exterior pixels that touch the circle with a corner, where
        # NumPy leaves 7e-15 and the device 0.)
        k = np.arange(n, dtype=np.float64)
        qx0, qx1 = (((k - 0.5) - xc) / a) ** 2, (((k + 0.5) - xc) / a) ** 2
        qy0, qy1 = (((k - 0.5) - yc) / b) ** 2, (((k + 0.5) - yc) / b) ** 2
        all_in = np.ones((n, n), dtype=bool)
        for qy in (qy0, qy1):
            for qx in (qx0, qx1):
                all_in &= (qx[None, :] + qy[:, None]) <= 1.0
        assert np.all(got[all_in] == 1.0), "a pixel with its four corners inside or on the ellipse is not exactly 1 -- " + msg
    _note("render", err / bnd)
    print(msg)
    assert err <= bnd, msg


RENDER_ELLIPSES = {**{k: (N, *v, 0.0) for k, v in ax.ELLIPSES.items()}, **{k: (N, *v) for k, v in ax.TILTED.items()},
                   "production: 4096, 512 circle": (*ax.PRODUCTION["4096: 512 x 512 centred"], 0.0)}


@pytest.mark.parametrize("name", list(RENDER_ELLIPSES))
def test_render_ellipse_against_exact_areas(name):
    n, xc, yc, a, b, th = RENDER_ELLIPSES[name]
    dev = _lib().DeviceFields(n, 1)
    try:
        got = dev.aperture_mask(_lib().SHAPE_ELLIPSE, _ell(xc, yc, a, b, th))
    finally:
        dev.close()
    _check_render(got, n, xc, yc, a, b, th, name)


# (xc, yc, w, h, theta, subpixels) on the N grid: the RECTS table of tests/test_aperture_restatements.py, other sub-sample
# counts, a rectangle over the far grid corner, and theta = 1e-300 (sin = 1e-300, cos = 1: the 2-D loop on the theta = 0 samples)
RENDER_RECTS = [(*r[1:], 32) for r in RECTS] + [
    (20.3, 19.1, 11.7, 4.2, 0.0, 1), (20.0, 20.0, 10.5, 6.25, 0.0, 4), (20.3, 19.1, 11.7, 4.2, 0.6, 4),
    (250.3, 253.9, 30.5, 9.25, 0.0, 32), (120.3, 131.1, 80.7, 33.2, 1e-300, 32), (127.6, 130.2, 50.5, 21.25, 0.3, 32),
]


@pytest.mark.parametrize("xc,yc,w,h,th,S", RENDER_RECTS)
def test_render_rectangle_is_the_sub_sample_count(xc, yc, w, h, th, S):
    want, margin = ax.rectangle_weights(N, xc, yc, w, h, th, S)
    if th != 0.0:  # (no sample close enough to an edge for the device's own sin / cos to move it across)
        assert margin >= 1e-9, margin
    dev = _lib().DeviceFields(N, 1)
    try:
        got = dev.aperture_mask(_lib().SHAPE_RECT, _rect(xc, yc, w, h, th, 0.0, S))
    finally:
        dev.close()
    _same(got, want, f"rectangle {(xc, yc, w, h, th, S)} (sample margin {margin:.3g})")
    if th == 1e-300:
        _same(got, ax.rectangle_weights(N, xc, yc, w, h, 0.0, S)[0], "theta = 1e-300 against theta = 0")


# ---- (b) paos_aperture ----------------------------------------------------------------------------------------------
def _aperture_batches():
    e, t = ax.ELLIPSES, ax.TILTED
    lib = _lib()
    ell = [[_ell(*e["generic decentred"], 0.0, 1.0), _ell(*e["pythagorean r=25"]), _ell(*e["straddles one edge"], enable=0.0),
            _ell(*e["pythagorean r=25"])],
           [_ell(*t["tilted 0.6"]), _ell(*e["sub-pixel across a boundary"], 0.0, 1.0), _ell(*e["centre on -0.5"]),
            _ell(*e["1100 x 40 flat"])],
           [_ell(*e["straddles one edge"], 0.0, 1.0), _ell(*e["sub-pixel on a corner"]), _ell(*e["straddles a corner"]),
            _ell(*e["pythagorean r=25"], 0.0, 1.0)],
           [_ell(*e[name], 0.0, 1.0) for name in ax.OBSCURED]]
    rect = [[_rect(*RECTS[0][1:]), _rect(*RECTS[7][1:], obsc=1.0), _rect(*RECTS[4][1:], enable=0.0), _rect(*RECTS[0][1:])],
            [_rect(*RECTS[1][1:], obsc=1.0), _rect(*RECTS[5][1:]), _rect(20.3, 19.1, 11.7, 4.2, 0.0, 0.0, 4), _rect(*RECTS[8][1:])]]
    return [(lib.SHAPE_ELLIPSE, b) for b in ell] + [(lib.SHAPE_RECT, b) for b in rect]


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_paos_aperture_applies_the_rendered_weights(precision):
    """Batches of four with a geometry per item, one item disabled (untouched bit for bit) and one a duplicate of
    another: the constant 1 + 0.5j turns into w + 0.5 w j, a random field into T(double(u) w)."""
    rng = np.random.default_rng(5)
    u = [rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N)) for _ in range(4)]
    dev = _lib().DeviceFields(N, 4, precision)
    try:
        for shape, blocks in _aperture_batches():
            ws = [_weights(dev, shape, b) for b in blocks]
            dev.fill(VALUE)
            dev.aperture(shape, blocks)
            for i, (b, w) in enumerate(zip(blocks, ws)):
                want = _times(np.full((N, N), VALUE), w, precision) if b[0] != 0.0 else np.full((N, N), VALUE)
                _same(dev.download(i), want, f"paos_aperture {precision} shape {shape} item {i} {b}")
            for i in range(4):
                dev.upload(i, u[i])
            dev.aperture(shape, blocks)
            for i, (b, w) in enumerate(zip(blocks, ws)):
                want = _times(_stored(u[i], precision), w, precision) if b[0] != 0.0 else _stored(u[i], precision)
                _same(dev.download(i), want, f"paos_aperture {precision} shape {shape} item {i} {b}, random field")
    finally:
        dev.close()


# ---- (b) the start paths --------------------------------------------------------------------------------------------
def _planned_box(shape, blocks, n):
    """The rows and columns the host would have the start write (run.py: _start_field): rows, cols per item, or None
    where the walk would write whole fields."""
    from paos_amd import run as prun

    plans = prun._Plans({"stop": False, "zernike": None, "phase_map": None} for _ in blocks)
    plans.ap = prun._SurfaceApertures.from_blocks(shape, blocks)
    rows = [[0, n] for _ in plans]
    prun._live_rows_after(plans, rows, n)
    if not (all(r[0] > 0 or r[1] < n for r in rows) and all(r[0] < r[1] for r in rows)):
        return None, None
    return rows, prun._live_cols_of(plans, n)


def _zernike_nothing(batch):
    """A Zernike surface with all-zero coefficients on a two-pixel disk at the grid centre: exp(i 0) = 1 exactly."""
    from paos_amd.planner import jacobi_recurrence, zernike_block
    from paos_amd.zernike import zernike_tables

    m, n, norm = zernike_tables(6, "noll", True)
    blk, nmax, kdim = zernike_block(m, n, norm, np.zeros(6), 1.0, 1.0, 2.0, 1.0e-6, nmax=int(n.max()))
    return nmax, kdim, jacobi_recurrence(nmax), np.array([blk] * batch)


def _start_pairs():
    lib = _lib()
    names = list(ax.ELLIPSES)
    ell = [[_ell(*ax.ELLIPSES[a]), _ell(*ax.ELLIPSES[b])] for a, b in zip(names, names[1:] + names[:1])]
    flat = [r for r in RECTS if r[5] == 0.0]
    rect = [[_rect(*a[1:]), _rect(*b[1:])] for a, b in zip(flat, flat[1:] + flat[:1])]
    return [(lib.SHAPE_ELLIPSE, p) for p in ell] + [(lib.SHAPE_RECT, p) for p in rect]


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_start_paths_write_the_rendered_weights_inside_the_planned_box(precision):
    """paos_start without stop, paos_start_rows / paos_start_box with the box the host plans, paos_start_zernike_box with
    all-zero coefficients -- two items with different geometries per call, every theta = 0 clear aperture of the tables.
    Inside the planned box the field is value w bit for bit; whatever was not written has weight 0; and no pixel with
    w != 0 lies outside the planned box: the agreement of host and device on the bounding box that the start box rests
    on, at centres on half-integers, extents on pixel boundaries and apertures across the grid's edges."""
    full = np.full((N, N), VALUE)
    boxes = fused = 0
    dev = _lib().DeviceFields(N, 2, precision)
    try:
        nmax, kdim, table, zblocks = _zernike_nothing(2)
        for shape, blocks in _start_pairs():
            ws = [_weights(dev, shape, b) for b in blocks]
            want = [_times(full, w, precision) for w in ws]
            rows, cols = _planned_box(shape, blocks, N)
            # (name, the call's window arguments -- None: the fused call --, the rows and columns that must be written)
            paths = [("start", {}, [(0, N)] * 2, [(0, N)] * 2)]
            if rows is not None:
                paths.append(("rows", dict(write_rows=rows), rows, [(0, N)] * 2))
                for (rl, rh), w in zip(rows, ws):
                    assert not w[:rl].any() and not w[rh:].any(), f"weight outside the planned rows {rows} of {blocks}"
            if rows is not None and cols is not None:
                boxes += 1
                paths.append(("box", dict(write_rows=rows, write_cols=cols), rows, cols))
                for (cl, ch), w in zip(cols, ws):
                    assert not w[:, :cl].any() and not w[:, ch:].any(), f"weight outside the planned columns {cols} of {blocks}"
                # (the walk lets a Zernike surface ride only when its disk lies inside the box: run.py, _zernike_rides)
                if all(c[0] <= N // 2 - 2 and N // 2 + 2 <= c[1] - 1 and r[0] <= N // 2 - 2 and N // 2 + 2 <= r[1] - 1
                       for r, c in zip(rows, cols)):
                    fused += 1
                    paths.append(("zernike box", None, rows, cols))
            for name, kw, prows, pcols in paths:
                for i in range(2):
                    dev.upload(i, np.full((N, N), SENTINEL))
                if kw is None:
                    dev.start_zernike(VALUE, shape, blocks, None, rows, cols, nmax, kdim, table, zblocks)
                else:
                    dev.start(VALUE, shape, blocks, None, **kw)
                for i in range(2):
                    got = dev.download(i)
                    written = got != SENTINEL
                    what = f"{name} {precision} shape {shape} item {i} of {blocks}"
                    (rl, rh), (cl, ch) = prows[i], pcols[i]
                    assert written[rl:rh, cl:ch].all(), f"{what}: the planned box is not written"
                    assert not ws[i][~written].any(), f"{what}: a pixel with weight was not written"
                    _same(got[written], want[i][written], what)
        assert boxes >= 16 and fused >= 4, (boxes, fused)
    finally:
        dev.close()


STOP_CASES = ["generic decentred", "pythagorean r=25", "straddles one edge", "sub-pixel across a boundary",
              "extents on pixel boundaries", "1100 x 40 flat"]


def test_start_with_stop_against_exact_areas():
    """ones -> aperture -> make_stop in one write (start_power_kernel + start_write_kernel), fp64: the power against the
    long-double sum of |value w_ref|^2 to 1e-13, the field against value w_ref / sqrt(power_ref) under
    (bound + 4 2^-53 w) |value| / sqrt(power): the weight's bound, and four roundings (1 / sqrt twice, the two products)."""
    from oracle.aperture_np import ellipse_mask

    dev = _lib().DeviceFields(N, 2)
    try:
        for name in STOP_CASES:
            xc, yc, a, b = ax.ELLIPSES[name]
            w, lo, _, sure1 = ax.ellipse_weights(N, xc, yc, a, b, 0.0)
            wl = w.astype(np.longdouble) + lo.astype(np.longdouble)
            v2 = np.longdouble(abs(VALUE) ** 2)
            power = np.sum(wl * wl) * v2
            blocks = [_ell(xc, yc, a, b), _ell(xc, yc, a, b, 0.0, 1.0)]  # (item 1: the obscuration, weight 1 - mask)
            dev.start(VALUE, _lib().SHAPE_ELLIPSE, blocks, [1.0, 0.0])
            got = dev.download(0)
            assert dev.norm2()[0] == pytest.approx(1.0, abs=1e-13)
            # The power the kernel divided by, from the pixel of the largest weight: it holds fl(fl(value w) / sqrt(power))
            # with w the render path's weight, which the start writes bit for bit (the test above) -- 1 wherever the
            # ellipse has an interior pixel; a sub-pixel ellipse has partial pixels only, and its w enters exactly too.
            wdev = _weights(dev, _lib().SHAPE_ELLIPSE, blocks[0])
            r, c = np.unravel_index(np.argmax(wdev), wdev.shape)
            assert (wdev[r, c] == 1.0) == bool(sure1.any())
            dev_power = float(v2) * wdev[r, c] ** 2 / abs(got[r, c]) ** 2
            rel = abs(dev_power / float(power) - 1.0)
            print(f"start with stop, {name}: power {dev_power!r} from a pixel of weight {wdev[r, c]!r}, relative error {rel:.3g}")
            assert rel < 1e-13, (name, dev_power, float(power))
            s = 1.0 / np.sqrt(power)
            want_re, want_im = np.longdouble(VALUE.real) * wl * s, np.longdouble(VALUE.imag) * wl * s
            err = np.hypot(got.real.astype(np.longdouble) - want_re, got.imag.astype(np.longdouble) - want_im)
            bnd = (ax.bound(a, b) + 4.0 * ax.U64 * w) * float(s) * abs(VALUE)
            yard_w = float(ax.ellipse_errors(ellipse_mask((N, N), xc, yc, a, b, 0.0), N, xc, yc, a, b).max())
            worst = float(np.max(err.astype(np.float64) / bnd))
            msg = (f"start with stop, {name}: field error {float(err.max()):.3g} is {worst:.3g} of its bound "
                   f"(largest bound {float(bnd.max()):.3g}); fp64 NumPy restatement of the weight {yard_w:.3g} of {ax.bound(a, b):.3g}")
            assert ax.bound(a, b) >= 2.0 * yard_w, msg
            _note("start_with_stop", worst)
            print(msg)
            assert worst <= 1.0, msg
            # ... and the item without stop, an obscuration, is value (1 - mask) with the render path's bits
            _same(dev.download(1), _times(np.full((N, N), VALUE), _weights(dev, _lib().SHAPE_ELLIPSE, blocks[1]), "fp64"),
                  f"start, obscuration item next to a stopped one, {name}")
    finally:
        dev.close()


# ---- (b) PAOS_PW_MASK on the pass kernels ---------------------------------------------------------------------------
ON, OFF, SCALE1 = 2, 3, 4  # block sets behind the aperture's two: transform on (forward) / off, and a scale by 1


def _pass_blocks(shape_blocks, mask_on=True):
    """[5][batch][5]: the aperture's two block sets, a forward transform's control block, a disabled one's, a scale of 1."""
    nb = len(shape_blocks)
    out = np.zeros((5, nb, 5))
    for i, (shape, b) in enumerate(shape_blocks):
        out[0, i] = [b[0] if mask_on else 0.0, b[1], b[2], b[3], b[4]]
        out[1, i] = [b[5], b[6], b[7], float(shape), 0.0]
        out[ON, i] = [1.0, 0.0, 0.0, 0.0, 0.0]
        out[SCALE1, i] = [1.0, 0.0, 0.0, 1.0, 0.0]
    return out


def _mask_pass(axis, slot, fft):
    p = {"axis": axis, "fft1": fft, "fft2": -1, "pre": [], "mid": [], "post": []}
    p[slot] = [(_lib().PW_MASK, 0, 0)]
    return p


def _generic_sets():
    lib = _lib()
    e = ax.ELLIPSES
    E, R = lib.SHAPE_ELLIPSE, lib.SHAPE_RECT
    return [[(E, _ell(*e["generic decentred"])), (R, _rect(*RECTS[0][1:])), (E, _ell(*ax.TILTED["tilted 0.6"])),
             (E, _ell(*e["pythagorean r=25"], 0.0, 1.0))],
            [(E, _ell(*e["straddles one edge"])), (R, _rect(*RECTS[7][1:], obsc=1.0)), (E, _ell(*e["sub-pixel across a boundary"])),
             (E, _ell(*e["1100 x 40 flat"]))]]


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_generic_pass_mask_in_every_slot(precision):
    """n = 256 runs on the generic pass kernel, whose PAOS_PW_MASK multiplies by a weight map that aperture_kernel renders
    (weights_out form) right before the pass: pre, mid and post slot, rows and columns, the transform disabled through
    its control block for an exact read-out; a random field in the pre slot."""
    rng = np.random.default_rng(11)
    u = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))
    full = np.full((N, N), VALUE)
    dev = _lib().DeviceFields(N, 4, precision)
    try:
        for items in _generic_sets():
            ws = [_weights(dev, s, b) for s, b in items]
            blocks = _pass_blocks(items)
            for axis in (0, 1):
                for slot in ("pre", "mid", "post"):
                    dev.fill(VALUE)
                    dev.run_passes([_mask_pass(axis, slot, OFF)], blocks)
                    for i, w in enumerate(ws):
                        _same(dev.download(i), _times(full, w, precision), f"generic {precision} axis {axis} {slot} item {i} {items[i]}")
                for i in range(4):
                    dev.upload(i, u)
                dev.run_passes([_mask_pass(axis, "pre", OFF)], blocks)
                for i, w in enumerate(ws):
                    _same(dev.download(i), _times(_stored(u, precision), w, precision),
                          f"generic {precision} axis {axis} item {i} {items[i]}, random field")
    finally:
        dev.close()


def test_generic_pass_takes_what_the_records_cannot_hold():
    """At 1024^2 the production kernels take a riding aperture as line records -- unless it is thinner than two pixels
    across the lines, tilted, or a rectangular obscuration: those passes run on the generic kernel (pass_program.h:
    lower_frugal), as does every pass with an operator in its post slot -- with the same weights."""
    n = 1024
    lib = _lib()
    E, R = lib.SHAPE_ELLIPSE, lib.SHAPE_RECT
    sets = [[(E, _ell(512.3, 511.1, 60.0, 1.5)), (E, _ell(512.0, 512.0, 1.5, 60.0))],
            [(E, _ell(500.3, 520.9, 90.7, 40.2, 0.6)), (E, _ell(512.0, 512.0, 40.0, 40.0))],
            [(R, _rect(512.3, 511.1, 300.7, 100.2, 0.0, 1.0)), (R, _rect(512.0, 512.0, 100.5, 60.25))]]
    full = np.full((n, n), VALUE)
    dev = lib.DeviceFields(n, 2)
    try:
        for items in sets:
            ws = [_weights(dev, s, b) for s, b in items]
            blocks = _pass_blocks(items)
            rendered = dev.record_set_stats()[1]
            for axis in (0, 1):
                for slot in ("pre", "mid", "post"):
                    dev.fill(VALUE)
                    dev.run_passes([_mask_pass(axis, slot, OFF)], blocks)
                    for i, w in enumerate(ws):
                        _same(dev.download(i), _times(full, w, "fp64"), f"1024 axis {axis} {slot} item {i} {items[i]}")
            assert dev.record_set_stats()[1] == rendered, "these passes were expected on the generic kernel (no line records)"
    finally:
        dev.close()


def test_generic_pass_at_1024_with_the_production_kernels_switched_off():
    """PAOS_NO_FRUGAL=1 keeps every pass on the generic kernel; the library reads the switch once per process, so the
    check runs in a process of its own (aperture_mask_worker.no_frugal_worker), forked from the server conftest.py
    started before this process touched the GPU: pre, mid and post slot, both axes, two batches of four = 12 passes."""
    import multiprocessing as mp

    ctx = mp.get_context("forkserver")
    out = ctx.Queue()
    proc = ctx.Process(target=aperture_mask_worker.no_frugal_worker, args=(out,))
    proc.start()
    try:
        status, detail = out.get(timeout=120)
        proc.join(timeout=60)
    finally:
        if proc.is_alive():  # (a worker that hangs must not stay behind with the GPU open)
            proc.kill()
            proc.join(timeout=30)
    assert proc.exitcode == 0
    assert status == "ok" and detail == 12, (status, detail)


# ---- (b) the line records of the production kernels -----------------------------------------------------------------
FAMILIES = [(1024, "fp64"), (2048, "fp64"), (4096, "fp64"), (2048, "fp32"), (4096, "fp32")]


def _frugal_items(n, axis):
    """The riding geometries of aperture_xprec.frugal_ellipses plus two rectangles (whose line factor and record must
    multiply to the stand-alone count exactly), as (shape, record)."""
    lib = _lib()
    items = [(lib.SHAPE_ELLIPSE, _ell(xc, yc, a, b, 0.0, o)) for xc, yc, a, b, o in ax.frugal_ellipses(n, axis)]
    h = n / 2.0
    items.append((lib.SHAPE_RECT, _rect(h + 0.3, h - 0.9, 300.7, 100.2)))
    items.append((lib.SHAPE_RECT, _rect(10.0, h + 17.3, 60.5, 200.25)))
    return items


def _check_riding_render(dev, items):
    """Truth for the riding ellipses too: the render path at this size against the exact areas."""
    for shape, b in items:
        if shape == _lib().SHAPE_ELLIPSE:
            m = dev.aperture_mask(shape, [1.0] + list(b[1:6]) + [0.0, 0.0])
            _check_render(m, dev.n, b[1], b[2], b[3], b[4], 0.0, f"riding ellipse {b[1:5]} at {dev.n}")


def _fused(tags):
    return bool(np.any(tags & 48))


def _riding_sets(n, axis, batch):
    """Every riding geometry (eight ellipses, two rectangles) in batches of ``batch``, ellipses and rectangles mixed."""
    items = _frugal_items(n, axis)
    order = [1, 2, 0, 3, 5, 8, 7, 9, 4, 6]  # (the two longest tip runs first)
    padded = order + order[:(-len(order)) % batch]
    return [[items[i] for i in padded[k:k + batch]] for k in range(0, len(padded), batch)]


@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("n,precision", FAMILIES)
def test_line_records_hand_out_the_rendered_weights(n, precision, axis):
    """One shape family of the production pass kernels (frugal_pass.h: frugal_slot) and one axis, every riding geometry
    (batches of four at 1024^2, of two above).  The mask in the slot in front of the transform and in the one behind
    it, the transform disabled: the constant field comes back as the render path's weights bit for bit.  The record
    statistics show that the pass read line records: the pre-slot pass renders the new geometry, the mid-slot pass
    finds that set.  The first batch again with the pruning off (the context's switch)."""
    lib = _lib()
    batch = 4 if n == 1024 else 2
    full = np.full((n, n), VALUE)
    dev = lib.DeviceFields(n, batch, precision)
    try:
        for k, items in enumerate(_riding_sets(n, axis, batch)):
            if precision == "fp64" and (n < 4096 or k == 0):  # (4096^2: the first batch, for the test's duration)
                _check_riding_render(dev, items)
            ws = [_weights(dev, s, b) for s, b in items]
            blocks = _pass_blocks(items)
            for slot, prune in (("pre", True), ("mid", True)) + ((("mid", False), ("pre", False)) if k == 0 else ()):
                dev.set_pruning(prune)
                found, rendered = dev.record_set_stats()
                dev.fill(VALUE)
                dev.run_passes([_mask_pass(axis, slot, OFF)], blocks)
                found2, rendered2 = dev.record_set_stats()
                what = f"{n} {precision} axis {axis} {slot}, transform off, pruning {prune}"
                if prune:
                    assert (found2, rendered2) == ((found, rendered + 1) if slot == "pre" else (found + 1, rendered)), \
                        f"{what}: the pass did not {'render' if slot == 'pre' else 'find'} line records: {(found, rendered)} -> {(found2, rendered2)}"
                else:  # (found, or rendered again for all lines where the kept set covers the live ones only)
                    assert found2 + rendered2 == found + rendered + 1, f"{what}: the pass read no line records"
                for i, w in enumerate(ws):
                    _same(dev.download(i), _times_frugal(full, w, precision), f"{what}, item {i} {items[i]}")
            dev.set_pruning(True)
    finally:
        dev.close()


@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("n,precision", FAMILIES)
def test_line_records_behind_a_running_transform_and_in_a_fused_launch(n, precision, axis):
    """The production case: the mask in the slot behind a RUNNING forward transform, and the same in the second pass of a
    two-pass chain that the library runs in one launch (asserted from the launch profile; the single pass is asserted
    to be one unfused launch).  The field is the unit impulse, 1 + 0.5j at position 0 of every line.  Its unscaled
    transform is the constant 1 + 0.5j bit for bit in all five families on the MI355X, which the test asserts on the store of the same program with the mask operator
    disabled -- so no case needs tests/test_gpu_xprec.py's transform bound -- and the masked store is then the render
    path's weights in the consumer's post-transform position order.  Two batches: the two longest tip runs (four
    ellipses at 1024^2), and the obscuration with a rectangle (at 1024^2 also the centre shifts 31.9 and 63.5)."""
    lib = _lib()
    batch = 4 if n == 1024 else 2
    items_all = _frugal_items(n, axis)
    sets = [[items_all[i] for i in ((1, 2, 0, 5) if batch == 4 else (1, 2))], [items_all[i] for i in ((7, 8, 3, 4) if batch == 4 else (7, 8))]]
    constant = np.full((n, n), VALUE)
    impulse = np.zeros((n, n), dtype=np.complex128)
    if axis == 0:
        impulse[:, 0] = VALUE
    else:
        impulse[0, :] = VALUE
    chain = [{"axis": axis, "fft1": OFF, "fft2": OFF, "pre": [(lib.PW_SCALE, 0, SCALE1)], "mid": [], "post": []}, _mask_pass(axis, "mid", ON)]
    dev = lib.DeviceFields(n, batch, precision)
    try:
        for items in sets:
            ws = [_weights(dev, s, b) for s, b in items]
            for what, program in (("behind a running transform", [_mask_pass(axis, "mid", ON)]), ("second pass of a fused launch", chain)):
                for mask_on in (False, True):
                    for i in range(batch):
                        dev.upload(i, impulse)
                    found, rendered = dev.record_set_stats()
                    dev.profile_begin(lib.KERNEL_PASS_ANY, max_launches=16)
                    dev.run_passes(program, _pass_blocks(items, mask_on))
                    _, tags = dev.profile_end_launches()
                    where = f"{n} {precision} axis {axis}, {what}, mask {'on' if mask_on else 'off'}"
                    assert tags.size == 1 and _fused(tags) == (len(program) == 2), f"{where}: not one {'fused' if len(program) == 2 else 'single'} launch (tags {tags})"
                    found2, rendered2 = dev.record_set_stats()
                    assert not mask_on or found2 + rendered2 == found + rendered + 1, f"{where}: the pass read no line records"
                    for i, w in enumerate(ws):
                        _same(dev.download(i), _times_frugal(constant, w, precision) if mask_on else constant, f"{where}, item {i} {items[i]}")
    finally:
        dev.close()


@pytest.mark.parametrize("n,precision", [(2048, "fp64"), (2048, "fp32")])
def test_line_records_on_a_random_field(n, precision):
    """The exact host expectation of the record consumer on a random field: fl(u w) in fp64; float32(u) float32(w) in fp32
    (it rounds the weight, where the stand-alone kernel rounds the product)."""
    rng = np.random.default_rng(n)
    u = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    dev = _lib().DeviceFields(n, 2, precision)
    try:
        for axis in (0, 1):
            items = _frugal_items(n, axis)[2:4]
            ws = [_weights(dev, s, b) for s, b in items]
            for i in range(2):
                dev.upload(i, u)
            dev.run_passes([_mask_pass(axis, "pre", OFF)], _pass_blocks(items))
            for i, w in enumerate(ws):
                _same(dev.download(i), _times_frugal(_stored(u, precision), w, precision), f"{n} {precision} axis {axis} item {i}, random field")
    finally:
        dev.close()


MODES = [("default", {}), ("pairs", {"PAOS_MASK_PAIRS": "1"}), ("lines", {"PAOS_MASK_PAIRS": "0"}), ("scan", {"PAOS_MASK_SCAN": "1"}),
         ("rect lines", {"PAOS_MASK_RECT_BLOCKS": "0"})]


@pytest.mark.parametrize("mode,env", MODES)
def test_every_record_renderer_and_pruning(mode, env):
    """mask_lines_kernel's renderers -- four, two or one line per wave through boundary windows, the chunk scan, rectangles
    by blocks of lines or line by line -- each forced through its switch (read per call), at 1024^2 on every riding
    geometry and both axes: the render path's weights bit for bit, with the dead-line pruning on and off (the context's
    switch, see the module's docstring); the context
    keys its kept record sets by the mode, and `rendered` shows that every geometry was rendered in this mode."""
    n, batch = 1024, 4
    full = np.full((n, n), VALUE)
    for name in env:
        assert os.environ.get(name) is None
    dev = _lib().DeviceFields(n, batch)
    os.environ.update(env)
    try:
        for axis in (0, 1):
            items_all = _frugal_items(n, axis)
            for k in range(0, len(items_all) - batch + 1, 3):
                items = items_all[k:k + batch]
                ws = [_weights(dev, s, b) for s, b in items]
                blocks = _pass_blocks(items)
                for prune in (True, False):
                    dev.set_pruning(prune)
                    found, rendered = dev.record_set_stats()
                    dev.fill(VALUE)
                    dev.run_passes([_mask_pass(axis, "pre", OFF)], blocks)
                    # (a new geometry is rendered; with the pruning off the set is found again -- or, where it was rendered
                    # for the live lines only and this pass reads all lines, rendered once more: passes.hip, run_passes_impl)
                    found2, rendered2 = dev.record_set_stats()
                    assert (rendered2 == rendered + 1 and found2 == found) if prune else (found2 + rendered2 == found + rendered + 1), (mode, axis, k, prune)
                    for i, w in enumerate(ws):
                        _same(dev.download(i), _times(full, w, "fp64"), f"{mode}, axis {axis}, pruning {prune}, item {i} {items[i]}")
    finally:
        for name in env:
            os.environ.pop(name, None)
        dev.close()


def test_zzz_report_observed():
    """Not a check: prints what this run measured, for OBSERVED_MI355X above."""
    print("observed, as fractions of the bounds:", {k: (None if v is None else float(f"{v:.3g}")) for k, v in OBSERVED.items()})
