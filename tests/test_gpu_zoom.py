"""Zoomed PSF windows on the GPU (paos_zoom_compute / paos_zoom_fetch, run_batch(psf_zoom=...)): the fragment layout of
the fp64 matrix instruction by a bit-exact permutation, windows against the NumPy restatement (tests/zoom_np.py) on the
field the same context returns, the bit-for-bit invariants, the chain end to end, and misuse of the C calls."""
import ctypes
import os

import numpy as np
import pytest

import focus_np
import zoom_np
from conftest import l2_rel_err, rel_err

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENS = os.path.join(ROOT, "data", "lens")
# the project's parity gates: max-norm relative to the peak and L2-relative
GATE = {"fp64": 1.0e-10, "fp32": 2.0e-5}
KERNEL_GATE = 1.0e-10  # the contractions run in fp64 in either kind of context


def _device(n, batch, precision="fp64"):
    from paos_amd import _lib

    return _lib.DeviceFields(n, batch, precision)


def _random_fields(n, batch, seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)) for _ in range(batch)]


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("n,m", [(64, 16), (64, 48), (256, 16), (256, 48)])
def test_permutation_is_bit_exact(n, m, precision):
    """s = 1 and integer centres: every weight row is a unit vector, so the window is a shifted copy of the field.  The
    field is small-integer valued and asymmetric in rows, columns, real and imaginary part: an operand or a result in
    the wrong lane or register (the f32 forms' row map puts 3 of every 4 results in the wrong row) shows as a wrong
    integer."""
    k, j = np.mgrid[0:n, 0:n]
    fields = [((3 * k + 7 * j + i) % 17 - 8) + 1j * ((5 * k - 11 * j - i) % 13 - 6) for i in range(2)]
    centres = np.array([[n / 2 + 9.0, n / 2 - 21.0], [3.0, n - 2.0]])  # (the second window wraps in both axes)
    dev = _device(n, 2, precision)
    try:
        for i, u in enumerate(fields):
            dev.upload(i, u)
        dev.zoom_compute(m, 1, centres, field=True)
        for i, u in enumerate(fields):
            cx, cy = (int(v) for v in centres[i])
            idx = np.arange(m) - m // 2
            want = u[np.ix_((cy + idx) % n, (cx + idx) % n)].astype(np.complex128)
            got = dev.zoom_fetch(i, "field")
            assert np.array_equal(got, want), (i, np.argwhere(got != want)[:4])
            assert np.array_equal(dev.zoom_fetch(i, "psf"), want.real**2 + want.imag**2)
    finally:
        dev.close()


CASES = [(64, 3, 16, 4, None),
         (256, 2, 48, 3, [[128.25, 127.5], [100.7, 131.3]]),
         (1024, 2, 256, 8, [[500.0, 520.0], [512.0, 40.0]]),
         (4096, 1, 64, 4, None)]


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("n,batch,m,s,centres", CASES)
def test_windows_against_the_restatement(n, batch, m, s, centres, precision):
    """Random normal fields; the reference is the restatement on the field downloaded from the same context, so the
    kernels are isolated from the field's own precision.  Gate 1e-10, max-norm relative to the peak and L2-relative, for
    the complex window and for its intensity.  Largest errors seen on an MI355X are printed (pytest -s)."""
    dev = _device(n, batch, precision)
    try:
        for i, u in enumerate(_random_fields(n, batch, 100 + n)):
            dev.upload(i, u)
        dev.zoom_compute(m, s, centres, field=True)
        worst = [0.0] * 4
        for i in range(batch):
            u = dev.download(i)
            cxy = (None, None) if centres is None else centres[i]
            want = zoom_np.window(u, m, s, *cxy)
            got, got_psf = dev.zoom_fetch(i, "field"), dev.zoom_fetch(i, "psf")
            errs = [rel_err(got, want), l2_rel_err(got, want), rel_err(got_psf, zoom_np.psf(want)),
                    l2_rel_err(got_psf, zoom_np.psf(want))]
            worst = [max(a, b) for a, b in zip(worst, errs)]
            assert all(e < KERNEL_GATE for e in errs), (i, errs)
        print(f"zoom {n}^2 B={batch} M={m} s={s} {precision}: field max {worst[0]:.2e} L2 {worst[1]:.2e}, "
              f"psf max {worst[2]:.2e} L2 {worst[3]:.2e} (gate {KERNEL_GATE:.0e})")
    finally:
        dev.close()


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_invariants(precision):
    n, m, s = 256, 48, 4
    fields = _random_fields(n, 3, 5)
    centres = np.array([[131.0, 120.0], [40.0, 200.0], [128.0, 128.0]])
    dev = _device(n, 3, precision)
    one = _device(n, 1, precision)
    try:
        for i, u in enumerate(fields):
            dev.upload(i, u)
        dev.zoom_compute(m, s, centres, field=True)
        first = [(dev.zoom_fetch(i, "field"), dev.zoom_fetch(i, "psf")) for i in range(3)]
        idx = np.arange(m)
        on = idx[(idx - m // 2) % s == 0]
        for i in range(3):
            U, I = first[i]
            u = dev.download(i)
            # grid-aligned samples are the field's samples
            rows = (int(centres[i, 1]) + (on - m // 2) // s) % n
            cols = (int(centres[i, 0]) + (on - m // 2) // s) % n
            assert np.array_equal(U[np.ix_(on, on)], u[np.ix_(rows, cols)])
            # the intensity is re * re + im * im of the complex window, in doubles
            assert np.array_equal(I, U.real * U.real + U.imag * U.imag)
        # a second identical call gives the same bits
        dev.zoom_compute(m, s, centres, field=True)
        for i in range(3):
            assert np.array_equal(dev.zoom_fetch(i, "field"), first[i][0]) and np.array_equal(dev.zoom_fetch(i, "psf"), first[i][1])
        # without the complex window the intensity is the same, and the complex window is refused
        dev.zoom_compute(m, s, centres)
        assert np.array_equal(dev.zoom_fetch(1, "psf"), first[1][1])
        from paos_amd._lib import PaosHipError

        with pytest.raises(PaosHipError):
            dev.zoom_fetch(1, "field")
        # item 1 of the batch of 3 equals the same field run alone
        one.upload(0, fields[1])
        one.zoom_compute(m, s, centres[1:2], field=True)
        assert np.array_equal(one.zoom_fetch(0, "field"), first[1][0]) and np.array_equal(one.zoom_fetch(0, "psf"), first[1][1])
        # a wrapped window equals the unwrapped window of the rolled field -- the same weights on the same samples, summed
        # in another order: equal to rounding (N eps times the weights' 1-norm, far below 1e-12 of the peak)
        one.zoom_compute(m, s, [[2.25, 253.5]], field=True)
        wrapped = one.zoom_fetch(0, "field")
        one.upload(0, np.roll(fields[1], (100, 40), axis=(0, 1)))
        one.zoom_compute(m, s, [[42.25, 97.5]], field=True)
        rolled = one.zoom_fetch(0, "field")
        assert np.max(np.abs(wrapped - rolled)) < 1.0e-12 * np.max(np.abs(fields[1]))
        assert rel_err(wrapped, zoom_np.window(one.download(0), m, s, 42.25, 97.5)) < KERNEL_GATE
    finally:
        dev.close()
        one.close()


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_hubble_end_to_end(precision):
    """run_batch(psf_zoom=...) at 256^2 against the restatement of the ORACLE's last-surface field, at the parity gate of
    the context's precision; with focus_planes the 0.0 plane's window equals the nominal record's bit for bit."""
    from paos_amd import PsfWindow
    from paos_amd.parse_config import parse_config
    from paos_amd.run import run_batch

    n = 256
    pup, par, wls, fields, chains = parse_config(os.path.join(LENS, "Hubble_simple.ini"))
    wls = [1e-6 * wls[0], 1.3e-6 * wls[0]]
    chains = [chains[0], chains[0]]
    num = chains[0][list(chains[0].keys())[-1]]["num"]
    gate = GATE[precision]
    window = PsfWindow(64, 4, centre="centroid", field=True)
    res = run_batch(pup, wls, n, par["zoom"], fields[0], chains, outputs=("psf",), precision=precision, psf_zoom=window,
                    focus_planes=[-1.0e-4, 0.0])
    for i, wl in enumerate(wls):
        saved, end = focus_np.oracle_end_state(pup, wl, n, par["zoom"], fields[0], chains[i])
        rec = res[i][num]
        want = zoom_np.window(saved[num]["wfo"], 64, 4, *rec["zoom_centre"])
        errs = [rel_err(rec["wfo_zoom"], want), l2_rel_err(rec["wfo_zoom"], want),
                rel_err(rec["psf_zoom"], zoom_np.psf(want)), l2_rel_err(rec["psf_zoom"], zoom_np.psf(want))]
        print(f"zoom Hubble_simple {n}^2 {precision} item {i}: field max {errs[0]:.2e} L2 {errs[1]:.2e}, "
              f"psf max {errs[2]:.2e} L2 {errs[3]:.2e} (gate {gate:.0e})")
        assert all(e < gate for e in errs), (i, errs)
        assert rec["zoom_dx"] == rec["dx"] / 4 and rec["zoom_dy"] == rec["dy"] / 4
        # the centroid of a centred PSF is the grid centre; the window's peak is the PSF's peak, bit for bit
        assert rec["zoom_centre"] == (n / 2, n / 2)
        assert rec["psf_zoom"][32, 32] == rec["psf"][n // 2, n // 2]
        stack = rec["focus"]
        assert [p["dz"] for p in stack] == [-1.0e-4, 0.0]
        assert np.array_equal(stack[1]["psf_zoom"], rec["psf_zoom"]) and np.array_equal(stack[1]["wfo_zoom"], rec["wfo_zoom"])
        assert stack[0]["psf_zoom"].shape == (64, 64) and not np.array_equal(stack[0]["psf_zoom"], rec["psf_zoom"])


def test_misuse_of_the_c_calls():
    """Every refusal of include/paos_hip.h, by the C calls themselves (the Python layer checks first, so it is bypassed);
    the context still computes correctly after each one."""
    from paos_amd import _lib

    n, m, s = 64, 16, 4
    dev = _device(n, 2)
    lib, ctx = dev._lib, dev._ctx
    try:
        fields = _random_fields(n, 2, 9)
        for i, u in enumerate(fields):
            dev.upload(i, u)
        out = np.zeros((m, m), dtype=np.complex128)
        outp = out.ctypes.data_as(ctypes.c_void_p)
        assert lib.paos_zoom_fetch(ctx, 0, _lib.ZOOM_PSF, outp) == 1  # nothing computed yet
        want = [zoom_np.window(dev.download(i), m, s) for i in range(2)]

        def still_works():
            dev.zoom_compute(m, s, field=True)
            for i in range(2):
                assert rel_err(dev.zoom_fetch(i, "field"), want[i]) < KERNEL_GATE

        def centres(*values):
            return np.array(values, dtype=np.float64).ctypes.data_as(_lib._dbl_p)

        refused = [(24, s, None), (8, s, None), (0, s, None), (1040, 64, None), (2048, 64, None), (128, 1, None),
                   (m, 0, None), (m, 65, None), (m, -1, None),
                   (m, s, centres(32.0, 32.0, float("nan"), 1.0)), (m, s, centres(float("inf"), 32.0, 3.0, 1.0)),
                   (m, s, centres(32.0, 32.0, 64.0, 1.0)), (m, s, centres(32.0, -0.5, 3.0, 1.0))]
        for size, over, ctr in refused:
            assert lib.paos_zoom_compute(ctx, size, over, ctr, 1) == 1, (size, over)
            assert lib.paos_last_error(ctx)
            still_works()
        assert lib.paos_zoom_compute(None, m, s, None, 0) == 1
        for item, what, ptr in [(-1, 0, outp), (2, 0, outp), (0, 2, outp), (0, -1, outp), (0, 0, None)]:
            assert lib.paos_zoom_fetch(ctx, item, what, ptr) == 1, (item, what)
        still_works()
        dev.zoom_compute(m, s)  # without the complex window: PAOS_ZOOM_FIELD is refused, PAOS_ZOOM_PSF served
        assert lib.paos_zoom_fetch(ctx, 0, _lib.ZOOM_FIELD, outp) == 1
        assert rel_err(dev.zoom_fetch(0, "psf"), zoom_np.psf(want[0])) < KERNEL_GATE
        # another window size reallocates; another oversampling starts the tables afresh
        dev.zoom_compute(48, 3, [[10.5, 60.25], [32.0, 32.0]], field=True)
        assert rel_err(dev.zoom_fetch(0, "field"), zoom_np.window(dev.download(0), 48, 3, 10.5, 60.25)) < KERNEL_GATE
        still_works()
    finally:
        dev.close()


def test_a_deferred_stop_factor_is_applied_first():
    """paos_zoom_compute reads the field every other reader sees.  The C calls, driven directly: a pass program whose last
    pass sums the power, paos_stop_defer_last_power (nothing sweeps the field: the factor 1 / sqrt(power) is pending),
    then the window -- which must be the window of the SCALED field, the one a download afterwards returns."""
    from paos_amd.passes import PassCompiler

    n, m, s = 1024, 32, 4
    dev = _device(n, 2)
    try:
        for i, u in enumerate(_random_fields(n, 2, 77)):
            dev.upload(i, u)
        before = dev.norm2()
        comp = PassCompiler(2, n)
        comp.ptp([[1.0, 1.0 / (n * 1.0e-5), 1.0 / (n * 1.0e-5), np.pi * 1.0e-6 * 2.0e-4, -1.0]] * 2)
        done, ticket = comp.flush(dev, final_intensity=2)
        assert done and ticket is not None
        dev.make_stop(power_known=True, defer=True)  # (paos_stop_defer_last_power: enqueues no sweep of the field)
        dev.zoom_compute(m, s, field=True)
        windows = [dev.zoom_fetch(i, "field") for i in range(2)]
        idx = np.arange(m)
        on = idx[(idx - m // 2) % s == 0]
        px = n // 2 + (on - m // 2) // s
        after = dev.norm2()
        dev.norm2_release(ticket)
        for i in range(2):
            u = dev.download(i)
            assert before[i] > 1.0e5 and abs(after[i] - 1.0) < 1.0e-10  # the stop's factor is far from 1
            assert np.array_equal(windows[i][np.ix_(on, on)], u[np.ix_(px, px)])
            assert rel_err(windows[i], zoom_np.window(u, m, s)) < KERNEL_GATE
    finally:
        dev.close()


def test_more_phase_tables_than_the_context_keeps():
    """The context keeps 256 phase tables.  A sub-pixel sweep takes it past them (the pool holds 255 when a call brings
    two new fractions): the windows stay correct before, at and after the point where the kept tables are dropped."""
    from paos_amd import _lib

    n, m, s = 64, 16, 2
    dev = _device(n, 1)
    try:
        u = _random_fields(n, 1, 3)[0]
        dev.upload(0, u)
        u = dev.download(0)
        # call 0 brings one fraction, every later call two new ones: 1, 3, ..., 255 tables, then 257 would not fit
        centres = [(30.0 + 0.5, 40.0 + 0.5)] + [(30.0 + (2 * k + 1) / 1024.0, 9.0 + (2 * k + 2) / 1024.0) for k in range(140)]
        for k, (cx, cy) in enumerate(centres):
            dev.zoom_compute(m, s, [[cx, cy]], field=True)
            if k < 3 or k > 120 or k % 16 == 0:
                assert rel_err(dev.zoom_fetch(0, "field"), zoom_np.window(u, m, s, cx, cy)) < KERNEL_GATE, k
        # a fraction that is kept is served without dropping anything; the first ones were dropped and are built again
        for cx, cy in (centres[-1], centres[0], centres[1]):
            dev.zoom_compute(m, s, [[cx, cy]], field=True)
            assert rel_err(dev.zoom_fetch(0, "field"), zoom_np.window(u, m, s, cx, cy)) < KERNEL_GATE
    finally:
        dev.close()
    # one call: 256 distinct fractions are served (a context that already keeps others drops them first, once), 257 refused
    nb = 129
    dev = _device(n, nb)
    try:
        rng = np.random.default_rng(8)
        base = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
        for i in range(nb):
            dev.upload(i, np.roll(base, i, axis=1))
        dev.zoom_compute(m, s, np.full((nb, 2), 20.7))  # (one table kept, which the next call has no room beside)
        ctr = np.array([[10.0 + (2 * i) / 512.0, 50.0 + (2 * i + 1) / 512.0] for i in range(nb)])
        ctr[128] = ctr[0]  # 256 distinct fractions
        dev.zoom_compute(m, s, ctr, field=True)
        for i in (0, 1, 77, 127, 128):
            assert rel_err(dev.zoom_fetch(i, "field"), zoom_np.window(dev.download(i), m, s, *ctr[i])) < KERNEL_GATE, i
        ctr[128] = [10.0 + 511.0 / 1024.0, 50.0 + 509.0 / 1024.0]  # 258
        with pytest.raises(ValueError):
            dev.zoom_compute(m, s, ctr)
        assert dev._lib.paos_zoom_compute(dev._ctx, m, s, ctr.ctypes.data_as(_lib._dbl_p), 1) == 1
        ctr[128] = ctr[5]
        dev.zoom_compute(m, s, ctr, field=True)
        for i in (0, 128):
            assert rel_err(dev.zoom_fetch(i, "field"), zoom_np.window(dev.download(i), m, s, *ctr[i])) < KERNEL_GATE, i
    finally:
        dev.close()
