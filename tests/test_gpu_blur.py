"""Blurred PSFs on the GPU (paos_blur_apply, run_batch(psf_blur=...); csrc/blur_pass.h): the blurred PSF against the
long-double reference of tests/blur_np.py on the fetched PSF, the system OTF behind it, the bit-for-bit invariants, the
dead-tile memo of the PSF-storing passes, the count of line transforms, the run_batch paths and misuse of the C calls.
Every assertion message of the long-double checks carries the kernel's error next to the NumPy restatement's and the
bound; ``pytest -s`` prints them as XPREC lines (profiles/r15_blur_xprec.md)."""
import ctypes

import numpy as np
import pytest

import blur_np
import detector_np
import otf_np
import products_xprec as px
import xprec_np as xp

pytestmark = pytest.mark.gpu

FIELD = {"us": 0.0, "ut": 0.0}
DX, DY = 1.0e-5, 1.3e-5  # the samplings of the direct calls, metres


def _fields(n, batch):
    """The structured PSF of products_xprec.otf_fields (row packing, self-mirror columns) first, its random one second,
    further seeded random fields behind them."""
    structured_last = px.otf_fields(n)
    rng = np.random.default_rng(626200 + n)
    extra = [rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)) for _ in range(max(0, batch - 2))]
    return (structured_last[::-1] + extra)[:batch]


def _params(batch):
    """Anisotropic sigmas that differ per item (metres); the last item of a batch of two or more has a pixel factor."""
    sx = np.array([(1.5 + 0.7 * i) * DX for i in range(batch)])
    sy = np.array([(0.6 + 1.1 * i) * DY for i in range(batch)])
    px_, py_ = np.zeros(batch), np.zeros(batch)
    px_[-1], py_[-1] = 2.0 * DX, 3.0 * DY
    if batch == 1:
        px_[0], py_[0] = 0.0, 0.0
    return sx, sy, px_, py_


def _tables(n, params, i):
    sx, sy, px_, py_ = params
    return blur_np.tables_of(n, DX, DY, sx[i], sy[i], px_[i], py_[i])


def _device(n, precision, fields):
    from paos_amd import _lib

    dev = _lib.DeviceFields(n, len(fields), precision)
    for i, u in enumerate(fields):
        dev.upload(i, u)
    dev.psf_keep()
    return dev


def _blurred(dev, params):
    dev.otf_compute()
    dev.blur_apply(DX, DY, *params)


# 2048^2 fp32: the 8-row blocks of the complex64 layout; 4096^2 fp64: one tile of two columns per workgroup
@pytest.mark.parametrize("n,batch,precision", [(64, 3, "fp64"), (256, 2, "fp64"), (2048, 1, "fp32"), (4096, 2, "fp64")])
def test_against_long_double(n, batch, precision):
    """P' against ifft2(T fft2(P)) in long double on the fetched PSF -- whole up to 2048^2, on sampled image rows and
    columns at 4096^2 -- at xprec_np.bound(n, 4, 1): the L2 error relative to the image, every element's error relative
    to the image's norm (blur_np.errors), the NumPy restatement in the context's precision within half of either.  Up to
    256^2 also the system OTF handed out afterwards against T OTF_ref at products_xprec.otf_bound with one more factor;
    at every size it is Hermitian and the MTF point-symmetric bit for bit, exactly 1 at zero frequency, and the cuts
    are the fetched array's."""
    xp.require_long_double()
    params = _params(batch)
    dev = _device(n, precision, _fields(n, batch))
    report = []
    h = n // 2
    try:
        psfs = [dev.psf_fetch(i) for i in range(batch)]
        if n <= 256:
            dev.otf_compute()
            optical = [px.otf_unshifted(dev.otf_fetch(i, "otf")) for i in range(batch)]
        _blurred(dev, params)
        cuts = dev.otf_cuts()
        for i in range(batch):
            tx, ty = _tables(n, params, i)
            got = dev.psf_fetch(i)
            yard = blur_np.blur(psfs[i], tx, ty, precision)
            norm = float(np.linalg.norm(yard if precision == "fp64" else blur_np.blur(psfs[i], tx, ty)))  # (a scale: fp64 is plenty)
            what = f"blur {precision} {n}^2 B={batch} item {i}"
            if n <= 2048:
                ref = blur_np.blur_reference(psfs[i], tx, ty)
                report.append(blur_np.check(got, ref, yard, norm, n, precision, what))
                assert abs(float(got.sum() - psfs[i].sum())) <= blur_np.bound(n, precision)[0] * norm * n
                del ref
            else:
                idx = blur_np.sample_indices(n)
                ref = blur_np.blur_reference_lines(psfs[i], tx, ty, idx)
                report.append(blur_np.check(got[idx, :], ref, yard[idx, :], norm, n, precision, f"{what} {idx.size} sampled rows"))
                ref = blur_np.blur_reference_lines(psfs[i], tx, ty, idx, rows=False)
                report.append(blur_np.check(got[:, idx], ref, yard[:, idx], norm, n, precision, f"{what} {idx.size} sampled columns"))
            # the system transfer functions
            centred, mtf = dev.otf_fetch(i, "otf"), dev.otf_fetch(i, "mtf")
            assert centred[h, h].real == 1.0 and centred[h, h].imag == 0.0 and mtf[h, h] == 1.0
            body = centred[1:, 1:]
            assert np.array_equal(body, np.conj(body[::-1, ::-1])) and np.array_equal(mtf[1:, 1:], mtf[1:, 1:][::-1, ::-1])
            assert np.array_equal(centred[0, 1:], np.conj(centred[0, 1:][::-1])) and np.array_equal(centred[1:, 0], np.conj(centred[1:, 0][::-1]))
            assert centred[0, 0].imag == 0.0
            want_x, want_y = otf_np.cuts_of(mtf)
            assert np.array_equal(cuts[i, 0], want_x) and np.array_equal(cuts[i, 1], want_y)
            if n <= 256:
                t = blur_np.transfer(tx, ty, blur_np.LDR)
                sys_ref = px.otf_reference(psfs[i]) * t
                sys_yard = px.otf_yardstick(psfs[i], precision) * blur_np.transfer(tx, ty)
                scales = px.otf_scales(sys_yard)
                b_l2, b_el = xp.bound(n, 2, 2, precision)  # products_xprec.otf_bound with one more factor
                for axis in (0, 1):
                    g_l2, g_el = px.otf_line_errors(px.otf_unshifted(centred), sys_ref, None, None, axis, scales)
                    y_l2, y_el = px.otf_line_errors(sys_yard, sys_ref, None, None, axis, scales)
                    msg = (f"system otf {what} axis {axis}: kernel L2 {g_l2:.3g} / element {g_el:.3g}; NumPy restatement L2 "
                           f"{y_l2:.3g} / element {y_el:.3g}; bound L2 {b_l2:.3g} / element {b_el:.3g}")
                    report.append(msg)
                    assert b_l2 >= 2 * y_l2 and b_el >= 2 * y_el, "bound tighter than twice the restatement -- " + msg
                    assert g_l2 <= b_l2 and g_el <= b_el, msg
                # ... and it is the optical one times T, one rounding per part
                assert np.max(np.abs(px.otf_unshifted(centred) - optical[i] * blur_np.transfer(tx, ty))) <= 4 * xp.U64
    finally:
        dev.close()
        print("\nXPREC " + "\nXPREC ".join(report))


@pytest.mark.parametrize("n,precision", [(128, "fp64"), (1024, "fp64"), (512, "fp32"), (4096, "fp32")])
def test_bit_for_bit_invariants(n, precision):
    """otf_compute + blur_apply on the same PSFs a second time gives the same bits; an item's P' does not depend on the
    batch size or on its place in the batch (against a batch-1 context); a second blur_apply compounds."""
    from paos_amd import _lib

    batch = 3 if n <= 1024 else 2
    fields, params = _fields(n, batch), _params(batch)
    dev = _device(n, precision, fields)
    one = _lib.DeviceFields(n, 1, precision)
    try:
        _blurred(dev, params)
        first = [dev.psf_fetch(i) for i in range(batch)]
        first_otf = dev.otf_fetch(batch - 1, "otf")
        dev.psf_keep()
        _blurred(dev, params)
        for i in range(batch):
            assert np.array_equal(dev.psf_fetch(i), first[i]), f"item {i}: a repeated run gives other bits"
        assert np.array_equal(dev.otf_fetch(batch - 1, "otf"), first_otf)
        for i in (0, batch - 1):
            one.upload(0, fields[i])
            one.psf_keep()
            one.otf_compute()
            one.blur_apply(DX, DY, *(p[i:i + 1] for p in params))
            assert np.array_equal(one.psf_fetch(0), first[i]), f"item {i} of {batch} differs from the same PSF run alone"
        if n <= 1024:
            dev.blur_apply(DX, DY, *params)  # T2 T1 on the spectrum that already carries T1
            tx, ty = _tables(n, params, 0)
            want = blur_np.blur(first[0], tx, ty)
            tol = blur_np.bound(n, precision)[1] * float(np.linalg.norm(want))
            assert float(np.max(np.abs(dev.psf_fetch(0) - want))) <= tol
    finally:
        dev.close()
        one.close()


def test_the_zero_memo_does_not_survive_a_blur():
    """A lean run_batch with psf_blur, then the same lean run without it on the same context: the PSFs the second run
    keeps equal a fresh context's bit for bit.  1024^2 complex128: the frugal storing pass leaves tiles it knows to be
    zero unwritten when the previous storing pass had the same live lines -- after a blur the buffer holds P' there."""
    from paos_amd import PsfBlur, _lib
    from paos_amd.chains import syn20_chain, syn20_wavelength
    from paos_amd.run import run_batch

    n, wls = 1024, [syn20_wavelength(k) for k in (0, 511)]
    chains = [syn20_chain() for _ in wls]
    dev, fresh = _lib.DeviceFields(n, 2), _lib.DeviceFields(n, 2)
    try:
        first = run_batch(1.0, wls, n, 4, FIELD, chains, outputs=(), keep_psf=True, dev=dev)
        sharp = [dev.psf_fetch(i) for i in range(2)]
        sigma = (3.0 * first[0][20]["dx"], 2.0 * first[0][20]["dy"])
        res = run_batch(1.0, wls, n, 4, FIELD, chains, outputs=(), dev=dev, psf_blur=PsfBlur(*sigma))
        assert res[0][20]["blur_sigma"] == sigma
        blurred = dev.psf_fetch(0)
        assert np.max(np.abs(blurred - sharp[0])) > 1e-3 * sharp[0].max(), "the blur left the PSF as it was"
        run_batch(1.0, wls, n, 4, FIELD, chains, outputs=(), keep_psf=True, dev=dev)
        run_batch(1.0, wls, n, 4, FIELD, chains, outputs=(), keep_psf=True, dev=fresh)
        for i in range(2):
            got, want = dev.psf_fetch(i), fresh.psf_fetch(i)
            same = got == want
            assert same.all(), f"item {i}: {int((~same).sum())} pixels of the blurred PSF survive, first at {np.argwhere(~same)[:3].tolist()}"
            assert np.array_equal(want, sharp[i])
    finally:
        dev.close()
        fresh.close()


@pytest.mark.parametrize("n", [256, 4096])
def test_line_transforms(n):
    """paos_profile_line_transforms around blur_apply: the row launch runs exactly batch N/2 lines (two PSF rows per
    line), both launches together at most batch (N + N/8) -- a complex inverse 2-D transform runs batch 2 N."""
    from paos_amd import _lib

    batch = 2
    dev = _device(n, "fp64", _fields(n, batch))
    try:
        dev.otf_compute()
        dev.profile_begin(_lib.KERNEL_PASS_ANY)
        dev.blur_apply(DX, DY, *_params(batch))
        lines = dev.profile_line_transforms()
        dev.profile_end_launches()
    finally:
        dev.close()
    print(f"blur_apply {n}^2: line transforms per item {lines / batch}")
    assert lines.size == 2 and lines[1] == batch * n / 2  # (columns first, then the packed rows)
    assert batch * n / 2 <= lines[0] and lines.sum() <= batch * (n + n / 8)


def test_run_batch_transforms_forward_once():
    """run_batch with psf_blur and mtf_cuts: against the same run without the blur, the timed pass launches differ by
    the two of blur_apply alone -- the OTF request does not transform a second time."""
    from paos_amd import PsfBlur, _lib
    from paos_amd.chains import syn20_chain, syn20_wavelength
    from paos_amd.run import run_batch

    n, wls = 256, [syn20_wavelength(k) for k in (0, 511)]
    chains = [syn20_chain() for _ in wls]
    counts = []
    dev = _lib.DeviceFields(n, 2)
    try:
        for blur in (None, PsfBlur(3.0e-5, 2.0e-5)):
            dev.profile_begin(_lib.KERNEL_PASS_ANY)
            run_batch(1.0, wls, n, 4, FIELD, chains, outputs=(), mtf_cuts=True, dev=dev, psf_blur=blur)
            counts.append(dev.profile_line_transforms())
            dev.profile_end_launches()
    finally:
        dev.close()
    plain, blurred = counts
    assert blurred.size == plain.size + 2  # (a second forward pair would make it + 4)
    # the plain run ends with otf_compute's rows and columns; the blurred one adds blur_apply's columns and rows behind them
    # (the walk's launches on the generic kernel at this size do not report their lines: only the tails are compared)
    assert np.array_equal(blurred[-4:-2], plain[-2:]) and plain[-2] == 2 * n / 2
    assert blurred[-1] == 2 * n / 2 and blurred[-2:].sum() <= 2 * (n + n / 8)


def test_run_batch_end_to_end():
    """SYN20 at 256^2 x 4: ``detector`` with a blur against detector_np applied to the restated P' of the oracle's PSF;
    the lean walk against the ordinary walk bit for bit; the dz == 0.0 plane of a focus stack equals the nominal record
    bit for bit."""
    from oracle.run_np import run as oracle_run
    from paos_amd import Detector, PsfBlur
    from paos_amd.chains import syn20_chain, syn20_wavelength
    from paos_amd.run import run_batch

    n, wls = 256, [syn20_wavelength(k) for k in (0, 170, 340, 511)]
    chains = [syn20_chain() for _ in wls]
    refs = [oracle_run(1.0, wl, n, 4, FIELD, chain)[20] for wl, chain in zip(wls, chains)]
    sx = [(1.0 + 0.5 * i) * refs[0]["dx"] for i in range(4)]
    sy = [(2.0 - 0.4 * i) * refs[0]["dy"] for i in range(4)]
    det = Detector(33, 29, 1.7 * refs[0]["dx"], 2.3 * refs[0]["dy"], xc=0.31 * refs[0]["dx"], yc=-0.62 * refs[0]["dy"])
    blur = PsfBlur(sx, sy, array=True)
    res = run_batch(1.0, wls, n, 4, FIELD, chains, outputs=("psf",), mtf_cuts=True, detector=det, psf_blur=blur)
    lean = run_batch(1.0, wls, n, 4, FIELD, chains, outputs=(), mtf_cuts=True, detector=det, psf_blur=blur)
    stack = run_batch(1.0, wls, n, 4, FIELD, chains, outputs=("psf",), mtf_cuts=True, detector=det, psf_blur=blur,
                      focus_planes=[6.0e-5, 0.0])
    for i, ref in enumerate(refs):
        rec = res[i][20]
        psf = ref["amplitude"] ** 2
        tabs = blur_np.tables_of(n, ref["dx"], ref["dy"], sx[i], sy[i])
        want = blur_np.blur(psf, *tabs)
        image = detector_np.rebin(want, det, ref["dx"], ref["dy"])
        errs = [float(np.max(np.abs(rec["psf_blur"] - want)) / want.max()), float(np.max(np.abs(rec["detector"] - image)) / image.max()),
                float(np.max(np.abs(rec["mtf_x"] - otf_np.cuts_of(otf_np.mtf(want))[0])))]
        print(f"run_batch SYN20 256^2 item {i}: psf_blur {errs[0]:.2e}, detector {errs[1]:.2e}, system mtf_x {errs[2]:.2e}")
        assert max(errs) <= 1.0e-10
        assert np.max(np.abs(rec["psf"] - psf)) <= 1.0e-10 * psf.max()  # 'psf' stays the optical one
        assert "blur_sigma" not in res[i][1] and rec["blur_sigma"] == (sx[i], sy[i])
        for key in ("psf_blur", "detector", "mtf_x", "mtf_y"):
            assert np.array_equal(lean[i][20][key], rec[key]), key
        assert "psf" not in lean[i][20]
        for p in stack[i][20]["focus"]:
            assert {"psf_blur", "detector", "mtf_x", "blur_sigma"} <= set(p)
            if p["dz"] == 0.0:
                for key in ("psf_blur", "detector", "mtf_x", "mtf_y"):
                    assert np.array_equal(p[key], rec[key]), key
            else:
                assert np.max(np.abs(p["psf_blur"] - blur_np.blur(p["psf"], *tabs))) <= 1.0e-10 * p["psf"].max()


def test_misuse_is_refused_and_the_context_stays_usable():
    from paos_amd import _lib

    n, batch = 128, 2
    dev = _lib.DeviceFields(n, batch, "fp64")
    lib, ctx = dev._lib, dev._ctx
    good = np.ascontiguousarray(np.tile([DX, DY, 2.0 * DX, 1.0 * DY, 0.0, 0.0], (batch, 1)))
    ptr = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))  # noqa: E731
    try:
        fields = _fields(n, batch)
        for i, u in enumerate(fields):
            dev.upload(i, u)
        dev.psf_keep()
        before = [dev.psf_fetch(i) for i in range(batch)]
        assert lib.paos_blur_apply(ctx, ptr(good)) == 1 and b"paos_otf_compute" in lib.paos_last_error(ctx)  # before any otf_compute
        dev.otf_compute()
        dev.psf_keep()
        assert lib.paos_blur_apply(ctx, ptr(good)) == 1 and b"stale" in lib.paos_last_error(ctx)
        dev.otf_compute()
        assert lib.paos_blur_apply(ctx, None) == 1 and lib.paos_blur_apply(None, ptr(good)) == 1
        for col, value in ((2, -1.0e-6), (3, float("nan")), (0, 0.0), (1, float("inf")), (4, -1.0), (5, float("inf"))):
            bad = good.copy()
            bad[1, col] = value
            assert lib.paos_blur_apply(ctx, ptr(bad)) == 1 and b"item 1" in lib.paos_last_error(ctx), (col, value)
        with pytest.raises(ValueError):
            dev.blur_apply([DX] * 3, DY, DX, DY)
        # nothing of the above touched the PSFs, the spectra or the field, and the context is still usable
        assert all(np.array_equal(dev.psf_fetch(i), before[i]) for i in range(batch))
        assert np.max(np.abs(dev.otf_fetch(1, "otf") - otf_np.otf(before[1]))) <= 1.0e-10
        assert lib.paos_blur_apply(ctx, ptr(good)) == 0
        want = blur_np.blur(before[1], *blur_np.tables_of(n, DX, DY, 2.0 * DX, 1.0 * DY))
        assert np.max(np.abs(dev.psf_fetch(1) - want)) <= 1.0e-10 * want.max()
        assert all(np.array_equal(dev.download(i), fields[i]) for i in range(batch))
        # other parameters on the same context: the tables kept for the call before are not served again
        dev.psf_keep()
        dev.otf_compute()
        dev.blur_apply(DX, DY, [2.0 * DX, 0.5 * DX], 3.0 * DY)
        for i, sx in enumerate((2.0 * DX, 0.5 * DX)):
            want = blur_np.blur(before[i], *blur_np.tables_of(n, DX, DY, sx, 3.0 * DY))
            assert np.max(np.abs(dev.psf_fetch(i) - want)) <= 1.0e-10 * want.max()
    finally:
        dev.close()
