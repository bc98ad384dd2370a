"""Transfer functions on the GPU (paos_otf_compute / paos_otf_fetch / paos_otf_cuts, run_batch(outputs=("mtf", "otf"),
mtf_cuts=True)): every grid size and both precisions against the NumPy restatement (tests/otf_np.py) on the fetched
PSF, the bit-for-bit invariants, the exact answer for a single bright pixel, an all-zero item, the count of line
transforms, the run_batch paths, and misuse of the C calls."""
import ctypes

import numpy as np
import pytest

import otf_np

pytestmark = pytest.mark.gpu

FIELD = {"us": 0.0, "ut": 0.0}
# the project's parity gates, max-abs on the DC-normalised result (|OTF| <= 1)
GATE = {"fp64": 1.0e-10, "fp32": 1.0e-6}


def _fields(n, batch, seed=0):
    """Random complex fields, seeded, with no symmetry."""
    rng = np.random.default_rng(8080 + n + seed)
    return [rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)) for _ in range(batch)]


def _device(n, precision, fields):
    from paos_amd import _lib

    dev = _lib.DeviceFields(n, len(fields), precision)
    for i, u in enumerate(fields):
        dev.upload(i, u)
    dev.psf_keep()
    return dev


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("n", [64, 128, 256, 512, 1024, 2048, 4096])
def test_against_the_restatement(n, precision):
    """OTF and MTF of two different random PSFs against ``otf_np`` on the fetched PSF: max-abs error <= 1e-10 in fp64
    contexts, <= 1e-6 in fp32 contexts.  Worst errors seen on an MI355X are printed (pytest -s) and recorded in
    profiles/r08_otf_bench.md."""
    dev = _device(n, precision, _fields(n, 2))
    try:
        dev.otf_compute()
        worst = 0.0
        for i in range(2):
            want = otf_np.otf(dev.psf_fetch(i))
            got, got_mtf = dev.otf_fetch(i, "otf"), dev.otf_fetch(i, "mtf")
            assert got.dtype == np.complex128 and got_mtf.dtype == np.float64 and got.shape == got_mtf.shape == (n, n)
            err = max(float(np.max(np.abs(got - want))), float(np.max(np.abs(got_mtf - np.abs(want)))))
            worst = max(worst, err)
        print(f"otf {n}^2 {precision}: worst max-abs error {worst:.2e} (gate {GATE[precision]:.0e})")
        assert worst <= GATE[precision]
    finally:
        dev.close()


@pytest.mark.parametrize("n,precision", [(64, "fp64"), (256, "fp64"), (4096, "fp64"), (256, "fp32"), (2048, "fp32")])
def test_exact_invariants(n, precision):
    """Zero frequency is 1 + 0i, the OTF is Hermitian and the MTF point-symmetric, the cuts are the fetched MTF's half row
    and half column -- all bit for bit -- and item 1 does not depend on item 0."""
    h = n // 2
    fields = _fields(n, 2)
    dev = _device(n, precision, fields)
    try:
        dev.otf_compute()
        cuts = dev.otf_cuts()
        keep = None
        for i in range(2):
            otf, mtf = dev.otf_fetch(i, "otf"), dev.otf_fetch(i, "mtf")
            assert otf[h, h].real == 1.0 and otf[h, h].imag == 0.0 and mtf[h, h] == 1.0
            # unshifted indices: OTF[(N - ky) % N][(N - kx) % N] == conj OTF[ky][kx]
            raw = np.fft.ifftshift(otf)
            mirrored = np.roll(raw[::-1, ::-1], (1, 1), axis=(0, 1))
            assert np.array_equal(mirrored.real, raw.real) and np.array_equal(mirrored.imag, -raw.imag)
            raw_mtf = np.fft.ifftshift(mtf)
            assert np.array_equal(np.roll(raw_mtf[::-1, ::-1], (1, 1), axis=(0, 1)), raw_mtf)
            want_x, want_y = otf_np.cuts_of(mtf)
            assert np.array_equal(cuts[i, 0], want_x) and np.array_equal(cuts[i, 1], want_y)
            keep = otf
        dev.upload(0, _fields(n, 1, seed=5)[0])
        dev.psf_keep()
        dev.otf_compute()
        assert np.array_equal(dev.otf_fetch(1, "otf"), keep), "item 1 depends on item 0"
    finally:
        dev.close()


@pytest.mark.parametrize("n", [256, 2048])
def test_single_pixel_gives_the_phase_ramp(n):
    """A one-hot PSF off centre in x only (item 0) and in y only (item 1), asymmetric: MTF == 1 and the OTF is the exact
    phase ramp with the right sign on both axes -- a transposed axis, a wrong mirror or a wrong checkerboard shows here."""
    h = n // 2
    spots = [(h, h + 5), (h - 9, h)]  # (row, column)
    fields = []
    for k0, j0 in spots:
        u = np.zeros((n, n), dtype=np.complex128)
        u[k0, j0] = 2.0 - 1.0j
        fields.append(u)
    ramps = [otf_np.phase_ramp(n, k0, j0) for k0, j0 in spots]
    for precision in ("fp64", "fp32"):
        dev = _device(n, precision, fields)
        try:
            dev.otf_compute()
            for i, (k0, j0) in enumerate(spots):
                want = ramps[i]
                got, mtf = dev.otf_fetch(i, "otf"), dev.otf_fetch(i, "mtf")
                err, merr = float(np.max(np.abs(got - want))), float(np.max(np.abs(mtf - 1.0)))
                print(f"one-hot {n}^2 {precision} spot {(k0, j0)}: ramp {err:.2e}, |MTF - 1| {merr:.2e}")
                assert err <= GATE[precision] and merr <= GATE[precision]
                for wrong in (np.conj(want), want.T):
                    assert np.max(np.abs(got - wrong)) > 0.1
        finally:
            dev.close()


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_an_all_zero_item_gives_zeros(precision):
    n = 128
    u = _fields(n, 1)[0]
    alone = _device(n, precision, [u, u])
    dev = _device(n, precision, [np.zeros((n, n), dtype=np.complex128), u])
    try:
        alone.otf_compute()
        dev.otf_compute()
        for what in ("otf", "mtf"):
            zero = dev.otf_fetch(0, what)
            assert not np.isnan(zero).any() and not zero.any()
            assert np.array_equal(dev.otf_fetch(1, what), alone.otf_fetch(1, what))
        cuts = dev.otf_cuts()
        assert not cuts[0].any() and np.array_equal(cuts[1], alone.otf_cuts()[1])
    finally:
        alone.close()
        dev.close()


@pytest.mark.parametrize("n", [256, 4096])
def test_line_transforms(n):
    """paos_profile_line_transforms around otf_compute: the row launch runs exactly batch N/2 lines (two PSF rows per
    line), both launches together at most batch (N + N/8) -- a complex 2-D transform runs batch 2 N."""
    from paos_amd import _lib

    batch = 2
    dev = _device(n, "fp64", _fields(n, batch))
    try:
        dev.profile_begin(_lib.KERNEL_PASS_ANY)
        dev.otf_compute()
        lines = dev.profile_line_transforms()
        dev.profile_end_launches()
    finally:
        dev.close()
    print(f"otf_compute {n}^2: line transforms per item {lines / batch}")
    assert lines.size == 2 and lines[0] == batch * n / 2
    assert batch * n / 2 <= lines[1] and lines.sum() <= batch * (n + n / 8)


def test_run_batch_end_to_end():
    """SYN20 at 256^2 x 4: ``mtf`` and the cuts against the restatement applied to the oracle's PSF; the lean walk's cuts
    equal the ordinary walk's bit for bit; the nominal plane of a focus stack equals the nominal record bit for bit and
    the other planes match the restatement on their fetched PSFs."""
    from oracle.run_np import run as oracle_run
    from paos_amd.chains import syn20_chain, syn20_wavelength
    from paos_amd.run import run_batch

    n, wls = 256, [syn20_wavelength(k) for k in (0, 170, 340, 511)]
    chains = [syn20_chain() for _ in wls]
    res = run_batch(1.0, wls, n, 4, FIELD, chains, outputs=("psf", "mtf"), mtf_cuts=True)
    lean = run_batch(1.0, wls, n, 4, FIELD, chains, outputs=(), mtf_cuts=True)
    delta = 6.0e-5
    stack = run_batch(1.0, wls, n, 4, FIELD, chains, outputs=("psf", "mtf"), mtf_cuts=True, focus_planes=[-delta, 0.0, delta])
    for i, wl in enumerate(wls):
        rec = res[i][20]
        ref = oracle_run(1.0, wl, n, 4, FIELD, chains[i])[20]
        want = otf_np.mtf(ref["amplitude"] ** 2)
        want_x, want_y = otf_np.cuts_of(want)
        errs = [float(np.max(np.abs(rec["mtf"] - want))), float(np.max(np.abs(rec["mtf_x"] - want_x))),
                float(np.max(np.abs(rec["mtf_y"] - want_y)))]
        print(f"run_batch SYN20 256^2 item {i}: mtf {errs[0]:.2e}, cuts {errs[1]:.2e} {errs[2]:.2e}")
        assert max(errs) <= GATE["fp64"]
        assert np.array_equal(rec["freq_x"], otf_np.freqs(n, ref["dx"])) and rec["freq_x"][-1] == 1.0 / (2.0 * ref["dx"])
        assert np.array_equal(rec["freq_y"], otf_np.freqs(n, ref["dy"]))
        assert "mtf" not in res[i][1] and "mtf_x" not in res[i][1]
        for key in ("mtf_x", "mtf_y", "freq_x", "freq_y"):
            assert np.array_equal(lean[i][20][key], rec[key]), key
        assert "mtf" not in lean[i][20] and "psf" not in lean[i][20]
        planes = stack[i][20]["focus"]
        assert np.array_equal(stack[i][20]["mtf"], rec["mtf"])
        for p in planes:
            if p["dz"] == 0.0:
                for key in ("mtf", "mtf_x", "mtf_y", "freq_x", "freq_y"):
                    assert np.array_equal(p[key], rec[key]), key
            else:
                assert np.max(np.abs(p["mtf"] - otf_np.mtf(p["psf"]))) <= GATE["fp64"]
                px, py = otf_np.cuts_of(p["mtf"])
                assert np.array_equal(p["mtf_x"], px) and np.array_equal(p["mtf_y"], py)
                assert np.max(np.abs(p["mtf"] - rec["mtf"])) > 1e-6


def test_misuse_is_refused_and_the_context_stays_usable():
    from paos_amd import _lib

    n, batch = 128, 2
    dev = _lib.DeviceFields(n, batch, "fp64")
    lib, ctx = dev._lib, dev._ctx
    out = np.empty((n, n), dtype=np.complex128)
    cuts = np.empty((batch, 2, n // 2 + 1))
    optr = out.ctypes.data_as(ctypes.c_void_p)
    cptr = cuts.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    try:
        fields = _fields(n, batch)
        for i, u in enumerate(fields):
            dev.upload(i, u)
        assert lib.paos_otf_compute(ctx) == 1 and b"PSF" in lib.paos_last_error(ctx)  # no PSF kept yet
        assert lib.paos_otf_compute(None) == 1
        dev.psf_keep()
        assert lib.paos_otf_fetch(ctx, 0, _lib.OTF_MTF, optr) == 1 and b"paos_otf_compute" in lib.paos_last_error(ctx)
        assert lib.paos_otf_cuts(ctx, cptr) == 1
        assert lib.paos_otf_compute(ctx) == 0
        for item, what, ptr in ((-1, 0, optr), (batch, 0, optr), (0, 2, optr), (0, -1, optr), (0, 0, None)):
            assert lib.paos_otf_fetch(ctx, item, what, ptr) == 1
        assert lib.paos_otf_cuts(ctx, None) == 1
        assert lib.paos_otf_fetch(ctx, 1, _lib.OTF_COMPLEX, optr) == 0
        first = out.copy()
        # a newer PSF makes the result stale: refused, not served from old data
        dev.psf_keep()
        assert lib.paos_otf_fetch(ctx, 1, _lib.OTF_COMPLEX, optr) == 1 and b"stale" in lib.paos_last_error(ctx)
        assert lib.paos_otf_cuts(ctx, cptr) == 1 and b"stale" in lib.paos_last_error(ctx)
        ticket = dev.psf_keep_power()
        dev.norm2_fetch(ticket)
        assert lib.paos_otf_fetch(ctx, 1, _lib.OTF_COMPLEX, optr) == 1
        # the context is still usable, and nothing of the above touched the field or the PSFs
        dev.otf_compute()
        assert np.array_equal(dev.otf_fetch(1, "otf"), first)
        assert np.max(np.abs(first - otf_np.otf(dev.psf_fetch(1)))) <= GATE["fp64"]
        assert all(np.array_equal(dev.download(i), fields[i]) for i in range(batch))
    finally:
        dev.close()
