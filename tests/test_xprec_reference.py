"""The extended-precision reference of tests/xprec_np.py, checked before its verdicts on the kernels are trusted
(tests/test_gpu_xprec.py): long-double transforms and phase factors against mpmath, and the restatement against the
NumPy model of the device contract (tests/fakes.py) on random programs."""
import numpy as np
import pytest

import xprec_np as xp
from fakes import ModelDevice
from paos_amd import _lib


def test_long_double_is_wide_enough_and_fft_keeps_it():
    xp.require_long_double()  # raises with the reason when the platform has no 80-bit long double or np.fft drops it
    assert np.finfo(np.longdouble).eps <= 1e-18
    assert np.fft.ifft(np.ones(16, dtype=xp.LD)).dtype == xp.LD


def _mpf(mp, x):
    """A long double as an mpf, exactly (its 64-bit significand is the sum of two doubles)."""
    x = np.longdouble(x)
    hi = float(x)
    return mp.mpf(hi) + mp.mpf(float(x - np.longdouble(hi)))


def test_long_double_fft_against_an_mpmath_dft():
    mp = pytest.importorskip("mpmath")
    xp.require_long_double()
    n = 64
    rng = np.random.default_rng(11)
    lines = (rng.standard_normal((3, n)) + 1j * rng.standard_normal((3, n))).astype(xp.LD)
    lines[2] = 0
    lines[2, n - 1] = 1  # an impulse at the last index
    with mp.workdps(40):
        w = [mp.exp(-2j * mp.pi * k / n) for k in range(n)]
        for inverse in (False, True):
            got = np.fft.ifft(lines, axis=1) * n if inverse else np.fft.fft(lines, axis=1)
            for line, g in zip(lines, got):
                x = [mp.mpc(mp.mpf(float(v.real)) + mp.mpf(float(v.imag)) * 1j) for v in line.astype(np.complex128)]
                err2 = ref2 = mp.mpf(0)
                for k in range(n):
                    acc = mp.mpc(0)
                    for j in range(n):
                        t = w[(j * k) % n]
                        acc += x[j] * (mp.conj(t) if inverse else t)
                    gk = mp.mpc(_mpf(mp, g[k].real), _mpf(mp, g[k].imag))
                    err2 += abs(gk - acc) ** 2
                    ref2 += abs(acc) ** 2
                assert float(mp.sqrt(err2 / ref2)) <= 1e-18, (inverse, float(mp.sqrt(err2 / ref2)))


def test_long_double_phase_factor_against_mpmath_up_to_1e12_rad():
    mp = pytest.importorskip("mpmath")
    xp.require_long_double()
    rng = np.random.default_rng(5)
    q = np.concatenate([10.0 ** rng.uniform(0, 11.99, 300), [9.99e11, 9.9e11, 1.0, 0.0]])
    q = np.concatenate([q, np.round(q[:50] / (np.pi / 2)) * (np.pi / 2)])  # near quadrant boundaries too
    ql = q.astype(np.longdouble)
    c, s = np.cos(ql), np.sin(ql)
    worst = 0.0
    with mp.workdps(50):
        for qi, ci, si in zip(q, c, s):
            a = mp.mpf(float(qi))  # the fp64 argument, exactly
            worst = max(worst, abs(float(_mpf(mp, ci) - mp.cos(a))), abs(float(_mpf(mp, si) - mp.sin(a))))
    assert worst <= 1e-18, worst


def _random_program(rng, n, batch):
    """A few passes with every operator kind but masks, random enables, both orders, signs and scales."""
    nb = 8
    blocks = np.zeros((nb, batch, 5))
    for b in range(nb):
        for i in range(batch):
            blocks[b, i] = [float(rng.random() < 0.8), rng.uniform(0.5, 2.0), rng.uniform(0.0, 2.0),
                            rng.uniform(-0.01, 0.01), rng.choice([-1.0, 1.0])]
    blocks[6, :, 1] = rng.random(batch) < 0.5  # transform control blocks [enable, inverse]
    blocks[6, :, 0] = 1.0
    blocks[7, :, 1] = rng.random(batch) < 0.5
    blocks[5, :, 3] = 1.0 / n  # a scale
    qph = [_lib.PW_QPHASE_CENTRED, _lib.PW_QPHASE_NATURAL]
    passes = []
    for axis in (0, 1, 0):
        passes.append({"axis": axis, "fft1": 6, "fft2": 7 if rng.random() < 0.5 else -1,
                       "pre": [(_lib.PW_SIGN, int(rng.choice([0, _lib.PWF_X_ONLY, _lib.PWF_Y_ONLY])), 0),
                               (int(rng.choice(qph)), _lib.PWF_MUL2PI, 1)],
                       "mid": [(_lib.PW_SCALE, 0, 5), (int(rng.choice(qph)), 0, 2)],
                       "post": [(int(rng.choice(qph)), _lib.PWF_MUL2PI, 3)]})
    passes.append({"axis": -1, "fft1": -1, "fft2": -1, "pre": [(_lib.PW_QPHASE_CENTRED, 0, 4)], "mid": [], "post": []})
    return passes, blocks


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_restatement_equals_the_model_device(seed):
    xp.require_long_double()
    n, batch = 64, 3
    rng = np.random.default_rng(seed)
    passes, blocks = _random_program(rng, n, batch)
    u0 = rng.standard_normal((batch, n, n)) + 1j * rng.standard_normal((batch, n, n))
    dev = ModelDevice(n, batch)
    dev.u[:] = u0
    dev.run_passes(passes, blocks)
    for i in range(batch):
        got = xp.run_item(u0[i], passes, blocks, i, n)
        assert got.dtype == xp.LD
        err = float(np.max(np.abs(got - dev.u[i])) / np.max(np.abs(got)))
        assert err < 1e-14, (seed, i, err)
    # ... and the restatement on a subset of lines equals the whole one there (row passes only)
    row_passes = [p for p in passes if p["axis"] in (0, -1)]
    lines = np.array([0, 5, 31, 63])
    for i in range(batch):
        whole = xp.run_item(u0[i], row_passes, blocks, i, n)
        part = xp.run_item(u0[i][lines], row_passes, blocks, i, n, rows=lines)
        assert np.array_equal(part, whole[lines])


def test_bounds_clear_the_numpy_yardstick():
    """The bound of every transform case is at least twice what NumPy's fp64 / complex64 FFT reaches (xprec_np.check
    asserts this per case; here at the small sizes, where log2 N leaves the least room)."""
    xp.require_long_double()
    rng = np.random.default_rng(3)
    for n in (64, 128, 256):
        u = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
        blocks = np.zeros((2, 1, 5))
        blocks[0, 0, 0] = 1.0
        blocks[1, 0] = [1.0, 0.0, 0.0, 0.0, 0.0]
        passes = [{"axis": 0, "fft1": 1, "fft2": 1, "pre": [(_lib.PW_SIGN, 0, 0)]}]
        for precision, dt in (("fp64", np.complex128), ("fp32", np.complex64)):
            uin = u.astype(dt)
            ref = xp.run_item(uin, passes, blocks, 0, n)
            yard = xp.run_item(uin, passes, blocks, 0, n, dtype=dt)
            xp.check(yard, ref, yard, 0, n, 2, 0, precision, f"NumPy at {n} {precision}")


def test_check_fails_a_subtly_wrong_transform():
    """A twiddle off by 1e-14 (what a lost Cody-Waite term costs at large arguments) is caught."""
    xp.require_long_double()
    n = 256
    rng = np.random.default_rng(4)
    u = rng.standard_normal((8, n)) + 1j * rng.standard_normal((8, n))
    blocks = np.array([[[1.0, 0.0, 0.0, 0.0, 0.0]]])
    passes = [{"axis": 0, "fft1": 0}]
    ref = xp.run_item(u, passes, blocks, 0, n, rows=np.arange(8))
    yard = xp.run_item(u, passes, blocks, 0, n, rows=np.arange(8), dtype=np.complex128)
    k = np.arange(n)
    bad = (u * np.exp(-2j * np.pi * k * 3 / n * (1 + 1e-14))).sum(axis=1)  # bin 3, slightly wrong twiddles
    got = yard.astype(np.complex128).copy()
    got[:, 3] = bad
    with pytest.raises(AssertionError):
        xp.check(got, ref, yard, 0, n, 1, 0, "fp64", "perturbed")


def test_sampled_lines_cover_edges_and_boundaries():
    for n in (64, 1024, 4096):
        s = xp.sample_lines(n, br=8)
        assert s[0] == 0 and s[-1] == n - 1 and np.all(np.diff(s) > 0)
        assert set(range(8)) <= set(s) and set(range(n - 8, n)) <= set(s)
        assert {7, 8, 15, 16, n // 2 - 1, n // 2, n - 9} <= set(s)
        assert s.size <= n // 16 + 160
