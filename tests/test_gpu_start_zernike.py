"""GPU tests of the fused first-field write (paos_start_zernike_box, csrc/pointwise.h: zernike_start_write_kernel): a lean
walk whose start is followed by a Zernike surface stores the field once, with the phase on it, instead of storing the masked
constant (paos_start_box) and rewriting it (paos_zernike_like).  Everything is compared bit for bit with the pair of calls,
which ``PAOS_FUSE_START=0`` (run.FUSE_START) forces.  1024^2 is the smallest grid of the production pass kernels."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ON_AXIS = {"us": 0.0, "ut": 0.0}
N = 1024


def _poison(dev, nb):
    for i in range(nb):
        dev.upload(i, np.full((dev.n, dev.n), complex(np.nan, np.nan)))


def _lean(dev, wls, chains, fused, stats=None, poison=True):
    """One lean step (bench.py's call) on ``dev`` -- on a buffer full of NaN -- with the fused start on or off; returns
    (results, [PSF per item])."""
    import paos_amd.run as prun
    from paos_amd.run import run_batch

    assert prun.FUSE_START is True
    if poison:
        _poison(dev, len(wls))
    prun.FUSE_START = fused
    try:
        res = run_batch(1.0, wls, dev.n, 4, ON_AXIS, chains, outputs=(), dev=dev, keep_psf=True, stats=stats)
    finally:
        prun.FUSE_START = True
    return res, [dev.psf_fetch(i) for i in range(len(wls))]


def _assert_identical(a, b, nb):
    (res_a, psf_a), (res_b, psf_b) = a, b
    for i in range(nb):
        assert sorted(res_a[i]) == sorted(res_b[i])
        for k in res_a[i]:  # every saved surface: the first (the start field's own power) and the image plane
            assert res_a[i][k]["power"] == res_b[i][k]["power"], (i, k, res_a[i][k]["power"], res_b[i][k]["power"])
        assert np.isfinite(psf_a[i]).all() and np.array_equal(psf_a[i], psf_b[i]), i


def test_sweep_batch_fused_against_pair():
    """SYN20, three sweep wavelengths (one start group, one wfe map): PSFs and the powers of both saved surfaces -- the first
    is the start field's own power, which the fused call sums from the weights because that field is never stored -- equal
    those of the pair bit for bit, on a poisoned buffer."""
    from paos_amd import _lib
    from paos_amd.chains import syn20_chain, syn20_wavelength

    wls = [syn20_wavelength(k) for k in (7, 333, 511)]
    chains = [syn20_chain() for _ in wls]
    dev = _lib.DeviceFields(N, len(wls))
    try:
        s_on, s_off = {}, {}
        fused = _lean(dev, wls, chains, True, s_on)
        pair = _lean(dev, wls, chains, False, s_off)
        assert s_on["fused_start"] == 1 and s_off["fused_start"] == 0
        assert 1 in fused[0][0] and fused[0][0][1]["power"] > 0.0
        _assert_identical(fused, pair, len(wls))
    finally:
        dev.close()


def test_sweep_of_nine_wavelengths_fused_against_pair():
    """SYN20, nine sweep wavelengths: one start group with one wfe map, so the fused kernel turns eight members at a time
    and then one -- the eight-wide loop and its tail, which groups of three and four never reach."""
    from paos_amd import _lib
    from paos_amd.chains import syn20_chain, syn20_wavelength

    wls = [syn20_wavelength(k) for k in (3, 59, 120, 181, 242, 303, 364, 425, 508)]
    chains = [syn20_chain() for _ in wls]
    dev = _lib.DeviceFields(N, len(wls))
    try:
        s_on = {}
        fused = _lean(dev, wls, chains, True, s_on)
        pair = _lean(dev, wls, chains, False)
        assert s_on["fused_start"] == 1
        _assert_identical(fused, pair, len(wls))
        assert not np.array_equal(fused[1][0], fused[1][8])  # (every member at its own wavelength)
    finally:
        dev.close()


def test_monte_carlo_batch_fused_against_pair():
    """Three items of one wavelength with their own coefficient vectors (one start group, three wfe maps: the weight is
    evaluated once per pixel, the polynomials once per item), and a fourth item that repeats the first's coefficients at
    another wavelength (a sub-group of two)."""
    from paos_amd import _lib
    from paos_amd.chains import syn20_chain, syn20_coefficients, syn20_wavelength

    wls = [syn20_wavelength(40)] * 3 + [syn20_wavelength(41)]
    chains = [syn20_chain(syn20_coefficients(rng_seed=s)) for s in (11, 12, 13, 11)]
    dev = _lib.DeviceFields(N, len(wls))
    try:
        s_on = {}
        fused = _lean(dev, wls, chains, True, s_on)
        pair = _lean(dev, wls, chains, False)
        assert s_on["fused_start"] == 1
        _assert_identical(fused, pair, len(wls))
        assert not np.array_equal(fused[1][0], fused[1][1])  # (the maps do differ)
    finally:
        dev.close()


def test_two_walked_steps_on_one_context_equal_a_fresh_context():
    """Two consecutive walked steps on one context (the second finds the start's power sums kept by the first: the key of
    paos_start_box, unchanged) against the second step alone on a fresh context, and against the pair on a third."""
    from paos_amd import _lib
    from paos_amd.chains import syn20_chain, syn20_wavelength

    nb = 3
    chains = [syn20_chain() for _ in range(nb)]
    wl_of = lambda g: [syn20_wavelength((g * nb + i) % 512) for i in range(nb)]  # noqa: E731
    dev = _lib.DeviceFields(N, nb)
    try:
        _lean(dev, wl_of(0), chains, True)
        stats = {}
        second = _lean(dev, wl_of(1), chains, True, stats, poison=False)
        assert stats["fused_start"] == 1
    finally:
        dev.close()
    for fused in (True, False):
        fresh = _lib.DeviceFields(N, nb)
        try:
            _assert_identical(second, _lean(fresh, wl_of(1), chains, fused), nb)
        finally:
            fresh.close()


def test_fallbacks_are_taken():
    """The pair runs, and the results are the parent path's, when the Zernike surface carries an elliptical orthonormal pupil,
    when a stop sits on the Zernike surface (it needs the field first), and in a call that is not lean
    (``outputs=("amplitude",)``); ``stats`` shows that the fused call was not made.  (A saved first surface -- SYN20's -- does
    not force the pair: its power is summed from the weights, see test_sweep_batch_fused_against_pair.)"""
    import paos_amd.run as prun
    from paos_amd import _lib
    from paos_amd.chains import syn20_chain, syn20_orthonorm_chain, syn20_wavelength
    from paos_amd.run import run_batch

    wls = [syn20_wavelength(k) for k in (3, 200)]
    stop_chain = syn20_chain()
    stop_chain[2] = dict(stop_chain[2], is_stop=True)
    dev = _lib.DeviceFields(N, len(wls))
    try:
        for chain in (syn20_orthonorm_chain(), stop_chain):
            chains = [chain for _ in wls]
            stats = {}
            on = _lean(dev, wls, chains, True, stats)
            assert stats["fused_start"] == 0
            _assert_identical(on, _lean(dev, wls, chains, False), len(wls))
        chains = [syn20_chain() for _ in wls]
        stats = {}
        got = run_batch(1.0, wls, N, 4, ON_AXIS, chains, outputs=("amplitude",), dev=dev, stats=stats)
        assert stats["fused_start"] == 0
        prun.FUSE_START = False
        try:
            want = run_batch(1.0, wls, N, 4, ON_AXIS, chains, outputs=("amplitude",), dev=dev)
        finally:
            prun.FUSE_START = True
        for i in range(len(wls)):
            for k in want[i]:
                assert np.array_equal(got[i][k]["amplitude"], want[i][k]["amplitude"]) and got[i][k]["power"] == want[i][k]["power"]
    finally:
        dev.close()


def test_the_fused_field_itself_equals_the_pair_inside_the_box():
    """The library call alone (no walk): paos_start_zernike_box against paos_start_box + paos_zernike_like on two poisoned
    contexts -- the stored fields are equal inside the box, still NaN outside it, and the ticket brings the start field's
    power as paos_norm2_enqueue_box sums it.  Items 0-1 share everything but the wavelength, item 2 has its own
    coefficients, item 3 its own (smaller, elliptical) aperture, Zernike radius and no stop."""
    from paos_amd import _lib
    from paos_amd.aperture import EllipticalAperture
    from paos_amd.run import _Plans, _zernike_tables, zernike_tables

    nb, n = 4, N
    rng = np.random.default_rng(5)
    blocks = [EllipticalAperture((n / 2, n / 2), a, b, 0.0).block(obscuration=False)
              for a, b in ((120.0, 120.0),) * 3 + ((90.5, 70.25),)]
    stops = [1.0, 1.0, 1.0, 0.0]
    rows = [[n // 2 - 123, n // 2 + 124]] * 3 + [[n // 2 - 73, n // 2 + 74]]
    cols = [[n // 2 - 123, n // 2 + 124]] * 3 + [[n // 2 - 93, n // 2 + 94]]
    m, nn, norm = zernike_tables(15, "standard", True)

    def zplan(coef, wl, radius):
        return {"aperture": None, "stop": False, "phase_map": None,
                "zernike": dict(m=m, n=nn, norm=norm, Z=coef, dx=1.0 / 240.0, dy=1.0 / 240.0, radius=radius, wl=wl, origin="x",
                                pupil=None)}

    c0, c2, c3 = (rng.normal(0.0, 30e-9, 15) for _ in range(3))
    plans = _Plans([zplan(c0, 1.0e-6, 0.5), zplan(c0, 1.3e-6, 0.5), zplan(c2, 1.0e-6, 0.5), zplan(c3, 0.9e-6, 0.25)])
    zs, nmax, kdim, table, build = _zernike_tables(plans)
    zb = build([z["Z"] for z in zs])
    a, b = _lib.DeviceFields(n, nb), _lib.DeviceFields(n, nb)
    try:
        _poison(a, nb)
        _poison(b, nb)
        ticket = a.start_zernike(1.0, _lib.SHAPE_ELLIPSE, blocks, stops, rows, cols, nmax, kdim, table, zb, power=True)
        b.start(1.0, _lib.SHAPE_ELLIPSE, blocks, stops, write_rows=rows, write_cols=cols)
        want_ticket = b.norm2_enqueue(rows, same_as=[0, 0, 0, 3], live_cols=cols)
        b.zernike(nmax, kdim, table, zb, same_as=[0, 0, 0, 3])
        assert np.array_equal(a.norm2_fetch(ticket), b.norm2_fetch(want_ticket))
        for i in range(nb):
            fa, fb = a.download(i, _lib.WHAT_FIELD), b.download(i, _lib.WHAT_FIELD)
            assert np.array_equal(fa, fb, equal_nan=True), i
            inside = fa[rows[i][0]:rows[i][1], cols[i][0]:cols[i][1]]
            assert np.isfinite(inside).all() and np.abs(inside).max() > 0.0 and np.isnan(fa[0, 0])
        assert not np.array_equal(a.download(0, _lib.WHAT_FIELD), a.download(1, _lib.WHAT_FIELD), equal_nan=True)
    finally:
        a.close()
        b.close()
