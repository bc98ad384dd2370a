"""GPU tests of the item grouping of the pointwise host code (csrc/item_groups.h as start_impl, zernike_apply and the power
reductions use it): in a batch whose items share aperture records, start fields and wfe maps in an interleaved pattern
(item_groups_worker.scenario), every item's field and power equal, bit for bit, those of the same item run alone in a batch of
one with the same calls -- and those of the whole batch with the sharing switched off (PAOS_SHARE_START=0, PAOS_SHARE_WFE=0;
read once per process, so each runs in a process of its own).  64^2: grouping cannot depend on the grid size."""
import numpy as np
import pytest

import item_groups_worker as w

pytestmark = pytest.mark.gpu

NAMES = ["start_rows", "start_box", "start_power", "zernike_like", "zernike", "fused", "fused_power"]
_cache = {}


def _results(precision):
    """(the batch of six, [each item alone]) -- evaluated once per precision, read by every test."""
    if precision not in _cache:
        _cache[precision] = (w.run_calls(list(range(6)), precision), [w.run_calls([i], precision) for i in range(6)])
    return _cache[precision]


def _assert_items_equal(precision, name):
    batch, alone = _results(precision)
    for i in range(6):
        got, want = np.asarray(batch[name][i]), np.asarray(alone[i][name][0])
        assert np.array_equal(got, want, equal_nan=True), (precision, name, i)
        assert np.isfinite(got).any() and np.abs(np.nan_to_num(got)).max() > 0.0, (precision, name, i)


@pytest.mark.parametrize("name", NAMES)
def test_every_item_of_the_batch_equals_the_item_alone(name):
    _assert_items_equal("fp64", name)


def test_the_batch_is_not_six_copies():
    """What the comparison rests on: the stop scales one member of an aperture group and not the other, the two wavelengths of
    map P give two fields, and the sums of items with one record and stop flag are one number."""
    batch, _ = _results("fp64")
    assert not np.array_equal(batch["start_box"][0], batch["start_box"][4], equal_nan=True)  # (stop on / off)
    assert np.array_equal(batch["start_box"][0], batch["start_box"][2], equal_nan=True)
    assert not np.array_equal(batch["fused"][0], batch["fused"][2], equal_nan=True)  # (one map, two wavelengths)
    assert batch["start_power"][0] == batch["start_power"][2] and batch["fused_power"] == batch["start_power"]


def test_every_item_of_an_fp32_batch_equals_the_item_alone():
    for name in NAMES:
        _assert_items_equal("fp32", name)


@pytest.mark.parametrize("switch", ["PAOS_SHARE_START", "PAOS_SHARE_WFE"])
def test_sharing_switched_off_gives_the_same_bits(switch):
    """The same batch in a fresh process with the switch at 0 (forked from the server conftest.py started before this process
    touched the GPU): every item evaluates its own start field / wfe map, and nothing changes."""
    import multiprocessing as mp

    ctx = mp.get_context("forkserver")
    out = ctx.Queue()
    proc = ctx.Process(target=w.switched_worker, args=(out, switch))
    proc.start()
    try:
        status, detail = out.get(timeout=120)
        proc.join(timeout=60)
    finally:
        if proc.is_alive():  # (a worker that hangs must not stay behind with the GPU open)
            proc.kill()
            proc.join(timeout=30)
    assert proc.exitcode == 0
    assert status == "ok", detail
    assert detail == w.digests(_results("fp64")[0])


def test_a_full_ticket_ring_refuses_before_anything_is_launched():
    """64 tickets out: every entry point that hands out a ticket refuses with the one message, on the host, and leaves field and
    PSF as they were; the tickets are all still good, and with them fetched the ring serves again."""
    from paos_amd import _lib

    sc = w.scenario()
    one = [0]
    dev = _lib.DeviceFields(w.N, 1)
    try:
        dev.start(w.VALUE, _lib.SHAPE_ELLIPSE, sc["blocks"][one], sc["stops"][one])
        dev.psf_keep()
        field, psf, power = dev.download(0), dev.psf_fetch(0), dev.norm2()
        tickets = [dev.norm2_enqueue() for _ in range(_lib.NORM_SLOTS)]
        zargs = (sc["nmax"], sc["kdim"], sc["table"], sc["zb"][one])
        refused = [
            lambda: dev.norm2_enqueue(),
            lambda: dev.norm2_enqueue(sc["rows"][one]),
            lambda: dev.norm2_enqueue(sc["rows"][one], same_as=[0], live_cols=sc["cols"][one]),
            lambda: dev.psf_keep_power(),
            lambda: dev.start_zernike(2.0, _lib.SHAPE_ELLIPSE, sc["blocks"][one], sc["stops"][one], sc["rows"][one], sc["cols"][one],
                                      *zargs, power=True),
        ]
        for call in refused:
            with pytest.raises(_lib.PaosHipError, match=r"64 power reductions outstanding: fetch earlier tickets \(paos_norm2_fetch\) first"):
                call()
        assert np.array_equal(dev.download(0), field) and np.array_equal(dev.psf_fetch(0), psf)
        for t in tickets:
            assert np.array_equal(dev.norm2_fetch(t), power)
        assert np.array_equal(dev.norm2_fetch(dev.norm2_enqueue()), power)
    finally:
        dev.close()


# ---- the 8-row complex64 layout (N >= 2048, fp32) for the entry points no other test drives on it ----------------------
def test_pupil_weights_on_the_8_row_layout():
    """paos_pupil_aperture and paos_pupil_upload at 2048^2 fp32, read back through the Gram sums as
    test_gpu_parity.test_zernike_gram_full_size_properties reads them, exactly: the count is the number of pupil pixels inside
    the unit disk and piston^2 sums to it -- for an aperture off the centre and for a random pupil, which no other layout
    would count right."""
    from paos_amd import _lib
    from paos_amd.aperture import EllipticalAperture
    from paos_amd.planner import gram_polynomials, jacobi_recurrence, zernike_block
    from paos_amd.zernike import Zernike, norm_factors

    n, k, dx = 2048, 6, 1.0 / 512
    m, nn = Zernike.j2mn(k, "noll")
    norm = norm_factors(m, nn, True)
    block, nmax, kdim = zernike_block(m, nn, norm, np.zeros(k), dx, dx, 0.5, 1.0e-6)
    poly, table = gram_polynomials(m, nn, norm), jacobi_recurrence(nmax)
    ax = (np.arange(n) - n // 2) * dx
    disk = np.sqrt(ax[None, :] ** 2 + ax[:, None] ** 2) / 0.5 <= 1.0
    dev = _lib.DeviceFields(n, 1, precision="fp32")
    try:
        ap = EllipticalAperture((n / 2 + 37.25, n / 2 - 90.5), 300.0, 170.0, 0.0).block(obscuration=False)
        dev.pupil_aperture(_lib.SHAPE_ELLIPSE, [ap])
        sums, counts = dev.zernike_gram(nmax, kdim, table, [block], poly)
        mask = dev.aperture_mask(_lib.SHAPE_ELLIPSE, ap)
        assert counts[0] == np.count_nonzero((mask != 0) & disk) > 0 and sums[0][0] == counts[0]
        pupil = (np.random.default_rng(2048).random((n, n)) < 0.5).astype(np.float64)
        dev.pupil_upload(0, pupil)
        sums, counts = dev.zernike_gram(nmax, kdim, table, [block], poly)
        assert counts[0] == np.count_nonzero((pupil != 0) & disk) > 0 and sums[0][0] == counts[0]
    finally:
        dev.close()


def test_fused_start_on_the_8_row_layout():
    """paos_start_zernike_box at 2048^2 fp32 against the pair it replaces (paos_start_box + paos_zernike_like, each held to a
    long-double reference on this layout by test_gpu_ledger_xprec / test_gpu_pointwise_xprec), bit for bit as
    test_gpu_start_zernike compares them at 1024^2 fp64."""
    from paos_amd import _lib
    from paos_amd.aperture import EllipticalAperture
    from paos_amd.run import _Plans, _zernike_tables, zernike_tables

    n, h = 2048, 1024
    blocks = [EllipticalAperture((n / 2, n / 2), 200.0, 150.5, 0.0).block(obscuration=False)]
    rows, cols = [[h - 153, h + 154]], [[h - 203, h + 204]]
    m, nn, norm = zernike_tables(15, "standard", True)
    coef = np.random.default_rng(8).normal(0.0, 30e-9, 15)
    plans = _Plans([{"aperture": None, "stop": False, "phase_map": None,
                     "zernike": dict(m=m, n=nn, norm=norm, Z=coef, dx=1.0 / 400.0, dy=1.0 / 400.0, radius=0.375, wl=1.0e-6,
                                     origin="x", pupil=None)}])
    zs, nmax, kdim, table, build = _zernike_tables(plans)
    zb = build([z["Z"] for z in zs])
    nan = np.full((n, n), complex(np.nan, np.nan))
    a, b = _lib.DeviceFields(n, 1, precision="fp32"), _lib.DeviceFields(n, 1, precision="fp32")
    try:
        a.upload(0, nan)
        b.upload(0, nan)
        ticket = a.start_zernike(w.VALUE, _lib.SHAPE_ELLIPSE, blocks, [1.0], rows, cols, nmax, kdim, table, zb, power=True)
        b.start(w.VALUE, _lib.SHAPE_ELLIPSE, blocks, [1.0], write_rows=rows, write_cols=cols)
        want_ticket = b.norm2_enqueue(rows, same_as=[0], live_cols=cols)
        b.zernike(nmax, kdim, table, zb, same_as=[0])
        assert np.array_equal(a.norm2_fetch(ticket), b.norm2_fetch(want_ticket))
        fa, fb = a.download(0), b.download(0)
        assert np.array_equal(fa, fb, equal_nan=True)
        inside = fa[rows[0][0]:rows[0][1], cols[0][0]:cols[0][1]]
        assert np.isfinite(inside).all() and np.abs(inside).max() > 0.0 and np.isnan(fa[0, 0])
        assert np.ptp(np.angle(inside[np.abs(inside) > 0])) > 0.0  # (the surface is on the field)
    finally:
        a.close()
        b.close()
