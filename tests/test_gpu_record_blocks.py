"""Ellipse line records rendered by blocks of 64 lines per wave (paos_amd/csrc/pointwise.h: mask_blocks_kernel,
record_blocks.h) -- the default -- against the three things they must equal bit for bit: the records of four lines per wave
(PAOS_MASK_BLOCKS=0), those of the chunk scan (PAOS_MASK_SCAN=1) and the stand-alone aperture kernel's weights.  As in
tests/test_gpu_aperture_xprec.py the weights are read off a constant field after a mask pass whose transform is off, at
1024^2 complex128 (the smallest grid with line records), on both axes.  The switches are read at every call and the context
keys its kept record sets by the mode, so every mode renders.

Besides: a record window that starts in the middle of a block of 64 lines, three renderings in one launch, the counters
(paos_record_block_stats) and one lean SYN20 step under both modes."""
import os

import numpy as np
import pytest

from test_gpu_aperture_xprec import OFF, VALUE, _ell, _lib, _mask_pass, _pass_blocks, _rect, _same, _times, _weights

pytestmark = pytest.mark.gpu

N = 1024
ZOOM4 = 128.00000004  # the pupil's pixel radius at zoom 4
MODES = [("blocks", {}), ("four lines", {"PAOS_MASK_BLOCKS": "0"}), ("scan", {"PAOS_MASK_SCAN": "1"})]
SWITCHES = ("PAOS_MASK_BLOCKS", "PAOS_MASK_SCAN", "PAOS_MASK_PAIRS")


class _mode:
    def __init__(self, env):
        self.env = env

    def __enter__(self):
        for name in SWITCHES:
            assert os.environ.get(name) is None, name
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for name in self.env:
            os.environ.pop(name, None)


def _cases():
    lib = _lib()
    E, R = lib.SHAPE_ELLIPSE, lib.SHAPE_RECT
    disk = _ell(512.0, 512.0, ZOOM4, ZOOM4)
    return {
        "zoom-4 disks": [(E, disk), (E, _ell(512.5, 511.5, ZOOM4, ZOOM4)), (E, _ell(511.5, 512.5, ZOOM4, ZOOM4))],
        "flat ellipses": [(E, _ell(512.0, 512.0, 300.0, 40.0)), (E, _ell(512.0, 512.0, 40.0, 300.0)), (E, _ell(500.3, 530.7, 300.0, 40.0))],
        "a = b = 6": [(E, _ell(512.0, 512.0, 6.0, 6.0)), (E, _ell(300.5, 700.25, 6.0, 6.0))],
        "across two grid edges": [(E, _ell(80.0, 900.0, 200.0, 200.0)), (E, _ell(900.0, 80.0, 200.0, 200.0))],
        "obscurations": [(E, _ell(512.0, 512.0, ZOOM4, ZOOM4, 0.0, 1.0)), (E, _ell(512.0, 512.0, 300.0, 40.0, 0.0, 1.0)),
                         (R, _rect(512.3, 511.1, 300.7, 100.2)), (E, _ell(512.5, 511.5, 40.0, 30.0, 0.0, 1.0))],
        "a rectangle's obscuration beside ellipses": [(R, _rect(512.3, 511.1, 300.7, 100.2, obsc=1.0)), (E, disk),
                                                      (E, _ell(512.0, 512.0, 60.0, 60.0, 0.0, 1.0)), (E, _ell(512.0, 512.0, 40.0, 300.0))],
        "items 1 and 3 identical": [(E, disk), (E, _ell(520.0, 500.0, 100.0, 90.0)), (E, _ell(512.5, 511.5, ZOOM4, ZOOM4)),
                                    (E, _ell(520.0, 500.0, 100.0, 90.0))],
    }


@pytest.mark.parametrize("name", ["zoom-4 disks", "flat ellipses", "a = b = 6", "across two grid edges", "obscurations",
                                  "a rectangle's obscuration beside ellipses", "items 1 and 3 identical"])
def test_block_records_equal_every_other_renderer_and_the_aperture_kernel(name):
    items = _cases()[name]
    full = np.full((N, N), VALUE)
    dev = _lib().DeviceFields(N, len(items))
    try:
        ws = [_weights(dev, s, b) for s, b in items]
        blocks = _pass_blocks(items)
        for axis in (0, 1):
            got = {}
            for mode, env in MODES:
                with _mode(env):
                    dev.fill(VALUE)
                    dev.run_passes([_mask_pass(axis, "pre", OFF)], blocks)
                    got[mode] = [dev.download(i) for i in range(len(items))]
            for i, w in enumerate(ws):
                want = _times(full, w, "fp64")
                for mode, _ in MODES:
                    _same(got[mode][i], want, f"{name}, axis {axis}, {mode}, item {i} {items[i]}: against the aperture kernel")
                    _same(got[mode][i], got["scan"][i], f"{name}, axis {axis}, {mode} against the scan, item {i}")
    finally:
        dev.close()


@pytest.mark.parametrize("axis", [0, 1])
def test_a_record_window_that_starts_inside_a_block(axis):
    """The zoom-4 disk behind an entry box of rows and columns [372, 660): the records are rendered for the live lines
    only, a window whose start is a multiple of the layout's block height and not of 64 (372 = 5 * 64 + 52).  What lies
    outside the box stands for zeros and holds NaN.  Pruning on and off: equal outputs, all finite, the weights inside."""
    lo, hi = 372, 660
    assert lo % 4 == 0 and lo % 64 != 0 and hi % 64 != 0
    items = [(_lib().SHAPE_ELLIPSE, _ell(512.0, 512.0, ZOOM4, ZOOM4)), (_lib().SHAPE_ELLIPSE, _ell(512.5, 511.5, ZOOM4, ZOOM4))]
    field = np.full((N, N), complex(np.nan, np.nan))
    field[lo:hi, lo:hi] = VALUE
    box = np.array([[lo, hi]] * len(items), dtype=np.float64)
    dev = _lib().DeviceFields(N, len(items))
    try:
        ws = [_weights(dev, s, b) for s, b in items]
        out = {}
        for prune in (True, False):
            dev.set_pruning(prune)
            for i in range(len(items)):
                dev.upload(i, field)
            dev.run_passes([_mask_pass(axis, "pre", OFF)], _pass_blocks(items), live_rows=box, rows_stale=True, live_cols=box)
            out[prune] = [dev.download(i) for i in range(len(items))]
        dev.set_pruning(True)
        for i, w in enumerate(ws):
            assert np.isfinite(out[True][i].real).all() and np.isfinite(out[True][i].imag).all(), i
            _same(out[True][i], out[False][i], f"axis {axis} item {i}: pruning on against off")
            want = np.zeros((N, N), dtype=np.complex128)
            want[lo:hi, lo:hi] = _times(np.full((N, N), VALUE), w, "fp64")[lo:hi, lo:hi]
            _same(out[True][i], want, f"axis {axis} item {i}: the weights inside the box, zeros outside")
    finally:
        dev.close()


def test_three_renderings_in_one_launch():
    """One program of three mask passes (the renderings of a program go out in one launch, one job each) against the same
    three as three programs: equal fields, and both the product of the three weight maps in order."""
    lib = _lib()
    E = lib.SHAPE_ELLIPSE
    sets = [[(E, _ell(512.0, 512.0, ZOOM4, ZOOM4)), (E, _ell(300.0, 400.0, 250.0, 90.0))],
            [(E, _ell(512.5, 511.5, 200.0, 210.0)), (E, _ell(330.0, 420.5, 6.0, 6.0))],
            [(E, _ell(500.0, 520.0, 40.0, 300.0)), (E, _ell(80.0, 900.0, 200.0, 200.0, 0.0, 1.0))]]
    axes = [0, 1, 0]
    nb = 2
    blocks = np.zeros((7, nb, 5))  # three apertures of two block sets each, and an all-zero control block: transform off
    for k, items in enumerate(sets):
        blocks[2 * k:2 * k + 2] = _pass_blocks(items)[0:2]
    off = 6

    def mask_pass(k):
        return {"axis": axes[k], "fft1": off, "fft2": -1, "pre": [(lib.PW_MASK, 0, 2 * k)], "mid": [], "post": []}

    dev = lib.DeviceFields(N, nb)
    try:
        ws = [[_weights(dev, s, b) for s, b in items] for items in sets]
        _, rendered = dev.record_set_stats()
        dev.fill(VALUE)
        dev.run_passes([mask_pass(0), mask_pass(1), mask_pass(2)], blocks)
        _, rendered2 = dev.record_set_stats()
        assert rendered2 == rendered + 3
        together = [dev.download(i) for i in range(nb)]
        with _mode({"PAOS_MASK_BLOCKS": "0"}):  # (another mode, so that the three are rendered again)
            dev.fill(VALUE)
            for k in range(3):
                dev.run_passes([mask_pass(k)], blocks)
            apart = [dev.download(i) for i in range(nb)]
        for i in range(nb):
            want = np.full((N, N), VALUE)
            for k in range(3):
                want = _times(want, ws[k][i], "fp64")
            _same(together[i], apart[i], f"item {i}: one program against three")
            _same(together[i], want, f"item {i}: the product of the three weight maps")
    finally:
        dev.close()


def _render_once(dev, items, axis=0):
    before = dev.record_block_stats()
    dev.fill(VALUE)
    dev.run_passes([_mask_pass(axis, "pre", OFF)], _pass_blocks(items))
    after = dev.record_block_stats()
    return tuple(b - a for a, b in zip(before, after))


def test_counters():
    """The zoom-4 disk: its bounding box has 257 lines (384 .. 640), of which the windows of 8 pixels alone fit 251 on the
    CPU; at least 95 % must be rendered by blocks, and fewer than a third of their window pixels -- 16 per line where the
    8-pixel windows fit, the fewest a line can have -- may need the exact overlap (3.6 of 16 on the CPU).  a = b = 6: no
    window fits a box of 13 pixels, every line is handed over.  Four lines per wave: the counters stand still."""
    lib = _lib()
    dev = lib.DeviceFields(N, 1)
    try:
        assert dev.record_block_stats() == (0, 0, 0)
        block, handed, undecided = _render_once(dev, [(lib.SHAPE_ELLIPSE, _ell(512.0, 512.0, ZOOM4, ZOOM4))])
        print(f"zoom-4 disk: {block} lines by blocks, {handed} handed over, {undecided} undecided pixels")
        assert block + handed == 257 and block >= 0.95 * 257, (block, handed)
        assert 0 < undecided < block * 16 / 3, (undecided, block)
        block, handed, undecided = _render_once(dev, [(lib.SHAPE_ELLIPSE, _ell(512.0, 512.0, 6.0, 6.0))], axis=1)
        assert (block, handed, undecided) == (0, 13, 0)
        with _mode({"PAOS_MASK_BLOCKS": "0"}):
            assert _render_once(dev, [(lib.SHAPE_ELLIPSE, _ell(512.0, 512.0, 100.0, 100.0))]) == (0, 0, 0)
    finally:
        dev.close()


def test_a_lean_syn20_step_is_the_same_under_both_modes():
    """One lean SYN20 step at 1024^2 x 4 (bench.py's call) with the records rendered by blocks and four lines per wave:
    PSFs and the powers of every saved surface equal bit for bit, and the blocks did render."""
    from paos_amd.chains import syn20_chain, syn20_wavelength
    from paos_amd.run import run_batch

    wls = [syn20_wavelength(k) for k in (0, 170, 333, 511)]
    out = {}
    for mode, env in MODES[:2]:
        dev = _lib().DeviceFields(N, len(wls))
        try:
            with _mode(env):
                res = run_batch(1.0, wls, N, 4, {"us": 0.0, "ut": 0.0}, [syn20_chain() for _ in wls], outputs=(), dev=dev, keep_psf=True)
                out[mode] = (res, [dev.psf_fetch(i) for i in range(len(wls))], dev.record_block_stats())
        finally:
            dev.close()
    (res_a, psf_a, stats_a), (res_b, psf_b, stats_b) = out["blocks"], out["four lines"]
    assert stats_a[0] > 20 * stats_a[1] and stats_a[2] > 0 and stats_b == (0, 0, 0), (stats_a, stats_b)
    for i in range(len(wls)):
        assert sorted(res_a[i]) == sorted(res_b[i])
        for k in res_a[i]:
            assert res_a[i][k]["power"] == res_b[i][k]["power"], (i, k)
        assert np.isfinite(psf_a[i]).all() and np.array_equal(psf_a[i], psf_b[i]), i
