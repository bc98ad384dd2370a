"""The narrow-window variant of the central-half builds of the 4096^2 complex128 pass kernel (frugal_pass.h: CH = 2;
frugal_launch.h: frugal_launch; pass_program.h: pick_narrow): a launch whose first pass loads, and whose last pass stores,
positions of [5 N / 16, 11 N / 16) = [1280, 2816) only neither loads, computes nor tests anything outside -- per thread the
elements k = 5 .. 10 of 16.

On the helpers of test_gpu_central_half.py.  Every case runs the same program three times through the C ABI: on a context
with the variant switched on (PAOS_NARROW_WINDOWS=1 when it is created), on one with it switched off (=0: the central-half
kernels) and on one with the pruning off altogether, whose fields hold real zeros outside the windows.  The three must agree
as numbers (np.array_equal, powers equal), the per-context counter (paos_narrow_window_stats) says which kernel the first
launch took, and sampled lines are held to the long-double restatement of xprec_np at its bound.  Buffers hold NaN outside
the windows' 8 x 8 blocks; line windows are 64 lines, batches 2 or 3 items.

What a launch stores is what the next pass reads: as in test_single_table_pass_on_the_central_half_build, a following pass
along the other axis carries an aperture that keeps a window of its lines (``TRIM``).  The planner widens an aperture's
bounding box by one pixel and rounds every window outward to whole block rows of the layout (4 lines), so the windows named
here are what the launch is given after that rounding: "loads (1279, 2816)" reach the kernel as [1276, 2816), an aperture
whose box begins at 1279 trims the stores to [1276, 2816).  (The rule itself, to the position: test_narrow_windows_host.py.)"""
import ctypes
import os

import numpy as np
import pytest

import test_gpu_central_half as tc
import test_gpu_xprec as tx
import xprec_np as xp

pytestmark = pytest.mark.gpu

N, L0, L1 = tc.N, tc.L0, tc.L1
LO, HI = 5 * N // 16, 11 * N // 16  # 1280, 2816

# (centre, extent) of the trimming aperture along the lines of the pass that carries it -> the window [floor(c - e + 0.5) - 1,
# ceil(c + e + 0.5) + 1), rounded outward to multiples of 4, that the launch in front of it stores
TRIM = {
    (1280, 2816): (2047.5, 766.9),   # 1280 .. 2816: its outermost pixels, 1281 and 2814, still carry weight
    (1532, 2564): (2047.5, 514.9),   # the window of a chain step
    (1276, 2816): (2047.0, 767.4),   # the box begins at 1279
}
ACROSS = 700.0  # the aperture's extent along the other direction: wider than the 64 live lines of the launch in front


def _device(lib, batch, narrow, pruning=True):
    """A context that read PAOS_NARROW_WINDOWS = ``narrow`` when it was created (the central-half builds stay on)."""
    old = os.environ.get("PAOS_NARROW_WINDOWS")
    os.environ["PAOS_NARROW_WINDOWS"] = "1" if narrow else "0"
    try:
        dev = tc._device(lib, batch, True, pruning)
    finally:
        if old is None:
            del os.environ["PAOS_NARROW_WINDOWS"]
        else:
            os.environ["PAOS_NARROW_WINDOWS"] = old
    return dev


def _narrow_stats(dev):
    """(narrow, other): frugal pass launches on the CH = 2 kernels / on any other, since the context was created."""
    narrow, other = ctypes.c_ulonglong(0), ctypes.c_ulonglong(0)
    dev._check(dev._lib.paos_narrow_window_stats(dev._ctx, ctypes.byref(narrow), ctypes.byref(other)), "paos_narrow_window_stats")
    return int(narrow.value), int(other.value)


def _run(lib, fields, passes, blocks, narrow, pruning=True, **kw):
    """-> (outputs, launch tags, powers or None, (central, plain), (narrow, other))."""
    dev = _device(lib, len(fields), narrow, pruning)
    try:
        for i, f in enumerate(fields):
            dev.upload(i, f)
        dev.profile_begin(lib.KERNEL_PASS_ANY, max_launches=64)
        ticket = dev.run_passes(passes, blocks, **kw)
        power = None if ticket is None else dev.norm2_fetch(ticket)
        _, tags = dev.profile_end_launches()
        out = [dev.download(i) for i in range(len(fields))]
        return out, tags, power, dev.central_half_stats(), _narrow_stats(dev)
    finally:
        dev.close()


def _three_ways(lib, axis, seeds, windows, passes, blocks, want_narrow, want_central=True):
    """Run the program on the three contexts and hold them to each other; returns the outputs of the first and the
    zero-filled inputs."""
    kw = tc._windows_kw(axis, windows)
    stale = [tc._boxed(s, axis, w) if w is not None else tx._field(N, s) for s, w in zip(seeds, windows)]
    on, tags, p_on, (central, plain), (narrow, other) = _run(lib, stale, passes, blocks, True, **kw)
    assert central + plain == tags.size and narrow + other == tags.size, (central, plain, narrow, other, tags)
    assert central == (1 if want_central else 0) and narrow == (1 if want_narrow else 0), (central, narrow, tags)
    assert tags[0] & 2, tags  # the first launch skips loads; it is the one the counters speak of
    if want_narrow:
        assert tags[0] & 4, tags  # ... and stores
    off, tags_off, p_off, (central_off, _), (narrow_off, _) = _run(lib, stale, passes, blocks, False, **kw)
    assert narrow_off == 0 and central_off == central and np.array_equal(tags, tags_off), (narrow_off, central_off, tags, tags_off)
    del stale
    zeros = [tc._boxed(s, axis, w, stale=False) if w is not None else tx._field(N, s) for s, w in zip(seeds, windows)]
    dense, _, p_dense, _, (narrow_dense, _) = _run(lib, zeros, passes, blocks, True, pruning=False)
    assert narrow_dense == 0, "a context without pruning plans no windows"
    for i, w in enumerate(windows):
        if w is not None:
            assert np.isfinite(on[i]).all(), f"item {i} window {w}: stale data reached the output"
        assert np.array_equal(on[i], off[i]), f"item {i} window {w}: narrow windows != central-half kernel"
        assert np.array_equal(on[i], dense[i]), f"item {i} window {w}: narrow windows != pruning off"
        if p_on is not None:
            assert p_on[i] == p_off[i] == p_dense[i], (i, p_on[i], p_off[i], p_dense[i])
    return on, zeros


def _program(lib, axis, count, batch=2, stores=(1280, 2816), last_nfft=2, mid_phase=True, fft1_off_item=None, last_off_item=None,
             aperture=None):
    """``count`` passes of one row / column chain (test_gpu_central_half._chain) and, behind them, a pass along the other axis
    whose aperture trims what the chain's launch stores to ``stores`` (None: no such pass, whole lines are stored).
    ``last_nfft`` = 1: the chain's last pass has one transform; ``mid_phase`` = False: no phase in its second slot;
    ``last_off_item``: that item's last transform is switched off.  -> passes, blocks, {block: aperture parameters}."""
    passes, blocks, mask_block = tc._chain(lib, axis, count, batch=batch, fft1_off_item=fft1_off_item, aperture=aperture)
    apertures = {} if mask_block is None else {mask_block: aperture}
    last = dict(passes[count - 1])
    if not mid_phase:
        last["mid"] = [op for op in last["mid"] if op[0] != lib.PW_QPHASE_NATURAL]
    if last_nfft == 1:
        del last["fft2"]
    extra = np.zeros((3, batch, 5))
    nb = blocks.shape[0]
    if last_off_item is not None:
        ctl = "fft2" if last_nfft == 2 else "fft1"
        extra[0] = blocks[last[ctl]]
        extra[0, last_off_item, 0] = 0.0
        last[ctl] = nb
    passes[count - 1] = last
    if stores is not None:
        c, e = TRIM[stores]
        # (aperture parameters: enable, x centre, y centre, x extent, y extent; a row pass's lines are counted along y)
        ap = [[1.0, N / 2, c, ACROSS, e] if axis == 1 else [1.0, c, N / 2, e, ACROSS] for _ in range(2)]
        for i in range(2):
            extra[1, i] = ap[i]
            extra[2, i] = [0.0, 0.0, 32.0, lib.SHAPE_ELLIPSE, 0.0]
        passes = passes + [{"axis": 1 - axis, "fft1": 0, "pre": [(lib.PW_MASK, 0, nb + 1)]}]
        apertures[nb + 1] = ap
    return passes, np.concatenate([blocks, extra]), apertures


def _masks(lib, apertures):
    masks = {}
    for block, ap in apertures.items():
        masks.update(tc._masks(lib, block, ap))
    return masks or None


def _check(lib, got, zeros, passes, blocks, apertures, axis, items, n_fft, k_phase, what):
    """Hold the outputs to the long-double restatement.  Without a trimming pass: the sampled live lines of the chain.  With
    one: the chain on its live lines, then the trimming pass on lines of the other axis that its aperture leaves non-zero --
    the first, the last and ten in between --, as test_single_table_pass_on_the_central_half_build does."""
    masks = _masks(lib, apertures)
    trimmed = passes[-1]["axis"] != axis
    if not trimmed:
        tc._check_lines(got, zeros, passes, blocks, axis, items, n_fft, k_phase, what, masks=masks)
        return
    other, trim_block = 1 - axis, passes[-1]["pre"][0][2]
    live = np.arange(L0, L1)
    for i in items:
        m = masks[trim_block][i]
        nonzero = np.nonzero(m.any(axis=1 if other == 0 else 0))[0]
        kept = np.unique(np.concatenate([nonzero[:: max(1, nonzero.size // 10)], nonzero[-1:]]))
        z = zeros[i]
        part = z[live] if axis == 0 else z[:, live]
        sel = {"rows": live} if axis == 0 else {"cols": live}
        refs = []
        for dt in (xp.LD, np.complex128):
            mid = xp.run_item(part, passes[:-1], blocks, i, N, masks=masks, dtype=dt, **sel)
            if other == 0:  # mid: [every row, live columns] -> rows `kept`, every column
                u = np.zeros((kept.size, N), dtype=dt)
                u[:, live] = mid[kept]
                refs.append(xp.run_item(u, passes[-1:], blocks, i, N, rows=kept, masks=masks, dtype=dt))
            else:           # mid: [live rows, every column] -> every row, columns `kept`
                u = np.zeros((N, kept.size), dtype=dt)
                u[live] = mid[:, kept]
                refs.append(xp.run_item(u, passes[-1:], blocks, i, N, cols=kept, masks=masks, dtype=dt))
        g = got[i][kept] if other == 0 else got[i][:, kept]
        dead = np.setdiff1d(np.arange(N), nonzero)
        assert not np.any(got[i][dead] if other == 0 else got[i][:, dead]), "lines the aperture zeroes"
        print("\nXPREC " + xp.check(g, refs[0], refs[1], other, N, n_fft + 1, k_phase, "fp64", f"{what} item {i}")[4])


# ---- windows that must take the narrow variant ------------------------------------------------------------------------------
NARROW = [((1280, 2816), (1280, 2816)), ((1532, 2564), (1532, 2564)), ((1280, 1281), (1280, 2816)), ((2815, 2816), (1280, 2816)),
          ((1535, 1537), (1280, 2816)), ((2559, 2561), (1280, 2816))]


@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("loads,stores", NARROW, ids=[f"{a}-{b}" for (a, b), _ in NARROW])
def test_windows_inside_take_the_narrow_variant(loads, stores, axis):
    """A fused two-pass launch that loads and stores exactly [1280, 2816) -- all of k = 5 .. 10 --, the quarter [1532, 2564) of a
    chain step, the single positions 1280 and 2815, and (1535, 1537) / (2559, 2561), which straddle one thread's k = 5 / 6 and
    k = 9 / 10 boundaries (positions 1536 and 2560)."""
    lib = tx._lib()
    passes, blocks, apertures = _program(lib, axis, 2, stores=stores)
    on, zeros = _three_ways(lib, axis, (3, 4), [loads, loads], passes, blocks, True)
    _check(lib, on, zeros, passes, blocks, apertures, axis, (0, 1), 4, 4, f"narrow windows, loads {loads} stores {stores} axis {axis}")


# ---- windows that must stay on the central-half kernel ---------------------------------------------------------------------
REFUSED = {
    "loads-1279-2816": ([(1279, 2816)] * 2, (1280, 2816)),
    "loads-1280-2817": ([(1280, 2817)] * 2, (1280, 2816)),
    "stores-1279-2816": ([(1532, 2564)] * 2, (1276, 2816)),
    "stores-whole-lines": ([(1532, 2564)] * 2, None),
    "one-item-outside": ([(1532, 2564), (1024, 1536), None], (1280, 2816)),
}


@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("case", list(REFUSED))
def test_a_window_outside_keeps_the_central_half_kernel(case, axis):
    """One position beyond either edge of the loads, stores that begin at 1279 behind narrow loads, stores of whole lines, or
    one item of the batch outside [1280, 2816) (it loads [1024, 1536): still the central half) send the whole launch to the
    CH = 1 kernel, with the same answers; the disabled third item comes back bit for bit."""
    lib = tx._lib()
    windows, stores = REFUSED[case]
    batch = len(windows)
    passes, blocks, apertures = _program(lib, axis, 2, batch=batch, stores=stores)
    on, zeros = _three_ways(lib, axis, (3, 4, 5)[:batch], windows, passes, blocks, False)
    if batch == 3:
        assert np.array_equal(on[2], tx._field(N, 5)), "the disabled item changed"
    _check(lib, on, zeros, passes, blocks, apertures, axis, (0, 1), 4, 4, f"refused {case} axis {axis}")


# ---- programs -----------------------------------------------------------------------------------------------------------------
# the aperture of the row cases: its partial runs on the sampled rows sit at columns 1535 .. 1537 and 2559 .. 2561, the
# boundaries between a thread's elements k = 5 / 6 (position 1536) and k = 9 / 10 (position 2560)
APERTURE = [[1.0, 2048.3, 2048.2, 512.0, 900.0], [1.0, 2047.6, 2050.0, 512.4, 1100.0]]
# passes of the chain, transforms of its last pass -> the LONG build of the launch
PROGRAMS = {"two": (2, 2), "two-one": (2, 1), "three": (3, 2), "three-one": (3, 1)}


@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("program", list(PROGRAMS))
def test_fused_programs_on_the_narrow_variant(program, axis):
    """Two and three passes in one launch, the last of them with two transforms (LONG = 2, 4) or with one (LONG = 1, 3: the
    launch ends on a slot, not on a transform)."""
    lib = tx._lib()
    count, last_nfft = PROGRAMS[program]
    passes, blocks, apertures = _program(lib, axis, count, stores=(1532, 2564), last_nfft=last_nfft)
    on, zeros = _three_ways(lib, axis, (6, 7), [(1532, 2564)] * 2, passes, blocks, True)
    n_fft = 2 * count - (2 - last_nfft)
    _check(lib, on, zeros, passes, blocks, apertures, axis, (0, 1), n_fft, 2 * count, f"{program} axis {axis}")


@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("shape", ["two-transforms", "one-transform", "no-mid-phase"])
def test_single_table_pass_on_the_narrow_variant(shape, axis):
    """The one-line single table passes: phases in both slots around two transforms, around one, and a second slot without a
    phase (KMID = 0)."""
    lib = tx._lib()
    passes, blocks, apertures = _program(lib, axis, 1, stores=(1532, 2564), last_nfft=1 if shape == "one-transform" else 2,
                                         mid_phase=shape != "no-mid-phase")
    on, zeros = _three_ways(lib, axis, (10, 11), [(1532, 2564)] * 2, passes, blocks, True)
    n_fft = 1 if shape == "one-transform" else 2
    _check(lib, on, zeros, passes, blocks, apertures, axis, (0, 1), n_fft, 2, f"single table pass, {shape}, axis {axis}")


@pytest.mark.parametrize("count", [1, 2], ids=["single", "two"])
def test_rows_with_an_aperture_in_the_trimmed_slot(count):
    """An aperture of the launch's own rides in the trimmed slot, in front of the first phase, with its partial runs at the
    k = 5 / 6 and k = 9 / 10 boundaries (APERTURE); it clips the loads of [1280, 2816) to its bounding box."""
    lib = tx._lib()
    axis = 0
    passes, blocks, apertures = _program(lib, axis, count, stores=(1532, 2564), aperture=APERTURE)
    on, zeros = _three_ways(lib, axis, (12, 13), [(1280, 2816)] * 2, passes, blocks, True)
    _check(lib, on, zeros, passes, blocks, apertures, axis, (0, 1), 2 * count, 2 * count, f"rows with an aperture, {count} passes")


@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("which", ["first-off", "last-off"])
def test_an_item_with_a_transform_switched_off(which, axis):
    """An item whose first transform is off beside one with it on; an item whose last transform is off -- it stores the
    elements k = 5 .. 10 as the slot in front left them."""
    lib = tx._lib()
    passes, blocks, apertures = _program(lib, axis, 2, stores=(1280, 2816), fft1_off_item=1 if which == "first-off" else None,
                                         last_off_item=1 if which == "last-off" else None)
    on, zeros = _three_ways(lib, axis, (8, 9), [(1532, 2564)] * 2, passes, blocks, True)
    _check(lib, on, zeros, passes, blocks, apertures, axis, (0, 1), 4, 4, f"{which} axis {axis}")


# ---- SYN20 end to end --------------------------------------------------------------------------------------------------------
def test_syn20_narrow_windows_change_nothing_at_4096():
    """Two wavelengths of the SYN20 sweep, the variant switched on and off: the saved field of surface 20, its PSF and both
    powers are equal as numbers, and the "on" contexts did launch narrow-window kernels."""
    import paos_amd.run as prun
    from paos_amd.chains import syn20_chain, syn20_wavelength

    lib = tx._lib()
    wls = [syn20_wavelength(k) for k in (0, 333)]
    out = {}
    for on in (True, False):
        for what in ("wfo", "psf"):
            dev = _device(lib, len(wls), on)
            try:
                res = prun.run_batch(1.0, wls, N, 4, {"us": 0.0, "ut": 0.0}, [syn20_chain() for _ in wls], outputs=(what,), dev=dev)
                out[on, what] = [(r[20][what], r[20]["power"], r[1]["power"]) for r in res]
                narrow, other = _narrow_stats(dev)
                central, _ = dev.central_half_stats()
            finally:
                dev.close()
            assert (narrow > 0) == on and other > 0 and central >= narrow, (on, what, narrow, other, central)
    for what in ("wfo", "psf"):
        for (a, pa, qa), (b, pb, qb) in zip(out[True, what], out[False, what]):
            assert np.array_equal(a, b), what
            assert pa == pb and qa == qb, (what, pa, pb, qa, qb)
