"""The central-half builds of the 4096^2 complex128 pass kernel (frugal_pass.h: CH; frugal_launch.h; passes.hip:
pick_build, `central`): a launch whose first pass loads positions of [N / 4, 3 N / 4) only skips the table factors, the
aperture weights and the first butterfly layer of the outer positions, which are exact zeros.

Every case runs the same program three times through the C ABI, on the harness of test_gpu_xprec.py: on a context with
the builds switched on (PAOS_CENTRAL_HALF=1 when it is created), on one with them switched off (=0) and on one with the
pruning off altogether (set_pruning(False)) whose fields hold real zeros outside the windows.  The three must agree as
numbers (np.array_equal), the per-context counter (central_half_stats) says which build the first launch took, and
sampled lines are held to the long-double restatement of xprec_np at its bound.  Buffers hold NaN outside the windows'
blocks; line windows are 64 lines, batches 2 or 3 items."""
import os

import numpy as np
import pytest

import test_gpu_xprec as tx
import xprec_np as xp

pytestmark = pytest.mark.gpu

N = 4096
L0, L1 = 2016, 2080                      # the 64 live lines of the first pass
SAMPLED = np.array([L0, L0 + 1, L0 + 7, L0 + 8, L0 + 31, L0 + 32, L1 - 2, L1 - 1])
CENTRAL = [(1024, 3072), (1532, 2564), (1279, 1281), (2000, 2001)]
REFUSED = [(1023, 3072), (1024, 3073)]


def _device(lib, batch, central, pruning=True):
    """A context that read PAOS_CENTRAL_HALF = ``central`` when it was created."""
    old = os.environ.get("PAOS_CENTRAL_HALF")
    os.environ["PAOS_CENTRAL_HALF"] = "1" if central else "0"
    try:
        dev = lib.DeviceFields(N, batch, "fp64")
    finally:
        if old is None:
            del os.environ["PAOS_CENTRAL_HALF"]
        else:
            os.environ["PAOS_CENTRAL_HALF"] = old
    if not pruning:
        dev.set_pruning(False)
    return dev


def _boxed(seed, axis, window, lines=(L0, L1), stale=True):
    """A field that lives on ``lines`` x ``window`` (positions along the lines of a pass along ``axis``): zeros around the
    box as far as its 8 x 8 blocks reach and NaN beyond them (``stale``), or zeros everywhere else."""
    lo, hi = window
    u = np.full((N, N), np.nan + 1j * np.nan if stale else 0.0, dtype=np.complex128)
    v = u if axis == 0 else u.T  # v[line, position]
    v[lines[0]:lines[1], (lo // 8) * 8:-(-hi // 8) * 8] = 0.0
    v[lines[0]:lines[1], lo:hi] = (tx._field(N, seed) if axis == 0 else tx._field(N, seed).T)[lines[0]:lines[1], lo:hi]
    return u


def _windows_kw(axis, windows, lines=(L0, L1)):
    """live_rows / live_cols of a batch whose item i loads ``windows[i]`` on ``lines`` (None: the whole grid, a bystander)."""
    ln = np.array([list(lines) if w is not None else [0, N] for w in windows], dtype=np.float64)
    ps = np.array([list(w) if w is not None else [0, N] for w in windows], dtype=np.float64)
    rows, cols = (ln, ps) if axis == 0 else (ps, ln)
    return {"live_rows": rows, "live_cols": cols, "rows_stale": True}


def _run(lib, fields, passes, blocks, central, pruning=True, intensity=False, **kw):
    """-> (outputs, launch tags, powers or None, (central, plain) launches of the context)."""
    dev = _device(lib, len(fields), central, pruning)
    try:
        for i, f in enumerate(fields):
            dev.upload(i, f)
        dev.profile_begin(lib.KERNEL_PASS_ANY, max_launches=64)
        if intensity:
            kw = dict(kw, final_intensity=1)
        ticket = dev.run_passes(passes, blocks, **kw)
        power = None if ticket is None else dev.norm2_fetch(ticket)
        _, tags = dev.profile_end_launches()
        out = [dev.psf_fetch(i) if intensity else dev.download(i) for i in range(len(fields))]
        return out, tags, power, dev.central_half_stats()
    finally:
        dev.close()


def _three_ways(lib, axis, seeds, windows, passes, blocks, want_central, lines=(L0, L1), intensity=False):
    """Run the program on the three contexts and hold them to each other; returns the outputs of the first."""
    kw = _windows_kw(axis, windows, lines)
    stale = [_boxed(s, axis, w, lines) if w is not None else tx._field(N, s) for s, w in zip(seeds, windows)]
    on, tags, p_on, (central, plain) = _run(lib, stale, passes, blocks, True, intensity=intensity, **kw)
    assert central + plain == tags.size and (central > 0) == want_central, (central, plain, tags)
    if want_central:
        assert central == 1 and tags[0] & 2, (central, tags)  # the first launch, and it skips loads
    off, tags_off, p_off, (central_off, _) = _run(lib, stale, passes, blocks, False, intensity=intensity, **kw)
    assert central_off == 0 and np.array_equal(tags, tags_off), (central_off, tags, tags_off)
    del stale
    zeros = [_boxed(s, axis, w, lines, stale=False) if w is not None else tx._field(N, s) for s, w in zip(seeds, windows)]
    dense, _, p_dense, (central_dense, _) = _run(lib, zeros, passes, blocks, True, pruning=False, intensity=intensity)
    assert central_dense == 0, "a context without pruning plans no windows"
    for i, w in enumerate(windows):
        if w is not None:
            assert np.isfinite(on[i]).all(), f"item {i} window {w}: stale data reached the output"
        assert np.array_equal(on[i], off[i]), f"item {i} window {w}: central-half build != ordinary build"
        assert np.array_equal(on[i], dense[i]), f"item {i} window {w}: central-half build != pruning off"
        if p_on is not None:
            assert p_on[i] == p_off[i] == p_dense[i], (i, p_on[i], p_off[i], p_dense[i])
    return on, zeros


def _chain(lib, axis, count, batch=2, fft1_off_item=None, aperture=None):
    """``count`` passes of one row / column chain (test_gpu_xprec._chain: phases along the lines in both slots), batch of
    ``batch`` (a third item has every operator disabled).  ``fft1_off_item``: that item's first transform is switched off.
    ``aperture``: [batch] ellipse parameters of an aperture in front of the first pass's phase (-> blocks, mask block)."""
    passes, blocks = tx._chain(lib, N, axis, count)
    blocks = blocks[:, :batch].copy()
    extra = np.zeros((3, batch, 5))
    extra[0] = blocks[0]
    if fft1_off_item is not None:
        extra[0, fft1_off_item, 0] = 0.0
        passes[0] = dict(passes[0], fft1=blocks.shape[0])
    mask_block = None
    if aperture is not None:
        mask_block = blocks.shape[0] + 1
        for i, ap in enumerate(aperture):
            extra[1, i] = ap
            extra[2, i] = [0.0, 0.0, 32.0, lib.SHAPE_ELLIPSE, 0.0]
        passes[0] = dict(passes[0], pre=[(lib.PW_MASK, 0, mask_block)] + list(passes[0]["pre"]))
    return passes, np.concatenate([blocks, extra]), mask_block


def _masks(lib, mask_block, aperture):
    if mask_block is None:
        return None
    dev = lib.DeviceFields(N, 1, "fp64")
    try:
        return {mask_block: [dev.aperture_mask(lib.SHAPE_ELLIPSE, list(ap) + [0.0, 0.0, 32.0]) for ap in aperture]}
    finally:
        dev.close()


def _check_lines(got, zeros, passes, blocks, axis, items, n_fft, k_phase, what, masks=None, psf=False):
    """The sampled live lines of ``items`` against the long-double restatement of the program on the zero-filled inputs."""
    sel = {"rows": SAMPLED} if axis == 0 else {"cols": SAMPLED}
    for i in items:
        part = zeros[i][SAMPLED] if axis == 0 else zeros[i][:, SAMPLED]
        ref = xp.run_item(part, passes, blocks, i, N, masks=masks, **sel)
        yard = xp.run_item(part, passes, blocks, i, N, masks=masks, dtype=np.complex128, **sel)
        g = got[i][SAMPLED] if axis == 0 else got[i][:, SAMPLED]
        if psf:
            ref, yard = ref.real ** 2 + ref.imag ** 2, np.abs(yard) ** 2
            b_l2, b_el = xp.bound(N, n_fft, k_phase, "fp64")
            g_l2, g_el = xp.line_errors(g, ref, axis)
            y_l2, y_el = xp.line_errors(yard, ref, axis)
            msg = f"{what} item {i}: PSF L2 {g_l2:.3g} / element {g_el:.3g}; NumPy {y_l2:.3g} / {y_el:.3g}; bound {2 * b_l2:.3g} / {2 * b_el:.3g}"
            assert g_l2 <= 2 * b_l2 and g_el <= 2 * b_el, msg  # (|u|^2: twice the field's relative error, as test_storing_builds_psf_and_power)
        else:
            msg = xp.check(g, ref, yard, axis, N, n_fft, k_phase, "fp64", f"{what} item {i}")[4]
        print("\nXPREC " + msg)


# ---- window edges -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("window", CENTRAL, ids=[f"{a}-{b}" for a, b in CENTRAL])
def test_windows_inside_the_central_half_take_the_new_build(window, axis):
    """A fused two-pass launch whose items load [1024, 3072) -- all of k = 4..11 --, the quarter [1532, 2564) of a chain
    step, [1279, 1281) (one thread's k = 4 and k = 5 only) and the single position 2000."""
    lib = tx._lib()
    passes, blocks, _ = _chain(lib, axis, 2)
    on, zeros = _three_ways(lib, axis, (3, 4), [window, window], passes, blocks, True)
    _check_lines(on, zeros, passes, blocks, axis, (0, 1), 4, 4, f"central half, window {window} axis {axis}")


# ---- refusals ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("windows", [[REFUSED[0], REFUSED[0]], [REFUSED[1], REFUSED[1]], [(1532, 2564), (512, 1536)]],
                         ids=["1023-3072", "1024-3073", "one-item-outside"])
def test_a_window_outside_the_central_half_keeps_the_old_build(windows):
    """One position beyond either edge -- or one item of the batch outside -- sends the whole launch to the ordinary
    build, with the same answers; the disabled third item comes back bit for bit."""
    lib = tx._lib()
    axis = 0
    passes, blocks, _ = _chain(lib, axis, 2, batch=3)
    on, zeros = _three_ways(lib, axis, (3, 4, 5), windows + [None], passes, blocks, False)
    assert np.array_equal(on[2], tx._field(N, 5)), "the disabled item changed"
    _check_lines(on, zeros, passes, blocks, axis, (0, 1), 4, 4, f"refused windows {windows}")


# ---- programs ---------------------------------------------------------------------------------------------------------
# the aperture of the row cases: its partial runs on the sampled rows sit at columns 1279 .. 1281 and 2815 .. 2817, the
# boundaries between a thread's elements k = 4 / 5 (position 1280) and k = 10 / 11 (position 2816)
APERTURE = [[1.0, 2048.3, 2048.2, 768.0, 900.0], [1.0, 2047.6, 2050.0, 768.4, 1100.0]]


@pytest.mark.parametrize("axis,masked", [(0, False), (0, True), (1, False)], ids=["rows", "rows-aperture", "cols"])
@pytest.mark.parametrize("program", ["two", "three", "psf", "fft1-off"])
def test_fused_programs_on_the_central_half_build(program, axis, masked):
    """Two and three passes in one launch, the PSF-storing last launch, and an item whose first transform is switched off
    beside one with it on -- rows with and without an aperture in front of the first phase, and columns.  The PSF-storing
    launch has no central-half build (it was built and measured slower, profiles/r11_central_half.md): it must stay on
    the ordinary build and give the same PSF and powers on all three contexts."""
    lib = tx._lib()
    window = (1024, 3072) if masked else (1532, 2564)
    count = 3 if program == "three" else 2
    aperture = APERTURE if masked else None
    passes, blocks, mask_block = _chain(lib, axis, count, fft1_off_item=1 if program == "fft1-off" else None, aperture=aperture)
    psf = program == "psf"
    on, zeros = _three_ways(lib, axis, (6, 7), [window, window], passes, blocks, not psf, intensity=psf)
    masks = _masks(lib, mask_block, aperture)
    _check_lines(on, zeros, passes, blocks, axis, (0, 1), 2 * count, 2 * count, f"{program} axis {axis} aperture {masked}",
                 masks=masks, psf=psf)


@pytest.mark.parametrize("axis,masked", [(0, False), (0, True), (1, False)], ids=["rows", "rows-aperture", "cols"])
def test_single_table_pass_on_the_central_half_build(axis, masked):
    """The ONE shape: a single table pass with a phase in front of its first transform that loads a quarter of its
    positions and -- an aperture in the next pass, along the other axis, keeps a quarter of ITS lines -- stores a
    quarter too (test_gpu_xprec.test_single_table_pass_on_one_line_workgroups, on either axis).  ``masked`` (the row
    single pass of a chain step): an aperture of its own rides in the trimmed slot, in front of the phase, with its
    partial runs at the k = 4 / 5 and k = 10 / 11 boundaries (APERTURE); it clips the loads of [1024, 3072) to its
    bounding box, 1548 positions, so the pass still loads and stores at most half of them."""
    lib = tx._lib()
    window = (1024, 3072) if masked else (1532, 2564)
    other = 1 - axis
    blocks = np.zeros((8, 2, 5))
    blocks[0, :] = [1.0, 0.0, 0.0, 0.0, 0.0]
    blocks[1, :] = [1.0, 1.0, 0.0, 0.0, 0.0]
    blocks[2, :] = [1.0, 0.0, 0.0, 1.0 / N, 0.0]
    for i, (s, t, sg) in enumerate(((0.8, 3e6, -1.0), (1.7, 5e10, 1.0))):
        sx, sy = (s, 0.0) if axis == 0 else (0.0, s)
        blocks[3, i] = [1.0, sx, sy, tx._corner_coef(t, N, sx, sy, True), sg]
    # (both extents inside the window: the first pass hands its window back -- phase, transform, 1 / N, inverse -- so a kept line
    # outside it would hold rounding noise only)
    ap = [[1.0, N / 2 + 0.3, N / 2 - 0.2, N / 10, N / 9], [1.0, N / 2 - 5.5, N / 2 + 7.25, N / 9, N / 10]]
    for i in range(2):
        blocks[4, i] = ap[i]
        blocks[5, i] = [0.0, 0.0, 32.0, lib.SHAPE_ELLIPSE, 0.0]
    pre = [(lib.PW_QPHASE_CENTRED, lib.PWF_MUL2PI, 3)]
    if masked:
        for i in range(2):
            blocks[6, i] = APERTURE[i]
            blocks[7, i] = [0.0, 0.0, 32.0, lib.SHAPE_ELLIPSE, 0.0]
        pre = [(lib.PW_MASK, 0, 6)] + pre
    passes = [{"axis": axis, "fft1": 0, "fft2": 1, "pre": pre, "mid": [(lib.PW_SCALE, 0, 2)]},
              {"axis": other, "fft1": 0, "pre": [(lib.PW_MASK, 0, 4)]}]
    on, zeros = _three_ways(lib, axis, (10, 11), [window, window], passes, blocks, True)
    masks = _masks(lib, 4, ap)
    if masked:
        masks.update(_masks(lib, 6, APERTURE))
    live = np.arange(L0, L1)  # the lines of the first pass
    for i in range(2):
        # first pass on its live lines; second pass on the (sampled) lines of the other axis the aperture leaves non-zero
        m = masks[4][i]
        kept = np.nonzero(m.any(axis=1 if other == 0 else 0))[0]
        kept = kept[:: max(1, kept.size // 12)]
        z = zeros[i]
        part = z[live] if axis == 0 else z[:, live]
        sel = {"rows": live} if axis == 0 else {"cols": live}
        mids = [xp.run_item(part, passes[:1], blocks, i, N, masks=masks, dtype=dt, **sel) for dt in (xp.LD, np.complex128)]
        refs = []
        for mid, dt in zip(mids, (xp.LD, np.complex128)):
            if other == 0:  # mid: [every row, live columns] -> rows `kept`, every column
                u = np.zeros((kept.size, N), dtype=dt)
                u[:, live] = mid[kept]
                refs.append(xp.run_item(u, passes[1:], blocks, i, N, rows=kept, masks=masks, dtype=dt))
            else:           # mid: [live rows, every column] -> every row, columns `kept`
                u = np.zeros((N, kept.size), dtype=dt)
                u[live] = mid[:, kept]
                refs.append(xp.run_item(u, passes[1:], blocks, i, N, cols=kept, masks=masks, dtype=dt))
        got = on[i][kept] if other == 0 else on[i][:, kept]
        dead = np.setdiff1d(np.arange(N), np.nonzero(m.any(axis=1 if other == 0 else 0))[0])
        assert not np.any(on[i][dead] if other == 0 else on[i][:, dead]), "lines the aperture zeroes"
        print("\nXPREC " + xp.check(got, refs[0], refs[1], other, N, 3, 1, "fp64", f"single table pass axis {axis} aperture {masked} item {i}")[4])


# ---- SYN20 end to end -------------------------------------------------------------------------------------------------
def test_syn20_central_half_changes_nothing_at_4096():
    """Two wavelengths of the SYN20 sweep, the builds switched on and off: the saved field of surface 20, its PSF and both
    powers are equal as numbers, and the "on" contexts did launch central-half builds."""
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
                central, plain = dev.central_half_stats()
            finally:
                dev.close()
            assert (central > 0) == on and plain > 0, (on, what, central, plain)
    for what in ("wfo", "psf"):
        for (a, pa, qa), (b, pb, qb) in zip(out[True, what], out[False, what]):
            assert np.array_equal(a, b), what
            assert pa == pb and qa == qb, (what, pa, pb, qa, qb)
