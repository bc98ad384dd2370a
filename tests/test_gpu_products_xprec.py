"""The four products read out behind the pass kernels -- zoomed windows (csrc/zoom_pass.h), transfer functions
(csrc/otf_pass.h), through-focus planes (csrc/focus_pass.h), detector images (csrc/detector_pass.h) -- against the
long-double references and the bounds of tests/products_xprec.py, where tests/test_gpu_zoom.py, test_gpu_otf.py and
test_gpu_focus.py gate at the project's 1e-10 parity level.  Every assertion message carries the kernel's error next to the
yardstick's (NumPy or a sequential fp64 loop in the kernel's precision) and the bound; ``pytest -s`` prints them as XPREC
lines (profiles/r13_products_xprec.md).  The detector tests run the loop that splits a batch at the scratch cap into a
second chunk, against tests/detector_np.py at the existing 1e-13 and bit for bit against an unchunked route."""
import numpy as np
import pytest

import detector_np
import otf_np
import products_xprec as px
import xprec_np as xp
from conftest import l2_rel_err, rel_err

pytestmark = pytest.mark.gpu


def _lib():
    from paos_amd import _lib as lib

    return lib


# ---- 1. zoomed windows --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("n,batch,m,s", px.ZOOM_CASES, ids=["-".join(map(str, c)) for c in px.ZOOM_CASES])
def test_zoom_windows_against_long_double_and_bit_for_bit(n, batch, m, s, precision):
    """Every build zoom_kernel<T, STAGE, PT> is launched as (tests/test_zoom_host.py proves the cases reach them all).
    First and last item: the complex window against Wy u Wx^T in long double on the field the context returns, held to
    4 x the sequential fp64 yardstick's own error and to the rigorous componentwise bound.  Every item: window and
    intensity equal, bit for bit, to the same field run alone in a batch-1 context -- csrc/zoom_pass.h promises the
    same bits whatever the batch size, the item's position or PT, and a batch-1 context runs both stages at PT 1."""
    lib = _lib()
    xp.require_long_double()
    pty, ptx = lib.zoom_tiles(n, batch, m)
    assert lib.zoom_tiles(n, 1, m) == (1, 1), "the batch-1 context no longer runs both stages at one tile per wave"
    assert pty > 1 or ptx > 1
    fields, ctr = px.zoom_fields(n, batch), px.zoom_centres(n, batch, m, s)
    rows = px.zoom_sample_rows(m, pty) if n >= px.ZOOM_SAMPLED_FROM else None
    dev = lib.DeviceFields(n, batch, precision)
    one = lib.DeviceFields(n, 1, precision)
    report = []
    try:
        for i, u in enumerate(fields):
            dev.upload(i, u)
        dev.zoom_compute(m, s, ctr, field=True)
        for i in range(batch):
            got, got_psf = dev.zoom_fetch(i, "field"), dev.zoom_fetch(i, "psf")
            one.upload(0, fields[i])
            one.zoom_compute(m, s, ctr[i:i + 1], field=True)
            alone, alone_psf = one.zoom_fetch(0, "field"), one.zoom_fetch(0, "psf")
            same = got == alone
            assert same.all(), (f"item {i} of {batch} (PT {pty} / {ptx}) differs from the same field run alone (PT 1 / 1) at "
                                f"{np.argwhere(~same)[:4].tolist()} of {int((~same).sum())} elements")
            assert np.array_equal(got_psf, alone_psf), f"item {i}: the intensity differs from the batch-1 run"
            assert np.array_equal(got_psf, got.real * got.real + got.imag * got.imag)
            if i in (0, batch - 1):
                u = dev.download(i)
                ref = px.zoom_reference(u, m, s, *ctr[i], rows=rows)
                yard = px.zoom_yardstick(u, m, s, *ctr[i], rows=rows)
                rig = px.zoom_rigorous_bound(u, m, s, *ctr[i], rows=rows)
                what = f"zoom {precision} {n}^2 B={batch} M={m} s={s} PT {pty}/{ptx} item {i}"
                report.append(px.zoom_check(got if rows is None else got[rows], ref, yard, rig, what)[0])
    finally:
        dev.close()
        one.close()
        print("\nXPREC " + "\nXPREC ".join(report))


# ---- 2. transfer functions ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("n", px.SIZES)
def test_otf_against_long_double(n, precision):
    """OTF and MTF of the seeded random PSF of tests/test_gpu_otf.py and of a structured one (products_xprec.py:
    otf_structured_psf) against fft2(ifftshift(P)) / dc in long double on the fetched PSF: the whole transform up to
    2048^2, sampled frequency columns and rows at 4096^2; per line, the zero-frequency element left out
    (products_xprec.py: otf_line_errors), at xprec_np.bound(n, 2, 1), NumPy's fft2 in the context's precision within
    half of it.  Zero frequency is exactly 1 + 0i; the cuts are the fetched MTF's half row and half column, bit for bit."""
    lib = _lib()
    xp.require_long_double()
    fields = px.otf_fields(n)
    h = n // 2
    dev = lib.DeviceFields(n, len(fields), precision)
    report = []
    try:
        for i, u in enumerate(fields):
            dev.upload(i, u)
        dev.psf_keep()
        dev.otf_compute()
        cuts = dev.otf_cuts()
        for i in range(len(fields)):
            psf = dev.psf_fetch(i)
            centred, centred_mtf = dev.otf_fetch(i, "otf"), dev.otf_fetch(i, "mtf")
            assert centred[h, h].real == 1.0 and centred[h, h].imag == 0.0 and centred_mtf[h, h] == 1.0
            want_x, want_y = otf_np.cuts_of(centred_mtf)
            assert np.array_equal(cuts[i, 0], want_x) and np.array_equal(cuts[i, 1], want_y)
            got, got_mtf = px.otf_unshifted(centred), px.otf_unshifted(centred_mtf)
            del centred, centred_mtf
            yard = px.otf_yardstick(psf, precision)
            scales = px.otf_scales(yard)
            what = f"{precision} {n}^2 item {i}"
            if n <= 2048:
                ref = px.otf_reference(psf)
                blocks = [(None, None, axis, got, got_mtf, ref, yard, f"axis {axis}") for axis in (0, 1)]
            else:
                idx = px.otf_sample_indices(n)
                blocks = [(None, idx, 1, got[:, idx], got_mtf[:, idx], px.otf_reference_lines(psf, idx), yard[:, idx],
                           f"{idx.size} sampled columns"),
                          (idx, None, 0, got[idx, :], got_mtf[idx, :], px.otf_reference_lines(psf, idx, rows=True).T,
                           yard[idx, :], f"{idx.size} sampled rows")]
            for kys, kxs, axis, g, gm, ref, y, where in blocks:
                report.append(px.otf_check(g, ref, y, kys, kxs, axis, scales, precision, f"otf {what} {where}"))
                report.append(px.otf_check(gm, np.abs(ref), np.abs(y), kys, kxs, axis, scales, precision,
                                           f"mtf {what} {where}", mtf=True))
    finally:
        dev.close()
        print("\nXPREC " + "\nXPREC ".join(report))


# ---- 3. through-focus planes ------------------------------------------------------------------------------------------------
FOCUS_INVARIANT_SIZES = (128, 512, 4096)  # the sizes tests/test_gpu_focus.py: test_invariants_bit_for_bit does not run


def _focus_check_plane(out, before, n, plane, precision, lines, report, tag):
    dt = px.DT[precision]
    for item in range(3):
        full2d = plane[item, 0] != 0.0 and plane[item, 1] != 0.0 and plane[item, 2] != 0.0
        what = f"focus {precision} {n}^2 {tag} item {item}"
        if full2d:
            ref = px.focus_restate(before[item], n, plane, item)
            yard = px.focus_restate(before[item].astype(dt), n, plane, item, dtype=dt)
            for axis in (0, 1):
                report.append(px.focus_check(out[item], ref, yard, axis, n, 1, precision, what + f" (full 2-D H) axis {axis}"))
            continue
        axis = 1 if item == 1 else 0
        part = before[item][:, lines] if axis else before[item][lines]
        got = out[item][:, lines] if axis else out[item][lines]
        k = 1 if plane[item, 0] != 0.0 else 0
        # (the disabled item: the plane is the round trip, and the reference is the field itself)
        ref = px.focus_restate(part, n, plane, item, lines=lines) if k else part.astype(xp.LD)
        yard = px.focus_restate(part.astype(dt), n, plane, item, lines=lines, dtype=dt)
        report.append(px.focus_check(got, ref, yard, axis, n, k, precision, what + (" (H = 1)" if k == 0 else f" (s{'xy'[axis]} = 0)")))


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("n", px.SIZES)
def test_focus_planes_against_long_double(n, precision):
    """One focus_begin, two planes with corner arguments of about 1e2 and 1e6 rad, a batch of 3: item 0 with sy = 0 and
    item 1 with sx = 0 (H varies along one axis only: the plane is a 1-D operation in exact arithmetic, restated in long
    double on sampled rows / columns), item 2 disabled (the round trip: the reference is the field itself) -- and, up to
    1024^2, a third plane whose item 2 carries a full 2-D H, against the whole-field long-double program.  Bound: four
    line transforms and one phase factor, xprec_np.bound(n, 4, 1) (fp32: plus the generic family's factor bound).  At the
    sizes the existing invariants test does not run, focus_begin leaves the field bit-identical and a plane computed
    again after another plane comes out bit-identical."""
    lib = _lib()
    xp.require_long_double()
    lines = xp.sample_lines(n)
    fields = [px.focus_field(n, i) for i in range(3)]
    planes = [px.focus_plane_blocks(n, t) for t in px.FOCUS_TARGETS]
    dev = lib.DeviceFields(n, 3, precision)
    report = []
    try:
        for i, u in enumerate(fields):
            dev.upload(i, u)
        del fields
        before = [dev.download(i) for i in range(3)]
        dev.focus_begin()
        if n in FOCUS_INVARIANT_SIZES:
            assert all(np.array_equal(dev.download(i), before[i]) for i in range(3)), "focus_begin changed the field"
        first = None
        for plane, target in zip(planes, px.FOCUS_TARGETS):
            dev.focus_plane(plane)
            out = [dev.download(i) for i in range(3)]
            _focus_check_plane(out, before, n, plane, precision, lines, report, f"corner {target:g} rad")
            first = out if first is None else first
        del out
        if n in FOCUS_INVARIANT_SIZES:
            dev.focus_plane(planes[0])
            assert all(np.array_equal(dev.download(i), first[i]) for i in range(3)), "a plane depends on its predecessors"
        del first
        if n <= 1024:
            plane = px.focus_plane_blocks(n, 3.0e4, full2d=True)
            dev.focus_plane(plane)
            out = [dev.download(i) for i in range(3)]
            _focus_check_plane(out, before, n, plane, precision, lines, report, "corner 3e+04 rad")
        dev.focus_end()
    finally:
        dev.close()
        print("\nXPREC " + "\nXPREC ".join(report))


# ---- 4. detector: the chunk loop ------------------------------------------------------------------------------------------
DX0 = 2.0e-6
DET_TOL = 1.0e-13  # the existing gate of tests/test_gpu_detector.py


def test_detector_accumulate_runs_a_second_chunk():
    """17 items whose footprints are all 1024 rows under a 4096 x 8 detector: 32 MiB of row scratch each, so 16 fill the
    512 MiB cap exactly and the 17th opens a second chunk, which resets the scratch offset, reserves again and relies on
    the accumulator carrying over.  Against detector_np.accumulate in item order at 1e-13, and bit for bit against the
    same 17 PSFs fed through a batch-1 context in 17 detector_add calls (which never chunk)."""
    from paos_amd.detector import Detector

    lib = _lib()
    n, batch = 1024, 17
    det = Detector(4096, 8, DX0 / 4 * 1.001, 128 * DX0 * 1.001, xc=0.3 * DX0, yc=-0.2 * DX0)
    dxs = DX0 / (1.0 + 0.1 * np.arange(batch) / (batch - 1))  # spread <= 1.1 x, none coarser than the detector was sized for
    dys = dxs[::-1].copy()
    w = 0.5 + np.arange(batch) / batch
    w[5] = 0.0
    # the footprint arithmetic, from det_edge's formula: every item covers all rows, the cap splits 16 + 1
    foot = [px.detector_footprint_rows(det.ny, det.pitch_y, det.yc, dy, n) for dy in dys]
    assert all(f == (0, n) for f in foot), foot
    rows_bytes = [(k1 - k0) * det.nx * 8 for k0, k1 in foot]
    assert rows_bytes[0] == 32 << 20 and 16 * rows_bytes[0] == px.DETECTOR_SCRATCH_BYTES
    assert px.detector_chunks(rows_bytes) == [(0, 16), (16, 17)]
    rng = np.random.default_rng(4242)
    u = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    dev = lib.DeviceFields(n, batch, "fp64")
    one = lib.DeviceFields(n, 1, "fp64")
    try:
        for i in range(batch):
            dev.upload(i, u)
        dev.psf_keep()
        dev.detector_begin(det)
        dev.detector_add(dxs, dys, w)
        image = dev.detector_fetch()
        psf = dev.psf_fetch(0)
        assert np.array_equal(dev.psf_fetch(batch - 1), psf)
        want = detector_np.accumulate([detector_np.rebin(psf, det, dxs[i], dys[i]) for i in range(batch)], w)
        e, e2 = rel_err(image, want), l2_rel_err(image, want)
        print(f"\nXPREC detector accumulate {n}^2 B={batch} {det.nx}x{det.ny}, chunks 16 + 1: max {e:.3g} L2 {e2:.3g} (gate {DET_TOL:g})")
        assert want.max() > 0.0 and e < DET_TOL and e2 < DET_TOL, (e, e2)
        # the 17th item arrived: the image differs from the first chunk's alone by its share
        one.upload(0, u)
        one.psf_keep()
        one.detector_begin(det)
        for i in range(batch):
            one.detector_add(dxs[i:i + 1], dys[i:i + 1], w[i:i + 1])
            if i == batch - 2:
                assert not np.array_equal(one.detector_fetch(), image), "the second chunk added nothing"
        assert np.array_equal(one.detector_fetch(), image), "the chunked batch differs from 17 single adds"
    finally:
        dev.close()
        one.close()


def test_detector_images_run_a_second_chunk():
    """Five 4096 x 4096 images of 128 MiB each: four fit the cap and the fifth is a second chunk.  Each against
    detector_np.rebin at 1e-13 and bit for bit against detector_images of a batch-1 context holding that PSF."""
    from paos_amd.detector import Detector

    lib = _lib()
    n, batch = 256, 5
    det = Detector(4096, 4096, DX0 / 16.5, DX0 / 16.5, xc=0.3 * DX0 / 16.5, yc=-0.4 * DX0 / 16.5)
    dxs = DX0 * (1.0 + 0.004 * np.arange(batch))
    dys = DX0 * (1.0 - 0.003 * np.arange(batch))
    image_bytes = det.nx * det.ny * 8
    foot = [px.detector_footprint_rows(det.ny, det.pitch_y, det.yc, dy, n) for dy in dys]
    rows_bytes = [(k1 - k0) * det.nx * 8 for k0, k1 in foot]
    assert image_bytes == 128 << 20 and all(0 < b <= 8 << 20 for b in rows_bytes), rows_bytes
    assert px.detector_chunks(rows_bytes, image_bytes) == [(0, 4), (4, 5)]
    rng = np.random.default_rng(4343)
    fields = [rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)) for _ in range(batch)]
    dev = lib.DeviceFields(n, batch, "fp64")
    one = lib.DeviceFields(n, 1, "fp64")
    try:
        for i, u in enumerate(fields):
            dev.upload(i, u)
        dev.psf_keep()
        dev.detector_begin(det)
        got = dev.detector_images(dxs, dys)
        assert got.shape == (batch, det.ny, det.nx)
        one.detector_begin(det)
        worst = [0.0, 0.0]
        for i in range(batch):
            want = detector_np.rebin(dev.psf_fetch(i), det, dxs[i], dys[i])
            e, e2 = rel_err(got[i], want), l2_rel_err(got[i], want)
            worst = [max(worst[0], e), max(worst[1], e2)]
            assert want.max() > 0.0 and e < DET_TOL and e2 < DET_TOL, (i, e, e2)
            del want
            one.upload(0, fields[i])
            one.psf_keep()
            alone = one.detector_images(dxs[i:i + 1], dys[i:i + 1])
            assert np.array_equal(alone[0], got[i]), f"image {i} differs from the batch-1 context's"
            del alone
        print(f"\nXPREC detector images {n}^2 B={batch} {det.nx}x{det.ny}, chunks 4 + 1: max {worst[0]:.3g} L2 {worst[1]:.3g} "
              f"(gate {DET_TOL:g})")
    finally:
        dev.close()
        one.close()
