"""The references and bounds of tests/products_xprec.py, checked without a device before their verdicts on the kernels
are trusted (tests/test_gpu_products_xprec.py): each long-double reference against an independent evaluation of the same
definition at 64^2 (to 1e-17 relative), the sampled routines against the whole ones, every yardstick within half of its
bound on the inputs the GPU tests use (256^2 and 1024^2, both precisions), the zoom yardstick within the rigorous
componentwise bound -- and each check failing on a value that is wrong by 1e-12 of itself."""
import numpy as np
import pytest

import otf_np
import products_xprec as px
import xprec_np as xp
import zoom_np

LD, LDR = xp.LD, np.longdouble


def _l2(got, ref):
    d = np.abs(np.asarray(got).astype(LD) - np.asarray(ref).astype(LD)).astype(LDR)
    r = np.abs(np.asarray(ref).astype(LD)).astype(LDR)
    return float(np.sqrt(np.sum(d * d) / np.sum(r * r)))


def test_long_double_first():
    xp.require_long_double()
    assert np.fft.fft2(np.ones((4, 4), dtype=LD)).dtype == LD


# ---- 64^2: the references against independent evaluations ----------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1])
def test_otf_reference_against_the_defining_double_sum(which):
    xp.require_long_double()
    n = 64
    u = px.otf_fields(n)[which]
    psf = u.real**2 + u.imag**2
    want = otf_np.otf_longdouble(psf)  # centred
    got = np.fft.fftshift(px.otf_reference(psf))
    assert got[n // 2, n // 2] == 1
    got[n // 2, n // 2] = want[n // 2, n // 2] = 0  # off-DC values against off-DC values
    assert _l2(got, want) <= 1e-17, _l2(got, want)


def _window_by_spectrum_ld(u, m, s, cx, cy):
    """zoom_np.window_by_spectrum with the spectrum and the basis kept in long double."""
    n = u.shape[0]
    spec = np.fft.fft2(np.asarray(u).astype(LD))
    k = np.fft.fftfreq(n, 1.0 / n).astype(LDR)

    def basis(c):
        t = zoom_np.positions(n, m, s, c)
        # (k t mod N in long double keeps the argument small: k is an integer, t has few bits)
        arg = 2 * zoom_np.PI * np.mod(t[:, None] * k[None, :], LDR(n)) / LDR(n)
        e = (np.cos(arg) + 1j * np.sin(arg)).astype(LD)
        e[:, n // 2] = np.cos(zoom_np.PI * t)
        return e

    return basis(cy) @ spec @ basis(cx).T / LDR(n * n)


@pytest.mark.parametrize("m,s,cx,cy", [(48, 3, 20.25, 40.5), (64, 4, 1.37, 61.38), (32, 2, 35.0, 27.0), (32, 4, 31.8125, 12.3)])
def test_zoom_reference_against_the_spectrum(m, s, cx, cy):
    xp.require_long_double()
    n = 64
    u = px.zoom_fields(n, 1)[0]
    got = px.zoom_reference(u, m, s, cx, cy)
    want = _window_by_spectrum_ld(u, m, s, cx, cy)
    assert got.dtype == LD and _l2(got, want) <= 1e-17, _l2(got, want)
    rows = np.array([0, 5, 16, m - 1])
    assert np.array_equal(px.zoom_reference(u, m, s, cx, cy, rows=rows), got[rows])
    # the weights are not rounded to double: they differ from the double-rounded ones, by less than an fp64 ulp
    w = px.zoom_weights(n, m, s, cy)
    assert w.dtype == LDR and np.array_equal(w.astype(np.float64), zoom_np.weight_matrix(n, m, s, cy))
    if cy != np.floor(cy):
        assert np.any(w != w.astype(np.float64).astype(LDR))


@pytest.mark.parametrize("target", px.FOCUS_TARGETS)
def test_focus_sampled_lines_against_the_whole_field_program(target):
    xp.require_long_double()
    n = 64
    plane = px.focus_plane_blocks(n, target)
    lines = xp.sample_lines(n)
    for item in range(3):
        u = px.focus_field(n, item)
        whole = px.focus_restate(u, n, plane, item)
        assert whole.dtype == LD
        axis = 1 if item == 1 else 0
        part = px.focus_restate(u[:, lines] if axis else u[lines], n, plane, item, lines=lines)
        want = whole[:, lines] if axis else whole[lines]
        assert _l2(part, want) <= 1e-17, (item, _l2(part, want))
        if item == 2:  # the disabled item: the round trip is the field itself
            assert _l2(whole, u) <= 1e-17


def test_focus_whole_field_program_is_the_definition():
    """The program against ifft2(H fft2(u)) written with np.fft directly (fp64; the full 2-D H of the second call)."""
    n = 64
    plane = px.focus_plane_blocks(n, 1.0e2, full2d=True)
    u = px.focus_field(n, 2)
    got = px.focus_restate(u, n, plane, 2, dtype=np.complex128)
    g = np.fft.fftfreq(n, 1.0 / n)
    q = plane[2, 3] * ((g * plane[2, 1])[None, :] ** 2 + (g * plane[2, 2])[:, None] ** 2)
    want = np.fft.ifft2(np.exp(-1j * q) * np.fft.fft2(u))
    assert np.max(np.abs(got - want)) <= 1e-13 * np.max(np.abs(u))
    assert abs(q[n // 2, n // 2] - 1.0e2) < 1e-10  # the corner argument


def test_otf_sampled_lines_equal_the_whole_transform():
    xp.require_long_double()
    n = 256
    idx = px.otf_sample_indices(n)
    assert {0, 1, 2, n // 2 - 1, n // 2, n // 2 + 1, n - 1} <= set(idx.tolist())
    for u in px.otf_fields(n):
        psf = u.real**2 + u.imag**2
        whole = px.otf_reference(psf)
        cols = px.otf_reference_lines(psf, idx)
        rows = px.otf_reference_lines(psf, idx, rows=True)
        assert cols.dtype == LD and cols.shape == (n, idx.size)
        assert _l2(cols, whole[:, idx]) <= 1e-17 and _l2(rows, whole[idx, :].T) <= 1e-17
        # ... and off-DC alone (the zero-frequency value dominates the L2 norm of its own line)
        for line, (got, want) in enumerate(((cols, whole[:, idx]), (rows, whole[idx, :].T))):
            got, want = got.copy(), want.copy()
            got[0, 0] = want[0, 0] = 0
            assert _l2(got, want) <= 1e-17, line


# ---- 256^2 and 1024^2: every yardstick within half of its bound, on the GPU tests' inputs --------------------------------
@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("n", [256, 1024])
def test_otf_yardstick_within_half_the_bound(n, precision):
    xp.require_long_double()
    for item, u in enumerate(px.otf_fields(n)):
        u = u.astype(px.DT[precision])  # what the context holds
        psf = u.real.astype(np.float64) ** 2 + u.imag.astype(np.float64) ** 2
        ref = px.otf_reference(psf)
        yard = px.otf_yardstick(psf, precision)
        scales = px.otf_scales(yard)
        for axis in (0, 1):
            # otf_check's first assertion is the one under test here (the yardstick stands in for the kernel)
            print(px.otf_check(yard, ref, yard, None, None, axis, scales, precision,
                               f"otf yardstick {n}^2 {precision} item {item} axis {axis}"))
            print(px.otf_check(np.abs(yard), np.abs(ref), np.abs(yard), None, None, axis, scales, precision,
                               f"mtf yardstick {n}^2 {precision} item {item} axis {axis}", mtf=True))
        # the sampled form of the 4096^2 check gives the same verdict on its lines
        idx = px.otf_sample_indices(n)
        print(px.otf_check(yard[:, idx], px.otf_reference_lines(psf, idx), yard[:, idx], None, idx, 1, scales, precision,
                           f"otf yardstick {n}^2 {precision} item {item} sampled columns"))
        print(px.otf_check(yard[idx, :], px.otf_reference_lines(psf, idx, rows=True).T, yard[idx, :], idx, None, 0, scales,
                           precision, f"otf yardstick {n}^2 {precision} item {item} sampled rows"))


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("n", [256, 1024])
def test_focus_yardsticks_within_half_the_bound(n, precision):
    xp.require_long_double()
    dt = px.DT[precision]
    lines = xp.sample_lines(n)
    for target in px.FOCUS_TARGETS:
        plane = px.focus_plane_blocks(n, target)
        for item in range(3):
            u = px.focus_field(n, item).astype(dt).astype(np.complex128)
            axis = 1 if item == 1 else 0
            part = u[:, lines] if axis else u[lines]
            ref = px.focus_restate(part, n, plane, item, lines=lines) if item < 2 else part.astype(LD)
            yard = px.focus_restate(part.astype(dt), n, plane, item, lines=lines, dtype=dt)
            print(px.focus_check(yard, ref, yard, axis, n, 0 if item == 2 else 1, precision,
                                 f"focus yardstick {n}^2 {precision} item {item} corner {target:g}"))
    plane = px.focus_plane_blocks(n, 3.0e4, full2d=True)
    u = px.focus_field(n, 2).astype(dt).astype(np.complex128)
    ref = px.focus_restate(u, n, plane, 2)
    yard = px.focus_restate(u.astype(dt), n, plane, 2, dtype=dt)
    for axis in (0, 1):
        print(px.focus_check(yard, ref, yard, axis, n, 1, precision, f"focus yardstick {n}^2 {precision} full 2-D H axis {axis}"))


ZOOM_CPU_CASES = [c for c in px.ZOOM_CASES if c in ((1024, 11, 192, 4), (256, 10, 240, 2), (256, 9, 496, 4))]


@pytest.mark.parametrize("n,batch,m,s", ZOOM_CPU_CASES)
def test_zoom_yardstick_within_the_rigorous_bound(n, batch, m, s):
    """The sequential fp64 yardstick on the GPU test's own fields and centres (first and last item): inside the rigorous
    componentwise bound, and far above the long-double reference's own error."""
    xp.require_long_double()
    from paos_amd import _lib

    pty, _ = _lib.zoom_tiles(n, batch, m)
    rows = px.zoom_sample_rows(m, pty) if n >= px.ZOOM_SAMPLED_FROM else None
    fields, ctr = px.zoom_fields(n, batch), px.zoom_centres(n, batch, m, s)
    for i in (0, batch - 1):
        ref = px.zoom_reference(fields[i], m, s, *ctr[i], rows=rows)
        yard = px.zoom_yardstick(fields[i], m, s, *ctr[i], rows=rows)
        rig = px.zoom_rigorous_bound(fields[i], m, s, *ctr[i], rows=rows)
        msg, ratio = px.zoom_check(yard, ref, yard, rig, f"zoom yardstick {n}^2 M={m} s={s} item {i}")
        print(msg)
        assert ratio == (1.0, 1.0)
        y_l2, y_el = px.zoom_errors(yard, ref)
        assert 1e-17 < y_l2 < 1e-14 and y_el < 1e-14, (y_l2, y_el)  # ~sqrt(n) u: what such a chain achieves
        # BLAS in fp64 (tests/zoom_np.py: window) is another correct evaluation: within the same gate
        blas = zoom_np.window(fields[i], m, s, *ctr[i])
        px.zoom_check(blas if rows is None else blas[rows], ref, yard, rig, "zoom_np.window")


def test_zoom_sample_rows_reach_what_they_promise():
    for m, pt in [(128, 8), (192, 8), (160, 4), (128, 4), (496, 4), (240, 2), (512, 4), (1024, 8)]:
        rows = set(px.zoom_sample_rows(m, pt, limit=64).tolist())
        tiles, group = m // 16, 16 * pt
        assert {0, m - 1} <= rows
        for g in range(group, m, group):
            assert {g - 1, g} <= rows, (m, pt, g)
        last0 = (-(-tiles // pt) - 1) * group
        for b in list(range(16, min(group, m), 16)) + list(range(last0 + 16, m, 16)):
            assert {b - 1, b} <= rows, (m, pt, b)
        if tiles % pt:
            assert any(last0 < r < m - 1 and r % 16 not in (0, 15) for r in rows), (m, pt)
    for n, batch, m, s in px.ZOOM_CASES:
        if n >= px.ZOOM_SAMPLED_FROM:
            from paos_amd import _lib

            assert px.zoom_sample_rows(m, _lib.zoom_tiles(n, batch, m)[0]).size <= 32


def test_zoom_centres_are_what_the_cases_ask_for():
    for n, batch, m, s in px.ZOOM_CASES:
        ctr = px.zoom_centres(n, batch, m, s)
        assert ctr.shape == (batch, 2) and np.all(ctr >= 0) and np.all(ctr < n)
        integer = [i for i in range(batch) if np.all(ctr[i] == np.floor(ctr[i]))]
        assert integer == [1]
        half = 0.5 * m / s
        assert ctr[0, 0] - half < 0 and ctr[0, 1] + half > n  # item 0's window wraps in both axes
        assert np.all(ctr[-1] != np.floor(ctr[-1]))


# ---- the checks fail on values wrong by 1e-12 of themselves -------------------------------------------------------------
def test_checks_fail_on_a_relative_error_of_1e_12():
    xp.require_long_double()
    n = 256
    u = px.otf_fields(n)[0]
    psf = u.real**2 + u.imag**2
    ref, yard = px.otf_reference(psf), px.otf_yardstick(psf, "fp64")
    assert np.max(np.abs(yard * (1 + 1e-12) - yard)) < 1e-10  # the old gate lets it through ...
    with pytest.raises(AssertionError):
        px.otf_check(yard * (1 + 1e-12), ref, yard, None, None, 1, px.otf_scales(yard), "fp64", "perturbed")  # ... this one does not
    m, s, cx, cy = 64, 4, 100.3, 77.7
    f = px.zoom_fields(n, 1)[0]
    ref, yard = px.zoom_reference(f, m, s, cx, cy), px.zoom_yardstick(f, m, s, cx, cy)
    rig = px.zoom_rigorous_bound(f, m, s, cx, cy)
    bad = yard.copy()
    bad.real *= 1 + 1e-12
    with pytest.raises(AssertionError):
        px.zoom_check(bad, ref, yard, rig, "perturbed")
    plane = px.focus_plane_blocks(n, 1.0e2)
    lines = xp.sample_lines(n)
    part = px.focus_field(n, 0)[lines]
    ref = px.focus_restate(part, n, plane, 0, lines=lines)
    yard = px.focus_restate(part, n, plane, 0, lines=lines, dtype=np.complex128)
    with pytest.raises(AssertionError):
        px.focus_check(yard * (1 + 1e-12), ref, yard, 0, n, 1, "fp64", "perturbed")


def test_detector_chunk_arithmetic():
    """The chunks of csrc/detector.hip: detector_run restated, on the two geometries the GPU tests use."""
    mib = 1 << 20
    assert px.DETECTOR_SCRATCH_BYTES == 512 * mib
    assert px.detector_chunks([32 * mib] * 17) == [(0, 16), (16, 17)]
    assert px.detector_chunks([32 * mib] * 16) == [(0, 16)]
    assert px.detector_chunks([mib] * 5, image_bytes=128 * mib) == [(0, 4), (4, 5)]
    assert px.detector_chunks([600 * mib, mib]) == [(0, 1), (1, 2)]  # an item larger than the cap runs alone
    # a detector 128 grid pitches tall per row, 8 rows, centred 0.2 pitches off: every grid row
    assert px.detector_footprint_rows(8, 128 * 1.001, -0.2, 1.0, 1024) == (0, 1024)
    assert px.detector_footprint_rows(8, 1.0, 0.0, 1.0, 1024) == (508, 517)
