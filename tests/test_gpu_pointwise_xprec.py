"""The pointwise kernels that do their own arithmetic against the long-double restatements of tests/pointwise_xprec.py:
zernike_kernel (maps, fields, wavelength groups, the row window of zernike_apply), zernike_gram_kernel + its final
stage (the Gram sums behind Zorthonorm / PolyOrthoNorm), psf_metrics_kernel + its final stage (power, centroid, peak,
encircled energy), and the host's refusal of requests whose answer would be NaN dressed up as a mask or a radius.

Every assertion message carries the kernel's error, the bound, and what the fp64 NumPy restatement of the reference
reaches on the same case (relative to the same scale).  Everything goes through the C ABI (``DeviceFields``)."""
import numpy as np
import pytest

import pointwise_xprec as px

pytestmark = pytest.mark.gpu

# Largest error observed on an MI355X over this module, as a fraction of the bound of its case: maps (wfe returned;
# C_MAP = 4, so 0.21 is 0.85 (nmax + 1) u E(p)), fields after the phase, Gram sums (C_GRAM = 8: 0.37 (nmax + 1 +
# log2 count) u sum E_i E_j), metric sums (C_METRIC = 2: 0.43 log2(npix) u sum).  test_zzz_report_observed prints this
# run's values.
OBSERVED_MI355X = {"map": 0.211, "field": 0.472, "gram": 0.0462, "metric": 0.214}
OBSERVED = {"map": None, "field": None, "gram": None, "metric": None}

OFFSETS = (0.0, 30.0, -90.0, 370.0)
DT = {"fp64": np.complex128, "fp32": np.complex64}
_CACHE = {}


def _lib():
    from paos_amd import _lib as lib

    return lib


def setup_module():
    px.require_long_double()


def _count(nmax, ordering):
    return (nmax // 2 + 1) ** 2 if ordering == "fringe" else (nmax + 1) * (nmax + 2) // 2


def _tables(nmax, ordering, normalize, seed=0):
    """(m, n, norm, coefficients): every term up to radial order nmax, seeded coefficients ~1e-7 in total."""
    from paos_amd.zernike import zernike_tables

    count = _count(nmax, ordering)
    m, n, norm = zernike_tables(count, ordering, normalize)
    rng = np.random.default_rng(100 * nmax + seed)
    return m, n, norm, rng.standard_normal(count) * 2e-7 / np.sqrt(count)


def _field(npix, seed):
    key = ("f", npix, seed)
    if key not in _CACHE:
        if len(_CACHE) > 8:
            _CACHE.clear()
        rng = np.random.default_rng(7 * npix + seed)
        _CACHE[key] = rng.standard_normal((npix, npix)) + 1j * rng.standard_normal((npix, npix))
    return _CACHE[key]


def _stored(f, precision):
    with np.errstate(over="ignore"):  # (poison values beyond fp32's range become inf, as they do in the context)
        return np.asarray(f).astype(DT[precision]).astype(np.complex128)


def _block(m, n, norm, z, it):
    from paos_amd.planner import zernike_block

    b, nmax, kdim = zernike_block(m, n, norm, z, it["dx"], it["dy"], it["radius"], it["wl"], origin=it["origin"],
                                  offset_deg=it["offset"], nmax=int(n.max()))
    if not it.get("enable", True):
        b = b.copy()
        b[0] = 0.0
    return b, nmax, kdim


def _run(npix, precision, m, n, norm, z, items, fields, want_wfe=False, same_as=None):
    """Upload, paos_zernike (or _like), download every item; returns (wfe of item 0 or None, outputs)."""
    from paos_amd.planner import jacobi_recurrence

    lib = _lib()
    blocks = [_block(m, n, norm, z, it) for it in items]
    nmax, kdim = blocks[0][1], blocks[0][2]
    dev = lib.DeviceFields(npix, len(items), precision)
    try:
        for i, f in enumerate(fields):
            dev.upload(i, f)
        wfe = dev.zernike(nmax, kdim, jacobi_recurrence(nmax), np.array([b[0] for b in blocks]), want_wfe=want_wfe,
                          same_as=same_as)
        return wfe, [dev.download(i) for i in range(len(items))]
    finally:
        dev.close()


def _note(kind, ratio):
    OBSERVED[kind] = ratio if OBSERVED[kind] is None else max(OBSERVED[kind], ratio)


def _check_field(got, u0, it, m, n, normalize, z, rows, cols, npix, precision, what):
    """The field at sampled pixels against u0 exp(2 pi i wfe_ld / wl); outside the disk: unchanged bit for bit."""
    ref, scale, masked = px.zernike_map(z, m, n, normalize, rows, cols, npix, it["dx"], it["dy"], it["radius"],
                                        it["offset"], it["origin"])
    nmax = int(n.max())
    g = got[rows, cols]
    u = _stored(u0, precision)[rows, cols]
    assert np.array_equal(g[masked], u[masked], equal_nan=True), f"{what}: a pixel outside the disk changed"
    ok = ~masked
    if not ok.any():
        return 0.0
    arg = (px.LD(2) * px.PI_LD) * ref[ok] / px.LD(it["wl"])
    want = u[ok].astype(np.clongdouble) * (np.cos(arg) + 1j * np.sin(arg))
    au = np.abs(u[ok])
    map_b = px.bound_map(nmax, scale[ok])
    # the map's bound through the phase, the fp64 roundings of 2 pi wfe and of its product with 1/wl (|arg| u each),
    # sincos_fast (4 u, tests/test_gpu_xprec.py) and the complex product (4 u); fp32: the store's rounding
    b = au * (2 * np.pi / it["wl"] * map_b + 2 * np.abs(arg.astype(np.float64)) * px.U64 + 8 * px.U64)
    if precision == "fp32":
        b = b + 2 * px.U32 * au
    err = np.abs(g[ok].astype(np.clongdouble) - want).astype(np.float64)
    yard_map = px.zernike_map_np(z, m, n, normalize, rows, cols, npix, it["dx"], it["dy"], it["radius"], it["offset"],
                                 it["origin"])[ok]
    yarg = 2.0 * np.pi * yard_map / it["wl"]
    yerr = np.abs((u[ok] * np.exp(1j * yarg)).astype(np.clongdouble) - want).astype(np.float64)
    worst = float(np.max(err / b))
    _note("field", worst)
    assert worst <= 1.0, (f"{what}: field error {np.max(err):.3g} is {worst:.3g} of its bound "
                          f"(max bound {np.max(b):.3g}); fp64 NumPy: {np.max(yerr / b):.3g} of the bound")
    return worst


def _check_map(wfe, it, m, n, normalize, z, rows, cols, npix, what):
    ref, scale, masked = px.zernike_map(z, m, n, normalize, rows, cols, npix, it["dx"], it["dy"], it["radius"],
                                        it["offset"], it["origin"])
    nmax = int(n.max())
    got, same = px.map_errors(wfe[rows, cols], ref, scale, masked)
    yard, _ = px.map_errors(px.zernike_map_np(z, m, n, normalize, rows, cols, npix, it["dx"], it["dy"], it["radius"],
                                              it["offset"], it["origin"]), ref, scale, masked)
    b = px.C_MAP * (nmax + 1) * px.U64
    msg = f"{what}: map error {got:.3g} x E(p), bound {b:.3g}, fp64 NumPy {yard:.3g}"
    assert same, "the mask differs -- " + msg
    assert b >= 2 * yard, "bound tighter than twice the yardstick -- " + msg
    _note("map", got / b)
    assert got <= b, msg


# ---- maps and fields: (nmax, ordering, normalize, npix, precision, dy / dx, offset, origin) ---------------------------
MAP_CASES = [
    (0, "ansi", True, 256, "fp64", 1.0, 0.0, "x"),
    (8, "ansi", True, 256, "fp64", 1.3, 30.0, "y"),
    (8, "noll", False, 2048, "fp64", 1.0, -90.0, "x"),
    (9, "standard", False, 1024, "fp32", 0.8, 30.0, "x"),
    (9, "noll", True, 256, "fp64", 0.7, 370.0, "y"),
    (20, "fringe", True, 2048, "fp32", 1.0, 370.0, "y"),
    (20, "noll", True, 4096, "fp64", 1.2, -90.0, "y"),
    (40, "standard", True, 512, "fp64", 0.9, 30.0, "x"),
    (40, "ansi", False, 4096, "fp64", 1.0, 0.0, "x"),
    (0, "fringe", False, 2048, "fp32", 1.1, -90.0, "x"),
]


@pytest.mark.parametrize("case", MAP_CASES, ids=lambda c: f"n{c[0]}-{c[1]}-{'norm' if c[2] else 'raw'}-{c[3]}-{c[4]}")
def test_zernike_map_and_field_against_long_double(case):
    """Item 0: its map (want_wfe) within bound_map with the mask bit-exact, its field within the propagated bound.
    Item 1: another radius, offset, origin and wavelength (a map of its own): its field.  Item 2: disabled, bit for bit.
    nmax 0 / 8 run the unrolled build, 9 / 20 / 40 the rolled one."""
    nmax, ordering, normalize, npix, precision, aspect, offset, origin = case
    m, n, norm, z = _tables(nmax, ordering, normalize)
    dx = 1e-5
    items = [dict(dx=dx, dy=dx * aspect, radius=0.45 * npix * dx, wl=0.6e-6, offset=offset, origin=origin),
             dict(dx=dx, dy=dx * aspect, radius=0.31 * npix * dx, wl=1.7e-6, offset=OFFSETS[(OFFSETS.index(offset) + 1) % 4],
                  origin="y" if origin == "x" else "x"),
             dict(dx=dx, dy=dx, radius=0.2 * npix * dx, wl=1e-6, offset=0.0, origin="x", enable=False)]
    fields = [_field(npix, s) for s in range(3)]
    wfe, out = _run(npix, precision, m, n, norm, z, items, fields, want_wfe=True)
    what = f"nmax {nmax} {ordering} normalize={normalize} {npix} {precision} dy/dx={aspect} offset {offset} origin {origin}"
    for i in range(2):
        rows, cols = px.sample_pixels(npix, items[i]["dx"], items[i]["dy"], items[i]["radius"],
                                      br=8, extra=384, seed=i)
        if i == 0:
            _check_map(wfe, items[0], m, n, normalize, z, rows, cols, npix, what)
        _check_field(out[i], fields[i], items[i], m, n, normalize, z, rows, cols, npix, precision, f"{what} item {i}")
    assert np.array_equal(out[2], _stored(fields[2], precision)), f"{what}: the disabled item changed"


# ---- edges of the disk and of the row window --------------------------------------------------------------------------
def _poisoned(npix, seed, it):
    """Seeded normals inside the disk, NaN / huge / tiny values outside it (the kernel must not touch those)."""
    f = _field(npix, seed).copy()
    yy, xx = np.mgrid[0:npix, 0:npix]
    x = (xx - npix // 2).astype(np.float64) * it["dx"]
    y = (yy - npix // 2).astype(np.float64) * it["dy"]
    out = np.sqrt(x * x + y * y) / it["radius"] > 1.0
    rng = np.random.default_rng(seed)
    poison = rng.choice(np.array([np.nan, 1e300, -5e-310, 3.5, np.inf]), size=out.sum()) + 1j * rng.standard_normal(out.sum())
    f[out] = poison
    return f


@pytest.mark.parametrize("precision,npix", [("fp64", 512), ("fp32", 2048)])
def test_zernike_edges_and_row_window(precision, npix):
    """The row window of zernike_apply (no wfe requested, so only [m_first, m_end) is walked) at its edges: a disk whose
    lowest rim row is the FIRST row of a block row (h = 64 rows) and one whose top rim row is the LAST row of one
    (h = 65), with exact dyadic sampling so that the axis pixels sit exactly on rho == 1; a disk larger than the grid (no
    window); a radius below one pixel (only the centre is inside).  Pixels outside the disk hold NaN / inf / huge
    values and must come back bit for bit; the rim pixels must be changed as the reference says."""
    m, n, norm, z = _tables(8, "ansi", True, seed=3)
    z = z * 3.0 + 1e-7 / len(z)  # every rim value well away from zero
    dy = 2.0**-14
    cases = [dict(dx=1.5 * dy, dy=dy, radius=64 * dy, wl=0.8e-6, offset=30.0, origin="x"),
             dict(dx=dy, dy=dy, radius=65 * dy, wl=1.1e-6, offset=0.0, origin="y"),
             dict(dx=dy, dy=dy, radius=2.0 * npix * dy, wl=1.0e-6, offset=-90.0, origin="x"),
             dict(dx=dy, dy=dy, radius=0.5 * dy, wl=0.5e-6, offset=370.0, origin="x")]
    br = 8 if (precision == "fp32" and npix >= 2048) else 4
    for k, it in enumerate(cases):
        f = _poisoned(npix, 10 + k, it)
        _, out = _run(npix, precision, m, n, norm, z, [it], [f])
        what = f"{precision} {npix} edge case {k} (radius {it['radius'] / it['dy']:.4g} rows)"
        c = npix // 2
        h = it["radius"] / it["dy"]
        if k < 2:
            top, bot = c - int(h), c + int(h)
            assert (bot % br == 0) if k == 0 else (top % br == br - 1), "the rim rows do not sit where intended"
            rows = np.array([top, top, bot, bot, c, c])
            cols = np.array([c, c + 1, c, c - 1, c - int(it["radius"] / it["dx"]), c])
            _, _, _, rho, _ = px.pixel_geometry(rows[[0, 2]], cols[[0, 2]], npix, it["dx"], it["dy"], it["radius"])
            assert np.all(rho == 1.0), "the axis rim pixels are not exactly on rho == 1"
            assert not np.array_equal(out[0][top, c], _stored(f, precision)[top, c]), f"{what}: the top rim pixel unchanged"
            assert not np.array_equal(out[0][bot, c], _stored(f, precision)[bot, c]), f"{what}: the bottom rim pixel unchanged"
        else:
            rows, cols = px.sample_pixels(npix, it["dx"], it["dy"], min(it["radius"], 0.49 * npix * it["dy"]), br=br,
                                          extra=256, seed=k)
        # every pixel outside the disk: bit for bit (NaN included)
        yy, xx = np.mgrid[0:npix, 0:npix]
        _, _, _, rho, _ = px.pixel_geometry(yy.ravel(), xx.ravel(), npix, it["dx"], it["dy"], it["radius"])
        outside = (rho > 1.0).reshape(npix, npix)
        if k == 3:
            assert outside.sum() == npix * npix - 1, "more than the centre pixel inside"
        assert np.array_equal(out[0][outside], _stored(f, precision)[outside], equal_nan=True), \
            f"{what}: a pixel outside the disk or the window changed"
        _check_field(out[0], f, it, m, n, True, z, np.concatenate([rows, [c]]), np.concatenate([cols, [c]]), npix,
                     precision, what)


# ---- wavelength groups ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("like", [False, True], ids=["zernike", "zernike_like"])
def test_zernike_groups_every_member_at_its_wavelength(like):
    """One coefficient set and sampling for 1, 7, 8, 9, 16 and 17 members at different wavelengths (one group: eight at
    a time, then the rest one by one) plus a disabled item that must come back bit for bit.  ``like``: the members hold
    copies of one field and say so (paos_zernike_like with twins); otherwise each holds its own."""
    npix = 256
    m, n, norm, z = _tables(9, "ansi", True, seed=5)
    base = dict(dx=1e-5, dy=1.2e-5, radius=0.4 * npix * 1e-5, offset=30.0, origin="y")
    rows, cols = px.sample_pixels(npix, base["dx"], base["dy"], base["radius"], extra=128, seed=2)
    for g in (1, 7, 8, 9, 16, 17):
        items = [dict(base, wl=0.5e-6 * (1.0 + 0.173 * i)) for i in range(g)]
        items.append(dict(base, wl=2e-6, enable=False))
        fields = [_field(npix, 0) if like else _field(npix, 20 + i) for i in range(g)] + [_field(npix, 99)]
        same = [0.0] * g + [float(g)] if like else None
        _, out = _run(npix, "fp64", m, n, norm, z, items, fields, same_as=same)
        for i in range(g):
            _check_field(out[i], fields[i], items[i], m, n, True, z, rows, cols, npix, "fp64",
                         f"group of {g} ({'like' if like else 'zernike'}) member {i}")
        assert np.array_equal(out[g], fields[g]), f"group of {g}: the disabled item changed"


# ---- Gram sums --------------------------------------------------------------------------------------------------------
def _pupil(npix, kind):
    if kind is None:
        return None
    yy, xx = np.mgrid[0:npix, 0:npix].astype(np.float64)
    c = npix / 2
    if kind == "ellipse":
        w = (((xx - c - 0.07 * npix) / (0.41 * npix)) ** 2 + ((yy - c + 0.03 * npix) / (0.33 * npix)) ** 2)
        return np.where(w <= 1.0, np.where(w > 0.95, 0.5, 1.0), 0.0)
    return ((np.abs(xx - c + 0.05 * npix) <= 0.36 * npix) & (np.abs(yy - c - 0.02 * npix) <= 0.27 * npix)).astype(float)


def _gram_gpu(npix, precision, m, n, norm, geo, pupil, K):
    from paos_amd.planner import gram_polynomials, jacobi_recurrence

    lib = _lib()
    b, nmax, kdim = _block(m[:K], n[:K], norm[:K], np.zeros(K), dict(geo, wl=1e-6))
    dev = lib.DeviceFields(npix, 2, precision)
    try:
        if pupil is not None:
            dev.pupil_upload(0, pupil)
            dev.pupil_upload(1, np.ones((npix, npix)))
        off = b.copy()
        off[0] = 0.0
        sums, counts = dev.zernike_gram(nmax, kdim, jacobi_recurrence(nmax), np.array([b, off]),
                                        gram_polynomials(m[:K], n[:K], norm[:K]), pupil=pupil is not None)
    finally:
        dev.close()
    assert counts[1] == 0 and not np.any(sums[1]), "the disabled item has sums"
    return sums[0], counts[0]


def _gram_ref(npix, m, n, geo, pupil, tag, normalize=True):
    """(long-double sums, envelope sums, count, fp64 NumPy sums), cached per (npix, K, tag)."""
    key = ("gram", npix, len(m), tag)
    if key not in _CACHE:
        ref, absum, count = px.gram_sums(m, n, normalize, npix, geo["dx"], geo["dy"], geo["radius"], geo["offset"],
                                         geo["origin"], pupil=pupil)
        yard = px.gram_sums_np(m, n, normalize, npix, geo["dx"], geo["dy"], geo["radius"], geo["offset"], geo["origin"],
                               pupil=pupil)
        _CACHE[key] = (ref, absum, count, yard)
    return _CACHE[key]


def _sub(vals, K, Kfull):
    """The i <= j < K entries of a row-by-row triangle of Kfull."""
    iu = np.triu_indices(Kfull)
    keep = (iu[0] < K) & (iu[1] < K)
    return np.asarray(vals)[keep]


def _check_gram(sums, count, ref, absum, cnt, yard, nmax, what):
    b = px.bound_gram(nmax, absum, cnt)
    err = np.abs(np.asarray(sums).astype(px.LD) - ref).astype(np.float64)
    yerr = np.abs(np.asarray(yard).astype(px.LD) - ref).astype(np.float64)
    msg = (f"{what}: worst sum error {np.max(err / b):.3g} of the bound ({np.max(err):.3g}); fp64 NumPy "
           f"{np.max(yerr / b):.3g} of the bound")
    assert count == cnt, f"{what}: pixel count {count} != {cnt}"
    assert np.all(b >= 2 * yerr), "bound tighter than twice the yardstick -- " + msg
    _note("gram", float(np.max(err / b)))
    assert np.all(err <= b), msg


GRAM_GEOS = {
    "plain": (None, dict(dx=1e-5, dy=1e-5, radius=0.47, offset=0.0, origin="x")),
    "ellipse-y-30": ("ellipse", dict(dx=1e-5, dy=1.1e-5, radius=0.47, offset=30.0, origin="y")),
    "rect": ("rect", dict(dx=1.2e-5, dy=1e-5, radius=0.44, offset=-90.0, origin="x")),
}


@pytest.mark.parametrize("geo_name", list(GRAM_GEOS))
def test_gram_sums_every_k_at_512(geo_name):
    """K = 1, 15, 36, 50, 51, 63, 64 at 512^2 (50 / 51: the first use of a thread's sixth pair accumulator; 64: the only
    K that uses the ninth, and 66,048 B of dynamic LDS): every sum within bound_gram of the long-double one, the count
    exact; then orthonorm_matrix of the GPU sums equals that of the long-double sums (no covariance entry near the
    1e-10 cut)."""
    from paos_amd.planner import orthonorm_matrix
    from paos_amd.zernike import zernike_tables

    npix = 512
    kind, geo = GRAM_GEOS[geo_name]
    geo = dict(geo, radius=geo["radius"] * npix * geo["dx"])  # (a fraction of the grid's width)
    m, n, norm = zernike_tables(64, "ansi", True)
    pupil = _pupil(npix, kind)
    ref, absum, cnt, yard = _gram_ref(npix, m, n, geo, pupil, geo_name)
    for K in (1, 15, 36, 50, 51, 63, 64):
        nmax = int(n[:K].max())
        sums, count = _gram_gpu(npix, "fp64", m, n, norm, geo, pupil, K)
        what = f"gram {geo_name} 512 K={K}"
        _check_gram(sums, count, _sub(ref, K, 64), _sub(absum, K, 64), cnt, _sub(yard, K, 64), nmax, what)
        if K in (15, 36):
            cov = np.asarray(_sub(ref, K, 64) / px.LD(cnt), dtype=np.float64)
            assert not np.any(np.abs(np.abs(cov) - 1e-10) <= 1e-13), f"{what}: a covariance entry is at the 1e-10 cut"
            mg = orthonorm_matrix(sums, count, K)
            ml = orthonorm_matrix(np.asarray(_sub(ref, K, 64), dtype=np.float64), cnt, K)
            my = orthonorm_matrix(_sub(yard, K, 64), cnt, K)
            full = np.empty((K, K))
            full[np.triu_indices(K)] = cov
            full.T[np.triu_indices(K)] = cov
            # first order: the sums' relative bound times the covariance's condition number
            tol = np.linalg.cond(full) * np.max(px.bound_gram(nmax, _sub(absum, K, 64), cnt)) / cnt / np.max(np.abs(full))
            d = float(np.max(np.abs(mg - ml)) / np.max(np.abs(ml)))
            dy = float(np.max(np.abs(my - ml)) / np.max(np.abs(ml)))
            msg = f"{what}: orthonorm_matrix of the GPU sums off by {d:.3g}, fp64 NumPy {dy:.3g}, bound {tol:.3g}"
            assert tol >= 2 * dy, "bound tighter than twice the yardstick -- " + msg
            assert d <= tol, msg


@pytest.mark.parametrize("npix,K,precision", [(2048, 36, "fp64"), (2048, 36, "fp32"), (4096, 15, "fp64")])
def test_gram_sums_large(npix, K, precision):
    """K = 36 at 2048^2 (fp64 and an fp32 context: 8-row blocks), K = 15 at 4096^2, origin y and an offset, no pupil."""
    from paos_amd.zernike import zernike_tables

    geo = dict(dx=1e-5, dy=0.95e-5, radius=0.3 * npix * 1e-5, offset=370.0, origin="y")
    m, n, norm = zernike_tables(K, "ansi", True)
    ref, absum, cnt, yard = _gram_ref(npix, m, n, geo, None, "large")
    sums, count = _gram_gpu(npix, precision, m, n, norm, geo, None, K)
    _check_gram(sums, count, ref, absum, cnt, yard, int(n.max()), f"gram {npix} {precision} K={K}")


def test_gram_refuses_k_above_64():
    from paos_amd.planner import gram_polynomials, jacobi_recurrence
    from paos_amd.zernike import zernike_tables

    lib = _lib()
    m, n, norm = zernike_tables(65, "ansi", True)
    b, nmax, kdim = _block(m, n, norm, np.zeros(65), dict(dx=1e-5, dy=1e-5, radius=1e-3, wl=1e-6, offset=0.0, origin="x"))
    dev = lib.DeviceFields(256, 1, "fp64")
    try:
        with pytest.raises(lib.PaosHipError, match=r"\(3\)"):
            dev.zernike_gram(nmax, kdim, jacobi_recurrence(nmax), np.array([b]), gram_polynomials(m, n, norm), pupil=False)
    finally:
        dev.close()


# ---- PSF metrics ------------------------------------------------------------------------------------------------------
def _psf_fields(npix, seeds):
    out = []
    yy, xx = np.mgrid[0:npix, 0:npix].astype(np.float64)
    for s in seeds:
        rng = np.random.default_rng(500 + s)
        cx, cy = npix * rng.uniform(0.3, 0.7, 2)
        w = npix * (0.01 + 0.03 * s)
        a = np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * w * w)) * (1.0 + 0.2 * rng.standard_normal((npix, npix)))
        out.append(a * np.exp(1j * rng.uniform(0, 6.28, (npix, npix))))
    return out


@pytest.mark.parametrize("npix,precision", [(4096, "fp64"), (2048, "fp32")])
def test_psf_metrics_against_long_double(npix, precision):
    """Three different items, 16 radii (some equal to a pixel's distance from the centre, one zero, one beyond the grid)
    about a fractional, non-symmetric centre: power, both moments (before the division) and every encircled power
    within bound_metric of the long-double sums; the peak bit for bit."""
    lib = _lib()
    fields = _psf_fields(npix, (0, 1, 2))
    centre = (npix / 2 + 37.25, npix / 2 - 101.625)
    radii = [0.0, 1.0, float(np.hypot(7 - 0.25, 3 + 0.625)), 10.0, 25.5, float(np.hypot(40 - 0.25, 41 - 0.375)), 64.0,
             100.0, 150.25, 200.0, 333.0, 500.0, 0.3 * npix, 0.45 * npix, 0.7 * npix, 2.0 * npix]
    dev = lib.DeviceFields(npix, 3, precision)
    try:
        for i, f in enumerate(fields):
            dev.upload(i, f)
        res = dev.psf_metrics(radii, centre)
        stored = [dev.download(i) for i in range(3)]
    finally:
        dev.close()
    for i in range(3):
        assert np.array_equal(stored[i], _stored(fields[i], precision))
        ref, scales = px.psf_metrics(stored[i], radii, centre)
        yard = px.psf_metrics_np(stored[i], radii, centre)
        r = res[i]
        got = np.array([r["power"], r["centroid"][0] * r["power"], r["centroid"][1] * r["power"], r["peak"], *r["encircled"]])
        b = px.bound_metric(npix * npix, scales)
        # (the moments come back divided by the power: multiplied back, one more rounding each way)
        slack = np.zeros_like(b)
        slack[1:3] = 4 * px.U64 * np.abs(got[1:3])
        err = np.abs(got.astype(px.LD) - ref).astype(np.float64)
        yerr = np.abs(yard.astype(px.LD) - ref).astype(np.float64)
        what = f"metrics {npix} {precision} item {i}"
        assert got[3] == float(ref[3]), f"{what}: peak {got[3]!r} != {float(ref[3])!r}"
        keep = np.arange(b.size) != 3
        bb = b[keep] + slack[keep]
        ratio = np.divide(err[keep], bb, out=np.where(err[keep] > 0, np.inf, 0.0), where=bb > 0)  # (an empty circle: exact)
        msg = (f"{what}: worst {np.max(ratio):.3g} of the bound (errors {err[keep]}); fp64 NumPy "
               f"{np.max(np.divide(yerr[keep], bb, out=np.zeros_like(bb), where=bb > 0)):.3g} of the bound")
        assert np.all(b[keep] >= 2 * yerr[keep]), "bound tighter than twice the yardstick -- " + msg
        _note("metric", float(np.max(ratio)))
        assert np.all(ratio <= 1.0), msg


# ---- host refusals ------------------------------------------------------------------------------------------------------
def test_psf_metrics_refuses_bad_radii_and_centre():
    lib = _lib()
    dev = lib.DeviceFields(256, 1, "fp64")
    try:
        dev.fill(1.0)
        for radii, centre in (([1.0, -2.0], None), ([np.nan], None), ([np.inf], None), ([3.0], (np.nan, 1.0)),
                              ([3.0], (1.0, np.inf))):
            with pytest.raises(lib.PaosHipError, match=r"\(1\)"):
                dev.psf_metrics(radii, centre)
        assert dev.psf_metrics([0.0, 3.0], (128.5, 127.25))[0]["power"] == 256 * 256
    finally:
        dev.close()


def test_zernike_refuses_nan_requests():
    """A NaN coefficient, a non-finite offset or a radius <= 0 would give NaN inside the disk, which the wfe map reports
    as masked: WFO.zernikes raises ValueError, and the C ABI refuses such a record (PAOS_EINVAL) -- the field untouched."""
    from paos_amd.wfo import WFO

    lib = _lib()
    wfo = WFO(0.01, 1e-6, 256, 4)
    try:
        for kw in (dict(Z=[0.0, np.nan, 1e-7], radius=0.005), dict(Z=[0.0, 1e-7, 1e-7], radius=0.005, offset=np.inf),
                   dict(Z=[1e-7] * 3, radius=0.0), dict(Z=[1e-7] * 3, radius=-0.005), dict(Z=[1e-7] * 3, radius=np.nan)):
            z = kw.pop("Z")
            with pytest.raises(ValueError):
                wfo.zernikes(np.arange(3), z, "ansi", True, **kw)
        assert np.array_equal(wfo.wfo, np.ones((256, 256), dtype=complex))
    finally:
        wfo._dev.close()
    m, n, norm, z = _tables(2, "ansi", True)
    from paos_amd.planner import jacobi_recurrence

    good, nmax, kdim = _block(m, n, norm, z, dict(dx=1e-5, dy=1e-5, radius=1e-3, wl=1e-6, offset=0.0, origin="x"))
    dev = lib.DeviceFields(256, 1, "fp64")
    try:
        dev.fill(1.0)
        for k, v in ((lib.ZERNIKE_HEAD + 1, np.nan), (3, 0.0), (3, -1e-3), (5, np.inf)):
            bad = good.copy()
            bad[k] = v
            with pytest.raises(lib.PaosHipError, match=r"\(1\)"):
                dev.zernike(nmax, kdim, jacobi_recurrence(nmax), np.array([bad]), want_wfe=True)
        assert np.array_equal(dev.download(0), np.ones((256, 256), dtype=complex))
    finally:
        dev.close()


def test_zzz_report_observed():
    """(last in the module) the largest errors seen, as fractions of their bounds -- for the constants' record."""
    print("\nXPREC pointwise observed (fraction of bound):", {k: (None if v is None else float(f"{v:.3g}"))
                                                           for k, v in OBSERVED.items()})
