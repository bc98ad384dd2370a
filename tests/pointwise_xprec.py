"""Extended-precision restatements of the pointwise kernels that do their own arithmetic (csrc/pointwise.h:
zernike_kernel, zernike_gram_kernel + zernike_gram_final_kernel, psf_metrics_kernel + psf_metrics_final_kernel) -- the
yardstick they are held to at the 1e-16 level (tests/test_gpu_pointwise_xprec.py).

What is formed in fp64, exactly as the reference and the kernels form it, so that every decision is shared bit for bit:

* Zernike: pixel coordinates x = (c - n//2) dx, y = (r - n//2) dy, rr = sqrt(x^2 + y^2), rho = rr / radius (wfo.py:620-633)
  and so the mask rho > 1 (and the pupil's);
* PSF metrics: the intensity I = re^2 + im^2 of the stored field, and which pixels lie inside a radius
  (d2 = dx^2 + dy^2 <= r^2 with dx = col - cx, dy = row - cy, no contraction -- the documented semantics).

What is evaluated in ``np.longdouble`` (x87 80-bit, eps ~1.1e-19): the radial part (-1)^k rho^|m| P_k^(|m|,0)(1 - 2 rho^2)
by its three-term recurrence with coefficients formed in long double, cos / sin(m phi) with phi = atan2(.) + offset in
long double, the normalisation, the sum over terms, the Gram sums and the metric sums.

Each check holds the kernel to a ``bound_*``: a stated multiple of u times the case's own scale.  Test infrastructure.
"""
import numpy as np

from xprec_np import U32, U64, require_long_double  # noqa: F401  (re-exported: one guard, one u for both references)

LD = np.longdouble
TWO_PI = 6.283185307179586
PI_LD = LD("3.14159265358979323846264338327950288")

# Multiples of u in the bounds (see bound_map / bound_gram / bound_metric).  Chosen from the fp64 NumPy restatements on
# the CPU (every bound at least twice what they reach, tests/test_pointwise_xprec_reference.py) and confirmed on an MI355X;
# the largest GPU error observed is beside each (tests/test_gpu_pointwise_xprec.py: OBSERVED_MI355X, fraction of bound).
C_MAP = 4.0     # map: C_MAP (nmax + 1) u E(p); observed 0.85 (nmax + 1) u E(p)
C_GRAM = 8.0    # Gram sum: C_GRAM (nmax + 1 + log2(count)) u sum_p E_i E_j; observed 0.37 (...)
C_METRIC = 2.0  # metric sum: C_METRIC log2(npix) u sum_p |term|; observed 0.43 log2(npix) u sum


# ---- Zernike ------------------------------------------------------------------------------------------------------
def pixel_geometry(rows, cols, n, dx, dy, radius, origin="x"):
    """fp64 x, y, rr, rho of pixels (rows[i], cols[i]) -- wfo.py:620-627, one rounding per operation like the kernels;
    and the long-double angle atan2 (origin x: atan2(y, x); origin y: atan2(x, y), wfo.py:629-632)."""
    r = np.asarray(rows, dtype=np.int64)
    c = np.asarray(cols, dtype=np.int64)
    x = (c - n // 2).astype(np.float64) * dx
    y = (r - n // 2).astype(np.float64) * dy
    rr = np.sqrt(x * x + y * y)
    rho = rr / radius
    a, b = (y, x) if origin == "x" else (x, y)
    phi = np.arctan2(a.astype(LD), b.astype(LD))
    return x, y, rr, rho, phi


def jacobi_ld(k_max, a, xj):
    """[P_0 .. P_k_max] of P_k^(a,0)(xj) in long double: the standard three-term recurrence, coefficients in long double."""
    xj = np.asarray(xj, dtype=LD)
    out = [np.ones_like(xj)]
    if k_max >= 1:
        out.append((LD(a + 2) * xj + LD(a)) / LD(2))
    for k in range(2, k_max + 1):
        kk, aa = LD(k), LD(a)
        den = LD(2) * kk * (kk + aa) * (LD(2) * kk + aa - LD(2))
        c1 = (LD(2) * kk + aa - LD(1)) * (LD(2) * kk + aa) * (LD(2) * kk + aa - LD(2))
        c2 = (LD(2) * kk + aa - LD(1)) * aa * aa
        c3 = LD(2) * (kk + aa - LD(1)) * (kk - LD(1)) * (LD(2) * kk + aa)
        out.append(((c1 * xj + c2) * out[-1] - c3 * out[-2]) / den)
    return out


def zernike_terms(m, n, normalize, rho, phi, offset_deg=0.0):
    """Per polynomial j: (value_j, envelope_j) at the pixels, long double.  value_j = norm_j R_j Phi_j.  envelope_j =
    norm_j rho^|m| max_{i <= k} |P_i|: the size of what the recurrences carry (a rounding error of the kernel is a few u
    of it, also where R_j or Phi_j pass through zero)."""
    rho_ld = np.asarray(rho, dtype=np.float64).astype(LD)
    ph = np.asarray(phi, dtype=LD) + LD(offset_deg) * PI_LD / LD(180)
    xj = LD(1) - LD(2) * rho_ld * rho_ld
    m = np.asarray(m, dtype=int)
    n = np.asarray(n, dtype=int)
    cache = {}
    vals, envs = [], []
    for mj, nj in zip(m, n):
        am, k = abs(int(mj)), (int(nj) - abs(int(mj))) // 2
        if am not in cache:
            cache[am] = jacobi_ld((int(n.max()) - am) // 2, am, xj)
        ps = cache[am]
        env = np.max(np.abs(np.stack(ps[:k + 1])), axis=0) * rho_ld**am
        rad = LD(-1) ** k * rho_ld**am * ps[k]
        az = np.ones_like(ph) if mj == 0 else (np.cos(LD(am) * ph) if mj > 0 else np.sin(LD(am) * ph))
        nrm = (np.sqrt(LD(nj + 1)) if mj == 0 else np.sqrt(LD(2) * LD(nj + 1))) if normalize else LD(1)
        vals.append(nrm * rad * az)
        envs.append(nrm * env)
    return vals, envs


def zernike_map(coeffs, m, n, normalize, rows, cols, npix, dx, dy, radius, offset_deg=0.0, origin="x", pupil=None):
    """(wfe (long double, NaN where masked), E(p), masked) at pixels (rows[i], cols[i]) of an npix^2 grid.  E(p) =
    sum_j |Z_j| envelope_j (zernike_terms).  ``pupil``: n x n weights, 0 = masked."""
    x, y, rr, rho, phi = pixel_geometry(rows, cols, npix, dx, dy, radius, origin)
    masked = rho > 1.0
    if pupil is not None:
        masked = masked | (np.asarray(pupil)[np.asarray(rows), np.asarray(cols)] == 0.0)
    vals, envs = zernike_terms(m, n, normalize, np.where(masked, 0.0, rho), phi, offset_deg)
    wfe = np.zeros(len(x), dtype=LD)
    scale = np.zeros(len(x), dtype=LD)
    for z, v, e in zip(np.asarray(coeffs, dtype=np.float64), vals, envs):
        wfe += LD(z) * v
        scale += abs(LD(z)) * e
    wfe[masked] = LD(np.nan)
    return wfe, scale, masked


def zernike_map_np(coeffs, m, n, normalize, rows, cols, npix, dx, dy, radius, offset_deg=0.0, origin="x"):
    """The fp64 NumPy restatement of the reference on the same pixels (oracle/zernike_np.py: scipy's Jacobi polynomials,
    rho**m, cos(m phi) with phi = atan2 + deg2rad(offset) in fp64) -- the yardstick."""
    from oracle import zernike_np

    x, y, rr, rho, _ = pixel_geometry(rows, cols, npix, dx, dy, radius, origin)
    phi = (np.arctan2(y, x) if origin == "x" else np.arctan2(x, y)) + np.deg2rad(offset_deg)
    m = np.asarray(m, dtype=int)
    n = np.asarray(n, dtype=int)
    nrm = zernike_np.norms(m, n, normalize)
    out = np.zeros(len(x))
    for z, mj, nj, nr in zip(np.asarray(coeffs, dtype=np.float64), m, n, nrm):
        az = np.ones_like(phi) if mj == 0 else (np.cos(mj * phi) if mj > 0 else np.sin(-mj * phi))
        out += z * (nr * zernike_np.radial(mj, nj, rho) * az)
    return np.where(rho > 1.0, np.nan, out)


def bound_map(nmax, scale, u=U64):
    """Per-pixel bound of a Zernike map value: C_MAP (nmax + 1) u E(p) -- the recurrences in rho, x and the angle run
    over at most nmax + 1 steps, each adding a few u of what they carry."""
    return C_MAP * (nmax + 1) * u * np.asarray(scale, dtype=np.float64)


def map_errors(got, ref, scale, masked):
    """(max error / E(p) over the unmasked pixels, mask agreement).  ``got``: fp64 map values (NaN = masked)."""
    got = np.asarray(got, dtype=np.float64)
    same_mask = bool(np.array_equal(np.isnan(got), masked))
    ok = ~masked
    if not ok.any():
        return 0.0, same_mask
    err = np.abs(got[ok].astype(LD) - ref[ok]) / np.maximum(scale[ok], LD(1e-300))
    return float(np.max(err)), same_mask


def sample_pixels(npix, dx, dy, radius, br=8, extra=256, seed=0):
    """(rows, cols) to check a map on: the centre; the whole centre row and column near the rim; the rows of the rim
    (first and last row inside the disk, one either side) and of block-row edges near it; both axes' rim pixels; a
    seeded random set over the grid.  Duplicates removed."""
    c = npix // 2
    rr, cc = [], []

    def add(r, cl):
        r = np.atleast_1d(np.asarray(r, dtype=np.int64))
        cl = np.atleast_1d(np.asarray(cl, dtype=np.int64))
        r, cl = np.broadcast_arrays(r, cl)
        keep = (r >= 0) & (r < npix) & (cl >= 0) & (cl < npix)
        rr.append(r[keep])
        cc.append(cl[keep])

    add(c, c)
    half_r = radius / dy
    half_c = radius / dx
    edge_cols = np.unique(np.clip(np.array([c - int(np.floor(half_c)) + d for d in (-1, 0, 1)]
                                           + [c + int(np.floor(half_c)) + d for d in (-1, 0, 1)]), 0, npix - 1))
    edge_rows = np.unique(np.clip(np.array([c - int(np.floor(half_r)) + d for d in (-2, -1, 0, 1)]
                                           + [c + int(np.floor(half_r)) + d for d in (-1, 0, 1, 2)]), 0, npix - 1))
    axis = np.unique(np.clip(np.linspace(0, npix - 1, 129).astype(np.int64), 0, npix - 1))
    add(c, axis)
    add(axis, c)
    add(c, edge_cols)
    add(edge_rows, c)
    # block-row edges next to the rim rows, and the rim rows themselves, across their whole chord
    for r in edge_rows:
        for rb in (r - r % br, r - r % br + br - 1):
            add(rb, np.linspace(0, npix - 1, 33).astype(np.int64))
        add(r, np.linspace(0, npix - 1, 65).astype(np.int64))
    rng = np.random.default_rng(seed)
    add(rng.integers(0, npix, extra), rng.integers(0, npix, extra))
    r = np.concatenate(rr)
    cl = np.concatenate(cc)
    key = np.unique(r * npix + cl)
    return key // npix, key % npix


# ---- Gram sums --------------------------------------------------------------------------------------------------------
def gram_sums(m, n, normalize, npix, dx, dy, radius, offset_deg=0.0, origin="x", pupil=None, chunk_rows=64):
    """(sums[K(K+1)/2] long double, abs-envelope sums[K(K+1)/2] (sum_p E_i E_j, see zernike_terms), count): sums of Z_i
    Z_j (i <= j, row by row) over the unmasked pixels of the whole grid, in row chunks."""
    k = len(m)
    iu = np.triu_indices(k)
    sums = np.zeros(len(iu[0]), dtype=LD)
    absum = np.zeros(len(iu[0]), dtype=LD)
    count = 0
    cols = np.arange(npix)
    for r0 in range(0, npix, chunk_rows):
        rows = np.arange(r0, min(npix, r0 + chunk_rows))
        rg, cg = np.meshgrid(rows, cols, indexing="ij")
        rg, cg = rg.ravel(), cg.ravel()
        _, _, _, rho, phi = pixel_geometry(rg, cg, npix, dx, dy, radius, origin)
        valid = rho <= 1.0
        if pupil is not None:
            valid &= np.asarray(pupil)[rg, cg] != 0.0
        if not valid.any():
            continue
        count += int(valid.sum())
        vals, envs = zernike_terms(m, n, normalize, rho[valid], phi[valid], offset_deg)
        for q, (i, j) in enumerate(zip(*iu)):
            sums[q] += np.sum(vals[i] * vals[j])
            absum[q] += np.sum(envs[i] * envs[j])
    return sums, absum, count


def gram_sums_np(m, n, normalize, npix, dx, dy, radius, offset_deg=0.0, origin="x", pupil=None, chunk_rows=256):
    """The fp64 restatement (oracle/zernike_np.py polynomials, np.sum per pair per chunk, chunk sums added in fp64):
    the yardstick of the Gram sums."""
    from oracle import zernike_np

    k = len(m)
    iu = np.triu_indices(k)
    sums = np.zeros(len(iu[0]))
    nrm = zernike_np.norms(m, n, normalize)
    cols = np.arange(npix)
    for r0 in range(0, npix, chunk_rows):
        rows = np.arange(r0, min(npix, r0 + chunk_rows))
        rg, cg = np.meshgrid(rows, cols, indexing="ij")
        rg, cg = rg.ravel(), cg.ravel()
        x, y, _, rho, _ = pixel_geometry(rg, cg, npix, dx, dy, radius, origin)
        valid = rho <= 1.0
        if pupil is not None:
            valid &= np.asarray(pupil)[rg, cg] != 0.0
        if not valid.any():
            continue
        phi = (np.arctan2(y, x) if origin == "x" else np.arctan2(x, y))[valid] + np.deg2rad(offset_deg)
        z = []
        for mj, nj, nr in zip(m, n, nrm):
            az = np.ones_like(phi) if mj == 0 else (np.cos(mj * phi) if mj > 0 else np.sin(-mj * phi))
            z.append(nr * zernike_np.radial(mj, nj, rho[valid]) * az)
        for q, (i, j) in enumerate(zip(*iu)):
            sums[q] += np.sum(z[i] * z[j])
    return sums


def bound_gram(nmax, absum, count, u=U64):
    """Per-sum bound: C_GRAM (nmax + 1 + log2(count)) u sum_p E_i E_j -- each product carries the two maps' errors
    (bound_map), and the sums over ``count`` pixels add a few u per level of a reduction tree of sum_p |Z_i Z_j| <=
    sum_p E_i E_j."""
    return C_GRAM * (nmax + 1 + np.log2(max(2, count))) * u * np.asarray(absum, dtype=np.float64)


# ---- PSF metrics --------------------------------------------------------------------------------------------------
def intensity(u):
    """I = re^2 + im^2 of the stored field in fp64 (the kernel's expression: the peak is compared bit for bit)."""
    u = np.asarray(u)
    re = u.real.astype(np.float64)
    im = u.imag.astype(np.float64)
    return re * re + im * im


def psf_metrics(u, radii, centre):
    """(values, scales) of one item, each [4 + nr]: power, sum I col, sum I row, peak, power within each radius -- sums
    in long double; the scale of each is the sum of its terms' magnitudes (the peak: itself).  Membership of a radius:
    fp64 d2 = dx^2 + dy^2 <= r^2 (dx = col - cx, dy = row - cy)."""
    I = intensity(u)
    npix = I.shape[0]
    cx, cy = centre
    Il = I.astype(LD)
    rows = np.arange(npix, dtype=np.float64)
    cols = np.arange(npix, dtype=np.float64)
    power = np.sum(Il)
    mx = np.sum(Il * cols.astype(LD)[None, :])
    my = np.sum(Il * rows.astype(LD)[:, None])
    vals = [power, mx, my, LD(np.max(I))]
    dxv = cols - cx
    dyv = rows - cy
    for r in radii:
        r2 = float(r) * float(r)
        lo = max(0, int(np.floor(cy - abs(r))) - 1)
        hi = min(npix, int(np.ceil(cy + abs(r))) + 2)
        d2 = (dxv * dxv)[None, :] + (dyv[lo:hi] * dyv[lo:hi])[:, None]
        vals.append(np.sum(np.where(d2 <= r2, Il[lo:hi], LD(0))))
    vals = np.array(vals, dtype=LD)
    scales = vals.copy()  # every term is >= 0 (rows, cols >= 0): the sums are their own magnitude
    return vals, scales


def psf_metrics_np(u, radii, centre):
    """fp64 restatement with plain np.sum: the yardstick."""
    I = intensity(u)
    npix = I.shape[0]
    cx, cy = centre
    rows = np.arange(npix, dtype=np.float64)
    cols = np.arange(npix, dtype=np.float64)
    out = [np.sum(I), np.sum(I * cols[None, :]), np.sum(I * rows[:, None]), np.max(I)]
    d2 = ((cols - cx) ** 2)[None, :] + ((rows - cy) ** 2)[:, None]
    for r in radii:
        out.append(np.sum(I[d2 <= float(r) * float(r)]))
    return np.array(out)


def bound_metric(npix2, scales, u=U64):
    """Per-value bound of a metric sum: C_METRIC log2(npix2) u (sum of its terms); the peak (index 3) is exact."""
    b = C_METRIC * np.log2(max(2, npix2)) * u * np.asarray(scales, dtype=np.float64)
    b[3] = 0.0
    return b
