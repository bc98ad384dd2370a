"""References of the wavefront fits (csrc/wavefront_pass.h, paos_amd/wavefront.py; README.md, "Wavefront fits").

* ``fit_sums_np``: the fp64 NumPy restatement of what the device returns -- the summary and the Gram matrix of the columns
  ``[Z_0 .. Z_{K-1}, phi]`` -- with the membership and the ``re'`` / ``im'`` operations written exactly as the definition
  has them (one rounding per operation; NumPy does not contract);
* ``fit_sums_ld``: the long-double reference -- it takes those fp64 ``re'``, ``im'``, evaluates ``atan2`` in long double,
  takes the polynomials from ``pointwise_xprec.zernike_terms`` and sums in long double -- with the bound of every value,
  built from the project's constants (``bound_gram``, ``C_METRIC``) and ``E_phi``, which is measured on the reference;
* ``WavefrontModelDevice``: ``fakes.ModelDevice`` with ``wavefront_fit`` / ``wavefront_fetch`` for the host tests.

Test infrastructure."""
import numpy as np

import pointwise_xprec as px
from fakes import ModelDevice

LD = np.longdouble
U64 = px.U64
SUMMARY = 10  # count, r_re, r_im, sum sqrt(I), sum I, phi_min, phi_max, fallback, sum w, sum w phi


def support(u, dx, dy, radius, min_intensity=0.0, pupil=None):
    """(rows, cols, ux, uy, I) of the pixels of Omega in row-major order: rho <= 1 with the kernels' geometry
    (pointwise_xprec.pixel_geometry), I = fl(fl(re re) + fl(im im)) > min_intensity, pupil weight != 0.  Only the box the
    disk can reach (two pixels of margin) is looked at."""
    u = np.asarray(u)
    n = u.shape[0]
    hx, hy = min(radius / abs(dx), n) if dx else n, min(radius / abs(dy), n) if dy else n
    c0, c1 = max(0, int(n // 2 - hx) - 2), min(n, int(n // 2 + hx) + 3)
    r0, r1 = max(0, int(n // 2 - hy) - 2), min(n, int(n // 2 + hy) + 3)
    rg, cg = np.meshgrid(np.arange(r0, r1), np.arange(c0, c1), indexing="ij")
    rg, cg = rg.ravel(), cg.ravel()
    x = (cg - n // 2).astype(np.float64) * dx
    y = (rg - n // 2).astype(np.float64) * dy
    rho = np.sqrt(x * x + y * y) / radius
    I = px.intensity(u[r0:r1, c0:c1]).ravel()
    member = (rho <= 1.0) & (I > min_intensity)
    if pupil is not None:
        member &= np.asarray(pupil)[rg, cg] != 0.0
    rg, cg = rg[member], cg[member]
    return rg, cg, u[rg, cg].real.astype(np.float64), u[rg, cg].imag.astype(np.float64), I[member]


def used_phasor(re, im):
    """(rx, ry, fallback): the reference phasor that is used -- 1 + 0i if the sum is zero or not finite."""
    fallback = (re == 0.0 and im == 0.0) or not (np.isfinite(re) and np.isfinite(im))
    return (1.0, 0.0, True) if fallback else (float(re), float(im), False)


def turned(ux, uy, rx, ry):
    """re', im' in fp64: re' = fl(fl(ux rx) + fl(uy ry)), im' = fl(fl(uy rx) - fl(ux ry))."""
    return ux * rx + uy * ry, uy * rx - ux * ry


def pack(columns, ux, uy, I, weight, r=None):
    """(summary[SUMMARY], sums[(K + 1)(K + 2) / 2]) in fp64 from the K polynomial columns at the pixels of Omega."""
    k = len(columns)
    summary = np.zeros(SUMMARY)
    sums = np.zeros((k + 1) * (k + 2) // 2)
    count = len(I)
    if count == 0:
        return summary, sums
    re, im = (np.sum(ux), np.sum(uy)) if r is None else r
    rx, ry, fallback = used_phasor(re, im)
    rp, ip = turned(ux, uy, rx, ry)
    phi = np.arctan2(ip, rp)
    w = I if weight == "intensity" else np.ones(count)
    cols = list(columns) + [phi]
    q = 0
    for i in range(k + 1):
        for j in range(i, k + 1):
            sums[q] = np.sum((w * cols[i]) * cols[j])
            q += 1
    summary[:] = [count, re, im, np.sum(np.sqrt(I)), np.sum(I), phi.min(), phi.max(), float(fallback), np.sum(w), np.sum(w * phi)]
    return summary, sums


def fit_sums_np(u, m, n, normalize, dx, dy, radius, offset_deg=0.0, origin="x", weight="uniform", min_intensity=0.0,
                pupil=None, r=None):
    """The fp64 restatement for one item (polynomials of oracle/zernike_np.py, plain np.sum).  ``r``: a reference phasor
    sum to use instead of the field's own."""
    rg, cg, ux, uy, I = support(u, dx, dy, radius, min_intensity, pupil)
    cols = columns_np(rg, cg, np.asarray(u).shape[0], m, n, normalize, dx, dy, radius, offset_deg, origin)
    return pack(cols, ux, uy, I, weight, r)


def columns_np(rg, cg, npix, m, n, normalize, dx, dy, radius, offset_deg=0.0, origin="x"):
    """The K polynomials at pixels (rg[i], cg[i]) in fp64, by oracle/zernike_np.py (the reference's own formulas)."""
    from oracle import zernike_np

    x, y, _, rho, _ = px.pixel_geometry(rg, cg, npix, dx, dy, radius, origin)
    phi = (np.arctan2(y, x) if origin == "x" else np.arctan2(x, y)) + np.deg2rad(offset_deg)
    m, n = np.asarray(m, dtype=int), np.asarray(n, dtype=int)
    cols = []
    for mj, nj, nr in zip(m, n, zernike_np.norms(m, n, normalize)):
        az = np.ones_like(phi) if mj == 0 else (np.cos(mj * phi) if mj > 0 else np.sin(-mj * phi))
        cols.append(nr * zernike_np.radial(mj, nj, np.minimum(rho, 1.0)) * az)
    return cols


def aberrated_field(npix, m, n, normalize, coeffs, wl, dx, dy, radius, amplitude=None, offset_deg=0.0, origin="x"):
    """a exp(2 pi i wfe / wl) on the whole grid, wfe = sum_j coeffs[j] Z_j inside the disk and 0 outside it (what
    WFO.zernikes leaves of a field a): the input of the round-trip tests."""
    rg, cg = np.meshgrid(np.arange(npix), np.arange(npix), indexing="ij")
    cols = columns_np(rg.ravel(), cg.ravel(), npix, m, n, normalize, dx, dy, radius, offset_deg, origin)
    rho = px.pixel_geometry(rg.ravel(), cg.ravel(), npix, dx, dy, radius, origin)[3]
    wfe = np.where(rho <= 1.0, sum(c * z for c, z in zip(coeffs, cols)), 0.0).reshape(npix, npix)
    a = np.ones((npix, npix)) if amplitude is None else amplitude
    return a * np.exp(2j * np.pi * wfe / wl)


def moments_ld(u, dx, dy, radius, min_intensity=0.0, pupil=None):
    """(values, bounds) of count, r_re, r_im, sum sqrt(I), sum I in long double: the bounds are the metric bound
    C_METRIC log2(count) u sum |term| (count: exact)."""
    _, _, ux, uy, I = support(u, dx, dy, radius, min_intensity, pupil)
    count = len(I)
    terms = [ux.astype(LD), uy.astype(LD), np.sqrt(I.astype(LD)), I.astype(LD)]
    vals = np.array([LD(count)] + [np.sum(t) for t in terms], dtype=LD)
    # (sqrt is rounded once more per term than a sum's own terms: one u of the term, inside C_METRIC log2(count) >= 2)
    scale = np.array([0.0] + [float(np.sum(np.abs(t))) for t in terms])
    return vals, px.C_METRIC * np.log2(max(2, count)) * U64 * scale


def fit_sums_ld(u, m, n, normalize, dx, dy, radius, r, offset_deg=0.0, origin="x", weight="uniform", min_intensity=0.0,
                pupil=None):
    """The long-double reference of the phase sums for one item, about the reference phasor sum ``r`` = (re, im) given
    (the GPU tests pass the device's, held to ``moments_ld`` first, so that the two references do not stack).  Returns a
    dict: ``sums`` / ``sums_bound`` [(K + 1)(K + 2) / 2]; ``sw``, ``swphi``, ``phi_min``, ``phi_max`` with their bounds;
    ``e_phi``; ``count``."""
    rg, cg, ux, uy, I = support(u, dx, dy, radius, min_intensity, pupil)
    m, n = np.asarray(m, dtype=int), np.asarray(n, dtype=int)
    k, count, nmax = len(m), len(I), int(n.max())
    out = {"count": count, "sums": np.zeros((k + 1) * (k + 2) // 2, dtype=LD), "sums_bound": np.zeros((k + 1) * (k + 2) // 2),
           "sw": LD(0), "sw_bound": 0.0, "swphi": LD(0), "swphi_bound": 0.0, "phi_min": 0.0, "phi_max": 0.0,
           "e_phi": 2.0 * U64 * np.pi}
    if count == 0:
        return out
    rx, ry, _ = used_phasor(*r)
    rp, ip = turned(ux, uy, rx, ry)
    phi = np.arctan2(ip.astype(LD), rp.astype(LD))
    # E_phi: 4 x the largest error of np.arctan2 against long double on these very inputs, floored at 2 u pi
    e_phi = max(4.0 * float(np.max(np.abs(np.arctan2(ip, rp).astype(LD) - phi))), 2.0 * U64 * np.pi)
    _, _, _, rho, ang = px.pixel_geometry(rg, cg, np.asarray(u).shape[0], dx, dy, radius, origin)
    vals, envs = px.zernike_terms(m, n, normalize, rho, ang, offset_deg)
    w = I.astype(LD) if weight == "intensity" else np.ones(count, dtype=LD)
    aphi = np.abs(phi)
    q = 0
    for i in range(k + 1):
        for j in range(i, k + 1):
            ci, cj = (vals[i] if i < k else phi), (vals[j] if j < k else phi)
            out["sums"][q] = np.sum(w * ci * cj)
            if j < k:
                out["sums_bound"][q] = px.bound_gram(nmax, float(np.sum(w * envs[i] * envs[j])), count)
            elif i < k:
                out["sums_bound"][q] = (px.bound_gram(nmax, float(np.sum(w * envs[i] * aphi)), count)
                                        + e_phi * float(np.sum(w * envs[i])))
            else:
                out["sums_bound"][q] = px.bound_gram(nmax, float(np.sum(w * phi * phi)), count) + 2.0 * e_phi * float(np.sum(w * aphi))
            q += 1
    metric = px.C_METRIC * np.log2(max(2, count)) * U64
    out.update(sw=np.sum(w), sw_bound=metric * float(np.sum(w)), swphi=np.sum(w * phi),
               swphi_bound=metric * float(np.sum(w * aphi)) + e_phi * float(np.sum(w)),
               phi_min=float(phi.min()), phi_max=float(phi.max()), e_phi=e_phi)
    return out


class WavefrontModelDevice(ModelDevice):
    """``fakes.ModelDevice`` plus the wavefront calls of ``DeviceFields``: the polynomials by the kernels' recurrences
    (``_zernike_terms``), the sums by ``pack``."""

    def wavefront_fit(self, nmax, kdim, table, blocks, poly, weight=0, min_intensity=None, pupil=False):
        self.log.append(("wavefront_fit", len(poly)))
        table = np.asarray(table).reshape(nmax + 1, kdim, 3)
        poly = np.asarray(poly)
        floors = np.zeros(self.batch) if min_intensity is None else np.broadcast_to(np.asarray(min_intensity, dtype=np.float64), (self.batch,))
        k = len(poly)
        self._wf = (np.zeros((self.batch, SUMMARY)), np.zeros((self.batch, (k + 1) * (k + 2) // 2)))
        for i, b in enumerate(np.asarray(blocks)):
            if not b[0]:
                continue
            rho, terms = self._zernike_terms(nmax, kdim, table, b)
            lookup = {(am, kk): (base, cm, sm) for am, kk, base, cm, sm in terms}
            I = px.intensity(self.u[i])
            member = (rho <= 1.0) & (I > floors[i])
            if pupil:
                member &= self.pupil[i] != 0.0
            cols = []
            for am, kk, is_sin, fac in poly:
                base, cm, sm = lookup[(int(am), int(kk))]
                cols.append((fac * base * (sm if is_sin else cm))[member])
            u = self.u[i][member]
            self._wf[0][i], self._wf[1][i] = pack(cols, u.real.copy(), u.imag.copy(), I[member],
                                                  "intensity" if weight else "uniform")

    def wavefront_fetch(self):
        if not hasattr(self, "_wf"):
            raise RuntimeError("paos_wavefront_fetch failed (1): no wavefront fit computed (paos_wavefront_fit)")
        return self._wf[0].copy(), self._wf[1].copy()
