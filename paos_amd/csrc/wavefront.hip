// wavefront.hip -- wavefront fits: Zernike content and OPD statistics of the field (paos_wavefront_*; kernels: wavefront_pass.h).
#include "host.h"

#include <algorithm>
#include <cmath>

#include "wavefront_pass.h"

namespace {

// workgroups of launch 1 / launch 2 per item: functions of the grid alone, so that an item's sums are added in the same
// order whatever the batch
int moment_blocks(const paos_ctx* c) {
  return (int)std::min<size_t>(std::max<size_t>(c->item_stride / (kPwThreads * 16), 1), 256);
}
int gram_blocks(const paos_ctx* c) {
  const size_t chunks = ((size_t)c->item_stride + kGramPix - 1) / kGramPix;
  return (int)std::min<size_t>(std::max<size_t>(chunks / 128, 1), 128);
}

// the pixels [lo, hi) along one axis that a disk of `half` pixels about n / 2 can reach, one pixel of margin either side
void reach(int n, double half, double* out) {
  const double mid = (double)(n / 2);
  out[0] = std::max(0.0, std::floor(mid - half) - 1.0);
  out[1] = std::min((double)n, std::ceil(mid + half) + 2.0);
}

}  // namespace

extern "C" {

int paos_wavefront_fit(paos_ctx* c, int nmax, int kdim, const double* table, const double* params, int param_stride, int K,
                       const double* poly, int weight_mode, int use_pupil, const double* min_intensity) {
  SETTLE_SCALE(c);
  if (c) (void)hipSetDevice(c->device);
  if (!c || !table || !params || !poly) return fail(c, PAOS_EINVAL, "paos_wavefront_fit: null argument");
  if (nmax < 0 || kdim < nmax / 2 + 1 || param_stride < ZP_HEAD)
    return fail(c, PAOS_EINVAL, "paos_wavefront_fit: inconsistent Zernike table dimensions");
  if (K < 1 || K > kWfMaxK) return fail(c, PAOS_EUNSUPPORTED, "paos_wavefront_fit: 1 <= K <= 63 polynomials");
  if (weight_mode != 0 && weight_mode != kWfIntensity) return fail(c, PAOS_EINVAL, "paos_wavefront_fit: unknown weight mode");
  if (use_pupil && !c->mask) return fail(c, PAOS_EINVAL, "paos_wavefront_fit: no pupil defined (paos_pupil_aperture / paos_pupil_upload)");
  const size_t batch = c->batch;
  std::vector<double> floors(batch, 0.0), rows(2 * batch, 0.0), cols(2 * batch, 0.0);
  for (size_t i = 0; i < batch; ++i) {
    const double* q = params + i * param_stride;
    if (min_intensity) {
      if (!std::isfinite(min_intensity[i]) || min_intensity[i] < 0.0)
        return fail(c, PAOS_EINVAL, "paos_wavefront_fit: min_intensity must be finite and >= 0");
      floors[i] = min_intensity[i];
    }
    if (q[ZP_ENABLE] == 0.0) continue;  // (an empty box)
    if (!(q[ZP_RADIUS] > 0.0)) return fail(c, PAOS_EINVAL, "paos_wavefront_fit: the radius must be > 0");
    for (int k = ZP_DX; k < ZP_HEAD; ++k)
      if (!std::isfinite(q[k])) return fail(c, PAOS_EINVAL, "paos_wavefront_fit: non-finite header value");
    // rho <= 1 needs |j - n/2| |dx| <= radius and |k - n/2| |dy| <= radius; a zero or tiny pitch reaches the whole grid
    const double hx = q[ZP_RADIUS] / std::fabs(q[ZP_DX]), hy = q[ZP_RADIUS] / std::fabs(q[ZP_DY]);
    reach(c->n, hx < (double)c->n ? hx : (double)c->n, &cols[2 * i]);
    reach(c->n, hy < (double)c->n ? hy : (double)c->n, &rows[2 * i]);
  }
  // poly[j] = {|m|, k, is_sin, factor}  ->  slot table + factors (paos_zernike_gram) ...
  const size_t ncoef = (size_t)(nmax + 1) * kdim;
  std::vector<double> slots(2 * ncoef, -1.0), fac(K);
  for (int j = 0; j < K; ++j) {
    const int am = (int)poly[4 * j], k = (int)poly[4 * j + 1], is_sin = poly[4 * j + 2] != 0.0;
    if (am < 0 || am > nmax || k < 0 || k >= kdim || am + 2 * k > nmax)
      return fail(c, PAOS_EINVAL, "paos_wavefront_fit: polynomial outside the recurrence table");
    double& slot = slots[2 * ((size_t)am * kdim + k) + (is_sin ? 1 : 0)];
    if (slot >= 0.0) return fail(c, PAOS_EINVAL, "paos_wavefront_fit: polynomial listed twice");
    slot = (double)j;
    fac[j] = poly[4 * j + 3];
  }
  // ... -> one record per step (am, k) of the recurrences, in the order the kernel walks them (wavefront_pass.h: steps)
  std::vector<double> steps;
  for (int am = 0; am <= nmax; ++am)
    for (int k = 0; k <= (nmax - am) / 2; ++k) {
      const size_t ci = (size_t)am * kdim + k;
      const int jc = (int)slots[2 * ci], js = (int)slots[2 * ci + 1];
      const double rec[kWfStep] = {table[3 * ci], table[3 * ci + 1], table[3 * ci + 2], (double)jc, (double)js,
                                   jc >= 0 ? fac[jc] : 0.0, js >= 0 ? fac[js] : 0.0, 0.0};
      steps.insert(steps.end(), rec, rec + kWfStep);
    }
  // summary | sums | r | the partials of launch 1 | the partials of launch 2
  const int nmb = moment_blocks(c), ngb = gram_blocks(c);
  const size_t npairs = (size_t)(K + 1) * (K + 2) / 2, nvals = npairs + kWfExtra;
  const size_t sums_off = batch * kWfSummary, r_off = sums_off + batch * npairs, mom_off = r_off + 2 * batch;
  const size_t gram_off = mom_off + kWfMoments * batch * nmb, total = gram_off + batch * ngb * nvals;
  if (total * sizeof(double) > c->wf_bytes) {
    c->wf_fitted = false;  // (what the old buffer held goes with it)
    if (c->wf_buf) {
      HIPCHK(c, hipStreamSynchronize(c->stream));
      (void)hipFree(c->wf_buf);
      c->wf_buf = nullptr;
      c->wf_bytes = 0;
    }
    HIPCHK(c, hipMalloc(&c->wf_buf, total * sizeof(double)));
    c->wf_bytes = total * sizeof(double);
  }
  const double *dp = nullptr, *dsteps = nullptr, *dfloor = nullptr, *drows = nullptr, *dcols = nullptr;
  int rc;
  ArenaBatch ab(c);
  if ((rc = ab.begin(arena_rounded(batch * param_stride) + arena_rounded(steps.size()) + arena_rounded(batch) + 2 * arena_rounded(2 * batch))))
    return rc;
  if ((rc = ab.add(params, batch * param_stride, &dp)) || (rc = ab.add(steps.data(), steps.size(), &dsteps)) ||
      (rc = ab.add(floors.data(), batch, &dfloor)) || (rc = ab.add(rows.data(), 2 * batch, &drows)) ||
      (rc = ab.add(cols.data(), 2 * batch, &dcols)) || (rc = ab.commit()))
    return arena_settled(c, rc);
  c->wf_fitted = false;
  double* summary = c->wf_buf;
  double* sums = c->wf_buf + sums_off;
  double* r_used = c->wf_buf + r_off;
  double* mom = c->wf_buf + mom_off;
  double* gram = c->wf_buf + gram_off;
  const double* pupil = use_pupil ? c->mask : nullptr;
  const int n = c->n;
  c->prof_next_lines = 0.0;
  c->prof_next_bytes = (double)batch * c->item_stride * elem_bytes(c);  // (at most: the box of every item)
  rc = dispatch_layout(c, [&](auto t, auto br) {
    using T = decltype(t);
    return TIMED_LAUNCH(c, (wf_moments_kernel<T, decltype(br)::value, Lay<T>::BC>), dim3(nmb, c->batch), dim3(kPwThreads), 0, 0,
                        PAOS_KERNEL_PASS_ANY, 0, (const cx<T>*)c->field, dp, param_stride, dfloor, pupil, drows, dcols, n, c->pitch,
                        c->item_stride, mom);
  });
  if (rc) return rc;
  c->prof_next_bytes = (double)batch * nmb * kWfMoments * sizeof(double);
  rc = TIMED_LAUNCH(c, wf_moments_final_kernel, dim3(c->batch), dim3(kPwThreads), 0, 0, PAOS_KERNEL_PASS_ANY, 0, (const double*)mom, nmb,
                    dp, param_stride, summary, r_used);
  if (rc) return rc;
  // K polynomial rows, phi and (intensity weights) w; the closing reduction of the pixel slots needs four rows of 128
  const bool weighted = weight_mode == kWfIntensity;
  const size_t lds = std::max<size_t>((size_t)(K + 1 + (weighted ? 1 : 0)) * kGramRow, (size_t)kWfExtra * kGramPix) * sizeof(double);
  c->prof_next_bytes = (double)batch * c->item_stride * elem_bytes(c);
  rc = dispatch_layout(c, [&](auto t, auto br) {
    using T = decltype(t);
    return dispatch_either<1, 0>(weighted, [&](auto wm) {
      return TIMED_LAUNCH(c, (wf_gram_kernel<T, decltype(br)::value, Lay<T>::BC, decltype(wm)::value != 0>), dim3(ngb, c->batch),
                          dim3(kGramThreads), lds, generic_lds_opt_in(lds), PAOS_KERNEL_PASS_ANY, 0, (const cx<T>*)c->field, dp,
                          param_stride, dfloor, pupil, drows, dcols, (const double*)r_used, n, c->pitch, c->item_stride, nmax, K,
                          dsteps, gram);
    });
  });
  if (rc) return rc;
  c->prof_next_bytes = (double)batch * (ngb + 1) * nvals * sizeof(double);
  rc = TIMED_LAUNCH(c, wf_final_kernel, dim3((unsigned)((nvals + 255) / 256), c->batch), dim3(256), 0, 0, PAOS_KERNEL_PASS_ANY, 0,
                    (const double*)gram, ngb, (int)npairs, sums, summary);
  if (rc) return rc;
  c->wf_pairs = (int)npairs;
  c->wf_fitted = true;
  return PAOS_OK;
}

int paos_wavefront_fetch(paos_ctx* c, double* summary, double* sums) {
  if (c) (void)hipSetDevice(c->device);
  if (!c || (!summary && !sums)) return fail(c, PAOS_EINVAL, "paos_wavefront_fetch: null context, or neither output asked for");
  if (!c->wf_buf || !c->wf_fitted) return fail(c, PAOS_EINVAL, "paos_wavefront_fetch: no wavefront fit computed (paos_wavefront_fit)");
  const size_t batch = c->batch;
  int rc = PAOS_OK;
  if (summary && (rc = copy_to_host(c, summary, c->wf_buf, batch * kWfSummary * sizeof(double)))) return rc;
  if (sums) rc = copy_to_host(c, sums, c->wf_buf + batch * kWfSummary, batch * c->wf_pairs * sizeof(double));
  return rc;
}

}  // extern "C"
