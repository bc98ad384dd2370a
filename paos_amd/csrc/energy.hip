// energy.hip -- encircled / ensquared energy of the kept PSFs about their own centres (paos_ee_*; kernels: energy_pass.h).
#include "host.h"

#include <algorithm>
#include <cmath>

#include "energy_pass.h"

namespace {

bool finite_positive(double v) { return std::isfinite(v) && v > 0.0; }

// workgroups of the sweep of launch 1: every thread gets at least eight pairs of pixels (a function of the grid alone)
int sum_blocks(const paos_ctx* c) {
  const size_t pairs = c->item_stride / 2;
  return (int)std::min<size_t>(std::max<size_t>(pairs / (kEeSumThreads * 8), 1), kEeMaxSumBlocks);
}

// bands of launch 2 for an item whose largest circle reaches `reach_y` rows either side of a centre the host does not
// know: the kernel starts at floor(cy - reach_y) - 1 rounded down to a whole band, so the rows up to cy + reach_y + 1 lie
// within 2 reach_y + 3 + kEeBandRows rows of it -- and never more bands than the grid has
int bands_for(int n, double reach_y) {
  const double rows = 2.0 * reach_y + 3.0 + (double)kEeBandRows;
  return (int)std::min(std::ceil(rows / kEeBandRows) + 1.0, (double)(n / kEeBandRows));
}

}  // namespace

extern "C" {

int paos_ee_compute(paos_ctx* c, int bins, int square, int centre_mode, const double* per_item) {
  if (c) (void)hipSetDevice(c->device);
  if (!c || !per_item) return fail(c, PAOS_EINVAL, "paos_ee_compute: null argument");
  if (!c->psf) return fail(c, PAOS_EINVAL, "paos_ee_compute: no PSF kept (paos_psf_keep)");
  if (bins < 1 || bins > kEeMaxBins) return fail(c, PAOS_EINVAL, "paos_ee_compute: bins must be in 1..1024");
  if (centre_mode != PAOS_EE_GIVEN && centre_mode != PAOS_EE_CENTROID && centre_mode != PAOS_EE_PEAK)
    return fail(c, PAOS_EINVAL, "paos_ee_compute: unknown centre mode");
  const int n = c->n, ncurves = square ? 2 : 1;
  const double half = 0.5 * (double)n;
  int nbands = 1;
  for (int i = 0; i < c->batch; ++i) {
    const double* q = per_item + (size_t)i * kEeItem;
    const std::string who = "paos_ee_compute: item " + std::to_string(i) + ": ";
    if (!finite_positive(q[0]) || !finite_positive(q[1])) return fail(c, PAOS_EINVAL, who + "the ring width and the aspect must be finite and positive");
    const double reach = (double)bins * q[0];
    if (reach > half || reach / q[1] > half) return fail(c, PAOS_EINVAL, who + "the largest circle is wider or taller than the grid");
    if (centre_mode == PAOS_EE_GIVEN && !(std::isfinite(q[2]) && std::isfinite(q[3]) && q[2] >= 0.0 && q[2] < n && q[3] >= 0.0 && q[3] < n))
      return fail(c, PAOS_EINVAL, who + "the centre must be finite and inside [0, n)");
    nbands = std::max(nbands, bands_for(n, reach / q[1]));
  }
  // summary | curves | the partials of launch 1 | the partials of launch 2: batch x bins x row bands, never n^2
  const int nsb = sum_blocks(c);
  const size_t batch = c->batch;
  const size_t curves_off = batch * kEeSummary, sums_off = curves_off + batch * ncurves * bins;
  const size_t rings_off = sums_off + batch * nsb * kEeSumVals, total = rings_off + batch * nbands * ncurves * bins;
  if (total * sizeof(double) > c->ee_bytes) {
    c->ee_computed = c->ee_valid = false;  // (what the old buffer held goes with it)
    if (c->ee_buf) {
      HIPCHK(c, hipStreamSynchronize(c->stream));
      (void)hipFree(c->ee_buf);
      c->ee_buf = nullptr;
      c->ee_bytes = 0;
    }
    HIPCHK(c, hipMalloc(&c->ee_buf, total * sizeof(double)));
    c->ee_bytes = total * sizeof(double);
  }
  const double* ditems = nullptr;
  int rc = arena_push(c, per_item, batch * kEeItem, &ditems);
  if (rc) return rc;
  c->ee_computed = c->ee_valid = false;
  double* summary = c->ee_buf;
  double* curves = c->ee_buf + curves_off;
  double* sums = c->ee_buf + sums_off;
  double* rings = c->ee_buf + rings_off;
  const double* psf = c->psf;
  c->prof_next_lines = 0.0;
  c->prof_next_bytes = (double)batch * c->item_stride * sizeof(double);
  rc = dispatch_layout(c, [&](auto t, auto br) {
    return TIMED_LAUNCH(c, (ee_sums_kernel<decltype(br)::value, Lay<decltype(t)>::BC>), dim3(nsb, c->batch), dim3(kEeSumThreads), 0, 0,
                        PAOS_KERNEL_PASS_ANY, 0, psf, c->item_stride, c->pitch, n, sums);
  });
  if (rc) return rc;
  c->prof_next_bytes = (double)batch * nsb * kEeSumVals * sizeof(double);
  rc = TIMED_LAUNCH(c, ee_centre_kernel, dim3(c->batch), dim3(kEeSumThreads), 0, 0, PAOS_KERNEL_PASS_ANY, 0, (const double*)sums, nsb, n,
                    centre_mode, ditems, summary);
  if (rc) return rc;
  const size_t lds = (size_t)ncurves * bins * sizeof(double);
  c->prof_next_bytes = (double)batch * nbands * kEeBandRows * (double)n * sizeof(double);  // (at most: the rows of the bands)
  rc = dispatch_layout(c, [&](auto t, auto br) {
    return TIMED_LAUNCH(c, (ee_rings_kernel<decltype(br)::value, Lay<decltype(t)>::BC>), dim3(nbands, c->batch), dim3(64), lds, 0,
                        PAOS_KERNEL_PASS_ANY, 0, psf, c->item_stride, c->pitch, n, ditems, (const double*)summary, bins, square ? 1 : 0, rings);
  });
  if (rc) return rc;
  c->prof_next_bytes = (double)batch * (nbands + 1) * ncurves * bins * sizeof(double);
  rc = TIMED_LAUNCH(c, ee_scan_kernel, dim3(ncurves, c->batch), dim3(kEeMaxBins), 0, 0, PAOS_KERNEL_PASS_ANY, 0, (const double*)rings, nbands,
                    bins, ncurves, curves);
  if (rc) return rc;
  c->ee_bins = bins;
  c->ee_curves = ncurves;
  c->ee_computed = c->ee_valid = true;
  return PAOS_OK;
}

int paos_ee_fetch(paos_ctx* c, double* summary, double* curves) {
  if (c) (void)hipSetDevice(c->device);
  if (!c || (!summary && !curves)) return fail(c, PAOS_EINVAL, "paos_ee_fetch: null context, or neither output asked for");
  if (!c->ee_buf || !c->ee_computed) return fail(c, PAOS_EINVAL, "paos_ee_fetch: no energy profiles computed (paos_ee_compute)");
  if (curves && !c->ee_valid)
    return fail(c, PAOS_EINVAL, "paos_ee_fetch: the PSFs were stored anew since paos_ee_compute: the curves are stale (compute again)");
  const size_t batch = c->batch;
  int rc = PAOS_OK;
  if (summary && (rc = copy_to_host(c, summary, c->ee_buf, batch * kEeSummary * sizeof(double)))) return rc;
  if (curves) rc = copy_to_host(c, curves, c->ee_buf + batch * kEeSummary, batch * c->ee_curves * c->ee_bins * sizeof(double));
  return rc;
}

}  // extern "C"
