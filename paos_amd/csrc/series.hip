// series.hip -- pointing series: detector frames and box flux of the kept PSFs (paos_series_*; kernels: series_pass.h).
#include "host.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "series_pass.h"
#include "series_plan.h"

namespace {

bool finite_positive(double v) { return std::isfinite(v) && v > 0.0; }

// (re)allocate a device buffer that work already on the stream may still read
int series_reserve(paos_ctx* c, double** buf, size_t* have, size_t bytes) {
  if (bytes <= *have) return PAOS_OK;
  if (*buf) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    (void)hipFree(*buf);
    *buf = nullptr;
    *have = 0;
  }
  HIPCHK(c, hipMalloc(buf, bytes));
  *have = bytes;
  return PAOS_OK;
}

// the pinned staging buffer of the parameters: free to write once the copy of the last call has run
int series_stage(paos_ctx* c, size_t bytes) {
  if (!c->series_ev) HIPCHK(c, hipEventCreateWithFlags(&c->series_ev, hipEventDisableTiming));
  else HIPCHK(c, hipEventSynchronize(c->series_ev));
  if (bytes <= c->series_host_bytes) return PAOS_OK;
  if (c->series_host) {
    (void)hipHostFree(c->series_host);
    c->series_host = nullptr;
    c->series_host_bytes = 0;
  }
  HIPCHK(c, hipHostMalloc(&c->series_host, bytes));
  c->series_host_bytes = bytes;
  return PAOS_OK;
}

}  // namespace

extern "C" {

int paos_series_compute(paos_ctx* c, const double* geom, const double* per_item, const double* offsets, int frames,
                        int per_item_offsets, const int* boxes, int nboxes, const double* response, double* host_frames) {
  if (c) (void)hipSetDevice(c->device);
  if (!c || !geom || !per_item || !offsets) return fail(c, PAOS_EINVAL, "paos_series_compute: null argument");
  if (!c->psf) return fail(c, PAOS_EINVAL, "paos_series_compute: no PSF kept (paos_psf_keep)");
  const double fnx = geom[0], fny = geom[1];
  if (!(fnx >= 1 && fnx <= 4096 && fnx == std::floor(fnx)) || !(fny >= 1 && fny <= 4096 && fny == std::floor(fny)))
    return fail(c, PAOS_EINVAL, "paos_series_compute: detector nx and ny must be integers in 1..4096");
  if (!finite_positive(geom[2]) || !finite_positive(geom[3])) return fail(c, PAOS_EINVAL, "paos_series_compute: detector pitch must be finite and positive");
  if (!std::isfinite(geom[4]) || !std::isfinite(geom[5])) return fail(c, PAOS_EINVAL, "paos_series_compute: detector centre must be finite");
  if (frames < 1 || frames > PAOS_SERIES_MAX_FRAMES) return fail(c, PAOS_EINVAL, "paos_series_compute: frames must be in 1..65536");
  if (nboxes < 0 || nboxes > PAOS_SERIES_MAX_BOXES) return fail(c, PAOS_EINVAL, "paos_series_compute: nboxes must be in 0..16");
  if (nboxes == 0 && !host_frames) return fail(c, PAOS_EINVAL, "paos_series_compute: neither boxes nor frames asked for: nothing to compute");
  if (nboxes > 0 && !boxes) return fail(c, PAOS_EINVAL, "paos_series_compute: null boxes");
  const int n = c->n, nx = (int)fnx, ny = (int)fny, batch = c->batch;
  const DetGeom g{nx, ny, geom[2], geom[3], geom[4], geom[5]};
  const size_t npix = (size_t)nx * ny;
  for (int a = 0; a < nboxes; ++a) {
    const int* b = boxes + 4 * a;
    if (!(0 <= b[0] && b[0] < b[1] && b[1] <= nx && 0 <= b[2] && b[2] < b[3] && b[3] <= ny))
      return fail(c, PAOS_EINVAL, "paos_series_compute: box " + std::to_string(a) + " is empty or not inside the detector");
  }
  const size_t offsets_stride = per_item_offsets ? (size_t)frames * 2 : 0;
  for (int i = 0; i < batch; ++i) {
    const double* q = per_item + (size_t)i * kSeriesItem;
    const std::string who = "paos_series_compute: item " + std::to_string(i) + ": ";
    if (!finite_positive(q[0]) || !finite_positive(q[1])) return fail(c, PAOS_EINVAL, who + "dx and dy must be finite and positive");
    if (!std::isfinite(q[2]) || !std::isfinite(q[3])) return fail(c, PAOS_EINVAL, who + "the origin x0, y0 must be finite");
    const double* o = offsets + (size_t)i * offsets_stride;
    for (int t = 0; t < frames; ++t) {
      const double ox = o[2 * t], oy = o[2 * t + 1];
      if (!std::isfinite(ox) || !std::isfinite(oy)) return fail(c, PAOS_EINVAL, who + "offset " + std::to_string(t) + " is not finite");
      const double gx = q[2] + ox, gy = q[3] + oy;
      const double xc = g.xc - gx, yc = g.yc - gy;
      if (!std::isfinite(gx) || !std::isfinite(gy) || !std::isfinite(xc) || !std::isfinite(yc))
        return fail(c, PAOS_EINVAL, who + "origin plus offset " + std::to_string(t) + ", or the detector centre minus it, overflows");
    }
  }
  if (response)
    for (size_t q = 0; q < npix; ++q)
      if (!std::isfinite(response[q])) return fail(c, PAOS_EINVAL, "paos_series_compute: the response must be finite");

  // parameters: per-item records | offsets | boxes (as doubles) | response
  const size_t noff = (per_item_offsets ? (size_t)batch : 1) * (size_t)frames * 2;
  const size_t items_at = 0, offsets_at = items_at + (size_t)batch * kSeriesItem, boxes_at = offsets_at + noff;
  const size_t response_at = boxes_at + (size_t)nboxes * 4, npar = response_at + (response ? npix : 0);
  const size_t cap = series_cap_bytes(getenv("PAOS_SERIES_SCRATCH_BYTES"), size_t(PAOS_DETECTOR_SCRATCH_MIB) << 20);
  const SeriesPlan plan = series_plan(batch, frames, npix, cap);
  c->series_done = false;
  int rc = series_stage(c, npar * sizeof(double));
  if (rc) return rc;
  if ((rc = series_reserve(c, &c->series_par, &c->series_par_bytes, npar * sizeof(double)))) return rc;
  if ((rc = series_reserve(c, &c->series_frames, &c->series_frames_bytes, series_plan_bytes(plan, npix)))) return rc;
  if (nboxes > 0 && (rc = series_reserve(c, &c->series_flux, &c->series_flux_bytes, (size_t)batch * frames * nboxes * sizeof(double))))
    return rc;
  double* h = c->series_host;
  std::memcpy(h + items_at, per_item, (size_t)batch * kSeriesItem * sizeof(double));
  std::memcpy(h + offsets_at, offsets, noff * sizeof(double));
  for (int k = 0; k < nboxes * 4; ++k) h[boxes_at + k] = (double)boxes[k];
  if (response) std::memcpy(h + response_at, response, npix * sizeof(double));
  HIPCHK(c, hipMemcpyAsync(c->series_par, h, npar * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipEventRecord(c->series_ev, c->stream));

  const double* par = c->series_par;
  const double* dresponse = response ? par + response_at : nullptr;
  const unsigned tiles = (unsigned)((npix + kSeriesThreads - 1) / kSeriesThreads);
  SeriesChunk ch{0, 0, 0, 0};
  while (series_next_chunk(plan, batch, frames, &ch)) {
    const dim3 grid(tiles, ch.nt, ch.ni);
    dispatch_layout(c, [&](auto t, auto br) {
      hipLaunchKernelGGL((series_frames_kernel<decltype(br)::value, Lay<decltype(t)>::BC>), grid, dim3(kSeriesThreads), 0, c->stream,
                         (const double*)c->psf, c->item_stride, c->pitch, n, par + items_at, par + offsets_at, offsets_stride, dresponse, g,
                         ch.i0, ch.t0, c->series_frames);
    });
    HIPCHK(c, hipGetLastError());
    if (nboxes > 0) {
      hipLaunchKernelGGL(series_flux_kernel, dim3(nboxes, ch.nt, ch.ni), dim3(kSeriesWave), 0, c->stream, (const double*)c->series_frames,
                         par + boxes_at, nboxes, nx, ny, ch.i0, ch.t0, frames, c->series_flux);
      HIPCHK(c, hipGetLastError());
    }
    if (host_frames)
      for (int li = 0; li < ch.ni; ++li) {
        double* dst = host_frames + ((size_t)(ch.i0 + li) * frames + ch.t0) * npix;
        if ((rc = copy_to_host(c, dst, c->series_frames + (size_t)li * ch.nt * npix, (size_t)ch.nt * npix * sizeof(double)))) return rc;
      }
  }
  c->series_nframes = frames;
  c->series_nboxes = nboxes;
  c->series_done = true;
  return PAOS_OK;
}

int paos_series_fetch(paos_ctx* c, double* flux) {
  if (c) (void)hipSetDevice(c->device);
  if (!c || !flux) return fail(c, PAOS_EINVAL, "paos_series_fetch: null context or output buffer");
  if (!c->series_done) return fail(c, PAOS_EINVAL, "paos_series_fetch: no series computed (paos_series_compute)");
  if (c->series_nboxes == 0) return fail(c, PAOS_EINVAL, "paos_series_fetch: the last paos_series_compute had no boxes");
  return copy_to_host(c, flux, c->series_flux, (size_t)c->batch * c->series_nframes * c->series_nboxes * sizeof(double));
}

}  // extern "C"
