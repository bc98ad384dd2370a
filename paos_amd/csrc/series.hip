// series.hip -- pointing series: detector frames and box flux of the kept PSFs (paos_series_*; kernels: series_pass.h), and
// the broadband sum of such frames over the items of a sweep, kept on the device (paos_series_sum_*; series_sum_plan.h).
#include "host.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "series_pass.h"
#include "series_plan.h"
#include "series_sum_plan.h"

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

// a pinned staging buffer of parameters (the per-item series and the broadband sum have one each): free to write once
// the copy of the last call that used it has run
int series_stage(paos_ctx* c, double** host, size_t* have, hipEvent_t* ev, size_t bytes) {
  if (!*ev) HIPCHK(c, hipEventCreateWithFlags(ev, hipEventDisableTiming));
  else HIPCHK(c, hipEventSynchronize(*ev));
  if (bytes <= *have) return PAOS_OK;
  if (*host) {
    (void)hipHostFree(*host);
    *host = nullptr;
    *have = 0;
  }
  HIPCHK(c, hipHostMalloc(host, bytes));
  *have = bytes;
  return PAOS_OK;
}

// what paos_detector_begin asks of a geometry; `who`: the calling entry point, for the message
int series_check_geom(paos_ctx* c, const std::string& who, const double* geom) {
  const double fnx = geom[0], fny = geom[1];
  if (!(fnx >= 1 && fnx <= 4096 && fnx == std::floor(fnx)) || !(fny >= 1 && fny <= 4096 && fny == std::floor(fny)))
    return fail(c, PAOS_EINVAL, who + "detector nx and ny must be integers in 1..4096");
  if (!finite_positive(geom[2]) || !finite_positive(geom[3])) return fail(c, PAOS_EINVAL, who + "detector pitch must be finite and positive");
  if (!std::isfinite(geom[4]) || !std::isfinite(geom[5])) return fail(c, PAOS_EINVAL, who + "detector centre must be finite");
  return PAOS_OK;
}

// per-item records dx, dy, x0, y0 and offsets against a detector centre: everything a frame's edges are formed from is finite
int series_check_items(paos_ctx* c, const std::string& entry, const double* per_item, const double* offsets, size_t offsets_stride,
                       int batch, int frames, double gxc, double gyc) {
  for (int i = 0; i < batch; ++i) {
    const double* q = per_item + (size_t)i * kSeriesItem;
    const std::string who = entry + "item " + std::to_string(i) + ": ";
    if (!finite_positive(q[0]) || !finite_positive(q[1])) return fail(c, PAOS_EINVAL, who + "dx and dy must be finite and positive");
    if (!std::isfinite(q[2]) || !std::isfinite(q[3])) return fail(c, PAOS_EINVAL, who + "the origin x0, y0 must be finite");
    const double* o = offsets + (size_t)i * offsets_stride;
    for (int t = 0; t < frames; ++t) {
      const double ox = o[2 * t], oy = o[2 * t + 1];
      if (!std::isfinite(ox) || !std::isfinite(oy)) return fail(c, PAOS_EINVAL, who + "offset " + std::to_string(t) + " is not finite");
      const double gx = q[2] + ox, gy = q[3] + oy;
      const double xc = gxc - gx, yc = gyc - gy;
      if (!std::isfinite(gx) || !std::isfinite(gy) || !std::isfinite(xc) || !std::isfinite(yc))
        return fail(c, PAOS_EINVAL, who + "origin plus offset " + std::to_string(t) + ", or the detector centre minus it, overflows");
    }
  }
  return PAOS_OK;
}

int series_check_boxes(paos_ctx* c, const std::string& entry, const int* boxes, int nboxes, int nx, int ny) {
  for (int a = 0; a < nboxes; ++a) {
    const int* b = boxes + 4 * a;
    if (!(0 <= b[0] && b[0] < b[1] && b[1] <= nx && 0 <= b[2] && b[2] < b[3] && b[3] <= ny))
      return fail(c, PAOS_EINVAL, entry + "box " + std::to_string(a) + " is empty or not inside the detector");
  }
  return PAOS_OK;
}

int series_check_response(paos_ctx* c, const std::string& entry, const double* response, size_t npix) {
  if (response)
    for (size_t q = 0; q < npix; ++q)
      if (!std::isfinite(response[q])) return fail(c, PAOS_EINVAL, entry + "the response must be finite");
  return PAOS_OK;
}

}  // namespace

extern "C" {

int paos_series_compute(paos_ctx* c, const double* geom, const double* per_item, const double* offsets, int frames,
                        int per_item_offsets, const int* boxes, int nboxes, const double* response, double* host_frames) {
  if (c) (void)hipSetDevice(c->device);
  if (!c || !geom || !per_item || !offsets) return fail(c, PAOS_EINVAL, "paos_series_compute: null argument");
  if (!c->psf) return fail(c, PAOS_EINVAL, "paos_series_compute: no PSF kept (paos_psf_keep)");
  const std::string entry = "paos_series_compute: ";
  int rc = series_check_geom(c, entry, geom);
  if (rc) return rc;
  if (frames < 1 || frames > PAOS_SERIES_MAX_FRAMES) return fail(c, PAOS_EINVAL, "paos_series_compute: frames must be in 1..65536");
  if (nboxes < 0 || nboxes > PAOS_SERIES_MAX_BOXES) return fail(c, PAOS_EINVAL, "paos_series_compute: nboxes must be in 0..16");
  if (nboxes == 0 && !host_frames) return fail(c, PAOS_EINVAL, "paos_series_compute: neither boxes nor frames asked for: nothing to compute");
  if (nboxes > 0 && !boxes) return fail(c, PAOS_EINVAL, "paos_series_compute: null boxes");
  const int n = c->n, nx = (int)geom[0], ny = (int)geom[1], batch = c->batch;
  const DetGeom g{nx, ny, geom[2], geom[3], geom[4], geom[5]};
  const size_t npix = (size_t)nx * ny;
  if ((rc = series_check_boxes(c, entry, boxes, nboxes, nx, ny))) return rc;
  const size_t offsets_stride = per_item_offsets ? (size_t)frames * 2 : 0;
  if ((rc = series_check_items(c, entry, per_item, offsets, offsets_stride, batch, frames, g.xc, g.yc))) return rc;
  if ((rc = series_check_response(c, entry, response, npix))) return rc;

  // parameters: per-item records | offsets | boxes (as doubles) | response
  const size_t noff = (per_item_offsets ? (size_t)batch : 1) * (size_t)frames * 2;
  const size_t items_at = 0, offsets_at = items_at + (size_t)batch * kSeriesItem, boxes_at = offsets_at + noff;
  const size_t response_at = boxes_at + (size_t)nboxes * 4, npar = response_at + (response ? npix : 0);
  const size_t cap = series_cap_bytes(getenv("PAOS_SERIES_SCRATCH_BYTES"), size_t(PAOS_DETECTOR_SCRATCH_MIB) << 20);
  const SeriesPlan plan = series_plan(batch, frames, npix, cap);
  c->series_done = false;
  if ((rc = series_stage(c, &c->series_host, &c->series_host_bytes, &c->series_ev, npar * sizeof(double)))) return rc;
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
                         par + boxes_at, nboxes, nx, ny, ch.i0, ch.t0, frames, c->series_flux, (const double*)nullptr);
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

// ---- broadband series sum (README.md, "Broadband series") ------------------------------------------------------------
int paos_series_sum_begin(paos_ctx* c, const double* geom, int frames) {
  if (c) (void)hipSetDevice(c->device);
  if (!c || !geom) return fail(c, PAOS_EINVAL, "paos_series_sum_begin: null context or geometry");
  const std::string entry = "paos_series_sum_begin: ";
  int rc = series_check_geom(c, entry, geom);
  if (rc) return rc;
  if (frames < 1 || frames > PAOS_SERIES_MAX_FRAMES) return fail(c, PAOS_EINVAL, entry + "frames must be in 1..65536");
  size_t count = 0;
  if (!series_sum_size(frames, (int)geom[0], (int)geom[1], &count))
    return fail(c, PAOS_EINVAL, entry + "frames x ny x nx must not exceed 2^27 doubles (PAOS_SERIES_SUM_MAX_DOUBLES)");
  c->sum_open = false;
  if ((rc = series_reserve(c, &c->sum_acc, &c->sum_acc_bytes, count * sizeof(double)))) return rc;
  HIPCHK(c, hipMemsetAsync(c->sum_acc, 0, count * sizeof(double), c->stream));
  c->sum_nx = (int)geom[0];
  c->sum_ny = (int)geom[1];
  c->sum_frames = frames;
  for (int k = 0; k < 4; ++k) c->sum_geom[k] = geom[2 + k];
  c->sum_open = true;
  return PAOS_OK;
}

int paos_series_sum_add(paos_ctx* c, const double* per_item, const double* offsets, int per_item_offsets, const double* weights,
                        int per_frame_weights) {
  if (c) (void)hipSetDevice(c->device);
  if (!c || !per_item || !offsets || !weights) return fail(c, PAOS_EINVAL, "paos_series_sum_add: null argument");
  const std::string entry = "paos_series_sum_add: ";
  if (!c->sum_open) return fail(c, PAOS_EINVAL, entry + "no sum open (paos_series_sum_begin)");
  if (!c->psf) return fail(c, PAOS_EINVAL, entry + "no PSF kept (paos_psf_keep)");
  const int n = c->n, batch = c->batch, frames = c->sum_frames;
  const DetGeom g{c->sum_nx, c->sum_ny, c->sum_geom[0], c->sum_geom[1], c->sum_geom[2], c->sum_geom[3]};
  const size_t npix = (size_t)g.nx * g.ny;
  const size_t offsets_stride = per_item_offsets ? (size_t)frames * 2 : 0;
  int rc = series_check_items(c, entry, per_item, offsets, offsets_stride, batch, frames, g.xc, g.yc);
  if (rc) return rc;
  const size_t nweights = (size_t)batch * (per_frame_weights ? (size_t)frames : 1);
  for (size_t k = 0; k < nweights; ++k)
    if (!std::isfinite(weights[k])) return fail(c, PAOS_EINVAL, entry + "weight " + std::to_string(k) + " is not finite");

  // parameters: per-item records | offsets | weights
  const size_t noff = (per_item_offsets ? (size_t)batch : 1) * (size_t)frames * 2;
  const size_t items_at = 0, offsets_at = items_at + (size_t)batch * kSeriesItem, weights_at = offsets_at + noff;
  const size_t npar = weights_at + nweights;
  if ((rc = series_stage(c, &c->sum_host, &c->sum_host_bytes, &c->sum_ev, npar * sizeof(double)))) return rc;
  if ((rc = series_reserve(c, &c->sum_par, &c->sum_par_bytes, npar * sizeof(double)))) return rc;
  double* h = c->sum_host;
  std::memcpy(h + items_at, per_item, (size_t)batch * kSeriesItem * sizeof(double));
  std::memcpy(h + offsets_at, offsets, noff * sizeof(double));
  std::memcpy(h + weights_at, weights, nweights * sizeof(double));
  HIPCHK(c, hipMemcpyAsync(c->sum_par, h, npar * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipEventRecord(c->sum_ev, c->stream));

  const double* par = c->sum_par;
  const size_t w_item = per_frame_weights ? (size_t)frames : 1, w_frame = per_frame_weights ? 1 : 0;
  const unsigned tiles = series_sum_tiles(npix, kSeriesThreads);
  SeriesSumRange r{0, 0};
  while (series_sum_next_range(frames, &r)) {
    const dim3 grid(tiles, r.nt, 1);
    dispatch_layout(c, [&](auto t, auto br) {
      hipLaunchKernelGGL((series_sum_kernel<decltype(br)::value, Lay<decltype(t)>::BC>), grid, dim3(kSeriesThreads), 0, c->stream,
                         (const double*)c->psf, c->item_stride, c->pitch, n, batch, par + items_at, par + offsets_at, offsets_stride,
                         par + weights_at, w_item, w_frame, g, r.t0, c->sum_acc);
    });
    HIPCHK(c, hipGetLastError());
  }
  return PAOS_OK;
}

int paos_series_sum_flux(paos_ctx* c, const int* boxes, int nboxes, const double* response, double* host_flux) {
  if (c) (void)hipSetDevice(c->device);
  if (!c || !boxes || !host_flux) return fail(c, PAOS_EINVAL, "paos_series_sum_flux: null argument");
  const std::string entry = "paos_series_sum_flux: ";
  if (!c->sum_open) return fail(c, PAOS_EINVAL, entry + "no sum open (paos_series_sum_begin)");
  if (nboxes < 1 || nboxes > PAOS_SERIES_MAX_BOXES) return fail(c, PAOS_EINVAL, entry + "nboxes must be in 1..16");
  const int nx = c->sum_nx, ny = c->sum_ny, frames = c->sum_frames;
  const size_t npix = (size_t)nx * ny;
  int rc = series_check_boxes(c, entry, boxes, nboxes, nx, ny);
  if (rc) return rc;
  if ((rc = series_check_response(c, entry, response, npix))) return rc;

  // parameters: boxes (as doubles) | response
  const size_t boxes_at = 0, response_at = boxes_at + (size_t)nboxes * 4, npar = response_at + (response ? npix : 0);
  if ((rc = series_stage(c, &c->sum_host, &c->sum_host_bytes, &c->sum_ev, npar * sizeof(double)))) return rc;
  if ((rc = series_reserve(c, &c->sum_par, &c->sum_par_bytes, npar * sizeof(double)))) return rc;
  if ((rc = series_reserve(c, &c->sum_flux, &c->sum_flux_bytes, (size_t)frames * nboxes * sizeof(double)))) return rc;
  double* h = c->sum_host;
  for (int k = 0; k < nboxes * 4; ++k) h[boxes_at + k] = (double)boxes[k];
  if (response) std::memcpy(h + response_at, response, npix * sizeof(double));
  HIPCHK(c, hipMemcpyAsync(c->sum_par, h, npar * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipEventRecord(c->sum_ev, c->stream));
  const double* par = c->sum_par;
  const double* dresponse = response ? par + response_at : nullptr;
  SeriesSumRange r{0, 0};
  while (series_sum_next_range(frames, &r)) {
    // (the flux kernel counts frames from its pointer: one "item" that holds the frames of this range)
    hipLaunchKernelGGL(series_flux_kernel, dim3(nboxes, r.nt, 1), dim3(kSeriesWave), 0, c->stream,
                       (const double*)c->sum_acc + (size_t)r.t0 * npix, par + boxes_at, nboxes, nx, ny, 0, r.t0, frames, c->sum_flux,
                       dresponse);
    HIPCHK(c, hipGetLastError());
  }
  return copy_to_host(c, host_flux, c->sum_flux, (size_t)frames * nboxes * sizeof(double));
}

int paos_series_sum_fetch(paos_ctx* c, double* host_frames) {
  if (c) (void)hipSetDevice(c->device);
  if (!c || !host_frames) return fail(c, PAOS_EINVAL, "paos_series_sum_fetch: null context or output buffer");
  if (!c->sum_open) return fail(c, PAOS_EINVAL, "paos_series_sum_fetch: no sum open (paos_series_sum_begin)");
  return copy_to_host(c, host_frames, c->sum_acc, (size_t)c->sum_frames * c->sum_nx * c->sum_ny * sizeof(double));
}

}  // extern "C"
