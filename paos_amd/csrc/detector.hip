// detector.hip -- broadband PSFs on a detector pixel grid (paos_detector_*; kernels: detector_pass.h).
#include "host.h"

#include <algorithm>
#include <cmath>

#include "detector_pass.h"

namespace {

constexpr int kThreads = 256;  // per workgroup of both contractions (their launch bounds)

constexpr size_t kDetScratchBytes = size_t(PAOS_DETECTOR_SCRATCH_MIB) << 20;  // per-chunk cap of the scratch buffers

bool finite_positive(double v) { return std::isfinite(v) && v > 0.0; }

// (re)allocate a scratch buffer that work already on the stream may still read
int det_reserve(paos_ctx* c, double** buf, size_t* have, size_t bytes) {
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

// A_i of every batch item, chunk by chunk in item order: added as w_i A_i into the accumulator (host_out == NULL) or
// written to host_out[i][ny][nx] (synchronises).  per_item holds `stride` doubles per item: dx, dy, w and, when
// stride == PAOS_DETECTOR_PLACED_ITEM, the image-plane position (x0, y0) of the item's grid centre.  The detector centre
// seen from the item is then xc - x0 (rounded once; x0 = 0 gives xc itself, so zero offsets change no bit).
int detector_run(paos_ctx* c, const double* per_item, int stride, double* host_out) {
  if (!c->psf) return fail(c, PAOS_EINVAL, "no PSF kept (paos_psf_keep)");
  if (!c->det_set) return fail(c, PAOS_EINVAL, "no detector (paos_detector_begin)");
  if (!per_item) return fail(c, PAOS_EINVAL, "null per-item parameters");
  const bool accumulate = host_out == nullptr, placed = stride == PAOS_DETECTOR_PLACED_ITEM;
  const int n = c->n, nx = c->det_nx, ny = c->det_ny;
  const DetGeom g{nx, ny, c->det_geom[0], c->det_geom[1], c->det_geom[2], c->det_geom[3]};
  const size_t npix = (size_t)nx * ny;
  std::vector<int> k0(c->batch), k1(c->batch);
  std::vector<double> cx(c->batch), cy(c->batch);
  for (int i = 0; i < c->batch; ++i) {
    const double* q = per_item + (size_t)stride * i;
    const double dx = q[0], dy = q[1], w = q[2];
    if (!finite_positive(dx) || !finite_positive(dy)) return fail(c, PAOS_EINVAL, "dx and dy must be finite and positive");
    if (accumulate && !std::isfinite(w)) return fail(c, PAOS_EINVAL, "weights must be finite");
    cx[i] = g.xc;
    cy[i] = g.yc;
    if (placed) {
      if (!std::isfinite(q[3]) || !std::isfinite(q[4])) return fail(c, PAOS_EINVAL, "item origins x0 and y0 must be finite");
      cx[i] = g.xc - q[3];
      cy[i] = g.yc - q[4];
      if (!std::isfinite(cx[i]) || !std::isfinite(cy[i])) return fail(c, PAOS_EINVAL, "detector centre minus item origin overflows");
    }
    // the item's footprint: the grid rows under detector rows 0 .. ny-1 (det_edge is monotonic in its index)
    k0[i] = det_lo(det_edge(0, ny, g.py, cy[i], dy, n), n);
    k1[i] = std::max(k0[i], det_hi(det_edge(ny, ny, g.py, cy[i], dy, n), n));
  }
  const dim3 block(kThreads);
  for (int start = 0; start < c->batch;) {
    // the next items in order whose scratch fits the cap (at least one)
    size_t rows_bytes = 0;
    int end = start, max_block_rows = 0;
    while (end < c->batch) {
      const size_t b = (size_t)(k1[end] - k0[end]) * nx * sizeof(double);
      const bool fits = rows_bytes + b <= kDetScratchBytes && (accumulate || (size_t)(end - start + 1) * npix * sizeof(double) <= kDetScratchBytes);
      if (end > start && !fits) break;
      rows_bytes += b;
      ++end;
    }
    const int cnt = end - start;
    std::vector<double> rec((size_t)cnt * kDetItem, 0.0);
    size_t off = 0;
    for (int li = 0; li < cnt; ++li) {
      const int i = start + li;
      double* r = rec.data() + (size_t)li * kDetItem;
      r[0] = per_item[(size_t)stride * i];
      r[1] = per_item[(size_t)stride * i + 1];
      r[2] = accumulate ? per_item[(size_t)stride * i + 2] : 0.0;
      r[3] = k0[i]; r[4] = k1[i]; r[5] = (double)off; r[6] = i;
      r[8] = cx[i]; r[9] = cy[i];
      off += (size_t)(k1[i] - k0[i]) * nx;
      if (k1[i] > k0[i]) max_block_rows = std::max(max_block_rows, (k1[i] - 1) / c->br - k0[i] / c->br + 1);
    }
    int rc = det_reserve(c, &c->det_rows, &c->det_rows_bytes, std::max(rows_bytes, sizeof(double)));
    if (rc) return rc;
    if (!accumulate && (rc = det_reserve(c, &c->det_out, &c->det_out_bytes, (size_t)cnt * npix * sizeof(double)))) return rc;
    const double* ditems = nullptr;
    if ((rc = arena_push(c, rec.data(), rec.size(), &ditems))) return rc;
    if (max_block_rows > 0) {
      const size_t threads = (size_t)max_block_rows * nx;
      const dim3 grid((unsigned)std::min<size_t>((threads + kThreads - 1) / kThreads, 16384), cnt);
      dispatch_layout(c, [&](auto t, auto br) {
        hipLaunchKernelGGL((detector_rows_kernel<decltype(br)::value, Lay<decltype(t)>::BC>), grid, block, 0, c->stream, (const double*)c->psf,
                           c->item_stride, c->pitch, n, ditems, g, c->det_rows);
      });
      HIPCHK(c, hipGetLastError());
    }
    const dim3 grid2((unsigned)std::min<size_t>((npix + kThreads - 1) / kThreads, 16384));
    hipLaunchKernelGGL(detector_cols_kernel, grid2, block, 0, c->stream, (const double*)c->det_rows, ditems, cnt, n, g,
                       accumulate ? c->det_img : c->det_out, accumulate ? 1 : 0);
    HIPCHK(c, hipGetLastError());
    if (!accumulate && (rc = copy_to_host(c, host_out + (size_t)start * npix, c->det_out, (size_t)cnt * npix * sizeof(double))))
      return rc;
    start = end;
  }
  return PAOS_OK;
}

}  // namespace

extern "C" {

int paos_detector_begin(paos_ctx* c, const double* geom) {
  if (c) (void)hipSetDevice(c->device);
  if (!c || !geom) return fail(c, PAOS_EINVAL, "null context or geometry");
  const double nx = geom[0], ny = geom[1];
  if (!(nx >= 1 && nx <= 4096 && nx == std::floor(nx)) || !(ny >= 1 && ny <= 4096 && ny == std::floor(ny)))
    return fail(c, PAOS_EINVAL, "detector nx and ny must be integers in 1..4096");
  if (!finite_positive(geom[2]) || !finite_positive(geom[3])) return fail(c, PAOS_EINVAL, "detector pitch must be finite and positive");
  if (!std::isfinite(geom[4]) || !std::isfinite(geom[5])) return fail(c, PAOS_EINVAL, "detector centre must be finite");
  const size_t bytes = (size_t)nx * (size_t)ny * sizeof(double);
  if (c->det_img && (size_t)c->det_nx * c->det_ny * sizeof(double) != bytes) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    (void)hipFree(c->det_img);
    c->det_img = nullptr;
  }
  c->det_set = false;
  if (!c->det_img) HIPCHK(c, hipMalloc(&c->det_img, bytes));
  HIPCHK(c, hipMemsetAsync(c->det_img, 0, bytes, c->stream));
  c->det_nx = (int)nx; c->det_ny = (int)ny;
  for (int k = 0; k < 4; ++k) c->det_geom[k] = geom[2 + k];
  c->det_set = true;
  return PAOS_OK;
}

int paos_detector_add(paos_ctx* c, const double* per_item) {
  if (c) (void)hipSetDevice(c->device);
  if (!c) return fail(c, PAOS_EINVAL, "null context");
  return detector_run(c, per_item, PAOS_DETECTOR_ITEM, nullptr);
}

int paos_detector_add_placed(paos_ctx* c, const double* per_item) {
  if (c) (void)hipSetDevice(c->device);
  if (!c) return fail(c, PAOS_EINVAL, "null context");
  return detector_run(c, per_item, PAOS_DETECTOR_PLACED_ITEM, nullptr);
}

int paos_detector_images(paos_ctx* c, const double* per_item, double* host_out) {
  if (c) (void)hipSetDevice(c->device);
  if (!c || !host_out) return fail(c, PAOS_EINVAL, "null context or output buffer");
  return detector_run(c, per_item, PAOS_DETECTOR_ITEM, host_out);
}

int paos_detector_images_placed(paos_ctx* c, const double* per_item, double* host_out) {
  if (c) (void)hipSetDevice(c->device);
  if (!c || !host_out) return fail(c, PAOS_EINVAL, "null context or output buffer");
  return detector_run(c, per_item, PAOS_DETECTOR_PLACED_ITEM, host_out);
}

int paos_detector_fetch(paos_ctx* c, double* host_out) {
  if (c) (void)hipSetDevice(c->device);
  if (!c || !host_out) return fail(c, PAOS_EINVAL, "null context or output buffer");
  if (!c->det_set) return fail(c, PAOS_EINVAL, "no detector (paos_detector_begin)");
  return copy_to_host(c, host_out, c->det_img, (size_t)c->det_nx * c->det_ny * sizeof(double));
}

}  // extern "C"
