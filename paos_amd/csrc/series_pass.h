// series_pass.h -- the launches of a pointing series (series.hip): detector frames of the kept PSFs while the line of
// sight moves, and the flux inside boxes of detector pixels (README.md, "Pointing series"); and of the broadband sum of
// such frames over the items of a batch (series_sum.hip; README.md, "Broadband series").
#pragma once
#include <hip/hip_runtime.h>

// det_edge, det_lo, det_hi and DetGeom come from detector_pass.h, so that both products form every edge by the same
// operations.  That header also defines a kernel that is not a template, which detector.hip owns: a second unit that
// includes the header has to give its copy another name (it is never launched from here).
#define detector_cols_kernel series_unit_detector_cols_kernel
#include "detector_pass.h"
#undef detector_cols_kernel

namespace paos {

enum { kSeriesItem = 4 };       // per-item record: dx, dy, x0, y0
constexpr int kSeriesThreads = 256;  // per workgroup of the frames kernel
constexpr int kSeriesWave = 64;      // the flux kernel's workgroup: one wave

// Frames: one thread = one detector pixel (row, m) of frame blockIdx.y of the chunk and item blockIdx.z of the chunk.  In
// frame t the item's grid centre lies at X = x0 + ox_t, Y = y0 + oy_t and the detector centre seen from the item at xc - X,
// yc - Y (two IEEE operations per axis; no contraction); from there on the value is the one the two contractions of
// detector_pass.h form, in their order: for the grid rows k under the detector row, ascending, r = sum_j P[k][j] fx(j, m)
// over ascending j, then a = a + r fy(k, row) -- without the R scratch in between, since the (k, j) window of a pixel is a
// few grid pixels a side and its lines stay in cache from one pixel to its neighbours and from one frame to the next.
// The detector edges depend on (t, m) and (t, row) only.  A pixel whose window misses the grid reads nothing and is +0.
// out: [items of the chunk][frames of the chunk][ny][nx]; with a response every value is multiplied by g[row][m] once.
// The value of detector pixel (row, m) in the frame whose offset is o = (ox, oy), of the item with record p = dx, dy, x0, y0
// and PSF `base`: the one place where it is formed, so that every kernel that needs a frame value forms the same double.
template <int BR, int BC>
__device__ __forceinline__ double series_pixel(const double* __restrict__ base, unsigned pitch, int n, const double* __restrict__ p,
                                               const double* __restrict__ o, const DetGeom& g, int row, int m) {
  const double dx = p[0], dy = p[1];
  const double gx = p[2] + o[0], gy = p[3] + o[1];
  const double xc = g.xc - gx, yc = g.yc - gy;
  const double e0x = det_edge(m, g.nx, g.px, xc, dx, n), e1x = det_edge(m + 1, g.nx, g.px, xc, dx, n);
  const double e0y = det_edge(row, g.ny, g.py, yc, dy, n), e1y = det_edge(row + 1, g.ny, g.py, yc, dy, n);
  const int jlo = det_lo(e0x, n), jhi = det_hi(e1x, n);
  const int klo = det_lo(e0y, n), khi = det_hi(e1y, n);
  double a = 0.0;
  for (int k = klo; k < khi; ++k) {
    const double fy = fmin((double)(k + 1), e1y) - fmax((double)k, e0y);
    if (!(fy > 0.0)) continue;
    const double* line = base + (size_t)(k / BR) * pitch + (size_t)(k % BR) * BC;
    double r = 0.0;
    for (int j = jlo; j < jhi; ++j) {
      const double fx = fmin((double)(j + 1), e1x) - fmax((double)j, e0x);
      if (fx > 0.0) r = r + line[(size_t)(j / BC) * (BR * BC) + (j % BC)] * fx;
    }
    a = a + r * fy;
  }
  return a;
}

template <int BR, int BC>
__global__ void __launch_bounds__(kSeriesThreads) series_frames_kernel(const double* __restrict__ psf, unsigned item_stride, unsigned pitch,
                                                                       int n, const double* __restrict__ items,
                                                                       const double* __restrict__ offsets, size_t offsets_stride,
                                                                       const double* __restrict__ response, DetGeom g, int item0,
                                                                       int frame0, double* __restrict__ out) {
  const size_t npix = (size_t)g.nx * g.ny;
  const size_t q = (size_t)blockIdx.x * kSeriesThreads + threadIdx.x;
  if (q >= npix) return;
  const int row = (int)(q / g.nx), m = (int)(q % g.nx);
  const int item = item0 + (int)blockIdx.z, t = frame0 + (int)blockIdx.y;
  double a = series_pixel<BR, BC>(psf + (size_t)item * item_stride, pitch, n, items + (size_t)item * kSeriesItem,
                                  offsets + (size_t)item * offsets_stride + (size_t)t * 2, g, row, m);
  if (response) a = a * response[q];
  out[((size_t)blockIdx.z * gridDim.y + blockIdx.y) * npix + q] = a;
}

// Broadband sum (README.md, "Broadband series"): one thread = one detector pixel of frame frame0 + blockIdx.y of the
// accumulator S[frames][ny][nx].  It loads S once, walks the items of the add in ascending order -- an item whose weight in
// this frame is 0.0 is skipped and nothing of it is read; the weight is the same for the whole workgroup, so the skip does
// not diverge -- adds fl(w F) with F from series_pixel, one rounding for the product and one for the sum, and stores S
// once.  weights[i * w_item + t * w_frame]: (1, 0) for one weight per item, (frames, 1) for one per item and frame.
template <int BR, int BC>
__global__ void __launch_bounds__(kSeriesThreads) series_sum_kernel(const double* __restrict__ psf, unsigned item_stride, unsigned pitch,
                                                                    int n, int batch, const double* __restrict__ items,
                                                                    const double* __restrict__ offsets, size_t offsets_stride,
                                                                    const double* __restrict__ weights, size_t w_item, size_t w_frame,
                                                                    DetGeom g, int frame0, double* __restrict__ sum) {
  const size_t npix = (size_t)g.nx * g.ny;
  const size_t q = (size_t)blockIdx.x * kSeriesThreads + threadIdx.x;
  if (q >= npix) return;
  const int row = (int)(q / g.nx), m = (int)(q % g.nx);
  const int t = frame0 + (int)blockIdx.y;
  double* s = sum + (size_t)t * npix + q;
  double a = *s;
  for (int i = 0; i < batch; ++i) {
    const double w = weights[(size_t)i * w_item + (size_t)t * w_frame];
    if (w == 0.0) continue;
    const double f = series_pixel<BR, BC>(psf + (size_t)i * item_stride, pitch, n, items + (size_t)i * kSeriesItem,
                                          offsets + (size_t)i * offsets_stride + (size_t)t * 2, g, row, m);
    a = a + w * f;
  }
  *s = a;
}

// Flux: one wave = one (box, frame, item) of the chunk.  Lane l adds the box's pixels q = l, l + 64, l + 128, ... in
// ascending order (q counts the box row-major) starting from +0.0; the 64 partial sums are combined by the tree
// p[l] = p[l] + p[l + s], s = 32, 16, 8, 4, 2, 1; p[0] is the flux.  No atomics: the order is the same whatever else runs.
// boxes: [nboxes][4] = m0, m1, n0, n1 (columns m0 .. m1-1, rows n0 .. n1-1), as doubles.  flux: [batch][frames][nboxes].
// With a response g[ny][nx] (the broadband sum applies it when reading) a pixel enters as fl(F g); nullptr: F itself.
__global__ void __launch_bounds__(kSeriesWave) series_flux_kernel(const double* __restrict__ frames, const double* __restrict__ boxes,
                                                                  int nboxes, int nx, int ny, int item0, int frame0, int total_frames,
                                                                  double* __restrict__ flux, const double* __restrict__ response) {
  const int box = (int)blockIdx.x, lane = (int)threadIdx.x;
  const double* b = boxes + (size_t)box * 4;
  const int m0 = (int)b[0], m1 = (int)b[1], n0 = (int)b[2], n1 = (int)b[3];
  const int w = m1 - m0, count = w * (n1 - n0);
  const size_t npix = (size_t)nx * ny;
  const double* f = frames + ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * npix;
  double p = 0.0;
  for (int q = lane; q < count; q += kSeriesWave) {
    const size_t at = (size_t)(n0 + q / w) * nx + (m0 + q % w);
    double v = f[at];
    if (response) v = v * response[at];
    p = p + v;
  }
#pragma unroll
  for (int s = kSeriesWave / 2; s >= 1; s >>= 1) p = p + __shfl_down(p, s, kSeriesWave);
  if (lane == 0) flux[((size_t)(item0 + (int)blockIdx.z) * total_frames + (frame0 + (int)blockIdx.y)) * nboxes + box] = p;
}

}  // namespace paos
