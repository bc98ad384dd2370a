// detector_pass.h -- the two contractions that rebin kept PSFs onto a detector pixel grid (detector.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace paos {

// ---- broadband PSFs on a detector pixel grid (paos_detector_*, include/paos_hip.h) -----------------------------------
// Grid column j of an item with pitch dx spans [(j - N/2 - 1/2) dx, (j - N/2 + 1/2) dx]; detector column m spans
// [xc + (m - nx/2) px, xc + (m + 1 - nx/2) px] (rows alike, with dy, yc, py).  Both are expressed in grid-pixel units,
// where column j spans [j, j + 1]: detector edge m sits at det_edge(m) below, and the overlap fraction
// fx(j, m) = max(0, min(j + 1, e(m + 1)) - max(j, e(m))).  The edge is formed by exactly these IEEE operations
// (no contraction: the library is built with -ffp-contract=off), so a NumPy restatement that writes them the same way
// gets the same fractions bit for bit.
// (g.xc / g.yc are not read by the kernels: every item carries its own detector centre in its record, measured from its
// grid centre -- the detector's (xc, yc), or xc - x0_i / yc - y0_i for an item placed at (x0_i, y0_i), paos_detector_*_placed)
struct DetGeom {
  int nx, ny;
  double px, py, xc, yc;
};
// per-item device record: dx, dy, w, k0, k1, scratch offset, batch item, (pad), detector centre x, y seen from the item
enum { kDetItem = 10 };

__host__ __device__ inline double det_edge(int m, int nd, double pitch, double centre, double d, int n) {
  const double t = (double)m - 0.5 * (double)nd;  // exact
  const double pos = centre + t * pitch;
  return pos / d + (0.5 * (double)n + 0.5);
}
// [floor(e0), ceil(e1)) clipped to [0, n): the grid lines a detector line can overlap
__host__ __device__ inline int det_lo(double e, int n) { return (int)fmin(fmax(floor(e), 0.0), (double)n); }
__host__ __device__ inline int det_hi(double e, int n) { return (int)fmin(fmax(ceil(e), 0.0), (double)n); }

// Row contraction: R[off + (k - k0) nx + m] = sum_j PSF[k, j] fx(j, m) for the rows [k0, k1) of the item's footprint.
// One thread = one detector column m and one block row of the PSF (BR rows): for each grid column j it reads the BR
// values of the block that holds (rows of the block row, j) -- the wave as a whole walks whole 64 / 128 B blocks.
template <int BR, int BC>
__global__ void __launch_bounds__(256) detector_rows_kernel(const double* __restrict__ psf, unsigned item_stride, unsigned pitch,
                                                            int n, const double* __restrict__ items, DetGeom g,
                                                            double* __restrict__ R) {
  const double* p = items + (size_t)blockIdx.y * kDetItem;
  const double dx = p[0], xc = p[8];
  const int k0 = (int)p[3], k1 = (int)p[4];
  if (k1 <= k0) return;
  const size_t off = (size_t)p[5];
  const int item = (int)p[6];
  const int kb0 = k0 / BR, nbr = (k1 - 1) / BR - kb0 + 1;
  const size_t total = (size_t)nbr * g.nx;
  for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
    const int kb = kb0 + (int)(t / g.nx), m = (int)(t % g.nx);
    const double e0 = det_edge(m, g.nx, g.px, xc, dx, n), e1 = det_edge(m + 1, g.nx, g.px, xc, dx, n);
    const int jlo = det_lo(e0, n), jhi = det_hi(e1, n);
    const double* base = psf + (size_t)item * item_stride + (size_t)kb * pitch;
    double acc[BR];
#pragma unroll
    for (int r = 0; r < BR; ++r) acc[r] = 0.0;
    for (int j = jlo; j < jhi; ++j) {
      const double f = fmin((double)(j + 1), e1) - fmax((double)j, e0);
      if (!(f > 0.0)) continue;
      const double* blk = base + (size_t)(j / BC) * (BR * BC) + (j % BC);
#pragma unroll
      for (int r = 0; r < BR; ++r) acc[r] += blk[r * BC] * f;
    }
#pragma unroll
    for (int r = 0; r < BR; ++r) {
      const int k = kb * BR + r;
      if (k >= k0 && k < k1) R[off + (size_t)(k - k0) * g.nx + m] = acc[r];
    }
  }
}

// Column contraction: A_i[row, m] = sum_k fy(k, row) R_i[k, m].  One thread = one detector pixel; it walks the items of
// the chunk in ascending order, so accumulate != 0 adds w_i A_i into out[row, m] item after item (image <- image + w_i A_i,
// each product and sum rounded once; no atomics); accumulate == 0 writes A_i to out[i][row][m].
__global__ void __launch_bounds__(256) detector_cols_kernel(const double* __restrict__ R, const double* __restrict__ items, int nitems,
                                                            int n, DetGeom g, double* __restrict__ out, int accumulate) {
  const size_t npix = (size_t)g.nx * g.ny;
  for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < npix; q += (size_t)gridDim.x * blockDim.x) {
    const int row = (int)(q / g.nx), m = (int)(q % g.nx);
    double acc = accumulate ? out[q] : 0.0;
    for (int li = 0; li < nitems; ++li) {
      const double* p = items + (size_t)li * kDetItem;
      const double dy = p[1], w = p[2], yc = p[9];
      const int k0 = (int)p[3], k1 = (int)p[4];
      const size_t off = (size_t)p[5];
      const double e0 = det_edge(row, g.ny, g.py, yc, dy, n), e1 = det_edge(row + 1, g.ny, g.py, yc, dy, n);
      const int klo = max(det_lo(e0, n), k0), khi = min(det_hi(e1, n), k1);
      double a = 0.0;
      for (int k = klo; k < khi; ++k) {
        const double f = fmin((double)(k + 1), e1) - fmax((double)k, e0);
        if (f > 0.0) a += R[off + (size_t)(k - k0) * g.nx + m] * f;
      }
      if (accumulate) acc = acc + w * a;
      else out[(size_t)li * npix + q] = a;
    }
    if (accumulate) out[q] = acc;
  }
}

}  // namespace paos
