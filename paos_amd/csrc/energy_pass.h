// energy_pass.h -- encircled / ensquared energy of the kept PSFs about their own centres (energy.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace paos {

// ---- energy profiles of the kept PSFs (paos_ee_*, include/paos_hip.h; README.md, "Encircled energy") ------------------
// Three launches, no float atomics, every sum in a fixed order:
//   1. ee_sums_kernel + ee_centre_kernel: one sweep over the PSF buffer in memory order -- S, Sx, Sy, the peak and its
//      first position in row-major order -- and from them the item's centre (the centroid's two divisions happen here,
//      on the device), written to summary[item][kEeSummary];
//   2. ee_rings_kernel: one wave per band of kEeBandRows rows that the largest circle can reach.  Along one side of a
//      row |x| grows with the lane, and the rounded d2 (and max(|x|, |y|)) with it, so the ring index is monotone
//      across the wave: a segmented shuffle scan sums every ring's run of pixels and the last lane of a run adds it to
//      the ring's LDS slot.  Which ring a pixel belongs to is settled by the comparisons of the definition
//      (d2 <= t_b, max(|x|, |y|) <= r_b); the square root only says where to start looking;
//   3. ee_scan_kernel: the bands' ring sums added in a fixed two-level order, then a log-depth inclusive scan across
//      the rings: ee[b] is the sum of rings 0 .. b.
// Every operation below is fp64 and rounded once (the library is built with -ffp-contract=off).
enum { kEeItem = 4 };      // per-item record: delta, aspect, given cx, given cy
enum { kEeSummary = 9 };   // S, Sx, Sy, peak, peak_col, peak_row, cx, cy, fallback
enum { kEeSumVals = 5 };   // per-workgroup partials of launch 1: S, Sx, Sy, peak, row-major index of the peak
enum { kEeSumThreads = 256, kEeMaxSumBlocks = 1024 };
enum { kEeBandRows = 16 };  // rows per wave of launch 2 (a multiple of both block heights)
enum { kEeBandGroup = 16 }; // bands per inner sum of launch 3
enum { kEeMaxBins = 1024 };

__host__ __device__ inline double ee_radius(int b, double delta) { return (double)(b + 1) * delta; }
__host__ __device__ inline double ee_radius2(int b, double delta) {
  const double r = ee_radius(b, delta);
  return r * r;
}

// the smallest b in [0, bins] with d2 <= t_b (bins: in no circle)
__device__ __forceinline__ int ee_circle_index(double d2, double delta, int bins) {
  const double q = fmin(sqrt(d2) / delta, (double)bins);
  int b = max((int)q - 1, 0);
  while (b > 0 && d2 <= ee_radius2(b - 1, delta)) --b;
  while (b < bins && !(d2 <= ee_radius2(b, delta))) ++b;
  return b;
}
// the smallest b in [0, bins] with m <= r_b, m = max(|x|, |y|)
__device__ __forceinline__ int ee_square_index(double m, double delta, int bins) {
  const double q = fmin(m / delta, (double)bins);
  int b = max((int)q - 1, 0);
  while (b > 0 && m <= ee_radius(b - 1, delta)) --b;
  while (b < bins && !(m <= ee_radius(b, delta))) ++b;
  return b;
}

struct EeMax {
  double v;
  unsigned at;  // row * n + col
};
__device__ __forceinline__ void ee_max_take(EeMax& a, double v, unsigned at) {
  if (v > a.v || (v == a.v && at < a.at)) a = {v, at};
}

// sum / first maximum over the workgroup in a fixed order: shuffle tree per wave, then the waves in order
__device__ __forceinline__ void ee_block_reduce(double (&s)[3], EeMax& mx, double (*sh)[kEeSumVals]) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int q = 0; q < 3; ++q) s[q] += __shfl_down(s[q], off, 64);
    const double ov = __shfl_down(mx.v, off, 64);
    const unsigned oa = __shfl_down(mx.at, off, 64);
    ee_max_take(mx, ov, oa);
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    sh[wave][0] = s[0]; sh[wave][1] = s[1]; sh[wave][2] = s[2]; sh[wave][3] = mx.v; sh[wave][4] = (double)mx.at;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) {
      s[0] += sh[w][0]; s[1] += sh[w][1]; s[2] += sh[w][2];
      ee_max_take(mx, sh[w][3], (unsigned)sh[w][4]);
    }
  }
}

// Launch 1: pairs of neighbouring columns (one 16 B load) in memory order.
template <int BR, int BC>
__global__ void __launch_bounds__(kEeSumThreads) ee_sums_kernel(const double* __restrict__ psf, unsigned item_stride, unsigned pitch,
                                                               int n, double* __restrict__ partial) {
  static_assert(BC == 2, "a pair of columns is one block line");
  __shared__ double sh[kEeSumThreads / 64][kEeSumVals];
  const int item = blockIdx.y;
  const double2* p = reinterpret_cast<const double2*>(psf + (size_t)item * item_stride);
  const unsigned pairs = item_stride / 2;
  double s[3] = {0.0, 0.0, 0.0};
  EeMax mx{-INFINITY, 0xffffffffu};
  for (unsigned q = blockIdx.x * blockDim.x + threadIdx.x; q < pairs; q += gridDim.x * blockDim.x) {
    const unsigned m = 2 * q, brow = m / pitch, rem = m % pitch;
    if (rem >= (unsigned)n * BR) continue;  // the padding of a block row
    const unsigned in = rem % (BR * BC);
    const unsigned row = brow * BR + in / BC, col = (rem / (BR * BC)) * BC;
    const double2 v = p[q];
    const double x0 = (double)col, x1 = (double)(col + 1), y = (double)row;
    s[0] += v.x; s[0] += v.y;
    s[1] += v.x * x0; s[1] += v.y * x1;
    s[2] += v.x * y; s[2] += v.y * y;
    ee_max_take(mx, v.x, row * n + col);
    ee_max_take(mx, v.y, row * n + col + 1);
  }
  ee_block_reduce(s, mx, sh);
  if (threadIdx.x == 0) {
    double* out = partial + ((size_t)item * gridDim.x + blockIdx.x) * kEeSumVals;
    out[0] = s[0]; out[1] = s[1]; out[2] = s[2]; out[3] = mx.v; out[4] = (double)mx.at;
  }
}

// ... the workgroups' partials in a fixed order, and the centre: summary[item] = S, Sx, Sy, peak, peak_col, peak_row, cx, cy, fallback
__global__ void __launch_bounds__(kEeSumThreads) ee_centre_kernel(const double* __restrict__ partial, int nblocks, int n, int centre_mode,
                                                                 const double* __restrict__ items, double* __restrict__ summary) {
  __shared__ double sh[kEeSumThreads / 64][kEeSumVals];
  const int item = blockIdx.x;
  double s[3] = {0.0, 0.0, 0.0};
  EeMax mx{-INFINITY, 0xffffffffu};
  for (int b = threadIdx.x; b < nblocks; b += blockDim.x) {
    const double* q = partial + ((size_t)item * nblocks + b) * kEeSumVals;
    s[0] += q[0]; s[1] += q[1]; s[2] += q[2];
    ee_max_take(mx, q[3], (unsigned)q[4]);
  }
  ee_block_reduce(s, mx, sh);
  if (threadIdx.x != 0) return;
  const double pc = (double)(mx.at % (unsigned)n), pr = (double)(mx.at / (unsigned)n);
  double cx, cy, fallback = 0.0;
  if (centre_mode == 0) {  // PAOS_EE_GIVEN
    cx = items[(size_t)item * kEeItem + 2];
    cy = items[(size_t)item * kEeItem + 3];
  } else if (centre_mode == 2) {  // PAOS_EE_PEAK
    cx = pc;
    cy = pr;
  } else {  // PAOS_EE_CENTROID
    cx = s[1] / s[0];
    cy = s[2] / s[0];
    if (!(s[0] > 0.0) || !(cx >= 0.0 && cx < (double)n) || !(cy >= 0.0 && cy < (double)n)) {
      cx = cy = 0.5 * (double)n;
      fallback = 1.0;
    }
  }
  double* out = summary + (size_t)item * kEeSummary;
  out[0] = s[0]; out[1] = s[1]; out[2] = s[2]; out[3] = mx.v; out[4] = pc; out[5] = pr; out[6] = cx; out[7] = cy; out[8] = fallback;
}

// the runs of equal keys (monotone across the wave) summed by a segmented shuffle scan; the last lane of a run adds it to its slot
__device__ __forceinline__ void ee_add_runs(double v, int key, int lane, int bins, double* slot) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const double vu = __shfl_up(v, off, 64);
    const int ku = __shfl_up(key, off, 64);
    if (lane >= off && ku == key) v = vu + v;
  }
  const int kn = __shfl_down(key, 1, 64);
  if ((lane == 63 || kn != key) && key < bins) slot[key] += v;
}

// Launch 2: band `blockIdx.x` of item `blockIdx.y`: the rows [first + band * kEeBandRows, + kEeBandRows), first = the
// first row the largest circle can reach rounded down to a whole band.  One wave per workgroup; LDS: [1 + square][bins].
template <int BR, int BC>
__global__ void __launch_bounds__(64) ee_rings_kernel(const double* __restrict__ psf, unsigned item_stride, unsigned pitch, int n,
                                                     const double* __restrict__ items, const double* __restrict__ summary, int bins,
                                                     int square, double* __restrict__ partial) {
  extern __shared__ __align__(16) double ee_lds[];
  const int item = blockIdx.y, band = blockIdx.x, lane = threadIdx.x;
  const int ncurves = 1 + square;
  const double delta = items[(size_t)item * kEeItem], aspect = items[(size_t)item * kEeItem + 1];
  const double cx = summary[(size_t)item * kEeSummary + 6], cy = summary[(size_t)item * kEeSummary + 7];
  double* ring = ee_lds;
  double* sq = ee_lds + bins;
  for (int b = lane; b < ncurves * bins; b += 64) ee_lds[b] = 0.0;
  __syncthreads();
  const double rmax = ee_radius(bins - 1, delta), tmax = rmax * rmax;
  const double reach_x = (double)bins * delta, reach_y = reach_x / aspect;  // (both <= n / 2: paos_ee_compute)
  const int first = ((int)fmax(floor(cy - reach_y) - 1.0, 0.0) / kEeBandRows) * kEeBandRows;
  const int k0 = first + band * kEeBandRows;
  if (k0 < n) {
    const int jl = (int)floor(cx);  // 0 <= cx < n
    const int nch = (int)fmin(ceil((reach_x + 2.0) / 64.0), (double)(n / 64));
    const double* base = psf + (size_t)item * item_stride;
    for (int kb = k0 / BR; kb < (k0 + kEeBandRows) / BR; ++kb) {
      double y[BR];
      bool live[BR];
      bool any = false;
#pragma unroll
      for (int r = 0; r < BR; ++r) {
        y[r] = ((double)(kb * BR + r) - cy) * aspect;
        // fl(x x + y y) >= y y: a row with y y > t_max holds no pixel of a circle, one with |y| > r_max none of a square
        live[r] = (y[r] * y[r] <= tmax) || (square && fabs(y[r]) <= rmax);
        any = any || live[r];
      }
      if (!any) continue;
      const double* rowbase = base + (size_t)kb * pitch;
      for (int side = 0; side < 2; ++side) {
        for (int ch = 0; ch < nch; ++ch) {
          // left: jl, jl - 1, ... (x <= 0); right: jl + 1, jl + 2, ... (x > 0): |x| grows with the lane on both
          const int j = side == 0 ? jl - 64 * ch - lane : jl + 1 + 64 * ch + lane;
          if (side == 0 ? jl - 64 * ch < 0 : jl + 1 + 64 * ch >= n) break;  // (the whole chunk is off the grid)
          const bool inside = j >= 0 && j < n;
          const double x = (double)j - cx;
          const double* blk = rowbase + (size_t)((inside ? j : 0) / BC) * (BR * BC) + ((inside ? j : 0) % BC);
          double v[BR];
#pragma unroll
          for (int r = 0; r < BR; ++r) v[r] = (inside && live[r]) ? blk[r * BC] : 0.0;
#pragma unroll
          for (int r = 0; r < BR; ++r) {
            if (!live[r] || __ballot(v[r] != 0.0) == 0) continue;  // (wave-uniform: zeros add nothing)
            const double d2 = x * x + y[r] * y[r];
            ee_add_runs(v[r], ee_circle_index(d2, delta, bins), lane, bins, ring);
            if (square) ee_add_runs(v[r], ee_square_index(fmax(fabs(x), fabs(y[r])), delta, bins), lane, bins, sq);
            __syncthreads();  // (one wave: orders this step's LDS updates before the next step's)
          }
        }
      }
    }
  }
  __syncthreads();
  double* out = partial + ((size_t)item * gridDim.x + band) * ncurves * bins;
  for (int b = lane; b < ncurves * bins; b += 64) out[b] = ee_lds[b];
}

// Launch 3: curve `blockIdx.x` (0 circles, 1 squares) of item `blockIdx.y`; thread b owns ring b.
__global__ void __launch_bounds__(kEeMaxBins) ee_scan_kernel(const double* __restrict__ partial, int nbands, int bins, int ncurves,
                                                            double* __restrict__ curves) {
  __shared__ double buf[2][kEeMaxBins];
  const int item = blockIdx.y, curve = blockIdx.x, b = threadIdx.x;
  double tot = 0.0;
  if (b < bins) {
    const double* p = partial + ((size_t)item * nbands * ncurves + curve) * bins + b;
    for (int g = 0; g < nbands; g += kEeBandGroup) {
      double s = 0.0;
      for (int q = g; q < min(g + kEeBandGroup, nbands); ++q) s += p[(size_t)q * ncurves * bins];
      tot += s;
    }
  }
  int cur = 0;
  buf[0][b] = tot;
  __syncthreads();
  for (int off = 1; off < bins; off <<= 1) {
    double v = buf[cur][b];
    if (b >= off) v = buf[cur][b - off] + v;
    buf[cur ^ 1][b] = v;
    cur ^= 1;
    __syncthreads();
  }
  if (b < bins) curves[((size_t)item * ncurves + curve) * bins + b] = buf[cur][b];
}

}  // namespace paos
