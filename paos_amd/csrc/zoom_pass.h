// zoom_pass.h -- zoomed PSF windows (paos_zoom_compute): the exact trigonometric interpolant of the last-surface field,
// sampled on an M x M window at 1/s of the grid pitch, as two dense contractions with REAL weights
//
//   stage Y:  T[x][p] = sum_k Wy[p][k] u[k][x]        (M x N x N,  u in the field's blocked layout, either precision)
//   stage X:  U[p][q] = sum_x Wx[q][x] T[x][p]        (M x M x N,  T complex128, kept transposed: p runs fastest)
//
// on the fp64 matrix instruction v_mfma_f64_16x16x4_f64.  Both stages are ONE kernel, out[d][w] = sum_k W[w][k] D[k][d]:
// the weights are the A operand (16 rows w x 4 k, one double per lane: row = lane & 15, k = lane >> 4), the complex data
// the B operand (4 k x 16 columns d: k = lane >> 4, column = lane & 15; a lane's one load of a complex number yields
// the operand of the real-part product and of the imaginary-part product, which share A), and the 16 x 16 results sit
// in four doubles per lane at column = lane & 15, row = (lane >> 4) + 4 * register -- the f64 form's own map, not the
// f32 forms' (lane >> 4) * 4 + register.  A wave owns 16 columns d and PT tiles of 16 rows w; its 2 PT accumulators
// (16 VGPRs per tile) stay in registers over the whole k loop, and every output element is one k-ordered chain inside
// one wave: no atomics, no split of the sum, the same bits whatever the batch size, the item's position or PT.
//
// Weights are not stored densely.  W[w][k] = tab[base[w] + ((off[w] - k) mod N)], where tab holds the s phase rows of
// the Dirichlet kernel for the centre's fractional part (paos_zoom_weights) and base / off are two numbers per fine
// sample (the row of its phase, and the grid pixel it sits on or just behind); a row whose sample falls on a grid
// pixel is a unit vector, so such samples are copies of the field, bit for bit.
#pragma once
#include "fft_core.h"

namespace paos {

typedef double zoom_f64x4 __attribute__((ext_vector_type(4)));

struct ZoomArgs {
  const void* src;        // STAGE 0: the batch of fields, complex<T>, blocked layout; STAGE 1: T, [item][N][M] complex128
  cx<double>* dst_c;      // STAGE 0: T; STAGE 1: the complex window [item][M][M], or null
  double* dst_i;          // STAGE 1: |U|^2, [item][M][M]
  const double* tabs;     // the context's phase tables
  const double* par;      // [item][2 (x, y)][2 (base, off)][M]
  int n, m;               // grid size, window size
  int nd;                 // tiles of 16 columns d: N / 16 (STAGE 0), M / 16 (STAGE 1)
  unsigned pitch;         // elements between block rows of the field's layout
  unsigned item_stride;   // elements between the fields of two items
  int br_shift;           // log2 of the layout's block height (blocks are 2 columns wide)
};

constexpr int kZoomWaves = 4;  // waves per workgroup: four neighbouring d tiles, the same w tiles (their A loads hit L1)

template <typename T, int STAGE>
__device__ __forceinline__ cx<double> zoom_load(const cx<T>* s, int k, int d, const ZoomArgs& a) {
  size_t idx;
  if (STAGE == 0) {
    const unsigned br = 1u << a.br_shift;
    idx = (size_t)((unsigned)k >> a.br_shift) * a.pitch + ((unsigned)d >> 1) * (br * 2) + ((unsigned)k & (br - 1)) * 2 + (d & 1);
  } else {
    idx = (size_t)k * a.m + d;
  }
  const cx<T> v = s[idx];
  return {(double)v.x, (double)v.y};
}

template <typename T, int STAGE, int PT>
__global__ void __launch_bounds__(64 * kZoomWaves) zoom_kernel(ZoomArgs a) {
  const int lane = threadIdx.x & 63;
  const int dt = blockIdx.x * kZoomWaves + (threadIdx.x >> 6);
  if (dt >= a.nd) return;  // (whole waves; the kernel has no barrier)
  const int item = blockIdx.z;
  const int wt0 = blockIdx.y * PT, ntw = a.m >> 4;
  const int col = lane & 15, kq = lane >> 4;
  const int d = dt * 16 + col;
  const int nmask = a.n - 1;
  // STAGE 0 contracts along y with the y weights, STAGE 1 along x with the x weights
  const double* par = a.par + ((size_t)item * 2 + (STAGE == 0 ? 1 : 0)) * 2 * a.m;
  const cx<T>* s = reinterpret_cast<const cx<T>*>(a.src) +
                   (STAGE == 0 ? (size_t)item * a.item_stride : (size_t)item * a.n * a.m);

  const double* row[PT];  // this lane's weight row of every tile (A operand: row = lane & 15), and where it starts
  int off[PT];
#pragma unroll
  for (int t = 0; t < PT; ++t) {
    const int w = (wt0 + t < ntw ? wt0 + t : wt0) * 16 + col;
    row[t] = a.tabs + (size_t)par[w];
    off[t] = (int)par[a.m + w];
  }
  zoom_f64x4 accr[PT], acci[PT];
#pragma unroll
  for (int t = 0; t < PT; ++t) accr[t] = acci[t] = zoom_f64x4{0.0, 0.0, 0.0, 0.0};

  // one step ahead: the data and the weights of step k0 + 4 are loaded before the products of step k0 are issued
  cx<double> v = zoom_load<T, STAGE>(s, kq, d, a);
  double wv[PT];
#pragma unroll
  for (int t = 0; t < PT; ++t) wv[t] = row[t][(off[t] - kq) & nmask];
  for (int k0 = 0; k0 < a.n; k0 += 4) {
    const int kn = (k0 + 4 < a.n ? k0 + 4 : k0) + kq;
    const cx<double> vn = zoom_load<T, STAGE>(s, kn, d, a);
    double wn[PT];
#pragma unroll
    for (int t = 0; t < PT; ++t) wn[t] = row[t][(off[t] - kn) & nmask];
#pragma unroll
    for (int t = 0; t < PT; ++t) {
      if (wt0 + t < ntw) {  // wave-uniform
        accr[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(wv[t], v.x, accr[t], 0, 0, 0);
        acci[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(wv[t], v.y, acci[t], 0, 0, 0);
      }
    }
    v = vn;
#pragma unroll
    for (int t = 0; t < PT; ++t) wv[t] = wn[t];
  }

  // results: column d = lane & 15, row w = (lane >> 4) + 4 * register of the tile; both stages store at [d][w]
#pragma unroll
  for (int t = 0; t < PT; ++t) {
    if (wt0 + t >= ntw) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int w = (wt0 + t) * 16 + kq + 4 * r;
      const double re = accr[t][r], im = acci[t][r];
      if (STAGE == 0) {
        a.dst_c[((size_t)item * a.n + d) * a.m + w] = {re, im};
      } else {
        const size_t o = ((size_t)item * a.m + d) * a.m + w;
        a.dst_i[o] = __dadd_rn(__dmul_rn(re, re), __dmul_rn(im, im));
        if (a.dst_c) a.dst_c[o] = {re, im};
      }
    }
  }
}

}  // namespace paos
