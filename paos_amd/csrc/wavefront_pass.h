// wavefront_pass.h -- wavefront fits: the Zernike content and the OPD statistics of the field at a surface (wavefront.hip).
#pragma once
#include "fft_core.h"
#include "item_window.h"
#include "pointwise_shared.h"

namespace paos {

// ---- wavefront fits (paos_wavefront_*, include/paos_hip.h; README.md, "Wavefront fits") ------------------------------
// The device forms sums; the fit itself is host algebra on them (paos_amd/wavefront.py).  Per item, with the header of its
// Zernike parameter block (ZP_*), a floor min_intensity and the weighting (w = 1, or w = I):
//   support   pixel (k, j) is in Omega iff rho <= 1 and I > min_intensity (and the pupil weight != 0), with
//             x = (double)(j - N/2) dx, y = (double)(k - N/2) dy, rr = sqrt(fl(x x) + fl(y y)), rho = rr / radius --
//             zernike_gram_kernel's arithmetic -- and I = fl(fl(re re) + fl(im im)) on the components widened to double;
//   phase     phi = atan2(im', re'), re' = fl(fl(ux rx) + fl(uy ry)), im' = fl(fl(uy rx) - fl(ux ry)): the field turned
//             back by the reference phasor r = sum_Omega u (1 + 0i if that sum is zero or not finite: fallback);
//   sums      A[p][q] = sum_Omega fl(fl(w c_p) c_q), p <= q row by row, over the K + 1 columns [Z_0 .. Z_{K-1}, phi].
// Three launches (four kernels), no float atomics, every sum in a fixed order that depends on the item's own request and
// the grid alone -- not on the batch, the item's place in it or what the other items ask for:
//   1. wf_moments_kernel + wf_moments_final_kernel: count, r, sum sqrt(I), sum I over Omega, inside the rows and columns
//      the disk can reach (the host passes the box, the kernel tests membership itself); the final stage applies the
//      fallback and leaves the r that is used in device memory, so the host does not wait in front of launch 2;
//   2. wf_gram_kernel: zernike_gram_kernel's structure -- 128-pixel chunks, the K polynomial values of a pixel from one
//      Jacobi recurrence and one rotation into LDS, each thread owning its (p, q) pairs -- with the column phi, the row of
//      weights, sum w and sum w phi, and phi's extremes; chunks without a pixel of Omega are skipped;
//   3. wf_final_kernel: the workgroups' sums added in order, min / max taken over them.
// Every operation is fp64 and rounded once (the library is built with -ffp-contract=off).
enum { kWfSummary = 10 };  // count, r_re, r_im, sum sqrt(I), sum I, phi_min, phi_max, fallback, sum w, sum w phi
enum { kWfMoments = 5 };   // per-workgroup partials of launch 1: count, r_re, r_im, sum sqrt(I), sum I
enum { kWfExtra = 4 };     // behind the pairs in a workgroup's partials of launch 2: sum w, sum w phi, phi_min, phi_max
enum { kWfMaxK = 63 };     // K + 1 <= 64 columns
enum { kWfIntensity = 1 }; // weight_mode: 0 uniform, 1 intensity
enum { kWfStep = 8 };      // A, B, C, row of the cos polynomial, of the sin polynomial, their factors, padding

// The header of an item's request as both sweeps read it, the pixel geometry and the membership test: one definition, so
// that launch 1 and launch 2 agree on Omega bit for bit.
struct WfItem {
  double dx, dy, radius, floor_i;
  const double* pupil;  // the item's weight map in the field's layout, or null
  int n;

  __device__ __forceinline__ WfItem(const double* p, const double* min_intensity, const double* pupil_all, int item, int n_,
                                    unsigned item_stride)
      : dx(p[ZP_DX]), dy(p[ZP_DY]), radius(p[ZP_RADIUS]), floor_i(min_intensity[item]),
        pupil(pupil_all ? pupil_all + (size_t)item * item_stride : nullptr), n(n_) {}

  __device__ __forceinline__ void geometry(int r, int c, double& x, double& y, double& rr, double& rho) const {
    x = (double)(c - n / 2) * dx;
    y = (double)(r - n / 2) * dy;
    rr = sqrt(__dadd_rn(__dmul_rn(x, x), __dmul_rn(y, y)));
    rho = rr / radius;
  }
  static __device__ __forceinline__ double intensity(double ux, double uy) { return __dadd_rn(__dmul_rn(ux, ux), __dmul_rn(uy, uy)); }
  __device__ __forceinline__ bool member(double rho, double I, size_t m) const {
    return rho <= 1.0 && I > floor_i && (!pupil || pupil[m] != 0.0);
  }
};

// Launch 1: the filtered walk of the item's box (ItemWindow), five sums per workgroup -> partial[value][item][workgroup]
template <typename T, int BR, int BC>
__global__ void __launch_bounds__(kPwThreads)
    wf_moments_kernel(const cx<T>* field, const double* params, int param_stride, const double* min_intensity, const double* pupil,
                      const double* rows, const double* cols, int n, unsigned pitch, unsigned item_stride, double* partial) {
  const int item = blockIdx.y;
  const double* p = params + (size_t)item * param_stride;
  if (p[ZP_ENABLE] == 0.0) return;  // (the final stage writes the zeros)
  __shared__ double sh[kPwThreads / 64];
  const cx<T>* f = field + (size_t)item * item_stride;
  const WfItem it(p, min_intensity, pupil, item, n, item_stride);
  const ItemWindow<BR, BC> win(rows, cols, item, n, pitch, item_stride);
  double acc[kWfMoments] = {0.0, 0.0, 0.0, 0.0, 0.0};
  const size_t step = (size_t)gridDim.x * blockDim.x;
  for (size_t m = win.start((size_t)blockIdx.x * blockDim.x + threadIdx.x, step); m < win.total; m += step) {
    if (win.skips(m)) continue;
    int r, c;
    if (!layout_unmap<BR, BC>(m, n, pitch, r, c)) continue;
    double x, y, rr, rho;
    it.geometry(r, c, x, y, rr, rho);
    if (!(rho <= 1.0)) continue;
    const double ux = (double)f[m].x, uy = (double)f[m].y;
    const double I = WfItem::intensity(ux, uy);
    if (!it.member(rho, I, m)) continue;
    acc[0] += 1.0;
    acc[1] += ux;
    acc[2] += uy;
    acc[3] += sqrt(I);
    acc[4] += I;
  }
  const size_t plane = (size_t)gridDim.y * gridDim.x;
#pragma unroll
  for (int v = 0; v < kWfMoments; ++v) {
    store_block_sum(acc[v], sh, partial + v * plane);
    __syncthreads();  // (sh is read by thread 0 until here)
  }
}

// ... and the workgroups' sums in order: summary[item][0 .. 4, 7], and the reference phasor that launch 2 turns the field
// back by, r_used[item][2].  A switched-off item gets zeros (and r = 1).
static __global__ void __launch_bounds__(kPwThreads)
    wf_moments_final_kernel(const double* partial, int nparts, const double* params, int param_stride, double* summary, double* r_used) {
  const int item = blockIdx.x;
  __shared__ double sh[kPwThreads / 64];
  const bool on = params[(size_t)item * param_stride + ZP_ENABLE] != 0.0;
  const size_t plane = (size_t)gridDim.x * nparts;
  double s[kWfMoments];
#pragma unroll
  for (int v = 0; v < kWfMoments; ++v) {
    double acc = 0.0;
    if (on)
      for (int i = threadIdx.x; i < nparts; i += blockDim.x) acc += partial[v * plane + (size_t)item * nparts + i];
    s[v] = block_sum(acc, sh);
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    double* out = summary + (size_t)item * kWfSummary;
    const bool fallback = on && ((s[1] == 0.0 && s[2] == 0.0) || !isfinite(s[1]) || !isfinite(s[2]));
#pragma unroll
    for (int v = 0; v < kWfMoments; ++v) out[v] = s[v];
    out[7] = fallback ? 1.0 : 0.0;
    const bool own = on && !fallback;
    r_used[2 * item] = own ? s[1] : 1.0;
    r_used[2 * item + 1] = own ? s[2] : 0.0;
  }
}

constexpr int kWfAcc = ((kWfMaxK + 1) * (kWfMaxK + 2) / 2 + kGramThreads - 1) / kGramThreads;
constexpr int kWfLoad = 8;  // pixels whose LDS reads a thread of launch 2 has in flight per pair, uniform weights (kGramPix is a multiple)

// Launch 2.  LDS: K rows of polynomial values, the row of phi and, WEIGHTED, the row of weights, kGramRow doubles each;
// the sums per pixel slot (sum w, sum w phi, the extremes) are reduced through the same rows at the end.
// steps: one record of kWfStep doubles per step (am, k) of the recurrences, in the order in which they are walked -- the
// constants A, B, C of the step, the rows of its cos and sin polynomial (-1: not asked for) and their factors -- so that a
// step costs one load of consecutive doubles whose address depends on nothing loaded before (zernike_gram_kernel looks the
// row up and then the factor under it).  Measured: the launch takes the same time either way -- it waits for the LDS reads
// of the products, not for the polynomials (profiles/r22_wavefront_bench.md).
// rows: the block rows [first, total) of ItemWindow bound the chunks that are walked.
template <typename T, int BR, int BC, bool WEIGHTED>
__global__ void __launch_bounds__(kGramThreads)
    wf_gram_kernel(const cx<T>* field, const double* params, int param_stride, const double* min_intensity,
                   const double* pupil, const double* rows, const double* cols, const double* r_used, int n, unsigned pitch,
                   unsigned item_stride, int nmax, int K, const double* steps, double* partial) {
  extern __shared__ __attribute__((aligned(16))) double wbuf[];  // [K + 1 (+ 1)][kGramRow]
  const int item = blockIdx.y, tid = threadIdx.x;
  const double* p = params + (size_t)item * param_stride;
  const int ncol = K + 1, npairs = ncol * (ncol + 1) / 2;
  double* out = partial + ((size_t)item * gridDim.x + blockIdx.x) * (npairs + kWfExtra);
  if (p[ZP_ENABLE] == 0.0) {
    for (int q = tid; q < npairs + 2; q += kGramThreads) out[q] = 0.0;
    if (tid == 0) { out[npairs + 2] = INFINITY; out[npairs + 3] = -INFINITY; }
    return;
  }
  const WfItem it(p, min_intensity, pupil, item, n, item_stride);
  const bool origin_y = p[ZP_ORIGIN_Y] != 0.0;
  const double co = p[ZP_COS_OFF], so = p[ZP_SIN_OFF];
  const double rx = r_used[2 * item], ry = r_used[2 * item + 1];
  const cx<T>* f = field + (size_t)item * item_stride;
  const ItemWindow<BR, BC> win(rows, cols, item, n, pitch, item_stride);
  double* phirow = wbuf + K * kGramRow;
  double* wrow = wbuf + (K + 1) * kGramRow;  // (WEIGHTED only)
  int pi[kWfAcc], pj[kWfAcc];
  double acc[kWfAcc];
#pragma unroll
  for (int a = 0; a < kWfAcc; ++a) {
    acc[a] = 0.0;
    // pair q = (i, j), i <= j, enumerated row by row over the K + 1 columns
    int q = tid + a * kGramThreads, i = 0;
    if (q < npairs) {
      while (q >= ncol - i) { q -= ncol - i; ++i; }
      pi[a] = i; pj[a] = i + q;
    } else {
      pi[a] = pj[a] = -1;
    }
  }
  double sw = 0.0, swphi = 0.0, lo = INFINITY, hi = -INFINITY;  // of pixel slot tid (tid < kGramPix)
  const size_t chunk_end = (win.total + kGramPix - 1) / kGramPix;
  for (size_t chunk = win.first / kGramPix + blockIdx.x; chunk < chunk_end; chunk += gridDim.x) {
    int valid = 0;
    if (tid < kGramPix) {
      const size_t m = chunk * kGramPix + tid;
      int r = 0, c = 0;
      double rr = 0.0, rho = 2.0, x = 0.0, y = 0.0, ux = 0.0, uy = 0.0, I = 0.0;
      if (m >= win.first && m < win.total && !win.skips(m) && layout_unmap<BR, BC>(m, n, pitch, r, c)) {
        it.geometry(r, c, x, y, rr, rho);
        if (rho <= 1.0) {
          ux = (double)f[m].x; uy = (double)f[m].y;
          I = WfItem::intensity(ux, uy);
          valid = it.member(rho, I, m);
        }
      }
      if (valid) {
        double c1 = 1.0, s1 = 0.0;
        if (rr > 0.0) {
          c1 = (origin_y ? y : x) / rr;
          s1 = (origin_y ? x : y) / rr;
        }
        const double cr = c1 * co - s1 * so, sr = s1 * co + c1 * so;
        const double xj = 1.0 - 2.0 * rho * rho;
        double rho_pow = 1.0, cm = 1.0, sm = 0.0;
        const double* st = steps;
        for (int am = 0; am <= nmax; ++am) {
          const int kmax = (nmax - am) / 2;
          double pkm1 = 0.0, pk = 1.0;
          for (int k = 0; k <= kmax; ++k, st += kWfStep) {
            if (k > 0) {
              const double pn = (st[0] * xj + st[1]) * pk - st[2] * pkm1;
              pkm1 = pk;
              pk = pn;
            }
            const int jc = (int)st[3], js = (int)st[4];
            const double base = rho_pow * pk;
            if (jc >= 0) wbuf[jc * kGramRow + tid] = st[5] * base * cm;
            if (js >= 0) wbuf[js * kGramRow + tid] = st[6] * base * sm;
          }
          rho_pow *= rho;
          const double cn = cm * cr - sm * sr;
          sm = sm * cr + cm * sr;
          cm = cn;
        }
        const double re = __dadd_rn(__dmul_rn(ux, rx), __dmul_rn(uy, ry));
        const double im = __dsub_rn(__dmul_rn(uy, rx), __dmul_rn(ux, ry));
        const double phi = atan2(im, re);
        const double w = WEIGHTED ? I : 1.0;
        phirow[tid] = phi;
        if (WEIGHTED) wrow[tid] = w;
        sw += w;
        swphi += __dmul_rn(w, phi);
        lo = fmin(lo, phi);
        hi = fmax(hi, phi);
      } else {
        for (int j = 0; j <= K; ++j) wbuf[j * kGramRow + tid] = 0.0;
        if (WEIGHTED) wrow[tid] = 0.0;
      }
    }
    if (!__syncthreads_or(valid)) continue;  // (also publishes wbuf)
#pragma unroll
    for (int a = 0; a < kWfAcc; ++a) {
      if (pi[a] < 0) continue;
      const double* zi = wbuf + pi[a] * kGramRow;
      const double* zj = wbuf + pj[a] * kGramRow;
      // kLoad pixels at a time, their LDS reads issued before the first product: read and used pixel by pixel, every pair
      // of pixels waits out the whole LDS latency.  The additions keep their order.  With the row of weights the eight
      // pixels in flight cost a wave per SIMD (171 registers), which costs more than they gain: pixel by pixel there
      // (K = 36 at 4096^2 x 32: uniform 27.3 ms against 32.5, intensity 40.2 against 37.4; profiles/r22_wavefront_bench.md).
      constexpr int kLoad = WEIGHTED ? 1 : kWfLoad;
      double sum = 0.0;
      for (int px = 0; px < kGramPix; px += kLoad) {
        double vi[kLoad], vj[kLoad], vw[kLoad];
#pragma unroll
        for (int t = 0; t < kLoad; ++t) {
          vi[t] = zi[px + t];
          vj[t] = zj[px + t];
          if (WEIGHTED) vw[t] = wrow[px + t];
        }
#pragma unroll
        for (int t = 0; t < kLoad; ++t) sum += WEIGHTED ? (vw[t] * vi[t]) * vj[t] : vi[t] * vj[t];
      }
      acc[a] += sum;
    }
    __syncthreads();
  }
#pragma unroll
  for (int a = 0; a < kWfAcc; ++a)
    if (pi[a] >= 0) out[tid + a * kGramThreads] = acc[a];
  // the sums and extremes of the 128 pixel slots, in slot order (the launcher sizes the LDS for these four rows of 128 at least)
  __syncthreads();
  if (tid < kGramPix) {
    wbuf[tid] = sw;
    wbuf[kGramPix + tid] = swphi;
    wbuf[2 * kGramPix + tid] = lo;
    wbuf[3 * kGramPix + tid] = hi;
  }
  __syncthreads();
  if (tid < kWfExtra) {
    const double* v = wbuf + tid * kGramPix;
    double t = v[0];
    for (int k = 1; k < kGramPix; ++k) t = tid < 2 ? t + v[k] : (tid == 2 ? fmin(t, v[k]) : fmax(t, v[k]));
    out[npairs + tid] = t;
  }
}

// Launch 3: out[item][q] = sum over workgroups, in order; summary[item][5, 6, 8, 9] = phi_min, phi_max (0 for an empty
// Omega), sum w, sum w phi
static __global__ void wf_final_kernel(const double* partial, int nblocks, int npairs, double* sums, double* summary) {
  const int item = blockIdx.y;
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  const int nvals = npairs + kWfExtra;
  if (q >= nvals) return;
  const double* in = partial + (size_t)item * nblocks * nvals + q;
  double t = in[0];
  for (int b = 1; b < nblocks; ++b) {
    const double v = in[(size_t)b * nvals];
    t = q < npairs + 2 ? t + v : (q == npairs + 2 ? fmin(t, v) : fmax(t, v));
  }
  double* s = summary + (size_t)item * kWfSummary;
  if (q < npairs) sums[(size_t)item * npairs + q] = t;
  else if (q == npairs) s[8] = t;
  else if (q == npairs + 1) s[9] = t;
  else s[q == npairs + 2 ? 5 : 6] = isfinite(t) ? t : 0.0;
}

}  // namespace paos
