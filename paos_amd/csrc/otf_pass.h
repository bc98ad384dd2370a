// otf_pass.h -- the 2-D transform of a REAL image: the kept PSFs to their spectra (paos_otf_compute), and the pointwise
// kernels that hand out OTF / MTF (paos_otf_fetch, paos_otf_cuts).  README.md, "Transfer functions".
//
// A PSF is real, so its spectrum is Hermitian, F[(N - ky) % N][(N - kx) % N] = conj F[ky][kx], and half of the work of a
// complex 2-D transform is redundant.  The two passes here run about N line transforms per item instead of 2 N:
//
//   rows:  line p < N/2 loads  z_p[c] = P[2p][c] + i P[2p+1][c]  (two rows of the PSF packed into one complex line),
//          transforms it along c and stores  Z_p  as row p of the spectrum buffer          PSF -> buffer, N/2 lines
//   cols:  column k <= N/2 untangles the two rows while it loads -- with  M = conj Z_p[(N - k) % N]
//              row 2p   of column k = (Z_p[k] + M) / 2          (the transform of PSF row 2p   at column k)
//              row 2p+1 of column k = (Z_p[k] - M) / (2 i)      (the transform of PSF row 2p+1 at column k)
//          -- transforms along the rows, multiplies by the checkerboard sign (-1)^(ky + kx) that stands for the
//          centred coordinates (fft_kernels.h: PWK_SIGN) and stores the column             buffer -> buffer, in place
//
// In place: a column tile reads rows < N/2 of its own columns and of their mirror columns, and writes its own columns.
// Only columns <= N/2 are written, and the mirror columns of those are > N/2 (or the column itself, for 0 and N/2), so no
// tile writes what another one reads; inside a workgroup every load precedes the first barrier of the transform and
// every store follows it.  Lines of the last workgroup that lie beyond column N/2 load nothing and store nothing.
// Afterwards columns 0 .. N/2 of the buffer hold  S'[ky][kx] = (-1)^(ky + kx) F[ky][kx]  in unshifted indices; the
// other half is its conjugate mirror and is never formed in memory (otf_value).
#pragma once
#include "fft_kernels.h"

namespace paos {

struct OtfArgs {
  const double* psf;      // the kept PSFs: doubles in the field's blocked layout
  void* spec;             // the spectrum buffer, complex<T>, the same layout
  const void* tw;         // exp(-2 pi i m / N), m < N, complex<T>
  unsigned pitch;         // elements between block rows of the layout
  unsigned item_stride;   // elements between batch items
};

// a row tile of the generic pass kernel (TileMap), over the N/2 packed lines
template <typename T, int N, int E, int LINES, int TILES, int BR, int BC, bool SPLIT, int MINW>
__global__ void __launch_bounds__(TILES* LINES* N / E, MINW)
    otf_row_kernel(OtfArgs a) {
  static_assert(BR % 2 == 0, "PSF rows 2p and 2p+1 share a block");
  static_assert((N / 2) % (LINES * TILES) == 0, "whole workgroups cover the N/2 packed lines");
  const int item = blockIdx.y;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const TileMap<N, E, LINES, TILES, 0, BR, BC> m(blockIdx.x, threadIdx.x, a.pitch);
  const double* s = a.psf + (size_t)item * a.item_stride;  // wave-uniform
  cx<T>* d = reinterpret_cast<cx<T>*>(a.spec) + (size_t)item * a.item_stride;
  void* lds = smem + (size_t)m.lds_line * line_lds_bytes<T, N, SPLIT>();
  const cx<T>* tw = reinterpret_cast<const cx<T>*>(a.tw);
  const unsigned src = (unsigned)layout_index<BR, BC>(2 * (m.row0 + m.line), m.t, a.pitch);  // row 2p; row 2p+1 is BC further

  cx<T> v[E];
#pragma unroll
  for (int k = 0; k < E; ++k) v[k] = {(T)s[src + (unsigned)k * m.stride], (T)s[src + BC + (unsigned)k * m.stride]};
  line_fft<T, N, E, SPLIT, 0>(v, lds, m.t, tw, false);
#pragma unroll
  for (int k = 0; k < E; ++k) d[m.base + (unsigned)k * m.stride] = v[k];
}

// a column tile of the generic pass kernel, over the columns 0 .. N/2 rounded up to whole workgroups
template <typename T, int N, int E, int LINES, int TILES, int BR, int BC, bool SPLIT, int MINW>
__global__ void __launch_bounds__(TILES* LINES* N / E, MINW)
    otf_col_kernel(OtfArgs a) {
  static_assert((N / 2) % (LINES * TILES) == 0, "the workgroup behind column N/2 ends at or before column N");
  static_assert((N / E) % 2 == 0, "a thread's rows share their parity");
  const int item = blockIdx.y;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const TileMap<N, E, LINES, TILES, 1, BR, BC> m(blockIdx.x, threadIdx.x, a.pitch);
  cx<T>* f = reinterpret_cast<cx<T>*>(a.spec) + (size_t)item * a.item_stride;  // wave-uniform
  void* lds = smem + (size_t)m.lds_line * line_lds_bytes<T, N, SPLIT>();
  const cx<T>* tw = reinterpret_cast<const cx<T>*>(a.tw);
  constexpr int TL = N / E;
  const int col = m.col0 + m.line;        // < N (static_assert above)
  const bool live = col <= N / 2;
  const int mir = (N - col) & (N - 1);
  const bool odd = (m.t & 1) != 0;        // rows t + k TL: PSF rows 2p+1 (odd) or 2p (even) of the packed lines p
  const T half = (T)0.5;

  cx<T> v[E];
#pragma unroll
  for (int k = 0; k < E; ++k) {
    v[k] = {(T)0, (T)0};
    if (live) {
      const int p = (m.t >> 1) + k * (TL / 2);
      const cx<T> z = f[layout_index<BR, BC>(p, col, a.pitch)];
      const cx<T> w = f[layout_index<BR, BC>(p, mir, a.pitch)];
      // (z + conj w) / 2  or  (z - conj w) / (2 i); the halving is exact
      v[k] = odd ? cx<T>{(z.y + w.y) * half, (w.x - z.x) * half} : cx<T>{(z.x + w.x) * half, (z.y - w.y) * half};
    }
  }
  line_fft<T, N, E, SPLIT, 0>(v, lds, m.t, tw, false);
  if (live) {
#pragma unroll
    for (int k = 0; k < E; ++k) {
      const bool neg = ((m.row(k) + col) & 1) != 0;
      f[m.base + (unsigned)k * m.stride] = neg ? cx<T>{-v[k].x, -v[k].y} : v[k];
    }
  }
}

// ---- pointwise: what the spectrum buffer stands for -------------------------------------------------------------------
// OTF at the UNSHIFTED index (ky, kx) of one item.  Columns 0 .. N/2 are in memory; the others are conjugate mirrors.
// The columns 0 and N/2 mirror onto themselves: their rows > N/2 are taken from the rows < N/2 as well, and the four
// points that are their own mirrors get an imaginary part of exactly zero -- so what is handed out is Hermitian bit for
// bit, whatever the rounding of the transforms.  Zero frequency is (dc != 0 ? 1 : 0) + 0 i by definition (dc times the
// rounded reciprocal of dc need not be 1).
template <typename T, int BR, int BC>
__device__ __forceinline__ cx<double> otf_value(const cx<T>* spec, int ky, int kx, int n, unsigned pitch, double dc, double scale) {
  const int h = n / 2;
  const bool selfx = kx == 0 || kx == h, selfy = ky == 0 || ky == h;
  const bool mirror = kx > h || (selfx && ky > h);
  const int ry = mirror ? (n - ky) & (n - 1) : ky, rx = mirror ? (n - kx) & (n - 1) : kx;
  if (ry == 0 && rx == 0) return {dc != 0.0 ? 1.0 : 0.0, 0.0};
  const cx<T> s = spec[layout_index<BR, BC>(ry, rx, pitch)];
  const double x = __dmul_rn((double)s.x, scale), y = __dmul_rn((double)s.y, scale);
  if (selfx && selfy) return {x, 0.0};
  return {x, mirror ? -y : y};
}

__device__ __forceinline__ double otf_scale(double dc) { return dc != 0.0 ? 1.0 / dc : 0.0; }

// one item, centred (zero frequency at pixel [N/2][N/2]), row-major: N x N doubles (complex = 0) or complex128
template <typename T, int BR, int BC>
__global__ void otf_fetch_kernel(const cx<T>* spec, void* out, int n, unsigned pitch, int complex_out) {
  const double dc = (double)spec[0].x;
  const double scale = otf_scale(dc);
  const size_t total = (size_t)n * n;
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int ky = (int)(i / n), kx = (int)(i % n);
    const cx<double> v = otf_value<T, BR, BC>(spec, (ky + n / 2) & (n - 1), (kx + n / 2) & (n - 1), n, pitch, dc, scale);
    if (complex_out) reinterpret_cast<cx<double>*>(out)[i] = v;
    else reinterpret_cast<double*>(out)[i] = hypot(v.x, v.y);
  }
}

// every item: |OTF| along fy = 0, fx >= 0 and along fx = 0, fy >= 0, zero frequency to Nyquist: out[item][2][N/2 + 1]
template <typename T, int BR, int BC>
__global__ void otf_cuts_kernel(const cx<T>* spec_all, double* out, int n, unsigned pitch, unsigned item_stride) {
  const int item = blockIdx.y;
  const cx<T>* spec = spec_all + (size_t)item * item_stride;
  const int len = n / 2 + 1;
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= 2 * len) return;
  const double dc = (double)spec[0].x;
  const int along_y = j / len, q = j % len;
  const cx<double> v = otf_value<T, BR, BC>(spec, along_y ? q : 0, along_y ? 0 : q, n, pitch, dc, otf_scale(dc));
  out[(size_t)item * 2 * len + j] = hypot(v.x, v.y);
}

}  // namespace paos
