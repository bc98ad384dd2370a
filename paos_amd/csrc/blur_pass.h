// blur_pass.h -- blurred PSFs (paos_blur_apply): a separable, real, even transfer function multiplied onto the spectrum
// paos_otf_compute left, and the way back to a REAL image -- the mirror of otf_pass.h.  README.md, "Blurred PSFs".
//
// The spectrum buffer holds  S'[ky][kx] = (-1)^(ky + kx) F[ky][kx],  F = fft2(P), for the columns kx <= N/2 (otf_pass.h).
// With  T[ky][kx] = ty[min(ky, N - ky)] tx[min(kx, N - kx)]  the blurred PSF is  P' = ifft2(T F).  T F is Hermitian like
// F, so again half of a complex inverse transform is redundant, and the two passes run about N line transforms per item:
//
//   cols:  column k <= N/2 loads S'[.][k], multiplies by  g = fl(tx[k] ty[min(ky, N - ky)])  (rounded to float in an fp32
//          context; real and imaginary part times g once each; g = 1 at zero frequency) and stores the product back to
//          its own column -- the buffer then holds the SYSTEM spectrum, which paos_otf_fetch / paos_otf_cuts hand out
//          as before.  It takes the checkerboard sign off, transforms along ky (inverse) to  G[r][k], the row transform
//          of the rows r of N P', and re-tangles row pairs: with  Z_p[c] = G[2p][c] + i G[2p+1][c]
//              (P[2p][k],     P[2p+1][k])     = (Re, Im) Z_p[k]     = (G[2p].x - G[2p+1].y, G[2p].y + G[2p+1].x)
//              (P[2p][N - k], P[2p+1][N - k]) = (Re, Im) Z_p[N - k] = (G[2p].x + G[2p+1].y, G[2p+1].x - G[2p].y)
//          since G[r][N - k] = conj G[r][k].  The columns 0 and N/2 mirror onto themselves; there G is real in exact
//          arithmetic and the real parts are taken.  Rows 2p and 2p+1 of a column sit in the lanes l and l ^ 2 of one
//          wave (TileMap: PAR = 2 columns, then the rows of a block), so each thread needs its partner's imaginary
//          part and nothing else: one quad permute per element, no trip through LDS.     buffer -> buffer and PSF
//   rows:  line p < N/2 loads  (P[2p][c], P[2p+1][c])  as one complex line -- the packing otf_row_kernel loads --
//          transforms it along c (inverse), scales by 1/N^2 (exact) and stores Re to row 2p, Im to row 2p+1.
//                                                                                              PSF -> PSF, in place
//
// Hazards.  The spectrum and the PSF buffer are distinct allocations.  A column tile reads and writes the spectrum in
// its own columns only (every thread the elements it loaded itself), and writes the PSF in its own columns k and their
// mirrors N - k: k <= N/2 <= N - k, and two columns <= N/2 have different mirrors, so no two tiles write one element and
// nothing reads the PSF during that launch.  A row tile reads and writes rows 2p, 2p+1 of its own lines, every thread
// the elements it loaded itself.  Lines of the last column workgroup beyond N/2 load nothing and store nothing (they
// still run the transform's barriers).  The row launch follows the column launch on the context's stream.
#pragma once
#include "fft_kernels.h"

namespace paos {

struct BlurArgs {
  double* psf;            // the kept PSFs: doubles in the field's blocked layout
  void* spec;             // the spectrum buffer of paos_otf_compute, complex<T>, the same layout
  const void* tw;         // exp(-2 pi i m / N), m < N, complex<T>
  const double* tabs;     // [item][2][N/2 + 1]: tx, ty of paos_blur_table
  double scale;           // 1 / N^2
  unsigned pitch;         // elements between block rows of the layout
  unsigned item_stride;   // elements between batch items
};

// the value of lane l ^ 2 (the same quad): a DPP quad permute [2, 3, 0, 1] per 32-bit half
__device__ __forceinline__ float lane_xor2(float v) {
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x4E, 0xF, 0xF, true));
}
__device__ __forceinline__ double lane_xor2(double v) {
  const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), 0x4E, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), 0x4E, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}

// a column tile of the generic pass kernel, over the columns 0 .. N/2 rounded up to whole workgroups
template <typename T, int N, int E, int LINES, int TILES, int BR, int BC, bool SPLIT, int MINW>
__global__ void __launch_bounds__(TILES* LINES* N / E, MINW)
    blur_col_kernel(BlurArgs a) {
  static_assert((N / 2) % (LINES * TILES) == 0, "the workgroup behind column N/2 ends at or before column N");
  static_assert((N / E) % 2 == 0, "a thread's rows share their parity");
  static_assert(LINES == 2 && BR % 2 == 0 && (LINES * (N / E)) % 4 == 0, "rows t and t ^ 1 of a column sit in lanes l and l ^ 2 of a quad");
  const int item = blockIdx.y;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const TileMap<N, E, LINES, TILES, 1, BR, BC> m(blockIdx.x, threadIdx.x, a.pitch);
  cx<T>* f = reinterpret_cast<cx<T>*>(a.spec) + (size_t)item * a.item_stride;  // wave-uniform
  double* psf = a.psf + (size_t)item * a.item_stride;
  void* lds = smem + (size_t)m.lds_line * line_lds_bytes<T, N, SPLIT>();
  const cx<T>* tw = reinterpret_cast<const cx<T>*>(a.tw);
  const double* tx = a.tabs + (size_t)item * 2 * (N / 2 + 1);
  const double* ty = tx + (N / 2 + 1);
  const int col = m.col0 + m.line;        // < N (static_assert above)
  const bool live = col <= N / 2;
  const bool self = col == 0 || col == N / 2;
  const bool odd = (m.t & 1) != 0;        // rows t + k TL: PSF rows 2p+1 (odd) or 2p (even)

  cx<T> v[E];
#pragma unroll
  for (int k = 0; k < E; ++k) v[k] = {(T)0, (T)0};
  if (live) {
    const double gx = tx[col];
#pragma unroll
    for (int k = 0; k < E; ++k) {
      const int row = m.row(k);
      const T g = (T)__dmul_rn(gx, ty[row <= N / 2 ? row : N - row]);
      const cx<T> s = f[m.base + (unsigned)k * m.stride];
      const cx<T> p = {s.x * g, s.y * g};
      f[m.base + (unsigned)k * m.stride] = p;  // the system spectrum, sign and all
      v[k] = ((row + col) & 1) ? cx<T>{-p.x, -p.y} : p;
    }
  }
  line_fft<T, N, E, SPLIT, 0>(v, lds, m.t, tw, true);
  const unsigned mbase = (unsigned)layout_index<BR, BC>(m.t, (N - col) & (N - 1), a.pitch);
#pragma unroll
  for (int k = 0; k < E; ++k) {
    const T oy = lane_xor2(v[k].y);  // (every lane of the wave takes part: dead lines hold zeros)
    if (live) {
      if (self) {
        psf[m.base + (unsigned)k * m.stride] = (double)v[k].x;
      } else {
        psf[m.base + (unsigned)k * m.stride] = (double)(odd ? v[k].x + oy : v[k].x - oy);
        psf[mbase + (unsigned)k * m.stride] = (double)(odd ? v[k].x - oy : v[k].x + oy);
      }
    }
  }
}

// a row tile of the generic pass kernel, over the N/2 packed lines, in place on the PSF buffer
template <typename T, int N, int E, int LINES, int TILES, int BR, int BC, bool SPLIT, int MINW>
__global__ void __launch_bounds__(TILES* LINES* N / E, MINW)
    blur_row_kernel(BlurArgs a) {
  static_assert(BR % 2 == 0, "PSF rows 2p and 2p+1 share a block");
  static_assert((N / 2) % (LINES * TILES) == 0, "whole workgroups cover the N/2 packed lines");
  const int item = blockIdx.y;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const TileMap<N, E, LINES, TILES, 0, BR, BC> m(blockIdx.x, threadIdx.x, a.pitch);
  double* s = a.psf + (size_t)item * a.item_stride;  // wave-uniform
  void* lds = smem + (size_t)m.lds_line * line_lds_bytes<T, N, SPLIT>();
  const cx<T>* tw = reinterpret_cast<const cx<T>*>(a.tw);
  const unsigned src = (unsigned)layout_index<BR, BC>(2 * (m.row0 + m.line), m.t, a.pitch);  // row 2p; row 2p+1 is BC further
  const T scale = (T)a.scale;

  cx<T> v[E];
#pragma unroll
  for (int k = 0; k < E; ++k) v[k] = {(T)s[src + (unsigned)k * m.stride], (T)s[src + BC + (unsigned)k * m.stride]};
  line_fft<T, N, E, SPLIT, 0>(v, lds, m.t, tw, true);
#pragma unroll
  for (int k = 0; k < E; ++k) {
    s[src + (unsigned)k * m.stride] = (double)(v[k].x * scale);
    s[src + BC + (unsigned)k * m.stride] = (double)(v[k].y * scale);
  }
}

}  // namespace paos
