// focus_pass.h -- the out-of-place passes of a through-focus stack (paos_focus_begin / paos_focus_plane).
//
// Every pass of fft_kernels.h works in place on the context's one field buffer.  A focus stack needs the forward
// spectrum of the last-surface field ONCE and an inverse transform per defocus plane, so the spectrum lives in a
// buffer of its own (same blocked layout, same pitch) and two of the four passes read one buffer and write the other:
//
//   begin:  rows[FFT]             field    -> spectrum     (the field is only read)
//           cols[FFT]             spectrum -> spectrum
//   plane:  cols[H 1/N | IFFT]    spectrum -> field        (the spectrum is only read)
//           rows[IFFT | 1/N]      field    -> field
//
// which is WFO.ptp (wfo.py:462-472) cut behind its forward 2-D transform: the same line transforms (fft_core.h), the
// same operators in the same order as the generic in-place ptp program  rows[FFT], cols[FFT | mid H 1/N | IFFT],
// rows[IFFT | mid 1/N]  (fft_kernels.h), hence the same roundings.  A tile is the generic kernel's tile (TileMap);
// tiles are disjoint in source and destination alike, so reading one buffer and writing the other needs no ordering
// beyond the stream's.
#pragma once
#include "fft_kernels.h"

namespace paos {

enum : int { FOCUS_FORWARD = 0,   // v = FFT(v)
             FOCUS_TRANSFER = 1,  // v = IFFT(1/N H v), H from the item's [enable, sx, sy, coef, sgn] block (natural order)
             FOCUS_INVERSE = 2 }; // v = 1/N IFFT(v)

struct FocusArgs {
  const void* src;        // batch of fields or spectra, complex<T>, blocked layout
  void* dst;              // the same layout; may be `src` (tiles are read whole before they are written)
  const void* tw;         // exp(-2 pi i m / N), m < N, complex<T>
  const double* params;   // FOCUS_TRANSFER: [item][FP_STRIDE]; enable = 0: H = 1 for that item
  double scale;           // the ortho factor 1/N of the inverse modes
  int mode;
  unsigned pitch;         // elements between block rows of the layout
  unsigned item_stride;   // elements between batch items
};

template <typename T, int N, int E, int LINES, int TILES, int AXIS, int BR, int BC, bool SPLIT, int MINW>
__global__ void __launch_bounds__(TILES* LINES* N / E, MINW)
    focus_pass_kernel(FocusArgs a) {
  const int item = blockIdx.y;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const TileMap<N, E, LINES, TILES, AXIS, BR, BC> m(blockIdx.x, threadIdx.x, a.pitch);
  const cx<T>* s = reinterpret_cast<const cx<T>*>(a.src) + (size_t)item * a.item_stride;  // wave-uniform
  cx<T>* d = reinterpret_cast<cx<T>*>(a.dst) + (size_t)item * a.item_stride;
  void* lds = smem + (size_t)m.lds_line * line_lds_bytes<T, N, SPLIT>();
  const cx<T>* tw = reinterpret_cast<const cx<T>*>(a.tw);

  cx<T> v[E];
#pragma unroll
  for (int k = 0; k < E; ++k) v[k] = s[m.base + (unsigned)k * m.stride];

  if (a.mode == FOCUS_TRANSFER) {
    const double* p = a.params + (size_t)item * FP_STRIDE;
    if (p[FP_ENABLE] != 0.0) {
      const PwOp h = {PWK_QPHASE_N, 0, 0};
#pragma unroll
      for (int k = 0; k < E; ++k) v[k] = apply_pw<T, 0>(v[k], h, p, m.row(k), m.col(k), N, nullptr, nullptr);
    }
#pragma unroll
    for (int k = 0; k < E; ++k) v[k] = {(T)__dmul_rn((double)v[k].x, a.scale), (T)__dmul_rn((double)v[k].y, a.scale)};
  }
  line_fft<T, N, E, SPLIT, 0>(v, lds, m.t, tw, a.mode != FOCUS_FORWARD);
  if (a.mode == FOCUS_INVERSE) {
#pragma unroll
    for (int k = 0; k < E; ++k) v[k] = {(T)__dmul_rn((double)v[k].x, a.scale), (T)__dmul_rn((double)v[k].y, a.scale)};
  }
#pragma unroll
  for (int k = 0; k < E; ++k) d[m.base + (unsigned)k * m.stride] = v[k];
}

}  // namespace paos
