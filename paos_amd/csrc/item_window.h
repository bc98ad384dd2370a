// item_window.h -- the blocked layout of one item and the window of it a lean step works on: which memory slot holds which
// pixel (layout_unmap), and the rows x columns box -- rounded outward to whole blocks -- that the start writes, the power
// sum reads and the zeroing spares.  One description, so that the three agree on the set of elements.  Index arithmetic
// only: it compiles as plain C++ too, so that a host program can walk it (tests/item_window_main.cpp).
#pragma once
#include <cstddef>

#if defined(__HIPCC__)
#define PAOS_WINDOW_FN __host__ __device__ __forceinline__
#else
#define PAOS_WINDOW_FN inline
#endif

namespace paos {

// memory index (inside one item) -> (row, col); false for pitch-padding slots
template <int BR, int BC>
PAOS_WINDOW_FN bool layout_unmap(size_t m, int n, unsigned pitch, int& row, int& col) {
  const unsigned brow = (unsigned)(m / pitch), rem = (unsigned)(m % pitch);
  if (rem >= (unsigned)n * BR) return false;
  const unsigned in = rem % (BR * BC);
  row = (int)(brow * BR + in / BC);
  col = (int)((rem / (BR * BC)) * BC + in % BC);
  return true;
}

// ``rows`` / ``cols`` (optional, [batch][2] each): the rows and columns [lo, hi) of item `item`; null = all of them.
// Block rows are contiguous in memory, so the rows are the range [first, total) of the item's slots; inside every block
// row the columns are the element offsets [in_lo, in_hi), which never reach the pitch padding behind n BR.
template <int BR, int BC>
struct ItemWindow {
  size_t first, total;
  unsigned in_lo, in_hi, pitch;
  bool windowed;  // columns were given: the dense walk covers the window of every block row, else whole block rows

  PAOS_WINDOW_FN ItemWindow(const double* rows, const double* cols, int item, int n, unsigned pitch_, unsigned item_stride)
      : first(0), total(item_stride), in_lo(0), in_hi((unsigned)n * BR), pitch(pitch_), windowed(cols != nullptr) {
    // (the columns first: in this order the fused start kernel keeps the scalar registers it had before the window was shared)
    if (cols) {
      in_lo = (unsigned)((int)cols[2 * item] / BC) * (BR * BC);
      const unsigned h = (unsigned)(((int)cols[2 * item + 1] + BC - 1) / BC) * (BR * BC);
      in_hi = h < in_hi ? h : in_hi;
    }
    if (rows) {
      first = (size_t)((int)rows[2 * item] / BR) * pitch;
      total = (size_t)(((int)rows[2 * item + 1] + BR - 1) / BR) * pitch;
      if (total > item_stride) total = item_stride;
    }
  }

  // The filtered walk (the summing kernels: it fixes the order of additions).  Thread `m` of `step` keeps the slots
  // m, m + step, ... it would have on the whole item -- those of [first, total) -- and skips the padding and what lies
  // outside the columns:   for (m = start(m, step); m < total; m += step) if (!skips(m)) ...
  PAOS_WINDOW_FN size_t start(size_t m, size_t step) const {
    if (m < first) m += (first - m + step - 1) / step * step;
    return m;
  }
  PAOS_WINDOW_FN bool skips(size_t m) const {
    const unsigned off = (unsigned)(m % pitch);
    return off >= in_hi || off < in_lo;
  }

  // The dense walk (the writing kernels): element(j), j < work(), are the slots of the window, each once.  Without
  // columns these are whole block rows, padding included (the start stores zeros there).
  PAOS_WINDOW_FN unsigned span() const { return in_hi > in_lo ? in_hi - in_lo : 0; }
  PAOS_WINDOW_FN size_t work() const { return windowed ? (total - first) / pitch * span() : total - first; }
  PAOS_WINDOW_FN size_t element(size_t j) const {
    const unsigned s = span();
    return windowed ? first + (j / s) * pitch + in_lo + (j % s) : first + j;
  }

  // pixel (r, c) lies outside the window (what the zeroing clears)
  PAOS_WINDOW_FN bool outside(int r, int c) const {
    const size_t brow = (size_t)(r / BR) * pitch;
    const unsigned off = (unsigned)(c / BC) * (BR * BC);
    return brow < first || brow >= total || off < in_lo || off >= in_hi;
  }
};

}  // namespace paos
