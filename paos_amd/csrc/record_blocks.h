// record_blocks.h -- what the block renderer of ellipse line records (pointwise.h: mask_blocks_kernel) decides without the
// exact overlap: the class of a window pixel from the squared quotients of its edges, and where the undecided pixels of a
// block's lines go in the wave's list.  Comparisons, sums and index arithmetic only: it compiles as plain C++ too, so that
// a host program can run it (tests/record_blocks_main.cpp).  Every translation unit that uses it is compiled without FMA
// contraction: the sums below are ellipse_pixel's, rounding by rounding.
#pragma once

#if defined(__HIPCC__)
#define PAOS_BLOCK_FN __host__ __device__ __forceinline__
#else
#define PAOS_BLOCK_FN inline
#endif

namespace paos {

enum : int { kPixelOut = 0, kPixelIn = 1, kPixelUndecided = 2 };

// (offset / semi-axis)^2, the term of x'^2 + y'^2 that an edge of a pixel contributes: ellipse_pixel's quotient at
// theta = 0 (x * 1 + y * 0 = x) and its square.  A pixel's upper edge is its neighbour's lower edge, (k + 1) - 0.5 and
// k + 0.5 being one double: a window of W pixels has W + 1 of these.
PAOS_BLOCK_FN double edge_square(double offset, double semi_axis) {
  const double u = offset / semi_axis;
  return u * u;
}

// The class of one pixel inside the bounding box.  lo_a <= hi_a: the offsets of its two edges along the line from the
// centre, uu_lo / uu_hi their edge_square; lo_c, hi_c, vv_lo, vv_hi: the same across the line (per line).
//   in:   the four corner sums are <= 1.0 -- ellipse_pixel's own first test, which returns 1.0;
//   out:  the point of the pixel nearest the centre lies outside by the margin of the scan's chunk test
//         (mask_line_render, chunk == 2): the pixel neither touches the ellipse nor holds its centre, ellipse_pixel returns 0.0;
//   undecided: anything else -- the caller evaluates the exact overlap.
// (IEEE addition commutes bit for bit, so one order of the two terms serves both axes.)
PAOS_BLOCK_FN int pixel_class(double lo_a, double hi_a, double uu_lo, double uu_hi, double lo_c, double hi_c, double vv_lo, double vv_hi) {
  if (uu_lo + vv_lo <= 1.0 && uu_hi + vv_lo <= 1.0 && uu_lo + vv_hi <= 1.0 && uu_hi + vv_hi <= 1.0) return kPixelIn;
  const double nu = lo_a > 0.0 ? uu_lo : (hi_a < 0.0 ? uu_hi : 0.0);
  const double nv = lo_c > 0.0 ? vv_lo : (hi_c < 0.0 ? vv_hi : 0.0);
  return nu + nv > 1.0 + 1.0e-9 ? kPixelOut : kPixelUndecided;
}

// The W pixels [w0, w0 + W) of a line's window: bit k of `in` / `undecided` = pixel w0 + k is in / undecided.
// centre, semi_axis: along the line.  W <= 32.
PAOS_BLOCK_FN void window_classes(int w0, int W, double centre, double semi_axis, double lo_c, double hi_c, double vv_lo, double vv_hi,
                                  unsigned& in, unsigned& undecided) {
  in = undecided = 0u;
  double lo_a = ((double)w0 - 0.5) - centre, uu_lo = edge_square(lo_a, semi_axis);
  for (int k = 0; k < W; ++k) {
    const double hi_a = ((double)(w0 + k) + 0.5) - centre, uu_hi = edge_square(hi_a, semi_axis);
    const int cls = pixel_class(lo_a, hi_a, uu_lo, uu_hi, lo_c, hi_c, vv_lo, vv_hi);
    in |= (cls == kPixelIn ? 1u : 0u) << k;
    undecided |= (cls == kPixelUndecided ? 1u : 0u) << k;
    lo_a = hi_a; uu_lo = uu_hi;
  }
}

// ---- the wave's list of undecided pixels ------------------------------------------------------------------------
// Line i of the block (0 <= i < lines <= 64) has counts[i] undecided pixels (0 for a line that fits no window or lies
// outside the box); they go to the entries [offset, offset + counts[i]) with offset the exclusive prefix sum of the counts.
// A line whose entries would end behind the capacity is handed to the per-line renderers, and so is every line with
// entries behind it (the offsets only grow); `total`, the largest prefix sum within the capacity, is where the kept entries end.
constexpr int kBlockListCap = 1024;  // entries per wave: 8 bytes each, an entry's code first and its weight afterwards

PAOS_BLOCK_FN void list_layout(const int* counts, int lines, int line, int& offset, int& total) {
  int run = 0;
  offset = total = 0;
  for (int i = 0; i < lines; ++i) {
    if (i == line) offset = run;
    run += counts[i];
    if (run <= kBlockListCap) total = run;
  }
}
PAOS_BLOCK_FN bool list_keeps(int offset, int count) { return offset + count <= kBlockListCap; }

// an entry before its evaluation: which line of the block, which pixel of its two windows (< 64 each)
PAOS_BLOCK_FN unsigned long long list_entry(int line, int pixel) { return ((unsigned long long)line << 6) | (unsigned long long)pixel; }
PAOS_BLOCK_FN int entry_line(unsigned long long e) { return (int)(e >> 6); }
PAOS_BLOCK_FN int entry_pixel(unsigned long long e) { return (int)(e & 63ull); }

// Lane `line` writes its entries: one per set bit of `undecided` (bit k = pixel k of the line's 2 W window pixels), in
// ascending order, at list[offset ...] -- nothing unless the line is kept.  Returns the number written.
PAOS_BLOCK_FN int list_write(unsigned long long* list, int line, int offset, unsigned long long undecided) {
  const int count = __builtin_popcountll(undecided);
  if (!list_keeps(offset, count)) return 0;
  int at = offset;
  for (unsigned long long m = undecided; m; m &= m - 1) list[at++] = list_entry(line, __builtin_ctzll(m));
  return count;
}

}  // namespace paos
