// item_window_main.cpp -- walks paos_amd/csrc/item_window.h on the host for tests/test_item_window_host.py (compiled with the
// address and undefined-behaviour sanitizers; no GPU, no library).  Commands (argv):
//   all                               every window of every layout (below); prints "N BR windows W" per layout and "ok",
//                                     or the first disagreement and exit status 1
//   walk N BR RLO RHI CLO CHI GRID    (a bound of -1: that axis is null) prints the slots of the filtered walk by GRID
//                                     workgroups (sorted), those of the dense walk (in order) and the pixels not outside
// What `all` holds every window to -- rows [lo, hi) and columns [lo, hi) rounded outward to whole blocks, the rule the
// zeroing kernel used to spell on (r, c):
//   * outside(r, c) is that rule;
//   * the filtered walk by 1, 3 and 1024 workgroups of 256 threads visits every non-padding slot that is not outside
//     exactly once, and nothing else;
//   * the dense walk visits the same slots exactly once; without columns it also visits the padding of its block rows
//     (the start stores zeros there), never a slot outside [first, total) or beyond the item.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../paos_amd/csrc/item_window.h"

using paos::ItemWindow;
using paos::layout_unmap;

constexpr int kPadBlocks = 3;           // PAOS_PAD_BLOCKS (host.h)
constexpr int kThreads = 256;           // kPwThreads (pointwise.h)
constexpr int kGrids[3] = {1, 3, 1024};  // 1024: the context's nparts
constexpr int kItem = 1;                // the windows of item 1: item 0's entries are never read

struct Bounds {
  int lo, hi;  // lo < 0: null
};

template <int BR, int BC>
struct Layout {
  int n;
  unsigned pitch, item_stride;
  explicit Layout(int n_) : n(n_), pitch((unsigned)n_ * BR + kPadBlocks * BR * BC), item_stride(pitch * (unsigned)(n_ / BR)) {}
};

struct Pixel {
  int r, c;  // of a slot; r < 0: pitch padding
};

// layout_unmap of every slot of an item, and that it is a bijection onto the n x n pixels
template <int BR, int BC>
bool unmap_all(const Layout<BR, BC>& l, std::vector<Pixel>& pixel) {
  std::vector<char> seen((size_t)l.n * l.n, 0);
  size_t pixels = 0;
  pixel.assign(l.item_stride, Pixel{-1, -1});
  for (size_t m = 0; m < l.item_stride; ++m) {
    int r, c;
    if (!layout_unmap<BR, BC>(m, l.n, l.pitch, r, c)) continue;
    if (r < 0 || r >= l.n || c < 0 || c >= l.n || seen[(size_t)r * l.n + c]++) return false;
    pixel[m] = {r, c};
    ++pixels;
  }
  return pixels == (size_t)l.n * l.n;
}

template <int BR, int BC>
ItemWindow<BR, BC> window(const Layout<BR, BC>& l, Bounds rows, Bounds cols, double* store) {
  // [2 items][2] per axis; item 0 holds values that would walk out of the item if they were read
  const double v[8] = {-1.0e9, 1.0e9, (double)rows.lo, (double)rows.hi, -1.0e9, 1.0e9, (double)cols.lo, (double)cols.hi};
  std::memcpy(store, v, sizeof v);
  return ItemWindow<BR, BC>(rows.lo < 0 ? nullptr : store, cols.lo < 0 ? nullptr : store + 4, kItem, l.n, l.pitch, l.item_stride);
}

// the rule, restated: bounds rounded outward to whole blocks
template <int BR, int BC>
struct Rule {
  int rlo, rhi, clo, chi;
  Rule(int n, Bounds rows, Bounds cols)
      : rlo(rows.lo < 0 ? 0 : rows.lo / BR * BR), rhi(rows.lo < 0 ? n : (rows.hi + BR - 1) / BR * BR),
        clo(cols.lo < 0 ? 0 : cols.lo / BC * BC), chi(cols.lo < 0 ? n : (cols.hi + BC - 1) / BC * BC) {}
  bool outside(int r, int c) const { return r < rlo || r >= rhi || c < clo || c >= chi; }
};

template <int BR, int BC, typename Visit>
void filtered_walk(const ItemWindow<BR, BC>& w, int grid, Visit&& visit) {
  const size_t step = (size_t)grid * kThreads;
  // (a thread at or beyond `total` has no slot: start() only moves a thread forward)
  for (size_t t = 0; t < step && t < w.total; ++t)
    for (size_t m = w.start(t, step); m < w.total; m += step)
      if (!w.skips(m)) visit(m);
}

static int fail(const char* what, int n, int br, Bounds rows, Bounds cols, size_t m) {
  std::printf("%s: n %d BR %d rows [%d, %d) cols [%d, %d) slot %zu\n", what, n, br, rows.lo, rows.hi, cols.lo, cols.hi, m);
  return 1;
}

// one window: every walk adds its own digit to count[m] (all zero before and after); returns 0 if all is as it should be
template <int BR, int BC>
int check(const Layout<BR, BC>& l, const std::vector<Pixel>& pixel, Bounds rows, Bounds cols, std::vector<unsigned>& count, bool whole_item) {
  double store[8];
  const ItemWindow<BR, BC> w = window(l, rows, cols, store);
  if (w.total > l.item_stride || w.first > w.total || w.first % l.pitch || w.total % l.pitch)
    return fail("range", l.n, BR, rows, cols, w.first);
  unsigned digit = 1;
  for (int grid : kGrids) {
    filtered_walk(w, grid, [&](size_t m) { count[m] += digit; });  // (m < total: the walk's own loop condition)
    digit <<= 4;
  }
  const size_t work = w.work();
  for (size_t j = 0; j < work; ++j) {
    const size_t m = w.element(j);
    if (m < w.first || m >= w.total) return fail("dense walk out of range", l.n, BR, rows, cols, m);
    count[m] += digit;
  }
  // No walk leaves [first, total) (the dense walk is held to it above, the filtered one by its loop), so the counts
  // outside are untouched; whole_item: outside() is held to the rule there too.
  const Rule<BR, BC> rule(l.n, rows, cols);
  for (size_t m = whole_item ? 0 : w.first; m < (whole_item ? l.item_stride : w.total); ++m) {
    const Pixel& p = pixel[m];
    const unsigned got = count[m];
    count[m] = 0;
    if (p.r < 0) {  // padding: the dense walk alone, once, and only without columns
      if (got != 0 && !(got == digit && cols.lo < 0)) return fail("padding visited", l.n, BR, rows, cols, m);
      continue;
    }
    const bool out = rule.outside(p.r, p.c);
    if (w.outside(p.r, p.c) != out) return fail("outside() is not the rule", l.n, BR, rows, cols, m);
    if (got != (out ? 0u : 0x1111u)) return fail("visits", l.n, BR, rows, cols, m);
  }
  return 0;
}

// every 0 <= lo < hi <= n, and null
static std::vector<Bounds> all_bounds(int n) {
  std::vector<Bounds> b{{-1, -1}};
  for (int lo = 0; lo < n; ++lo)
    for (int hi = lo + 1; hi <= n; ++hi) b.push_back({lo, hi});
  return b;
}

// Every row window (and null) with null columns; every column window (and null) with a short row window that moves and
// changes its length from one to the next (1 to 11 rows: one to four block rows); every sixteenth column window with null
// rows, the longest walk.  The two axes set different members of the window, so their full product would add no new
// arithmetic.  outside() is asked about the whole item at n = 16 and for every fourth window at n = 64, else about the
// block rows of the window.
template <int BR, int BC>
int check_layout(int n) {
  const Layout<BR, BC> l(n);
  std::vector<Pixel> pixel;
  if (!unmap_all(l, pixel)) return fail("layout_unmap is no bijection", n, BR, {-1, -1}, {-1, -1}, 0);
  const std::vector<Bounds> b = all_bounds(n);
  std::vector<unsigned> count(l.item_stride, 0u);
  size_t windows = 0;
  for (size_t i = 0; i < b.size(); ++i) {
    const bool whole = n <= 16 || i % 4 == 0;
    const int lo = (int)(i * 5 % (size_t)n), hi = lo + 1 + (int)(i % 11);
    if (check(l, pixel, b[i], {-1, -1}, count, whole) || check(l, pixel, {lo, hi < n ? hi : n}, b[i], count, whole)) return 1;
    windows += 2;
    if (i % 16 == 0) {
      if (check(l, pixel, {-1, -1}, b[i], count, true)) return 1;
      ++windows;
    }
  }
  std::printf("%d %d windows %zu\n", n, BR, windows);
  return 0;
}

template <int BR, int BC>
int walk(int n, Bounds rows, Bounds cols, int grid) {
  const Layout<BR, BC> l(n);
  double store[8];
  const ItemWindow<BR, BC> w = window(l, rows, cols, store);
  std::vector<char> seen(l.item_stride, 0);
  filtered_walk(w, grid, [&](size_t m) { seen[m] = 1; });
  std::printf("filtered");
  for (size_t m = 0; m < l.item_stride; ++m)
    if (seen[m]) std::printf(" %zu", m);
  std::printf("\ndense");
  for (size_t j = 0; j < w.work(); ++j) std::printf(" %zu", w.element(j));
  std::printf("\ninside");
  for (int r = 0; r < n; ++r)
    for (int c = 0; c < n; ++c)
      if (!w.outside(r, c)) std::printf(" %d,%d", r, c);
  std::printf("\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !std::strcmp(argv[1], "all")) {
    for (int n : {16, 64})
      if (check_layout<4, 2>(n) || check_layout<8, 2>(n)) return 1;
    std::printf("ok\n");
    return 0;
  }
  if (argc == 9 && !std::strcmp(argv[1], "walk")) {
    const int n = std::atoi(argv[2]), br = std::atoi(argv[3]), grid = std::atoi(argv[8]);
    const Bounds rows{std::atoi(argv[4]), std::atoi(argv[5])}, cols{std::atoi(argv[6]), std::atoi(argv[7])};
    if (br == 4) return walk<4, 2>(n, rows, cols, grid);
    if (br == 8) return walk<8, 2>(n, rows, cols, grid);
  }
  std::fprintf(stderr, "usage: item_window_main all | walk N BR RLO RHI CLO CHI GRID\n");
  return 2;
}
