// The host side of tests/test_record_blocks_host.py: paos_amd/csrc/record_blocks.h -- the pixel classes and the list layout
// of the block renderer of ellipse line records -- compiled as plain C++ with the sanitizers and driven from stdin.
//
//   ellipse n axis xc yc a b     (doubles as C hex floats) for every line of the bounding box inside the grid:
//                                "L line W wl0 wr0 classes" -- the window width that fits (0: none, the line is handed
//                                over), the two window starts and one letter per window pixel, left window first:
//                                i = in (mask 1.0), o = out (mask 0.0), u = undecided
//   layout c0 c1 ...             per-line counts of undecided pixels (at most 64 lines, at most 64 each):
//                                "offsets ...", "kept ...", "total T", "used U" (entries written: the highest index + 1)
//                                and "guard ok" (nothing written behind the capacity, every entry where its line's
//                                offset says, in ascending pixel order)
//
// window_fit below restates pointwise.h's in plain doubles (that one needs the device compiler); the classes and the layout
// are the header's own functions, the ones the kernel calls.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../paos_amd/csrc/record_blocks.h"

namespace {

struct Geom {
  double xc, yc, a, b;
  int ixmin, ixmax, iymin, iymax;
  int lo(int axis) const { return axis == 0 ? ixmin : iymin; }
  int hi(int axis) const { return axis == 0 ? ixmax : iymax; }
  double sum2(int axis, double al, double ac) const {
    const double u = al / (axis == 0 ? a : b), v = ac / (axis == 0 ? b : a);
    return axis == 0 ? u * u + v * v : v * v + u * u;
  }
};

Geom make_geom(double xc, double yc, double a, double b) {
  Geom g{xc, yc, a, b, 0, 0, 0, 0};
  const double xe = std::sqrt(a * a), ye = std::sqrt(b * b);
  g.ixmin = (int)std::floor(xc - xe + 0.5); g.ixmax = (int)std::ceil(xc + xe + 0.5);
  g.iymin = (int)std::floor(yc - ye + 0.5); g.iymax = (int)std::ceil(yc + ye + 0.5);
  return g;
}

bool window_fit(int W, int M, const Geom& g, int axis, int line, int n, int& wl0, int& wr0) {
  const double sa = axis == 0 ? g.a : g.b, sc = axis == 0 ? g.b : g.a;
  const double ca = axis == 0 ? g.xc : g.yc, cc = axis == 0 ? g.yc : g.xc;
  const double lo_c = ((double)line - 0.5) - cc, hi_c = ((double)line + 0.5) - cc;
  const double near_c = (lo_c > 0.0 ? lo_c : (hi_c < 0.0 ? -hi_c : 0.0)) / sc;
  const double far_c = std::fmax(std::fabs(lo_c), std::fabs(hi_c)) / sc;
  const double half_long = near_c < 1.0 ? sa * std::sqrt(1.0 - near_c * near_c) : 0.0;
  const double half_short = far_c < 1.0 ? sa * std::sqrt(1.0 - far_c * far_c) : 0.0;
  const int box_lo = std::max(0, g.lo(axis)), box_hi = std::min(n, g.hi(axis));
  wl0 = std::max(box_lo, (int)std::floor(ca - half_long) - M);
  const int wl1 = (int)std::ceil(ca - half_short) + M;
  const int wr1 = std::min(box_hi - 1, (int)std::ceil(ca + half_long) + M);
  wr0 = wr1 - (W - 1);
  const int wr_need = (int)std::floor(ca + half_short) - M;
  bool ok = wl1 - wl0 < W && wr_need >= wr0 && wl0 + W <= wr0 && half_long > 0.0;
  if (ok) {
    const double ia = ((double)(wl0 + W) - 0.5) - ca, ib = ((double)(wr0 - 1) + 0.5) - ca;
    ok = g.sum2(axis, ia, lo_c) <= 1.0 && g.sum2(axis, ib, lo_c) <= 1.0 && g.sum2(axis, ia, hi_c) <= 1.0 && g.sum2(axis, ib, hi_c) <= 1.0;
    const double nc = lo_c > 0.0 ? lo_c : (hi_c < 0.0 ? hi_c : 0.0);
    if (ok && wl0 > box_lo) {
      const double hi_a = ((double)(wl0 - 1) + 0.5) - ca;
      ok = hi_a < 0.0 && g.sum2(axis, hi_a, nc) > 1.0 + 1.0e-9;
    }
    if (ok && wr1 + 1 < box_hi) {
      const double lo_a = ((double)(wr1 + 1) - 0.5) - ca;
      ok = lo_a > 0.0 && g.sum2(axis, lo_a, nc) > 1.0 + 1.0e-9;
    }
  }
  return ok;
}

void ellipse(std::istringstream& in) {
  int n, axis;
  std::string w[4];
  in >> n >> axis >> w[0] >> w[1] >> w[2] >> w[3];
  const Geom g = make_geom(std::strtod(w[0].c_str(), nullptr), std::strtod(w[1].c_str(), nullptr), std::strtod(w[2].c_str(), nullptr),
                           std::strtod(w[3].c_str(), nullptr));
  const int l0 = std::max(0, axis == 0 ? g.iymin : g.ixmin), l1 = std::min(n, axis == 0 ? g.iymax : g.ixmax);
  const bool meets = std::max(0, g.lo(axis)) < std::min(n, g.hi(axis));
  for (int line = l0; line < l1 && meets; ++line) {
    static const int widths[3][2] = {{8, 1}, {16, 3}, {32, 3}};
    int W = 0, wl0 = 0, wr0 = 0;
    for (int t = 0; t < 3 && W == 0; ++t)
      if (window_fit(widths[t][0], widths[t][1], g, axis, line, n, wl0, wr0)) W = widths[t][0];
    if (W == 0) {
      std::printf("L %d 0 0 0 -\n", line);
      continue;
    }
    const double sa = axis == 0 ? g.a : g.b, sc = axis == 0 ? g.b : g.a, ca = axis == 0 ? g.xc : g.yc, cc = axis == 0 ? g.yc : g.xc;
    const double lo_c = ((double)line - 0.5) - cc, hi_c = ((double)line + 0.5) - cc;
    const double vv_lo = paos::edge_square(lo_c, sc), vv_hi = paos::edge_square(hi_c, sc);
    std::string classes;
    for (int side = 0; side < 2; ++side) {
      unsigned in_bits, und_bits;
      paos::window_classes(side == 0 ? wl0 : wr0, W, ca, sa, lo_c, hi_c, vv_lo, vv_hi, in_bits, und_bits);
      for (int k = 0; k < W; ++k) classes += (in_bits >> k) & 1u ? 'i' : ((und_bits >> k) & 1u ? 'u' : 'o');
    }
    std::printf("L %d %d %d %d %s\n", line, W, wl0, wr0, classes.c_str());
  }
  std::printf("end\n");
}

int layout(std::istringstream& in) {
  std::vector<int> counts;
  for (int c; in >> c;) counts.push_back(c);
  const int lines = (int)counts.size();
  if (lines > 64) return 2;
  const unsigned long long kFree = ~0ull;
  // exactly the capacity: a write behind it is the address sanitizer's to report
  std::vector<unsigned long long> list(paos::kBlockListCap, kFree);
  std::vector<int> offsets(lines), kept(lines);
  int total = 0, used = 0;
  bool ok = true;
  for (int i = 0; i < lines; ++i) {
    int t;
    paos::list_layout(counts.data(), lines, i, offsets[i], t);
    if (i == 0) total = t;
    ok = ok && t == total;
    kept[i] = paos::list_keeps(offsets[i], counts[i]) ? 1 : 0;
    // the count's pixels spread over the 64 window pixels: every other one first, then the rest
    unsigned long long und = 0ull;
    if (counts[i] < 0 || counts[i] > 64) return 2;
    for (int k = 0; k < counts[i]; ++k) und |= 1ull << (k < 32 ? 2 * k + 1 : 2 * (k - 32));
    const int wrote = paos::list_write(list.data(), i, offsets[i], und);
    ok = ok && wrote == (kept[i] ? counts[i] : 0);
    if (wrote) {
      used = std::max(used, offsets[i] + wrote);
      int at = offsets[i], last = -1;
      for (int k = 0; k < 64; ++k)
        if ((und >> k) & 1ull) {
          const unsigned long long e = list[at++];
          ok = ok && paos::entry_line(e) == i && paos::entry_pixel(e) == k && k > last;
          last = k;
        }
    }
  }
  for (int at = used; at < paos::kBlockListCap; ++at) ok = ok && list[at] == kFree;
  std::printf("offsets");
  for (int v : offsets) std::printf(" %d", v);
  std::printf("\nkept");
  for (int v : kept) std::printf(" %d", v);
  std::printf("\ntotal %d\nused %d\nguard %s\ncapacity %d\n", total, used, ok ? "ok" : "BAD", paos::kBlockListCap);
  return 0;
}

}  // namespace

int main() {
  std::string text;
  while (std::getline(std::cin, text)) {
    std::istringstream in(text);
    std::string what;
    if (!(in >> what)) continue;
    if (what == "ellipse") ellipse(in);
    else if (what == "layout") { if (int rc = layout(in)) return rc; }
    else return 1;
  }
  return 0;
}
