// pass_records.h -- the records of a pass program that host and device share: the layout of a parameter block, the per-item
// record of a frugal pass with its slots, phases and aperture lines, the descriptor of a phase table, the name of a build of
// the pass kernel (FrugalBuild; frugal_built says which names have one) and a pass as lowered for those kernels.  Plain C++:
// no HIP, no context, so that the planner of pass_program.h and a plain C++ program (tests/pass_program_main.cpp) can use
// them.  fft_kernels.h, frugal_pass.h, frugal_launch.h and host.h include this header.
#pragma once
#include "../../include/paos_hip.h"

#include <type_traits>
#include <vector>

namespace paos {

template <typename T>
struct cx;  // fft_core.h; only pointers to it appear here

// a per-item parameter block of a pointwise operator: [enable, sx, sy, coef, sgn] (doubles)
enum : int { FP_ENABLE = 0, FP_SX = 1, FP_SY = 2, FP_COEF = 3, FP_SGN = 4, FP_STRIDE = 5 };
// FFT control block: [enable, inverse, -, -, -]
enum : int { FC_ENABLE = 0, FC_INVERSE = 1 };

// The device sincos has no huge-argument path (fft_core.h: sincos_fast): the host refuses a phase whose argument at the
// grid corner reaches this (pass_program.h: check_phase_args).
constexpr double kMaxPhaseArg = 1.0e12;

constexpr int kFrugalMaxPre = 2, kFrugalMaxMid = 3;

struct FrugalPhase {
  double sx, sy, coef, sgn, m2, natural;  // natural != 0: np.fft.fftfreq index order
};
// A convex aperture along one line (a row for row passes, a column for column passes):
//   pos < p0: w_out | p0 <= pos < p1: vals[pos-p0] | p1 <= pos < p2: w_in |
//   p2 <= pos < p3: vals[kMaskW + pos-p2] | pos >= p3: w_out          (times the line factor lm)
// rendered by mask_lines_kernel (pointwise.h) with the same per-pixel functions the stand-alone
// aperture kernel uses, so values and the {0, partial, 1} classification are identical.
constexpr int kMaskW = 192;  // longest partial run per side the records can hold
struct MaskLine {
  int p0, p1, p2, p3;
  double lm;  // line multiplier (rectangles: the separable count of the other axis / 32)
  double pad;
};
struct FrugalSlot {
  double sign_on, scale;
  double mask_on, w_in, w_out;   // aperture riding on this slot (0/1), interior / exterior weight
  const MaskLine* lines;          // [N] records of THIS item for the pass axis
  const double* vals;             // [N][2 * kMaskW]
  // Round 4 (complex128): when every phase of the slot varies ALONG the line only -- the row / column factors of the
  // separable pass programs -- its factor is the same on every line of the pass: [N] factors of THIS item by position,
  // filled by phase_table_kernel right before the pass with the arithmetic of frugal_slot (slot_factor) and read back
  // instead of being evaluated 16 times per thread on each of a thousand lines.  nullptr: the slot evaluates.
  const cx<double>* table;
};
static_assert(sizeof(FrugalSlot) == 8 * sizeof(double), "record of 8-byte fields");
// per-item record, doubles: [fft1_on, fft1_inv, fft2_on, fft2_inv, pruning ranges, pre slot, pre phases[2],
// mid slot, mid phases[3]]
struct FrugalItem {
  double active;  // 0: the item takes no part in this pass (no load, no store)
  double fft1_on, fft1_inv, fft2_on, fft2_inv;
  // Pruning (zero lines of a field stay zero under every operator of a pass, and a transform of a
  // zero line is a zero line): the host tracks which rows / columns an aperture has just zeroed.
  //   lines outside [line_lo, line_hi) come out zero: tiles made of such lines only are not
  //     processed -- written with zeros when line_fill != 0, otherwise left alone because the next
  //     pass (along the other axis) will not read them;
  //   positions along a line outside [pos_lo, pos_hi) are known to be zero (and may hold stale
  //     data): they are not loaded.
  // Full ranges [0, N) switch all of it off.  Bounds are multiples of the block height.
  double line_lo, line_hi, line_fill, pos_lo, pos_hi;
  // positions along a line outside [spos_lo, spos_hi) need not be STORED: the next pass (along the other axis)
  // does not process the tiles of those lines -- an aperture in it is about to zero them
  double spos_lo, spos_hi;
  FrugalSlot pre;
  FrugalPhase pre_ph[kFrugalMaxPre];
  FrugalSlot mid;
  FrugalPhase mid_ph[kFrugalMaxMid];
};

// One phase table (frugal_pass.h: phase_table_kernel): the slot (`mid` = 0: in front of the first transform, 1: behind it) of
// the pass whose item records start at items[item_base], with `k` phases, along `axis`.
struct PhaseSlotDesc { int item_base, mid, k, axis; };

}  // namespace paos

#ifndef PAOS_LONG_ONE_LINE
#define PAOS_LONG_ONE_LINE 1
#endif
#ifndef PAOS_SINGLE_ONE_LINE
#define PAOS_SINGLE_ONE_LINE 1   // 0 (A/B builds): single table passes keep the two-line workgroups whatever they load and store
#endif

// One build of the pass kernel, by name: the record the planner picks per launch (pass_program.h: pick_build) and
// frugal_launch.h turns into template arguments (frugal_built says which records have a build).  The fields stand in
// frugal_launch<>'s order.
struct FrugalBuild {
  int axis;      // 0 rows, 1 columns
  int kpre;      // phases in front of the first transform: 0 .. kFrugalMaxPre (table builds: 1 = however many)
  int kmid;      // phases behind it: 0 .. kFrugalMaxMid (table builds likewise)
  int nfft;      // transforms of the launch's first pass: 1 or 2
  int store;     // 0 the field, 1 the PSF instead (FrugalArgs::psf), 2 the field and its power (FrugalArgs::pow_partial)
  int tab;       // every slot with phases reads FrugalSlot::table
  int fuse;      // the transforms of the NEXT one or two passes of the program that ride along: 0, [1], [2], 3 = [2][1], 4 = [2][2]
                 // (same axis, same lines; their item records follow this pass's in FrugalArgs::items: [2 or 3][batch])
  int one_line;  // a single table pass on the one-line workgroups of the fused launches
  int central;   // every active item of the first pass loads positions of [n / 4, 3 n / 4) only: the central-half build
};
// ... as the nine ints that cross the C ABI (paos_pass_builds, paos_frugal_built) and that frugal_unfold walks
constexpr int kBuildFields = 9;
static_assert(sizeof(FrugalBuild) == kBuildFields * sizeof(int), "a record of ints");
inline void build_to_ints(const FrugalBuild& b, int* rec) {
  const int v[kBuildFields] = {b.axis, b.kpre, b.kmid, b.nfft, b.store, b.tab, b.fuse, b.one_line, b.central};
  for (int k = 0; k < kBuildFields; ++k) rec[k] = v[k];
}
inline FrugalBuild build_from_ints(const int* rec) {
  return FrugalBuild{rec[0], rec[1], rec[2], rec[3], rec[4], rec[5], rec[6], rec[7], rec[8]};
}

// Which builds exist of the family (T, N): THE statement of it -- frugal_dispatch instantiates a kernel exactly where this
// holds, and pick_build (pass_program.h) asks here before it names a one-line or a central-half build.
//   evaluating slots (tab = 0): any number of phases per slot; the PSF store where both slots have at most one (what a chain
//     can end on: the last column pass of a separable program usually has the column half of a phase in front of its first
//     transform), field + power where the first has at most one (what a program that ends on a saved surface ends with);
//   table slots (tab = 1): one build for any number of phases per slot (kpre, kmid = 1: "has phases"), any store;
//   fused launches (fuse = 1 .. 4): table slots with phases in both, behind a two-transform pass, any store;
//   one-line workgroups (one_line = 1, round 5): field-storing single table passes of complex128 at 4096^2 and 2048^2;
//   central half (central = 1, round 11; frugal_pass.h: frugal_pass_kernel, CH): 4096^2 complex128 table slots with kpre = 1, on
//     the one-line workgroups -- the field-storing fused launches and the one-line single passes.  The PSF-storing fused build
//     (two-line workgroups; the last column launch of a step loads a quarter too) was built and measured as well: 0.97 ->
//     1.10 ms per launch, so it keeps the ordinary build (profiles/r11_central_half.md).
//     Round 23: every central-half build holds a second kernel, the narrow-window variant (CH = 2), for launches that load
//     and store inside [5 n / 16, 11 n / 16).  It has no name of its own here: which of the two kernels a launch of the build
//     takes is decided per launch (pass_program.h: pick_narrow) and handed to frugal_launch beside the record
//     (profiles/r23_narrow_windows.md).
template <typename T, int N>
constexpr bool frugal_built(const FrugalBuild& b) {
  constexpr bool kOneLineSizes = sizeof(T) == 8 && (N == 4096 || N == 2048) && PAOS_LONG_ONE_LINE != 0;
  if (b.axis < 0 || b.axis > 1 || b.kpre < 0 || b.kpre > paos::kFrugalMaxPre || b.kmid < 0 || b.kmid > paos::kFrugalMaxMid) return false;
  if (b.nfft < 1 || b.nfft > 2 || b.store < 0 || b.store > 2 || b.fuse < 0 || b.fuse > 4) return false;
  if ((b.tab | b.one_line | b.central) & ~1) return false;
  if (b.one_line && !(kOneLineSizes && PAOS_SINGLE_ONE_LINE != 0 && b.tab && !b.fuse && b.store == 0)) return false;
  if (b.central && !(kOneLineSizes && N == 4096 && b.tab && b.kpre == 1 && b.store == 0 && (b.fuse || b.one_line))) return false;
  if (b.fuse) return b.tab && b.kpre == 1 && b.kmid == 1 && b.nfft == 2;
  if (b.tab) return b.kpre <= 1 && b.kmid <= 1 && b.kpre + b.kmid > 0;
  return b.store == 0 || (b.kpre <= 1 && (b.store == 2 || b.kmid <= 1));
}

// f(T{}, std::integral_constant<int, N>) for the family (element type, grid size) of the frugal pass kernel: the one place
// that lists them -- complex128 at 1024, 2048 and 4096, complex64 at 2048 and 4096.  `none` for every other (precision, n).
template <typename R, typename F>
R dispatch_family(int precision, int n, R none, F&& f) {
  if (precision == PAOS_F64) {
    if (n == 1024) return f(double{}, std::integral_constant<int, 1024>{});
    if (n == 2048) return f(double{}, std::integral_constant<int, 2048>{});
    if (n == 4096) return f(double{}, std::integral_constant<int, 4096>{});
  } else if (precision == PAOS_F32) {
    if (n == 2048) return f(float{}, std::integral_constant<int, 2048>{});
    if (n == 4096) return f(float{}, std::integral_constant<int, 4096>{});
  }
  return none;
}

// One pass of a program, lowered for the frugal kernels before anything is launched, so that the
// planner can look ahead.
struct LoweredPass {
  bool ok = false;
  std::vector<paos::FrugalItem> items;
  int kpre = 0, kmid = 0, nfft = 1, mask_block = -1, mask_slot = -1;
  std::vector<double> mask_shared;  // [batch] 1: the item reads the line records of an earlier, identical item
  std::vector<int> mask_rep;        // [batch] item whose records this item reads (-1: none)
  int mask_set = -1;                // which of the context's record sets this pass reads
  int mask_shapes = 3;              // bit s: some item's aperture has shape s (0 ellipse, 1 rectangle) and renders its own records
  int mask_lo = 0, mask_hi = 0;     // lines whose records this pass reads (pass_program.h: record_window, behind the pruning plan)
  bool mask_render = false;         // ... and whether it has to be rendered first
};
