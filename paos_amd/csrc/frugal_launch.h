// frugal_launch.h -- from the run-time shape of a frugal pass (axis, phases per slot, transforms, what it stores) to the
// launch of its compile-time build.  Each frugal_<family>.hip instantiates this for one (type, N) and nothing else.
#pragma once
#include "host.h"

namespace {

#ifndef PAOS_LONG_ONE_LINE
#define PAOS_LONG_ONE_LINE 1
#endif
#ifndef PAOS_SINGLE_ONE_LINE
#define PAOS_SINGLE_ONE_LINE 1   // 0 (A/B builds): single table passes keep the two-line workgroups whatever they load and store
#endif
// Round 11, CH = 1: the central-half build of the shape (frugal_pass.h: frugal_pass_kernel, CH) -- for the launches whose first
// pass loads positions of [N / 4, 3 N / 4) only (launch_lowered: FrugalArgs::central).  Built for 4096^2 complex128, table
// slots, KPRE = 1 and the shapes a chain step launches with such a window: the field-storing LONG builds and the one-line
// single passes.  The PSF-storing LONG build (two-line workgroups; the last column launch of a step loads a quarter too)
// was built and measured as well: 0.97 -> 1.10 ms per launch, so it keeps the ordinary build (profiles/r11_central_half.md).
template <typename T, int N, int KPRE, int TAB>
constexpr bool frugal_central() { return sizeof(T) == 8 && N == 4096 && KPRE == 1 && TAB != 0; }
template <typename T, int N, int AXIS, int KPRE, int KMID, int NFFT, int STORE = 0, int TAB = 0, int LONG = 0, int ONE = 0, int CH = 0>
int frugal_launch(paos_ctx* c, const FrugalArgs& args) {
  using C = FftCfg<T, N>;
  static_assert(CH == 0 || frugal_central<T, N, KPRE, TAB>(), "no central-half build of this shape");
  // Round 5: the launches that run two or three passes of a chain (LONG builds) and store the field are bound by the latency
  // chain of a workgroup -- exchanges, barriers, table reads -- not by bytes (they move a sixteenth of the grid): at 4096^2
  // complex128 they run on ONE-line workgroups of 256 threads, four per CU with one wave each per SIMD instead of two of
  // 512 threads (-6 ... -8 % rows, -2 ... -3 % columns, bit-identical: profiles/r05_fftbench_fused_variants.txt).  The 16- /
  // 32-byte pieces such tiles take out of every 128-byte block, which rule them out for byte-bound passes, cost nothing
  // here.  (The PSF- / power-summing builds keep the two-line tiles: their partial sums are laid out per two-line tile.)
  // ONE = 1: a single table pass that loads AND stores at most half of its positions (the two passes of the first stretch since
  // the start box) is as latency-bound as the fused launches and takes the same shape (launch_lowered decides per launch).
  constexpr bool kOneLine = PAOS_LONG_ONE_LINE != 0 && (LONG != 0 || ONE != 0) && STORE == 0 && sizeof(T) == 8 && N == 4096;
  // ... and at 2048^2, where a line is 128 threads and the workgroup already two lines of them: four workgroups per CU instead
  // of three (frugal_pass.h: OCC)
  // (1024^2: measured too -- four rows per workgroup keep four twiddles per thread in registers and the shapes spill 30-100 B:
  // fused two-pass launches 0.866 -> 0.878 ms, three-pass 1.22 -> 1.31: stays on three workgroups per CU.  profiles/r05_ab_variants_bench.txt)
  constexpr int kOcc = (PAOS_LONG_ONE_LINE != 0 && (LONG != 0 || ONE != 0) && STORE == 0 && sizeof(T) == 8 && N == 2048) ? 1 : 0;
  constexpr int LINES = kOneLine ? 1 : (AXIS == 0 ? C::FR_ROW_LINES : C::COL_LINES);
  constexpr int TILES = AXIS == 0 ? C::ROW_TILES : C::COL_TILES;
  // several workgroups share the 160 KiB of LDS: c128 exchanges re and im in turn; a c64 line
  // fits whole (the same 35 KiB) and so needs half the barriers -- except in the 4-line row tiles
  constexpr bool SPLIT = sizeof(T) == 8 || LINES > 2;
  FrugalArgs a = args;
  unsigned groups = N / LINES / TILES;
  a.wg0 = 0;
  // TileMap renumbers the tiles that share 128-byte lines inside aligned groups of workgroups (siblings 8 apart: one XCD):
  // 16 for half-block row tiles and whole-block column tiles, 32 for the quarter-block row tiles of the one-line builds
  constexpr unsigned kAlign = (kOneLine && AXIS == 0) ? 32 : 16;
  static_assert((N / LINES / TILES) % kAlign == 0, "TileMap renumbers tiles inside aligned groups of workgroups");
  if (a.live_hi > a.live_lo) {  // launch the workgroups of live lines only, in whole groups
    const unsigned per = LINES * TILES;
    a.wg0 = (a.live_lo / per) / kAlign * kAlign;
    unsigned end = ((a.live_hi + per - 1) / per + kAlign - 1) / kAlign * kAlign;
    if (end > groups) end = groups;
    groups = end - a.wg0;
  }
  const dim3 grid(groups, c->batch), block(TILES * LINES * N / C::E);
  constexpr size_t kMaxPad = 8192;
  const size_t lds = frugal_lds_bytes<T, N, LINES, TILES, SPLIT, KPRE, KMID, C::E, STORE, kOcc>() + (c->lds_pad < kMaxPad ? c->lds_pad : kMaxPad);
  auto kern = frugal_pass_kernel<T, N, C::E, LINES, TILES, AXIS, C::BR, C::BC, SPLIT, KPRE, KMID, NFFT, STORE, TAB, LONG, kOcc, CH>;
  ++(CH != 0 ? c->central_launches : c->plain_launches);  // paos_central_half_stats
  return TIMED_LAUNCH(c, kern, grid, block, lds, frugal_lds_bytes<T, N, LINES, TILES, SPLIT, KPRE, KMID, C::E, STORE, kOcc>() + kMaxPad,
                      AXIS == 0 ? PAOS_KERNEL_PASS_ROWS : PAOS_KERNEL_PASS_COLS, c->prof_next_tag, PAOS_FRUGAL_PASS(a));
}

template <typename T, int N, int AXIS, int KPRE, int KMID>
int frugal_nfft(paos_ctx* c, const FrugalArgs& a, int nfft) {
  // (the digit-swapped two-transform variant NFFT = 3 of frugal_pass.h is built by tools/fftbench.hip only:
  // measured in round 2 with parity unchanged and no gain, profiles/r02_fftbench_digit_swapped_experiment.txt)
  if (a.tab && a.fuse) {  // ... and the launch runs the next pass -- or the next two -- of the program as well (LONG builds)
    if constexpr (KPRE == 1 && KMID == 1) {
      if (nfft < 2) return fail(c, PAOS_EINVAL, "a fused chain starts with a two-transform pass");
#define PAOS_LONG_CASE(L)                                                           \
  case L:                                                                           \
    if constexpr (frugal_central<T, N, 1, 1>() && PAOS_LONG_ONE_LINE != 0) {  /* (the one-line builds only) */ \
      if (a.central && !a.psf && !a.pow_partial) return frugal_launch<T, N, AXIS, 1, 1, 2, 0, 1, L, 0, 1>(c, a);  \
    }                                                                               \
    if (a.psf) return frugal_launch<T, N, AXIS, 1, 1, 2, 1, 1, L>(c, a);            \
    if (a.pow_partial) return frugal_launch<T, N, AXIS, 1, 1, 2, 2, 1, L>(c, a);    \
    return frugal_launch<T, N, AXIS, 1, 1, 2, 0, 1, L>(c, a);
      switch (a.fuse) {
        PAOS_LONG_CASE(1)
        PAOS_LONG_CASE(2)
        PAOS_LONG_CASE(3)
        PAOS_LONG_CASE(4)
      }
#undef PAOS_LONG_CASE
      return fail(c, PAOS_EINVAL, "a launch runs at most three passes");
    } else {
      return fail(c, PAOS_EINVAL, "no fused build of this pass shape");
    }
  }
  if (a.tab) {  // the slots read their factors from tables: one build for any number of phases per slot
    if constexpr (KPRE <= 1 && KMID <= 1 && KPRE + KMID > 0) {
      if (a.psf) return nfft >= 2 ? frugal_launch<T, N, AXIS, KPRE, KMID, 2, 1, 1>(c, a) : frugal_launch<T, N, AXIS, KPRE, KMID, 1, 1, 1>(c, a);
      if (a.pow_partial) return nfft >= 2 ? frugal_launch<T, N, AXIS, KPRE, KMID, 2, 2, 1>(c, a) : frugal_launch<T, N, AXIS, KPRE, KMID, 1, 2, 1>(c, a);
      if constexpr (sizeof(T) == 8 && (N == 4096 || N == 2048) && PAOS_LONG_ONE_LINE != 0) {
        if constexpr (frugal_central<T, N, KPRE, 1>()) {
          if (a.one_line && a.central && PAOS_SINGLE_ONE_LINE != 0)
            return nfft >= 2 ? frugal_launch<T, N, AXIS, KPRE, KMID, 2, 0, 1, 0, 1, 1>(c, a) : frugal_launch<T, N, AXIS, KPRE, KMID, 1, 0, 1, 0, 1, 1>(c, a);
        }
        if (a.one_line && PAOS_SINGLE_ONE_LINE != 0) return nfft >= 2 ? frugal_launch<T, N, AXIS, KPRE, KMID, 2, 0, 1, 0, 1>(c, a) : frugal_launch<T, N, AXIS, KPRE, KMID, 1, 0, 1, 0, 1>(c, a);
      }
      return nfft >= 2 ? frugal_launch<T, N, AXIS, KPRE, KMID, 2, 0, 1>(c, a) : frugal_launch<T, N, AXIS, KPRE, KMID, 1, 0, 1>(c, a);
    } else {
      return fail(c, PAOS_EINVAL, "no table build of this pass shape");
    }
  }
  if constexpr (KPRE <= 1 && KMID <= 1) {  // the shapes a chain can end on: also built with the PSF store (KPRE = 1: round 4,
    // the last column pass of a separable program usually has the column half of a phase in front of its first transform)
    if (a.psf) return nfft >= 2 ? frugal_launch<T, N, AXIS, KPRE, KMID, 2, 1>(c, a) : frugal_launch<T, N, AXIS, KPRE, KMID, 1, 1>(c, a);
  } else {
    if (a.psf) return fail(c, PAOS_EUNSUPPORTED, "no PSF-storing build of this pass shape");
  }
  if constexpr (KPRE <= 1) {  // ... and the shapes a program that ends on a saved surface ends with: field + its power
    if (a.pow_partial) return nfft >= 2 ? frugal_launch<T, N, AXIS, KPRE, KMID, 2, 2>(c, a) : frugal_launch<T, N, AXIS, KPRE, KMID, 1, 2>(c, a);
  } else {
    if (a.pow_partial) return fail(c, PAOS_EUNSUPPORTED, "no power-summing build of this pass shape");
  }
  return nfft >= 2 ? frugal_launch<T, N, AXIS, KPRE, KMID, 2>(c, a) : frugal_launch<T, N, AXIS, KPRE, KMID, 1>(c, a);
}
template <typename T, int N, int AXIS, int KPRE>
int frugal_kmid(paos_ctx* c, const FrugalArgs& a, int kmid, int nfft) {
  switch (kmid) {
    case 0: return frugal_nfft<T, N, AXIS, KPRE, 0>(c, a, nfft);
    case 1: return frugal_nfft<T, N, AXIS, KPRE, 1>(c, a, nfft);
    case 2: return frugal_nfft<T, N, AXIS, KPRE, 2>(c, a, nfft);
    default: return frugal_nfft<T, N, AXIS, KPRE, 3>(c, a, nfft);
  }
}
template <typename T, int N, int AXIS>
int frugal_kpre(paos_ctx* c, const FrugalArgs& a, int kpre, int kmid, int nfft) {
  switch (kpre) {
    case 0: return frugal_kmid<T, N, AXIS, 0>(c, a, kmid, nfft);
    case 1: return frugal_kmid<T, N, AXIS, 1>(c, a, kmid, nfft);
    default: return frugal_kmid<T, N, AXIS, 2>(c, a, kmid, nfft);
  }
}
template <typename T, int N>
int frugal_axis(paos_ctx* c, const FrugalArgs& a, int axis, int kpre, int kmid, int nfft) {
  return axis == 0 ? frugal_kpre<T, N, 0>(c, a, kpre, kmid, nfft) : frugal_kpre<T, N, 1>(c, a, kpre, kmid, nfft);
}

}  // namespace
