// frugal_launch.h -- from the name of a build of the frugal pass kernel (pass_records.h: FrugalBuild; frugal_built says which
// names have a build) to its launch: what a build's workgroup looks like (FrugalGeometry), the launch (frugal_launch) and the step from
// the run-time record to the template arguments (frugal_dispatch).  Each frugal_<family>.hip instantiates frugal_dispatch for
// one (type, N) and nothing else.
#pragma once
#include "host.h"
#include "pass_records.h"

// (which names have a build: frugal_built<T, N>, with PAOS_LONG_ONE_LINE / PAOS_SINGLE_ONE_LINE, in pass_records.h)

// ... what a launch of a name without a build fails with
inline int frugal_not_built(paos_ctx* c, const FrugalBuild& b) {
  if (b.tab && b.fuse) {
    if (b.kpre != 1 || b.kmid != 1) return fail(c, PAOS_EINVAL, "no fused build of this pass shape");
    if (b.nfft < 2) return fail(c, PAOS_EINVAL, "a fused chain starts with a two-transform pass");
    if (b.fuse > 4) return fail(c, PAOS_EINVAL, "a launch runs at most three passes");
  }
  if (b.tab && !(b.kpre <= 1 && b.kmid <= 1 && b.kpre + b.kmid > 0)) return fail(c, PAOS_EINVAL, "no table build of this pass shape");
  if (b.store == 1 && !b.tab) return fail(c, PAOS_EUNSUPPORTED, "no PSF-storing build of this pass shape");
  if (b.store == 2 && !b.tab) return fail(c, PAOS_EUNSUPPORTED, "no power-summing build of this pass shape");
  return fail(c, PAOS_EINVAL, "no build of this pass shape");
}

// The workgroup of a build: what frugal_pass_kernel's remaining template arguments and the launch follow from.
// LINES_, TILES_ != 0 (tools/fftbench.hip, tools/timeline.hip): another tile than the library's, everything else as derived here.
template <typename T, int N, int AXIS, int KPRE, int KMID, int STORE = 0, int LONG = 0, int ONE = 0, int LINES_ = 0, int TILES_ = 0>
struct FrugalGeometry {
  using C = FftCfg<T, N>;
  // Round 5: the launches that run two or three passes of a chain (LONG builds) and store the field are bound by the latency
  // chain of a workgroup -- exchanges, barriers, table reads -- not by bytes (they move a sixteenth of the grid): at 4096^2
  // complex128 they run on ONE-line workgroups of 256 threads, four per CU with one wave each per SIMD instead of two of
  // 512 threads (-6 ... -8 % rows, -2 ... -3 % columns, bit-identical: profiles/r05_fftbench_fused_variants.txt).  The 16- /
  // 32-byte pieces such tiles take out of every 128-byte block, which rule them out for byte-bound passes, cost nothing
  // here.  (The PSF- / power-summing builds keep the two-line tiles: their partial sums are laid out per two-line tile.)
  // ONE = 1: a single table pass that loads AND stores at most half of its positions (the two passes of the first stretch since
  // the start box) is as latency-bound as the fused launches and takes the same shape (pick_build decides per launch).
  static constexpr bool kLatencyBound = PAOS_LONG_ONE_LINE != 0 && (LONG != 0 || ONE != 0) && STORE == 0 && sizeof(T) == 8;
  static constexpr bool kOneLine = kLatencyBound && N == 4096;
  // ... and at 2048^2, where a line is 128 threads and the workgroup already two lines of them: four workgroups per CU instead
  // of three (frugal_pass.h: OCC)
  // (1024^2: measured too -- four rows per workgroup keep four twiddles per thread in registers and the shapes spill 30-100 B:
  // fused two-pass launches 0.866 -> 0.878 ms, three-pass 1.22 -> 1.31: stays on three workgroups per CU.  profiles/r05_ab_variants_bench.txt)
  static constexpr int OCC = (kLatencyBound && N == 2048) ? 1 : 0;
  static constexpr int LINES = LINES_ != 0 ? LINES_ : (kOneLine ? 1 : (AXIS == 0 ? C::FR_ROW_LINES : C::COL_LINES));
  static constexpr int TILES = TILES_ != 0 ? TILES_ : (AXIS == 0 ? C::ROW_TILES : C::COL_TILES);
  // several workgroups share the 160 KiB of LDS: c128 exchanges re and im in turn; a c64 line
  // fits whole (the same 35 KiB) and so needs half the barriers -- except in the 4-line row tiles
  static constexpr bool SPLIT = sizeof(T) == 8 || LINES > 2;
  static constexpr int GROUPS = N / LINES / TILES, THREADS = TILES * LINES * N / C::E;
  static constexpr size_t LDS = frugal_lds_bytes<T, N, LINES, TILES, SPLIT, KPRE, KMID, C::E, STORE, OCC>();
  // TileMap renumbers the tiles that share 128-byte lines inside aligned groups of workgroups (siblings 8 apart: one XCD):
  // 16 for half-block row tiles and whole-block column tiles, 32 for the quarter-block row tiles of the one-line builds
  static constexpr unsigned ALIGN = (LINES == 1 && AXIS == 0) ? 32 : 16;
};

namespace {

// narrow (central-half builds only, CH = 1): the launch takes the narrow-window variant of the build, the CH = 2 kernel of the
// same shape -- a property of the launch (pass_program.h: pick_narrow), not of the build's name
template <typename T, int N, int AXIS, int KPRE, int KMID, int NFFT, int STORE, int TAB, int LONG, int ONE, int CH>
int frugal_launch(paos_ctx* c, const FrugalArgs& args, bool narrow) {
  using C = FftCfg<T, N>;
  using G = FrugalGeometry<T, N, AXIS, KPRE, KMID, STORE, LONG, ONE>;
  FrugalArgs a = args;
  unsigned groups = G::GROUPS;
  a.wg0 = 0;
  static_assert(G::GROUPS % G::ALIGN == 0, "TileMap renumbers tiles inside aligned groups of workgroups");
  if (a.live_hi > a.live_lo) {  // launch the workgroups of live lines only, in whole groups
    const unsigned per = G::LINES * G::TILES;
    a.wg0 = (a.live_lo / per) / G::ALIGN * G::ALIGN;
    unsigned end = ((a.live_hi + per - 1) / per + G::ALIGN - 1) / G::ALIGN * G::ALIGN;
    if (end > groups) end = groups;
    groups = end - a.wg0;
  }
  const dim3 grid(groups, c->batch), block(G::THREADS);
  constexpr size_t kMaxPad = 8192;
  const size_t lds = G::LDS + (c->lds_pad < kMaxPad ? c->lds_pad : kMaxPad);
  auto kern = frugal_pass_kernel<T, N, C::E, G::LINES, G::TILES, AXIS, C::BR, C::BC, G::SPLIT, KPRE, KMID, NFFT, STORE, TAB, LONG, G::OCC, CH>;
  if constexpr (CH == 1) {
    if (narrow) kern = frugal_pass_kernel<T, N, C::E, G::LINES, G::TILES, AXIS, C::BR, C::BC, G::SPLIT, KPRE, KMID, NFFT, STORE, TAB, LONG, G::OCC, 2>;
  } else {
    narrow = false;
  }
  ++(CH != 0 ? c->central_launches : c->plain_launches);  // paos_central_half_stats (a narrow launch is a central one)
  ++(narrow ? c->narrow_launches : c->other_launches);    // paos_narrow_window_stats
  return TIMED_LAUNCH(c, kern, grid, block, lds, G::LDS + kMaxPad, AXIS == 0 ? PAOS_KERNEL_PASS_ROWS : PAOS_KERNEL_PASS_COLS,
                      c->prof_next_tag, PAOS_FRUGAL_PASS(a));
}

// From the run-time record to the template arguments, one field per step: V... are the fields unfolded so far, X the value
// the next one is compared with.  Behind the last field: the launch, where the name has a build.
constexpr int kFrugalFieldMax[] = {1, kFrugalMaxPre, kFrugalMaxMid, 2, 2, 1, 4, 1, 1};  // (FrugalBuild's fields, in order)
template <typename T, int N, int X, int... V>
int frugal_unfold(paos_ctx* c, const FrugalBuild& b, const FrugalArgs& a, bool narrow) {
  constexpr int I = sizeof...(V), kFields = sizeof(kFrugalFieldMax) / sizeof(int);
  static_assert(kFields == kBuildFields, "one maximum per field");
  int field[kBuildFields];
  build_to_ints(b, field);
  if (field[I] != X) {
    if constexpr (X < kFrugalFieldMax[I]) return frugal_unfold<T, N, X + 1, V...>(c, b, a, narrow);
    else return frugal_not_built(c, b);
  } else if constexpr (I + 1 < kFields) {
    return frugal_unfold<T, N, 0, V..., X>(c, b, a, narrow);
  } else if constexpr (frugal_built<T, N>(FrugalBuild{V..., X})) {
    return frugal_launch<T, N, V..., X>(c, a, narrow);
  } else {
    return frugal_not_built(c, b);
  }
}
template <typename T, int N>
int frugal_dispatch(paos_ctx* c, const FrugalBuild& b, const FrugalArgs& a, bool narrow = false) {
  return frugal_unfold<T, N, 0>(c, b, a, narrow);
}

}  // namespace
