// series_sum_plan.h -- the size rule and the launch ranges of a broadband series sum (series.hip, paos_series_sum_*).
// Plain C++: no HIP, so that a stand-alone program can walk it on the host (tests/test_series_sum_plan_host.py).
#pragma once
#include <cstddef>

#include "series_plan.h"

namespace paos {

// the accumulator S[frames][ny][nx] holds at most 2^27 doubles (1 GiB); include/paos_hip.h: PAOS_SERIES_SUM_MAX_DOUBLES
constexpr size_t kSeriesSumMaxDoubles = size_t(1) << 27;
constexpr int kSeriesSumMaxFrames = 65536;

// the size rule on a count of doubles
inline bool series_sum_fits(size_t doubles) { return doubles >= 1 && doubles <= kSeriesSumMaxDoubles; }

// Doubles of S for `frames` frames of an nx x ny detector, formed in size_t (65536 x 4096 x 4096 = 2^40 fits); false when
// an argument is out of range or the accumulator would be larger than the rule allows -- before anything is allocated.
inline bool series_sum_size(int frames, int nx, int ny, size_t* doubles) {
  if (frames < 1 || frames > kSeriesSumMaxFrames || nx < 1 || nx > 4096 || ny < 1 || ny > 4096) return false;
  const size_t count = (size_t)frames * (size_t)nx * (size_t)ny;
  if (!series_sum_fits(count)) return false;
  if (doubles) *doubles = count;
  return true;
}

// One launch: frames [t0, t0 + nt), nt <= kSeriesMaxChunkFrames (a grid dimension).  Ranges run in frame order.
struct SeriesSumRange {
  int t0, nt;
};
// the range behind `r` (start with {0, 0}); false when every frame has been covered
inline bool series_sum_next_range(int frames, SeriesSumRange* r) {
  const int t0 = r->t0 + r->nt;
  if (t0 >= frames) return false;
  r->t0 = t0;
  r->nt = frames - t0 < kSeriesMaxChunkFrames ? frames - t0 : kSeriesMaxChunkFrames;
  return true;
}

// workgroups of `threads` pixels that cover one frame
inline unsigned series_sum_tiles(size_t npix, int threads) { return (unsigned)((npix + (size_t)threads - 1) / (size_t)threads); }

}  // namespace paos
