// series_plan.h -- how a pointing series is cut into chunks (series.hip).  Plain C++: no HIP, so that a stand-alone
// program can walk every plan on the host (tests/test_series_plan_host.py).
#pragma once
#include <cstddef>
#include <cstdlib>

namespace paos {

// frames of one chunk are a grid dimension of both launches
constexpr int kSeriesMaxChunkFrames = 32768;

// The frame buffer holds [items][frames][npix] doubles of one chunk and never more than `cap` bytes -- except that a chunk
// always holds at least one frame of every item, or of ONE item if even a frame of every item does not fit.
struct SeriesPlan {
  int items = 0;   // items per chunk (the last group of a frame range may be shorter)
  int frames = 0;  // frames per chunk (the last chunk may be shorter)
};

inline SeriesPlan series_plan(int batch, int frames, size_t npix, size_t cap) {
  SeriesPlan p;
  const size_t one = npix * sizeof(double);  // one frame of one item
  const size_t all = one * (size_t)batch;    // one frame of every item
  if (all <= cap) {
    size_t f = cap / all;
    if (f > (size_t)frames) f = (size_t)frames;
    if (f > (size_t)kSeriesMaxChunkFrames) f = (size_t)kSeriesMaxChunkFrames;
    p.items = batch;
    p.frames = (int)f;
  } else {
    size_t k = cap / one;
    if (k < 1) k = 1;
    p.items = (int)k;  // (k < batch: all > cap)
    p.frames = 1;
  }
  return p;
}

// bytes of the frame buffer a plan needs
inline size_t series_plan_bytes(const SeriesPlan& p, size_t npix) { return (size_t)p.items * (size_t)p.frames * npix * sizeof(double); }

// One chunk: frames [t0, t0 + nt) of items [i0, i0 + ni).  Chunks run in frame order; within a frame range, in item order.
struct SeriesChunk {
  int t0, nt, i0, ni;
};
// the chunk behind `c` (start with {0, 0, 0, 0}); false when the series is done
inline bool series_next_chunk(const SeriesPlan& p, int batch, int frames, SeriesChunk* c) {
  int t0 = c->t0, i0 = c->i0 + c->ni;
  if (c->nt == 0) i0 = 0;           // the first chunk
  else if (i0 >= batch) { t0 += c->nt; i0 = 0; }
  if (t0 >= frames) return false;
  c->t0 = t0;
  c->nt = frames - t0 < p.frames ? frames - t0 : p.frames;
  c->i0 = i0;
  c->ni = batch - i0 < p.items ? batch - i0 : p.items;
  return true;
}

// PAOS_SERIES_SCRATCH_BYTES: a positive integer; anything else leaves the default
inline size_t series_cap_bytes(const char* env, size_t fallback) {
  if (!env || !*env) return fallback;
  char* end = nullptr;
  const unsigned long long v = std::strtoull(env, &end, 10);
  if (end == env || *end != '\0' || v == 0 || env[0] == '-') return fallback;
  return (size_t)v;
}

}  // namespace paos
