// zoom.hip -- zoomed windows by exact band-limited interpolation (paos_zoom_*; kernels: zoom_pass.h).
#include "host.h"

#include <cmath>

#include "zoom_pass.h"

extern "C" {

// ---- zoomed windows (include/paos_hip.h; kernels: zoom_pass.h) -------------------------------
int paos_zoom_weights(int n, int s, double frac, double* w, int* carry) {
  if (n < 2 || (n & 1) || n > (1 << 20)) return fail(nullptr, PAOS_EINVAL, "paos_zoom_weights: n must be even, 2 .. 2^20");
  if (s < 1 || s > 64) return fail(nullptr, PAOS_EINVAL, "paos_zoom_weights: s must be 1 .. 64");
  if (!(frac >= 0.0 && frac < 1.0)) return fail(nullptr, PAOS_EINVAL, "paos_zoom_weights: frac must lie in [0, 1)");
  if (!w || !carry) return fail(nullptr, PAOS_EINVAL, "paos_zoom_weights: null argument");
  const long double pi = 3.141592653589793238462643383279502884L;
  for (int b = 0; b < s; ++b) {
    long double phi = (long double)frac + (long double)b / (long double)s;
    carry[b] = 0;
    if (phi >= 1.0L) {
      phi -= 1.0L;
      carry[b] = 1;
    }
    double* row = w + (size_t)b * n;
    if (phi == 0.0L) {
      for (int k = 0; k < n; ++k) row[k] = 0.0;
      row[0] = 1.0;
      continue;
    }
    const long double sn = sinl(pi * phi);
    for (int m = -n / 2; m < n / 2; ++m) {
      const long double v = sn / ((long double)n * tanl(pi * ((long double)m + phi) / (long double)n));
      row[m < 0 ? m + n : m] = (double)((m & 1) ? -v : v);
    }
  }
  return PAOS_OK;
}

}  // extern "C"

namespace {

const char* const kZoomBadSize = "the window size must be a multiple of 16 in 16 .. 1024";

bool zoom_size_ok(int m) { return m >= 16 && m <= 1024 && !(m & 15); }

// the largest number of 16-row tiles per wave (8, 4, 2, 1) that still leaves a wave for every SIMD of the chip
int zoom_tiles_per_wave(int tiles, long waves_at_one) {
  int pt = 8;
  while (pt > 1 && (pt > tiles || waves_at_one / pt < 1024)) pt /= 2;
  return pt;
}

}  // namespace

extern "C" {

int paos_zoom_tiles(int n, int batch, int m, int* pt_y, int* pt_x) {
  if (n < 16 || (n & 15) || n > (1 << 20)) return fail(nullptr, PAOS_EINVAL, "paos_zoom_tiles: n must be a multiple of 16 in 16 .. 2^20");
  if (batch < 1) return fail(nullptr, PAOS_EINVAL, "paos_zoom_tiles: batch must be at least 1");
  if (!zoom_size_ok(m)) return fail(nullptr, PAOS_EINVAL, std::string("paos_zoom_tiles: ") + kZoomBadSize);
  if (!pt_y || !pt_x) return fail(nullptr, PAOS_EINVAL, "paos_zoom_tiles: null argument");
  const int tiles = m / 16;
  // a wave owns 16 columns d: N / 16 column tiles in stage Y (d runs over the grid), M / 16 in stage X (over the window)
  *pt_y = zoom_tiles_per_wave(tiles, (long)batch * (n / 16) * tiles);
  *pt_x = zoom_tiles_per_wave(tiles, (long)batch * tiles * tiles);
  return PAOS_OK;
}

}  // extern "C"

namespace {

constexpr int kZoomMaxTables = 256;  // tables the pool keeps; also the most distinct fractional parts of one call

// Slots of the [s][n] phase tables of `fracs` (distinct values, all of ONE call) in the context's pool.  Every slot of
// the call is resolved here, and whatever frees or moves tables happens before the first of them is handed out: the
// pool starts afresh (once) under another oversampling or when the call's new fractions do not fit beside the pooled
// ones; it grows (once) to hold them.  Tables missing afterwards are built on the host and uploaded.
int zoom_table_slots(paos_ctx* c, int s, const std::vector<double>& fracs, std::vector<int>& slots) {
  const size_t tab = (size_t)s * c->n;
  if ((int)fracs.size() > kZoomMaxTables)
    return fail(c, PAOS_EINVAL, "paos_zoom_compute: more than " + std::to_string(kZoomMaxTables) +
                                    " distinct fractional parts among the centres of one call");
  auto find = [&](double f) {
    for (size_t k = 0; k < c->zoom_fracs.size(); ++k)
      if (c->zoom_fracs[k] == f) return (int)k;
    return -1;
  };
  int missing = 0;
  if (c->zoom_s == s)
    for (double f : fracs) missing += find(f) < 0;
  if (c->zoom_s != s || (int)c->zoom_fracs.size() + missing > kZoomMaxTables) {
    if (!c->zoom_fracs.empty()) HIPCHK(c, hipStreamSynchronize(c->stream));  // windows enqueued so far still read their tables
    c->zoom_fracs.clear();
    c->zoom_carry.clear();
    c->zoom_s = s;
    if (c->zoom_tabs) (void)hipFree(c->zoom_tabs);
    c->zoom_tabs = nullptr;
    c->zoom_cap = 0;
    missing = (int)fracs.size();
  }
  const int used = (int)c->zoom_fracs.size();
  if (used + missing > c->zoom_cap) {  // grow: the tables move, so whatever reads them has to finish first
    int cap = c->zoom_cap ? c->zoom_cap : 4;
    while (cap < used + missing) cap *= 2;
    double* grown = nullptr;
    if (hipMalloc(&grown, (size_t)cap * tab * sizeof(double)) != hipSuccess) {
      (void)hipGetLastError();
      return fail(c, PAOS_EHIP, "paos_zoom_compute: no memory for the phase tables");
    }
    if (used) {
      hipError_t e = hipMemcpyAsync(grown, c->zoom_tabs, (size_t)used * tab * sizeof(double), hipMemcpyDeviceToDevice, c->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(c->stream);  // (everything that read the old pool, then the copy)
      if (e != hipSuccess) {
        (void)hipFree(grown);
        return fail(c, PAOS_EHIP, std::string("paos_zoom_compute: moving the phase tables: ") + hipGetErrorString(e));
      }
    }
    if (c->zoom_tabs) (void)hipFree(c->zoom_tabs);
    c->zoom_tabs = grown;
    c->zoom_cap = cap;
  }
  slots.resize(fracs.size());
  std::vector<double> host(tab);
  for (size_t k = 0; k < fracs.size(); ++k) {
    int slot = find(fracs[k]);
    if (slot < 0) {
      slot = (int)c->zoom_fracs.size();  // (< zoom_cap: room was made above)
      std::vector<int> carry(s);
      int rc = paos_zoom_weights(c->n, s, fracs[k], host.data(), carry.data());
      if (rc) return rc;
      // (a blocking copy into a slot nothing reads yet: the table is on the device before the launches that use it are enqueued)
      HIPCHK(c, hipMemcpy(c->zoom_tabs + (size_t)slot * tab, host.data(), tab * sizeof(double), hipMemcpyHostToDevice));
      c->zoom_fracs.push_back(fracs[k]);
      c->zoom_carry.push_back(std::move(carry));
    }
    slots[k] = slot;
  }
  return PAOS_OK;
}

template <typename T, int STAGE>
void zoom_launch(paos_ctx* c, const ZoomArgs& a, int pt) {
  const dim3 block(64 * kZoomWaves);
  const dim3 grid((a.nd + kZoomWaves - 1) / kZoomWaves, ((a.m >> 4) + pt - 1) / pt, c->batch);
  switch (pt) {
    case 8: hipLaunchKernelGGL((zoom_kernel<T, STAGE, 8>), grid, block, 0, c->stream, a); break;
    case 4: hipLaunchKernelGGL((zoom_kernel<T, STAGE, 4>), grid, block, 0, c->stream, a); break;
    case 2: hipLaunchKernelGGL((zoom_kernel<T, STAGE, 2>), grid, block, 0, c->stream, a); break;
    default: hipLaunchKernelGGL((zoom_kernel<T, STAGE, 1>), grid, block, 0, c->stream, a); break;
  }
}

}  // namespace

extern "C" {

int paos_zoom_compute(paos_ctx* c, int m, int s, const double* centres, int want_field) {
  SETTLE_SCALE(c);  // a deferred stop factor belongs to the field the window is taken of
  if (c) (void)hipSetDevice(c->device);
  if (!c) return fail(c, PAOS_EINVAL, "null context");
  if (!zoom_size_ok(m)) return fail(c, PAOS_EINVAL, std::string("paos_zoom_compute: ") + kZoomBadSize);
  if (s < 1 || s > 64) return fail(c, PAOS_EINVAL, "paos_zoom_compute: the oversampling must be an integer in 1 .. 64");
  if ((long)m > (long)s * c->n) return fail(c, PAOS_EINVAL, "paos_zoom_compute: the window is wider than the grid (m > s n)");
  const int n = c->n, nb = c->batch;
  if (centres)
    for (int i = 0; i < 2 * nb; ++i)
      if (!std::isfinite(centres[i]) || !(centres[i] >= 0.0 && centres[i] < (double)n))
        return fail(c, PAOS_EINVAL, "paos_zoom_compute: the centre of item " + std::to_string(i / 2) + " is not finite or outside [0, n)");
  // scratch and results, allocated on first use and again when the window size changes
  if (c->zoom_m != m) {
    if (c->zoom_m) HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->zoom_t) (void)hipFree(c->zoom_t);
    if (c->zoom_psf) (void)hipFree(c->zoom_psf);
    if (c->zoom_field) (void)hipFree(c->zoom_field);
    c->zoom_t = nullptr;
    c->zoom_psf = nullptr;
    c->zoom_field = nullptr;
    c->zoom_m = 0;
    c->zoom_done = c->zoom_has_field = false;
    if (hipMalloc(&c->zoom_t, (size_t)16 * nb * m * n) != hipSuccess ||
        hipMalloc(&c->zoom_psf, (size_t)8 * nb * m * m) != hipSuccess) {
      (void)hipGetLastError();
      if (c->zoom_t) (void)hipFree(c->zoom_t);
      c->zoom_t = nullptr;
      return fail(c, PAOS_EHIP, "paos_zoom_compute: no memory for the scratch of " + std::to_string((size_t)16 * nb * m * n) + " bytes");
    }
    c->zoom_m = m;
  }
  if (want_field && !c->zoom_field) {
    if (hipMalloc(&c->zoom_field, (size_t)16 * nb * m * m) != hipSuccess) {
      (void)hipGetLastError();
      c->zoom_field = nullptr;
      return fail(c, PAOS_EHIP, "paos_zoom_compute: no memory for the complex windows");
    }
  }
  // per item and axis: the table of the centre's fractional part, then per fine sample the row of its phase in the
  // pool (base) and the grid pixel it sits on or just behind (off)
  std::vector<double> fracs;     // the distinct fractional parts of this call's centres
  std::vector<int> which(2 * nb);  // [item][axis] -> index into fracs
  for (int k = 0; k < 2 * nb; ++k) {
    const double ctr = centres ? centres[k] : (double)(n / 2);
    const double fr = ctr - std::floor(ctr);
    size_t at = 0;
    while (at < fracs.size() && fracs[at] != fr) ++at;
    if (at == fracs.size()) fracs.push_back(fr);
    which[k] = (int)at;
  }
  std::vector<int> slots;
  int rc = zoom_table_slots(c, s, fracs, slots);  // (every slot of the call, before any of them is used)
  if (rc) return rc;
  std::vector<double> par((size_t)nb * 4 * m);
  for (int i = 0; i < nb; ++i)
    for (int axis = 0; axis < 2; ++axis) {
      const double ctr = centres ? centres[2 * i + axis] : (double)(n / 2);
      const double fl = std::floor(ctr);
      const int slot = slots[which[2 * i + axis]];
      const std::vector<int>& carry = c->zoom_carry[slot];
      double* base = par.data() + ((size_t)i * 2 + axis) * 2 * m;
      double* off = base + m;
      for (int q = 0; q < m; ++q) {
        const int t = q - m / 2;
        int a = t >= 0 ? t / s : -((-t + s - 1) / s);  // floor division
        const int b = t - s * a;
        a += carry[b];
        base[q] = (double)(((size_t)slot * s + b) * n);
        off[q] = (double)((((long)fl + a) % n + n) % n);
      }
    }
  rc = arena_reserve(c, par.size());
  if (rc) return rc;
  const double* dpar = nullptr;
  rc = arena_push(c, par.data(), par.size(), &dpar);
  if (rc) return rc;
  ZoomArgs a{};
  a.tabs = c->zoom_tabs;
  a.par = dpar;
  a.n = n;
  a.m = m;
  a.pitch = c->pitch;
  a.item_stride = c->item_stride;
  a.br_shift = c->br == 8 ? 3 : 2;
  static_assert(PAOS_BR == 4 && PAOS_F32_BR == 8, "zoom_load takes the block height as a shift");
  // stage Y: the field -> T
  a.src = c->field;
  a.dst_c = c->zoom_t;
  a.nd = n / 16;
  int pty = 1, ptx = 1;
  rc = paos_zoom_tiles(n, nb, m, &pty, &ptx);  // the one rule of the launch plan, as the host-side query reports it
  if (rc) return rc;
  dispatch_layout(c, [&](auto t, auto) { zoom_launch<decltype(t), 0>(c, a, pty); });
  HIPCHK(c, hipGetLastError());
  // stage X: T -> the windows
  a.src = c->zoom_t;
  a.dst_c = want_field ? c->zoom_field : nullptr;
  a.dst_i = c->zoom_psf;
  a.nd = m / 16;
  zoom_launch<double, 1>(c, a, ptx);
  HIPCHK(c, hipGetLastError());
  c->zoom_done = true;
  c->zoom_has_field = want_field != 0;
  return PAOS_OK;
}

int paos_zoom_fetch(paos_ctx* c, int item, int what, void* host_out) {
  if (c) (void)hipSetDevice(c->device);
  if (!c || !host_out || item < 0 || item >= c->batch || (what != PAOS_ZOOM_PSF && what != PAOS_ZOOM_FIELD))
    return fail(c, PAOS_EINVAL, "paos_zoom_fetch: bad item/what or null buffer");
  if (!c->zoom_done) return fail(c, PAOS_EINVAL, "paos_zoom_fetch: no window computed (paos_zoom_compute first)");
  if (what == PAOS_ZOOM_FIELD && !c->zoom_has_field)
    return fail(c, PAOS_EINVAL, "paos_zoom_fetch: the complex window was not asked for (paos_zoom_compute: want_field)");
  const size_t m2 = (size_t)c->zoom_m * c->zoom_m;
  if (what == PAOS_ZOOM_FIELD) return copy_to_host(c, host_out, c->zoom_field + (size_t)item * m2, m2 * 16);
  return copy_to_host(c, host_out, c->zoom_psf + (size_t)item * m2, m2 * 8);
}

}  // extern "C"
