// focus_otf.hip -- the products that run on the generic pass kernel's tile shapes (FftCfg): through-focus stacks
// (paos_focus_*, the out-of-place passes of focus_pass.h), the transfer functions of the kept PSFs (paos_otf_*, the packed
// real-input passes of otf_pass.h) and the blurred PSFs made from those spectra (paos_blur_*, the packed real-output passes
// of blur_pass.h).  One unit for focus and OTF: compiled on its own, otf_pass.h's complex128 kernels come out with
// the operands of some additions exchanged (same results, other bytes; profiles/r10_unit_split.md).
#include "host.h"

#include <algorithm>
#include <cmath>

#include "blur_pass.h"
#include "focus_pass.h"
#include "otf_pass.h"

namespace {

// ---- one launcher for the passes of all three products ---------------------------------------------------------------
// The generic pass kernel's tile along AXIS (FftCfg: one tile shape per grid size and type, 64 .. 4096)
template <typename T_, int N_, int AXIS_>
struct Tile {
  using T = T_;
  using C = FftCfg<T, N_>;
  static constexpr int N = N_, AXIS = AXIS_;
  static constexpr int LINES = AXIS == 0 ? C::ROW_LINES : C::COL_LINES;
  static constexpr int TILES = AXIS == 0 ? C::ROW_TILES : C::COL_TILES;
  static constexpr bool SPLIT = AXIS == 0 ? C::ROW_SPLIT : C::COL_SPLIT;
  static constexpr int PER_WG = LINES * TILES;  // lines per workgroup
};
// One pass of a product on those tiles.  What differs between the products is passed in: kernel(Tile<..>{}), the kernel's
// build for the tile; `lines`, how many lines along `axis` the launch has to cover (whole workgroups: the grid along x);
// `bytes`, what the launch moves, for the launch timer (its lines: those of whole workgroups)
template <typename Kernel, typename Args>
int tile_pass(paos_ctx* c, int axis, int lines, double bytes, Kernel kernel, const Args& a) {
  return dispatch_layout(c, [&](auto t, auto) {
    return dispatch_n(c, [&](auto n) {
      return dispatch_either<0, 1>(axis == 0, [&](auto ax) {
        using L = Tile<decltype(t), decltype(n)::value, decltype(ax)::value>;
        const int wgs = (lines + L::PER_WG - 1) / L::PER_WG;
        const dim3 grid(wgs, c->batch), block(L::PER_WG * L::N / L::C::E);
        const size_t lds = (size_t)L::PER_WG * line_lds_bytes<typename L::T, L::N, L::SPLIT>();
        c->prof_next_tag = 0;
        c->prof_next_bytes = bytes;
        c->prof_next_lines = (double)c->batch * wgs * L::PER_WG;
        return TIMED_LAUNCH(c, kernel(L{}), grid, block, lds, generic_lds_opt_in(lds),
                            L::AXIS == 0 ? PAOS_KERNEL_PASS_ROWS : PAOS_KERNEL_PASS_COLS, 0, a);
      });
    });
  });
}
// the packed real passes (OTF, blur): rows: the N/2 packed lines, columns: 0 .. N/2 (rounded up to whole workgroups)
int packed_lines(const paos_ctx* c, int axis) { return axis == 0 ? c->n / 2 : c->n / 2 + 1; }

// ---- through-focus stacks: the out-of-place passes of focus_pass.h ----------------------
int focus_pass(paos_ctx* c, int axis, int mode, const void* src, void* dst, const double* dparams) {
  FocusArgs a{};
  a.src = src; a.dst = dst; a.tw = c->tw; a.params = dparams;
  a.scale = 1.0 / c->n;
  a.mode = mode;
  a.pitch = c->pitch; a.item_stride = c->item_stride;
  // a full pass -- every line of every item is loaded, transformed once and stored
  return tile_pass(c, axis, c->n, (double)c->batch * c->n * c->n * 2.0 * (double)elem_bytes(c), [](auto tile) {
    using L = decltype(tile);
    using C = typename L::C;
    return focus_pass_kernel<typename L::T, L::N, C::E, L::LINES, L::TILES, L::AXIS, C::BR, C::BC, L::SPLIT, C::MINW>;
  }, a);
}

}  // namespace

extern "C" {

// ---- through-focus stacks (include/paos_hip.h) --------------------------------------------
int paos_focus_begin(paos_ctx* c) {
  SETTLE_SCALE(c);  // a deferred stop factor belongs to the field the spectrum is taken of
  if (c) (void)hipSetDevice(c->device);
  if (!c) return fail(c, PAOS_EINVAL, "null context");
  if (c->focus_open) return fail(c, PAOS_EINVAL, "paos_focus_begin: a focus stack is already open (paos_focus_end first)");
  if (!c->focus_spec) HIPCHK(c, hipMalloc(&c->focus_spec, (size_t)c->item_stride * c->batch * elem_bytes(c)));
  int rc = focus_pass(c, 0, FOCUS_FORWARD, c->field, c->focus_spec, nullptr);
  if (rc) return rc;
  rc = focus_pass(c, 1, FOCUS_FORWARD, c->focus_spec, c->focus_spec, nullptr);
  if (rc) return rc;
  c->focus_open = true;
  return PAOS_OK;
}

int paos_focus_plane(paos_ctx* c, const double* params) {
  if (c) (void)hipSetDevice(c->device);
  if (!c || !params) return fail(c, PAOS_EINVAL, "null argument");
  if (!c->focus_open) return fail(c, PAOS_EINVAL, "paos_focus_plane: no focus stack is open (paos_focus_begin first)");
  for (int i = 0; i < c->batch; ++i)
    for (int k = 0; k < FP_STRIDE; ++k)
      if (!std::isfinite(params[(size_t)i * FP_STRIDE + k]))
        return fail(c, PAOS_EINVAL, "paos_focus_plane: non-finite parameter of item " + std::to_string(i));
  DROP_SCALE(c);  // the field is overwritten: what the context knew about it (its power, a pending factor) is void
  const double* dparams = nullptr;
  int rc = arena_push(c, params, (size_t)c->batch * FP_STRIDE, &dparams);
  if (rc) return rc;
  rc = focus_pass(c, 1, FOCUS_TRANSFER, c->focus_spec, c->field, dparams);
  if (rc) return rc;
  return focus_pass(c, 0, FOCUS_INVERSE, c->field, c->field, nullptr);
}

int paos_focus_end(paos_ctx* c) {
  if (c) (void)hipSetDevice(c->device);
  if (!c) return fail(c, PAOS_EINVAL, "null context");
  if (!c->focus_open) return fail(c, PAOS_EINVAL, "paos_focus_end: no focus stack is open");
  HIPCHK(c, hipStreamSynchronize(c->stream));  // the planes enqueued so far still read the spectrum
  HIPCHK(c, hipFree(c->focus_spec));
  c->focus_spec = nullptr;
  c->focus_open = false;
  return PAOS_OK;
}

}  // extern "C"

namespace {

constexpr int kThreads = 256;  // per workgroup of the fetch and cut sweeps

// ---- transfer functions: the packed real-input passes of otf_pass.h -----------------------
int otf_pass(paos_ctx* c, int axis) {
  OtfArgs a{};
  a.psf = c->psf; a.spec = c->otf_spec; a.tw = c->tw;
  a.pitch = c->pitch; a.item_stride = c->item_stride;
  // the bytes it moves: rows: N/2 x 2 PSF rows in, N/2 lines out; columns: N/2 rows of the column and of its mirror in, N rows out
  const double n = c->n, eb = (double)elem_bytes(c);
  const double bytes = axis == 0 ? c->batch * n * (n * 8.0 + c->n / 2 * eb) : c->batch * (double)(c->n / 2 + 1) * 2.0 * n * eb;
  return tile_pass(c, axis, packed_lines(c, axis), bytes, [](auto tile) {
    using L = decltype(tile);
    using C = typename L::C;
    if constexpr (L::AXIS == 0) return otf_row_kernel<typename L::T, L::N, C::E, L::LINES, L::TILES, C::BR, C::BC, L::SPLIT, C::MINW>;
    else return otf_col_kernel<typename L::T, L::N, C::E, L::LINES, L::TILES, C::BR, C::BC, L::SPLIT, C::MINW>;
  }, a);
}

// fetch and cuts share their preconditions
int otf_ready(paos_ctx* c, const char* who) {
  if (!c->otf_spec || !c->otf_computed) return fail(c, PAOS_EINVAL, std::string(who) + ": no transfer functions computed (paos_otf_compute)");
  if (!c->otf_valid)
    return fail(c, PAOS_EINVAL, std::string(who) + ": the PSFs were stored anew since paos_otf_compute: the transfer functions are stale (compute again)");
  return PAOS_OK;
}

// ---- blurred PSFs: the packed real-output passes of blur_pass.h ---------------------------
// columns first (spectrum -> PSF buffer), then the N/2 packed lines in place on the PSF buffer
int blur_pass(paos_ctx* c, int axis, const BlurArgs& a) {
  // the bytes it moves: columns: N/2 + 1 columns of the spectrum in and out, N columns of doubles out; rows: the PSF in and out
  const double n = c->n, eb = (double)elem_bytes(c);
  const double bytes = axis == 0 ? c->batch * n * n * 16.0 : c->batch * n * ((c->n / 2 + 1) * 2.0 * eb + n * 8.0);
  return tile_pass(c, axis, packed_lines(c, axis), bytes, [](auto tile) {
    using L = decltype(tile);
    using C = typename L::C;
    if constexpr (L::AXIS == 0) return blur_row_kernel<typename L::T, L::N, C::E, L::LINES, L::TILES, C::BR, C::BC, L::SPLIT, C::MINW>;
    else return blur_col_kernel<typename L::T, L::N, C::E, L::LINES, L::TILES, C::BR, C::BC, L::SPLIT, C::MINW>;
  }, a);
}

// why paos_blur_table refuses (n, d, sigma, pixel), or null
const char* blur_table_refusal(int n, double d, double sigma, double pixel) {
  if (n < 2 || (n & 1) || n > (1 << 20)) return "n must be even, 2 .. 2^20";
  if (!std::isfinite(d) || !(d > 0.0)) return "the pitch must be finite and positive";
  if (!std::isfinite(sigma) || sigma < 0.0) return "sigma must be finite and >= 0";
  if (!std::isfinite(pixel) || pixel < 0.0) return "the pixel width must be finite and >= 0";
  return nullptr;
}

}  // namespace

extern "C" {

// ---- blurred PSFs (include/paos_hip.h) ------------------------------------------------------
int paos_blur_table(int n, double d, double sigma, double pixel, double* t) {
  if (const char* why = blur_table_refusal(n, d, sigma, pixel)) return fail(nullptr, PAOS_EINVAL, std::string("paos_blur_table: ") + why);
  if (!t) return fail(nullptr, PAOS_EINVAL, "paos_blur_table: null argument");
  const long double pi = 3.141592653589793238462643383279502884L;
  const long double s = (long double)sigma, p = (long double)pixel, nd = (long double)n * (long double)d;
  for (int m = 0; m <= n / 2; ++m) {
    const long double f = (long double)m / nd;
    const long double x = pi * (p * f);
    const long double sinc = x == 0.0L ? 1.0L : sinl(x) / x;
    t[m] = (double)(expl(-2.0L * pi * pi * (s * s) * (f * f)) * sinc);
  }
  return PAOS_OK;
}

int paos_blur_apply(paos_ctx* c, const double* per_item) {
  if (c) (void)hipSetDevice(c->device);
  if (!c || !per_item) return fail(c, PAOS_EINVAL, "paos_blur_apply: null argument");
  int rc = otf_ready(c, "paos_blur_apply");
  if (rc) return rc;
  for (int i = 0; i < c->batch; ++i) {
    const double* q = per_item + (size_t)i * PAOS_BLUR_ITEM;  // dx, dy, sigma_x, sigma_y, pixel_x, pixel_y
    for (int ax = 0; ax < 2; ++ax)
      if (const char* why = blur_table_refusal(c->n, q[ax], q[2 + ax], q[4 + ax]))
        return fail(c, PAOS_EINVAL, "paos_blur_apply: item " + std::to_string(i) + (ax ? ", y: " : ", x: ") + why);
  }
  const int len = c->n / 2 + 1;
  std::vector<double>& tabs = c->blur_tabs;
  if (tabs.empty()) {
    tabs.resize((size_t)c->batch * 2 * len);
    c->blur_key.assign((size_t)c->batch * 2 * 3, -1.0);  // (no table is evaluated for a negative d)
  }
  for (int i = 0; i < c->batch; ++i) {
    const double* q = per_item + (size_t)i * PAOS_BLUR_ITEM;
    for (int ax = 0; ax < 2; ++ax) {
      double* key = c->blur_key.data() + ((size_t)i * 2 + ax) * 3;
      if (key[0] == q[ax] && key[1] == q[2 + ax] && key[2] == q[4 + ax]) continue;  // the table kept is this one
      key[0] = -1.0;
      rc = paos_blur_table(c->n, q[ax], q[2 + ax], q[4 + ax], tabs.data() + ((size_t)i * 2 + ax) * len);
      if (rc) return rc;
      key[0] = q[ax]; key[1] = q[2 + ax]; key[2] = q[4 + ax];
    }
  }
  rc = arena_reserve(c, tabs.size());
  if (rc) return rc;
  const double* dtabs = nullptr;
  rc = arena_push(c, tabs.data(), tabs.size(), &dtabs);
  if (rc) return rc;
  BlurArgs a{};
  a.psf = c->psf; a.spec = c->otf_spec; a.tw = c->tw; a.tabs = dtabs;
  a.scale = 1.0 / ((double)c->n * (double)c->n);
  a.pitch = c->pitch; a.item_stride = c->item_stride;
  // the PSF buffer is rewritten as a whole: what the context knew about zeros in it (the dead-tile memo of the storing
  // passes) is void.  The spectrum is rewritten along with it, so the transfer functions stay valid: those of P'.
  c->psf_zero_axis = -1;
  c->ee_valid = false;  // (energy curves read the PSFs themselves: those of P are stale)
  for (int axis = 1; axis >= 0; --axis) {
    rc = blur_pass(c, axis, a);
    if (rc) {
      c->otf_valid = false;  // (a launch failed half way: neither buffer is to be trusted)
      return rc;
    }
  }
  return PAOS_OK;
}

// ---- transfer functions (include/paos_hip.h) ------------------------------------------------
int paos_otf_compute(paos_ctx* c) {
  if (c) (void)hipSetDevice(c->device);
  if (!c) return fail(c, PAOS_EINVAL, "null context");
  if (!c->psf) return fail(c, PAOS_EINVAL, "paos_otf_compute: no PSF kept (paos_psf_keep)");
  if (!c->otf_spec) HIPCHK(c, hipMalloc(&c->otf_spec, (size_t)c->item_stride * c->batch * elem_bytes(c)));
  c->otf_valid = false;
  int rc = otf_pass(c, 0);
  if (rc) return rc;
  rc = otf_pass(c, 1);
  if (rc) return rc;
  c->otf_computed = c->otf_valid = true;
  return PAOS_OK;
}

int paos_otf_fetch(paos_ctx* c, int item, int what, void* host_out) {
  if (c) (void)hipSetDevice(c->device);
  if (!c || !host_out || item < 0 || item >= c->batch || (what != PAOS_OTF_MTF && what != PAOS_OTF_COMPLEX))
    return fail(c, PAOS_EINVAL, "paos_otf_fetch: bad item/what or null buffer");
  int rc = otf_ready(c, "paos_otf_fetch");
  if (rc) return rc;
  const int cplx = what == PAOS_OTF_COMPLEX;
  const size_t n2 = (size_t)c->n * c->n;
  const dim3 grid((unsigned)std::min<size_t>((n2 + kThreads - 1) / kThreads, 2048)), block(kThreads);
  dispatch_layout(c, [&](auto t, auto br) {
    using T = decltype(t);
    hipLaunchKernelGGL((otf_fetch_kernel<T, decltype(br)::value, Lay<T>::BC>), grid, block, 0, c->stream,
                       (const cx<T>*)c->otf_spec + (size_t)item * c->item_stride, c->staging, c->n, c->pitch, cplx);
  });
  HIPCHK(c, hipGetLastError());
  return copy_to_host(c, host_out, c->staging, n2 * (cplx ? 16 : 8));
}

int paos_otf_cuts(paos_ctx* c, double* host_out) {
  if (c) (void)hipSetDevice(c->device);
  if (!c || !host_out) return fail(c, PAOS_EINVAL, "paos_otf_cuts: null argument");
  int rc = otf_ready(c, "paos_otf_cuts");
  if (rc) return rc;
  const int len = c->n / 2 + 1;
  const size_t bytes = (size_t)c->batch * 2 * len * sizeof(double);
  if (!c->otf_cuts) HIPCHK(c, hipMalloc(&c->otf_cuts, bytes));
  const dim3 grid((2 * len + kThreads - 1) / kThreads, c->batch), block(kThreads);
  dispatch_layout(c, [&](auto t, auto br) {
    using T = decltype(t);
    hipLaunchKernelGGL((otf_cuts_kernel<T, decltype(br)::value, Lay<T>::BC>), grid, block, 0, c->stream, (const cx<T>*)c->otf_spec,
                       c->otf_cuts, c->n, c->pitch, c->item_stride);
  });
  HIPCHK(c, hipGetLastError());
  return copy_to_host(c, host_out, c->otf_cuts, bytes);
}

}  // extern "C"
