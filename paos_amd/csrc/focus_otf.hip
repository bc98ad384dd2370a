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

// ---- through-focus stacks: the out-of-place passes of focus_pass.h ----------------------
// the generic pass kernel's geometry (FftCfg: one tile shape per grid size and type, 64 .. 4096)
template <typename T, int N, int AXIS>
int focus_launch(paos_ctx* c, const FocusArgs& a) {
  using C = FftCfg<T, N>;
  constexpr int LINES = AXIS == 0 ? C::ROW_LINES : C::COL_LINES;
  constexpr int TILES = AXIS == 0 ? C::ROW_TILES : C::COL_TILES;
  constexpr bool SPLIT = AXIS == 0 ? C::ROW_SPLIT : C::COL_SPLIT;
  const dim3 grid(N / LINES / TILES, c->batch), block(TILES * LINES * N / C::E);
  const size_t lds = (size_t)TILES * LINES * line_lds_bytes<T, N, SPLIT>();
  // for the launch timer: a full pass -- every line of every item is loaded, transformed once and stored
  c->prof_next_tag = 0;
  c->prof_next_bytes = (double)c->batch * N * N * 2.0 * (double)elem_bytes(c);
  c->prof_next_lines = (double)c->batch * N;
  return TIMED_LAUNCH(c, focus_pass_kernel<T, N, C::E, LINES, TILES, AXIS, C::BR, C::BC, SPLIT, C::MINW>, grid, block, lds,
                      generic_lds_opt_in(lds), AXIS == 0 ? PAOS_KERNEL_PASS_ROWS : PAOS_KERNEL_PASS_COLS, 0, a);
}

template <typename T>
int focus_pass_t(paos_ctx* c, int axis, const FocusArgs& a) {
  return dispatch_n(c, [&](auto n) {
    constexpr int N = decltype(n)::value;
    return axis == 0 ? focus_launch<T, N, 0>(c, a) : focus_launch<T, N, 1>(c, a);
  });
}

int focus_pass(paos_ctx* c, int axis, int mode, const void* src, void* dst, const double* dparams) {
  FocusArgs a{};
  a.src = src; a.dst = dst; a.tw = c->tw; a.params = dparams;
  a.scale = 1.0 / c->n;
  a.mode = mode;
  a.pitch = c->pitch; a.item_stride = c->item_stride;
  return c->precision == PAOS_F64 ? focus_pass_t<double>(c, axis, a) : focus_pass_t<float>(c, axis, a);
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
// the generic pass kernel's geometry again; rows: the N/2 packed lines, columns: 0 .. N/2 rounded up to whole workgroups
template <typename T, int N, int AXIS>
int otf_launch(paos_ctx* c, const OtfArgs& a) {
  using C = FftCfg<T, N>;
  constexpr int LINES = AXIS == 0 ? C::ROW_LINES : C::COL_LINES;
  constexpr int TILES = AXIS == 0 ? C::ROW_TILES : C::COL_TILES;
  constexpr bool SPLIT = AXIS == 0 ? C::ROW_SPLIT : C::COL_SPLIT;
  constexpr int PER_WG = LINES * TILES;
  constexpr int WGS = AXIS == 0 ? N / 2 / PER_WG : (N / 2 + 1 + PER_WG - 1) / PER_WG;
  const dim3 grid(WGS, c->batch), block(TILES * LINES * N / C::E);
  const size_t lds = (size_t)TILES * LINES * line_lds_bytes<T, N, SPLIT>();
  auto kern = [] {
    if constexpr (AXIS == 0) return otf_row_kernel<T, N, C::E, LINES, TILES, C::BR, C::BC, SPLIT, C::MINW>;
    else return otf_col_kernel<T, N, C::E, LINES, TILES, C::BR, C::BC, SPLIT, C::MINW>;
  }();
  // for the launch timer: the lines the launch transforms (the column launch: those of its last workgroup that lie beyond
  // column N/2 included) and the bytes it moves (rows: N/2 x 2 PSF rows in, N/2 lines out; columns: N/2 rows of the
  // column and of its mirror in, N rows out)
  const double eb = (double)elem_bytes(c);
  c->prof_next_tag = 0;
  c->prof_next_lines = (double)c->batch * WGS * PER_WG;
  c->prof_next_bytes = AXIS == 0 ? (double)c->batch * N * (N * 8.0 + N / 2 * eb) : (double)c->batch * (N / 2 + 1) * 2.0 * N * eb;
  return TIMED_LAUNCH(c, kern, grid, block, lds, generic_lds_opt_in(lds), AXIS == 0 ? PAOS_KERNEL_PASS_ROWS : PAOS_KERNEL_PASS_COLS, 0, a);
}

template <typename T>
int otf_pass_t(paos_ctx* c, int axis, const OtfArgs& a) {
  return dispatch_n(c, [&](auto n) {
    constexpr int N = decltype(n)::value;
    return axis == 0 ? otf_launch<T, N, 0>(c, a) : otf_launch<T, N, 1>(c, a);
  });
}

int otf_pass(paos_ctx* c, int axis) {
  OtfArgs a{};
  a.psf = c->psf; a.spec = c->otf_spec; a.tw = c->tw;
  a.pitch = c->pitch; a.item_stride = c->item_stride;
  return c->precision == PAOS_F64 ? otf_pass_t<double>(c, axis, a) : otf_pass_t<float>(c, axis, a);
}

// fetch and cuts share their preconditions
int otf_ready(paos_ctx* c, const char* who) {
  if (!c->otf_spec || !c->otf_computed) return fail(c, PAOS_EINVAL, std::string(who) + ": no transfer functions computed (paos_otf_compute)");
  if (!c->otf_valid)
    return fail(c, PAOS_EINVAL, std::string(who) + ": the PSFs were stored anew since paos_otf_compute: the transfer functions are stale (compute again)");
  return PAOS_OK;
}

// ---- blurred PSFs: the packed real-output passes of blur_pass.h ---------------------------
// otf_launch's geometry; columns first (spectrum -> PSF buffer), then the N/2 packed lines in place on the PSF buffer
template <typename T, int N, int AXIS>
int blur_launch(paos_ctx* c, const BlurArgs& a) {
  using C = FftCfg<T, N>;
  constexpr int LINES = AXIS == 0 ? C::ROW_LINES : C::COL_LINES;
  constexpr int TILES = AXIS == 0 ? C::ROW_TILES : C::COL_TILES;
  constexpr bool SPLIT = AXIS == 0 ? C::ROW_SPLIT : C::COL_SPLIT;
  constexpr int PER_WG = LINES * TILES;
  constexpr int WGS = AXIS == 0 ? N / 2 / PER_WG : (N / 2 + 1 + PER_WG - 1) / PER_WG;
  const dim3 grid(WGS, c->batch), block(TILES * LINES * N / C::E);
  const size_t lds = (size_t)TILES * LINES * line_lds_bytes<T, N, SPLIT>();
  auto kern = [] {
    if constexpr (AXIS == 0) return blur_row_kernel<T, N, C::E, LINES, TILES, C::BR, C::BC, SPLIT, C::MINW>;
    else return blur_col_kernel<T, N, C::E, LINES, TILES, C::BR, C::BC, SPLIT, C::MINW>;
  }();
  // for the launch timer: the lines the launch transforms (columns: those of the last workgroup beyond N/2 included) and
  // the bytes it moves (columns: N/2 + 1 columns of the spectrum in and out, N columns of doubles out; rows: the PSF in and out)
  const double eb = (double)elem_bytes(c);
  c->prof_next_tag = 0;
  c->prof_next_lines = (double)c->batch * WGS * PER_WG;
  c->prof_next_bytes = AXIS == 0 ? (double)c->batch * N * N * 16.0 : (double)c->batch * N * ((N / 2 + 1) * 2.0 * eb + N * 8.0);
  return TIMED_LAUNCH(c, kern, grid, block, lds, generic_lds_opt_in(lds), AXIS == 0 ? PAOS_KERNEL_PASS_ROWS : PAOS_KERNEL_PASS_COLS, 0, a);
}

template <typename T>
int blur_pass_t(paos_ctx* c, int axis, const BlurArgs& a) {
  return dispatch_n(c, [&](auto n) {
    constexpr int N = decltype(n)::value;
    return axis == 0 ? blur_launch<T, N, 0>(c, a) : blur_launch<T, N, 1>(c, a);
  });
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
  for (int axis = 1; axis >= 0; --axis) {
    rc = c->precision == PAOS_F64 ? blur_pass_t<double>(c, axis, a) : blur_pass_t<float>(c, axis, a);
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
  if (c->precision == PAOS_F64)
    hipLaunchKernelGGL((otf_fetch_kernel<double, BR, Lay<double>::BC>), grid, block, 0, c->stream,
                       (const cx<double>*)c->otf_spec + (size_t)item * c->item_stride, c->staging, c->n, c->pitch, cplx);
  else
    F32_BR_SWITCH(c, hipLaunchKernelGGL((otf_fetch_kernel<float, FBR, Lay<float>::BC>), grid, block, 0, c->stream,
                       (const cx<float>*)c->otf_spec + (size_t)item * c->item_stride, c->staging, c->n, c->pitch, cplx));
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
  if (c->precision == PAOS_F64)
    hipLaunchKernelGGL((otf_cuts_kernel<double, BR, Lay<double>::BC>), grid, block, 0, c->stream,
                       (const cx<double>*)c->otf_spec, c->otf_cuts, c->n, c->pitch, c->item_stride);
  else
    F32_BR_SWITCH(c, hipLaunchKernelGGL((otf_cuts_kernel<float, FBR, Lay<float>::BC>), grid, block, 0, c->stream,
                       (const cx<float>*)c->otf_spec, c->otf_cuts, c->n, c->pitch, c->item_stride));
  HIPCHK(c, hipGetLastError());
  return copy_to_host(c, host_out, c->otf_cuts, bytes);
}

}  // extern "C"
