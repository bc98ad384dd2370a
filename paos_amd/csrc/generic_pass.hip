// generic_pass.hip -- the generic pass kernel (fft_kernels.h: fused_pass_kernel) for every grid size and both types:
// the passes the frugal kernels do not serve (N < 1024, complex64 below 2048, unusual operator lists).
#include "host.h"

namespace {

template <typename T, int N, int AXIS, int FEAT>
int pass_launch(paos_ctx* c, const PassArgs& a) {
  using C = FftCfg<T, N>;
  constexpr int BC = C::BC;
  constexpr int LINES = AXIS == 0 ? C::ROW_LINES : C::COL_LINES;
  constexpr int TILES = AXIS == 0 ? C::ROW_TILES : C::COL_TILES;
  constexpr bool SPLIT = AXIS == 0 ? C::ROW_SPLIT : C::COL_SPLIT;
  const dim3 grid(N / LINES / TILES, a.batch), block(TILES * LINES * N / C::E);  // (a.batch: c->batch, or 1 for the PSD scratch item)
  const size_t lds = (size_t)TILES * LINES * line_lds_bytes<T, N, SPLIT>();
  // (the attribute belongs to the device's copy of the function; one process may drive several GPUs: opt_in_lds)
  return TIMED_LAUNCH(c, fused_pass_kernel<T, N, C::E, LINES, TILES, AXIS, C::BR, BC, SPLIT, C::MINW, 1, 0, FEAT>, grid, block, lds,
                      generic_lds_opt_in(lds), AXIS == 0 ? PAOS_KERNEL_PASS_ROWS : PAOS_KERNEL_PASS_COLS, 0, a);
}

template <typename T>
int pass_t(paos_ctx* c, int axis, const PassArgs& a, int feat) {
  return dispatch_n(c, [&](auto n) {
    constexpr int N = decltype(n)::value;
    if (feat) return axis == 0 ? pass_launch<T, N, 0, 3>(c, a) : pass_launch<T, N, 1, 3>(c, a);
    return axis == 0 ? pass_launch<T, N, 0, 0>(c, a) : pass_launch<T, N, 1, 0>(c, a);
  });
}

}  // namespace

int generic_pass(paos_ctx* c, int axis, const PassArgs& a, int feat) {
  return dispatch_layout(c, [&](auto t, auto) { return pass_t<decltype(t)>(c, axis, a, feat); });
}
