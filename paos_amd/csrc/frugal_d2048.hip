// frugal_d2048.hip -- the frugal pass kernels of 2048^2 complex128.
#include "frugal_launch.h"

int paos_frugal_d2048(paos_ctx* c, const FrugalArgs& a, int axis, int kpre, int kmid, int nfft) {
  return frugal_axis<double, 2048>(c, a, axis, kpre, kmid, nfft);
}
