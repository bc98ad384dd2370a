// frugal_f2048.hip -- the frugal pass kernels of 2048^2 complex64.
#include "frugal_launch.h"

int paos_frugal_f2048(paos_ctx* c, const FrugalArgs& a, int axis, int kpre, int kmid, int nfft) {
  return frugal_axis<float, 2048>(c, a, axis, kpre, kmid, nfft);
}
