// frugal_d1024.hip -- the frugal pass kernels of 1024^2 complex128.
#include "frugal_launch.h"

int paos_frugal_d1024(paos_ctx* c, const FrugalArgs& a, int axis, int kpre, int kmid, int nfft) {
  return frugal_axis<double, 1024>(c, a, axis, kpre, kmid, nfft);
}
