// frugal_d4096.hip -- the frugal pass kernels of 4096^2 complex128.
#include "frugal_launch.h"

int paos_frugal_d4096(paos_ctx* c, const FrugalArgs& a, int axis, int kpre, int kmid, int nfft) {
  return frugal_axis<double, 4096>(c, a, axis, kpre, kmid, nfft);
}
