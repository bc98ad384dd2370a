// frugal_f4096.hip -- the frugal pass kernels of 4096^2 complex64.
#include "frugal_launch.h"

int paos_frugal_f4096(paos_ctx* c, const FrugalArgs& a, int axis, int kpre, int kmid, int nfft) {
  return frugal_axis<float, 4096>(c, a, axis, kpre, kmid, nfft);
}
