// frugal_f4096.hip -- the frugal pass kernels of 4096^2 complex64.
#include "frugal_launch.h"

template <>
int frugal_family<float, 4096>(paos_ctx* c, const FrugalBuild& b, const FrugalArgs& a, bool narrow) { return frugal_dispatch<float, 4096>(c, b, a, narrow); }
