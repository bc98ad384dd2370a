// frugal_d4096.hip -- the frugal pass kernels of 4096^2 complex128.
#include "frugal_launch.h"

template <>
int frugal_family<double, 4096>(paos_ctx* c, const FrugalBuild& b, const FrugalArgs& a, bool narrow) { return frugal_dispatch<double, 4096>(c, b, a, narrow); }
