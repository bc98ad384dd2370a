// frugal_d1024.hip -- the frugal pass kernels of 1024^2 complex128.
#include "frugal_launch.h"

template <>
int frugal_family<double, 1024>(paos_ctx* c, const FrugalBuild& b, const FrugalArgs& a, bool narrow) { return frugal_dispatch<double, 1024>(c, b, a, narrow); }
