// frugal_d2048.hip -- the frugal pass kernels of 2048^2 complex128.
#include "frugal_launch.h"

template <>
int frugal_family<double, 2048>(paos_ctx* c, const FrugalBuild& b, const FrugalArgs& a, bool narrow) { return frugal_dispatch<double, 2048>(c, b, a, narrow); }
