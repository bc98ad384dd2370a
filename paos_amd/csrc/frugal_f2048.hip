// frugal_f2048.hip -- the frugal pass kernels of 2048^2 complex64.
#include "frugal_launch.h"

template <>
int frugal_family<float, 2048>(paos_ctx* c, const FrugalBuild& b, const FrugalArgs& a, bool narrow) { return frugal_dispatch<float, 2048>(c, b, a, narrow); }
