// phase_tables.h -- the separable phase tables of the generic pass kernel (fft_kernels.h: table_phase, FEAT bit 0;
// opt-in, PAOS_PHASE_TABLES=1) and the kernel that fills them.  Included by the one unit that launches it (passes.hip):
// the kernel is no template, so every unit that saw it would compile a copy.
#pragma once
#include "fft_kernels.h"

namespace paos {

// Fills the tables of one pass program: grid = (ceil(2N / 256), items, tables).  Entry j < N is
// the column factor exp(i sgn A_x(j)), entry N + i the row factor; A = [2 pi] coef fl((g s)^2) as
// an exact double-double product, reduced by the library sincos on the head plus a first-order
// correction for the tail (|tail| <= ulp(head), second order 1e-20).
struct TableJob {
  int block;   // parameter block set
  int kind;    // PWK_QPHASE_C or PWK_QPHASE_N
  int flags;
};
constexpr int kMaxTables = 32;
struct TableArgs {
  const double* blocks;
  cx<double>* tables;
  int batch, n, count;
  TableJob jobs[kMaxTables];
};

static __global__ void phase_table_kernel(TableArgs a) {
  const int item = blockIdx.y, tb = blockIdx.z;
  const TableJob job = a.jobs[tb];
  const double* p = a.blocks + ((size_t)job.block * a.batch + item) * FP_STRIDE;
  if (p[FP_ENABLE] == 0.0) return;
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= 2 * a.n) return;
  const int idx = j < a.n ? j : j - a.n;
  const int g = job.kind == PWK_QPHASE_C ? idx - a.n / 2 : (idx < a.n / 2 ? idx : idx - a.n);
  const double w = (double)g * (j < a.n ? p[FP_SX] : p[FP_SY]);
  const double X = __dmul_rn(w, w);
  double hi = __dmul_rn(p[FP_COEF], X);
  double lo = fma(p[FP_COEF], X, -hi);
  if (job.flags & PWF_MUL2PI) {
    const double h2 = __dmul_rn(6.283185307179586, hi);
    lo = fma(6.283185307179586, hi, -h2) + 6.283185307179586 * lo;
    hi = h2;
  }
  double sn, cs;
  sincos(hi, &sn, &cs);
  const double c2 = fma(-lo, sn, cs), s2 = fma(lo, cs, sn);
  a.tables[((size_t)tb * a.batch + item) * 2 * a.n + j] = {c2, p[FP_SGN] * s2};
}

}  // namespace paos
