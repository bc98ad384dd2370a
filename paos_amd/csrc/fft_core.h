// fft_core.h -- register-radix Stockham FFT building blocks for gfx950 (CDNA4).
//
// One "line" (a row or a column of the N x N field) is transformed by N/E
// threads that hold E complex elements each in VGPRs.  Every stage is a radix-E
// (last stage: the remaining radix) DFT done entirely in registers; between
// stages the line is exchanged through LDS with the Stockham auto-sort index
// map, so the result comes out in natural order and the first load / last store
// hit global memory with unit stride across lanes.  No MFMA: a c128 FFT has
// ~2 flop/byte, far below the machine balance, so the pass is HBM-bound and the
// job of this file is to keep every global access a full 128-byte line.
//
// Replaces, on the GPU, numpy.fft.fft2 / ifft2 as called by the reference at
// paos/classes/wfo.py:462-472 (ptp), :493-509 (stw), :535-545 (wts).
#pragma once
#include <hip/hip_runtime.h>

namespace paos {

template <typename T>
struct cx {
  T x, y;
};

template <typename T>
__device__ __forceinline__ cx<T> cadd(cx<T> a, cx<T> b) { return {a.x + b.x, a.y + b.y}; }
template <typename T>
__device__ __forceinline__ cx<T> csub(cx<T> a, cx<T> b) { return {a.x - b.x, a.y - b.y}; }
template <typename T>
__device__ __forceinline__ cx<T> cmul(cx<T> a, cx<T> b) {
  return {fma(a.x, b.x, -(a.y * b.y)), fma(a.x, b.y, a.y * b.x)};
}
template <typename T>
__device__ __forceinline__ cx<T> cconj(cx<T> a) { return {a.x, -a.y}; }
// a - i b, a + i b, and (re, im) -> (p.x re + q.x im_or_re ...) helpers used by the butterflies:
template <typename T>
__device__ __forceinline__ cx<T> sub_ib(cx<T> a, cx<T> b) { return {a.x + b.y, a.y - b.x}; }
template <typename T>
__device__ __forceinline__ cx<T> add_ib(cx<T> a, cx<T> b) { return {a.x - b.y, a.y + b.x}; }
// a + c b and a - c b for a real c (FMA)
template <typename T>
__device__ __forceinline__ cx<T> fma_real(T c, cx<T> b, cx<T> a) { return {fma(c, b.x, a.x), fma(c, b.y, a.y)}; }
// (b.x - tau b.y, b.y + tau b.x) = b (1 + i tau)
template <typename T>
__device__ __forceinline__ cx<T> rot_tau(cx<T> b, T tau) { return {fma(-tau, b.y, b.x), fma(tau, b.x, b.y)}; }
// a - i c b and a + i c b for a real c
template <typename T>
__device__ __forceinline__ cx<T> fma_mic(T c, cx<T> b, cx<T> a) { return {fma(c, b.y, a.x), fma(-c, b.x, a.y)}; }
template <typename T>
__device__ __forceinline__ cx<T> fma_pic(T c, cx<T> b, cx<T> a) { return {fma(-c, b.y, a.x), fma(c, b.x, a.y)}; }
// v (c + i s) for compile-time c, s
template <typename T>
__device__ __forceinline__ cx<T> cmul_const(cx<T> v, T c, T s) { return {fma(v.x, c, -(v.y * s)), fma(v.x, s, v.y * c)}; }
// (v.x p, v.y q)
template <typename T>
__device__ __forceinline__ cx<T> scale2(cx<T> v, T p, T q) { return {v.x * p, v.y * q}; }

// ---- complex64 on the packed fp32 pipe --------------------------------------------------------
// A complex64 value is a (re, im) register pair, and gfx950 has packed fp32 arithmetic on such pairs
// (v_pk_add / mul / fma_f32) whose operand modifiers pick halves (op_sel) and flip signs (neg_lo / neg_hi) per
// lane: a complex sum is ONE instruction, a complex product two, a +- i b one.  Left to itself the compiler
// vectorises across unrelated values instead and spends a quarter of the vector instructions of a complex64
// pass on register moves (546 v_mov_b32 of 2316, round 2).  These overloads spell the operations out; the two
// with lane-wise negation of a variable operand -- which the compiler does not fold into the modifiers -- are
// two lines of assembly.  Per byte moved a complex64 pass has twice the points of a complex128 one, so this is
// what lets the fp32 mode approach 2x instead of 1.5x.
typedef float f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f2 pk(cx<float> a) { return f2{a.x, a.y}; }
__device__ __forceinline__ cx<float> unpk(f2 v) { return {v.x, v.y}; }
__device__ __forceinline__ cx<float> cadd(cx<float> a, cx<float> b) { return unpk(pk(a) + pk(b)); }
__device__ __forceinline__ cx<float> csub(cx<float> a, cx<float> b) { return unpk(pk(a) - pk(b)); }
__device__ __forceinline__ cx<float> cmul(cx<float> a, cx<float> b) {
  f2 t, r;
  const f2 av = pk(a), bv = pk(b);
  asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[0,1]" : "=v"(t) : "v"(av), "v"(bv));                       // (a.x b.x, a.x b.y)
  asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[1,0,0]"                    // (-a.y b.y, a.y b.x) + t
      : "=v"(r) : "v"(av), "v"(bv), "v"(t));
  return unpk(r);
}
// The same product where ``b`` may come straight out of the transcendental unit (v_sin_f32 / v_cos_f32): gfx950
// wants one wait state between such an instruction and a consumer of its result.  The compiler inserts it for the
// instructions it emits itself but does not look into inline assembly, so the wait state is part of the text.
__device__ __forceinline__ cx<float> cmul_after_trans(cx<float> a, cx<float> b) {
  f2 t, r;
  const f2 av = pk(a), bv = pk(b);
  asm("s_nop 0\n\tv_pk_mul_f32 %0, %1, %2 op_sel_hi:[0,1]" : "=v"(t) : "v"(av), "v"(bv));
  asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[1,0,0]" : "=v"(r) : "v"(av), "v"(bv), "v"(t));
  return unpk(r);
}
__device__ __forceinline__ cx<float> sub_ib(cx<float> a, cx<float> b) {  // (a.x + b.y, a.y - b.x)
  f2 r;
  asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_hi:[0,1]" : "=v"(r) : "v"(pk(a)), "v"(pk(b)));
  return unpk(r);
}
__device__ __forceinline__ cx<float> add_ib(cx<float> a, cx<float> b) {  // (a.x - b.y, a.y + b.x)
  f2 r;
  asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[0,1]" : "=v"(r) : "v"(pk(a)), "v"(pk(b)));
  return unpk(r);
}
__device__ __forceinline__ cx<float> fma_real(float c, cx<float> b, cx<float> a) {
  return unpk(__builtin_elementwise_fma(f2{c, c}, pk(b), pk(a)));
}
__device__ __forceinline__ cx<float> rot_tau(cx<float> b, float tau) {
  const f2 bv = pk(b);
  return unpk(__builtin_elementwise_fma(bv.yx, f2{-tau, tau}, bv));
}
__device__ __forceinline__ cx<float> fma_mic(float c, cx<float> b, cx<float> a) {
  return unpk(__builtin_elementwise_fma(pk(b).yx, f2{c, -c}, pk(a)));
}
__device__ __forceinline__ cx<float> fma_pic(float c, cx<float> b, cx<float> a) {
  return unpk(__builtin_elementwise_fma(pk(b).yx, f2{-c, c}, pk(a)));
}
__device__ __forceinline__ cx<float> cmul_const(cx<float> v, float c, float s) {
  const f2 vv = pk(v);
  return unpk(__builtin_elementwise_fma(vv.yy, f2{-s, c}, vv.xx * f2{c, s}));
}
__device__ __forceinline__ cx<float> scale2(cx<float> v, float p, float q) { return unpk(pk(v) * f2{p, q}); }

// sin and cos of a double: three-term Cody-Waite reduction by pi/2 + the classic minimax
// kernels on [-pi/4, pi/4].  With FMA the first reduction step a - n*pio2_1 is exact for any
// n (the difference needs <= 34 bits), the later steps round at 1e-16 of |r| <= 1, and the
// three-term pi/2 is good to 8.5e-32 * n, so the result is ~1 ulp for |a| up to 2^40
// (the rounding trick below needs |a * 2/pi| < 2^51); the
// library validates on the host that no phase argument exceeds kMaxPhaseArg (pass_records.h; pass_program.h: check_phase_args)
// so the kernels carry no Payne-Hanek fallback.  ~45 instructions, branch-free.
__device__ __forceinline__ void sincos_fast(double a, double* sn, double* cs) {
  // round(a * 2/pi) by the 1.5 * 2^52 trick: the integer lands in the low mantissa bits, so its
  // two low bits (the quadrant) are read straight from the register, no conversion
  const double kMagic = 6755399441055744.0;
  const double nb = fma(a, 0.63661977236758134308, kMagic);  // 2/pi
  const unsigned q = (unsigned)__double2loint(nb);
  const double n = nb - kMagic;
  double r = fma(-n, 1.57079632673412561417e+00, a);
  r = fma(-n, 6.07710050630396597660e-11, r);
  r = fma(-n, 2.02226624879595063154e-21, r);
  const double z = r * r;
  double ps = fma(z, 1.58969099521155010221e-10, -2.50507602534068634195e-08);
  ps = fma(z, ps, 2.75573137070700676789e-06);
  ps = fma(z, ps, -1.98412698298579493134e-04);
  ps = fma(z, ps, 8.33333333332248946124e-03);
  ps = fma(z, ps, -1.66666666666666324348e-01);
  const double s = fma(r * z, ps, r);
  double pc = fma(z, -1.13596475577881948265e-11, 2.08757232129817482790e-09);
  pc = fma(z, pc, -2.75573143513906633035e-07);
  pc = fma(z, pc, 2.48015872894767294178e-05);
  pc = fma(z, pc, -1.38888888888741095749e-03);
  pc = fma(z, pc, 4.16666666666666019037e-02);
  const double c = fma(z * z, pc, fma(z, -0.5, 1.0));
  const bool odd = (q & 1u) != 0;
  const double s1 = odd ? c : s;
  const double c1 = odd ? s : c;
  // signs: sin flips in quadrants 2, 3; cos in 1, 2 -- an XOR on the sign bit
  const int sflip = (int)((q & 2u) << 30), cflip = (int)(((q + 1u) & 2u) << 30);
  *sn = __hiloint2double(__double2hiint(s1) ^ sflip, __double2loint(s1));
  *cs = __hiloint2double(__double2hiint(c1) ^ cflip, __double2loint(c1));
}

// cos(2 pi m / 32), m = 0..8 (first octant pair); everything else by symmetry.
__device__ constexpr double kCos32[9] = {
    1.0,
    0.98078528040323044913,
    0.92387953251128675613,
    0.83146961230254523708,
    0.70710678118654752440,
    0.55557023301960222474,
    0.38268343236508977173,
    0.19509032201612826785,
    0.0};

__host__ __device__ constexpr double cos32(int m) {
  m &= 31;
  if (m > 16) m = 32 - m;
  return (m > 8) ? -kCos32[16 - m] : kCos32[m];
}
__host__ __device__ constexpr double sin32(int m) { return cos32(m - 8); }

// v * W_R^m with W_R = exp(-2 pi i / R) for DIR = +1 (forward) and its
// conjugate for DIR = -1.  m is a compile-time constant after unrolling, so
// the trivial cases fold away.
template <int R, int DIR, typename T>
__device__ __forceinline__ cx<T> mulw(cx<T> v, int m) {
  const int m32 = (m * (32 / R)) & 31;
  if (m32 == 0) return v;
  if (m32 == 16) return {-v.x, -v.y};
  if (m32 == 8) return (DIR > 0) ? cx<T>{v.y, -v.x} : cx<T>{-v.y, v.x};    // * -/+ i
  if (m32 == 24) return (DIR > 0) ? cx<T>{-v.y, v.x} : cx<T>{v.y, -v.x};   // * +/- i
  const T c = (T)cos32(m32);
  const T s = (T)((DIR > 0) ? -sin32(m32) : sin32(m32));
  return cmul_const(v, c, s);
}

// ---- 16-point DFT with the inner twiddles folded into the butterflies (Linzer-Feig) ---------------
// The 4 x 4 decomposition below multiplies nine of the sixteen intermediate values by W16^m between its two
// layers: 8 non-trivial complex products, 32 of the 160 fp64 instructions.  With w = c (1 + i tau), tau = tan,
//   w b = c u,  u = (b.x - tau b.y, b.y + tau b.x)           2 FMA instead of 4 instructions,
// and the factor c rides on the FMA that replaces the butterfly's addition:  a +- w b = fma(+-c, u, a).
// For the pair  w1 b1 +- w3 b3 = c1 (u1 +- (c3 / c1) u3)  the factor c1 moves one level down the same way.
// A radix-4 butterfly with three twiddled inputs costs 22 FMA instead of 28 instructions; the DFT 144 instead
// of 160 -- 16 fewer per transform stage, six stages per two-transform pass, in kernels that run at the rate of
// the fp64 pipe (profiles/r02_valu_mix_fftbench.txt).  All constants are compile-time; cos(2 pi m / 16) is never
// zero for the m used here (m = 4, the multiplication by -+i, is kept exact and free).
template <int M16, int DIR>
struct W16 {  // W16^M16 for DIR = +1 (exp(-2 pi i M16 / 16)), its conjugate for DIR = -1
  static constexpr int m32 = (M16 * 2) & 31;
  static constexpr bool quarter = m32 == 8 || m32 == 24;  // * -+i: exact, no arithmetic
  static constexpr bool times_minus_i = (m32 == 8) == (DIR > 0);
  static constexpr double c = cos32(m32);
  static constexpr double s = (DIR > 0) ? -sin32(m32) : sin32(m32);
  static constexpr double tau = quarter ? 0.0 : s / c;
};
template <typename T>
__device__ __forceinline__ cx<T> lf_u(cx<T> b, double tau) { return rot_tau(b, (T)tau); }
// out[k2], k2 = 0..3, of the radix-4 butterfly over (b0, W^K1 b1, W^2K1 b2, W^3K1 b3), W = W16
template <int K1, int DIR, typename T>
__device__ __forceinline__ void lf_twiddled_dft4(const cx<T>* b, cx<T>* out) {
  using W1 = W16<K1, DIR>;
  using W2 = W16<2 * K1, DIR>;
  using W3 = W16<3 * K1, DIR>;
  static_assert(!W1::quarter && !W3::quarter, "K1 and 3 K1 are never multiples of 4 here");
  cx<T> t0, t1;
  if constexpr (W2::quarter) {
    const cx<T> wb = W2::times_minus_i ? cx<T>{b[2].y, -b[2].x} : cx<T>{-b[2].y, b[2].x};
    t0 = cadd(b[0], wb);
    t1 = csub(b[0], wb);
  } else {
    const cx<T> u2 = lf_u(b[2], W2::tau);
    t0 = fma_real((T)W2::c, u2, b[0]);
    t1 = fma_real((T)-W2::c, u2, b[0]);
  }
  const cx<T> u1 = lf_u(b[1], W1::tau), u3 = lf_u(b[3], W3::tau);
  constexpr double rho = W3::c / W1::c;
  const cx<T> t2 = fma_real((T)rho, u3, u1);   // (w1 b1 + w3 b3) / c1
  const cx<T> t3 = fma_real((T)-rho, u3, u1);  // (w1 b1 - w3 b3) / c1
  constexpr T c1 = (T)W1::c;
  out[0] = fma_real(c1, t2, t0);
  out[2] = fma_real(-c1, t2, t0);
  if constexpr (DIR > 0) {  // t1 -+ i c1 t3
    out[1] = fma_mic(c1, t3, t1);
    out[3] = fma_pic(c1, t3, t1);
  } else {
    out[1] = fma_pic(c1, t3, t1);
    out[3] = fma_mic(c1, t3, t1);
  }
}

template <int R, int DIR, typename T>
__device__ __forceinline__ void dft(cx<T>* v);

template <int DIR, typename T>
__device__ __forceinline__ void dft16_lf(cx<T>* v) {
  cx<T> y[16];
#pragma unroll
  for (int n2 = 0; n2 < 4; ++n2) {  // first layer: n = 4 n1 + n2 -> a[k1], untwiddled
    cx<T> a[4] = {v[n2], v[4 + n2], v[8 + n2], v[12 + n2]};
    dft<4, DIR>(a);
#pragma unroll
    for (int k1 = 0; k1 < 4; ++k1) y[k1 * 4 + n2] = a[k1];
  }
  cx<T> o[4];
  {
    cx<T> b[4] = {y[0], y[1], y[2], y[3]};
    dft<4, DIR>(b);
#pragma unroll
    for (int k2 = 0; k2 < 4; ++k2) v[4 * k2] = b[k2];
  }
  lf_twiddled_dft4<1, DIR>(y + 4, o);
#pragma unroll
  for (int k2 = 0; k2 < 4; ++k2) v[1 + 4 * k2] = o[k2];
  lf_twiddled_dft4<2, DIR>(y + 8, o);
#pragma unroll
  for (int k2 = 0; k2 < 4; ++k2) v[2 + 4 * k2] = o[k2];
  lf_twiddled_dft4<3, DIR>(y + 12, o);
#pragma unroll
  for (int k2 = 0; k2 < 4; ++k2) v[3 + 4 * k2] = o[k2];
}

// dft16_lf of a line whose outer quarters are exact zeros: v[0..3] = v[12..15] = {0, 0} (the first stage of a pass that loads
// the central half of its positions at most -- frugal_pass.h: CH).  Each first-layer radix-4 then has the inputs (0, a, b, 0),
// and what dft<4> makes of them -- t0 = 0 + b, t1 = 0 - b, t2 = a + 0, t3 = a - 0 -- is b, -b, a, a: four complex additions,
// in the order and with the operands of the full butterfly, so the live sums keep their bits (an exact zero may change its
// sign).  The second layer is dft16_lf's.  Forward transforms only (the pass kernel conjugates around an inverse one).
// NARROW (round 23, CH = 2): v[4] and v[11] are exact zeros too -- the live inputs are v[5..10].  The butterfly n2 = 0 then has
// the inputs (0, 0, b, 0) and n2 = 3 has (0, a, 0, 0); with every x +- 0 of dft<4> written out their outputs are b, -b, b, -b
// and a, -i a, -a, +i a: copies, negations and swaps, no addition.  n2 = 1 and n2 = 2 keep the four additions.
template <int DIR, bool NARROW = false, typename T>
__device__ __forceinline__ void dft16_lf_central(cx<T>* v) {
  static_assert(DIR > 0, "the pass kernel runs forward transforms only");
  cx<T> y[16];
#pragma unroll
  for (int n2 = 0; n2 < 4; ++n2) {
    const cx<T> a = v[4 + n2], b = v[8 + n2];
    const cx<T> nb = {-b.x, -b.y};
    if (NARROW && n2 == 0) {         // a = 0: t2 = t3 = 0
      y[0 * 4 + n2] = b;
      y[1 * 4 + n2] = nb;
      y[2 * 4 + n2] = b;
      y[3 * 4 + n2] = nb;
    } else if (NARROW && n2 == 3) {  // b = 0: t0 = t1 = 0
      y[0 * 4 + n2] = a;
      y[1 * 4 + n2] = cx<T>{a.y, -a.x};   // -i a
      y[2 * 4 + n2] = cx<T>{-a.x, -a.y};
      y[3 * 4 + n2] = cx<T>{-a.y, a.x};   // +i a
    } else {
      y[0 * 4 + n2] = cadd(b, a);     // t0 + t2
      y[1 * 4 + n2] = sub_ib(nb, a);  // t1 - i t3
      y[2 * 4 + n2] = csub(b, a);     // t0 - t2
      y[3 * 4 + n2] = add_ib(nb, a);  // t1 + i t3
    }
  }
  cx<T> o[4];
  {
    cx<T> b[4] = {y[0], y[1], y[2], y[3]};
    dft<4, DIR>(b);
#pragma unroll
    for (int k2 = 0; k2 < 4; ++k2) v[4 * k2] = b[k2];
  }
  lf_twiddled_dft4<1, DIR>(y + 4, o);
#pragma unroll
  for (int k2 = 0; k2 < 4; ++k2) v[1 + 4 * k2] = o[k2];
  lf_twiddled_dft4<2, DIR>(y + 8, o);
#pragma unroll
  for (int k2 = 0; k2 < 4; ++k2) v[2 + 4 * k2] = o[k2];
  lf_twiddled_dft4<3, DIR>(y + 12, o);
#pragma unroll
  for (int k2 = 0; k2 < 4; ++k2) v[3 + 4 * k2] = o[k2];
}

// In-place DFT of R points held in registers, natural order in and out.
template <int R, int DIR, typename T>
__device__ __forceinline__ void dft(cx<T>* v) {
  if constexpr (R == 16) {
    dft16_lf<DIR>(v);
  } else if constexpr (R == 2) {
    cx<T> a = v[0], b = v[1];
    v[0] = cadd(a, b);
    v[1] = csub(a, b);
  } else if constexpr (R == 4) {
    cx<T> t0 = cadd(v[0], v[2]), t1 = csub(v[0], v[2]);
    cx<T> t2 = cadd(v[1], v[3]), t3 = csub(v[1], v[3]);
    v[0] = cadd(t0, t2);
    v[2] = csub(t0, t2);
    if constexpr (DIR > 0) {
      v[1] = sub_ib(t1, t3);
      v[3] = add_ib(t1, t3);
    } else {
      v[1] = add_ib(t1, t3);
      v[3] = sub_ib(t1, t3);
    }
  } else if constexpr (R > 4) {
    // R = A * B, n = B n1 + n2, k = k1 + A k2:
    //   W_R^{nk} = W_A^{n1 k1} W_R^{n2 k1} W_B^{n2 k2}
    constexpr int A = 4, B = R / 4;
    cx<T> y[R];
#pragma unroll
    for (int n2 = 0; n2 < B; ++n2) {
      cx<T> a[A];
#pragma unroll
      for (int n1 = 0; n1 < A; ++n1) a[n1] = v[B * n1 + n2];
      dft<A, DIR>(a);
#pragma unroll
      for (int k1 = 0; k1 < A; ++k1) y[k1 * B + n2] = mulw<R, DIR>(a[k1], n2 * k1);
    }
#pragma unroll
    for (int k1 = 0; k1 < A; ++k1) {
      cx<T> b[B];
#pragma unroll
      for (int n2 = 0; n2 < B; ++n2) b[n2] = y[k1 * B + n2];
      dft<B, DIR>(b);
#pragma unroll
      for (int k2 = 0; k2 < B; ++k2) v[k1 + A * k2] = b[k2];
    }
  }
}

// LDS padding: one extra slot every 16 so that the stride-R scatter of the
// first exchange and the stride-1 gather both stay conflict-free.
__device__ __forceinline__ constexpr int lds_pad(int i) { return i + (i >> 4); }
template <int N>
constexpr int lds_line_slots() { return N + (N >> 4); }

template <int N, int E, int NS>
struct StageInfo {
  static constexpr int REM = N / NS;               // points still to combine
  static constexpr int R = (REM >= E) ? E : REM;   // radix of this stage
  static constexpr int TPT = E / R;                // butterflies per thread
  static constexpr bool LAST = (NS * R == N);
};

// radix of the final stage / butterflies per thread in it
template <int N, int E, int NS = 1>
constexpr int last_radix() {
  if constexpr (StageInfo<N, E, NS>::LAST) return StageInfo<N, E, NS>::R;
  else return last_radix<N, E, NS * StageInfo<N, E, NS>::R>();
}

// Slot k of the register file after the transform holds X[t + outslot(k) * TL]
// (TL = N / E threads per line); before it, slot k holds x[t + k * TL].
template <int N, int E>
__device__ __forceinline__ constexpr int outslot(int k) {
  constexpr int RL = last_radix<N, E>();
  constexpr int TPTL = E / RL;
  return (k / RL) + (k % RL) * TPTL;
}

// Twiddle powers v[r] *= w^r.  w^r = (w^4)^a * w^b keeps only five powers live
// (w, w^2, w^3, w^4 and the running (w^4)^a) instead of R of them, and bounds
// the product depth at R/4 + 1.
template <int R, typename T>
__device__ __forceinline__ void apply_twiddle_powers(cx<T>* v, cx<T> w1) {
  v[1] = cmul(v[1], w1);
  if constexpr (R > 2) {
    const cx<T> w2 = cmul(w1, w1);
    const cx<T> w3 = cmul(w2, w1);
    v[2] = cmul(v[2], w2);
    v[3] = cmul(v[3], w3);
    if constexpr (R > 4) {
      const cx<T> w4 = cmul(w2, w2);
      cx<T> base = w4;
#pragma unroll
      for (int a = 1; a < R / 4; ++a) {
        v[4 * a] = cmul(v[4 * a], base);
        v[4 * a + 1] = cmul(v[4 * a + 1], cmul(base, w1));
        v[4 * a + 2] = cmul(v[4 * a + 2], cmul(base, w2));
        v[4 * a + 3] = cmul(v[4 * a + 3], cmul(base, w3));
        if (a + 1 < R / 4) base = cmul(base, w4);
      }
    }
  }
}

// Register-frugal twiddle powers: a running product, two twiddles live (vs five above).
// Error grows linearly (<= R roundings, ~2e-15 for R = 16): well inside the parity budget.
template <int R, typename T>
__device__ __forceinline__ void apply_twiddle_chain(cx<T>* v, cx<T> w1) {
  cx<T> w = w1;
#pragma unroll
  for (int r = 1; r < R; ++r) {
    v[r] = cmul(v[r], w);
    if (r + 1 < R) w = cmul(w, w1);
  }
}

// All stages of one line.  ``lds`` is this line's exchange area: cx<T> slots
// when !SPLIT, T slots (real and imaginary parts exchanged one after the other,
// halving the LDS footprint) when SPLIT.  ``tw`` = exp(-2 pi i m / N), m < N.
// FR (frugal): sequential twiddle chain and scheduling fences between the phases of a stage,
// which keeps a 4096-point c128 pass at ~118 VGPRs -- four waves per SIMD, i.e. two 512-thread
// workgroups per CU whose load / compute / store phases overlap (profiles/r01_vgpr_experiments.txt).
#define PAOS_FENCE() do { if constexpr (FR != 0) __builtin_amdgcn_sched_barrier(0); } while (0)
// ``circle`` (frugal complex128 kernels, else nullptr): exp(+2 pi i m / 256), m < 256, in LDS.  The
// stage whose twiddles are 256th roots of unity (NS * R == 256: w^r = exp(-2 pi i k r / 256) with
// k r < 256) reads its 15 powers from it instead of multiplying them up -- 15 ds_read_b128 for
// 14 complex products.
// ``w1_last`` (optional): the base twiddles tw[t + s TL] of the butterflies s = 0 .. TPT - 1 a thread runs in the LAST stage
// (N = 4096: one, k = t; N = 2048: two) -- per-thread constants the caller keeps in registers, so that the stage needs no
// table in LDS (the four-per-CU shapes of frugal_pass.h only fit without the 4 KiB table).
// CH != 0 (the first stage, NS = 1, of 16-point-per-thread complex128 lines): slots 0..3 and 12..15 hold exact zeros
// (dft16_lf_central); CH = 2: slots 4 and 11 too; the later stages are the ordinary ones.
template <typename T, int N, int E, int DIR, bool SPLIT, int NS = 1, int FR = 0, int CH = 0>
__device__ __forceinline__ void fft_stages(cx<T>* v, void* lds, int t,
                                           const cx<T>* __restrict__ tw, const cx<double>* circle = nullptr,
                                           const cx<T>* w1_last = nullptr) {
  using S = StageInfo<N, E, NS>;
  constexpr int TL = N / E;
  constexpr int R = S::R;
  constexpr int TPT = S::TPT;

#pragma unroll
  for (int s = 0; s < TPT; ++s) {
    if constexpr (NS > 1) {
      const int j = t + s * TL;
      const int k = j & (NS - 1);
      if constexpr (FR != 0 && sizeof(T) == 8 && NS * R == 256) {
        // two reads in flight ahead of the product that consumes them; the fences keep the scheduler
        // from hoisting all fifteen (60 VGPRs) above the first product
        cx<double> wa = circle[k], wb = circle[2 * k];
#pragma unroll
        for (int r = 1; r < R; ++r) {
          const cx<double> w = wa;
          wa = wb;
          if (r + 2 < R) wb = circle[k * (r + 2)];
          v[s * R + r] = cmul(v[s * R + r], cx<T>{(T)w.x, (T)(DIR > 0 ? -w.y : w.y)});
          PAOS_FENCE();
        }
      } else {
        cx<T> w1 = (w1_last != nullptr && NS * R == N) ? w1_last[s] : tw[k * (N / (NS * R))];
        if constexpr (DIR < 0) w1.y = -w1.y;
        if constexpr (FR != 0) apply_twiddle_chain<R>(v + s * R, w1);
        else apply_twiddle_powers<R>(v + s * R, w1);
      }
      PAOS_FENCE();
    }
    if constexpr (CH != 0 && NS == 1) {
      static_assert(R == 16 && TPT == 1, "central-half first stage: one 16-point butterfly per thread");
      dft16_lf_central<DIR, CH == 2>(v);
    } else {
      dft<R, DIR>(v + s * R);
    }
    PAOS_FENCE();
  }

  if constexpr (!S::LAST) {
    using SN = StageInfo<N, E, NS * R>;
    constexpr int R2 = SN::R;
    constexpr int TPT2 = SN::TPT;
    // Scatter/gather slots are pad(base) + a compile-time offset (no carry out of
    // the low four bits for power-of-two radices), so each thread needs one LDS
    // address VGPR per exchange and the ds_* immediates carry the rest.
    constexpr bool LIN_R = (TL % 16 == 0) && ((N / R2) % 16 == 0);
    int wb[TPT];
#pragma unroll
    for (int s = 0; s < TPT; ++s) {
      const int j = t + s * TL;
      wb[s] = lds_pad((j / NS) * (NS * R) + (j & (NS - 1)));
    }
    const int rb = lds_pad(t);
    auto ridx = [&](int s, int r) -> int {
      const int off = s * TL + r * (N / R2);
      return LIN_R ? rb + lds_pad(off) : lds_pad(t + off);
    };
    if constexpr (!SPLIT) {
      cx<T>* l = reinterpret_cast<cx<T>*>(lds);
#pragma unroll
      for (int s = 0; s < TPT; ++s)
#pragma unroll
        for (int r = 0; r < R; ++r) l[wb[s] + lds_pad(r * NS)] = v[s * R + r];
      __syncthreads();
#pragma unroll
      for (int s = 0; s < TPT2; ++s)
#pragma unroll
        for (int r = 0; r < R2; ++r) v[s * R2 + r] = l[ridx(s, r)];
      if constexpr (!SN::LAST) __syncthreads();
    } else {
      T* l = reinterpret_cast<T*>(lds);
#pragma unroll
      for (int part = 0; part < 2; ++part) {
#pragma unroll
        for (int s = 0; s < TPT; ++s)
#pragma unroll
          for (int r = 0; r < R; ++r) l[wb[s] + lds_pad(r * NS)] = part ? v[s * R + r].y : v[s * R + r].x;
        __syncthreads();
#pragma unroll
        for (int s = 0; s < TPT2; ++s)
#pragma unroll
          for (int r = 0; r < R2; ++r) {
            const T val = l[ridx(s, r)];
            if (part) v[s * R2 + r].y = val; else v[s * R2 + r].x = val;
          }
        if (part == 0 || !SN::LAST) __syncthreads();
      }
    }
    PAOS_FENCE();
    fft_stages<T, N, E, DIR, SPLIT, NS * R, FR, 0>(v, lds, t, tw, circle, w1_last);
  }
}

// Undo the output slot permutation in registers (compile-time renaming), so
// that slot k holds X[t + k * TL] again -- lets a forward transform feed an
// inverse one with no LDS trip in between (fused ptp column pass).
template <int N, int E, typename T>
__device__ __forceinline__ void unpermute_slots(cx<T>* v) {
  cx<T> tmp[E];
#pragma unroll
  for (int k = 0; k < E; ++k) tmp[outslot<N, E>(k)] = v[k];
#pragma unroll
  for (int k = 0; k < E; ++k) v[k] = tmp[k];
}

// --------------------------------------------------------------------------
// HBM layout of a field.  Blocks of BR rows x BC columns are contiguous, blocks
// are ordered row-major.  BR = 1 is plain row-major.  The library uses BR x BC = 4 x 2: with
// c128 a block is exactly one 128-byte line, which the column pass (2 columns per workgroup)
// moves whole and the row pass moves whole (4 rows per workgroup) or in halves (2 rows, N >= 2048).
// ``pitch`` = elements from one block-row to the next: n * BR when dense; the
// context pads it by a few blocks so that the column pass (stride = pitch) does
// not march through HBM channels with a power-of-two stride.
template <int BR, int BC>
__device__ __host__ __forceinline__ constexpr size_t layout_index(int row, int col, size_t pitch) {
  return (size_t)(row / BR) * pitch + (size_t)(col / BC) * (BR * BC) + (row % BR) * BC + (col % BC);
}

}  // namespace paos
