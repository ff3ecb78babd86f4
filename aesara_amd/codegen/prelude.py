"""The HIP text every generated kernel starts with (argument blocks, packs, non-temporal
accesses, the scalar helpers restating the reference ScalarOps) and the dtype tables."""
from __future__ import annotations

from .._lib import AHIP_MAXD, AHIP_MAXOPS

CTYPE = {
    "bool": "unsigned char", "int8": "signed char", "int16": "short", "int32": "int",
    "int64": "long long", "uint8": "unsigned char", "uint16": "unsigned short",
    "uint32": "unsigned int", "uint64": "unsigned long long", "float32": "float",
    "float64": "double",
}
# type used for values held in registers (bool is a real C++ bool there)
RTYPE = dict(CTYPE, bool="bool")

PRELUDE = r"""
typedef long long i64;
#ifndef NAN
#define NAN __builtin_nanf("")
#endif
#ifndef INFINITY
#define INFINITY __builtin_huge_valf()
#endif
#define AHIP_MAXD %d
#define AHIP_MAXOPS %d
struct Args {
  i64 n; i64 shape[AHIP_MAXD]; i64 stride[AHIP_MAXOPS][AHIP_MAXD]; void* ptr[AHIP_MAXOPS];
  void* ws; void* out; i64 aux0; i64 aux1; int nd; int nops;
};
// horizontally fused full reductions (ahip_ewh_args): jobs share one grid
#define AHIP_HJOBS 16
#define AHIP_HOPS 6
struct ArgsH {
  i64 n[AHIP_HJOBS]; void* ptr[AHIP_HJOBS][AHIP_HOPS]; void* out[AHIP_HJOBS];
  unsigned wg0[AHIP_HJOBS + 1]; int njobs; void* ws; i64 aux1;
};
template <typename T, int N> struct alignas((sizeof(T) * N) >= 16 ? 16 : (sizeof(T) * N)) Pack { T v[N]; };

template <typename T, int N> __device__ __forceinline__ Pack<T, N> nt_load(const Pack<T, N>* p) {
  Pack<T, N> r;
  if constexpr (sizeof(T) * N >= 16) {
    typedef unsigned int u4 __attribute__((ext_vector_type(4)));
    const u4* q = (const u4*)p;
    u4* d = (u4*)&r;
#pragma unroll
    for (unsigned i = 0; i < sizeof(T) * N / 16; ++i) d[i] = __builtin_nontemporal_load(q + i);
  } else {
    r = *p;
  }
  return r;
}

template <typename T, int N> __device__ __forceinline__ void nt_store(Pack<T, N>* p, const Pack<T, N>& r) {
  if constexpr (sizeof(T) * N >= 16) {
    typedef unsigned int u4 __attribute__((ext_vector_type(4)));
    u4* q = (u4*)p;
    const u4* d = (const u4*)&r;
#pragma unroll
    for (unsigned i = 0; i < sizeof(T) * N / 16; ++i) __builtin_nontemporal_store(d[i], q + i);
  } else {
    *p = r;
  }
}

// ---- scalar helpers (reference: aesara/scalar/basic.py, scalar/math.py c_code) ----
template <typename T> __device__ __forceinline__ T idiv_floor(T x, T y) {  // FloorDivide :2039
  if (y == 0) return 0;
  T q = x / y;
  if ((x %% y != 0) && ((x < 0) != (y < 0))) q -= 1;
  return q;
}
template <typename T> __device__ __forceinline__ T udiv_floor(T x, T y) { return y == 0 ? 0 : x / y; }
template <typename T> __device__ __forceinline__ T imod_py(T x, T y) {      // Mod :2144
  if (y == 0) return 0;
  T r = x %% y;
  if (r != 0 && ((r < 0) != (y < 0))) r += y;
  return r;
}
template <typename T> __device__ __forceinline__ T umod(T x, T y) { return y == 0 ? 0 : x %% y; }
__device__ __forceinline__ float fmod_py(float x, float y) {
  if (y == 0.0f) return fmodf(x, y);
  float r = fmodf(x, y);
  if (r != 0.0f && ((r < 0.0f) != (y < 0.0f))) r += y;
  return r;
}
__device__ __forceinline__ double fmod_py(double x, double y) {
  if (y == 0.0) return fmod(x, y);
  double r = fmod(x, y);
  if (r != 0.0 && ((r < 0.0) != (y < 0.0))) r += y;
  return r;
}
template <typename T> __device__ __forceinline__ T ipow(T b, T e) {
  T r = 1;
  if (e < 0) return (b == 1) ? 1 : ((b == (T)-1) ? ((e & 1) ? (T)-1 : 1) : 0);
  while (e) { if (e & 1) r *= b; b *= b; e >>= 1; }
  return r;
}
template <typename T> __device__ __forceinline__ T upow(T b, T e) {
  T r = 1;
  while (e) { if (e & 1) r *= b; b *= b; e >>= 1; }
  return r;
}
// ScalarMaximum/ScalarMinimum c_code (:1745): NaN propagates
template <typename T> __device__ __forceinline__ T fmax_nan(T x, T y) { return (y > x) ? y : ((x >= y) ? x : (T)NAN); }
template <typename T> __device__ __forceinline__ T fmin_nan(T x, T y) { return (y < x) ? y : ((x <= y) ? x : (T)NAN); }
template <typename T> __device__ __forceinline__ T imax(T x, T y) { return x > y ? x : y; }
// MulWithoutZeros.c_code (tensor/math.py:2731): zeros are skipped, 0 is the identity
template <typename T> __device__ __forceinline__ T mwz_(T x, T y) { return x == 0 ? y : (y == 0 ? x : (T)(y * x)); }
template <typename T> __device__ __forceinline__ T imin(T x, T y) { return x < y ? x : y; }
// x / c for a loop-invariant c with r = 1/c precomputed: Markstein refinement gives the correctly
// rounded quotient when c and r are normal numbers (ok: hoisted, wave-uniform) and nothing
// overflowed (a non-finite q or residual makes res non-finite); otherwise the full division.
__device__ __forceinline__ bool recip_ok(double c, double r) {
  return fabs(c) >= 2.2250738585072014e-308 && fabs(c) < INFINITY &&
         fabs(r) >= 2.2250738585072014e-308 && fabs(r) < INFINITY;
}
__device__ __forceinline__ bool recip_ok(float c, float r) {
  return fabsf(c) >= 1.17549435e-38f && fabsf(c) < INFINITY &&
         fabsf(r) >= 1.17549435e-38f && fabsf(r) < INFINITY;
}
__device__ __forceinline__ double fdiv_inv(double x, double c, double r, bool ok) {
  const double q = x * r;
  double res = fma(fma(-q, c, x), r, q);
  if (__builtin_expect(!(ok && fabs(res) < INFINITY), 0)) {
    asm volatile("" ::: "memory");   // keep the full division out of line (no if-conversion)
    res = x / c;
  }
  return res;
}
__device__ __forceinline__ float fdiv_inv(float x, float c, float r, bool ok) {
  const float q = x * r;
  float res = fmaf(fmaf(-q, c, x), r, q);
  if (__builtin_expect(!(ok && fabsf(res) < INFINITY), 0)) {
    asm volatile("" ::: "memory");
    res = x / c;
  }
  return res;
}
// (K * y) / c with K = +-2^k a literal, correctly rounded like fdiv_inv: the real number is
// y / (c / K); c / K and K * r = RN(1 / (c / K)) are exact scalings, loop invariant, so the scaling
// multiply of every element goes away and the refinement runs on (y, c / K, K * r).  Full division
// of the scaled operands when any of c, r, c / K, K * r is not a normal number.
template <typename T> __device__ __forceinline__ T fdiv_inv_s(T y, T K, T c, T r, bool ok) {
  const T cK = c * ((T)1 / K), rK = r * K;
  const T q = y * rK;
  T res = fma(fma(-q, cK, y), rK, q);
  if (__builtin_expect(!(ok && recip_ok(cK, rK) && fabs(res) < (T)INFINITY), 0)) {
    asm volatile("" ::: "memory");
    res = (K * y) / c;
  }
  return res;
}
// tolerance mode (AESARA_HIP_FASTDIV=1): x * (1/c) without the refinement — at most 1.5 ulp from
// the quotient (north_star's bar is 1e-6 rel); the full division when c or 1/c is not a normal number
template <typename T> __device__ __forceinline__ T fdiv_rcp_s(T y, T K, T c, T r, bool ok) {
  T res = y * (K * r);            // (K * y) / c, K a power of two: K * r is exact and loop invariant
  if (__builtin_expect(!ok, 0)) {
    asm volatile("" ::: "memory");
    res = (K * y) / c;
  }
  return res;
}
template <typename T> __device__ __forceinline__ T fdiv_rcp(T x, T c, T r, bool ok) {
  T res = x * r;
  if (__builtin_expect(!ok, 0)) {
    asm volatile("" ::: "memory");
    res = x / c;
  }
  return res;
}
__device__ __forceinline__ float sigmoid_(float x) { return 1.0f / (1.0f + expf(-x)); }   // Sigmoid :1110
__device__ __forceinline__ double sigmoid_(double x) { return 1.0 / (1.0 + exp(-x)); }
__device__ __forceinline__ float softplus_(float x) {                                      // Softplus :1173
  return x < -37.0f ? expf(x) : (x < 18.0f ? log1pf(expf(x)) : (x < 33.3f ? x + expf(-x) : x));
}
__device__ __forceinline__ double softplus_(double x) {
  return x < -37.0 ? exp(x) : (x < 18.0 ? log1p(exp(x)) : (x < 33.3 ? x + exp(-x) : x));
}
// Psi :361 — the reference's C body: Bernardo (1976), Algorithm AS 103 (0 for x <= 0, like it)
__device__ __forceinline__ double psi_as103(double x) {
  double y = x, psi = 0.0;
  if (y <= 0.0) return psi;
  if (y <= 1.0e-5) return -0.5772156649 - 1.0 / y;
  while (y < 8.5) { psi = psi - 1.0 / y; y = y + 1; }
  double R = 1.0 / y;
  psi = psi + log(y) - .5 * R;
  R = R * R;
  psi = psi - R * (8.333333333e-2 - R * (8.333333333e-3 - R * 3.968253968e-3));
  return psi;
}
// TriGamma :454 — the reference's C body: Algorithm AS 121 (0 for x <= 0, like it)
__device__ __forceinline__ double trigamma_as121(double x) {
  if (x <= 0) return 0.0;
  if (x <= 0.0001) return 1.0 / x / x;
  double value = 0.0, z = x;
  while (z < 5.0) { value += 1.0 / z / z; z += 1.0; }
  const double y = 1.0 / z / z;
  value += 0.5 * y + (1.0 + y * (0.1666666667 + y * (-0.03333333333 + y * (0.02380952381 + y * -0.03333333333)))) / z;
  return value;
}
// Gamma :283 (C: tgamma): exact at the small integers like the C library's (ocml's tgamma(1) is one
// ulp low: truncating it into an integer output — gamma_inplace on an int64 array — gave 0)
__device__ inline double gamma_(double x) {
  if (x == floor(x) && x >= 1.0 && x <= 23.0) {
    double p = 1.0;
    for (int i = 2; i < (int)x; ++i) p *= (double)i;
    return p;
  }
  return tgamma(x);
}
__device__ inline float gamma_(float x) { return (float)gamma_((double)x); }
// I0 :1064 / I1 :1038 (scipy.special.i0 / i1): even / odd in x; the device library's routines are
// evaluated on |x|
__device__ inline double bessel_i0_(double x) { return cyl_bessel_i0(fabs(x)); }
__device__ inline float bessel_i0_(float x) { return cyl_bessel_i0f(fabsf(x)); }
__device__ inline double bessel_i1_(double x) { return copysign(cyl_bessel_i1(fabs(x)), x); }
__device__ inline float bessel_i1_(float x) { return copysignf(cyl_bessel_i1f(fabsf(x)), x); }
// Regularised incomplete gamma functions (GammaInc :580 / GammaIncC :629 / Chi2SF :538 / GammaU :836
// / GammaL :877: the reference's C bodies call GammaP / GammaQ / upperGamma / lowerGamma of
// scalar/c_code/gamma.c): the power series for x < k + 1, the continued fraction (modified Lentz)
// otherwise, both scaled by exp(k log x - x - lgamma(k)).  NaN for k <= 0 or x < 0 like the reference.
__device__ inline double igam_series_(double k, double x) {
  double term = 1.0 / k, sum = term, n = k;
  for (int i = 0; i < 1024; ++i) {
    n += 1.0; term *= x / n; sum += term;
    if (fabs(term) < fabs(sum) * 2.2204460492503131e-16) break;
  }
  return sum;
}
__device__ inline double igam_cfrac_(double k, double x) {
  const double tiny = 2.2204460492503131e-16 * 2.2204460492503131e-16 * 2.2204460492503131e-16;   // gamma.c TINY
  double b = x + 1.0 - k, c = 1.0 / tiny, d = 1.0 / b, f = d;
  for (int i = 1; i < 1024; ++i) {
    const double a = -(double)i * ((double)i - k);
    b += 2.0;
    d = a * d + b; if (fabs(d) < tiny) d = tiny;
    c = b + a / c; if (fabs(c) < tiny) c = tiny;
    d = 1.0 / d;
    const double e = d * c;
    f *= e;
    if (fabs(e - 1.0) < 2.2204460492503131e-16) break;
  }
  return f;
}
// upperGamma / lowerGamma of gamma.c: ALWAYS the continued fraction / the series (whatever x is)
__device__ inline double gamma_upper_(double k, double x) {
  if (!(k > 0.0) || !(x > 0.0)) return NAN;
  return igam_cfrac_(k, x) * exp(k * log(x) - x);
}
__device__ inline double gamma_lower_(double k, double x) {
  if (!(k > 0.0) || !(x > 0.0)) return NAN;
  return igam_series_(k, x) * exp(k * log(x) - x);
}
__device__ inline double gamma_p_(double k, double x) {
  if (!(k > 0.0) || !(x >= 0.0)) return NAN;
  if (x == 0.0) return 0.0;
  const double w = exp(k * log(x) - x - lgamma(k));
  return x < k + 1.0 ? igam_series_(k, x) * w : 1.0 - igam_cfrac_(k, x) * w;
}
__device__ inline double gamma_q_(double k, double x) {
  if (!(k > 0.0) || !(x >= 0.0)) return NAN;
  if (x == 0.0) return 1.0;
  const double w = exp(k * log(x) - x - lgamma(k));
  return x < k + 1.0 ? 1.0 - igam_series_(k, x) * w : igam_cfrac_(k, x) * w;
}
__device__ __forceinline__ float log1mexp_(float x) { return x < -0.6931471805599453f ? log1pf(-expf(x)) : logf(-expm1f(x)); }
__device__ __forceinline__ double log1mexp_(double x) { return x < -0.6931471805599453 ? log1p(-exp(x)) : log(-expm1(x)); }
__device__ __forceinline__ float round_away(float x) { return x < 0 ? ceilf(x - 0.5f) : floorf(x + 0.5f); }
__device__ __forceinline__ double round_away(double x) { return x < 0 ? ceil(x - 0.5) : floor(x + 0.5); }

// ---- float64 exp through a 64-entry table (Tang's scheme; tools/gen_exp_table.py prints the
// constants): x = (64 k + j) ln2/64 + r with |r| <= ln2/128, exp(x) = 2^k * T[j] * (1 + p(r)).
// T = 2^(j/64) correctly rounded, one copy per wavefront in LDS (no barrier: a wave reads only
// what it wrote).  |x| >= 708, infinities and NaN: the argument is clamped first and 2^k applied
// by v_ldexp_f64 (denormal results, overflow, underflow), behind a rare branch.  Measured
// against expl over 2e7 arguments: <= 1.02 ulp (the C library: 0.51, ocml's exp: 1).  Replaces
// Exp.c_code (scalar/basic.py:3102) `exp(x)` for float64 only.
__device__ const double AHIP_EXP2_64[64] = {
  0x1.0000000000000p+0, 0x1.02c9a3e778061p+0, 0x1.059b0d3158574p+0, 0x1.0874518759bc8p+0,
  0x1.0b5586cf9890fp+0, 0x1.0e3ec32d3d1a2p+0, 0x1.11301d0125b51p+0, 0x1.1429aaea92de0p+0,
  0x1.172b83c7d517bp+0, 0x1.1a35beb6fcb75p+0, 0x1.1d4873168b9aap+0, 0x1.2063b88628cd6p+0,
  0x1.2387a6e756238p+0, 0x1.26b4565e27cddp+0, 0x1.29e9df51fdee1p+0, 0x1.2d285a6e4030bp+0,
  0x1.306fe0a31b715p+0, 0x1.33c08b26416ffp+0, 0x1.371a7373aa9cbp+0, 0x1.3a7db34e59ff7p+0,
  0x1.3dea64c123422p+0, 0x1.4160a21f72e2ap+0, 0x1.44e086061892dp+0, 0x1.486a2b5c13cd0p+0,
  0x1.4bfdad5362a27p+0, 0x1.4f9b2769d2ca7p+0, 0x1.5342b569d4f82p+0, 0x1.56f4736b527dap+0,
  0x1.5ab07dd485429p+0, 0x1.5e76f15ad2148p+0, 0x1.6247eb03a5585p+0, 0x1.6623882552225p+0,
  0x1.6a09e667f3bcdp+0, 0x1.6dfb23c651a2fp+0, 0x1.71f75e8ec5f74p+0, 0x1.75feb564267c9p+0,
  0x1.7a11473eb0187p+0, 0x1.7e2f336cf4e62p+0, 0x1.82589994cce13p+0, 0x1.868d99b4492edp+0,
  0x1.8ace5422aa0dbp+0, 0x1.8f1ae99157736p+0, 0x1.93737b0cdc5e5p+0, 0x1.97d829fde4e50p+0,
  0x1.9c49182a3f090p+0, 0x1.a0c667b5de565p+0, 0x1.a5503b23e255dp+0, 0x1.a9e6b5579fdbfp+0,
  0x1.ae89f995ad3adp+0, 0x1.b33a2b84f15fbp+0, 0x1.b7f76f2fb5e47p+0, 0x1.bcc1e904bc1d2p+0,
  0x1.c199bdd85529cp+0, 0x1.c67f12e57d14bp+0, 0x1.cb720dcef9069p+0, 0x1.d072d4a07897cp+0,
  0x1.d5818dcfba487p+0, 0x1.da9e603db3285p+0, 0x1.dfc97337b9b5fp+0, 0x1.e502ee78b3ff6p+0,
  0x1.ea4afa2a490dap+0, 0x1.efa1bee615a27p+0, 0x1.f50765b6e4540p+0, 0x1.fa7c1819e90d8p+0,
};
__device__ __forceinline__ double exp_tbl64(double x, const double* tbl) {
  const bool big = ((unsigned)__double2hiint(x) & 0x7fffffffu) >= 0x40862000u;   // |x| >= 708, inf, NaN
  double xc = x;
  if (__builtin_expect(big, 0)) {
    asm volatile("" ::: "memory");   // rare: keep it a branch (no if-conversion into the hot path)
    xc = fmin(fmax(x, -1000.0), 1000.0);
  }
  double s;                                                     // x * 64/ln2 + 1.5 * 2^52: k lands in the low word
  asm("v_fma_f64 %%0, %%1, %%2, %%3" : "=v"(s) : "v"(xc), "v"(0x1.71547652b82fep+6), "s"(0x1.8p+52));
  const int ki = __double2loint(s);
  const double kd = s - 0x1.8p+52;
  double r = fma(kd, -0x1.62e42ff000000p-7, xc);                // k * C1 is exact (33-bit C1)
  r = fma(kd, 0x1.718432a1b0e26p-41, r);
  const double T = tbl[ki & 63];
  const double r2 = r * r;
  // Horner steps with a constant addend as three-address v_fma_f64 with the constant in an
  // SGPR pair (the compiler's two-address v_fmac_f64 copies the constant into the destination
  // first: one v_mov_b64 per step)
  double q;
  asm("v_fma_f64 %%0, %%1, %%2, %%3" : "=v"(q) : "v"(r), "s"(0x1.11111d8fbe766p-7), "v"(0x1.55556b3304ec0p-5));
  asm("v_fma_f64 %%0, %%1, %%2, %%3" : "=v"(q) : "v"(q), "v"(r), "s"(0x1.5555555555255p-3));
  asm("v_fma_f64 %%0, %%1, %%2, %%3" : "=v"(q) : "v"(q), "v"(r), "s"(0x1.ffffffffff57fp-2));
  const double p = fma(r2, q, r);
  const double m = fma(T, p, T);                                // T * e^r, in [0.99, 2.01)
  // |x| < 708: the result is a normal number and 2^k is an add into the exponent field
  int hi;
  asm("v_lshl_add_u32 %%0, %%1, 14, %%2" : "=v"(hi) : "v"(ki & ~63), "v"(__double2hiint(m)));
  double res = __hiloint2double(hi, __double2loint(m));
  if (__builtin_expect(big, 0)) {
    asm volatile("" ::: "memory");
    res = ldexp(m, ki >> 6);        // denormal results, overflow to inf, underflow to 0
    if (x != x) res = x;
  }
  return res;
}

// ---- cross-lane reduction plumbing (64-wide wavefronts) ----
template <typename T> __device__ __forceinline__ T shfl_xor_(T v, int m) {
  if constexpr (sizeof(T) == 8) {
    union { T t; int i[2]; } u; u.t = v;
    u.i[0] = __shfl_xor(u.i[0], m, 64); u.i[1] = __shfl_xor(u.i[1], m, 64);
    return u.t;
  } else if constexpr (sizeof(T) == 4) {
    union { T t; int i; } u; u.t = v; u.i = __shfl_xor(u.i, m, 64); return u.t;
  } else {
    int i = (int)v; i = __shfl_xor(i, m, 64); return (T)i;
  }
}
// DPP move of a whole value (32-bit pieces): ctrl 0xB1 / 0x4E = quad_perm [1,0,3,2] / [2,3,0,1],
// 0x141 = row_half_mirror, 0x140 = row_mirror.  After combining with these four in turn every lane
// of a 16-lane row holds the row's fold; lane_get_ then reads the four row leaders (uniform).
template <typename T, int CTRL> __device__ __forceinline__ T dpp_mov_(T v) {
  if constexpr (sizeof(T) == 8) {
    union { T t; int i[2]; } u; u.t = v;
    u.i[0] = __builtin_amdgcn_update_dpp(u.i[0], u.i[0], CTRL, 0xf, 0xf, false);
    u.i[1] = __builtin_amdgcn_update_dpp(u.i[1], u.i[1], CTRL, 0xf, 0xf, false);
    return u.t;
  } else if constexpr (sizeof(T) == 4) {
    union { T t; int i; } u; u.t = v;
    u.i = __builtin_amdgcn_update_dpp(u.i, u.i, CTRL, 0xf, 0xf, false);
    return u.t;
  } else {
    int i = (int)v; i = __builtin_amdgcn_update_dpp(i, i, CTRL, 0xf, 0xf, false); return (T)i;
  }
}
template <typename T> __device__ __forceinline__ T lane_get_(T v, int lane) {
  if constexpr (sizeof(T) == 8) {
    union { T t; int i[2]; } u; u.t = v;
    u.i[0] = __builtin_amdgcn_readlane(u.i[0], lane); u.i[1] = __builtin_amdgcn_readlane(u.i[1], lane);
    return u.t;
  } else if constexpr (sizeof(T) == 4) {
    union { T t; int i; } u; u.t = v; u.i = __builtin_amdgcn_readlane(u.i, lane); return u.t;
  } else {
    int i = (int)v; i = __builtin_amdgcn_readlane(i, lane); return (T)i;
  }
}
""" % (AHIP_MAXD, AHIP_MAXOPS)
