// shared_div.h -- correctly rounded binary32 quotients of several numerators by ONE denominator, at one reciprocal per denominator: host and device.
//
// hipcc lowers every binary32 `n / d` to eleven VALU instructions: two v_div_scale_f32 (which pre-scale operands whose quotient, reciprocal or
// residual would leave the normal range), v_rcp_f32, two fma that refine the reciprocal, a multiply and two residual/correction pairs (the last
// correction being v_div_fmas_f32, which undoes the scaling), and v_div_fixup_f32 (zero, inf, NaN, and the sign of a zero quotient).  Three
// quotients by the same d -- Normalize, a triangle's u, v, t by det -- repeat the scaling, the reciprocal and its refinement three times.
// For operands of ordinary magnitude v_div_scale_f32 returns its input, v_div_fmas_f32 is a plain fma and v_div_fixup_f32 passes its input
// through: what is left is
//     y = rcp(d);  e = fma(-d, y, 1);  y = fma(e, y, y)                                          once per denominator   (SharedReciprocal)
//     q = n * y;   r = fma(-d, q, n);  q = fma(r, y, q);   r = fma(-d, q, n);  q = fma(r, y, q)    per numerator          (SharedQuotient)
// the compiler's own operations in the compiler's own order, on the same v_rcp_f32 seed: the quotient has the bits the plain `n / d` has on
// this device.  That those bits are RN(n / d) whatever the last bit of the seed holds for every denominator but those with a mantissa of
// ALL ONES, the classical exception of the fma refinement (Markstein) -- and Normalize's everyday case: the rounded length of a vector that
// is already unit length up to rounding is 0x1.fffffep-1 for about three lanes in ten.  There 1 / d = 2^-k (1 + 2^-24 + 2^-48 ...) lies just
// above a midpoint; from a seed of 2^-k the refined reciprocal, and then +-2^j times it corrected, are ties that round back to even, and the
// sequence returns 2^(j-k) where the quotient is one ulp above.  For that denominator SharedReciprocal therefore does not refine: it
// returns RN(1 / d) itself, 2^-k (1 + 2^-23), whose bits are 0x7f000000 - bits(|d|) (an integer subtraction and a select; the refinement
// of v_rcp_f32's seed gives the same float on this device, or the plain operator would miss +-2^j / d, and it does not).  On the host
// (tests/test_shared_division.py, 1e8 pairs of the range below) the sequence equals `n / d` with the seed at RN(1 / d) and one ulp either
// side.  tests/test_shared_division_gpu.py compares the device's bits with the plain operator's and with the correctly rounded quotient
// over all 2^23 mantissas of the denominator and the all-ones denominators of every binade.
//
// THE RANGE in which nothing is scaled and nothing leaves the normal numbers (SharedDivSafe*):
//     2^-20 <= |d| < 2^40,     every numerator is +-0 or 2^-60 <= |n| < 2^41          (inf and NaN are outside)
//   * y: 2^-40 < |1 / d| <= 2^20, normal; e = 1 - d y is 0 or a multiple of 2^-48 (ulp(d) ulp(y) >= 2^-24 2^-24 |d y|): normal or zero.
//   * q: 2^-100 <= |n / d| < 2^61, normal, far from overflow.
//   * r = n - d q is exact in binary32 when q is within an ulp of n / d (the classical residual lemma) PROVIDED it is not below the normal
//     range: it is a multiple of ulp(d) ulp(q) >= 2^-46 |d q| / 4 >= 2^-48 |n| >= 2^-108: normal or zero.
//   * v_div_scale_f32 scales when d is subnormal, when 1 / d or n / d is subnormal, when the exponents of n and d differ by 96 or more, or when
//     n's biased exponent is 23 or less (|n| < 2^-103): none of these inside the range (exponent difference at most 41 + 20 = 61).
//   * a numerator +-0: q = +-0, r and the corrections are zeros whose sign depends on the addition order; v_div_fixup_f32 returns the zero of
//     sign(n) ^ sign(d), and so does the last line of SharedQuotient, for every numerator (a no-op on a non-zero quotient).
// Outside the range the caller evaluates the plain `n / d` expressions (device: the whole wave does, Div3 / Div2 / DivByLength below).
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AMBER_SHARED_DIV_FN __host__ __device__ inline
#else
#define AMBER_SHARED_DIV_FN inline
#endif

namespace shared_div {

constexpr uint32_t kAbsMask = 0x7fffffffu;
constexpr uint32_t kDenLo = (127u - 20u) << 23, kDenHi = (127u + 40u) << 23;      // bits of 2^-20, 2^40
constexpr uint32_t kNumLo = (127u - 60u) << 23, kNumHi = (127u + 41u) << 23;      // bits of 2^-60, 2^41

AMBER_SHARED_DIV_FN uint32_t Bits(float x) { uint32_t b; memcpy(&b, &x, 4); return b; }
AMBER_SHARED_DIV_FN float FromBits(uint32_t b) { float x; memcpy(&x, &b, 4); return x; }

// seed: an approximation of 1 / d good to one ulp (device: v_rcp_f32).  kPositiveD: the caller knows d > 0 (a length).
// A mantissa of all ones: |d| = 2^E (2 - 2^-23) with bits (E + 127) << 23 | 0x7fffff, RN(1 / |d|) = 2^(-E-1) (1 + 2^-23) with bits
// (126 - E) << 23 | 1 = 0x7f000000 - bits(|d|); normal for every d of the range.
template <bool kPositiveD = false>
AMBER_SHARED_DIV_FN float SharedReciprocal(float d, float seed) {
  const float e = __builtin_fmaf(-d, seed, 1.0f);
  const float y = __builtin_fmaf(e, seed, seed);
  const uint32_t b = Bits(d);
  const uint32_t exact = kPositiveD ? 0x7f000000u - b : ((0x7f000000u - (b & kAbsMask)) | (b & ~kAbsMask));
  return (b | 0xff800000u) == 0xffffffffu ? FromBits(exact) : y;
}
// n / d, given y = SharedReciprocal(d, .).  kPositiveD: the caller knows d > 0 (a length), the quotient takes n's sign.
template <bool kPositiveD = false>
AMBER_SHARED_DIV_FN float SharedQuotient(float n, float d, float y) {
  float q = n * y;
  float r = __builtin_fmaf(-d, q, n);
  q = __builtin_fmaf(r, y, q);
  r = __builtin_fmaf(-d, q, n);
  q = __builtin_fmaf(r, y, q);
  const uint32_t sign = (kPositiveD ? Bits(n) : Bits(n) ^ Bits(d)) & ~kAbsMask;
  return FromBits((Bits(q) & kAbsMask) | sign);
}

// The guard, in integer keys.  A numerator's key (bits - 1) & 0x7fffffff is |n|'s bit pattern less one, and puts +-0 at the TOP (0x7fffffff):
// "n is +-0 or |n| >= 2^-60" is one signed lower bound on the key, and the smallest key of a group decides it for the group (v_min3_i32).
AMBER_SHARED_DIV_FN int32_t NumeratorKey(float n) { return static_cast<int32_t>((Bits(n) - 1u) & kAbsMask); }
AMBER_SHARED_DIV_FN int32_t Min3(int32_t a, int32_t b, int32_t c) { const int32_t m = a < b ? a : b; return m < c ? m : c; }
AMBER_SHARED_DIV_FN uint32_t Max3(uint32_t a, uint32_t b, uint32_t c) { const uint32_t m = a > b ? a : b; return m > c ? m : c; }

// Any signs.  Both bounds of d ride along with the numerators': d's magnitude is moved by the (constant) distance between its bound and the
// numerators' bound, so that ONE signed minimum carries every lower bound and ONE unsigned maximum every upper bound; a single compare decides.
AMBER_SHARED_DIV_FN bool SharedDivSafe3(float a, float b, float c, float d) {
  const uint32_t ad = Bits(d) & kAbsMask;
  const int32_t low = Min3(NumeratorKey(a), NumeratorKey(b), NumeratorKey(c));
  const int32_t low_d = static_cast<int32_t>(ad) - static_cast<int32_t>(kDenLo - kNumLo) - 1;             // d = 2^-20 has the key of n = 2^-60; |d| = 0 goes negative
  const uint32_t high = Max3(Bits(a) & kAbsMask, Bits(b) & kAbsMask, Bits(c) & kAbsMask);
  const uint32_t high_d = ad + (kNumHi - kDenHi);                                                          // d = 2^40 has the bits of n = 2^41 (no wrap: ad < 2^31)
  const int32_t room_low = (low < low_d ? low : low_d) - static_cast<int32_t>(kNumLo - 1u);               // >= 0: every lower bound holds
  const int32_t room_high = static_cast<int32_t>(kNumHi - 1u - (high > high_d ? high : high_d));         // >= 0: every upper bound holds (the maximum is below 2^31 + 2^23: no wrap either)
  return (room_low < room_high ? room_low : room_high) >= 0;
}
AMBER_SHARED_DIV_FN bool SharedDivSafe2(float a, float b, float d) { return SharedDivSafe3(a, b, b, d); }

// Normalize's guard: the denominator is l = sqrt(x x + y y + z z), rounded after every operation.  l is +0, positive or NaN, so the test of
// d is one unsigned compare of (bits - bits(2^-20)) that also rejects a set sign bit; and the numerators need no upper bound: for l in range
// the sum of squares is below 2^80 (nothing overflowed), each rounded square is at most the rounded sum times (1 + 2^-23), so
// |x|, |y|, |z| <= l (1 + 2^-22) < 2^41.
AMBER_SHARED_DIV_FN bool SharedNormalizeSafe(float x, float y, float z, float l) {
  const uint32_t room_low = static_cast<uint32_t>(Min3(NumeratorKey(x), NumeratorKey(y), NumeratorKey(z)) - static_cast<int32_t>(kNumLo - 1u));   // sign bit set: a numerator too small
  const uint32_t span = Bits(l) - kDenLo;                                                                   // < kDenHi - kDenLo: l in range
  return ((room_low & ~kAbsMask) | span) < kDenHi - kDenLo;
}

}  // namespace shared_div

#if defined(__HIPCC__)
namespace shared_div {
// The wave keeps the fast path's quotients only when EVERY active lane is in range (one v_cmp into vcc and a branch: no scalar register is
// held); otherwise the whole wave evaluates the plain expressions, in place, and gets today's bits.  The source computes the fast path first
// and lets the fallback overwrite it: on operands out of range the fast path produces values nobody reads, and the compiler is free to
// sink it into the other arm (it does).
__device__ __forceinline__ void Div3(float a, float b, float c, float d, float& qa, float& qb, float& qc) {
  const float y = SharedReciprocal(d, __builtin_amdgcn_rcpf(d));
  qa = SharedQuotient(a, d, y); qb = SharedQuotient(b, d, y); qc = SharedQuotient(c, d, y);
  if (__builtin_expect(__any(!SharedDivSafe3(a, b, c, d)), 0)) { qa = a / d; qb = b / d; qc = c / d; }
}
__device__ __forceinline__ void Div2(float a, float b, float d, float& qa, float& qb) {
  const float y = SharedReciprocal(d, __builtin_amdgcn_rcpf(d));
  qa = SharedQuotient(a, d, y); qb = SharedQuotient(b, d, y);
  if (__builtin_expect(__any(!SharedDivSafe2(a, b, d)), 0)) { qa = a / d; qb = b / d; }
}
// x / l, y / l, z / l for l = the rounded length of (x, y, z)
__device__ __forceinline__ void DivByLength(float x, float y, float z, float l, float& qx, float& qy, float& qz) {
  const float r = SharedReciprocal<true>(l, __builtin_amdgcn_rcpf(l));
  qx = SharedQuotient<true>(x, l, r); qy = SharedQuotient<true>(y, l, r); qz = SharedQuotient<true>(z, l, r);
  if (__builtin_expect(__any(!SharedNormalizeSafe(x, y, z, l)), 0)) { qx = x / l; qy = y / l; qz = z / l; }
}
}  // namespace shared_div
#endif
