// exact_sqrt.h -- the correctly rounded binary32 square root from ONE v_rsq_f32 seed, and Normalize's length and three quotients from that same
// seed: host and device.
//
// hipcc lowers `__builtin_sqrtf(x)` to sixteen VALU instructions: a scale by 2^32 for tiny operands (v_mul, v_cmp, v_cndmask), v_sqrt_f32, the
// two integer neighbours of its result, two residual fma, two v_cmp + v_cndmask pairs that pick among the three candidates, the un-scale
// (v_mul, v_cndmask) and v_cmp_class + v_cndmask for 0 and inf: five compare/select pairs, which are most of its price.  For an operand of
// ordinary magnitude none of them is needed.  From r, an approximation of 1 / sqrt(x) (device: v_rsq_f32, good to one ulp):
//     g = x r;   h = r / 2;                                               g ~ sqrt(x), h ~ 1 / (2 sqrt(x)), each to a few ulp
//     e = fma(-h, g, 1/2);   g = fma(g, e, g);   h = fma(h, e, h);        one coupled Newton step: both now good to well under an ulp
//     d = fma(-g, g, x);     s = fma(d, h, g)                             the residual of g, EXACT, and the final correction
// (ExactSqrt).  The last fma rounds g + d h, which differs from sqrt(x) by about (d h)^2 / (2 g), some 2^-46 g, and the square root of a
// binary32 number is never a midpoint of two floats; that it never lies THAT close to one is what the exhaustive check establishes.  The textbook
// sequence (Markstein; the same steps close the compiler's own binary64 sqrt); what makes it usable HERE is that a one-operand function can be
// checked exhaustively: tests/test_exact_sqrt.py runs all 2^24 operands of two adjacent binades (both exponent parities: every other binade
// is one of the two scaled by a power of four, and every operation above scales with it exactly) with the seed at the float nearest to
// 1 / sqrt(x) and at every offset from -3 to +3 ulp of it, every mantissa of the lowest and of the highest binade of the range below, and strided
// mantissas of every binade between; tests/test_exact_sqrt_gpu.py compares the device's bits with __builtin_sqrtf over ALL 2^32 bit patterns
// and reports how far v_rsq_f32 lies from the nearest float (inside that window).  The result has sqrtf's bits; what changes is the price.
//
// THE RANGE in which no intermediate leaves the normal numbers (ExactSqrtSafe*):     2^-60 <= x < 2^60
// (+0, -0, negative numbers, subnormals, inf and NaN are outside)
//   * r: 2^-30 < r <= 2^30; g and s: 2^-30 <= . < 2^30; h: 2^-31 < h <= 2^29.  All normal.
//   * e = 1/2 - h g: h g is within 2^-21 of 1/2, so |e| < 2^-21, and it is a multiple of ulp(h) ulp(g) >= 2^-24 2^-24 h g / 4 > 2^-52: normal or zero.
//   * d = x - g g is exact in binary32 when g is within an ulp of sqrt(x) (the residual lemma) PROVIDED it is not below the normal range: it
//     is a multiple of ulp(g)^2 >= 2^-48 g^2 / 4 >= 2^-50 x >= 2^-110: normal or zero.  |d h| <= ulp(g): the last fma is far from any limit.
// Outside the range the caller evaluates __builtin_sqrtf (device: the whole wave does, Sqrt1 / Sqrt2 / NormalizeFused below).  A 24-bit
// uniform that comes out 0 (2^-24 per lane, 2^-18 per wave) is the everyday operand outside the range and simply takes that path.
//
// NORMALIZE.  l = sqrt(s), s = x x + y y + z z, then x / l, y / l, z / l through shared_div.h, whose reciprocal starts from v_rcp_f32(l).
// The refined h above is 1 / (2 l) to well under an ulp of the TRUE root, so h + h (exact) is within 2 ulp of RN(1 / l) -- l itself is
// rounded, which moves 1 / l by up to half an ulp -- and can stand in for that seed: v_rcp_f32 disappears, and one guard serves the root
// and the three quotients (ExactNormalizeSafe: 2^-40 <= s < 2^60, so that 2^-20 <= l < 2^30 lies inside shared_div.h's range for a
// denominator; components +-0 or at least 2^-60 as there; they need no upper bound, as there).  shared_div.h's statement covers seeds to one
// ulp; tests/test_exact_sqrt.py runs SharedReciprocal<true> + SharedQuotient<true> from h + h and from every offset to +-3 ulp of it over 1e8
// vectors (a third of them of unit length already, where l has the all-ones mantissa whose reciprocal comes from its bits) against `/`.
#pragma once
#include "shared_div.h"

namespace exact_sqrt {

using shared_div::Bits;
using shared_div::FromBits;

constexpr uint32_t kLo = (127u - 60u) << 23, kHi = (127u + 60u) << 23;          // bits of 2^-60, 2^60
constexpr uint32_t kSumLo = (127u - 40u) << 23;                                 // bits of 2^-40: Normalize's sum of squares

// seed: an approximation of 1 / sqrt(x) (device: v_rsq_f32).  half_reciprocal: the refined h ~ 1 / (2 sqrt(x)).
AMBER_SHARED_DIV_FN float ExactSqrt(float x, float seed, float& half_reciprocal) {
  float g = x * seed;
  float h = 0.5f * seed;
  const float e = __builtin_fmaf(-h, g, 0.5f);
  g = __builtin_fmaf(g, e, g);
  h = __builtin_fmaf(h, e, h);
  const float d = __builtin_fmaf(-g, g, x);
  half_reciprocal = h;
  return __builtin_fmaf(d, h, g);
}
AMBER_SHARED_DIV_FN float ExactSqrt(float x, float seed) { float h; return ExactSqrt(x, seed, h); }

// The guards, in integer keys: bits - bits(2^-60) as an unsigned number is below the span for the range and for nothing else (a set sign
// bit, zero and the subnormals wrap to the top; inf and NaN lie above).  Two operands: the larger key decides (v_max_u32, one compare).
AMBER_SHARED_DIV_FN bool ExactSqrtSafe(float x) { return Bits(x) - kLo < kHi - kLo; }
AMBER_SHARED_DIV_FN bool ExactSqrtSafe2(float a, float b) {
  const uint32_t ka = Bits(a) - kLo, kb = Bits(b) - kLo;
  return (ka > kb ? ka : kb) < kHi - kLo;
}
// Normalize: s the rounded sum of squares of (x, y, z).  The numerators' test is shared_div.h's (the sign bit of room_low: one too small).
AMBER_SHARED_DIV_FN bool ExactNormalizeSafe(float x, float y, float z, float s) {
  using namespace shared_div;
  const uint32_t room_low = static_cast<uint32_t>(Min3(NumeratorKey(x), NumeratorKey(y), NumeratorKey(z)) - static_cast<int32_t>(kNumLo - 1u));
  const uint32_t span = Bits(s) - kSumLo;
  return ((room_low & ~kAbsMask) | span) < kHi - kSumLo;
}
// x / l, y / l, z / l for l = ExactSqrt(s, seed, h): the reciprocal's seed is h + h (reciprocal_seed: the host check moves it by whole ulps).
AMBER_SHARED_DIV_FN void QuotientsByRoot(float x, float y, float z, float l, float reciprocal_seed, float& qx, float& qy, float& qz) {
  const float r = shared_div::SharedReciprocal<true>(l, reciprocal_seed);
  qx = shared_div::SharedQuotient<true>(x, l, r); qy = shared_div::SharedQuotient<true>(y, l, r); qz = shared_div::SharedQuotient<true>(z, l, r);
}

}  // namespace exact_sqrt

#if defined(__HIPCC__)
namespace exact_sqrt {
// As shared_div.h's Div3: the fast form first; if ANY active lane is out of range the whole wave evaluates __builtin_sqrtf in place (one
// v_cmp into vcc and a branch: no scalar register is held) and gets the bits it always had.
__device__ __forceinline__ float Sqrt1(float x) {
  float s = ExactSqrt(x, __builtin_amdgcn_rsqf(x));
  if (__builtin_expect(__any(!ExactSqrtSafe(x)), 0)) s = __builtin_sqrtf(x);
  return s;
}
// two roots under one guard and one vote (the lobe's sqrt(r0), sqrt(1 - r0))
__device__ __forceinline__ void Sqrt2(float a, float b, float& sa, float& sb) {
  sa = ExactSqrt(a, __builtin_amdgcn_rsqf(a)); sb = ExactSqrt(b, __builtin_amdgcn_rsqf(b));
  if (__builtin_expect(__any(!ExactSqrtSafe2(a, b)), 0)) { sa = __builtin_sqrtf(a); sb = __builtin_sqrtf(b); }
}
// (x, y, z) / sqrt(s), s their rounded sum of squares: one v_rsq_f32, no v_rcp_f32, one guard for the root and the three quotients
__device__ __forceinline__ void NormalizeFused(float x, float y, float z, float s, float& qx, float& qy, float& qz) {
  float h;
  const float l = ExactSqrt(s, __builtin_amdgcn_rsqf(s), h);
  QuotientsByRoot(x, y, z, l, h + h, qx, qy, qz);
  if (__builtin_expect(__any(!ExactNormalizeSafe(x, y, z, s)), 0)) { const float lp = __builtin_sqrtf(s); qx = x / lp; qy = y / lp; qz = z / lp; }
}
}  // namespace exact_sqrt
#endif
