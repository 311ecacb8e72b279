// Host check of amber_amd/csrc/hip/shared_div.h (tests/test_shared_division.py builds and runs it; nothing of the library, nothing loaded into python).
//   shared_division_main [pairs]      default 100 000 000 random (numerator, denominator) pairs inside the guard's range
// Every pair runs with the reciprocal seed at RN(1 / d) and one ulp either side of it (v_rcp_f32 is good to one ulp) and must equal `n / d`,
// which the host divides correctly rounded.  Then the guards against a plain float statement of the range, at and around every boundary and
// on random bit patterns, and Normalize's quotients on random vectors.  Prints the first mismatches and one summary line; exit status 1 on any error.
#include <initializer_list>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "shared_div.h"

using namespace shared_div;

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t Next() { g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17; return static_cast<uint32_t>(g_state >> 32); }

static float Make(uint32_t sign, int exponent, uint32_t mantissa) { return FromBits((sign << 31) | (static_cast<uint32_t>(exponent + 127) << 23) | (mantissa & 0x7fffffu)); }
static uint32_t Mantissa(uint32_t r) {            // random, with all-zeros and all-ones and their neighbours over-represented
  switch (r & 15u) { case 0: return 0u; case 1: return 0x7fffffu; case 2: return 1u; case 3: return 0x7ffffeu; default: return Next(); }
}
static float Denominator() { const uint32_t r = Next(); return Make(r >> 31, -20 + static_cast<int>((r >> 8) % 60u), Mantissa(r)); }
static float Numerator() { const uint32_t r = Next(); return Make(r >> 31, -60 + static_cast<int>((r >> 8) % 101u), Mantissa(r)); }

static unsigned long long g_pairs = 0, g_mismatches[3] = {0, 0, 0};       // per seed: RN(1 / d), one ulp below it (in magnitude), one ulp above
static void CheckPair(float n, float d) {
  const float want = n / d, rn = 1.0f / d;
  const float seeds[3] = {rn, FromBits(Bits(rn) - 1u), FromBits(Bits(rn) + 1u)};
  for (int s = 0; s < 3; s++) {
    const float y = SharedReciprocal(d, seeds[s]);
    const float got = SharedQuotient(n, d, y);
    bool bad = Bits(got) != Bits(want);
    if (d > 0.0f) bad = bad || Bits(SharedQuotient<true>(n, d, y)) != Bits(want) || Bits(SharedReciprocal<true>(d, seeds[s])) != Bits(y);      // the forms for a known-positive d
    if (bad) { if (g_mismatches[s] < 4) printf("MISMATCH n=%a d=%a seed=%a (RN %+d ulp) got=%a want=%a\n", n, d, seeds[s], s == 0 ? 0 : (s == 1 ? -1 : 1), got, want); g_mismatches[s]++; }
  }
  g_pairs++;
}

// the range, said plainly
static bool DenInRange(float d) { const float a = fabsf(d); return a >= 0x1p-20f && a < 0x1p40f; }
static bool NumInRange(float n) { const float a = fabsf(n); return a == 0.0f || (a >= 0x1p-60f && a < 0x1p41f); }
static unsigned long long g_guard_cases = 0, g_guard_errors = 0;
static void CheckGuard(float a, float b, float c, float d) {
  const bool want = DenInRange(d) && NumInRange(a) && NumInRange(b) && NumInRange(c);
  if (SharedDivSafe3(a, b, c, d) != want || SharedDivSafe2(a, b, d) != (DenInRange(d) && NumInRange(a) && NumInRange(b))) {
    if (g_guard_errors < 10) printf("GUARD a=%a b=%a c=%a d=%a want %d\n", a, b, c, d, want);
    g_guard_errors++;
  }
  g_guard_cases++;
}
static float Length(float x, float y, float z) { const float s = x * x + y * y + z * z; return sqrtf(s); }      // -ffp-contract=off: every operation rounds
static void CheckNormalize(float x, float y, float z) {
  const float l = Length(x, y, z);
  const bool want = l >= 0x1p-20f && l < 0x1p40f && (x == 0.0f || fabsf(x) >= 0x1p-60f) && (y == 0.0f || fabsf(y) >= 0x1p-60f) && (z == 0.0f || fabsf(z) >= 0x1p-60f);
  const bool got = SharedNormalizeSafe(x, y, z, l);
  bool bad = got != want;
  if (got) {
    bad = bad || !(fabsf(x) < 0x1p41f && fabsf(y) < 0x1p41f && fabsf(z) < 0x1p41f);                              // the bound the guard does not test
    const float r = SharedReciprocal<true>(l, 1.0f / l);
    bad = bad || Bits(SharedQuotient<true>(x, l, r)) != Bits(x / l) || Bits(SharedQuotient<true>(y, l, r)) != Bits(y / l) || Bits(SharedQuotient<true>(z, l, r)) != Bits(z / l);
  }
  if (bad) { if (g_guard_errors < 10) printf("NORMALIZE x=%a y=%a z=%a l=%a want %d got %d\n", x, y, z, l, want, got); g_guard_errors++; }
  g_guard_cases++;
}

int main(int argc, char** argv) {
  const unsigned long long n_pairs = argc > 1 ? strtoull(argv[1], nullptr, 10) : 100000000ull;
  // ---- quotients: structured pairs, then random ones
  unsigned long long zero_sign_errors = 0;
  for (int k = 0; k < 4096; k++) {
    const float d = Denominator();
    for (int u = -2; u <= 2; u++) {                                     // n within 2 ulp of d, of either sign; quotients next to 1
      const float n = FromBits(Bits(d) + static_cast<uint32_t>(u));
      if (DenInRange(n)) { CheckPair(n, d); CheckPair(-n, d); }
    }
    for (float z : {0.0f, -0.0f}) {                                     // +-0 / d keeps the IEEE sign
      const float y = SharedReciprocal(d, 1.0f / d);
      if (Bits(SharedQuotient(z, d, y)) != Bits(z / d)) zero_sign_errors++;
      if (d > 0.0f && Bits(SharedQuotient<true>(z, d, y)) != Bits(z / d)) zero_sign_errors++;
      CheckPair(z, d);
    }
  }
  for (int en = -60; en < 41; en++)                                     // every exponent pair with the extreme mantissas
    for (int ed = -20; ed < 40; ed++)
      for (uint32_t mn : {0u, 1u, 0x7ffffeu, 0x7fffffu, 0x400000u})
        for (uint32_t md : {0u, 1u, 0x7ffffeu, 0x7fffffu, 0x400000u}) { CheckPair(Make(0, en, mn), Make(0, ed, md)); CheckPair(Make(1, en, mn), Make(0, ed, md)); CheckPair(Make(0, en, mn), Make(1, ed, md)); }
  while (g_pairs < n_pairs) {
    const float d = Denominator(), n = Numerator();
    if (!SharedDivSafe3(n, n, n, d)) { g_guard_errors++; continue; }    // generated inside the range: the guard must accept it
    CheckPair(n, d);
  }
  // ---- the guards: one ulp inside and outside every boundary, in every slot; zeros, subnormals, inf, NaN; random bit patterns
  const float special[] = {0.0f, -0.0f, FromBits(1u), FromBits(0x007fffffu), FromBits(0x00800000u), INFINITY, -INFINITY, NAN, -NAN, FromBits(0x7f800001u), FromBits(0x7f7fffffu),
                           0x1p-20f, FromBits(Bits(0x1p-20f) - 1u), FromBits(Bits(0x1p-20f) + 1u), 0x1p40f, FromBits(Bits(0x1p40f) - 1u), FromBits(Bits(0x1p40f) + 1u),
                           0x1p-60f, FromBits(Bits(0x1p-60f) - 1u), FromBits(Bits(0x1p-60f) + 1u), 0x1p41f, FromBits(Bits(0x1p41f) - 1u), FromBits(Bits(0x1p41f) + 1u), 1.0f, 3.0f,
                           0x1.fffffep0f, 0x1.fffffcp0f, 0x1.fffffep-1f, 0x1.fffffep-20f, 0x1.fffffep39f, 0x1.fffffep-60f};        // all-ones mantissas (and the one below) at the boundaries and between
  const int n_special = static_cast<int>(sizeof special / sizeof special[0]);
  for (int sa = 0; sa < 2; sa++)
    for (int i = 0; i < n_special; i++)
      for (int j = 0; j < n_special; j++) {
        const float v = sa ? -special[i] : special[i], w = special[j];
        CheckGuard(v, 1.0f, -2.0f, w); CheckGuard(1.0f, v, -2.0f, w); CheckGuard(1.0f, -2.0f, v, w); CheckGuard(v, v, v, w); CheckGuard(w, 1.0f, 1.0f, v);
        CheckNormalize(v, w, 0.0f); CheckNormalize(0.0f, v, w); CheckNormalize(w, 1.0f, v); CheckNormalize(v, 0.0f, 0.0f);
      }
  for (int k = 0; k < 4000000; k++) {
    const uint32_t r = Next();
    // any bit pattern in one slot, in-range values elsewhere; then any bit patterns everywhere
    const float any = FromBits(Next());
    switch (r & 3u) { case 0: CheckGuard(any, Numerator(), Numerator(), Denominator()); break; case 1: CheckGuard(Numerator(), any, Numerator(), Denominator()); break;
                      case 2: CheckGuard(Numerator(), Numerator(), any, Denominator()); break; default: CheckGuard(Numerator(), Numerator(), Numerator(), any); }
    CheckGuard(FromBits(Next()), FromBits(Next()), FromBits(Next()), FromBits(Next()));
    CheckNormalize(FromBits(Next()), FromBits(Next()), FromBits(Next()));
    CheckNormalize(Numerator(), Numerator(), Numerator());
    const float s = Make(0, static_cast<int>((r >> 8) % 100u) - 50, 0u);       // vectors of scene magnitude at many scales, components next to zero included
    CheckNormalize(s * (static_cast<float>(Next() >> 8) * 0x1p-23f - 1.0f), s * (static_cast<float>(Next() >> 8) * 0x1p-23f - 1.0f), (r & 4u) ? 0.0f : s * 0x1p-30f);
  }
  printf("pairs checked %llu, mismatches with the seed at RN %llu, one ulp below %llu, one ulp above %llu, zero sign errors %llu, guard cases %llu, guard errors %llu\n",
         g_pairs, g_mismatches[0], g_mismatches[1], g_mismatches[2], zero_sign_errors, g_guard_cases, g_guard_errors);
  return (g_mismatches[0] || g_mismatches[1] || g_mismatches[2] || zero_sign_errors || g_guard_errors) ? 1 : 0;
}
