// Host check of amber_amd/csrc/hip/exact_sqrt.h (tests/test_exact_sqrt.py builds and runs it; nothing of the library, nothing loaded into python).
//   exact_sqrt_main [vectors [stride]]      default 100 000 000 vectors, mantissa stride 1 (every mantissa of the exhaustive binades)
// Roots: ExactSqrt must equal sqrtf, which the host rounds correctly, with the seed at the float nearest to 1 / sqrt(x) and at every offset
// from -3 to +3 ulp of it: every mantissa of [1, 2) and [2, 4) (both exponent parities), every mantissa of the lowest and the highest binade of
// the guard's range, strided mantissas of every binade between.  Then the guards against a plain float statement of the range, and
// Normalize: the length from ExactSqrt, the three quotients from a reciprocal seeded with h + h moved by -3 ... +3 ulp, against `/`.
// Prints the first mismatches and one summary line; exit status 1 on any error.
#include <initializer_list>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "exact_sqrt.h"

using namespace exact_sqrt;

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t Next() { g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17; return static_cast<uint32_t>(g_state >> 32); }
static float Make(int exponent, uint32_t mantissa) { return FromBits((static_cast<uint32_t>(exponent + 127) << 23) | (mantissa & 0x7fffffu)); }
static float Offset(float v, int k) { return FromBits(Bits(v) + static_cast<uint32_t>(k)); }
static float NearestRsq(float x) { return static_cast<float>(1.0 / sqrt(static_cast<double>(x))); }

static unsigned long long g_roots = 0, g_root_mismatches = 0;
static void CheckRoot(float x) {
  const float want = sqrtf(x), rn = NearestRsq(x);
  for (int k = -3; k <= 3; k++) {
    const float got = ExactSqrt(x, Offset(rn, k));
    if (Bits(got) != Bits(want)) { if (g_root_mismatches < 8) printf("ROOT x=%a seed RN %+d ulp got=%a want=%a\n", x, k, got, want); g_root_mismatches++; }
    g_roots++;
  }
}

static bool InRange(float x) { return x >= 0x1p-60f && x < 0x1p60f; }          // false for NaN
static unsigned long long g_guard_cases = 0, g_guard_errors = 0;
static void CheckGuard(float a, float b) {
  if (ExactSqrtSafe(a) != InRange(a) || ExactSqrtSafe2(a, b) != (InRange(a) && InRange(b)) || ExactSqrtSafe2(b, a) != (InRange(a) && InRange(b))) {
    if (g_guard_errors < 10) printf("GUARD a=%a b=%a\n", a, b);
    g_guard_errors++;
  }
  g_guard_cases++;
}
// a component has a lower bound only: one that is too large, inf or NaN shows in the sum of squares, which the guard is given
static bool ComponentInRange(float n) { const float a = fabsf(n); return a == 0.0f || !(a < 0x1p-60f); }
static void CheckNormalizeGuard(float x, float y, float z, float s) {
  const bool want = s >= 0x1p-40f && s < 0x1p60f && ComponentInRange(x) && ComponentInRange(y) && ComponentInRange(z);
  if (ExactNormalizeSafe(x, y, z, s) != want) { if (g_guard_errors < 10) printf("NORMALIZE GUARD x=%a y=%a z=%a s=%a want %d\n", x, y, z, s, want); g_guard_errors++; }
  g_guard_cases++;
}

static unsigned long long g_vectors = 0, g_all_ones = 0, g_quotient_mismatches = 0, g_seed_histogram[7] = {0, 0, 0, 0, 0, 0, 0};
static int g_seed_low = 0, g_seed_high = 0;                                   // extreme distances of h + h from RN(1 / l), in ulp
static void CheckNormalize(float x, float y, float z, int rsq_offset) {
  const float s = x * x + y * y + z * z;                                        // -ffp-contract=off: every operation rounds
  CheckNormalizeGuard(x, y, z, s);
  if (!ExactNormalizeSafe(x, y, z, s)) return;                                  // (a component scaled below 2^-60: the fallback's case, not counted)
  float h;
  const float l = ExactSqrt(s, Offset(NearestRsq(s), rsq_offset), h);
  bool bad = Bits(l) != Bits(sqrtf(s)) || !(l >= 0x1p-20f && l < 0x1p40f) || !(fabsf(x) < 0x1p41f && fabsf(y) < 0x1p41f && fabsf(z) < 0x1p41f);   // shared_div.h's range
  const float seed = h + h, wx = x / l, wy = y / l, wz = z / l;
  const int distance = static_cast<int>(Bits(seed)) - static_cast<int>(Bits(1.0f / l));
  if (distance < g_seed_low) g_seed_low = distance;
  if (distance > g_seed_high) g_seed_high = distance;
  g_seed_histogram[distance < -3 ? 0 : (distance > 3 ? 6 : distance + 3)]++;
  if ((Bits(l) & 0x7fffffu) == 0x7fffffu) g_all_ones++;
  // the quotients depend on the seed through the refined reciprocal alone: evaluate them once per DISTINCT reciprocal of the seven seeds
  uint32_t seen[7]; int n_seen = 0;
  for (int k = -3; k <= 3 && !bad; k++) {
    const float moved = Offset(seed, k);
    const uint32_t r = Bits(shared_div::SharedReciprocal<true>(l, moved));
    bool known = false;
    for (int j = 0; j < n_seen; j++) known = known || seen[j] == r;
    if (known) continue;
    seen[n_seen++] = r;
    float qx, qy, qz;
    QuotientsByRoot(x, y, z, l, moved, qx, qy, qz);
    if (Bits(qx) != Bits(wx) || Bits(qy) != Bits(wy) || Bits(qz) != Bits(wz)) { bad = true; printf("QUOTIENT seed h + h %+d ulp (h + h is %+d ulp from RN(1 / l)): ", k, distance); }
  }
  if (bad) { if (g_quotient_mismatches < 8) printf("NORMALIZE x=%a y=%a z=%a l=%a\n", x, y, z, l); g_quotient_mismatches++; }
  g_vectors++;
}

int main(int argc, char** argv) {
  const unsigned long long n_vectors = argc > 1 ? strtoull(argv[1], nullptr, 10) : 100000000ull;
  const uint32_t stride = argc > 2 ? static_cast<uint32_t>(strtoul(argv[2], nullptr, 10)) : 1u;
  // ---- roots
  for (int e : {0, 1, -60, 59})                                               // both parities; the two ends of the range
    for (uint32_t m = 0; m < 0x800000u; m += stride) CheckRoot(Make(e, m));
  for (int e = -60; e < 60; e++) {
    for (uint32_t m = static_cast<uint32_t>(e + 60) % 251u; m < 0x800000u; m += 251u * stride) CheckRoot(Make(e, m));
    for (uint32_t m : {0u, 1u, 2u, 0x7ffffdu, 0x7ffffeu, 0x7fffffu, 0x400000u, 0x3fffffu}) CheckRoot(Make(e, m));
  }
  // ---- the guards: one ulp inside and outside each bound; zeros, subnormals, negatives, inf, NaN; random bit patterns
  const float special[] = {0.0f, -0.0f, FromBits(1u), FromBits(0x007fffffu), FromBits(0x00800000u), INFINITY, -INFINITY, NAN, -NAN, FromBits(0x7f800001u), FromBits(0xffc12345u), FromBits(0x7f7fffffu),
                           0x1p-60f, Offset(0x1p-60f, -1), Offset(0x1p-60f, 1), 0x1p60f, Offset(0x1p60f, -1), Offset(0x1p60f, 1), 0x1p-40f, Offset(0x1p-40f, -1), Offset(0x1p-40f, 1),
                           -0x1p-60f, -0x1p60f, -1.0f, -0x1p-61f, 1.0f, 2.0f, 3.0f, 0x1.fffffep-1f, 0x1p-61f, 0x1p61f};
  const int n_special = static_cast<int>(sizeof special / sizeof special[0]);
  for (int i = 0; i < n_special; i++)
    for (int j = 0; j < n_special; j++) {
      CheckGuard(special[i], special[j]);
      CheckNormalizeGuard(special[i], 1.0f, -2.0f, special[j]); CheckNormalizeGuard(1.0f, special[i], 0.0f, special[j]); CheckNormalizeGuard(-0.0f, 1.0f, special[i], special[j]);
      CheckNormalizeGuard(special[i], special[i], special[i], special[j]);
    }
  for (uint32_t k = 0; k < 4000000u / stride; k++) {
    const float a = FromBits(Next()), b = FromBits(Next()), in = Make(static_cast<int>(Next() % 120u) - 60, Next());
    CheckGuard(a, b); CheckGuard(a, in); CheckGuard(in, Make(static_cast<int>(Next() % 120u) - 60, Next()));
    CheckNormalizeGuard(a, b, in, FromBits(Next())); CheckNormalizeGuard(in, a, in, in); CheckNormalizeGuard(in, in, in, Make(static_cast<int>(Next() % 100u) - 40, Next()));
  }
  // ---- Normalize: random magnitudes 2^-15 ... 2^15, components next to zero and exact zeros among them; a third of the vectors normalised
  //      beforehand (their length rounds to 1 or to 0x1.fffffep-1, the all-ones mantissa); axis vectors with every kind of length
  unsigned long long k = 0;
  while (g_vectors < n_vectors && g_guard_errors < 10) {
    const uint32_t r = Next();
    const float scale = Make(static_cast<int>((r >> 8) % 31u) - 15, 0u);
    float x = scale * (static_cast<float>(Next() >> 8) * 0x1p-23f - 1.0f), y = scale * (static_cast<float>(Next() >> 8) * 0x1p-23f - 1.0f), z = scale * (static_cast<float>(Next() >> 8) * 0x1p-23f - 1.0f);
    switch (r & 15u) { case 0: z = 0.0f; break; case 1: y = -0.0f; z = 0.0f; break; case 2: x *= 0x1p-20f; break; case 3: y *= 0x1p-30f; z = 0.0f; break; default: break; }
    if (x == 0.0f && y == 0.0f && z == 0.0f) continue;
    if (k % 3u == 0u) { const float l = sqrtf(x * x + y * y + z * z); x = x / l; y = y / l; z = z / l; }
    CheckNormalize(x, y, z, static_cast<int>(k % 7u) - 3);
    k++;
  }
  printf("roots checked %llu, root mismatches %llu, guard cases %llu, guard errors %llu, vectors checked %llu, all-ones lengths %llu, quotient mismatches %llu, "
         "h + h from RN(1 / l) in ulp: lowest %d, highest %d\n",
         g_roots, g_root_mismatches, g_guard_cases, g_guard_errors, g_vectors, g_all_ones, g_quotient_mismatches, g_seed_low, g_seed_high);
  printf("h + h from RN(1 / l), vectors at <= -3, -2, -1, 0, +1, +2, >= +3 ulp: %llu %llu %llu %llu %llu %llu %llu\n",
         g_seed_histogram[0], g_seed_histogram[1], g_seed_histogram[2], g_seed_histogram[3], g_seed_histogram[4], g_seed_histogram[5], g_seed_histogram[6]);
  return (g_root_mismatches || g_guard_errors || g_quotient_mismatches) ? 1 : 0;
}
