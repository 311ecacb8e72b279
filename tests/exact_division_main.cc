// Stand-alone host check of amber_amd/csrc/hip/exact_div.h (tests/test_exact_division.py builds and runs it; no HIP, no library).
// For every divisor d of the list below and every dividend n of its list: Quotient == n / d and Remainder == n % d.  Prints the number of
// (d, n) pairs checked and the number of mismatches; exit status 0 only if there is none.
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "exact_div.h"

namespace {
// SplitMix64: the seeded source of the random divisors, multipliers and dividends
struct Rng {
  uint64_t s;
  uint64_t Next() { uint64_t z = (s += 0x9e3779b97f4a7c15ull); z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); }
  uint32_t Next32() { return static_cast<uint32_t>(Next() >> 32); }
};
}  // namespace

int main() {
  const uint32_t kMax = 0xffffffffu;
  std::vector<uint32_t> divisors = {1u, 2u, 3u, 5u, 7u, 8u, 63u, 64u, 65u, 1000u, 1023u, 1024u, 1025u, 3840u, 65535u, 65536u, 65537u,
                                    0x7fffffffu, 0x80000000u, 0x80000001u, kMax};
  Rng rd{20261018u};
  for (int i = 0; i < 10000; ++i) {
    // every magnitude: a random width of 1 .. 32 bits, then random bits below the leading one
    const uint32_t bits = 1u + rd.Next32() % 32u;
    uint32_t d = rd.Next32() >> (32u - bits);
    d |= 1u << (bits - 1u);
    divisors.push_back(d);
  }
  std::vector<uint32_t> random_n(10000);
  Rng rn{977u};
  for (auto& n : random_n) {
    const uint32_t bits = 1u + rn.Next32() % 32u;
    n = rn.Next32() >> (32u - bits);
  }
  uint64_t checked = 0, bad = 0;
  std::vector<uint32_t> ns;
  for (size_t di = 0; di < divisors.size(); ++di) {
    const uint32_t d = divisors[di];
    const ExactDiv dv = MakeExactDiv(d);
    ns.clear();
    const uint32_t fixed[] = {0u, 1u, d - 1u, d, d + 1u /* wraps to 0 for d = 2^32 - 1 */, 0x7fffffffu, 0x80000001u, kMax - 1u, kMax};
    ns.insert(ns.end(), fixed, fixed + sizeof fixed / sizeof fixed[0]);
    Rng rk{0x5eedull + di};
    const uint32_t kmax = kMax / d;                                   // the multiples k * d that fit 32 bits: k = 1 .. kmax
    for (int i = 0; i < 64; ++i) {
      const uint32_t k = 1u + static_cast<uint32_t>(rk.Next() % kmax);
      const uint32_t kd = k * d;
      ns.push_back(kd - 1u); ns.push_back(kd); if (kd != kMax) ns.push_back(kd + 1u);
    }
    ns.insert(ns.end(), random_n.begin(), random_n.end());
    for (const uint32_t n : ns) {
      const uint32_t q = Quotient(dv, n), r = Remainder(dv, d, n);
      ++checked;
      if (q != n / d || r != n % d) {
        if (bad < 20) std::printf("MISMATCH d=%" PRIu32 " n=%" PRIu32 ": quotient %" PRIu32 " (want %" PRIu32 "), remainder %" PRIu32 " (want %" PRIu32 ")\n", d, n, q, n / d, r, n % d);
        ++bad;
      }
    }
  }
  static_assert(sizeof(ExactDiv) == 8, "two dwords");
  std::printf("divisors %zu, pairs checked %" PRIu64 ", mismatches %" PRIu64 "\n", divisors.size(), checked, bad);
  return bad == 0 ? 0 : 1;
}
