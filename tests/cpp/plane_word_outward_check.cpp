// CPU check of bvh_build.h's PlaneWordOutward, the binary64 form of PlaneWord that the device builder calls (bvh_device_build.inc);
// tests/test_device_build_abi.py compiles and runs it with hipcc, no GPU needed.  On random and edge planes -- zero, +-2^-14 of the half
// extent (the edge of binary16's denormal range), +-1 (the grid's ends), flat boxes, a grid without extent at a large offset -- its words
//   * satisfy PlaneWord's inequalities in long double:  gmin + value(min) * step <= mn  and  gmin + value(max) * step >= mx,
//   * are never a binary16 denormal, infinity or NaN, and stay inside |value| <= 1 + one binary16 step on a grid that covers the box,
//   * are at most kMaxStepsLooser = 1 binary16 step looser than PlaneWord's (and never more than one step tighter: both searches stop at
//     the same guard, evaluated in different precisions).
#include <cstdio>
#include <random>
#include "../../amber_amd/csrc/hip/bvh_build.h"

using namespace amber_bvh;

static const int kMaxStepsLooser = 1;
static long bad = 0, n = 0, differ = 0;

// number of F16Step moves from a to b in direction `up` (a small count, or -1 if b is not reached within 4 moves)
static int StepsBetween(uint16_t a, uint16_t b, bool up) {
  for (int k = 0; k <= 4; k++) { if (a == b) return k; a = F16Step(a, up); }
  return -1;
}

static void Check(float mn, float mx, float gmid, float half, bool covered) {
  const uint32_t w = PlaneWordOutward(mn, mx, gmid, half), ref = PlaneWord(mn, mx, gmid, half);
  const uint16_t lo = w & 0xffffu, hi = w >> 16, rlo = ref & 0xffffu, rhi = ref >> 16;
  for (uint16_t h : {lo, hi}) {
    const int e = (h >> 10) & 31, m = h & 1023;
    if (e == 31 || (e == 0 && m != 0)) { bad++; std::printf("non-normal value %04x\n", h); }
  }
  const long double pl = (long double)gmid + (long double)F16Value(lo) * half, ph = (long double)gmid + (long double)F16Value(hi) * half;
  if (!(pl <= (long double)mn) || !(ph >= (long double)mx)) { bad++; if (bad < 10) std::printf("not conservative: [%g, %g] stored [%Lg, %Lg]\n", mn, mx, pl, ph); }
  if (covered && (std::fabs(F16Value(lo)) > 1.0 + 0x1p-10 || std::fabs(F16Value(hi)) > 1.0 + 0x1p-10)) { bad++; if (bad < 10) std::printf("beyond the reach: %g %g\n", F16Value(lo), F16Value(hi)); }
  // looser = further out: the min word below the reference's, the max word above it
  const int lo_out = StepsBetween(rlo, lo, false), lo_in = StepsBetween(rlo, lo, true), hi_out = StepsBetween(rhi, hi, true), hi_in = StepsBetween(rhi, hi, false);
  const bool lo_ok = (lo_out >= 0 && lo_out <= kMaxStepsLooser) || (lo_in >= 0 && lo_in <= 1), hi_ok = (hi_out >= 0 && hi_out <= kMaxStepsLooser) || (hi_in >= 0 && hi_in <= 1);
  if (!lo_ok || !hi_ok) { bad++; if (bad < 10) std::printf("[%g, %g] on (%g, %g): words %04x %04x, PlaneWord's %04x %04x\n", mn, mx, gmid, half, lo, hi, rlo, rhi); }
  if (w != ref) differ++;
  n++;
}

int main() {
  std::mt19937_64 rng(2024);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  for (int trial = 0; trial < 400; trial++) {
    const double scale = std::pow(10.0, -4.0 + 10.0 * U(rng));                 // half extents from 1e-4 to 1e6
    const double centre = (U(rng) - 0.5) * std::pow(10.0, -2.0 + 9.0 * U(rng)) * (trial % 5 == 0 ? 0.0 : 1.0);
    const float gmid = static_cast<float>(centre), half = static_cast<float>(scale);
    for (int k = 0; k < 500; k++) {
      double a = centre + (2.0 * U(rng) - 1.0) * scale, b = centre + (2.0 * U(rng) - 1.0) * scale;
      if (k % 7 == 0) a = centre + (U(rng) - 0.5) * scale * 1e-5;               // planes next to the centre: the denormal range of the value
      if (k % 11 == 0) b = a;                                                  // a flat box
      if (a > b) std::swap(a, b);
      const float mn = static_cast<float>(a), mx = static_cast<float>(b);
      if (!(mn <= mx)) continue;
      Check(mn, mx, gmid, half, std::fabs(double(mn) - gmid) <= half && std::fabs(double(mx) - gmid) <= half);
    }
    // edge planes of this grid: the centre, +-2^-14 and its neighbours, +-1 (the ends), +-(1 - 2^-11), exactly representable values
    for (double u : {0.0, 0x1p-14, -0x1p-14, 0x1p-14 * 0.999, -0x1p-14 * 0.999, 0x1p-14 * 1.001, -0x1p-14 * 1.001, 0x1p-15, -0x1p-24, 1.0, -1.0, 1.0 - 0x1p-11, -1.0 + 0x1p-11, 0.5, -0.25, 0.333251953125})
      for (double v : {u, 1.0, 0.0}) {
        double a = double(gmid) + u * half, b = double(gmid) + v * half;
        if (a > b) std::swap(a, b);
        const float mn = static_cast<float>(a), mx = static_cast<float>(b);
        Check(mn, mx, gmid, half, std::fabs(double(mn) - gmid) <= half && std::fabs(double(mx) - gmid) <= half);
      }
  }
  // a scene with no extent on an axis, away from the origin: F16AxisGrid's floor keeps a usable step, the flat box is found in a few steps
  for (double coord : {1234.5, -0.37, 6.0e5, 0.0, 1e-20, -7.25e3}) {
    float mid, half;
    F16AxisGrid(coord, coord, mid, half);
    const float c = static_cast<float>(coord);
    Check(c, c, mid, half, true);
  }
  std::printf("%ld boxes, %ld violations, %ld words differ from PlaneWord's (each by one step)\n", n, bad, differ);
  return (bad == 0 && n > 150000) ? 0 : 1;
}
