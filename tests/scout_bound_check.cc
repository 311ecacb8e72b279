// scout_bound_check.cc -- tests/test_scout_bound_host.py compiles this alone (no HIP) and runs it: the suspect rule of csrc/hip/scout_bound.h against the true
// weights.  For every draw of (lens, guard quantities, sequence of scatter weights) the weight's true magnitude -- the eye weight and the quotients sw_i / p
// multiplied in binary64, every factor the exact real quotient of the binary32 inputs -- must stay below 2^(bound / 16) for as long as the rule has not
// called the path suspect.  Prints "draws checked worst" and exits 0, or the first violation and 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

#include "../amber_amd/csrc/hip/scout_bound.h"

static uint32_t Bits(float x) { uint32_t b; std::memcpy(&b, &x, 4); return b; }
static float FromBits(uint32_t b) { float x; std::memcpy(&x, &b, 4); return x; }

int main(int argc, char** argv) {
  const long n_draws = argc > 1 ? std::atol(argv[1]) : 1000000;
  std::mt19937_64 rng(20260101u);
  auto uni = [&](double lo, double hi) { return lo + (hi - lo) * (double(rng() >> 11) * 0x1p-53); };
  auto log_uniform = [&](double lo2, double hi2) { return float(std::exp2(uni(lo2, hi2))); };
  const float identity[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  const float origin[3] = {0, 0, 0};
  const float blades[9] = {0.05f, 0, 0, 0, 0.05f, 0, -0.05f, 0, 0};
  long checked = 0, established = 0, suspects = 0;
  double worst = -1e300;                                                     // largest log2|w| - bound / 16 seen: must stay <= 0
  for (long k = 0; k < n_draws; k++) {
    // ---- a lens: mostly sane, sometimes far out (then the host must refuse or still be right)
    amber_scout::LensFacts f{};
    f.kind = (rng() & 3u) == 0u ? 1u : 0u;
    f.local_ = identity; f.global_ = identity; f.origin = origin; f.blade_vertices = blades; f.n_vertices = 3;
    const bool wild = (rng() & 7u) == 0u;
    f.sensor_distance = log_uniform(wild ? -30 : -8, wild ? 30 : 4) * ((rng() & 15u) ? 1.f : -1.f);
    f.focus_distance = log_uniform(wild ? -30 : -4, wild ? 30 : 12);
    f.p_area = log_uniform(wild ? -80 : -20, wild ? 80 : 20);
    f.sensor_w = log_uniform(-10, 3); f.sensor_h = log_uniform(-10, 3);
    f.size_over_area = log_uniform(wild ? -70 : 0, wild ? 70 : 40);
    f.inv_scene_area = 1.0f / (f.sensor_w * f.sensor_h);
    uint32_t bound = 0;
    double log2_w;                                                           // log2 of the true |weight| so far
    if (!amber_scout::EyeWeightBound(f, &bound)) continue;                   // the handle renders with the full kernel: nothing to check
    established++;
    // ---- the eye weight at the worst the guards allow, and anywhere inside
    const double dz = (rng() & 1u) ? double(amber_scout::kMinZ) : uni(double(amber_scout::kMinZ), 1.0);
    if (f.kind == 0u) {
      const double nz = (rng() & 1u) ? 1.0001 : uni(0.0, 1.0001), dloc = (rng() & 1u) ? 1.01 : uni(1e-3, 1.01);
      const double factor = std::pow(nz / dz, 4.0);
      const double pdf_dir = double(float(double(f.size_over_area) * (double(f.sensor_distance) * f.sensor_distance) / std::pow(dloc, 4.0)));
      log2_w = std::log2(factor / double(f.p_area) / pdf_dir);
    } else {
      const double dl_z = (rng() & 1u) ? 1.0 : dz, dl_len = std::fmax(dl_z, uni(dl_z, 1.01));
      const double gf = std::pow(dl_z, 4.0) / (double(f.sensor_distance) * f.sensor_distance * dl_len * dl_len);
      log2_w = std::log2(gf / double(f.inv_scene_area));
    }
    if (log2_w < -1e300) log2_w = -1e300;
    // ---- bounces: the scatter weights of PathShade, p = min(0.9375, Max3(sw)); a path continues only while p > 0
    const int n_bounces = 1 + int(rng() % 200u);
    const unsigned style = unsigned(rng() % 6u);
    for (int b = 0; b < n_bounces; b++) {
      float sw[3];
      for (int c = 0; c < 3; c++) {
        switch (style) {
          case 0: sw[c] = float(uni(0.0, 0.95)); break;                                 // Lambertian albedos
          case 1: sw[c] = 1.0f; break;                                                  // mirrors and glass at sw = 1
          case 2: sw[c] = log_uniform(-140, 120) * ((rng() & 1u) ? 1.f : -1.f); break;  // huge, tiny and negative components
          case 3: sw[c] = float(uni(0.9, 1.1)); break;                                  // around the roulette threshold
          case 4: sw[c] = FromBits(uint32_t(rng()) & ((rng() & 1u) ? 0xffffffffu : 0x007fffffu)); break;   // any bit pattern, subnormals
          default: sw[c] = c == 0 ? log_uniform(-149, -120) : -log_uniform(-130, 10); break;   // p down to subnormal under larger negative components
        }
      }
      float mw = sw[0]; if (mw < sw[1]) mw = sw[1]; if (mw < sw[2]) mw = sw[2];            // Max3
      float p = 0.9375f; if (mw < p) p = mw;
      if (!(p > 0.0f)) break;                                                             // Uniform(rng) >= p: the path ends
      bound = amber_scout::BounceBound(bound, Bits(sw[0]), Bits(sw[1]), Bits(sw[2]), Bits(p));
      if (bound > amber_scout::kLimit) { suspects++; break; }                             // suspect: replayed, nothing claimed
      double a = 0;
      for (int c = 0; c < 3; c++) a = std::fmax(a, std::fabs(double(sw[c])));
      log2_w += std::log2(a / double(p));
      checked++;
      const double over = log2_w - double(bound) / 16.0;
      if (over > worst) worst = over;
      if (over > 0) {
        std::printf("VIOLATION draw %ld bounce %d: log2|w| = %.6f > bound %.4f (sw %a %a %a, p %a)\n", k, b, log2_w, double(bound) / 16.0, sw[0], sw[1], sw[2], p);
        return 1;
      }
    }
  }
  std::printf("%ld draws, %ld with a bound, %ld bounces checked, %ld ended suspect, worst excess %.6f bits\n", n_draws, established, checked, suspects, worst);
  return established > n_draws / 2 && checked > n_draws ? 0 : 2;
}
