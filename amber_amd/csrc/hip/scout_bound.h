// scout_bound.h -- the suspect rule of pt_megakernel's weight-free instantiation (AMBER_KERNEL_SCOUT, pt_megakernel.inc): an upper bound of log2 of the
// largest path-weight magnitude, kept per lane as a small integer, from which the kernel decides which paths pt_replay.inc must trace again with weights.
// Plain C++ on bit patterns and binary64, shared by the device (PathShade), the host (create: EyeWeightBound) and tests/scout_bound_check.cc, which
// compiles it alone.
//
// WHY A BOUND.  The full kernel emits a record iff a path's final measurement is anything but +0.  measurement += weight * Radiance, and Radiance is
// (+0, +0, +0) except on a DiffuseLight seen from its front, whose scatter weight 0 ends the path.  Away from such a hit a term is weight * (+0): +0 or -0
// (and +0 + -0 = +0) unless a weight component is inf or NaN.  So a path that never holds an inf or NaN weight component ends with measurement +0 unless its
// LAST hit has Radiance other than (+0, +0, +0) -- which the scout sees without any weight.  The rule flags every path that MIGHT hold such a component:
//
//   |w_i| <= 2^(bound / 16) for every component i, as long as bound <= kLimit (2^126 < FLT_MAX: no product has overflowed, so none is inf, so none is NaN).
//
//  * Start: every component is the eye weight ew.  EyeWeightBound (host) proves |ew| <= 2^(bound0 / 16) for every ray whose guard quantity (GenerateEyeRay<kScout>:
//    direction.z -- NaN unless direction is finite and |sensor_distance - aperture_point.z| >= kMinGap; pinhole: the ray's local z) has magnitude in
//    [kMinZ, inf) -- the kernel sets `suspect` for a lane whose guard fails (NaN fails it) -- or it reports that it cannot (a lens outside the ranges below),
//    and the handle renders with the full kernel.
//  * Bounce (PathShade :156): w_i <- RN(w_i * RN(sw_i / p)), p = min(0.9375, Max3(sw)) > 0 on a path that continues.  With a = max |sw_i|, BounceBound adds
//      0               when a <= p: every quotient has magnitude <= 1 (RN is monotone and 1 is representable), and |RN(w q)| <= |w| for |q| <= 1;
//      2 (sixteenths)  when p = 0.9375 and a <= 1: |q| <= RN(1 / 0.9375) and RN(1 / 0.9375) (1 + 2^-24) < 2^(1/8);
//      16 (E(a) - E(p) + 1) otherwise, E the biased exponent: a <= (2 - 2^-23) 2^E(a), p >= 2^E(p) (p normal), so |q| <= (2 - 2^-23) 2^(E(a) - E(p)), a
//                      representable number that RN cannot exceed, and (2 - 2^-23)(1 + 2^-24) < 2 covers the rounding of the product.  (The bound is never
//                      below 0, i.e. 2^(bound/16) >= 1, so a subnormal product, whose rounding is not relative, is below it anyway.)
//    and sets `suspect` when a is inf or NaN (any component: a NaN has the largest magnitude bits) or p is subnormal.
//  * bound > kLimit: `suspect`.  The bound never decreases and saturates at kSuspect, so the bit is sticky.
// An ordinary long chain costs nothing: a 130-bounce refraction chain at sw = 1 adds 2 per bounce (16.25 bits), a Lambertian bounce with rho <= 0.9375 adds 0.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define AMBER_SCOUT_HD __host__ __device__
#else
#define AMBER_SCOUT_HD
#endif

namespace amber_scout {

constexpr uint32_t kLimit = 126u * 16u;          // sixteenths of a bit: |w| <= 2^126
constexpr uint32_t kSuspect = 0x40000000u;       // the saturated bound: the lane's path is replayed
constexpr float kMinZ = 0.015625f;               // 2^-6: the eye ray's guard quantity must reach this magnitude (89.1 degrees off the axis)
constexpr float kMinGap = 9.094947017729282e-13f;  // 2^-40: thin lens, the least |sensor_distance - aperture_point.z| (its square is a normal number)

AMBER_SCOUT_HD inline uint32_t BounceBound(uint32_t bound, uint32_t sx_bits, uint32_t sy_bits, uint32_t sz_bits, uint32_t p_bits) {
  const uint32_t ax = sx_bits & 0x7fffffffu, ay = sy_bits & 0x7fffffffu, az = sz_bits & 0x7fffffffu;
  uint32_t a = ax > ay ? ax : ay;
  a = a > az ? a : az;                                                       // magnitudes order like their bit patterns; a NaN is above every number
  uint32_t inc = ((a >> 23) - (p_bits >> 23) + 1u) * 16u;
  if (p_bits == 0x3f700000u && a <= 0x3f800000u) inc = 2u;                   // p = 0.9375, a <= 1
  if (a <= p_bits) inc = 0u;
  bound += inc;
  if (a >= 0x7f800000u || p_bits < 0x00800000u || p_bits >= 0x7f800000u) bound = kSuspect;   // inf, NaN; p subnormal, zero, negative (never on a path that continues)
  return bound < kSuspect ? bound : kSuspect;
}

// What EyeWeightBound needs of a lens: DevLens's constants, the aperture blades' vertices (world), the sensor's size in the scene.
struct LensFacts {
  uint32_t kind;                                 // 0 thin, 1 pinhole (AMBER_LENS_*)
  const float* local_; const float* global_;     // 3 x 3, row major
  const float* origin;
  float sensor_distance, focus_distance, p_area, size_over_area, inv_scene_area;
  float sensor_w, sensor_h;                      // scene units
  const float* blade_vertices; uint32_t n_vertices;   // 3 floats each
};

// bound0 (sixteenths of a bit) with |ew| <= 2^(bound0 / 16) for every eye ray of this lens whose guard quantity z has kMinZ <= |z| < inf; false: not established.
// The ranges (lengths and positions of magnitude in [2^-20, 2^20], p_area, size_over_area and inv_scene_area in [2^-60, 2^60], matrices orthonormal to 1e-3) keep the squared lengths GenerateEyeRay forms from overflowing, and
//   thin lens:  ew = factor / p_area / pdf_dir.  factor = (n.z / direction.z)^4 with n = Normalize(sensor_point - aperture_point): the guard's gap makes the
//               squared length of that difference a normal number, so |n.z| <= 1.0001, and |direction.z| >= kMinZ: factor <= (1.0001 / kMinZ)^4.  The guard
//               also says direction is finite, and it is not 0, so ray_dir = Normalize(global_ direction) is a unit vector (or 0, if direction was the
//               finite garbage a subnormal squared length leaves and its image's squared length overflowed): |dloc.z| <= 1.01, a row of local_ times it, and
//               pdf_dir = size_over_area sd^2 / dloc.z^4 is a positive normal number or inf (then ew = 0), never below size_over_area sd^2 / 1.01^4;
//   pinhole:    ew = gf / inv_scene_area, gf = dl.z^2 / |point|^2 = dl.z^4 / (sd^2 |dl|^2) <= dl.z^2 / sd^2 <= 1.03 / sd^2, the guard |dl.z| >= kMinZ
//               keeping sd / dl.z and |point|^2 in range.
// One more bit covers the roundings of the binary32 quotients and of the conversion from binary64.
inline bool EyeWeightBound(const LensFacts& f, uint32_t* bound0) {
  const double kHi = 1048576.0, kLo = 1.0 / 1048576.0;
  auto in_range = [&](double x) { return std::isfinite(x) && std::fabs(x) >= kLo && std::fabs(x) <= kHi; };
  auto positive = [&](double x) { return x >= 0x1p-60 && x <= 0x1p60; };     // the factors that only scale the weight: the products below stay normal numbers
  if (f.kind > 1u) return false;
  if (!in_range(f.sensor_distance) || !in_range(f.sensor_w) || !in_range(f.sensor_h) || !(f.sensor_w > 0) || !(f.sensor_h > 0)) return false;
  for (int c = 0; c < 3; c++) if (!(std::fabs(double(f.origin[c])) <= kHi)) return false;
  for (const float* m : {f.local_, f.global_})
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) {
        double rr = 0, cc = 0;                                               // rows and columns orthonormal
        for (int k = 0; k < 3; k++) { rr += double(m[3 * i + k]) * m[3 * j + k]; cc += double(m[3 * k + i]) * m[3 * k + j]; }
        const double want = i == j ? 1.0 : 0.0;
        if (!(std::fabs(rr - want) <= 1e-3) || !(std::fabs(cc - want) <= 1e-3)) return false;
      }
  const double sd2 = double(f.sensor_distance) * f.sensor_distance;
  double log2_bound;
  if (f.kind == 1u) {
    if (!positive(f.inv_scene_area)) return false;
    log2_bound = std::log2(1.03 / (sd2 * f.inv_scene_area));
  } else {
    if (!in_range(f.focus_distance) || !positive(f.p_area) || !positive(f.size_over_area)) return false;
    for (uint32_t k = 0; k < 3u * f.n_vertices; k++) if (!(std::fabs(double(f.blade_vertices[k])) <= kHi)) return false;
    const double factor_max = std::pow(1.0001 / double(kMinZ), 4.0), pdf_min = double(f.size_over_area) * sd2 / std::pow(1.01, 4.0);
    log2_bound = std::log2(factor_max / double(f.p_area) / pdf_min);
  }
  if (!std::isfinite(log2_bound)) return false;
  const double sixteenths = std::ceil(16.0 * (log2_bound + 1.0));
  const double b = sixteenths < 0 ? 0.0 : sixteenths;
  if (b > double(kLimit) - 16.0 * 16.0) return false;                        // less than 16 bits of the budget left: every path would be replayed
  *bound0 = static_cast<uint32_t>(b);
  return true;
}

}  // namespace amber_scout
