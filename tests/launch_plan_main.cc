// Stand-alone host check of amber_amd/csrc/hip/launch_plan.h (tests/test_launch_plan.py builds and runs it; no HIP, no library).
// The samples and the record slots of the next launch for the three kinds of launches.  Every expected value is a literal worked out by hand from
// the launch loops as they stood before the arithmetic moved into the header; the derivation is written next to it.  AMBER_ACCUM_CHUNK is 8.
// Prints the number of cases and of failures; exit status 0 only if there is none.
#include <cstdint>
#include <cstdio>

#include "launch_plan.h"

namespace {
using amber_plan::Launch;
int g_cases = 0, g_failures = 0;
// fits false: the band is too large for any launch, which the plan says with n = 0 although samples are left
void Expect(const char* what, const Launch& got, bool fits, uint32_t n, uint64_t slots) {
  ++g_cases;
  if (fits ? got.n == n && got.slots == slots : got.n == 0) return;
  ++g_failures;
  std::printf("FAILED %s: n %u slots %llu (want n %u slots %llu)\n", what, got.n, static_cast<unsigned long long>(got.slots), n, static_cast<unsigned long long>(slots));
}
}  // namespace

int main() {
  static_assert(AMBER_ACCUM_CHUNK == 8u, "the expected values below are worked out for chunks of 8 samples");
  static_assert(amber_plan::kMaxPathsPerLaunch == 1073741824ull && amber_plan::kMaxRecordSlots == 50331648ull && amber_plan::kMaxPartialFloats == 805306368ull, "limits");
  using amber_plan::PathLaunch; using amber_plan::ItemLaunch; using amber_plan::LightLaunch;
  const uint64_t S = 528384;                 // the slack of a device with 256 CUs: 256 * 8 * 4 * 64 + 4096
  const uint32_t kVga = 327680;              // 640 x 512:   max_samples = 2^30 / 327680 = 3276 -> 3272 (whole chunks)
  const uint32_t kHd = 2073600;              // 1920 x 1080: max_samples = 2^30 / 2073600 = 517 -> 512

  // ---- path launches, density unknown: a slot for every path; more than 4 Mi (4194304) paths and more than a chunk -> one chunk
  Expect("paths vga 8 unknown", PathLaunch(kVga, 8, false, 0.0, 0.0, S), true, 8, 2621440 + S);           // 327680 * 8 = 2621440 <= 4 Mi
  Expect("paths vga 56 unknown", PathLaunch(kVga, 56, false, 0.0, 0.0, S), true, 8, 2621440 + S);         // 327680 * 56 = 18350080 > 4 Mi -> n = 8
  Expect("paths hd 8 unknown", PathLaunch(kHd, 8, false, 0.0, 0.0, S), true, 8, 16588800 + S);            // > 4 Mi paths but n is not above a chunk: 2073600 * 8
  Expect("paths vga 12 unknown", PathLaunch(kVga, 12, false, 0.0, 0.0, S), true, 12, 3932160 + S);        // 327680 * 12 = 3932160 <= 4 Mi: a small job stays whole
  Expect("paths vga 0 unknown", PathLaunch(kVga, 0, false, 0.0, 0.0, S), true, 0, S);
  Expect("paths vga 1 unknown", PathLaunch(kVga, 1, false, 0.0, 0.0, S), true, 1, 327680 + S);
  // ---- density known: per_sample = max(1e-9, density * 1.5) * n_pixels; slots = min(n_pixels * n, uint64(per_sample * n) + 1) + slack
  // 0.5: per_sample = 245760; want = 245760 * 56 = 13762560, with S below 48 Mi (50331648): no shortening
  Expect("paths vga 56 d0.5", PathLaunch(kVga, 56, true, 0.5, 0.0, S), true, 56, 13762561 + S);
  // 1.0: n = min(1024, 512) = 512; per_sample = 3110400; want = 1592524800 and all = 1061683200 are both beyond 48 Mi ->
  // fit = (50331648 - 528384) / 3110400 = 16.01 -> 16; slots = min(2073600 * 16 = 33177600, 49766401) + S
  Expect("paths hd 1024 d1.0", PathLaunch(kHd, 1024, true, 1.0, 0.0, S), true, 16, 33177600 + S);
  // 20: per_sample = 62208000 > 48 Mi: fit = 0 -> one chunk all the same; slots = min(2073600 * 8, ...) + S
  Expect("paths hd 64 d20", PathLaunch(kHd, 64, true, 20.0, 0.0, S), true, 8, 16588800 + S);
  // 3.0: want = 1474560 * 56 = 82575360 is beyond 48 Mi, but a slot for every path (18350080 + S) is not: no shortening, every path a slot
  Expect("paths vga 56 d3.0", PathLaunch(kVga, 56, true, 3.0, 0.0, S), true, 56, 18350080 + S);
  // more samples than one launch numbers: n = 3272; per_sample = 0.015 * 327680 = 4915.2; want = 16082534.4
  Expect("paths vga 5000 d0.01", PathLaunch(kVga, 5000, true, 0.01, 0.0, S), true, 3272, 16082535 + S);
  Expect("paths vga 0 d0.5", PathLaunch(kVga, 0, true, 0.5, 0.0, S), true, 0, S);                         // min(0, 0 + 1) + S
  Expect("paths vga 1 d0.5", PathLaunch(kVga, 1, true, 0.5, 0.0, S), true, 1, 245761 + S);                // min(327680, 245760 + 1) + S
  // the test hook: density 0.5 * 0.02 = 0.01, per_sample = 4915.2, want = 275251.2 -> 275251 + 1 + 64
  Expect("paths vga 56 d0.5 hook", PathLaunch(kVga, 56, true, 0.5, 0.02, 64), true, 56, 275316);
  // 2^28 pixels: 2^30 / 2^28 = 4 samples, less than a chunk
  Expect("paths 2^28 pixels", PathLaunch(1u << 28, 8, false, 0.0, 0.0, S), false, 0, 0);
  // 2^27 pixels: exactly one chunk fits; density 0: per_sample = 1e-9 * 2^27 = 0.134, want = 1.07 -> 1 + 1 slots
  Expect("paths 2^27 pixels", PathLaunch(1u << 27, 56, true, 0.0, 0.0, S), true, 8, 2 + S);
  // ---- item launches: max_chunks = min(768 Mi / (3 * n_pixels), (2^31 - 1) / n_pixels)
  Expect("items hd 2048", ItemLaunch(kHd, 2048), true, 1032, 0);                                           // min(805306368 / 6220800 = 129, 1035) * 8
  Expect("items hd 1016", ItemLaunch(kHd, 1016), true, 1016, 0);                                           // what is left after that launch
  Expect("items hd 0", ItemLaunch(kHd, 0), true, 0, 0);
  Expect("items hd 1", ItemLaunch(kHd, 1), true, 1, 0);
  Expect("items 2^28 pixels", ItemLaunch(1u << 28, 56), true, 8, 0);                                       // 3 * 2^28 = 768 Mi exactly: one chunk (by items: 7)
  Expect("items 2^28 + 1 pixels", ItemLaunch((1u << 28) + 1u, 56), false, 0, 0);                           // 3 * n_pixels > 768 Mi
  // ---- light launches: max_units = (2^31 - 1) / n_paths; engine BVH counts chunks, the others samples (whole chunks)
  Expect("light hd bvh", LightLaunch(kHd, true, 100000), true, 8280, 0);                                   // 1035 * 8
  Expect("light hd list", LightLaunch(kHd, false, 100000), true, 1032, 0);                                 // 1035 / 8 * 8
  Expect("light 2^29 list", LightLaunch(1u << 29, false, 100), true, 3, 0);                                // 3 units, fewer than a chunk: 3 samples
  Expect("light 2^29 bvh", LightLaunch(1u << 29, true, 100), true, 24, 0);
  Expect("light 2^31 paths", LightLaunch(1u << 31, false, 100), false, 0, 0);
  Expect("light hd 0", LightLaunch(kHd, false, 0), true, 0, 0);
  Expect("light hd 1", LightLaunch(kHd, true, 1), true, 1, 0);
  std::printf("cases %d, failures %d\n", g_cases, g_failures);
  return g_failures == 0 ? 0 : 1;
}
