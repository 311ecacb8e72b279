// launch_plan.h -- how many samples the next launch of a render pass takes, and how many record slots it is given: the arithmetic of the launch
// loops of pt_launch.inc as pure functions (host only, no HIP), so that it can be checked by itself (tests/launch_plan_main.cc).
// Every pass is split into launches on accumulation-chunk boundaries, which leaves the summation order unchanged.
#pragma once
#include <algorithm>
#include <cstdint>

#include "../../../include/amber_hip.h"

namespace amber_plan {

constexpr uint64_t kMaxPathsPerLaunch = 1ull << 30;       // q and its bitmap index stay 32-bit; bitmap 128 MiB
constexpr uint64_t kMaxRecordSlots = 48ull << 20;         // 28 B per slot (record + sorted measurement): 1.3 GiB at most
constexpr uint64_t kMaxPartialFloats = 768ull << 20;      // pt_bvh_megakernel's per-item sums: 3 GiB

// The next launch: n of the samples that are left -- 0 although some are left: not even the smallest launch is possible -- and, for a path
// launch, the record slots it is given.
struct Launch { uint32_t n; uint64_t slots; };

// Path-granular launches (pt_megakernel, pt_bvh_pool_kernel) over n_pixels != 0 band pixels.  The record buffer is sized from the density the
// previous launch measured (record slots per path) with a margin of one half; the very first launch of a handle has a slot for EVERY path, is at most
// one chunk unless the job is small, and doubles as the probe.  `slack`: slots that stay unused on top.  test_density_scale > 0: the test hook that
// mis-sizes the buffer (a wrong estimate must only cost a repeated launch).
inline Launch PathLaunch(uint32_t n_pixels, uint32_t samples_left, bool density_known, double rec_density, double test_density_scale, uint64_t slack) {
  const uint64_t max_samples = kMaxPathsPerLaunch / n_pixels / AMBER_ACCUM_CHUNK * AMBER_ACCUM_CHUNK;
  if (max_samples == 0) return {0, 0};
  uint32_t n = samples_left;
  if (n > max_samples) n = static_cast<uint32_t>(max_samples);
  uint64_t slots;
  if (!density_known) {
    if (static_cast<uint64_t>(n_pixels) * n > (4ull << 20) && n > AMBER_ACCUM_CHUNK) n = AMBER_ACCUM_CHUNK;
    slots = static_cast<uint64_t>(n_pixels) * n + slack;
  } else {
    double density = rec_density;
    if (test_density_scale > 0) density *= test_density_scale;
    const double per_sample = std::max(1e-9, density * 1.5) * static_cast<double>(n_pixels);   // slots one sample of the band needs, with margin
    const uint64_t all = static_cast<uint64_t>(n_pixels) * n;
    const double want = per_sample * n;
    if (want + static_cast<double>(slack) > static_cast<double>(kMaxRecordSlots) && all + slack > kMaxRecordSlots) {
      // a dense scene: shorter launches instead of a larger buffer
      uint64_t fit = static_cast<uint64_t>((static_cast<double>(kMaxRecordSlots) - static_cast<double>(slack)) / per_sample) / AMBER_ACCUM_CHUNK * AMBER_ACCUM_CHUNK;
      if (fit < AMBER_ACCUM_CHUNK) fit = AMBER_ACCUM_CHUNK;
      if (n > fit) n = static_cast<uint32_t>(fit);
    }
    const uint64_t all_n = static_cast<uint64_t>(n_pixels) * n;
    slots = std::min<uint64_t>(all_n, static_cast<uint64_t>(per_sample * n) + 1u) + slack;
  }
  return {n, slots};
}

// Item launches (pt_bvh_megakernel: lanes own (pixel, chunk) items) over n_pixels != 0 band pixels: at most kMaxPartialFloats of per-item sums and
// fewer than 2^31 items.
inline Launch ItemLaunch(uint32_t n_pixels, uint32_t samples_left) {
  uint64_t max_chunks = kMaxPartialFloats / (static_cast<uint64_t>(n_pixels) * 3u);
  const uint64_t by_items = 0x7fffffffull / n_pixels;
  if (by_items < max_chunks) max_chunks = by_items;
  if (max_chunks == 0) return {0, 0};
  uint32_t n = samples_left;
  const uint64_t cap = max_chunks * AMBER_ACCUM_CHUNK;
  if (n > cap) n = static_cast<uint32_t>(cap);
  return {n, 0};
}

// Light-tracing launches over n_paths != 0 light paths.  One launch numbers its work units with 31 bits -- pt_megakernel: (light path, pass) pairs;
// pt_bvh_megakernel (`bvh`): (light path, chunk of passes) items -- so a long range of passes is traced in several launches, each a whole number of chunks.
inline Launch LightLaunch(uint32_t n_paths, bool bvh, uint32_t samples_left) {
  const uint64_t max_units = 0x7fffffffull / n_paths;
  if (max_units == 0) return {0, 0};
  uint64_t max_samples = bvh ? max_units * AMBER_ACCUM_CHUNK : max_units / AMBER_ACCUM_CHUNK * AMBER_ACCUM_CHUNK;
  if (max_samples == 0) max_samples = max_units;               // fewer than a chunk fits: any split is valid for light tracing (nothing is summed across launches)
  uint32_t n = samples_left;
  if (n > max_samples) n = static_cast<uint32_t>(max_samples);
  return {n, 0};
}

}  // namespace amber_plan
