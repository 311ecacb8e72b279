// lt_photons.inc -- amber_hip_lt_trace_photons: the vertices of the light paths, in (sample, path, bounce) order, into the caller's buffer.
// Part of the one translation unit pt_host.hip (kernels are launched from there); see its header comment and include/amber_hip.h for the contract.
//
// The trace launch is light tracing's own (LtTraceLaunches, pt_launch.inc), with the vertex sink of PathShade (dev_shading.h, SINK_PHOTONS) instead
// of the splat: it leaves the 64-byte records of one launch in the handle's staging buffer in arrival order -- slots come from an atomic counter,
// claimed once per wave -- and counts its casts in a counter of the call's own.  What is new here takes them to the caller, the way
// lt_accumulate.inc takes splats to the framebuffer:
//   1. order      an index permutation sorted by (sample, path, bounce): two stable radix sorts (rocPRIM), first by bounce (as many bits as
//                 max_depth can set; all 32 when it is 0), then by (sample, path) relative to the launch, packed into the bits that the launch's
//                 pass count and the call's path range can set.  The scratch is lt_accumulate.inc's (LtAccumBufs: keys, permutations, rocPRIM's).
//   2. gather     the records into `out` at the running offset, four lanes per record, 16 bytes each: the records move once.
// Launches run in pass order, so their concatenation is the global order.  The key names a record completely: the output does not depend on the
// arrival order.  A launch that runs out of staging slots is repeated once with the buffer it asked for (the protocol of LtRenderPass).

namespace {

static_assert(sizeof(AmberPhoton) == 64 && sizeof(AmberPhotonInfo) == 32, "a photon is four float4");
static_assert(offsetof(AmberPhoton, object) == 12 && offsetof(AmberPhoton, path) == 28 && offsetof(AmberPhoton, sample) == 44 && offsetof(AmberPhoton, bounce) == 60, "the sink's layout");

// key = bounce, index = identity
__global__ void __launch_bounds__(256) photon_key_bounce_kernel(const float4* __restrict__ rec, uint32_t n, unsigned long long* __restrict__ key, uint32_t* __restrict__ index) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  key[i] = __float_as_uint(rec[static_cast<size_t>(i) * 4u + 3u].w);
  index[i] = i;
}

// key = (sample - first_sample) << path_bits | (path - path_begin) of the records in bounce order
__global__ void __launch_bounds__(256) photon_key_path_kernel(const float4* __restrict__ rec, const uint32_t* __restrict__ index, uint32_t n, uint32_t first_sample, uint32_t path_begin,
                                                              uint32_t path_bits, unsigned long long* __restrict__ key) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const size_t r = static_cast<size_t>(index[i]) * 4u;
  const uint32_t path = __float_as_uint(rec[r + 1u].w), sample = __float_as_uint(rec[r + 2u].w);
  key[i] = (static_cast<unsigned long long>(sample - first_sample) << path_bits) | (path - path_begin);
}

// out[i] = rec[index[i]]: four lanes per record, one float4 each (a wave writes 1 KiB of consecutive bytes)
__global__ void __launch_bounds__(256) photon_gather_kernel(const float4* __restrict__ rec, const uint32_t* __restrict__ index, uint32_t n, float4* __restrict__ out) {
  const uint64_t t = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
  const uint64_t i = t >> 2;
  if (i >= n) return;
  out[t] = rec[static_cast<size_t>(index[i]) * 4u + (t & 3u)];
}

int EnsurePhotonStaging(amber_hip_pt* h, uint32_t capacity) {
  PhotonBufs& s = h->photons;
  if (s.capacity < AMBER_PHOTON_CAPACITY0) s.capacity = AMBER_PHOTON_CAPACITY0;
  if (s.capacity < capacity) s.capacity = capacity;
  AMBER_TRY(Grow(h, s.staging, static_cast<size_t>(s.capacity) * 4u, "photons"));
  if (!s.count) HIP_TRY(s.count.alloc(1));
  if (!s.rays) HIP_TRY(s.rays.alloc(1));
  return AMBER_OK;
}

// The n records of a launch over the passes from first_sample (n_launch_samples of them) at the staging buffer (0 < n < 2^31, any order), in key
// order to dst (device, 16-byte aligned).  Enqueued on the handle's stream; the scratch may grow first, which waits for the stream.
int PhotonOrder(amber_hip_pt* h, uint32_t n, uint32_t first_sample, uint32_t n_launch_samples, uint32_t path_begin, uint32_t n_paths, float4* dst) {
  PhotonBufs& s = h->photons;
  LtAccumBufs& k = h->lt;
  const hipStream_t st = h->stream;
  for (int b = 0; b < 2; b++) {
    AMBER_TRY(Grow(h, k.key[b], n, "photon keys"));
    AMBER_TRY(Grow(h, k.index[b], n, "photon order"));
  }
  const uint32_t max_depth = h->scene.max_depth;
  const unsigned int bounce_bits = max_depth == 0u || max_depth == 0xffffffffu ? 32u : BitsFor(max_depth + 1u);   // 1 <= bounce <= max_depth
  const uint32_t path_bits = BitsFor(n_paths);
  const unsigned int path_end = path_bits + BitsFor(n_launch_samples);
  size_t bytes_a = 0, bytes_b = 0;
  HIP_TRY(rocprim::radix_sort_pairs(nullptr, bytes_a, k.key[0].p, k.key[1].p, k.index[0].p, k.index[1].p, n, 0u, bounce_bits, st));
  HIP_TRY(rocprim::radix_sort_pairs(nullptr, bytes_b, k.key[0].p, k.key[1].p, k.index[1].p, k.index[0].p, n, 0u, path_end, st));
  AMBER_TRY(Grow(h, k.temp, std::max(bytes_a, bytes_b), "sort scratch"));
  const dim3 grid((n + 255u) / 256u), wg(256);
#ifdef AMBER_LAB
  if (s.stage_timing) HIP_TRY(hipEventRecord(s.ev[2].v, st));           // (ev[0], ev[1]: around the trace kernel, LtTraceLaunches)
#endif
  hipLaunchKernelGGL(photon_key_bounce_kernel, grid, wg, 0, st, s.staging.p, n, k.key[0].p, k.index[0].p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(rocprim::radix_sort_pairs(k.temp.p, bytes_a, k.key[0].p, k.key[1].p, k.index[0].p, k.index[1].p, n, 0u, bounce_bits, st));
  hipLaunchKernelGGL(photon_key_path_kernel, grid, wg, 0, st, s.staging.p, k.index[1].p, n, first_sample, path_begin, path_bits, k.key[0].p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(rocprim::radix_sort_pairs(k.temp.p, bytes_b, k.key[0].p, k.key[1].p, k.index[1].p, k.index[0].p, n, 0u, path_end, st));   // stable: ties stay in bounce order
#ifdef AMBER_LAB
  if (s.stage_timing) HIP_TRY(hipEventRecord(s.ev[3].v, st));
#endif
  hipLaunchKernelGGL(photon_gather_kernel, dim3(static_cast<uint32_t>((static_cast<uint64_t>(n) * 4u + 255u) / 256u)), wg, 0, st, s.staging.p, k.index[0].p, n, dst);
  HIP_TRY(hipGetLastError());
#ifdef AMBER_LAB
  if (s.stage_timing) {
    HIP_TRY(hipEventRecord(s.ev[4].v, st));
    HIP_TRY(hipEventSynchronize(s.ev[4].v));
    float a = 0, b = 0;
    HIP_TRY(hipEventElapsedTime(&a, s.ev[2].v, s.ev[3].v)); HIP_TRY(hipEventElapsedTime(&b, s.ev[3].v, s.ev[4].v));
    s.sort_ms += a; s.gather_ms += b;
  }
#endif
  return AMBER_OK;
}

int TracePhotons(amber_hip_pt* h, uint32_t first_sample, uint32_t n_samples, uint32_t path_begin, uint32_t path_end, uint32_t surfaces,
                 AmberPhoton* out, uint64_t capacity, AmberPhotonInfo* info, uint32_t flags) {
  const std::string name = "amber_hip_lt_trace_photons";
  if (info) *info = AmberPhotonInfo{};
  if (!h) return Fail(AMBER_EINVAL, name + ": null handle");
  if (static_cast<uint64_t>(first_sample) + n_samples > 0xffffffffull) return Fail(AMBER_EINVAL, name + ": sample index overflow");
  const uint32_t all_paths = h->scene.sensor.w * h->scene.sensor.h;          // image.Size() light paths per pass
  if (path_begin > path_end || path_end > all_paths) return Fail(AMBER_EINVAL, name + ": bad light-path range");
  if (surfaces == 0u || (surfaces & ~static_cast<uint32_t>(AMBER_PHOTON_ALL))) return Fail(AMBER_EINVAL, name + ": surfaces must be a non-empty set of AMBER_PHOTON_* bits");
  if (flags & ~static_cast<uint32_t>(AMBER_PHOTONS_HOST)) return Fail(AMBER_EINVAL, name + ": unknown flag bits");
  if (!out && capacity) return Fail(AMBER_EINVAL, name + ": null output pointer with a capacity");
  const bool host = (flags & AMBER_PHOTONS_HOST) != 0u;
  if (!host && (reinterpret_cast<uintptr_t>(out) & 15u)) return Fail(AMBER_EINVAL, name + ": the device pointer must be 16-byte aligned");
  if (h->lights_stale) return Fail(AMBER_EINVAL, name + ": lights are stale after amber_hip_pt_update_objects: re-create the handle");
  if (h->engine == AMBER_ENGINE_WAVEFRONT) return Fail(AMBER_EINVAL, name + ": light tracing runs on the work-queue kernel (engine auto, list, two_phase or bvh)");
#if AMBER_BVH_WIDE
  return Fail(AMBER_EINVAL, name + ": not part of an AMBER_BVH_WIDE measurement build");
#endif
  const uint32_t n_paths = path_end - path_begin;
  if (n_samples == 0 || n_paths == 0 || h->scene.n_lights == 0) return AMBER_OK;
  HIP_TRY(hipSetDevice(h->device));
  AMBER_TRY(ResolvePending(h));   // (the work-queue head is shared with the render launches: a pass in flight that may have to be repeated stands first)
  AMBER_TRY(EnsurePhotonStaging(h, 0u));
  PhotonBufs& s = h->photons;
  HIP_TRY(hipMemsetAsync(s.rays.p, 0, sizeof(unsigned long long), h->stream));
  const bool counting = out == nullptr;
  AmberPhotonInfo total{};
  uint64_t written = 0;
  bool fits = true, repeated = false;
  unsigned long long rays_kept = 0;
  LtSink<float4> sink{s.staging, s.count.p, s.rays.p, surfaces};
#ifdef AMBER_LAB
  if (s.stage_timing) {
    for (Event& e : s.ev) if (!e.v) HIP_TRY(hipEventCreate(&e.v));
    sink.ev_begin = s.ev[0].v; sink.ev_end = s.ev[1].v;
  }
#endif
  const int rc = LtTraceLaunches(h, first_sample, n_samples, path_begin, n_paths, false, s.capacity, sink,
                                 [&](uint32_t first, uint32_t n, unsigned int produced, unsigned long long, unsigned long long rays_now, bool* again) -> int {
    total.n_launches++;
#ifdef AMBER_LAB
    if (s.stage_timing) { float ms = 0; HIP_TRY(hipEventElapsedTime(&ms, s.ev[0].v, s.ev[1].v)); s.trace_ms += ms; }   // (the launch has been waited for)
#endif
    const bool wanted = !counting && fits && total.n_photons + produced <= capacity;     // the records of this launch have a place in `out`
    if (wanted && produced > s.capacity) {
      // out of staging slots: nothing of this launch reaches `out`, the call's ray counter goes back, the buffer grows to what the launch reported
      // and the (deterministic) launch runs once more
      if (repeated) return Fail(AMBER_EHIP, name + ": a repeated launch produced more records than it reported the first time");
      if (produced > 0x7fffffffu) return Fail(AMBER_ENOMEM, name + ": more than 2^31 records in one launch");
      HIP_TRY(hipMemcpyAsync(s.rays.p, &rays_kept, sizeof rays_kept, hipMemcpyHostToDevice, h->stream));
      HIP_TRY(hipStreamSynchronize(h->stream));
      AMBER_TRY(EnsurePhotonStaging(h, produced));
      repeated = true; total.n_repeats++; *again = true;
      return AMBER_OK;
    }
    repeated = false;
    rays_kept = rays_now;
    if (!wanted) {
      if (!counting) fits = false;                         // `out` is too small: the call goes on counting, so that the caller learns what it needs
    } else if (produced) {
      if (!host) AMBER_TRY(PhotonOrder(h, produced, first, n, path_begin, n_paths, reinterpret_cast<float4*>(out + written)));
      else {
        AMBER_TRY(Grow(h, s.sorted, static_cast<size_t>(produced) * 4u, "sorted photons"));
        AMBER_TRY(PhotonOrder(h, produced, first, n, path_begin, n_paths, s.sorted.p));
        HIP_TRY(hipMemcpyAsync(out + written, s.sorted.p, static_cast<size_t>(produced) * sizeof(AmberPhoton), hipMemcpyDeviceToHost, h->stream));
      }
      written += produced;
    }
    total.n_photons += produced;
    return AMBER_OK;
  });
  if (rc != AMBER_OK) return rc;
  HIP_TRY(hipStreamSynchronize(h->stream));
  total.n_rays = rays_kept;
  total.n_written = !counting && fits ? written : 0u;
  if (info) *info = total;
  if (!counting && !fits) return Fail(AMBER_ENOMEM, name + ": photon buffer too small: " + std::to_string(total.n_photons) + " records needed");
  return AMBER_OK;
}

}  // namespace
