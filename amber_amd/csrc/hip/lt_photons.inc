// lt_photons.inc -- amber_hip_lt_trace_photons: the vertices of the light paths, in (sample, path, bounce) order, into the caller's buffer.
// Part of the one translation unit pt_host.hip (kernels are launched from there); see its header comment and include/amber_hip.h for the contract.
//
// The trace launch is light tracing's own (LtTraceLaunches, pt_launch.inc), with the vertex sink of PathShade (dev_shading.h, SINK_PHOTONS) instead
// of the splat: it leaves the 64-byte records of one launch in the handle's staging buffer in arrival order -- slots come from an atomic counter,
// claimed once per wave -- and counts its casts in a counter of the call's own.  What is new here takes them to the caller, the way
// lt_accumulate.inc takes splats to the framebuffer:
//   1. order      an index permutation sorted by (sample, path, bounce): two stable radix sorts (rocPRIM), first by bounce (as many bits as
//                 max_depth can set; all 32 when it is 0), then by (sample, path) relative to the launch, packed into the bits that the launch's
//                 pass count and the call's path range can set.  The sort is the handle's (IndexSortBufs: keys, permutations, rocPRIM's scratch).
//   2. gather     the records into `out` at the running offset, four lanes per record, 16 bytes each: the records move once.
// Launches run in pass order, so their concatenation is the global order.  The key names a record completely: the output does not depend on the
// arrival order.  A launch that runs out of staging slots is repeated once with the buffer it asked for (RepeatOutgrownLaunch, as in LtRenderPass).

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
  IndexSortBufs& sort = h->sort;
  const hipStream_t st = h->stream;
  const uint32_t max_depth = h->scene.max_depth;
  const unsigned int bounce_bits = max_depth == 0u || max_depth == 0xffffffffu ? 32u : BitsFor(max_depth + 1u);   // 1 <= bounce <= max_depth
  const uint32_t path_bits = BitsFor(n_paths);
  AMBER_TRY(sort.Prepare(h, n, bounce_bits, path_bits + BitsFor(n_launch_samples), "photon keys", "photon order"));
  const dim3 grid((n + 255u) / 256u), wg(256);
  AMBER_TRY(s.clock.Mark(2, st));                                       // (events 0, 1: around the trace kernel, LtTraceLaunches)
  hipLaunchKernelGGL(photon_key_bounce_kernel, grid, wg, 0, st, s.staging.p, n, sort.keys(), sort.order());
  HIP_TRY(hipGetLastError());
  AMBER_TRY(sort.Pass(0));
  hipLaunchKernelGGL(photon_key_path_kernel, grid, wg, 0, st, s.staging.p, sort.order(), n, first_sample, path_begin, path_bits, sort.keys());
  HIP_TRY(hipGetLastError());
  AMBER_TRY(sort.Pass(1));
  AMBER_TRY(s.clock.Mark(3, st));
  hipLaunchKernelGGL(photon_gather_kernel, dim3(static_cast<uint32_t>((static_cast<uint64_t>(n) * 4u + 255u) / 256u)), wg, 0, st, s.staging.p, sort.order(), n, dst);
  HIP_TRY(hipGetLastError());
  AMBER_TRY(s.clock.Mark(4, st));
  return s.clock.Lap(2, 4);
}

int TracePhotons(amber_hip_pt* h, uint32_t first_sample, uint32_t n_samples, uint32_t path_begin, uint32_t path_end, uint32_t surfaces,
                 AmberPhoton* out, uint64_t capacity, AmberPhotonInfo* info, uint32_t flags) {
  const std::string prefix = "amber_hip_lt_trace_photons: ";
  if (info) *info = AmberPhotonInfo{};
  if (!h) return Fail(AMBER_EINVAL, prefix + "null handle");
  AMBER_TRY(LtCheck(h, prefix, "OP", first_sample, n_samples, path_begin, path_end));
  if (surfaces == 0u || (surfaces & ~static_cast<uint32_t>(AMBER_PHOTON_ALL))) return Fail(AMBER_EINVAL, prefix + "surfaces must be a non-empty set of AMBER_PHOTON_* bits");
  if (flags & ~static_cast<uint32_t>(AMBER_PHOTONS_HOST)) return Fail(AMBER_EINVAL, prefix + "unknown flag bits");
  if (!out && capacity) return Fail(AMBER_EINVAL, prefix + "null output pointer with a capacity");
  const bool host = (flags & AMBER_PHOTONS_HOST) != 0u;
  if (!host && (reinterpret_cast<uintptr_t>(out) & 15u)) return Fail(AMBER_EINVAL, prefix + "the device pointer must be 16-byte aligned");
  AMBER_TRY(LtCheck(h, prefix, "SW", first_sample, n_samples, path_begin, path_end));
  AMBER_TRY(RefuseWideBuild(prefix));
  const uint32_t n_paths = path_end - path_begin;
  if (LtNothingToDo(h, n_samples, n_paths)) return AMBER_OK;
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
  AMBER_TRY(s.clock.Get(0, &sink.ev_begin));
  AMBER_TRY(s.clock.Get(1, &sink.ev_end));
  const int rc = LtTraceLaunches(h, first_sample, n_samples, path_begin, n_paths, false, s.capacity, sink,
                                 [&](uint32_t first, uint32_t n, unsigned int produced, unsigned long long, unsigned long long rays_now, bool* again) -> int {
    total.n_launches++;
    AMBER_TRY(s.clock.Lap(0, 1));                          // (the launch has been waited for)
    const bool wanted = !counting && fits && total.n_photons + produced <= capacity;     // the records of this launch have a place in `out`
    // out of staging slots: nothing of this launch reaches `out` (the ray counter is the call's own)
    if (wanted && produced > s.capacity) return RepeatOutgrownLaunch(h, prefix, produced, s.rays.p, rays_kept, EnsurePhotonStaging, &repeated, &total.n_repeats, again);
    repeated = false;
    rays_kept = rays_now;
    if (!wanted) {
      if (!counting) fits = false;                         // `out` is too small: the call goes on counting, so that the caller learns what it needs
    } else if (produced) {
      if (!host) AMBER_TRY(PhotonOrder(h, produced, first, n, path_begin, n_paths, reinterpret_cast<float4*>(out + written)));
      else {
        // through the handle's staging (HostStaging: the copy of the launch before has been waited for; Grow waits before it frees)
        DevBuf<uint8_t>& sorted = h->staging.out;
        AMBER_TRY(Grow(h, sorted, static_cast<size_t>(produced) * sizeof(AmberPhoton), "sorted photons"));
        AMBER_TRY(PhotonOrder(h, produced, first, n, path_begin, n_paths, reinterpret_cast<float4*>(sorted.p)));
        HIP_TRY(hipMemcpyAsync(out + written, sorted.p, static_cast<size_t>(produced) * sizeof(AmberPhoton), hipMemcpyDeviceToHost, h->stream));
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
  if (!counting && !fits) return Fail(AMBER_ENOMEM, prefix + "photon buffer too small: " + std::to_string(total.n_photons) + " records needed");
  return AMBER_OK;
}

}  // namespace
