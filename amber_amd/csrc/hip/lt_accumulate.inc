// lt_accumulate.inc -- amber_hip_lt_render_pass: a light-tracing pass into the handle's framebuffer on the device, in the reference's order.
// Part of the one translation unit pt_host.hip (kernels are launched from there); see its header comment and include/amber_hip.h for the contract.
//
// The trace launch is amber_hip_lt_trace_range's (LtTraceLaunches, pt_launch.inc).  It leaves the splat records of one launch in arrival order: the
// slot of a record comes from an atomic counter.  What is new here takes them to the framebuffer:
//   1. order      an index permutation sorted by (pixel, pass, path, bounce), all four full 32-bit fields: two stable 64-bit radix sorts (rocPRIM),
//                 first by (path, bounce), then by (pixel, pass).  The 32-byte records never move; the colours are gathered once, into sorted order.
//   2. sum        one thread per pixel run (a record whose predecessor names another pixel is a run's head) walks its records in order, forms the
//                 pass image's value P_s from +0 and adds it to the framebuffer at each pass boundary.  The additions of one pixel are a dependent
//                 chain by definition; the parallelism is across pixels.  A pixel belongs to one thread of the launch: plain loads and stores.
// The result does not depend on the arrival order: the sort key names a record completely.

namespace {

// key = (path, bounce), index = identity
__global__ void __launch_bounds__(256) lt_key_path_kernel(const DevSplat* __restrict__ rec, uint32_t n, unsigned long long* __restrict__ key, uint32_t* __restrict__ index) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint4 r = *reinterpret_cast<const uint4*>(&rec[i]);            // path, sample, bounce, pixel
  key[i] = (static_cast<unsigned long long>(r.x) << 32) | r.z;
  index[i] = i;
}

// key = (pixel, pass) of the records in (path, bounce) order
__global__ void __launch_bounds__(256) lt_key_pixel_kernel(const DevSplat* __restrict__ rec, const uint32_t* __restrict__ index, uint32_t n, unsigned long long* __restrict__ key) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint4 r = *reinterpret_cast<const uint4*>(&rec[index[i]]);
  key[i] = (static_cast<unsigned long long>(r.w) << 32) | r.y;
}

// the colours into sorted order: what the sum reads is contiguous per run
__global__ void __launch_bounds__(256) lt_gather_kernel(const DevSplat* __restrict__ rec, const uint32_t* __restrict__ index, uint32_t n, float4* __restrict__ value) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  value[i] = *reinterpret_cast<const float4*>(&rec[index[i]].rgb[0]);  // rgb, pad
}

constexpr int kLtSumBatch = 8;              // records of a run loaded ahead of the chain of additions that consumes them

// key: (pixel, pass) ascending, equal keys in (path, bounce) order.  The thread of a run's head does the run; every other thread leaves.
__global__ void __launch_bounds__(256) lt_sum_kernel(const unsigned long long* __restrict__ key, const float4* __restrict__ value, uint32_t n, uint32_t n_pixels,
                                                     float* __restrict__ fb, unsigned int* __restrict__ longest) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const unsigned long long head = key[i];
  const uint32_t pixel = static_cast<uint32_t>(head >> 32);
  if (i != 0u && static_cast<uint32_t>(key[i - 1u] >> 32) == pixel) return;
  if (pixel >= n_pixels) return;                                       // (no record names such a pixel: the lens response and the hook's check see to it)
  float* const dst = fb + static_cast<size_t>(pixel) * 3u;
  float sr = dst[0], sg = dst[1], sb = dst[2];
  float pr = 0.0f, pg = 0.0f, pb = 0.0f;                               // P_s[pixel]
  uint32_t pass = static_cast<uint32_t>(head), run = 0u, best = 0u;
  bool more = true;
  for (uint32_t j = i; more; j += kLtSumBatch) {
    unsigned long long k[kLtSumBatch];
    float4 v[kLtSumBatch];
#pragma unroll
    for (int b = 0; b < kLtSumBatch; b++) {
      const uint32_t at = j + b < n ? j + b : n - 1u;
      k[b] = key[at]; v[b] = value[at];
    }
#pragma unroll
    for (int b = 0; b < kLtSumBatch; b++) {
      if (more && (j + b >= n || static_cast<uint32_t>(k[b] >> 32) != pixel)) more = false;
      if (more) {
        const uint32_t s = static_cast<uint32_t>(k[b]);
        if (s != pass) {                                               // the pass image is complete: sum += image
          sr = sr + pr; sg = sg + pg; sb = sb + pb;
          pr = 0.0f; pg = 0.0f; pb = 0.0f;
          best = run > best ? run : best; run = 0u; pass = s;
        }
        pr = pr + v[b].x; pg = pg + v[b].y; pb = pb + v[b].z;
        run++;
      }
    }
  }
  sr = sr + pr; sg = sg + pg; sb = sb + pb;
  best = run > best ? run : best;
  dst[0] = sr; dst[1] = sg; dst[2] = sb;
  if (best > *reinterpret_cast<volatile unsigned int*>(longest)) atomicMax(longest, best);   // (a counter of the info struct, not the framebuffer)
}

uint32_t BitsFor(uint32_t below) {            // bits that hold every value < below
  uint32_t bits = 0;
  while (bits < 32u && (below - 1u) >> bits) bits++;
  return below > 1u ? bits : 1u;
}

int EnsureLtSplats(amber_hip_pt* h, uint32_t capacity) {
  LtAccumBufs& s = h->lt;
  if (s.capacity < AMBER_LT_SPLAT_CAPACITY0) s.capacity = AMBER_LT_SPLAT_CAPACITY0;
  if (s.capacity < capacity) s.capacity = capacity;
  AMBER_TRY(Grow(h, h->d_splats, s.capacity, "splats"));
  if (!h->d_splat_count) HIP_TRY(h->d_splat_count.alloc(1));
  if (!s.longest) HIP_TRY(s.longest.alloc(1));
  return AMBER_OK;
}

// The n records at h->d_splats (0 < n < 2^31, any order) into the framebuffer.  path_bits: the bits of `path` that can be set (32: any).  Enqueued on
// the handle's stream; the buffers may grow first, which waits for the stream.
int LtAccumulate(amber_hip_pt* h, uint32_t n, uint32_t path_bits) {
  LtAccumBufs& s = h->lt;
  const uint32_t n_pixels = h->scene.sensor.w * h->scene.sensor.h;
  const hipStream_t st = h->stream;
  for (int k = 0; k < 2; k++) {
    AMBER_TRY(Grow(h, s.key[k], n, "splat keys"));
    AMBER_TRY(Grow(h, s.index[k], n, "splat order"));
  }
  AMBER_TRY(Grow(h, s.value, n, "sorted splats"));
  // (path, bounce): bounce has no bound (max_depth == 0), all its 32 bits count; (pixel, pass): pass is any 32-bit value, pixel < n_pixels
  const unsigned int path_end = 32u + path_bits, pixel_end = 32u + BitsFor(n_pixels);
  size_t bytes_a = 0, bytes_b = 0;
  HIP_TRY(rocprim::radix_sort_pairs(nullptr, bytes_a, s.key[0].p, s.key[1].p, s.index[0].p, s.index[1].p, n, 0u, path_end, st));
  HIP_TRY(rocprim::radix_sort_pairs(nullptr, bytes_b, s.key[0].p, s.key[1].p, s.index[1].p, s.index[0].p, n, 0u, pixel_end, st));
  AMBER_TRY(Grow(h, s.temp, std::max(bytes_a, bytes_b), "sort scratch"));
  const dim3 grid((n + 255u) / 256u), wg(256);
#ifdef AMBER_LAB
  if (s.stage_timing) {
    for (Event& e : s.ev) if (!e.v) HIP_TRY(hipEventCreate(&e.v));
    HIP_TRY(hipEventRecord(s.ev[0].v, st));
  }
#endif
  hipLaunchKernelGGL(lt_key_path_kernel, grid, wg, 0, st, h->d_splats.p, n, s.key[0].p, s.index[0].p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(rocprim::radix_sort_pairs(s.temp.p, bytes_a, s.key[0].p, s.key[1].p, s.index[0].p, s.index[1].p, n, 0u, path_end, st));
  hipLaunchKernelGGL(lt_key_pixel_kernel, grid, wg, 0, st, h->d_splats.p, s.index[1].p, n, s.key[0].p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(rocprim::radix_sort_pairs(s.temp.p, bytes_b, s.key[0].p, s.key[1].p, s.index[1].p, s.index[0].p, n, 0u, pixel_end, st));   // stable: ties stay in (path, bounce) order
  hipLaunchKernelGGL(lt_gather_kernel, grid, wg, 0, st, h->d_splats.p, s.index[0].p, n, s.value.p);
  HIP_TRY(hipGetLastError());
#ifdef AMBER_LAB
  if (s.stage_timing) HIP_TRY(hipEventRecord(s.ev[1].v, st));
#endif
  hipLaunchKernelGGL(lt_sum_kernel, grid, wg, 0, st, s.key[1].p, s.value.p, n, n_pixels, h->d_fb.p, s.longest.p);
  HIP_TRY(hipGetLastError());
#ifdef AMBER_LAB
  if (s.stage_timing) {
    HIP_TRY(hipEventRecord(s.ev[2].v, st));
    HIP_TRY(hipEventSynchronize(s.ev[2].v));
    float a = 0, b = 0;
    HIP_TRY(hipEventElapsedTime(&a, s.ev[0].v, s.ev[1].v)); HIP_TRY(hipEventElapsedTime(&b, s.ev[1].v, s.ev[2].v));
    s.sort_ms += a; s.sum_ms += b;
  }
#endif
  return AMBER_OK;
}

// A handle whose framebuffer is the whole frame: light paths land anywhere in it
bool WholeFrame(const amber_hip_pt* h) { return h->row_begin == 0u && h->row_end == h->scene.sensor.h && h->stripe_period == 0u && h->stripe_rows == 0u; }

int LtRenderPass(amber_hip_pt* h, uint32_t first_sample, uint32_t n_samples, AmberLtPassInfo* info) {
  const std::string name = "amber_hip_lt_render_pass";
  if (info) *info = AmberLtPassInfo{};
  if (!h) return Fail(AMBER_EINVAL, name + ": null handle");
  if (static_cast<uint64_t>(first_sample) + n_samples > 0xffffffffull) return Fail(AMBER_EINVAL, name + ": sample index overflow");
  if (h->engine == AMBER_ENGINE_WAVEFRONT) return Fail(AMBER_EINVAL, name + ": light tracing runs on the work-queue kernel (engine auto, list, two_phase or bvh)");
  if (h->lights_stale) return Fail(AMBER_EINVAL, name + ": lights are stale after amber_hip_pt_update_objects: re-create the handle");
  if (!WholeFrame(h)) return Fail(AMBER_EINVAL, name + ": the handle renders a band or stripes of the frame; light paths land anywhere in it (use amber_hip_lt_trace_range and merge on the host)");
  if (n_samples == 0 || h->scene.n_lights == 0) return AMBER_OK;
  HIP_TRY(hipSetDevice(h->device));
  AMBER_TRY(ResolvePending(h));   // the order of the sums: a path-tracing pass in flight must stand first
  AMBER_TRY(EnsureLtSplats(h, 0u));
  LtAccumBufs& s = h->lt;
  HIP_TRY(hipMemsetAsync(s.longest.p, 0, sizeof(unsigned int), h->stream));
  const uint32_t n_paths = h->scene.sensor.w * h->scene.sensor.h;
  AmberLtPassInfo total{};
  unsigned long long rays_begin = 0, rays_kept = 0;
  bool have_begin = false, repeated = false;
  const int rc = LtTraceLaunches(h, first_sample, n_samples, 0u, n_paths, true, s.capacity, SplatLtSink(h),
                                 [&](uint32_t, uint32_t, unsigned int produced, unsigned long long rays_before, unsigned long long rays_now, bool* again) -> int {
    if (!have_begin) { rays_begin = rays_kept = rays_before; have_begin = true; }
    total.n_launches++;
    if (produced > s.capacity) {
      // out of slots: nothing of this launch reaches the framebuffer, the ray counter goes back, the buffer grows to what the launch reported
      // and the (deterministic) launch runs once more
      if (repeated) return Fail(AMBER_EHIP, name + ": a repeated launch produced more records than it reported the first time");
      if (produced > 0x7fffffffu) return Fail(AMBER_ENOMEM, name + ": more than 2^31 records in one launch");
      HIP_TRY(hipMemcpyAsync(h->d_rays, &rays_kept, sizeof rays_kept, hipMemcpyHostToDevice, h->stream));
      HIP_TRY(hipStreamSynchronize(h->stream));
      AMBER_TRY(EnsureLtSplats(h, produced));
      repeated = true; total.n_repeats++; *again = true;
      return AMBER_OK;
    }
    repeated = false;
    rays_kept = rays_now;
    total.n_splats += produced;
    return produced ? LtAccumulate(h, produced, BitsFor(n_paths)) : AMBER_OK;
  });
  if (rc != AMBER_OK) return rc;
  unsigned int longest = 0;
  HIP_TRY(hipMemcpyAsync(&longest, s.longest.p, sizeof longest, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  total.n_rays = rays_kept - rays_begin; total.longest_run = longest;
  if (info) *info = total;
  return AMBER_OK;
}

}  // namespace
