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
  IndexSortBufs& sort = h->sort;
  const uint32_t n_pixels = h->scene.sensor.w * h->scene.sensor.h;
  const hipStream_t st = h->stream;
  // (path, bounce): bounce has no bound (max_depth == 0), all its 32 bits count; (pixel, pass): pass is any 32-bit value, pixel < n_pixels
  AMBER_TRY(sort.Prepare(h, n, 32u + path_bits, 32u + BitsFor(n_pixels), "splat keys", "splat order"));
  AMBER_TRY(Grow(h, s.value, n, "sorted splats"));
  const dim3 grid((n + 255u) / 256u), wg(256);
  AMBER_TRY(s.clock.Mark(0, st));
  hipLaunchKernelGGL(lt_key_path_kernel, grid, wg, 0, st, h->d_splats.p, n, sort.keys(), sort.order());
  HIP_TRY(hipGetLastError());
  AMBER_TRY(sort.Pass(0));
  hipLaunchKernelGGL(lt_key_pixel_kernel, grid, wg, 0, st, h->d_splats.p, sort.order(), n, sort.keys());
  HIP_TRY(hipGetLastError());
  AMBER_TRY(sort.Pass(1));
  hipLaunchKernelGGL(lt_gather_kernel, grid, wg, 0, st, h->d_splats.p, sort.order(), n, s.value.p);
  HIP_TRY(hipGetLastError());
  AMBER_TRY(s.clock.Mark(1, st));
  hipLaunchKernelGGL(lt_sum_kernel, grid, wg, 0, st, sort.sorted_keys(), s.value.p, n, n_pixels, h->d_fb.p, s.longest.p);
  HIP_TRY(hipGetLastError());
  AMBER_TRY(s.clock.Mark(2, st));
  return s.clock.Lap(0, 2);
}

// A handle whose framebuffer is the whole frame: light paths land anywhere in it
bool WholeFrame(const amber_hip_pt* h) { return h->row_begin == 0u && h->row_end == h->scene.sensor.h && h->stripe_period == 0u && h->stripe_rows == 0u; }

int LtRenderPass(amber_hip_pt* h, uint32_t first_sample, uint32_t n_samples, AmberLtPassInfo* info) {
  const std::string prefix = "amber_hip_lt_render_pass: ";
  if (info) *info = AmberLtPassInfo{};
  if (!h) return Fail(AMBER_EINVAL, prefix + "null handle");
  const uint32_t n_paths = h->scene.sensor.w * h->scene.sensor.h;
  AMBER_TRY(LtCheck(h, prefix, "OWS", first_sample, n_samples, 0u, n_paths));
  if (!WholeFrame(h)) return Fail(AMBER_EINVAL, prefix + "the handle renders a band or stripes of the frame; light paths land anywhere in it (use amber_hip_lt_trace_range and merge on the host)");
  if (LtNothingToDo(h, n_samples, n_paths)) return AMBER_OK;
  HIP_TRY(hipSetDevice(h->device));
  AMBER_TRY(ResolvePending(h));   // the order of the sums: a path-tracing pass in flight must stand first
  AMBER_TRY(EnsureLtSplats(h, 0u));
  LtAccumBufs& s = h->lt;
  HIP_TRY(hipMemsetAsync(s.longest.p, 0, sizeof(unsigned int), h->stream));
  AmberLtPassInfo total{};
  unsigned long long rays_begin = 0, rays_kept = 0;
  bool have_begin = false, repeated = false;
  const int rc = LtTraceLaunches(h, first_sample, n_samples, 0u, n_paths, true, s.capacity, SplatLtSink(h),
                                 [&](uint32_t, uint32_t, unsigned int produced, unsigned long long rays_before, unsigned long long rays_now, bool* again) -> int {
    if (!have_begin) { rays_begin = rays_kept = rays_before; have_begin = true; }
    total.n_launches++;
    // out of slots: nothing of this launch reaches the framebuffer
    if (produced > s.capacity) return RepeatOutgrownLaunch(h, prefix, produced, h->d_rays.p, rays_kept, EnsureLtSplats, &repeated, &total.n_repeats, again);
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
