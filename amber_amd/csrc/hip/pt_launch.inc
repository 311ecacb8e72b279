// pt_launch.inc -- the host side of a render launch: grids, the timed-launch bracket, the one loop that splits a pass into launches (planned by
// launch_plan.h), the path-granular launch with its record buffer and its repeat, the item launch of engine BVH, the launches of light tracing.
// Part of the one translation unit pt_host.hip (the handle is defined there); see its header comment.
//
// Where a pass adds its sums is an argument (`target`): the framebuffer, or amber_hip_pt_render_batch's batch buffer.  Only two launches write it,
// reduce_flagged_kernel (FinishPathLaunch: LaunchPaths, and the lab build's LaunchLabRecords) and reduce_partials_kernel (RenderPassBvhItems).

namespace {
using amber_plan::kMaxPathsPerLaunch;

// launch() -- the render kernel(s) of one launch, whatever is enqueued in front of them already on the stream -- and the check that the runtime took
// it; `timed`: between the two events of a pair (amber_hip_pt_kernel_time counts the launch).  When the pool of 64 pairs is used up the finished
// launches are folded into the running totals (one stream synchronisation every 64 launches), so long renders (--spp 0 until expiry) do not grow it.
template <typename F>
int TimedLaunch(amber_hip_pt* h, bool timed, F&& launch) {
  LaunchTimer& t = h->timer;
  if (timed && t.used == 64) {
    HIP_TRY(hipStreamSynchronize(h->stream));
    for (size_t i = 0; i < t.used; i++) {
      float ms = 0;
      HIP_TRY(hipEventElapsedTime(&ms, t.events[i].first.v, t.events[i].second.v));
      t.folded_ms += ms;
    }
    t.folded_launches += static_cast<uint32_t>(t.used);
    t.used = 0;
  }
  if (timed && t.used == t.events.size()) {
    std::pair<Event, Event> ev;
    HIP_TRY(hipEventCreate(&ev.first.v)); HIP_TRY(hipEventCreate(&ev.second.v));
    t.events.push_back(std::move(ev));
  }
  std::pair<Event, Event>* const ev = timed ? &t.events[t.used++] : nullptr;
  if (ev) HIP_TRY(hipEventRecord(ev->first.v, h->stream));
  AMBER_TRY(launch());
  HIP_TRY(hipGetLastError());
  if (ev) HIP_TRY(hipEventRecord(ev->second.v, h->stream));
  return AMBER_OK;
}

// The samples [first_sample, first_sample + n_samples) in launches: plan(samples left, &launch) says how many the next one takes (launch_plan.h; none:
// the message `too_large`), enqueue(first, launch, &again) enqueues it -- and sets `again` to have exactly this launch planned and enqueued once more.
template <typename Plan, typename Enqueue>
int SplitSamples(uint32_t first_sample, uint32_t n_samples, const char* too_large, Plan&& plan, Enqueue&& enqueue) {
  uint32_t done = 0;
  while (done < n_samples) {
    amber_plan::Launch l{};
    AMBER_TRY(plan(n_samples - done, &l));
    if (l.n == 0) return Fail(AMBER_EINVAL, too_large);
    bool again = false;
    AMBER_TRY(enqueue(first_sample + done, l, &again));
    if (!again) done += l.n;
  }
  return AMBER_OK;
}

// Workgroups of the persistent kernels that fit a CU at once: pt_bvh_megakernel is bounded by its 24-entry LDS traversal stacks and
// VGPRs; the others are capped to AMBER_MEGAKERNEL_WAVES_PER_SIMD by their launch bounds.
uint32_t ResidentBlocksPerCu(uint32_t hit_engine) {
  return hit_engine == AMBER_ENGINE_BVH ? static_cast<uint32_t>(AMBER_BVH_WGS) : (AMBER_MEGAKERNEL_WAVES_PER_SIMD > 5 ? static_cast<uint32_t>(AMBER_MEGAKERNEL_WAVES_PER_SIMD) : 5u);   // uncapped: 87 VGPRs -> 5
}

// Workgroups of 256 threads for n_items work units (one thread each), `resident` at the most.
uint32_t BlocksFor(uint64_t n_items, uint32_t resident) {
  const uint64_t by_work = n_items / 256u + (n_items % 256u != 0u);
  return by_work < resident ? static_cast<uint32_t>(by_work) : resident;
}

// The grid of every persistent launch: workgroups of 256 threads, as many as fit the device at once, fewer if n_items work units (one
// thread each) do not need them.  The default n_items gives the largest grid, for which engine REFERENCE_BVH's stack is sized.  `pool`:
// pt_bvh_pool_kernel's grid (lab build).
uint32_t PersistentBlocks(const amber_hip_pt* h, uint64_t n_items, bool pool) {
  uint32_t n_blocks = static_cast<uint32_t>(h->n_cus) * ResidentBlocksPerCu(h->hit_engine);
#ifdef AMBER_LAB
  if (pool) n_blocks = static_cast<uint32_t>(h->n_cus) * static_cast<uint32_t>(AMBER_BVH_POOL_WGS);
#endif
  return BlocksFor(n_items, n_blocks);
}

// The one mapping from a handle's closest-hit engine to the engine its kernels are instantiated with: f(std::integral_constant<int, kEngine>).
// Each caller picks its kernel with `if constexpr`, so nothing is instantiated that is never launched.
template <typename F>
int WithHitEngine(uint32_t hit_engine, F&& f) {
  switch (hit_engine) {
    case AMBER_ENGINE_TWO_PHASE: return f(std::integral_constant<int, ENGINE_TWO_PHASE>());
    case kHitTwoPhaseN: return f(std::integral_constant<int, ENGINE_TWO_PHASE_N>());
    case AMBER_ENGINE_BVH: return f(std::integral_constant<int, ENGINE_BVH>());
    case AMBER_ENGINE_REFERENCE_BVH: return f(std::integral_constant<int, ENGINE_REF_BVH>());
    default: return f(std::integral_constant<int, ENGINE_LIST>());
  }
}

// Engine REFERENCE_BVH's stack has one column per thread of the largest grid (create; the handle remembers how many): a launch must not have more
// threads.  Every launch site of a kernel that walks that tree -- the render passes, light tracing, the ray queries, which share the one stack -- asks
// here first, before it takes anything (an event pair) it would have to give back.
int CheckRefStack(const amber_hip_pt* h, uint32_t n_blocks) {
  if (h->hit_engine == AMBER_ENGINE_REFERENCE_BVH && static_cast<uint64_t>(n_blocks) * 256u > h->ref_stack_threads)
    return Fail(AMBER_EINVAL, "engine REFERENCE_BVH: a grid of " + std::to_string(n_blocks) + " workgroups outgrows the traversal stack (" + std::to_string(h->ref_stack_threads) + " threads)");
  return AMBER_OK;
}

// Grows a buffer of the handle to at least n elements.  It may be in use: the stream is synchronised before it is freed.
template <typename T>
int Grow(amber_hip_pt* h, DevBuf<T>& b, size_t n, const char* what) {
  if (n <= b.n) return AMBER_OK;
  HIP_TRY(hipStreamSynchronize(h->stream));
  const hipError_t e = b.alloc(n);
  if (e != hipSuccess) return Fail(AMBER_ENOMEM, std::string("hipMalloc(") + what + "): " + hipGetErrorString(e));
  return AMBER_OK;
}

// (the labels name the caller's keys and permutation in an out-of-memory message)
int IndexSortBufs::Prepare(amber_hip_pt* h, uint32_t n_items, unsigned int end_bit0, unsigned int end_bit1, const char* keys_label, const char* order_label) {
  for (int k = 0; k < 2; k++) {
    AMBER_TRY(Grow(h, key[k], n_items, keys_label));
    AMBER_TRY(Grow(h, index[k], n_items, order_label));
  }
  stream = h->stream; n = n_items; end_bit[0] = end_bit0; end_bit[1] = end_bit1; cur = 0;
  temp_bytes[0] = temp_bytes[1] = 0;
  for (int i = 0; i < (end_bit1 ? 2 : 1); i++)               // (a null pointer: rocPRIM states the temporary storage pass i needs)
    HIP_TRY(rocprim::radix_sort_pairs(nullptr, temp_bytes[i], key[0].p, key[1].p, index[i].p, index[i ^ 1].p, n, 0u, end_bit[i], stream));
  return Grow(h, temp, std::max(temp_bytes[0], temp_bytes[1]), "sort scratch");
}

// What every launch of a render kernel states first: the scene, the seed, the handle's band, the samples and their chunks (with the dividers).
RenderArgs MakeRenderArgs(const amber_hip_pt* h, uint64_t hashed_seed, uint32_t n_pixels, uint32_t first_sample, uint32_t n_samples) {
  RenderArgs a{};
  a.scene = h->scene; a.hashed_seed = hashed_seed; a.SetBand(h->row_begin, h->stripe_rows, h->stripe_period); a.n_pixels = n_pixels;
  a.SetSamples(first_sample, n_samples); a.n_chunks = (n_samples + AMBER_ACCUM_CHUNK - 1) / AMBER_ACCUM_CHUNK;
  return a;
}

// ---- path-granular launches (pt_megakernel for engines LIST / TWO_PHASE, pt_bvh_pool_kernel for engine BVH) --------------
// One launch = megakernel + rank / scan / place / reduce.  The record buffer is sized from the density the previous launch
// measured (amber_plan::PathLaunch); the very first launch of a handle doubles as the probe.  A launch that still runs out of
// slots leaves its target and the ray total untouched (the device-side kernels check the counter); the host notices when it next
// touches the handle (ResolvePending), grows the buffer and repeats exactly that launch, so results never depend on the sizing.

// record slots that stay unused because every wave reserves them AMBER_REC_BLOCK at a time, plus a floor
uint64_t RecordSlack(const amber_hip_pt* h) { return static_cast<uint64_t>(h->n_cus) * 8u * 4u * AMBER_REC_BLOCK + 4096u; }

int EnsureRecordCapacity(amber_hip_pt* h, uint64_t slots) {
  PathLaunchBufs& p = h->paths;
  if (slots <= p.rec_capacity) return AMBER_OK;
  if (slots > 0xfffffff0ull) return Fail(AMBER_ENOMEM, "record buffer beyond 2^32 slots");
  p.rec_capacity = 0;
  AMBER_TRY(Grow(h, p.records, slots, "path records"));
  AMBER_TRY(Grow(h, p.sorted, slots * 3u, "path records"));
  p.rec_capacity = static_cast<uint32_t>(slots);
  return AMBER_OK;
}

int EnsureLaunchCtl(amber_hip_pt* h) {                                       // queue head | record count | rays of the launch: one block, one memset per launch
  PathLaunchBufs& p = h->paths;
  if (!p.launch_ctl) {
    HIP_TRY(p.launch_ctl.alloc(4));
    p.rec_count = p.launch_ctl + 1;
    p.rays_launch = reinterpret_cast<unsigned long long*>(p.launch_ctl + 2);
  }
  return AMBER_OK;
}

// Two-phase engine, once per handle: the candidate mask of every band pixel's eye rays (pixel_mask_kernel), enqueued on the render stream by
// create -- in front of the handle's first launch.  The buffer is allocated once and owned by the handle (amber_hip_pt_destroy releases it
// whatever step failed).  `timing` != null (amber_hip_kat_pixel_masks): run the kernel (again) between two events and report its duration.
int StartPixelMasks(amber_hip_pt* h, float* timing) {
  const uint32_t n_pixels = static_cast<uint32_t>(BandPixels(h));
  if (!(h->two_phase && h->env.pixel_mask) || n_pixels == 0 || (h->pixel_mask_ready && !timing)) return AMBER_OK;
  if (!h->d_pixel_mask) HIP_TRY(h->d_pixel_mask.alloc(n_pixels));
  PixelMaskArgs pm{};
  for (int i = 0; i < 4; i++) for (int c = 0; c < 3; c++) pm.ap[i][c] = static_cast<double>(h->aperture_rect[i][c]) - static_cast<double>(h->scene.fp_center[c]);
  pm.inv_w = 1.0 / static_cast<double>(h->scene.sensor.wf); pm.inv_h = 1.0 / static_cast<double>(h->scene.sensor.hf);
  pm.focal_scale = h->lens.kind == 1u ? -(8.0 * static_cast<double>(h->scene.fp_reach) + 1.0) / static_cast<double>(h->lens.sensor_distance)
                                      : static_cast<double>(h->lens.focus_distance) / -static_cast<double>(h->lens.sensor_distance);
  pm.row_begin = h->row_begin; pm.stripe_rows = h->stripe_rows; pm.stripe_period = h->stripe_period; pm.n_pixels = n_pixels;
  pm.block = (h->stripe_rows == 0u || h->stripe_rows % 4u == 0u) ? 4u : 1u;
  if (h->env.pixel_mask_block && (h->stripe_rows == 0u || h->stripe_rows % h->env.pixel_mask_block == 0u)) pm.block = h->env.pixel_mask_block;   // measurement hook
  pm.local_rows = h->local_rows;
  pm.blocks_x = (h->scene.sensor.w + pm.block - 1u) / pm.block;
  pm.n_blocks = pm.blocks_x * ((h->local_rows + pm.block - 1u) / pm.block);
  {
    // "does plane i cut the aperture rectangle?" -- the kernel's own expressions (binary64, the slack of its first lines), evaluated once
    const DevScene& sc = h->scene;
    const double cx = sc.fp_center[0], cy = sc.fp_center[1], cz = sc.fp_center[2], reach = sc.fp_reach;
    const double world_mag = std::max(std::max(std::fabs(cx), std::max(std::fabs(cy), std::fabs(cz))) + reach,
                                      std::max(std::fabs(double(h->lens.origin[0])), std::max(std::fabs(double(h->lens.origin[1])), std::fabs(double(h->lens.origin[2])))));
    const double slack = 1e-5 * reach + 32.0 * 5.9604644775390625e-08 * world_mag;
    pm.planes_cut_a = h->host_planes.size() > 32 ? 0xffffffffu : 0u;
    for (size_t i = 0; i < h->host_planes.size() && i < 32; i++) {
      const DevPlane& q = h->host_planes[i];
      bool above = true, below = true;
      for (int k = 0; k < 4; k++) {
        const double sa = double(q.n[0]) * pm.ap[k][0] + double(q.n[1]) * pm.ap[k][1] + double(q.n[2]) * pm.ap[k][2] - double(q.d0);
        above = above && sa > 10.0 * slack; below = below && sa < -10.0 * slack;
      }
      if (!(above || below)) pm.planes_cut_a |= 1u << i;
    }
  }
  Event ev0, ev1;
  if (timing) { HIP_TRY(hipEventCreate(&ev0.v)); HIP_TRY(hipEventCreate(&ev1.v)); HIP_TRY(hipEventRecord(ev0.v, h->stream)); }
  hipLaunchKernelGGL(pixel_mask_kernel, dim3((pm.n_blocks + 15u) / 16u), dim3(256), 0, h->stream, h->scene, pm, h->d_pixel_mask);   // 16 lanes per block of pixels
  HIP_TRY(hipGetLastError());
  if (timing) { HIP_TRY(hipEventRecord(ev1.v, h->stream)); HIP_TRY(hipEventSynchronize(ev1.v)); HIP_TRY(hipEventElapsedTime(timing, ev0.v, ev1.v)); }
  h->pixel_mask_ready = true;
  return AMBER_OK;
}

// pt_megakernel of the handle's engine, or pt_bvh_pool_kernel (`pool`, lab build); kSig: their signature instantiations (lab build)
template <bool kSig>
int LaunchPathKernel(const amber_hip_pt* h, bool pool, uint32_t n_blocks, const RenderArgs& a) {
  return WithHitEngine(h->hit_engine, [&](auto engine) -> int {
    constexpr int kEngine = decltype(engine)::value;
#ifdef AMBER_LAB
    if (kEngine == ENGINE_BVH && pool) { hipLaunchKernelGGL((pt_bvh_pool_kernel<kSig>), dim3(n_blocks), dim3(256), 0, h->stream, a); return AMBER_OK; }
#endif
    hipLaunchKernelGGL((pt_megakernel<kEngine, false, kSig>), dim3(n_blocks), dim3(256), 0, h->stream, a);
    return AMBER_OK;
  });
}

// A scouted launch (the handle's choice, amber_prep::DecideScout): pt_megakernel's weight-free instantiation leaves a placeholder record for every path that
// ends on a light or is suspect, replay_records_kernel traces those again with their weights and overwrites the placeholders (pt_replay.inc) -- the record
// buffer then holds what the full kernel would have written, plus +0 terms.  Stream order is all that joins the two; `replay` false: the scout alone
// (amber_hip_kat_scout_flags reads its bitmap).
int LaunchScoutedPaths(const amber_hip_pt* h, uint32_t n_blocks, const RenderArgs& a, bool replay) {
#if AMBER_SCOUT
  hipLaunchKernelGGL((pt_megakernel<ENGINE_TWO_PHASE | AMBER_KERNEL_SCOUT>), dim3(n_blocks), dim3(256), 0, h->stream, a);
  if (replay) hipLaunchKernelGGL((replay_records_kernel<ENGINE_TWO_PHASE>), dim3(static_cast<uint32_t>(h->n_cus) * 8u), dim3(256), 0, h->stream, a);
  return AMBER_OK;
#else
  return Fail(AMBER_EINVAL, "this build has no scout (AMBER_SCOUT=0)");
#endif
}

// A path launch in three parts, so that the reduction serves whatever produced the records: BeginPathLaunch (buffers, counters and bitmap ready),
// the producer's kernel, FinishPathLaunch (rank / scan / place / reduce, the launch becomes the pending one).

// Before the kernel: the bitmap, the touched bits and the ranks sized for n samples of n_pixels pixels, the control block zeroed, the bitmap cleared
// if the previous launch left it dirty, the touched bits cleared.  `sig`: a signature launch (nothing is reduced, so its bits stay).
int BeginPathLaunch(amber_hip_pt* h, uint32_t n, uint32_t n_pixels, bool sig) {
  PathLaunchBufs& p = h->paths;
  const uint64_t n_paths = static_cast<uint64_t>(n_pixels) * n;
  const size_t need_words = static_cast<size_t>((n_paths + 31u) / 32u) + 4u;
  if (need_words > p.flags.n) {
    AMBER_TRY(Grow(h, p.flags, need_words, "path bitmap"));
    p.flags_dirty = true;
  }
  const size_t touched_words = static_cast<size_t>(n_pixels) / 32u + 2u;
  AMBER_TRY(Grow(h, p.touched, touched_words, "touched pixels"));
  AMBER_TRY(Grow(h, p.excl, n_pixels, "pixel ranks"));
  AMBER_TRY(Grow(h, p.block_sum, static_cast<size_t>(n_pixels) / 256u + 2u, "pixel ranks"));
  AMBER_TRY(EnsureLaunchCtl(h));
  if (!p.h_rec_count.v) HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&p.h_rec_count.v), sizeof(unsigned int), hipHostMallocDefault));
  if (!p.pending_event.v) HIP_TRY(hipEventCreateWithFlags(&p.pending_event.v, hipEventDisableTiming));
  HIP_TRY(hipMemsetAsync(p.launch_ctl, 0, 4 * sizeof(unsigned int), h->stream));
  // The bitmap is cleared by the reduction itself where it can be (whole words per pixel); the host clears all of it only when a
  // launch left it dirty: the first use, sample counts that are not multiples of 32, signature launches, a launch that ran out of slots.
  if (p.flags_dirty) HIP_TRY(hipMemsetAsync(p.flags, 0, p.flags.n * sizeof(uint32_t), h->stream));
  p.flags_dirty = sig || (n & 31u) != 0u;
  HIP_TRY(hipMemsetAsync(p.touched, 0, touched_words * sizeof(uint32_t), h->stream));
  return AMBER_OK;
}

// What the record producers are handed: the buffers BeginPathLaunch prepared, in the kernels' argument block
void SetRecordArgs(const amber_hip_pt* h, RenderArgs& a) {
  const PathLaunchBufs& p = h->paths;
  a.flags = p.flags; a.touched = p.touched; a.records = p.records; a.rec_count = p.rec_count; a.rec_capacity = p.rec_capacity;
  a.ray_count = p.rays_launch; a.next_item = p.launch_ctl;
}

// After the kernel: the records of samples [first, first + n) ranked, placed and summed into `target`, the record counter on its way to the host, and
// the launch remembered as the one in flight.  `cannot_run_out`: it had a slot for every record it can produce.
int FinishPathLaunch(amber_hip_pt* h, uint32_t first, uint32_t n, uint32_t n_pixels, float* target, const RecordProducer& producer, bool cannot_run_out) {
  PathLaunchBufs& p = h->paths;
  const uint32_t n_rank_blocks = (n_pixels + 255u) / 256u;
  hipLaunchKernelGGL(rec_rank_kernel, dim3(n_rank_blocks), dim3(256), 0, h->stream, p.flags, p.touched, n_pixels, n, p.excl, p.block_sum);
  hipLaunchKernelGGL(rec_scan_blocks_kernel, dim3(1), dim3(1024), 0, h->stream, p.block_sum, n_rank_blocks, p.rec_count, p.rec_capacity, h->d_rays, p.rays_launch);
  hipLaunchKernelGGL(rec_place_kernel, dim3(static_cast<uint32_t>(h->n_cus) * 8u), dim3(256), 0, h->stream, p.records, p.rec_count, p.rec_capacity, p.flags,
                     p.excl, p.block_sum, n, MakeExactDiv(n), p.sorted);
  hipLaunchKernelGGL(reduce_flagged_kernel, dim3(n_rank_blocks), dim3(256), 0, h->stream, target, p.flags, p.touched, p.sorted, p.excl, p.block_sum,
                     p.rec_count, p.rec_capacity, n_pixels, n);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(p.h_rec_count.v, p.rec_count, sizeof(unsigned int), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipEventRecord(p.pending_event.v, h->stream));
  p.pending = true; p.pending_first = first; p.pending_n = n; p.pending_target = target; p.pending_producer = producer;
  p.pending_checked = cannot_run_out;
  ++p.n_launches;
  return AMBER_OK;
}

// Enqueues one launch over samples [first, first + n) of the band, its sums added to `target`.  `sig` != nullptr: the signature variant of the same
// kernel; nothing is reduced (amber_hip_pt_signatures).  `scout_only` (amber_hip_kat_scout_flags): the scout of a scouting handle without its replay; nothing is
// reduced either, the bitmap stays as the scout left it.
int LaunchPaths(amber_hip_pt* h, uint32_t first, uint32_t n, uint32_t n_pixels, float* target, unsigned long long* sig, bool scout_only = false) {
  PathLaunchBufs& p = h->paths;
  const uint64_t n_paths = static_cast<uint64_t>(n_pixels) * n;
#ifdef AMBER_LAB
  const bool bvh = h->hit_engine == AMBER_ENGINE_BVH && !h->bvh_paths;       // pt_bvh_pool_kernel (bvh_paths: pt_megakernel<ENGINE_BVH>)
#else
  const bool bvh = false;
  if (sig) return Fail(AMBER_EINVAL, "path signatures are part of the lab build");
#endif
  const uint32_t n_blocks = PersistentBlocks(h, n_paths, bvh);
  AMBER_TRY(CheckRefStack(h, n_blocks));
  {
    // measurements carried across bounces (degenerate paths only): pt_megakernel 3 floats per thread of the grid, pt_bvh_pool_kernel per ray of a wave
    size_t carried = static_cast<size_t>(PersistentBlocks(h)) * 256u * 3u * 2u;   // own slots + parked slots
#ifdef AMBER_LAB
    if (bvh) carried = static_cast<size_t>(h->n_cus) * AMBER_BVH_POOL_WGS * 4u * AMBER_BVH_POOL_CARRIED_PER_WAVE;
#endif
    AMBER_TRY(Grow(h, p.carried, carried, "carried measurements"));
  }
#ifdef AMBER_LAB
  if (bvh) AMBER_TRY(Grow(h, h->d_bvh_stack, static_cast<size_t>(h->n_cus) * AMBER_BVH_POOL_WGS * 256u * AMBER_BVH_POOL_GLOBAL_LEVELS, "traversal stacks"));
#endif
  AMBER_TRY(BeginPathLaunch(h, n, n_pixels, sig != nullptr || scout_only));
  RenderArgs a = MakeRenderArgs(h, h->hashed_seed, n_pixels, first, n);
  a.scout_bound0 = h->scout_bound0;
  a.pixel_mask = h->pixel_mask_ready ? h->d_pixel_mask : nullptr;
  SetRecordArgs(h, a);
  a.stamps = h->d_stamps;
  a.bvh_stack = h->d_bvh_stack; a.carried = p.carried; a.sig = sig; a.n_items = static_cast<uint32_t>(n_paths);
  AMBER_TRY(TimedLaunch(h, !scout_only, [&]() -> int {                    // (the lab's look at the scout's flags is not a render launch: kernel_time() does not count it)
#ifdef AMBER_LAB
    if (sig) return LaunchPathKernel<true>(h, bvh, n_blocks, a);
#endif
    if (h->scout) return LaunchScoutedPaths(h, n_blocks, a, !scout_only);
    return LaunchPathKernel<false>(h, bvh, n_blocks, a);
  }));
  if (sig || scout_only) return AMBER_OK;
  return FinishPathLaunch(h, first, n, n_pixels, target, RecordProducer{}, n_paths + RecordSlack(h) <= p.rec_capacity);   // a slot for every path: cannot run out
}

#ifdef AMBER_LAB
int LaunchLabRecords(amber_hip_pt* h, uint32_t n, uint32_t n_pixels, float* target, const RecordProducer& producer);   // lab_api.inc
#endif

// The host is about to read results or to enqueue work whose order matters: looks at the record counter of the launch in flight (waits for it),
// remembers the density, and repeats the launch -- exactly that one, from the producer it had, into the target it had -- with a larger buffer if it
// ran out of slots.
int ResolvePending(amber_hip_pt* h) {
  PathLaunchBufs& p = h->paths;
  while (p.pending) {
    HIP_TRY(hipEventSynchronize(p.pending_event.v));
    p.pending = false;
    const uint64_t used = *p.h_rec_count.v;
    const uint64_t n_paths = BandPixels(h) * p.pending_n;
    p.rec_density = n_paths ? static_cast<double>(used) / static_cast<double>(n_paths) : 0.0;
    p.density_known = true;
    if (used <= p.rec_capacity) break;
    // out of slots: nothing of that launch reached its target or the ray total (and its bits are still set)
    p.flags_dirty = true;
    ++p.n_repeats;
    AMBER_TRY(EnsureRecordCapacity(h, used + used / 4u + RecordSlack(h)));
#ifdef AMBER_LAB
    if (p.pending_producer.lab) {
      const RecordProducer producer = p.pending_producer;
      AMBER_TRY(LaunchLabRecords(h, p.pending_n, static_cast<uint32_t>(BandPixels(h)), p.pending_target, producer));
      continue;
    }
#endif
    AMBER_TRY(LaunchPaths(h, p.pending_first, p.pending_n, static_cast<uint32_t>(BandPixels(h)), p.pending_target, nullptr));
  }
  return AMBER_OK;
}

// The sums must stand before this call reads them (or moves on to another target): a launch in flight whose record buffer was sized from an
// estimate may have to be repeated, so it is waited for; one with a slot for every path, and every launch of the item kernel, needs no waiting.
int SettlePending(amber_hip_pt* h) { return h->paths.pending && !h->paths.pending_checked ? ResolvePending(h) : AMBER_OK; }

// sig != null (amber_hip_pt_signatures): one launch of the signature instantiation, its records discarded
int RenderPassPaths(amber_hip_pt* h, uint32_t first_sample, uint32_t n_samples, uint32_t n_pixels, float* target, unsigned long long* sig) {
  PathLaunchBufs& p = h->paths;
  if (sig) {
    AMBER_TRY(EnsureRecordCapacity(h, RecordSlack(h)));
    return LaunchPaths(h, first_sample, n_samples, n_pixels, target, sig);
  }
  const uint64_t slack = h->env.test_density_scale > 0 ? 64u : RecordSlack(h);   // (test hook: no cushion either)
  return SplitSamples(first_sample, n_samples, "band too large for one launch", [&](uint32_t left, amber_plan::Launch* l) -> int {
    // the previous launch must stand before the next one adds to the target (the order of the sums is part of the
    // contract), unless it had a slot for every path
    if (p.pending && (!p.pending_checked || !p.density_known)) AMBER_TRY(ResolvePending(h));
    *l = amber_plan::PathLaunch(n_pixels, left, p.density_known, p.rec_density, h->env.test_density_scale, slack);
    return AMBER_OK;
  }, [&](uint32_t first, const amber_plan::Launch& l, bool*) -> int {
    if (l.slots > p.rec_capacity) {
      if (p.pending) AMBER_TRY(ResolvePending(h));     // the buffer is in use
      AMBER_TRY(EnsureRecordCapacity(h, l.slots));
    }
    return LaunchPaths(h, first, l.n, n_pixels, target, nullptr);
  });
}

// Engine BVH, default scheduler (pt_bvh_megakernel: lanes own (pixel, chunk) items), per-item sums added to `target` by reduce_partials_kernel.
// sig != null (amber_hip_pt_signatures): one launch of the signature instantiation; nothing reaches the target or the ray total
int RenderPassBvhItems(amber_hip_pt* h, uint32_t first_sample, uint32_t n_samples, uint32_t n_pixels, float* target, unsigned long long* sig) {
#ifndef AMBER_LAB
  if (sig) return Fail(AMBER_EINVAL, "path signatures are part of the lab build");
#endif
  return SplitSamples(first_sample, n_samples, "band too large for one launch", [&](uint32_t left, amber_plan::Launch* l) -> int {
    *l = amber_plan::ItemLaunch(n_pixels, left);
    return AMBER_OK;
  }, [&](uint32_t first, const amber_plan::Launch& l, bool*) -> int {
    const uint32_t n_chunks = (l.n + AMBER_ACCUM_CHUNK - 1) / AMBER_ACCUM_CHUNK;
    AMBER_TRY(Grow(h, h->d_partial, static_cast<size_t>(n_chunks) * n_pixels * 3u, "partial sums"));
    if (sig && l.n != n_samples) return Fail(AMBER_EINVAL, "too many paths for one signature launch");
    if (sig) AMBER_TRY(EnsureLaunchCtl(h));
    RenderArgs a = MakeRenderArgs(h, h->hashed_seed, n_pixels, first, l.n);
    a.partial = h->d_partial; a.ray_count = sig ? h->paths.rays_launch : h->d_rays; a.next_item = h->d_next; a.stamps = h->d_stamps;
    a.n_items = n_pixels * n_chunks; a.sig = sig; a.shade_batch = h->bvh_shade_batch;
    // persistent workers: one workgroup of 4 waves per CU and resident wave slot, fewer if the queue is short
    const uint32_t n_blocks = PersistentBlocks(h, a.n_items);
    HIP_TRY(hipMemsetAsync(h->d_next, 0, sizeof(unsigned int), h->stream));
    AMBER_TRY(TimedLaunch(h, true, [&]() -> int {
#ifdef AMBER_LAB
      if (sig) { hipLaunchKernelGGL((pt_bvh_megakernel<false, 24, true>), dim3(n_blocks), dim3(256), 0, h->stream, a); return AMBER_OK; }
#endif
      hipLaunchKernelGGL((pt_bvh_megakernel<false, 24>), dim3(n_blocks), dim3(256), 0, h->stream, a);
      return AMBER_OK;
    }));
    if (sig) return AMBER_OK;                                  // the signature launch: nothing reaches the target
    const uint32_t n_elems = n_pixels * 3u;
    hipLaunchKernelGGL(reduce_partials_kernel, dim3((n_elems + 255u) / 256u), dim3(256), 0, h->stream, target, h->d_partial, n_elems, n_chunks);
    HIP_TRY(hipGetLastError());
    return AMBER_OK;
  });
}

// The samples [first, first + n) of the band's n_pixels pixels through the handle's work-queue kernels, the sums added to `target`: path-granular
// launches, or the item launches of engine BVH's default scheduler.  sig != null: their signature instantiations instead (lab build).
int RenderSamples(amber_hip_pt* h, uint32_t first, uint32_t n, uint32_t n_pixels, float* target, unsigned long long* sig) {
  if (h->hit_engine != AMBER_ENGINE_BVH || h->bvh_pool || h->bvh_paths) return RenderPassPaths(h, first, n, n_pixels, target, sig);
  return RenderPassBvhItems(h, first, n, n_pixels, target, sig);
}

// What the launches of light tracing write and count into (`sink`): the splat records of amber_hip_lt_trace_range / amber_hip_lt_render_pass with the
// handle's ray counter (SplatLtSink), or the vertex records of amber_hip_lt_trace_photons with a counter of that call's own (records of float4: the
// kernels' kPhotons instantiations, photon_surfaces their mask).  The buffer is named, not pointed to: the callback may grow it between two launches.
template <typename T>
struct LtSink {
  const DevBuf<T>& records; unsigned int* count; unsigned long long* rays; uint32_t photon_surfaces;
  hipEvent_t ev_begin = nullptr, ev_end = nullptr;          // measurements: recorded around the kernel of every launch
};
LtSink<DevSplat> SplatLtSink(const amber_hip_pt* h) { return LtSink<DevSplat>{h->d_splats, h->d_splat_count.p, h->d_rays.p, 0u}; }

// The argument checks the entry points of light tracing share, in the order `order` names them -- 'O' sample overflow, 'P' the light-path range,
// 'W' engine WAVEFRONT, 'S' stale lights: which message an input gets that fails several of them is part of each entry point's behaviour.
int LtCheck(const amber_hip_pt* h, const std::string& prefix, const char* order, uint32_t first_sample, uint32_t n_samples, uint32_t path_begin, uint32_t path_end) {
  for (const char* c = order; *c; c++) {
    if (*c == 'O' && static_cast<uint64_t>(first_sample) + n_samples > 0xffffffffull) return Fail(AMBER_EINVAL, prefix + "sample index overflow");
    if (*c == 'P' && (path_begin > path_end || path_end > h->scene.sensor.w * h->scene.sensor.h)) return Fail(AMBER_EINVAL, prefix + "bad light-path range");   // image.Size() light paths per pass
    if (*c == 'W' && h->engine == AMBER_ENGINE_WAVEFRONT) return Fail(AMBER_EINVAL, prefix + "light tracing runs on the work-queue kernel (engine auto, list, two_phase or bvh)");
    if (*c == 'S' && h->lights_stale) return Fail(AMBER_EINVAL, prefix + "lights are stale after amber_hip_pt_update_objects: re-create the handle");
  }
  return AMBER_OK;
}
bool LtNothingToDo(const amber_hip_pt* h, uint32_t n_samples, uint32_t n_paths) { return n_samples == 0 || n_paths == 0 || h->scene.n_lights == 0; }

// A launch of LtTraceLaunches produced more records than its buffer holds.  Nothing of it counts: the sink's ray counter goes back to what the launches
// before left (rays_kept), the buffer grows to what the launch reported (ensure) and the (deterministic) launch runs once more -- once: `repeated`
// is the caller's, cleared by every launch that fits.
int RepeatOutgrownLaunch(amber_hip_pt* h, const std::string& prefix, unsigned int produced, unsigned long long* d_rays, unsigned long long rays_kept,
                         int (*ensure)(amber_hip_pt*, uint32_t), bool* repeated, uint32_t* n_repeats, bool* again) {
  if (*repeated) return Fail(AMBER_EHIP, prefix + "a repeated launch produced more records than it reported the first time");
  if (produced > 0x7fffffffu) return Fail(AMBER_ENOMEM, prefix + "more than 2^31 records in one launch");
  HIP_TRY(hipMemcpyAsync(d_rays, &rays_kept, sizeof rays_kept, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  AMBER_TRY(ensure(h, produced));
  *repeated = true; (*n_repeats)++; *again = true;
  return AMBER_OK;
}

// The launches of light tracing over the passes [first_sample, first_sample + n_samples) of the light paths [path_begin, path_begin + n_paths): what
// amber_hip_lt_trace_range, amber_hip_lt_render_pass and amber_hip_lt_trace_photons share.  Each launch leaves its records at sink.records in arrival
// order (at most `capacity` of them, read again before every launch: the callback may have grown the buffer) and is waited for; then
//   after_launch(first, n, produced, rays_before, rays_now, &again)
// sees the passes of the launch, the records it produced (also beyond the capacity) and the sink's ray counter before the first launch and now.
// It returns a status other than AMBER_OK to stop, or sets `again` to have exactly this launch repeated.  `timed`: amber_hip_pt_kernel_time counts
// the launches.  n_samples and n_paths are not zero.
// Launches run in pass order and each one's records are sorted, so the concatenation is in (pass, path, bounce) order.
template <typename T, typename F>
int LtTraceLaunches(amber_hip_pt* h, uint32_t first_sample, uint32_t n_samples, uint32_t path_begin, uint32_t n_paths, bool timed, const uint32_t& capacity, const LtSink<T>& sink,
                    F&& after_launch) {
  const bool bvh = h->hit_engine == AMBER_ENGINE_BVH;
  const char* const too_many = "too many light paths for one launch";
  if (amber_plan::LightLaunch(n_paths, bvh, n_samples).n == 0) return Fail(AMBER_EINVAL, too_many);      // (before anything is enqueued)
  unsigned long long rays_before = 0, rays_now = 0;
  HIP_TRY(hipMemcpyAsync(&rays_before, sink.rays, sizeof rays_before, hipMemcpyDeviceToHost, h->stream));
  return SplitSamples(first_sample, n_samples, too_many, [&](uint32_t left, amber_plan::Launch* l) -> int {
    *l = amber_plan::LightLaunch(n_paths, bvh, left);
    return AMBER_OK;
  }, [&](uint32_t first, const amber_plan::Launch& l, bool* again) -> int {
    const uint32_t n_chunks = (l.n + AMBER_ACCUM_CHUNK - 1) / AMBER_ACCUM_CHUNK;
    const uint64_t n_work = bvh ? static_cast<uint64_t>(n_paths) * n_chunks : static_cast<uint64_t>(n_paths) * l.n;
    RenderArgs a = MakeRenderArgs(h, h->hashed_seed_lt, n_paths, first, l.n);
    a.SetBand(0u, 0u, 0u);                                    // light paths have no band; every divider of the launch is a valid record all the same
    a.ray_count = sink.rays; a.next_item = h->d_next;
    a.splats = reinterpret_cast<DevSplat*>(sink.records.p); a.splat_count = sink.count; a.splat_capacity = capacity; a.photon_surfaces = sink.photon_surfaces;
    a.path_offset = path_begin; a.n_items = static_cast<uint32_t>(n_work); a.shade_batch = h->bvh_shade_batch;
    const uint32_t n_blocks = PersistentBlocks(h, a.n_items);
    AMBER_TRY(CheckRefStack(h, n_blocks));
    HIP_TRY(hipMemsetAsync(sink.count, 0, sizeof(unsigned int), h->stream));
    HIP_TRY(hipMemsetAsync(h->d_next, 0, sizeof(unsigned int), h->stream));
    if (sink.ev_begin) HIP_TRY(hipEventRecord(sink.ev_begin, h->stream));
    AMBER_TRY(TimedLaunch(h, timed, [&]() -> int {
      return WithHitEngine(h->hit_engine, [&](auto engine) -> int {
        constexpr int kEngine = decltype(engine)::value;
        constexpr bool kPhotons = std::is_same<T, float4>::value;            // the vertex sink's records
        if constexpr (kEngine == ENGINE_BVH && kPhotons) hipLaunchKernelGGL((pt_bvh_megakernel<true, 24, false, true>), dim3(n_blocks), dim3(256), 0, h->stream, a);
        else if constexpr (kEngine == ENGINE_BVH) hipLaunchKernelGGL((pt_bvh_megakernel<true, 24>), dim3(n_blocks), dim3(256), 0, h->stream, a);   // light tracing on engine BVH: always the item kernel
        else if constexpr (kPhotons) hipLaunchKernelGGL((pt_megakernel<kEngine | AMBER_KERNEL_PHOTONS, true>), dim3(n_blocks), dim3(256), 0, h->stream, a);
        else hipLaunchKernelGGL((pt_megakernel<kEngine, true>), dim3(n_blocks), dim3(256), 0, h->stream, a);
        return AMBER_OK;
      });
    }));
    if (sink.ev_end) HIP_TRY(hipEventRecord(sink.ev_end, h->stream));
    unsigned int produced = 0;
    HIP_TRY(hipMemcpyAsync(&produced, sink.count, sizeof produced, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(&rays_now, sink.rays, sizeof rays_now, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return after_launch(first, l.n, produced, rays_before, rays_now, again);
  });
}

}  // namespace
