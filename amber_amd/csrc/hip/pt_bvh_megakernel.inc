// pt_bvh_megakernel.inc -- engine BVH on deep trees: the item kernel with the resumable per-lane traversal, and the reduction of its per-item sums.
// Part of the one translation unit pt_host.hip (kernels are launched from there); see its header comment.

// Engine BVH worker.  Same work queue, item walk and accumulation order as pt_megakernel, but the closest-hit query
// is a per-lane tree traversal whose length varies by an order of magnitude between the lanes of a wave (1M-sphere
// scene: 24 % VALU lane utilisation when every bounce waits for the slowest lane).  Traversal is therefore
// RESUMABLE (BvhTrav in registers, stack in LDS): the wave keeps running traversal rounds until
// AMBER_BVH_SHADE_BATCH lanes have finished theirs (or nobody traverses any more), shades exactly those lanes --
// hit resolution, material sampling, Russian roulette, regeneration -- starts their next rays and resumes.  Lanes
// never wait for more than a batch to fill; results do not depend on the schedule (paths are independent and a
// lane's samples are still summed in order).
#ifndef AMBER_BVH_SHADE_BATCH
#define AMBER_BVH_SHADE_BATCH 52   // config 3 at 128 spp, one process (descent budget 5): 24 -> 173 ms, 32 -> 172, 40 -> 166, 48 -> 162, 52 -> 160, 56 -> 160.5, 60 -> 164, 64 (wait for all lanes) -> 181
#endif
// kStack: entries of the per-lane LDS stack (chosen from the tree depth at create time).  24 entries = 24 KB per
// workgroup let 5 workgroups share a CU (96 VGPRs), 32 entries only 4: config 3, 128 spp: 193 vs 208 ms.
#ifndef AMBER_BVH_WGS
#define AMBER_BVH_WGS 5
#endif
// kSig (tests only, amber_hip_pt_signatures): the same kernel also hashes every cast's hit object and hit distance and stores the pair
// at the path's end -- config 3's PRODUCT kernel compared with the oracle path by path, like pt_megakernel's signature instantiation.
// kPhotons (with kLight, amber_hip_lt_trace_photons): a vertex record per selected hit instead of the splats (PathShade, SINK_PHOTONS).
template <bool kLight, int kStack, bool kSig = false, bool kPhotons = false>
__global__ void __launch_bounds__(256, kStack <= 24 && !kSig ? AMBER_BVH_WGS : 4) pt_bvh_megakernel(const RenderArgs a) {
  const DevScene& sc = a.scene;
  const uint32_t lane = threadIdx.x & 63u;
  __shared__ int32_t lds_stack[kStack * 256];
  // the item's running sum is touched once per PATH (2.6 rays): it lives in LDS ([component][thread]: conflict-free), not in three of
  // the 96 registers the traversal loop is short of -- the compiler used to keep it in scratch
  __shared__ float lds_sum[6 * 256];                       // rows 0-2: the item's sum; rows 3-5: the measurement of the path in flight.  (Two more rows for y, z of the
                                                           // throughput -- what the compiler spills next -- make 32 KB per workgroup: five no longer fit a CU, 113 ms instead of 101 at 128 spp)
  float* const my_sum = lds_sum + threadIdx.x;

  WaveClaim claim;
  bool lane_done = false, have_item = false, alive = false, traversing = false;
  uint32_t s = 0, s_end = 0, pixel = 0, slot = 0;          // the pixel's x, y are recomputed where a path starts: two registers less
  PathRay ray;                                              // (ray.meas lives in LDS between bounces: rows 3-5 of lds_sum)
  ray.o = v3(0.f, 0.f, 0.f); ray.d = v3(0.f, 0.f, 1.f); ray.w = v3(0.f, 0.f, 0.f);
  ray.rng = 1; ray.casts = 0; ray.origin_slot = -1;
  uint32_t rays_wave = 0;                                   // wave-uniform (SGPR): rays shaded by this wave
  PathSig sig; sig.Reset();                                 // kSig only
  BvhTrav tr; HitRec hit;
  BvhIdle(tr, hit);
#ifdef AMBER_STAMPS
  StampCtx stamp_store{}, stamp_shade{}; StampCtx* stamp_ctx = &stamp_store;     // counters here; PathShade's clocks go to a dummy
#define AMBER_SHADE_STAMP_ARG , &stamp_shade
  stamp_ctx->last = __builtin_amdgcn_s_memtime();
#else
#define AMBER_SHADE_STAMP_ARG
#endif

  for (;;) {
    bool need = !alive && s >= s_end && !lane_done;
    if (need && have_item) {                                // item finished: publish its sum
      if (!kLight) {
        float* p = a.partial + static_cast<size_t>(slot) * 3u;
        p[0] = my_sum[0]; p[1] = my_sum[256]; p[2] = my_sum[512];
      }
      have_item = false;
    }
    uint32_t item = 0;
    if (ServeLanes<64u>(claim, a.next_item, a.n_items, lane, need, item)) {     // hand out work items, 64 to a claim
      const uint32_t plocal = item / a.n_chunks, chunk = item - plocal * a.n_chunks;
      // (plain divisions, once per item: the exact dividers of exact_div.h were measured here and the kernel was no faster, EXPERIMENTS.md)
      const uint32_t lrow = plocal / sc.sensor.w;
      const uint32_t px = plocal - lrow * sc.sensor.w;
      const uint32_t py = a.row_begin + (a.stripe_rows ? (lrow / a.stripe_rows) * a.stripe_period + lrow % a.stripe_rows : lrow);
      pixel = kLight ? a.path_offset + plocal : px + py * sc.sensor.w;      // light tracing: the light path's index
      slot = chunk * a.n_pixels + plocal;
      s = a.first_sample + chunk * AMBER_ACCUM_CHUNK;
      const uint32_t left = a.first_sample + a.n_samples - s;
      s_end = s + (left < AMBER_ACCUM_CHUNK ? left : AMBER_ACCUM_CHUNK);
      my_sum[0] = 0.f; my_sum[256] = 0.f; my_sum[512] = 0.f;
      have_item = true;
      need = false;
    }
    if (need) lane_done = true;
    if (__ballot(!lane_done) == 0ull) break;

    AMBER_CLK(0);
    if (!alive && !lane_done) {                             // regenerate: next sample of the item, start its traversal
      AMBER_COUNT_ROUNDS(3);
      ray.rng = XorShiftSeed(a.hashed_seed, pixel, s);
      if (kLight) {
        GenerateLightRay(sc, ray.rng, ray.o, ray.d, ray.w, ray.origin_slot);
      } else {
        float ew;
        const uint32_t py = pixel / sc.sensor.w;
        GenerateEyeRay(sc, pixel - py * sc.sensor.w, py, ray.rng, ray.o, ray.d, ew, ray.origin_slot);
        ray.w = v3(ew, ew, ew);
      }
      my_sum[768] = 0.f; my_sum[1024] = 0.f; my_sum[1280] = 0.f;
      ray.casts = 0;
      alive = true;
      ++s;
      if (kSig) sig.Reset();
      BvhBegin(sc, ray.o, ray.d, tr, hit);
      traversing = true;
    }

    AMBER_CLK(1);
    for (;;) {                                              // traversal rounds until a batch of lanes is ready to shade
      const unsigned long long tm = __ballot(traversing);
      if (tm == 0ull) break;
      if (static_cast<uint32_t>(__popcll(__ballot(alive && !traversing))) >= a.shade_batch) break;
      if (traversing) {
        AMBER_COUNT_ROUNDS(2);
        traversing = BvhRound(sc, lds_stack, ray.o, ray.d, tr, hit, kStack AMBER_STAMP_ARG);
        if (!traversing && tr.overflow) ClosestHitLeafList(sc, ray.o, ray.d, hit);
      }
    }

    AMBER_CLK(6);
    rays_wave += static_cast<uint32_t>(__popcll(__ballot(alive && !traversing)));
    if (alive && !traversing) {                             // shade the lanes whose closest hit is known
      V3& meas = ray.meas;
      meas = v3(my_sum[768], my_sum[1024], my_sum[1280]);     // the measurement is read and written once per bounce: LDS, not registers held across the traversal
      if (kLight) {
        if (kPhotons) BvhResolveIndex(sc, hit);               // a vertex names its object
        const typename std::conditional<kPhotons, PhotonSink, SplatSink>::type sink = MakeLightSink<kPhotons>(a, pixel, s - 1u);
        BounceExtras extras; extras.sink = &sink;
        alive = PathShade<LightBounceCfg<ENGINE_BVH, kPhotons>>(sc, nullptr, hit, ray, extras AMBER_SHADE_STAMP_ARG);
      } else if (kSig) {
        BvhResolveIndex(sc, hit);                             // only the signature variant reports object indices
        Bounce b;
        BounceExtras extras; extras.trace = &b;
        alive = PathShade<TracedBounceCfg<ENGINE_BVH>>(sc, nullptr, hit, ray, extras AMBER_SHADE_STAMP_ARG);
        sig.Add(b);
        if (!alive) {                                         // path (band pixel, sample s - 1) of this launch
          const uint32_t plocal = slot % a.n_pixels;
          a.sig[static_cast<size_t>(plocal) * a.n_samples + (s - 1u - a.first_sample)] = sig.Packed();
        }
      } else {
        alive = PathShade<BounceCfg<ENGINE_BVH>>(sc, nullptr, hit, ray, BounceExtras{} AMBER_SHADE_STAMP_ARG);
      }
      if (alive) { my_sum[768] = meas.x; my_sum[1024] = meas.y; my_sum[1280] = meas.z; }
      if (alive) { BvhBegin(sc, ray.o, ray.d, tr, hit); traversing = true; }
      else { my_sum[0] = my_sum[0] + meas.x; my_sum[256] = my_sum[256] + meas.y; my_sum[512] = my_sum[512] + meas.z; }   // sequential sum over the item's samples
    }
    AMBER_CLK(5);
  }

#undef AMBER_SHADE_STAMP_ARG
#ifdef AMBER_STAMPS
#ifdef AMBER_BVH_CLOCKS
  if (a.stamps) for (int k = 0; k < 8; k++) atomicAdd(a.stamps + k, stamp_ctx->acc[k] >> 6);      // lane-time / 64
#else
  if (a.stamps) for (int k = 0; k < 8; k++) if (stamp_ctx->acc[k]) atomicAdd(a.stamps + k, stamp_ctx->acc[k]);
#endif
#endif
  if (lane == 0 && rays_wave) atomicAdd(a.ray_count, static_cast<unsigned long long>(rays_wave));
}

// fb[e] += partial[0][e] + partial[1][e] + ... in chunk order (e = pixel*3 + channel of the band)
__global__ void reduce_partials_kernel(float* __restrict__ fb, const float* __restrict__ partial, uint32_t n_elems, uint32_t n_chunks) {
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_elems) return;
  float v = fb[e];
  for (uint32_t c = 0; c < n_chunks; ++c) v = v + partial[static_cast<size_t>(c) * n_elems + e];
  fb[e] = v;
}

