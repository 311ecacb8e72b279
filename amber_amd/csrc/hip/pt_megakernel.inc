// pt_megakernel.inc -- the path-granular work-queue kernel (engines LIST, TWO_PHASE, BVH on shallow trees; light tracing).
// Part of the one translation unit pt_host.hip (kernels are launched from there); see its header comment.

// pt_megakernel: persistent waves, work unit = ONE PATH, lanes decoupled from pixels.
//
//  * Paths of a launch are numbered q = plocal * n_samples + k (band pixel, sample offset): 64 consecutive paths are 64
//    samples of one pixel (coherent eye rays, first hits and materials).  A wave claims AMBER_CLAIM_PATHS paths with ONE
//    atomicAdd on the global queue head.
//  * Eye rays are generated 64 at a time, by ALL lanes of the wave, into the wave's pool in LDS (SoA, 64 slots); a lane
//    whose path has ended pops the next ray from the pool (ballot + mbcnt rank), whichever path that is.  Round 1's
//    kernel regenerated in place, i.e. the whole wave executed the eye-ray code for the half of its lanes whose paths had
//    just ended -- 16 % of the kernel at 48 % lane utilisation; here that code runs once per 64 paths with every lane
//    busy, and no lane ever waits: a generation round happens only when the pool cannot serve a lane.
//  * Accumulation.  Lanes no longer own pixels, so a path that ends with a non-zero measurement (it reached a light:
//    2e-5 of the Cornell paths) appends a record {q, rgb} and sets bit q of a bitmap (EmitRecords); the rank / place /
//    reduce kernels below then form, per pixel, exactly the sums of the numerical contract -- samples of a chunk of
//    AMBER_ACCUM_CHUNK in order, chunk sums added to the framebuffer in chunk order (DESIGN.md section 8) -- skipping the
//    +0 terms, which is exact: a running binary32 sum that starts at +0 never becomes -0, and x + (+0) = x for every
//    other x.  HBM per launch: the bitmap (n_paths / 8 bytes, cleared and read once) and 16 B per record.
//  * kLight: the same worker loop traces LIGHT paths (algorithm_lt.cc:112-163): path q = (light path index, pass),
//    nothing is stored at a path's end, Eye hits append splat records instead.
//  * kPhotons (with kLight, amber_hip_lt_trace_photons; kEngineSink = engine | AMBER_KERNEL_PHOTONS): the same light paths append a vertex record per
//    selected hit instead (PathShade, SINK_PHOTONS).
//  * kSig (tests only, amber_hip_pt_signatures): the same kernel also hashes every cast's hit object and hit distance and
//    stores the pair at the path's end -- the PRODUCT kernel's paths, compared with the oracle's one by one.
#define AMBER_WAVE_TIME_SLOTS 8192u          /* diagnostic build: per-wave timestamps behind the 8 section sums of RenderArgs.stamps */
#ifndef AMBER_MEGAKERNEL_WAVES_PER_SIMD
#define AMBER_MEGAKERNEL_WAVES_PER_SIMD 6
#endif
// Paths a wave claims from the global queue head with one atomicAdd.  One L2 word retires ~88 returning atomics per
// microsecond (MI355X_MICROARCH.md, "dequeue"): claiming 64 paths at a time (1.7e7 atomics per config-2 launch) made the
// queue head the bottleneck -- 190 ms per launch; 1024 paths (16 generation rounds) is 15 atomics per microsecond, and the
// tail it can leave on one wave is ~35 iterations (80 us).  Round 3 measured the queue again (tools/launch_fixed_cost.py, kernel time
// = fixed + slope * spp on config 2's frame): a claim costs the wave 4.4 us (512 / 1024 / 2048 / 4096 paths per claim: slope 51.67 /
// 50.97 / 50.60 / 50.21 us per spp, i.e. 0.75 ms of a 52.8-ms launch at 1024), the fixed part of a launch is 0.59 / 0.63 / 0.81 / 1.17 ms
// -- 0.5 ms of it independent of the claim size (9 % of a rank's step when 8 GPUs share config 2) -- and it is NOT the idle -> busy
// transition (8 launches back to back cost the same each, tools/launch_back_to_back.py).  Tried and dropped: guided claims
// ((paths left) / (2 waves), 256 .. 1024, from a fresh load of the queue head): +4 ms per launch -- the extra load of the hot word costs
// more than a claim -- and a static first claim per wave (no start-up burst of 6144 atomics): -0.05 ms, within noise of its cost.
#ifndef AMBER_CLAIM_PATHS
#define AMBER_CLAIM_PATHS 1024u
#endif
// Pool slot: the whole state of a path between two bounces in four 16-byte chunks {o.xyz d.x} {d.yz w.xy} {w.z rng q}
// {casts | carried-flag, origin slot, signature hashes}.  kScout: three chunks {o.xyz d.x} {d.yz rng} {q casts origin-slot bound} -- no weight, nothing carried.
// (A carried measurement itself travels through global memory, next to the slot: the kernel copies it.)  Park below writes a slot; the pop in the kernel
// is the layout's other implementation, written out there: through a helper pt_megakernel<2,0,0> loses its pinned instruction stream (EXPERIMENTS.md).
template <bool kLight, bool kScout = false> struct PoolLayout {
  static constexpr int kChunks = kScout ? 3 : 4;
  static __device__ __forceinline__ void Park(uint4* slot, V3 o, V3 d, V3 w, uint64_t rng, uint32_t q, uint32_t casts, bool carries, int origin_slot, const PathSig& sig, uint32_t scout_bound) {
    slot[0] = make_uint4(__float_as_uint(o.x), __float_as_uint(o.y), __float_as_uint(o.z), __float_as_uint(d.x));
    if constexpr (kScout) {
      slot[1] = make_uint4(__float_as_uint(d.y), __float_as_uint(d.z), static_cast<uint32_t>(rng), static_cast<uint32_t>(rng >> 32));
      slot[2] = make_uint4(q, casts, static_cast<uint32_t>(origin_slot), scout_bound);
    } else {
      slot[1] = make_uint4(__float_as_uint(d.y), __float_as_uint(d.z), __float_as_uint(w.x), __float_as_uint(w.y));
      slot[2] = make_uint4(__float_as_uint(w.z), static_cast<uint32_t>(rng), static_cast<uint32_t>(rng >> 32), q);
      slot[3] = make_uint4(casts | (carries ? 0x80000000u : 0u), static_cast<uint32_t>(origin_slot), sig.obj, sig.t);
    }
  }
};

// Traversal-stack entries of pt_megakernel<ENGINE_BVH> (a deeper tree renders with pt_bvh_megakernel): 12 KB of LDS next to the 16-KB
// pool, five workgroups per CU (16 entries: four).  Where the two schedulers cross over (tools/mesh_workloads.py, 1024^2 @ 256 spp, a room
// with a tessellated ball): Cornell's tree of depth 6, 30.7 ms against 44.2 for pt_bvh_megakernel; 1.3 k triangles, depth 12: 52.7 against
// 54.7; 5 k triangles, depth 14 (built with 16 entries): 64.9 against 57.6 -- beyond depth 12 the resumable item kernel wins.
#ifndef AMBER_PATH_BVH_STACK
#define AMBER_PATH_BVH_STACK 12
#endif
// The vertex sink is selected by a bit of the engine argument, not by a fourth parameter: the symbols of the instantiations that exist are what tests
// and tools find the headline kernel's ISA by, and a parameter more, defaulted or not, renames every one of them.
#define AMBER_KERNEL_PHOTONS 0x100
// AMBER_KERNEL_SCOUT, another bit of the engine argument for the same reason: THE SCOUT, the eye-path loop without the path weight.  A path's weight reaches the
// image only through measurement += weight * Radiance, which is not +0 only where the path ends on a light (2e-5 of the Cornell paths) or after a weight has
// become inf or NaN; Russian roulette reads the scatter weight, never the accumulated one.  So the scout traces every path with the same rays, draws and tests
// but forms no eye weight (GenerateEyeRay<.., kScout>), no weight quotients and products (PathShade, SINK_SCOUT) and carries neither the weight nor a
// measurement (three pool chunks); in the weight's place a lane keeps an integer bound of what the weight can have grown to (scout_bound.h).  A path that ends
// on a light whose Radiance is not (+0, +0, +0), or whose bound says a weight may have overflowed (`suspect`), leaves a placeholder record {q, 0, 0, 0};
// replay_records_kernel (pt_replay.inc) then traces exactly those paths again with the full bounce and overwrites the placeholders.  Instantiated for
// ENGINE_TWO_PHASE eye paths without signatures; -DAMBER_SCOUT=0 compiles the feature out (A/B builds), AMBER_PT_FLAG_NO_SCOUT selects the full kernel per handle.
#define AMBER_KERNEL_SCOUT 0x200
#ifndef AMBER_SCOUT
#define AMBER_SCOUT 1
#endif
// What the eye-path instantiations compile a bounce for: kCold (below) selects the arithmetic family -- Normalize's three quotients through one reciprocal
// (shared_div.h) and the square roots from one v_rsq_f32 seed (exact_sqrt.h; the switch bits: dev_math.h).  replay_records_kernel takes the same, cold.
template <int kEngine_, bool kCold> struct PathBounceCfg : BounceCfg<kEngine_> {
  static constexpr bool kDivBasis = kCold && (AMBER_SHARED_DIV_NORMALIZE & 1), kDivHit = kCold && (AMBER_SHARED_DIV_NORMALIZE & 2);
  static constexpr uint32_t kSqrtMask = kCold ? static_cast<uint32_t>(AMBER_EXACT_SQRT) : 0u;
  static constexpr bool kPremask = true;
  static constexpr int kBvhStackCap = AMBER_PATH_BVH_STACK;
};
template <int kEngine_, bool kCold> struct PathSigCfg : PathBounceCfg<kEngine_, kCold> { static constexpr bool kTrace = true; };
template <int kEngine_, bool kCold> struct PathScoutCfg : PathBounceCfg<kEngine_, kCold> { static constexpr int kSink = SINK_SCOUT; };
template <int kEngine_, bool kPhotons> struct PathLightCfg : LightBounceCfg<kEngine_, kPhotons> { static constexpr int kBvhStackCap = AMBER_PATH_BVH_STACK; };
template <int kEngineSink, bool kLight = false, bool kSig = false>
__global__ void __launch_bounds__(256, (kEngineSink & ~(AMBER_KERNEL_PHOTONS | AMBER_KERNEL_SCOUT)) == ENGINE_BVH ? 5 : AMBER_MEGAKERNEL_WAVES_PER_SIMD) pt_megakernel(const RenderArgs a) {
  constexpr int kEngine = kEngineSink & ~(AMBER_KERNEL_PHOTONS | AMBER_KERNEL_SCOUT);
  constexpr bool kPhotons = (kEngineSink & AMBER_KERNEL_PHOTONS) != 0;
  constexpr bool kScout = (kEngineSink & AMBER_KERNEL_SCOUT) != 0;
  static_assert(kLight || !kPhotons, "vertices are recorded along light paths");
  static_assert(!kScout || (kEngine == ENGINE_TWO_PHASE && !kLight && !kSig), "the scout is the headline kernel's loop");
  const DevScene& sc = a.scene;
  const uint32_t lane = threadIdx.x & 63u;
  // What a bounce of this kernel is handed besides the path.  Declared HERE, ahead of the loop, for the pinned instruction stream only: declared next to
  // the call, pt_megakernel<2,0,0> differs from its parent by one commuted s_and_b64.  So `trace` and `sink` hold addresses of block-local objects that
  // end with their block: every field a configuration reads is set again in front of each call, and nothing may read `extras` anywhere else.
  BounceExtras extras;
  constexpr bool kTwoPhase = EngineTraits<kEngine>::kTwoPhase;
  using Pool = PoolLayout<kLight, kScout>;
  constexpr int kChunks = Pool::kChunks;
  constexpr bool kCold = !kLight && kEngine != ENGINE_BVH;    // cold kernel arguments are read next to their use (AMBER_ARG below)
  // a cold argument, read next to its use (pt_args.h).  Two families keep the plain form: the light tracer (its bounces read n_samples and
  // first_sample themselves, and with these reads the kernel reserved scratch) and engine BVH's one-shot traversal (measured: Cornell through
  // ENGINE_BVH 118.6 -> 120.0 ms, the room mesh 52.7 -> 53.6 ms with cold reads, EXPERIMENTS.md).
  // The arithmetic of PathBounceCfg, for the bounce and the eye ray: the same family, for the same kind of reason (the light tracers and <ENGINE_BVH> were
  // not measured with it and keep the plain divisions and roots)
  constexpr bool kDivEye = kCold && (AMBER_SHARED_DIV_NORMALIZE & 4);
  constexpr uint32_t kSqrtMask = PathBounceCfg<kEngine, kCold>::kSqrtMask;
#define AMBER_ARG(cold, field) (kCold ? AMBER_COLD(cold, field) : a.field)
#define AMBER_COLD_OPEN() (kCold ? ColdArgs::Open() : ColdArgs{nullptr})
  __shared__ uint4 lds_pool[4][64 * kChunks];                 // [wave][slot * kChunks + chunk]
  // engine BVH on a SHALLOW tree (mid-size scenes, RenderPassPaths): the closest hit is one uninterrupted per-lane traversal (ClosestHitBvh),
  // its stack [level][thread] in LDS -- a few dozen node visits differ little between the lanes of a wave, so nothing has to be resumable,
  // and the path-granular scheduling above (coherent primary rounds, no lane waits for a shading batch) is what a small scene gains most from
  const EngineLds lds = StageEngineLds<kEngine, AMBER_PATH_BVH_STACK>(sc);
  const uint32_t wave_in_block = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform, and the compiler knows it: what derives from it stays in SGPRs
  uint4* pool = lds_pool[wave_in_block];

  uint32_t claim_next = 0, claim_end = 0;    // wave-uniform: paths claimed from the global queue, not yet generated
  uint32_t pool_count = 0;                   // wave-uniform: rays in the pool (slots [0, pool_count))
  uint32_t rec_next = 0, rec_end = 0;        // wave-uniform: the wave's open block of record slots
  bool exhausted = false;                    // wave-uniform: the global queue is empty
  bool retired = false, alive = false;
  uint32_t q = 0;                            // path of this lane
  // The measurement is NOT kept in registers between bounces: emitted radiance is non-zero only on a DiffuseLight, whose
  // scatter weight 0 ends the path, so a path that continues has measurement +0 -- unless a weight has become inf or NaN
  // (inf * 0 = NaN: degenerate scenes), and such a path parks its measurement in global memory and sets `carries`.
  bool carries = false;
  // (its address is formed where it is used, from a thread index the optimiser cannot see through: hoisted out of the
  //  persistent loop, the pointer is the one value the register cap pushes into scratch)
  // (kCold: the block index goes through an empty asm per use.  blockIdx.x * 256 as a 64-bit pair is loop-invariant, and held across the loop
  //  it is a scalar register pair that the loop does not have: with the eye ray's shared division the allocator parked it in lanes and
  //  fetched it back at each of the four uses -- tests/test_headline_kernel_spills.py.  The other two families keep the plain expression.)
  auto block_index = []() -> size_t { uint32_t b = blockIdx.x; if (kCold) asm volatile("" : "+s"(b)); return b; };
  auto carried_slot = [&]() -> float* {
    const uint32_t t = wave_in_block * 64u + BvhStackHybrid::LaneId();     // = threadIdx.x, from an SGPR and two v_mbcnt
    return AMBER_ARG(AMBER_COLD_OPEN(), carried) + (block_index() * 256u + t) * 3u;
  };
#define AMBER_CARRIED() carried_slot()
  // a carried measurement travels with its ray: parked with it (a second block of slots, one per pool slot of the wave) and handed to
  // the lane that pops the ray -- rays change lanes since the primary rounds
  auto carried_parked = [&](uint32_t pool_slot) -> float* {
    return AMBER_ARG(AMBER_COLD_OPEN(), carried) + (static_cast<size_t>(gridDim.x) * 256u + (block_index() * 4u + wave_in_block) * 64u + pool_slot) * 3u;
  };
  V3 o = v3(0.f, 0.f, 0.f), d = v3(0.f, 0.f, 1.f), w = v3(0.f, 0.f, 0.f);
  uint64_t rng = 1;
  uint32_t casts = 0;
  uint32_t scout_bound = 0;                  // kScout: scout_bound.h's bound of log2 |weight|, sixteenths of a bit; above kLimit: `suspect`
  uint32_t rays_wave = 0;                    // wave-uniform (SGPR): rays cast by this wave
  int origin_slot = -1;                      // filter-program slot of the triangle the current ray starts on
  PathSig sig; sig.Reset();                  // kSig only
#ifdef AMBER_STAMPS
  StampCtx stamp_store{}; StampCtx* stamp_ctx = &stamp_store;
  stamp_ctx->last = __builtin_amdgcn_s_memtime();
  unsigned long long* wave_times = a.stamps ? a.stamps + 8 + 4ull * ((blockIdx.x * 4u + wave_in_block) % AMBER_WAVE_TIME_SLOTS) : nullptr;
  if (wave_times && lane == 0) { wave_times[0] = wall_clock64(); wave_times[1] = 0; wave_times[2] = 0; }
#endif

  for (;;) {
    AMBER_STAMP(6);
    const bool need = !alive && !retired;
    const unsigned long long mask = __ballot(need);
    bool primary = false;                                     // wave-uniform: this iteration's rays are 64 fresh paths whose candidates are known (premask)
    uint32_t premask = 0u;
    if (mask) {                                               // wave-uniform
      const uint32_t n_need = static_cast<uint32_t>(__popcll(mask));
      const uint32_t rank = WaveRank(mask);
      // (1) the parked rays first
      const uint32_t take = pool_count < n_need ? pool_count : n_need;
      if (kScout) {
        if (need && rank < take) {                            // pop
          const uint32_t sl = pool_count - 1u - rank;
          const uint4 c0 = pool[sl * kChunks + 0], c1 = pool[sl * kChunks + 1], c2 = pool[sl * kChunks + 2];
          o = v3(__uint_as_float(c0.x), __uint_as_float(c0.y), __uint_as_float(c0.z));
          d = v3(__uint_as_float(c0.w), __uint_as_float(c1.x), __uint_as_float(c1.y));
          rng = static_cast<uint64_t>(c1.z) | (static_cast<uint64_t>(c1.w) << 32);
          q = c2.x; casts = c2.y; origin_slot = static_cast<int>(c2.z); scout_bound = c2.w;
          alive = true;
        }
      } else if (need && rank < take) {                       // pop
        const uint32_t sl = pool_count - 1u - rank;
        const uint4 c0 = pool[sl * kChunks + 0], c1 = pool[sl * kChunks + 1], c2 = pool[sl * kChunks + 2], c3 = pool[sl * kChunks + 3];
        o = v3(__uint_as_float(c0.x), __uint_as_float(c0.y), __uint_as_float(c0.z));
        d = v3(__uint_as_float(c0.w), __uint_as_float(c1.x), __uint_as_float(c1.y));
        w = v3(__uint_as_float(c1.z), __uint_as_float(c1.w), __uint_as_float(c2.x));
        rng = static_cast<uint64_t>(c2.y) | (static_cast<uint64_t>(c2.z) << 32);
        q = c2.w;
        casts = c3.x & 0x7fffffffu; carries = (c3.x >> 31) != 0u;
        if (!kLight && carries) { const float* from = carried_parked(sl); float* to = AMBER_CARRIED(); to[0] = from[0]; to[1] = from[1]; to[2] = from[2]; }
        origin_slot = static_cast<int>(c3.y);
        if (kSig) { sig.obj = c3.z; sig.t = c3.w; }
        alive = true;
      }
      __builtin_amdgcn_wave_barrier();                        // (compiler fence: the park below overwrites the slots just read)
      pool_count -= take;
      if (take < n_need && !exhausted) {
        // (2) the pool is empty and lanes still wait: a PRIMARY ROUND.  Every lane that holds a ray parks it in the pool;
        // all 64 lanes then start the next 64 paths of the queue TOGETHER -- 64 samples of one pixel: one coherent iteration
        // (first hits, materials) at full width; the parked rays go to whichever lanes lose their path afterwards.
        AMBER_STAMP(0);
        if (claim_next == claim_end) {                        // claim the next block of paths from the global queue
          const ColdArgs cold = AMBER_COLD_OPEN();   // the queue: cold arguments, read here (pt_args.h)
          const uint32_t size = AMBER_CLAIM_PATHS;                         // (claims sized from what is left of the queue were measured neutral and removed: EXPERIMENTS.md, round 4)
          uint32_t base = 0;
          const uint32_t n_items = AMBER_ARG(cold, n_items);
          if (lane == 0) base = atomicAdd(AMBER_ARG(cold, next_item), size);
          base = __builtin_amdgcn_readfirstlane(base);
          if (base >= n_items) exhausted = true;
          else { claim_next = base; claim_end = n_items - base < size ? n_items : base + size; }
#ifdef AMBER_STAMPS
          if (wave_times && lane == 0) { if (exhausted) wave_times[2] = wall_clock64(); else if (wave_times[1] == 0) wave_times[1] = wall_clock64(); }
#endif
        }
        if (!exhausted) {
          const uint32_t n_new = claim_end - claim_next < 64u ? claim_end - claim_next : 64u;
          const uint32_t gbase = claim_next;
          claim_next += n_new;
          const unsigned long long m_alive = __ballot(alive);
          if (alive) {                                        // park (pool_count is 0 here)
            const uint32_t sl = WaveRank(m_alive);
            Pool::Park(pool + sl * kChunks, o, d, w, rng, q, casts, carries, origin_slot, sig, scout_bound);
            if (!kLight && !kScout && carries) { const float* from = AMBER_CARRIED(); float* to = carried_parked(sl); to[0] = from[0]; to[1] = from[1]; to[2] = from[2]; }
          }
          pool_count = static_cast<uint32_t>(__popcll(m_alive));
          __builtin_amdgcn_wave_barrier();
          alive = lane < n_new;
          // what places the 64 new paths in the frame is needed once per round, never by a bounce: cold arguments, read here (pt_args.h)
          const ColdArgs cold = AMBER_COLD_OPEN();
          if (alive) {
            q = gbase + lane;
            // the divisors are launch constants: exact multiply-and-shift dividers formed by the host (exact_div.h), no divide sequences here
            const uint32_t n_samples = AMBER_ARG(cold, n_samples), first_sample = AMBER_ARG(cold, first_sample);
            const uint32_t plocal = Quotient(AMBER_ARG(cold, div_samples), q), sample = first_sample + (q - plocal * n_samples);
            if (kLight) {
              rng = XorShiftSeed(a.hashed_seed, a.path_offset + plocal, sample);
              GenerateLightRay(sc, rng, o, d, w, origin_slot);
            } else {
              const uint32_t lrow = Quotient(AMBER_ARG(cold, div_width), plocal);
              const EyeRayScene eye{AMBER_ARG(cold, scene.lens), AMBER_ARG(cold, scene.blades), AMBER_ARG(cold, scene.sensor)};
              const uint32_t row_begin = AMBER_ARG(cold, row_begin), stripe_rows = AMBER_ARG(cold, stripe_rows);
              const uint32_t px = plocal - lrow * eye.sensor.w;
              uint32_t py = row_begin + lrow;
              if (stripe_rows) {                              // 0 = contiguous rows: no divider
                const uint32_t band = Quotient(AMBER_ARG(cold, div_stripe_rows), lrow);
                py = row_begin + band * AMBER_ARG(cold, stripe_period) + (lrow - band * stripe_rows);
              }
              rng = XorShiftSeed(AMBER_ARG(cold, hashed_seed), px + py * eye.sensor.w, sample);   // Image index x + y*W (image.h:116-124)
              float ew;
              bool near_edge = false;
              GenerateEyeRay<kDivEye, SqrtModeOf(kSqrtMask, 4u), kScout>(eye, px, py, rng, o, d, ew, origin_slot, &near_edge);
              if (kScout) {                                   // ew: the guard quantity, not a weight; NaN fails the guard
                scout_bound = (Abs(ew) >= amber_scout::kMinZ && Abs(ew) < __builtin_inff()) ? AMBER_ARG(cold, scout_bound0) : amber_scout::kSuspect;
              } else w = v3(ew, ew, ew);                  // Leading<RGB>(.., Radiant(weight)) lens_basic.h:139-144
              // (the pointer is read here and once more below, not held across the bookkeeping above: the two scalar registers it would occupy
              //  there are what the dividers need, and the loop has none to spare -- tests/test_headline_kernel_spills.py)
              const uint32_t* const pixel_mask = kTwoPhase ? AMBER_ARG(cold, pixel_mask) : nullptr;
              if (kTwoPhase && pixel_mask) {
                // the candidates of this pixel's beam, plus the ray's own aperture blade (the self trip decides it exactly), plus
                // every blade when the aperture sample lies on a blade's boundary (only then can a neighbour's exact test see it)
                // (origin_slot is GenerateEyeRay's here, a plain slot below 32: only PathShade sets the flat-self mark, AMBER_FLAT_SELF)
                premask = pixel_mask[plocal] | (origin_slot >= 0 ? 1u << origin_slot : 0u) | (near_edge ? AMBER_ARG(cold, scene.blade_mask) : 0u);
              }
            }
            carries = false;
            casts = 0;
            if (kSig) sig.Reset();
          }
          primary = kTwoPhase && !kLight && AMBER_ARG(AMBER_COLD_OPEN(), pixel_mask) != nullptr;
          AMBER_STAMP(1);
        }
      }
      if (!alive && !retired && pool_count == 0u && exhausted) retired = true;   // queue and pool empty: this lane retires
      if (__ballot(!retired) == 0ull) break;
    }

    rays_wave += static_cast<uint32_t>(__popcll(__ballot(alive)));
    bool emit = false;
    V3 meas = v3(0.f, 0.f, 0.f);
    if (alive) {
      if (!kLight && !kScout && carries) meas = ld3(AMBER_CARRIED());
      // (The lane's path stays in separate locals, handed over one by one: held as one PathRay across the loop, the same instructions come out in
      //  other registers -- EXPERIMENTS.md, device fold -- and the headline instantiations' instruction streams are pinned)
      extras.use_premask = primary; extras.premask = premask;
      if (kLight) {
        const uint32_t plocal = Quotient(a.div_samples, q);
        const typename std::conditional<kPhotons, PhotonSink, SplatSink>::type sink = MakeLightSink<kPhotons>(a, a.path_offset + plocal, a.first_sample + (q - plocal * a.n_samples));
        extras.sink = &sink;
        alive = PathStepOn<PathLightCfg<kEngine, kPhotons>>(sc, lds, o, d, w, meas, rng, casts, origin_slot, extras AMBER_STAMP_ARG);
      } else if (kSig) {
        Bounce b;
        extras.trace = &b;
        alive = PathStepOn<PathSigCfg<kEngine, kCold>>(sc, lds, o, d, w, meas, rng, casts, origin_slot, extras AMBER_STAMP_ARG);
        sig.Add(b);
        if (!alive) AMBER_ARG(AMBER_COLD_OPEN(), sig)[q] = sig.Packed();
      } else if (kScout) {
        extras.scout_bound = &scout_bound;
        alive = PathStepOn<PathScoutCfg<kEngine, kCold>>(sc, lds, o, d, w, meas, rng, casts, origin_slot, extras AMBER_STAMP_ARG);
        // meas: the last hit's own Radiance.  The placeholder is what the record holds until the replay has traced the path with its weight
        emit = !alive && (((__float_as_uint(meas.x) | __float_as_uint(meas.y) | __float_as_uint(meas.z)) != 0u) || scout_bound > amber_scout::kLimit);
        meas = v3(0.f, 0.f, 0.f);
      } else {
        alive = PathStepOn<PathBounceCfg<kEngine, kCold>>(sc, lds, o, d, w, meas, rng, casts, origin_slot, extras AMBER_STAMP_ARG);
      }
      if (!kLight && !kScout) {
        const bool nz = (__float_as_uint(meas.x) | __float_as_uint(meas.y) | __float_as_uint(meas.z)) != 0u;   // anything but +0 (RGB)
        emit = !alive && nz;
        if (alive && nz) { float* c = AMBER_CARRIED(); c[0] = meas.x; c[1] = meas.y; c[2] = meas.z; carries = true; }
      }
    }
    if (!kLight && !kCold) EmitRecords(a, emit, q, meas, rec_next, rec_end);
    if (kCold) {
      EmitRecords([]() {                                      // the record buffers: cold arguments, read when a wave has a record to write (2e-5 of the Cornell paths)
        const ColdArgs cold = ColdArgs::Open();
        return RecordSink{AMBER_COLD(cold, records), AMBER_COLD(cold, flags), AMBER_COLD(cold, touched), AMBER_COLD(cold, rec_count), AMBER_COLD(cold, rec_capacity), AMBER_COLD(cold, div_samples)};
      }, emit, q, meas, rec_next, rec_end);
    }
  }

#undef AMBER_COLD_OPEN
#undef AMBER_ARG
#undef AMBER_CARRIED
  if (!kLight) CloseRecords(a, rec_next, rec_end);
#ifdef AMBER_STAMPS
  if (lane == 0 && a.stamps) for (int k = 0; k < 8; k++) atomicAdd(a.stamps + k, stamp_ctx->acc[k]);
  if (wave_times && lane == 0) wave_times[3] = wall_clock64();
#endif
  // one atomic per wave for the ray counter
  if (lane == 0 && rays_wave) atomicAdd(a.ray_count, static_cast<unsigned long long>(rays_wave));
}

