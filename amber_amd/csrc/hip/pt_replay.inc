// pt_replay.inc -- replay_records_kernel: the second half of a scouted launch (pt_megakernel.inc, AMBER_KERNEL_SCOUT).  Part of the one translation unit
// pt_host.hip; enqueued by LaunchPaths (pt_launch.inc) on the handle's stream between the scout and FinishPathLaunch, inside the launch's event pair.
//
// The scout leaves a placeholder record {q, 0, 0, 0} (and bit q of the bitmap) for every path that ends on a light or is `suspect` (scout_bound.h).  Here ONE
// LANE PER RECORD traces that path again from its number alone -- q -> (band pixel, sample) -> (px, py) by the primary round's own bookkeeping, XorShiftSeed,
// the full GenerateEyeRay, the full PathStep until the path ends, the measurement in registers -- and overwrites the record's rgb.  The device functions and
// their template arguments are those of pt_megakernel<kEngine>, so the sums are the full kernel's to the bit; that a path restarted from (pixel, sample) in a
// per-item kernel reproduces the rendered one is what path_query_kernel and kat_trace_kernel already rest on.  The front end is theirs too (StageEngineLds).
//
// A replayed measurement of (+0, +0, +0) -- the scout's rule is a superset: a light of Radiance -0, a weight that reached 0, a suspect path that stayed finite --
// stays in the buffer as a +0 term.  That is exact: the full kernel has no term there, the reduction's chunk sums start at +0 and add in sample order, the
// pixel's value is +0 or a sum of such sums, neither is ever -0, and x + (+0) = x for every other x, NaN included (reduce_flagged_kernel's own argument for
// leaving the +0 terms OUT, read the other way).  Un-marking the slot would instead need the bit cleared and the pixel's `touched` bit reconsidered.
//
// The loop bound is read once; a launch that ran out of slots is repeated by the host as ever (what is replayed of it is discarded with it).  No atomics, no
// rays counted: the scout has counted every cast of every path.
// pt_megakernel's bounce for this engine, cold family; the stack cap is not that kernel's (no AMBER_PATH_BVH_STACK levels are staged here) but the default
template <int kEngine> struct ReplayBounceCfg : PathBounceCfg<kEngine, true> { static constexpr int kBvhStackCap = AMBER_BVH_STACK; };
template <int kEngine>
__global__ void __launch_bounds__(256) replay_records_kernel(const RenderArgs a) {
  const DevScene& sc = a.scene;
  const EngineLds lds = StageEngineLds<kEngine, 1>(sc);                      // (ends with a barrier: before anything diverges)
  // pt_megakernel's arithmetic family for this engine (its kCold block): the same bits by each switch's own contract, and the same instructions besides
  constexpr bool kDivEye = (AMBER_SHARED_DIV_NORMALIZE & 4) != 0;
  constexpr uint32_t kSqrtMask = ReplayBounceCfg<kEngine>::kSqrtMask;
  const BounceExtras no_extras;
  const uint32_t claimed = *a.rec_count;
  const uint32_t n = claimed < a.rec_capacity ? claimed : a.rec_capacity;
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
    const uint32_t q = a.records[i].x;
    if (q == AMBER_REC_UNUSED) continue;
    const uint32_t plocal = Quotient(a.div_samples, q), sample = a.first_sample + (q - plocal * a.n_samples);
    const uint32_t lrow = Quotient(a.div_width, plocal), px = plocal - lrow * sc.sensor.w;
    const uint32_t py = FrameRow(a.row_begin, a.stripe_rows, a.stripe_period, a.div_stripe_rows, lrow);
    uint64_t rng = XorShiftSeed(a.hashed_seed, px + py * sc.sensor.w, sample);
    V3 o, d;
    float ew;
    int origin_slot = -1;
    GenerateEyeRay<kDivEye, SqrtModeOf(kSqrtMask, 4u)>(sc, px, py, rng, o, d, ew, origin_slot);
    V3 w = v3(ew, ew, ew), meas = v3(0.f, 0.f, 0.f);
    uint32_t casts = 0;
#ifdef AMBER_STAMPS
    StampCtx stamp_store{}; StampCtx* stamp_ctx = &stamp_store;
#endif
    while (PathStepOn<ReplayBounceCfg<kEngine>>(sc, lds, o, d, w, meas, rng, casts, origin_slot, no_extras AMBER_STAMP_ARG)) {}
    a.records[i] = make_uint4(q, __float_as_uint(meas.x), __float_as_uint(meas.y), __float_as_uint(meas.z));
  }
}
