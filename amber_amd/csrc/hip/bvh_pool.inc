// bvh_pool.inc -- pt_bvh_pool_kernel: engine BVH's path-tracing worker (LAB BUILD ONLY; included by pt_host.hip under -DAMBER_LAB).
//
// Round 2's worker (pt_bvh_megakernel, still used for light tracing) bound one ray to a lane until its shading: a lane
// whose traversal had finished waited until 52 lanes of the wave had -- 27 % of all lane time on the 1M-sphere scene,
// and every traversal trip of the wave ran with the 38 lanes that were still traversing (profiles/r02e_config3_counters.txt).
// Here a wave owns 64 + kWait rays:
//   * 64 are IN FLIGHT, one per lane, traversal state in registers (BvhTrav, the ray, the best hit);
//   * kWait WAIT in LDS entries, each either READY (ray + slab operands, computed when the ray was made) or DONE (ray +
//     hit).  A lane whose traversal finishes swaps with a READY entry in place -- its finished ray goes into the entry,
//     the waiting one onto the lane -- so the lanes keep traversing.  Only when no READY entry is left does a lane HOLD
//     its finished ray in registers.
//   * Shading runs as a wave-level pass once DONE entries + holding lanes reach AMBER_BVH_POOL_SHADE: holding lanes shade
//     their own ray, the other lanes take DONE entries (their own traversal stays in their registers); a path that ended
//     is replaced by the next path of the queue in the same pass; the continued / new ray gets its slab operands (all
//     participating lanes at once) and becomes READY again, or goes straight back in flight on a holding lane.
//   * Everything of a path that traversal does not need -- throughput, sampler state, path index, cast count: 7 dwords --
//     stays in LDS for all 64 + kWait rays, indexed by a ray id that travels with the ray.
//   * The per-lane traversal stack keeps AMBER_BVH_POOL_STACK levels in LDS ([level][lane]) and the rest in global memory
//     (BvhStackHybrid): 2 KB per wave instead of 6, which is what pays for the pool.
// LDS per wave (kWait 32, 8 stack levels): 2048 stack + 96 x 32 path state + 32 x 80 entries + 2 x 128 queues = 7936 B,
// 31 KB per workgroup: 5 workgroups per CU as before.
// The measurement of a path is not carried between bounces: emitted radiance is non-zero only on a DiffuseLight, whose
// scatter weight 0 ends the path, so before its last bounce a path's measurement is +0 -- unless a weight has become
// inf or NaN (inf * 0), which degenerate scenes produce; such a path parks its measurement in global memory (`carried`)
// and sets a flag, and stays bit-exact.
// Results do not depend on any of this scheduling: paths are independent, and sums are formed by path index afterwards.
#ifndef AMBER_BVH_POOL_WGS
#define AMBER_BVH_POOL_WGS 5
#endif
#ifndef AMBER_BVH_POOL_WAIT
#define AMBER_BVH_POOL_WAIT 24          // waiting rays per wave (a multiple of 4, <= 64)
#endif
#ifndef AMBER_BVH_POOL_STACK
#define AMBER_BVH_POOL_STACK 12         // traversal-stack levels kept in LDS
#endif
#ifndef AMBER_BVH_POOL_SHADE
#define AMBER_BVH_POOL_SHADE 48         // shade when DONE entries + holding lanes reach this
#endif
// Paths a wave claims with one atomicAdd.  A claim is ~650 rays, ~0.4 ms of one wave on the 1M-sphere scene: the tail it
// can leave; 5e8 paths / 256 = 2e6 atomics per launch = 12 per microsecond (the L2 retires ~88 on one address).
#define AMBER_BVH_CLAIM_PATHS 256u
#ifndef AMBER_BVH_POOL_SWAP_MIN
#define AMBER_BVH_POOL_SWAP_MIN 1       // lanes that must be waiting for a ray before a swap step runs
#endif

template <bool kSig> struct BvhPoolLayout {
  static constexpr int kWait = AMBER_BVH_POOL_WAIT;
  static constexpr int kRays = 64 + kWait;
  static constexpr int kPathQ = kSig ? 3 : 2;                       // uint4 per path-state record
  static constexpr int kStackWords = AMBER_BVH_POOL_STACK * 64;
  static constexpr int kPathWords = kRays * kPathQ * 4;
  static constexpr int kEntryWords = kWait * 20;                     // 5 uint4 per entry
  static constexpr int kQueueWords = 2 * kWait;
  static constexpr int kWaveWords = kStackWords + kPathWords + kEntryWords + kQueueWords;
  static_assert(kWait >= 4 && kWait <= 64 && kWait % 4 == 0, "AMBER_BVH_POOL_WAIT must be a multiple of 4 in [4, 64]");
  static_assert(kWaveWords % 4 == 0, "every wave's LDS block must stay 16-byte aligned");
};
// ints of global traversal stack per thread of the grid, and floats of carried measurements per wave
#define AMBER_BVH_POOL_GLOBAL_LEVELS (AMBER_BVH_STACK - AMBER_BVH_POOL_STACK)
#define AMBER_BVH_POOL_CARRIED_PER_WAVE ((64 + AMBER_BVH_POOL_WAIT) * 3)

enum : uint32_t { LS_IDLE = 0u, LS_TRAV = 1u, LS_FIN = 2u, LS_HOLD = 3u, LS_FRESH = 4u };

template <bool kSig>
__global__ void __launch_bounds__(256, kSig ? 2 : AMBER_BVH_POOL_WGS) pt_bvh_pool_kernel(const RenderArgs a) {
  using L = BvhPoolLayout<kSig>;
  constexpr uint32_t kWait = L::kWait, kPathQ = L::kPathQ;
  const DevScene& sc = a.scene;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);        // the compiler must KNOW it is wave-uniform: every pointer below stays in SGPRs
  __shared__ uint4 lds_all[L::kWaveWords];                          // 4 waves x kWaveWords dwords
  uint32_t* wbase = reinterpret_cast<uint32_t*>(lds_all) + wave * L::kWaveWords;
  const BvhStackHybrid stack{(LdsInts)(reinterpret_cast<int32_t*>(wbase)), (GlobalInts)(a.bvh_stack + (blockIdx.x * 256u + wave * 64u)), gridDim.x * 256u,
                             AMBER_BVH_POOL_STACK, AMBER_BVH_STACK};
  uint4* path = reinterpret_cast<uint4*>(wbase + L::kStackWords);                                     // [ray id][kPathQ]
  uint4* entry = reinterpret_cast<uint4*>(wbase + L::kStackWords + L::kPathWords);                    // [entry][5]
  uint32_t* ready_q = wbase + L::kStackWords + L::kPathWords + L::kEntryWords;                        // rings of entry ids
  uint32_t* done_q = ready_q + kWait;
  float* carried = a.carried + static_cast<size_t>(blockIdx.x * 4u + wave) * AMBER_BVH_POOL_CARRIED_PER_WAVE;

  // wave-uniform (SGPRs)
  uint32_t rhead = 0, rcount = 0, dhead = 0, dcount = 0;            // READY / DONE rings
  uint32_t n_unfilled = kWait;                                      // entries that have not received their first ray yet
  WaveClaim claim;                                                  // paths claimed from the queue, not yet handed to a lane
  uint32_t rec_next = 0, rec_end = 0, rays_wave = 0;
  // per lane: the ray in flight (or held)
  uint32_t st = LS_FRESH, r = lane;
  V3 o = v3(0.f, 0.f, 0.f), d = v3(0.f, 0.f, 1.f);
  BvhTrav tr; HitRec hit;
  BvhIdle(tr, hit);
#ifdef AMBER_STAMPS
  StampCtx stamp_store{}, stamp_shade{}; StampCtx* stamp_ctx = &stamp_store;      // counters here; PathShade's clocks go to a dummy
#define AMBER_POOL_SHADE_STAMP_ARG , &stamp_shade
  stamp_ctx->last = __builtin_amdgcn_s_memtime();
#else
#define AMBER_POOL_SHADE_STAMP_ARG
#endif
#define AMBER_WRAP(x_) ((x_) >= kWait ? (x_) - kWait : (x_))     /* ring index; x_ < 2 kWait */
#define AMBER_F2U(x_) __float_as_uint(x_)
#define AMBER_U2F(x_) __uint_as_float(x_)

  for (;;) {
    // ---- A. lanes whose traversal has just finished, and lanes without a ray, take READY entries ---------------------
    {
      const bool fin = st == LS_FIN;
      const bool want = fin || st == LS_IDLE;
      const unsigned long long m = __ballot(want);
      if (static_cast<uint32_t>(__popcll(m)) >= AMBER_BVH_POOL_SWAP_MIN && rcount != 0u) {   // wave-uniform
        const uint32_t rank = WaveRank(m), n_want = static_cast<uint32_t>(__popcll(m));
        const uint32_t take = n_want < rcount ? n_want : rcount;
        const bool got = want && rank < take;
        uint32_t e = 0;
        if (got) {
          AMBER_COUNT_LEAVES(3);
          e = ready_q[AMBER_WRAP(rhead + rank)];
          const uint4 c0 = entry[e * 5u], c1 = entry[e * 5u + 1u], c2 = entry[e * 5u + 2u], c3 = entry[e * 5u + 3u], c4 = entry[e * 5u + 4u];
          if (fin) {                                                  // the finished ray takes the waiting one's place
            entry[e * 5u] = make_uint4(AMBER_F2U(o.x), AMBER_F2U(o.y), AMBER_F2U(o.z), AMBER_F2U(d.x));
            entry[e * 5u + 1u] = make_uint4(AMBER_F2U(d.y), AMBER_F2U(d.z), r, static_cast<uint32_t>(hit.slot));
            entry[e * 5u + 2u] = make_uint4(AMBER_F2U(hit.t), AMBER_F2U(hit.u), AMBER_F2U(hit.v), static_cast<uint32_t>(hit.idx));
          }
          o = v3(AMBER_U2F(c0.x), AMBER_U2F(c0.y), AMBER_U2F(c0.z));
          d = v3(AMBER_U2F(c0.w), AMBER_U2F(c1.x), AMBER_U2F(c1.y));
          r = c1.z;
          const uint32_t fl = c1.w;                                   // bits 0..2: rot per axis; bit 3: NaN ray (nothing to traverse)
          tr.A = v3(AMBER_U2F(c2.x), AMBER_U2F(c2.y), AMBER_U2F(c2.z)); tr.neg_slack = AMBER_U2F(c2.w);
          tr.b_in = v3(AMBER_U2F(c3.x), AMBER_U2F(c3.y), AMBER_U2F(c3.z));
          tr.b_out = v3(AMBER_U2F(c3.w), AMBER_U2F(c4.x), AMBER_U2F(c4.y));
          tr.rot[0] = (fl & 1u) ? 16u : 0u; tr.rot[1] = (fl & 2u) ? 16u : 0u; tr.rot[2] = (fl & 4u) ? 16u : 0u;
          tr.cur = (fl & 8u) ? AMBER_BVH_DONE : sc.bvh_root; tr.pend = 0; tr.sp = 0; tr.overflow = false;
          hit.t = 3.402823466e+38f; hit.u = 0.f; hit.v = 0.f; hit.idx = -1; hit.slot = -1;
          st = LS_TRAV;
        }
        const bool swapped = got && fin;
        const unsigned long long ms = __ballot(swapped);
        if (ms != 0ull) {
          const uint32_t rk = WaveRank(ms);
          if (swapped) done_q[AMBER_WRAP(AMBER_WRAP(dhead + dcount) + rk)] = e;
          dcount += static_cast<uint32_t>(__popcll(ms));
        }
        rhead = AMBER_WRAP(rhead + take); rcount -= take;
      }
      if (st == LS_FIN) st = LS_HOLD;                                 // nothing was waiting: the lane keeps its finished ray
    }
    __builtin_amdgcn_wave_barrier();                                  // (compiler fence; one wave's LDS instructions execute in order)

    // ---- B. shading pass ---------------------------------------------------------------------------------------------
    const unsigned long long m_hold = __ballot(st == LS_HOLD), m_fresh = __ballot(st == LS_FRESH), m_trav = __ballot(st == LS_TRAV);
    if (m_trav == 0ull && m_hold == 0ull && m_fresh == 0ull && dcount == 0u && rcount == 0u) break;
    const uint32_t n_hold = static_cast<uint32_t>(__popcll(m_hold));
    const bool fill = n_unfilled != 0u && !claim.exhausted && (m_hold | m_fresh) != ~0ull;
    if (m_fresh != 0ull || n_hold + dcount >= AMBER_BVH_POOL_SHADE || (m_trav == 0ull && n_hold + dcount != 0u) || fill) {
      AMBER_CLK(0);
      const bool hold = st == LS_HOLD, fresh = st == LS_FRESH;
      const bool free_lane = !hold && !fresh;
      const unsigned long long mf = __ballot(free_lane);
      const uint32_t rank_free = WaveRank(mf), n_free = static_cast<uint32_t>(__popcll(mf));
      const uint32_t n_take = dcount < n_free ? dcount : n_free;
      uint32_t n_fill = 0;
      if (!claim.exhausted) { n_fill = n_free - n_take; if (n_fill > n_unfilled) n_fill = n_unfilled; }
      const bool lds_shade = free_lane && rank_free < n_take;
      const bool filler = free_lane && !lds_shade && rank_free < n_take + n_fill;
      uint32_t e = 0, sr = r;
      V3 so = o, sd = d;
      HitRec sh = hit;
      if (lds_shade) {
        e = done_q[AMBER_WRAP(dhead + rank_free)];
        const uint4 c0 = entry[e * 5u], c1 = entry[e * 5u + 1u], c2 = entry[e * 5u + 2u];
        so = v3(AMBER_U2F(c0.x), AMBER_U2F(c0.y), AMBER_U2F(c0.z));
        sd = v3(AMBER_U2F(c0.w), AMBER_U2F(c1.x), AMBER_U2F(c1.y));
        sr = c1.z;
        sh.slot = static_cast<int>(c1.w); sh.t = AMBER_U2F(c2.x); sh.u = AMBER_U2F(c2.y); sh.v = AMBER_U2F(c2.z); sh.idx = static_cast<int>(c2.w);
      } else if (filler) {
        e = kWait - n_unfilled + (rank_free - n_take);
        sr = 64u + e;                                                 // ray ids 64.. belong to the entries at the start
      }
      dhead = AMBER_WRAP(dhead + n_take); dcount -= n_take; n_unfilled -= n_fill;

      const bool shading = hold || lds_shade;
      rays_wave += static_cast<uint32_t>(__popcll(__ballot(shading)));
      V3 sw = v3(0.f, 0.f, 0.f), meas = v3(0.f, 0.f, 0.f);
      uint64_t srng = 1;
      uint32_t sq = 0, scasts = 0, sflags = 0;
      PathSig sg; sg.Reset();
      bool have = false, emit = false;
      if (shading) {
        AMBER_COUNT_ROUNDS(3);
        const uint4 p0 = path[sr * kPathQ], p1 = path[sr * kPathQ + 1u];
        sw = v3(AMBER_U2F(p0.x), AMBER_U2F(p0.y), AMBER_U2F(p0.z)); scasts = p0.w;
        srng = static_cast<uint64_t>(p1.x) | (static_cast<uint64_t>(p1.y) << 32); sq = p1.z; sflags = p1.w;
        if (kSig) { const uint4 p2 = path[sr * kPathQ + (kPathQ - 1u)]; sg.obj = p2.x; sg.t = p2.y; }
        if (sflags & 1u) meas = ld3(carried + sr * 3u);               // degenerate paths only (see the file comment)
        PathRay ray{so, sd, sw, meas, srng, scasts, -1};
        if (kSig) {
          Bounce b;
          BounceExtras extras; extras.trace = &b;
          have = PathShade<TracedBounceCfg<ENGINE_BVH>>(sc, nullptr, sh, ray, extras AMBER_POOL_SHADE_STAMP_ARG);
          sg.Add(b);
          if (!have) a.sig[sq] = sg.Packed();
        } else {
          have = PathShade<BounceCfg<ENGINE_BVH>>(sc, nullptr, sh, ray, BounceExtras{} AMBER_POOL_SHADE_STAMP_ARG);
        }
        so = ray.o; sd = ray.d; sw = ray.w; meas = ray.meas; srng = ray.rng; scasts = ray.casts;
        const bool nz = (AMBER_F2U(meas.x) | AMBER_F2U(meas.y) | AMBER_F2U(meas.z)) != 0u;   // anything but +0 (RGB)
        emit = !have && nz;
        if (have && nz) { carried[sr * 3u] = meas.x; carried[sr * 3u + 1u] = meas.y; carried[sr * 3u + 2u] = meas.z; sflags |= 1u; }
      }
      EmitRecords(a, emit, sq, meas, rec_next, rec_end);

      // the next paths of the queue for the lanes whose path ended, the lanes that start, and the entries to fill
      const bool want_path = (shading && !have) || fresh || filler;
      if (ServeLanes<AMBER_BVH_CLAIM_PATHS>(claim, a.next_item, a.n_items, lane, want_path, sq)) {                                                 // algorithm_pt.cc:125-136: the path's sampler and eye ray
        const PathPlace at = PlacePath(a, sq);
        srng = PathSeed(a, at, at.k);
        float ew; int os;
        GenerateEyeRay(sc, at.px, at.py, srng, so, sd, ew, os);
        sw = v3(ew, ew, ew);                                          // Leading<RGB>(.., Radiant(weight)) lens_basic.h:139-144
        scasts = 0; sflags = 0; sg.Reset();
        have = true;
      }
      if (have) {                                                     // slab operands of the ray that will be traversed next
        BvhTrav nt; HitRec nh;
        BvhBegin(sc, so, sd, nt, nh);
        path[sr * kPathQ] = make_uint4(AMBER_F2U(sw.x), AMBER_F2U(sw.y), AMBER_F2U(sw.z), scasts);
        path[sr * kPathQ + 1u] = make_uint4(static_cast<uint32_t>(srng), static_cast<uint32_t>(srng >> 32), sq, sflags);
        if (kSig) path[sr * kPathQ + (kPathQ - 1u)] = make_uint4(sg.obj, sg.t, 0u, 0u);
        if (free_lane) {                                              // it waits in the entry; this lane's own traversal goes on
          const uint32_t fl = (nt.rot[0] ? 1u : 0u) | (nt.rot[1] ? 2u : 0u) | (nt.rot[2] ? 4u : 0u) | (nt.cur == AMBER_BVH_DONE ? 8u : 0u);
          entry[e * 5u] = make_uint4(AMBER_F2U(so.x), AMBER_F2U(so.y), AMBER_F2U(so.z), AMBER_F2U(sd.x));
          entry[e * 5u + 1u] = make_uint4(AMBER_F2U(sd.y), AMBER_F2U(sd.z), sr, fl);
          entry[e * 5u + 2u] = make_uint4(AMBER_F2U(nt.A.x), AMBER_F2U(nt.A.y), AMBER_F2U(nt.A.z), AMBER_F2U(nt.neg_slack));
          entry[e * 5u + 3u] = make_uint4(AMBER_F2U(nt.b_in.x), AMBER_F2U(nt.b_in.y), AMBER_F2U(nt.b_in.z), AMBER_F2U(nt.b_out.x));
          entry[e * 5u + 4u] = make_uint4(AMBER_F2U(nt.b_out.y), AMBER_F2U(nt.b_out.z), 0u, 0u);
        } else {                                                      // a holding / starting lane: straight back in flight
          o = so; d = sd; tr = nt; hit = nh; r = sr; st = LS_TRAV;
        }
      } else if (!free_lane) {
        st = LS_IDLE;                                                 // the queue is empty: this lane has no ray any more
      }
      const bool pushes = have && free_lane;
      const unsigned long long mp = __ballot(pushes);
      if (mp != 0ull) {
        const uint32_t rk = WaveRank(mp);
        if (pushes) ready_q[AMBER_WRAP(AMBER_WRAP(rhead + rcount) + rk)] = e;
        rcount += static_cast<uint32_t>(__popcll(mp));
      }
      __builtin_amdgcn_wave_barrier();
      AMBER_CLK(5);
      continue;                                                       // step A first: idle lanes may take what has just become READY
    }

    // ---- C. one traversal round of the lanes in flight ----------------------------------------------------------------
    AMBER_CLK(6);
    if (st == LS_TRAV) {
      AMBER_COUNT_ROUNDS(2);
      const bool more = BvhRoundOn(sc, stack, o, d, tr, hit AMBER_STAMP_ARG);
      if (!more) {
        if (tr.overflow) ClosestHitLeafList(sc, o, d, hit);
        if (kSig) BvhResolveIndex(sc, hit);                         // only the signature variant reports object indices
        st = LS_FIN;
      }
    }
    AMBER_CLK(1);
  }

  CloseRecords(a, rec_next, rec_end);
#undef AMBER_POOL_SHADE_STAMP_ARG
#undef AMBER_WRAP
#undef AMBER_F2U
#undef AMBER_U2F
#ifdef AMBER_STAMPS
#ifdef AMBER_BVH_CLOCKS
  if (a.stamps) for (int k = 0; k < 8; k++) atomicAdd(a.stamps + k, stamp_ctx->acc[k] >> 6);      // lane-time / 64
#else
  if (a.stamps) for (int k = 0; k < 8; k++) if (stamp_ctx->acc[k]) atomicAdd(a.stamps + k, stamp_ctx->acc[k]);
#endif
#endif
  if (lane == 0u && rays_wave) atomicAdd(a.ray_count, static_cast<unsigned long long>(rays_wave));
}
