// wavefront.inc -- engine WAVEFRONT: the streaming formulation of the same path tracer (LAB BUILD ONLY; included by pt_host.hip under -DAMBER_LAB).
//
// This is the design the north star sketches: ray state lives in SoA arrays in HBM (coalesced 4-byte-per-lane
// loads and stores), one kernel launch advances every live ray by one bounce, and the survivors are written to the
// next queue compacted with a wave ballot + prefix count (one atomicAdd per wave).  It shares every device function
// (eye ray, closest hit, materials, Russian roulette) and the accumulation order with the work-queue megakernel, so
// its images and ray counts are bit-identical to the other engines; it exists to MEASURE the streaming design on
// this workload (EXPERIMENTS.md, engine WAVEFRONT: HBM traffic 200x higher, lanes always full in the closest-hit phases).
//
// Per batch of <= kWfMaxChunks accumulation chunks:  generate -> { bounce }* -> reduce.
//   path id  pid = (chunk * n_pixels + pixel) * AMBER_ACCUM_CHUNK + j      (j-th sample of the chunk)
//   queues   13 x 4 B per ray: origin, direction, throughput, sampler state (2), pid, casts  = 52 B
//   meas     12 B per path, touched only when a light is hit; reduce sums the samples of a chunk in order.
// One queue head per wave would serialise on a single address (an MI355X L2 atomic unit retires ~88 returning atomics
// per microsecond per address; bounce 0 of config 2 has 1.7e7 waves), so every queue is cut into kWfShards shards
// with their own heads: wave w reads shard w % kWfShards and appends to the SAME shard of the next queue, hence a
// shard never holds more rays than it started with and its capacity is fixed at ceil(n_paths / kWfShards).
#define AMBER_WF_SHARDS 256u

struct WfQueue {
  float* f[9];        // ox oy oz dx dy dz wx wy wz
  uint32_t* u[4];     // rng_lo rng_hi pid casts
};

struct WfArgs {
  DevScene scene;
  WfQueue in, out;
  float* meas;                      // [n_paths][3]
  unsigned int* counts;             // counts[k * AMBER_WF_SHARDS + s] = rays in shard s of the queue consumed by bounce k
  uint32_t shard_capacity;          // rays per shard (multiple of 64)
  unsigned long long* ray_count;
  uint64_t hashed_seed;
  uint32_t row_begin, stripe_rows, stripe_period, n_pixels;
  ExactDiv div_stripe_rows, div_width;   // lrow / stripe_rows (unused when 0), plocal / scene.sensor.w: exact dividers (exact_div.h)
  void SetBand(uint32_t row_begin_, uint32_t stripe_rows_, uint32_t stripe_period_) {    // the fields and their dividers together (as RenderArgs::SetBand; call once `scene` is set)
    row_begin = row_begin_; stripe_rows = stripe_rows_; stripe_period = stripe_period_;
    div_stripe_rows = MakeExactDiv(stripe_rows_); div_width = MakeExactDiv(scene.sensor.w);
  }
  uint32_t first_sample, n_samples; // samples of this batch
  uint32_t n_paths;                 // n_chunks * n_pixels * AMBER_ACCUM_CHUNK
  uint32_t bounce;
};

__global__ void __launch_bounds__(256) wf_generate_kernel(const WfArgs a) {
  const DevScene& sc = a.scene;
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t pid = blockIdx.x * blockDim.x + threadIdx.x; pid < a.n_paths; pid += stride) {
    const uint32_t j = pid & (AMBER_ACCUM_CHUNK - 1u);
    const uint32_t cp = pid / AMBER_ACCUM_CHUNK;
    const uint32_t chunk = cp / a.n_pixels, plocal = cp - chunk * a.n_pixels;
    const uint32_t s_rel = chunk * AMBER_ACCUM_CHUNK + j;
    float* m = a.meas + static_cast<size_t>(pid) * 3u;
    m[0] = 0.f; m[1] = 0.f; m[2] = 0.f;
    const bool live = s_rel < a.n_samples;             // the last chunk may be short
    const PathPlace at = PlacePixel(a, plocal);
    uint64_t rng = PathSeed(a, at, s_rel);
    V3 o = v3(0.f, 0.f, 0.f), d = v3(0.f, 0.f, 1.f); float ew = 0.f; int origin_slot = -1;
    if (live) GenerateEyeRay(sc, at.px, at.py, rng, o, d, ew, origin_slot);
    // compact the live paths into queue 0 (all paths are live except in a short last chunk)
    const unsigned long long mask = __ballot(live);
    const uint32_t n_live = static_cast<uint32_t>(__popcll(mask));
    const uint32_t shard = (pid >> 6) % AMBER_WF_SHARDS;      // wave-uniform (64 consecutive pids per wave trip)
    uint32_t base = 0;
    if ((threadIdx.x & 63u) == 0u && n_live) base = atomicAdd(a.counts + shard, n_live);
    base = __builtin_amdgcn_readfirstlane(base) + shard * a.shard_capacity;
    if (live) {
      const uint32_t k = base + WaveRank(mask);
      a.out.f[0][k] = o.x; a.out.f[1][k] = o.y; a.out.f[2][k] = o.z;
      a.out.f[3][k] = d.x; a.out.f[4][k] = d.y; a.out.f[5][k] = d.z;
      a.out.f[6][k] = ew; a.out.f[7][k] = ew; a.out.f[8][k] = ew;
      a.out.u[0][k] = static_cast<uint32_t>(rng); a.out.u[1][k] = static_cast<uint32_t>(rng >> 32);
      a.out.u[2][k] = pid; a.out.u[3][k] = static_cast<uint32_t>(origin_slot + 1) << 24;   // casts = 0 | (slot+1) << 24
    }
  }
}

template <int kEngine>
__global__ void __launch_bounds__(256) wf_bounce_kernel(const WfArgs a) {
  const DevScene& sc = a.scene;
  const EngineLds lds = StageEngineLds<kEngine, AMBER_BVH_STACK>(sc);
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;          // global wave id
  const uint32_t n_waves = (gridDim.x * blockDim.x) >> 6;                       // multiple of AMBER_WF_SHARDS
  const uint32_t shard = wave % AMBER_WF_SHARDS, wq = wave / AMBER_WF_SHARDS, waves_per_shard = n_waves / AMBER_WF_SHARDS;
  const uint32_t n_in = a.counts[a.bounce * AMBER_WF_SHARDS + shard];
  unsigned int* out_count = a.counts + (a.bounce + 1) * AMBER_WF_SHARDS + shard;
  const uint32_t shard_base = shard * a.shard_capacity;
  uint32_t rays = 0;
  // every lane of a wave runs the same number of trips (the closest-hit loops are wave-uniform)
  for (uint32_t base_k = wq * 64u; base_k < n_in; base_k += waves_per_shard * 64u) {
    const uint32_t k = base_k + lane;
    bool alive = k < n_in;
    const uint32_t kk = shard_base + (alive ? k : n_in - 1u);
    PathRay ray;
    ray.o = v3(a.in.f[0][kk], a.in.f[1][kk], a.in.f[2][kk]);
    ray.d = v3(a.in.f[3][kk], a.in.f[4][kk], a.in.f[5][kk]);
    ray.w = v3(a.in.f[6][kk], a.in.f[7][kk], a.in.f[8][kk]);
    ray.rng = static_cast<uint64_t>(a.in.u[0][kk]) | (static_cast<uint64_t>(a.in.u[1][kk]) << 32);
    const uint32_t pid = a.in.u[2][kk];
    ray.casts = a.in.u[3][kk] & 0x00ffffffu;
    ray.origin_slot = static_cast<int>(a.in.u[3][kk] >> 24) - 1;
    if (alive) {
      V3& meas = ray.meas;
      meas = v3(0.f, 0.f, 0.f);
#ifdef AMBER_STAMPS
      StampCtx stamp_store{}; StampCtx* stamp_ctx = &stamp_store;
#endif
      alive = PathStep<BounceCfg<kEngine>>(sc, lds, ray, BounceExtras{} AMBER_STAMP_ARG);
      ++rays;
      // measurement += weight * Le : non-zero only when a light was hit; x + (+-0) == x, so skipping zeros is exact
      if (__float_as_uint(meas.x) << 1 || __float_as_uint(meas.y) << 1 || __float_as_uint(meas.z) << 1) {
        float* m = a.meas + static_cast<size_t>(pid) * 3u;
        m[0] = m[0] + meas.x; m[1] = m[1] + meas.y; m[2] = m[2] + meas.z;
      }
    }
    const unsigned long long mask = __ballot(alive);
    const uint32_t n_live = static_cast<uint32_t>(__popcll(mask));
    uint32_t base = 0;
    if (lane == 0u && n_live) base = atomicAdd(out_count, n_live);
    base = __builtin_amdgcn_readfirstlane(base) + shard_base;
    if (alive) {
      const uint32_t q = base + WaveRank(mask);
      a.out.f[0][q] = ray.o.x; a.out.f[1][q] = ray.o.y; a.out.f[2][q] = ray.o.z;
      a.out.f[3][q] = ray.d.x; a.out.f[4][q] = ray.d.y; a.out.f[5][q] = ray.d.z;
      a.out.f[6][q] = ray.w.x; a.out.f[7][q] = ray.w.y; a.out.f[8][q] = ray.w.z;
      a.out.u[0][q] = static_cast<uint32_t>(ray.rng); a.out.u[1][q] = static_cast<uint32_t>(ray.rng >> 32);
      a.out.u[2][q] = pid; a.out.u[3][q] = ray.casts | (static_cast<uint32_t>(ray.origin_slot + 1) << 24);
    }
  }
  unsigned long long r = rays;
  for (int off = 32; off > 0; off >>= 1) r += __shfl_down(r, off, 64);
  if (lane == 0 && r) atomicAdd(a.ray_count, r);
}

// fb[pixel] += sum_j meas[(chunk*n_pixels + pixel)*32 + j] (j in sample order), chunks in order
__global__ void wf_reduce_kernel(float* __restrict__ fb, const float* __restrict__ meas, uint32_t n_pixels, uint32_t n_chunks) {
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;          // pixel*3 + channel
  if (e >= n_pixels * 3u) return;
  const uint32_t pixel = e / 3u, c = e - pixel * 3u;
  float v = fb[e];
  for (uint32_t chunk = 0; chunk < n_chunks; ++chunk) {
    const float* m = meas + (static_cast<size_t>(chunk) * n_pixels + pixel) * AMBER_ACCUM_CHUNK * 3u + c;
    float s = 0.f;
    for (uint32_t j = 0; j < AMBER_ACCUM_CHUNK; ++j) s = s + m[j * 3u];   // short chunks: the tail entries are zero
    v = v + s;
  }
  fb[e] = v;
}
