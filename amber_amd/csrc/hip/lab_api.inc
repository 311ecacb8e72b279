// lab_api.inc -- LAB BUILD ONLY (-DAMBER_LAB, libamber_hip_lab.so): host side of the streaming engine and the known-answer / signature entry points (include/amber_hip_lab.h).
// Part of the one translation unit pt_host.hip (kernels are launched from there); see its header comment.

namespace {
// The known-answer kernels' engines: those of the render kernels but REFERENCE_BVH, which the kat_* entry points refuse first
constexpr const char* kKatNoRefBvh = "the known-answer kernels have no instantiation for AMBER_ENGINE_REFERENCE_BVH (its traversal stack belongs to the render kernels' grid): compare amber_hip_pt_signatures instead";
template <typename F>
void WithKatEngine(const amber_hip_pt* h, F&& f) {
  WithHitEngine(h->hit_engine, [&](auto engine) -> int { if constexpr (decltype(engine)::value != ENGINE_REF_BVH) f(engine); return AMBER_OK; });
}

// Engine WAVEFRONT host loop: batches of <= max_chunks accumulation chunks; per batch generate, then bounce launches
// until the live-ray count read back from the device is zero, then the ordered reduction into the framebuffer.
int RenderPassWavefront(amber_hip_pt* h, uint32_t first_sample, uint32_t n_samples) {
  const uint32_t n_pixels = static_cast<uint32_t>(BandPixels(h));
  const uint64_t kMaxPaths = 1ull << 28;                       // 268 M paths: 2 x 14 GB of queues + 3.2 GB of measurements
  uint64_t max_chunks = kMaxPaths / (static_cast<uint64_t>(n_pixels) * AMBER_ACCUM_CHUNK);
  if (max_chunks == 0) return Fail(AMBER_EINVAL, "band too large for the wavefront engine");
  const uint32_t kMaxBounces = 4096;
  const uint64_t cap = max_chunks * AMBER_ACCUM_CHUNK;
  return SplitSamples(first_sample, n_samples, "band too large for the wavefront engine", [&](uint32_t left, amber_plan::Launch* l) -> int {
    *l = {left > cap ? static_cast<uint32_t>(cap) : left, 0};
    return AMBER_OK;
  }, [&](uint32_t first, const amber_plan::Launch& l, bool*) -> int {
    const uint32_t n = l.n;
    const uint32_t n_chunks = (n + AMBER_ACCUM_CHUNK - 1) / AMBER_ACCUM_CHUNK;
    const size_t n_paths = static_cast<size_t>(n_chunks) * n_pixels * AMBER_ACCUM_CHUNK;
    // every queue array holds AMBER_WF_SHARDS shards of shard_capacity rays
    const size_t shard_capacity = ((n_paths + AMBER_WF_SHARDS - 1) / AMBER_WF_SHARDS + 63) / 64 * 64 + 64;
    const size_t q_len = shard_capacity * AMBER_WF_SHARDS;
    const size_t n_counts = static_cast<size_t>(kMaxBounces + 2) * AMBER_WF_SHARDS;
    const size_t bytes = (26 * q_len + 3 * n_paths) * 4 + n_counts * sizeof(unsigned int);
    AMBER_TRY(Grow(h, h->d_wf, bytes / sizeof(float), "wavefront queues"));
    float* base = h->d_wf;
    WfQueue q[2];
    for (int k = 0; k < 2; k++) {
      for (int c = 0; c < 9; c++) q[k].f[c] = base + (static_cast<size_t>(k) * 13 + c) * q_len;
      for (int c = 0; c < 4; c++) q[k].u[c] = reinterpret_cast<uint32_t*>(base + (static_cast<size_t>(k) * 13 + 9 + c) * q_len);
    }
    float* meas = base + 26 * q_len;
    unsigned int* counts = reinterpret_cast<unsigned int*>(meas + 3 * n_paths);
    HIP_TRY(hipMemsetAsync(counts, 0, n_counts * sizeof(unsigned int), h->stream));
    WfArgs a;
    a.scene = h->scene; a.meas = meas; a.counts = counts; a.ray_count = h->d_rays; a.hashed_seed = h->hashed_seed;
    a.SetBand(h->row_begin, h->stripe_rows, h->stripe_period); a.n_pixels = n_pixels;
    a.first_sample = first; a.n_samples = n; a.n_paths = static_cast<uint32_t>(n_paths); a.bounce = 0; a.shard_capacity = static_cast<uint32_t>(shard_capacity);
    const uint32_t n_blocks = 2048u;                          // 8192 waves = 32 per shard
    AMBER_TRY(TimedLaunch(h, true, [&]() -> int {
      a.out = q[0]; a.in = q[1];
      hipLaunchKernelGGL(wf_generate_kernel, dim3(n_blocks), dim3(256), 0, h->stream, a);
      HIP_TRY(hipGetLastError());
      uint32_t bounce = 0;
      for (;;) {
        const uint32_t burst = bounce < 16 ? 8 : 16;            // launches enqueued before the live count is read back
        for (uint32_t k = 0; k < burst && bounce < kMaxBounces; k++, bounce++) {
          a.bounce = bounce; a.in = q[bounce & 1]; a.out = q[(bounce + 1) & 1];
          WithHitEngine(h->hit_engine, [&](auto engine) -> int {          // instantiated for TWO_PHASE and BVH (the engines WAVEFRONT resolves to), else LIST
            constexpr int kEngine = decltype(engine)::value == ENGINE_TWO_PHASE || decltype(engine)::value == ENGINE_BVH ? decltype(engine)::value : ENGINE_LIST;
            hipLaunchKernelGGL(wf_bounce_kernel<kEngine>, dim3(n_blocks), dim3(256), 0, h->stream, a);
            return AMBER_OK;
          });
          HIP_TRY(hipGetLastError());
        }
        unsigned int shard_live[AMBER_WF_SHARDS];
        HIP_TRY(hipMemcpyAsync(shard_live, counts + static_cast<size_t>(bounce) * AMBER_WF_SHARDS, sizeof shard_live, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        unsigned long long live = 0;
        for (unsigned int v : shard_live) live += v;
        if (live == 0) break;
        if (bounce >= kMaxBounces) return Fail(AMBER_EHIP, "wavefront engine: path longer than 4096 bounces");
      }
      return AMBER_OK;
    }));
    const uint32_t n_elems = n_pixels * 3u;
    hipLaunchKernelGGL(wf_reduce_kernel, dim3((n_elems + 255u) / 256u), dim3(256), 0, h->stream, h->d_fb, meas, n_pixels, n_chunks);
    HIP_TRY(hipGetLastError());
    return AMBER_OK;
  });
}

// One path launch over n samples of the band whose records come from kat_accumulate_kernel (amber_hip_kat_accumulate): LaunchPaths with the other
// producer.  ResolvePending repeats it from here when it ran out of slots.
int LaunchLabRecords(amber_hip_pt* h, uint32_t n, uint32_t n_pixels, float* target, const RecordProducer& producer) {
  AMBER_TRY(BeginPathLaunch(h, n, n_pixels, false));
  RenderArgs a = MakeRenderArgs(h, h->hashed_seed, n_pixels, 0u, n);
  SetRecordArgs(h, a);
  a.n_items = n_pixels * n;
  AMBER_TRY(TimedLaunch(h, false, [&]() -> int {
    hipLaunchKernelGGL(kat_accumulate_kernel, dim3((producer.n_waves + 3u) / 4u), dim3(256), 0, h->stream, a, producer.q, producer.rgb, producer.n_items,
                       producer.n_waves, producer.rays);
    return AMBER_OK;
  }));
  return FinishPathLaunch(h, 0u, n, n_pixels, target, producer, false);
}

// The stage hooks (amber_hip_kat_*_stage_ms): the first call switches the stage's clock on; every call reports the sums of the clock's intervals
// since the call before (a null pointer: not asked for, or not a stage) and zeroes them.
template <int kN>
int StageMs(const char* name, amber_hip_pt* h, StageClock<kN>* clock, double* const (&out)[kN - 1]) { return Guarded(name, [&]() -> int {
  if (!h) return Fail(AMBER_EINVAL, "null handle");
  clock->on = true;
  for (int i = 0; i < kN - 1; i++) { if (out[i]) *out[i] = clock->ms[i]; clock->ms[i] = 0; }
  return AMBER_OK;
}); }

}  // namespace

extern "C" {

// ---- KAT entry points -----------------------------------------------------------------------------
int amber_hip_kat_cast(amber_hip_pt* h, uint32_t n, const float* origins, const float* dirs,
                       int32_t* out_object, float* out_t, float* out_pos, float* out_normal) { return Guarded("amber_hip_kat_cast", [&]() -> int {
  if (h && h->hit_engine == AMBER_ENGINE_REFERENCE_BVH) return Fail(AMBER_EINVAL, kKatNoRefBvh);
  if (!h || !origins || !dirs || !out_object || !out_t || !out_pos || !out_normal) return Fail(AMBER_EINVAL, "null argument");
  if (n == 0) return AMBER_OK;
  HIP_TRY(hipSetDevice(h->device));
  DevBuf<float> d_o, d_d, d_t, d_p, d_n; DevBuf<int32_t> d_i;
  HIP_TRY(d_o.alloc(3 * n)); HIP_TRY(d_d.alloc(3 * n)); HIP_TRY(d_t.alloc(n)); HIP_TRY(d_p.alloc(3 * n)); HIP_TRY(d_n.alloc(3 * n)); HIP_TRY(d_i.alloc(n));
  HIP_TRY(hipMemcpy(d_o.p, origins, 3ull * n * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_d.p, dirs, 3ull * n * 4, hipMemcpyHostToDevice));
  WithKatEngine(h, [&](auto engine) { hipLaunchKernelGGL(kat_cast_kernel<decltype(engine)::value>, dim3((n + 255) / 256), dim3(256), 0, h->stream, h->scene, n, d_o.p, d_d.p, d_i.p, d_t.p, d_p.p, d_n.p); });
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipMemcpy(out_object, d_i.p, 4ull * n, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(out_t, d_t.p, 4ull * n, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(out_pos, d_p.p, 12ull * n, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(out_normal, d_n.p, 12ull * n, hipMemcpyDeviceToHost));
  return AMBER_OK;
}); }

int amber_hip_kat_phase_a(amber_hip_pt* h, uint32_t n, const float* origins, const float* dirs, int axis_loops, uint32_t* out_mask, uint64_t mask_capacity, uint32_t* out_n_groups) { return Guarded("amber_hip_kat_phase_a", [&]() -> int {
  if (!h || !origins || !dirs || !out_mask) return Fail(AMBER_EINVAL, "null argument");
  if (!h->two_phase) return Fail(AMBER_EINVAL, "amber_hip_kat_phase_a: the handle's engine has no Phase A (two-phase engines only)");
  const uint32_t n_groups = h->hit_engine == kHitTwoPhaseN ? h->scene.n_groups : 1u;
  if (out_n_groups) *out_n_groups = n_groups;
  if (static_cast<uint64_t>(n) * n_groups > mask_capacity) return Fail(AMBER_EINVAL, "amber_hip_kat_phase_a: out_mask holds fewer than n * n_groups words (at most four groups)");
  if (n == 0) return AMBER_OK;
  HIP_TRY(hipSetDevice(h->device));
  DevBuf<float> d_o, d_d; DevBuf<uint32_t> d_m;
  HIP_TRY(d_o.alloc(3ull * n)); HIP_TRY(d_d.alloc(3ull * n)); HIP_TRY(d_m.alloc(static_cast<size_t>(n) * n_groups));
  HIP_TRY(hipMemcpy(d_o.p, origins, 12ull * n, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_d.p, dirs, 12ull * n, hipMemcpyHostToDevice));
  const dim3 grid((n + 255) / 256), block(256);
  if (h->hit_engine == kHitTwoPhaseN) {
    if (axis_loops) hipLaunchKernelGGL((kat_phase_a_kernel<true, true>), grid, block, 0, h->stream, h->scene, n, d_o.p, d_d.p, d_m.p);
    else hipLaunchKernelGGL((kat_phase_a_kernel<true, false>), grid, block, 0, h->stream, h->scene, n, d_o.p, d_d.p, d_m.p);
  } else {
    if (axis_loops) hipLaunchKernelGGL((kat_phase_a_kernel<false, true>), grid, block, 0, h->stream, h->scene, n, d_o.p, d_d.p, d_m.p);
    else hipLaunchKernelGGL((kat_phase_a_kernel<false, false>), grid, block, 0, h->stream, h->scene, n, d_o.p, d_d.p, d_m.p);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipMemcpy(out_mask, d_m.p, 4ull * n * n_groups, hipMemcpyDeviceToHost));
  return AMBER_OK;
}); }

int amber_hip_kat_sample(amber_hip_pt* h, uint32_t n, const uint32_t* material, const float* normals,
                         const float* dirs_out, uint64_t* rng_state, float* out_dir_in, float* out_weight) { return Guarded("amber_hip_kat_sample", [&]() -> int {
  if (!h || !material || !normals || !dirs_out || !rng_state || !out_dir_in || !out_weight) return Fail(AMBER_EINVAL, "null argument");
  if (n == 0) return AMBER_OK;
  for (uint32_t i = 0; i < n; i++)
    if ((material[i] & 0x7fffffffu) >= h->n_materials) return Fail(AMBER_EINVAL, "material index out of range");   // bit 31: SampleImportance
  HIP_TRY(hipSetDevice(h->device));
  DevBuf<uint32_t> d_m; DevBuf<float> d_n, d_d, d_o, d_w; DevBuf<uint64_t> d_r;
  HIP_TRY(d_m.alloc(n)); HIP_TRY(d_n.alloc(3 * n)); HIP_TRY(d_d.alloc(3 * n)); HIP_TRY(d_o.alloc(3 * n)); HIP_TRY(d_w.alloc(3 * n)); HIP_TRY(d_r.alloc(n));
  HIP_TRY(hipMemcpy(d_m.p, material, 4ull * n, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_n.p, normals, 12ull * n, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_d.p, dirs_out, 12ull * n, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_r.p, rng_state, 8ull * n, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(kat_sample_kernel, dim3((n + 255) / 256), dim3(256), 0, h->stream, h->scene, n, d_m.p, d_n.p, d_d.p, d_r.p, d_o.p, d_w.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipMemcpy(rng_state, d_r.p, 8ull * n, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(out_dir_in, d_o.p, 12ull * n, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(out_weight, d_w.p, 12ull * n, hipMemcpyDeviceToHost));
  return AMBER_OK;
}); }

int amber_hip_kat_eye(amber_hip_pt* h, uint32_t n, const uint32_t* pixel, const uint32_t* sample, float* out7) { return Guarded("amber_hip_kat_eye", [&]() -> int {
  if (!h || !pixel || !sample || !out7) return Fail(AMBER_EINVAL, "null argument");
  if (n == 0) return AMBER_OK;
  const uint32_t npx = h->scene.sensor.w * h->scene.sensor.h;
  for (uint32_t i = 0; i < n; i++) if (pixel[i] >= npx) return Fail(AMBER_EINVAL, "pixel index out of range");
  HIP_TRY(hipSetDevice(h->device));
  DevBuf<uint32_t> d_p, d_s; DevBuf<float> d_o;
  HIP_TRY(d_p.alloc(n)); HIP_TRY(d_s.alloc(n)); HIP_TRY(d_o.alloc(7 * n));
  HIP_TRY(hipMemcpy(d_p.p, pixel, 4ull * n, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_s.p, sample, 4ull * n, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(kat_eye_kernel, dim3((n + 255) / 256), dim3(256), 0, h->stream, h->scene, h->hashed_seed, n, d_p.p, d_s.p, d_o.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipMemcpy(out7, d_o.p, 28ull * n, hipMemcpyDeviceToHost));
  return AMBER_OK;
}); }

int amber_hip_kat_light_ray(amber_hip_pt* h, uint32_t n, uint64_t* rng_state, float* out_origin, float* out_dir, float* out_weight,
                            uint32_t* out_light) { return Guarded("amber_hip_kat_light_ray", [&]() -> int {
  if (!h || !rng_state || !out_origin || !out_dir || !out_weight || !out_light) return Fail(AMBER_EINVAL, "null argument");
  if (h->scene.n_lights == 0) return Fail(AMBER_EINVAL, "amber_hip_kat_light_ray: the handle's scene has no lights");
  if (h->lights_stale) return Fail(AMBER_EINVAL, "lights are stale after amber_hip_pt_update_objects: re-create the handle");
  if (n == 0) return AMBER_OK;
  if (n > 0x3fffffffu) return Fail(AMBER_EINVAL, "too many items for one call");
  HIP_TRY(hipSetDevice(h->device));
  DevBuf<uint64_t> d_r; DevBuf<float> d_o, d_d, d_w; DevBuf<uint32_t> d_l;
  HIP_TRY(d_r.alloc(n)); HIP_TRY(d_o.alloc(3ull * n)); HIP_TRY(d_d.alloc(3ull * n)); HIP_TRY(d_w.alloc(3ull * n)); HIP_TRY(d_l.alloc(n));
  HIP_TRY(hipMemcpy(d_r.p, rng_state, 8ull * n, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(kat_light_ray_kernel, dim3((n + 255) / 256), dim3(256), 0, h->stream, h->scene, n, d_r.p, d_o.p, d_d.p, d_w.p, d_l.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipMemcpy(rng_state, d_r.p, 8ull * n, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(out_origin, d_o.p, 12ull * n, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(out_dir, d_d.p, 12ull * n, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(out_weight, d_w.p, 12ull * n, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(out_light, d_l.p, 4ull * n, hipMemcpyDeviceToHost));
  return AMBER_OK;
}); }

int amber_hip_kat_lens_response(amber_hip_pt* h, uint32_t n, const float* position, const float* direction_out, uint32_t* out_reached,
                                uint32_t* out_pixel, float* out_value) { return Guarded("amber_hip_kat_lens_response", [&]() -> int {
  if (!h || !position || !direction_out || !out_reached || !out_pixel || !out_value) return Fail(AMBER_EINVAL, "null argument");
  if (n == 0) return AMBER_OK;
  if (n > 0x3fffffffu) return Fail(AMBER_EINVAL, "too many items for one call");
  HIP_TRY(hipSetDevice(h->device));
  DevBuf<float> d_p, d_d, d_v; DevBuf<uint32_t> d_r, d_x;
  HIP_TRY(d_p.alloc(3ull * n)); HIP_TRY(d_d.alloc(3ull * n)); HIP_TRY(d_v.alloc(n)); HIP_TRY(d_r.alloc(n)); HIP_TRY(d_x.alloc(n));
  HIP_TRY(hipMemcpy(d_p.p, position, 12ull * n, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_d.p, direction_out, 12ull * n, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(kat_lens_response_kernel, dim3((n + 255) / 256), dim3(256), 0, h->stream, h->scene, n, d_p.p, d_d.p, d_r.p, d_x.p, d_v.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipMemcpy(out_reached, d_r.p, 4ull * n, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(out_pixel, d_x.p, 4ull * n, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(out_value, d_v.p, 4ull * n, hipMemcpyDeviceToHost));
  return AMBER_OK;
}); }

int amber_hip_kat_radiance(amber_hip_pt* h, uint32_t n, const uint32_t* material, const float* normals, const float* dirs_out,
                           float* out) { return Guarded("amber_hip_kat_radiance", [&]() -> int {
  if (!h || !material || !normals || !dirs_out || !out) return Fail(AMBER_EINVAL, "null argument");
  if (n == 0) return AMBER_OK;
  if (n > 0x3fffffffu) return Fail(AMBER_EINVAL, "too many items for one call");
  for (uint32_t i = 0; i < n; i++) if (material[i] >= h->n_materials) return Fail(AMBER_EINVAL, "material index out of range");
  HIP_TRY(hipSetDevice(h->device));
  DevBuf<uint32_t> d_m; DevBuf<float> d_n, d_d, d_o;
  HIP_TRY(d_m.alloc(n)); HIP_TRY(d_n.alloc(3ull * n)); HIP_TRY(d_d.alloc(3ull * n)); HIP_TRY(d_o.alloc(3ull * n));
  HIP_TRY(hipMemcpy(d_m.p, material, 4ull * n, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_n.p, normals, 12ull * n, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_d.p, dirs_out, 12ull * n, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(kat_radiance_kernel, dim3((n + 255) / 256), dim3(256), 0, h->stream, h->scene, n, d_m.p, d_n.p, d_d.p, d_o.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipMemcpy(out, d_o.p, 12ull * n, hipMemcpyDeviceToHost));
  return AMBER_OK;
}); }

int amber_hip_kat_trace(amber_hip_pt* h, uint32_t n, const uint32_t* pixel, const uint32_t* sample,
                        uint32_t max_bounces, uint32_t* out_records, uint32_t* out_casts) { return Guarded("amber_hip_kat_trace", [&]() -> int {
  if (h && h->hit_engine == AMBER_ENGINE_REFERENCE_BVH) return Fail(AMBER_EINVAL, kKatNoRefBvh);
  if (!h || !pixel || !sample || !out_records || !out_casts || max_bounces == 0) return Fail(AMBER_EINVAL, "bad argument");
  if (n == 0) return AMBER_OK;
  const uint32_t npx = h->scene.sensor.w * h->scene.sensor.h;
  for (uint32_t i = 0; i < n; i++) if (pixel[i] >= npx) return Fail(AMBER_EINVAL, "pixel index out of range");
  HIP_TRY(hipSetDevice(h->device));
  DevBuf<uint32_t> d_p, d_s, d_r, d_c;
  const size_t nrec = static_cast<size_t>(n) * max_bounces * 11;
  HIP_TRY(d_p.alloc(n)); HIP_TRY(d_s.alloc(n)); HIP_TRY(d_r.alloc(nrec)); HIP_TRY(d_c.alloc(n));
  HIP_TRY(hipMemcpy(d_p.p, pixel, 4ull * n, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_s.p, sample, 4ull * n, hipMemcpyHostToDevice));
  HIP_TRY(hipMemsetAsync(d_r.p, 0, nrec * 4, h->stream));
  WithKatEngine(h, [&](auto engine) { hipLaunchKernelGGL(kat_trace_kernel<decltype(engine)::value>, dim3((n + 255) / 256), dim3(256), 0, h->stream, h->scene, h->hashed_seed, n, d_p.p, d_s.p, max_bounces, d_r.p, d_c.p); });
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipMemcpy(out_records, d_r.p, nrec * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(out_casts, d_c.p, 4ull * n, hipMemcpyDeviceToHost));
  return AMBER_OK;
}); }

int amber_hip_kat_signatures(amber_hip_pt* h, uint32_t first_sample, uint32_t n_samples, uint64_t* out) { return Guarded("amber_hip_kat_signatures", [&]() -> int {
  if (h && h->hit_engine == AMBER_ENGINE_REFERENCE_BVH) return Fail(AMBER_EINVAL, kKatNoRefBvh);
  if (!h || !out || n_samples == 0) return Fail(AMBER_EINVAL, "bad argument");
  if (static_cast<uint64_t>(first_sample) + n_samples > 0xffffffffull) return Fail(AMBER_EINVAL, "sample index overflow");
  const uint64_t n = BandPixels(h) * n_samples;
  if (n == 0) return AMBER_OK;
  if ((n + 255) / 256 > 0x7fffffffull) return Fail(AMBER_EINVAL, "too many paths for one call");
  HIP_TRY(hipSetDevice(h->device));
  DevBuf<unsigned long long> d_out;
  HIP_TRY(d_out.alloc(n));
  const dim3 grid(static_cast<uint32_t>((n + 255) / 256));
  WithKatEngine(h, [&](auto engine) { hipLaunchKernelGGL(kat_signature_kernel<decltype(engine)::value>, grid, dim3(256), 0, h->stream, h->scene, h->hashed_seed, n, first_sample, n_samples, h->row_begin, h->stripe_rows, h->stripe_period, MakeExactDiv(h->stripe_rows), d_out.p); });
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipMemcpy(out, d_out.p, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return AMBER_OK;
}); }

// Traversal alone (bvh_stream.inc): closest hits of n rays through engine BVH's resumable traversal in a kernel that does nothing
// else, `waves` resident waves per SIMD (4, 5, 6 or 8), idle lanes refilled once `refill_min` of a wave's lanes are idle.
// Returns t (NaN = miss) and the object index per ray, and the kernel time of `repeats` launches (the best one).
int amber_hip_kat_traversal_rate(amber_hip_pt* h, uint32_t n, const float* origins, const float* dirs, uint32_t waves, uint32_t refill_min, uint32_t repeats,
                                 float* out_t, int32_t* out_object, double* best_ms, uint32_t* out_rounds) { return Guarded("amber_hip_kat_traversal_rate", [&]() -> int {
  // one launch walks the ray array `repeats` times (a launch of n * repeats rays); best_ms is the time of that launch
  if (!h || !origins || !dirs || !out_t || !out_object || n == 0) return Fail(AMBER_EINVAL, "bad argument");
  if (h->hit_engine != AMBER_ENGINE_BVH) return Fail(AMBER_EINVAL, "the handle's engine is not BVH");
  if (refill_min == 0 || refill_min > 64) return Fail(AMBER_EINVAL, "refill_min must be in [1, 64]");
  const uint64_t n_virtual = static_cast<uint64_t>(n) * (repeats ? repeats : 1u);
  if (n_virtual > 0xfffffeffull) return Fail(AMBER_EINVAL, "n * repeats must stay below 2^32");
  HIP_TRY(hipSetDevice(h->device));
  AMBER_TRY(ResolvePending(h));
  std::vector<float4> packed(2ull * n);
  for (uint32_t i = 0; i < n; i++) {
    packed[2ull * i] = make_float4(origins[3ull * i], origins[3ull * i + 1], origins[3ull * i + 2], 0.f);
    packed[2ull * i + 1] = make_float4(dirs[3ull * i], dirs[3ull * i + 1], dirs[3ull * i + 2], 0.f);
  }
  DevBuf<float4> d_rays; DevBuf<float2> d_out; DevBuf<unsigned int> d_next; DevBuf<int32_t> d_stack; DevBuf<uint32_t> d_rounds;
  if (out_rounds) HIP_TRY(d_rounds.alloc(n));
  HIP_TRY(d_rays.alloc(2ull * n)); HIP_TRY(d_out.alloc(n)); HIP_TRY(d_next.alloc(1));
  const uint32_t n_blocks = static_cast<uint32_t>(h->n_cus) * (waves >= 4 && waves <= 8 ? waves : 5u);
  HIP_TRY(d_stack.alloc(static_cast<size_t>(n_blocks) * 256u * AMBER_BVH_STACK));
  HIP_TRY(hipMemcpy(d_rays.p, packed.data(), packed.size() * sizeof(float4), hipMemcpyHostToDevice));
  Event ev0, ev1;                                                        // released on every exit path
  HIP_TRY(hipEventCreate(&ev0.v)); HIP_TRY(hipEventCreate(&ev1.v));
  const hipEvent_t e0 = ev0.v, e1 = ev1.v;
  double best = 1e300;
  const uint32_t nv = static_cast<uint32_t>(n_virtual);
  for (uint32_t rep = 0; rep < 2u; rep++) {                              // a warm-up launch and the measured one
    HIP_TRY(hipMemsetAsync(d_next.p, 0, sizeof(unsigned int), h->stream));
    HIP_TRY(hipEventRecord(e0, h->stream));
    switch (waves) {
      case 4: hipLaunchKernelGGL((bvh_trace_rate_kernel<4, 24>), dim3(n_blocks), dim3(256), 0, h->stream, h->scene, nv, d_rays.p, d_out.p, d_next.p, d_stack.p, refill_min, n, d_rounds.p); break;
      case 6: hipLaunchKernelGGL((bvh_trace_rate_kernel<6, 24>), dim3(n_blocks), dim3(256), 0, h->stream, h->scene, nv, d_rays.p, d_out.p, d_next.p, d_stack.p, refill_min, n, d_rounds.p); break;
      case 8: hipLaunchKernelGGL((bvh_trace_rate_kernel<8, 16>), dim3(n_blocks), dim3(256), 0, h->stream, h->scene, nv, d_rays.p, d_out.p, d_next.p, d_stack.p, refill_min, n, d_rounds.p); break;
      default: hipLaunchKernelGGL((bvh_trace_rate_kernel<5, 24>), dim3(n_blocks), dim3(256), 0, h->stream, h->scene, nv, d_rays.p, d_out.p, d_next.p, d_stack.p, refill_min, n, d_rounds.p); break;
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(e1, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    float ms = 0; HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    if (rep == 1u || ms < best) best = ms;
  }
  std::vector<float2> res(n);
  HIP_TRY(hipMemcpy(res.data(), d_out.p, n * sizeof(float2), hipMemcpyDeviceToHost));
  if (out_rounds) HIP_TRY(hipMemcpy(out_rounds, d_rounds.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
  std::vector<uint32_t> prims(h->scene.n_objects);
  HIP_TRY(hipMemcpy(prims.data(), h->scene.bvh_prims, prims.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
  for (uint32_t i = 0; i < n; i++) {
    int32_t slot; std::memcpy(&slot, &res[i].y, 4);
    out_object[i] = slot < 0 ? -1 : static_cast<int32_t>(prims[slot]);
    out_t[i] = slot < 0 ? std::nanf("") : res[i].x;
  }
  if (best_ms) *best_ms = best;
  return AMBER_OK;
}); }

int amber_hip_kat_pixel_masks(amber_hip_pt* h, uint32_t* out_mask, uint32_t* out_slot_of_object, uint32_t* out_always_mask, double* kernel_ms) { return Guarded("amber_hip_kat_pixel_masks", [&]() -> int {
  if (!h) return Fail(AMBER_EINVAL, "null handle");
  if (!h->two_phase) return Fail(AMBER_EINVAL, "pixel masks belong to the two-phase engine");
  HIP_TRY(hipSetDevice(h->device));
  AMBER_TRY(ResolvePending(h));
  const uint32_t n_pixels = static_cast<uint32_t>(BandPixels(h));
  if (out_mask || kernel_ms) {                                 // the slot table and the always-mask below do not need the kernel
    float ms = 0;
    AMBER_TRY(StartPixelMasks(h, kernel_ms ? &ms : nullptr));
    if (!h->pixel_mask_ready) return Fail(AMBER_EINVAL, "pixel masks are switched off (AMBER_PIXEL_MASK=0) or the band is empty");
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (out_mask) HIP_TRY(hipMemcpy(out_mask, h->d_pixel_mask, static_cast<size_t>(n_pixels) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (kernel_ms) *kernel_ms = static_cast<double>(ms);
  }
  if (out_slot_of_object) {
    for (uint32_t i = 0; i < h->scene.n_objects; i++) out_slot_of_object[i] = 0xffffffffu;
    for (size_t k = 0; k < h->prog_order.size(); k++) if (h->prog_order[k] < h->scene.n_objects) out_slot_of_object[h->prog_order[k]] = static_cast<uint32_t>(k);
  }
  if (out_always_mask) *out_always_mask = h->scene.always_mask | h->scene.blade_mask;
  return AMBER_OK;
}); }

int amber_hip_kat_bvh_dump(amber_hip_pt* h, uint32_t* nodes, uint32_t node_capacity, uint32_t* prims, uint32_t prim_capacity, AmberBvhDump* info) { return Guarded("amber_hip_kat_bvh_dump", [&]() -> int {
  if (!h || !info) return Fail(AMBER_EINVAL, "null argument");
  if (h->hit_engine != AMBER_ENGINE_BVH) return Fail(AMBER_EINVAL, "the handle's engine is not BVH");
  HIP_TRY(hipSetDevice(h->device));
  AMBER_TRY(ResolvePending(h));
  HIP_TRY(hipStreamSynchronize(h->stream));
  static_assert(sizeof(DevBvhNodeQ) == 8 * sizeof(uint32_t), "a dumped node is 8 words");
  info->n_nodes = h->build.n_nodes; info->n_prims = h->scene.n_objects; info->root = h->scene.bvh_root; info->depth = h->build.depth;
  for (int c = 0; c < 3; c++) { info->gmin[c] = h->scene.bvh_gmin[c]; info->step[c] = h->scene.bvh_step[c]; info->reach[c] = h->scene.bvh_reach[c]; }
  const uint32_t n_nodes = std::min(node_capacity, info->n_nodes), n_prims = std::min(prim_capacity, info->n_prims);
  if (nodes && n_nodes) HIP_TRY(hipMemcpy(nodes, h->scene.bvh_nodes, static_cast<size_t>(n_nodes) * sizeof(DevBvhNodeQ), hipMemcpyDeviceToHost));
  if (prims && n_prims) HIP_TRY(hipMemcpy(prims, h->scene.bvh_prims, static_cast<size_t>(n_prims) * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return AMBER_OK;
}); }

int amber_hip_pt_signatures(amber_hip_pt* h, uint32_t first_sample, uint32_t n_samples, uint64_t* out) { return Guarded("amber_hip_pt_signatures", [&]() -> int {
  if (!h || !out || n_samples == 0) return Fail(AMBER_EINVAL, "bad argument");
  if (static_cast<uint64_t>(first_sample) + n_samples > 0xffffffffull) return Fail(AMBER_EINVAL, "sample index overflow");
  if (h->engine == AMBER_ENGINE_WAVEFRONT) return Fail(AMBER_EINVAL, "signatures come from the work-queue kernels (engines list, two_phase, bvh)");
  const uint32_t n_pixels = static_cast<uint32_t>(BandPixels(h));
  const uint64_t n = static_cast<uint64_t>(n_pixels) * n_samples;
  if (n == 0) return AMBER_OK;
  if (n > kMaxPathsPerLaunch) return Fail(AMBER_EINVAL, "too many paths for one call");
  HIP_TRY(hipSetDevice(h->device));
  AMBER_TRY(ResolvePending(h));
  HIP_TRY(hipStreamSynchronize(h->stream));
  AMBER_TRY(Grow(h, h->d_sig, n, "signatures"));
  HIP_TRY(hipMemsetAsync(h->d_sig, 0, n * sizeof(unsigned long long), h->stream));
  AMBER_TRY(RenderSamples(h, first_sample, n_samples, n_pixels, h->d_fb, h->d_sig));   // (nothing of a signature launch reaches the target)
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipMemcpy(out, h->d_sig, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return AMBER_OK;
}); }

int amber_hip_kat_lt_accumulate(amber_hip_pt* h, const AmberSplat* records, uint32_t n) { return Guarded("amber_hip_kat_lt_accumulate", [&]() -> int {
  if (!h || (n && !records)) return Fail(AMBER_EINVAL, "null argument");
  if (!WholeFrame(h)) return Fail(AMBER_EINVAL, "amber_hip_kat_lt_accumulate: the handle renders a band or stripes of the frame");
  if (n > 0x7fffffffu) return Fail(AMBER_EINVAL, "too many records for one call");
  const uint32_t npx = h->scene.sensor.w * h->scene.sensor.h;
  for (uint32_t i = 0; i < n; i++) if (records[i].pixel >= npx) return Fail(AMBER_EINVAL, "pixel index out of range");
  if (n == 0) return AMBER_OK;
  HIP_TRY(hipSetDevice(h->device));
  AMBER_TRY(ResolvePending(h));
  AMBER_TRY(EnsureLtSplats(h, n));
  static_assert(sizeof(AmberSplat) == sizeof(DevSplat), "splat layouts must agree");
  HIP_TRY(hipMemcpyAsync(h->d_splats, records, static_cast<size_t>(n) * sizeof(DevSplat), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipMemsetAsync(h->lt.longest.p, 0, sizeof(unsigned int), h->stream));
  AMBER_TRY(LtAccumulate(h, n, 32u));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return AMBER_OK;
}); }

int amber_hip_kat_accumulate(amber_hip_pt* h, uint32_t n_samples, const uint32_t* q, const float* rgb, uint32_t n_items, uint32_t n_waves, uint32_t rec_capacity,
                             uint64_t rays, AmberAccumulateInfo* info) { return Guarded("amber_hip_kat_accumulate", [&]() -> int {
  if (info) *info = AmberAccumulateInfo{};
  if (!h || (n_items && (!q || !rgb))) return Fail(AMBER_EINVAL, "null argument");
  if (n_samples == 0 || n_waves == 0) return Fail(AMBER_EINVAL, "amber_hip_kat_accumulate: n_samples and n_waves must not be zero");
  if (n_waves > (1u << 20)) return Fail(AMBER_EINVAL, "amber_hip_kat_accumulate: more than 2^20 waves");
  const uint64_t n_paths = BandPixels(h) * n_samples;
  if (n_paths >= (1ull << 32)) return Fail(AMBER_EINVAL, "amber_hip_kat_accumulate: n_pixels * n_samples must stay below 2^32");
  {
    std::vector<uint32_t> seen;
    seen.reserve(n_items);
    for (uint32_t i = 0; i < n_items; i++) {
      if (q[i] == AMBER_REC_UNUSED) continue;
      if (q[i] >= n_paths) return Fail(AMBER_EINVAL, "amber_hip_kat_accumulate: item " + std::to_string(i) + ": path index out of range");
      seen.push_back(q[i]);
    }
    std::sort(seen.begin(), seen.end());
    if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) return Fail(AMBER_EINVAL, "amber_hip_kat_accumulate: a path index occurs twice");
  }
  HIP_TRY(hipSetDevice(h->device));
  AMBER_TRY(ResolvePending(h));                                  // what is in flight stands first: it uses the record buffer
  PathLaunchBufs& p = h->paths;
  if (rec_capacity != 0 && rec_capacity < p.rec_capacity)
    return Fail(AMBER_EINVAL, "amber_hip_kat_accumulate: rec_capacity " + std::to_string(rec_capacity) + " is below the " + std::to_string(p.rec_capacity) + " slots the handle's record buffer has");
  const uint32_t n_pixels = static_cast<uint32_t>(BandPixels(h));
  if (n_pixels == 0) return AMBER_OK;                            // empty band
  AMBER_TRY(EnsureRecordCapacity(h, rec_capacity ? rec_capacity : static_cast<uint64_t>(n_items) + RecordSlack(h)));
  DevBuf<uint32_t> d_q; DevBuf<float> d_rgb;                     // live until the launch stands (ResolvePending below repeats it from them)
  HIP_TRY(d_q.alloc(n_items ? n_items : 1u)); HIP_TRY(d_rgb.alloc(n_items ? 3ull * n_items : 1u));
  if (n_items) {
    HIP_TRY(hipMemcpy(d_q.p, q, 4ull * n_items, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_rgb.p, rgb, 12ull * n_items, hipMemcpyHostToDevice));
  }
  RecordProducer producer;
  producer.lab = true; producer.q = d_q.p; producer.rgb = d_rgb.p; producer.n_items = n_items; producer.n_waves = n_waves; producer.rays = rays;
  const uint64_t launches0 = p.n_launches, repeats0 = p.n_repeats;
  AMBER_TRY(LaunchLabRecords(h, n_samples, n_pixels, h->d_fb, producer));
  const int rc = ResolvePending(h);
  p.pending = false; p.pending_producer = RecordProducer{};      // (whatever happened: the device inputs end with this call)
  AMBER_TRY(rc);
  const size_t used_words = static_cast<size_t>((n_paths + 31u) / 32u);
  std::vector<uint32_t> words(used_words);
  if (used_words) HIP_TRY(hipMemcpyAsync(words.data(), p.flags, used_words * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (info) {
    info->n_launches = static_cast<uint32_t>(p.n_launches - launches0); info->n_repeats = static_cast<uint32_t>(p.n_repeats - repeats0);
    info->rec_count = *p.h_rec_count.v;
    info->flag_words_set = static_cast<uint32_t>(std::count_if(words.begin(), words.end(), [](uint32_t w) { return w != 0u; }));
    info->flags_dirty = p.flags_dirty ? 1u : 0u;
  }
  return AMBER_OK;
}); }

int amber_hip_kat_scout_flags(amber_hip_pt* h, uint32_t first_sample, uint32_t n_samples, uint32_t* out_flags, uint64_t n_words, uint32_t* out_scouts, uint32_t* out_bound0) {
  return Guarded("amber_hip_kat_scout_flags", [&]() -> int {
  if (!h || !out_flags) return Fail(AMBER_EINVAL, "null argument");
  if (out_scouts) *out_scouts = h->scout ? 1u : 0u;
  if (out_bound0) *out_bound0 = h->scout_bound0;
  const uint64_t n_paths = BandPixels(h) * n_samples, need_words = (n_paths + 31u) / 32u;
  if (n_samples == 0 || n_paths > kMaxPathsPerLaunch || static_cast<uint64_t>(first_sample) + n_samples > 0xffffffffull) return Fail(AMBER_EINVAL, "amber_hip_kat_scout_flags: no samples, or more paths than one launch takes");
  if (n_words < need_words) return Fail(AMBER_EINVAL, "amber_hip_kat_scout_flags: the bitmap of this launch has " + std::to_string(need_words) + " words");
  std::memset(out_flags, 0, n_words * sizeof(uint32_t));
  if (!h->scout || n_paths == 0) return AMBER_OK;
  HIP_TRY(hipSetDevice(h->device));
  AMBER_TRY(ResolvePending(h));
  AMBER_TRY(EnsureRecordCapacity(h, n_paths + RecordSlack(h)));            // a slot for every path: the scout's records are not looked at, but none is written out of bounds either way
  AMBER_TRY(LaunchPaths(h, first_sample, n_samples, static_cast<uint32_t>(BandPixels(h)), nullptr, nullptr, true));
  HIP_TRY(hipMemcpyAsync(out_flags, h->paths.flags, need_words * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return AMBER_OK;
}); }

int amber_hip_kat_lt_stage_ms(amber_hip_pt* h, double* sort_ms, double* sum_ms) {
  return StageMs("amber_hip_kat_lt_stage_ms", h, h ? &h->lt.clock : nullptr, {sort_ms, sum_ms});
}
int amber_hip_kat_photon_stage_ms(amber_hip_pt* h, double* trace_ms, double* sort_ms, double* gather_ms) {
  return StageMs("amber_hip_kat_photon_stage_ms", h, h ? &h->photons.clock : nullptr, {trace_ms, nullptr, sort_ms, gather_ms});   // (between trace and sort the host reads the counters)
}
int amber_hip_kat_pm_stage_ms(amber_hip_pt* h, double* build_ms, double* gather_ms) {
  return StageMs("amber_hip_kat_pm_stage_ms", h, h ? &h->pm.clock : nullptr, {build_ms, gather_ms});
}

int amber_hip_kat_bsdf(amber_hip_pt* h, uint32_t n, const int32_t* object, const float* normal, const float* dir_out, const float* dir_in, float* rgb_out) {
  return Guarded("amber_hip_kat_bsdf", [&]() -> int {
  if (!h || !object || !normal || !dir_out || !dir_in || !rgb_out) return Fail(AMBER_EINVAL, "null argument");
  if (n == 0) return AMBER_OK;
  if (n > 0x3fffffffu) return Fail(AMBER_EINVAL, "too many items for one call");
  for (uint32_t i = 0; i < n; i++) if (object[i] < 0 || static_cast<uint32_t>(object[i]) >= h->scene.n_objects) return Fail(AMBER_EINVAL, "object index out of range");
  HIP_TRY(hipSetDevice(h->device));
  DevBuf<int32_t> d_obj; DevBuf<float> d_n, d_o, d_i, d_rgb;
  HIP_TRY(d_obj.alloc(n)); HIP_TRY(d_n.alloc(3ull * n)); HIP_TRY(d_o.alloc(3ull * n)); HIP_TRY(d_i.alloc(3ull * n)); HIP_TRY(d_rgb.alloc(3ull * n));
  HIP_TRY(hipMemcpy(d_obj.p, object, 4ull * n, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_n.p, normal, 12ull * n, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_o.p, dir_out, 12ull * n, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_i.p, dir_in, 12ull * n, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(kat_bsdf_kernel, dim3((n + 255) / 256), dim3(256), 0, h->stream, h->scene, n, d_obj.p, d_n.p, d_o.p, d_i.p, d_rgb.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipMemcpy(rgb_out, d_rgb.p, 12ull * n, hipMemcpyDeviceToHost));
  return AMBER_OK;
}); }

int amber_hip_kat_math(int device, int mode, uint32_t n, const float* x, float* out) { return Guarded("amber_hip_kat_math", [&]() -> int {
  if (!x || !out || mode < 0 || mode > 3) return Fail(AMBER_EINVAL, "bad argument");
  if (n == 0) return AMBER_OK;
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) return Fail(AMBER_ENODEVICE, "no such HIP device");
  HIP_TRY(hipSetDevice(device));
  const size_t n_in = mode == 1 ? 2ull * n : n, n_out = mode == 1 ? n : 2ull * n;
  DevBuf<float> d_x, d_o;
  HIP_TRY(d_x.alloc(n_in)); HIP_TRY(d_o.alloc(n_out));
  HIP_TRY(hipMemcpy(d_x.p, x, n_in * 4, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(kat_math_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, mode, n, d_x.p, d_o.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, d_o.p, n_out * 4, hipMemcpyDeviceToHost));
  return AMBER_OK;
}); }

int amber_hip_kat_division(int device, int mode, uint32_t n, const float* x, float* out) { return Guarded("amber_hip_kat_division", [&]() -> int {
  if (!x || !out || mode < 0 || mode > 3) return Fail(AMBER_EINVAL, "bad argument");
  if (n == 0) return AMBER_OK;
  if (n > 0x3fffffffu) return Fail(AMBER_EINVAL, "too many groups for one call");
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) return Fail(AMBER_ENODEVICE, "no such HIP device");
  HIP_TRY(hipSetDevice(device));
  DevBuf<float> d_x, d_o;
  HIP_TRY(d_x.alloc(4ull * n)); HIP_TRY(d_o.alloc(3ull * n));
  HIP_TRY(hipMemcpy(d_x.p, x, 16ull * n, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(kat_division_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, mode, n, d_x.p, d_o.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, d_o.p, 12ull * n, hipMemcpyDeviceToHost));
  return AMBER_OK;
}); }

int amber_hip_kat_sqrt(int device, int mode, uint32_t n, const float* x, float* out) { return Guarded("amber_hip_kat_sqrt", [&]() -> int {
  if (!x || !out || mode < 0 || mode > 4) return Fail(AMBER_EINVAL, "bad argument");
  if (n == 0) return AMBER_OK;
  if (n > 0x3fffffffu) return Fail(AMBER_EINVAL, "too many items for one call");
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) return Fail(AMBER_ENODEVICE, "no such HIP device");
  HIP_TRY(hipSetDevice(device));
  const size_t width = mode <= 1 ? 1u : (mode <= 3 ? 3u : 2u);           // floats per item, in and out
  DevBuf<float> d_x, d_o;
  HIP_TRY(d_x.alloc(width * n)); HIP_TRY(d_o.alloc(width * n));
  HIP_TRY(hipMemcpy(d_x.p, x, width * n * 4, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(kat_sqrt_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, mode, n, d_x.p, d_o.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, d_o.p, width * n * 4, hipMemcpyDeviceToHost));
  return AMBER_OK;
}); }

int amber_hip_kat_sqrt_sweep(int device, uint32_t first_bits, uint64_t count, AmberSqrtSweep* out) { return Guarded("amber_hip_kat_sqrt_sweep", [&]() -> int {
  if (!out || count == 0 || static_cast<uint64_t>(first_bits) + count > (1ull << 32)) return Fail(AMBER_EINVAL, "bad argument");
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) return Fail(AMBER_ENODEVICE, "no such HIP device");
  HIP_TRY(hipSetDevice(device));
  static_assert(sizeof(SqrtSweepCounters) == sizeof(AmberSqrtSweep), "the kernel's counters are the C record");
  DevBuf<SqrtSweepCounters> d_c;
  HIP_TRY(d_c.alloc(1));
  HIP_TRY(hipMemset(d_c.p, 0, sizeof(SqrtSweepCounters)));
  const uint64_t blocks = (count + 255u) / 256u;
  hipLaunchKernelGGL(kat_sqrt_sweep_kernel, dim3(static_cast<uint32_t>(blocks < 8192u ? blocks : 8192u)), dim3(256), 0, 0, first_bits, static_cast<unsigned long long>(count), d_c.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, d_c.p, sizeof(SqrtSweepCounters), hipMemcpyDeviceToHost));
  return AMBER_OK;
}); }

}  // extern "C"
