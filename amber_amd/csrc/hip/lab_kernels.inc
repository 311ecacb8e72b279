// lab_kernels.inc -- LAB BUILD ONLY (-DAMBER_LAB, libamber_hip_lab.so): the known-answer kernels the tests compare stage by stage with the oracle.
// Part of the one translation unit pt_host.hip (kernels are launched from there); see its header comment.

// ------------------------------------------------------------------------------------------------
// known-answer kernels (same device functions)
// ------------------------------------------------------------------------------------------------
template <int kEngine>
__global__ void kat_cast_kernel(const DevScene sc, uint32_t n, const float* org, const float* dir,
                                int32_t* out_obj, float* out_t, float* out_pos, float* out_n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t k = ClampToLastItem(i, n);
  const EngineLds lds = StageEngineLds<kEngine, AMBER_BVH_STACK>(sc);
  const V3 o = ld3(org + 3 * k), d = ld3(dir + 3 * k);
  HitRec h;
#ifdef AMBER_STAMPS
  StampCtx stamp_store{}; StampCtx* stamp_ctx = &stamp_store;
#endif
  ClosestHit<kEngine>(sc, lds.objects, lds.stack, o, d, -1, h AMBER_STAMP_ARG);
  if (i >= n) return;
  out_obj[i] = h.idx;
  if (h.idx < 0) {
    out_t[i] = __builtin_nanf("");
    for (int c = 0; c < 3; c++) { out_pos[3 * i + c] = 0.f; out_n[3 * i + c] = 0.f; }
    return;
  }
  V3 pos, nrm; uint32_t mat;
  ResolveHit<kEngine>(sc, lds.objects, h, o, d, pos, nrm, mat);
  out_t[i] = h.t;
  out_pos[3 * i] = pos.x; out_pos[3 * i + 1] = pos.y; out_pos[3 * i + 2] = pos.z;
  out_n[3 * i] = nrm.x; out_n[3 * i + 1] = nrm.y; out_n[3 * i + 2] = nrm.z;
}

// Phase A on its own (amber_hip_kat_phase_a): the candidate mask of every ray in every group of the filter program, out[i * n_groups + g], through the
// function the closest hit calls; kAxis: with the axis-slab loops, or with the general slab loop on the same records.  No exact test runs.
template <bool kMulti, bool kAxis>
__global__ void kat_phase_a_kernel(const DevScene sc, uint32_t n, const float* org, const float* dir, uint32_t* out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t k = ClampToLastItem(i, n);
  const V3 o = ld3(org + 3 * k), d = ld3(dir + 3 * k);
  const uint32_t n_groups = kMulti ? sc.n_groups : 1u;
  for (uint32_t g = 0; g < n_groups; ++g) {
    const FilterView fv = g == 0u ? SceneView(sc) : GroupView(sc, static_cast<int>(g));
    const uint32_t cand = PhaseA<kMulti, kAxis>(sc, fv, o, d, kMulti ? fv.always_mask : sc.always_mask);
    if (i < n) out[static_cast<size_t>(i) * n_groups + g] = cand;
  }
}

__global__ void kat_sample_kernel(const DevScene sc, uint32_t n, const uint32_t* material, const float* normals,
                                  const float* dirs_out, uint64_t* rng_state, float* out_dir, float* out_w) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const DevMaterial m = sc.materials[material[i] & 0x7fffffffu];
  uint64_t rng = rng_state[i];
  V3 di, w;
  if (material[i] >> 31) SampleImportance(m, ld3(normals + 3 * i), ld3(dirs_out + 3 * i), rng, di, w);   // bit 31: the light-tracing side
  else SampleLight(m, ld3(normals + 3 * i), ld3(dirs_out + 3 * i), rng, di, w);
  rng_state[i] = rng;
  out_dir[3 * i] = di.x; out_dir[3 * i + 1] = di.y; out_dir[3 * i + 2] = di.z;
  out_w[3 * i] = w.x; out_w[3 * i + 1] = w.y; out_w[3 * i + 2] = w.z;
}

__global__ void kat_eye_kernel(const DevScene sc, uint64_t hashed_seed, uint32_t n, const uint32_t* pixel,
                               const uint32_t* sample, float* out7) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t rng = XorShiftSeed(hashed_seed, pixel[i], sample[i]);
  V3 o, d; float w; int origin_slot;
  GenerateEyeRay(sc, pixel[i] % sc.sensor.w, pixel[i] / sc.sensor.w, rng, o, d, w, origin_slot);
  float* p = out7 + 7 * i;
  p[0] = o.x; p[1] = o.y; p[2] = o.z; p[3] = d.x; p[4] = d.y; p[5] = d.z; p[6] = w;
}

// The start of a light path from the item's own state, as pt_megakernel's light instantiation calls it.  out_light: the position in the light
// table, formed once more from the first draw (GenerateLightRay hands back only what a path needs).
__global__ void kat_light_ray_kernel(const DevScene sc, uint32_t n, uint64_t* rng_state, float* out_org, float* out_dir, float* out_w, uint32_t* out_light) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t rng = rng_state[i];
  uint64_t first = rng;
  const float x = Uniform(first) * sc.total_power;                        // the choice, recomputed: the first draw against the running sums
  uint32_t pos = 0;
  while (pos + 1u < sc.n_lights && sc.lights[pos].cum_power < x) ++pos;
  V3 o, d, w; int origin_slot;
  GenerateLightRay(sc, rng, o, d, w, origin_slot);
  rng_state[i] = rng;
  out_org[3 * i] = o.x; out_org[3 * i + 1] = o.y; out_org[3 * i + 2] = o.z;
  out_dir[3 * i] = d.x; out_dir[3 * i + 1] = d.y; out_dir[3 * i + 2] = d.z;
  out_w[3 * i] = w.x; out_w[3 * i + 1] = w.y; out_w[3 * i + 2] = w.z;
  out_light[i] = pos;
}

__global__ void kat_lens_response_kernel(const DevScene sc, uint32_t n, const float* position, const float* direction_out,
                                         uint32_t* out_reached, uint32_t* out_pixel, float* out_value) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t pixel = 0u; float value = 0.f;
  const bool reached = LensResponse(sc, ld3(position + 3 * i), ld3(direction_out + 3 * i), pixel, value);
  out_reached[i] = reached ? 1u : 0u;
  out_pixel[i] = reached ? pixel : 0u;
  out_value[i] = reached ? value : 0.f;
}

__global__ void kat_radiance_kernel(const DevScene sc, uint32_t n, const uint32_t* material, const float* normals, const float* dirs_out, float* out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const V3 r = Radiance(sc.materials[material[i]], ld3(normals + 3 * i), ld3(dirs_out + 3 * i));
  out[3 * i] = r.x; out[3 * i + 1] = r.y; out[3 * i + 2] = r.z;
}

__global__ void kat_bsdf_kernel(const DevScene sc, uint32_t n, const int32_t* object, const float* normals, const float* dirs_out, const float* dirs_in, float* out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const V3 r = BSDF(sc.materials[sc.objects[object[i]].material], ld3(normals + 3 * i), ld3(dirs_out + 3 * i), ld3(dirs_in + 3 * i));
  out[3 * i] = r.x; out[3 * i + 1] = r.y; out[3 * i + 2] = r.z;
}

template <int kEngine>
__global__ void kat_trace_kernel(const DevScene sc, uint64_t hashed_seed, uint32_t n, const uint32_t* pixel,
                                 const uint32_t* sample, uint32_t max_bounces, uint32_t* out_records, uint32_t* out_casts) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t k = ClampToLastItem(i, n);
  const EngineLds lds = StageEngineLds<kEngine, AMBER_BVH_STACK>(sc);
  PathRay ray;
  ray.rng = XorShiftSeed(hashed_seed, pixel[k], sample[k]);
  float ew;
  GenerateEyeRay(sc, pixel[k] % sc.sensor.w, pixel[k] / sc.sensor.w, ray.rng, ray.o, ray.d, ew, ray.origin_slot);
  ray.w = v3(ew, ew, ew); ray.meas = v3(0.f, 0.f, 0.f); ray.casts = 0;
  bool alive = true;
  // all lanes iterate together so that the scene loop stays wave-uniform; finished lanes idle
  while (__any(alive)) {
    if (alive) {
      Bounce b;
#ifdef AMBER_STAMPS
      StampCtx stamp_store{}; StampCtx* stamp_ctx = &stamp_store;
#endif
      BounceExtras extras; extras.trace = &b;
      alive = PathStep<TracedBounceCfg<kEngine>>(sc, lds, ray, extras AMBER_STAMP_ARG);
      if (i < n && ray.casts <= max_bounces) {
        uint32_t* r = out_records + (static_cast<size_t>(i) * max_bounces + (ray.casts - 1)) * 11u;
        r[0] = static_cast<uint32_t>(b.object);
        r[1] = __float_as_uint(b.t);
        r[2] = __float_as_uint(b.pos.x); r[3] = __float_as_uint(b.pos.y); r[4] = __float_as_uint(b.pos.z);
        r[5] = __float_as_uint(b.weight_before.x); r[6] = __float_as_uint(b.weight_before.y); r[7] = __float_as_uint(b.weight_before.z);
        r[8] = __float_as_uint(ray.meas.x); r[9] = __float_as_uint(ray.meas.y); r[10] = __float_as_uint(ray.meas.z);
      }
    }
  }
  if (i < n) out_casts[i] = ray.casts;
}

// Path signatures of the handle's band (amber_hip_kat_signatures): thread i traces the path of (band pixel i / n_samples,
// sample first_sample + i % n_samples) with the render kernels' device functions and writes FNV-1a-32 over the object index
// of every cast (low word; 0xffffffff = miss) and over the bits of every hit distance (high word).
template <int kEngine>
__global__ void kat_signature_kernel(const DevScene sc, uint64_t hashed_seed, uint64_t n, uint32_t first_sample, uint32_t n_samples,
                                     uint32_t row_begin, uint32_t stripe_rows, uint32_t stripe_period, ExactDiv div_stripe_rows, unsigned long long* out) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  const uint64_t k = ClampToLastItem(i, n);
  const EngineLds lds = StageEngineLds<kEngine, AMBER_BVH_STACK>(sc);
  const uint32_t plocal = static_cast<uint32_t>(k / n_samples), smp = first_sample + static_cast<uint32_t>(k % n_samples);
  const uint32_t lrow = plocal / sc.sensor.w, px = plocal - lrow * sc.sensor.w;
  const uint32_t py = FrameRow(row_begin, stripe_rows, stripe_period, div_stripe_rows, lrow);
  PathRay ray;
  ray.rng = XorShiftSeed(hashed_seed, px + py * sc.sensor.w, smp);
  float ew;
  GenerateEyeRay(sc, px, py, ray.rng, ray.o, ray.d, ew, ray.origin_slot);
  ray.w = v3(ew, ew, ew); ray.meas = v3(0.f, 0.f, 0.f); ray.casts = 0;
  PathSig sig; sig.Reset();
  bool alive = true;
  while (__any(alive)) {
    if (alive) {
      Bounce b;
#ifdef AMBER_STAMPS
      StampCtx stamp_store{}; StampCtx* stamp_ctx = &stamp_store;
#endif
      BounceExtras extras; extras.trace = &b;
      alive = PathStep<TracedBounceCfg<kEngine>>(sc, lds, ray, extras AMBER_STAMP_ARG);
      sig.Add(b);
    }
  }
  if (i < n) out[i] = sig.Packed();
}

// The caller's records through the product's own emitters (amber_hip_kat_accumulate).  Wave w of n_waves takes the trips w, w + n_waves, ... of 64
// consecutive items; lane l of trip t holds item 64 t + l (past n_items: a lane that emits nothing) and the whole wave calls EmitRecords, as a wave of
// the render kernels does when its paths end; after its last trip it closes its open block.  q[i] = AMBER_REC_UNUSED: item i emits nothing.  The host
// has checked every other q against the launch's path count, so no store leaves the bitmap, the touched bits or -- EmitRecords' own check -- the
// record buffer.  One lane adds `rays` to the launch's ray counter.
__global__ void __launch_bounds__(256) kat_accumulate_kernel(const RenderArgs a, const uint32_t* __restrict__ q, const float* __restrict__ rgb, uint32_t n_items,
                                                             uint32_t n_waves, unsigned long long rays) {
  const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
  if (wave >= n_waves) return;                                              // (whole waves)
  const uint32_t n_trips = n_items / 64u + (n_items % 64u != 0u);
  uint32_t rec_next = 0u, rec_end = 0u;
  for (uint32_t t = wave; t < n_trips; t += n_waves) {
    const uint64_t i = static_cast<uint64_t>(t) * 64u + lane;
    const uint32_t path = i < n_items ? q[i] : AMBER_REC_UNUSED;
    const bool emit = path != AMBER_REC_UNUSED;
    const V3 meas = emit ? ld3(rgb + 3u * i) : v3(0.f, 0.f, 0.f);
    EmitRecords(a, emit, path, meas, rec_next, rec_end);
  }
  CloseRecords(a, rec_next, rec_end);
  if (wave == 0u && lane == 0u) atomicAdd(a.ray_count, rays);
}

__global__ void kat_math_kernel(int mode, uint32_t n, const float* x, float* out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (mode == 0) { float s, c; SinCos(x[i], s, c); out[2 * i] = s; out[2 * i + 1] = c; }
  else if (mode == 1) out[i] = Pow(x[2 * i], x[2 * i + 1]);
  else {                                                    // 2: Pow4, 3: Pow5 -- the double's two words
    const double d = mode == 2 ? Pow4(x[i]) : Pow5(x[i]);
    const unsigned long long b = static_cast<unsigned long long>(__double_as_longlong(d));
    out[2 * i] = __uint_as_float(static_cast<uint32_t>(b)); out[2 * i + 1] = __uint_as_float(static_cast<uint32_t>(b >> 32));
  }
}

// Groups {a, b, c, d} of four floats.  0: a / d, b / d, c / d through shared_div.h's Div3 (one reciprocal; the wave falls back when a lane is
// out of range); 1: the plain-operator expressions; 2 / 3: Normalize({a, b, c}) through the shared and the plain form (d is not read).
// Whole waves run to the end (the last item stands in for the lanes past n): Div3's guard is a wave vote.
__global__ void kat_division_kernel(int mode, uint32_t n, const float* x, float* out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t k = ClampToLastItem(i, n);
  const float a = x[4ull * k], b = x[4ull * k + 1], c = x[4ull * k + 2], d = x[4ull * k + 3];
  V3 q;
  if (mode == 0) shared_div::Div3(a, b, c, d, q.x, q.y, q.z);
  else if (mode == 1) q = v3(a / d, b / d, c / d);
  else if (mode == 2) q = Normalize<true>(v3(a, b, c));
  else q = Normalize<false>(v3(a, b, c));
  if (i >= n) return;
  out[3ull * i] = q.x; out[3ull * i + 1] = q.y; out[3ull * i + 2] = q.z;
}

// exact_sqrt.h on the device.  0: x[i] -> sqrt through Sqrt1 (one v_rsq_f32 seed; the wave falls back when a lane is out of range); 1: __builtin_sqrtf;
// 2 / 3: groups {a, b, c} -> Normalize through the fused form (the root's half-reciprocal seeds the division) and through the plain form;
// 4: pairs {a, b} -> their roots through Sqrt2 (one guard, one vote).  Whole waves run to the end, as above: the guards are wave votes.
__global__ void kat_sqrt_kernel(int mode, uint32_t n, const float* x, float* out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const size_t k = ClampToLastItem(i, n);
  if (mode <= 1) {
    const float v = x[k];
    const float s = mode == 0 ? exact_sqrt::Sqrt1(v) : __builtin_sqrtf(v);
    if (i < n) out[i] = s;
  } else if (mode <= 3) {
    const V3 v = v3(x[3 * k], x[3 * k + 1], x[3 * k + 2]);
    const V3 q = mode == 2 ? Normalize<true, SQRT_FUSED>(v) : Normalize<false>(v);
    if (i < n) { out[3ull * i] = q.x; out[3ull * i + 1] = q.y; out[3ull * i + 2] = q.z; }
  } else {
    float sa, sb;
    exact_sqrt::Sqrt2(x[2 * k], x[2 * k + 1], sa, sb);
    if (i < n) { out[2ull * i] = sa; out[2ull * i + 1] = sb; }
  }
}

// Every bit pattern of [first_bits, first_bits + count): Sqrt1 against __builtin_sqrtf, bit for bit (64 consecutive patterns per wave trip: the
// bounds of the range are multiples of 64, so a wave is inside or outside as a whole).  For the patterns inside the range also how far
// v_rsq_f32 lies, in ulp, from the float nearest to 1 / sqrt(x) formed in binary64: the window that the host check of exact_sqrt.h has to cover.
struct SqrtSweepCounters { unsigned long long mismatches, in_range; uint32_t n_offenders, offenders[8]; int32_t seed_low, seed_high; };
__global__ void kat_sqrt_sweep_kernel(uint32_t first_bits, unsigned long long count, SqrtSweepCounters* counters) {
  const unsigned long long stride = static_cast<unsigned long long>(gridDim.x) * blockDim.x;
  uint32_t mismatches = 0, in_range = 0;
  int32_t low = 0, high = 0;
  for (unsigned long long i = static_cast<unsigned long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < count; i += stride) {
    const uint32_t bits = first_bits + static_cast<uint32_t>(i);
    const float x = __uint_as_float(bits);
    const float fast = exact_sqrt::Sqrt1(x), plain = __builtin_sqrtf(x);
    if (__float_as_uint(fast) != __float_as_uint(plain)) {
      ++mismatches;
      const uint32_t slot = atomicAdd(&counters->n_offenders, 1u);
      if (slot < 8u) counters->offenders[slot] = bits;
    }
    if (exact_sqrt::ExactSqrtSafe(x)) {
      ++in_range;
      const float nearest = static_cast<float>(1.0 / __builtin_sqrt(static_cast<double>(x)));
      const int32_t distance = static_cast<int32_t>(__float_as_uint(__builtin_amdgcn_rsqf(x))) - static_cast<int32_t>(__float_as_uint(nearest));
      low = distance < low ? distance : low;
      high = distance > high ? distance : high;
    }
  }
  for (int step = 32; step > 0; step >>= 1) {                          // the wave's extremes and sums in its first lane
    const int32_t other_low = __shfl_xor(low, step), other_high = __shfl_xor(high, step);
    low = other_low < low ? other_low : low;
    high = other_high > high ? other_high : high;
    mismatches += __shfl_xor(mismatches, step);
    in_range += __shfl_xor(in_range, step);
  }
  if ((threadIdx.x & 63u) == 0u) {
    if (mismatches) atomicAdd(&counters->mismatches, static_cast<unsigned long long>(mismatches));
    if (in_range) atomicAdd(&counters->in_range, static_cast<unsigned long long>(in_range));
    if (low < 0) atomicMin(&counters->seed_low, low);
    if (high > 0) atomicMax(&counters->seed_high, high);
  }
}

