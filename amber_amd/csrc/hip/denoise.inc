// denoise.inc -- amber_hip_pt_denoise: the edge-avoiding a-trous wavelet transform (Dammertz, Sewtz, Hanika, Lensch, HPG 2010) of the band's mean
// image, guided by the AOV buffer, between accumulation and the output stage.  The edge-stopping weights are compactly supported polynomials,
// clamp0(1 - d * k), not exponentials: the filter is a fixed sequence of binary32 operations, each rounded alone (-ffp-contract=off), and the
// contract of include/amber_hip.h states it operation by operation (its numpy restatement: tests/denoise_reference.py).  Part of the one translation
// unit pt_host.hip; the output stage is resolve.inc's kernel on the last colour buffer with n = 1 (x / 1.0f == x).
//
//   denoise_prepare_kernel   one thread per band pixel: reads the sums (12 bytes) and the AOV sums (32 bytes), writes c0 = sum / n (12 bytes) and the
//                            guide record {a.xyz, z}{n.xyz, rz} (32 bytes): the divisions by coverage and the reciprocal of the depth are done once
//                            per pixel here, not once per tap.
//   denoise_level_kernel     one level, the step an argument: one thread per pixel, a workgroup of four waves is a tile of 64 x 4 pixels and every wave
//                            64 consecutive pixels of one row -- at any step each of the 25 taps is then one coalesced row segment per wave at a
//                            uniform offset (768 bytes of colour, 2 KiB of guide).  Both loops are fully unrolled, so the centre tap (w = hw, nothing
//                            computed) and the 25 products hw are resolved at compile time; a tap outside the band loads the centre pixel instead and
//                            adds +0 (no branch, same bits: see the loop).  The three quotients S / S_w go through one reciprocal (shared_div.h: the
//                            same bits as the plain quotient; S_w >= 9/64 is always in range, tiny or non-finite S send the wave to the plain form).
// A level reads every 44-byte pixel record 25 times and writes 12 bytes: a cache-bandwidth problem (L1 / L2), which HBM sees about once per level.
// No LDS, no scratch, no atomics, no tuning surface: 256 threads per workgroup, registers left to the compiler (129 VGPR: 3 waves per SIMD).
// Buffers of the handle, grown on first use: two colour buffers used ping-pong (level i reads [i & 1], writes [(i + 1) & 1]) and the guide buffer;
// AMBER_RESOLVE_HOST stages through resolve's d_resolve_out.
namespace {

struct DenoiseLevelArgs {
  const float* cin;                               // c_i: 3 floats per band pixel
  float* cout;                                    // c_{i+1}
  const float4* guide;                            // two float4 per band pixel: {a.xyz, z} {n.xyz, rz}
  uint32_t width, rows, blocks_x;                 // the band; tiles of 64 pixels per tile row
  int32_t step;                                   // 2^i
  float k_normal, k_albedo, k_depth, k_color;     // k_color: kc_i
};

__global__ void __launch_bounds__(256) denoise_prepare_kernel(const float* __restrict__ fb, const float4* __restrict__ aov, float* __restrict__ c0,
                                                              float4* __restrict__ guide, uint64_t n_pixels, float n) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
  if (i >= n_pixels) return;
  const float* s = fb + 3u * i;
  float* c = c0 + 3u * i;
  c[0] = s[0] / n; c[1] = s[1] / n; c[2] = s[2] / n;
  const float4 a0 = aov[2u * i], a1 = aov[2u * i + 1u];
  const float cov = a1.w;
  float4 g0 = make_float4(0.f, 0.f, 0.f, 0.f), g1 = g0;
  if (cov > 0.f) {
    g0.x = a0.x / cov; g0.y = a0.y / cov; g0.z = a0.z / cov; g0.w = a0.w / cov;
    g1.x = a1.x / cov; g1.y = a1.y / cov; g1.z = a1.z / cov;
  }
  g1.w = g0.w > 0.f ? 1.0f / g0.w : 0.f;
  guide[2u * i] = g0; guide[2u * i + 1u] = g1;
}

__device__ __forceinline__ float DenoiseSq(float u0, float u1, float u2, float v0, float v1, float v2) {
  const float d0 = u0 - v0, d1 = u1 - v1, d2 = u2 - v2;
  return (d0 * d0 + d1 * d1) + d2 * d2;
}
__device__ __forceinline__ float DenoiseClamp0(float t) { return t > 0.f ? t : 0.f; }     // 0 for a NaN t
// (tn * ta) * tz: the three guide stops of a tap q seen from p, guide records {a.xyz, z} {n.xyz, rz} (denoise_variance.inc's kernels use it too)
__device__ __forceinline__ float DenoiseGuideStop(const float4& pa, const float4& pn, const float4& qa, const float4& qn, float k_normal, float k_albedo, float k_depth) {
  const float tn = DenoiseClamp0(1.0f - DenoiseSq(pn.x, pn.y, pn.z, qn.x, qn.y, qn.z) * k_normal);
  const float ta = DenoiseClamp0(1.0f - DenoiseSq(pa.x, pa.y, pa.z, qa.x, qa.y, qa.z) * k_albedo);
  const float tz = DenoiseClamp0(1.0f - (fabsf(pa.w - qa.w) * pn.w) * k_depth);
  return (tn * ta) * tz;
}

// the grid is one-dimensional (a band of one column may have 2^30 tile rows): tile b is tile column b % blocks_x of tile row b / blocks_x
__global__ void __launch_bounds__(256) denoise_level_kernel(const DenoiseLevelArgs a) {
  constexpr float kH[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
  const uint32_t by = blockIdx.x / a.blocks_x, bx = blockIdx.x - by * a.blocks_x;
  const uint32_t x = bx * 64u + (threadIdx.x & 63u), y = by * 4u + (threadIdx.x >> 6);
  if (x >= a.width || y >= a.rows) return;
  const uint64_t p = static_cast<uint64_t>(y) * a.width + x;
  const float* cp = a.cin + 3u * p;
  const float pr = cp[0], pg = cp[1], pb = cp[2];
  const float4 pa = a.guide[2u * p], pn = a.guide[2u * p + 1u];                // {a.xyz, z} {n.xyz, rz}
  float sr = 0.f, sg = 0.f, sb = 0.f, sw = 0.f;
#pragma unroll
  for (int dy = -2; dy <= 2; dy++) {
    const int64_t qy = static_cast<int64_t>(y) + dy * a.step;
    const bool row_inside = qy >= 0 && qy < static_cast<int64_t>(a.rows);
#pragma unroll
    for (int dx = -2; dx <= 2; dx++) {
      const float hw = kH[dy + 2] * kH[dx + 2];                                // exact
      if (dy == 0 && dx == 0) {
        sr = sr + hw * pr; sg = sg + hw * pg; sb = sb + hw * pb; sw = sw + hw;
        continue;
      }
      const int64_t qx = static_cast<int64_t>(x) + dx * a.step;
      const bool inside = row_inside && qx >= 0 && qx < static_cast<int64_t>(a.width);
      {
        const uint64_t q = inside ? static_cast<uint64_t>(qy) * a.width + static_cast<uint64_t>(qx) : p;     // a tap outside loads the centre and adds nothing
        const float* cq = a.cin + 3u * q;
        const float qr = cq[0], qg = cq[1], qb = cq[2];
        const float4 qa = a.guide[2u * q], qn = a.guide[2u * q + 1u];
        const float tc = DenoiseClamp0(1.0f - DenoiseSq(pr, pg, pb, qr, qg, qb) * a.k_color);
        const float e = DenoiseGuideStop(pa, pn, qa, qn, a.k_normal, a.k_albedo, a.k_depth) * tc;
        const float w = hw * (e * e);
        // branch-free: an outside tap adds +0 four times, which leaves the sums' bits as they are (a sum is never -0: it starts at +0, and
        // x + y is -0 only when both are).  With a branch per tap the compiler waits for every tap's loads where it uses them (46 VGPR, 76
        // waits); without, the loads of a row of taps are in flight together (129 VGPR, 3 waves per SIMD): measured 10 % faster at 1920 x 1080.
        sr = sr + (inside ? w * qr : 0.f); sg = sg + (inside ? w * qg : 0.f); sb = sb + (inside ? w * qb : 0.f); sw = sw + (inside ? w : 0.f);
      }
    }
  }
  float cr, cg, cb;
  shared_div::Div3(sr, sg, sb, sw, cr, cg, cb);
  float* o = a.cout + 3u * p;
  o[0] = cr; o[1] = cg; o[2] = cb;
}

static_assert(sizeof(AmberDenoiseParams) == 32, "AmberDenoiseParams is 32 bytes");

// What the output arguments of amber_hip_pt_denoise and amber_hip_pt_denoise_variance (denoise_variance.inc) must satisfy, checked in this order, and
// what the launches need of them.  AMBER_OK with n_pixels == 0: an empty band, nothing to do.
struct DenoiseOutput { uint32_t width, rows, blocks_x; uint64_t n_pixels, want, n_tiles; bool host, mirror; };

int CheckDenoiseOutput(const amber_hip_pt* h, const std::string& name, uint32_t format, const void* out, uint64_t out_bytes, uint32_t flags, DenoiseOutput& o) {
  o = DenoiseOutput{};
  if (format > AMBER_RESOLVE_RGBA8) return Fail(AMBER_EINVAL, name + ": unknown format " + std::to_string(format));
  if (flags & ~static_cast<uint32_t>(AMBER_RESOLVE_HOST | AMBER_RESOLVE_MIRROR_X)) return Fail(AMBER_EINVAL, name + ": unknown flag bits");
  if (h->stripe_period != 0u) return Fail(AMBER_EINVAL, name + ": a striped handle's local rows are not neighbours in the frame; filter a contiguous band");
  const uint32_t width = h->scene.sensor.w, rows = h->local_rows;
  const uint64_t n_pixels = static_cast<uint64_t>(rows) * width;
  const uint64_t want = n_pixels * kResolveBytesPerPixel[format];
  if (out_bytes != want)
    return Fail(AMBER_EINVAL, name + ": out_bytes is " + std::to_string(out_bytes) + ", the band takes exactly " + std::to_string(want) + " (" + std::to_string(rows) +
                                  " rows of " + std::to_string(width) + " pixels, " + std::to_string(kResolveBytesPerPixel[format]) + " bytes each)");
  if (n_pixels == 0) return AMBER_OK;                                         // empty band
  if (!out) return Fail(AMBER_EINVAL, name + ": null output pointer");
  const bool host = (flags & AMBER_RESOLVE_HOST) != 0u;
  if (!host && format != AMBER_RESOLVE_RGB8 && reinterpret_cast<uintptr_t>(out) % 4u != 0u)
    return Fail(AMBER_EINVAL, name + ": a device pointer for MEAN_F32 or RGBA8 must be 4-byte aligned");
  const uint32_t blocks_x = (width + 63u) / 64u;
  const uint64_t n_tiles = static_cast<uint64_t>(blocks_x) * ((rows + 3u) / 4u);
  if (n_tiles > 0x7fffffffull) return Fail(AMBER_EINVAL, name + ": band too large for one launch");
  o.width = width; o.rows = rows; o.blocks_x = blocks_x; o.n_pixels = n_pixels; o.want = want; o.n_tiles = n_tiles;
  o.host = host; o.mirror = (flags & AMBER_RESOLVE_MIRROR_X) != 0u;
  return AMBER_OK;
}

int Denoise(amber_hip_pt* h, uint32_t n_samples, const AmberDenoiseParams* params, uint32_t format, void* out, uint64_t out_bytes, uint32_t flags) {
  const std::string name = "amber_hip_pt_denoise";
  if (!h) return Fail(AMBER_EINVAL, name + ": null handle");
  if (!params) return Fail(AMBER_EINVAL, name + ": null params");
  if (n_samples == 0) return Fail(AMBER_EINVAL, name + ": n_samples is 0");
  if (params->levels < 1u || params->levels > 8u) return Fail(AMBER_EINVAL, name + ": levels is " + std::to_string(params->levels) + ", not 1 .. 8");
  const float k[4] = {params->k_normal, params->k_albedo, params->k_depth, params->k_color};
  const char* k_name[4] = {"k_normal", "k_albedo", "k_depth", "k_color"};
  for (int i = 0; i < 4; i++)
    if (!(k[i] >= 0.f) || std::isinf(k[i])) return Fail(AMBER_EINVAL, name + ": " + k_name[i] + " is negative, NaN or infinite");
  if (params->reserved[0] | params->reserved[1] | params->reserved[2]) return Fail(AMBER_EINVAL, name + ": reserved fields must be 0");
  DenoiseOutput o{};
  { const int rc = CheckDenoiseOutput(h, name, format, out, out_bytes, flags, o); if (rc != AMBER_OK || o.n_pixels == 0) return rc; }
  const uint32_t width = o.width, rows = o.rows, blocks_x = o.blocks_x;
  const uint64_t n_pixels = o.n_pixels, want = o.want, n_tiles = o.n_tiles;
  const bool host = o.host;
  HIP_TRY(hipSetDevice(h->device));
  if (h->pending && !h->pending_checked) { const int rc = ResolvePending(h); if (rc != AMBER_OK) return rc; }      // as resolve: the sums must stand
  { const int rc = EnsureAov(h, name.c_str()); if (rc != AMBER_OK) return rc; }
  for (DevBuf<float>& c : h->d_denoise_color) { const int rc = Grow(h, c, static_cast<size_t>(n_pixels) * 3u, "denoise colour"); if (rc != AMBER_OK) return rc; }
  { const int rc = Grow(h, h->d_denoise_guide, static_cast<size_t>(n_pixels) * 2u, "denoise guide"); if (rc != AMBER_OK) return rc; }
  void* d_out = out;
  if (host) {
    const int rc = Grow(h, h->d_resolve_out, want, "resolve staging"); if (rc != AMBER_OK) return rc;
    d_out = h->d_resolve_out.p;
  }
  hipLaunchKernelGGL(denoise_prepare_kernel, dim3(static_cast<uint32_t>((n_pixels + 255u) / 256u)), dim3(256), 0, h->stream, h->d_fb.p, h->d_aov.p,
                     h->d_denoise_color[0].p, h->d_denoise_guide.p, n_pixels, static_cast<float>(n_samples));
  DenoiseLevelArgs a{};
  a.guide = h->d_denoise_guide; a.width = width; a.rows = rows; a.blocks_x = blocks_x;
  a.k_normal = params->k_normal; a.k_albedo = params->k_albedo; a.k_depth = params->k_depth; a.k_color = params->k_color;
  for (uint32_t i = 0; i < params->levels; i++) {
    a.cin = h->d_denoise_color[i & 1u]; a.cout = h->d_denoise_color[(i + 1u) & 1u]; a.step = 1 << i;
    hipLaunchKernelGGL(denoise_level_kernel, dim3(static_cast<uint32_t>(n_tiles)), dim3(256), 0, h->stream, a);
    a.k_color = a.k_color * 4.0f;                                             // kc_{i+1} = kc_i * 4
  }
  const float* filtered = h->d_denoise_color[params->levels & 1u];
  const bool mirror = (flags & AMBER_RESOLVE_MIRROR_X) != 0u;
  if (format == AMBER_RESOLVE_MEAN_F32) LaunchResolve<AMBER_RESOLVE_MEAN_F32>(h, filtered, mirror, d_out, n_pixels, 1.0f);
  else if (format == AMBER_RESOLVE_RGB8) LaunchResolve<AMBER_RESOLVE_RGB8>(h, filtered, mirror, d_out, n_pixels, 1.0f);
  else LaunchResolve<AMBER_RESOLVE_RGBA8>(h, filtered, mirror, d_out, n_pixels, 1.0f);
  HIP_TRY(hipGetLastError());
  if (host) {
    HIP_TRY(hipMemcpyAsync(out, d_out, want, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
  }
  return AMBER_OK;
}

}  // namespace
