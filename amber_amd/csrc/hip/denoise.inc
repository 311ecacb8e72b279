// denoise.inc -- amber_hip_pt_denoise: the edge-avoiding a-trous wavelet transform (Dammertz, Sewtz, Hanika, Lensch, HPG 2010) of the band's mean
// image, guided by the AOV buffer, between accumulation and the output stage.  The edge-stopping weights are compactly supported polynomials,
// clamp0(1 - d * k), not exponentials: the filter is a fixed sequence of binary32 operations, each rounded alone (-ffp-contract=off), and the
// contract of include/amber_hip.h states it operation by operation (its numpy restatement: tests/denoise_reference.py).  Part of the one translation
// unit pt_host.hip; the output stage is resolve.inc's kernel on the last colour buffer with n = 1 (x / 1.0f == x).  From image_stage.inc: the
// stops' device helpers and the guide record, the checks of the parameters and of the output arguments, the output tail.  LaunchDenoiseLevels
// here runs the levels for amber_hip_pt_temporal too.
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
// AMBER_RESOLVE_HOST stages through the output tail's buffer.
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
  float4 g0, g1;
  GuideRecord(aov[2u * i], aov[2u * i + 1u], g0, g1);
  guide[2u * i] = g0; guide[2u * i + 1u] = g1;
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

// What every filter does once its arguments have passed: the device, the sums (as resolve: a pass that may have to be repeated must stand) and the AOV buffer
int BeginFilter(amber_hip_pt* h, const std::string& name) {
  HIP_TRY(hipSetDevice(h->device));
  AMBER_TRY(SettlePending(h));
  return EnsureAov(h, name.c_str());
}

// The levels 0 .. levels - 1 over the colour in the first colour buffer (both grown by the caller), ping-pong; the buffer that holds the last level's output
const float* LaunchDenoiseLevels(amber_hip_pt* h, const BandOutput& o, const float4* guide, uint32_t levels, float k_normal, float k_albedo, float k_depth, float k_color) {
  DenoiseLevelArgs a{};
  a.guide = guide; a.width = o.width; a.rows = o.rows; a.blocks_x = o.blocks_x;
  a.k_normal = k_normal; a.k_albedo = k_albedo; a.k_depth = k_depth; a.k_color = k_color;
  for (uint32_t i = 0; i < levels; i++) {
    a.cin = h->img.denoise_color[i & 1u]; a.cout = h->img.denoise_color[(i + 1u) & 1u]; a.step = 1 << i;
    hipLaunchKernelGGL(denoise_level_kernel, dim3(static_cast<uint32_t>(o.n_tiles)), dim3(256), 0, h->stream, a);
    a.k_color = a.k_color * 4.0f;                                             // kc_{i+1} = kc_i * 4
  }
  return h->img.denoise_color[levels & 1u];
}

int Denoise(amber_hip_pt* h, uint32_t n_samples, const AmberDenoiseParams* params, uint32_t format, void* out, uint64_t out_bytes, uint32_t flags) {
  const std::string name = "amber_hip_pt_denoise";
  AMBER_TRY(CheckFilterParams(name, h, params, n_samples, 1u, &AmberDenoiseParams::k_color, "k_color"));
  BandOutput o{};
  { const int rc = CheckBandOutput(h, name, true, format, out, out_bytes, flags, o); if (rc != AMBER_OK || o.n_pixels == 0) return rc; }
  AMBER_TRY(BeginFilter(h, name));
  ImageStageBufs& img = h->img;
  for (DevBuf<float>& c : img.denoise_color) AMBER_TRY(Grow(h, c, static_cast<size_t>(o.n_pixels) * 3u, "denoise colour"));
  AMBER_TRY(Grow(h, img.denoise_guide, static_cast<size_t>(o.n_pixels) * 2u, "denoise guide"));
  hipLaunchKernelGGL(denoise_prepare_kernel, dim3(static_cast<uint32_t>((o.n_pixels + 255u) / 256u)), dim3(256), 0, h->stream, h->d_fb.p, img.aov.p,
                     img.denoise_color[0].p, img.denoise_guide.p, o.n_pixels, static_cast<float>(n_samples));
  const float* filtered = LaunchDenoiseLevels(h, o, img.denoise_guide, params->levels, params->k_normal, params->k_albedo, params->k_depth, params->k_color);
  return WriteBandOutput(h, o, format, filtered, 1.0f, out);
}

}  // namespace
