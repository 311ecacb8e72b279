// denoise_variance.inc -- batch moments (amber_hip_pt_render_batch's fold, amber_hip_pt_moments_clear / _moments_download / amber_hip_pt_device_moments)
// and amber_hip_pt_denoise_variance: the a-trous filter of denoise.inc with its colour stop replaced by a luminance stop that is scaled by a per-pixel
// estimate of the variance of the mean, which is filtered along with the colour (Schied et al., HPG 2017, without the temporal part).  A fixed sequence of
// binary32 operations, each rounded alone; the contract of include/amber_hip.h states it (its numpy restatement: tests/denoise_variance_reference.py).
// Part of the one translation unit pt_host.hip.  The guide buffer and its prepare kernel are denoise.inc's own; the three guide stops (DenoiseGuideStop),
// the luminance, the moments' BandBuf, the checks of the parameters and of the output arguments and the output tail are image_stage.inc's.
//
//   moments_fold_kernel     one thread per band pixel, after a batch has been rendered into the handle's batch buffer instead of the framebuffer (the
//                           `target` of pt_launch.inc's launches): fb = fb + B, and the luminance of B / n into the pixel's {m1, m2, batches, pad}
//                           (one float4 load and store).
//   dv_moments_kernel       one thread per band pixel: {u1, u2, e, batches} -- the two divisions by `batches` once per pixel, not once per tap.
//   dv_variance_kernel      one thread per band pixel, denoise_level_kernel's tiling: the (2R + 1)^2 taps of step 3 over the guide and those records;
//                           writes the first colour-and-variance record {c0.rgb, var_0}.  Runs once per call; R is an argument.
//   dv_level_kernel         the hot path, one level, the step an argument: denoise_level_kernel's tiling (a wave is 64 consecutive pixels of a row), both
//                           loops fully unrolled, outside taps branch-free.  Colour and variance travel as ONE 16-byte record per pixel, so a tap is one
//                           float4 load next to the two guide float4s (denoise.inc: three 4-byte loads and two float4s); the 9 taps of gv read the
//                           variance word of the neighbours' records.  S / S_w through one reciprocal (shared_div.h); S_v / (S_w * S_w) is a plain quotient
//                           (its own denominator).  The last level writes 12-byte colours for resolve.inc's kernel.
// No LDS, no scratch, no atomics, no tuning surface.  Buffers of the handle, grown on first use: two record buffers used ping-pong (the second one holds
// dv_moments_kernel's records until level 0 overwrites it), denoise.inc's first colour buffer (c0 in, c_levels out) and its guide buffer.
namespace {

static_assert(sizeof(AmberMomentsPixel) == 16, "a moments pixel is one float4");
static_assert(sizeof(AmberDenoiseVarianceParams) == 32, "AmberDenoiseVarianceParams is 32 bytes");

__global__ void __launch_bounds__(256) moments_fold_kernel(float* __restrict__ fb, const float* __restrict__ batch, float4* __restrict__ moments, uint64_t n_pixels,
                                                           float n) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
  if (i >= n_pixels) return;
  const float* b = batch + 3u * i;
  float* s = fb + 3u * i;
  const float b0 = b[0], b1 = b[1], b2 = b[2];
  s[0] = s[0] + b0; s[1] = s[1] + b1; s[2] = s[2] + b2;
  const float y = DvLuminance(b0 / n, b1 / n, b2 / n);
  float4 m = moments[i];
  m.x = m.x + y; m.y = m.y + y * y; m.z = m.z + 1.0f;
  moments[i] = m;
}

__global__ void __launch_bounds__(256) dv_moments_kernel(const float4* __restrict__ moments, float4* __restrict__ u, uint64_t n_pixels) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
  if (i >= n_pixels) return;
  const float4 m = moments[i];
  float4 r = make_float4(0.f, 0.f, 0.f, m.z);
  if (m.z > 0.f) { r.x = m.x / m.z; r.y = m.y / m.z; r.z = 1.0f; }
  u[i] = r;
}

struct DvArgs {
  const float4* in;                               // level: {c_i.rgb, var_i} per band pixel; variance: {u1, u2, e, batches}
  float4* out;                                    // level: {c_{i+1}.rgb, var_{i+1}}; variance: {c0.rgb, var_0}
  const float* c0;                                // variance: 3 floats per band pixel
  float* out3;                                    // level: not null on the last level -- c_levels, 3 floats per band pixel, instead of `out`
  const float4* guide;                            // two float4 per band pixel: {a.xyz, z} {n.xyz, rz}
  uint32_t width, rows, blocks_x;                 // the band; tiles of 64 pixels per tile row
  int32_t step;                                   // level: 2^i; variance: R
  float k_normal, k_albedo, k_depth, k_lum;
};

__global__ void __launch_bounds__(256) dv_variance_kernel(const DvArgs a) {
  const uint32_t by = blockIdx.x / a.blocks_x, bx = blockIdx.x - by * a.blocks_x;
  const uint32_t x = bx * 64u + (threadIdx.x & 63u), y = by * 4u + (threadIdx.x >> 6);
  if (x >= a.width || y >= a.rows) return;
  const uint64_t p = static_cast<uint64_t>(y) * a.width + x;
  const float4 pa = a.guide[2u * p], pn = a.guide[2u * p + 1u];
  const float4 up = a.in[p];
  float a1 = 0.f, a2 = 0.f, gs = 0.f;
  for (int dy = -a.step; dy <= a.step; dy++) {
    const int64_t qy = static_cast<int64_t>(y) + dy;
    if (qy < 0 || qy >= static_cast<int64_t>(a.rows)) continue;
    for (int dx = -a.step; dx <= a.step; dx++) {
      const int64_t qx = static_cast<int64_t>(x) + dx;
      if (qx < 0 || qx >= static_cast<int64_t>(a.width)) continue;
      const uint64_t q = static_cast<uint64_t>(qy) * a.width + static_cast<uint64_t>(qx);
      const float4 uq = a.in[q];
      float g = up.z;
      if (q != p) g = DenoiseGuideStop(pa, pn, a.guide[2u * q], a.guide[2u * q + 1u], a.k_normal, a.k_albedo, a.k_depth) * uq.z;
      a1 = a1 + g * uq.x; a2 = a2 + g * uq.y; gs = gs + g;
    }
  }
  float v = 0.f;
  if (gs > 0.f) { const float mu = a1 / gs; v = DenoiseClamp0(a2 / gs - mu * mu); }
  if (up.w > 0.f) v = v / up.w;
  const float* c = a.c0 + 3u * p;
  a.out[p] = make_float4(c[0], c[1], c[2], v);
}

__global__ void __launch_bounds__(256) dv_level_kernel(const DvArgs a) {
  constexpr float kH[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
  const uint32_t by = blockIdx.x / a.blocks_x, bx = blockIdx.x - by * a.blocks_x;
  const uint32_t x = bx * 64u + (threadIdx.x & 63u), y = by * 4u + (threadIdx.x >> 6);
  if (x >= a.width || y >= a.rows) return;
  const uint64_t p = static_cast<uint64_t>(y) * a.width + x;
  const float4 pc = a.in[p];
  const float4 pa = a.guide[2u * p], pn = a.guide[2u * p + 1u];
  // gv: the 3 x 3 binomial blur of the variance at unit spacing, coordinates clamped to the band, in row-major order
  float gv = 0.f;
  {
    const uint32_t xs[3] = {x > 0u ? x - 1u : 0u, x, x + 1u < a.width ? x + 1u : x};
    const uint32_t ys[3] = {y > 0u ? y - 1u : 0u, y, y + 1u < a.rows ? y + 1u : y};
#pragma unroll
    for (int j = 0; j < 3; j++) {
      const uint64_t row = static_cast<uint64_t>(ys[j]) * a.width;
#pragma unroll
      for (int i = 0; i < 3; i++) {
        const float wt = (j == 1 ? 0.5f : 0.25f) * (i == 1 ? 0.5f : 0.25f);      // {1,2,1} x {1,2,1} / 16: exact
        gv = gv + wt * (i == 1 && j == 1 ? pc.w : a.in[row + xs[i]].w);
      }
    }
  }
  const float rp = 1.0f / (a.k_lum * gv + 1e-10f);
  const float lp = DvLuminance(pc.x, pc.y, pc.z);
  float sr = 0.f, sg = 0.f, sb = 0.f, sv = 0.f, sw = 0.f;
#pragma unroll
  for (int dy = -2; dy <= 2; dy++) {
    const int64_t qy = static_cast<int64_t>(y) + dy * a.step;
    const bool row_inside = qy >= 0 && qy < static_cast<int64_t>(a.rows);
#pragma unroll
    for (int dx = -2; dx <= 2; dx++) {
      const float hw = kH[dy + 2] * kH[dx + 2];                                // exact
      if (dy == 0 && dx == 0) {
        sr = sr + hw * pc.x; sg = sg + hw * pc.y; sb = sb + hw * pc.z; sv = sv + (hw * hw) * pc.w; sw = sw + hw;
        continue;
      }
      const int64_t qx = static_cast<int64_t>(x) + dx * a.step;
      const bool inside = row_inside && qx >= 0 && qx < static_cast<int64_t>(a.width);
      const uint64_t q = inside ? static_cast<uint64_t>(qy) * a.width + static_cast<uint64_t>(qx) : p;     // a tap outside loads the centre and adds nothing
      const float4 qc = a.in[q];
      const float d = lp - DvLuminance(qc.x, qc.y, qc.z);
      const float tl = DenoiseClamp0(1.0f - (d * d) * rp);
      const float e = DenoiseGuideStop(pa, pn, a.guide[2u * q], a.guide[2u * q + 1u], a.k_normal, a.k_albedo, a.k_depth) * tl;
      const float w = hw * (e * e);
      // branch-free as in denoise_level_kernel: an outside tap adds +0, which leaves the sums' bits as they are (no sum is ever -0)
      sr = sr + (inside ? w * qc.x : 0.f); sg = sg + (inside ? w * qc.y : 0.f); sb = sb + (inside ? w * qc.z : 0.f);
      sv = sv + (inside ? (w * w) * qc.w : 0.f); sw = sw + (inside ? w : 0.f);
    }
  }
  float cr, cg, cb;
  shared_div::Div3(sr, sg, sb, sw, cr, cg, cb);
  if (a.out3) { float* o = a.out3 + 3u * p; o[0] = cr; o[1] = cg; o[2] = cb; }
  else a.out[p] = make_float4(cr, cg, cb, sv / (sw * sw));
}

// The moments buffer of the band, zeroed by the first call that needs it: image_stage.inc's BandBuf
BandBuf MomentsBuf(amber_hip_pt* h) { return {{&h->img.moments}, 1, 1u, "moments buffer"}; }
int EnsureMoments(amber_hip_pt* h, const char* name) { return EnsureBand(h, MomentsBuf(h), name); }
int MomentsClear(amber_hip_pt* h) { return BandClear(h, MomentsBuf, "amber_hip_pt_moments_clear"); }
int MomentsDownload(amber_hip_pt* h, AmberMomentsPixel* out) { return BandDownload(h, MomentsBuf, out, "amber_hip_pt_moments_download"); }
int DeviceMoments(amber_hip_pt* h, void** dptr, uint64_t* n_pixels) { return BandPointer(h, MomentsBuf, dptr, n_pixels, "amber_hip_pt_device_moments"); }

// After a batch has been rendered into the handle's batch buffer: the framebuffer and the moments take it.
int FoldBatch(amber_hip_pt* h, uint32_t n_samples) {
  const uint64_t n_pixels = BandPixels(h);
  hipLaunchKernelGGL(moments_fold_kernel, dim3(static_cast<uint32_t>((n_pixels + 255u) / 256u)), dim3(256), 0, h->stream, h->d_fb.p, h->img.batch.p, h->img.moments.p, n_pixels,
                     static_cast<float>(n_samples));
  HIP_TRY(hipGetLastError());
  return AMBER_OK;
}

int DenoiseVariance(amber_hip_pt* h, uint32_t n_samples, const AmberDenoiseVarianceParams* params, uint32_t format, void* out, uint64_t out_bytes, uint32_t flags) {
  const std::string name = "amber_hip_pt_denoise_variance";
  const FilterExtra<AmberDenoiseVarianceParams> radius{&AmberDenoiseVarianceParams::var_radius, "var_radius", 0u, 3u, false};
  AMBER_TRY(CheckFilterParams(name, h, params, n_samples, 1u, &AmberDenoiseVarianceParams::k_lum, "k_lum", &radius));
  BandOutput o{};
  { const int rc = CheckBandOutput(h, name, true, format, out, out_bytes, flags, o); if (rc != AMBER_OK || o.n_pixels == 0) return rc; }
  const uint64_t n_pixels = o.n_pixels;
  AMBER_TRY(BeginFilter(h, name));
  AMBER_TRY(EnsureMoments(h, name.c_str()));
  ImageStageBufs& img = h->img;
  AMBER_TRY(Grow(h, img.denoise_color[0], static_cast<size_t>(n_pixels) * 3u, "denoise colour"));
  AMBER_TRY(Grow(h, img.denoise_guide, static_cast<size_t>(n_pixels) * 2u, "denoise guide"));
  for (DevBuf<float4>& r : img.dv_record) AMBER_TRY(Grow(h, r, static_cast<size_t>(n_pixels), "denoise records"));
  const dim3 per_pixel(static_cast<uint32_t>((n_pixels + 255u) / 256u)), tiles(static_cast<uint32_t>(o.n_tiles));
  hipLaunchKernelGGL(denoise_prepare_kernel, per_pixel, dim3(256), 0, h->stream, h->d_fb.p, img.aov.p, img.denoise_color[0].p, img.denoise_guide.p, n_pixels,
                     static_cast<float>(n_samples));
  hipLaunchKernelGGL(dv_moments_kernel, per_pixel, dim3(256), 0, h->stream, img.moments.p, img.dv_record[1].p, n_pixels);
  DvArgs a{};
  a.guide = img.denoise_guide; a.width = o.width; a.rows = o.rows; a.blocks_x = o.blocks_x;
  a.k_normal = params->k_normal; a.k_albedo = params->k_albedo; a.k_depth = params->k_depth; a.k_lum = params->k_lum;
  a.in = img.dv_record[1]; a.out = img.dv_record[0]; a.c0 = img.denoise_color[0]; a.step = static_cast<int32_t>(params->var_radius);
  hipLaunchKernelGGL(dv_variance_kernel, tiles, dim3(256), 0, h->stream, a);
  a.c0 = nullptr;
  for (uint32_t i = 0; i < params->levels; i++) {
    a.in = img.dv_record[i & 1u]; a.out = img.dv_record[(i + 1u) & 1u]; a.step = 1 << i;
    a.out3 = i + 1u == params->levels ? img.denoise_color[0].p : nullptr;
    hipLaunchKernelGGL(dv_level_kernel, tiles, dim3(256), 0, h->stream, a);
  }
  return WriteBandOutput(h, o, format, img.denoise_color[0], 1.0f, out);
}

}  // namespace
