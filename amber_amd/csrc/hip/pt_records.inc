// pt_records.inc -- from path records to ordered per-pixel sums (rec_rank / scan / place, reduce_flagged) and the per-pixel candidate masks (pixel_mask_kernel).
// Part of the one translation unit pt_host.hip (kernels are launched from there); see its header comment.

// ---- from records to ordered per-pixel sums ------------------------------------------------------------------------
// The records of a launch arrive in no order.  The bitmap gives every record its place: record of path q goes to
//   sorted[ base(pixel of q) + (set bits of that pixel below q) ],   base(p) = set bits of all pixels before p,
// so reduce_flagged_kernel can walk a pixel's bits in sample order and read its measurements consecutively.
//   rec_rank_kernel        per pixel: number of set bits, exclusive prefix within the workgroup, workgroup total
//   rec_scan_blocks_kernel one workgroup: exclusive prefix over the workgroup totals; also folds the launch's ray count
//                          into the handle's total
//   rec_place_kernel       per record slot: q -> place, copy the measurement
// All of them, and the reduction, do NOTHING when the launch ran out of record slots (*rec_count > capacity): the host
// then repeats the launch with a larger buffer and the framebuffer and ray total have not been touched.
__device__ __forceinline__ uint32_t PixelBits(const uint32_t* __restrict__ flags, uint32_t q0, uint32_t q1) {   // set bits in [q0, q1)
  if (q0 == q1) return 0u;
  const uint32_t w0 = q0 >> 5, w1 = (q1 - 1u) >> 5;
  const uint32_t lo = 0xffffffffu << (q0 & 31u), hi = 0xffffffffu >> (31u - ((q1 - 1u) & 31u));
  if (w0 == w1) return static_cast<uint32_t>(__popc(flags[w0] & lo & hi));
  uint32_t c = static_cast<uint32_t>(__popc(flags[w0] & lo)) + static_cast<uint32_t>(__popc(flags[w1] & hi));
  for (uint32_t wd = w0 + 1u; wd < w1; ++wd) c += static_cast<uint32_t>(__popc(flags[wd]));
  return c;
}
__global__ void rec_rank_kernel(const uint32_t* __restrict__ flags, const uint32_t* __restrict__ touched, uint32_t n_pixels, uint32_t n_samples,
                                uint32_t* __restrict__ excl, uint32_t* __restrict__ block_sum) {
  __shared__ uint32_t part[256];
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  // only a touched pixel's bits are read: on the Cornell box that is 2e-2 of the pixels, and the bitmap is 128 MB per launch
  const bool any = p < n_pixels && ((touched[p >> 5] >> (p & 31u)) & 1u) != 0u;
  const uint32_t c = any ? PixelBits(flags, p * n_samples, p * n_samples + n_samples) : 0u;
  part[threadIdx.x] = c;
  __syncthreads();
  for (uint32_t off = 1; off < 256u; off <<= 1) {             // Hillis-Steele inclusive scan
    const uint32_t v = threadIdx.x >= off ? part[threadIdx.x - off] : 0u;
    __syncthreads();
    part[threadIdx.x] += v;
    __syncthreads();
  }
  if (p < n_pixels) excl[p] = part[threadIdx.x] - c;
  if (threadIdx.x == 255u) block_sum[blockIdx.x] = part[255];
}
__global__ void rec_scan_blocks_kernel(uint32_t* __restrict__ block_sum, uint32_t n_blocks, const unsigned int* __restrict__ rec_count, uint32_t rec_capacity,
                                       unsigned long long* __restrict__ ray_total, unsigned long long* __restrict__ ray_launch) {
  __shared__ uint32_t part[1024];
  __shared__ uint32_t carry;
  if (threadIdx.x == 0) {
    carry = 0u;
    if (*rec_count <= rec_capacity) *ray_total += *ray_launch;            // the launch stands: its rays count
  }
  __syncthreads();
  for (uint32_t base = 0; base < n_blocks; base += 1024u) {
    const uint32_t i = base + threadIdx.x;
    const uint32_t c = i < n_blocks ? block_sum[i] : 0u;
    part[threadIdx.x] = c;
    __syncthreads();
    for (uint32_t off = 1; off < 1024u; off <<= 1) {
      const uint32_t v = threadIdx.x >= off ? part[threadIdx.x - off] : 0u;
      __syncthreads();
      part[threadIdx.x] += v;
      __syncthreads();
    }
    if (i < n_blocks) block_sum[i] = carry + part[threadIdx.x] - c;
    __syncthreads();
    if (threadIdx.x == 1023u) carry += part[1023];
    __syncthreads();
  }
}
__global__ void rec_place_kernel(const uint4* __restrict__ records, const unsigned int* __restrict__ rec_count, uint32_t rec_capacity, const uint32_t* __restrict__ flags,
                                 const uint32_t* __restrict__ excl, const uint32_t* __restrict__ block_sum, uint32_t n_samples, ExactDiv div_samples, float* __restrict__ sorted) {
  const uint32_t n = *rec_count;
  if (n > rec_capacity) return;                               // out of slots: the launch is repeated
  for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x) {
    const uint4 r = records[k];
    if (r.x == AMBER_REC_UNUSED) continue;
    const uint32_t p = Quotient(div_samples, r.x);
    const uint32_t at = block_sum[p >> 8] + excl[p] + PixelBits(flags, p * n_samples, r.x);
    float* s = sorted + static_cast<size_t>(at) * 3u;
    s[0] = __uint_as_float(r.y); s[1] = __uint_as_float(r.z); s[2] = __uint_as_float(r.w);
  }
}

// fb[pixel] += the measurements of the launch's paths, in the order of the numerical contract: within a chunk of
// AMBER_ACCUM_CHUNK consecutive samples (counted from the launch's first sample) a sequential binary32 sum, chunk sums
// added to the framebuffer value in chunk order.  Only paths whose bit is set contribute a term; every other term is +0,
// and both the chunk sum (starts at +0) and the framebuffer value (cleared to +0) can never be -0, so leaving the +0
// terms out changes no bit.  One thread per band pixel; its measurements are sorted[base ..] in sample order.
__global__ void reduce_flagged_kernel(float* __restrict__ fb, uint32_t* __restrict__ flags, const uint32_t* __restrict__ touched, const float* __restrict__ sorted,
                                      const uint32_t* __restrict__ excl, const uint32_t* __restrict__ block_sum, const unsigned int* __restrict__ rec_count,
                                      uint32_t rec_capacity, uint32_t n_pixels, uint32_t n_samples) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pixels) return;
  if (*rec_count > rec_capacity) return;                       // out of slots: the launch is repeated
  if (((touched[p >> 5] >> (p & 31u)) & 1u) == 0u) return;     // no path of this pixel carried a measurement
  const uint32_t q0 = p * n_samples;                           // n_pixels * n_samples < 2^32 (RenderPassPaths splits launches)
  const float* m = sorted + static_cast<size_t>(block_sum[p >> 8] + excl[p]) * 3u;
  float v0 = fb[3u * p], v1 = fb[3u * p + 1u], v2 = fb[3u * p + 2u];
  if ((n_samples & 31u) == 0u && (32u % AMBER_ACCUM_CHUNK) == 0u) {
    // The pixel owns whole words: walk the SET bits only (a touched pixel of the Cornell box has one or two among 1024) -- the same
    // sums in the same order: samples of a chunk in order from +0, chunk sums onto the pixel in chunk order.  The bit-by-bit loop
    // below took 0.135 ms per launch of a rank's share of config 2 on 8 GPUs, 2 % of its step.  Consumed words are cleared on the
    // way, so that the bitmap is all zero again for the next launch and the host does not have to clear 128 MB per launch.
    const uint32_t w0 = q0 >> 5, nw = n_samples >> 5;
    constexpr uint32_t kChunkMask = AMBER_ACCUM_CHUNK >= 32u ? 0xffffffffu : ((1u << (AMBER_ACCUM_CHUNK & 31u)) - 1u);
    auto consume = [&](uint32_t wd, uint32_t bits) {
      if (bits == 0u) return;
      flags[w0 + wd] = 0u;
      for (uint32_t sh = 0; sh < 32u; sh += AMBER_ACCUM_CHUNK) {
        uint32_t b = (bits >> sh) & kChunkMask;
        if (b == 0u) continue;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f;
        while (b) { b &= b - 1u; s0 = s0 + m[0]; s1 = s1 + m[1]; s2 = s2 + m[2]; m += 3; }
        v0 = v0 + s0; v1 = v1 + s1; v2 = v2 + s2;
      }
    };
    uint32_t wd = 0;
    if ((w0 & 3u) == 0u) {                                     // four words per load: a pixel's 1024 samples are 8 loads issued together, not 32 in turn
      for (; wd + 16u <= nw; wd += 16u) {
        const uint4* f4 = reinterpret_cast<const uint4*>(flags + w0 + wd);
        const uint4 a0 = f4[0], a1 = f4[1], a2 = f4[2], a3 = f4[3];
        if ((a0.x | a0.y | a0.z | a0.w | a1.x | a1.y | a1.z | a1.w | a2.x | a2.y | a2.z | a2.w | a3.x | a3.y | a3.z | a3.w) == 0u) continue;
        consume(wd + 0u, a0.x); consume(wd + 1u, a0.y); consume(wd + 2u, a0.z); consume(wd + 3u, a0.w);
        consume(wd + 4u, a1.x); consume(wd + 5u, a1.y); consume(wd + 6u, a1.z); consume(wd + 7u, a1.w);
        consume(wd + 8u, a2.x); consume(wd + 9u, a2.y); consume(wd + 10u, a2.z); consume(wd + 11u, a2.w);
        consume(wd + 12u, a3.x); consume(wd + 13u, a3.y); consume(wd + 14u, a3.z); consume(wd + 15u, a3.w);
      }
    }
    for (; wd < nw; ++wd) consume(wd, flags[w0 + wd]);
    fb[3u * p] = v0; fb[3u * p + 1u] = v1; fb[3u * p + 2u] = v2;
    return;
  }
  for (uint32_t c0 = 0; c0 < n_samples; c0 += AMBER_ACCUM_CHUNK) {
    const uint32_t c1 = c0 + AMBER_ACCUM_CHUNK < n_samples ? c0 + AMBER_ACCUM_CHUNK : n_samples;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
    bool hit = false;
    for (uint32_t k = c0; k < c1; ++k) {
      const uint32_t q = q0 + k;
      if ((flags[q >> 5] >> (q & 31u)) & 1u) {
        s0 = s0 + m[0]; s1 = s1 + m[1]; s2 = s2 + m[2];
        m += 3;
        hit = true;
      }
    }
    if (hit) { v0 = v0 + s0; v1 = v1 + s1; v2 = v2 + s2; }
  }
  fb[3u * p] = v0; fb[3u * p + 1u] = v1; fb[3u * p + 2u] = v2;
  // (a pixel that does not own whole words leaves its bits: the host clears the bitmap before the next launch, LaunchPaths)
}

// ---- per-pixel candidate masks of the primary rays (two-phase engine) ---------------------------------------------------------
// All eye rays of pixel (px, py) lie in one thin BEAM: every ray starts in the aperture (thin lens: lens_thin.cc:70-107; inside the
// rectangle A that bounds the blades in the lens plane) and passes through the image of its jittered sensor point on the focal plane
// (inside the rectangle F: the image of the pixel; the direction is Normalize(-fd/sd * sensor_point - aperture_point), which does not
// depend on where in the aperture the ray starts), or starts at the pinhole (A = one point).  The mask of a pixel has a bit for every
// object of the filter program that SOME ray of that beam can hit -- the closest hit of every one of the pixel's eye rays, whatever its
// sample index, is then found among the mask's objects, and a primary round needs no Phase A.  Conservative by construction:
//  * plane records: the hit points of the beam on a plane form a convex region whenever the plane cuts neither A nor F and no ray is
//    close to parallel to it (before the focal plane the beam is conv(A u F), behind it F + cone(F - A): both convex, and a plane that
//    separates or misses A and F meets them only in edges that lie on CORNER rays a_i -> f_j); barycentric coordinates are affine on
//    the plane, so each one's maximum over the region is attained on one of the 16 corner rays.  A triangle is dropped only if one of
//    its three coordinates stays below -tolerance on all 16, or if every corner ray meets the plane behind its origin.  Planes that cut
//    A or F, or that a corner ray grazes, keep all their triangles.
//  * spheres: kept unless the central ray passes the centre farther away than the radius plus the beam's half width there.
//  * the same tolerances as Phase A (DevPlane.kt / ktol scaled by the largest 1 / |n.d| of the corner rays) plus a position slack of
//    1e-5 of the model size for the difference between a binary32 eye ray and the ideal one; A is inflated by 1e-3 of its size, F by
//    2 % of the pixel.  Aperture blades are NOT part of the mask: a ray's own blade and, on blade boundaries, its neighbours are added
//    per ray where the path starts.
// Double precision throughout, once per handle (the mask depends on scene and sensor only).  Since round 5 one mask serves a BLOCK of 4 x 4 band
// pixels (F = the image of the whole block): a pixel's beam is as wide as the aperture nearly everywhere, so sixteen neighbours share their
// candidates -- config 2: 2.10 candidates per pixel instead of 1.97, the render kernel unchanged (tools/pixel_mask_blocks.py,
// profiles/r05_pixel_mask_blocks.txt), and the kernel takes 0.07 ms instead of 1.0.
struct PixelMaskArgs {
  double ap[4][3];                // corners of the aperture's bounding rectangle in the lens plane (inflated), RELATIVE TO THE FILTER CENTRE; pinhole: the origin
  double inv_w, inv_h;            // 1 / sensor width, height (pixels)
  double focal_scale;             // thin lens: -focus_distance / sensor_distance; pinhole: -(8 reach + 1) / sensor_distance (a point far along the ray)
  uint32_t planes_cut_a;          // bit i: plane i of the filter program passes within the slack of the aperture rectangle (the same for every pixel: tested on the host)
  uint32_t row_begin, stripe_rows, stripe_period, n_pixels;
  uint32_t block;                 // a mask serves a block of block x block band pixels (4, or 1 when the stripes are not whole blocks): the beam of a pixel's eye rays is as
  uint32_t blocks_x, n_blocks;    // wide as the APERTURE nearly everywhere, so 16 pixels share their candidates at a sixteenth of the work (round 5: 1.0 -> < 0.1 ms)
  uint32_t local_rows;
};
// SIXTEEN LANES PER BLOCK OF PIXELS, lane k = corner ray a_(k >> 2) -> f_(k & 3) (round 4: per pixel).  Round 3's kernel ran one thread per pixel with the 16
// directions and the 16 plane points in per-thread arrays: 128 VGPRs, 1 728 B of scratch, 3.7 ms per config-2 handle -- more than the first
// 64 samples per pixel of the render it prepares.  Here a lane keeps ITS ray (3 + 3 doubles); "on all 16 corner rays" is a vote
// (__ballot, masked to the pixel's 16 lanes), the maxima a plane needs are butterfly reductions over the 16 lanes, the aperture
// corners are wave-uniform kernel arguments (SGPRs), and a lane forms only its own corner of F.  Same tests as before with two
// differences, both towards keeping a candidate: a NaN coordinate keeps its triangle (fmax used to skip it), and the gradient norms
// of a record's affine rows are bounded by their 1-norms (no square roots).
__device__ __forceinline__ double Max16(double x) {               // maximum over the 16 lanes of a pixel (lanes 16 g .. 16 g + 15)
#pragma unroll
  for (int m = 1; m < 16; m <<= 1) x = fmax(x, __shfl_xor(x, m, 16));
  return x;
}
__global__ void __launch_bounds__(256) pixel_mask_kernel(const DevScene sc, const PixelMaskArgs pm, uint32_t* __restrict__ out) {
  const uint32_t b_raw = blockIdx.x * 16u + (threadIdx.x >> 4), k = threadIdx.x & 15u;     // 16 pixel blocks per workgroup of 256
  const bool live = b_raw < pm.n_blocks;
  const uint32_t b = live ? b_raw : pm.n_blocks - 1u;              // whole groups of 16 lanes stay active (votes, shuffles); only `live` groups store
  const uint32_t shift = threadIdx.x & 48u;                        // position of the block's 16 lanes in the wave's 64-bit votes
  auto all16 = [&](bool c) { return ((__ballot(c) >> shift) & 0xffffull) == 0xffffull; };
  auto any16 = [&](bool c) { return ((__ballot(c) >> shift) & 0xffffull) != 0ull; };
  const uint32_t brow = b / pm.blocks_x, lrow = brow * pm.block, px = (b - brow * pm.blocks_x) * pm.block;   // first band row and column of the block
  const uint32_t py = pm.row_begin + (pm.stripe_rows ? (lrow / pm.stripe_rows) * pm.stripe_period + lrow % pm.stripe_rows : lrow);   // (a block never straddles two stripes)
  const double span = static_cast<double>(pm.block);              // the block covers pixels [px, px + span) x [py, py + span)
  const DevLens& L = *sc.lens;
  const double cx = sc.fp_center[0], cy = sc.fp_center[1], cz = sc.fp_center[2];
  const double reach = sc.fp_reach;
  // Position slack (world units): 1e-5 of the model size, plus the binary32 grid of WORLD coordinates -- an eye ray is defined by the
  // reference's binary32 arithmetic on world coordinates (blade point, aperture_point = local (point - lens origin), ...), so in a scene
  // that lies 1e4 of its size from the world origin (the fuzzer's --scaled scenes) the actual ray is a few 1e-4 of the scene away from
  // the ideal one.  The same amount widens A (host) and F (below).
  const double world_mag = fmax(fmax(fabs(cx), fmax(fabs(cy), fabs(cz))) + reach, fmax(fabs(double(L.origin[0])), fmax(fabs(double(L.origin[1])), fabs(double(L.origin[2])))));
  const double slack = 1e-5 * reach + 32.0 * 5.9604644775390625e-08 * world_mag;
  // this lane's corner ray: from a_ = A[k >> 2] towards fk = F[k & 3], the corner (k & 1, k & 2) of the pixel's image on the focal plane
  const uint32_t ki = k >> 2, kj = k & 3u;
  double a_[3], fk[3];
  for (int c = 0; c < 3; c++) a_[c] = ki == 0u ? pm.ap[0][c] : (ki == 1u ? pm.ap[1][c] : (ki == 2u ? pm.ap[2][c] : pm.ap[3][c]));
  {
    // (an IEEE binary64 division is 64 SIMD cycles on gfx950: the wave-uniform quotients are kernel arguments)
    const double ux = (static_cast<double>(px) + ((kj & 1u) ? span + 0.02 : -0.02)) * pm.inv_w;
    const double uy = (static_cast<double>(py) + ((kj & 2u) ? span + 0.02 : -0.02)) * pm.inv_h;
    const double sx = (ux - 0.5) * sc.sensor.sw, sy = (uy - 0.5) * sc.sensor.sh, sz = L.sensor_distance;
    // thin lens: the point of the focal plane all rays of this sensor point pass through; pinhole: a point far along the ray
    const double kk = pm.focal_scale;
    const double fl[3] = {kk * sx + ((kk * ((kj & 1u) ? 1.0 : -1.0) >= 0) ? slack : -slack), kk * sy + ((kk * ((kj & 2u) ? 1.0 : -1.0) >= 0) ? slack : -slack), kk * sz};   // outwards by the slack
    for (int c = 0; c < 3; c++) fk[c] = L.origin[c] + L.global_[3 * c] * fl[0] + L.global_[3 * c + 1] * fl[1] + L.global_[3 * c + 2] * fl[2];
    fk[0] -= cx; fk[1] -= cy; fk[2] -= cz;
  }
  double Dk[3];
  {
    const double v[3] = {fk[0] - a_[0], fk[1] - a_[1], fk[2] - a_[2]};
    const double inv_l = 1.0 / sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    for (int c = 0; c < 3; c++) Dk[c] = v[c] * inv_l;                  // unit up to two roundings: far inside every tolerance below
  }
  uint32_t mask = 0u, bit = 1u;
  const DevPlane* pl = sc.planes;
  const DevTriFilter* tr = sc.tri_filters;
  for (uint32_t pi = 0; pi < sc.n_planes; ++pi, ++pl) {
    const double n[3] = {pl->n[0], pl->n[1], pl->n[2]}, d0 = pl->d0;
    const uint32_t nt = pl->n_tris & 0x7fffffffu, np = pl->n_pairs;
    // does the plane cut A or F?  (all corners strictly on one side, with the slack; the lanes of a pixel hold every corner of both)
    bool all = false;
    {
      const double sf = n[0] * fk[0] + n[1] * fk[1] + n[2] * fk[2] - d0;
      if (!(all16(sf > 10.0 * slack) || all16(sf < -10.0 * slack))) all = true;
      if ((pm.planes_cut_a >> (pi & 31u)) & 1u) all = true;            // the aperture's side of the same question: pixel-independent
    }
    const double nd = n[0] * Dk[0] + n[1] * Dk[1] + n[2] * Dk[2];
    if (any16(!(fabs(nd) >= 4.0 * AMBER_GRAZING))) all = true;       // a corner ray grazes the plane (or NaN): no convexity argument
    if (any16(nd > 0) && any16(!(nd > 0))) all = true;                // corner rays meet the plane from both sides
    if (all) {                                                         // (uniform over the pixel's 16 lanes)
      for (uint32_t r = 0; r < 2u * np + nt; r++, bit <<= 1) mask |= bit;
      tr += np + nt;
      continue;
    }
    const double inv_nd = 1.0 / nd;
    const double t = (d0 - (n[0] * a_[0] + n[1] * a_[1] + n[2] * a_[2])) * inv_nd;
    const double P[3] = {a_[0] + t * Dk[0], a_[1] + t * Dk[1], a_[2] + t * Dk[2]};
    const double rho_max = Max16(fabs(inv_nd)) * 1.000001, t_max = Max16(t);
    if (t_max < static_cast<double>(AMBER_KEPS) - static_cast<double>(pl->kt) * rho_max - slack) {   // every ray meets the plane behind its origin
      bit <<= (2u * np + nt); tr += np + nt;
      continue;
    }
    const double ptol = static_cast<double>(pl->ktol) * rho_max;
    for (uint32_t r = 0; r < np + nt; ++r, ++tr) {
      // |gradient| of the two affine rows, bounded by their 1-norms
      const double g0 = fabs(double(tr->c[0][0])) + fabs(double(tr->c[1][0])) + fabs(double(tr->c[2][0]));
      const double g1 = fabs(double(tr->c[0][1])) + fabs(double(tr->c[1][1])) + fabs(double(tr->c[2][1]));
      const double tol = ptol + (g0 + g1) * slack + 1e-6;               // barycentric units
      const double u = tr->c[0][0] * P[0] + tr->c[1][0] * P[1] + tr->c[2][0] * P[2] + tr->c[3][0];
      const double v = tr->c[0][1] * P[0] + tr->c[1][1] * P[1] + tr->c[2][1] * P[2] + tr->c[3][1];
      // a triangle is dropped only if ONE of its coordinates is below -tol on all 16 corner rays.
      // pair record: (u, v) = (beta, alpha) of the first triangle; the second one's coordinates are (-beta, 1 - alpha, beta + alpha)
      const bool drop1 = all16(u < -tol) || all16(v < -tol) || all16(1.0 - u - v < -tol);   // a NaN coordinate votes "keep"
      mask |= drop1 ? 0u : bit; bit <<= 1;
      if (r < np) {
        const bool drop2 = all16(-u < -tol) || all16(1.0 - v < -tol) || all16(u + v < -tol);
        mask |= drop2 ? 0u : bit; bit <<= 1;
      }
    }
  }
  // spheres: the central ray against the sphere inflated by the beam's half width at the sphere's depth
  if (sc.n_sphere_filters) {
    double ac[3] = {0, 0, 0}, fc[3] = {0, 0, 0};
    for (int i = 0; i < 4; i++) for (int c = 0; c < 3; c++) { ac[c] += 0.25 * pm.ap[i][c]; fc[c] += 0.25 * __shfl(fk[c], i, 16); }   // lanes 0..3 of the pixel hold F[0..3]
    double dc[3] = {fc[0] - ac[0], fc[1] - ac[1], fc[2] - ac[2]};
    const double inv_lc = 1.0 / sqrt(dc[0] * dc[0] + dc[1] * dc[1] + dc[2] * dc[2]);
    for (int c = 0; c < 3; c++) dc[c] *= inv_lc;
    const double inv_dd = 1.0 / (Dk[0] * dc[0] + Dk[1] * dc[1] + Dk[2] * dc[2]);
    const double off = (a_[0] - ac[0]) * dc[0] + (a_[1] - ac[1]) * dc[1] + (a_[2] - ac[2]) * dc[2];
    auto half_width = [&](double tau) {                                // largest distance of a corner ray from the central one in the plane at depth tau
      const double s_ = (tau - off) * inv_dd;
      double e2 = 0;
      for (int c = 0; c < 3; c++) { const double e = a_[c] + s_ * Dk[c] - (ac[c] + tau * dc[c]); e2 += e * e; }
      return sqrt(Max16(fmax(0.0, e2)));                               // (fmax(0, NaN) = 0: a NaN ray is skipped, as the serial loop's fmax did)
    };
    const DevSphereFilter* sp = sc.sphere_filters;
    for (uint32_t r_ = 0; r_ < sc.n_sphere_filters; ++r_, ++sp, bit <<= 1) {
      const double co[3] = {sp->c[0] - ac[0], sp->c[1] - ac[1], sp->c[2] - ac[2]};
      const double r = sqrt(static_cast<double>(sp->r2)) * 1.001 + slack;
      const double tau = co[0] * dc[0] + co[1] * dc[1] + co[2] * dc[2];
      const double d2 = co[0] * co[0] + co[1] * co[1] + co[2] * co[2] - tau * tau;
      const double hw = fmax(half_width(tau - r), half_width(tau + r));
      const double lim = (r + hw) * 1.02 + slack;
      const bool miss = d2 > lim * lim;                                  // NaN -> keep
      mask |= miss ? 0u : bit;
    }
  }
  // lane k stores the block's mask for its pixel (k % block, k / block) of the block, where the band has one
  const uint32_t sx = px + k % pm.block, sr = lrow + k / pm.block;
  if (live && k < pm.block * pm.block && sx < sc.sensor.w && sr < pm.local_rows) out[sr * sc.sensor.w + sx] = mask & ~sc.blade_mask;
}

