/*
 * amber_hip_lab.h -- entry points of the LAB build (libamber_hip_lab.so = the product's sources compiled with -DAMBER_LAB).
 *
 * Not part of the product: libamber_hip.so exports none of these.  The lab library contains everything the product does -- the same kernels
 * from the same files -- plus (1) the known-answer kernels through which tests/ compare single stages with the oracle, (2) the signature
 * instantiations of the product kernels (per-path hashes of hit objects and distances), (3) the schedulers that were built, measured slower
 * and kept provably equal: engine WAVEFRONT (wavefront.inc: SoA ray queues in HBM, one launch per bounce, ballot / prefix-sum compaction --
 * the north star's formulation), AMBER_PT_FLAG_BVH_POOL (bvh_pool.inc) and the traversal-only kernel (bvh_stream.inc).
 */
#ifndef AMBER_HIP_LAB_H
#define AMBER_HIP_LAB_H

#include "amber_hip.h"

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)   /* the libraries are built with -fvisibility=hidden: what these headers declare is what they export */

/* ---- known-answer entry points (same device functions as the render kernels) --------------
 * Used by tests/ to compare individual stages against the oracle.  All buffers are HOST
 * pointers; n items; synchronous. */
/* closest hit: out_object = object index or -1 */
int amber_hip_kat_cast(amber_hip_pt*, uint32_t n, const float* origins /*n*3*/, const float* dirs /*n*3*/,
                       int32_t* out_object, float* out_t, float* out_pos /*n*3*/, float* out_normal /*n*3*/);
/* Phase A of the two-phase closest hit on its own: the candidate mask of every ray in every group of the handle's filter program (one group for
 * up to 32 objects, else up to four), out_mask[i * n_groups + g], bit k = program slot k of group g, through the function the render kernels call;
 * no exact test runs.  axis_loops != 0: the axis slabs run in their reduced form (the product's default); 0: the general slab loop runs the same
 * records.  The two masks are equal bit for bit.  Phase A does not read a ray's origin slot (the self trip that follows it does), so none is
 * passed.  mask_capacity: words behind out_mask, at least n * n_groups (4 n always suffices); *out_n_groups (may be null) is set either way.
 * AMBER_EINVAL for a handle of another engine. */
int amber_hip_kat_phase_a(amber_hip_pt*, uint32_t n, const float* origins /*n*3*/, const float* dirs /*n*3*/, int axis_loops,
                          uint32_t* out_mask, uint64_t mask_capacity, uint32_t* out_n_groups);
/* material sampling with a per-item XorShift state; returns dir_in, weight and the advanced state.
 * material[i]: the material index, | 0x80000000 for SampleImportance (the light-tracing side) instead of SampleLight */
int amber_hip_kat_sample(amber_hip_pt*, uint32_t n, const uint32_t* material /*n*/, const float* normals,
                         const float* dirs_out, uint64_t* rng_state /*n, in/out*/, float* out_dir_in, float* out_weight);
/* eye rays for (pixel index, sample) pairs: out = origin[3] dir[3] weight */
int amber_hip_kat_eye(amber_hip_pt*, uint32_t n, const uint32_t* pixel, const uint32_t* sample, float* out7);
/* The start of a light path (GenerateLightRay: the light chosen by cumulative power, a point of its surface, a cosine-weighted direction,
 * weight = irradiance / pdf_area) exactly as the light-tracing kernel calls it, item i from the XorShift state rng_state[i]; the state after
 * the call is written back, so the number of draws shows.  out_light[i] = the position of the chosen light in the handle's light table
 * (AmberFlatScene.lights order; amber_host_kat_scene_lights gives that table for a host scene).  AMBER_EINVAL, without a launch, for a handle
 * whose scene has no lights or whose lights are stale. */
int amber_hip_kat_light_ray(amber_hip_pt*, uint32_t n, uint64_t* rng_state /*n, in/out*/, float* out_origin /*n*3*/, float* out_dir /*n*3*/,
                            float* out_weight /*n*3*/, uint32_t* out_light /*n*/);
/* Lens::Response of Ray(position[i], direction_out[i]) through LensResponse, the inverse camera of the light-tracing kernel (and the
 * arithmetic amber_hip_pt_temporal's reprojection repeats): out_reached[i] = 1 when the ray reaches the sensor, then out_pixel[i] = x + y * width
 * and out_value[i] = the response; both are written as 0 where out_reached[i] = 0. */
int amber_hip_kat_lens_response(amber_hip_pt*, uint32_t n, const float* position /*n*3*/, const float* direction_out /*n*3*/,
                                uint32_t* out_reached /*n*/, uint32_t* out_pixel /*n*/, float* out_value /*n*/);
/* Radiance() of material[i] (an index into the handle's material table; AMBER_EINVAL when out of range) seen from dir_out at a surface with
 * the given normal: the emitter's rho where dir_out . normal > 0, else 0. */
int amber_hip_kat_radiance(amber_hip_pt*, uint32_t n, const uint32_t* material /*n*/, const float* normals /*n*3*/, const float* dirs_out /*n*3*/,
                           float* out /*n*3*/);
/* The light table Scene::Flatten() hands to amber_hip_pt_create for this host scene (no device needed): call with lights = NULL for the
 * count, then with a buffer of *n_lights records. */
struct amber_host_scene;
int amber_host_kat_scene_lights(const struct amber_host_scene*, AmberFlatLight* lights, uint32_t* n_lights);
/* full per-path trace: for item i writes up to max_bounces records of
 * {object(int32 as float bits), t, pos[3], weight[3], measurement[3]} (11 x 4 bytes) and the cast count */
int amber_hip_kat_trace(amber_hip_pt*, uint32_t n, const uint32_t* pixel, const uint32_t* sample,
                        uint32_t max_bounces, uint32_t* out_records /*n*max_bounces*11*/, uint32_t* out_casts /*n*/);
/* Path signatures of the handle's rows for samples [first_sample, first_sample + n_samples): out[(band pixel * n_samples) + k]
 * = FNV-1a-32 over the object index of every cast of that path (0xffffffff = miss) in the low word -- two paths have
 * DIVERGED iff these differ -- and FNV-1a-32 over the bits of every hit distance in the high word.  out: host pointer,
 * local_rows * width * n_samples entries. */
int amber_hip_kat_signatures(amber_hip_pt*, uint32_t first_sample, uint32_t n_samples, uint64_t* out);
/* The same signatures from the PRODUCT render kernel (pt_megakernel / pt_bvh_megakernel / pt_bvh_pool_kernel instantiated with the hashing
 * switched on: identical scheduling, work queue, ray pool and device functions), so that the kernel that renders -- not
 * only the per-thread known-answer kernel above -- is compared with the oracle path by path
 * (algorithm_pt.cc:125-160).  Same layout as amber_hip_kat_signatures.  Leaves the framebuffer and the ray count untouched. */
int amber_hip_pt_signatures(amber_hip_pt*, uint32_t first_sample, uint32_t n_samples, uint64_t* out);
/* Engine BVH's traversal in a kernel of its own (no shading, no path state): closest hits of n rays, `waves` resident waves per SIMD
 * (4, 5, 6 or 8), idle lanes refilled once `refill_min` of a wave's 64 lanes are idle; out_t = NaN for a miss; best_ms = the fastest of
 * `repeats` launches; out_rounds (may be NULL): per ray, the number of wave rounds it was in flight for.  A measurement (DESIGN.md
 * section 5) that doubles as a known-answer test of the traversal. */
int amber_hip_kat_traversal_rate(amber_hip_pt*, uint32_t n, const float* origins, const float* dirs, uint32_t waves, uint32_t refill_min,
                                 uint32_t repeats, float* out_t, int32_t* out_object, double* best_ms, uint32_t* out_rounds);
/* Two-phase engine: the per-pixel candidate masks of the primary rays (pixel_mask_kernel, one mask per 4 x 4 block of pixels; for scenes of more than 32
 * objects the masks describe group 0 -- the aperture blades and the first 26 objects).
 * out_mask: one word per band pixel, bit k = the object in filter-program slot k can be hit by SOME eye ray of the pixel (aperture blades
 * excluded: they are added per ray).  out_slot_of_object: n_objects entries, the slot of every scene object (0xffffffff: none).
 * out_always_mask: the slots that are candidates of EVERY ray whatever the pixel (objects the filter program has no record for, and the
 * aperture blades, which a primary ray adds itself).  kernel_ms: duration of the mask kernel (create has run it once; asking for the duration runs it again between two events).
 * Any pointer may be NULL. */
int amber_hip_kat_pixel_masks(amber_hip_pt*, uint32_t* out_mask, uint32_t* out_slot_of_object, uint32_t* out_always_mask, double* kernel_ms);
/* Engine BVH's tree as the device holds it, built by the host or by the device (AMBER_PT_FLAG_DEVICE_BUILD): copies up to node_capacity nodes
 * (8 words each: six plane words min | max << 16 for left x y z, right x y z, then the left and right child references) and up to
 * prim_capacity entries of the leaf order (leaf slot -> object index); info always receives the sizes and the scalars.  nodes / prims may be NULL. */
typedef struct { uint32_t n_nodes, n_prims; int32_t root; uint32_t depth; float gmin[3], step[3], reach[3]; } AmberBvhDump;
int amber_hip_kat_bvh_dump(amber_hip_pt*, uint32_t* nodes, uint32_t node_capacity, uint32_t* prims, uint32_t prim_capacity, AmberBvhDump* info);
/* amber_hip_lt_render_pass's device path on the caller's records: uploads the n records (host memory) in the given order into the handle's splat
 * buffer -- growing it as a launch that ran out of slots would -- and runs exactly the ordering and the ordered sum of lt_accumulate.inc into the
 * framebuffer; `path` is sorted with all its 32 bits.  Real scenes splat rarely (the aperture catches about 1e-4 of the light paths): only this hook
 * puts the sort and the sum under load.  Synchronous.  AMBER_EINVAL for a pixel >= width * height or a banded handle; n == 0 changes nothing. */
int amber_hip_kat_lt_accumulate(amber_hip_pt*, const AmberSplat* records /* host */, uint32_t n);
/* "Accumulation without owners"  on the caller's records: ONE path launch over n_samples samples of the handle's band pixels, added
 * to the handle's framebuffer, exactly as amber_hip_pt_render_pass enqueues it -- the same bitmap, rank / scan / place / reduce kernels, the same host
 * state (the bitmap that is cleared only when a launch left it dirty, the record buffer, the repeat of a launch that ran out of slots) -- except that
 * the records come from a kernel that feeds q[i], rgb[i] (host arrays, n_items entries) to the product's EmitRecords: wave w of n_waves takes the trips
 * w, w + n_waves, ... of 64 consecutive items (the last trip padded with lanes that emit nothing) and calls CloseRecords after its last one, so the caller
 * decides how many lanes emit per trip.  q[i] = path index = band pixel * n_samples + sample; 0xffffffff: lane i emits nothing (its path ended with
 * +0).  Real scenes leave most branches of the reduction cold (the Cornell box sets one or two bits per touched pixel); only this hook puts chosen bit
 * patterns, record counts and slot boundaries under them.  tests/path_accumulate_reference.py restates the sum it must give.
 * rec_capacity: the record slots the launch sees -- 0: a slot per item plus the slack every render launch has; otherwise exactly this many (the buffer
 * grows to it; a value below what the handle's buffer already holds is refused, so use a fresh handle for a small one).  A launch that runs out is
 * repeated with a larger buffer by the product's own code.  `rays` is what the launch adds to its ray counter: it reaches the handle's total once,
 * with the launch that stands.
 * AMBER_EINVAL, before anything is enqueued: n_samples == 0, n_waves == 0, band pixels * n_samples >= 2^32, a q other than the marker that is
 * >= band pixels * n_samples or occurs twice, a non-zero rec_capacity below the buffer's.  n_items == 0 is a launch without records.  Any engine.
 * Synchronous: the launch has been settled and the stream waited for.  info (may be NULL): launches and repeats of this call, the record counter of the
 * launch that stood, the non-zero words in the bitmap's used range afterwards, and whether the host holds the bitmap for dirty. */
typedef struct { uint32_t n_launches, n_repeats, rec_count, flag_words_set, flags_dirty; } AmberAccumulateInfo;
int amber_hip_kat_accumulate(amber_hip_pt*, uint32_t n_samples, const uint32_t* q /* host, n_items */, const float* rgb /* host, n_items * 3 */, uint32_t n_items,
                             uint32_t n_waves, uint32_t rec_capacity, uint64_t rays, AmberAccumulateInfo* info);
/* The scout's verdict (csrc/hip/pt_megakernel.inc, AMBER_KERNEL_SCOUT; scout_bound.h): one launch of the handle's weight-free kernel over samples
 * [first_sample, first_sample + n_samples) of the band, WITHOUT the replay and without the reduction, and the launch's bitmap as the scout left it --
 * bit q = band pixel * n_samples + sample offset is set iff the scout flagged path q (it ends on a light whose Radiance is not +0, or it is suspect).
 * out_flags: host, n_words >= ceil(band pixels * n_samples / 32) words.  Nothing reaches the framebuffer or the ray total.  out_scouts (may be NULL):
 * 1 if the handle scouts, 0 if it renders with the full kernel (then nothing is launched and out_flags is zeroed); out_bound0 (may be NULL): the host's bound of
 * log2 |eye weight| for the handle's lens in sixteenths of a bit, the value every path's bound starts from.  AMBER_EINVAL: n_samples == 0, more
 * paths than one launch takes, too few words.  Synchronous. */
int amber_hip_kat_scout_flags(amber_hip_pt*, uint32_t first_sample, uint32_t n_samples, uint32_t* out_flags, uint64_t n_words, uint32_t* out_scouts, uint32_t* out_bound0);
/* Measurement: the first call switches on the timing of that device path with events (every accumulation then waits for the stream); every call
 * returns the milliseconds spent ordering (keys, sorts, gather) and summing since the previous call.  Either pointer may be NULL. */
int amber_hip_kat_lt_stage_ms(amber_hip_pt*, double* sort_ms, double* sum_ms);
/* the same for amber_hip_lt_trace_photons: hipEvent milliseconds of its trace kernels, its sorts (keys included) and its gathers since the previous call;
 * the first call switches the timing on (every launch's gather is then waited for) */
int amber_hip_kat_photon_stage_ms(amber_hip_pt*, double* trace_ms, double* sort_ms, double* gather_ms);
/* the same for the photon map: hipEvent milliseconds of amber_hip_pm_build (first kernel to last; the wait for the bounds lies in between) and of
 * amber_hip_pm_gather's kernels since the previous call; the first call switches the timing on (every gather then waits for its kernel) */
int amber_hip_kat_pm_stage_ms(amber_hip_pt*, double* build_ms, double* gather_ms);
/* Scene::BSDF alone (csrc/hip/dev_shading.h): rgb_out[i] = rho * SymmetricBSDF(normal[i], dir_out[i], dir_in[i]) of the material of objects[object[i]],
 * the factor amber_hip_pm_gather multiplies a photon's weight with.  Host arrays, three floats per item; an object index out of range is AMBER_EINVAL. */
int amber_hip_kat_bsdf(amber_hip_pt*, uint32_t n, const int32_t* object, const float* normal, const float* dir_out, const float* dir_in, float* rgb_out);
/* the engine's sin/cos/pow on device: mode 0 = sincos(x[i]) -> out[2i], out[2i+1] ; mode 1 = pow(x[2i], x[2i+1]) -> out[i] ;
 * mode 2 / 3 = x[i]^4 / x[i]^5 in binary64 -> out[2i], out[2i+1] = low, high word of the double */
int amber_hip_kat_math(int device, int mode, uint32_t n, const float* x, float* out);
/* the engine's shared-denominator division on device (csrc/hip/shared_div.h): x = n groups {a, b, c, d}, out = n groups of three.
 * mode 0 = a / d, b / d, c / d through one reciprocal (the wave falls back to mode 1's code when a lane is out of range) ; mode 1 = the plain
 * operator expressions ; mode 2 / 3 = Normalize({a, b, c}) through the shared and the plain form (d is not read) */
int amber_hip_kat_division(int device, int mode, uint32_t n, const float* x, float* out);
/* the engine's square root from one v_rsq_f32 seed on device (csrc/hip/exact_sqrt.h).  mode 0 = sqrt(x[i]) in the guarded fast form (the wave
 * falls back to mode 1's code when a lane is out of range) ; mode 1 = __builtin_sqrtf ; mode 2 / 3 = n groups {a, b, c} -> Normalize through the
 * fused form (root and quotients from the one seed) and through the plain form ; mode 4 = n pairs {a, b} -> their two roots under one guard */
int amber_hip_kat_sqrt(int device, int mode, uint32_t n, const float* x, float* out);
/* mode 0 against mode 1 over the bit patterns [first_bits, first_bits + count), generated on the device (first_bits + count <= 2^32):
 * how many differ, the first few that do (n_offenders counts them all), how many lie in the fast form's range, and for those the extreme
 * signed distances in ulp of v_rsq_f32(x) from the float nearest to 1 / sqrt(x) (formed in binary64 on the device) */
typedef struct { uint64_t mismatches, in_range; uint32_t n_offenders, offenders[8]; int32_t seed_low, seed_high; } AmberSqrtSweep;
int amber_hip_kat_sqrt_sweep(int device, uint32_t first_bits, uint64_t count, AmberSqrtSweep* out);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
