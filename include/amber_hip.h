/*
 * amber_hip.h -- C ABI of the MI355X (gfx950) path-tracing engine.
 *
 * This is the drop-in boundary for amber's unidirectional path tracer.  The reference side of
 * the boundary is
 *     rendering::Algorithm<RGB>::Render(scene, sensor, context)
 *         /root/reference/include/amber/rendering/algorithm.h:40-45
 * as implemented by PathTracing<RGB>
 *         /root/reference/src/amber/rendering/algorithm_pt.cc:82-160.
 * The reference has no FFI; an integrator inside amber would be a C++ class deriving from
 * Algorithm<RGB> that flattens the scene and calls the functions below (INTEGRATION.md shows
 * that adapter; amber_amd/csrc/amber/ holds a complete one).  Plain pointers and sizes only.
 *
 * Threading: a handle is owned by ONE host thread at a time (one handle per GPU).
 * Errors: every int-returning function returns AMBER_OK (0) or a negative AMBER_E* code and
 * records a message retrievable with amber_hip_last_error() (thread-local).
 * There is NO CPU fallback: without a usable HIP device amber_hip_pt_create fails with
 * AMBER_ENODEVICE.
 */
#ifndef AMBER_HIP_H
#define AMBER_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)   /* the libraries are built with -fvisibility=hidden: what these headers declare is what they export */

#define AMBER_HIP_ABI_VERSION 3   /* 3 (round 5): the known-answer / signature entry points, engine WAVEFRONT and AMBER_PT_FLAG_BVH_POOL moved to the lab library
                                    (amber_hip_lab.h); AMBER_PT_FLAG_BVH_ITEMS added.  2 (round 4): lt ranges, stream; a stream-ordered read of
                                    amber_hip_pt_device_framebuffer() needs amber_hip_pt_sync() first when a launch may have run out of record slots.
                                    Still 3 with AMBER_PT_FLAG_DEVICE_BUILD and amber_hip_pt_build_info(): a flag bit that older libraries ignore and
                                    a new function; nothing that existed changed its layout or meaning.  Still 3 with amber_hip_pt_update_objects(): a new function.
                                    Still 3 with amber_hip_pt_cast_rays() / amber_hip_pt_occluded(): two new functions and their two structs.
                                    Still 3 with amber_hip_pt_update_lens(): a new function.  Still 3 with amber_hip_pt_resolve(): a new function.
                                    Still 3 with amber_hip_pt_aov_pass() / _aov_clear() / _aov_download() / amber_hip_pt_device_aov(): four new functions and their struct.
                                    Still 3 with amber_hip_pt_trace_paths() / amber_hip_sampler_state(): two new functions and their two structs.
                                    Still 3 with amber_hip_lt_trace_photons(): one function, two structs, constants.
                                    Still 3 with amber_hip_pm_build() / _pm_gather() / _pm_release(): three functions, three structs, a flag */

/* Accumulation granule: within a render pass the samples of a pixel are summed sequentially in chunks of
 * AMBER_ACCUM_CHUNK consecutive samples (starting at first_sample), and the chunk sums are added to the
 * framebuffer in chunk order.  Part of the numerical contract (the oracle restates it).  8 keeps the work queue
 * fine-grained: with 32 the tail of an 8-way sharded render cost 10 % (EXPERIMENTS.md, multi-GPU). */
#define AMBER_ACCUM_CHUNK 8u

enum {
  AMBER_OK = 0,
  AMBER_EINVAL = -1,     /* bad argument / malformed flat scene */
  AMBER_ENODEVICE = -2,  /* no HIP device / device index out of range */
  AMBER_EHIP = -3,       /* a HIP runtime call failed (message has hipGetErrorString) */
  AMBER_ENOMEM = -4
};

/* ---- flattened scene -------------------------------------------------------------------
 * Produced by scene::Scene::Flatten() (amber_amd/csrc/amber/scene.h).  Object order is the
 * scene's insertion order: closest-hit ties are resolved toward the LOWER index, which is the
 * semantics of the reference's List acceleration (acceleration_list.h:51-68).
 */
enum { AMBER_PRIM_TRIANGLE = 0, AMBER_PRIM_SPHERE = 1, AMBER_PRIM_DISK = 2, AMBER_PRIM_CYLINDER = 3 };
enum {
  AMBER_MAT_LAMBERTIAN = 0,    /* material_lambertian.cc:61-70   rho = kd               */
  AMBER_MAT_PHONG = 1,         /* material_phong.cc:81-106       rho = ks, param = exponent */
  AMBER_MAT_SPECULAR = 2,      /* material_specular.cc:62-70     rho = ks               */
  AMBER_MAT_REFRACTION = 3,    /* material_refraction.cc:177-220 param = ior, r0 = Fresnel(ior) */
  AMBER_MAT_DIFFUSE_LIGHT = 4, /* material_diffuse_light.h:127-194 rho = radiance       */
  AMBER_MAT_EYE = 5            /* material_eye.h:146-155 (aperture pass-through)        */
};

typedef struct {
  uint32_t kind;       /* AMBER_PRIM_* */
  uint32_t material;   /* index into AmberFlatScene.materials */
  /* triangle: v0[3] v1[3] v2[3] normal[3]   (normal = Normalize(Cross(v1-v0, v2-v0)),
   *                                          primitive_triangle.cc:59-68, computed by the host)
   * sphere:   center[3] radius
   * disk:     center[3] normal[3] radius
   * cylinder: center[3] normal[3] radius height */
  float    p[12];
} AmberFlatObject;

typedef struct {
  uint32_t kind;       /* AMBER_MAT_* */
  float    rho[3];
  float    param;
  float    r0;
} AmberFlatMaterial;

/* lens (all derived values computed by the host object model).
 * kind AMBER_LENS_THIN:    lens_thin.cc:32-57.
 * kind AMBER_LENS_PINHOLE: lens_pinhole.cc:31-106; sensor_distance as given, n_blades = 1 (the degenerate aperture
 *                          triangle origin/origin/origin that the reference inserts into the scene), focus_distance and
 *                          p_area unused. */
enum { AMBER_LENS_THIN = 0, AMBER_LENS_PINHOLE = 1 };
typedef struct {
  float    origin[3];
  float    global_[9];         /* Matrix3, row-major */
  float    local_[9];          /* global_.Inverse() */
  float    focus_distance;
  float    sensor_distance;    /* 1 / (1/focal_length - 1/focus_distance) */
  float    p_area;             /* 1 / (blade area * n_blades) */
  uint32_t n_blades;
  uint32_t first_blade_object; /* objects[first_blade_object + i] is aperture blade i */
  uint32_t kind;               /* AMBER_LENS_* */
} AmberFlatThinLens;

/* One entry per SurfaceType::Light object, in the order of scene::LightSet (sorted by power, light_set.h:61-82):
 * cumulative power, pdf_area = Sum(Irradiance) / total power, Irradiance = radiance * pi.  Used by light tracing only. */
typedef struct {
  uint32_t object;        /* index into objects */
  float    cum_power;
  float    pdf_area;
  float    irradiance[3];
} AmberFlatLight;

typedef struct {
  const AmberFlatObject*   objects;
  uint32_t                 n_objects;
  const AmberFlatMaterial* materials;
  uint32_t                 n_materials;
  AmberFlatThinLens        lens;
  const AmberFlatLight*    lights;      /* may be NULL when n_lights == 0 */
  uint32_t                 n_lights;
} AmberFlatScene;

/* rendering::Sensor, sensor.h:34-92 / application.cc:89-94 */
typedef struct {
  uint32_t width, height;
  float    scene_width, scene_height;
} AmberSensor;

typedef struct {
  uint64_t seed;        /* global seed of the per-(pixel,sample) XorShift sampler */
  uint32_t max_depth;   /* 0 = Russian roulette only (reference behaviour, algorithm_pt.cc:137-157) */
  int32_t  device;      /* HIP device ordinal */
  uint32_t row_begin;   /* this handle renders framebuffer rows [row_begin, row_end) -- multi-GPU sharding */
  uint32_t row_end;     /* 0,0 = all rows */
  void*    stream;      /* hipStream_t to launch on; NULL = a NON-BLOCKING stream owned by the handle (it does not synchronise
                           with the legacy default stream: order other work after it with amber_hip_pt_sync or by enqueueing
                           on amber_hip_pt_stream); NULL + AMBER_PT_FLAG_NULL_STREAM in `reserved` = the legacy default stream */
  uint32_t engine;      /* AMBER_ENGINE_* */
  uint32_t stripe_rows; /* 0: every row of [row_begin,row_end).  S > 0: only the rows y with                */
  uint32_t stripe_period; /* (y - row_begin) % stripe_period < S  (interleaved stripes: rank r of N uses     */
  uint32_t reserved;    /* row_begin = r*S, row_end = height, stripe_period = N*S).  Local rows are compact.      */
                        /* `reserved` carries AMBER_PT_FLAG_* bits (0 = none). row_begin == row_end != 0: empty band.   */
} AmberPtParams;
enum {
  AMBER_PT_FLAG_NULL_STREAM = 1u,
  AMBER_PT_FLAG_BVH_POOL = 2u,    /* LAB BUILD ONLY (the product answers AMBER_EINVAL): engine BVH scheduled with the per-wave ray pool
                                     (pt_bvh_pool_kernel).  Same results bit for bit; measured slower on the 1M-sphere scene. */
  AMBER_PT_FLAG_BVH_ITEMS = 4u,   /* engine BVH: always pt_bvh_megakernel.  By default a tree of depth <= 12 (scenes of a few hundred
                                     objects) renders with the path-granular kernel and a one-shot per-lane traversal
                                     (pt_megakernel<ENGINE_BVH>): same results bit for bit, faster on shallow trees. */
  AMBER_PT_FLAG_DEVICE_BUILD = 8u,/* engine BVH (AUTO past 80 objects, AMBER_ENGINE_BVH, WAVEFRONT over either): create builds the tree on the
                                     device -- Morton order, radix-tree hierarchy, the host builder's bounds, padding and outward binary16
                                     planes -- instead of the host's binned-SAH build: a much shorter create, a tree that renders somewhat slower
                                     (INTEGRATION.md gives the break-even), the same image bit for bit (the answer never depends on the tree).
                                     A Morton tree deeper than the traversal's limit is replaced by the host's (amber_hip_pt_build_info says
                                     so).  Any other engine: accepted, no effect. */
  AMBER_PT_FLAG_NO_SCOUT = 16u  /* the 32-object two-phase engine (AUTO up to 32 objects, AMBER_ENGINE_TWO_PHASE): by default a pass traces every path
                                     WITHOUT its weight (the weight reaches the image only where a path ends on a light: 2e-5 of the Cornell paths) and
                                     traces again, with weights, the paths that end on a light or whose weight may have overflowed; with this bit
                                     every path carries its weight.  Same image and ray count bit for bit; a measurement switch.  A lens whose eye
                                     weight the host cannot bound (constants that are not finite, or beyond 2^+-20) renders as with the bit set.
                                     Older libraries ignore the bit, so the ABI version stays.  Any other engine: accepted, no effect. */
};

/* All engines are the same persistent work-queue kernel; they differ in how a lane finds its closest hit.
 * Engines 1-4 return the List-semantics answer (closest finite hit, ties to the lower object index: acceleration_list.h:51-68).
 * REFERENCE_BVH returns the hit the reference's command line finds: Cast through the reference's own BVH
 * (acceleration_bvh.h:134-403), which differs from List on distance ties and on hits the reference's traversal loses
 * (INTEGRATION.md section 3). */
enum {
  AMBER_ENGINE_AUTO = 0,       /* TWO_PHASE when the scene has <= 80 objects, BVH otherwise */
  AMBER_ENGINE_LIST = 1,       /* exact test of every object, wave-uniform scan (object data in SGPRs) */
  AMBER_ENGINE_TWO_PHASE = 2,  /* conservative wave-uniform candidate filter, then exact tests of the candidates only; <= 128 objects
                                  (beyond 32 the objects are dealt into groups of 32, one filter program each) */
  AMBER_ENGINE_BVH = 3,        /* host-built flattened 2-wide BVH, per-lane traversal with an LDS stack, exact leaf tests */
  AMBER_ENGINE_WAVEFRONT = 4,  /* LAB BUILD ONLY (the product answers AMBER_EINVAL): streaming formulation -- SoA ray queues in HBM, one launch
                                  per bounce, ballot/prefix-sum compaction; closest hit as AUTO.  Same results; kept to measure that design. */
  /* 5 is reserved (the library's own id of the two-phase engine over groups of 32 objects; create answers AMBER_EINVAL) */
  AMBER_ENGINE_REFERENCE_BVH = 6  /* the reference's own tree, built at create as acceleration_bvh.h:134-312 builds it (same topology, boxes and
                                  object order) and walked per lane in the order of BVH::Node::Cast (:340-403) with the reference's slab test
                                  (aabb.cc:28-62): ties and lost hits exactly as the reference's command line resolves them.  Never chosen by AUTO: 1.1x (1M spheres) to 2x
                                  (the Cornell box) the time of the engine AUTO picks (unquantised 64-byte nodes, large leaves, a stack in global
                                  memory), and the build sorts every node four times like the reference does (1M objects: under 2 s). */
};

#pragma GCC visibility push(hidden)            /* the handle is opaque: its members (and their constructors) are not part of the ABI */
typedef struct amber_hip_pt amber_hip_pt;
#pragma GCC visibility pop

/* Uploads the flattened scene to HBM and allocates the band framebuffer (zeroed). */
int  amber_hip_pt_create(const AmberFlatScene* scene, const AmberSensor* sensor,
                         const AmberPtParams* params, amber_hip_pt** out);
/* Adds, for every pixel of the band, the path measurements of samples [first_sample, first_sample + n_samples)
 * to the device framebuffer (binary32; order: see AMBER_ACCUM_CHUNK).  Asynchronous. */
int  amber_hip_pt_render_pass(amber_hip_pt*, uint32_t first_sample, uint32_t n_samples);
/* Zeroes the device framebuffer and the ray counter (asynchronous). */
int  amber_hip_pt_clear(amber_hip_pt*);
/* Waits for the handle's stream. */
int  amber_hip_pt_sync(amber_hip_pt*);
/* Copies the band framebuffer (the handle's rows in increasing y, width*3 floats per row, RGB sums --
 * NOT divided by the sample count) and the ray count (Scene::Cast calls) to the host.  Synchronises. */
int  amber_hip_pt_download(amber_hip_pt*, float* rgb_sum, uint64_t* ray_count);
/* Device pointer of the band framebuffer (float, rows*width*3) for zero-copy hand-off to RCCL. */
int  amber_hip_pt_device_framebuffer(amber_hip_pt*, void** dptr, uint64_t* n_floats);
/* The hipStream_t every launch and copy of this handle is enqueued on (NULL = the legacy default stream): work that
 * consumes the device framebuffer (an RCCL gather, a peer copy) is ordered after the render by enqueueing it there. */
int  amber_hip_pt_stream(amber_hip_pt*, void** stream);
/* Number of framebuffer rows this handle owns (after striping). */
int  amber_hip_pt_local_rows(amber_hip_pt*, uint32_t* n_rows);
/* Engine BVH's tree as create built it (after amber_hip_pt_update_objects in mode REBUILD: as that call built it).  Works for every handle. */
enum { AMBER_BUILD_NONE = 0,            /* the handle's engine has no such tree (LIST, TWO_PHASE, REFERENCE_BVH) */
       AMBER_BUILD_HOST = 1, AMBER_BUILD_DEVICE = 2,
       AMBER_BUILD_HOST_FALLBACK = 3 }; /* AMBER_PT_FLAG_DEVICE_BUILD was set, the host built the tree: fallback_reason */
enum { AMBER_BUILD_REASON_NONE = 0,
       AMBER_BUILD_REASON_DEPTH = 1,    /* the Morton tree is deeper than the traversal's limit (30 levels): clustered or coincident objects */
       AMBER_BUILD_REASON_WIDE = 2,     /* an AMBER_BVH_WIDE measurement build: the device builder writes 2-wide nodes only */
       AMBER_BUILD_REASON_BOUNDS = 3 }; /* the scene's bounds are not finite: no Morton order */
typedef struct {
  uint32_t where;            /* AMBER_BUILD_* */
  uint32_t fallback_reason;  /* AMBER_BUILD_REASON_* */
  uint32_t n_nodes;          /* inner nodes (0: the whole scene is one leaf) */
  uint32_t n_leaves;
  uint32_t depth;            /* inner nodes on the longest way from the root to a leaf */
  uint32_t pad;
  double   tree_ms;          /* host wall time of the tree stage of create, everything it waits for included: build, quantisation, the leaf-order
                                arrays and their way into device memory; after a fallback, both attempts */
  double   create_ms;        /* host wall time of amber_hip_pt_create */
} AmberBuildInfo;
int  amber_hip_pt_build_info(amber_hip_pt*, AmberBuildInfo* out);
/* New geometry for the scene objects [first, first + count) of a live handle (objects[0 .. count), host memory, scene index order), and engine
 * BVH's tree made valid again on the device.  Afterwards the handle renders what a handle created on the new scene renders, bit for bit (the
 * answer never depends on the tree).  Still ABI version 3: a new function.
 *   REFIT    keeps the topology and the leaf order of the tree in use -- whoever built it -- and recomputes every box.  Cheapest; the tree
 *            degrades as objects move far against their own size (INTEGRATION.md has the measured curve).
 *   REBUILD  builds the Morton tree again, as AMBER_PT_FLAG_DEVICE_BUILD does at create, into the arrays the handle owns; a host-built tree is
 *            replaced by it, amber_hip_pt_build_info then reports the new tree.  A Morton tree deeper than the traversal's limit is not used:
 *            the call refits the tree in use instead and says so (mode_used, fallback_reason).
 * Geometry only: every new record keeps the kind and the material of the one it replaces, and an aperture blade in the range must equal the
 * resident record bit for bit (the lens and its blades change through amber_hip_pt_update_lens, below).  Objects with NaN parameters are accepted as create accepts them.
 * Lights: path tracing does not read the lights table, so emitting objects move like any other; but cum_power and pdf_area were computed by
 * the caller from the old geometry, so once the record of an object named by an AmberFlatLight has changed, amber_hip_lt_trace / _range
 * answer AMBER_EINVAL until the handle is re-created.
 * Engines: only where the closest-hit engine is BVH (AUTO past 80 objects, AMBER_ENGINE_BVH).  LIST, TWO_PHASE (AUTO on small scenes: their
 * create takes half a millisecond), REFERENCE_BVH (its tree is the reference's, built by the reference's sorts), the lab engine WAVEFRONT and
 * AMBER_BVH_WIDE measurement builds answer AMBER_EINVAL: re-create the handle.
 * Cost: always a pass over the WHOLE scene on the device -- the sphere slack and the needle reach of every object's box depend on the scene
 * diagonal and the plane words on the scene bounds -- only the upload is proportional to count.
 * Order: stream-ordered after everything enqueued on the handle before it and before everything after; a pass enqueued before renders the
 * old scene.  The framebuffer and the ray counter are NOT cleared (amber_hip_pt_clear is the caller's decision).  The call waits for the
 * handle's stream before it returns (twice in all: a small read-back, and the end).  All or nothing: on an AMBER_EINVAL / AMBER_ENOMEM return the
 * handle renders exactly what it rendered before; after AMBER_EHIP (a HIP runtime call failed half way) the handle is to be destroyed.
 * count == 0: AMBER_OK, nothing changes. */
enum { AMBER_UPDATE_REFIT = 0, AMBER_UPDATE_REBUILD = 1 };
typedef struct {
  uint32_t mode_used;        /* AMBER_UPDATE_*: what was done */
  uint32_t fallback_reason;  /* AMBER_BUILD_REASON_DEPTH: a requested REBUILD became a REFIT; 0 otherwise */
  uint32_t n_nodes, depth;   /* of the tree now in use */
  float    area_before, area_after; /* of the tree in use before / after the call (equal when count == 0); tree quality: sum over the inner nodes of both child boxes' surface areas / the root's surface area, from the
                                       planes the traversal reads; informative (summed in arrival order: the last bits vary) */
  double   update_ms;        /* host wall time of the call, everything it waits for included */
} AmberUpdateInfo;
int  amber_hip_pt_update_objects(amber_hip_pt*, uint32_t first, uint32_t count, const AmberFlatObject* objects, uint32_t mode,
                                 AmberUpdateInfo* info /* may be NULL */);
/* The camera of a live handle moved: a new lens and the new records of its aperture blades (blades[0 .. lens->n_blades), host memory; the blades
 * are scene objects and sit in engine BVH's tree), and that tree made valid again on the device.  Afterwards the handle renders, light-traces and
 * answers ray queries exactly as a handle created on the same scene with the new lens and the new blade records does, bit for bit: images, ray
 * counts, amber_hip_lt_trace records, amber_hip_pt_cast_rays hits (the answer never depends on the tree).  Still ABI version 3: a new function.
 * What may change: every value of AmberFlatThinLens -- origin, both matrices, focus_distance, sensor_distance, p_area -- and the geometry of the
 * blades.  kind, n_blades and first_blade_object must equal the resident lens's, and every blade record stays a triangle of the resident
 * blade's material; otherwise AMBER_EINVAL.  The arrays keep their sizes; nothing is reallocated in the steady state.  NaN values are accepted
 * as create accepts them.  The sensor is not part of the call.  Everything create derives from the lens and the blades (the constants of the
 * device's lens record, the blade array) is derived again by create's own function.
 * Engines, modes, order and failure are amber_hip_pt_update_objects': it is that update with the blades as the changed objects, and the lens
 * changes at its commit point.
 *   Engines  only where the closest-hit engine is BVH (AUTO past 80 objects, AMBER_ENGINE_BVH).  LIST, TWO_PHASE, REFERENCE_BVH, the lab engine
 *            WAVEFRONT and AMBER_BVH_WIDE measurement builds answer AMBER_EINVAL: re-create the handle (on LIST / TWO_PHASE the create is the update).
 *   Modes    REFIT and REBUILD as above; a Morton tree deeper than the traversal's limit falls back to REFIT (mode_used, fallback_reason);
 *            amber_hip_pt_build_info follows a REBUILD.
 *   Cost     a pass over the WHOLE scene on the device, whatever moved: a camera that leaves the old bounds changes the scene diagonal and with it
 *            every box and every plane word.  What amber_hip_pt_update_objects costs for n_blades objects in the same mode.
 *   Order    stream-ordered after everything enqueued on the handle before it and before everything after; a pass or a ray query enqueued before
 *            sees the old lens.  The framebuffer and the ray counter are NOT cleared.  The call waits for the handle's stream before it returns.
 *   Failure  all or nothing on AMBER_EINVAL / AMBER_ENOMEM; after AMBER_EHIP the handle is to be destroyed.  A NULL lens or blades: AMBER_EINVAL.
 * Lights: blades are never lights, so the lights table stays valid; amber_hip_lt_trace keeps working and its lens response uses the new lens.
 * Later amber_hip_pt_update_objects calls whose range covers a blade compare against the records of the last lens update. */
int  amber_hip_pt_update_lens(amber_hip_pt*, const AmberFlatThinLens* lens, const AmberFlatObject* blades /* lens->n_blades records, host memory */,
                              uint32_t mode /* AMBER_UPDATE_REFIT | AMBER_UPDATE_REBUILD */, AmberUpdateInfo* info /* may be NULL */);
/* The caller's own rays through the handle's closest-hit engine: Scene::Cast (cast_rays) and the visibility test built on it (occluded).  Still
 * ABI version 3: two new functions.
 *   cast_rays  hits[i] = what the handle's engine returns for Scene::Cast(rays[i]): LIST, TWO_PHASE (both forms) and BVH the closest finite hit, ties
 *              to the lower scene index (acceleration_list.h:51-68); REFERENCE_BVH the hit the reference's own tree finds.  The reference's kEPS
 *              threshold is inside the primitive tests; there is no t_min.  dir is used as given, never normalised: t is in units of |dir|, exactly
 *              as in the render kernels.  pos and normal are the reference's Intersect() output (a triangle's pos from its barycentrics, not
 *              o + t d).  t_max filters the answer: the hit is reported iff t <= t_max; otherwise, and on a miss, object = -1, t = NaN, pos and normal
 *              0.  A NaN t_max is therefore always a miss: pass INFINITY for "unbounded".  A ray with a NaN component hits nothing.  object is a
 *              scene index (the position in AmberFlatScene.objects), never a leaf slot.
 *   occluded   occluded[i] = 1 iff cast_rays on the same ray would report a hit, else 0.  Defined through the closest hit; computed by an any-hit walk
 *              where the engine has one (BVH: the walk ends at the first primitive hit with t <= t_max), by the closest hit elsewhere.
 * Memory: by default rays and the output are DEVICE pointers on the handle's device, and the call is asynchronous and stream-ordered on the
 * handle's stream like amber_hip_pt_render_pass: a query enqueued before amber_hip_pt_update_objects / amber_hip_pt_update_lens sees the old scene, one enqueued after it the
 * new one; read the output after amber_hip_pt_sync, or from work enqueued on amber_hip_pt_stream.  With AMBER_RAYS_HOST both are HOST pointers: the
 * call stages through buffers the handle owns (a million rays at a time) and returns after the copy back.
 * Neither function touches the framebuffer, the ray counter or amber_hip_pt_kernel_time.  Scratch (engine BVH's traversal stacks and work counter,
 * the staging buffers) is allocated by the first query, sized by the launch and not by n, reused by every later query and released by destroy (the
 * staging buffers, which every call that takes host pointers shares, also by amber_hip_pm_release; the next such call allocates them again).
 * n == 0: AMBER_OK.  AMBER_EINVAL: n > 2^31, a NULL pointer with n > 0, unknown flag bits, an AMBER_BVH_WIDE measurement build.  A handle of the lab
 * engine WAVEFRONT answers as engine AUTO does (its closest hit is AUTO's). */
typedef struct { float origin[3]; float t_max; float dir[3]; uint32_t pad; } AmberRay;      /* 32 bytes: two float4 loads */
typedef struct { float t; int32_t object; float pos[3]; float normal[3]; } AmberRayHit;     /* 32 bytes */
enum { AMBER_RAYS_HOST = 1u };   /* rays / out are host pointers: the call stages them and waits */
int  amber_hip_pt_cast_rays(amber_hip_pt*, uint64_t n, const AmberRay* rays, AmberRayHit* hits, uint32_t flags);
int  amber_hip_pt_occluded(amber_hip_pt*, uint64_t n, const AmberRay* rays, uint8_t* occluded, uint32_t flags);
/* Radiance along the caller's own rays: the render kernels' bounce loop (PathTracing::Thread::Render, algorithm_pt.cc:137-157: closest hit, Radiance,
 * SampleLight, Russian roulette) started from rays of the caller's choosing instead of a camera pixel -- irradiance probes, light maps, shading a hit
 * found with cast_rays, paths started elsewhere.  Still ABI version 3: two new functions and their two structs.
 * Definition.  Every operation is binary32 and rounded alone; the arithmetic is the render kernels' own device functions.  For ray i:
 *   r = rays[i].rng_state; r == 0 is replaced by 0x9E3779B97F4A7C15 (a zero xorshift state draws 0 forever, and Russian roulette would never end a path)
 *   sum = (+0, +0, +0), casts = 0
 *   for k = 0 .. n_samples - 1, in this order: one path starts at (origin, dir, weight) with measurement +0, no origin object, and the sampler stream r
 *     as the previous sample left it; it takes bounces (one Scene::Cast each, then Radiance, SampleLight, Russian roulette with the handle's
 *     max_depth) until one ends it; then sum = sum + measurement per channel, casts += the path's casts
 *   out[i] = {sum, casts (mod 2^32), r after the last sample, 0, 0}
 * A ray with a NaN component in origin or dir misses at its first cast, as in cast_rays: the cast is counted and nothing is drawn.  dir is used as
 * given and never normalised.  The pads of a ray are ignored.
 * Consequences.  A path whose first hit is a light seen from its front gives 0 + weight * rho with 1 cast and one draw (the light's scatter weight is
 * 0, so roulette ends it).  A miss gives +0 with 1 cast and no draw.  A call with n_samples = a + b equals a call with a followed by a call with b
 * started from the returned states, the two sums added in that order.  The result for ray i does not depend on n, on its position in the batch or on
 * the other rays.  With rng_state = amber_hip_sampler_state(seed, pixel, s) advanced by the draws of the eye-ray generator (5 for a thin lens, 2 for
 * a pinhole), the eye ray of (pixel, s) and its weight, one sample reproduces the measurement and the cast count of that path of
 * amber_hip_pt_render_pass.
 * max_depth: 0 = the handle's own (AmberPtParams.max_depth); any other value replaces it for this call only.
 * amber_hip_sampler_state(seed, pixel, sample): the state the render kernels' sampler starts (pixel, sample) with, XorShiftSeed(SplitMix64(seed),
 * pixel, sample), never 0 -- for decorrelated streams of one's own, or to reproduce a rendered path.  Host arithmetic only; no device, no handle.
 * Memory, order and errors as amber_hip_pt_cast_rays: DEVICE pointers by default, asynchronous and stream-ordered on the handle's stream (a query
 * enqueued before amber_hip_pt_update_objects / amber_hip_pt_update_lens sees the old scene, one enqueued after it the new one); with AMBER_RAYS_HOST
 * HOST pointers staged through buffers the handle owns (half a million rays at a time), returning after the copy back.  The call never touches the
 * framebuffer, the ray counter or amber_hip_pt_kernel_time.  n == 0 or n_samples == 0: AMBER_OK, nothing written.  AMBER_EINVAL, the handle left
 * working: a NULL handle, a NULL pointer with work to do, n > 2^31, n_samples > 65536, unknown flag bits, an AMBER_BVH_WIDE measurement build.
 * Engines: every product engine in both builds, AMBER_PT_FLAG_DEVICE_BUILD and AMBER_PT_FLAG_BVH_ITEMS handles included; a handle of the lab engine
 * WAVEFRONT answers as engine AUTO does.  On engine BVH an origin outside the scene's bounding sphere takes the scan of every object on that first
 * cast, as in amber_hip_pt_aov_pass.  The work is one lane per ray, the samples of a ray in sequence: few rays with many samples keep few lanes busy. */
typedef struct { float origin[3]; uint32_t pad0; float dir[3]; uint32_t pad1;
                 float weight[3]; uint32_t pad2; uint64_t rng_state; uint64_t pad3; } AmberPathRay;     /* 64 bytes: four float4 */
typedef struct { float rgb[3]; uint32_t casts; uint64_t rng_state; uint32_t pad[2]; } AmberPathResult;  /* 32 bytes: two float4 */
int  amber_hip_pt_trace_paths(amber_hip_pt*, uint64_t n, const AmberPathRay* rays, AmberPathResult* out,
                              uint32_t n_samples, uint32_t max_depth /* 0: the handle's */, uint32_t flags /* AMBER_RAYS_HOST */);
uint64_t amber_hip_sampler_state(uint64_t seed, uint32_t pixel, uint32_t sample);
/* The output stage on the device: the framebuffer's sums as the mean image or as the 8-bit image the reference's command line writes
 * (postprocess::Filmic, then postprocess::Gamma(2.2): filmic.cc:30-66, gamma.cc:36-52), without the round trip amber_hip_pt_download + a host tone
 * map.  Covers every pixel of the handle's band in amber_hip_pt_download's layout: amber_hip_pt_local_rows rows in increasing y, compact, width
 * pixels each.  Still ABI version 3: a new function.
 * Arithmetic, with s the RGB sum of a pixel; every operation binary32 and rounded alone, in this order, per component:
 *   mean   = s / (float)n_samples                               (what HipPathTracing::Render divides by)
 *   AMBER_RESOLVE_MEAN_F32   writes mean: 3 floats, 12 bytes per pixel, NaN payloads as the division leaves them
 *   mapped = Map(mean * 16) / Map(0.70f),  Map(h) = (h*(h*kA + kB*kC) + kD*kE) / (h*(h*kA + kB) + kD*kF) - kE/kF   (the constant products and
 *            kE/kF are binary32 constants; kA .. kF = 0.22, 0.30, 0.10, 0.20, 0.01, 0.30)
 *   v      = 255 * min(1, powf(mapped, 1 / 2.2f)),  min(1, p) = (p < 1) ? p : 1 -- std::min<float>(1, p): a NaN p gives 1
 *   byte   = v >= 0 ? (uint8_t)v : 0                            (truncation)
 *   AMBER_RESOLVE_RGB8       3 bytes per pixel: R, G, B
 *   AMBER_RESOLVE_RGBA8      4 bytes per pixel: R, G, B, 255 -- one aligned 32-bit word, the layout of a display surface
 * Negative, NaN and infinite means therefore give 255, as they do on the host.  The bytes EQUAL those of the host's output stage (amber_host_tonemap,
 * the reference's Filmic + Gamma with glibc 2.35's powf) in the product's arithmetic, AMBER_MATH_GLIBC.  In an AMBER_MATH_PORTABLE measurement build
 * powf is the portable form and single bytes may differ by one; MEAN_F32 is the same in both.
 * AMBER_RESOLVE_MIRROR_X: input column i of a row is written to column width-1-i, the x-mirror ExportPNG and ExportEXR apply (cli/image.cc:45-71);
 * rows stay where they are.
 * Memory and order: by default out is a DEVICE pointer on the handle's device and the call is asynchronous and stream-ordered on the handle's
 * stream, like amber_hip_pt_render_pass: a resolve enqueued after a pass sees that pass, one enqueued before amber_hip_pt_clear the sums before the
 * clear; read the output after amber_hip_pt_sync or from work enqueued on amber_hip_pt_stream.  (One exception to "asynchronous": after a pass
 * whose record buffer was sized from an estimate -- see AMBER_HIP_ABI_VERSION, 2 -- the call first waits for that pass, as amber_hip_pt_clear does.)
 * A 16-byte aligned out (any allocation's start) takes the vector path; MEAN_F32 and RGBA8 need 4-byte alignment at least.  With AMBER_RESOLVE_HOST
 * out is a HOST pointer of any alignment: the call stages through a buffer the handle owns -- grown on first use, reused, released by destroy -- and
 * returns after the copy back.  The call never writes the framebuffer, the ray counter or amber_hip_pt_kernel_time, and it does not read the
 * scene: every engine, both builds.
 * out_bytes must be exactly rows * width * {12, 3, 4}, so that a wrong buffer cannot be overrun; an empty band: AMBER_OK with out_bytes == 0.
 * AMBER_EINVAL, with no effect: a NULL handle, n_samples == 0, an unknown format, unknown flag bits, out == NULL with a non-empty band, any other
 * out_bytes, a misaligned device pointer. */
enum { AMBER_RESOLVE_MEAN_F32 = 0, AMBER_RESOLVE_RGB8 = 1, AMBER_RESOLVE_RGBA8 = 2 };   /* format */
enum { AMBER_RESOLVE_HOST = 1u, AMBER_RESOLVE_MIRROR_X = 2u };                          /* flags */
int  amber_hip_pt_resolve(amber_hip_pt*, uint32_t n_samples, uint32_t format, void* out, uint64_t out_bytes, uint32_t flags);
/* First-hit AOVs: the guide images a denoiser, an edge-aware filter or a compositor takes with a low-sample image -- albedo, depth, shading normal
 * and coverage of the first surface each pixel's eye rays see -- summed over samples on the device.  Still ABI version 3: four new functions and one struct.
 * Definition.  For a band pixel p = (px, py) and a sample index s, ray(p, s) is the eye ray the render kernels generate for that pixel and sample
 * (the sampler seeded by (seed, px + py * width, s), the same draw order, the same aperture blade), and hit(p, s) is what the handle's closest-hit
 * engine returns for the first Scene::Cast of that path: the answer amber_hip_pt_cast_rays gives for that ray with t_max = INFINITY.
 * amber_hip_pt_aov_pass(h, first_sample, n_samples) visits s = first_sample ... first_sample + n_samples - 1 in this order, for every pixel of the
 * band; where hit(p, s) is a hit every component of the pixel's AmberAovPixel gets ONE binary32 addition, v = v + term:
 *   albedo    rho[3] of the hit object's material exactly as AmberFlatMaterial stores it, whatever the material kind: a DiffuseLight's radiance,
 *             an Eye blade's whatever the table holds
 *   depth     the hit's t (in units of |dir|; eye-ray directions are normalised)
 *   normal    the reference's Intersect() normal, AmberRayHit.normal: not flipped towards the ray, not renormalised
 *   coverage  1.0f
 * A miss adds nothing.  The buffer starts at +0 and there is no chunking: one call over [a, a + m + n) and the two calls [a, a + m), [a + m, a + m + n)
 * leave the same bits.  The values are raw SUMS: divide by the sample count (a mean over all samples, misses counting as 0) or by coverage (a mean
 * over the samples that hit).
 * Buffer and order.  The first of these four calls on a handle allocates the buffer (rows * width * 32 bytes) and zeroes it; amber_hip_pt_destroy
 * releases it; a handle that never calls them pays nothing.  aov_pass and aov_clear are asynchronous and stream-ordered on the handle's stream like
 * amber_hip_pt_render_pass: a pass enqueued before amber_hip_pt_update_objects / amber_hip_pt_update_lens sees the old scene and lens, one enqueued
 * after it the new ones.  None of the four touches the framebuffer, the ray counter or amber_hip_pt_kernel_time; amber_hip_pt_clear does not clear the
 * AOV buffer and aov_clear does not clear the framebuffer.
 *   aov_download  copies the band's pixels to the host in amber_hip_pt_download's layout (local rows in increasing y, width pixels each); synchronises.
 *   device_aov    the device pointer of the buffer and the band's pixel count, for zero-copy consumers: read it after amber_hip_pt_sync or from work
 *                 enqueued on amber_hip_pt_stream.  n_pixels may be NULL.
 * Engines: every product engine in both builds; AMBER_PT_FLAG_DEVICE_BUILD and AMBER_PT_FLAG_BVH_ITEMS change nothing in the answer; a handle of the
 * lab engine WAVEFRONT answers as engine AUTO does.  The work is one thread per band pixel looping over the samples, so a band of few pixels is slow
 * however many samples it takes.
 * n_samples == 0: AMBER_OK.  An empty band: AMBER_OK, nothing written, n_pixels == 0 (and a NULL device pointer).  AMBER_EINVAL: a NULL handle, a NULL
 * out or dptr, first_sample + n_samples > 2^32 - 1, aov_pass in an AMBER_BVH_WIDE measurement build.  AMBER_ENOMEM: the buffer could not be allocated. */
typedef struct { float albedo[3]; float depth; float normal[3]; float coverage; } AmberAovPixel;   /* 32 bytes: two float4 */
int  amber_hip_pt_aov_pass(amber_hip_pt*, uint32_t first_sample, uint32_t n_samples);
int  amber_hip_pt_aov_clear(amber_hip_pt*);
int  amber_hip_pt_aov_download(amber_hip_pt*, AmberAovPixel* out);      /* band layout of amber_hip_pt_download: local rows in increasing y, width pixels each; synchronises */
int  amber_hip_pt_device_aov(amber_hip_pt*, void** dptr, uint64_t* n_pixels);
/* A device filter between accumulation and the output stage: the edge-avoiding a-trous wavelet transform (Dammertz, Sewtz, Hanika, Lensch, HPG 2010)
 * of the band's mean image, guided by the AOV buffer, with compactly supported polynomial edge-stopping weights instead of exponentials: a fixed
 * sequence of binary32 operations, no transcendental function.  Still ABI version 3: a new function and one struct.
 * Every operation is binary32 and rounded alone.  Band pixel p = (x, y) uses local row y; fb is the framebuffer's sums, A the AOV sums.
 *   1. input colour   c0(p) = fb(p) / (float)n_samples, per channel (amber_hip_pt_resolve's mean)
 *   2. guide          cov = A.coverage.  If cov > 0: a = A.albedo / cov, n = A.normal / cov (not renormalised), z = A.depth / cov; otherwise
 *                     a = n = 0 and z = 0.  rz = (z > 0) ? 1 / z : 0.
 *   3. level step     level i = 0 .. levels-1 has step s = 2^i, input c_i and output c_{i+1}.  The taps are q = (x + dx*s, y + dy*s), dy = -2..2 the
 *                     outer loop and dx = -2..2 the inner loop, both ascending.  A tap outside the band is skipped: nothing is added for it.
 *                     hw = H[dy] * H[dx] with H = {1/16, 1/4, 3/8, 1/4, 1/16} (these products are exact).
 *   4. tap weight     the centre tap: w = hw (not computed, so sum_w >= 9/64 always).  Every other tap, with
 *                     sq(u, v) = ((u0-v0)*(u0-v0) + (u1-v1)*(u1-v1)) + (u2-v2)*(u2-v2) and clamp0(t) = (t > 0) ? t : 0 (so NaN gives 0):
 *                       tn = clamp0(1 - sq(n_p, n_q) * k_normal)
 *                       ta = clamp0(1 - sq(a_p, a_q) * k_albedo)
 *                       tz = clamp0(1 - (|z_p - z_q| * rz_p) * k_depth)
 *                       tc = clamp0(1 - sq(c_i(p), c_i(q)) * kc_i),  kc_0 = k_color, kc_{i+1} = kc_i * 4
 *                       e  = ((tn * ta) * tz) * tc
 *                       w  = hw * (e * e)
 *   5. accumulation   S_r, S_g, S_b and S_w start at 0; each tap adds w * c_i(q) per channel and w, in tap order; c_{i+1}(p) = S / S_w.
 *   6. output stage   c_levels goes through amber_hip_pt_resolve's output stage unchanged: AMBER_RESOLVE_MEAN_F32 is c_levels itself, RGB8 / RGBA8
 *                     its Filmic + Gamma bytes.
 * format, out, out_bytes and flags mean exactly what they mean for amber_hip_pt_resolve (formats MEAN_F32 / RGB8 / RGBA8, flags AMBER_RESOLVE_HOST
 * and AMBER_RESOLVE_MIRROR_X, the same size and alignment checks); the call is stream-ordered on the handle's stream unless HOST, and first waits
 * for a pass whose record buffer was sized from an estimate, as resolve does.  It reads the framebuffer and the AOV buffer (allocated and zeroed here
 * if no amber_hip_pt_aov_* call has: all-zero guides, only the colour stop acts) and writes only out and buffers of its own (two colour buffers
 * and a guide buffer, 56 bytes per band pixel, grown on first use, released by destroy): the framebuffer, the AOV buffer, the ray counter and
 * amber_hip_pt_kernel_time are untouched.  Every engine, both builds.
 * Not part of it: albedo demodulation (materials are per object, so albedo edges are object edges), temporal accumulation (amber_hip_pt_temporal keeps the frames), variance guidance, a halo
 * across ranks (a band filters within itself: a tap outside the band is a tap outside the image), the command line and the C++ adapter.
 * AMBER_EINVAL, with a message and the handle left working: a NULL handle or params, n_samples == 0, levels outside 1..8, a negative, NaN or infinite
 * k_*, non-zero reserved, an unknown format or flag, any other out_bytes, out == NULL with a non-empty band, a misaligned device pointer, a striped
 * handle (stripe_period != 0: its local rows are not neighbours in the frame).  An empty band: AMBER_OK. */
typedef struct { uint32_t levels; float k_normal; float k_albedo; float k_depth; float k_color; uint32_t reserved[3]; } AmberDenoiseParams;  /* 32 bytes */
int  amber_hip_pt_denoise(amber_hip_pt*, uint32_t n_samples, const AmberDenoiseParams* params,
                          uint32_t format, void* out, uint64_t out_bytes, uint32_t flags);
/* Batch moments: a per-pixel record of how much the batches of a frame disagree, the input a variance-guided filter needs and nothing else in the
 * handle keeps (the render kernels keep only the paths that reach a light or chunk sums, the framebuffer only the total).  Still ABI version 3: four new
 * functions and one struct.  No render kernel changes: a batch is a render_pass whose sums land in a buffer of their own first.
 * Definition.  Every operation is binary32 and rounded alone.  B(p) is what amber_hip_pt_render_pass(first_sample, n_samples) leaves in a framebuffer
 * that held +0.  amber_hip_pt_render_batch(h, first_sample, n_samples) does, per band pixel and channel, fb = fb + B, adds the batch's rays to the ray
 * counter and its launches to amber_hip_pt_kernel_time exactly as render_pass does, and then, with b = B / (float)n_samples per channel:
 *   Y = (0.2126f * b_r + 0.7152f * b_g) + 0.0722f * b_b;   m1 = m1 + Y;   m2 = m2 + Y * Y;   batches = batches + 1.0f;   pad stays 0.
 * Consequences.  For n_samples <= AMBER_ACCUM_CHUNK the batch is one chunk, and the framebuffer gets the very bits render_pass gives it (fb + (0 + chunk)
 * is fb + chunk; the one exception is a pixel whose sum somebody uploaded as -0, which a batch without light turns into +0).  A longer batch is summed
 * first, chunk by chunk from +0, and added once: its own, stated, order, not render_pass's.  The caller chooses the granularity: four calls of one
 * sample give per-sample moments of a 4-spp frame, eight calls of eight batch moments of a 64-spp frame.  m2 / batches - (m1 / batches)^2 estimates the
 * variance of ONE batch's luminance; the variance of the frame's mean is that over `batches`, which assumes batches of equal size.
 * Buffers and order.  The rules of the AOV functions: the first of these calls (or amber_hip_pt_denoise_variance) allocates the moments buffer
 * (rows * width * 16 bytes) and zeroes it; amber_hip_pt_clear does not clear the moments and moments_clear does not clear the framebuffer;
 * amber_hip_pt_update_objects / _update_lens leave the moments alone; destroy releases everything; a handle that never calls these pays nothing.
 * render_batch also owns a batch buffer (12 bytes per band pixel, grown on first use).  render_batch and moments_clear are asynchronous and
 * stream-ordered on the handle's stream like render_pass, with render_pass's exception: where a pass's record buffer was sized from an estimate (see
 * AMBER_HIP_ABI_VERSION, 2) the call waits for that pass -- an earlier one before the batch starts, the batch's own before its sums are folded.
 *   moments_download  copies the band's pixels to the host in amber_hip_pt_download's layout; synchronises.
 *   device_moments    the device pointer of the buffer and the band's pixel count, as amber_hip_pt_device_aov.  n_pixels may be NULL.
 * Engines: every product engine in both builds, AMBER_PT_FLAG_BVH_ITEMS and AMBER_PT_FLAG_DEVICE_BUILD included; a handle of the lab engine WAVEFRONT
 * answers AMBER_EINVAL to render_batch.
 * n_samples == 0: AMBER_OK, nothing changes, not even batches.  An empty band: AMBER_OK.  AMBER_EINVAL as render_pass gives it: a NULL handle (or out,
 * or dptr), first_sample + n_samples > 2^32 - 1.  After any other error of render_batch nothing of the batch has reached the framebuffer or the moments. */
typedef struct { float m1, m2, batches, pad; } AmberMomentsPixel;   /* 16 bytes: one float4 */
int  amber_hip_pt_render_batch(amber_hip_pt*, uint32_t first_sample, uint32_t n_samples);
int  amber_hip_pt_moments_clear(amber_hip_pt*);
int  amber_hip_pt_moments_download(amber_hip_pt*, AmberMomentsPixel* out);      /* band layout of amber_hip_pt_download; synchronises */
int  amber_hip_pt_device_moments(amber_hip_pt*, void** dptr, uint64_t* n_pixels);
/* amber_hip_pt_denoise with the colour stop replaced by a luminance stop that the variance of the mean scales, and that variance filtered along with
 * the colour (after Schied et al., HPG 2017, without its temporal part): what a frame of a few very bright pixels in black needs, which the colour stop
 * of amber_hip_pt_denoise returns unchanged.  Still ABI version 3: a new function and one struct.
 * Every operation is binary32 and rounded alone.  fb, A, the band, sq, clamp0, H, hw and the order of the taps are amber_hip_pt_denoise's; M is the
 * moments buffer; lum(c) = (0.2126f * c_r + 0.7152f * c_g) + 0.0722f * c_b.
 *   1. input          c0 = fb / (float)n_samples.  The guide (a, n, z, rz) is exactly steps 1 and 2 of amber_hip_pt_denoise.
 *   2. moments        if M.batches > 0: u1 = M.m1 / M.batches, u2 = M.m2 / M.batches, e = 1; otherwise u1 = u2 = e = 0.
 *   3. variance of the mean   R = var_radius.  The taps are q = (x + dx, y + dy), dy = -R..R the outer loop and dx the inner, both ascending; a tap outside
 *                     the band is skipped.  The centre tap has g = e_p; every other tap g = ((tn * ta) * tz) * e_q with tn, ta, tz the three guide stops
 *                     of amber_hip_pt_denoise's step 4 and this call's k_*.  A1, A2 and G start at 0; each tap adds g * u1_q, g * u2_q and g.
 *                     If G > 0: mu = A1 / G, v = clamp0(A2 / G - mu * mu); otherwise v = 0.  var_0(p) = (batches_p > 0) ? v / batches_p : v.
 *                     R = 0 is the pixel's own batch variance; R > 0 pools the neighbours on the same surface, which is what a pixel whose samples
 *                     are all zero next to a firefly needs.
 *   4. level i        step 2^i, taps, hw and the centre tap (w = hw, not computed) as amber_hip_pt_denoise.
 *                     gv(p) = the 3 x 3 binomial blur of var_i at unit spacing at every level, coordinates clamped to the band (so the weights
 *                     {1,2,1} x {1,2,1} / 16 always sum to 1), summed from 0 in row-major order, each term weight * var_i.
 *                     r_p = 1 / (k_lum * gv(p) + 1e-10f).
 *                     A non-centre tap: d = lum(c_i(p)) - lum(c_i(q)), tl = clamp0(1 - (d * d) * r_p), e = ((tn * ta) * tz) * tl, w = hw * (e * e).
 *                     S_r, S_g, S_b, S_v and S_w start at 0; each tap adds w * c_i(q) per channel, (w * w) * var_i(q) and w, in tap order.
 *                     c_{i+1} = S / S_w, var_{i+1} = S_v / (S_w * S_w).  No per-level scaling of k_lum: the variance shrinks by itself.
 *   5. output stage   c_levels goes through amber_hip_pt_resolve's output stage, as in amber_hip_pt_denoise.
 * k_lum = 16 cuts a tap off where the luminances differ by four standard deviations of the (blurred) estimate.  A NaN colour reaches every pixel that
 * has it for a tap at some level, as in amber_hip_pt_denoise, and no further; a pixel without batches takes part with e = 0.
 * format, out, out_bytes and flags mean exactly what they mean for amber_hip_pt_denoise, and so do the stream order and the wait for an estimated
 * pass, the striped-handle and empty-band rules and the size and alignment checks.  The call reads the framebuffer, the AOV buffer and the moments
 * buffer (each of the latter two allocated and zeroed here if nobody has touched it) and never writes them, the ray counter or
 * amber_hip_pt_kernel_time.  It writes out and buffers of its own: two record buffers of 16 bytes per band pixel, and amber_hip_pt_denoise's first
 * colour buffer and guide buffer (a later amber_hip_pt_denoise fills them again: its bytes do not change).  Every engine, both builds.
 * Not part of it: firefly clamping, temporal reprojection (amber_hip_pt_temporal reprojects the frames, with amber_hip_pt_denoise's colour stop), albedo demodulation, a halo across ranks, the command line and the C++ adapter.
 * AMBER_EINVAL as amber_hip_pt_denoise gives it (k_lum in k_color's place), plus var_radius > 3 and non-zero reserved.  An empty band: AMBER_OK. */
typedef struct { uint32_t levels; float k_normal; float k_albedo; float k_depth; float k_lum; uint32_t var_radius; uint32_t reserved[2]; } AmberDenoiseVarianceParams;  /* 32 bytes */
int  amber_hip_pt_denoise_variance(amber_hip_pt*, uint32_t n_samples, const AmberDenoiseVarianceParams* params,
                                   uint32_t format, void* out, uint64_t out_bytes, uint32_t flags);
/* Reprojected frame history: what an interactive caller, who moves the camera with amber_hip_pt_update_lens and renders a few samples per frame, needs
 * to keep the last dozen frames instead of starting every frame from nothing.  The handle keeps a per-pixel history; amber_hip_pt_temporal does, per
 * frame, "accumulate into the history, optionally filter, output".  Still ABI version 3: four new functions and two structs.  The call does not read the
 * scene: every engine, both builds, path-traced and light-traced frames alike.
 * The frame loop:  update_lens / update_objects;  clear;  render_pass or lt_render_pass of this frame's samples (a fresh first_sample per frame);
 * aov_clear, aov_pass;  temporal(n_samples, ...).
 * Every operation is binary32 and rounded alone.  fb, A, the band, sq, clamp0 and the guide stops tn, ta, tz are amber_hip_pt_denoise's; lum is
 * amber_hip_pt_denoise_variance's.  Band pixel p = (px, ly) has local row ly and global row py = row_begin + ly; W, H, wf = (float)W, hf = (float)H,
 * sw = scene_width and sh = scene_height are the sensor's.  M . v is the matrix-vector product with each row (m0 * v.x + m1 * v.y) + m2 * v.z; dot(v, v)
 * is (v.x * v.x + v.y * v.y) + v.z * v.z; sqrt and / are correctly rounded.
 *   1. this frame     c = fb / (float)n_samples.  cov = A.coverage; the guide record (a, z)(n, rz) is exactly steps 1 and 2 of amber_hip_pt_denoise.
 *                     Y = lum(c).
 *   2. state          two history buffers and two guide buffers, used ping-pong (history: AmberHistoryPixel; guide: the record of step 1 as the call
 *                     that wrote the history formed it), 2 * (32 + 32) bytes per band pixel, allocated and zeroed by the first of these calls that needs them (temporal_reset never does),
 *                     released by destroy; a snapshot of the lens of the previous call; an "empty" flag, set at create and by temporal_reset.  Primed
 *                     names (H', guide', lens') are the previous call's.  "guide'(q) had coverage" means rz'(q) > 0: the record keeps no coverage word,
 *                     and a hit at a mean depth that is not positive counts as none.
 *   3. reprojection   While the history is empty nothing is reprojected: every pixel is reset (step 4).  Otherwise up to four taps q_k with weights b_k and
 *                     an expected depth d:
 *      lens unchanged (every value of AmberFlatThinLens the handle was given last -- origin, both matrices, focus_distance, sensor_distance, p_area,
 *                     n_blades, kind -- has the bits of the snapshot's): one tap q_0 = p with b_0 = 1, and d = z_p.  (Deliberate: a static camera is an
 *                     exact running mean, not a bilinear tap with a weight one ulp off 1.)
 *      lens changed   through the chief ray, which the pinhole and the thin lens share.  A pixel with cov > 0:
 *                       uvx = ((float)px + 0.5f) / wf,  uvy = ((float)py + 0.5f) / hf
 *                       s = ((uvx - 0.5f) * sw, (uvy - 0.5f) * sh, sensor_distance)
 *                       g = global_ . (-s),  dir = g / sqrt(dot(g, g))  per component
 *                       P = origin + z_p * dir  per component
 *                       v = P - origin',  dl = local_' . v,  t = sensor_distance' / dl.z,  pt = t * dl
 *                       fx = (pt.x / sw + 0.5f) * wf - 0.5f,  fy = (pt.y / sh + 0.5f) * hf - 0.5f,  d = sqrt(dot(v, v))
 *                     valid iff dl.z < 0 and fx > -1 and fx < wf and fy > -1 and fy < hf (each comparison false for a NaN); nothing is converted to an
 *                     integer before this test.  ix = floor(fx), ax = fx - ix, ux = 1 - ax, and iy, ay, uy alike.  The taps, in this order:
 *                     (ix, iy) with b = ux * uy, (ix + 1, iy) with ax * uy, (ix, iy + 1) with ux * ay, (ix + 1, iy + 1) with ax * ay; iy counts
 *                     global rows.  An invalid reprojection has no taps.
 *      accepting      a tap of a pixel with cov > 0 is accepted iff it lies inside the band (a band reprojects within itself, as it filters within
 *                     itself), H'(q).length > 0, guide'(q) had coverage, and (tn * ta) * tz > 0 with the stops taken between this pixel's guide and
 *                     guide'(q), d in place of z_p and 1 / d in place of rz_p, and this call's k_normal, k_albedo, k_depth.  Acceptance is binary: the
 *                     stops do not scale the weight.
 *      cov == 0       (background; any cov that is not > 0.)  Lens unchanged: the one tap is accepted iff H'(p).length > 0 and guide'(p) had no coverage
 *                     either.  Lens changed: no taps.
 *      sums           S_r, S_g, S_b, S_len, S_m1, S_m2 and B start at 0; each accepted tap, in tap order, adds b * H'(q).field and b.  The history is
 *                     KEPT iff B > 0.01f; then h.field = S_field / B.  Otherwise the pixel is RESET.
 *   4. blend          kept:  N = min(h.length + 1, (float)max_history) (the comparison (h.length + 1 < m) ? h.length + 1 : m), alpha = 1 / N, and
 *                     x = h.x + (x_now - h.x) * alpha for the three channels (x_now = c), for m1 (x_now = Y) and for m2 (x_now = Y * Y).
 *                     reset: N = 1, color = c, m1 = Y, m2 = Y * Y.
 *                     {color, N, m1, m2, 0, 0} and this frame's guide record go into the other pair of buffers, which becomes the current one; the
 *                     lens is snapshot and the empty flag cleared.  m2 - m1 * m1 is then the temporal variance of the luminance; this call only keeps it.
 *   5. filter, output levels == 0: the accumulated colour goes through amber_hip_pt_resolve's output stage.  levels >= 1: steps 3 to 5 of
 *                     amber_hip_pt_denoise run `levels` times with c_0 = the accumulated colour, this frame's guide record, k_color and its x 4
 *                     schedule; c_levels goes through the output stage.
 * format, out, out_bytes and flags mean exactly what they mean for amber_hip_pt_denoise, with the same checks in the same order, and so do the stream
 * order, the wait for an estimated pass, the striped-handle and empty-band rules.  The call reads the framebuffer and the AOV buffer (allocated and
 * zeroed here if nobody has touched it: every pixel is background) and never writes them, the moments, the ray counter or amber_hip_pt_kernel_time; it
 * writes out, the history and amber_hip_pt_denoise's two colour buffers (a later amber_hip_pt_denoise fills its buffers again: its bytes do not
 * change).  amber_hip_pt_clear, _aov_clear, _update_objects and _update_lens leave the history alone: a moved object is caught by the depth and normal
 * stops, not by motion vectors.
 *   temporal_reset    empties the history: the next call is a first call, and until then the history reads as zeros.  Asynchronous, stream-ordered.
 *   history_download  copies the current history to the host in amber_hip_pt_download's layout; synchronises.  A history never used reads as zeros.
 *   device_history    the device pointer of the CURRENT history buffer and the band's pixel count, as amber_hip_pt_device_aov; the next
 *                     amber_hip_pt_temporal makes the other buffer current, so ask again after every call.  n_pixels may be NULL.
 * Not part of it: feeding the filtered colour back into the history (the history holds unfiltered means only), variance-guided levels on the temporal
 * moments, motion of moved objects, a halo across ranks, the command line and the C++ adapter.
 * AMBER_EINVAL, with the handle and the history left as they were: a NULL handle or params (or out, or dptr, for the companions), n_samples == 0,
 * levels > 8, max_history outside 1 .. 65535, a negative, NaN or infinite k_*, non-zero reserved, and amber_hip_pt_denoise's checks of format, flags,
 * out_bytes, out and a striped handle.  An empty band: AMBER_OK.  After any other error nothing of the call has reached the history. */
typedef struct { uint32_t levels;        /* 0 .. 8: a-trous levels after accumulation, 0 = none */
                 uint32_t max_history;   /* 1 .. 65535: cap on the history length N */
                 float k_normal, k_albedo, k_depth, k_color;
                 uint32_t reserved[2]; } AmberTemporalParams;                    /* 32 bytes */
typedef struct { float color[3]; float length; float m1, m2; float pad[2]; } AmberHistoryPixel;  /* 32 bytes: two float4 */
int  amber_hip_pt_temporal(amber_hip_pt*, uint32_t n_samples, const AmberTemporalParams* params,
                           uint32_t format, void* out, uint64_t out_bytes, uint32_t flags);
int  amber_hip_pt_temporal_reset(amber_hip_pt*);
int  amber_hip_pt_history_download(amber_hip_pt*, AmberHistoryPixel* out);      /* band layout of amber_hip_pt_download; synchronises */
int  amber_hip_pt_device_history(amber_hip_pt*, void** dptr, uint64_t* n_pixels);
/* Per-launch timing of the dominant kernel, measured with hipEvents on the handle's stream:
 * number of timed launches since create/clear and their total duration. */
int  amber_hip_pt_kernel_time(amber_hip_pt*, uint32_t* n_launches, double* total_ms);
void amber_hip_pt_destroy(amber_hip_pt*);

/* ---- light tracing (rendering::LightTracing, algorithm_lt.cc:112-163) on the same kernels -----------
 * Traces width*height light paths for every pass in [first_sample, first_sample + n_samples) (path i of pass s is seeded
 * by (seed, i, s)) and returns the splats they make on the sensor, sorted in the reference's accumulation order
 * (pass, path, bounce).  value = weight * response / image.Size() is ready to be added to pixel `pixel`.
 * Synchronous.  AMBER_ENOMEM if more than `capacity` splats were produced (n_out then holds the number needed). */
typedef struct { uint32_t path, sample, bounce, pixel; float rgb[3]; uint32_t pad; } AmberSplat;
int amber_hip_lt_trace(amber_hip_pt*, uint32_t first_sample, uint32_t n_samples, AmberSplat* out, uint32_t capacity,
                       uint32_t* n_out, uint64_t* ray_count);
/* The same for the light paths [path_begin, path_end) only: light paths are independent, so the path index shards across
 * devices the way pixels do for path tracing -- every device traces its range of every pass, the caller merges the sorted
 * lists (HipLightTracing::Render; reference: algorithm_lt.cc:82-95 parallelises lt exactly like pt). */
int amber_hip_lt_trace_range(amber_hip_pt*, uint32_t first_sample, uint32_t n_samples, uint32_t path_begin, uint32_t path_end,
                             AmberSplat* out, uint32_t capacity, uint32_t* n_out, uint64_t* ray_count);

/* ---- light tracing into the device framebuffer -----------------------------------------------------------------------------------------------
 * amber_hip_lt_render_pass accumulates the light-tracing passes [first_sample, first_sample + n_samples) into the handle's framebuffer on the
 * device, in the reference's order, bit for bit: no record leaves the GPU, and the frame can go on through amber_hip_pt_resolve,
 * amber_hip_pt_denoise and amber_hip_pt_device_framebuffer like a path-traced one.
 * Definition.  Every operation is binary32 and rounded alone.  R is the record list amber_hip_lt_trace(h, first_sample, n_samples, ...) returns; it is
 * already in (pass, path, bounce) order.  For each pass s ascending, P_s starts at +0 everywhere; each record of pass s, in list order, does
 * P_s[pixel].c = P_s[pixel].c + rgb[c] for c = 0, 1, 2; then fb[p].c = fb[p].c + P_s[p].c for every pixel p that received at least one record in pass s.
 * All other pixels are untouched.  This equals the reference's `sum += image` (algorithm_lt.cc:112-123), except for a sum somebody uploaded as -0
 * (which + 0 would turn into +0), and it is exactly the loop at the end of HipLightTracing::Render.
 * Splitting.  The sum is pass by pass, with no chunking: one call over [a, a + m + n) and the two calls [a, a + m), [a + m, a + m + n) leave the same
 * bits, at any boundary.  This differs from amber_hip_pt_render_pass, whose sums are formed per accumulation chunk.
 * Framebuffer and counters.  The framebuffer is the one amber_hip_pt_render_pass writes; it is not cleared.  amber_hip_pt_clear, _download, _resolve,
 * _denoise and _device_framebuffer work on it as they are; after n passes resolve(n) gives the mean HipLightTracing returns.  The handle's ray counter
 * grows by exactly the ray_count amber_hip_lt_trace reports for the same range, once.  amber_hip_pt_kernel_time counts the trace launches.
 * Running out of record slots.  The handle sizes its own splat buffer: it starts at AMBER_LT_SPLAT_CAPACITY0 records and keeps what it grew to.  When
 * a launch produces more than fits, nothing of that launch reaches the framebuffer, the ray counter is put back to its value before the launch, the
 * buffer grows to the count the launch reported and the (deterministic) launch is repeated once.  n_repeats counts these.  A call may also split its
 * passes into smaller launches.
 * info (may be NULL) reports the totals of the call: records that reached the framebuffer, rays, trace launches (the repeated ones included), repeats;
 * longest_run is the largest number of records one pixel received in one pass.  It is zeroed first, whatever the call then answers.
 * Order.  The call is stream-ordered after everything enqueued on the handle (a pass of amber_hip_pt_render_pass whose record buffer was sized from an
 * estimate is waited for and stands first).  It waits for the stream before it returns, because it reads the record count per launch, as
 * amber_hip_lt_trace does.
 * Whole frame only.  A handle with a band or stripes (row_begin / row_end / stripe_period set) answers AMBER_EINVAL: light paths land anywhere in the
 * frame.  Several devices stay on amber_hip_lt_trace_range plus the host merge.
 * AMBER_EINVAL, with no effect: a NULL handle; first_sample + n_samples > 2^32 - 1; stale lights (as amber_hip_lt_trace); the lab engine WAVEFRONT; a
 * banded or striped handle.  AMBER_OK with nothing changed: n_samples == 0, or a scene without lights.
 * Every engine on which amber_hip_lt_trace works, AMBER_PT_FLAG_BVH_ITEMS and AMBER_PT_FLAG_DEVICE_BUILD included.  Still ABI version 3: a new
 * function, a new struct, a new constant. */
#define AMBER_LT_SPLAT_CAPACITY0 65536u   /* records the handle's splat buffer holds before the first growth */
typedef struct { uint64_t n_splats, n_rays; uint32_t n_launches, n_repeats, longest_run, pad; } AmberLtPassInfo;  /* 32 bytes */
int amber_hip_lt_render_pass(amber_hip_pt*, uint32_t first_sample, uint32_t n_samples, AmberLtPassInfo* info /* may be NULL */);

/* ---- light-path vertices: photons ------------------------------------------------------------------------------------------------------------
 * amber_hip_lt_trace_photons returns the vertices of the light paths amber_hip_lt_trace traces, instead of the splats they make: the list the
 * reference's photon family starts from (PhotonMap::Build, photon_map.h:108-153: the loop of LightTracing::Thread::Render, which stores
 * (position, -ray.Direction(), weight) where that one splats), and the light subpaths of the bidirectional family (GenerateLightSubpath).
 * Definition.  Every operation is binary32 and rounded alone; the arithmetic is the light-tracing kernel's own device functions.  Light path i of
 * pass s is the one amber_hip_lt_trace traces: its sampler starts at amber_hip_sampler_state(seed + 0x6C74, i, s), then GenerateLightRay and the
 * loop of algorithm_lt.cc:135-162 with the handle's max_depth.  At the k-th cast of the path (k counts from 1, as AmberSplat.bounce does), if the
 * cast hits an object whose material kind `surfaces` selects, one record is made, before the material is sampled: pos and normal are the
 * reference's Intersect() output (as in AmberRayHit), object is the scene index (never a leaf slot), dir_out the negated ray direction, weight the
 * path weight on arrival (PhotonMap::Build divides it by its n_photons: the caller's job, one division), path = i (the absolute light-path
 * index), sample = s, bounce = k.  A vertex at k == max_depth is recorded, then the path ends.
 * The call covers the passes [first_sample, first_sample + n_samples) of the light paths [path_begin, path_end).  The records are written in
 * ascending (sample, path, bounce) order; that key names a record completely, so the output does not depend on scheduling, on the engine (except
 * REFERENCE_BVH, which follows the reference's tree on ties, as everywhere), or on how the call splits its passes into launches.  Hence, bit for
 * bit: one call over [a, a + m + n) equals the call over [a, a + m) followed by the call over [a + m, a + m + n); two calls over adjacent path
 * ranges, merged by key, equal one call over the union; a call with mask m equals the call with AMBER_PHOTON_ALL filtered by material kind.
 * Sizing.  The handle owns an arrival-order staging buffer that starts at AMBER_PHOTON_CAPACITY0 records and keeps what it grew to.  A launch that
 * produces more records than fit is deterministic: the buffer grows to the count the launch reported and the launch is repeated once (n_repeats
 * counts these), the protocol of amber_hip_lt_render_pass.  `out` is the caller's buffer, `capacity` its size in records.  When the call needs
 * more than `capacity` records it answers AMBER_ENOMEM, info->n_photons holds the number the whole call needs, `out` is unspecified and the handle
 * stays working.  out == NULL with capacity == 0 is a counting call: AMBER_OK, n_photons set, n_written == 0.  Otherwise AMBER_OK with
 * n_written == n_photons; records beyond n_written are untouched.  n_rays is the number of casts: for [0, W*H) the ray_count amber_hip_lt_trace
 * reports for the same passes.  info (may be NULL) is zeroed first, whatever the call then answers.
 * Memory and order.  `out` is a device pointer, 16-byte aligned, and the call is stream-ordered on the handle's stream; it waits for the stream
 * before it returns, because it reads a count per launch, as amber_hip_lt_trace does.  With AMBER_PHOTONS_HOST `out` is a host pointer, staged
 * through a buffer the handle owns.  The call never touches the framebuffer, the handle's ray counter or amber_hip_pt_kernel_time.  What it
 * allocates it allocates on first use (a handle that never calls it pays nothing); destroy releases it.  A call after amber_hip_pt_update_lens
 * sees the new blades.
 * AMBER_EINVAL, with no effect: a NULL handle; first_sample + n_samples > 2^32 - 1; path_begin > path_end or path_end > W*H; surfaces == 0 or
 * unknown bits in it; unknown flag bits; out == NULL with capacity > 0; a misaligned device pointer; stale lights; the lab engine WAVEFRONT; an
 * AMBER_BVH_WIDE build.  AMBER_OK with zero photons: n_samples == 0, an empty path range, a scene without lights.
 * Banded and striped handles are accepted: light paths do not know the band, and the path range is how several devices share the work, as with
 * amber_hip_lt_trace_range.  Every engine on which amber_hip_lt_trace works, AMBER_PT_FLAG_BVH_ITEMS and AMBER_PT_FLAG_DEVICE_BUILD included.
 * Not here: the nearest-neighbour search and the density estimate (the photon map below has them); eye subpaths; the pdf and geometry-factor fields of SubpathEvent;
 * the command line and the C++ adapter.  Still ABI version 3: one function, two structs, constants. */
enum { AMBER_PHOTON_DIFFUSE = 1u,   /* AMBER_MAT_LAMBERTIAN, AMBER_MAT_PHONG   (SurfaceType::Diffuse)  */
       AMBER_PHOTON_SPECULAR = 2u,  /* AMBER_MAT_SPECULAR, AMBER_MAT_REFRACTION (SurfaceType::Specular) */
       AMBER_PHOTON_LIGHT = 4u,     /* AMBER_MAT_DIFFUSE_LIGHT */
       AMBER_PHOTON_EYE = 8u,       /* AMBER_MAT_EYE: the aperture blades */
       AMBER_PHOTON_ALL = 15u };
enum { AMBER_PHOTONS_HOST = 1u };   /* out is a host pointer: the call stages the records and copies them back */
#define AMBER_PHOTON_CAPACITY0 65536u   /* records the handle's photon staging buffer holds before the first growth */
typedef struct { float pos[3]; int32_t object; float dir_out[3]; uint32_t path;
                 float weight[3]; uint32_t sample; float normal[3]; uint32_t bounce; } AmberPhoton;      /* 64 bytes: four float4 */
typedef struct { uint64_t n_photons, n_written, n_rays; uint32_t n_launches, n_repeats; } AmberPhotonInfo; /* 32 bytes */
int amber_hip_lt_trace_photons(amber_hip_pt*, uint32_t first_sample, uint32_t n_samples, uint32_t path_begin, uint32_t path_end,
                               uint32_t surfaces, AmberPhoton* out, uint64_t capacity, AmberPhotonInfo* info /* may be NULL */, uint32_t flags);

/* ---- photon map: grid build and k-nearest radiance gather -------------------------------------------------------------------------------------
 * What the reference's photon family does with the list above: PhotonMap::Search(point, radius, k), then sum(photon.Weight() * BSDF) * kernel()
 * * weight (algorithm_sppm.cc:200-214, the same loop in algorithm_mppm.cc; algorithm_ups.cc merges the same way).  A handle owns ONE photon map:
 * amber_hip_pm_build makes it from the caller's AmberPhoton records (only pos, dir_out and weight are read) and replaces the one before,
 * amber_hip_pm_gather answers queries against it, amber_hip_pm_release or destroy ends it.  A handle that never calls these pays nothing.
 * Every operation is binary32 and rounded alone, with no contraction; tests/photon_map_reference.py restates all of it in numpy.
 *
 * The grid (build).  Photons with a non-finite pos component are dropped (n_dropped).  Over the rest, lo[a] is the minimum and hi[a] the maximum
 * of pos[a] (order-independent; -0 orders below +0).  c = cell_size, inv = 1.0f / c, dims[a] = (uint32)floorf((hi[a] - lo[a]) * inv) + 1.  The
 * limits are dims[a] <= 1024 and dims[0] * dims[1] * dims[2] <= 2^22.  While a limit is exceeded, or a product (hi[a] - lo[a]) * inv is not below
 * 2^31: c = c * 2, inv and dims again, n_doublings counts the step.  info->cell_size is the c used.  (An extent hi[a] - lo[a] that overflows
 * binary32 has no such c: AMBER_EINVAL, and the map before stays.)  cellf(x, a) = floorf((x - lo[a]) * inv); a photon's cell is
 * (iz * dims[1] + iy) * dims[0] + ix with i* = cellf(pos[*], *), inside the grid by construction (floorf and the two operations are monotone).
 * Within a cell photons stand in ascending input index: a stable sort of the input order by cell.  max_cell_count is the largest cell's count.
 * n == 0, or everything dropped: a valid EMPTY map -- dims, lo, hi and max_cell_count are 0, cell_size is the argument, and gather answers
 * all-zero results.  The map copies what it needs: the caller's buffer is free when build returns.  Build is stream-ordered after everything
 * enqueued on the handle and waits for the stream, because it reads the bounds back, as amber_hip_lt_trace_photons reads its counts.  build_ms is
 * the host's wall-clock time of the call.  info (may be NULL) is zeroed first, whatever the call then answers.
 *
 * The gather, for query i.  r2 = radius * radius.  The all-zero result {0, 0, 0, 0, +0, 0} answers: a non-finite pos component; a radius that is
 * NaN, infinite or <= 0; an object outside [0, n_objects).  Per axis clo = cellf(pos[a] - radius, a), chi = cellf(pos[a] + radius, a), compared AS
 * FLOATS with 0 and dims[a] - 1 before any conversion (chi < 0 or clo > dims[a] - 1 on some axis: nothing is visited), then clamped to the grid.
 * Visit order: iz in the outer loop, then iy, then ix, all ascending; within a cell, the cell's order.  A visited photon is in radius iff d2 < r2
 * with dx = photon.x - pos.x (likewise dy, dz), d2 = (dx * dx + dy * dy) + dz * dz; N = n_in_radius counts them.  The cell range loses none: cellf
 * is monotone and pos[a] - radius is correctly rounded.
 * Selection.  k == 0 or N <= k: all of them are used, n_used = N, r2_used = r2.  Otherwise T is the k-th smallest d2, counting multiplicity; used
 * are the photons with d2 < T plus the first k - #{d2 < T} photons IN VISIT ORDER with d2 == T; n_used = k, r2_used = T.  Whenever no two photons
 * tie at the k-th distance this is the set KDTree::Search ends with (kdtree.h:235-246: a max-heap of k, the radius shrinking to its top).
 * Sum.  S = (+0, +0, +0); over the used photons in visit order S[c] = S[c] + photon.weight[c] * (rho[c] * fs), rho that of the material of
 * objects[object], fs = SymmetricBSDF(normal, dir_out, photon.dir_out): 0 when Dot(dir_out, n) * Dot(dir_in, n) <= 0; Lambertian
 * (material_lambertian.cc:35-49) 1 / (float)kPI; Phong (material_phong.cc:40-61) ((e + 2) / (2 * (float)kPI)) * powf(max(0, Dot(PerfectReflection(
 * dir_in, n, cos_i), dir_out)), e) with the library's powf (amber_hip_math_mode); every other material kind 0 (the reference gathers on
 * SurfaceType::Diffuse only).  rgb[c] = (S[c] * kern) * weight[c], kern = 1 / (((float)kPI * radius) * radius) (kernel.h:52: the QUERY's radius,
 * also when k shrank the search, as in the reference); with AMBER_PM_RAW_SUM rgb = S.  The order of the sum is this call's own, not the
 * reference's heap order.
 * The result for query i does not depend on n, on its position in the batch or on the other queries.
 * Memory and order as amber_hip_pt_cast_rays: DEVICE pointers (16-byte aligned) by default, asynchronous and stream-ordered on the handle's stream;
 * with AMBER_RAYS_HOST host pointers, staged through handle-owned buffers, and the call returns after the copy back.  Neither call touches the
 * framebuffer, the ray counter or amber_hip_pt_kernel_time; amber_hip_pt_update_objects (the gather reads the object's material index as the
 * update left it) and amber_hip_pt_update_lens leave the map alone.  amber_hip_pm_release waits for the stream and frees the map and its scratch.
 * AMBER_EINVAL, with no effect and the handle left working: a NULL handle; a NULL pointer with work to do; n > 2^31 for either call; a cell_size
 * that is NaN, infinite or <= 0; k > 2^31; unknown flag bits; a misaligned device pointer; gather before any build or after release (also with
 * n == 0).  AMBER_OK with nothing written: gather with n == 0 on a handle that has a map.
 * Not here: the integrators (sppm, mppm, ups) and their radius statistics; the eye-path walk past specular bounces; the indices of the photons a
 * query used; maps over several devices.  Still ABI version 3: three functions, three structs, a flag. */
typedef struct { float pos[3]; float radius; float normal[3]; int32_t object;
                 float dir_out[3]; uint32_t pad0; float weight[3]; uint32_t pad1; } AmberGatherQuery;   /* 64 bytes: four float4 */
typedef struct { float rgb[3]; uint32_t n_used; float r2_used; uint32_t n_in_radius; uint32_t pad[2]; } AmberGatherResult; /* 32 bytes */
typedef struct { uint64_t n_photons, n_dropped; uint32_t dims[3]; uint32_t n_doublings;
                 float cell_size; float lo[3]; float hi[3]; uint32_t max_cell_count; double build_ms; } AmberPhotonMapInfo; /* 72 bytes */
enum { AMBER_PM_RAW_SUM = 2u };   /* gather flag, next to AMBER_RAYS_HOST = 1u: rgb is the plain sum S */
int amber_hip_pm_build(amber_hip_pt*, const AmberPhoton* photons, uint64_t n, float cell_size,
                       uint32_t flags /* AMBER_PHOTONS_HOST */, AmberPhotonMapInfo* info /* may be NULL */);
int amber_hip_pm_gather(amber_hip_pt*, uint64_t n, const AmberGatherQuery* q, AmberGatherResult* out,
                        uint32_t k /* 0: no cap */, uint32_t flags /* AMBER_RAYS_HOST | AMBER_PM_RAW_SUM */);
int amber_hip_pm_release(amber_hip_pt*);

const char* amber_hip_last_error(void);
int         amber_hip_abi_version(void);
/* Arithmetic of sin / cos / pow the library was built with: AMBER_MATH_GLIBC (the product) executes glibc 2.35's
 * binary32 sincosf / powf -- the functions the reference calls (sampling.h:249-250, 279) -- operation for operation;
 * AMBER_MATH_PORTABLE (-DAMBER_BUILD_PORTABLE_MATH, measurement builds only) round 1's + - * / forms. */
enum { AMBER_MATH_PORTABLE = 1, AMBER_MATH_GLIBC = 2 };
int         amber_hip_math_mode(void);
int         amber_hip_device_count(void);

/* The known-answer entry points of the tests (amber_hip_kat_*), amber_hip_pt_signatures, engine WAVEFRONT and AMBER_PT_FLAG_BVH_POOL belong to
 * the LAB build, libamber_hip_lab.so: include/amber_hip_lab.h.  libamber_hip.so exports exactly what this header declares (plus the C shim of
 * the host object model, include/amber_host.h, and that model's C++ classes, amber_amd/csrc/amber/). */

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
