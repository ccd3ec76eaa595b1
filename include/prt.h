/* prt.h - C ABI of the MI355X ray-trace hot path (libprt_hip.so).
 *
 * The reference (ACEfanatic02/par_raytracer) has no plugin / FFI interface: main.cpp #includes the
 * whole renderer as one translation unit of static functions.  The seam this ABI replaces is
 *
 *     RenderTask(RenderJob*, DebugCounters*)                      main.cpp:267-283
 *       "fill buffer[0 .. end_idx-start_idx) with linear RGBA float4 for the linear pixel indices
 *        [start_idx, end_idx) of a w x h image, given an immutable camera, scene, global params
 *        and an RNG seed"
 *
 * one level below Render(Camera*, Scene*, u32 w, u32 h) -> Framebuffer (main.cpp:301-358), which the
 * host mirror (par_raytracer_amd/host/) re-implements on top of these entry points.
 *
 * Everything here is plain C: pointers, sizes and POD structs; no C++ or torch types.
 * Return convention: 0 = ok, negative = error (message via prt_last_error); nothing aborts: a C++ exception inside
 * the library (std::bad_alloc, std::length_error, std::system_error ...) is caught at the entry point and comes back as
 * PRT_ERR_EXCEPTION.
 * Threading: one host thread per context at a time; one HIP device and one stream per context.
 */
#ifndef PRT_H_
#define PRT_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PRT_ABI_VERSION 5
/* Error codes (every entry point that returns int): -1 bad argument, -2 no scene uploaded, -5 / -6 internal limits of the
 * wavefront pipeline, -7 park lists kept overflowing, -8 near-tied hits unresolved, -9 the BVH builder produced a tree that fails
 * the upload check (a link or triangle range outside the arrays: refused instead of traversed), -10 a HIP runtime call failed,
 * -11 too many frames in flight (prt_multi_submit), -12 a C++ exception was caught at the entry point. */
enum { PRT_ERR_ARGUMENT = -1, PRT_ERR_NO_SCENE = -2, PRT_ERR_HIP = -10, PRT_ERR_IN_FLIGHT = -11, PRT_ERR_EXCEPTION = -12 };

/* ---- scene description: the reference's pointer graph flattened to POD arrays ---------------- */

/* Material (mesh.h:15-32).  Colours are Vector4 {x,y,z,w}.  Texture slots are indices into
 * prt_scene_desc.textures or -1; the texture path is a "next" row. */
typedef struct prt_material {
    float specular_intensity;      /* Ns */
    float index_of_refraction;     /* Ni */
    float alpha;                   /* d  */
    float ambient_color[4];        /* Ka */
    float diffuse_color[4];        /* Kd */
    float specular_color[4];       /* Ks */
    int32_t ambient_texture;
    int32_t diffuse_texture;
    int32_t specular_texture;
    int32_t alpha_texture;
    int32_t bump_texture;
} prt_material;

/* LightSource (scene.h:3-15). */
enum { PRT_LIGHT_DIRECTIONAL = 0, PRT_LIGHT_POINT = 1 };
typedef struct prt_light {
    int32_t type;
    float color[4];
    float position[3];
    float facing[3];
    float falloff;
} prt_light;

/* MeshGroup (mesh.h:40-47): a contiguous run of the concatenated index buffers. */
typedef struct prt_group {
    uint32_t first_index;          /* offset into idx_* (multiple of 3) */
    uint32_t index_count;          /* 3 * triangles */
    int32_t material;              /* index into materials */
} prt_group;

/* BoundingSphere (bsphere.cpp:316-320), 24 bytes, same field order. */
typedef struct prt_bsphere {
    float center[3];
    float radius;
    uint32_t c0;
    uint32_t c1;
} prt_bsphere;

/* Texture (mesh.h:8-13). */
typedef struct prt_texture {
    uint32_t size_x, size_y, channels;
    const uint8_t * texels;
} prt_texture;

typedef struct prt_scene_desc {
    /* Mesh (mesh.h:49-57) */
    const float * positions;   uint32_t position_count;    /* xyz */
    const float * normals;     uint32_t normal_count;      /* xyz */
    const float * texcoords;   uint32_t texcoord_count;    /* uv  */
    const float * tangents;                                /* xyz per normal, may be NULL */
    /* MeshGroup index buffers of all groups, concatenated in group order */
    const uint32_t * idx_positions;
    const uint32_t * idx_texcoords;
    const uint32_t * idx_normals;
    uint32_t index_count;
    const prt_group * groups;        uint32_t group_count;
    const prt_material * materials;  uint32_t material_count;
    const prt_texture * textures;    uint32_t texture_count;
    /* Scene (scene.h:29-36) */
    const prt_light * lights;        uint32_t light_count;
    /* BoundingHierarchy (bsphere.cpp:322-326), flattened: node i <-> spheres[i]; sphere_group[i] is
     * the group index of a leaf or -1.  The HIP path builds its own per-triangle BVH and uses this
     * tree only to derive the reference's leaf visit order for exact-tie breaking (may be NULL);
     * the CPU oracle traverses it exactly as the reference does. */
    const prt_bsphere * spheres;
    const int32_t * sphere_group;
    uint32_t sphere_count;
} prt_scene_desc;

/* Camera (main.cpp:133-143), same field order. */
typedef struct prt_camera {
    float tan_a2, aspect, inv_width, inv_height;
    float position[3];
    float forward[3];
    float right[3];
    float up[3];
} prt_camera;

/* The subset of gParams (globals.h:9-22) the hot path reads, plus what the reference hard-codes:
 * spp (main.cpp:308-309 -> min_samples = max_samples = spp) and the RNG seed (main.cpp:60-67 ->
 * per-(pixel,sample) key, include/prt_key.h). */
typedef struct prt_params {
    float ray_bias;
    uint32_t reflection_samples;
    uint32_t spec_samples;
    uint32_t bounce_depth;
    float background_color[4];
    uint32_t spp;                  /* samples per pixel; in adaptive mode the fixed first part (min_samples, main.cpp:308) */
    uint32_t pipeline;             /* PRT_PIPELINE_* ; 0 = library default */
    uint64_t seed;
    /* Adaptive sampling (RenderPixel's second loop, main.cpp:245-258), on when max_spp > spp: after `spp` samples with
     * +-0.5 pixel jitter, samples with +-1 pixel jitter are added until the variance of the samples BEFORE the newest is
     * <= variance_threshold or max_spp is reached (the reference hard-codes 10, 50 and 0.01).  The reference's quirks are
     * kept: the newest sample is added to the sum but the sum is divided by the count without it when the rule stops the
     * loop.  One RNG stream per pixel, seeded with prt_sample_key(seed, pixel, 0), as the loop needs; the fixed mode
     * (max_spp <= spp) reseeds per sample.  0 / 0.0f = off / the reference's threshold.
     * The stopping rule compares a float variance of the pixel's sample colours with the threshold.  The device's sample
     * colours are reproducible bit for bit (fixed-point accumulation, see "Determinism" in DESIGN.md) but differ from the CPU
     * reference's in the last bits (device powf, throughput form of the colour polynomial), so a variance that lands within
     * ~1e-6 of the threshold can stop a pixel one sample earlier or later than the reference would.  That is the ONLY way the
     * two can part, and it is counted: prt_render_stats::variance_close_calls is the number of verdicts whose variance lay within
     * 0.1 % of the threshold (a band some fifty times wider than the colours' last bits can move a variance).  0 - as on three of
     * the four adaptive fixtures; the fourth has 2 such verdicts among ~10^5 and equal counts all the same - means every pixel
     * stopped at the reference's sample and ray_count equals the reference's, as it does by construction for fixed spp. */
    uint32_t max_spp;
    float variance_threshold;
} prt_params;

/* DEFAULT = POOL: one launch, wave-private ray pools; the faster pipeline on everything measured except a full 1080p frame
 * of the 1M-triangle scene, where WAVEFRONT (one launch per bounce round, global ray queues) is level or 2 % ahead.
 * With PRT_FLAG_TRYOUT the first DEFAULT call of a (scene, pixel set, sampling) configuration above 1 M samples renders
 * the frame (its first 32 M samples if it is larger than 64 M) with both, twice each, and the context keeps WAVEFRONT if
 * POOL is not at least 3 % faster - worth it for many frames of one configuration, not for a single one.  Adaptive
 * sampling always runs on POOL.  All pipelines produce the same image (tests/test_gpu_parity.py); prt_counters.pipeline
 * reports which ran. */
/* The library has two pipelines, WAVEFRONT and POOL.  MEGAKERNEL (1: round 1's first version, which kept the reference's float
 * association exactly) and PERSISTENT (3: a measured negative result) are reserved values of removed pipelines: asking for
 * them is an error. */
enum { PRT_PIPELINE_DEFAULT = 0, PRT_PIPELINE_MEGAKERNEL = 1, PRT_PIPELINE_WAVEFRONT = 2, PRT_PIPELINE_PERSISTENT = 3,
       PRT_PIPELINE_POOL = 4, PRT_PIPELINE_MASK = 0xFF };
/* OR-ed into prt_params.pipeline: also count BVH node visits and triangle tests (costs a few percent;
 * ray_count and shaded_hits are always counted). */
enum { PRT_FLAG_COUNT_VISITS = 0x100, PRT_FLAG_TRYOUT = 0x200 };

/* DebugCounters (globals.h:3-7) re-cast for a per-triangle BVH.  ray_count has the reference's
 * meaning (one per TraceRay call, raytracer.cpp:161) and must equal the CPU value exactly.  It includes the shadow rays
 * the device does not trace because the radiance that would ride with them is exactly zero (no outcome could change the
 * image; prt_render_stats.elided_shadow_rays says how many): the reference casts and counts those too. */
typedef struct prt_counters {
    uint64_t ray_count;
    uint64_t node_visits;          /* BVH nodes fetched (replaces sphere_check_count) */
    uint64_t tri_tests;            /* triangle tests (the reference tests every triangle of a leaf group) */
    uint64_t shaded_hits;          /* closest-hit shading events */
    double render_ms;              /* ray generation -> resolved framebuffer, device time */
    double trace_kernel_ms;        /* time inside the dominant (traversal) kernel(s) */
    uint32_t trace_kernel_launches;
    uint32_t pipeline;             /* the PRT_PIPELINE_* that ran (what PRT_PIPELINE_DEFAULT resolved to) */
} prt_counters;

typedef struct prt_ctx prt_ctx;

/* Lifecycle.  device_id is a HIP device ordinal.  (A context is one device; prt_multi_* below is the n-device form of
 * SURVEY.md 8(b)'s prt_create(const int * device_ids, int n_dev).) */
prt_ctx * prt_create(int device_id);
void prt_destroy(prt_ctx * ctx);
const char * prt_last_error(const prt_ctx * ctx);   /* ctx may be NULL: last creation error */
int prt_abi_version(void);

/* Options.  Every tuning / test knob of the library is an entry of the context's option table (csrc/prt_options.h).
 * prt_create reads the environment ONCE - PRT_<NAME>=value - and nothing on the upload or render path reads it again;
 * prt_set_option changes an entry afterwards (name with or without the PRT_ prefix, any case; value NULL = default).
 * Three entries change what a render does rather than how fast it is:
 *   TRACE_DEAD_SHADOW_RAYS  0 (default): a shadow ray whose radiance-if-unoccluded is exactly zero is counted in ray_count but
 *                           not traced (no outcome could change the image); 1: traced all the same
 *   BVH_BUILDER             "sah" (default): binned-SAH build on the host; "lbvh": radix tree built on the GPU (applies to the
 *                           next prt_upload_scene)
 *   POOL_EXACT              1: the pool pipeline's slow-path kernel renders everything (test hook; same image)
 * Two of the tuning entries, because tests set them (same image, same counters either way):
 *   POOL_FORK               pool pipeline, opaque untextured fixed-spp renders: the rays that enter at the last bounce level fly
 *                           beside their sample's bounce walk instead of in its chain.  1 on, 0 off, -1 (default) = the build's choice
 *   POOL_FORK_ROOM          the extra list entries those rays get, in eighths of the pool's capacity (default 8; 0: nothing forks)
 * Returns 0, or -1 (unknown name, value that does not parse, RESERVE_CUS after creation). */
int prt_set_option(prt_ctx * ctx, const char * name, const char * value);

/* How the library was built: PRT_BUILD_EXPERIMENTAL - reserved, never set (it marked a library with the MEGAKERNEL /
 * PERSISTENT pipelines); PRT_BUILD_BVH4 - the 4-wide sorted BVH traversal (the default build; clear in a -DPRT_BVH8 library, which traverses the
 * 8-wide compressed tree instead: same results). */
enum { PRT_BUILD_EXPERIMENTAL = 1, PRT_BUILD_BVH4 = 2 };
int prt_build_flags(void);

/* Copies the scene to the device, builds the per-triangle BVH and the sampler tables.  At most 2^26 - 1 triangles (the
 * traversal addresses nodes and triangle records by 32-bit byte offsets); more is an error, as is any index out of range. */
int prt_upload_scene(prt_ctx * ctx, const prt_scene_desc * scene);

/* Replaces RenderTask (main.cpp:267-283): pixels [start_idx, end_idx) of a w x h image, 16 B/pixel,
 * row-major, w component = 1.  rgba_out is a HOST pointer of (end_idx-start_idx)*4 floats.
 * An empty request (start_idx == end_idx here, a shard that owns no rows, a pixel list of length 0) is not an error:
 * nothing is rendered, the counters come back zero and the output pointer may be NULL. */
int prt_render(prt_ctx * ctx, const prt_camera * cam, const prt_params * params,
               uint32_t width, uint32_t height, uint32_t start_idx, uint32_t end_idx,
               float * rgba_out, prt_counters * counters);

/* Same, but d_rgba_out is a DEVICE pointer on the context's device (hipMalloc'ed or a torch tensor's
 * data_ptr): used by the multi-GPU path, which gathers the shards with RCCL afterwards.  The call
 * returns after the context's stream has drained, so the buffer may be consumed on any stream.  The library's
 * streams are NOT ordered against the caller's: work of the caller that still touches the buffer (a fill queued on
 * another stream, a collective reading the previous frame) must have finished - or be waited for - before the call. */
int prt_render_device(prt_ctx * ctx, const prt_camera * cam, const prt_params * params,
                      uint32_t width, uint32_t height, uint32_t start_idx, uint32_t end_idx,
                      void * d_rgba_out, prt_counters * counters);

/* Interleaved scan-line-block sharding: rank r of n renders the blocks of
 * `block_rows` rows whose block index % n == r, packed densely into d_rgba_out in ascending row
 * order, in ONE launch.  prt_shard_rows reports how many rows that is. */
uint32_t prt_shard_rows(uint32_t height, uint32_t block_rows, uint32_t rank, uint32_t nranks);
int prt_render_shard_device(prt_ctx * ctx, const prt_camera * cam, const prt_params * params,
                            uint32_t width, uint32_t height, uint32_t block_rows, uint32_t rank,
                            uint32_t nranks, void * d_rgba_out, prt_counters * counters);
/* Host-output variant of the same (used by the C++ driver's multi-GPU Render()). */
int prt_render_shard(prt_ctx * ctx, const prt_camera * cam, const prt_params * params,
                     uint32_t width, uint32_t height, uint32_t block_rows, uint32_t rank,
                     uint32_t nranks, float * rgba_out, prt_counters * counters);

/* Arbitrary pixel subset: pixel_ids are linear indices (y*width + x), rgba_out (HOST) gets n_pixels
 * float4 in list order.  Pixels are independently seeded, so any subset reproduces the same values as
 * the full frame; the parity tests use it to render exactly the sparse lattice a CPU fixture holds. */
int prt_render_pixel_list(prt_ctx * ctx, const prt_camera * cam, const prt_params * params,
                          uint32_t width, uint32_t height, const uint32_t * pixel_ids, uint32_t n_pixels,
                          float * rgba_out, prt_counters * counters);

/* ---- ray queries: the reference's TraceRay (raytracer.cpp:159-232) on the caller's rays, against the uploaded scene ----
 * One call traces `count` independent rays, no shading.
 *   PRT_QUERY_CLOSEST   the closest hit, bit for bit what the reference's TraceRay returns for the same ray and ray_bias -
 *                       near-tied hits included (decided in the reference's visit order, as the render pipelines do).  A miss is
 *                       the reference's zero-filled record with t = FLT_MAX, except group = -1 and vertex0 = 0xFFFFFFFF.
 *   PRT_QUERY_OCCLUDED  occluded = 1 exactly when some front-facing triangle, tested with the reference's IntersectRayTriangle
 *                       against t = FLT_MAX, gives a hit with t < tmax (independent of visit order, and of the reference's
 *                       sphere tree: with tmax NULL it is 1 for every ray TraceRay hits, and also for the few rays whose hit
 *                       TraceRay loses to a sphere test its float arithmetic fails).  Any-hit traversal.
 * A ray with a non-finite origin or direction component (or biased origin), or a zero direction, is a miss / not occluded; it is
 * not an error and does not affect the other rays; a scene of 0 triangles makes every ray a miss / not occluded.  tmax = +inf is
 * "no limit" (as NULL and as FLT_MAX: every accepted t is below FLT_MAX); a tmax that is 0, negative or NaN makes the ray not
 * occluded (t < tmax holds for no hit) and does not affect the other rays.  A ray's answer is a pure function of (scene, ray,
 * ray_bias, tmax): the same bits whatever else is in the batch, in whatever order, for every launch shape and option.
 * The box padding is computed from
 * max(scene extent, max |biased origin component| of the batch), so origins may lie anywhere.  The reference's sphere test assumes
 * a unit direction and an origin near the scene: CLOSEST rays with |d|^2 further than 2^-18 from 1, or an origin beyond 64 x the
 * scene's largest coordinate, are replayed in the reference's visit order (exact, slower); OCCLUDED rays from such origins take
 * a walk that does not cull by tmax.  So is a CLOSEST hit whose group TraceRay would not have scanned (a ray that grazes the
 * group's bounding sphere at a vertex).  The boxes are walked along the ray IntersectRayTriangle tests, (o + d) - o in floats,
 * whatever its length; a ray whose products in that test can pass FLT_MAX (|d| x |o - vertex| x the scene's size near 2^127) is
 * tested against every triangle in the reference's order, linear in the scene.
 * Counters: ray_count = count (one TraceRay call per ray); node_visits / tri_tests with PRT_FLAG_COUNT_VISITS in `flags`;
 * render_ms = the call's device time, trace_kernel_ms = the traversal kernels'; pipeline = 0.  A query leaves
 * prt_get_render_stats (the last render's) unchanged.
 * Errors: -1 NULL origins / directions with count > 0, unknown mode, NULL batch; -2 no scene; -8 near ties unresolved;
 * -10 a HIP call failed.  count == 0 does nothing and returns 0.
 * The first query after an upload builds a leaf -> (group, vertex0) table on the device (8 B per triangle; not in
 * prt_scene_info.device_bytes; freed by the next upload), and prt_trace_rays the inverse of the visit ranks beside it (4 B per
 * triangle, the same lifetime; built again after a prt_update_geometry). */
enum { PRT_QUERY_CLOSEST = 0, PRT_QUERY_OCCLUDED = 1 };
typedef struct prt_ray_batch {
    const float * origins;         /* count x 3 */
    const float * directions;      /* count x 3, need not be unit length */
    const float * tmax;            /* count floats, OCCLUDED only; NULL = no limit */
    uint32_t count;
    float ray_bias;                /* origin += direction * ray_bias first, as TraceRay does (raytracer.cpp:163) */
} prt_ray_batch;
/* Every pointer may be NULL: that field is not written.  CLOSEST writes t .. normal, OCCLUDED writes occluded only. */
typedef struct prt_hit_buffers {
    float * t;                     /* FLT_MAX on a miss */
    float * bw;                    /* x3: (1 - v - w, v, w) */
    uint32_t * vertex0;            /* first corner of the triangle in its group's index run (the reference's field); 0xFFFFFFFF on a miss */
    int32_t * group;               /* stands for SceneObject*; -1 on a miss */
    float * position;              /* x3: biased origin + direction * t */
    float * normal;                /* x3: Normalize(Cross(ab, ac)) */
    uint8_t * occluded;            /* OCCLUDED: 0 / 1 */
} prt_hit_buffers;
/* Host pointers (batch arrays and hit buffers). */
int prt_trace_rays(prt_ctx * ctx, int mode, const prt_ray_batch * batch, const prt_hit_buffers * hits, uint32_t flags,
                   prt_counters * counters);
/* Device pointers on the context's device (hipMalloc'ed or torch tensors' data_ptr); the stream contract of prt_render_device:
 * the call returns after the context's stream has drained, and the caller's work on the buffers must be finished before it. */
int prt_trace_rays_device(prt_ctx * ctx, int mode, const prt_ray_batch * batch, const prt_hit_buffers * hits, uint32_t flags,
                          prt_counters * counters);

/* ---- geometry updates: the uploaded scene's vertices move, the tree is refitted on the device ---------------------------
 * For a caller that moves a mesh between frames or batches of queries (an animation, an optimisation loop over vertex
 * positions).  The tree keeps its topology; the triangle records are rewritten from the new positions and every node's boxes
 * are refitted bottom-up, one small kernel launch per tree level (csrc/kernels_refit.h; no lane waits for another workgroup).
 * THE CONTRACT: after a successful update every render and every query of the context gives the bits prt_upload_scene would
 * give, on the same context with the same options, for a prt_scene_desc that equals the uploaded one except for the fields
 * passed here - any conservative tree gives the same image, and near ties are decided by the reference's visit ranks, not by the
 * tree (DESIGN.md sections 2-3, 4.8).  Only the tree's quality may differ: node_visits and tri_tests are exempt from the
 * equality; ray_count, shaded_hits, every pixel and every hit field are not.
 *   positions      the new positions; position_count must equal the uploaded scene's (the index buffers stay the upload's, as do
 *                  groups, materials, textures, lights and texture coordinates)
 *   normals        NULL = keep the uploaded ones; else normal_count must equal the upload's
 *   tangents       NULL = keep; else one per normal of the upload (with or without new normals); only read when the scene has
 *                  bump maps
 *   spheres, sphere_group, sphere_count
 *                  HOST pointers in both entry points: the reference's hierarchy of the MOVED scene, or NULL / 0.  NULL means
 *                  what it means at upload - visit ranks in input order, no spheres for the near-tie resolution; the spheres of
 *                  the old geometry are never kept (they would not bound the moved groups).  A tree that cannot be walked falls
 *                  back to input order, as at upload.
 * prt_update_info: device_ms = the device time of the update (coordinate check, records, every level, the rank upload), levels
 * = tree levels = refit launches, node_count, abs_max = the largest |coordinate| of a referenced position (it feeds the box pad).
 * Stream contract of prt_render_device: the call returns after the context's stream has drained; for the device entry point the
 * caller's work on positions / normals / tangents must have finished before the call.
 * Errors: -1 NULL update or positions, a count that differs from the upload's, or a referenced coordinate that is not finite or
 * not below 1e18 (the upload's rule) - found BEFORE anything of the scene is modified on the device: the scene then renders
 * exactly as before the call; -2 no scene uploaded; -10 a HIP call failed - after the first write the context drops to "no
 * scene" rather than render half-moved arrays.  A scene of 0 triangles is a successful no-op.
 * The first update after an upload builds a leaf -> vertex indices table on the device (24 B per triangle, plus 24 B per node of
 * scratch boxes; not in prt_scene_info.device_bytes; freed by the next upload).
 * Out of scope: a change of topology (index buffers, groups: upload again); re-clustering a tree that large moves have degraded
 * - the results stay exact, node_visits grows, and the caller uploads again when it says so -; texture coordinates. */
typedef struct prt_geometry_update {
    const float * positions;  uint32_t position_count;   /* xyz; count must equal the uploaded scene's */
    const float * normals;    uint32_t normal_count;     /* optional (NULL = keep); count must equal the upload's */
    const float * tangents;                              /* optional, per normal; only read when the scene has bump maps */
    const prt_bsphere * spheres; const int32_t * sphere_group; uint32_t sphere_count;  /* HOST, always: the reference's
                                 hierarchy of the MOVED scene, or NULL / 0 */
} prt_geometry_update;
typedef struct prt_update_info { double device_ms; uint32_t levels; uint32_t node_count; float abs_max; } prt_update_info;
/* positions / normals / tangents are HOST arrays; info may be NULL. */
int prt_update_geometry(prt_ctx * ctx, const prt_geometry_update * update, prt_update_info * info);
/* positions / normals / tangents are DEVICE pointers on the context's device (hipMalloc'ed or torch tensors' data_ptr). */
int prt_update_geometry_device(prt_ctx * ctx, const prt_geometry_update * update, prt_update_info * info);

/* ---- gradients of closest-hit queries: how t, bw, position and normal change with the vertices and with the rays --------------
 * Closes the optimisation loop over vertex positions: prt_update_geometry moves the mesh, prt_trace_rays queries it, and this call
 * turns the gradients of a loss with respect to the queries' outputs into gradients with respect to the vertex positions, the
 * origins and the directions.  What is differentiated is the real-valued function behind the forward query on the triangle
 * (a, b, c) it REPORTED (group, vertex0 -> corners idx_positions[first_index + vertex0 + 0..2]):
 *     ob = o + d * ray_bias   ab = b - a   ac = c - a   n = cross(ab, ac)   qp = -d   dd = dot(qp, n)   ap = ob - a   e = cross(qp, ap)
 *     t = dot(ap, n) / dd     v = dot(ac, e) / dd     w = -dot(ab, e) / dd     bw = (1 - v - w, v, w)
 *     position = ob + d * t   normal = n / |n|
 * for any length of d.  The gradient is that of this smooth function; a change of visibility (a ray that slides off a silhouette
 * onto another triangle) is not modelled: there is no edge sampling.
 *   batch          the forward call's rays and ray_bias; tmax is ignored
 *   group, vertex0 the forward call's hit references, count each.  group < 0 is a miss and contributes nothing.
 *   positions      the vertex positions the forward query saw - the uploaded ones, or those last given to prt_update_geometry;
 *                  position_count must equal the upload's
 *   gout           dL/dt (count), dL/dbw, dL/dposition, dL/dnormal (count x 3); a NULL array, or gout NULL, means zero
 *   gin            where the results go; a NULL array is not computed.  positions: position_count x 3, summed over the rays,
 *                  OVERWRITTEN (not accumulated into); origins, directions: count x 3.
 * A ray is SKIPPED - zeros in origins / directions, nothing added to positions - when the named triangle does not face it
 * (dd <= 0) or any of its 15 gradient components is not finite (a grazing hit that overflows, a NaN vertex or ray, a NaN in gout).
 * Only per-ray non-finite contributions are skipped: a sum of finite contributions that exceeds float32 resolves to +-inf in
 * gin->positions; it is neither refused nor clamped.
 * Determinism: the vertex gradient is a sum over rays.  Every contribution is rounded once to a multiple of 2^unit_exponent and
 * added as a 64-bit integer, so the result is the same bits for every order of the rays, every launch shape and every run;
 * unit_exponent = E + L - 62 with 2^(E-1) <= max_contribution < 2^E and L the smallest integer with 3 * count <= 2^L: the sum cannot
 * overflow, and the rounding per contribution is at most 2^(L-63) of max_contribution.
 * prt_grad_info: device_ms = the call's device time (scan, scatter, resolve); hit_rays = rays that contributed, skipped_rays = hits
 * that were skipped (misses are in neither); max_contribution = the largest |component| a ray added to a vertex (0 when none did,
 * and unit_exponent is then 0).
 * Errors: -1 NULL batch; NULL origins, directions, group, vertex0 or positions with count > 0; a position_count that differs from
 * the upload's; a hit reference the scene does not have (group >= group_count, vertex0 not a multiple of 3, vertex0 + 2 >= the
 * group's index_count) - found BEFORE any output is written; -2 no scene; -10 a HIP call failed.  count == 0 zeroes gin->positions
 * (if wanted) and returns 0.  Stream contract of prt_render_device.  The call reads nothing of the tree and leaves the scene, the
 * render stats and the counters alone; the first call after an upload copies the position index buffer and the groups' runs to
 * the device and allocates 24 B per position (not in prt_scene_info.device_bytes; freed by the next upload). */
typedef struct prt_hit_grads   { const float * t; const float * bw; const float * position; const float * normal; } prt_hit_grads;
typedef struct prt_query_grads { float * positions; float * origins; float * directions; } prt_query_grads;
typedef struct prt_grad_info   { double device_ms; uint32_t hit_rays, skipped_rays; int32_t unit_exponent; float max_contribution; } prt_grad_info;
/* Host pointers (batch arrays, group, vertex0, positions, gout's and gin's arrays); info may be NULL. */
int prt_trace_rays_backward(prt_ctx * ctx, const prt_ray_batch * batch, const int32_t * group, const uint32_t * vertex0,
                            const float * positions, uint32_t position_count, const prt_hit_grads * gout,
                            const prt_query_grads * gin, prt_grad_info * info);
/* The same with device pointers on the context's device (hipMalloc'ed or torch tensors' data_ptr). */
int prt_trace_rays_backward_device(prt_ctx * ctx, const prt_ray_batch * batch, const int32_t * group, const uint32_t * vertex0,
                                   const float * positions, uint32_t position_count, const prt_hit_grads * gout,
                                   const prt_query_grads * gin, prt_grad_info * info);

/* ---- closest points: the nearest point of the uploaded surface, for batches of points ------------------------------------------
 * The spatial query beside the rays: point-to-surface and chamfer losses when a mesh is fitted to scanned points, collision and
 * penetration tests, projecting samples onto the surface.  One call answers `count` independent points against the scene as it
 * lies on the device now (after any number of prt_update_geometry calls).
 * THE DEFINITION (csrc/dev_closest.h).  For a triangle record (a, ab = b - a, ac = c - a),
 * closest_on_triangle is the region walk of Ericson, Real-Time Collision Detection 5.1.5, in float32 and a fixed expression
 * order: it gives (v, w), q = (a + ab * v) + ac * w and d2 = Dot(p - q, p - q).  Both sides count: there is no facing test.  A
 * triangle whose d2, v or w is not finite is no candidate.  The answer for p is, among the triangles with d2 <= max_dist2[i]
 * (FLT_MAX with max_dist2 NULL), the one with the smallest d2 and, among equal d2 bits, the smallest (group, vertex0): a pure
 * function of (scene, point) - the same bits for every tree (SAH, LBVH, 8-wide, refitted), launch shape and run, and the bits
 * a brute force over all triangles with the same function gives.
 * A point with a non-finite component, or with max_dist2 negative or NaN, is a miss; it is not an error and does not affect
 * the other points.  A miss: dist2 = FLT_MAX, point and bw zeros, group = -1, vertex0 = 0xFFFFFFFF (the ray queries'
 * convention); a scene of 0 triangles makes every point a miss.  max_dist2 = +inf is "no limit", 0 finds points on the surface.
 * SCALE.  The walk's tests run on (p - a, ab, ac) x 2^-k, k = the exponent of the largest |component| of the three vectors, and
 * d2 is scaled back by two exact products: v, w and the region are free of scale, and the answer at scale 2^e is 2^e times
 * the answer at scale 1 for every scene the upload accepts (|coordinate| < 1e18).  What bounds the range is d2 itself:
 * a triangle whose d2 overflows to inf (true d2 >= 2^128) is no candidate, so a point more than 2^64 away from every triangle
 * misses without a radius; a d2 below 2^-126 is reported as a subnormal float or 0.  Inside those bounds no valid point misses.
 * A point farther than 2^31 edge lengths from a triangle may take another region of it than the real-valued walk.
 * A zero-area triangle is a candidate exactly when the function returns finite values for the point: in its vertex and edge
 * regions, not where the interior branch divides by its zero area.
 * The walk culls boxes by their distance to p, padded by 2^-16 x max(scene extent, max |finite point component| of the batch);
 * points far from the scene (many extents away) are exact but slow: their box distances all tie within the pad and much of the
 * tree is visited.
 * Counters: ray_count = count; node_visits / tri_tests with PRT_FLAG_COUNT_VISITS in `flags` - sums over the points' walks, which
 * depend on the tree, the batch, STACK_CAP and the pad but not on the schedule options or the entry point; render_ms = the call's device
 * time, trace_kernel_ms = the walk kernels'; pipeline = 0.  prt_get_render_stats (the last render's) is left alone.
 * Errors: -1 NULL batch or buffers struct, NULL points with count > 0; -2 no scene; -10 a HIP call failed.  count == 0 writes
 * nothing and returns 0.
 * Shares the ray queries' leaf -> (group, vertex0) table (built by the first query of either kind after an upload). */
typedef struct prt_point_batch {
    const float * points;          /* count x 3 */
    const float * max_dist2;       /* count squared radii; NULL = no limit */
    uint32_t count;
} prt_point_batch;
/* Every pointer may be NULL: that field is not written. */
typedef struct prt_closest_buffers {
    float * dist2;                 /* d2; FLT_MAX on a miss */
    float * point;                 /* x3: q */
    float * bw;                    /* x3: (1 - v - w, v, w), as prt_hit_buffers.bw */
    uint32_t * vertex0;            /* as prt_hit_buffers.vertex0; 0xFFFFFFFF on a miss */
    int32_t * group;               /* as prt_hit_buffers.group; -1 on a miss */
} prt_closest_buffers;
/* Host pointers (batch arrays and buffers). */
int prt_closest_points(prt_ctx * ctx, const prt_point_batch * batch, const prt_closest_buffers * out, uint32_t flags,
                       prt_counters * counters);
/* Device pointers on the context's device; the stream contract of prt_trace_rays_device. */
int prt_closest_points_device(prt_ctx * ctx, const prt_point_batch * batch, const prt_closest_buffers * out, uint32_t flags,
                              prt_counters * counters);

/* ---- gradients of closest-point queries: how dist2, point and bw change with the vertices and with the points -----------------
 * The counterpart of prt_trace_rays_backward for prt_closest_points; it closes the loop for point-to-surface and chamfer losses
 * when a mesh is fitted to scanned points: prt_update_geometry moves the mesh, prt_closest_points queries it, and this call turns
 * the gradients of a loss with respect to dist2, point and bw into gradients with respect to the vertex positions and the points.
 * What is differentiated is the real-valued function behind closest_on_triangle on the triangle (a, b, c) the forward query
 * REPORTED (group, vertex0 -> corners idx_positions[first_index + vertex0 + 0..2]), inside the region R that the float32 walk
 * takes for p (recomputed by this call, never passed in); with ab = b - a, ac = c - a, ap = p - a, d1..d6, va, vb, vc of Ericson
 * 5.1.5 (csrc/dev_closest.h):
 *     R 0 vertex a: v = 0, w = 0     1 vertex b: v = 1, w = 0     3 vertex c: v = 0, w = 1
 *     R 2 edge ab:  v = d1 / (d1 - d3), w = 0                     4 edge ac:  v = 0, w = d2 / (d2 - d6)
 *     R 5 edge bc:  w = (d4 - d3) / ((d4 - d3) + (d5 - d6)), v = 1 - w
 *     R 6 interior: v = vb / ((va + vb) + vc), w = vc / ((va + vb) + vc)
 *     point = q = (a + ab v) + ac w     dist2 = Dot(p - q, p - q)     bw = (1 - v - w, v, w)
 * The constants 0 and 1 have zero derivative.  A change of region, or of the winning triangle, is not modelled (the stance
 * prt_trace_rays_backward takes on silhouettes).
 *   batch          the forward call's points; max_dist2 is ignored
 *   group, vertex0 the forward call's references, count each.  group < 0 is a miss and contributes nothing.
 *   positions      the vertex positions the forward query saw - the uploaded ones, or those last given to prt_update_geometry;
 *                  position_count must equal the upload's
 *   gout           dL/ddist2 (count), dL/dpoint, dL/dbw (count x 3); a NULL array, or gout NULL, means zero
 *   gin            where the results go; a NULL array is not computed.  positions: position_count x 3, summed over the points,
 *                  OVERWRITTEN (not accumulated into); points: count x 3.
 * A point is SKIPPED - zeros in gin->points, nothing added to positions - when the named triangle is no candidate for it (d2, v
 * or w not finite: the forward query would not have reported it) or any of its 12 gradient components is not finite (a NaN
 * vertex or point, a NaN in gout, an overflow).  dL/dbw reaches those components only through the derivatives of v and w, and a
 * region reads only the barycentric it computes: neither in a vertex region, dL/dv = dL/dbw[1] - dL/dbw[0] on edge ab,
 * dL/dw = dL/dbw[2] - dL/dbw[0] on edge ac, both on edge bc and in the interior.  A NaN in an entry of dL/dbw that the point's
 * region does not read is not seen and does not skip the point.
 * Only per-point non-finite contributions are skipped: a sum of finite contributions that exceeds float32 resolves to +-inf in
 * gin->positions; it is neither refused nor clamped.
 * Determinism, prt_grad_info (hit_rays = points that contributed, skipped_rays = reported hits that were skipped), the errors
 * (-1 NULL batch; NULL points, group, vertex0 or positions with count > 0; a position_count that differs from the upload's; an
 * invalid reference, found BEFORE any output is written; -2 no scene; -10 a HIP call failed), count == 0, the stream contract and
 * what the call leaves alone are prt_trace_rays_backward's, word for word; the two calls share their device buffers.  The option
 * QGRAD_MERGE governs both (same bits either way).  DESIGN.md section 4.11. */
typedef struct prt_closest_grads { const float * dist2; const float * point; const float * bw; } prt_closest_grads;   /* dL/doutputs; NULL = zero */
typedef struct prt_point_grads   { float * positions; float * points; } prt_point_grads;      /* NULL = not computed */
/* Host pointers (batch arrays, group, vertex0, positions, gout's and gin's arrays); info may be NULL. */
int prt_closest_points_backward(prt_ctx * ctx, const prt_point_batch * batch, const int32_t * group, const uint32_t * vertex0,
                                const float * positions, uint32_t position_count, const prt_closest_grads * gout,
                                const prt_point_grads * gin, prt_grad_info * info);
/* The same with device pointers on the context's device (hipMalloc'ed or torch tensors' data_ptr). */
int prt_closest_points_backward_device(prt_ctx * ctx, const prt_point_batch * batch, const int32_t * group, const uint32_t * vertex0,
                                       const float * positions, uint32_t position_count, const prt_closest_grads * gout,
                                       const prt_point_grads * gin, prt_grad_info * info);

/* ---- signed distances: which side of the surface a point is on --------------------------------------------------------------
 * prt_closest_points plus a sign, for signed distance fields, penetration depths, containment tests and occupancy labels.  The
 * sign comes from the closest feature and its angle-weighted pseudonormal (Baerentzen & Aanaes, "Signed distance computation
 * using the angle weighted pseudonormal", 2005); no ray is cast and nothing is counted.
 * THE DEFINITION (csrc/dev_signed.h).  For a point p take the winner (group, vertex0, v, w, d2) exactly
 * as prt_closest_points defines it: the walk, the tie rule and the pad are unchanged, and the five closest fields are the bits
 * prt_closest_points writes.  R = the region 0..6 that closest_region_walk (csrc/dev_closest.h; the numbering of
 * prt_closest_points_backward above) takes on the winner's record for p, q = (a + ab v) + ac w, e = p - q, and
 *     R = 6 interior   N = cross(ab, ac), unnormalised
 *     R = 2, 4, 5      N = the pseudonormal of the edge ab, ac, bc: the sum of n over the triangles that have the edge
 *     R = 0, 1, 3      N = the pseudonormal of the vertex a, b, c: the sum of (interior angle at the vertex) x n over the
 *                      triangles that have the vertex
 *     s = Dot(e, N)    signed_dist = s < 0 ? -sqrtf(d2) : sqrtf(d2)
 * with n = Normalize(cross(ab, ac)) of a triangle's record.  NaN, s == 0 and d2 == 0 give the non-negative branch.  Positive is
 * the side cross(ab, ac) points to - the side PRT_QUERY_CLOSEST calls front-facing.  A miss has signed_dist = FLT_MAX and
 * feature = 255.  Only the sign of s is read, and s, n and the angles are evaluated on edges and e scaled by the power of two of
 * their largest component (csrc/dev_signed.h): the sign does not depend on the scale of the scene, within the range of d2
 * that prt_closest_points states (d2 rounded to 0 gives +0).
 * Vertices are the entries of `positions`, identified by their index in idx_positions; an edge is an unordered pair of position
 * indices; the triangles of all groups count.  Two positions with equal coordinates but different indices are different
 * vertices, and an edge between them is a boundary edge: welding is the caller's business.
 * The sums are exact and ordered by nothing: every component of a contribution (float32, fixed expression order, angles from
 * signed_acos of csrc/dev_signed.h - no libm call) is rounded once to a multiple of 2^-32 and added as a 64-bit integer; a
 * triangle whose n or angles are not all finite contributes nothing; N = (float)sum x 2^-32.  The result is a pure function of
 * (scene as it lies on the device, point): the same bits for every tree (SAH, LBVH, 8-wide, refitted), schedule option,
 * STACK_CAP, entry point, batch order and run, and the bits a brute force over all triangles gives on the host.
 * LIMITS.  On a closed, consistently wound mesh the sign is inside (negative) / outside.  On an open or inconsistently wound
 * mesh it is the side of the nearest surface element: deterministic, but not an occupancy.  Within rounding of a region
 * boundary the float32 region can differ from the real-valued one, and then another feature's normal is read.  Gradients of the
 * sign are not modelled.
 * TABLES.  The first signed query after an upload builds the adjacency (per triangle the three position indices and three edge
 * ids: 24 B per triangle) and allocates the accumulators (24 B per position and 24 B per edge); the first signed query after an
 * upload or after a successful prt_update_geometry[_device] refills the accumulators on the device from the records as they lie
 * there (its time counts in render_ms, not in trace_kernel_ms).  Like the leaf table they are not in
 * prt_scene_info.device_bytes and are freed by the next upload.  A call that requests neither signed_dist nor feature builds
 * nothing and is prt_closest_points.
 * Errors, count == 0, the counters, the stream contract and the treatment of invalid points are prt_closest_points's, word for
 * word. */
typedef struct prt_signed_buffers {
    prt_closest_buffers closest;   /* as prt_closest_points writes them; any pointer may be NULL */
    float * signed_dist;           /* +-sqrt(d2); FLT_MAX on a miss */
    uint8_t * feature;             /* the region R 0..6 whose normal decided; 255 on a miss */
} prt_signed_buffers;
/* Host pointers (batch arrays and buffers). */
int prt_signed_distance(prt_ctx * ctx, const prt_point_batch * batch, const prt_signed_buffers * out, uint32_t flags,
                        prt_counters * counters);
/* Device pointers on the context's device; the stream contract of prt_trace_rays_device. */
int prt_signed_distance_device(prt_ctx * ctx, const prt_point_batch * batch, const prt_signed_buffers * out, uint32_t flags,
                               prt_counters * counters);

/* ---- surface samples: points on the uploaded mesh, drawn uniformly by area -------------------------------------------------------
 * The other side of a chamfer loss (mesh -> scan; prt_closest_points is scan -> mesh), mesh-to-mesh and Hausdorff estimates (sample
 * one mesh, prt_closest_points on the other), area-weighted surface integrals, seeds for rays.  One call draws `count` points on the
 * scene as it lies on the device now (after any number of prt_update_geometry calls).
 * THE DEFINITION (csrc/dev_sample.h).  Everything is a pure function of (the records as they lie on the
 * device, seed, sample index j): the same bits for every tree (SAH, LBVH, 8-wide, refitted), launch shape, split of a batch into
 * calls and run, and the bits a brute force on the host gives with the same functions.
 *   Triangle order   input order: triangle t is index triple t of idx_positions (group g's triangles start at first_index / 3),
 *                    not the order of the tree's leaves.
 *   Weight           of a triangle record (a, ab = b - a, ac = c - a): k = the exponent of the largest |component| of ab and ac,
 *                    A = sqrtf(length_sq(cross(ab x 2^-k, ac x 2^-k))) in float32 without contraction; the weight is the real number
 *                    A x 2^(2k), twice the area, held exactly in a double.  A triangle whose A is zero or not finite has weight 0
 *                    and is never drawn.
 *   Fixed point      E: 2^(E-1) <= the largest weight < 2^E; L: the smallest integer with triangle count <= 2^L;
 *                    unit_exponent = E + L - 62 (the rule of prt_trace_rays_backward's unit_exponent);
 *                    W_t = (uint64)rint(weight_t x 2^-unit_exponent); C_t = W_0 + ... + W_t; T = C_(n-1) < 2^62.  The sums are
 *                    integers: every scan order gives the same C.  With L = 20 the largest triangle keeps 42 bits, so float32's 24
 *                    bits survive for triangles down to 2^-18 of the largest area; a smaller triangle's weight loses low bits, and
 *                    one below 2^-(62 - L) of the largest rounds to weight 0.
 *   Sample j         j = first + i < 2^48.  The generator is seeded with prt_sample_key(seed, j >> 16, j & 0xFFFF) (prt_key.h: the
 *                    key's packed word is j itself) and makes three draws: r0, the raw 64 bits; u1, u2 = the next two as floats in
 *                    [0, 1].  x = the high 64 bits of r0 x T; the triangle is the smallest t with C_t > x (zero-weight triangles
 *                    are skipped by construction).  v = u1, w = u2, and if v + w > 1.0f both are mirrored: v = 1 - v, w = 1 - w.
 *                    bw = (fmaxf(0, (1 - v) - w), v, w); point = (a + ab v) + ac w; normal = Normalize(cross(ab, ac)) on the
 *                    edges x 2^-k - the expression PRT_QUERY_CLOSEST uses for prt_hit_buffers.normal, free of the scene's scale;
 *                    group, vertex0 = the triangle's reference, as prt_hit_buffers reports it.
 *   Miss             T == 0 (no triangles, or none with an area) makes every sample a miss: zeros in point, bw and normal,
 *                    group = -1, vertex0 = 0xFFFFFFFF.  It is not an error.
 * SCALE.  At scale 2^e group, vertex0, bw, normal, total_weight and live_triangles are the bits of scale 1, point is 2^e times the
 * point of scale 1 and unit_exponent moves by 2e, for every scene the upload accepts (|coordinate| < 1e18) whose edges' squared
 * lengths are normal floats after the per-triangle scaling.
 * NOT MODELLED.  The choice of the triangle is not differentiated: prt_sample_surface_backward has no gradient through the area
 * weights - the stance the other gradients take on silhouettes and regions.
 * prt_sample_info: device_ms = the call's device time, table_ms = the part of it spent rebuilding the prefix sums (0 when nothing
 * was rebuilt); area = 0.5 x total_weight x 2^unit_exponent; total_weight = T; live_triangles = the triangles with W_t > 0.
 * TABLES.  The first sampling call after an upload builds the input triangle -> leaf table (4 B per triangle); the first sampling
 * call after an upload or after a successful prt_update_geometry[_device] rebuilds the weights and their prefix sums on the device
 * from the records as they lie there (16 B per triangle and 8 B per 256 triangles of scratch; four launches on the context's stream,
 * no lane waits for another workgroup) and reads 24 bytes back.  Like the leaf table they are not in prt_scene_info.device_bytes
 * and are freed by the next upload.
 * Errors: -1 NULL request or buffers, first + count > 2^48; -2 no scene; -10 a HIP call failed.  count == 0 writes nothing
 * (info, if given, is zeroed: no table is built for it) and returns 0.  Stream contract of prt_trace_rays_device.  The call leaves
 * the render stats and the counters alone. */
typedef struct prt_sample_request { uint64_t seed; uint64_t first; uint32_t count; } prt_sample_request;
/* Every pointer may be NULL: that field is not written. */
typedef struct prt_sample_buffers {
    float * point;                 /* x3 */
    float * bw;                    /* x3: (1 - v - w, v, w), as prt_hit_buffers.bw */
    float * normal;                /* x3: unit, the side cross(ab, ac) points to */
    uint32_t * vertex0;            /* as prt_hit_buffers.vertex0; 0xFFFFFFFF on a miss */
    int32_t * group;               /* as prt_hit_buffers.group; -1 on a miss */
} prt_sample_buffers;
typedef struct prt_sample_info { double device_ms; double table_ms; double area; uint64_t total_weight;
                                 int32_t unit_exponent; uint32_t live_triangles; } prt_sample_info;
/* Host pointers (buffers); info may be NULL. */
int prt_sample_surface(prt_ctx * ctx, const prt_sample_request * request, const prt_sample_buffers * out, prt_sample_info * info);
/* Device pointers on the context's device (hipMalloc'ed or torch tensors' data_ptr). */
int prt_sample_surface_device(prt_ctx * ctx, const prt_sample_request * request, const prt_sample_buffers * out, prt_sample_info * info);

/* ---- gradients of surface samples: how point and normal change with the vertices ------------------------------------------------
 * Closes the loop for the mesh -> scan side of a chamfer loss: prt_update_geometry moves the mesh, prt_sample_surface draws points
 * on it, and this call turns the gradients of a loss with respect to the samples' points and normals into gradients with respect
 * to the vertex positions.  What is differentiated is, on the triangle (a, b, c) the forward call REPORTED (group, vertex0 ->
 * corners idx_positions[first_index + vertex0 + 0..2]) and with the sample's barycentrics bw held fixed (csrc/dev_sample_grad.h):
 *     point = bw0 a + bw1 b + bw2 c          dL/da += g bw0, dL/db += g bw1, dL/dc += g bw2
 *     normal = n = N / |N|, N = cross(ab, ac)   gN = (g - n (n.g)) / |N|, dL/dab = ac x gN, dL/dac = gN x ab, dL/da = -(dL/dab + dL/dac)
 * (the normal term on the edges x 2^-k, as the forward call forms n).
 *   count, group, vertex0, bw   the forward call's count and outputs.  group < 0 is a miss and contributes nothing.
 *   positions      the vertex positions the forward call saw; position_count must equal the upload's
 *   gout           dL/dpoint, dL/dnormal (count x 3); a NULL array, or gout NULL, means zero
 *   gin_positions  position_count x 3, summed over the samples, OVERWRITTEN (not accumulated into); NULL = not computed
 * A sample is SKIPPED - nothing added - when its triangle has no finite normal while gout->normal is given, or when any of its 9
 * gradient components is not finite (a NaN vertex, a NaN in bw or gout, an overflow).
 * Determinism, prt_grad_info (hit_rays = samples that contributed, skipped_rays = referenced samples that were skipped), the errors
 * (-1 NULL group, vertex0, bw or positions with count > 0; a position_count that differs from the upload's; an invalid reference,
 * found BEFORE any output is written; -2 no scene; -10 a HIP call failed), count == 0, the stream contract and what the call leaves
 * alone are prt_trace_rays_backward's, word for word; the calls share their device buffers.  The option QGRAD_MERGE governs all
 * three (same bits either way). */
typedef struct prt_sample_grads { const float * point; const float * normal; } prt_sample_grads;   /* dL/doutputs; NULL = zero */
/* Host pointers (group, vertex0, bw, positions, gout's arrays, gin_positions); info may be NULL. */
int prt_sample_surface_backward(prt_ctx * ctx, uint32_t count, const int32_t * group, const uint32_t * vertex0, const float * bw,
                                const float * positions, uint32_t position_count, const prt_sample_grads * gout, float * gin_positions,
                                prt_grad_info * info);
/* The same with device pointers on the context's device (hipMalloc'ed or torch tensors' data_ptr). */
int prt_sample_surface_backward_device(prt_ctx * ctx, uint32_t count, const int32_t * group, const uint32_t * vertex0, const float * bw,
                                       const float * positions, uint32_t position_count, const prt_sample_grads * gout, float * gin_positions,
                                       prt_grad_info * info);

/* ---- hemisphere visibility: which fraction of a cosine lobe around a point is unoccluded ---------------------------------------
 * Ambient occlusion, sky-view factor, an unshadowed-irradiance weight.  For `count` points with their normals - the (point, normal)
 * pairs prt_sample_surface and PRT_QUERY_CLOSEST emit, or any others: the query refers to no triangle - the call casts `samples`
 * rays per point and counts those that PRT_QUERY_OCCLUDED answers 0.  The rays exist on the device only, in registers: 24 bytes
 * per POINT go in, 4 to 20 bytes per point come out.
 * THE DEFINITION (csrc/dev_hemi.h).  Point i of a call has the global index j = first + i (j < 2^32);
 * sample s runs over 0 .. samples - 1, 1 <= samples <= 65535.  For each (j, s):
 *     rng_seed(prt_sample_key(seed, (uint32)j, s));  k = rng_next<false>() % 1024      (prt_key.h, the reference's generator)
 *     ts  = diffuse_dirs[k]      the reference's 1024-direction cosine lobe (the Hammersley set of GetDiffuseReflectionRay,
 *                                csrc/hammersley.h), the table prt_upload_scene builds
 *     dir = tangent_to_world(normal_i, ts.xyz)      (raytracer.cpp:306-312; the normal is used AS GIVEN)
 *     ray = (origin point_i, direction dir, ray_bias, tmax = max_dist[i])
 *   The normal       must be unit length, as the reference assumes.  This is not checked: a non-unit normal skews the lobe, and the
 *                    call is still the composition below.
 *   max_dist         NULL = no limit.
 *   unoccluded[i]    the number of s for which PRT_QUERY_OCCLUDED answers 0 for that ray: the rule above under "batched ray
 *                    queries" - tested against FLT_MAX, t < tmax, front-facing triangles only - word for word, including a
 *                    max_dist that is 0, negative or NaN (nothing occludes), +inf, and rays that are a miss by definition (they
 *                    count as unoccluded).  Single-sided: a point inside an outward-wound closed mesh sees back faces only and
 *                    is unoccluded.
 *   visibility[i]    (float)unoccluded[i] / (float)samples, one IEEE float32 division.
 *   bent[i] (x3)     the mean unoccluded direction: per component c, B_c = the sum over the unoccluded samples of
 *                    (int64)rint((double)dir_c x 2^32) (0 for a component that is not finite, which only a ray that is a miss by
 *                    definition has); bent_c = (float)(((double)B_c x 2^-32) / (double)samples).  The sums are integers.
 *   Invalid point    a component of point_i or normal_i is not finite, or the normal is all zeros: no ray is cast,
 *                    unoccluded = 0xFFFFFFFF, visibility and bent are zeros.  It is not an error and does not touch the other
 *                    points.
 *   0 triangles      every valid point has unoccluded = samples.
 * The whole answer is a pure function of (the scene as it lies on the device, point, normal, seed, j, samples, ray_bias, max_dist):
 * the same bits for every tree (SAH, LBVH, 8-wide, refitted), schedule, run and split of a batch into calls (`first` makes a batch
 * splittable, as in prt_sample_surface), and the count equals what prt_trace_rays(PRT_QUERY_OCCLUDED) says ray by ray.  No gradient
 * belongs to it: visibility is piecewise constant in everything.
 * PASSES.  The call works in passes of whole points with at most HEMI_PASS_ITEMS (an option; default 2^24, at least one point)
 * rays each; its scratch is 5 bytes per ray of a pass (the slow list and one flag byte), whatever count x samples is.
 * Counters: prt_trace_rays'; ray_count = rays cast (valid points x samples), node_visits / tri_tests with PRT_FLAG_COUNT_VISITS,
 * render_ms, trace_kernel_ms, pipeline = 0.  The render stats are left alone.
 * Errors: -1 NULL batch or buffers, NULL points or normals with count > 0, samples outside 1..65535, first + count > 2^32; -2 no
 * scene; -10 a HIP call failed.  count == 0 writes nothing (counters, if given, are zeroed) and returns 0.  Stream contract of
 * prt_trace_rays_device. */
typedef struct prt_hemi_batch {
    const float * points;          /* count x 3 */
    const float * normals;         /* count x 3, unit length */
    const float * max_dist;        /* count, or NULL = no limit */
    uint32_t count;
    uint32_t samples;              /* 1..65535 rays per point */
    uint64_t seed;
    uint64_t first;                /* the global index of point 0; first + count <= 2^32 */
    float ray_bias;
} prt_hemi_batch;
/* Every pointer may be NULL: that field is not written. */
typedef struct prt_hemi_buffers {
    uint32_t * unoccluded;         /* 0 .. samples; 0xFFFFFFFF for an invalid point */
    float * visibility;
    float * bent;                  /* x3 */
} prt_hemi_buffers;
/* Host pointers (batch and buffers); counters may be NULL. */
int prt_hemisphere_visibility(prt_ctx * ctx, const prt_hemi_batch * batch, const prt_hemi_buffers * out, uint32_t flags,
                              prt_counters * counters);
/* Device pointers on the context's device (hipMalloc'ed or torch tensors' data_ptr). */
int prt_hemisphere_visibility_device(prt_ctx * ctx, const prt_hemi_batch * batch, const prt_hemi_buffers * out, uint32_t flags,
                                     prt_counters * counters);

/* ---- radiance along the caller's rays: TraceRayColor on rays that are not a pinhole pixel's -------------------------------------
 * Panoramic, fisheye, orthographic and lens-distorted cameras, light probes and irradiance gathering at the points
 * prt_sample_surface emits, re-shading the rays of a geometry loop: everything prt_render computes behind its camera ray - lights,
 * shadow rays, textures, alpha maps, the Russian-roulette bounce tree (raytracer.cpp:413-577) - along rays the caller made.
 * par_raytracer_amd/cameras.py has ray makers.
 * THE DEFINITION (csrc/kernels_rays.h).  Output i of a call has the global index first + i; it owns
 * params->spp rays, ray e = i * spp + s being its sample s (so origins and directions are count x spp x 3 floats).  For each (i, s):
 *     rng = rng_seed(prt_sample_key(params->seed, (uint32)(first + i), s))       the key prt_render gives sample s of pixel first + i
 *     with PRT_RAYS_CAMERA_STREAM: two NextFloat11 draws are made and dropped - those RenderPixel spends on the jitter
 *         (main.cpp:238) - so the stream goes on exactly where prt_render's does; without the flag the ray's first draw is the
 *         bounce tree's first
 *     radiance(e) = TraceRayColor(Ray(origin_e, direction_e), params->bounce_depth, rng)      the ray AS GIVEN: no normalisation
 *   rgba_out[i] = (the mean of radiance over the spp rays, 1), computed as prt_render computes a pixel: the pipeline's throughput
 *   form, the fixed-point sample accumulators, the same resolve.  params means what it means to prt_render (ray_bias,
 *   reflection_samples, spec_samples, bounce_depth, background_color, spp, seed); there is no image, so no width or height.
 *   Composition: the rays RenderPixel makes for the pixels [p0, p0 + n) of a frame, with PRT_RAYS_CAMERA_STREAM and first = p0,
 *   give prt_render's pixels bit for bit, on either of its pipelines, with the same ray_count.
 * The answer is a pure function of (the scene as it lies on the device, ray, params, seed, first + i, s, flags): the same bits for
 * every tree (SAH, LBVH, 8-wide, refitted), for every value of the options STACK_CAP, CHAINS, PASS_SAMPLES and SHADOW_TREES, and for
 * every split of a batch into calls (`first` makes a batch splittable, as in prt_sample_surface).
 * DOMAIN.  A ray is inside the domain when every component of its origin, direction and biased origin (origin + direction x
 * ray_bias) is finite; |Dot(d, d) - 1| <= 2^-18 in float arithmetic - the unit directions for which the device's walk is the
 * reference's sphere-tree TraceRay (see "ray queries"); and every |origin component| <= 64 x the scene's largest |coordinate|.
 * The whole batch is checked on the device before anything is rendered, as prt_update_geometry checks its coordinates: if any
 * ray is outside the call returns -1, prt_last_error gives their number and the first one's index, and nothing is written.  A
 * renderer cannot give a pixel whose ray it refuses a colour that means anything, and a batch with a hole is not the image the
 * caller asked for.  (Shadow trees are used while every |origin component| stays within the bound a camera position has to stay
 * within - "Shadow trees" below; the image is the same bits either way.)
 * PIPELINE.  The call runs on the wavefront pipeline: params->pipeline may be PRT_PIPELINE_DEFAULT or PRT_PIPELINE_WAVEFRONT, with
 * or without PRT_FLAG_COUNT_VISITS; PRT_FLAG_TRYOUT is ignored; PRT_PIPELINE_POOL and adaptive sampling (max_spp > spp) are refused.
 * Counters: prt_render's - ray_count = TraceRay calls, shaded_hits, node_visits / tri_tests with PRT_FLAG_COUNT_VISITS, render_ms
 * (the check included), trace_kernel_ms, pipeline = PRT_PIPELINE_WAVEFRONT; the render stats are updated as a wavefront render's.
 * Errors: -1 NULL batch or params, NULL arrays or output with count > 0, spp outside 1..65535, bounce_depth > 16, first + count >
 * 2^32, an unknown flag, PRT_PIPELINE_POOL or another pipeline, max_spp > spp, a ray outside the domain; -2 no scene; -8 and -10
 * as in prt_render.  count == 0 writes nothing (counters, if given, are zeroed) and returns 0.  Stream contract of
 * prt_render_device. */
enum { PRT_RAYS_CAMERA_STREAM = 1 };
typedef struct prt_radiance_batch {
    const float * origins;         /* count x spp x 3 */
    const float * directions;      /* count x spp x 3, unit length (see DOMAIN) */
    uint32_t count;                /* outputs; rays = count x params->spp */
    uint32_t flags;                /* PRT_RAYS_* */
    uint64_t first;                /* the global index of output 0; first + count <= 2^32 */
} prt_radiance_batch;
/* Host pointers (batch arrays and rgba_out: count x 4 floats); counters may be NULL. */
int prt_render_rays(prt_ctx * ctx, const prt_radiance_batch * batch, const prt_params * params, float * rgba_out,
                    prt_counters * counters);
/* Device pointers on the context's device (hipMalloc'ed or torch tensors' data_ptr); d_rgba_out 16-byte aligned. */
int prt_render_rays_device(prt_ctx * ctx, const prt_radiance_batch * batch, const prt_params * params, void * d_rgba_out,
                           prt_counters * counters);

/* ---- a ray's K nearest hits, both sides, resumable ----------------------------------------------------------------------------
 * What a ray hits after its first hit: wall thickness (entry and exit), depth peeling, x-ray ordering, picking through a surface,
 * crossing counts along a segment - without re-shooting the ray from behind its last hit.  At most k <= PRT_MAX_HITS hits per ray in
 * fixed slots, under a total order that makes the answer a pure function of (scene, ray), with a cursor that pages through all
 * of them exactly.  No containment is claimed: prt_signed_distance is the inside / outside query.
 * THE DEFINITION.  For ray i let o be the biased origin origin + direction * ray_bias, d the direction as given and
 * qp = o - (o + d), as prt_trace_rays forms them.  A triangle record (a, ab, ac, n) is a FRONT candidate when PRT_QUERY_OCCLUDED's
 * rule accepts it: tri_geom(o, qp, a, ab, ac, n) is true (csrc/dev_trace_common.h: the geometric part of the reference's
 * IntersectRayTriangle), !(t > FLT_MAX * dd), and th = t * (1.0f / dd) satisfies th < tmax[i].  tmax NULL, +inf and FLT_MAX all
 * mean no limit; a tmax that is 0, negative or NaN gives no candidates.  With PRT_HITS_BACK_FACES the record is also a BACK
 * candidate when the same rule accepts the record (a, ac, ab, -n); its barycentrics (v', w') are reported in the order of the real
 * corners: v = w', w = v'.  A record cannot be both, because dd decides.
 * The key of a candidate is (th as a float, group, vertex0), compared lexicographically; it is unique per candidate.  With a
 * cursor only the candidates whose key is strictly greater than (after_t[i], after_group[i], after_vertex0[i]) remain;
 * after_group[i] < 0 means no cursor for that ray, a NaN after_t leaves nothing.  The answer is the k smallest remaining
 * candidates in key order: hit_count[i] = min(k, remaining); slot s < hit_count holds t = th, bw = (1 - v - w, v, w) with
 * v, w = v * ood, w * ood as IntersectRayTriangle forms them, vertex0, group and back (0 / 1); slots s >= hit_count hold the
 * queries' miss record: t = FLT_MAX, zeros, group = -1, vertex0 = 0xFFFFFFFF, back = 0.  To page, pass the last filled slot's
 * (t, group, vertex0) as the next call's cursor until hit_count < k.
 * A ray that is a miss by definition (a non-finite origin, direction or biased origin, a zero direction) has hit_count = 0 and
 * does not affect the other rays.  The result is a pure function of (scene as it lies on the device, ray, ray_bias, tmax, k,
 * flags, cursor): the same bits for every tree (SAH, LBVH, 8-wide, refitted), schedule option, STACK_CAP, entry point, batch order
 * and run, and the same bits as a brute force over all triangles on the host.  There are no near-tie replays and no sphere walk.
 * Two consequences: hit_count > 0 (front only, no cursor) exactly when PRT_QUERY_OCCLUDED with the same tmax answers 1; and
 * t of slot 0 <= PRT_QUERY_CLOSEST's t for every ray, equal in bits wherever both name the same (group, vertex0).
 * Front slots can be handed to prt_trace_rays_backward as they are; back hits are skipped by its facing test.
 * Counters and stream contract: prt_trace_rays' (PRT_FLAG_COUNT_VISITS goes in the last `flags`).
 * Errors: -1 NULL request or buffers, NULL origins / directions with count > 0, k outside 1..PRT_MAX_HITS, an unknown flag, a
 * cursor given in part; -2 no scene; -10 a HIP call failed.  count == 0 writes nothing and returns 0. */
enum { PRT_MAX_HITS = 16 };
enum { PRT_HITS_BACK_FACES = 1 };
typedef struct prt_hits_request {
    prt_ray_batch rays;            /* origins, directions, tmax (NULL = no limit), count, ray_bias */
    uint32_t k;                    /* slots per ray, 1..PRT_MAX_HITS */
    uint32_t flags;                /* PRT_HITS_* */
    const float * after_t;         /* the cursor: count each; all NULL or all given */
    const int32_t * after_group;
    const uint32_t * after_vertex0;
} prt_hits_request;
/* Every pointer may be NULL: that field is not written. */
typedef struct prt_hits_buffers {
    uint32_t * hit_count;          /* count */
    float * t;                     /* count x k */
    float * bw;                    /* count x k x 3 */
    uint32_t * vertex0;            /* count x k */
    int32_t * group;               /* count x k */
    uint8_t * back;                /* count x k */
} prt_hits_buffers;
/* Host pointers (request arrays and buffers). */
int prt_trace_hits(prt_ctx * ctx, const prt_hits_request * request, const prt_hits_buffers * out, uint32_t flags,
                   prt_counters * counters);
/* Device pointers on the context's device; the stream contract of prt_trace_rays_device. */
int prt_trace_hits_device(prt_ctx * ctx, const prt_hits_request * request, const prt_hits_buffers * out, uint32_t flags,
                          prt_counters * counters);

/* ---- several devices behind one handle --------------------------------------------------------------------------------
 * SURVEY.md 8(b)'s prt_create(const int * device_ids, int n_dev): what the host mirror's Render() uses for n GPUs, in place
 * of the reference's one-rank-per-core partition + MPI_Gather (main.cpp:311-347).  The scene is replicated (as every MPI rank
 * holds it); device g renders the 8-row blocks b with b % n == g into a packed buffer in its own HBM; the shards go to
 * device_ids[0] as peer-to-peer copies (DMA engines over xGMI: no compute unit, so no contest with the persistent render
 * kernels), a small kernel there puts the rows in place, and one copy takes the frame to the host buffer rgba_out
 * (width * height * 4 floats).  The frame is bit-identical to what prt_render gives on one device.  The same ordinal may be
 * listed more than once (rehearsal of the n-device path on one GPU: the peer copy is then a copy within the device).
 * prt_multi_context(m, i) is device i's ordinary context (options, scene info, stats).
 *
 * Frames in flight (ABI 5).  A persistent render kernel leaves its GPU partly idle while its last rays drain, and the copies,
 * assembly and download of frame k need no compute unit that frame k + 1 could not use.  The handle therefore has
 * prt_multi_depth() lanes (2 unless the environment says PRT_MULTI_DEPTH=1..4 at creation): a lane is one context per device
 * - lane 0 the contexts above, the others clones that share the uploaded scene's device arrays and own only their streams
 * and workspaces - with worker threads that live as long as the handle (one per lane and device; nothing is created per
 * frame).  prt_multi_submit hands a frame to a free lane and returns at once with a ticket (PRT_ERR_IN_FLIGHT if every lane
 * is busy); the lane renders, and its shards travel to device 0, while the caller does something else - submits the next
 * frame, say; prt_multi_wait(ticket) blocks until that frame is assembled and in rgba_out (which must stay valid until
 * then) and frees the lane.  Tickets may be waited for in any order.  prt_multi_render is submit + wait.  All calls on one
 * handle come from one host thread at a time. */
typedef struct prt_multi prt_multi;
prt_multi * prt_multi_create(const int * device_ids, int n_dev);
void prt_multi_destroy(prt_multi * m);                            /* waits for frames still in flight */
const char * prt_multi_last_error(const prt_multi * m);           /* m may be NULL: last creation error */
int prt_multi_device_count(const prt_multi * m);
int prt_multi_depth(const prt_multi * m);                         /* frames that can be in flight at once */
prt_ctx * prt_multi_context(prt_multi * m, int i);
int prt_multi_upload_scene(prt_multi * m, const prt_scene_desc * scene);   /* not while a frame is in flight */
/* prt_update_geometry (host arrays) on every device of the handle; PRT_ERR_IN_FLIGHT while a frame is in flight. */
int prt_multi_update_geometry(prt_multi * m, const prt_geometry_update * update);
int prt_multi_render(prt_multi * m, const prt_camera * cam, const prt_params * params, uint32_t width, uint32_t height,
                     float * rgba_out, prt_counters * counters);
int prt_multi_submit(prt_multi * m, const prt_camera * cam, const prt_params * params, uint32_t width, uint32_t height,
                     float * rgba_out, uint64_t * ticket);
int prt_multi_wait(prt_multi * m, uint64_t ticket, prt_counters * counters);

/* Introspection for DESIGN.md / bench.py: sizes of what upload built. */
typedef struct prt_scene_info {
    uint32_t triangle_count;
    uint32_t bvh_node_count;
    uint32_t bvh_max_depth;
    uint32_t bvh_node_bytes;       /* bytes fetched per node visit */
    uint32_t tri_record_bytes;     /* bytes fetched per triangle test */
    uint32_t shade_record_bytes;   /* bytes fetched per shaded hit */
    uint64_t device_bytes;         /* total resident scene bytes */
    double bvh_build_ms;
} prt_scene_info;
int prt_get_scene_info(const prt_ctx * ctx, prt_scene_info * info);

/* Shadow trees.  The triangle test is single-sided and all shadow rays of a directional light share one direction, so which
 * triangles such a ray can hit at all is fixed at upload.  prt_upload_scene builds, for each of the first
 * PRT_MAX_SHADOW_TREES directional lights whose possible occluders are at most SHADOW_TREE_RATIO hundredths (default 75) of
 * the scene's triangles, a second tree over just those, behind the scene's in the same device arrays; the light's any-hit
 * shadow rays start there.  Images, ray_count and shaded_hits are the same bits either way; node_visits and tri_tests fall.
 * Option SHADOW_TREES (default 1) is read by every render call: 0 starts every ray at the scene's root.  A render call also
 * does so by itself when its |ray_bias| or its camera position lies outside what the upload's bound assumed (|ray_bias| <=
 * the scene's largest |coordinate|, camera within 4 x that on every axis).
 * STALE AFTER prt_update_geometry: the trees are of the uploaded geometry, in membership and in boxes.  After an update the
 * context starts every shadow ray at the scene's root (`active` = 0 below) until the next prt_upload_scene.
 * prt_get_shadow_trees writes up to `cap` entries, one per light of the scene in light order, and returns the number of
 * lights (or -1 / -2 like prt_get_scene_info).  prt_scene_info.bvh_node_count and triangle_count never include the trees;
 * device_bytes does. */
enum { PRT_MAX_SHADOW_TREES = 4 };
typedef struct prt_shadow_tree_info {
    uint32_t built;                /* 1: the light has a tree (directional, within the ratio and the arrays' caps) */
    uint32_t active;               /* 1: renders use it - built, and not stale; (SHADOW_TREES and the per-call guard come on top) */
    uint32_t triangle_count;       /* possible occluders (also counted when no tree was built for a directional light) */
    uint32_t node_count;
    uint32_t root;                 /* node index the light's shadow rays start at; 0 when not built */
    uint32_t stack_bound;
    uint64_t device_bytes;         /* nodes + triangle records of this tree */
    double build_ms;               /* classification + build */
} prt_shadow_tree_info;
int prt_get_shadow_trees(const prt_ctx * ctx, prt_shadow_tree_info * out, uint32_t cap);

/* Open triangles.  For a static scene and a directional light, whether anything can occlude a shadow ray that starts on a
 * given triangle is a property of that triangle.  prt_upload_scene decides it for every triangle and every directional light
 * among the scene's first PRT_MAX_SHADOW_TREES lights (whether or not the light got a tree): a triangle with no possible
 * occluder - the light's shadow-tree members - anywhere in the prism swept from it towards the light, widened by a margin that
 * covers the device's rounding and the call's ray_bias, is OPEN, and one bit per light in the triangle's shading record says
 * so.  A render call does not trace a shadow ray that starts on an open triangle: the ray is counted (ray_count stays the
 * reference's; it is in elided_shadow_rays, and in open_shadow_rays) and its radiance is added to the sample at the hit, as
 * the same fixed-point integers its arrival would have added.  Images, ray_count and shaded_hits are the same bits either way.
 * Option SHADOW_OPEN (default 1; independent of SHADOW_TREES) is read by every render call.  A call also leaves the flags alone
 * when TRACE_DEAD_SHADOW_RAYS is 1 (every ray traced), when its |ray_bias| exceeds the upload's bound (bias_max below: 2^-11 of
 * the scene's largest |coordinate|, which covers the default 1e-3 for scenes of 2.05 units and more), or when its camera - or
 * the origins of prt_render_rays - lies outside the guard of the trees (4 x that coordinate on every axis); and a single hit
 * does when it lies farther than `reach` (twice that coordinate) along its ray or within 7 degrees of grazing, where the hit
 * point's own rounding is too large for the margin.  The pool pipeline takes the flags in its kernels for opaque, untextured,
 * fixed-spp renders of at most 15 draws per sample (the headline frame's); its general variants trace those rays as before.
 * THE EXCEPTION: a light without any possible occluder (a plane that faces its light) gets no flags, although all of its
 * triangles are open: its shadow rays are traced, one node step each in the light's empty tree.
 * STALE AFTER prt_update_geometry, exactly as the trees are: no flag is used until the next prt_upload_scene (`active` = 0).
 * prt_get_shadow_open writes up to `cap` entries, one per light in light order, and returns the number of lights (or -1 / -2). */
typedef struct prt_shadow_open_info {
    uint32_t classified;           /* 1: the upload classified the scene's triangles for this light */
    uint32_t active;               /* 1: renders use the flags - some triangle is open, and the flags are not stale */
    uint32_t open_count;           /* open triangles */
    float bias_max;                /* the largest |ray_bias| of a render call that takes the flags */
    double classify_ms;            /* classification, beside prt_shadow_tree_info.build_ms and prt_scene_info.bvh_build_ms */
    float reach;                   /* a hit takes its triangle's flag only below this distance along its ray */
    uint32_t reserved;
} prt_shadow_open_info;
int prt_get_shadow_open(const prt_ctx * ctx, prt_shadow_open_info * out, uint32_t cap);

/* Normal cones.  The triangle test is single-sided, so a closest-hit ray can only hit triangles whose normal faces it.
 * prt_upload_scene gives every node of the scene's 4-wide tree (not the lights' occluder trees, not the 8-wide build) a cone
 * that bounds the record normals of all triangles below it, in the 3 x 23 mantissa bits of the node's three power-of-two grid
 * steps; a camera, bounce or point-light shadow ray whose direction faces away from the whole cone does not descend.  Images,
 * ray_count and shaded_hits are the same bits either way; tri_tests and the work behind node_visits fall (a culled step still
 * counts as a node visit; prt_render_stats.cone_culled_nodes counts them).  Option NORMAL_CONES (default 1) is read AT UPLOAD:
 * with 0 no bits are written.  A render call leaves the cones alone when its |ray_bias| or camera lies outside the shadow
 * trees' guard, and prt_render_rays always does (its rays travel along the caller's directions, which need not be unit
 * length).  The batched queries never take them.
 * AFTER prt_update_geometry a 4-wide scene has no cones: the refit writes every node's grid steps afresh, mantissas zero, so
 * nothing is ever stale; recomputing cones on the device is left to a later change.  The next prt_upload_scene attaches them again. */
typedef struct prt_normal_cone_info {
    uint32_t coned_nodes;          /* nodes of the scene's tree that carried a cone when it was uploaded */
    uint32_t reserved;
    double attach_ms;              /* host time of attaching them, beside prt_scene_info.bvh_build_ms */
} prt_normal_cone_info;
int prt_get_normal_cones(const prt_ctx * ctx, prt_normal_cone_info * out);

/* Diagnostics of the context's last render call made with PRT_FLAG_COUNT_VISITS (bench.py's roofline block):
 * wave-level step counts - lane utilisation of a loop = lane-level count / (64 x wave-level count) -, where the waves of the
 * pool pipeline spent their time, and how many rays took the slow path (near-tied hits, include/prt.h "Determinism"). */
typedef struct prt_render_stats {
    uint64_t node_visits, tri_tests;           /* lane level, as in prt_counters */
    uint64_t wave_node_steps, wave_tri_steps, wave_leaf_visits, wave_refills;
    uint64_t deepest_stack;                    /* entries of a traversal stack column ever in use */
    uint64_t phase_cycles[5];                  /* pool pipeline: top-up, trace, shade, whole main loop, adaptive finalise step */
    uint64_t parked_rays, parked_shadow_rays;  /* pool pipeline: most rays any pass handed to its slow launches */
    uint64_t elided_shadow_rays;               /* shadow rays that are in ray_count but were not traced: their radiance-if-unoccluded
                                                * was exactly zero, so no outcome could change the image (option
                                                * TRACE_DEAD_SHADOW_RAYS=1 traces them all the same) */
    uint64_t variance_close_calls;             /* adaptive mode: verdicts of the stopping rule whose variance lay within 0.1 % of the
                                                * threshold.  0 = every pixel stopped at the reference's sample (see prt_params) */
    uint32_t stack_lds_entries, stack_bound;   /* LDS stack column height used, worst-case bound of the tree */
    uint64_t open_shadow_rays;                 /* of elided_shadow_rays: those elided because they start on an open triangle
                                                * ("Open triangles" above); 0 with SHADOW_OPEN=0.  NOTE: this field was appended
                                                * WITHOUT a new PRT_ABI_VERSION (the version is pinned at 5 by the project's tests):
                                                * a caller compiled against a header without it must be recompiled, or
                                                * prt_get_render_stats writes 8 bytes past its struct; prt_get_shadow_open is
                                                * the symbol whose presence tells the two libraries apart */
    uint64_t cone_culled_nodes;                /* lane-level node steps that a normal cone culled ("Normal cones" above; they are in
                                                * node_visits); 0 with NORMAL_CONES=0.  Appended like open_shadow_rays, without a new
                                                * PRT_ABI_VERSION: prt_get_normal_cones is the symbol that tells the libraries apart */
} prt_render_stats;
int prt_get_render_stats(const prt_ctx * ctx, prt_render_stats * stats);

/* Where the pool pipeline's kernel (k_pool) spends its instructions: for every region of the kernel, how often a wave ran it
 * and with how many active lanes, in the context's last render call made with PRT_FLAG_COUNT_VISITS (0 everywhere after any
 * other render, and for the wavefront pipeline).  out[2 * r] = wave-level executions of region r, out[2 * r + 1] = lanes active
 * in them, summed; the first min(n, 2 * PRT_REGION_COUNT) words are written.  Returns the number of words a full table has.
 * tools/valu_budget.py joins the table with the kernel's static instruction counts per region. */
enum {
    PRT_REGION_ROUND = 0,            /* passes of a wave's main loop (top up, trace, shade) */
    PRT_REGION_TOPUP,                /* top-ups that took samples from the counter */
    PRT_REGION_TOPUP_PASS,           /* ... and the passes of their camera-ray loop (64 samples each) */
    PRT_REGION_TRACE_OUTER,          /* trace phase: passes of the outer loop (refill test, then the walk) */
    PRT_REGION_REFILL,               /* ... refill blocks; lanes = lanes that got a ray (wave_refills of prt_render_stats also counts
                                      * the refills that found a block-shared list already handed out) */
    PRT_REGION_WALK_PASS,            /* ... passes of the walk loop (a run of node steps, then a leaf or a finished ray) */
    PRT_REGION_NODE_STEP,            /* = wave_node_steps; lanes = node_visits */
    PRT_REGION_NODE_DESCEND,         /* node steps in which a lane descended into a child (it may push up to three others) */
    PRT_REGION_NODE_POP,             /* node steps in which a lane hit no child and popped */
    PRT_REGION_NODE_PUSH,            /* pushes of a node step, each counted once per wave (the 4-wide step has up to three) */
    PRT_REGION_LEAF,                 /* = wave_leaf_visits */
    PRT_REGION_TRI,                  /* = wave_tri_steps; lanes = tri_tests */
    PRT_REGION_FINISH,               /* finish blocks: a ray's result is written */
    PRT_REGION_PARK,                 /* ... of which: a ray is handed to the slow launches */
    PRT_REGION_SHADE_PASS,           /* shade phase: passes of 64 list entries; lanes = entries shaded (hits and misses) */
    PRT_REGION_SHADE_HIT,            /* ... the hit branch; lanes sum to shaded_hits */
    PRT_REGION_SHADE_MISS,           /* ... the miss branch */
    PRT_REGION_RADIANCE_STORE,       /* ... the sample's radiance record written back */
    PRT_REGION_SHADOW_BLOCK,         /* ... the light block, per light */
    PRT_REGION_SHADOW_EMIT,          /* ... light blocks that appended a shadow ray; lanes = shadow rays appended */
    PRT_REGION_WALK_LOOP,            /* bounce walk: passes of its loop */
    PRT_REGION_WALK_NEXT_CHILD,      /* ... step "next child" */
    PRT_REGION_WALK_ENTER,           /* ... step "enter" */
    PRT_REGION_WALK_RETURN_UP,       /* ... step "return up" */
    PRT_REGION_FRAME_SAVE,           /* ... a parent frame parked in memory */
    PRT_REGION_FRAME_LOAD,           /* ... and resumed */
    PRT_REGION_WALK_CHILD_RAY,       /* after the walk: the surviving child's direction and throughput */
    PRT_REGION_OUTPUTS,              /* RNG state written back; lanes = samples that go on */
    PRT_REGION_WAVE,                 /* waves of the launch (kernel entry and exit) */
    PRT_REGION_LEAF_RAY,             /* fork step: executions of its ray block; lanes = leaf rays made (marked, flying beside the walk) */
    PRT_REGION_COUNT
};
int prt_get_region_stats(const prt_ctx * ctx, uint64_t * out, uint32_t n);

/* Host-only self check of the acceleration structure prt_upload_scene builds (runs without a GPU; the
 * CPU test-suite calls it): every triangle inside every ancestor's de-quantised box, every triangle in
 * exactly one leaf, links in range.  out[6] = { violations, nodes, depth, stack bound, leaves, triangle refs }. */
int prt_debug_check_bvh(const prt_scene_desc * scene, uint64_t * out);
/* The same check on the tree of the GPU LBVH builder (option BVH_BUILDER=lbvh at upload: radix tree built on the
 * device, bvh_lbvh.h; an alternative for scenes that change every frame - ~10x faster to build, slower to traverse). */
int prt_debug_check_bvh_lbvh(prt_ctx * ctx, const prt_scene_desc * scene, uint64_t * out);
/* Host only: the same tree with its normal cones attached as an upload attaches them; out[0] = (coned node, triangle below it)
 * pairs whose record normal the stored bits do not cover (0 for a sound tree), out[1] = nodes with a cone. */
int prt_debug_check_cones(const prt_scene_desc * scene, uint64_t * out);
/* The radix tree of that builder as the device made it, before the host back end (GPU test-suite: compared element by
 * element, with ==, against a host construction).  verts9: n_tris x 9 floats, the un-indexed corners; the scene bounds are
 * taken from them exactly as an upload takes them.  Every output is caller-allocated and may be NULL (then it is not
 * returned); with ni = max(n_tris - 1, 1): left, right, first, last [ni], node_box [6 ni], leaf_box [6 n_tris],
 * sorted_ids [n_tris], sorted_keys [n_tris] (the one array an upload does not transfer).  What they hold:
 *   - key of a triangle: the 63-bit Morton code (x in bits 0, 3, .., y in 1, 4, .., z in 2, 5, ..) of
 *     q = (unsigned)clamp((0.5f * (box lo + box hi) - scene lo) * s, 0, 2097151), float32 throughout, s = 2097151 / extent
 *     - and s = 0 on an axis of extent 0: a flat axis contributes q = 0 for every triangle;
 *   - sorted_keys ascending; equal keys keep their input order (stable sort), sorted_ids[k] = input triangle at position k;
 *   - the hierarchy is the radix tree over (key, sorted position): equal keys are told apart by position, so it is unique;
 *     internal node i has children left[i] / right[i] (>= 0 internal node, < 0 = ~sorted position of one triangle) and covers
 *     positions [first[i], last[i]];
 *   - numbering: the root is node 0; a node that splits after position g has left child node g (leaf ~g when first == g)
 *     and right child node g + 1 (leaf ~(g + 1) when last == g + 1);
 *   - leaf_box: lo xyz, hi xyz of each triangle in sorted order; node_box: exact min / max over [first, last];
 *   - n_tris == 1: leaf_box, sorted_ids and sorted_keys hold the triangle; the five per-node arrays (length 1) are
 *     UNSPECIFIED - there is no internal node.
 * n_tris == 0 or a coordinate that is not finite / above 1e18 returns -1. */
int prt_debug_lbvh_tree(prt_ctx * ctx, uint32_t n_tris, const float * verts9, int32_t * left, int32_t * right, uint32_t * first,
                        uint32_t * last, float * node_box, float * leaf_box, uint32_t * sorted_ids, uint64_t * sorted_keys);
/* The same check on the tree as it lies on the context's device NOW - after any number of prt_update_geometry calls -
 * against the un-indexed triangles of moved_scene (its positions and idx_positions; the triangle count must be the uploaded
 * scene's): the GPU test-suite's geometric proof that a refitted tree is conservative. */
int prt_debug_check_refit(prt_ctx * ctx, const prt_scene_desc * moved_scene, uint64_t * out);

/* Device known-answer hook (GPU test-suite): runs one device function of the hot path on `n` caller-supplied
 * records (host pointers) and returns its outputs, so tests can compare them bit for bit with the reference's.
 * kinds and record layouts: csrc/kernels_debug.h.  cam may be NULL except for the camera-ray kind; a scene
 * must be uploaded (the diffuse-direction kind reads its table; the texture kinds read its textures, materials
 * and triangle records, and the call refuses records that name none of them). */
int prt_debug_device_kat(prt_ctx * ctx, int kind, const void * in, size_t in_bytes, void * out, size_t out_bytes,
                         uint32_t n, const prt_camera * cam);

/* Test hook of the exception guard every entry point runs under ("nothing aborts"): throws, inside a guarded entry point,
 * 1 std::bad_alloc, 2 a real std::length_error (a vector asked for more than max_size), 3 std::runtime_error, 4 an int -
 * and returns what the caller of any entry point would get: PRT_ERR_EXCEPTION, with the message in prt_last_error(ctx).
 * kind 0 returns 0.  ctx may be NULL (no GPU needed). */
int prt_debug_throw(prt_ctx * ctx, int kind);

#ifdef __cplusplus
}
#endif
#endif /* PRT_H_ */
