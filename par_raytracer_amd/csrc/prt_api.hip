// prt_api.hip - implementation of the C ABI in include/prt.h: context, scene upload, render dispatch.
//
// One prt_ctx = one HIP device + one stream + one resident scene.  Upload builds the per-triangle BVH (bvh_build.cpp on the
// host, or bvh_lbvh.h on the device), has scene_pack.cpp flatten the scene into the records of dev_scene.h - host code with no
// HIP call in it -, uploads the arrays and only then commits: the scene is four structs of the context (SceneArrays, SceneDesc,
// SceneKeep, SceneTables), written together at the end of prt_upload_scene.  Render launches the selected pipeline on the
// context's stream; nothing in the render path allocates when the workspace from a previous call is large enough.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <condition_variable>
#include <mutex>
#include <new>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../../include/prt.h"
#include "bvh_build.h"
#include "scene_pack.h"
#include "prt_options.h"
#include "dev_scene.h"
#include "tex_upload.h"
#include "kernels_wave.h"
#include "kernels_pool.h"
#include "kernels_resolve.h"
#include "bvh_lbvh.h"
#include "kernels_debug.h"
#include "kernels_query.h"
#include "kernels_refit.h"
#include "kernels_query_grad.h"
#include "kernels_closest.h"
#include "kernels_closest_grad.h"
#include "kernels_signed.h"
#include "kernels_sample.h"
#include "kernels_sample_grad.h"
#include "kernels_hemi.h"
#include "kernels_rays.h"
#include "kernels_hits.h"
#include "hammersley.h"

using namespace prt;

#ifndef PRT_ADAPT_WAVES
#define PRT_ADAPT_WAVES 4         // waves per SIMD of the untextured adaptive kernel (128 VGPRs)
#endif
#ifndef PRT_POOL_FORK_DEFAULT
#define PRT_POOL_FORK_DEFAULT 1   // leaf rays fly beside the bounce walk (kernels_pool.h FORKS) when the option POOL_FORK is not set
#endif
#ifndef PRT_POOL_SHARED_DEFAULT
#define PRT_POOL_SHARED_DEFAULT 1 // block-shared pools (kernels_pool.h) for fixed-spp renders when the option POOL_SHARED is not set
#endif
#ifndef PRT_POOL_BLOCK
#define PRT_POOL_BLOCK 256        // threads per workgroup of the fixed-spp pool kernel (experiments: 320, 640 with block-shared pools)
#endif
#ifndef PRT_QGRAD_MERGE_DEFAULT
#define PRT_QGRAD_MERGE_DEFAULT 1 // prt_trace_rays_backward, prt_closest_points_backward: lanes of a wave on one triangle merge their adds (same bits either way)
#endif
#ifndef PRT_DEEP_WAVES
#define PRT_DEEP_WAVES PRT_POOL_WAVES   // waves per SIMD of the fixed-spp kernel for bounce trees of more than 15 draws (C5)
#endif
#ifndef PRT_POOL_WAVES
#define PRT_POOL_WAVES 5          // waves per SIMD of the fixed-spp pool kernel: 96 VGPRs (6 = 80 VGPRs spills, profiles/r03_ab_bvh8.txt)
#endif

// The acceleration structure the library is built with (dev_trace.h): the 4-wide sorted tree, or -DPRT_BVH8 the 8-wide one
// of round 3.
enum { BVH_WIDTH = BVH_NODE_BYTES == 4 * BVH8_NODE_DWORDS ? 8 : 4 };

namespace {

std::string g_create_error;

#define HIP_TRY(ctx, call)                                                                                   \
    do {                                                                                                     \
        hipError_t e_ = (call);                                                                              \
        if (e_ != hipSuccess) {                                                                              \
            (ctx)->error = std::string(#call) + ": " + hipGetErrorString(e_);                                \
            return -10;                                                                                      \
        }                                                                                                    \
    } while (0)

template <typename T>
struct DevBuf {
    T * p = nullptr;
    size_t n = 0;
    bool borrowed = false;               // p belongs to another DevBuf (clone_context: the scene arrays of the context cloned)
    void borrow(const DevBuf & o) { release(); p = o.p; n = o.n; borrowed = o.p != nullptr; }
    hipError_t ensure(size_t count) {
        if (count <= n && p) return hipSuccess;
        if (p && !borrowed) (void)hipFree(p);
        borrowed = false;
        p = nullptr;
        n = 0;
        hipError_t e = hipMalloc((void **)&p, std::max<size_t>(count, 1) * sizeof(T));
        if (e == hipSuccess) n = count;
        return e;
    }
    hipError_t upload(const T * v, size_t count) {
        hipError_t e = ensure(count);
        if (e != hipSuccess || !count) return e;
        return hipMemcpy(p, v, count * sizeof(T), hipMemcpyHostToDevice);
    }
    hipError_t upload(const std::vector<T> & v) { return upload(v.data(), v.size()); }
    void release() {
        if (p && !borrowed) (void)hipFree(p);
        borrowed = false;
        p = nullptr;
        n = 0;
    }
    size_t bytes() const { return n * sizeof(T); }
};

// The uploaded scene on the device: the arrays a clone borrows (clone_context).  What the host knows about them is the
// context's SceneDesc (scene_pack.h); the kernels' view of them is its DevScene.
struct SceneArrays {
    DevBuf<float4> nodes, tris, shade, diffuse_dirs;
    DevBuf<unsigned int> tri_rank;
    DevBuf<DevMaterial> materials;
    DevBuf<DevLight> lights;              // two copies of the table, desc.light_stride apart: shadow-tree roots in DevLight::pad, then every root at 0
    DevBuf<DevTexture> textures;
    DevBuf<unsigned int> texels;
    DevBuf<float> srgb_lut;
    DevBuf<float4> tri_uv, tri_tan;
    DevBuf<float4> ref_spheres;           // the reference's sphere tree for near-tie resolution (dev_trace_common.h RefSphereWalk)

    void borrow(const SceneArrays & o) {
        nodes.borrow(o.nodes); tris.borrow(o.tris); shade.borrow(o.shade); diffuse_dirs.borrow(o.diffuse_dirs);
        tri_rank.borrow(o.tri_rank); materials.borrow(o.materials); lights.borrow(o.lights);
        textures.borrow(o.textures); texels.borrow(o.texels); srgb_lut.borrow(o.srgb_lut);
        tri_uv.borrow(o.tri_uv); tri_tan.borrow(o.tri_tan); ref_spheres.borrow(o.ref_spheres);
    }
    void release() { borrow(SceneArrays()); }
    // Through the null stream.  The arrays a scene does not have (textures, tangents, spheres) keep what they held.
    hipError_t upload(const PackedScene & p) {
        hipError_t e = nodes.upload(reinterpret_cast<const float4 *>(p.nodes.data()), p.nodes.size() / 4);
        if (e == hipSuccess) e = tris.upload(p.tris);
        if (e == hipSuccess) e = shade.upload(p.shade);
        if (e == hipSuccess) e = tri_rank.upload(p.rank);
        if (e == hipSuccess) e = materials.upload(p.materials);
        if (e == hipSuccess) e = lights.upload(p.lights);
        if (e == hipSuccess) e = diffuse_dirs.upload(p.diffuse_dirs);
        if (e == hipSuccess && !p.ref_spheres.empty()) e = ref_spheres.upload(p.ref_spheres);
        if (e == hipSuccess && p.desc.textured) e = textures.upload(p.textures);
        if (e == hipSuccess && p.desc.textured) e = texels.upload(p.texels);
        if (e == hipSuccess && p.desc.textured) e = srgb_lut.upload(p.srgb_lut);
        if (e == hipSuccess && p.desc.textured) e = tri_uv.upload(p.tri_uv);
        if (e == hipSuccess && p.keep.bumped) e = tri_tan.upload(p.tri_tan);
        return e;
    }
    // The kernels' pointers; the optional arrays only where the scene has them.
    void point(DevScene & sc, bool textured, bool bumped, bool spheres) const {
        sc.nodes = nodes.p;
        sc.tris = tris.p;
        sc.shade = shade.p;
        sc.tri_rank = tri_rank.p;
        sc.materials = materials.p;
        sc.lights = lights.p;
        sc.diffuse_dirs = diffuse_dirs.p;
        sc.textures = textured ? textures.p : nullptr;
        sc.texels = textured ? texels.p : nullptr;
        sc.srgb_lut = textured ? srgb_lut.p : nullptr;
        sc.tri_uv = textured ? tri_uv.p : nullptr;
        sc.tri_tan = bumped ? tri_tan.p : nullptr;
        sc.ref_spheres = spheres ? ref_spheres.p : nullptr;
    }
};

// The device tables that calls build on first use from what the upload kept (SceneKeep; their host halves are in
// scene_pack.cpp), with the generation of the geometry each was filled from.  None is in prt_scene_info.device_bytes - a
// render-only user pays no device memory for them -, later calls reuse them, and the next upload frees them.
struct SceneTables {
    // ray queries (prt_trace_rays, kernels_query.h): the first query after an upload builds the leaf -> (group, vertex0) table
    // from the leaf order and the groups.
    DevBuf<uint2> q_leaf_map;             // leaf slot -> (group, vertex0)
    DevBuf<unsigned int> q_slot_of_rank;  // prt_trace_rays: the inverse of tri_rank (scan_closest); built with q_leaf_map's lifetime,
                                          // and again after a prt_update_geometry that ranks the triangles anew
    // geometry updates (prt_update_geometry, kernels_refit.h): the first update builds the leaf slot -> vertex indices table from
    // the index buffers (24 B per triangle).
    DevBuf<unsigned int> rf_table;        // leaf slot -> three position indices, three normal indices
    // query gradients (prt_trace_rays_backward, kernels_query_grad.h; prt_closest_points_backward, kernels_closest_grad.h).  Built
    // by the first call of either kind after an upload from the position index buffer and the groups.
    DevBuf<unsigned int> qg_idx;          // the position index buffer
    DevBuf<unsigned int> qg_runs;         // (first_index, index_count) per group
    DevBuf<long long> qg_acc;             // position_count x 3 fixed-point accumulators
    // signed distances (prt_signed_distance, dev_signed.h).  The adjacency table is topology: built by the first signed query
    // after an upload from the position index buffer and the leaf order.  The accumulators are geometry: k_signed_normals refills
    // them at the first signed query after an upload or a prt_update_geometry, which both bump geom_generation.
    uint64_t sg_generation = 0;           // of the records sg_acc was filled from; 0 = never
    DevBuf<unsigned int> sg_adj;          // leaf slot -> three position indices, three edge ids (24 B per triangle)
    DevBuf<long long> sg_acc;             // (position_count + sg_edge_count) x 3 fixed-point accumulators (24 B each)
    uint32_t sg_edge_count = 0;
    // surface samples (prt_sample_surface, dev_sample.h).  The input triangle -> leaf slot table is topology: the inverse of
    // the leaf order, built by the first sampling call after an upload (4 B per triangle).  The weights and their prefix sums are
    // geometry: rebuilt on the device (kernels_sample.h) by the first sampling call after an upload or a prt_update_geometry
    // (8 B per triangle of sums, 8 B per triangle of weights and 8 B per tile of scratch).
    uint64_t sm_generation = 0;           // of the records sm_prefix was built from; 0 = never
    DevBuf<unsigned int> sm_slot_of_input;
    DevBuf<double> sm_weight;
    DevBuf<unsigned long long> sm_prefix, sm_tile_sum;

    void release() {
        q_leaf_map.release(); q_slot_of_rank.release();
        rf_table.release();
        qg_idx.release(); qg_runs.release(); qg_acc.release();
        sg_adj.release(); sg_acc.release();
        sg_edge_count = 0;
        sg_generation = 0;
        sm_slot_of_input.release(); sm_weight.release(); sm_prefix.release(); sm_tile_sum.release();
        sm_generation = 0;
    }
};

}  // namespace

enum { PRT_MAX_CHAINS = 8 };

struct prt_ctx {
    int device = 0;
    PrtOptions opt;                       // every knob, read from the environment once at creation (prt_options.h, prt_set_option)
    hipStream_t stream = nullptr;
    hipEvent_t ev[4] = { nullptr, nullptr, nullptr, nullptr };
    std::string error;
    bool has_scene = false;

    // The uploaded scene.  prt_upload_scene empties `keep` and `tables` at its top, fills `arrays`, and commits `desc` and `keep`
    // in one step at its end, once every array lies on the device (has_scene says which side of that step the context is on).
    // A clone borrows `arrays`, copies `desc` and `scene`, and has no `keep` and no `tables` (clone_context).
    SceneArrays arrays;
    SceneDesc desc;                       // scene_pack.h: what the host knows about the arrays
    SceneKeep keep;                       // scene_pack.h: host memory for prt_update_geometry, the gradients, signed distances, sampling
    SceneTables tables;
    DevScene scene;                       // the kernels' view: SceneArrays::point, the counts, spec_dirs
    uint64_t geom_generation = 0;         // of the records on the device: an upload and a prt_update_geometry bump it (SceneTables)
    DevBuf<float4> spec_dirs;             // [material][spec_samples], rebuilt when a render asks for another spec_samples (build_spec_table)
    unsigned int spec_table_samples = 0;
    // PRT_PIPELINE_DEFAULT: which pipeline won the try-out for a (scene, pixel set, sampling) configuration
    struct TuneEntry { uint64_t key[6]; unsigned int pipeline; };
    std::vector<TuneEntry> tuned;
    uint64_t scene_epoch = 0;

    // render workspace
    DevBuf<float4> sample_rgb;
    DevBuf<float4> frame_out;
    DevBuf<DevCounters> counters;
    DevBuf<unsigned long long> ring_ws;
    DevBuf<unsigned int> pixel_list;
    // wavefront pipeline workspace
    // one set per chain: the frame is split into two halves that run their rounds on two streams, so that one
    // half's (latency-bound) k_shade overlaps the other half's (issue-bound) k_trace
    struct ChainWs {
        DevBuf<float4> f4;                // one slab carved into the float4 arrays of WaveBuffers
        DevBuf<ulonglong2> rng;
        DevBuf<unsigned int> counts;
        DevBuf<unsigned int> overflow;
        DevBuf<int> slow_stack;
        hipStream_t stream = nullptr;
        hipEvent_t ev_t0 = nullptr, ev_t1 = nullptr, ev_done = nullptr, ev_first = nullptr;
        unsigned int * host_counts = nullptr;   // pinned
    } chain[PRT_MAX_CHAINS];
    DevBuf<unsigned int> wf_counts;       // persistent / pool pipelines' sample counter
    DevBuf<float4> pool_f4;               // pool pipeline: the waves' private ray lists
    prt_render_stats last_stats;          // of the last render call (prt_get_render_stats)
    uint64_t last_regions[2 * PRT_REGION_COUNT] = {};      // ... and its region table (prt_get_region_stats)
    DevBuf<float4> pool_park;             // pool pipeline: rays parked for the slow launches (kernels_pool.h PoolBuffers::park)
    size_t pool_park_cap = 1u << 18, pool_spark_cap = 1u << 18;     // entries; enlarged when a frame needed more (render_pixels)
    DevCounters * host_counters = nullptr;                            // pinned: the render's counters arrive here on the context's stream
    DevBuf<unsigned int> pool_fin;        // adaptive mode: per-wave lists of pixels to finalise
    DevBuf<PoolArgs> pool_args;           // k_pool's arguments (read per phase from memory, kernels_pool.h)
    DevBuf<unsigned long long> wave_times;  // DEBUG_UTIL + counting render: (start, counter dry, exit) wall clock of every wave of the fast kernel
    unsigned int wave_times_n = 0;
    DevBuf<float4> adapt_f4;              // adaptive mode: scratch [max_spp][n] + running sums [n] + final colours [n]
    int cu_count = 0;                     // compute units this context may fill (all of the device's minus PRT_RESERVE_CUS)
    int reserved_cus = 0;
    DevBuf<int> stack_spill;
    // ray queries (prt_trace_rays, kernels_query.h)
    DevBuf<unsigned int> q_work;          // the batch's control words (BatchShared::work, dev_wave_loop.h)
    DevBuf<unsigned int> q_slow;          // rays handed to k_query_exact
    DevBuf<int> q_exact_stack;
    DevBuf<int> q_hits_lists;             // k_hits_exact's list columns (HitsArgs::exact_lists, kernels_hits.h)
    DevBuf<float> q_io;                   // host entry point: the batch and the requested fields on the device
    DevBuf<unsigned char> q_occ;
    DevBuf<unsigned char> q_hemi_flags;   // prt_hemisphere_visibility: one byte per item of a pass
    DevBuf<unsigned long long> rays_words;  // prt_render_rays: k_rays_check's three words
    // geometry updates (prt_update_geometry, kernels_refit.h): the scratch boxes and the inputs, reused by later updates
    DevBuf<RefitBox> rf_boxes;            // every node's exact float box
    DevBuf<unsigned int> rf_bounds;       // k_refit_bounds' two words
    DevBuf<float> rf_in;                  // host entry point: positions, normals, tangents on the device
    // query gradients (prt_trace_rays_backward, kernels_query_grad.h; prt_closest_points_backward, kernels_closest_grad.h)
    DevBuf<unsigned int> qg_words;        // k_qgrad_scan's control words
    DevBuf<float> qg_io;                  // host entry point: the inputs and the requested gradients on the device
    // surface samples (prt_sample_surface, dev_sample.h)
    DevBuf<unsigned long long> sm_words;
    unsigned long long sm_host_words[SAMPLE_WORDS] = {};   // the table's control words as last read back
    unsigned long long sm_read_words[SAMPLE_WORDS] = {};   // ... and where a rebuild's copy of them lands (it outlives a failed call)
};

namespace {

f3 ld3(const float * p) { return mk3(p[0], p[1], p[2]); }

// Dwords of `entries` traversal-stack entries for `lanes` lanes: the ONE place that knows how many dwords an entry of this
// build's traversal has (STACK_ENTRY_INTS: 1 for the 4-wide tree's links, 2 for the 8-wide tree's (base, masks) pairs).
// Every stack area - the LDS columns, their spill columns, the exact kernels' full-height global columns - is sized here.
size_t stack_dwords(size_t entries, size_t lanes) { return entries * lanes * (size_t)STACK_ENTRY_INTS; }


// ImportanceSamplePhong(Hammersley(samp, count), e) (raytracer.cpp:290-300).
float4 phong_tangent_dir(uint32_t samp, uint32_t count, float e) {
    float xi_x = (float)samp / (float)count;
    float xi_y = radical_inverse_vdc(samp);
    float phi = 2.0f * kPi32 * xi_x;
    float cp = cosf(phi);
    float sp = sinf(phi);
    float ct = powf(1.0f - xi_y, 1.0f / (e + 1.0f));
    float st = sqrtf(1.0f - (ct * ct));
    return make_float4(cp * st, sp * st, ct, 0.0f);
}

// Worst-case RNG draws of one sample: 2 jitter draws + the bounce tree (raytracer.cpp:416-417, 520).
uint64_t max_rng_draws(uint32_t depth, uint32_t refl, uint32_t spec) {
    // node(i): draws inside a surviving invocation with iters = i, child(i) = 1 roulette draw + node(i)
    uint64_t node = 0;                                // iters = 0: no children
    for (uint32_t i = 1; i <= depth; ++i) {
        uint64_t child = 1 + node;
        node = (uint64_t)refl * (1 + child) + (uint64_t)spec * child;
        if (node > (1ull << 40)) break;
    }
    return 2 + node;
}

// material_ns: the scene's specular exponents (SceneDesc::material_ns; the upload builds the table before it commits them).
int build_spec_table(prt_ctx * ctx, const std::vector<float> & material_ns, unsigned int spec_samples) {
    unsigned int n = std::max(1u, spec_samples);
    std::vector<float4> table(material_ns.size() * (size_t)n);
    for (size_t m = 0; m < material_ns.size(); ++m)
        for (unsigned int s = 0; s < n; ++s) table[m * n + s] = phong_tangent_dir(s, n, material_ns[m]);
    HIP_TRY(ctx, ctx->spec_dirs.upload(table));
    ctx->spec_table_samples = n;
    ctx->scene.spec_dirs = ctx->spec_dirs.p;
    ctx->scene.spec_samples = n;
    return 0;
}

// ---- the persistent traversal grid, written once: k_trace (wavefront pipeline), k_query, k_closest ----------------------------

// Blocks of `kernel` (`block` threads, `lds` bytes of dynamic LDS) resident on a compute unit, 8 at the most; `fallback` where the
// runtime cannot say.
template <typename Kernel>
int resident_blocks(Kernel kernel, int block, size_t lds, int fallback) {
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, block, lds) != hipSuccess || per_cu < 1) per_cu = fallback;
    return std::min(per_cu, 8);
}

// Blocks per compute unit, the lane-refill thresholds and the smallest chunk of a persistent grid, after the options' clamps
// (tuning knobs for experiments, not part of the ABI).  k_pool takes its keep_min and node_min from here too.
struct TraceRule {
    int per_cu, keep_min, node_min;
    unsigned int chunk_min;
};

TraceRule trace_rule(const PrtOptions & opt, int resident) {
    TraceRule r = { resident, 40, 32, 128u };
    if (opt.trace_blocks_per_cu >= 0) r.per_cu = std::max(1, std::min(resident, (int)opt.trace_blocks_per_cu));
    if (opt.keep_min >= 0) r.keep_min = std::max(1, std::min(64, (int)opt.keep_min));
    if (opt.node_min >= 0) r.node_min = std::max(0, std::min(64, (int)opt.node_min));
    if (opt.chunk_min >= 0) r.chunk_min = (unsigned int)std::max(64ll, std::min(512ll, opt.chunk_min));
    return r;
}

// The rule of a kernel with 256-thread blocks: as many blocks as are resident.
template <typename Kernel>
TraceRule trace_rule(const prt_ctx * ctx, Kernel kernel, size_t lds) {
    return trace_rule(ctx->opt, resident_blocks(kernel, 256, lds, 2));
}

struct TraceGrid { unsigned int grid, chunk; };

// The grid for n_rays under `per_cu` blocks of 256 per compute unit, and the rays reserved per head atomic: ~1/8 of a wave's
// fair share, whole waves, chunk_min..512.
TraceGrid trace_grid(const prt_ctx * ctx, int per_cu, unsigned int chunk_min, unsigned int n_rays) {
    constexpr unsigned int BLOCK = 256;
    TraceGrid g;
    g.grid = std::max(1u, std::min((unsigned int)per_cu * (unsigned int)ctx->cu_count, (n_rays + BLOCK - 1) / BLOCK));
    g.chunk = n_rays / (g.grid * (BLOCK / 64) * 8u);
    g.chunk = std::max(chunk_min, std::min(512u, (g.chunk / 64u) * 64u));
    return g;
}

// The LDS stack column's entries per lane (dev_trace.h LdsStack); option STACK_CAP is a test hook that forces the spill area into use.
unsigned int lds_stack_entries(const prt_ctx * ctx) {
    unsigned int stack_cap = STACK_LDS_CAP_DEFAULT;
    if (ctx->opt.stack_cap >= 0) stack_cap = (unsigned int)std::max(2ll, std::min(40ll, ctx->opt.stack_cap));
    return std::min(ctx->desc.stack_bound, stack_cap);
}

struct PixelSet {
    uint32_t n_pixels;
    uint32_t first_pixel;                      // contiguous range when nranks <= 1
    uint32_t block_rows, rank, nranks;         // interleaved row blocks otherwise
    const unsigned int * d_pixel_list;         // explicit list (device pointer) or NULL
};

// prt_render_rays: the caller's rays take the camera's place as the source of the primary rays (kernels_rays.h).
struct RaySource {
    RaysArgs A;                                // the arrays on the device; the call's k_rays_check has passed them
    float origin_abs_max;                      // ... and reduced the largest |origin component|
};

// The wavefront pipeline (kernels_wave.h): raygen, then rounds of {persistent trace, shade} until no ray is
// left.  Queue sizes come back to the host once per round (8 bytes, pinned): they size the next launches, end
// the loop and sum to ray_count (every queued ray is one TraceRay call, raytracer.cpp:161).
//
// Large frames are split into two CHAINS (sample halves) that run their rounds on two streams, the second chain
// starting when the first has finished its first trace: from then on one chain's k_shade (latency / HBM bound)
// tends to run beside the other chain's k_trace (vector-issue bound).  The persistent trace grid is capped so
// that a shade workgroup still fits on every CU; k_shade uses 256-thread workgroups in this mode for the same
// reason.  One host thread drives both chains, waiting on whichever round finishes next.
struct Chain {
    WaveBuffers B;
    DevParams P;
    prt_ctx::ChainWs * ws;
    unsigned int n_closest = 0, n_shadow = 0, round = 0, launches = 0;
    int cur = 0;
    bool active = false;
    unsigned long long rays = 0;
    float trace_ms = 0.0f;
};

int chain_setup(prt_ctx * ctx, Chain & c, int index, const DevParams & P, bool ring, unsigned int base, unsigned int n_samples) {
    prt_ctx::ChainWs & w = ctx->chain[index];
    c.ws = &w;
    c.P = P;
    const size_t N = n_samples;
    const unsigned int levels = std::max(1u, P.bounce_depth);
    const unsigned int fr4 = ctx->desc.textured ? 7u : ring ? 5u : 4u;
    const unsigned int n_lights = std::max(1u, ctx->scene.light_count);
    // float4 slab: frames + 2x3 closest queues + hits + 3 shadow arrays (accum aliases the shared sample_rgb)
    const size_t f4_total = (size_t)levels * fr4 * N + 6 * N + N + 3 * N * n_lights;
    HIP_TRY(ctx, w.f4.ensure(f4_total));
    HIP_TRY(ctx, w.rng.ensure(ring ? 2 * N : N));
    HIP_TRY(ctx, w.counts.ensure(16));
    HIP_TRY(ctx, w.overflow.ensure(N * (1 + (size_t)n_lights)));
    {
        // k_trace_exact's fixed grid: full-height stack columns for the rays k_trace hands over (near ties, overflowed columns)
        const size_t exact_lanes = 64 * 256;
        HIP_TRY(ctx, w.slow_stack.ensure(stack_dwords(std::max(ctx->desc.stack_bound, 4u), exact_lanes)));
        c.P.exact_stack = w.slow_stack.p;
        c.P.exact_stack_stride = (unsigned int)exact_lanes;
    }
    WaveBuffers & B = c.B;
    memset(&B, 0, sizeof(B));
    B.n_samples = n_samples;
    B.sample_base = base;
    B.accum = reinterpret_cast<Accum *>(ctx->sample_rgb.p) + base;
    B.rng = w.rng.p;
    B.rng_aux = ring ? w.rng.p + N : nullptr;
    B.ring = ring ? ctx->ring_ws.p + (size_t)16 * base : nullptr;   // this chain's own [16][n_samples] block of the shared ring workspace
    B.ring_step = 1;
    B.ring_stride = n_samples;
    float4 * f = w.f4.p;
    B.frames = f; f += (size_t)levels * fr4 * N;
    for (int q = 0; q < 2; ++q) { B.rq_o[q] = f; f += N; B.rq_d[q] = f; f += N; B.rq_t[q] = f; f += N; }
    B.hits = f; f += N;
    B.sq_o = f; f += N * n_lights;
    B.sq_d = f; f += N * n_lights;
    B.sq_c = f; f += N * n_lights;
    B.counts = w.counts.p;
    B.overflow = w.overflow.p;
    c.n_closest = n_samples;
    c.n_shadow = 0;
    c.active = n_samples > 0;
    return 0;
}

struct WaveTuning {
    TraceRule rule;                            // per_cu: what a chain's k_trace may take (render_wavefront)
    int multi_light, shade_block;
    bool ring, count_visits;
    size_t lds;
};

// Enqueue one round of a chain: counters reset, trace, overflow re-trace, shade, counts -> pinned host memory.
int chain_issue_round(prt_ctx * ctx, Chain & c, const WaveTuning & t) {
    constexpr int BLOCK = 256;
    hipStream_t stream = c.ws->stream;
    const WaveBuffers & B = c.B;
    c.rays += (unsigned long long)c.n_closest + c.n_shadow;
    HIP_TRY(ctx, hipMemsetAsync(B.counts, 0, 32, stream));
    const unsigned int total = c.n_closest + c.n_shadow;
    const TraceGrid g = trace_grid(ctx, t.rule.per_cu, t.rule.chunk_min, total);
    HIP_TRY(ctx, hipEventRecord(c.ws->ev_t0, stream));
    if (t.count_visits)
        hipLaunchKernelGGL((k_trace<BLOCK, true>), dim3(g.grid), dim3(BLOCK), t.lds, stream, ctx->scene, c.P, B, c.cur, c.n_closest, c.n_shadow,
                           t.rule.keep_min, t.rule.node_min, g.chunk, t.multi_light, ctx->counters.p);
    else
        hipLaunchKernelGGL((k_trace<BLOCK, false>), dim3(g.grid), dim3(BLOCK), t.lds, stream, ctx->scene, c.P, B, c.cur, c.n_closest, c.n_shadow,
                           t.rule.keep_min, t.rule.node_min, g.chunk, t.multi_light, ctx->counters.p);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(c.ws->ev_t1, stream));
    if (c.round == 0) HIP_TRY(ctx, hipEventRecord(c.ws->ev_first, stream));
    c.launches++;
    {
        // rays with a near-tied hit; the kernel reads the list length on the device and normally finds it zero
        constexpr unsigned int OVF_BLOCKS = 64;
        if (t.count_visits)
            hipLaunchKernelGGL(k_trace_exact<true>, dim3(OVF_BLOCKS), dim3(256), 0, stream, ctx->scene, c.P, B, c.cur, c.n_closest, t.multi_light, ctx->counters.p);
        else
            hipLaunchKernelGGL(k_trace_exact<false>, dim3(OVF_BLOCKS), dim3(256), 0, stream, ctx->scene, c.P, B, c.cur, c.n_closest, t.multi_light, ctx->counters.p);
        HIP_TRY(ctx, hipGetLastError());
    }
    if (c.n_closest) {
        if (t.shade_block == 1024) {
            const unsigned int sgrid = (c.n_closest + 1023) / 1024;
            if (ctx->desc.textured) hipLaunchKernelGGL((k_shade<true, 1024, true>), dim3(sgrid), dim3(1024), 0, stream, ctx->scene, c.P, B, c.cur, c.n_closest, ctx->counters.p);
            else if (t.ring) hipLaunchKernelGGL((k_shade<true, 1024, false>), dim3(sgrid), dim3(1024), 0, stream, ctx->scene, c.P, B, c.cur, c.n_closest, ctx->counters.p);
            else hipLaunchKernelGGL((k_shade<false, 1024, false>), dim3(sgrid), dim3(1024), 0, stream, ctx->scene, c.P, B, c.cur, c.n_closest, ctx->counters.p);
        } else {
            const unsigned int sgrid = (c.n_closest + 255) / 256;
            if (ctx->desc.textured) hipLaunchKernelGGL((k_shade<true, 256, true>), dim3(sgrid), dim3(256), 0, stream, ctx->scene, c.P, B, c.cur, c.n_closest, ctx->counters.p);
            else if (t.ring) hipLaunchKernelGGL((k_shade<true, 256, false>), dim3(sgrid), dim3(256), 0, stream, ctx->scene, c.P, B, c.cur, c.n_closest, ctx->counters.p);
            else hipLaunchKernelGGL((k_shade<false, 256, false>), dim3(sgrid), dim3(256), 0, stream, ctx->scene, c.P, B, c.cur, c.n_closest, ctx->counters.p);
        }
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipMemcpyAsync(c.ws->host_counts, B.counts, 32, hipMemcpyDeviceToHost, stream));
    HIP_TRY(ctx, hipEventRecord(c.ws->ev_done, stream));
    return 0;
}

// Wait for the chain's round in flight; returns with its next queue sizes loaded.
int chain_finish_round(prt_ctx * ctx, Chain & c) {
    HIP_TRY(ctx, hipEventSynchronize(c.ws->ev_done));
    float ms = 0.0f;
    HIP_TRY(ctx, hipEventElapsedTime(&ms, c.ws->ev_t0, c.ws->ev_t1));
    c.trace_ms += ms;
    if (ctx->opt.debug_rounds) fprintf(stderr, "[prt] round %u: %u closest + %u shadow rays, k_trace %.3f ms\n", c.round, c.n_closest, c.n_shadow, ms);
    const unsigned int n_lights = std::max(1u, ctx->scene.light_count);
    const unsigned int next_closest = c.n_closest ? c.ws->host_counts[0] : 0;
    const unsigned int next_shadow = c.n_closest ? c.ws->host_counts[1] : 0;
    if (c.n_closest) c.rays += c.ws->host_counts[4];          // shadow rays of this round's hits that were counted, not traced
    if (next_closest > c.B.n_samples || next_shadow > c.B.n_samples * n_lights) { ctx->error = "prt_render: wavefront queue overflow"; return -6; }
    c.n_closest = next_closest;
    c.n_shadow = next_shadow;
    c.cur ^= 1;
    c.round++;
    if (c.round > 100000) { ctx->error = "prt_render: wavefront loop did not terminate"; return -5; }
    c.active = c.n_closest + c.n_shadow > 0;
    return 0;
}

// rays: the primary rays come from the caller's arrays, not from cam; the pass's first sample is ray `ray_base` of them.
int render_wavefront(prt_ctx * ctx, const DevCamera & cam, const RaySource * rays, unsigned long long ray_base, const DevParams & P, bool ring,
                     bool count_visits, unsigned int n_samples, size_t lds, unsigned long long * ray_count, float * trace_ms, unsigned int * launches) {
    constexpr int BLOCK = 256;
    WaveTuning t;
    t.lds = lds;
    t.ring = ring;
    t.count_visits = count_visits;
    t.rule = count_visits ? trace_rule(ctx, k_trace<BLOCK, true>, lds) : trace_rule(ctx, k_trace<BLOCK, false>, lds);
    const PrtOptions & opt = ctx->opt;
    int n_chains = n_samples >= (1u << 23) ? 2 : 1;          // measured +2 % on 16.6 M samples; small frames: not worth the extra launches
    const int split_per_cu = opt.trace_blocks_per_cu >= 0 ? t.rule.per_cu : 4;
    if (opt.chains >= 0) n_chains = std::max(1, std::min((int)PRT_MAX_CHAINS, (int)opt.chains));
    // chains start on a pixel and a wave boundary
    const unsigned int unit = P.spp * 64u;
    while (n_chains > 1 && (unsigned long long)unit * n_chains > n_samples) n_chains--;
    if (n_chains >= 2) t.rule.per_cu = std::min(t.rule.per_cu, split_per_cu);
    t.shade_block = n_chains >= 2 ? 256 : 1024;
    if (opt.shade_block >= 0) t.shade_block = opt.shade_block == 256 ? 256 : 1024;
    t.multi_light = ctx->scene.light_count > 1 ? 1 : 0;

    Chain chain[PRT_MAX_CHAINS];
    int rc = 0;
    {
        unsigned int base = 0;
        const unsigned int per = (unsigned int)((((unsigned long long)n_samples + n_chains - 1) / n_chains + unit - 1) / unit * unit);
        for (int c = 0; c < n_chains; ++c) {
            const unsigned int n = c + 1 == n_chains ? n_samples - base : std::min(per, n_samples - base);
            if ((rc = chain_setup(ctx, chain[c], c, P, ring, base, n))) return rc;
            base += n;
        }
    }

    for (int c = 0; c < n_chains; ++c) {
        hipStream_t st = chain[c].ws->stream;
        if (c >= 1) {
            // the extra streams start after everything already queued on the main stream (scene upload, memsets)
            HIP_TRY(ctx, hipEventRecord(ctx->chain[c].ev_done, ctx->stream));
            HIP_TRY(ctx, hipStreamWaitEvent(st, ctx->chain[c].ev_done, 0));
        }
        const unsigned int gen_grid = (chain[c].B.n_samples + 255) / 256;
        if (gen_grid) {
            const unsigned long long chain_base = ray_base + chain[c].B.sample_base;      // in the caller's arrays
            if (rays && ring) hipLaunchKernelGGL(k_raygen_rays<true>, dim3(gen_grid), dim3(256), 0, st, rays->A, chain[c].P, chain[c].B, chain_base);
            else if (rays) hipLaunchKernelGGL(k_raygen_rays<false>, dim3(gen_grid), dim3(256), 0, st, rays->A, chain[c].P, chain[c].B, chain_base);
            else if (ring) hipLaunchKernelGGL(k_raygen<true>, dim3(gen_grid), dim3(256), 0, st, cam, chain[c].P, chain[c].B);
            else hipLaunchKernelGGL(k_raygen<false>, dim3(gen_grid), dim3(256), 0, st, cam, chain[c].P, chain[c].B);
            HIP_TRY(ctx, hipGetLastError());
        }
    }
    // first rounds: chain c starts tracing when chain c-1's first trace is done (staggered phases from then on)
    for (int c = 0; c < n_chains; ++c) {
        if (!chain[c].active) continue;
        if (c >= 1 && chain[c - 1].launches) HIP_TRY(ctx, hipStreamWaitEvent(chain[c].ws->stream, chain[c - 1].ws->ev_first, 0));
        if ((rc = chain_issue_round(ctx, chain[c], t))) return rc;
    }
    for (;;) {
        bool any = false;
        for (int c = 0; c < n_chains; ++c) {
            if (!chain[c].active) continue;
            any = true;
            if ((rc = chain_finish_round(ctx, chain[c]))) return rc;
            if (chain[c].active && (rc = chain_issue_round(ctx, chain[c], t))) return rc;
        }
        if (!any) break;
    }
    for (int c = 1; c < n_chains; ++c) {
        // the resolve runs on the main stream: it has to see every chain's results
        HIP_TRY(ctx, hipEventRecord(ctx->chain[c].ev_done, chain[c].ws->stream));
        HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->chain[c].ev_done, 0));
    }
    *ray_count = 0;
    *trace_ms = 0.0f;
    *launches = 0;
    for (int c = 0; c < n_chains; ++c) { *ray_count += chain[c].rays; *trace_ms += chain[c].trace_ms; *launches += chain[c].launches; }
    return 0;
}

// The wave-pool pipeline (kernels_pool.h): one launch; per-sample arrays as in the wavefront pipeline (chain 0's
// workspace, without the global queues), plus cap (+ cap * lights shadow) ray slots per resident wave.
// RINGMEM = 0: no sample can make more than 15 RNG draws (and the scene is opaque, untextured, fixed spp): the
// general-RNG variant runs without its draw ring in memory (dev_rng.h).
template <int BLOCK, int WAVES, bool LDSTAB, bool RING, bool COUNT, bool TEX, bool ADAPT, int RINGMEM, bool EXACT, bool SHARED = false>
int launch_pool_kernel(prt_ctx * ctx, unsigned int grid, size_t lds, const PoolArgs * d_args) {
    hipLaunchKernelGGL((k_pool<BLOCK, WAVES, LDSTAB, RING, COUNT, TEX, ADAPT, RINGMEM, EXACT, SHARED>), dim3(grid), dim3(BLOCK), lds, ctx->stream, d_args, ctx->counters.p);
    HIP_TRY(ctx, hipGetLastError());       // a template variant that cannot launch (LDS, registers) is reported here, by name of its cause
    return 0;
}

template <int BLOCK, int WAVES, bool LDSTAB, bool RING, bool TEX, bool ADAPT, int RINGMEM = 1>
int launch_pool(prt_ctx * ctx, bool count, const DevCamera & cam, DevParams P, unsigned int n_samples, unsigned int stack_entries) {
    // the stack columns double as the shading phase's frame storage (WFRAME_LDS_DWORDS per lane)
    const size_t lds = std::max(stack_dwords(stack_entries, BLOCK), (size_t)((RING && RINGMEM == 1) ? WFRAME_LDS_DWORDS : WFRAME_LDS_DWORDS_NOPOS) * BLOCK) * sizeof(int);
    const PrtOptions & opt = ctx->opt;
    // Three launches (kernels_pool.h PoolBuffers::park): the fast kernel, which parks the rays it cannot finish - a hit with
    // company within a few ulp, a stack column that overflowed -; k_pool_parked_shadows for the parked shadow rays; the EXACT
    // kernel, adopting the parked closest-hit rays.  Normally nothing is parked and the two follow-ups leave at once.
    // Option POOL_EXACT (tests): the EXACT kernel does the whole render.
    const bool exact_only = opt.pool_exact != 0;
    int per_cu = 0;
    // Block-shared pools (kernels_pool.h, round 4): the workgroup owns a pool, not the wave.  Option POOL_SHARED: 1 / 0 force it
    // on / off; the EXACT kernels (the adopting launch, POOL_EXACT) always keep wave-private pools.
    // Default (profiles/r04_ab_shared_pools.txt, same-process A/B): ON for the kernel of the default bounce tree (fixed spp, at
    // most 15 draws per sample, opaque untextured scene: RINGMEM = 0) - the full C4 frame 1.5 - 2 % faster, its 1/2 .. 1/16
    // shards 1.5 - 3.5 % -; OFF for the adaptive mode, whose short rounds lose 11 % to the four waves waiting for each other at
    // every phase boundary, and for deep bounce trees (C5: 886 -> 949 ms; that variant spills 59 dwords shared, 31 private).
    const bool shared = !exact_only && (opt.pool_shared >= 0 ? opt.pool_shared != 0 : (PRT_POOL_SHARED_DEFAULT != 0 && !ADAPT && !TEX && RINGMEM == 0));
    void (* const sized_as)(const PoolArgs *, DevCounters *) =
        exact_only ? k_pool<BLOCK, WAVES, LDSTAB, RING, false, TEX, ADAPT, RINGMEM, true, false>
        : shared   ? k_pool<BLOCK, WAVES, LDSTAB, RING, false, TEX, ADAPT, RINGMEM, false, true>
        : count    ? k_pool<BLOCK, WAVES, LDSTAB, RING, true, TEX, ADAPT, RINGMEM, false, false>
                   : k_pool<BLOCK, WAVES, LDSTAB, RING, false, TEX, ADAPT, RINGMEM, false, false>;
    per_cu = resident_blocks(sized_as, BLOCK, lds, 1);
    if (opt.pool_blocks_per_cu >= 0) per_cu = std::max(1, std::min(per_cu, (int)opt.pool_blocks_per_cu));
    if (opt.debug_util) fprintf(stderr, "[prt] k_pool<%d,%d,%d>: %d blocks per CU\n", BLOCK, WAVES, (int)LDSTAB, per_cu);
    const unsigned int max_blocks = (unsigned int)per_cu * (unsigned int)ctx->cu_count;
    const unsigned int grid = std::max(1u, std::min(max_blocks, (n_samples + BLOCK - 1) / BLOCK));
    const unsigned int waves = grid * (BLOCK / 64);
    // slots per wave: half of a wave's fair share of the samples (measured on C4 shards: larger pools leave the
    // waves unbalanced when the sample counter runs out, smaller ones trace at low lane utilisation); whole
    // waves, 64..512
    unsigned int cap = (n_samples / waves / 2u + 63u) / 64u * 64u;
    cap = std::max(64u, std::min(512u, cap));
    if (shared && opt.pool_shared_cap >= 0) cap = (unsigned int)std::max(64ll, std::min(1024ll, opt.pool_shared_cap / 64 * 64));
    // adaptive mode: a pixel stays in its pool for all its samples (up to 50 x several rounds), so what a wave takes it keeps;
    // smaller pools leave more of the frame on the counter for the waves whose pixels end early (C4: 512 slots 195 ms,
    // 256 168 ms, 64 - 192 161 - 164 ms, profiles/r02_adaptive_pool_capacity.txt; round 3, once the variance rule no longer
    // walks the stored samples: 512 160, 256 145, 192 133 - 138, 128 129 - 133, 64 138 ms, profiles/r03_adaptive.txt)
    if (ADAPT) cap = std::min(cap, 128u);
    if (opt.pool_cap >= 0) cap = (unsigned int)std::max(64ll, std::min(4096ll, opt.pool_cap / 64 * 64));
    // experiment POOL_FAIR = k: every wave's pool holds k / 8 of a fair share and takes at most that at once (8 = the whole
    // frame resident from the start, no second generation of samples; profiles/r04_ab_shared_pools.txt section 6)
    unsigned int topup_max = 0xFFFFFFFFu;
    if (opt.pool_fair > 0) {
        const unsigned int fair = (unsigned int)(((unsigned long long)n_samples * (unsigned long long)opt.pool_fair / 8ull + waves - 1u) / waves);
        cap = std::max(64u, std::min(4096u, (fair + 63u) / 64u * 64u));
        topup_max = std::max(1u, fair);
    }
    // block-shared: the same slots, owned by the block's waves together (`cap` is per UNIT from here on)
    const unsigned int units = shared ? grid : waves;
    if (shared) cap *= (unsigned int)(BLOCK / 64);
    const unsigned int n_lights = std::max(1u, ctx->scene.light_count);
    // Leaf rays beside the walk (kernels_pool.h FORKS; options POOL_FORK, POOL_FORK_ROOM): the kernels of opaque untextured
    // fixed-spp renders.  Their lists get room / 8 of the capacity on top of it - `cap` stays the bound on entries with a walk in
    // progress - and a shade pass forks only when the next list holds its worst case.  No room, or a bounce tree whose bounds
    // would not fit the fields of the block's reservation word (PCTL_FORK_RES): lcap = cap, and nothing forks.
    constexpr bool FORKS = !ADAPT && !TEX && RINGMEM == 0;
    unsigned int lcap = cap;
    if (FORKS && (opt.pool_fork >= 0 ? opt.pool_fork != 0 : PRT_POOL_FORK_DEFAULT != 0)) {
        const unsigned long long eighths = (unsigned long long)std::max(0ll, std::min(64ll, opt.pool_fork_room >= 0 ? opt.pool_fork_room : 8ll));
        const unsigned int per = shared ? (unsigned int)(BLOCK / 64) : 1u;          // the adopting launch divides a shared pool's lists by this
        const unsigned long long l = cap + (unsigned long long)cap * eighths / 8ull / per * per;
        const unsigned long long widest = 1ull + P.reflection_samples + P.spec_samples;
        if (l <= (1ull << 17) && l * widest < (1ull << 20)) lcap = (unsigned int)l;
    }
    const unsigned int scap = lcap * n_lights;

    prt_ctx::ChainWs & w = ctx->chain[0];
    const size_t N = n_samples;
    const unsigned int levels = std::max(1u, P.bounce_depth);
    const unsigned int fr4 = TEX ? 7u : (RING && RINGMEM == 1) ? 5u : 4u;       // kernels_wave.h wframe_save
    HIP_TRY(ctx, w.f4.ensure((size_t)levels * fr4 * N));
    HIP_TRY(ctx, w.rng.ensure(RING ? 2 * N : N));
    HIP_TRY(ctx, ctx->pool_f4.ensure((size_t)units * (7u * (size_t)lcap + 3u * (size_t)scap)));
    // [0] sample counter, [1] parked closest-hit / finalise entries, [2] parked shadow rays, [3] the adopting launch's counter
    HIP_TRY(ctx, ctx->wf_counts.ensure(16));          // zeroed by k_pool_store_args below
    // Park lists: sized for what scenes with coincident geometry need in practice, never for the worst case (every sample's
    // ray parked: 48 bytes x samples x (1 + lights)).  The kernels count what they could not store; render_pixels looks at
    // the counts after the frame and, if a list was too short, enlarges it and renders the frame again.
    // The clamps are the true worst cases: a sample is parked at most once (it leaves the pool) plus, in adaptive mode, one
    // deferred finalise step per pixel; parked SHADOW rays pile up until the fast kernel has ended, and every shaded hit of a
    // sample's bounce tree - up to sum over levels of (reflection + specular samples)^level of them - emits one per light.
    size_t hits_per_sample = 1, level_nodes = 1;
    for (unsigned int l = 0; l < P.bounce_depth && hits_per_sample < (1u << 20); ++l) {
        level_nodes *= std::max<size_t>(1, (size_t)P.reflection_samples + P.spec_samples);
        hits_per_sample += level_nodes;
    }
    const size_t worst_spark = N * n_lights * std::min<size_t>(hits_per_sample, 1u << 20);
    // (forking kernels: besides its one ray with a walk in progress a sample can have every leaf of its bounce tree parked)
    const size_t park_worst = N + (ADAPT ? N : 0) + (lcap > cap ? N * std::min<size_t>(level_nodes, 1u << 20) : 0);
    const size_t park_cap = std::min<size_t>(ctx->pool_park_cap, park_worst), spark_cap = std::min<size_t>(ctx->pool_spark_cap, worst_spark);
    HIP_TRY(ctx, ctx->pool_park.ensure(3 * (park_cap + spark_cap)));
    // the EXACT launch's lanes continue their LDS stack columns in memory; k_pool_parked_shadows has full-height columns
    const unsigned int grid2 = exact_only ? grid : std::max(1u, std::min(grid, (unsigned int)ctx->cu_count));
    const size_t exact_lanes = (size_t)POOL_PARKED_SHADOW_BLOCKS * 256, spill_lanes = (size_t)grid2 * BLOCK;
    const size_t spill_entries = ctx->desc.stack_bound > stack_entries ? ctx->desc.stack_bound - stack_entries : 0;
    const size_t exact_ints = stack_dwords(std::max(ctx->desc.stack_bound, 4u), exact_lanes);
    HIP_TRY(ctx, ctx->stack_spill.ensure(exact_ints + stack_dwords(spill_entries, spill_lanes)));
    P.exact_stack = ctx->stack_spill.p;
    P.exact_stack_stride = (unsigned int)exact_lanes;
    P.stack_spill = spill_entries ? ctx->stack_spill.p + exact_ints : nullptr;
    P.stack_spill_stride = (unsigned int)spill_lanes;

    WaveBuffers B;
    memset(&B, 0, sizeof(B));
    B.n_samples = n_samples;
    B.sample_base = 0;
    B.accum = reinterpret_cast<Accum *>(ctx->sample_rgb.p);
    B.rng = w.rng.p;
    B.rng_aux = RING ? w.rng.p + N : nullptr;
    B.ring = RING && RINGMEM != 0 ? ctx->ring_ws.p : nullptr;
    B.ring_step = ADAPT ? 16u : 1u;                              // WaveBuffers::ring: pixel-major in adaptive mode
    B.ring_stride = ADAPT ? 1u : (unsigned int)n_samples;
    B.frames = w.f4.p;
    PoolBuffers Q;
    memset(&Q, 0, sizeof(Q));
    Q.cq = ctx->pool_f4.p;
    Q.hits = Q.cq + (size_t)units * 6u * lcap;
    Q.sq = Q.hits + (size_t)units * lcap;
    Q.head = ctx->wf_counts.p;
    Q.cap = cap;
    Q.lcap = lcap;
    Q.scap = scap;
    Q.park = ctx->pool_park.p;
    Q.spark = ctx->pool_park.p + 3 * park_cap;
    Q.park_count = ctx->wf_counts.p + 1;
    Q.park_cap = (unsigned int)park_cap;
    Q.spark_cap = (unsigned int)spark_cap;
    Q.adopt = 0;
    Q.fin = nullptr; Q.scratch = nullptr; Q.jobsum = nullptr; Q.final_rgb = nullptr;
    Q.wave_times = nullptr;
    ctx->wave_times_n = 0;
    if (count && opt.debug_util && !exact_only) {
        HIP_TRY(ctx, ctx->wave_times.ensure(3u * (size_t)waves));
        Q.wave_times = ctx->wave_times.p;
        ctx->wave_times_n = waves;
    }
    if (ADAPT) {
        // n_samples counts PIXELS here: the unit in the pool is a pixel that runs its samples one after the other
        HIP_TRY(ctx, ctx->pool_fin.ensure((size_t)units * cap));
        HIP_TRY(ctx, ctx->adapt_f4.ensure(((size_t)P.max_spp + 2u) * N));
        Q.fin = ctx->pool_fin.p;
        Q.scratch = ctx->adapt_f4.p;
        Q.jobsum = Q.scratch + (size_t)P.max_spp * N;
        Q.final_rgb = Q.jobsum + N;
    }
    // guided top-ups: adaptive mode by default (a pixel is a chain of up to max_spp samples: the pixels started last are the frame's tail)
    Q.guided = (unsigned int)std::max(0ll, std::min(64ll, opt.pool_guided >= 0 ? opt.pool_guided : (ADAPT ? 16ll : 0ll)));
    Q.guided_min = (unsigned int)std::max(1ll, std::min(512ll, opt.pool_guided_min >= 0 ? opt.pool_guided_min : 8ll));
    Q.topup_max = topup_max == 0xFFFFFFFFu ? topup_max : topup_max * (shared ? (unsigned int)(BLOCK / 64) : 1u);
    Q.topup_min = ADAPT ? std::max(64u, cap / 2u) : std::max(64u, cap / 4u);
    if (opt.pool_topup >= 0) Q.topup_min = (unsigned int)std::max(1ll, std::min((long long)cap, opt.pool_topup * (shared ? BLOCK / 64 : 1)));   // the option counts per wave
    const TraceRule lanes = trace_rule(opt, per_cu);         // for its two lane thresholds; the pool's grid has options of its own
    const int multi_light = ctx->scene.light_count > 1 ? 1 : 0;
    PoolArgs A;
    memset(&A, 0, sizeof(A));
    A.sc = ctx->scene;
    A.cam = cam;
    A.P = P;
    A.B = B;
    A.Q = Q;
    A.keep_min = lanes.keep_min;
    A.node_min = lanes.node_min;
    A.node_frac = 4;
    if (opt.node_frac >= 0) A.node_frac = std::max(0, std::min(8, (int)opt.node_frac));
    A.multi_light = multi_light;
    HIP_TRY(ctx, ctx->pool_args.ensure(2));
    // the adopting launch's units are waves whatever the fast kernel's were: a quarter of a shared pool's slots each, in the
    // same buffers (grid2 <= grid, so its waves' lists fit where the blocks' lists lie)
    hipLaunchKernelGGL(k_pool_store_args, dim3(1), dim3(64), 0, ctx->stream, A, ctx->pool_args.p, ctx->wf_counts.p, 16u,
                       exact_only ? (unsigned int *)nullptr : ctx->wf_counts.p + 3, shared ? (unsigned int)(BLOCK / 64) : 1u);
    HIP_TRY(ctx, hipGetLastError());
    int rc;
    if (exact_only) {
        return count ? launch_pool_kernel<BLOCK, WAVES, LDSTAB, RING, true, TEX, ADAPT, RINGMEM, true>(ctx, grid, lds, ctx->pool_args.p)
                     : launch_pool_kernel<BLOCK, WAVES, LDSTAB, RING, false, TEX, ADAPT, RINGMEM, true>(ctx, grid, lds, ctx->pool_args.p);
    }
    if (shared)
        rc = count ? launch_pool_kernel<BLOCK, WAVES, LDSTAB, RING, true, TEX, ADAPT, RINGMEM, false, true>(ctx, grid, lds, ctx->pool_args.p)
                   : launch_pool_kernel<BLOCK, WAVES, LDSTAB, RING, false, TEX, ADAPT, RINGMEM, false, true>(ctx, grid, lds, ctx->pool_args.p);
    else
        rc = count ? launch_pool_kernel<BLOCK, WAVES, LDSTAB, RING, true, TEX, ADAPT, RINGMEM, false>(ctx, grid, lds, ctx->pool_args.p)
                   : launch_pool_kernel<BLOCK, WAVES, LDSTAB, RING, false, TEX, ADAPT, RINGMEM, false>(ctx, grid, lds, ctx->pool_args.p);
    if (rc) return rc;
    if (count) hipLaunchKernelGGL(k_pool_parked_shadows<true>, dim3(POOL_PARKED_SHADOW_BLOCKS), dim3(256), 0, ctx->stream, ctx->pool_args.p, ctx->counters.p);
    else hipLaunchKernelGGL(k_pool_parked_shadows<false>, dim3(POOL_PARKED_SHADOW_BLOCKS), dim3(256), 0, ctx->stream, ctx->pool_args.p, ctx->counters.p);
    HIP_TRY(ctx, hipGetLastError());
    // the adopting launch: one block per compute unit; they find the park list empty and leave at once - except in scenes
    // with coincident geometry, where they finish what the first launch set aside
    return count ? launch_pool_kernel<BLOCK, WAVES, LDSTAB, RING, true, TEX, ADAPT, RINGMEM, true>(ctx, grid2, lds, ctx->pool_args.p + 1)
                 : launch_pool_kernel<BLOCK, WAVES, LDSTAB, RING, false, TEX, ADAPT, RINGMEM, true>(ctx, grid2, lds, ctx->pool_args.p + 1);
}

// The fixed-spp resolve: the samples are the wavefront / pool pipelines' fixed-point accumulators (dev_scene.h Accum)
void launch_resolve(hipStream_t stream, const void * samples, float4 * out, unsigned int n_px, unsigned int spp, ResolveMap map) {
    const unsigned int grid2 = (unsigned int)(((unsigned long long)n_px * spp + 255ull) / 256ull);
    switch (spp) {
        case 2: hipLaunchKernelGGL((k_resolve_pow2<2, true>), dim3(grid2), dim3(256), 0, stream, samples, out, n_px, map); break;
        case 4: hipLaunchKernelGGL((k_resolve_pow2<4, true>), dim3(grid2), dim3(256), 0, stream, samples, out, n_px, map); break;
        case 8: hipLaunchKernelGGL((k_resolve_pow2<8, true>), dim3(grid2), dim3(256), 0, stream, samples, out, n_px, map); break;
        case 16: hipLaunchKernelGGL((k_resolve_pow2<16, true>), dim3(grid2), dim3(256), 0, stream, samples, out, n_px, map); break;
        case 32: hipLaunchKernelGGL((k_resolve_pow2<32, true>), dim3(grid2), dim3(256), 0, stream, samples, out, n_px, map); break;
        case 64: hipLaunchKernelGGL((k_resolve_pow2<64, true>), dim3(grid2), dim3(256), 0, stream, samples, out, n_px, map); break;
        default: hipLaunchKernelGGL(k_resolve<true>, dim3((n_px + 255) / 256), dim3(256), 0, stream, samples, out, n_px, spp, map);
    }
}

// GPU radix-tree build + host collapse / quantise.  verts: 9 floats per triangle.
int build_bvh_lbvh(prt_ctx * ctx, const float * verts, uint32_t n_tris, uint32_t leaf_max, BvhWide * bvh) {
    float lo[3], hi[3];
    lbvh_scene_bounds(verts, n_tris, lo, hi);
    LbvhTree tree;
    double device_ms = 0.0;
    HIP_TRY(ctx, build_lbvh_tree(verts, n_tris, lo, hi, ctx->stream, &tree, &device_ms));
    build_bvh_wide_from_radix_tree(BVH_WIDTH, n_tris, leaf_max, tree.left.data(), tree.right.data(), tree.first.data(), tree.last.data(),
                                   tree.node_box.data(), tree.leaf_box.data(), tree.sorted_ids.data(), bvh, &ctx->opt.bvh);
    if (ctx->opt.debug_util) fprintf(stderr, "[prt] LBVH: %u triangles, radix tree on the device in %.2f ms\n", n_tris, device_ms);
    return 0;
}

int render_pixels(prt_ctx * ctx, const prt_camera * cam_in, const prt_params * params, uint32_t width, uint32_t height,
                  const PixelSet & px, float4 * d_out, prt_counters * counters);

// Renders the pixel set into d_out (device, float4 per pixel, packed in local pixel order).  Synchronous.
// rays (prt_render_rays): output i of the set is the mean over the caller's rays i * spp .. of it, not a pixel of cam_in (null);
// wavefront pipeline, fixed spp, item order = ray order.
int render_pixels_once(prt_ctx * ctx, const prt_camera * cam_in, const prt_params * params, uint32_t width, uint32_t height,
                       const PixelSet & px, float4 * d_out, prt_counters * counters, bool * park_overflow, const RaySource * rays = nullptr) {
    *park_overflow = false;
    if (!ctx->has_scene) { ctx->error = "prt_render: no scene uploaded"; return -2; }
    if ((!cam_in && !rays) || !params || !width || !height) { ctx->error = "prt_render: null camera / params or empty image"; return -1; }
    if (params->spp == 0 || params->spp > 65535) { ctx->error = "prt_render: spp must be in 1..65535 (prt_key.h packs the sample in 16 bits)"; return -1; }
    if (params->bounce_depth > 16) { ctx->error = "prt_render: bounce_depth > 16 not supported"; return -1; }
    if ((uint64_t)width * height >= (1ull << 32)) { ctx->error = "prt_render: image has 2^32 pixels or more"; return -1; }
    if (px.n_pixels == 0) {                 // RenderTask with start_idx == end_idx (main.cpp:273): nothing to do, not an error
        if (counters) { memset(counters, 0, sizeof(*counters)); counters->pipeline = params->pipeline & PRT_PIPELINE_MASK; }
        return 0;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t stream = ctx->stream;

    if (std::max(1u, params->spec_samples) != ctx->spec_table_samples) {
        HIP_TRY(ctx, hipStreamSynchronize(stream));
        int rc = build_spec_table(ctx, ctx->desc.material_ns, params->spec_samples);
        if (rc) return rc;
        HIP_TRY(ctx, hipDeviceSynchronize());      // the table went through the null stream
    }

    DevCamera cam;
    memset(&cam, 0, sizeof(cam));
    if (!rays) {
        cam.position = ld3(cam_in->position);
        cam.forward = ld3(cam_in->forward);
        cam.right_scaled = ld3(cam_in->right) * cam_in->tan_a2 * cam_in->aspect;      // main.cpp:170
        cam.up_scaled = ld3(cam_in->up) * cam_in->tan_a2;                              // main.cpp:171
        cam.inv_width = cam_in->inv_width;
        cam.inv_height = cam_in->inv_height;
    }

    DevParams P;
    P.ray_bias = params->ray_bias;
    P.reflection_samples = params->reflection_samples;
    P.spec_samples = params->spec_samples;
    P.bounce_depth = params->bounce_depth;
    P.background = mk3(params->background_color[0], params->background_color[1], params->background_color[2]);
    P.spp = params->spp;
    P.seed = params->seed;
    const bool adaptive = params->max_spp > params->spp;            // RenderPixel's second loop (main.cpp:245-258)
    P.max_spp = adaptive ? params->max_spp : params->spp;
    P.variance_threshold = params->variance_threshold > 0.0f ? params->variance_threshold : 0.01f;    // main.cpp:254
    P.width = width;
    P.height = height;
    // (where the primary rays start: the camera position, or the largest |origin component| of the caller's rays)
    float extent = ctx->desc.scene_abs_max;
    if (rays) extent = std::max(extent, rays->origin_abs_max);
    else for (int a = 0; a < 3; ++a) extent = std::max(extent, fabsf(cam_in->position[a]));
    P.box_pad = extent * (1.0f / 65536.0f);
    P.first_pixel = px.first_pixel;
    P.shard_block_rows = std::max(1u, px.block_rows);
    P.shard_rank = px.rank;
    P.shard_nranks = std::max(1u, px.nranks);
    P.pixel_list = px.d_pixel_list;
    const PrtOptions & opt = ctx->opt;
    ctx->scene.tie_widen_max = (unsigned int)std::max(0ll, std::min(64ll, opt.tie_widen_max));
    {
        // which copy of the light table: the shadow-tree roots, or every root at 0 - the option, trees of an older geometry, or a
        // call whose shadow-ray origins the upload's exclusion bound does not cover (include/prt.h "Shadow trees")
        bool trees = opt.shadow_trees != 0 && ctx->desc.shadow_trees_fresh && fabsf(params->ray_bias) <= ctx->desc.shadow_bias_max;
        if (rays) trees = trees && rays->origin_abs_max <= ctx->desc.shadow_cam_max;
        else for (int a = 0; a < 3; ++a) trees = trees && fabsf(cam_in->position[a]) <= ctx->desc.shadow_cam_max;
        ctx->scene.lights = ctx->arrays.lights.p + (trees ? 0u : ctx->desc.light_stride);
    }
    P.elide_dead_shadow_rays = opt.trace_dead_shadow_rays ? 0u : 1u;
    {
        // the nodes' normal cones (dev_scene.h): for directions the library normalised itself - not the caller's, which
        // prt_render_rays' first rays and their alpha continuations carry - and for origins inside the bound the upload
        // computed them for, which is the trees' guard
        bool cones = !rays && fabsf(params->ray_bias) <= ctx->desc.shadow_bias_max;
        for (int a = 0; a < 3 && cones; ++a) cones = fabsf(cam_in->position[a]) <= ctx->desc.shadow_cam_max;
        P.no_cones = cones ? 0u : (unsigned int)TRACE_NO_CONE;
    }
    {
        // the open-triangle flags (include/prt.h "Open triangles"): their own option, never while every ray is to be traced, and
        // only for a call inside the bounds they were computed for - the bias, and the camera guard the trees use
        bool open = opt.shadow_open != 0 && !opt.trace_dead_shadow_rays && ctx->desc.shadow_trees_fresh && ctx->desc.shadow_open_reach > 0.0f &&
                    fabsf(params->ray_bias) <= ctx->desc.shadow_open_bias_max;
        if (rays) open = open && rays->origin_abs_max <= ctx->desc.shadow_cam_max;
        else for (int a = 0; a < 3; ++a) open = open && fabsf(cam_in->position[a]) <= ctx->desc.shadow_cam_max;
        P.open_reach = open ? ctx->desc.shadow_open_reach : 0.0f;
    }
    // tiled work order: sets made of full-width rows only (a whole frame or a range that starts at a row, row-block shards)
    P.tile_pixels = 0;
    if (!rays && !px.d_pixel_list && width % 8u == 0u && !opt.no_tiles) {
        const bool rows = px.nranks > 1 ? std::max(1u, px.block_rows) % 8u == 0u : px.first_pixel % width == 0u;
        if (rows) P.tile_pixels = px.n_pixels / (8u * width) * (8u * width);
    }

    P.work_reverse_n = (opt.work_reverse > 0 && !px.d_pixel_list && !rays) ? px.n_pixels : 0u;
    P.work_scatter_n = 0; P.work_scatter_mul = 1;
    if (opt.work_scatter > 0 && !px.d_pixel_list && P.tile_pixels >= 64u) {
        // a multiplier near n / golden ratio spreads consecutive chunks far apart; coprime to n, and (n - 1) * mul must fit 32 bits
        const unsigned int n = P.tile_pixels / 8u;
        unsigned long long mul = std::max<unsigned long long>(3ull, (unsigned long long)((double)n * 0.6180339887));
        mul = std::min<unsigned long long>(mul, 0xFFFFFFFFull / n);
        if (!(mul & 1ull)) mul -= 1ull;                       // odd, and never above the 32-bit limit
        auto gcd = [](unsigned long long a, unsigned long long b) { while (b) { const unsigned long long t = a % b; a = b; b = t; } return a; };
        while (mul > 1ull && gcd(mul, n) != 1ull) mul -= 2ull;
        if (mul > 1ull) { P.work_scatter_n = n; P.work_scatter_mul = (unsigned int)mul; }
    }
    const bool count_visits = (params->pipeline & PRT_FLAG_COUNT_VISITS) != 0;
    // the compact 2-register RNG only covers opaque scenes with <= 15 draws per sample; textured scenes always take the
    // general variant (an alpha map can make any hit translucent)
    const bool ring = adaptive || ctx->desc.any_translucent || ctx->desc.textured || max_rng_draws(P.bounce_depth, P.reflection_samples, P.spec_samples) > 15;

    unsigned int pipeline = params->pipeline & PRT_PIPELINE_MASK;
    if (adaptive) {
        // a pixel's samples form a chain on one RNG stream with a data-dependent length: only the pool pipeline, whose
        // work items carry their own state machine, runs it
        if (pipeline != PRT_PIPELINE_DEFAULT && pipeline != PRT_PIPELINE_POOL) { ctx->error = "prt_render: adaptive sampling (max_spp > spp) runs on PRT_PIPELINE_POOL (or DEFAULT) only"; return -1; }
        if (params->max_spp > 4096) { ctx->error = "prt_render: max_spp above 4096 is not supported"; return -1; }
        pipeline = PRT_PIPELINE_POOL;
    }
    if (pipeline == PRT_PIPELINE_DEFAULT) {
        // Measured on MI355X (tools/pool_cross.py, tools/pool_scene_cross.py): the wavefront pipeline's steady state is
        // ~12 % faster (its k_trace runs 6 waves per SIMD, k_pool 4), but each of its ~8 rounds costs a launch ramp, a
        // drain tail and a host round trip, ~1 ms per frame in total.  So the single-launch pool pipeline wins when a
        // frame takes less than ~6 ms on the wavefront pipeline - every C4 shard of a 4..8 GPU run, but also a full 1080p
        // frame of a scene whose rays are short (C3: 4.75 vs 5.85 ms).  Sample count alone cannot tell those apart, so in
        // the range where either can win the first call of a configuration renders the frame with both (twice each: the
        // first run of a pipeline allocates its workspace) and keeps the faster; the images are the same.  Outside
        // that range - and always when PRT_POOL_MAX_SAMPLES is set - the size decides.  (Below 1 M samples: pool.)
        // The try-out is opt-in (PRT_FLAG_TRYOUT): without it DEFAULT is the pool pipeline.
        const unsigned long long ns = (unsigned long long)px.n_pixels * params->spp;
        if (opt.pool_max_samples >= 0) {
            pipeline = ns <= (unsigned long long)opt.pool_max_samples ? PRT_PIPELINE_POOL : PRT_PIPELINE_WAVEFRONT;
        } else if (!(params->pipeline & PRT_FLAG_TRYOUT) || ns <= (1ull << 20)) {
            pipeline = PRT_PIPELINE_POOL;       // no try-out asked for (a one-off render would pay for it five-fold), or too small to matter
        } else {
            prt_ctx::TuneEntry e;
            e.key[0] = ctx->scene_epoch;
            e.key[1] = (uint64_t)px.n_pixels | (uint64_t)params->spp << 32;
            e.key[2] = (uint64_t)width | (uint64_t)height << 32;
            e.key[3] = (uint64_t)params->bounce_depth | (uint64_t)params->reflection_samples << 32;      // full-width fields: no aliasing
            e.key[4] = (uint64_t)params->spec_samples | (uint64_t)px.nranks << 32;
            e.key[5] = (uint64_t)px.block_rows | (uint64_t)(px.d_pixel_list ? 1 : 0) << 32;
            for (const prt_ctx::TuneEntry & t : ctx->tuned)
                if (!memcmp(t.key, e.key, sizeof(e.key))) pipeline = t.pipeline;
            if (pipeline == PRT_PIPELINE_DEFAULT) {
                // calls that will run in several passes (more than 64 M samples) try the two pipelines on their first
                // 32 M samples only (C5, 4K x 64 spp at depth 8: pool 1005 ms, wavefront 1181 ms per frame)
                PixelSet trial = px;
                const bool whole = ns <= (64ull << 20);
                if (!whole) trial.n_pixels = (uint32_t)std::max<unsigned long long>(64, ((32ull << 20) / params->spp) / 64 * 64);
                const unsigned int cand[2] = { PRT_PIPELINE_POOL, PRT_PIPELINE_WAVEFRONT };
                double ms[2] = { 0.0, 0.0 };
                prt_counters c;
                for (int run = 0; run < 4; ++run) {                        // pool, wavefront (cold), pool, wavefront (timed)
                    prt_params pp = *params;
                    pp.pipeline = (params->pipeline & ~(uint32_t)PRT_PIPELINE_MASK) | cand[run & 1];
                    int rc = render_pixels(ctx, cam_in, &pp, width, height, trial, d_out, &c);
                    if (rc) return rc;
                    ms[run & 1] = c.render_ms;
                }
                // run-to-run noise is 2-3 %: the pool pipeline has to win by more than that to displace the other
                e.pipeline = ms[0] <= 0.97 * ms[1] ? PRT_PIPELINE_POOL : PRT_PIPELINE_WAVEFRONT;
                if (ctx->tuned.size() >= 64) ctx->tuned.erase(ctx->tuned.begin());
                ctx->tuned.push_back(e);
                if (opt.debug_util) fprintf(stderr, "[prt] default pipeline try-out: pool %.3f ms, wavefront %.3f ms\n", ms[0], ms[1]);
                // the call itself is then served by the winner like every later one, so that the counters (pipeline, kernel
                // times) describe the pipeline this configuration will keep
                (void)whole;
                pipeline = e.pipeline;
            }
        }
    }
    if (pipeline == PRT_PIPELINE_MEGAKERNEL || pipeline == PRT_PIPELINE_PERSISTENT) {
        // reserved values (include/prt.h): round 1's megakernel and the persistent single-launch pipeline, measured and removed
        ctx->error = "prt_render: the experimental pipelines (MEGAKERNEL, PERSISTENT) are not built into this library";
        return -1;
    }
    if (pipeline != PRT_PIPELINE_WAVEFRONT && pipeline != PRT_PIPELINE_POOL) { ctx->error = "prt_render: unknown pipeline"; return -1; }

    // The pool kernel always runs its general-RNG variant: with the draw ring in memory it fits 96 VGPRs with 29 dwords
    // spilled and runs 5 waves per SIMD, where the 2-register RNG variant spills 105 (measured: 14.7 vs 15.3 ms per C4 frame
    // at 4 waves per SIMD; same random numbers either way).
    const bool ring_eff = ring || pipeline == PRT_PIPELINE_POOL;

    // Passes.  The per-sample workspace (radiance, RNG, pending frames, ray queues) is 100 B .. 1 KB per sample, so a
    // 4K x 64 spp frame (530 M samples) does not fit any GPU in one piece: the call's pixel set is rendered in passes of
    // whole pixels, each at most 64 M samples and at most 64 GB of workspace (PRT_PASS_SAMPLES / PRT_PASS_MB override).
    // One pass for everything up to 4K x 8 spp.
    const unsigned int unit_spp = adaptive ? 1u : P.spp;            // work items per pixel: samples, or the pixel itself
    const unsigned long long total_samples = (unsigned long long)px.n_pixels * unit_spp;
    unsigned int pass_pixels = px.n_pixels;
    {
        const unsigned long long lv = std::max(1u, P.bounce_depth), fr4 = ctx->desc.textured ? 7 : ring_eff ? 5 : 4, nl = std::max(1u, ctx->scene.light_count);
        unsigned long long per_sample = 32 + (ring ? 128 : 0);
        if (pipeline == PRT_PIPELINE_WAVEFRONT) per_sample += (lv * fr4 + 7 + 3 * nl) * 16 + (ring ? 32 : 16) + 4 * (1 + nl);
        if (pipeline == PRT_PIPELINE_POOL) per_sample += lv * fr4 * 16 + 32;
        if (adaptive) per_sample += ((unsigned long long)P.max_spp + 2) * 16;
        // A pass ends with a drain (the waves run dry one by one), so fewer, larger passes are faster - C5: 8 passes 1,046 - 1,076
        // ms, 4 passes 1,002, 3 passes 977 - 992 (profiles/r02_c5_pass_size.txt) - and 288 GB are there to be used: up to 192 M
        // samples and 160 GB of workspace per pass, but no more than 80 % of what the device has free plus what this context
        // already holds (a second context on the same GPU - two frames in flight - gets what is left, not an allocation failure).
        unsigned long long max_samples = 192ull << 20, max_mb = 160ull << 10;
        {
            size_t free_b = 0, total_b = 0;
            if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
                unsigned long long held = ctx->sample_rgb.bytes() + ctx->ring_ws.bytes() + ctx->pool_f4.bytes() + ctx->adapt_f4.bytes() +
                                          ctx->stack_spill.bytes() + ctx->pool_fin.bytes();
                for (int c = 0; c < PRT_MAX_CHAINS; ++c) held += ctx->chain[c].f4.bytes() + ctx->chain[c].rng.bytes() + ctx->chain[c].overflow.bytes() + ctx->chain[c].slow_stack.bytes();
                const unsigned long long budget_mb = (unsigned long long)(0.8 * (double)(free_b + held)) >> 20;
                max_mb = std::max(1024ull, std::min(max_mb, budget_mb));
            }
        }
        if (opt.pass_samples >= 0) max_samples = std::max(1ull, (unsigned long long)opt.pass_samples);
        if (opt.pass_mb >= 0) max_mb = std::max(1ull, (unsigned long long)opt.pass_mb);
        max_samples = std::min(max_samples, std::max(1ull, (max_mb << 20) / per_sample));
        max_samples = std::min(max_samples, 0x7FFFFFFFull);
        if (total_samples > max_samples) {
            unsigned long long pp = std::max(1ull, max_samples / unit_spp);
            if (pp > 64) pp = pp / 64 * 64;                                 // passes start on a wave boundary
            pass_pixels = (unsigned int)std::min<unsigned long long>(pp, px.n_pixels);
        }
    }
    const size_t n_samples64 = (size_t)pass_pixels * unit_spp;              // work items of the largest pass
    if (n_samples64 > 0x7FFFFFFFull) { ctx->error = "prt_render: spp too large for one pixel per pass"; return -1; }
    HIP_TRY(ctx, ctx->sample_rgb.ensure(2 * n_samples64));      // 32-byte fixed-point accumulators
    HIP_TRY(ctx, ctx->counters.ensure(1));
    if (ring) HIP_TRY(ctx, ctx->ring_ws.ensure(n_samples64 * 16));

    // Traversal stack: LDS column of up to STACK_LDS_CAP entries per lane (occupancy); the rest of the worst-case bound
    // - 3 pushes per 4-wide level are possible, nothing real comes close - lives in a per-lane global column behind it
    // (dev_trace.h LdsStack).
    constexpr int BLOCK = 256;
    const unsigned int stack_entries = lds_stack_entries(ctx);
    const size_t lds = stack_dwords(stack_entries, BLOCK) * sizeof(int);
    P.stack_lds_entries = stack_entries;
    P.stack_spill = nullptr;
    P.stack_spill_stride = 0;     // the pool and wavefront pipelines size their spill columns where they know their grids (launch_pool, chain_setup)

    HIP_TRY(ctx, hipMemsetAsync(ctx->counters.p, 0, sizeof(DevCounters), stream));
    HIP_TRY(ctx, hipEventRecord(ctx->ev[0], stream));
    unsigned int launches = 0;
    unsigned long long host_ray_count = 0;
    float trace_ms_accum = 0.0f;
    const bool single_launch = pipeline == PRT_PIPELINE_POOL;
    for (unsigned int p0 = 0; p0 < px.n_pixels; p0 += pass_pixels) {
        const unsigned int n_px = std::min(pass_pixels, px.n_pixels - p0);
        const unsigned int n_samples = n_px * unit_spp;
        const bool last_pass = p0 + n_px == px.n_pixels;
        P.local_base = p0;
        if (single_launch) HIP_TRY(ctx, hipEventRecord(ctx->ev[2], stream));
        int rc = 0;
        if (pipeline == PRT_PIPELINE_POOL) {
            // 256-thread blocks, the Hammersley direction table in global memory (staging it in LDS measured 17.04 vs 17.15 ms:
            // nothing).  Small blocks retire - and let the blocks of the next frame's kernel in - at a finer grain: with two
            // frames in flight a 1/8-frame shard takes 2.24 ms per frame instead of 2.59 with 512-thread blocks.
            // Untextured fixed-spp renders: 5 waves per SIMD (96 VGPRs, 23 dwords spilled).  Textured (64 spilled at 96) and
            // adaptive (68 spilled at 96, no gain measured: profiles/r02_experiments.txt item 11) renders: 4 waves per SIMD.
            // 6 waves (80 VGPRs) spill 90-230 dwords: 29 ms.
            // last argument (k_pool's RINGMEM): 0 = no sample passes 15 draws (and the scene is opaque and untextured): no draw ring
            // in memory; 1 = draw ring, materials may be translucent; 2 = draw ring, opaque scene: the translucency paths and the
            // frames' hit position fold away as they do for 0.  2 is used for the adaptive mode (-3.6 % on C4 10..50 spp); the
            // fixed-spp kernel for deep bounce trees allocates worse with it at 96 VGPRs (47 dwords spilled instead of 31: +1 %)
            // and stays on 1 (profiles/r03_adaptive.txt item 7)
            const bool opaque = !ctx->desc.any_translucent && !ctx->desc.textured;
            if (adaptive)
                rc = ctx->desc.textured ? launch_pool<256, 4, false, true, true, true>(ctx, count_visits, cam, P, n_samples, stack_entries)
                   : opaque ? launch_pool<256, PRT_ADAPT_WAVES, false, true, false, true, 2>(ctx, count_visits, cam, P, n_samples, stack_entries)
                            : launch_pool<256, PRT_ADAPT_WAVES, false, true, false, true, 1>(ctx, count_visits, cam, P, n_samples, stack_entries);
            else
                rc = ctx->desc.textured ? launch_pool<256, 4, false, true, true, false>(ctx, count_visits, cam, P, n_samples, stack_entries)
                   : !ring ? launch_pool<PRT_POOL_BLOCK, PRT_POOL_WAVES, false, true, false, false, 0>(ctx, count_visits, cam, P, n_samples, stack_entries)
                           : launch_pool<PRT_POOL_BLOCK, PRT_DEEP_WAVES, false, true, false, false, 1>(ctx, count_visits, cam, P, n_samples, stack_entries);
            launches += 1;
        } else {
            unsigned long long n_rays = 0;
            float tms = 0.0f;
            unsigned int nl = 0;
            rc = render_wavefront(ctx, cam, rays, (unsigned long long)p0 * P.spp, P, ring, count_visits, n_samples, lds, &n_rays, &tms, &nl);
            host_ray_count += n_rays;
            trace_ms_accum += tms;
            launches += nl;
        }
        if (rc) return rc;
        HIP_TRY(ctx, hipGetLastError());
        if (single_launch) HIP_TRY(ctx, hipEventRecord(ctx->ev[3], stream));
        // work items of this pass -> their places in the call's output (tiled work order, dev_scene.h local_of_work)
        ResolveMap rmap;
        rmap.base = p0; rmap.width = P.width; rmap.tile_pixels = P.tile_pixels; rmap.reverse_n = P.work_reverse_n; rmap.scatter_n = P.work_scatter_n; rmap.scatter_mul = P.work_scatter_mul;
        if (adaptive)       // k_pool<ADAPT> has already divided by each pixel's own sample count
            hipLaunchKernelGGL(k_resolve<false>, dim3((n_px + 255) / 256), dim3(256), 0, stream,
                               ctx->adapt_f4.p + ((size_t)P.max_spp + 1u) * n_samples, d_out, n_px, 1u, rmap);
        else
            launch_resolve(stream, ctx->sample_rgb.p, d_out, n_px, P.spp, rmap);
        HIP_TRY(ctx, hipGetLastError());
        if (single_launch && (counters || !last_pass)) {
            // the next pass reuses ev[2] / ev[3] (and the workspace is stream ordered anyway): take this pass's time now
            float tms = 0.0f;
            HIP_TRY(ctx, hipEventSynchronize(ctx->ev[3]));
            HIP_TRY(ctx, hipEventElapsedTime(&tms, ctx->ev[2], ctx->ev[3]));
            trace_ms_accum += tms;
        }
    }
    // the counters travel on the context's own stream into pinned memory, in front of the event the host waits for: no
    // synchronous copy through the null stream, which CU-masked (blocking) streams of other contexts would be ordered against
    HIP_TRY(ctx, hipMemcpyAsync(ctx->host_counters, ctx->counters.p, sizeof(DevCounters), hipMemcpyDeviceToHost, stream));
    HIP_TRY(ctx, hipEventRecord(ctx->ev[1], stream));
    HIP_TRY(ctx, hipEventSynchronize(ctx->ev[1]));

    *park_overflow = false;
    DevCounters h = *ctx->host_counters;
    if (pipeline == PRT_PIPELINE_POOL && (h.park_over[0] || h.park_over[1])) {
        // a park list was too short for one of this call's launches (kernels_pool.h PoolBuffers::park): rays were dropped.  The
        // device decided that per launch, against the capacity that launch's lists had (every pass clamps them to its own
        // worst case).  Longer lists, then the caller renders the frame again: a capacity above the largest demand seen is
        // above every pass's demand, and a pass whose clamp is smaller than that cannot want more than its clamp.
        if (opt.debug_util) fprintf(stderr, "[prt] park lists too short (a pass wanted %llu ray / %llu shadow-ray entries): enlarging\n",
                                    (unsigned long long)h.park_over[0], (unsigned long long)h.park_over[1]);
        ctx->pool_park_cap = std::max<size_t>(ctx->pool_park_cap, (size_t)h.park_over[0] + (size_t)h.park_over[0] / 2);
        ctx->pool_spark_cap = std::max<size_t>(ctx->pool_spark_cap, (size_t)h.park_over[1] + (size_t)h.park_over[1] / 2);
        *park_overflow = true;
        return 0;
    }
    if (h.near_tie_unresolved) {
        // resolve_near_ties ran out of widenings (dev_trace.h): some hit among near-coincident candidates was decided over an
        // incomplete candidate set.  Never seen on real geometry; reported, not hidden.
        char msg[160];
        snprintf(msg, sizeof(msg), "prt_render: %llu near-tied hits could not be resolved within %lld widenings of the candidate set",
                 (unsigned long long)h.near_tie_unresolved, opt.tie_widen_max);
        ctx->error = msg;
        return -8;
    }
    if (counters) {
        {
            prt_render_stats & rs = ctx->last_stats;
            memset(&rs, 0, sizeof(rs));
            rs.node_visits = h.node_visits; rs.tri_tests = h.tri_tests;
            rs.wave_node_steps = h.wave_node_steps; rs.wave_tri_steps = h.wave_tri_steps; rs.wave_leaf_visits = h.wave_leaf_steps;
            rs.wave_refills = h.wave_refills; rs.deepest_stack = h.max_sp;
            for (int k = 0; k < 5; ++k) rs.phase_cycles[k] = h.phase_cycles[k];
            rs.parked_rays = h.park_peak[0]; rs.parked_shadow_rays = h.park_peak[1];
            rs.elided_shadow_rays = h.elided_shadow_rays;
            rs.open_shadow_rays = h.open_shadow_rays;
            rs.cone_culled_nodes = h.cone_culled_nodes;
            rs.variance_close_calls = h.variance_close_calls;
            rs.stack_lds_entries = stack_entries; rs.stack_bound = ctx->desc.stack_bound;
            // k_pool's COUNT variants fill the table; the steps that have counters of their own are copied into their rows
            uint64_t * const rg = ctx->last_regions;
            for (int k = 0; k < 2 * PRT_REGION_COUNT; ++k) rg[k] = pipeline == PRT_PIPELINE_POOL ? h.region[k] : 0;
            if (pipeline == PRT_PIPELINE_POOL && h.region[2 * PRT_REGION_WAVE]) {
                rg[2 * PRT_REGION_NODE_STEP] = h.wave_node_steps; rg[2 * PRT_REGION_NODE_STEP + 1] = h.node_visits;
                rg[2 * PRT_REGION_LEAF] = h.wave_leaf_steps;
                rg[2 * PRT_REGION_TRI] = h.wave_tri_steps; rg[2 * PRT_REGION_TRI + 1] = h.tri_tests;
            }
        }
        float ms = 0.0f;
        const float trace_ms = trace_ms_accum;
        HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
        if (pipeline == PRT_PIPELINE_WAVEFRONT) h.ray_count = host_ray_count;      // every queued ray is one TraceRay call
        else host_ray_count = h.ray_count;
        if (opt.debug_util && h.wave_node_steps)
            fprintf(stderr, "[prt] lane utilisation: node loop %.1f%% (%llu wave steps), triangle tests %.1f%% (%llu wave steps, %llu leaf visits), %llu refills (%.1f rays each)\n",
                    100.0 * (double)h.node_visits / (64.0 * (double)h.wave_node_steps), (unsigned long long)h.wave_node_steps,
                    100.0 * (double)h.tri_tests / (64.0 * (double)h.wave_tri_steps), (unsigned long long)h.wave_tri_steps,
                    (unsigned long long)h.wave_leaf_steps, (unsigned long long)h.wave_refills,
                    h.wave_refills ? (double)host_ray_count / (double)h.wave_refills : 0.0);
        if (opt.debug_util && h.wave_node_step_rays)
            fprintf(stderr, "[prt] k_pool node loop, lane slots per wave step: %.1f%% walking, %.1f%% holding a ray but not walking (at a leaf, or done), %.1f%% without a ray\n",
                    100.0 * (double)h.node_visits / (64.0 * (double)h.wave_node_steps),
                    100.0 * ((double)h.wave_node_step_rays - (double)h.node_visits) / (64.0 * (double)h.wave_node_steps),
                    100.0 * (64.0 * (double)h.wave_node_steps - (double)h.wave_node_step_rays) / (64.0 * (double)h.wave_node_steps));
        if (opt.debug_util && h.drain_node_steps && h.wave_node_steps)
            fprintf(stderr, "[prt] k_pool round drains (node steps taken after a round's list ran dry): %.1f%% of the wave-level node steps, %.1f%% of their lane slots hold a ray; "
                            "the steps before the list ran dry: %.1f%% of lane slots hold a ray\n",
                    100.0 * (double)h.drain_node_steps / (double)h.wave_node_steps, 100.0 * (double)h.drain_node_step_rays / (64.0 * (double)h.drain_node_steps),
                    100.0 * ((double)h.wave_node_step_rays - (double)h.drain_node_step_rays) / (64.0 * ((double)h.wave_node_steps - (double)h.drain_node_steps)));
        if (opt.debug_util && h.phase_cycles[3])
            fprintf(stderr, "[prt] k_pool wave time by phase: top-up %.1f%%, trace %.1f%%, shade %.1f%% of the main loop\n",
                    100.0 * (double)h.phase_cycles[0] / (double)h.phase_cycles[3], 100.0 * (double)h.phase_cycles[1] / (double)h.phase_cycles[3],
                    100.0 * (double)h.phase_cycles[2] / (double)h.phase_cycles[3]);
        if (opt.debug_util && h.wave_count)
            fprintf(stderr, "[prt] k_pool waves: %llu, main loop mean %.3f of the longest wave's (what the others idle at the end of the frame: %.1f%%)\n",
                    (unsigned long long)h.wave_count, (double)h.wave_cycles_sum / (double)h.wave_count / (double)h.wave_cycles_max,
                    100.0 * (1.0 - (double)h.wave_cycles_sum / (double)h.wave_count / (double)h.wave_cycles_max));
        if (opt.debug_util && ctx->wave_times_n && pipeline == PRT_PIPELINE_POOL) {
            // where the end of the frame goes: every wave's (start, sample counter dry, exit) on the 100 MHz wall clock
            std::vector<unsigned long long> wt(3u * (size_t)ctx->wave_times_n);
            if (hipMemcpy(wt.data(), ctx->wave_times.p, wt.size() * 8, hipMemcpyDeviceToHost) == hipSuccess) {
                unsigned long long t0 = ~0ull;
                for (size_t i = 0; i < wt.size(); i += 3) t0 = std::min(t0, wt[i]);
                std::vector<double> start, dry, end, chain;
                for (size_t i = 0; i < wt.size(); i += 3) {
                    start.push_back((double)(wt[i] - t0) * 1e-5);
                    end.push_back((double)(wt[i + 2] - t0) * 1e-5);
                    if (wt[i + 1]) { dry.push_back((double)(wt[i + 1] - t0) * 1e-5); chain.push_back((double)(wt[i + 2] - wt[i + 1]) * 1e-5); }
                }
                auto pct = [](std::vector<double> & v, double q) { if (v.empty()) return 0.0; std::sort(v.begin(), v.end()); return v[std::min(v.size() - 1, (size_t)(q * (double)v.size()))]; };
                fprintf(stderr, "[prt] k_pool waves on the wall clock (ms since the first wave started; last pass): start p50 %.3f max %.3f | counter dry p10 %.3f p50 %.3f p90 %.3f max %.3f | exit p10 %.3f p50 %.3f p90 %.3f p99 %.3f max %.3f | exit - dry p50 %.3f p90 %.3f max %.3f\n",
                        pct(start, 0.5), pct(start, 1.0), pct(dry, 0.1), pct(dry, 0.5), pct(dry, 0.9), pct(dry, 1.0),
                        pct(end, 0.1), pct(end, 0.5), pct(end, 0.9), pct(end, 0.99), pct(end, 1.0), pct(chain, 0.5), pct(chain, 0.9), pct(chain, 1.0));
            }
        }
        if (opt.debug_util && h.phase_cycles[3] && h.phase_cycles[4])
            fprintf(stderr, "[prt] k_pool adaptive finalise step (store the sample, variance rule, next camera ray): %.1f%% of the main loop\n",
                    100.0 * (double)h.phase_cycles[4] / (double)h.phase_cycles[3]);
        if (opt.debug_util && h.wave_node_steps)
            fprintf(stderr, "[prt] deepest stack %llu entries (LDS column %u, bound %u); %llu of %llu node visits (%.1f%%) hit no child after a hit was known\n",
                    (unsigned long long)h.max_sp, stack_entries, ctx->desc.stack_bound, (unsigned long long)h.culled,
                    (unsigned long long)h.node_visits, 100.0 * (double)h.culled / (double)h.node_visits);
        memset(counters, 0, sizeof(*counters));
        counters->ray_count = h.ray_count;
        counters->node_visits = h.node_visits;
        counters->tri_tests = h.tri_tests;
        counters->shaded_hits = h.shaded_hits;
        counters->render_ms = ms;
        counters->trace_kernel_ms = trace_ms;
        counters->trace_kernel_launches = launches;
        counters->pipeline = pipeline;
    }
    return 0;
}

int render_pixels(prt_ctx * ctx, const prt_camera * cam_in, const prt_params * params, uint32_t width, uint32_t height,
                  const PixelSet & px, float4 * d_out, prt_counters * counters) {
    for (int attempt = 0; attempt < 4; ++attempt) {
        bool park_overflow = false;
        const int rc = render_pixels_once(ctx, cam_in, params, width, height, px, d_out, counters, &park_overflow);
        if (rc || !park_overflow) return rc;
    }
    ctx->error = "prt_render: the pool pipeline's park lists kept overflowing";
    return -7;
}

// ---- batched queries: what the five of them share -------------------------------------------------------------------------------

// The arrays of a call whose arrays are host pointers.  Each is described once - the pointer in the kernel's argument struct (it
// holds the caller's host pointer on entry), its bytes, whether it is wanted and which way it travels - and carve(), upload() and
// download() loop over the description.  The device copies lie in one slab of 4-byte words, in the order of the description.
struct StageList {
    struct Field {
        void * slot;                       // the address of the pointer: the caller's array before carve(), the device copy after it
        void * host;
        size_t bytes;
        bool on, out, in_slab;
    };
    Field f[16];                           // (the ray gradients' twelve arrays are the most a call has)
    size_t n = 0;
    template <typename T>
    void in(T ** slot, size_t bytes) { f[n++] = { (void *)slot, nullptr, bytes, *slot != nullptr, false, true }; }
    // in_slab = false: device memory of its own, which the caller puts into the slot after carve()
    template <typename T>
    void out(T ** slot, size_t bytes, bool on, bool in_slab = true) { f[n++] = { (void *)slot, nullptr, bytes, on, true, in_slab }; }

    static size_t words(const Field & x) { return (x.bytes + 3) / 4; }
    // Sizes the slab and points every slot at its part of it; the slot of an array that is not wanted becomes null.
    hipError_t carve(DevBuf<float> & slab) {
        size_t total = 0;
        for (size_t i = 0; i < n; ++i) if (f[i].on && f[i].in_slab) total += words(f[i]);
        const hipError_t e = slab.ensure(total);
        if (e != hipSuccess) return e;
        float * p = slab.p;
        for (size_t i = 0; i < n; ++i) {
            memcpy(&f[i].host, f[i].slot, sizeof(void *));
            void * dev = nullptr;
            if (f[i].on && f[i].in_slab) { dev = p; p += words(f[i]); }
            if (f[i].in_slab || !f[i].on) memcpy(f[i].slot, &dev, sizeof(void *));
        }
        return hipSuccess;
    }
    hipError_t copy(bool out, hipStream_t stream) const {
        for (size_t i = 0; i < n; ++i) {
            if (!f[i].on || f[i].out != out || (out && !f[i].bytes)) continue;
            void * dev;
            memcpy(&dev, f[i].slot, sizeof(void *));
            const hipError_t e = out ? hipMemcpyAsync(f[i].host, dev, f[i].bytes, hipMemcpyDeviceToHost, stream)
                                     : hipMemcpyAsync(dev, f[i].host, f[i].bytes, hipMemcpyHostToDevice, stream);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    }
    hipError_t upload(hipStream_t stream) const { return copy(false, stream); }
    hipError_t download(hipStream_t stream) const { return copy(true, stream); }
};

// The leaf -> (group, vertex0) table of the queries (prt_trace_rays, prt_closest_points), built by the first of them after an upload.
int ensure_leaf_map(prt_ctx * ctx, const char * who) {
    if (ctx->tables.q_leaf_map.p) return 0;
    const uint32_t n_tris = ctx->scene.tri_count;
    if (ctx->keep.tri_order.size() != n_tris) { ctx->error = std::string(who) + ": the scene's leaf order is not available"; return -2; }
    HIP_TRY(ctx, ctx->tables.q_leaf_map.upload(keep_leaf_map(ctx->keep)));
    HIP_TRY(ctx, hipDeviceSynchronize());              // the upload went through the null stream
    return 0;
}

int ensure_signed_tables(prt_ctx * ctx, ClosestArgs & A);

// Dwords of dynamic LDS a walk keeps behind its stack columns: prt_trace_hits' sorted lists, 2 k words per lane (kernels_hits.h).
template <typename Args>
size_t walk_list_dwords(const Args &, size_t) { return 0; }
size_t walk_list_dwords(const HitsArgs & A, size_t lanes) { return 2 * (size_t)A.k * lanes; }

// The fast walk on its persistent grid, then the exact kernel for the items it set aside; its fixed grid reads the list's length
// on the device.
template <typename Fast, typename Exact, typename Args>
int launch_walk(prt_ctx * ctx, Fast fast, Exact exact, const Args & A, unsigned int fields) {
    constexpr int BLOCK = 256;
    const size_t lds = (stack_dwords(A.stack_lds_entries, BLOCK) + walk_list_dwords(A, BLOCK)) * sizeof(int);
    const TraceRule rule = trace_rule(ctx, fast, lds);
    const TraceGrid g = trace_grid(ctx, rule.per_cu, rule.chunk_min, A.count);
    hipLaunchKernelGGL(fast, dim3(g.grid), dim3(BLOCK), lds, ctx->stream, ctx->scene, A, ctx->tables.q_leaf_map.p, fields, rule.keep_min, rule.node_min,
                       g.chunk, ctx->counters.p);
    HIP_TRY(ctx, hipGetLastError());
    constexpr unsigned int SLOW_BLOCKS = 64;               // A.exact_stack holds SLOW_BLOCKS * 256 columns
    hipLaunchKernelGGL(exact, dim3(SLOW_BLOCKS), dim3(256), 0, ctx->stream, ctx->scene, A, ctx->tables.q_leaf_map.p, fields, ctx->counters.p);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

// What a query supplies to run_batch: its argument struct, its name in the error texts, and the steps that are its own.
struct RayWalk {
    typedef QueryArgs Args;
    int mode;
    static const char * name() { return "prt_trace_rays"; }
    int prepare(prt_ctx * ctx, QueryArgs & A) const {
        ctx->scene.tie_widen_max = (unsigned int)std::max(0ll, std::min(64ll, ctx->opt.tie_widen_max));
        A.replay_beyond = 64.0f * ctx->desc.scene_abs_max;
        A.scene_max = ctx->desc.scene_abs_max;
        const uint32_t n_tris = ctx->scene.tri_count;
        if (!ctx->tables.q_slot_of_rank.p && n_tris) {
            std::vector<unsigned int> rank(n_tris), slot_of_rank(n_tris, 0u);
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));          // an update's copy of the ranks runs on it
            HIP_TRY(ctx, hipMemcpy(rank.data(), ctx->arrays.tri_rank.p, (size_t)n_tris * sizeof(unsigned int), hipMemcpyDeviceToHost));
            for (uint32_t slot = 0; slot < n_tris; ++slot) {
                if (rank[slot] >= n_tris) { ctx->error = "prt_trace_rays: the scene's visit ranks are not a permutation"; return -2; }
                slot_of_rank[rank[slot]] = slot;
            }
            HIP_TRY(ctx, ctx->tables.q_slot_of_rank.upload(slot_of_rank));
            HIP_TRY(ctx, hipDeviceSynchronize());          // the upload went through the null stream
        }
        A.slot_of_rank = ctx->tables.q_slot_of_rank.p;
        return 0;
    }
    int tables(prt_ctx *, QueryArgs &, unsigned int) const { return 0; }
    static void (*pad_kernel())(QueryArgs) { return k_query_pad; }
    int launch(prt_ctx * ctx, const QueryArgs & A, unsigned int fields, bool count) const {
        if (mode == PRT_QUERY_OCCLUDED)
            return count ? launch_walk(ctx, k_query<256, QUERY_OCCLUDED, true>, k_query_exact<QUERY_OCCLUDED, true>, A, fields)
                         : launch_walk(ctx, k_query<256, QUERY_OCCLUDED, false>, k_query_exact<QUERY_OCCLUDED, false>, A, fields);
        return count ? launch_walk(ctx, k_query<256, QUERY_CLOSEST, true>, k_query_exact<QUERY_CLOSEST, true>, A, fields)
                     : launch_walk(ctx, k_query<256, QUERY_CLOSEST, false>, k_query_exact<QUERY_CLOSEST, false>, A, fields);
    }
    int verdict(prt_ctx * ctx, const DevCounters & h) const {
        if (h.near_tie_unresolved) {
            char msg[160];
            snprintf(msg, sizeof(msg), "prt_trace_rays: %llu near-tied hits could not be resolved within %lld widenings of the candidate set",
                     (unsigned long long)h.near_tie_unresolved, ctx->opt.tie_widen_max);
            ctx->error = msg;
            return -8;
        }
        if (ctx->opt.debug_util && h.wave_node_steps)
            fprintf(stderr, "[prt] k_query: node loop %.1f%% of lanes (%llu wave steps), triangle tests %.1f%% (%llu wave steps, %llu leaf visits), %llu refills\n",
                    100.0 * (double)h.node_visits / (64.0 * (double)h.wave_node_steps), (unsigned long long)h.wave_node_steps,
                    100.0 * (double)h.tri_tests / (64.0 * (double)h.wave_tri_steps), (unsigned long long)h.wave_tri_steps,
                    (unsigned long long)h.wave_leaf_steps, (unsigned long long)h.wave_refills);
        return 0;
    }
};

struct PointWalk {
    typedef ClosestArgs Args;
    static const char * name() { return "prt_closest_points"; }
    int prepare(prt_ctx *, ClosestArgs &) const { return 0; }
    // prt_signed_distance: a refill of the accumulators counts in render_ms
    int tables(prt_ctx * ctx, ClosestArgs & A, unsigned int fields) const { return (fields & (CF_SIGNED | CF_FEATURE)) ? ensure_signed_tables(ctx, A) : 0; }
    static void (*pad_kernel())(ClosestArgs) { return k_closest_pad; }
    int launch(prt_ctx * ctx, const ClosestArgs & A, unsigned int fields, bool count) const {
        return count ? launch_walk(ctx, k_closest<256, true>, k_closest_exact<true>, A, fields)
                     : launch_walk(ctx, k_closest<256, false>, k_closest_exact<false>, A, fields);
    }
    int verdict(prt_ctx *, const DevCounters &) const { return 0; }
};

struct HitsWalk {
    typedef HitsArgs Args;
    bool back;
    static const char * name() { return "prt_trace_hits"; }
    int prepare(prt_ctx * ctx, HitsArgs & A) const {
        A.replay_beyond = 64.0f * ctx->desc.scene_abs_max;
        A.scene_max = ctx->desc.scene_abs_max;
        HIP_TRY(ctx, ctx->q_hits_lists.ensure(2 * (size_t)HITS_MAX * 64 * 256));       // one column per lane of the exact kernel's grid
        A.exact_lists = ctx->q_hits_lists.p;
        return 0;
    }
    int tables(prt_ctx *, HitsArgs &, unsigned int) const { return 0; }
    static void (*pad_kernel())(QueryArgs) { return k_query_pad; }                  // (a HitsArgs is a QueryArgs)
    int launch(prt_ctx * ctx, const HitsArgs & A, unsigned int fields, bool count) const {
        if (back)
            return count ? launch_walk(ctx, k_hits<256, true, true>, k_hits_exact<true, true>, A, fields)
                         : launch_walk(ctx, k_hits<256, true, false>, k_hits_exact<true, false>, A, fields);
        return count ? launch_walk(ctx, k_hits<256, false, true>, k_hits_exact<false, true>, A, fields)
                     : launch_walk(ctx, k_hits<256, false, false>, k_hits_exact<false, false>, A, fields);
    }
    int verdict(prt_ctx *, const DevCounters &) const { return 0; }
};

// The items a batch's walk hands out - the slow list holds as many at the most: the batch's rays or points, unless the query
// makes several items of each (prt_hemisphere_visibility: a pass's points x samples).
template <typename Args>
size_t batch_items(const Args & A) { return A.count; }
size_t batch_items(const HemiArgs & A) { return (size_t)A.count * A.samples; }

// One batch on the device: A's inputs and outputs are device pointers; pad_max < 0 asks the pad kernel for the inputs' extent.
// Synchronous (returns after the context's stream has drained).  The work words, the slow list and the exact stacks are shared by
// all queries (a context runs one call at a time).
template <typename Walk>
int run_batch(prt_ctx * ctx, const Walk & q, typename Walk::Args A, unsigned int fields, bool count_visits, prt_counters * counters) {
    const int map_rc = ensure_leaf_map(ctx, Walk::name());
    if (map_rc) return map_rc;
    hipStream_t stream = ctx->stream;
    if (const int rc = q.prepare(ctx, A)) return rc;
    // LDS stack column as the render pipelines size it; the exact kernel's fixed grid gets full-height global columns
    A.stack_lds_entries = lds_stack_entries(ctx);
    const size_t exact_lanes = 64 * 256;
    HIP_TRY(ctx, ctx->q_exact_stack.ensure(stack_dwords(std::max(ctx->desc.stack_bound, 4u), exact_lanes)));
    A.exact_stack = ctx->q_exact_stack.p;
    A.exact_stack_stride = (unsigned int)exact_lanes;
    HIP_TRY(ctx, ctx->q_work.ensure(BATCH_WORDS));
    HIP_TRY(ctx, ctx->q_slow.ensure(batch_items(A)));
    HIP_TRY(ctx, ctx->counters.ensure(1));
    A.work = ctx->q_work.p;
    A.slow = ctx->q_slow.p;
    const bool device_pad = A.pad_max < 0.0f;
    if (device_pad) A.pad_max = ctx->desc.scene_abs_max;

    HIP_TRY(ctx, hipMemsetAsync(ctx->counters.p, 0, sizeof(DevCounters), stream));
    HIP_TRY(ctx, hipMemsetAsync(A.work, 0, BATCH_WORDS * sizeof(unsigned int), stream));
    HIP_TRY(ctx, hipEventRecord(ctx->ev[0], stream));
    if (const int rc = q.tables(ctx, A, fields)) return rc;
    if (device_pad) {
        hipLaunchKernelGGL(Walk::pad_kernel(), dim3(std::min(1024u, (A.count + 255) / 256)), dim3(256), 0, stream, A);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipEventRecord(ctx->ev[2], stream));
    if (const int rc = q.launch(ctx, A, fields, count_visits)) return rc;
    HIP_TRY(ctx, hipEventRecord(ctx->ev[3], stream));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->host_counters, ctx->counters.p, sizeof(DevCounters), hipMemcpyDeviceToHost, stream));
    HIP_TRY(ctx, hipEventRecord(ctx->ev[1], stream));
    HIP_TRY(ctx, hipEventSynchronize(ctx->ev[1]));
    const DevCounters h = *ctx->host_counters;
    if (const int rc = q.verdict(ctx, h)) return rc;
    if (counters) {
        float ms = 0.0f, tms = 0.0f;
        HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
        HIP_TRY(ctx, hipEventElapsedTime(&tms, ctx->ev[2], ctx->ev[3]));
        memset(counters, 0, sizeof(*counters));
        counters->ray_count = A.count;                     // one TraceRay call per ray
        counters->node_visits = h.node_visits;
        counters->tri_tests = h.tri_tests;
        counters->render_ms = ms;
        counters->trace_kernel_ms = tms;
        counters->trace_kernel_launches = 2;
        counters->pipeline = 0;
    }
    return 0;
}

unsigned int query_fields(int mode, const prt_hit_buffers * o) {
    if (!o) return 0u;
    if (mode == PRT_QUERY_OCCLUDED) return o->occluded ? (unsigned int)QF_OCCLUDED : 0u;
    return (o->t ? QF_T : 0) | (o->bw ? QF_BW : 0) | (o->vertex0 ? QF_VERTEX0 : 0) | (o->group ? QF_GROUP : 0) |
           (o->position ? QF_POSITION : 0) | (o->normal ? QF_NORMAL : 0);
}

// The checks both entry points share; 1 = nothing to trace (count 0: counters zeroed), 0 = go on, < 0 = error.
int query_check(prt_ctx * ctx, int mode, const prt_ray_batch * b, prt_counters * counters) {
    if (!ctx) return -1;
    if (mode != PRT_QUERY_CLOSEST && mode != PRT_QUERY_OCCLUDED) { ctx->error = "prt_trace_rays: unknown mode"; return -1; }
    if (!b) { ctx->error = "prt_trace_rays: null batch"; return -1; }
    if (b->count && (!b->origins || !b->directions)) { ctx->error = "prt_trace_rays: null origins or directions"; return -1; }
    if (!ctx->has_scene) { ctx->error = "prt_trace_rays: no scene uploaded"; return -2; }
    if (b->count == 0) {
        if (counters) memset(counters, 0, sizeof(*counters));
        return 1;
    }
    return 0;
}

// ---- closest points (prt_closest_points, kernels_closest.h) ------------------------------------------------------------------

unsigned int closest_fields(const prt_closest_buffers * o) {
    return (o->dist2 ? CF_DIST2 : 0) | (o->point ? CF_POINT : 0) | (o->bw ? CF_BW : 0) | (o->vertex0 ? CF_VERTEX0 : 0) | (o->group ? CF_GROUP : 0);
}

unsigned int signed_fields(const prt_signed_buffers * o) {
    return closest_fields(&o->closest) | (o->signed_dist ? CF_SIGNED : 0) | (o->feature ? CF_FEATURE : 0);
}

// The tables of prt_signed_distance (dev_signed.h) into A.sign: the adjacency once per upload, the accumulators once per
// geometry generation (k_signed_normals on the context's stream, ahead of the walk that reads them).
int ensure_signed_tables(prt_ctx * ctx, ClosestArgs & A) {
    const uint32_t n_tris = ctx->scene.tri_count, n_pos = ctx->keep.position_count;
    if (ctx->keep.tri_order.size() != n_tris || ctx->keep.idx_positions.size() != 3 * (size_t)n_tris) {
        ctx->error = "prt_signed_distance: the scene's index buffer is not available";
        return -2;
    }
    if (!ctx->tables.sg_adj.p) {
        uint32_t edge_count = 0;
        const std::vector<unsigned int> adj = keep_signed_adjacency(ctx->keep, &edge_count);
        hipError_t e = ctx->tables.sg_adj.upload(adj);
        if (e == hipSuccess) e = ctx->tables.sg_acc.ensure(3 * ((size_t)n_pos + edge_count));
        if (e == hipSuccess) e = hipDeviceSynchronize();          // the upload went through the null stream
        if (e != hipSuccess) {
            ctx->tables.sg_adj.release(); ctx->tables.sg_acc.release();
            ctx->error = std::string("prt_signed_distance: table upload: ") + hipGetErrorString(e);
            return -10;
        }
        ctx->tables.sg_edge_count = edge_count;
        ctx->tables.sg_generation = 0;
    }
    A.sign.adj = ctx->tables.sg_adj.p;
    A.sign.acc = ctx->tables.sg_acc.p;
    A.sign.position_count = n_pos;
    A.sign.edge_count = ctx->tables.sg_edge_count;
    if (ctx->tables.sg_generation != ctx->geom_generation) {
        const size_t words = 3 * ((size_t)n_pos + ctx->tables.sg_edge_count);
        const unsigned int cap = (unsigned int)std::max(1, ctx->cu_count) * 8u;
        const unsigned int grid0 = (unsigned int)std::max<size_t>(1, std::min<size_t>((words + 255) / 256, cap));
        hipLaunchKernelGGL(k_signed_normals, dim3(grid0), dim3(256), 0, ctx->stream, ctx->arrays.tris.p, n_tris, A.sign, 0);
        HIP_TRY(ctx, hipGetLastError());
        if (n_tris) {
            const unsigned int grid1 = std::max(1u, std::min((n_tris + 255u) / 256u, cap));
            hipLaunchKernelGGL(k_signed_normals, dim3(grid1), dim3(256), 0, ctx->stream, ctx->arrays.tris.p, n_tris, A.sign, 1);
            HIP_TRY(ctx, hipGetLastError());
        }
        ctx->tables.sg_generation = ctx->geom_generation;
    }
    return 0;
}

// The checks both entry points share; 1 = nothing to do (count 0: counters zeroed), 0 = go on, < 0 = error.
int closest_check(prt_ctx * ctx, const prt_point_batch * b, const prt_closest_buffers * o, prt_counters * counters) {
    if (!ctx) return -1;
    if (!b || !o) { ctx->error = "prt_closest_points: null batch or buffers"; return -1; }
    if (b->count && !b->points) { ctx->error = "prt_closest_points: null points"; return -1; }
    if (!ctx->has_scene) { ctx->error = "prt_closest_points: no scene uploaded"; return -2; }
    if (b->count == 0) {
        if (counters) memset(counters, 0, sizeof(*counters));
        return 1;
    }
    return 0;
}

}  // namespace

// =============================================================================================================
// "Nothing aborts" (include/prt.h): the entry points below use std::vector / std::string / std::thread / new, and an
// exception that leaves an extern "C" function is std::terminate - an abort of the CALLER's process.  Every entry point
// that can allocate therefore runs its body inside PRT_API_TRY ... PRT_API_CATCH_*: std::bad_alloc, std::length_error,
// std::system_error and anything else become PRT_ERR_EXCEPTION (-12) with the message in prt_last_error.
namespace {
int api_exception(std::string * err, const char * where) noexcept {
    char what[256] = "unknown C++ exception";
    try { throw; }
    catch (const std::bad_alloc &) { snprintf(what, sizeof(what), "out of host memory (std::bad_alloc)"); }
    catch (const std::exception & e) { snprintf(what, sizeof(what), "C++ exception: %s", e.what()); }
    catch (...) {}
    try { if (err) *err = std::string(where) + ": " + what; } catch (...) {}      // the message itself may not fit: keep the code
    return PRT_ERR_EXCEPTION;
}
}  // namespace
#define PRT_API_TRY try {
#define PRT_API_CATCH_RC(ctx, where) } catch (...) { prt_ctx * c_ = (ctx); return api_exception(c_ ? &c_->error : &g_create_error, where); }
#define PRT_API_CATCH_RC_MULTI(m, where) } catch (...) { prt_multi * m_ = (m); return api_exception(m_ ? &m_->error : &g_create_error, where); }
#define PRT_API_CATCH_PTR(where) } catch (...) { (void)api_exception(&g_create_error, where); return nullptr; }
#define PRT_API_CATCH_VOID } catch (...) {}

// =============================================================================================================
namespace {

// prt_update_geometry / prt_update_geometry_device: `device` says where positions / normals / tangents live.  Everything that
// can refuse the update - the arguments, the coordinates (k_refit_bounds) - comes before the first write to the scene's
// arrays; a HIP failure after it leaves the context without a scene rather than with half-moved arrays.
int update_geometry(prt_ctx * ctx, const prt_geometry_update * u, prt_update_info * info, bool device) {
    if (!ctx) return -1;
    if (info) memset(info, 0, sizeof(*info));
    if (!u || !u->positions) { ctx->error = "prt_update_geometry: null update or null positions"; return -1; }
    if (!ctx->has_scene) { ctx->error = "prt_update_geometry: upload a scene first"; return -2; }
    if (u->position_count != ctx->keep.position_count) { ctx->error = "prt_update_geometry: position_count differs from the uploaded scene's"; return -1; }
    if (u->normals && u->normal_count != ctx->keep.normal_count) { ctx->error = "prt_update_geometry: normal_count differs from the uploaded scene's"; return -1; }
    const uint32_t n_tris = ctx->scene.tri_count, n_nodes = ctx->scene.node_count;
    const uint32_t levels = ctx->keep.level_first.empty() ? 0u : (uint32_t)ctx->keep.level_first.size() - 1u;
    if (info) { info->levels = levels; info->node_count = n_nodes; info->abs_max = ctx->desc.scene_abs_max; }
    if (n_tris == 0) return 0;                                    // nothing references a position: nothing moves
    if (!levels || ctx->keep.tri_order.size() != n_tris || ctx->keep.idx_positions.size() != 3 * (size_t)n_tris) {
        ctx->error = "prt_update_geometry: the uploaded tree is not level-ordered and cannot be refitted (upload the moved scene instead)";
        return -9;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t stream = ctx->stream;
    HIP_TRY(ctx, hipStreamSynchronize(stream));

    // ---- host work that can fail, first: the reference's ranks for the moved scene's sphere tree
    std::vector<uint32_t> rank_of_input;
    std::vector<float4> ref_spheres;
    reference_ranks(ctx->keep.groups.data(), (uint32_t)ctx->keep.groups.size(), u->spheres, u->sphere_group, u->sphere_count, n_tris, rank_of_input, ref_spheres);
    std::vector<unsigned int> rank((size_t)n_tris + 1, 0u);
    for (uint32_t slot = 0; slot < n_tris; ++slot) rank[slot] = rank_of_input[ctx->keep.tri_order[slot]];

    // ---- the update's own device arrays (not the scene's): table, scratch boxes, the two words of k_refit_bounds, inputs
    if (!ctx->tables.rf_table.p) {
        hipError_t e = ctx->tables.rf_table.upload(keep_refit_table(ctx->keep));
        if (e != hipSuccess) { ctx->tables.rf_table.release(); ctx->error = std::string("prt_update_geometry: table upload: ") + hipGetErrorString(e); return -10; }
    }
    HIP_TRY(ctx, ctx->rf_boxes.ensure(n_nodes));
    HIP_TRY(ctx, ctx->rf_bounds.ensure(2));
    const bool with_tangents = u->tangents && ctx->keep.bumped && ctx->arrays.tri_tan.p;      // one per normal of the upload
    RefitArgs A;
    memset(&A, 0, sizeof(A));
    A.positions = u->positions;
    A.normals = u->normals;
    A.tangents = with_tangents ? u->tangents : nullptr;
    if (!device) {
        const size_t np = 3 * (size_t)u->position_count, nn = u->normals ? 3 * (size_t)u->normal_count : 0;
        const size_t nt = with_tangents ? 3 * (size_t)ctx->keep.normal_count : 0;
        HIP_TRY(ctx, ctx->rf_in.ensure(np + nn + nt));
        float * p = ctx->rf_in.p;
        HIP_TRY(ctx, hipMemcpyAsync(p, u->positions, np * sizeof(float), hipMemcpyHostToDevice, stream));
        A.positions = p; p += np;
        if (nn) { HIP_TRY(ctx, hipMemcpyAsync(p, u->normals, nn * sizeof(float), hipMemcpyHostToDevice, stream)); A.normals = p; p += nn; }
        if (nt) { HIP_TRY(ctx, hipMemcpyAsync(p, u->tangents, nt * sizeof(float), hipMemcpyHostToDevice, stream)); A.tangents = p; }
    }
    A.table = ctx->tables.rf_table.p;
    A.n_tris = n_tris;
    A.node_count = n_nodes;
    A.nodes = ctx->arrays.nodes.p; A.tris = ctx->arrays.tris.p; A.shade = ctx->arrays.shade.p;
    A.tri_tan = with_tangents ? ctx->arrays.tri_tan.p : nullptr;
    A.boxes = ctx->rf_boxes.p;
    A.bounds = ctx->rf_bounds.p;

    // ---- the coordinates, before anything of the scene is written
    HIP_TRY(ctx, hipEventRecord(ctx->ev[0], stream));
    HIP_TRY(ctx, hipMemsetAsync(A.bounds, 0, 2 * sizeof(unsigned int), stream));
    {
        const unsigned int want = (3u * n_tris + 255u) / 256u;
        const unsigned int grid = std::max(1u, std::min(want, (unsigned int)std::max(1, ctx->cu_count) * 8u));
        hipLaunchKernelGGL(k_refit_bounds, dim3(grid), dim3(256), 0, stream, A);
        HIP_TRY(ctx, hipGetLastError());
    }
    unsigned int bounds[2] = { 0u, 0u };
    HIP_TRY(ctx, hipMemcpyAsync(bounds, A.bounds, sizeof(bounds), hipMemcpyDeviceToHost, stream));
    HIP_TRY(ctx, hipStreamSynchronize(stream));
    if (bounds[1]) { ctx->error = "prt_update_geometry: vertex coordinate is not finite or exceeds 1e18"; return -1; }
    float abs_max;
    memcpy(&abs_max, &bounds[0], 4);

    // ---- from here on the scene's arrays change: a failure leaves the context without a scene
#define REFIT_TRY(call)                                                                                      \
    do {                                                                                                     \
        hipError_t e_ = (call);                                                                              \
        if (e_ != hipSuccess) {                                                                              \
            ctx->error = std::string(#call) + ": " + hipGetErrorString(e_);                                  \
            ctx->has_scene = false;                                                                          \
            return -10;                                                                                      \
        }                                                                                                    \
    } while (0)
    hipLaunchKernelGGL(k_refit_records, dim3((n_tris + 255u) / 256u), dim3(256), 0, stream, A);
    REFIT_TRY(hipGetLastError());
    for (uint32_t l = levels; l-- > 0;) {                         // deepest level first; the stream is the only ordering
        const unsigned int first = ctx->keep.level_first[l], count = ctx->keep.level_first[l + 1] - first;
        hipLaunchKernelGGL(k_refit_level<BVH_WIDTH>, dim3((count + 63u) / 64u), dim3(64), 0, stream, A, first, count);
        REFIT_TRY(hipGetLastError());
    }
    REFIT_TRY(hipMemcpyAsync(ctx->arrays.tri_rank.p, rank.data(), rank.size() * sizeof(unsigned int), hipMemcpyHostToDevice, stream));
    ctx->tables.q_slot_of_rank.release();                                // the next prt_trace_rays inverts the new ranks (the stream has drained by then)
    if (!ref_spheres.empty()) {
        REFIT_TRY(ctx->arrays.ref_spheres.ensure(ref_spheres.size()));
        REFIT_TRY(hipMemcpyAsync(ctx->arrays.ref_spheres.p, ref_spheres.data(), ref_spheres.size() * sizeof(float4), hipMemcpyHostToDevice, stream));
    }
    REFIT_TRY(hipEventRecord(ctx->ev[1], stream));
    REFIT_TRY(hipStreamSynchronize(stream));
    float ms = 0.0f;
    REFIT_TRY(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
#undef REFIT_TRY
    ctx->scene.ref_spheres = ref_spheres.empty() ? nullptr : ctx->arrays.ref_spheres.p;      // spheres of the old geometry are never kept
    ctx->desc.info.device_bytes += ref_spheres.size() * sizeof(float4) - ctx->desc.ref_sphere_bytes;
    ctx->desc.ref_sphere_bytes = ref_spheres.size() * sizeof(float4);
    ctx->desc.scene_abs_max = abs_max;
    // the shadow trees are of the uploaded geometry, in membership and in boxes: every shadow ray starts at the scene's root
    // until the next upload (render_pixels_once)
    ctx->desc.shadow_trees_fresh = false;
    for (prt_shadow_tree_info & si : ctx->desc.shadow_info) si.active = 0;
    // ... and so are the open-triangle flags: k_refit_records leaves the word where it is, no render reads it until the next upload
    for (prt_shadow_open_info & oi : ctx->desc.shadow_open_info) oi.active = 0;
    // the refit wrote every node's grid steps afresh, mantissas zero (dev_refit.h): the scene's tree carries no cone any more
    ctx->desc.cone_info.coned_nodes = 0;
    ctx->tuned.clear();                                           // a refitted tree may change which pipeline wins a try-out
    ctx->geom_generation++;                                       // the pseudonormals of prt_signed_distance are of the old records
    if (info) { info->device_ms = ms; info->abs_max = abs_max; }
    return 0;
}

// ---- what the two gradient calls share (prt_trace_rays_backward, prt_closest_points_backward): the device data, the scan's
// verdict, the vertex gradient's last step and the info.  `what` is the entry point's name, for the error text.

// The grid of the scan and scatter kernels: one lane per query, capped at 8 blocks of 256 per compute unit.
unsigned int grad_grid(const prt_ctx * ctx, uint32_t count) {
    return std::max(1u, std::min((count + 255u) / 256u, (unsigned int)std::max(1, ctx->cu_count) * 8u));
}

// The calls' own device data, built on the first gradient call of either kind after an upload: the position index buffer and
// the groups' runs; the control words; np accumulators when the vertex gradient is wanted.
int grad_prepare(prt_ctx * ctx, const char * what, size_t np, bool want_positions) {
    if (ctx->keep.idx_positions.size() != 3 * (size_t)ctx->scene.tri_count) { ctx->error = std::string(what) + ": the scene's index buffer is not available"; return -2; }
    if (!ctx->tables.qg_idx.p || !ctx->tables.qg_runs.p) {
        HIP_TRY(ctx, ctx->tables.qg_idx.upload(ctx->keep.idx_positions));
        HIP_TRY(ctx, ctx->tables.qg_runs.upload(keep_group_runs(ctx->keep)));
        HIP_TRY(ctx, hipDeviceSynchronize());                     // the uploads went through the null stream
    }
    HIP_TRY(ctx, ctx->qg_words.ensure(QGRAD_WORDS));
    if (want_positions) HIP_TRY(ctx, ctx->tables.qg_acc.ensure(np));
    return 0;
}

struct GradScan { unsigned int words[QGRAD_WORDS]; float m; int unit_exponent; };

// After the scan kernel's launch: its four words on the host.  An invalid reference refuses the call (-1) - no output of the
// caller's has been written yet.  Else M and the unit exponent of the batch.
int grad_scan_verdict(prt_ctx * ctx, const char * what, const char * queries, uint32_t count, hipStream_t stream, GradScan * out) {
    HIP_TRY(ctx, hipGetLastError());
    memset(out, 0, sizeof(*out));
    HIP_TRY(ctx, hipMemcpyAsync(out->words, ctx->qg_words.p, sizeof(out->words), hipMemcpyDeviceToHost, stream));
    HIP_TRY(ctx, hipStreamSynchronize(stream));
    if (out->words[QGRAD_W_INVALID]) {
        char msg[240];
        snprintf(msg, sizeof(msg), "%s: %u %s name a triangle the scene does not have (group out of range, vertex0 not a multiple of 3 or past its "
                 "group's run)", what, out->words[QGRAD_W_INVALID], queries);
        ctx->error = msg;
        return -1;
    }
    memcpy(&out->m, &out->words[QGRAD_W_MAX], 4);
    out->unit_exponent = out->m > 0.0f ? qgrad_unit_exponent(out->m, count) : 0;
    return 0;
}

// After the scatter: the accumulators to the caller's floats, or zeros when nothing was added; then the call's closing event.
int grad_resolve(prt_ctx * ctx, bool adds, float * g_positions, uint32_t position_count, int unit_exponent, hipStream_t stream) {
    const size_t np = 3 * (size_t)position_count;
    if (adds) {
        QGradArgs R;                                              // k_qgrad_resolve reads these four fields
        memset(&R, 0, sizeof(R));
        R.g_positions = g_positions; R.acc = ctx->tables.qg_acc.p; R.position_count = position_count; R.unit_exponent = unit_exponent;
        hipLaunchKernelGGL(k_qgrad_resolve, dim3((unsigned int)((np + 255) / 256)), dim3(256), 0, stream, R);
        HIP_TRY(ctx, hipGetLastError());
    } else if (g_positions && np) {
        HIP_TRY(ctx, hipMemsetAsync(g_positions, 0, np * sizeof(float), stream));
    }
    HIP_TRY(ctx, hipEventRecord(ctx->ev[1], stream));
    return 0;
}

int grad_fill_info(prt_ctx * ctx, const GradScan & scan, prt_grad_info * info) {
    if (!info) return 0;
    float ms = 0.0f;
    HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
    info->device_ms = ms;
    info->hit_rays = scan.words[QGRAD_W_HIT];
    info->skipped_rays = scan.words[QGRAD_W_SKIPPED];
    info->unit_exponent = scan.unit_exponent;
    info->max_contribution = scan.m;
    return 0;
}

// What a gradient call supplies to grad_backward: the caller's arguments, its argument struct filled from them, the description of
// its arrays for a call with host pointers, its kernels and when its scatter has something to do.
struct RayGrad {
    typedef QGradArgs Args;
    const prt_ray_batch * b;
    const int32_t * group;
    const uint32_t * vertex0;
    const float * positions;
    const prt_hit_grads * gout;
    const prt_query_grads * gin;
    static const char * required() { return "null origins, directions, group, vertex0 or positions"; }
    static const char * items() { return "rays"; }
    bool complete() const { return b->origins && b->directions && group && vertex0 && positions; }
    float * want_positions() const { return gin ? gin->positions : nullptr; }
    void fill(QGradArgs & A) const {
        A.origins = b->origins; A.dirs = b->directions; A.group = group; A.vertex0 = vertex0; A.positions = positions;
        if (gout) { A.g_t = gout->t; A.g_bw = gout->bw; A.g_pos = gout->position; A.g_nrm = gout->normal; }
        if (gin) { A.g_origins = gin->origins; A.g_dirs = gin->directions; A.g_positions = gin->positions; }
        A.ray_bias = b->ray_bias;
    }
    float ** g_positions(QGradArgs & A, float **) const { return &A.g_positions; }
    void stage(StageList & l, QGradArgs & A, float ** g_pos, size_t n, size_t np) const {
        l.in(&A.origins, 12 * n); l.in(&A.dirs, 12 * n); l.in(&A.group, 4 * n); l.in(&A.vertex0, 4 * n); l.in(&A.positions, 4 * np);
        l.in(&A.g_t, 4 * n); l.in(&A.g_bw, 12 * n); l.in(&A.g_pos, 12 * n); l.in(&A.g_nrm, 12 * n);
        l.out(&A.g_origins, 12 * n, A.g_origins != nullptr); l.out(&A.g_dirs, 12 * n, A.g_dirs != nullptr);
        l.out(g_pos, 4 * np, *g_pos != nullptr);
    }
    static bool scatter_writes(const QGradArgs & A) { return A.g_origins || A.g_dirs; }
    static void (*scan())(QGradArgs) { return k_qgrad_scan; }
    static void (*scatter(bool merge))(QGradArgs) { return merge ? k_qgrad_scatter<true> : k_qgrad_scatter<false>; }
};

struct PointGrad {
    typedef CGradArgs Args;
    const prt_point_batch * b;
    const int32_t * group;
    const uint32_t * vertex0;
    const float * positions;
    const prt_closest_grads * gout;
    const prt_point_grads * gin;
    static const char * required() { return "null points, group, vertex0 or positions"; }
    static const char * items() { return "points"; }
    bool complete() const { return b->points && group && vertex0 && positions; }
    float * want_positions() const { return gin ? gin->positions : nullptr; }
    void fill(CGradArgs & A) const {
        A.points = b->points; A.group = group; A.vertex0 = vertex0; A.positions = positions;
        if (gout) { A.g_dist2 = gout->dist2; A.g_point = gout->point; A.g_bw = gout->bw; }
        if (gin) A.g_points = gin->points;
    }
    float ** g_positions(CGradArgs &, float ** own) const { return own; }      // CGradArgs has none: k_qgrad_resolve gets it
    void stage(StageList & l, CGradArgs & A, float ** g_pos, size_t n, size_t np) const {
        l.in(&A.points, 12 * n); l.in(&A.group, 4 * n); l.in(&A.vertex0, 4 * n); l.in(&A.positions, 4 * np);
        l.in(&A.g_dist2, 4 * n); l.in(&A.g_point, 12 * n); l.in(&A.g_bw, 12 * n);
        l.out(&A.g_points, 12 * n, A.g_points != nullptr);
        l.out(g_pos, 4 * np, *g_pos != nullptr);
    }
    static bool scatter_writes(const CGradArgs & A) { return A.g_points != nullptr; }
    static void (*scan())(CGradArgs) { return k_cgrad_scan; }
    static void (*scatter(bool merge))(CGradArgs) { return merge ? k_cgrad_scatter<true> : k_cgrad_scatter<false>; }
};

// prt_trace_rays_backward, prt_closest_points_backward and their _device forms: `what` is the name in the error texts, `device`
// says where the caller's arrays live.  Nothing of the tree is read and nothing of the scene, the render stats or the counters is
// written.  The scan kernel validates every reference before the first write to an output of the caller's.
template <typename Grad>
int grad_backward(prt_ctx * ctx, const char * what, const Grad & q, uint32_t position_count, prt_grad_info * info, bool device) {
    if (!ctx) return -1;
    if (info) memset(info, 0, sizeof(*info));
    if (!q.b) { ctx->error = std::string(what) + ": null batch"; return -1; }
    if (q.b->count && !q.complete()) { ctx->error = std::string(what) + ": " + Grad::required(); return -1; }
    if (!ctx->has_scene) { ctx->error = std::string(what) + ": no scene uploaded"; return -2; }
    if (position_count != ctx->keep.position_count) { ctx->error = std::string(what) + ": position_count differs from the uploaded scene's"; return -1; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t stream = ctx->stream;
    const uint32_t count = q.b->count;
    const size_t n = count, np = 3 * (size_t)position_count;
    float * const want_p = q.want_positions();
    if (n == 0) {                                                 // nothing to add: the vertex gradient is zero
        if (want_p && np) {
            if (device) { HIP_TRY(ctx, hipMemsetAsync(want_p, 0, np * sizeof(float), stream)); HIP_TRY(ctx, hipStreamSynchronize(stream)); }
            else memset(want_p, 0, np * sizeof(float));
        }
        return 0;
    }
    if (const int rc = grad_prepare(ctx, what, np, want_p != nullptr)) return rc;
    typename Grad::Args A;
    memset(&A, 0, sizeof(A));
    q.fill(A);
    float * own_g_positions = want_p;
    float ** const g_positions = q.g_positions(A, &own_g_positions);
    StageList io;
    if (!device) {                                                // inputs, then the requested gradients, in one slab of 4-byte words
        q.stage(io, A, g_positions, n, np);
        HIP_TRY(ctx, io.carve(ctx->qg_io));
        if (io.upload(stream) != hipSuccess) { ctx->error = std::string(what) + ": copying the inputs to the device failed"; return -10; }
    }
    A.idx_positions = ctx->tables.qg_idx.p;
    A.group_runs = ctx->tables.qg_runs.p;
    A.words = ctx->qg_words.p;
    A.count = count; A.group_count = (unsigned int)ctx->keep.groups.size(); A.position_count = position_count;

    // ---- the references and the batch's largest contribution, before any output is written
    const unsigned int grid = grad_grid(ctx, count);
    HIP_TRY(ctx, hipEventRecord(ctx->ev[0], stream));
    HIP_TRY(ctx, hipMemsetAsync(A.words, 0, QGRAD_WORDS * sizeof(unsigned int), stream));
    hipLaunchKernelGGL(Grad::scan(), dim3(grid), dim3(256), 0, stream, A);
    GradScan scan;
    if (const int rc = grad_scan_verdict(ctx, what, Grad::items(), count, stream, &scan)) return rc;
    const bool adds = want_p && scan.words[QGRAD_W_HIT] && scan.m > 0.0f;   // else the vertex gradient is zero
    A.unit_exponent = scan.unit_exponent;
    A.acc = adds ? ctx->tables.qg_acc.p : nullptr;
    if (adds) HIP_TRY(ctx, hipMemsetAsync(A.acc, 0, np * sizeof(long long), stream));
    if (adds || Grad::scatter_writes(A)) {
        const bool merge = ctx->opt.qgrad_merge < 0 ? PRT_QGRAD_MERGE_DEFAULT != 0 : ctx->opt.qgrad_merge != 0;
        hipLaunchKernelGGL(Grad::scatter(merge), dim3(grid), dim3(256), 0, stream, A);
        HIP_TRY(ctx, hipGetLastError());
    }
    if (const int rc = grad_resolve(ctx, adds, *g_positions, position_count, A.unit_exponent, stream)) return rc;
    if (!device) HIP_TRY(ctx, io.download(stream));
    HIP_TRY(ctx, hipStreamSynchronize(stream));
    return grad_fill_info(ctx, scan, info);
}

// batch_pad's extent of a batch of rays on the host: the scene's, and the valid rays' biased origins (k_query_pad's rule;
// work[BATCH_W_EXTENT] stays 0).
float ray_batch_extent(const prt_ctx * ctx, const prt_ray_batch * batch) {
    float extent = ctx->desc.scene_abs_max;
    for (size_t i = 0; i < batch->count; ++i) {
        const f3 o = ld3(batch->origins + 3 * i), d = ld3(batch->directions + 3 * i), ob = o + d * batch->ray_bias;
        const bool ok = std::isfinite(o.x) && std::isfinite(o.y) && std::isfinite(o.z) && std::isfinite(d.x) && std::isfinite(d.y) &&
                        std::isfinite(d.z) && std::isfinite(ob.x) && std::isfinite(ob.y) && std::isfinite(ob.z);
        if (ok) extent = std::max(extent, std::max(std::max(fabsf(ob.x), fabsf(ob.y)), fabsf(ob.z)));
    }
    return extent;
}

// prt_trace_rays and prt_trace_rays_device after query_check: `device` says where the caller's arrays live.
int trace_rays(prt_ctx * ctx, int mode, const prt_ray_batch * batch, const prt_hit_buffers * hits, uint32_t flags, prt_counters * counters,
               bool device) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t n = batch->count;
    const unsigned int fields = query_fields(mode, hits);
    QueryArgs A;
    memset(&A, 0, sizeof(A));
    A.origins = batch->origins; A.dirs = batch->directions; A.tmax = mode == PRT_QUERY_OCCLUDED ? batch->tmax : nullptr;
    A.count = batch->count; A.ray_bias = batch->ray_bias;
    if (hits) {
        A.t = hits->t; A.bw = hits->bw; A.vertex0 = hits->vertex0; A.group = hits->group;
        A.position = hits->position; A.normal = hits->normal; A.occluded = hits->occluded;
    }
    A.pad_max = -1.0f;                                     // the origins' extent is reduced on the device (k_query_pad)
    const RayWalk walk = { mode };
    if (device) return run_batch(ctx, walk, A, fields, (flags & PRT_FLAG_COUNT_VISITS) != 0, counters);
    // device copies: origins, directions, tmax, then the requested fields (float-sized words; occluded in its own bytes)
    StageList io;
    io.in(&A.origins, 12 * n); io.in(&A.dirs, 12 * n); io.in(&A.tmax, 4 * n);
    io.out(&A.t, 4 * n, fields & QF_T); io.out(&A.bw, 12 * n, fields & QF_BW); io.out(&A.vertex0, 4 * n, fields & QF_VERTEX0);
    io.out(&A.group, 4 * n, fields & QF_GROUP); io.out(&A.position, 12 * n, fields & QF_POSITION); io.out(&A.normal, 12 * n, fields & QF_NORMAL);
    io.out(&A.occluded, n, fields & QF_OCCLUDED, false);
    HIP_TRY(ctx, io.carve(ctx->q_io));
    if (fields & QF_OCCLUDED) { HIP_TRY(ctx, ctx->q_occ.ensure(n)); A.occluded = ctx->q_occ.p; }
    A.pad_max = ray_batch_extent(ctx, batch);
    hipStream_t stream = ctx->stream;
    HIP_TRY(ctx, io.upload(stream));
    if (const int rc = run_batch(ctx, walk, A, fields, (flags & PRT_FLAG_COUNT_VISITS) != 0, counters)) return rc;
    HIP_TRY(ctx, io.download(stream));
    HIP_TRY(ctx, hipStreamSynchronize(stream));
    return 0;
}

// ---- K nearest hits (prt_trace_hits, kernels_hits.h) ----------------------------------------------------------------------------

unsigned int hits_fields(const prt_hits_buffers * o) {
    return (o->hit_count ? HITF_COUNT : 0) | (o->t ? HITF_T : 0) | (o->bw ? HITF_BW : 0) | (o->vertex0 ? HITF_VERTEX0 : 0) |
           (o->group ? HITF_GROUP : 0) | (o->back ? HITF_BACK : 0);
}

// The checks both entry points share; 1 = nothing to trace (count 0: counters zeroed), 0 = go on, < 0 = error.
int hits_check(prt_ctx * ctx, const prt_hits_request * q, const prt_hits_buffers * o, prt_counters * counters) {
    if (!ctx) return -1;
    if (!q || !o) { ctx->error = "prt_trace_hits: null request or buffers"; return -1; }
    if (q->rays.count && (!q->rays.origins || !q->rays.directions)) { ctx->error = "prt_trace_hits: null origins or directions"; return -1; }
    if (q->k < 1 || q->k > PRT_MAX_HITS) { ctx->error = "prt_trace_hits: k must be 1.." + std::to_string((int)PRT_MAX_HITS); return -1; }
    if (q->flags & ~(uint32_t)PRT_HITS_BACK_FACES) { ctx->error = "prt_trace_hits: unknown flag"; return -1; }
    const int given = (q->after_t ? 1 : 0) + (q->after_group ? 1 : 0) + (q->after_vertex0 ? 1 : 0);
    if (given != 0 && given != 3) { ctx->error = "prt_trace_hits: after_t, after_group and after_vertex0 must all be given, or none"; return -1; }
    if (!ctx->has_scene) { ctx->error = "prt_trace_hits: no scene uploaded"; return -2; }
    if (q->rays.count == 0) {
        if (counters) memset(counters, 0, sizeof(*counters));
        return 1;
    }
    return 0;
}

// prt_trace_hits and prt_trace_hits_device after hits_check: `device` says where the caller's arrays live.
int trace_hits(prt_ctx * ctx, const prt_hits_request * q, const prt_hits_buffers * o, uint32_t flags, prt_counters * counters, bool device) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t n = q->rays.count, slots = n * q->k;
    const unsigned int fields = hits_fields(o);
    HitsArgs A;
    memset(&A, 0, sizeof(A));
    A.origins = q->rays.origins; A.dirs = q->rays.directions; A.tmax = q->rays.tmax;
    A.count = q->rays.count; A.ray_bias = q->rays.ray_bias;
    A.k = q->k;
    A.after_t = q->after_t; A.after_group = q->after_group; A.after_vertex0 = q->after_vertex0;
    A.hit_count = o->hit_count; A.t = o->t; A.bw = o->bw; A.vertex0 = o->vertex0; A.group = o->group; A.back = o->back;
    A.pad_max = -1.0f;                                     // the origins' extent is reduced on the device (k_query_pad)
    const HitsWalk walk = { (q->flags & PRT_HITS_BACK_FACES) != 0 };
    if (device) return run_batch(ctx, walk, A, fields, (flags & PRT_FLAG_COUNT_VISITS) != 0, counters);
    // device copies: the rays, the cursor, then the requested fields (float-sized words; the back bytes last, rounded up)
    StageList io;
    io.in(&A.origins, 12 * n); io.in(&A.dirs, 12 * n); io.in(&A.tmax, 4 * n);
    io.in(&A.after_t, 4 * n); io.in(&A.after_group, 4 * n); io.in(&A.after_vertex0, 4 * n);
    io.out(&A.hit_count, 4 * n, fields & HITF_COUNT); io.out(&A.t, 4 * slots, fields & HITF_T); io.out(&A.bw, 12 * slots, fields & HITF_BW);
    io.out(&A.vertex0, 4 * slots, fields & HITF_VERTEX0); io.out(&A.group, 4 * slots, fields & HITF_GROUP);
    io.out(&A.back, slots, fields & HITF_BACK);
    HIP_TRY(ctx, io.carve(ctx->q_io));
    A.pad_max = ray_batch_extent(ctx, &q->rays);
    hipStream_t stream = ctx->stream;
    HIP_TRY(ctx, io.upload(stream));
    if (const int rc = run_batch(ctx, walk, A, fields, (flags & PRT_FLAG_COUNT_VISITS) != 0, counters)) return rc;
    HIP_TRY(ctx, io.download(stream));
    HIP_TRY(ctx, hipStreamSynchronize(stream));
    return 0;
}

// prt_closest_points, prt_signed_distance and their _device forms after closest_check: `o` holds the requested fields' pointers,
// `device` says where they and the batch's arrays live.
int closest_points(prt_ctx * ctx, const prt_point_batch * batch, const prt_signed_buffers & o, unsigned int fields, uint32_t flags,
                   prt_counters * counters, bool device) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t n = batch->count;
    ClosestArgs A;
    memset(&A, 0, sizeof(A));
    A.points = batch->points; A.max_dist2 = batch->max_dist2; A.count = batch->count;
    A.dist2 = o.closest.dist2; A.point = o.closest.point; A.bw = o.closest.bw; A.vertex0 = o.closest.vertex0; A.group = o.closest.group;
    A.signed_dist = o.signed_dist; A.feature = o.feature;
    A.pad_max = -1.0f;                                     // the points' extent is reduced on the device (k_closest_pad)
    if (device) return run_batch(ctx, PointWalk(), A, fields, (flags & PRT_FLAG_COUNT_VISITS) != 0, counters);
    // device copies: points, max_dist2, then the requested fields (float-sized words; the feature bytes last, rounded up)
    StageList io;
    io.in(&A.points, 12 * n); io.in(&A.max_dist2, 4 * n);
    io.out(&A.dist2, 4 * n, fields & CF_DIST2); io.out(&A.point, 12 * n, fields & CF_POINT); io.out(&A.bw, 12 * n, fields & CF_BW);
    io.out(&A.vertex0, 4 * n, fields & CF_VERTEX0); io.out(&A.group, 4 * n, fields & CF_GROUP); io.out(&A.signed_dist, 4 * n, fields & CF_SIGNED);
    io.out(&A.feature, n, fields & CF_FEATURE);
    HIP_TRY(ctx, io.carve(ctx->q_io));
    // batch_pad's extent from the finite points, on the host (k_closest_pad's rule; work[BATCH_W_EXTENT] stays 0)
    float extent = ctx->desc.scene_abs_max;
    for (size_t i = 0; i < n; ++i) {
        const f3 q = ld3(batch->points + 3 * i);
        if (std::isfinite(q.x) && std::isfinite(q.y) && std::isfinite(q.z)) extent = std::max(extent, std::max(std::max(fabsf(q.x), fabsf(q.y)), fabsf(q.z)));
    }
    A.pad_max = extent;
    hipStream_t stream = ctx->stream;
    HIP_TRY(ctx, io.upload(stream));
    if (const int rc = run_batch(ctx, PointWalk(), A, fields, (flags & PRT_FLAG_COUNT_VISITS) != 0, counters)) return rc;
    HIP_TRY(ctx, io.download(stream));
    HIP_TRY(ctx, hipStreamSynchronize(stream));
    return 0;
}

// ---- hemisphere visibility (prt_hemisphere_visibility, kernels_hemi.h) ----------------------------------------------------------

unsigned int hemi_fields(const prt_hemi_buffers * o) {
    return (o->unoccluded ? HF_UNOCCLUDED : 0) | (o->visibility ? HF_VISIBILITY : 0) | (o->bent ? HF_BENT : 0);
}

// What prt_hemisphere_visibility supplies to run_batch, one pass of whole points at a time.
struct HemiWalk {
    typedef HemiArgs Args;
    static const char * name() { return "prt_hemisphere_visibility"; }
    int prepare(prt_ctx * ctx, HemiArgs & A) const {
        A.replay_beyond = 64.0f * ctx->desc.scene_abs_max;
        A.scene_max = ctx->desc.scene_abs_max;
        HIP_TRY(ctx, ctx->q_hemi_flags.ensure(batch_items(A)));
        A.flags = ctx->q_hemi_flags.p;
        return 0;
    }
    int tables(prt_ctx *, HemiArgs &, unsigned int) const { return 0; }
    static void (*pad_kernel())(HemiArgs) { return k_hemi_pad; }
    // The walk on its persistent grid, the exact kernel for the items it set aside, then the reduction of the pass's flags.
    template <typename Fast, typename Exact>
    static int walk(prt_ctx * ctx, Fast fast, Exact exact, const HemiArgs & A, unsigned int fields) {
        constexpr int BLOCK = 256;
        const size_t lds = stack_dwords(A.stack_lds_entries, BLOCK) * sizeof(int);
        const TraceRule rule = trace_rule(ctx, fast, lds);
        const TraceGrid g = trace_grid(ctx, rule.per_cu, rule.chunk_min, (unsigned int)batch_items(A));
        hipLaunchKernelGGL(fast, dim3(g.grid), dim3(BLOCK), lds, ctx->stream, ctx->scene, A, rule.keep_min, rule.node_min, g.chunk, ctx->counters.p);
        HIP_TRY(ctx, hipGetLastError());
        hipLaunchKernelGGL(exact, dim3(64), dim3(256), 0, ctx->stream, ctx->scene, A, ctx->counters.p);      // A.exact_stack holds 64 * 256 columns
        HIP_TRY(ctx, hipGetLastError());
        const bool wave = A.samples >= (unsigned int)HEMI_WAVE_SAMPLES, bent = (fields & HF_BENT) != 0;
        const unsigned int cap = (unsigned int)std::max(1, ctx->cu_count) * 8u;
        const unsigned int want = wave ? (A.count + 3u) / 4u : (A.count + 255u) / 256u;
        const unsigned int grid = std::max(1u, std::min(want, cap));
        void (*reduce)(DevScene, HemiArgs, unsigned int, DevCounters *) =
            wave ? (bent ? k_hemi_reduce<true, true> : k_hemi_reduce<true, false>) : (bent ? k_hemi_reduce<false, true> : k_hemi_reduce<false, false>);
        hipLaunchKernelGGL(reduce, dim3(grid), dim3(256), 0, ctx->stream, ctx->scene, A, fields, ctx->counters.p);
        HIP_TRY(ctx, hipGetLastError());
        return 0;
    }
    int launch(prt_ctx * ctx, const HemiArgs & A, unsigned int fields, bool count) const {
        return count ? walk(ctx, k_hemi<256, true>, k_hemi_exact<true>, A, fields) : walk(ctx, k_hemi<256, false>, k_hemi_exact<false>, A, fields);
    }
    int verdict(prt_ctx *, const DevCounters &) const { return 0; }
};

// The checks both entry points share; 1 = nothing to do (count 0: counters zeroed), 0 = go on, < 0 = error.
int hemi_check(prt_ctx * ctx, const prt_hemi_batch * b, const prt_hemi_buffers * o, prt_counters * counters) {
    if (!ctx) return -1;
    if (!b || !o) { ctx->error = "prt_hemisphere_visibility: null batch or buffers"; return -1; }
    if (b->count && (!b->points || !b->normals)) { ctx->error = "prt_hemisphere_visibility: null points or normals"; return -1; }
    if (b->samples < 1 || b->samples > 65535) {
        ctx->error = "prt_hemisphere_visibility: samples must be in 1..65535 (prt_key.h packs the sample in 16 bits)";
        return -1;
    }
    if (b->first > (1ull << 32) || (unsigned long long)b->count > (1ull << 32) - b->first) {
        ctx->error = "prt_hemisphere_visibility: first + count exceeds 2^32 (the point index is the key's pixel word)";
        return -1;
    }
    if (!ctx->has_scene) { ctx->error = "prt_hemisphere_visibility: no scene uploaded"; return -2; }
    if (b->count == 0) {
        if (counters) memset(counters, 0, sizeof(*counters));
        return 1;
    }
    return 0;
}

// prt_hemisphere_visibility and prt_hemisphere_visibility_device after hemi_check: `device` says where the arrays live.  The call
// runs in passes of whole points (option HEMI_PASS_ITEMS items each at the most): the slow list and the flags are sized for a
// pass, whatever count x samples is.
int hemisphere_visibility(prt_ctx * ctx, const prt_hemi_batch * b, const prt_hemi_buffers * o, uint32_t flags, prt_counters * counters, bool device) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t n = b->count;
    const unsigned int fields = hemi_fields(o);
    HemiArgs A;
    memset(&A, 0, sizeof(A));
    A.points = b->points; A.normals = b->normals; A.max_dist = b->max_dist;
    A.samples = b->samples; A.seed = b->seed; A.ray_bias = b->ray_bias;
    A.unoccluded = o->unoccluded; A.visibility = o->visibility; A.bent = o->bent;
    A.pad_max = -1.0f;                                     // the points' extent is reduced on the device (k_hemi_pad)
    hipStream_t stream = ctx->stream;
    StageList io;
    if (!device) {
        io.in(&A.points, 12 * n); io.in(&A.normals, 12 * n); io.in(&A.max_dist, 4 * n);
        io.out(&A.unoccluded, 4 * n, fields & HF_UNOCCLUDED); io.out(&A.visibility, 4 * n, fields & HF_VISIBILITY); io.out(&A.bent, 12 * n, fields & HF_BENT);
        HIP_TRY(ctx, io.carve(ctx->q_io));
        // batch_pad's extent from the valid points, on the host (k_hemi_pad's rule and hemi_pad's sum; work[BATCH_W_EXTENT] stays 0)
        float extent = 0.0f;
        for (size_t i = 0; i < n; ++i) {
            const f3 p = ld3(b->points + 3 * i), nr = ld3(b->normals + 3 * i);
            if (hemi_point_valid(p, nr)) extent = std::max(extent, std::max(std::max(fabsf(p.x), fabsf(p.y)), fabsf(p.z)));
        }
        A.pad_max = std::max(ctx->desc.scene_abs_max, extent + fabsf(b->ray_bias));
        if (!(A.pad_max >= 0.0f)) A.pad_max = ctx->desc.scene_abs_max;          // a NaN bias: every ray is a miss by definition
        HIP_TRY(ctx, io.upload(stream));
    }
    const long long want_items = ctx->opt.hemi_pass_items >= 0 ? ctx->opt.hemi_pass_items : (1ll << 24);
    const size_t pass_points = hemi_pass_points((unsigned long long)want_items, b->samples);
    prt_counters total;
    memset(&total, 0, sizeof(total));
    for (size_t at = 0; at < n; at += pass_points) {
        HemiArgs P = A;
        P.points += 3 * at; P.normals += 3 * at;
        if (P.max_dist) P.max_dist += at;
        if (P.unoccluded) P.unoccluded += at;
        if (P.visibility) P.visibility += at;
        if (P.bent) P.bent += 3 * at;
        P.count = (unsigned int)std::min(pass_points, n - at);
        P.first = (unsigned int)(b->first + at);
        prt_counters c;
        if (const int rc = run_batch(ctx, HemiWalk(), P, fields, (flags & PRT_FLAG_COUNT_VISITS) != 0, &c)) return rc;
        total.ray_count += ctx->host_counters->ray_count;                   // k_hemi_reduce: the pass's valid points x samples
        total.node_visits += c.node_visits;
        total.tri_tests += c.tri_tests;
        total.render_ms += c.render_ms;
        total.trace_kernel_ms += c.trace_kernel_ms;
        total.trace_kernel_launches += 3;
    }
    if (!device) {
        HIP_TRY(ctx, io.download(stream));
        HIP_TRY(ctx, hipStreamSynchronize(stream));
    }
    if (counters) *counters = total;
    return 0;
}

// ---- radiance along the caller's rays (prt_render_rays, kernels_rays.h) -----------------------------------------------------------

// The checks both entry points share; 1 = nothing to do (count 0: counters zeroed), 0 = go on, < 0 = error.
int rays_check(prt_ctx * ctx, const prt_radiance_batch * b, const prt_params * params, const void * out, prt_counters * counters) {
    if (!ctx) return -1;
    if (!b || !params) { ctx->error = "prt_render_rays: null batch or params"; return -1; }
    if (b->count && (!b->origins || !b->directions || !out)) { ctx->error = "prt_render_rays: null origins, directions or output"; return -1; }
    if (b->flags & ~(uint32_t)PRT_RAYS_CAMERA_STREAM) { ctx->error = "prt_render_rays: unknown flag"; return -1; }
    if (params->spp == 0 || params->spp > 65535) { ctx->error = "prt_render_rays: spp must be in 1..65535 (prt_key.h packs the sample in 16 bits)"; return -1; }
    if (params->bounce_depth > 16) { ctx->error = "prt_render_rays: bounce_depth > 16 not supported"; return -1; }
    if (b->first > (1ull << 32) || (unsigned long long)b->count > (1ull << 32) - b->first) {
        ctx->error = "prt_render_rays: first + count exceeds 2^32 (the output index is the key's pixel word)";
        return -1;
    }
    if (params->max_spp > params->spp) { ctx->error = "prt_render_rays: adaptive sampling (max_spp > spp) is not supported for caller rays"; return -1; }
    const unsigned int pipeline = params->pipeline & PRT_PIPELINE_MASK;
    if (pipeline != PRT_PIPELINE_DEFAULT && pipeline != PRT_PIPELINE_WAVEFRONT) {
        ctx->error = "prt_render_rays: runs on PRT_PIPELINE_WAVEFRONT (or DEFAULT) only";
        return -1;
    }
    if (!ctx->has_scene) { ctx->error = "prt_render_rays: no scene uploaded"; return -2; }
    if (b->count == 0) {
        if (counters) memset(counters, 0, sizeof(*counters));
        return 1;
    }
    return 0;
}

// prt_render_rays and prt_render_rays_device after rays_check: `device` says where the arrays live.  The domain check comes before
// anything is rendered or written; the render itself is render_pixels_once with the rays in the camera's place.
int render_rays(prt_ctx * ctx, const prt_radiance_batch * b, const prt_params * params, float4 * out, prt_counters * counters, bool device) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t stream = ctx->stream;
    const size_t n = b->count;
    const unsigned long long n_rays = (unsigned long long)n * params->spp;
    RaySource src;
    memset(&src, 0, sizeof(src));
    RaysArgs & A = src.A;
    A.origins = b->origins; A.directions = b->directions;
    A.n_rays = n_rays;
    A.ray_bias = params->ray_bias;
    A.origin_max = 64.0f * ctx->desc.scene_abs_max;
    A.first = (unsigned int)b->first;
    A.camera_stream = (b->flags & PRT_RAYS_CAMERA_STREAM) ? 1u : 0u;
    StageList io;
    if (!device) {
        io.out(&out, 16 * n, true);                        // first in the slab: k_resolve stores float4
        io.in(&A.origins, 12 * (size_t)n_rays); io.in(&A.directions, 12 * (size_t)n_rays);
        HIP_TRY(ctx, io.carve(ctx->q_io));
        HIP_TRY(ctx, io.upload(stream));
    }
    HIP_TRY(ctx, ctx->rays_words.ensure(RAYS_WORDS));
    A.words = ctx->rays_words.p;

    // ---- the domain, before anything is rendered
    HIP_TRY(ctx, hipEventRecord(ctx->ev[2], stream));
    HIP_TRY(ctx, hipMemsetAsync(A.words, 0, RAYS_W_FIRST * sizeof(unsigned long long), stream));
    HIP_TRY(ctx, hipMemsetAsync(A.words + RAYS_W_FIRST, 0xFF, sizeof(unsigned long long), stream));
    {
        const unsigned long long want = (n_rays + 255ull) / 256ull;
        const unsigned int grid = (unsigned int)std::max(1ull, std::min(want, (unsigned long long)std::max(1, ctx->cu_count) * 8ull));
        hipLaunchKernelGGL(k_rays_check, dim3(grid), dim3(256), 0, stream, A);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipEventRecord(ctx->ev[3], stream));
    unsigned long long words[RAYS_WORDS] = { 0ull, 0ull, 0ull };
    HIP_TRY(ctx, hipMemcpyAsync(words, A.words, sizeof(words), hipMemcpyDeviceToHost, stream));
    HIP_TRY(ctx, hipStreamSynchronize(stream));
    if (words[RAYS_W_OUTSIDE]) {
        char msg[256];
        snprintf(msg, sizeof(msg), "prt_render_rays: %llu of %llu rays lie outside the domain (a component that is not finite, a direction that is not "
                 "unit length, an origin beyond 64 x the scene's extent); the first is ray %llu", words[RAYS_W_OUTSIDE], n_rays, words[RAYS_W_FIRST]);
        ctx->error = msg;
        return -1;
    }
    float check_ms = 0.0f;
    HIP_TRY(ctx, hipEventElapsedTime(&check_ms, ctx->ev[2], ctx->ev[3]));
    const unsigned int extent_bits = (unsigned int)words[RAYS_W_EXTENT];
    memcpy(&src.origin_abs_max, &extent_bits, 4);

    prt_params pp = *params;
    pp.pipeline = PRT_PIPELINE_WAVEFRONT | (params->pipeline & PRT_FLAG_COUNT_VISITS);
    const PixelSet px = { b->count, (uint32_t)b->first, 1, 0, 1, nullptr };
    bool park_overflow = false;            // the pool pipeline's
    if (const int rc = render_pixels_once(ctx, nullptr, &pp, 1, 1, px, out, counters, &park_overflow, &src)) return rc;
    if (counters) counters->render_ms += check_ms;
    if (!device) {
        HIP_TRY(ctx, io.download(stream));
        HIP_TRY(ctx, hipStreamSynchronize(stream));
    }
    return 0;
}

// ---- surface samples (prt_sample_surface, kernels_sample.h) ------------------------------------------------------------------------

unsigned int sample_fields(const prt_sample_buffers * o) {
    return (o->point ? SF_POINT : 0) | (o->bw ? SF_BW : 0) | (o->normal ? SF_NORMAL : 0) | (o->vertex0 ? SF_VERTEX0 : 0) | (o->group ? SF_GROUP : 0);
}

// The tables of prt_sample_surface into T: the input -> slot table once per upload, the prefix sums once per geometry generation
// (four launches on the context's stream, between ev[2] and ev[3]; their control words travel to sm_read_words behind them, valid
// after the caller's synchronisation).  *rebuilt says whether they ran.
int ensure_sample_table(prt_ctx * ctx, SampleTable & T, bool * rebuilt) {
    const uint32_t n_tris = ctx->scene.tri_count;
    *rebuilt = false;
    if (ctx->keep.tri_order.size() != n_tris) { ctx->error = "prt_sample_surface: the scene's leaf order is not available"; return -2; }
    if (!ctx->tables.sm_slot_of_input.p) {
        std::vector<unsigned int> slot_of_input;
        if (!keep_slot_of_input(ctx->keep, &slot_of_input)) { ctx->error = "prt_sample_surface: the scene's leaf order is not a permutation"; return -2; }
        hipError_t e = ctx->tables.sm_slot_of_input.upload(slot_of_input);
        if (e == hipSuccess) e = hipDeviceSynchronize();          // the upload went through the null stream
        if (e != hipSuccess) {
            ctx->tables.sm_slot_of_input.release();
            ctx->error = std::string("prt_sample_surface: table upload: ") + hipGetErrorString(e);
            return -10;
        }
        ctx->tables.sm_generation = 0;
    }
    const unsigned int n_tiles = (n_tris + (unsigned int)SAMPLE_TILE - 1u) / (unsigned int)SAMPLE_TILE;
    HIP_TRY(ctx, ctx->tables.sm_weight.ensure(n_tris));
    HIP_TRY(ctx, ctx->tables.sm_prefix.ensure(n_tris));
    HIP_TRY(ctx, ctx->tables.sm_tile_sum.ensure(n_tiles));
    HIP_TRY(ctx, ctx->sm_words.ensure(SAMPLE_WORDS));
    T.tris = ctx->arrays.tris.p;
    T.slot_of_input = ctx->tables.sm_slot_of_input.p;
    T.weight = ctx->tables.sm_weight.p;
    T.C = ctx->tables.sm_prefix.p;
    T.tile_sum = ctx->tables.sm_tile_sum.p;
    T.words = ctx->sm_words.p;
    T.n_tris = n_tris;
    T.n_tiles = n_tiles;
    if (ctx->tables.sm_generation == ctx->geom_generation) return 0;
    hipStream_t stream = ctx->stream;
    HIP_TRY(ctx, hipEventRecord(ctx->ev[2], stream));
    HIP_TRY(ctx, hipMemsetAsync(T.words, 0, SAMPLE_WORDS * sizeof(unsigned long long), stream));
    if (n_tris) {
        const unsigned int cap = (unsigned int)std::max(1, ctx->cu_count) * 8u;
        const unsigned int lanes_grid = std::max(1u, std::min(n_tiles, cap));
        hipLaunchKernelGGL(k_sample_weights, dim3(lanes_grid), dim3(256), 0, stream, T);
        HIP_TRY(ctx, hipGetLastError());
        hipLaunchKernelGGL(k_sample_tiles, dim3(lanes_grid), dim3(SAMPLE_TILE), 0, stream, T);
        HIP_TRY(ctx, hipGetLastError());
        hipLaunchKernelGGL(k_sample_totals, dim3(1), dim3(SAMPLE_TILE), 0, stream, T);
        HIP_TRY(ctx, hipGetLastError());
        hipLaunchKernelGGL(k_sample_offsets, dim3(lanes_grid), dim3(256), 0, stream, T);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipEventRecord(ctx->ev[3], stream));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->sm_read_words, T.words, SAMPLE_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    *rebuilt = true;
    return 0;
}

// prt_sample_surface and prt_sample_surface_device: `device` says where the buffers live.
int sample_surface(prt_ctx * ctx, const prt_sample_request * rq, const prt_sample_buffers * out, prt_sample_info * info, bool device) {
    if (!ctx) return -1;
    if (info) memset(info, 0, sizeof(*info));
    if (!rq || !out) { ctx->error = "prt_sample_surface: null request or buffers"; return -1; }
    if (rq->first > (1ull << 48) || (unsigned long long)rq->count > (1ull << 48) - rq->first) {
        ctx->error = "prt_sample_surface: first + count exceeds 2^48 (the sample index is the key's packed word)";
        return -1;
    }
    if (!ctx->has_scene) { ctx->error = "prt_sample_surface: no scene uploaded"; return -2; }
    if (rq->count == 0) return 0;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (const int rc = ensure_leaf_map(ctx, "prt_sample_surface")) return rc;
    hipStream_t stream = ctx->stream;
    const size_t n = rq->count;
    const unsigned int fields = sample_fields(out);
    SampleArgs A;
    memset(&A, 0, sizeof(A));
    A.seed = rq->seed; A.first = rq->first; A.count = rq->count;
    A.point = out->point; A.bw = out->bw; A.normal = out->normal; A.vertex0 = out->vertex0; A.group = out->group;
    StageList io;
    if (!device) {
        io.out(&A.point, 12 * n, fields & SF_POINT); io.out(&A.bw, 12 * n, fields & SF_BW); io.out(&A.normal, 12 * n, fields & SF_NORMAL);
        io.out(&A.vertex0, 4 * n, fields & SF_VERTEX0); io.out(&A.group, 4 * n, fields & SF_GROUP);
        HIP_TRY(ctx, io.carve(ctx->q_io));
    }
    HIP_TRY(ctx, hipEventRecord(ctx->ev[0], stream));
    SampleTable T;
    memset(&T, 0, sizeof(T));
    bool rebuilt = false;
    if (const int rc = ensure_sample_table(ctx, T, &rebuilt)) return rc;
    hipLaunchKernelGGL(k_sample, dim3(grad_grid(ctx, rq->count)), dim3(256), 0, stream, T, A, ctx->tables.q_leaf_map.p, fields);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(ctx->ev[1], stream));
    if (!device) HIP_TRY(ctx, io.download(stream));
    HIP_TRY(ctx, hipStreamSynchronize(stream));
    if (rebuilt) {
        memcpy(ctx->sm_host_words, ctx->sm_read_words, sizeof(ctx->sm_host_words));
        ctx->tables.sm_generation = ctx->geom_generation;
    }
    if (info) {
        float ms = 0.0f, tms = 0.0f;
        HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
        if (rebuilt) HIP_TRY(ctx, hipEventElapsedTime(&tms, ctx->ev[2], ctx->ev[3]));
        info->device_ms = ms;
        info->table_ms = tms;
        info->total_weight = ctx->sm_host_words[SAMPLE_W_TOTAL];
        info->unit_exponent = sample_unit_exponent(ctx->sm_host_words[SAMPLE_W_MAX], ctx->scene.tri_count);
        info->live_triangles = (uint32_t)ctx->sm_host_words[SAMPLE_W_LIVE];
        info->area = 0.5 * (double)info->total_weight * qgrad_pow2(info->unit_exponent);
    }
    return 0;
}

// What prt_sample_surface_backward supplies to grad_backward (RayGrad, PointGrad).
struct SampleGrad {
    typedef SGradArgs Args;
    struct Batch { uint32_t count; };
    Batch batch;
    const Batch * b;
    const int32_t * group;
    const uint32_t * vertex0;
    const float * bw;
    const float * positions;
    const prt_sample_grads * gout;
    float * gin_positions;
    static const char * required() { return "null group, vertex0, bw or positions"; }
    static const char * items() { return "samples"; }
    bool complete() const { return group && vertex0 && bw && positions; }
    float * want_positions() const { return gin_positions; }
    void fill(SGradArgs & A) const {
        A.group = group; A.vertex0 = vertex0; A.bw = bw; A.positions = positions;
        if (gout) { A.g_point = gout->point; A.g_normal = gout->normal; }
    }
    float ** g_positions(SGradArgs &, float ** own) const { return own; }      // SGradArgs has none: k_qgrad_resolve gets it
    void stage(StageList & l, SGradArgs & A, float ** g_pos, size_t n, size_t np) const {
        l.in(&A.group, 4 * n); l.in(&A.vertex0, 4 * n); l.in(&A.bw, 12 * n); l.in(&A.positions, 4 * np);
        l.in(&A.g_point, 12 * n); l.in(&A.g_normal, 12 * n);
        l.out(g_pos, 4 * np, *g_pos != nullptr);
    }
    static bool scatter_writes(const SGradArgs &) { return false; }            // no per-sample gradient: the draws have no inputs
    static void (*scan())(SGradArgs) { return k_sgrad_scan; }
    static void (*scatter(bool merge))(SGradArgs) { return merge ? k_sgrad_scatter<true> : k_sgrad_scatter<false>; }
};

int sample_surface_backward(prt_ctx * ctx, uint32_t count, const int32_t * group, const uint32_t * vertex0, const float * bw, const float * positions,
                            uint32_t position_count, const prt_sample_grads * gout, float * gin_positions, prt_grad_info * info, bool device) {
    SampleGrad q = { { count }, nullptr, group, vertex0, bw, positions, gout, gin_positions };
    q.b = &q.batch;
    return grad_backward(ctx, "prt_sample_surface_backward", q, position_count, info, device);
}

}  // namespace

extern "C" {

int prt_abi_version(void) { return PRT_ABI_VERSION; }

int prt_build_flags(void) {
    int f = 0;                            // (PRT_BUILD_EXPERIMENTAL is never set: include/prt.h)
#if !defined(PRT_BVH8)
    f |= PRT_BUILD_BVH4;
#endif
    return f;
}

const char * prt_last_error(const prt_ctx * ctx) { return ctx ? ctx->error.c_str() : g_create_error.c_str(); }

prt_ctx * prt_create(int device_id) {
    PRT_API_TRY
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        g_create_error = std::string("prt_create: no HIP device available (") + hipGetErrorString(e) + ")";
        return nullptr;
    }
    if (device_id < 0 || device_id >= n) {
        g_create_error = "prt_create: device ordinal out of range";
        return nullptr;
    }
    if ((e = hipSetDevice(device_id)) != hipSuccess) {
        g_create_error = std::string("prt_create: hipSetDevice: ") + hipGetErrorString(e);
        return nullptr;
    }
    prt_ctx * ctx = new prt_ctx;
    ctx->device = device_id;
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device_id) == hipSuccess) ctx->cu_count = prop.multiProcessorCount;
        if (ctx->cu_count <= 0) ctx->cu_count = 256;
    }
    memset(&ctx->scene, 0, sizeof(ctx->scene));
    memset(&ctx->desc.info, 0, sizeof(ctx->desc.info));
    memset(&ctx->last_stats, 0, sizeof(ctx->last_stats));
    prt_options_from_env(ctx->opt);       // the environment is read here and nowhere else
    // PRT_RESERVE_CUS=k (multi-GPU callers): the context's streams are created with a CU mask that leaves k compute units to
    // others - the RCCL gather of the previous frame must not wait for a wave slot while this context's persistent kernels
    // hold every one of theirs (bench.py sets it for N > 1 with frames in flight).  The persistent grids are sized for the
    // CUs that are left.  WHICH k matters: the mask's bits are XCD-major (32 per XCD), workgroups go round the XCDs, so
    // clearing the last 8 bits takes a quarter of ONE XCD and leaves 35 of the grid's blocks without a slot there (C4 frame
    // +7.5 %); every 32nd bit takes one CU of each XCD (+4.2 % for 3.1 % of the CUs).  Measured: profiles/r03_cu_mask.txt.
    // A CU-masked stream is a BLOCKING stream (ordered against the null stream): callers keep their own work off the null
    // stream (bench.py does; the same file shows what happens otherwise).
    std::vector<uint32_t> cu_mask;
    {
        const int reserve = (int)ctx->opt.reserve_cus;
        if (reserve > 0 && reserve < ctx->cu_count) {
            cu_mask.assign((size_t)(ctx->cu_count + 31) / 32, 0u);
            const int pattern = (int)ctx->opt.reserve_pattern, stride = ctx->cu_count / reserve;
            int kept = 0;
            for (int cu = 0; cu < ctx->cu_count; ++cu) {
                const bool off = pattern == 1 ? cu < reserve
                               : pattern == 2 ? (cu % stride == stride - 1 && cu / stride < reserve)
                               : pattern == 3 ? false
                               : cu >= ctx->cu_count - reserve;
                if (!off) { cu_mask[(size_t)cu >> 5] |= 1u << (cu & 31); ++kept; }
            }
            ctx->reserved_cus = ctx->cu_count - kept;
            ctx->cu_count = kept;
        }
    }
    auto make_stream = [&](hipStream_t * st) -> hipError_t {
        if (!cu_mask.empty()) return hipExtStreamCreateWithCUMask(st, (uint32_t)cu_mask.size(), cu_mask.data());
        return hipStreamCreateWithFlags(st, hipStreamNonBlocking);
    };
    e = make_stream(&ctx->stream);
    for (int i = 0; i < 4 && e == hipSuccess; ++i) e = hipEventCreate(&ctx->ev[i]);
    ctx->chain[0].stream = ctx->stream;
    if (ctx->opt.pool_park_cap >= 0) ctx->pool_park_cap = ctx->pool_spark_cap = (size_t)std::max(1ll, ctx->opt.pool_park_cap);   // tests: start tiny, grow
    if (e == hipSuccess) e = ctx->counters.ensure(1);          // DevScene::near_tie_unresolved points into it
    if (e == hipSuccess) e = hipHostMalloc((void **)&ctx->host_counters, sizeof(DevCounters), hipHostMallocDefault);
    for (int c = 1; c < PRT_MAX_CHAINS && e == hipSuccess; ++c) e = make_stream(&ctx->chain[c].stream);
    for (int c = 0; c < PRT_MAX_CHAINS && e == hipSuccess; ++c) {
        prt_ctx::ChainWs & w = ctx->chain[c];
        e = hipEventCreate(&w.ev_t0);
        if (e == hipSuccess) e = hipEventCreate(&w.ev_t1);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&w.ev_done, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&w.ev_first, hipEventDisableTiming);
        if (e == hipSuccess) e = hipHostMalloc((void **)&w.host_counts, 64, hipHostMallocDefault);
    }
    if (e != hipSuccess) {
        g_create_error = std::string("prt_create: stream/event creation: ") + hipGetErrorString(e);
        prt_destroy(ctx);                  // releases whatever was created before the failure (every handle starts out null)
        return nullptr;
    }
    return ctx;
    PRT_API_CATCH_PTR("prt_create")
}

void prt_destroy(prt_ctx * ctx) {
    PRT_API_TRY
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    ctx->arrays.release(); ctx->tables.release(); ctx->spec_dirs.release();
    ctx->sample_rgb.release(); ctx->frame_out.release(); ctx->counters.release(); ctx->ring_ws.release(); ctx->pixel_list.release(); ctx->wf_counts.release(); ctx->stack_spill.release(); ctx->pool_f4.release(); ctx->pool_park.release(); ctx->pool_fin.release(); ctx->pool_args.release(); ctx->adapt_f4.release(); ctx->wave_times.release();
    ctx->q_work.release(); ctx->q_slow.release(); ctx->q_exact_stack.release(); ctx->q_hits_lists.release(); ctx->q_io.release(); ctx->q_occ.release(); ctx->q_hemi_flags.release(); ctx->rays_words.release();
    ctx->rf_boxes.release(); ctx->rf_bounds.release(); ctx->rf_in.release();
    ctx->qg_words.release(); ctx->qg_io.release();
    ctx->sm_words.release();
    for (int c = 0; c < PRT_MAX_CHAINS; ++c) {
        prt_ctx::ChainWs & w = ctx->chain[c];
        w.f4.release(); w.rng.release(); w.counts.release(); w.overflow.release(); w.slow_stack.release();
        if (w.ev_t0) (void)hipEventDestroy(w.ev_t0);
        if (w.ev_t1) (void)hipEventDestroy(w.ev_t1);
        if (w.ev_done) (void)hipEventDestroy(w.ev_done);
        if (w.ev_first) (void)hipEventDestroy(w.ev_first);
        if (w.host_counts) (void)hipHostFree(w.host_counts);
        if (c >= 1 && w.stream) (void)hipStreamDestroy(w.stream);
    }
    for (int i = 0; i < 4; ++i) if (ctx->ev[i]) (void)hipEventDestroy(ctx->ev[i]);
    if (ctx->host_counters) (void)hipHostFree(ctx->host_counters);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
    PRT_API_CATCH_VOID
}

int prt_set_option(prt_ctx * ctx, const char * name, const char * value) {
    PRT_API_TRY
    if (!ctx || !name) return -1;
    const char * bare = !strncasecmp(name, "PRT_", 4) ? name + 4 : name;
    if (!strcasecmp(bare, "RESERVE_CUS")) { ctx->error = "prt_set_option: RESERVE_CUS shapes the context's streams and is read at creation only (environment PRT_RESERVE_CUS)"; return -1; }
    if (prt_option_set(ctx->opt, bare, value)) { ctx->error = std::string("prt_set_option: unknown option or bad value: ") + name; return -1; }
    ctx->opt.bvh.debug = ctx->opt.debug_util;
    if (!strcasecmp(bare, "POOL_PARK_CAP")) {
        ctx->pool_park_cap = ctx->pool_spark_cap = ctx->opt.pool_park_cap >= 0 ? (size_t)std::max(1ll, ctx->opt.pool_park_cap) : (size_t)1 << 18;
    }
    ctx->tuned.clear();                 // a knob may change which pipeline wins the try-out
    return 0;
    PRT_API_CATCH_RC(ctx, "prt_set_option")
}

int prt_get_render_stats(const prt_ctx * ctx, prt_render_stats * stats) {
    PRT_API_TRY
    if (!ctx || !stats) return -1;
    *stats = ctx->last_stats;
    return 0;
    PRT_API_CATCH_RC(nullptr, "prt_get_render_stats")
}

int prt_get_region_stats(const prt_ctx * ctx, uint64_t * out, uint32_t n) {
    PRT_API_TRY
    if (!ctx || (!out && n)) return -1;
    for (uint32_t k = 0; k < n && k < 2u * PRT_REGION_COUNT; ++k) out[k] = ctx->last_regions[k];
    return 2 * PRT_REGION_COUNT;
    PRT_API_CATCH_RC(nullptr, "prt_get_region_stats")
}

int prt_upload_scene(prt_ctx * ctx, const prt_scene_desc * s) {
    PRT_API_TRY
    if (!ctx) return -1;
    int rc = check_scene_desc(s, &ctx->error);                 // scene_pack.cpp, like everything below that needs no device
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    // The old scene goes here; the new one arrives in ONE step at the end, when all of it lies on the device.  Until then the
    // context holds nothing of it: a failed upload leaves it describing no scene, never half of one.
    ctx->tables.release();
    ctx->keep = SceneKeep();
    ctx->has_scene = false;

    // ---- BVH over un-indexed triangles
    auto t0 = std::chrono::steady_clock::now();
    const uint32_t n_tris = s->index_count / 3;
    std::vector<float> verts;
    if ((rc = unindex_scene(s, &verts, &ctx->error))) return rc;
    BvhWide bvh;
    ScenePackOptions how;
    how.threads = std::min(std::max(1u, std::thread::hardware_concurrency()), 16u);
    how.leaf_max = BVH_LEAF_MAX;
    if (ctx->opt.leaf_max >= 0) how.leaf_max = (unsigned int)std::max(1ll, std::min(4ll, ctx->opt.leaf_max));   // experiment knob
    how.sah_trav_cost = (float)ctx->opt.sah_trav_cost;                                                          // experiment knob
    how.shadow_tree_ratio = (uint32_t)std::max(0ll, std::min(100ll, ctx->opt.shadow_tree_ratio));
    how.normal_cones = ctx->opt.normal_cones != 0;
    how.bvh = &ctx->opt.bvh;
    if (ctx->opt.bvh_builder_lbvh) {
        // fast build for scenes that change every frame: radix tree on the GPU (bvh_lbvh.h), same quantised wide back end
        if ((rc = build_bvh_lbvh(ctx, verts.data(), n_tris, how.leaf_max, &bvh))) return rc;
    } else {
        build_bvh_wide(BVH_WIDTH, verts.data(), n_tris, how.leaf_max, how.threads, &bvh, how.sah_trav_cost, how.bvh);
    }
    const double build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    // every address the traversal kernels will form from the tree is checked on the host before the tree is uploaded (bvh_check.cpp)
    if (const char * bad = validate_bvh_links(bvh, n_tris)) { ctx->error = std::string("prt_upload_scene: the builder produced a broken tree - ") + bad; return -9; }

    // ---- every array and what describes it, on the host (the shadow trees are built and checked in there)
    PackedScene packed;
    if ((rc = pack_scene(s, verts, std::move(bvh), how, &packed, &ctx->error))) return rc;
    packed.desc.info.bvh_build_ms = build_ms;

    // ---- onto the device
    HIP_TRY(ctx, ctx->arrays.upload(packed));
    DevScene & sc = ctx->scene;
    ctx->arrays.point(sc, packed.desc.textured, packed.keep.bumped, !packed.ref_spheres.empty());
    sc.light_count = packed.light_count;
    sc.material_count = packed.material_count;
    sc.tri_count = n_tris;
    sc.node_count = packed.desc.info.bvh_node_count;
    sc.tie_widen_max = 8;                                     // render_pixels_once sets the option's value per call
    sc.near_tie_unresolved = &ctx->counters.p->near_tie_unresolved;
    if ((rc = build_spec_table(ctx, packed.desc.material_ns, 1))) return rc;
    HIP_TRY(ctx, hipDeviceSynchronize());      // uploads went through the null stream; renders use the context's non-blocking streams

    // ---- the commit: only now does the context describe the new scene
    ctx->desc = std::move(packed.desc);
    ctx->keep = std::move(packed.keep);
    ctx->has_scene = true;
    ctx->scene_epoch++;
    ctx->geom_generation++;
    ctx->tuned.clear();
    return 0;
    PRT_API_CATCH_RC(ctx, "prt_upload_scene")
}

int prt_get_scene_info(const prt_ctx * ctx, prt_scene_info * info) {
    PRT_API_TRY
    if (!ctx || !info) return -1;
    if (!ctx->has_scene) return -2;
    *info = ctx->desc.info;
    return 0;
    PRT_API_CATCH_RC(nullptr, "prt_get_scene_info")
}

int prt_get_shadow_trees(const prt_ctx * ctx, prt_shadow_tree_info * out, uint32_t cap) {
    PRT_API_TRY
    if (!ctx || (!out && cap)) return -1;
    if (!ctx->has_scene) return -2;
    for (size_t l = 0; l < ctx->desc.shadow_info.size() && l < cap; ++l) out[l] = ctx->desc.shadow_info[l];
    return (int)ctx->desc.shadow_info.size();
    PRT_API_CATCH_RC(nullptr, "prt_get_shadow_trees")
}

int prt_get_normal_cones(const prt_ctx * ctx, prt_normal_cone_info * out) {
    PRT_API_TRY
    if (!ctx || !out) return -1;
    if (!ctx->has_scene) return -2;
    *out = ctx->desc.cone_info;
    return 0;
    PRT_API_CATCH_RC(nullptr, "prt_get_normal_cones")
}

static_assert((float)ShadowOpenBounds::min_cos == PRT_SHADOW_OPEN_MIN_COS, "the margins assume the kernels' grazing threshold");
int prt_get_shadow_open(const prt_ctx * ctx, prt_shadow_open_info * out, uint32_t cap) {
    PRT_API_TRY
    if (!ctx) return -1;
    if (!ctx->has_scene) return -2;
    for (uint32_t l = 0; l < cap && l < ctx->desc.shadow_open_info.size() && out; ++l) out[l] = ctx->desc.shadow_open_info[l];
    return (int)ctx->desc.shadow_open_info.size();
    PRT_API_CATCH_RC(nullptr, "prt_get_shadow_open")
}

int prt_render_device(prt_ctx * ctx, const prt_camera * cam, const prt_params * params, uint32_t width, uint32_t height,
                      uint32_t start_idx, uint32_t end_idx, void * d_rgba_out, prt_counters * counters) {
    PRT_API_TRY
    if (!ctx) return -1;
    if ((!d_rgba_out && end_idx != start_idx) || end_idx < start_idx || (uint64_t)end_idx > (uint64_t)width * height) {
        ctx->error = "prt_render: bad output pointer or pixel range";
        return -1;
    }
    PixelSet px = { end_idx - start_idx, start_idx, 1, 0, 1, nullptr };
    return render_pixels(ctx, cam, params, width, height, px, (float4 *)d_rgba_out, counters);
    PRT_API_CATCH_RC(ctx, "prt_render_device")
}

int prt_render(prt_ctx * ctx, const prt_camera * cam, const prt_params * params, uint32_t width, uint32_t height,
               uint32_t start_idx, uint32_t end_idx, float * rgba_out, prt_counters * counters) {
    PRT_API_TRY
    if (!ctx) return -1;
    if ((!rgba_out && end_idx != start_idx) || end_idx < start_idx) { ctx->error = "prt_render: bad output pointer or pixel range"; return -1; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t n = end_idx - start_idx;
    HIP_TRY(ctx, ctx->frame_out.ensure(n));
    int rc = prt_render_device(ctx, cam, params, width, height, start_idx, end_idx, ctx->frame_out.p, counters);
    if (rc) return rc;
    if (n) HIP_TRY(ctx, hipMemcpy(rgba_out, ctx->frame_out.p, n * sizeof(float4), hipMemcpyDeviceToHost));
    return 0;
    PRT_API_CATCH_RC(ctx, "prt_render")
}

uint32_t prt_shard_rows(uint32_t height, uint32_t block_rows, uint32_t rank, uint32_t nranks) {
    if (!block_rows || !nranks || rank >= nranks) return 0;
    uint32_t rows = 0;
    for (uint64_t b = rank; b * block_rows < height; b += nranks) rows += std::min<uint64_t>(block_rows, height - b * block_rows);
    return rows;
}

int prt_render_shard_device(prt_ctx * ctx, const prt_camera * cam, const prt_params * params, uint32_t width, uint32_t height,
                            uint32_t block_rows, uint32_t rank, uint32_t nranks, void * d_rgba_out, prt_counters * counters) {
    PRT_API_TRY
    if (!ctx) return -1;
    if (!block_rows || !nranks || rank >= nranks) { ctx->error = "prt_render_shard: bad arguments"; return -1; }
    if (!d_rgba_out && prt_shard_rows(height, block_rows, rank, nranks)) { ctx->error = "prt_render_shard: null output"; return -1; }
    PixelSet px = { prt_shard_rows(height, block_rows, rank, nranks) * width, 0, block_rows, rank, nranks, nullptr };
    if (nranks == 1) { px.block_rows = 1; }
    return render_pixels(ctx, cam, params, width, height, px, (float4 *)d_rgba_out, counters);
    PRT_API_CATCH_RC(ctx, "prt_render_shard_device")
}

int prt_render_shard(prt_ctx * ctx, const prt_camera * cam, const prt_params * params, uint32_t width, uint32_t height,
                     uint32_t block_rows, uint32_t rank, uint32_t nranks, float * rgba_out, prt_counters * counters) {
    PRT_API_TRY
    if (!ctx) return -1;
    const size_t n = (size_t)prt_shard_rows(height, block_rows, rank, nranks) * width;
    if (!rgba_out && n) { ctx->error = "prt_render_shard: null output"; return -1; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, ctx->frame_out.ensure(n));
    int rc = prt_render_shard_device(ctx, cam, params, width, height, block_rows, rank, nranks, ctx->frame_out.p, counters);
    if (rc) return rc;
    if (n) HIP_TRY(ctx, hipMemcpy(rgba_out, ctx->frame_out.p, n * sizeof(float4), hipMemcpyDeviceToHost));
    return 0;
    PRT_API_CATCH_RC(ctx, "prt_render_shard")
}

int prt_render_pixel_list(prt_ctx * ctx, const prt_camera * cam, const prt_params * params, uint32_t width, uint32_t height,
                          const uint32_t * pixel_ids, uint32_t n_pixels, float * rgba_out, prt_counters * counters) {
    PRT_API_TRY
    if (!ctx) return -1;
    if ((!pixel_ids || !rgba_out) && n_pixels) { ctx->error = "prt_render_pixel_list: null pixel list or output"; return -1; }
    for (uint32_t i = 0; i < n_pixels; ++i)
        if ((uint64_t)pixel_ids[i] >= (uint64_t)width * height) { ctx->error = "prt_render_pixel_list: pixel id outside the image"; return -1; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, ctx->pixel_list.ensure(n_pixels));
    HIP_TRY(ctx, ctx->frame_out.ensure(n_pixels));
    if (n_pixels) HIP_TRY(ctx, hipMemcpyAsync(ctx->pixel_list.p, pixel_ids, (size_t)n_pixels * 4, hipMemcpyHostToDevice, ctx->stream));
    if (n_pixels) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));     // pixel_ids is the caller's memory
    PixelSet px = { n_pixels, 0, 1, 0, 1, ctx->pixel_list.p };
    int rc = render_pixels(ctx, cam, params, width, height, px, ctx->frame_out.p, counters);
    if (rc) return rc;
    if (n_pixels) HIP_TRY(ctx, hipMemcpy(rgba_out, ctx->frame_out.p, (size_t)n_pixels * sizeof(float4), hipMemcpyDeviceToHost));
    return 0;
    PRT_API_CATCH_RC(ctx, "prt_render_pixel_list")
}

int prt_trace_rays_device(prt_ctx * ctx, int mode, const prt_ray_batch * batch, const prt_hit_buffers * hits, uint32_t flags,
                          prt_counters * counters) {
    PRT_API_TRY
    const int chk = query_check(ctx, mode, batch, counters);
    if (chk) return chk > 0 ? 0 : chk;
    return trace_rays(ctx, mode, batch, hits, flags, counters, true);
    PRT_API_CATCH_RC(ctx, "prt_trace_rays_device")
}

int prt_trace_rays(prt_ctx * ctx, int mode, const prt_ray_batch * batch, const prt_hit_buffers * hits, uint32_t flags,
                   prt_counters * counters) {
    PRT_API_TRY
    const int chk = query_check(ctx, mode, batch, counters);
    if (chk) return chk > 0 ? 0 : chk;
    return trace_rays(ctx, mode, batch, hits, flags, counters, false);
    PRT_API_CATCH_RC(ctx, "prt_trace_rays")
}

int prt_trace_hits_device(prt_ctx * ctx, const prt_hits_request * request, const prt_hits_buffers * out, uint32_t flags,
                          prt_counters * counters) {
    PRT_API_TRY
    const int chk = hits_check(ctx, request, out, counters);
    if (chk) return chk > 0 ? 0 : chk;
    return trace_hits(ctx, request, out, flags, counters, true);
    PRT_API_CATCH_RC(ctx, "prt_trace_hits_device")
}

int prt_trace_hits(prt_ctx * ctx, const prt_hits_request * request, const prt_hits_buffers * out, uint32_t flags,
                   prt_counters * counters) {
    PRT_API_TRY
    const int chk = hits_check(ctx, request, out, counters);
    if (chk) return chk > 0 ? 0 : chk;
    return trace_hits(ctx, request, out, flags, counters, false);
    PRT_API_CATCH_RC(ctx, "prt_trace_hits")
}

int prt_closest_points_device(prt_ctx * ctx, const prt_point_batch * batch, const prt_closest_buffers * out, uint32_t flags,
                              prt_counters * counters) {
    PRT_API_TRY
    const int chk = closest_check(ctx, batch, out, counters);
    if (chk) return chk > 0 ? 0 : chk;
    const prt_signed_buffers o = { *out, nullptr, nullptr };
    return closest_points(ctx, batch, o, closest_fields(out), flags, counters, true);
    PRT_API_CATCH_RC(ctx, "prt_closest_points_device")
}

int prt_closest_points(prt_ctx * ctx, const prt_point_batch * batch, const prt_closest_buffers * out, uint32_t flags,
                       prt_counters * counters) {
    PRT_API_TRY
    const int chk = closest_check(ctx, batch, out, counters);
    if (chk) return chk > 0 ? 0 : chk;
    const prt_signed_buffers o = { *out, nullptr, nullptr };
    return closest_points(ctx, batch, o, closest_fields(out), flags, counters, false);
    PRT_API_CATCH_RC(ctx, "prt_closest_points")
}

int prt_signed_distance_device(prt_ctx * ctx, const prt_point_batch * batch, const prt_signed_buffers * out, uint32_t flags,
                               prt_counters * counters) {
    PRT_API_TRY
    const int chk = closest_check(ctx, batch, out ? &out->closest : nullptr, counters);
    if (chk) return chk > 0 ? 0 : chk;
    return closest_points(ctx, batch, *out, signed_fields(out), flags, counters, true);
    PRT_API_CATCH_RC(ctx, "prt_signed_distance_device")
}

int prt_signed_distance(prt_ctx * ctx, const prt_point_batch * batch, const prt_signed_buffers * out, uint32_t flags,
                        prt_counters * counters) {
    PRT_API_TRY
    const int chk = closest_check(ctx, batch, out ? &out->closest : nullptr, counters);
    if (chk) return chk > 0 ? 0 : chk;
    return closest_points(ctx, batch, *out, signed_fields(out), flags, counters, false);
    PRT_API_CATCH_RC(ctx, "prt_signed_distance")
}

int prt_hemisphere_visibility_device(prt_ctx * ctx, const prt_hemi_batch * batch, const prt_hemi_buffers * out, uint32_t flags,
                                     prt_counters * counters) {
    PRT_API_TRY
    const int chk = hemi_check(ctx, batch, out, counters);
    if (chk) return chk > 0 ? 0 : chk;
    return hemisphere_visibility(ctx, batch, out, flags, counters, true);
    PRT_API_CATCH_RC(ctx, "prt_hemisphere_visibility_device")
}

int prt_hemisphere_visibility(prt_ctx * ctx, const prt_hemi_batch * batch, const prt_hemi_buffers * out, uint32_t flags,
                              prt_counters * counters) {
    PRT_API_TRY
    const int chk = hemi_check(ctx, batch, out, counters);
    if (chk) return chk > 0 ? 0 : chk;
    return hemisphere_visibility(ctx, batch, out, flags, counters, false);
    PRT_API_CATCH_RC(ctx, "prt_hemisphere_visibility")
}

int prt_render_rays_device(prt_ctx * ctx, const prt_radiance_batch * batch, const prt_params * params, void * d_rgba_out, prt_counters * counters) {
    PRT_API_TRY
    const int chk = rays_check(ctx, batch, params, d_rgba_out, counters);
    if (chk) return chk < 0 ? chk : 0;
    return render_rays(ctx, batch, params, (float4 *)d_rgba_out, counters, true);
    PRT_API_CATCH_RC(ctx, "prt_render_rays_device")
}

int prt_render_rays(prt_ctx * ctx, const prt_radiance_batch * batch, const prt_params * params, float * rgba_out, prt_counters * counters) {
    PRT_API_TRY
    const int chk = rays_check(ctx, batch, params, rgba_out, counters);
    if (chk) return chk < 0 ? chk : 0;
    return render_rays(ctx, batch, params, (float4 *)rgba_out, counters, false);
    PRT_API_CATCH_RC(ctx, "prt_render_rays")
}

int prt_update_geometry(prt_ctx * ctx, const prt_geometry_update * update, prt_update_info * info) {
    PRT_API_TRY
    return update_geometry(ctx, update, info, false);
    PRT_API_CATCH_RC(ctx, "prt_update_geometry")
}

int prt_update_geometry_device(prt_ctx * ctx, const prt_geometry_update * update, prt_update_info * info) {
    PRT_API_TRY
    return update_geometry(ctx, update, info, true);
    PRT_API_CATCH_RC(ctx, "prt_update_geometry_device")
}

int prt_trace_rays_backward(prt_ctx * ctx, const prt_ray_batch * batch, const int32_t * group, const uint32_t * vertex0, const float * positions,
                            uint32_t position_count, const prt_hit_grads * gout, const prt_query_grads * gin, prt_grad_info * info) {
    PRT_API_TRY
    return grad_backward(ctx, "prt_trace_rays_backward", RayGrad{ batch, group, vertex0, positions, gout, gin }, position_count, info, false);
    PRT_API_CATCH_RC(ctx, "prt_trace_rays_backward")
}

int prt_trace_rays_backward_device(prt_ctx * ctx, const prt_ray_batch * batch, const int32_t * group, const uint32_t * vertex0,
                                   const float * positions, uint32_t position_count, const prt_hit_grads * gout,
                                   const prt_query_grads * gin, prt_grad_info * info) {
    PRT_API_TRY
    return grad_backward(ctx, "prt_trace_rays_backward", RayGrad{ batch, group, vertex0, positions, gout, gin }, position_count, info, true);
    PRT_API_CATCH_RC(ctx, "prt_trace_rays_backward_device")
}

int prt_closest_points_backward(prt_ctx * ctx, const prt_point_batch * batch, const int32_t * group, const uint32_t * vertex0,
                                const float * positions, uint32_t position_count, const prt_closest_grads * gout,
                                const prt_point_grads * gin, prt_grad_info * info) {
    PRT_API_TRY
    return grad_backward(ctx, "prt_closest_points_backward", PointGrad{ batch, group, vertex0, positions, gout, gin }, position_count, info, false);
    PRT_API_CATCH_RC(ctx, "prt_closest_points_backward")
}

int prt_closest_points_backward_device(prt_ctx * ctx, const prt_point_batch * batch, const int32_t * group, const uint32_t * vertex0,
                                       const float * positions, uint32_t position_count, const prt_closest_grads * gout,
                                       const prt_point_grads * gin, prt_grad_info * info) {
    PRT_API_TRY
    return grad_backward(ctx, "prt_closest_points_backward", PointGrad{ batch, group, vertex0, positions, gout, gin }, position_count, info, true);
    PRT_API_CATCH_RC(ctx, "prt_closest_points_backward_device")
}

int prt_sample_surface(prt_ctx * ctx, const prt_sample_request * request, const prt_sample_buffers * out, prt_sample_info * info) {
    PRT_API_TRY
    return sample_surface(ctx, request, out, info, false);
    PRT_API_CATCH_RC(ctx, "prt_sample_surface")
}

int prt_sample_surface_device(prt_ctx * ctx, const prt_sample_request * request, const prt_sample_buffers * out, prt_sample_info * info) {
    PRT_API_TRY
    return sample_surface(ctx, request, out, info, true);
    PRT_API_CATCH_RC(ctx, "prt_sample_surface_device")
}

int prt_sample_surface_backward(prt_ctx * ctx, uint32_t count, const int32_t * group, const uint32_t * vertex0, const float * bw,
                                const float * positions, uint32_t position_count, const prt_sample_grads * gout, float * gin_positions,
                                prt_grad_info * info) {
    PRT_API_TRY
    return sample_surface_backward(ctx, count, group, vertex0, bw, positions, position_count, gout, gin_positions, info, false);
    PRT_API_CATCH_RC(ctx, "prt_sample_surface_backward")
}

int prt_sample_surface_backward_device(prt_ctx * ctx, uint32_t count, const int32_t * group, const uint32_t * vertex0, const float * bw,
                                       const float * positions, uint32_t position_count, const prt_sample_grads * gout, float * gin_positions,
                                       prt_grad_info * info) {
    PRT_API_TRY
    return sample_surface_backward(ctx, count, group, vertex0, bw, positions, position_count, gout, gin_positions, info, true);
    PRT_API_CATCH_RC(ctx, "prt_sample_surface_backward_device")
}

// The geometric check of bvh_check.cpp on the tree as it lies on the device NOW (after any number of updates), against the
// un-indexed triangles of `s`: the GPU suite's proof that a refitted tree is conservative (out[0..5]: bvh_build.h).
int prt_debug_check_refit(prt_ctx * ctx, const prt_scene_desc * s, uint64_t * out) {
    PRT_API_TRY
    if (!ctx) return -1;
    if (!s || !out || s->index_count % 3) { ctx->error = "prt_debug_check_refit: null scene or output"; return -1; }
    if (!ctx->has_scene) { ctx->error = "prt_debug_check_refit: upload a scene first"; return -2; }
    const uint32_t n_tris = s->index_count / 3;
    if (n_tris != ctx->scene.tri_count || ctx->keep.tri_order.size() != n_tris) { ctx->error = "prt_debug_check_refit: the scene's triangle count differs from the uploaded scene's"; return -1; }
    for (uint32_t i = 0; i < s->index_count; ++i)
        if (s->idx_positions[i] >= s->position_count) { ctx->error = "prt_debug_check_refit: vertex index out of range"; return -1; }
    std::vector<float> verts((size_t)n_tris * 9);
    for (uint32_t t = 0; t < n_tris; ++t)
        for (int c = 0; c < 3; ++c) memcpy(&verts[(size_t)t * 9 + 3 * c], s->positions + 3 * (size_t)s->idx_positions[3 * t + c], 12);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    BvhWide bvh;
    bvh.node_dwords = BVH_WIDTH == 8 ? BVH8_NODE_DWORDS : BVH4_NODE_DWORDS;
    bvh.node_count = ctx->scene.node_count;
    bvh.max_depth = ctx->desc.info.bvh_max_depth;
    bvh.stack_bound = ctx->desc.stack_bound;
    bvh.nodes.resize((size_t)bvh.node_count * bvh.node_dwords);
    bvh.tri_order = ctx->keep.tri_order;
    HIP_TRY(ctx, hipMemcpy(bvh.nodes.data(), ctx->arrays.nodes.p, bvh.nodes.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (const char * bad = validate_bvh_links(bvh, n_tris)) { ctx->error = std::string("prt_debug_check_refit: ") + bad; return -9; }
    check_bvh_wide(verts.data(), n_tris, bvh, out);
    return 0;
    PRT_API_CATCH_RC(ctx, "prt_debug_check_refit")
}

int prt_debug_device_kat(prt_ctx * ctx, int kind, const void * in, size_t in_bytes, void * out, size_t out_bytes, uint32_t n,
                         const prt_camera * cam_in) {
    PRT_API_TRY
    if (!ctx) return -1;
    if (!ctx->has_scene) { ctx->error = "prt_debug_device_kat: upload a scene first"; return -2; }
    if (!in || !out || !n) { ctx->error = "prt_debug_device_kat: null buffers"; return -1; }
    if (kind == KAT_TEXTURE) {                                  // the kinds that follow indices into the scene: checked here, not on the device
        if (in_bytes != (size_t)n * 12 || out_bytes != (size_t)n * 16) { ctx->error = "prt_debug_device_kat: KAT_TEXTURE takes 3 floats and gives 4 per record"; return -1; }
        if (!ctx->desc.textured) { ctx->error = "prt_debug_device_kat: KAT_TEXTURE needs a scene with texture maps"; return -2; }
        for (uint32_t i = 0; i < n; ++i) {
            const float ti = ((const float *)in)[3 * (size_t)i];
            if (!(ti >= 0.0f && ti < (float)ctx->desc.kat_textures.size()) || ctx->desc.kat_textures[(size_t)ti].size_x < 2) {
                ctx->error = "prt_debug_device_kat: KAT_TEXTURE record names no usable texture";
                return -1;
            }
        }
    }
    if (kind == KAT_TEXTURED_HIT) {
        if (in_bytes != (size_t)n * 12 || out_bytes != (size_t)n * 64) { ctx->error = "prt_debug_device_kat: KAT_TEXTURED_HIT takes 3 floats and gives 16 per record"; return -1; }
        for (uint32_t i = 0; i < n; ++i) {
            const float slot = ((const float *)in)[3 * (size_t)i];
            if (!(slot >= 0.0f && slot < (float)ctx->scene.tri_count)) { ctx->error = "prt_debug_device_kat: KAT_TEXTURED_HIT record names no triangle"; return -1; }
        }
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // scratch buffers owned by DevBuf objects: released on every return path
    struct Scratch {
        DevBuf<unsigned char> in, out;
        ~Scratch() { in.release(); out.release(); }
    } scratch;
    HIP_TRY(ctx, scratch.in.ensure(in_bytes));
    HIP_TRY(ctx, scratch.out.ensure(out_bytes));
    void * d_in = scratch.in.p;
    void * d_out = scratch.out.p;
    HIP_TRY(ctx, ctx->ring_ws.ensure((size_t)16 * n));
    // everything on the context's stream: it is a non-blocking stream, so work on the null stream (a plain hipMemset)
    // is NOT ordered against the kernel below
    HIP_TRY(ctx, hipMemcpyAsync(d_in, in, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(d_out, 0, out_bytes, ctx->stream));
    DevCamera cam;
    memset(&cam, 0, sizeof(cam));
    if (cam_in) {
        cam.position = ld3(cam_in->position);
        cam.forward = ld3(cam_in->forward);
        cam.right_scaled = ld3(cam_in->right) * cam_in->tan_a2 * cam_in->aspect;
        cam.up_scaled = ld3(cam_in->up) * cam_in->tan_a2;
        cam.inv_width = cam_in->inv_width;
        cam.inv_height = cam_in->inv_height;
    }
    hipLaunchKernelGGL(k_debug_kat, dim3((n + 63) / 64), dim3(64), 0, ctx->stream, kind, d_in, d_out, n, ctx->scene, cam, ctx->ring_ws.p);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(out, d_out, out_bytes, hipMemcpyDeviceToHost));
    return 0;
    PRT_API_CATCH_RC(ctx, "prt_debug_device_kat")
}

// Host-only self check of the acceleration structure (no GPU needed; used by the CPU test-suite): builds the wide BVH for
// `scene` exactly as prt_upload_scene does and runs the link validation and the geometric check of bvh_check.cpp on it
// (out[0..5]: bvh_build.h check_bvh_wide).
int prt_debug_check_bvh(const prt_scene_desc * s, uint64_t * out) {
    PRT_API_TRY
    if (!s || !out || s->index_count % 3) return -1;
    const uint32_t n_tris = s->index_count / 3;
    std::vector<float> verts((size_t)n_tris * 9);
    for (uint32_t t = 0; t < n_tris; ++t)
        for (int c = 0; c < 3; ++c) memcpy(&verts[(size_t)t * 9 + 3 * c], s->positions + 3 * (size_t)s->idx_positions[3 * t + c], 12);
    PrtOptions opt;
    prt_options_from_env(opt);                  // the test-suite selects the collapse rule through the environment
    BvhWide bvh;
    build_bvh_wide(BVH_WIDTH, verts.data(), n_tris, BVH_LEAF_MAX, 4, &bvh, 1.0f, &opt.bvh);
    if (validate_bvh_links(bvh, n_tris)) return -9;          // what prt_upload_scene checks before it uploads a tree
    check_bvh_wide(verts.data(), n_tris, bvh, out);
    return 0;
    PRT_API_CATCH_RC(nullptr, "prt_debug_check_bvh")
}

// The normal cones of the same tree (bvh_build.h attach_normal_cones, over the record normals and the origin bound of an upload):
// out[0] = (coned node, triangle below it) pairs the stored bits do not cover (check_bvh_cones), out[1] = nodes with a cone.
int prt_debug_check_cones(const prt_scene_desc * s, uint64_t * out) {
    PRT_API_TRY
    if (!s || !out || s->index_count % 3) return -1;
    const uint32_t n_tris = s->index_count / 3;
    std::vector<float> verts((size_t)n_tris * 9), normals((size_t)n_tris * 3);
    float abs_max = 0.0f;
    for (uint32_t t = 0; t < n_tris; ++t) {
        for (int c = 0; c < 3; ++c) memcpy(&verts[(size_t)t * 9 + 3 * c], s->positions + 3 * (size_t)s->idx_positions[3 * t + c], 12);
        float4 rec[3];
        tri_record(ld3(&verts[(size_t)t * 9]), ld3(&verts[(size_t)t * 9 + 3]), ld3(&verts[(size_t)t * 9 + 6]), rec);
        normals[(size_t)t * 3] = rec[2].y; normals[(size_t)t * 3 + 1] = rec[2].z; normals[(size_t)t * 3 + 2] = rec[2].w;
        for (int k = 0; k < 9; ++k) abs_max = std::max(abs_max, fabsf(verts[(size_t)t * 9 + k]));
    }
    PrtOptions opt;
    prt_options_from_env(opt);
    BvhWide bvh;
    build_bvh_wide(BVH_WIDTH, verts.data(), n_tris, BVH_LEAF_MAX, 4, &bvh, 1.0f, &opt.bvh);
    if (validate_bvh_links(bvh, n_tris)) return -9;
    attach_normal_cones(bvh, normals.data(), n_tris, 32.0 * (double)abs_max, 4);
    out[0] = check_bvh_cones(verts.data(), n_tris, bvh, 32.0 * (double)abs_max, &out[1]);
    return 0;
    PRT_API_CATCH_RC(nullptr, "prt_debug_check_cones")
}

// The same check on the tree of the GPU LBVH builder (needs a context: the radix tree is built on its device).
int prt_debug_check_bvh_lbvh(prt_ctx * ctx, const prt_scene_desc * s, uint64_t * out) {
    PRT_API_TRY
    if (!ctx || !s || !out || s->index_count % 3) return -1;
    const uint32_t n_tris = s->index_count / 3;
    std::vector<float> verts((size_t)n_tris * 9);
    for (uint32_t t = 0; t < n_tris; ++t)
        for (int c = 0; c < 3; ++c) memcpy(&verts[(size_t)t * 9 + 3 * c], s->positions + 3 * (size_t)s->idx_positions[3 * t + c], 12);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    BvhWide bvh;
    int rc = build_bvh_lbvh(ctx, verts.data(), n_tris, BVH_LEAF_MAX, &bvh);
    if (rc) return rc;
    if (const char * bad = validate_bvh_links(bvh, n_tris)) { ctx->error = bad; return -9; }
    check_bvh_wide(verts.data(), n_tris, bvh, out);
    return 0;
    PRT_API_CATCH_RC(ctx, "prt_debug_check_bvh_lbvh")
}

// The device's radix tree itself, before the host back end: the arrays build_lbvh_tree returns, copied out (include/prt.h).
int prt_debug_lbvh_tree(prt_ctx * ctx, uint32_t n_tris, const float * verts, int32_t * left, int32_t * right, uint32_t * first, uint32_t * last,
                        float * node_box, float * leaf_box, uint32_t * sorted_ids, uint64_t * sorted_keys) {
    PRT_API_TRY
    if (!ctx) return -1;
    if (!n_tris || !verts) { ctx->error = "prt_debug_lbvh_tree: no triangles"; return -1; }
    for (size_t i = 0; i < (size_t)n_tris * 9; ++i)
        if (!(fabsf(verts[i]) < 1e18f)) { ctx->error = "prt_debug_lbvh_tree: vertex coordinate is not finite or exceeds 1e18"; return -1; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    float lo[3], hi[3];
    lbvh_scene_bounds(verts, n_tris, lo, hi);
    LbvhTree tree;
    HIP_TRY(ctx, build_lbvh_tree(verts, n_tris, lo, hi, ctx->stream, &tree, nullptr, sorted_keys != nullptr));
    const size_t n = n_tris, ni = tree.left.size();
    if (left) memcpy(left, tree.left.data(), ni * 4);
    if (right) memcpy(right, tree.right.data(), ni * 4);
    if (first) memcpy(first, tree.first.data(), ni * 4);
    if (last) memcpy(last, tree.last.data(), ni * 4);
    if (node_box) memcpy(node_box, tree.node_box.data(), ni * 24);
    if (leaf_box) memcpy(leaf_box, tree.leaf_box.data(), n * 24);
    if (sorted_ids) memcpy(sorted_ids, tree.sorted_ids.data(), n * 4);
    if (sorted_keys) memcpy(sorted_keys, tree.sorted_keys.data(), n * 8);
    return 0;
    PRT_API_CATCH_RC(ctx, "prt_debug_lbvh_tree")
}

}  // extern "C"

// =============================================================================================================
// Several devices behind one handle (prt_create(const int * device_ids, int n_dev)) - the product's
// multi-GPU path.  Replaces the reference's partition + MPI_Gather (main.cpp:311-347): the scene is replicated (as every
// MPI rank holds it), device g renders the row blocks b with b % n == g into a packed buffer in its own HBM, the shards
// travel to device 0 over the fabric as peer-to-peer copies - DMA engines over xGMI, no compute unit involved, so they
// do not compete with the persistent render kernels for wave slots the way a collective's kernels do -, one small kernel
// on device 0 puts the rows where they belong, and ONE copy takes the frame to the host.
//
// Round 4: FRAMES IN FLIGHT.  A persistent kernel leaves its GPU partly idle while its last rays drain (a 1/8 shard of the
// headline frame: 2.1 ms at one frame at a time, 1.75 ms per frame with two in flight, profiles/r03_shards_frames_in_flight.txt),
// and the copies / assembly / download of frame k need no compute unit that frame k + 1 could not use.  The handle
// therefore holds `depth` LANES (default 2, PRT_MULTI_DEPTH): a lane is one context per device - lane 0 the contexts
// prt_multi_context() returns, the others CLONES that share the uploaded scene's device arrays and own only their streams
// and workspaces - plus the lane's shard / staging / frame buffers.  prt_multi_submit() hands a frame to a free lane and
// returns; the lane's worker threads - one per device, created ONCE with the handle, not per frame - render and send
// their shards; prt_multi_wait() assembles and downloads.  prt_multi_render() is submit + wait.
__global__ void k_assemble_shards(const float4 * staging, float4 * frame, unsigned int width, unsigned int height,
                                  unsigned int block_rows, unsigned int n_dev, unsigned int max_shard_rows) {
    const unsigned int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= width * height) return;
    const unsigned int y = i / width, x = i - y * width;
    const unsigned int b = y / block_rows, g = b % n_dev;
    const unsigned int local_row = (b / n_dev) * block_rows + (y - b * block_rows);
    frame[i] = staging[((size_t)g * max_shard_rows + local_row) * width + x];
}

enum { PRT_MULTI_BLOCK_ROWS = 8, PRT_MULTI_MAX_DEPTH = 4 };

struct MultiLane {
    std::vector<prt_ctx *> ctx;              // per device; lane 0: the handle's own contexts, else clones of them
    std::vector<DevBuf<float4> > shard;      // per device: its packed shard (device g's memory)
    DevBuf<float4> staging, frame;           // device 0: every shard side by side; the assembled frame
    std::vector<hipEvent_t> done;            // per device: its peer copy has landed
    // the frame in flight on this lane (written by submit under the handle's mutex, read by the lane's workers)
    bool busy = false;
    uint64_t ticket = 0;
    prt_camera cam;
    prt_params params;
    uint32_t width = 0, height = 0;
    float * rgba_out = nullptr;
    unsigned int pending = 0;                // workers that have not finished this frame yet
    std::vector<uint64_t> job;               // per device: generation of the job handed to its worker
    std::vector<int> rc;
    std::vector<std::string> err;
    std::vector<prt_counters> ctr;
};

struct prt_multi {
    std::vector<int> devices;
    std::vector<MultiLane> lane;
    std::vector<std::thread> workers;        // lanes x devices, alive as long as the handle
    std::mutex mu;
    std::condition_variable cv_work, cv_done;
    bool quit = false;
    uint64_t next_ticket = 1;
    std::string error;
};

namespace {

// A second context on src's device that SHARES the uploaded scene's device arrays (it does not own them: src must
// outlive it and must not be re-uploaded while it exists) and has streams, events and workspaces of its own.
prt_ctx * clone_context(prt_ctx * src) {
    prt_ctx * c = prt_create(src->device);
    if (!c) return nullptr;
    c->opt = src->opt;
    c->arrays.borrow(src->arrays);
    c->desc = src->desc;
    c->scene = src->scene;
    c->scene.near_tie_unresolved = &c->counters.p->near_tie_unresolved;      // its own counters
    c->scene.spec_dirs = nullptr;
    c->spec_table_samples = 0;              // its own specular direction table, built at its first render
    c->pool_park_cap = src->pool_park_cap; c->pool_spark_cap = src->pool_spark_cap;
    c->has_scene = src->has_scene;
    c->scene_epoch = 1;
    return c;
}

void multi_worker(prt_multi * m, unsigned int f, unsigned int g) {
    MultiLane & L = m->lane[f];
    uint64_t seen = 0;
    for (;;) {
        {
            std::unique_lock<std::mutex> lk(m->mu);
            m->cv_work.wait(lk, [&] { return m->quit || L.job[g] != seen; });
            if (m->quit) return;
            seen = L.job[g];
        }
        int rc = 0;
        std::string err;
        prt_counters ctr;
        memset(&ctr, 0, sizeof(ctr));
        try {
            const unsigned int n = (unsigned int)L.ctx.size();
            prt_ctx * c = L.ctx[g], * c0 = L.ctx[0];
            const size_t rows = prt_shard_rows(L.height, PRT_MULTI_BLOCK_ROWS, g, n);
            const uint32_t max_rows = prt_shard_rows(L.height, PRT_MULTI_BLOCK_ROWS, 0, n);      // rank 0 owns the most rows
            hipError_t e = hipSuccess;
            if (!c || !c0) { rc = PRT_ERR_NO_SCENE; err = "prt_multi worker: the lane has lost a context"; }
            if (!rc) e = hipSetDevice(c->device);
            if (!rc && e == hipSuccess) e = L.shard[g].ensure(std::max<size_t>(1, rows * L.width));
            if (!rc && e != hipSuccess) { rc = PRT_ERR_HIP; err = std::string("shard buffer: ") + hipGetErrorString(e); }
            if (!rc) {
                rc = prt_render_shard_device(c, &L.cam, &L.params, L.width, L.height, PRT_MULTI_BLOCK_ROWS, g, n, L.shard[g].p, &ctr);
                if (rc) err = prt_last_error(c);
            }
            if (!rc && n > 1) {
                // the shard's trip to device 0, queued on the rendering context's own stream: a shard that is done travels
                // while the others still render
                if (rows) e = hipMemcpyPeerAsync(L.staging.p + (size_t)g * max_rows * L.width, c0->device, L.shard[g].p, c->device,
                                                 rows * L.width * sizeof(float4), c->stream);
                if (e == hipSuccess) e = hipEventRecord(L.done[g], c->stream);
                if (e != hipSuccess) { rc = PRT_ERR_HIP; err = std::string("peer copy: ") + hipGetErrorString(e); }
            }
        } catch (...) {
            rc = api_exception(&err, "prt_multi worker");
        }
        {
            std::lock_guard<std::mutex> lk(m->mu);
            L.rc[g] = rc;
            try { L.err[g] = err; } catch (...) {}
            L.ctr[g] = ctr;
            if (--L.pending == 0) m->cv_done.notify_all();
        }
    }
}

void multi_release_lane(MultiLane & L, bool destroy_ctx) {
    for (size_t g = 0; g < L.ctx.size(); ++g) {
        if (!L.ctx[g]) continue;
        (void)hipSetDevice(L.ctx[g]->device);
        if (L.ctx[g]->stream) (void)hipStreamSynchronize(L.ctx[g]->stream);
        if (g < L.shard.size()) L.shard[g].release();
        if (g < L.done.size() && L.done[g]) { (void)hipEventDestroy(L.done[g]); L.done[g] = nullptr; }
    }
    if (!L.ctx.empty() && L.ctx[0]) {
        (void)hipSetDevice(L.ctx[0]->device);
        L.staging.release();
        L.frame.release();
    }
    if (destroy_ctx)
        for (size_t g = 0; g < L.ctx.size(); ++g) { prt_destroy(L.ctx[g]); L.ctx[g] = nullptr; }
}

// Every stream of every lane drained: after a failure nothing of the failed frame is still writing into staging / frame.
void multi_quiesce(prt_multi * m) {
    for (MultiLane & L : m->lane)
        for (prt_ctx * c : L.ctx)
            if (c && c->stream) { (void)hipSetDevice(c->device); (void)hipStreamSynchronize(c->stream); }
}

}  // namespace

extern "C" {

prt_multi * prt_multi_create(const int * device_ids, int n_dev) {
    PRT_API_TRY
    if (!device_ids || n_dev < 1) { g_create_error = "prt_multi_create: no devices"; return nullptr; }
    prt_multi * m = new prt_multi;
    m->devices.assign(device_ids, device_ids + n_dev);
    long long depth = 2;
    if (const char * v = getenv("PRT_MULTI_DEPTH")) depth = atoll(v);        // creation only, like every PRT_* variable
    depth = std::max(1ll, std::min((long long)PRT_MULTI_MAX_DEPTH, depth));
    m->lane.resize((size_t)depth);
    for (MultiLane & L : m->lane) {
        L.ctx.assign((size_t)n_dev, nullptr);
        L.shard.resize((size_t)n_dev);
        L.done.assign((size_t)n_dev, nullptr);
        L.job.assign((size_t)n_dev, 0);
        L.rc.assign((size_t)n_dev, 0);
        L.err.resize((size_t)n_dev);
        L.ctr.resize((size_t)n_dev);
    }
    for (int g = 0; g < n_dev; ++g) {
        prt_ctx * c = prt_create(device_ids[g]);
        if (!c) { prt_multi_destroy(m); return nullptr; }
        m->lane[0].ctx[(size_t)g] = c;
    }
    for (MultiLane & L : m->lane)
        for (int g = 0; g < n_dev; ++g) {
            prt_ctx * c0 = m->lane[0].ctx[0], * c = m->lane[0].ctx[(size_t)g];
            if (hipSetDevice(c->device) != hipSuccess || hipEventCreateWithFlags(&L.done[(size_t)g], hipEventDisableTiming) != hipSuccess) {
                g_create_error = "prt_multi_create: event creation failed";
                prt_multi_destroy(m);
                return nullptr;
            }
            // direct loads / stores between the devices where the fabric offers them (the copies work either way)
            if (&L == &m->lane[0] && g > 0 && c->device != c0->device) {
                int can = 0;
                if (hipDeviceCanAccessPeer(&can, c0->device, c->device) == hipSuccess && can) {
                    (void)hipSetDevice(c0->device);
                    (void)hipDeviceEnablePeerAccess(c->device, 0);
                    (void)hipGetLastError();             // "already enabled" is fine
                }
            }
        }
    // the workers: one per (lane, device), for the life of the handle (round 3 created and joined n threads per frame)
    for (unsigned int f = 0; f < (unsigned int)depth; ++f)
        for (unsigned int g = 0; g < (unsigned int)n_dev; ++g) m->workers.emplace_back(multi_worker, m, f, g);
    return m;
    PRT_API_CATCH_PTR("prt_multi_create")
}

void prt_multi_destroy(prt_multi * m) {
    PRT_API_TRY
    if (!m) return;
    {
        std::unique_lock<std::mutex> lk(m->mu);
        // frames still in flight finish first (their buffers and contexts go away below)
        m->cv_done.wait(lk, [&] { for (MultiLane & L : m->lane) if (L.pending) return false; return true; });
        m->quit = true;
    }
    m->cv_work.notify_all();
    for (std::thread & t : m->workers) if (t.joinable()) t.join();
    for (size_t f = m->lane.size(); f-- > 0;) multi_release_lane(m->lane[f], true);      // the clones before the contexts they borrow from
    delete m;
    PRT_API_CATCH_VOID
}

const char * prt_multi_last_error(const prt_multi * m) { return m ? m->error.c_str() : g_create_error.c_str(); }
int prt_multi_device_count(const prt_multi * m) { return m ? (int)m->devices.size() : 0; }
int prt_multi_depth(const prt_multi * m) { return m ? (int)m->lane.size() : 0; }
prt_ctx * prt_multi_context(prt_multi * m, int i) { return m && i >= 0 && (size_t)i < m->devices.size() ? m->lane[0].ctx[(size_t)i] : nullptr; }

int prt_multi_upload_scene(prt_multi * m, const prt_scene_desc * scene) {
    PRT_API_TRY
    if (!m) return -1;
    {
        std::lock_guard<std::mutex> lk(m->mu);
        for (MultiLane & L : m->lane)
            if (L.busy) { m->error = "prt_multi_upload_scene: a frame is still in flight (prt_multi_wait it first)"; return PRT_ERR_IN_FLIGHT; }
    }
    // the other lanes' contexts borrow lane 0's scene arrays: they go before those are replaced, and come back after
    for (size_t f = 1; f < m->lane.size(); ++f)
        for (size_t g = 0; g < m->lane[f].ctx.size(); ++g) { prt_destroy(m->lane[f].ctx[g]); m->lane[f].ctx[g] = nullptr; }
    for (size_t g = 0; g < m->devices.size(); ++g) {
        const int rc = prt_upload_scene(m->lane[0].ctx[g], scene);
        if (rc) { m->error = prt_last_error(m->lane[0].ctx[g]); return rc; }
    }
    for (size_t f = 1; f < m->lane.size(); ++f)
        for (size_t g = 0; g < m->devices.size(); ++g) {
            m->lane[f].ctx[g] = clone_context(m->lane[0].ctx[g]);
            if (m->lane[f].ctx[g]) continue;
            // a lane is whole or absent: prt_multi_submit takes none with a context missing
            for (size_t k = 0; k < g; ++k) { prt_destroy(m->lane[f].ctx[k]); m->lane[f].ctx[k] = nullptr; }
            m->error = std::string("prt_multi_upload_scene: ") + g_create_error;
            return PRT_ERR_HIP;
        }
    return 0;
    PRT_API_CATCH_RC_MULTI(m, "prt_multi_upload_scene")
}

int prt_multi_update_geometry(prt_multi * m, const prt_geometry_update * update) {
    PRT_API_TRY
    if (!m) return -1;
    {
        std::lock_guard<std::mutex> lk(m->mu);
        for (MultiLane & L : m->lane)
            if (L.busy) { m->error = "prt_multi_update_geometry: a frame is still in flight (prt_multi_wait it first)"; return PRT_ERR_IN_FLIGHT; }
    }
    // no lane is busy: every render call has returned with its stream drained.  Lane 0's contexts own the scene arrays ...
    int rc = 0;
    for (size_t g = 0; g < m->devices.size() && !rc; ++g) {
        rc = prt_update_geometry(m->lane[0].ctx[g], update, nullptr);
        if (rc) m->error = prt_last_error(m->lane[0].ctx[g]);
    }
    // ... and the other lanes' contexts share them, with a copy of what describes them: it follows (also after a failure:
    // a context that lost its scene takes its clones' with it)
    for (size_t f = 1; f < m->lane.size(); ++f)
        for (size_t g = 0; g < m->devices.size(); ++g) {
            prt_ctx * src = m->lane[0].ctx[g], * c = m->lane[f].ctx[g];
            if (!src || !c) continue;
            c->arrays.ref_spheres.borrow(src->arrays.ref_spheres);              // the update may have allocated or enlarged it
            c->scene.ref_spheres = src->scene.ref_spheres;
            c->desc = src->desc;
            c->has_scene = src->has_scene;
            c->tuned.clear();
        }
    return rc;
    PRT_API_CATCH_RC_MULTI(m, "prt_multi_update_geometry")
}

#define MULTI_TRY(m, call)                                                                                   \
    do {                                                                                                     \
        hipError_t e_ = (call);                                                                              \
        if (e_ != hipSuccess) { (m)->error = std::string(#call) + ": " + hipGetErrorString(e_); multi_quiesce(m); return PRT_ERR_HIP; } \
    } while (0)

int prt_multi_submit(prt_multi * m, const prt_camera * cam, const prt_params * params, uint32_t width, uint32_t height,
                     float * rgba_out, uint64_t * ticket) {
    PRT_API_TRY
    if (!m || m->devices.empty()) return -1;
    if (!cam || !params || !ticket) { m->error = "prt_multi_submit: null camera, params or ticket"; return -1; }
    if (!rgba_out && width && height) { m->error = "prt_multi_submit: null output"; return -1; }
    const unsigned int n = (unsigned int)m->devices.size();
    MultiLane * L = nullptr;
    {
        std::lock_guard<std::mutex> lk(m->mu);
        for (MultiLane & c : m->lane)
            if (!c.busy && std::find(c.ctx.begin(), c.ctx.end(), nullptr) == c.ctx.end()) { L = &c; break; }
        if (!L) { m->error = "prt_multi_submit: every lane has a frame in flight (prt_multi_wait the oldest ticket first)"; return PRT_ERR_IN_FLIGHT; }
        L->busy = true;                      // reserved; the workers start below, when the buffers are there
    }
    const uint32_t max_rows = prt_shard_rows(height, PRT_MULTI_BLOCK_ROWS, 0, n);
    prt_ctx * c0 = L->ctx[0];
    hipError_t e = hipSetDevice(c0->device);
    if (e == hipSuccess && n > 1) e = L->staging.ensure((size_t)n * max_rows * width);
    if (e == hipSuccess && n > 1) e = L->frame.ensure((size_t)width * height);
    if (e != hipSuccess) {
        std::lock_guard<std::mutex> lk(m->mu);
        L->busy = false;
        m->error = std::string("prt_multi_submit: buffers on device 0: ") + hipGetErrorString(e);
        return PRT_ERR_HIP;
    }
    {
        std::lock_guard<std::mutex> lk(m->mu);
        L->cam = *cam; L->params = *params; L->width = width; L->height = height; L->rgba_out = rgba_out;
        L->ticket = m->next_ticket++;
        L->pending = n;
        for (unsigned int g = 0; g < n; ++g) { L->rc[g] = 0; L->err[g].clear(); L->job[g]++; }
        *ticket = L->ticket;
    }
    m->cv_work.notify_all();
    return 0;
    PRT_API_CATCH_RC_MULTI(m, "prt_multi_submit")
}

int prt_multi_wait(prt_multi * m, uint64_t ticket, prt_counters * counters) {
    PRT_API_TRY
    if (!m || m->devices.empty()) return -1;
    const unsigned int n = (unsigned int)m->devices.size();
    MultiLane * L = nullptr;
    {
        std::unique_lock<std::mutex> lk(m->mu);
        for (MultiLane & c : m->lane)
            if (c.busy && c.ticket == ticket) { L = &c; break; }
        if (!L) { m->error = "prt_multi_wait: no frame with this ticket is in flight"; return -1; }
        m->cv_done.wait(lk, [&] { return L->pending == 0; });
    }
    // from here on the lane's workers are idle: its fields are this thread's
    struct Release { prt_multi * m; MultiLane * L; ~Release() { std::lock_guard<std::mutex> lk(m->mu); L->busy = false; } } release = { m, L };
    for (unsigned int g = 0; g < n; ++g)
        if (L->rc[g]) { m->error = L->err[g]; multi_quiesce(m); return L->rc[g]; }
    prt_ctx * c0 = L->ctx[0];
    const size_t n_px = (size_t)L->width * L->height;
    MULTI_TRY(m, hipSetDevice(c0->device));
    if (n == 1) {
        // one device: its "shard" is the frame (the render call returned with its stream drained)
        if (n_px) MULTI_TRY(m, hipMemcpy(L->rgba_out, L->shard[0].p, n_px * sizeof(float4), hipMemcpyDeviceToHost));
    } else {
        const uint32_t max_rows = prt_shard_rows(L->height, PRT_MULTI_BLOCK_ROWS, 0, n);
        for (unsigned int g = 0; g < n; ++g) MULTI_TRY(m, hipStreamWaitEvent(c0->stream, L->done[g], 0));
        if (n_px) {
            hipLaunchKernelGGL(k_assemble_shards, dim3((unsigned int)((n_px + 255) / 256)), dim3(256), 0, c0->stream, L->staging.p, L->frame.p,
                               L->width, L->height, (unsigned int)PRT_MULTI_BLOCK_ROWS, n, max_rows);
            MULTI_TRY(m, hipGetLastError());
            MULTI_TRY(m, hipMemcpyAsync(L->rgba_out, L->frame.p, n_px * sizeof(float4), hipMemcpyDeviceToHost, c0->stream));
        }
        MULTI_TRY(m, hipStreamSynchronize(c0->stream));
    }
    if (counters) {
        prt_counters sum;
        memset(&sum, 0, sizeof(sum));
        for (unsigned int g = 0; g < n; ++g) {
            const prt_counters & c = L->ctr[g];
            sum.ray_count += c.ray_count; sum.node_visits += c.node_visits; sum.tri_tests += c.tri_tests;
            sum.shaded_hits += c.shaded_hits; sum.trace_kernel_launches += c.trace_kernel_launches;
            sum.render_ms = std::max(sum.render_ms, c.render_ms);                   // the devices run concurrently
            sum.trace_kernel_ms = std::max(sum.trace_kernel_ms, c.trace_kernel_ms);
            sum.pipeline = c.pipeline;
        }
        *counters = sum;
    }
    return 0;
    PRT_API_CATCH_RC_MULTI(m, "prt_multi_wait")
}

int prt_multi_render(prt_multi * m, const prt_camera * cam, const prt_params * params, uint32_t width, uint32_t height,
                     float * rgba_out, prt_counters * counters) {
    PRT_API_TRY
    uint64_t ticket = 0;
    const int rc = prt_multi_submit(m, cam, params, width, height, rgba_out, &ticket);
    if (rc) return rc;
    return prt_multi_wait(m, ticket, counters);
    PRT_API_CATCH_RC_MULTI(m, "prt_multi_render")
}

// Test hook of the exception guard (tests/test_host_side.py): throws the given kind of C++ exception inside a guarded
// entry point and returns what the caller of any entry point would get.  ctx may be NULL (no GPU needed).
int prt_debug_throw(prt_ctx * ctx, int kind) {
    PRT_API_TRY
    if (kind == 1) throw std::bad_alloc();
    if (kind == 2) { std::vector<float> v; v.resize(v.max_size() + 1); return (int)v.size(); }     // the real thing: std::length_error
    if (kind == 3) throw std::runtime_error("thrown on request");
    if (kind == 4) throw 42;
    return 0;
    PRT_API_CATCH_RC(ctx, "prt_debug_throw")
}

}  // extern "C"
