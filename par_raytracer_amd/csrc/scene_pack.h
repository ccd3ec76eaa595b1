// scene_pack.h - the host half of prt_upload_scene: the checks of the description, the un-indexing, the reference's visit ranks
// and the layout of every array the upload puts on the device, with no HIP call in it and no prt_ctx in sight.  hipcc compiles
// scene_pack.cpp into the library beside bvh_build.cpp; g++ compiles it against tests/hip_shim into tests/scene_pack_host_harness.cpp
// and the shadow harnesses, which run it under ASan and UBSan.  prt_api.hip keeps the device half: the tree builders' choice,
// the uploads, the commit into the context.
//
// What the upload leaves in the context is three structs: SceneDesc (what the host knows about the arrays on the device; a clone
// copies it whole), SceneKeep (host memory that later calls read: refit, gradients, signed distances, sampling) and, in
// prt_api.hip, SceneArrays (the device buffers).  pack_scene fills the first two and the arrays' host images in a PackedScene;
// the context takes them over only when every array lies on the device.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "dev_scene.h"
#include "bvh_build.h"

namespace prt {

// Everything the host knows about the scene arrays on the device, and that a context sharing them (clone_context) must know too.
// Plain data: copied whole.
struct SceneDesc {
    prt_scene_info info = prt_scene_info();
    float scene_abs_max = 0.0f;
    unsigned int stack_bound = 0;
    unsigned int light_stride = 1;        // the light table's two copies lie this far apart: shadow-tree roots in DevLight::pad, then every root at 0
    bool any_translucent = false;
    bool point_lights = false;            // any point light: its shadow rays use the hit distance (raytracer.cpp:396), so they can be near-tied too
    bool textured = false;                // any material has a texture map: the TEX kernel variants run
    std::vector<float> material_ns;       // for rebuilding spec_dirs when spec_samples changes
    std::vector<DevTexture> kat_textures; // host copy of the texture table: prt_debug_device_kat checks KAT_TEXTURE's indices against it
    uint64_t ref_sphere_bytes = 0;        // info.device_bytes' share of the reference's sphere tree (prt_update_geometry replaces it)
    // shadow trees (include/prt.h): one entry per light; fresh = of the geometry on the device (an update makes them stale);
    // origin_max = the |coordinate| of a shadow ray's origin that the exclusion bound covers (bvh_build.h), and what a
    // render call's |ray_bias| and camera position may be for its shadow rays to stay inside it
    std::vector<prt_shadow_tree_info> shadow_info;
    bool shadow_trees_fresh = false;
    float shadow_bias_max = 0.0f, shadow_cam_max = 0.0f;
    // open triangles (include/prt.h): one entry per light; the flags lie in the shading records and go stale with the trees
    // (shadow_trees_fresh).  A call takes them while its |ray_bias| is at most open_bias_max and its hits lie below open_reach,
    // the bounds the upload computed them for; open_reach = 0: no light has flags.
    std::vector<prt_shadow_open_info> shadow_open_info;
    float shadow_open_bias_max = 0.0f, shadow_open_reach = 0.0f;
    // normal cones (dev_scene.h): nodes of the scene's tree that carry one, and what attaching them cost.  They hold for the calls
    // the shadow trees hold for (shadow_bias_max, shadow_cam_max); a refit clears them node by node, so they are never stale.
    prt_normal_cone_info cone_info = prt_normal_cone_info();
};

// What the upload keeps on the host for later calls: the queries' leaf map, prt_update_geometry's table and ranks, the gradients'
// runs, the signed distances' adjacency, the sampling table (the functions at the end of this header).  Host memory only.
struct SceneKeep {
    std::vector<uint32_t> tri_order;      // leaf slot -> input triangle
    std::vector<prt_group> groups;
    std::vector<uint32_t> idx_positions, idx_normals;
    std::vector<unsigned int> level_first;   // levels + 1 entries; empty: the tree is not level-ordered (never, for finish_wide's)
    uint32_t position_count = 0, normal_count = 0;
    bool bumped = false;                  // a material has a bump map: the tangent records exist
};

// The arrays as the device will hold them, and what describes them.
struct PackedScene {
    std::vector<uint32_t> nodes;          // the scene's tree, then the shadow trees with their links rebased; node_dwords per node
    std::vector<float4> tris;             // 3 per record: the scene's in leaf order, the all-zero dummy, then each shadow tree's with a dummy of its own
    std::vector<float4> shade;            // 4 per record of the scene (+ dummy)
    std::vector<float4> tri_uv, tri_tan;  // 2 / 3 per record; empty unless textured / bumped
    std::vector<unsigned int> rank;
    std::vector<DevMaterial> materials;
    std::vector<DevLight> lights;         // 2 x light_stride
    std::vector<float4> diffuse_dirs;
    std::vector<DevTexture> textures;
    std::vector<unsigned int> texels;
    std::vector<float> srgb_lut;
    std::vector<float4> ref_spheres;      // empty: the scene came without a usable sphere tree
    std::vector<uint32_t> shadow_rec_tri; // the input triangle of every record behind the scene's own (0xFFFFFFFF: a tree's dummy); host only
    uint32_t light_count = 0, material_count = 0;
    SceneDesc desc;
    SceneKeep keep;
};

struct ScenePackOptions {
    uint32_t leaf_max = 4;
    float sah_trav_cost = 1.0f;
    uint32_t shadow_tree_ratio = 75;      // hundredths of the scene's triangles
    bool normal_cones = true;             // attach_normal_cones on the scene's tree (4-wide only; never on the lights' occluder trees)
    const BvhBuildOptions * bvh = nullptr;
    uint32_t threads = 1;
};

// The description's checks, in prt_upload_scene's order: 0, or the return code with the message in *error.
int check_scene_desc(const prt_scene_desc * s, std::string * error);
// 9 floats per input triangle; refuses (-1, *verts untouched) a coordinate that is not finite or exceeds 1e18.  s has passed the checks.
int unindex_scene(const prt_scene_desc * s, std::vector<float> * verts, std::string * error);

// The reference's visit rank of every input triangle - the leaves of its sphere tree in the order TraceRay pops them (c1
// first), ascending index inside a group - and the tree as the device's near-tie resolution reads it (RefSphereWalk).  Without
// a usable tree (none given, a cycle, a group named twice, triangles left over): input order, and no spheres.
void reference_ranks(const prt_group * groups, uint32_t group_count, const prt_bsphere * spheres, const int32_t * sphere_group,
                     uint32_t sphere_count, uint32_t n_tris, std::vector<uint32_t> & rank_of_input, std::vector<float4> & ref_spheres);

// Every array of a checked description over its un-indexed vertices and a tree built over them (either builder's;
// validate_bvh_links has passed it).  The tree's leaf order moves into out->keep.  0, or the return code with the message in
// *error and *out untouched.  info.bvh_build_ms is the caller's to fill.
int pack_scene(const prt_scene_desc * s, const std::vector<float> & verts, BvhWide && bvh, const ScenePackOptions & opt, PackedScene * out,
               std::string * error);

// ---- the host halves of the tables that later calls build on first use (their device halves are in prt_api.hip)
// leaf slot -> (group, vertex0), + the dummy slot: prt_trace_rays, prt_closest_points
std::vector<uint2> keep_leaf_map(const SceneKeep & k);
// leaf slot -> three position indices, three normal indices (dev_refit.h REFIT_TABLE_WORDS): prt_update_geometry
std::vector<unsigned int> keep_refit_table(const SceneKeep & k);
// leaf slot -> three position indices, three edge ids (the distinct unordered pairs of position indices, numbered in sorted
// order); *edge_count = how many edges there are: prt_signed_distance
std::vector<unsigned int> keep_signed_adjacency(const SceneKeep & k, uint32_t * edge_count);
// (first_index, index_count) per group: the gradient calls
std::vector<unsigned int> keep_group_runs(const SceneKeep & k);
// input triangle -> leaf slot; false: the leaf order is not a permutation: prt_sample_surface
bool keep_slot_of_input(const SceneKeep & k, std::vector<unsigned int> * slot_of_input);

}  // namespace prt
