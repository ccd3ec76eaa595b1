// scene_pack.cpp - see scene_pack.h.  Host code only: nothing here calls the HIP runtime.
#include "scene_pack.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>

#include "dev_refit.h"
#include "hammersley.h"
#include "tex_upload.h"

namespace prt {

namespace {

f3 ld3(const float * p) { return mk3(p[0], p[1], p[2]); }

int refuse(std::string * error, int rc, const char * what) {
    *error = what;
    return rc;
}

}  // namespace

int check_scene_desc(const prt_scene_desc * s, std::string * error) {
    if (!s || (s->index_count % 3) != 0) return refuse(error, -1, "prt_upload_scene: null scene or index_count not a multiple of 3");
    if (s->material_count == 0) return refuse(error, -1, "prt_upload_scene: at least one material is required");
    const uint32_t n_tris = s->index_count / 3;
    if (n_tris >= (1u << 26)) return refuse(error, -1, "prt_upload_scene: 2^26 triangles or more (the traversal addresses nodes and triangles by 32-bit byte offsets)");

    // the groups' runs and every index the kernels will follow
    std::vector<uint8_t> covered(n_tris, 0);
    for (uint32_t g = 0; g < s->group_count; ++g) {
        const prt_group & pg = s->groups[g];
        if (pg.first_index % 3 || pg.index_count % 3 || (uint64_t)pg.first_index + pg.index_count > s->index_count)
            return refuse(error, -1, "prt_upload_scene: group index range is not a whole run of triangles inside the index buffers");
        if (pg.material < 0 || (uint32_t)pg.material >= s->material_count) return refuse(error, -1, "prt_upload_scene: group material out of range");
        for (uint32_t t = pg.first_index / 3; t < (pg.first_index + pg.index_count) / 3; ++t) covered[t] = 1;
    }
    for (uint32_t t = 0; t < n_tris; ++t)
        if (!covered[t]) return refuse(error, -1, "prt_upload_scene: triangle not covered by any group");
    for (uint32_t i = 0; i < s->index_count; ++i)
        if (s->idx_positions[i] >= s->position_count || s->idx_normals[i] >= s->normal_count || s->idx_texcoords[i] >= s->texcoord_count)
            return refuse(error, -1, "prt_upload_scene: vertex index out of range (the reference would read out of bounds here)");
    bool textured = false, bumped = false;
    for (uint32_t m = 0; m < s->material_count; ++m) {
        const prt_material & pm = s->materials[m];
        const int32_t slots[5] = { pm.ambient_texture, pm.diffuse_texture, pm.specular_texture, pm.alpha_texture, pm.bump_texture };
        for (int k = 0; k < 5; ++k) {
            if (slots[k] < 0) continue;
            textured = true;
            if (k == 4) bumped = true;
            if (!s->textures || (uint32_t)slots[k] >= s->texture_count) return refuse(error, -1, "prt_upload_scene: material texture slot out of range");
            const prt_texture & t = s->textures[slots[k]];
            // size - 2 is the sampling scale (texture.cpp:63-64): below 2 it wraps around as u32 in the reference
            if (!t.texels || t.size_x < 2 || t.size_y < 2 || t.channels < 1 || t.channels > 4)
                return refuse(error, -1, "prt_upload_scene: texture needs texels, 1..4 channels and at least 2 x 2 texels");
        }
    }
    if (textured && s->texture_count >= DEV_TEX_NONE) return refuse(error, -1, "prt_upload_scene: more than 65534 textures");
    if (bumped && !s->tangents) return refuse(error, -1, "prt_upload_scene: a material has a bump map but the scene has no tangents");
    return 0;
}

int unindex_scene(const prt_scene_desc * s, std::vector<float> * out, std::string * error) {
    const uint32_t n_tris = s->index_count / 3;
    std::vector<float> verts((size_t)n_tris * 9);
    for (uint32_t t = 0; t < n_tris; ++t)
        for (int c = 0; c < 3; ++c) memcpy(&verts[(size_t)t * 9 + 3 * c], s->positions + 3 * (size_t)s->idx_positions[3 * t + c], 12);
    for (size_t i = 0; i < verts.size(); ++i)
        if (!(fabsf(verts[i]) < 1e18f)) return refuse(error, -1, "prt_upload_scene: vertex coordinate is not finite or exceeds 1e18");
    out->swap(verts);
    return 0;
}

void reference_ranks(const prt_group * groups, uint32_t group_count, const prt_bsphere * spheres, const int32_t * sphere_group,
                     uint32_t sphere_count, uint32_t n_tris, std::vector<uint32_t> & rank_of_input, std::vector<float4> & ref_spheres) {
    rank_of_input.assign(n_tris, 0u);
    ref_spheres.clear();
    std::vector<uint32_t> group_base(group_count, 0);
    bool ranked = false;
    if (spheres && sphere_group && sphere_count) {
        std::vector<uint32_t> stack(1, 0u);
        std::vector<uint8_t> seen(group_count, 0);
        std::vector<uint32_t> first_rank(sphere_count, 0), pop_order(sphere_count, 0);
        std::vector<uint8_t> popped(sphere_count, 0);
        uint32_t next = 0, visited = 0;
        bool ok = true;
        while (!stack.empty() && ok) {
            uint32_t i = stack.back();
            stack.pop_back();
            if (i >= sphere_count || ++visited > 2 * sphere_count || popped[i]) { ok = false; break; }
            popped[i] = 1;
            pop_order[i] = visited - 1;
            first_rank[i] = next;                         // the first triangle the reference meets below this sphere
            const prt_bsphere & bs = spheres[i];
            if (bs.c0 && bs.c1) {
                stack.push_back(bs.c0);
                stack.push_back(bs.c1);
            } else {
                int32_t g = sphere_group[i];
                if (g < 0 || (uint32_t)g >= group_count || seen[g]) { ok = false; break; }
                seen[g] = 1;
                group_base[g] = next;
                next += groups[g].index_count / 3;
            }
        }
        ranked = ok && next == n_tris;
        if (ranked) {
            ref_spheres.resize(2 * (size_t)sphere_count, make_float4(0, 0, 0, 0));
            for (uint32_t i = 0; i < sphere_count; ++i) {
                const prt_bsphere & bs = spheres[i];
                ref_spheres[2 * (size_t)i] = make_float4(bs.center[0], bs.center[1], bs.center[2], bs.radius);
                const bool inner = bs.c0 && bs.c1 && popped[i];
                const uint32_t w[4] = { inner ? bs.c0 : 0u, inner ? bs.c1 : 0u, inner ? first_rank[bs.c0] : 0u, pop_order[i] };
                float4 f;
                memcpy(&f, w, 16);
                ref_spheres[2 * (size_t)i + 1] = f;
            }
        }
    }
    if (ranked) {
        for (uint32_t g = 0; g < group_count; ++g) {
            uint32_t first = groups[g].first_index / 3, cnt = groups[g].index_count / 3;
            for (uint32_t k = 0; k < cnt; ++k) rank_of_input[first + k] = group_base[g] + k;
        }
    } else {
        for (uint32_t t = 0; t < n_tris; ++t) rank_of_input[t] = t;
    }
}

int pack_scene(const prt_scene_desc * s, const std::vector<float> & verts, BvhWide && bvh, const ScenePackOptions & opt, PackedScene * out,
               std::string * error) {
    const uint32_t n_tris = s->index_count / 3;
    const int width = bvh.node_dwords == BVH8_NODE_DWORDS ? 8 : 4;
    const uint32_t node_bytes = 4u * bvh.node_dwords;
    PackedScene P;
    SceneDesc & desc = P.desc;

    std::vector<int32_t> tri_material(n_tris, 0);
    for (uint32_t g = 0; g < s->group_count; ++g) {
        const prt_group & pg = s->groups[g];
        for (uint32_t t = pg.first_index / 3; t < (pg.first_index + pg.index_count) / 3; ++t) tri_material[t] = pg.material;
    }
    bool textured = false, bumped = false;
    for (uint32_t m = 0; m < s->material_count; ++m) {
        const prt_material & pm = s->materials[m];
        textured = textured || pm.ambient_texture >= 0 || pm.diffuse_texture >= 0 || pm.specular_texture >= 0 || pm.alpha_texture >= 0 || pm.bump_texture >= 0;
        bumped = bumped || pm.bump_texture >= 0;
    }

    // ---- reference visit rank: leaves of the sphere tree in the order TraceRay pops them (c1 first)
    std::vector<uint32_t> rank_of_input;
    reference_ranks(s->groups, s->group_count, s->spheres, s->sphere_group, s->sphere_count, n_tris, rank_of_input, P.ref_spheres);

    // ---- device records in BVH leaf order
    const uint32_t n_rec = n_tris + 1;                              // + the all-zero dummy triangle empty BVH slots point at
    std::vector<float4> & tris = P.tris, & shade = P.shade, & tri_uv = P.tri_uv, & tri_tan = P.tri_tan;
    tris.assign((size_t)n_rec * 3, make_float4(0, 0, 0, 0));
    shade.assign((size_t)n_rec * 4, make_float4(0, 0, 0, 0));
    P.rank.assign(n_rec, 0);
    tri_uv.assign(textured ? (size_t)n_rec * 2 : 0, make_float4(0, 0, 0, 0));
    tri_tan.assign(bumped ? (size_t)n_rec * 3 : 0, make_float4(0, 0, 0, 0));
    float abs_max = 0.0f;
    // input triangle t's 48-byte record at `slot` of the record array; returns n
    auto put_tri_record = [&](uint32_t t, size_t slot) {
        return tri_record(ld3(&verts[(size_t)t * 9]), ld3(&verts[(size_t)t * 9 + 3]), ld3(&verts[(size_t)t * 9 + 6]), &tris[slot * 3]);
    };
    std::vector<float> rec_normals((size_t)n_tris * 3);          // per INPUT triangle: n as its record holds it (the shadow trees classify by it)
    for (uint32_t slot = 0; slot < n_tris; ++slot) {
        const uint32_t t = bvh.tri_order[slot];
        const f3 n = put_tri_record(t, slot);
        { const float4 stored = tris[(size_t)slot * 3 + 2]; rec_normals[(size_t)t * 3] = stored.y; rec_normals[(size_t)t * 3 + 1] = stored.z; rec_normals[(size_t)t * 3 + 2] = stored.w; }
        const float * n0 = s->normals + 3 * (size_t)s->idx_normals[3 * t + 0];
        const float * n1 = s->normals + 3 * (size_t)s->idx_normals[3 * t + 1];
        const float * n2 = s->normals + 3 * (size_t)s->idx_normals[3 * t + 2];
        const float * u0 = s->texcoords + 2 * (size_t)s->idx_texcoords[3 * t + 0];
        const float * u1 = s->texcoords + 2 * (size_t)s->idx_texcoords[3 * t + 1];
        const float * u2 = s->texcoords + 2 * (size_t)s->idx_texcoords[3 * t + 2];
        float mbits;
        int32_t mi = tri_material[t];
        memcpy(&mbits, &mi, 4);
        shade[(size_t)slot * 4 + 0] = make_float4(n0[0], n0[1], n0[2], n1[0]);
        shade[(size_t)slot * 4 + 1] = make_float4(n1[1], n1[2], n2[0], n2[1]);
        // the geometric normal n = Cross(ab, ac) rides in the shading record too, so a shaded hit costs ONE 64 B
        // gather instead of two; texture coordinates and tangents have their own arrays, only for textured scenes
        shade[(size_t)slot * 4 + 2] = make_float4(n2[2], n.x, n.y, n.z);
        shade[(size_t)slot * 4 + 3] = make_float4(0.0f, 0.0f, 0.0f, mbits);
        if (textured) tex_pack_uv(u0, u1, u2, &tri_uv[(size_t)slot * 2]);              // tex_upload.h
        if (bumped) {                                             // mesh->tangents[idx_normals[...]], raytracer.cpp:470-473
            const float * g0 = s->tangents + 3 * (size_t)s->idx_normals[3 * t + 0];
            const float * g1 = s->tangents + 3 * (size_t)s->idx_normals[3 * t + 1];
            const float * g2 = s->tangents + 3 * (size_t)s->idx_normals[3 * t + 2];
            tex_pack_tangents(g0, g1, g2, &tri_tan[(size_t)slot * 3]);
        }
        P.rank[slot] = rank_of_input[t];
        for (int k = 0; k < 9; ++k) abs_max = std::max(abs_max, fabsf(verts[(size_t)t * 9 + k]));
    }

    P.materials.resize(s->material_count);
    desc.material_ns.resize(s->material_count);
    for (uint32_t m = 0; m < s->material_count; ++m) {
        const prt_material & pm = s->materials[m];
        DevMaterial & d = P.materials[m];
        memset(&d, 0, sizeof(d));
        for (int k = 0; k < 3; ++k) { d.ambient[k] = pm.ambient_color[k]; d.diffuse[k] = pm.diffuse_color[k]; d.specular[k] = pm.specular_color[k]; }
        d.specular_intensity = pm.specular_intensity;
        d.index_of_refraction = pm.index_of_refraction;
        d.alpha = pm.alpha;
        tex_pack_material_slots(pm, d);
        desc.material_ns[m] = pm.specular_intensity;
        if (!(pm.alpha >= 1.0f)) desc.any_translucent = true;      // alpha < 1 (or NaN): continuation rays, unbounded draws
    }
    // textures: RGBA8 by GetTexel's channel rules (texture.cpp:27-41) + the 256 values Color_SRGBToLinear can take
    if (textured) {                                                // tex_upload.h
        if (!tex_expand_rgba8(s->textures, s->texture_count, P.textures, P.texels)) return refuse(error, -1, "prt_upload_scene: more than 2^32 texels");
        tex_fill_srgb_lut(P.srgb_lut);
    }
    desc.kat_textures = P.textures;
    const uint32_t light_stride = std::max(1u, s->light_count);
    std::vector<DevLight> & lights = P.lights;                    // [0, stride): shadow-tree roots in pad; [stride, 2 stride): every root 0
    lights.resize(2 * (size_t)light_stride);
    memset(lights.data(), 0, lights.size() * sizeof(DevLight));
    for (uint32_t l = 0; l < s->light_count; ++l) {
        const prt_light & pl = s->lights[l];
        DevLight & d = lights[l];
        d.type = pl.type;
        for (int k = 0; k < 3; ++k) { d.color[k] = pl.color[k]; d.position[k] = pl.position[k]; d.facing[k] = pl.facing[k]; }
        d.falloff = pl.falloff;
    }
    for (uint32_t l = 0; l < s->light_count; ++l) desc.point_lights = desc.point_lights || s->lights[l].type == PRT_LIGHT_POINT;
    P.diffuse_dirs.resize(1024);
    for (uint32_t i = 0; i < 1024; ++i) P.diffuse_dirs[i] = diffuse_tangent_dir(i);

    // ---- shadow trees (include/prt.h, bvh_build.h): behind the scene's nodes and records, links rebased
    // origins the bounds below cover: a shadow ray starts at (hit + n * bias) + d * bias; the hit is taken to lie within 16 extents of
    // the origin for a camera within 4 and a bias of at most one extent; render_pixels_once holds a call to that
    const double shadow_origin_max = 32.0 * (double)abs_max;
    // ---- normal cones (bvh_build.h): on the scene's tree only - every triangle of a light's occluder tree faces its rays
    if (opt.normal_cones && width == 4 && abs_max > 0.0f) {
        const auto tc = std::chrono::steady_clock::now();
        desc.cone_info.coned_nodes = attach_normal_cones(bvh, rec_normals.data(), n_tris, shadow_origin_max, opt.threads);
        desc.cone_info.attach_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tc).count();
    }
    std::vector<uint32_t> & node_words = P.nodes;
    node_words = std::move(bvh.nodes);
    uint32_t all_nodes = bvh.node_count, all_recs = n_rec;
    unsigned int stack_bound = bvh.stack_bound;
    std::vector<prt_shadow_tree_info> & shadow_info = desc.shadow_info;
    shadow_info.assign(s->light_count, prt_shadow_tree_info());
    uint32_t shadow_trees = 0;
    // open triangles (bvh_build.h): for the same lights, whatever the size rule says about a tree; bit l of the first spare
    // word of a triangle's shading record, the integer's bits in the float
    std::vector<prt_shadow_open_info> & open_info = desc.shadow_open_info;
    open_info.assign(s->light_count, prt_shadow_open_info());
    const ShadowOpenBounds open_bounds = shadow_open_bounds((double)abs_max);
    std::vector<uint32_t> open_mask;                             // per INPUT triangle
    bool any_open = false;
    std::vector<std::vector<uint32_t>> occluder_ids(std::min<uint32_t>(s->light_count, (uint32_t)PRT_MAX_SHADOW_TREES));   // one pass over the normals per light: the tree loop below takes the list
    for (uint32_t l = 0; l < s->light_count && l < (uint32_t)PRT_MAX_SHADOW_TREES && abs_max > 0.0f; ++l) {
        if (s->lights[l].type != 0) continue;
        const auto to = std::chrono::steady_clock::now();
        const float dir[3] = { lights[l].facing[0] * -1.0f, lights[l].facing[1] * -1.0f, lights[l].facing[2] * -1.0f };   // as the kernels form it
        std::vector<uint32_t> & ids = occluder_ids[l];
        shadow_occluders(rec_normals.data(), n_tris, dir, shadow_origin_max, &ids);
        std::vector<uint8_t> open;
        prt_shadow_open_info & oi = open_info[l];
        oi.bias_max = (float)open_bounds.bias_max; oi.reach = (float)open_bounds.reach;
        oi.open_count = shadow_open_flags(verts.data(), rec_normals.data(), n_tris, dir, ids, open_bounds, opt.threads, &open);
        if (oi.open_count) {
            if (open_mask.empty()) open_mask.assign(n_tris, 0u);
            for (uint32_t t = 0; t < n_tris; ++t) open_mask[t] |= (uint32_t)open[t] << l;
            any_open = true;
        }
        oi.classified = 1;
        oi.active = oi.open_count ? 1u : 0u;
        oi.classify_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - to).count();
    }
    if (any_open)
        for (uint32_t slot = 0; slot < n_tris; ++slot) memcpy(&shade[(size_t)slot * 4 + 3].x, &open_mask[bvh.tri_order[slot]], 4);
    for (uint32_t l = 0; l < s->light_count && abs_max > 0.0f; ++l) {
        if (s->lights[l].type != 0 || shadow_trees >= (uint32_t)PRT_MAX_SHADOW_TREES) continue;
        prt_shadow_tree_info & si = shadow_info[l];
        const auto ts = std::chrono::steady_clock::now();
        const float dir[3] = { lights[l].facing[0] * -1.0f, lights[l].facing[1] * -1.0f, lights[l].facing[2] * -1.0f };   // as the kernels form it
        ShadowTreeBuild sb;
        sb.width = width; sb.leaf_max = opt.leaf_max; sb.threads = opt.threads; sb.trav_cost = opt.sah_trav_cost; sb.opt = opt.bvh;
        sb.ratio_percent = opt.shadow_tree_ratio;
        ShadowTreeResult sr;
        std::vector<uint32_t> rec_tri;
        BvhWide sub;
        const char * bad = append_shadow_tree(sb, verts.data(), rec_normals.data(), n_tris, dir, shadow_origin_max, &node_words, all_nodes, all_recs, &rec_tri, &sr, &sub,
                                              l < occluder_ids.size() ? &occluder_ids[l] : nullptr);
        if (!bad && sr.built) bad = validate_bvh_links(sub, sr.triangle_count);
        if (bad) { *error = std::string("prt_upload_scene: the builder produced a broken shadow tree - ") + bad; return -9; }
        si.triangle_count = sr.triangle_count;
        si.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ts).count();
        if (!sr.built) continue;
        tris.resize(((size_t)all_recs + rec_tri.size()) * 3, make_float4(0, 0, 0, 0));
        for (size_t i = 0; i < rec_tri.size(); ++i)
            if (rec_tri[i] != 0xFFFFFFFFu) put_tri_record(rec_tri[i], (size_t)all_recs + i);         // (the tree's own dummy record stays all-zero)
        P.shadow_rec_tri.insert(P.shadow_rec_tri.end(), rec_tri.begin(), rec_tri.end());
        si.built = si.active = 1;
        si.node_count = sr.node_count;
        si.root = sr.root;
        si.stack_bound = sr.stack_bound;
        si.device_bytes = (uint64_t)sr.node_count * node_bytes + (uint64_t)rec_tri.size() * 48u;
        const int root = (int)sr.root;
        memcpy(&lights[l].pad, &root, 4);
        all_nodes += sr.node_count;
        all_recs += (uint32_t)rec_tri.size();
        stack_bound = std::max(stack_bound, sr.stack_bound);
        shadow_trees++;
    }
    for (uint32_t l = 0; l < light_stride; ++l) { lights[light_stride + l] = lights[l]; lights[light_stride + l].pad = 0.0f; }

    P.light_count = s->light_count;
    P.material_count = s->material_count;
    desc.scene_abs_max = abs_max;
    desc.stack_bound = stack_bound;
    desc.shadow_bias_max = abs_max;
    desc.shadow_cam_max = 4.0f * abs_max;
    desc.shadow_open_bias_max = any_open ? (float)open_bounds.bias_max : 0.0f;       // (both exact in float: powers of two times abs_max)
    desc.shadow_open_reach = any_open ? (float)open_bounds.reach : 0.0f;
    desc.light_stride = light_stride;
    desc.shadow_trees_fresh = true;
    desc.textured = textured;
    desc.ref_sphere_bytes = P.ref_spheres.size() * sizeof(float4);
    prt_scene_info & info = desc.info;
    info.triangle_count = n_tris;
    info.bvh_node_count = bvh.node_count;
    info.bvh_max_depth = bvh.max_depth;
    info.bvh_node_bytes = node_bytes;
    info.tri_record_bytes = 48;
    info.shade_record_bytes = 64;
    // (the specular direction table: one sample per material until a render asks for more)
    info.device_bytes = node_words.size() * sizeof(uint32_t) + tris.size() * sizeof(float4) + shade.size() * sizeof(float4) + P.rank.size() * sizeof(unsigned int) +
                        P.materials.size() * sizeof(DevMaterial) + lights.size() * sizeof(DevLight) + P.diffuse_dirs.size() * sizeof(float4) +
                        P.materials.size() * sizeof(float4) + P.textures.size() * sizeof(DevTexture) + P.texels.size() * sizeof(unsigned int) +
                        P.srgb_lut.size() * sizeof(float) + tri_uv.size() * sizeof(float4) + tri_tan.size() * sizeof(float4) + desc.ref_sphere_bytes;

    SceneKeep & keep = P.keep;
    if (!(width == 8 ? refit_level_table<8>(node_words.data(), bvh.node_count, &keep.level_first)      // (the scene's own tree: the array's front)
                     : refit_level_table<4>(node_words.data(), bvh.node_count, &keep.level_first))) keep.level_first.clear();
    keep.tri_order.swap(bvh.tri_order);
    keep.groups.assign(s->groups, s->groups + s->group_count);
    // what a later prt_update_geometry needs
    keep.idx_positions.assign(s->idx_positions, s->idx_positions + s->index_count);
    keep.idx_normals.assign(s->idx_normals, s->idx_normals + s->index_count);
    keep.position_count = s->position_count;
    keep.normal_count = s->normal_count;
    keep.bumped = bumped;
    *out = std::move(P);
    return 0;
}

std::vector<uint2> keep_leaf_map(const SceneKeep & k) {
    const uint32_t n_tris = (uint32_t)k.tri_order.size();
    std::vector<uint2> of_input(n_tris), map((size_t)n_tris + 1, make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu));
    for (uint32_t g = 0; g < (uint32_t)k.groups.size(); ++g) {
        const prt_group & pg = k.groups[g];
        for (uint32_t i = 0; i < pg.index_count / 3; ++i) of_input[pg.first_index / 3 + i] = make_uint2(g, 3u * i);   // IntersectRayMesh's vertex0 = i
    }
    for (uint32_t slot = 0; slot < n_tris; ++slot) map[slot] = of_input[k.tri_order[slot]];
    return map;
}

std::vector<unsigned int> keep_refit_table(const SceneKeep & k) {
    const uint32_t n_tris = (uint32_t)k.tri_order.size();
    std::vector<unsigned int> table((size_t)n_tris * REFIT_TABLE_WORDS);
    for (uint32_t slot = 0; slot < n_tris; ++slot) {
        const uint32_t t = k.tri_order[slot];
        for (uint32_t c = 0; c < 3; ++c) {
            table[(size_t)slot * REFIT_TABLE_WORDS + c] = k.idx_positions[3 * (size_t)t + c];
            table[(size_t)slot * REFIT_TABLE_WORDS + 3 + c] = k.idx_normals[3 * (size_t)t + c];
        }
    }
    return table;
}

std::vector<unsigned int> keep_signed_adjacency(const SceneKeep & k, uint32_t * edge_count) {
    const uint32_t n_tris = (uint32_t)k.tri_order.size();
    // edge ids: the distinct unordered pairs of position indices, numbered in sorted order
    std::vector<uint64_t> keys(3 * (size_t)n_tris);
    for (uint32_t t = 0; t < n_tris; ++t) {
        const uint32_t * v = &k.idx_positions[3 * (size_t)t];
        const uint32_t pair[3][2] = { { v[0], v[1] }, { v[0], v[2] }, { v[1], v[2] } };      // ab, ac, bc
        for (int e = 0; e < 3; ++e)
            keys[3 * (size_t)t + e] = (uint64_t)std::min(pair[e][0], pair[e][1]) << 32 | std::max(pair[e][0], pair[e][1]);
    }
    std::vector<uint64_t> edges(keys);
    std::sort(edges.begin(), edges.end());
    edges.erase(std::unique(edges.begin(), edges.end()), edges.end());
    std::vector<unsigned int> adj(6 * (size_t)n_tris);
    for (uint32_t slot = 0; slot < n_tris; ++slot) {
        const uint32_t t = k.tri_order[slot];
        for (int e = 0; e < 3; ++e) {
            adj[6 * (size_t)slot + e] = k.idx_positions[3 * (size_t)t + e];
            adj[6 * (size_t)slot + 3 + e] = (unsigned int)(std::lower_bound(edges.begin(), edges.end(), keys[3 * (size_t)t + e]) - edges.begin());
        }
    }
    *edge_count = (uint32_t)edges.size();
    return adj;
}

std::vector<unsigned int> keep_group_runs(const SceneKeep & k) {
    std::vector<unsigned int> runs(2 * k.groups.size());
    for (size_t g = 0; g < k.groups.size(); ++g) { runs[2 * g] = k.groups[g].first_index; runs[2 * g + 1] = k.groups[g].index_count; }
    return runs;
}

bool keep_slot_of_input(const SceneKeep & k, std::vector<unsigned int> * slot_of_input) {
    const uint32_t n_tris = (uint32_t)k.tri_order.size();
    slot_of_input->assign(n_tris, 0u);
    for (uint32_t slot = 0; slot < n_tris; ++slot) {
        if (k.tri_order[slot] >= n_tris) return false;
        (*slot_of_input)[k.tri_order[slot]] = slot;
    }
    return true;
}

}  // namespace prt
