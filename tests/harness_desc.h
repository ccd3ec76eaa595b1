// harness_desc.h - a prt_scene_desc a host harness owns (tests/*_host_harness.cpp), for the harnesses that hand the product's own
// scene packing (par_raytracer_amd/csrc/scene_pack.h) a description instead of re-typing what the upload does with one.
#pragma once

#include <cstring>
#include <string>
#include <vector>

#include "scene_pack.h"
#include "prt_options.h"

// The arrays a description points into; desc() points a prt_scene_desc at them as they are when it is called.
struct OwnedScene {
    std::vector<float> positions, normals, texcoords, tangents;
    std::vector<uint32_t> idx_positions, idx_texcoords, idx_normals;
    std::vector<prt_group> groups;
    std::vector<prt_material> materials;
    std::vector<prt_texture> textures;
    std::vector<prt_light> lights;
    std::vector<prt_bsphere> spheres;
    std::vector<int32_t> sphere_group;

    prt_scene_desc desc() const {
        prt_scene_desc d;
        memset(&d, 0, sizeof(d));
        d.positions = positions.data(); d.position_count = (uint32_t)(positions.size() / 3);
        d.normals = normals.data(); d.normal_count = (uint32_t)(normals.size() / 3);
        d.texcoords = texcoords.data(); d.texcoord_count = (uint32_t)(texcoords.size() / 2);
        d.tangents = tangents.empty() ? nullptr : tangents.data();
        d.idx_positions = idx_positions.data(); d.idx_texcoords = idx_texcoords.data(); d.idx_normals = idx_normals.data();
        d.index_count = (uint32_t)idx_positions.size();
        d.groups = groups.data(); d.group_count = (uint32_t)groups.size();
        d.materials = materials.data(); d.material_count = (uint32_t)materials.size();
        d.textures = textures.empty() ? nullptr : textures.data(); d.texture_count = (uint32_t)textures.size();
        d.lights = lights.data(); d.light_count = (uint32_t)lights.size();
        d.spheres = spheres.empty() ? nullptr : spheres.data();
        d.sphere_group = sphere_group.empty() ? nullptr : sphere_group.data();
        d.sphere_count = (uint32_t)spheres.size();
        return d;
    }
};

static prt_material plain_material() {
    prt_material m;
    memset(&m, 0, sizeof(m));
    m.specular_intensity = 10.0f; m.index_of_refraction = 1.0f; m.alpha = 1.0f;
    for (int k = 0; k < 3; ++k) { m.ambient_color[k] = 0.1f; m.diffuse_color[k] = 0.7f; m.specular_color[k] = 0.2f; }
    m.ambient_texture = m.diffuse_texture = m.specular_texture = m.alpha_texture = m.bump_texture = -1;
    return m;
}

// A directional light whose shadow rays run along d: the kernels and the upload form the direction as facing * -1.
static prt_light light_towards(const float d[3]) {
    prt_light l;
    memset(&l, 0, sizeof(l));
    l.type = PRT_LIGHT_DIRECTIONAL;
    for (int k = 0; k < 3; ++k) { l.color[k] = 1.0f; l.facing[k] = -d[k]; }
    return l;
}

// Un-indexed triangles (9 floats each) as a description: every corner a position of its own, one normal, one texture
// coordinate, one group, one material, no lights yet.
static OwnedScene flat_scene(const std::vector<float> & verts) {
    OwnedScene s;
    s.positions = verts;
    s.normals = { 0.0f, 1.0f, 0.0f };
    s.texcoords = { 0.0f, 0.0f };
    s.idx_positions.resize(verts.size() / 3);
    for (size_t i = 0; i < s.idx_positions.size(); ++i) s.idx_positions[i] = (uint32_t)i;
    s.idx_texcoords.assign(s.idx_positions.size(), 0u);
    s.idx_normals.assign(s.idx_positions.size(), 0u);
    const prt_group g = { 0u, (uint32_t)s.idx_positions.size(), 0 };
    s.groups.push_back(g);
    s.materials.push_back(plain_material());
    return s;
}

// check, un-index, build the tree of `width` as prt_upload_scene's host builder does, validate, pack: the upload's host half.
// Returns the return code of the step that refused (the message in *error), or 0; *verts gets the un-indexed vertices.
static int pack_as_upload(const prt_scene_desc & d, int width, const prt::ScenePackOptions & how, prt::PackedScene * out, std::vector<float> * verts,
                          std::string * error) {
    if (int rc = prt::check_scene_desc(&d, error)) return rc;
    if (int rc = prt::unindex_scene(&d, verts, error)) return rc;
    const uint32_t n_tris = d.index_count / 3;
    prt::BvhWide bvh;
    prt::build_bvh_wide(width, verts->data(), n_tris, how.leaf_max, how.threads, &bvh, how.sah_trav_cost, how.bvh);
    if (const char * bad = prt::validate_bvh_links(bvh, n_tris)) { *error = bad; return -9; }
    return prt::pack_scene(&d, *verts, std::move(bvh), how, out, error);
}

// The scene's own tree as the packed arrays hold it: the front of the node array, the kept leaf order.
static prt::BvhWide packed_scene_tree(const prt::PackedScene & P) {
    prt::BvhWide t;
    t.node_dwords = P.desc.info.bvh_node_bytes / 4u;
    t.node_count = P.desc.info.bvh_node_count;
    t.max_depth = P.desc.info.bvh_max_depth;
    t.stack_bound = P.desc.stack_bound;
    t.nodes.assign(P.nodes.begin(), P.nodes.begin() + (size_t)t.node_count * t.node_dwords);
    t.tri_order = P.keep.tri_order;
    return t;
}

// A built shadow tree read back out of the shared arrays and moved home again (node 0, record 0): it must pass the checks of a
// tree of its own over *own, the vertices of its records' input triangles.  *rec_base = where its records lie in P.tris.
static prt::BvhWide packed_shadow_tree_home(const prt::PackedScene & P, const std::vector<float> & verts, uint32_t light, std::vector<float> * own,
                                            uint32_t * rec_base) {
    const uint32_t n_rec = P.desc.info.triangle_count + 1u;
    uint32_t base = n_rec;                                     // the trees lie one behind the other, in light order
    for (uint32_t l = 0; l < light; ++l)
        if (P.desc.shadow_info[l].built) base += P.desc.shadow_info[l].triangle_count + 1u;
    const prt_shadow_tree_info & si = P.desc.shadow_info[light];
    prt::BvhWide t;
    t.node_dwords = P.desc.info.bvh_node_bytes / 4u;
    t.node_count = si.node_count;
    t.stack_bound = si.stack_bound;
    t.nodes.assign(P.nodes.begin() + (size_t)si.root * t.node_dwords, P.nodes.begin() + ((size_t)si.root + si.node_count) * t.node_dwords);
    prt::BvhWide home = t;
    prt::rebase_bvh_nodes(t, 0u - si.root, 0u - base, home.nodes.data());
    own->assign((size_t)si.triangle_count * 9, 0.0f);
    for (uint32_t i = 0; i < si.triangle_count; ++i) {
        memcpy(&(*own)[(size_t)i * 9], &verts[(size_t)P.shadow_rec_tri[base - n_rec + i] * 9], 36);
        home.tri_order.push_back(i);
    }
    *rec_base = base;
    return home;
}
