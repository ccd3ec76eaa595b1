// scene_pack_host_harness.cpp - the host half of prt_upload_scene (par_raytracer_amd/csrc/scene_pack.cpp) on the host: the checks
// of the description, the un-indexing and the packing, called as the upload calls them (tests/harness_desc.h pack_as_upload), and
// every array they lay out compared with an independent copy - tests/harness_mesh.h's records() and leaf_map(), and the scene
// description itself.  It prints one line per fact and tests/test_scene_pack_host.py asserts on them:
//   case     one line per accepted scene: for every property the number of records, slots or bytes that differ from what the
//            independent copy says (0 everywhere), and the counts that show the case is not vacuous
//   refusal  one line per refused description: the return code, whether the outputs were left untouched, the message
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <vector>

#include "harness_mesh.h"
#include "harness_desc.h"

using namespace prt;

#if defined(PRT_BVH8)
enum { WIDTH = 8 };
#else
enum { WIDTH = 4 };
#endif

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static double rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (double)(g_rng >> 11) / 9007199254740992.0; }

static ScenePackOptions defaults(const BvhBuildOptions * bopt) {
    ScenePackOptions how;                                         // leaf_max 4, trav cost 1, ratio 75: the upload's defaults
    how.threads = 2;
    how.bvh = bopt;
    return how;
}

template <class T>
static bool same_bytes(const std::vector<T> & a, const std::vector<T> & b) {
    return a.size() == b.size() && (a.empty() || !memcmp(a.data(), b.data(), a.size() * sizeof(T)));
}

static bool same_packed(const PackedScene & a, const PackedScene & b) {
    return same_bytes(a.nodes, b.nodes) && same_bytes(a.tris, b.tris) && same_bytes(a.shade, b.shade) && same_bytes(a.tri_uv, b.tri_uv) &&
           same_bytes(a.tri_tan, b.tri_tan) && same_bytes(a.rank, b.rank) && same_bytes(a.materials, b.materials) && same_bytes(a.lights, b.lights) &&
           same_bytes(a.diffuse_dirs, b.diffuse_dirs) && same_bytes(a.textures, b.textures) && same_bytes(a.texels, b.texels) &&
           same_bytes(a.srgb_lut, b.srgb_lut) && same_bytes(a.ref_spheres, b.ref_spheres) && same_bytes(a.keep.tri_order, b.keep.tri_order) &&
           same_bytes(a.keep.level_first, b.keep.level_first) && a.desc.stack_bound == b.desc.stack_bound &&
           a.desc.info.device_bytes == b.desc.info.device_bytes;
}

static uint32_t bits_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

// One accepted scene: pack it, compare everything, print the line.
static void accepted(const char * name, const OwnedScene & S) {
    const prt_scene_desc d = S.desc();
    BvhBuildOptions bopt;
    const ScenePackOptions how = defaults(&bopt);
    PackedScene P, again;
    std::vector<float> verts, verts2;
    std::string error;
    const int rc = pack_as_upload(d, WIDTH, how, &P, &verts, &error);
    if (rc) { printf("case %s width %d | rc %d error %s\n", name, (int)WIDTH, rc, error.c_str()); return; }
    const int rc2 = pack_as_upload(d, WIDTH, how, &again, &verts2, &error);
    const uint32_t n = d.index_count / 3;
    const uint32_t * order = P.keep.tri_order.data();

    // the triangle records: the scene's n + 1 at the front of the array, the dummy all-zero
    const std::vector<float4> expect = mesh::records(verts, n, order);
    unsigned long long records_diff = P.tris.size() < expect.size() ? expect.size() : 0;
    for (size_t i = 0; i < expect.size() && !records_diff; ++i) records_diff += memcmp(&P.tris[i], &expect[i], 16) != 0;
    unsigned long long dummy_nonzero = 0;
    for (int k = 0; k < 3; ++k) { const float4 z = P.tris[(size_t)n * 3 + k]; dummy_nonzero += (bits_of(z.x) | bits_of(z.y) | bits_of(z.z) | bits_of(z.w)) != 0; }
    for (int k = 0; k < 4; ++k) { const float4 z = P.shade[(size_t)n * 4 + k]; dummy_nonzero += (bits_of(z.x) | bits_of(z.y) | bits_of(z.z) | bits_of(z.w)) != 0; }

    // the shading records: three normals, the stored geometric normal, the material's bits; the open flags in the spare word
    std::vector<int32_t> material_of(n, -1);
    for (uint32_t g = 0; g < d.group_count; ++g)
        for (uint32_t t = d.groups[g].first_index / 3; t < (d.groups[g].first_index + d.groups[g].index_count) / 3; ++t) material_of[t] = d.groups[g].material;
    std::vector<float> stored(3 * (size_t)n);                       // per input triangle, out of the independent records
    for (uint32_t slot = 0; slot < n; ++slot) {
        const float4 r2 = expect[(size_t)slot * 3 + 2];
        stored[(size_t)order[slot] * 3] = r2.y; stored[(size_t)order[slot] * 3 + 1] = r2.z; stored[(size_t)order[slot] * 3 + 2] = r2.w;
    }
    std::vector<uint32_t> open_mask(n, 0u);
    unsigned long long open_total = 0;
    float A = 0.0f;
    for (float x : verts) A = fmaxf(A, fabsf(x));
    for (uint32_t l = 0; l < d.light_count && l < (uint32_t)PRT_MAX_SHADOW_TREES && A > 0.0f; ++l) {
        if (d.lights[l].type != PRT_LIGHT_DIRECTIONAL) continue;
        const float dir[3] = { d.lights[l].facing[0] * -1.0f, d.lights[l].facing[1] * -1.0f, d.lights[l].facing[2] * -1.0f };
        std::vector<uint32_t> occ;
        shadow_occluders(stored.data(), n, dir, 32.0 * (double)A, &occ);
        std::vector<uint8_t> open;
        open_total += shadow_open_flags(verts.data(), stored.data(), n, dir, occ, shadow_open_bounds((double)A), 1, &open);
        for (uint32_t t = 0; t < n; ++t) open_mask[t] |= (uint32_t)open[t] << l;
    }
    unsigned long long shade_diff = 0, open_diff = 0;
    for (uint32_t slot = 0; slot < n; ++slot) {
        const uint32_t t = order[slot];
        float want[12];
        for (int c = 0; c < 3; ++c) memcpy(&want[3 * c], d.normals + 3 * (size_t)d.idx_normals[3 * t + c], 12);
        memcpy(&want[9], &stored[(size_t)t * 3], 12);
        shade_diff += memcmp(&P.shade[(size_t)slot * 4], want, 48) != 0;
        const float4 last = P.shade[(size_t)slot * 4 + 3];
        shade_diff += bits_of(last.w) != (uint32_t)material_of[t] || bits_of(last.y) != 0 || bits_of(last.z) != 0;
        open_diff += bits_of(last.x) != open_mask[t];
    }

    // the leaf map and the ranks
    std::vector<uint32_t> runs;
    for (uint32_t g = 0; g < d.group_count; ++g) { runs.push_back(d.groups[g].first_index); runs.push_back(d.groups[g].index_count); }
    const std::vector<uint2> map = keep_leaf_map(P.keep), map_expect = mesh::leaf_map(runs, d.group_count, n, order);
    const unsigned long long leaf_map_diff = same_bytes(map, map_expect) ? 0 : 1;
    std::vector<uint32_t> rank_of_input;
    std::vector<float4> spheres;
    reference_ranks(d.groups, d.group_count, d.spheres, d.sphere_group, d.sphere_count, n, rank_of_input, spheres);
    unsigned long long rank_diff = P.rank.size() != (size_t)n + 1, rank_moved = 0;
    for (uint32_t slot = 0; slot < n && !rank_diff; ++slot) { rank_diff += P.rank[slot] != rank_of_input[order[slot]]; rank_moved += rank_of_input[order[slot]] != order[slot]; }

    // the two light tables: the built trees' roots in the first copy's pad, 0 in the second's
    unsigned long long pad_diff = P.lights.size() != 2 * (size_t)P.desc.light_stride, built = 0, reread_bad = 0, box_violations = 0, refs_diff = 0;
    for (uint32_t l = 0; l < d.light_count && !pad_diff; ++l) {
        const prt_shadow_tree_info & si = P.desc.shadow_info[l];
        pad_diff += bits_of(P.lights[l].pad) != (si.built ? si.root : 0u);
        pad_diff += bits_of(P.lights[P.desc.light_stride + l].pad) != 0u;
        pad_diff += memcmp(&P.lights[l], &P.lights[P.desc.light_stride + l], offsetof(DevLight, pad)) != 0;
        if (!si.built) continue;
        built++;
        std::vector<float> own;
        uint32_t rec_base = 0;
        const BvhWide home = packed_shadow_tree_home(P, verts, l, &own, &rec_base);
        reread_bad += validate_bvh_links(home, si.triangle_count) != nullptr;
        uint64_t out[6] = { 0, 0, 0, 0, 0, 0 };
        if (si.triangle_count) check_bvh_wide(own.data(), si.triangle_count, home, out);
        box_violations += out[0];
        refs_diff += out[5] != si.triangle_count;
    }
    const char * scene_bad = validate_bvh_links(packed_scene_tree(P), n);

    // device_bytes: the sum of the array sizes, the one-sample specular table (16 B per material) among them
    const unsigned long long bytes = P.nodes.size() * 4ull + (P.tris.size() + P.shade.size() + P.tri_uv.size() + P.tri_tan.size() + P.diffuse_dirs.size() +
                                     P.ref_spheres.size() + P.materials.size()) * 16ull + P.rank.size() * 4ull + P.materials.size() * sizeof(DevMaterial) +
                                     P.lights.size() * sizeof(DevLight) + P.textures.size() * sizeof(DevTexture) + P.texels.size() * 4ull + P.srgb_lut.size() * 4ull;
    printf("case %s width %d | rc 0 triangles %u records_diff %llu dummy_nonzero %llu shade_diff %llu open_diff %llu open %llu leaf_map_diff %llu rank_diff %llu "
           "rank_moved %llu pad_diff %llu trees %llu reread_bad %llu box_violations %llu refs_diff %llu validate %s bytes_diff %lld repack_same %d "
           "textured %d bumped %d uv %zu tan %zu textures %zu spheres %zu point_lights %d translucent %d rank_of_first %u\n",
           name, (int)WIDTH, n, records_diff, dummy_nonzero, shade_diff, open_diff, open_total, leaf_map_diff, rank_diff, rank_moved, pad_diff, built, reread_bad,
           box_violations, refs_diff, scene_bad ? "bad" : "null", (long long)(P.desc.info.device_bytes - bytes), (int)(rc2 == 0 && same_packed(P, again)),
           (int)P.desc.textured, (int)P.keep.bumped, P.tri_uv.size(), P.tri_tan.size(), P.textures.size(), P.ref_spheres.size(), (int)P.desc.point_lights,
           (int)P.desc.any_translucent, n ? rank_of_input[0] : 0u);
}

// ---- the scenes

static OwnedScene empty_scene() { return flat_scene(std::vector<float>()); }

static OwnedScene one_triangle() { return flat_scene({ 0, 0, 0,  1, 0, 0,  0, 0, 1 }); }

// 12 triangles, 8 shared positions, 6 face normals, two groups with a material each, the reference's sphere tree over the groups,
// one directional and one point light.
static OwnedScene cube() {
    OwnedScene s;
    for (int i = 0; i < 8; ++i) { s.positions.push_back(i & 1 ? 1.0f : -1.0f); s.positions.push_back(i & 2 ? 1.0f : -1.0f); s.positions.push_back(i & 4 ? 1.0f : -1.0f); }
    const float fn[6][3] = { { -1, 0, 0 }, { 1, 0, 0 }, { 0, -1, 0 }, { 0, 1, 0 }, { 0, 0, -1 }, { 0, 0, 1 } };
    const uint32_t quad[6][4] = { { 0, 4, 6, 2 }, { 1, 3, 7, 5 }, { 0, 1, 5, 4 }, { 2, 6, 7, 3 }, { 0, 2, 3, 1 }, { 4, 5, 7, 6 } };   // outward
    for (int f = 0; f < 6; ++f) {
        s.normals.insert(s.normals.end(), fn[f], fn[f] + 3);
        const uint32_t tri[6] = { quad[f][0], quad[f][1], quad[f][2], quad[f][0], quad[f][2], quad[f][3] };
        for (int k = 0; k < 6; ++k) { s.idx_positions.push_back(tri[k]); s.idx_normals.push_back((uint32_t)f); s.idx_texcoords.push_back(0u); }
    }
    s.texcoords = { 0.0f, 0.0f };
    const prt_group g0 = { 0u, 15u, 1 }, g1 = { 15u, 21u, 0 };
    s.groups = { g0, g1 };
    s.materials = { plain_material(), plain_material() };
    s.materials[1].alpha = 0.5f;
    const float d[3] = { 0.35f, 1.0f, 0.2f };
    s.lights.push_back(light_towards(d));
    prt_light p = light_towards(d);
    p.type = PRT_LIGHT_POINT; p.position[1] = 5.0f; p.falloff = 0.01f;
    s.lights.push_back(p);
    const prt_bsphere root = { { 0, 0, 0 }, 2.0f, 1u, 2u }, a = { { 0, 0, 0 }, 2.0f, 0u, 0u };
    s.spheres = { root, a, a };
    s.sphere_group = { -1, 0, 1 };                                 // c1 is popped first: group 1's triangles get the low ranks
    return s;
}

static const uint8_t g_texels[2 * 2 * 3] = { 255, 0, 0,  0, 255, 0,  0, 0, 255,  128, 128, 128 };
static const uint8_t g_bump[2 * 2] = { 0, 64, 128, 255 };

// Two triangles with a 2 x 2 texture in the diffuse slot and a bump map: the uv and tangent records exist.
static OwnedScene textured_quad() {
    OwnedScene s;
    s.positions = { 0, 0, 0,  1, 0, 0,  1, 0, 1,  0, 0, 1 };
    s.normals = { 0, 1, 0,  0.1f, 0.9f, 0,  0, 0.9f, 0.1f };
    s.tangents = { 1, 0, 0,  0.9f, 0.1f, 0,  0.9f, 0, 0.1f };
    s.texcoords = { 0, 0,  1, 0,  1, 1,  0, 1 };
    s.idx_positions = { 0, 2, 1,  0, 3, 2 };
    s.idx_texcoords = { 0, 2, 1,  0, 3, 2 };
    s.idx_normals = { 0, 1, 2,  2, 1, 0 };
    const prt_group g = { 0u, 6u, 0 };
    s.groups = { g };
    s.materials = { plain_material() };
    s.materials[0].diffuse_texture = 0;
    s.materials[0].bump_texture = 1;
    const prt_texture t0 = { 2u, 2u, 3u, g_texels }, t1 = { 2u, 2u, 1u, g_bump };
    s.textures = { t0, t1 };
    const float d[3] = { 0.0f, 1.0f, 0.0f };
    s.lights.push_back(light_towards(d));
    return s;
}

// A closed mesh of 2 * SEG * (RINGS - 1) triangles: a sphere of RINGS x SEG quads whose vertices are moved along their radius by
// the seeded generator (it stays closed and star-shaped), in two groups, with vertex normals, under two directional lights.
// About half of it faces away from either light - the occluders, under the 75 % of the default size rule - and the lit side of a
// star-shaped body is mostly open.
static OwnedScene seeded_closed_mesh() {
    enum { RINGS = 10, SEG = 16 };
    OwnedScene s;
    auto put = [&](double theta, double phi) {
        const float r = 1.0f + 0.25f * (float)rnd();
        const float p[3] = { r * (float)(sin(theta) * cos(phi)), r * (float)cos(theta), r * (float)(sin(theta) * sin(phi)) };
        s.positions.insert(s.positions.end(), p, p + 3);
        const float inv = 1.0f / r;
        const float nn[3] = { p[0] * inv, p[1] * inv, p[2] * inv };
        s.normals.insert(s.normals.end(), nn, nn + 3);
    };
    put(0.0, 0.0);                                                 // vertex 0: the north pole; then RINGS - 1 rings; last: the south pole
    for (int i = 1; i < RINGS; ++i)
        for (int j = 0; j < SEG; ++j) put(3.14159265358979 * i / RINGS, 6.28318530717959 * j / SEG);
    put(3.14159265358979, 0.0);
    const uint32_t south = (uint32_t)(s.positions.size() / 3 - 1);
    auto ring = [&](int i, int j) { return 1u + (uint32_t)(i - 1) * SEG + (uint32_t)(j % SEG); };
    auto tri = [&](uint32_t a, uint32_t b, uint32_t c) { const uint32_t v[3] = { a, b, c }; s.idx_positions.insert(s.idx_positions.end(), v, v + 3); };
    for (int j = 0; j < SEG; ++j) tri(0u, ring(1, j + 1), ring(1, j));
    for (int i = 1; i < RINGS - 1; ++i)
        for (int j = 0; j < SEG; ++j) { tri(ring(i, j), ring(i, j + 1), ring(i + 1, j)); tri(ring(i, j + 1), ring(i + 1, j + 1), ring(i + 1, j)); }
    for (int j = 0; j < SEG; ++j) tri(south, ring(RINGS - 1, j), ring(RINGS - 1, j + 1));
    s.idx_normals = s.idx_positions;
    s.texcoords = { 0.0f, 0.0f };
    s.idx_texcoords.assign(s.idx_positions.size(), 0u);
    const uint32_t half = (uint32_t)(s.idx_positions.size() / 6) * 3u;
    const prt_group g0 = { 0u, half, 0 }, g1 = { half, (uint32_t)s.idx_positions.size() - half, 1 };
    s.groups = { g0, g1 };
    s.materials = { plain_material(), plain_material() };
    const float sun[3] = { 0.35f, 1.0f, 0.2f }, low[3] = { -0.8f, 0.25f, 0.1f };
    s.lights = { light_towards(sun), light_towards(low) };
    return s;
}

// ---- the refusals: the cube with one thing wrong at a time

static void refusal(const char * name, const prt_scene_desc * d) {
    std::string error = "untouched";
    std::vector<float> verts(7, 42.0f);
    int rc = check_scene_desc(d, &error);
    if (!rc) rc = unindex_scene(d, &verts, &error);
    const bool untouched = verts == std::vector<float>(7, 42.0f);
    printf("refusal %s | rc %d untouched %d message %s\n", name, rc, (int)untouched, error.c_str());
}

static void refusals() {
    const OwnedScene base = cube();
    refusal("null_scene", nullptr);
    { prt_scene_desc d = base.desc(); d.index_count = 35; refusal("index_count", &d); }
    { prt_scene_desc d = base.desc(); d.material_count = 0; refusal("no_material", &d); }
    { prt_scene_desc d = base.desc(); d.index_count = 3u << 26; refusal("triangle_cap", &d); }
    { OwnedScene s = base; s.groups[0].first_index = 1; s.groups[0].index_count = 12; prt_scene_desc d = s.desc(); refusal("group_first", &d); }
    { OwnedScene s = base; s.groups[1].index_count = 20; prt_scene_desc d = s.desc(); refusal("group_count", &d); }
    { OwnedScene s = base; s.groups[1].index_count = 24; prt_scene_desc d = s.desc(); refusal("group_past_end", &d); }
    { OwnedScene s = base; s.groups[1].first_index = 0xFFFFFFFCu; s.groups[1].index_count = 6; prt_scene_desc d = s.desc(); refusal("group_wraps", &d); }
    { OwnedScene s = base; s.groups[0].material = -1; prt_scene_desc d = s.desc(); refusal("material_negative", &d); }
    { OwnedScene s = base; s.groups[0].material = 2; prt_scene_desc d = s.desc(); refusal("material_past_end", &d); }
    { OwnedScene s = base; s.groups[1].first_index = 18; s.groups[1].index_count = 18; prt_scene_desc d = s.desc(); refusal("uncovered", &d); }
    { OwnedScene s = base; s.idx_positions[7] = 8; prt_scene_desc d = s.desc(); refusal("position_index", &d); }
    { OwnedScene s = base; s.idx_normals[35] = 6; prt_scene_desc d = s.desc(); refusal("normal_index", &d); }
    { OwnedScene s = base; s.idx_texcoords[0] = 1; prt_scene_desc d = s.desc(); refusal("texcoord_index", &d); }
    { OwnedScene s = base; s.materials[0].specular_texture = 0; prt_scene_desc d = s.desc(); refusal("texture_slot_no_table", &d); }
    const OwnedScene quad = textured_quad();
    { OwnedScene s = quad; s.materials[0].alpha_texture = 2; prt_scene_desc d = s.desc(); refusal("texture_slot_past_end", &d); }
    { OwnedScene s = quad; s.textures[0].texels = nullptr; prt_scene_desc d = s.desc(); refusal("texture_no_texels", &d); }
    { OwnedScene s = quad; s.textures[0].size_y = 1; prt_scene_desc d = s.desc(); refusal("texture_one_row", &d); }
    { OwnedScene s = quad; s.textures[1].channels = 0; prt_scene_desc d = s.desc(); refusal("texture_no_channels", &d); }
    { OwnedScene s = quad; s.textures[1].channels = 5; prt_scene_desc d = s.desc(); refusal("texture_five_channels", &d); }
    { OwnedScene s = quad; s.textures.resize(65535, s.textures[0]); prt_scene_desc d = s.desc(); refusal("texture_count", &d); }
    { OwnedScene s = quad; s.tangents.clear(); prt_scene_desc d = s.desc(); refusal("bump_without_tangents", &d); }
    { OwnedScene s = base; s.positions[4] = INFINITY; prt_scene_desc d = s.desc(); refusal("coordinate_inf", &d); }
    { OwnedScene s = base; s.positions[4] = NAN; prt_scene_desc d = s.desc(); refusal("coordinate_nan", &d); }
    { OwnedScene s = base; s.positions[23] = -1e18f; prt_scene_desc d = s.desc(); refusal("coordinate_1e18", &d); }
    // the controls: what is refused above passes untouched, and so does a coordinate just inside the rule
    { prt_scene_desc d = base.desc(); refusal("control_cube", &d); }
    { prt_scene_desc d = quad.desc(); refusal("control_quad", &d); }
    { OwnedScene s = base; s.positions[23] = -9.9e17f; prt_scene_desc d = s.desc(); refusal("control_9e17", &d); }
}

int main() {
    accepted("empty", empty_scene());
    accepted("one_triangle", one_triangle());
    accepted("cube", cube());
    accepted("textured_quad", textured_quad());
    accepted("closed_mesh", seeded_closed_mesh());
    refusals();
    return 0;
}
