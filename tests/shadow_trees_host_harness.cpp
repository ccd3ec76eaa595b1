// shadow_trees_host_harness.cpp - the shadow trees of a directional light (par_raytracer_amd/csrc/bvh_build.h) on the host: the
// classification, the trees as prt_upload_scene appends them behind the scene's (pack_scene of scene_pack.cpp, the very function
// it calls) and the device traversal (dev_trace*.h through tests/hip_shim, one lane at a time) started at their roots.  It prints
// one line per fact and tests/test_shadow_trees_host.py asserts on them:
//   exclusion  no excluded triangle ever has the device's dd = Dot(o - (o + d), n) > 0: random origins, origins on the
//              surface, origins 4 x outside the bounds, origins at the bound and next to powers of two, for the scene scaled by
//              2^-20, 1, 2^10, 2^14, 2^17 and 2^20; the normal is the one read back out of the record
//   margin     synthetic normals swept through the rule's margin, origins at +-M: see margin_sweep
//   edge       triangles edge-on to the light (dot == 0 exactly, and one ulp either side), of zero area, with a normal that is
//              huge or not finite: kept, or dead for every origin tried
//   brute      for thousands of shadow rays started as a render starts them, hit / miss of the light's tree == hit / miss of a
//              loop over ALL triangles with the hot loop's tri_test == hit / miss of the scene's tree
//   links      validate_bvh_links and check_bvh_wide pass on every appended tree, read back out of the shared arrays, for a
//              scene with 0, 1 and 2 directional lights and for an empty set (a plane that faces its light)
//
//   g++ -O1 -std=c++17 -ffp-contract=off -Itests/hip_shim -Ipar_raytracer_amd/csrc [-DPRT_BVH8] tests/shadow_trees_host_harness.cpp
//       par_raytracer_amd/csrc/scene_pack.cpp par_raytracer_amd/csrc/bvh_build.cpp par_raytracer_amd/csrc/bvh_check.cpp -pthread -o /tmp/st && /tmp/st
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "harness_mesh.h"
#include "harness_desc.h"
#include "harness_scene.h"

using namespace prt;

#if defined(PRT_BVH8)
enum { WIDTH = 8 };
#else
enum { WIDTH = 4 };
#endif

static void put_record(std::vector<float4> & tris, size_t slot, const float * v) {           // prt_upload_scene's own function
    tri_record(mk3(v[0], v[1], v[2]), mk3(v[3], v[4], v[5]), mk3(v[6], v[7], v[8]), &tris[slot * 3]);
}

static float abs_max_of(const std::vector<float> & v) { float m = 0.0f; for (float x : v) m = fmaxf(m, fabsf(x)); return m; }

// The normal as the record of triangle tri9 holds it: written by put_record, read back out of the record.
static void stored_normal(const float * tri9, float n[3]) {
    std::vector<float4> rec(3);
    put_record(rec, 0, tri9);
    n[0] = rec[2].y; n[1] = rec[2].z; n[2] = rec[2].w;
}
static std::vector<float> stored_normals(const std::vector<float> & verts) {
    std::vector<float> n(verts.size() / 3);
    for (size_t t = 0; t < verts.size() / 9; ++t) stored_normal(&verts[t * 9], &n[t * 3]);
    return n;
}

// The device's dd for origin o, direction d and a stored normal.
static float device_dd(f3 o, f3 d, const float n[3]) {
    const f3 qp = o - (o + d);                               // raytracer.cpp:88-89, dev_trace4.h trav_leaf
    return dot3(qp, mk3(n[0], n[1], n[2]));
}

// Origins for one triangle: k-th of a fixed family.  A = the scene's largest |coordinate|, M = the bound's origin_max.
static f3 origin_for(int k, const float * t, float A, float M, f3 d) {
    const f3 a = mk3(t[0], t[1], t[2]), b = mk3(t[3], t[4], t[5]), c = mk3(t[6], t[7], t[8]);
    const float u = (float)rnd(), v = (float)rnd() * (1.0f - u);
    const f3 on = a + (b - a) * u + (c - a) * v;
    switch (k % 8) {
    case 0: return mk3((float)(rnd() * 2 - 1) * A, (float)(rnd() * 2 - 1) * A, (float)(rnd() * 2 - 1) * A);            // inside the bounds
    case 1: return on;                                                                                                // on the surface
    case 2: return on + normalize3(cross3(b - a, c - a)) * (A * 1e-4f) + d * (A * 1e-4f);                             // ... biased as a render does
    case 3: return mk3((float)(rnd() * 2 - 1) * 4.0f * A, (float)(rnd() * 2 - 1) * 4.0f * A, (float)(rnd() * 2 - 1) * 4.0f * A);   // 4 x outside
    case 4: return mk3(rnd() < 0.5 ? M : -M, rnd() < 0.5 ? M : -M, rnd() < 0.5 ? M : -M);                             // at the bound
    case 5: {                                                                                                         // next to a power of two: o + d crosses a binade
        const float p = ldexpf(1.0f, (int)(rnd() * 8) + ilogbf(fmaxf(A, 1e-30f)) - 5);
        f3 o = mk3(p, -p, p);
        o.x = nextafterf(o.x, rnd() < 0.5 ? 0.0f : 2.0f * p); o.y = nextafterf(o.y, rnd() < 0.5 ? 0.0f : -2.0f * p);
        return o - d * (float)rnd();
    }
    case 6: return d * (float)((rnd() * 2 - 1) * M / fmax(1e-30, fmax(fabs(d.x), fmax(fabs(d.y), fabs(d.z)))));      // along the light
    default: return mk3(0.0f, (float)(rnd() * 2 - 1) * M, -0.0f);
    }
}

struct Scene {
    std::vector<float> verts;
    PackedScene P;                                               // as prt_upload_scene lays it out (scene_pack.h)
    uint32_t n_tris = 0, node_count = 0, stack_bound = 0;
    struct Tree { prt_shadow_tree_info r; uint32_t rec_base; f3 d; };
    std::vector<Tree> trees;
};

// prt_upload_scene's host half (tests/harness_desc.h pack_as_upload: check, un-index, tree, pack) on the triangles of S under
// one directional light per direction: the scene's tree and records, then one tree per light behind them.  Prints the links lines.
static void upload(Scene & S, const char * name, const std::vector<f3> & dirs, uint32_t ratio) {
    OwnedScene owned = flat_scene(S.verts);
    for (const f3 & dv : dirs) { const float d[3] = { dv.x, dv.y, dv.z }; owned.lights.push_back(light_towards(d)); }
    BvhBuildOptions bopt;
    ScenePackOptions how;
    how.leaf_max = 4; how.threads = 2; how.sah_trav_cost = 1.0f; how.shadow_tree_ratio = ratio; how.bvh = &bopt;
    std::string error;
    std::vector<float> verts;
    const int rc = pack_as_upload(owned.desc(), WIDTH, how, &S.P, &verts, &error);
    const char * append = rc ? error.c_str() : "null";           // a broken shadow tree refuses the whole upload
    S.n_tris = (uint32_t)(S.verts.size() / 9);
    S.node_count = S.P.desc.info.bvh_node_count;
    S.stack_bound = S.P.desc.stack_bound;
    printf("links %s width %d lights %zu | scene validate %s\n", name, (int)WIDTH, dirs.size(), rc || validate_bvh_links(packed_scene_tree(S.P), S.n_tris) ? "bad" : "null");
    for (size_t l = 0; l < dirs.size() && !rc; ++l) {
        Scene::Tree T;
        T.d = dirs[l];
        T.r = S.P.desc.shadow_info[l];
        T.rec_base = 0;
        uint64_t out[6] = { 0, 0, 0, 0, 0, 0 };
        const char * reread = "skipped";
        if (T.r.built) {
            // the tree read back out of the shared arrays: moved home again it must pass the checks of a tree of its own
            std::vector<float> own;
            const BvhWide home = packed_shadow_tree_home(S.P, verts, (uint32_t)l, &own, &T.rec_base);
            reread = validate_bvh_links(home, T.r.triangle_count) ? "bad" : "null";
            if (T.r.triangle_count) check_bvh_wide(own.data(), T.r.triangle_count, home, out);
        }
        printf("links %s width %d light %zu | built %u occluders %u of %u nodes %u root %u append %s reread %s violations %llu refs %llu\n", name, (int)WIDTH, l,
               T.r.built, T.r.triangle_count, S.n_tris, T.r.node_count, T.r.root, append, reread,
               (unsigned long long)out[0], (unsigned long long)out[5]);
        S.trees.push_back(T);
    }
}

// Shadow rays as a render starts them (kernels_wave.h shade_entry_on): from a point of the surface, off along the normal and the
// light by the bias.  Hit / miss of the light's tree, of the scene's tree and of a loop over every triangle.
static void brute(const Scene & S, const char * name, int n_rays) {
    mesh::Walk lane(S.P.nodes.data(), S.node_count, S.P.tris, S.n_tris, S.stack_bound);
    const DevScene & sc = lane.sc;
    GlobalStack & stk = lane.stk;
    const float A = abs_max_of(S.verts), pad = A * (1.0f / 65536.0f), bias = 1e-3f;
    for (size_t l = 0; l < S.trees.size(); ++l) {
        const Scene::Tree & T = S.trees[l];
        unsigned long long mism_tree = 0, mism_scene = 0, hits = 0, nodes_tree = 0, nodes_scene = 0;
        for (int k = 0; k < n_rays; ++k) {
            const float * t = &S.verts[(size_t)(uint32_t)(rnd() * S.n_tris) * 9];
            const f3 a = mk3(t[0], t[1], t[2]), b = mk3(t[3], t[4], t[5]), c = mk3(t[6], t[7], t[8]);
            const float u = (float)rnd(), v = (float)rnd() * (1.0f - u);
            f3 gn = normalize3(cross3(b - a, c - a));
            if (k % 7 == 3) gn = gn * -1.0f;                                   // now and then from the back side
            const f3 o = (a + (b - a) * u + (c - a) * v) + gn * bias;
            const f3 ob = o + T.d * bias;                                      // raytracer.cpp:163
            const f3 qp = ob - (ob + T.d);
            bool any = false;
            for (uint32_t s = 0; s < S.n_tris && !any; ++s) {
                const float4 r0 = S.P.tris[3 * (size_t)s], r1 = S.P.tris[3 * (size_t)s + 1], r2 = S.P.tris[3 * (size_t)s + 2];
                float ht, hv, hw;
                bool near;
                any = tri_test(ob, T.d, qp, mk3(r0.x, r0.y, r0.z), mk3(r0.w, r1.x, r1.y), mk3(r1.z, r1.w, r2.x), mk3(r2.y, r2.z, r2.w),
                               3.402823466e+38f, ht, hv, hw, near);
            }
            TraceStats s0, s1;
            const HitRec h0 = trace_ray<GlobalStack, true>(sc, ob, T.d, TRACE_ANY, pad, stk, s0);
            const HitRec h1 = T.r.built ? trace_ray<GlobalStack, true>(sc, ob, T.d, TRACE_ANY, pad, stk, s1, (int)T.r.root) : h0;
            if ((h0.tri >= 0) != any) mism_scene++;
            if ((h1.tri >= 0) != any) mism_tree++;
            if (h1.tri >= 0 && T.r.built && (uint32_t)h1.tri < T.rec_base) mism_tree++;             // a hit outside the tree's own records
            hits += any;
            nodes_scene += s0.nodes; nodes_tree += s1.nodes;
        }
        printf("brute %s width %d light %zu | rays %d hits %llu tree_mismatches %llu scene_mismatches %llu node_visits %llu -> %llu\n", name, (int)WIDTH, l,
               n_rays, hits, mism_tree, mism_scene, nodes_scene, nodes_tree);
    }
}

static void exclusion(const char * name, const std::vector<float> & base, int scale_exp, f3 d, int per_tri) {
    std::vector<float> verts = base;
    for (float & x : verts) x = ldexpf(x, scale_exp);                              // exact
    const uint32_t n = (uint32_t)(verts.size() / 9);
    const float A = abs_max_of(verts), M = 32.0f * A;
    const float dd3[3] = { d.x, d.y, d.z };
    unsigned long long excluded = 0, tried = 0, violations = 0;
    const std::vector<float> normals = stored_normals(verts);
    // decided: triangles whose membership the M-dependent term of the margin decides - left out, but kept were the rounding
    // term E = u (M + 2 D) four times as large - so that a scale passes on the strength of that term or not at all
    unsigned long long decided = 0;
    for (uint32_t t = 0; t < n; ++t) {
        const float * nt = &normals[(size_t)t * 3];
        if (!shadow_tri_excluded(nt, dd3, 32.0 * (double)A)) continue;
        excluded++;
        if (!shadow_tri_excluded(nt, dd3, 4.0 * 32.0 * (double)A)) decided++;
        for (int k = 0; k < per_tri; ++k) {
            const f3 o = origin_for(k, &verts[(size_t)t * 9], A, M, d);
            tried++;
            if (device_dd(o, d, nt) > 0.0f) violations++;
        }
    }
    printf("exclusion %s scale 2^%d | triangles %u excluded %llu decided %llu origins %llu violations %llu\n", name, scale_exp, n, excluded, decided, tried, violations);
}

// Triangles at the edge of the rule, light from straight above (facing (0, -1, 0), d = (0, 1, 0)).
static void edges() {
    const f3 d = mk3(0.0f, 1.0f, 0.0f);
    const float dd3[3] = { 0.0f, 1.0f, 0.0f };
    struct Case { const char * name; float v[9]; };
    std::vector<Case> cases;
    // vertical walls: n has no y component at all
    cases.push_back({ "edge_on_x", { 1, 0, 0,  1, 1, 0,  1, 0, 1 } });
    cases.push_back({ "edge_on_skew", { 0.3f, 0.1f, 0.7f,  0.3f + 0.25f, 0.9f, 0.7f + 0.5f,  0.3f + 0.5f, 0.2f, 0.7f + 1.0f } });
    for (int s = -1; s <= 1; s += 2) {                           // ... and one ulp of one coordinate either side of it
        Case c = { s < 0 ? "edge_on_minus_ulp" : "edge_on_plus_ulp", { 1, 0, 0,  1, 1, 0.5f,  1, 0, 1 } };   // n.y = ab.z * ac.x = -+ half an ulp
        c.v[6] = nextafterf(1.0f, s < 0 ? 0.0f : 2.0f);
        cases.push_back(c);
    }
    cases.push_back({ "zero_area_point", { 2, 2, 2,  2, 2, 2,  2, 2, 2 } });
    cases.push_back({ "zero_area_line", { 0, 0, 0,  1, 1, 1,  2, 2, 2 } });
    cases.push_back({ "huge_normal", { 0, 0, 0,  0, 0, 1e17f,  1e17f, 0, 0 } });
    cases.push_back({ "inf_normal", { 0, 0, 0,  0, 0, 3e30f,  3e30f, 0, 0 } });
    cases.push_back({ "nan_normal", { 0, 0, 0,  3e30f, 0, 3e30f,  3e30f, 0, 3e30f } });
    cases.push_back({ "tiny_normal", { 0, 0, 0,  0, 0, 1e-25f,  1e-25f, 0, 0 } });
    cases.push_back({ "faces_light", { 0, 0, 0,  0, 0, 1,  1, 0, 0 } });              // n = (0, 1, 0): the one that must go
    cases.push_back({ "faces_away", { 0, 0, 0,  1, 0, 0,  0, 0, 1 } });
    for (const Case & c : cases) {
        float n[3];
        stored_normal(c.v, n);
        const bool excluded = shadow_tri_excluded(n, dd3, 32.0 * 4.0);
        unsigned long long alive = 0;
        for (int k = 0; k < 4000; ++k) {
            const f3 o = origin_for(k, c.v, 4.0f, 128.0f, d);
            if (device_dd(o, d, n) > 0.0f) alive++;
        }
        printf("edge %s | excluded %d alive_origins %llu n %g %g %g\n", c.name, (int)excluded, alive, n[0], n[1], n[2]);
    }
}

// Normals at the margin itself.  For a light direction d and an origin bound M the rule leaves a normal out iff
// d.n >= N1 * margin(M, D).  Synthetic normals n = t + s * c, t perpendicular to d and c along it, with s swept through the
// margin in fine steps: every normal the rule leaves out is put through the device expression with origins whose components
// are +-M, +-M next to a binade, and +-M / 2 - where fl(o + d) rounds the most - in all sign patterns; and the sweep must find
// both verdicts, so that the boundary really lies inside it.  A constant too small in shadow_tri_excluded shows as a violation.
static void margin_sweep(const char * name, f3 d, float M) {
    const float dd3[3] = { d.x, d.y, d.z };
    const f3 c = d, t = normalize3(cross3(d, fabsf(d.x) < 0.9f ? mk3(1, 0, 0) : mk3(0, 1, 0)));
    const double u = 5.9604644775390625e-8, D = fmax(fabs(d.x), fmax(fabs(d.y), fabs(d.z)));
    const double E = u * ((double)M + 2.0 * D);
    unsigned long long out_n = 0, in_n = 0, tried = 0, violations = 0, alive_kept = 0;
    for (int i = -400; i <= 400; ++i) {
        const float s = (float)(E * 2.0 * (1.0 + i / 200.0));                     // s from -2 E to 6 E: the margin is ~E (1 + small) x N1 / |n|
        for (int scale = -3; scale <= 3; scale += 3) {
            const f3 nv = (t + c * s) * ldexpf(1.0f, 4 * scale);
            const float n[3] = { nv.x, nv.y, nv.z };
            const bool excluded = shadow_tri_excluded(n, dd3, (double)M);
            (excluded ? out_n : in_n)++;
            for (int k = 0; k < 64; ++k) {
                float o[3];
                for (int a = 0; a < 3; ++a) {
                    const float m = (k >> 3) % 3 == 0 ? M : (k >> 3) % 3 == 1 ? nextafterf(ldexpf(1.0f, ilogbf(M)), k & 32 ? 0.0f : 2.0f * M) : 0.5f * M + (float)rnd() * 0.5f * M;
                    o[a] = (k >> a & 1) ? -m : m;
                }
                const float dd = device_dd(mk3(o[0], o[1], o[2]), d, n);
                if (excluded) { tried++; if (dd > 0.0f) violations++; }
                else if (dd > 0.0f) alive_kept++;
            }
        }
    }
    printf("margin %s M %g | excluded %llu kept %llu origins %llu violations %llu kept_alive %llu\n", name, (double)M, out_n, in_n, tried, violations, alive_kept);
}

int main() {
    const f3 sun = normalize3(mk3(0.35f, 1.0f, 0.2f)), low = normalize3(mk3(-0.8f, 0.25f, 0.1f));      // d = facing * -1: towards the light
    const std::vector<float> base = harness_scene(24);
    const int scales[6] = { -20, 0, 10, 14, 17, 20 };             // 2^10 .. 2^17: where the rounding of o + d decides who stays
    for (int e : scales) {
        exclusion("sun", base, e, sun, 64);
        exclusion("low", base, e, low, 64);
        exclusion("axis", base, e, mk3(0.0f, 1.0f, 0.0f), 64);
    }
    const float Ms[4] = { 128.0f, 22656.0f, 4.0e6f, 2.5e8f };
    for (float M : Ms) {
        margin_sweep("sun", sun, M);
        margin_sweep("low", low, M);
        margin_sweep("axis", mk3(0.0f, 1.0f, 0.0f), M);
    }
    edges();
    {
        Scene S; S.verts = base;
        upload(S, "none", {}, 75);
    }
    {
        Scene S; S.verts = base;
        upload(S, "one", { sun }, 75);
        brute(S, "one", 3000);
    }
    {
        Scene S; S.verts = base;
        upload(S, "two", { sun, low }, 100);
        brute(S, "two", 3000);
    }
    {
        Scene S; S.verts = base;
        upload(S, "ratio", { low }, 10);                          // the size rule says no: nothing appended
    }
    {
        Scene S;                                                  // a plane that faces its light: the empty set
        for (int i = 0; i < 6; ++i)
            for (int j = 0; j < 6; ++j) {
                const float x0 = (float)i - 3.0f, z0 = (float)j - 3.0f, x1 = x0 + 1.0f, z1 = z0 + 1.0f;
                const float q[18] = { x0, 0, z0,  x0, 0, z1,  x1, 0, z0,   x1, 0, z0,  x0, 0, z1,  x1, 0, z1 };
                S.verts.insert(S.verts.end(), q, q + 18);
            }
        upload(S, "plane", { sun }, 75);
        brute(S, "plane", 500);
    }
    return 0;
}
