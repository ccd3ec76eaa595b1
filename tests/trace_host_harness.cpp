// trace_host_harness.cpp - the DEVICE traversal code (par_raytracer_amd/csrc/dev_trace*.h), compiled for the host with
// tests/hip_shim and run one lane at a time against a brute-force restatement of the reference's hit filter.
//
// What it checks, with no GPU: that trace_ray() over the BVH the library builds (4-wide sorted by default; -DPRT_BVH8: 8-wide, slots sorted along one
// axis) returns, for every ray, exactly the hit the reference's sequential filter returns over ALL triangles
// in visit order (raytracer.cpp:104, 149, 208-220) - t, barycentrics and triangle bit for bit, near ties included - and
// that any-hit rays agree on occluded / not occluded.  Scene: a wavy height field plus floating, doubled and coplanar
// triangles (harness_scene.h).  Built and run by tests/test_trace_host.py.
//
//   trace_host --file PATH        triangles and rays from a file instead (tests/test_trace_edges_host.py): uint32 triangle count,
//                                 uint32 ray count, 9 floats per triangle in input order, 3 floats per origin, 3 per direction.
//                                 The rays go the queries' way: the traversal starts with trav_start<true> (directions of any
//                                 length), the box pad is 2^-16 of the largest |coordinate| of scene and origins, and a ray
//                                 whose triangle test overflows (ray_overflows) is scanned over every triangle instead -
//                                 the count of those is printed.
//   trace_host --file-plain PATH  the same, but through the renders' start of a traversal (trav_init's absolute clamp), for comparison.
//
//   g++ -O1 -std=c++17 -ffp-contract=off -Itests/hip_shim -Ipar_raytracer_amd/csrc tests/trace_host_harness.cpp \
//       par_raytracer_amd/csrc/bvh_build.cpp -pthread -o /tmp/trace_host && /tmp/trace_host
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "harness_mesh.h"
#include "harness_scene.h"

using namespace prt;

// The file of --file: false when it cannot be read whole.
static bool load_case(const char * path, std::vector<float> & verts, std::vector<float> & rays) {
    FILE * f = fopen(path, "rb");
    if (!f) return false;
    uint32_t head[2] = { 0, 0 };
    bool ok = fread(head, 4, 2, f) == 2 && head[0] > 0;
    if (ok) {
        verts.resize((size_t)head[0] * 9);
        rays.resize((size_t)head[1] * 6);
        ok = fread(verts.data(), 4, verts.size(), f) == verts.size() && fread(rays.data(), 4, rays.size(), f) == rays.size();
    }
    fclose(f);
    return ok;
}

int main(int argc, char ** argv) {
    const bool any_length = argc > 2 && !strcmp(argv[1], "--file"), from_file = any_length || (argc > 2 && !strcmp(argv[1], "--file-plain"));
    std::vector<float> verts, file_rays;
    if (from_file && !load_case(argv[2], verts, file_rays)) { fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
    const int grid = argc > 1 ? atoi(argv[1]) : 48;
    const int n_rays = from_file ? (int)(file_rays.size() / 6) : argc > 2 ? atoi(argv[2]) : 20000;
    if (!from_file) verts = harness_scene(grid);
    const uint32_t n_tris = (uint32_t)(verts.size() / 9);

    BvhWide bvh;
    mesh::build_tree(verts, n_tris, &bvh);
    const std::vector<float4> tris = mesh::records(verts, n_tris, bvh.tri_order.data());        // device records, in leaf order
    std::vector<unsigned int> rank(n_tris + 1, 0);
    for (uint32_t slot = 0; slot < n_tris; ++slot) rank[slot] = bvh.tri_order[slot];            // the "reference visit order": input order
    std::vector<uint32_t> slot_of_rank(n_tris);
    for (uint32_t slot = 0; slot < n_tris; ++slot) slot_of_rank[rank[slot]] = slot;
    unsigned long long unresolved = 0;
    mesh::Walk lane(bvh, tris, n_tris);
    DevScene & sc = lane.sc;
    sc.tri_rank = rank.data();
    sc.tie_widen_max = 8;
    sc.near_tie_unresolved = &unresolved;
    GlobalStack & stk = lane.stk;
    TraceStats & st = lane.st;

    float pad = 16.0f / 65536.0f, scene_max = 0.0f;
    unsigned long long scanned = 0;
    if (from_file) {
        for (float x : verts) scene_max = fmaxf(scene_max, fabsf(x));
        float m = scene_max;
        for (int k = 0; k < 3 * n_rays; ++k) m = fmaxf(m, fabsf(file_rays[k]));
        pad = m * (1.0f / 65536.0f);
    }
    unsigned long long mismatches = 0, hits = 0, any_mismatches = 0, near = 0;
    for (int k = 0; k < n_rays; ++k) {
        f3 o, d;
        if (from_file) {
            o = mk3(file_rays[3 * (size_t)k], file_rays[3 * (size_t)k + 1], file_rays[3 * (size_t)k + 2]);
            const float * dp = &file_rays[3 * (size_t)n_rays + 3 * (size_t)k];
            d = mk3(dp[0], dp[1], dp[2]);
        } else if (k % 3 == 0) {                             // from above, downwards: terrain and decals head-on
            o = mk3((float)(rnd() * 10 - 5), 3.0f, (float)(rnd() * 10 - 5));
            d = normalize3(mk3((float)(rnd() - 0.5) * 0.6f, -1.0f, (float)(rnd() - 0.5) * 0.6f));
        } else if (k % 3 == 1) {                             // grazing
            o = mk3((float)(rnd() * 10 - 5), (float)(rnd() * 1.5), (float)(rnd() * 10 - 5));
            d = normalize3(mk3((float)(rnd() - 0.5), (float)(rnd() - 0.5) * 0.2f, (float)(rnd() - 0.5)));
        } else {                                             // anything, axis-parallel now and then
            o = mk3((float)(rnd() * 10 - 5), (float)(rnd() * 3), (float)(rnd() * 10 - 5));
            d = mk3((float)(rnd() - 0.5), (float)(rnd() - 0.5), (float)(rnd() - 0.5));
            if (k % 30 == 2) d = mk3(0.0f, -1.0f, 0.0f);
            if (k % 30 == 5) d = mk3(1.0f, 0.0f, 0.0f);
            d = normalize3(d);
        }
        // the reference: its sequential filter over every triangle in visit (= input) order
        const f3 qp = o - (o + d);
        float best = 3.402823466e+38f, bv = 0, bw = 0;
        int btri = -1;
        for (uint32_t r = 0; r < n_tris; ++r) {
            const uint32_t slot = slot_of_rank[r];
            const float4 r0 = tris[(size_t)slot * 3], r1 = tris[(size_t)slot * 3 + 1], r2 = tris[(size_t)slot * 3 + 2];
            float t, v, w;
            if (tri_test_ref(o, qp, mk3(r0.x, r0.y, r0.z), mk3(r0.w, r1.x, r1.y), mk3(r1.z, r1.w, r2.x), mk3(r2.y, r2.z, r2.w), best, t, v, w)) {
                best = t; bv = v; bw = w; btri = (int)slot;
            }
        }
        if (btri >= 0) {                                     // rays whose hit has company within 2^-19: resolve_near_ties decides them
            unsigned int company = 0;
            for (uint32_t slot = 0; slot < n_tris; ++slot) {
                const float4 r0 = tris[(size_t)slot * 3], r1 = tris[(size_t)slot * 3 + 1], r2 = tris[(size_t)slot * 3 + 2];
                float t, dd, v, w;
                if (tri_geom(o, qp, mk3(r0.x, r0.y, r0.z), mk3(r0.w, r1.x, r1.y), mk3(r1.z, r1.w, r2.x), mk3(r2.y, r2.z, r2.w), t, dd, v, w) &&
                    t / dd <= best * PRT_TIE_NEAR) company++;
            }
            if (company > 1) near++;
        }
        const bool scan = from_file && ray_overflows(scene_max, o, d);
        if (scan) scanned++;
        const HitRec h = scan ? scan_closest<true>(sc, slot_of_rank.data(), o, d, st)
                       : any_length ? trace_ray<GlobalStack, true, true>(sc, o, d, TRACE_CLOSEST, pad, stk, st)
                                    : trace_ray<GlobalStack, true>(sc, o, d, TRACE_CLOSEST, pad, stk, st);
        if (btri >= 0) hits++;
        if (h.tri != btri || (btri >= 0 && (memcmp(&h.t, &best, 4) || memcmp(&h.v, &bv, 4) || memcmp(&h.w, &bw, 4)))) {
            if (mismatches < 10) fprintf(stderr, "ray %d: traversal (t %.9g tri %d) reference (t %.9g tri %d)\n", k, h.t, h.tri, best, btri);
            mismatches++;
        }
        const HitRec a = scan ? scan_any_below<true>(sc, o, d, 3.402823466e+38f, st)
                       : any_length ? trace_ray<GlobalStack, true, true>(sc, o, d, TRACE_ANY, pad, stk, st)
                                    : trace_ray<GlobalStack, true>(sc, o, d, TRACE_ANY, pad, stk, st);
        if ((a.tri >= 0) != (btri >= 0)) any_mismatches++;
    }
    printf("%u triangles, %u nodes, depth %u, stack bound %u; %d rays, %llu hits, %llu with a near tie; "
           "closest-hit mismatches %llu, any-hit mismatches %llu, unresolved near ties %llu; %.2f node visits and %.2f triangle tests per traversal\n",
           n_tris, bvh.node_count, bvh.max_depth, bvh.stack_bound, n_rays, hits, near, mismatches, any_mismatches, unresolved,
           (double)st.nodes / (2.0 * n_rays), (double)st.tris / (2.0 * n_rays));
    if (from_file) printf("%llu rays scanned over every triangle (ray_overflows)\n", scanned);
    return (mismatches || any_mismatches || unresolved) ? 1 : 0;
}
