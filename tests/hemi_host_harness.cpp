// hemi_host_harness.cpp - the definition of prt_hemisphere_visibility (par_raytracer_amd/csrc/dev_hemi.h, include/prt.h), compiled
// for the host with tests/hip_shim and run one lane at a time.  The rays come from hemi_index, hemi_point_valid and hemi_ray over
// the table of csrc/hammersley.h (the functions prt_upload_scene fills DevScene::diffuse_dirs with); every ray is answered twice:
//   brute force   over ALL triangles in input order, PRT_QUERY_OCCLUDED's rule as include/prt.h states it: on the biased origin o
//                 with qp = o - (o + d), tri_geom is true, !(t > FLT_MAX * dd), t * (1 / dd) < tmax;
//   the walk      the device traversal (csrc/dev_trace*.h) over the tree bvh_build.cpp builds (4-wide by default, -DPRT_BVH8:
//                 8-wide), routed as k_hemi_exact routes an item: scan_any_below for rays whose triangle test overflows,
//                 query_any_unculled from far origins, query_any_below otherwise.
// The counts, the fixed-point sums and the outputs come from the brute force's flags through hemi_fix, hemi_visibility and
// hemi_bent.  tests/hemi_cases.py writes the cases and reads the results; tests/test_hemi_host.py asserts that the walk equals the
// brute force for every ray, tests/test_gpu_hemi.py compares the device with the results bit for bit.
//
//   g++ -O1 -std=c++17 -ffp-contract=off -Itests/hip_shim -Ipar_raytracer_amd/csrc tests/hemi_host_harness.cpp \
//       par_raytracer_amd/csrc/bvh_build.cpp -pthread -o hemi_host && ./hemi_host cases.bin results.bin
//   ./hemi_host --table out.bin     the 1024 table entries (4 x f32 each), nothing else
//
// cases.bin: u32 case count, then per case 8 x u32 (positions, indices, points, samples, flags: 1 = max_dist present, 0, 0, 0),
// u64 seed, u64 first, f32 ray_bias, f32 0, positions (x3 f32), idx_positions (u32), points (x3 f32), normals (x3 f32), max_dist
// (f32 per point, when present).
// results.bin, per case: per ray (point-major, points x samples) the table index k (u32), the direction (x3 f32), the brute
// force's flag and the walk's (u8 each: 1 = unoccluded; both 0 for the rays of an invalid point, which are not cast); then per
// point unoccluded (u32), visibility (f32), bent (x3 f32) and the sums B (x3 i64); then u64 rays cast.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>            // tests/hip_shim: one lane at a time
using std::isfinite;

#include "dev_hemi.h"
#include "hammersley.h"
#include "harness_io.h"
#include "harness_mesh.h"

using namespace prt;

int main(int argc, char ** argv) {
    std::vector<float4> table(1024);
    for (uint32_t i = 0; i < 1024; ++i) table[i] = diffuse_tangent_dir(i);
    if (argc == 3 && !strcmp(argv[1], "--table")) {
        FILE * f = fopen(argv[2], "wb");
        if (!f) return 2;
        wr(f, table);
        return fclose(f) ? 2 : 0;
    }
    if (argc != 3) { fprintf(stderr, "usage: hemi_host in.bin out.bin | hemi_host --table out.bin\n"); return 2; }
    FILE * fin, * fout;
    if (!open_in_out(argc, argv, "hemi_host", &fin, &fout)) return 2;
    const uint32_t n_cases = rd<uint32_t>(fin, 1)[0];
    unsigned long long mismatches = 0;
    for (uint32_t ci = 0; ci < n_cases; ++ci) {
        const std::vector<uint32_t> hd = rd<uint32_t>(fin, 8);
        const uint32_t n_pos = hd[0], n_idx = hd[1], n_points = hd[2], samples = hd[3], n_tris = n_idx / 3;
        const std::vector<unsigned long long> keys = rd<unsigned long long>(fin, 2);
        const std::vector<float> fl = rd<float>(fin, 2);
        const unsigned long long seed = keys[0], first = keys[1];
        const float ray_bias = fl[0];
        const std::vector<float> pos = rd<float>(fin, 3 * (size_t)n_pos);
        const std::vector<uint32_t> idx = rd<uint32_t>(fin, n_idx);
        const std::vector<float> points = rd<float>(fin, 3 * (size_t)n_points), normals = rd<float>(fin, 3 * (size_t)n_points);
        const std::vector<float> max_dist = rd<float>(fin, (hd[4] & 1u) ? n_points : 0);

        // the tree, and the records: `brute` in input order, `tris` in the tree's leaf order
        const std::vector<float> verts = mesh::unindexed(pos, idx);
        BvhWide bvh;
        if (n_tris) mesh::build_tree(verts, n_tris, &bvh);
        const std::vector<float4> brute = mesh::records(verts, n_tris, nullptr), tris = mesh::records(verts, n_tris, bvh.tri_order.data());
        std::vector<unsigned int> rank(n_tris + 1, 0);
        for (uint32_t slot = 0; slot < n_tris; ++slot) rank[slot] = bvh.tri_order[slot];
        unsigned long long unresolved = 0;
        mesh::Walk lane(bvh, tris, n_tris);
        DevScene & sc = lane.sc;
        sc.tri_rank = rank.data();
        sc.tie_widen_max = 8;
        sc.near_tie_unresolved = &unresolved;
        sc.diffuse_dirs = table.data();
        GlobalStack & stk = lane.stk;
        TraceStats & st = lane.st;

        // the pad and the routing thresholds, as the host entry point computes them
        float scene_max = 0.0f, extent = 0.0f;
        for (uint32_t k = 0; k < n_idx; ++k)
            for (int c = 0; c < 3; ++c) scene_max = fmaxf(scene_max, fabsf(pos[3 * (size_t)idx[k] + c]));
        for (uint32_t i = 0; i < n_points; ++i) {
            const f3 p = mk3(points[3 * i], points[3 * i + 1], points[3 * i + 2]), n = mk3(normals[3 * i], normals[3 * i + 1], normals[3 * i + 2]);
            if (hemi_point_valid(p, n)) extent = fmaxf(extent, fmaxf(fmaxf(fabsf(p.x), fabsf(p.y)), fabsf(p.z)));
        }
        const float pad = fmaxf(scene_max, extent + fabsf(ray_bias)) * (1.0f / 65536.0f), far_beyond = 64.0f * scene_max;

        const size_t n_rays = (size_t)n_points * samples;
        std::vector<uint32_t> ks(n_rays, 0), unoccluded(n_points);
        std::vector<float> dirs(3 * n_rays, 0.0f), visibility(n_points), bent(3 * (size_t)n_points);
        std::vector<unsigned char> flag_brute(n_rays, 0), flag_walk(n_rays, 0);
        std::vector<long long> sums(3 * (size_t)n_points);
        unsigned long long cast = 0;
        for (uint32_t i = 0; i < n_points; ++i) {
            const f3 p = mk3(points[3 * i], points[3 * i + 1], points[3 * i + 2]), n = mk3(normals[3 * i], normals[3 * i + 1], normals[3 * i + 2]);
            const float tmax = max_dist.empty() ? 3.402823466e+38f : max_dist[i];
            if (!hemi_point_valid(p, n)) {
                unoccluded[i] = 0xFFFFFFFFu;
                visibility[i] = bent[3 * i] = bent[3 * i + 1] = bent[3 * i + 2] = 0.0f;
                sums[3 * i] = sums[3 * i + 1] = sums[3 * i + 2] = 0;
                continue;
            }
            cast += samples;
            uint32_t count = 0;
            long long B[3] = { 0, 0, 0 };
            for (uint32_t s = 0; s < samples; ++s) {
                const size_t e = (size_t)i * samples + s;
                const uint32_t k = hemi_index(seed, (uint32_t)(first + i), s);
                const float4 ts = table[k];
                f3 ob, d;
                const bool is_ray = hemi_ray(p, n, mk3(ts.x, ts.y, ts.z), ray_bias, ob, d);
                ks[e] = k;
                dirs[3 * e] = d.x; dirs[3 * e + 1] = d.y; dirs[3 * e + 2] = d.z;
                bool free_brute = true, free_walk = true;
                if (is_ray) {
                    const f3 qp = ob - (ob + d);
                    for (uint32_t t = 0; t < n_tris && free_brute; ++t) {
                        const float4 r0 = brute[(size_t)t * 3], r1 = brute[(size_t)t * 3 + 1], r2 = brute[(size_t)t * 3 + 2];
                        float tt, dd, v, w;
                        if (!tri_geom(ob, qp, mk3(r0.x, r0.y, r0.z), mk3(r0.w, r1.x, r1.y), mk3(r1.z, r1.w, r2.x), mk3(r2.y, r2.z, r2.w), tt, dd, v, w)) continue;
                        if (tt > 3.402823466e+38f * dd) continue;
                        if (tt * (1.0f / dd) < tmax) free_brute = false;
                    }
                    if (n_tris) {
                        const bool far = fmaxf(fmaxf(fabsf(ob.x), fabsf(ob.y)), fabsf(ob.z)) > far_beyond;
                        const HitRec h = ray_overflows(scene_max, ob, d) ? scan_any_below<true>(sc, ob, d, tmax, st)
                                       : far ? query_any_unculled<GlobalStack, true>(sc, ob, d, tmax, pad, stk, st)
                                             : query_any_below<GlobalStack, true>(sc, ob, d, tmax, pad, stk, st);
                        free_walk = h.tri < 0;
                    }
                }
                flag_brute[e] = free_brute ? 1 : 0;
                flag_walk[e] = free_walk ? 1 : 0;
                if (free_brute != free_walk) mismatches++;
                if (free_brute) {
                    count++;
                    B[0] += hemi_fix(d.x); B[1] += hemi_fix(d.y); B[2] += hemi_fix(d.z);
                }
            }
            unoccluded[i] = count;
            visibility[i] = hemi_visibility(count, samples);
            for (int c = 0; c < 3; ++c) { sums[3 * i + c] = B[c]; bent[3 * i + c] = hemi_bent(B[c], samples); }
        }
        wr(fout, ks); wr(fout, dirs); wr(fout, flag_brute); wr(fout, flag_walk);
        wr(fout, unoccluded); wr(fout, visibility); wr(fout, bent); wr(fout, sums);
        wr(fout, std::vector<unsigned long long>(1, cast));
    }
    fclose(fin);
    printf("%u cases, %llu rays on which the walk and the brute force differ\n", n_cases, mismatches);
    return fclose(fout) ? 2 : 0;
}
