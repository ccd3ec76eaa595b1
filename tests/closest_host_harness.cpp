// closest_host_harness.cpp - the closest-point definition and walk (par_raytracer_amd/csrc/dev_closest.h), compiled for the host
// with tests/hip_shim and run one lane at a time: the tree is built by bvh_build.cpp (4-wide by default, -DPRT_BVH8: 8-wide), the
// records and the leaf -> (group, vertex0) table laid out as prt_upload_scene and the queries lay them out, and every point is
// answered twice - by closest_point_walk over the tree, and by a brute force of closest_on_triangle over every triangle with the
// tie rule (closest_takes).  A case that carries a stack cap is walked a third time, the way one lane of k_closest walks it: on an
// LDS stack column of that many entries, to tell which points the kernel hands to k_closest_exact.  tests/closest_cases.py writes
// the cases and reads the results; tests/test_closest_host.py and tests/test_closest_cases_host.py assert on them,
// tests/test_gpu_closest.py and tests/test_gpu_closest_schedules.py compare the device with the brute force.
//
//   g++ -O1 -std=c++17 -ffp-contract=off -Itests/hip_shim -Ipar_raytracer_amd/csrc tests/closest_host_harness.cpp
//       par_raytracer_amd/csrc/bvh_build.cpp -pthread -o /tmp/closest_host && /tmp/closest_host cases.bin results.bin
//
// cases.bin: u32 case count, then per case 6 x u32 (points, positions, indices, groups, flags, stack cap - read with flag 4, else
// 0), the points (x3 f32), with flag 1 max_dist2 (f32 per point), with flag 2 an input triangle per point (u32), then positions
// (x3 f32), idx_positions (u32), the groups' (first_index, index_count) (2 x u32).
// results.bin, per case: i32 mismatches between walk and brute force, u32 points decided by the tie rule, u64 node visits and
// u64 triangle tests of the walk, then dist2, point (x3), bw (x3), vertex0, group of the brute force and the same five arrays of
// the walk.  With flag 4 then: u32 the cap in effect (the case's, clamped to 2..40 and to the tree's stack_bound as run_batch
// clamps STACK_CAP) and per point u32 listed = the marker of the capped walk carries TRAV_FLAG_OVERFLOW (0 for an invalid point,
// which is never walked).  With flag 2 nothing is walked: per case the same 24-byte header (zeros), then d2, v, w (f32) and
// finite (u32) of closest_on_triangle(point i, its triangle).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include <hip/hip_runtime.h>            // tests/hip_shim: one lane at a time
using std::isfinite;

#include "dev_closest.h"
#include "harness_io.h"
#include "harness_mesh.h"

using namespace prt;

struct Answers {
    std::vector<float> dist2, point, bw;
    std::vector<unsigned int> vertex0;
    std::vector<int> group;
    explicit Answers(size_t n) : dist2(n), point(3 * n), bw(3 * n), vertex0(n), group(n) {}
    // closest_emit of kernels_closest.h, field for field
    void emit(size_t i, const HitRec & h, const std::vector<float4> & tris, const std::vector<uint2> & leaf_map) {
        const bool hit = h.tri >= 0;
        dist2[i] = hit ? h.t : 3.402823466e+38f;
        f3 q = mk3(0.0f, 0.0f, 0.0f);
        if (hit) {
            const float4 r0 = tris[(size_t)h.tri * 3], r1 = tris[(size_t)h.tri * 3 + 1], r2 = tris[(size_t)h.tri * 3 + 2];
            q = closest_point_of(mk3(r0.x, r0.y, r0.z), mk3(r0.w, r1.x, r1.y), mk3(r1.z, r1.w, r2.x), h.v, h.w);
        }
        point[3 * i] = q.x; point[3 * i + 1] = q.y; point[3 * i + 2] = q.z;
        bw[3 * i] = hit ? 1.0f - h.v - h.w : 0.0f; bw[3 * i + 1] = hit ? h.v : 0.0f; bw[3 * i + 2] = hit ? h.w : 0.0f;
        const uint2 m = hit ? leaf_map[(size_t)h.tri] : make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
        group[i] = (int)m.x;
        vertex0[i] = m.y;
    }
    bool same(size_t i, const Answers & o) const {
        return !memcmp(&dist2[i], &o.dist2[i], 4) && !memcmp(&point[3 * i], &o.point[3 * i], 12) && !memcmp(&bw[3 * i], &o.bw[3 * i], 12) &&
               vertex0[i] == o.vertex0[i] && group[i] == o.group[i];
    }
    void write(FILE * f) const { wr(f, dist2); wr(f, point); wr(f, bw); wr(f, vertex0); wr(f, group); }
};

// One point as one lane of k_closest walks it (kernels_closest.h): an LDS stack column of `cap` entries, node steps and leaf steps
// in turn until the walk is done, then the marker's flags.  True when a push was dropped: the kernel lists the point.
static bool lane_lists_point(const DevScene & sc, f3 p, float max_d2, float pad, unsigned int cap, std::vector<int> & lds,
                             const uint2 * leaf_map) {
    LdsStack<1> stack;
    stack.attach(lds.data(), 0);
    stack.cap = cap;
    TravRay r;
    TraceStats st;
    point_init(r, p, max_d2, stack);
    while (!trav_done(r)) {
        while (trav_walking(r)) point_node_step<LdsStack<1>, false>(sc, r, stack, st, pad);
        if (!trav_done(r)) point_leaf<LdsStack<1>, false>(sc, r, stack, st, leaf_map);
    }
    return (trav_end_flags(r, stack) & TRAV_FLAG_OVERFLOW) != 0;
}

int main(int argc, char ** argv) {
    FILE * fin, * fout;
    if (!open_in_out(argc, argv, "closest_host", &fin, &fout)) return 2;
    const uint32_t n_cases = rd<uint32_t>(fin, 1)[0];
    for (uint32_t ci = 0; ci < n_cases; ++ci) {
        const std::vector<uint32_t> hd = rd<uint32_t>(fin, 6);
        const uint32_t n = hd[0], n_pos = hd[1], n_idx = hd[2], n_groups = hd[3], flags = hd[4], n_tris = n_idx / 3;
        const std::vector<float> pts = rd<float>(fin, 3 * (size_t)n);
        const std::vector<float> radius2 = rd<float>(fin, (flags & 1u) ? n : 0);
        const std::vector<uint32_t> pair_tri = rd<uint32_t>(fin, (flags & 2u) ? n : 0);
        const std::vector<float> pos = rd<float>(fin, 3 * (size_t)n_pos);
        const std::vector<uint32_t> idx = rd<uint32_t>(fin, n_idx);
        const std::vector<uint32_t> runs = rd<uint32_t>(fin, 2 * (size_t)n_groups);

        const std::vector<float> verts = mesh::unindexed(pos, idx);
        float abs_max = 0.0f;
        for (float v : verts) abs_max = std::max(abs_max, fabsf(v));
        uint64_t header[3] = { 0, 0, 0 };

        if (flags & 2u) {                                     // the function alone, on (point, triangle) pairs
            std::vector<float> d2(n), v(n), w(n);
            std::vector<uint32_t> ok(n);
            for (uint32_t i = 0; i < n; ++i) {
                const float * q = &verts[9 * (size_t)pair_tri[i]];
                const f3 a = mk3(q[0], q[1], q[2]), b = mk3(q[3], q[4], q[5]), c = mk3(q[6], q[7], q[8]);
                ok[i] = closest_on_triangle(mk3(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]), a, b - a, c - a, d2[i], v[i], w[i]) ? 1u : 0u;
            }
            fwrite(header, 8, 3, fout);
            wr(fout, d2); wr(fout, v); wr(fout, w); wr(fout, ok);
            continue;
        }

        BvhWide bvh;
        mesh::build_tree(verts, n_tris, &bvh);
        // device records and the leaf table, in the tree's leaf order
        const std::vector<float4> tris = mesh::records(verts, n_tris, bvh.tri_order.data());
        const std::vector<uint2> leaf_map = mesh::leaf_map(runs, n_groups, n_tris, bvh.tri_order.data());
        mesh::Walk lane(bvh, tris, n_tris);
        const DevScene & sc = lane.sc;
        GlobalStack & stk = lane.stk;
        TraceStats & st = lane.st;

        float extent = abs_max;                               // the pad's rule: 2^-16 x max(scene, finite points of the batch)
        for (uint32_t i = 0; i < n; ++i) {
            const f3 p = mk3(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]);
            if (isfinite(p.x) && isfinite(p.y) && isfinite(p.z)) extent = std::max(extent, std::max(std::max(fabsf(p.x), fabsf(p.y)), fabsf(p.z)));
        }
        const float pad = extent * (1.0f / 65536.0f);

        const unsigned int cap = std::min((unsigned int)bvh.stack_bound, std::max(2u, std::min(40u, hd[5])));
        std::vector<int> lds((size_t)cap * STACK_ENTRY_INTS, 0);
        std::vector<uint32_t> listed((flags & 4u) ? n : 0, 0u);

        Answers brute(n), walk(n);
        int32_t mismatches = 0;
        uint32_t tie_points = 0;
        for (uint32_t i = 0; i < n; ++i) {
            const f3 p = mk3(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]);
            const float max_d2 = (flags & 1u) ? radius2[i] : 3.402823466e+38f;
            const bool valid = isfinite(p.x) && isfinite(p.y) && isfinite(p.z) && max_d2 >= 0.0f;
            HitRec b, h;
            b.t = max_d2; b.v = b.w = 0.0f; b.tri = -1;
            h = b;
            if (valid) {
                for (uint32_t slot = 0; slot < n_tris; ++slot) {
                    const float4 r0 = tris[(size_t)slot * 3], r1 = tris[(size_t)slot * 3 + 1], r2 = tris[(size_t)slot * 3 + 2];
                    float d2, v, w;
                    if (closest_on_triangle(p, mk3(r0.x, r0.y, r0.z), mk3(r0.w, r1.x, r1.y), mk3(r1.z, r1.w, r2.x), d2, v, w) &&
                        closest_takes(d2, slot, b, leaf_map.data())) { b.t = d2; b.v = v; b.w = w; b.tri = (int)slot; }
                }
                if (b.tri >= 0) {                             // decided by the tie rule: another triangle has the same d2 bits
                    uint32_t equal = 0;
                    for (uint32_t slot = 0; slot < n_tris; ++slot) {
                        const float4 r0 = tris[(size_t)slot * 3], r1 = tris[(size_t)slot * 3 + 1], r2 = tris[(size_t)slot * 3 + 2];
                        float d2, v, w;
                        if (closest_on_triangle(p, mk3(r0.x, r0.y, r0.z), mk3(r0.w, r1.x, r1.y), mk3(r1.z, r1.w, r2.x), d2, v, w) && d2 == b.t) equal++;
                    }
                    if (equal > 1) tie_points++;
                }
                h = closest_point_walk<GlobalStack, true>(sc, p, max_d2, pad, stk, st, leaf_map.data());
                if (flags & 4u) listed[i] = lane_lists_point(sc, p, max_d2, pad, cap, lds, leaf_map.data()) ? 1u : 0u;
            }
            brute.emit(i, b, tris, leaf_map);
            walk.emit(i, h, tris, leaf_map);
            if (!brute.same(i, walk)) {
                if (mismatches < 10) fprintf(stderr, "case %u point %u: walk (d2 %.9g tri %d) brute force (d2 %.9g tri %d)\n", ci, i, h.t, h.tri, b.t, b.tri);
                mismatches++;
            }
        }
        const uint32_t h32[2] = { (uint32_t)mismatches, tie_points };
        fwrite(h32, 4, 2, fout);
        header[0] = st.nodes; header[1] = st.tris;
        fwrite(header, 8, 2, fout);
        brute.write(fout);
        walk.write(fout);
        if (flags & 4u) { fwrite(&cap, 4, 1, fout); wr(fout, listed); }
        printf("case %u: %u triangles, %u nodes, %u points, %d mismatches, %u decided by the tie rule, %.1f node visits and %.1f triangle tests per point\n",
               ci, n_tris, bvh.node_count, n, mismatches, tie_points, n ? (double)st.nodes / n : 0.0, n ? (double)st.tris / n : 0.0);
    }
    fclose(fin);
    return fclose(fout) ? 2 : 0;
}
