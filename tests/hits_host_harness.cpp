// hits_host_harness.cpp - the K-nearest-hits definition and walks (par_raytracer_amd/csrc/dev_hits.h), compiled for the host with
// tests/hip_shim and run one lane at a time: the tree is built by bvh_build.cpp (4-wide by default, -DPRT_BVH8: 8-wide), the records
// and the leaf -> (group, vertex0) table laid out as prt_upload_scene and the queries lay them out, and every ray is answered
// three times:
//   brute   the definition of include/prt.h over all records in input order, written out here and not through dev_hits.h's leaf
//           step: both forms of every record through tri_geom, the FLT_MAX reject, th < tmax; collect, sort by key, apply the
//           cursor, cut at k;
//   walk    routed as k_hits_exact routes it: hits_scan for a ray whose triangle test overflows, the walk that culls by geometry
//           only for a far origin, else the culled walk - on a global stack and a global list column;
//   lane    as one lane of k_hits walks it: an LDS stack column of the case's cap (0: the default) and an LDS list column.  Rays
//           that k_hits lists at the start are not walked (listed = 1); a ray whose push was dropped is listed = 2 and its slots
//           are not compared.
// tests/hits_cases.py writes the cases and reads the results; tests/test_hits_host.py asserts on them, tests/test_gpu_hits.py and
// tests/test_gpu_hits_schedules.py compare the device with the brute force.
//
// cases.bin: u32 case count, then per case 8 x u32 (rays, positions, indices, groups, flags, k, full, stack cap) and f32 ray_bias;
// origins and directions (x3 f32); with flag 1 tmax (f32 per ray); with flag 4 the cursor: after_t (f32), after_group (i32),
// after_vertex0 (u32); then positions (x3 f32), idx_positions (u32), the groups' (first_index, index_count) (2 x u32).  Flag 2:
// PRT_HITS_BACK_FACES.
// results.bin, per case: i32 rays on which walk and brute differ, i32 rays on which the unlisted lane and brute differ, u64 node
// visits and u64 triangle tests of the walk; the brute force's hit_count (u32), t, bw (x3), vertex0, group (per slot), back (u8 per
// slot); the walk's same six; then per ray u32 remaining (candidates behind the cursor, before the cut), u32 route (0 a miss by
// definition or a tmax that admits nothing, 1 culled walk, 2 far origin, 3 overflow), u32 listed; then, `full` > 0, the first
// `full` remaining candidates per ray in key order: t (f32), group (i32), vertex0 (u32), back (u8), the miss record behind them.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>            // tests/hip_shim: one lane at a time
using std::isfinite;

#include "dev_hits.h"
#include "harness_io.h"
#include "harness_mesh.h"

using namespace prt;

struct Candidate {
    float th, v, w;
    unsigned int group, vertex0, back;
};
static bool key_less(const Candidate & a, const Candidate & b) {
    if (a.th < b.th) return true;
    if (a.th != b.th) return false;
    return a.group < b.group || (a.group == b.group && a.vertex0 < b.vertex0);
}

struct Answers {
    unsigned int k;
    std::vector<uint32_t> hit_count, vertex0;
    std::vector<float> t, bw;
    std::vector<int32_t> group;
    std::vector<uint8_t> back;
    Answers(size_t n, unsigned int k_) : k(k_), hit_count(n, 0u), vertex0(n * k_, 0xFFFFFFFFu), t(n * k_, 3.402823466e+38f), bw(3 * n * k_, 0.0f),
                                         group(n * k_, -1), back(n * k_, 0) {}
    void slot(size_t i, unsigned int s, float th, float v, float w, unsigned int g, unsigned int v0, unsigned int b) {
        const size_t at = i * k + s;
        t[at] = th;
        bw[3 * at] = 1.0f - v - w; bw[3 * at + 1] = v; bw[3 * at + 2] = w;
        vertex0[at] = v0; group[at] = (int32_t)g; back[at] = (uint8_t)b;
    }
    bool same(size_t i, const Answers & o) const {
        return hit_count[i] == o.hit_count[i] && !memcmp(&t[i * k], &o.t[i * k], 4 * k) && !memcmp(&bw[3 * i * k], &o.bw[3 * i * k], 12 * k) &&
               !memcmp(&vertex0[i * k], &o.vertex0[i * k], 4 * k) && !memcmp(&group[i * k], &o.group[i * k], 4 * k) && !memcmp(&back[i * k], &o.back[i * k], k);
    }
    void write(FILE * f) const { wr(f, hit_count); wr(f, t); wr(f, bw); wr(f, vertex0); wr(f, group); wr(f, back); }
    template <class LIST>
    void take(size_t i, const DevScene & sc, const LIST & list, const uint2 * leaf_map, f3 ob, f3 d, unsigned int n) {
        const f3 qp = ob - (ob + d);
        hit_count[i] = n;
        for (unsigned int s = 0; s < n; ++s) {
            const HitSlot h = hits_slot(sc, list, leaf_map, ob, qp, s);
            slot(i, s, h.t, h.v, h.w, h.m.x, h.m.y, h.back);
        }
    }
};

// One ray as one lane of k_hits walks it (kernels_hits.h HitsJob).  Returns false when a push was dropped.
template <bool BACK>
static bool lane_walk(const DevScene & sc, f3 ob, f3 d, float tmax, float pad, unsigned int cap, std::vector<int> & lds, const LdsHitList<1> & list,
                      unsigned int k, const HitsCursor & cur, const uint2 * leaf_map, unsigned int & n) {
    LdsStack<1> stack;
    stack.attach(lds.data(), 0);
    stack.cap = cap;
    TravRay r;
    TraceStats st;
    hits_start(r, ob, d, tmax, pad, stack);
    float unused = 0.0f;
    while (!trav_done(r)) {
        while (trav_walking(r)) trav_node_step<LdsStack<1>, false>(sc, r, stack, st, pad);
        if (!trav_done(r)) hits_leaf<LdsStack<1>, LdsHitList<1>, BACK, false, true>(sc, r, stack, st, list, k, cur, leaf_map, unused);
    }
    n = (unsigned int)r.best.tri;
    return (trav_end_flags(r, stack) & TRAV_FLAG_OVERFLOW) == 0;
}

int main(int argc, char ** argv) {
    FILE * fin, * fout;
    if (!open_in_out(argc, argv, "hits_host", &fin, &fout)) return 2;
    const uint32_t n_cases = rd<uint32_t>(fin, 1)[0];
    for (uint32_t ci = 0; ci < n_cases; ++ci) {
        const std::vector<uint32_t> hd = rd<uint32_t>(fin, 8);
        const uint32_t n = hd[0], n_pos = hd[1], n_idx = hd[2], n_groups = hd[3], flags = hd[4], k = hd[5], full = hd[6], n_tris = n_idx / 3;
        const float ray_bias = rd<float>(fin, 1)[0];
        if (k < 1 || k > HITS_MAX) { fprintf(stderr, "hits_host: k out of range\n"); return 2; }
        const std::vector<float> org = rd<float>(fin, 3 * (size_t)n), dir = rd<float>(fin, 3 * (size_t)n);
        const std::vector<float> tmaxs = rd<float>(fin, (flags & 1u) ? n : 0);
        const std::vector<float> after_t = rd<float>(fin, (flags & 4u) ? n : 0);
        const std::vector<int32_t> after_group = rd<int32_t>(fin, (flags & 4u) ? n : 0);
        const std::vector<uint32_t> after_vertex0 = rd<uint32_t>(fin, (flags & 4u) ? n : 0);
        const std::vector<float> pos = rd<float>(fin, 3 * (size_t)n_pos);
        const std::vector<uint32_t> idx = rd<uint32_t>(fin, n_idx);
        const std::vector<uint32_t> runs = rd<uint32_t>(fin, 2 * (size_t)n_groups);
        const bool back_faces = (flags & 2u) != 0;

        const std::vector<float> verts = mesh::unindexed(pos, idx);
        float abs_max = 0.0f;
        for (float v : verts) abs_max = std::max(abs_max, fabsf(v));
        BvhWide bvh;
        mesh::build_tree(verts, n_tris, &bvh);
        // device records and the leaf table in the tree's leaf order; the brute force's in input order
        const std::vector<float4> tris = mesh::records(verts, n_tris, bvh.tri_order.data()), tris_in = mesh::records(verts, n_tris, nullptr);
        const std::vector<uint2> leaf_map = mesh::leaf_map(runs, n_groups, n_tris, bvh.tri_order.data()), map_in = mesh::leaf_map(runs, n_groups, n_tris, nullptr);
        mesh::Walk lane(bvh, tris, n_tris);
        const DevScene & sc = lane.sc;

        std::vector<f3> obs(n), ds(n);
        std::vector<uint8_t> valid(n);
        float extent = abs_max;                               // the pad's rule: 2^-16 x max(scene, valid biased origins of the batch)
        for (uint32_t i = 0; i < n; ++i) {
            const f3 o = mk3(org[3 * i], org[3 * i + 1], org[3 * i + 2]);
            const f3 d = mk3(dir[3 * i], dir[3 * i + 1], dir[3 * i + 2]);
            const f3 ob = o + d * ray_bias;
            obs[i] = ob; ds[i] = d;
            valid[i] = isfinite(o.x) && isfinite(o.y) && isfinite(o.z) && isfinite(d.x) && isfinite(d.y) && isfinite(d.z) && isfinite(ob.x) &&
                       isfinite(ob.y) && isfinite(ob.z) && !(d.x == 0.0f && d.y == 0.0f && d.z == 0.0f);
            if (isfinite(o.x) && isfinite(o.y) && isfinite(o.z) && isfinite(d.x) && isfinite(d.y) && isfinite(d.z) && isfinite(ob.x) &&
                isfinite(ob.y) && isfinite(ob.z)) extent = std::max(extent, std::max(std::max(fabsf(ob.x), fabsf(ob.y)), fabsf(ob.z)));
        }
        const float pad = extent * (1.0f / 65536.0f), replay_beyond = 64.0f * abs_max;

        const unsigned int cap = std::min((unsigned int)bvh.stack_bound, hd[7] ? std::max(2u, std::min(40u, hd[7])) : (unsigned int)STACK_LDS_CAP_DEFAULT);
        std::vector<int> lds((size_t)cap * STACK_ENTRY_INTS, 0), lds_list(2 * (size_t)HITS_MAX, 0), glob_list(2 * (size_t)HITS_MAX, 0);
        LdsHitList<1> llist;
        llist.attach(lds_list.data(), 0);
        GlobalHitList glist;
        glist.attach(glob_list.data(), 0, 1);

        Answers brute(n, k), walk(n, k), lanes(n, k);
        std::vector<uint32_t> remaining(n, 0u), route(n, 0u), listed(n, 0u);
        std::vector<float> full_t((size_t)n * full, 3.402823466e+38f);
        std::vector<int32_t> full_group((size_t)n * full, -1);
        std::vector<uint32_t> full_vertex0((size_t)n * full, 0xFFFFFFFFu);
        std::vector<uint8_t> full_back((size_t)n * full, 0);
        int32_t mismatches = 0, lane_mismatches = 0;
        std::vector<Candidate> cand;
        for (uint32_t i = 0; i < n; ++i) {
            const f3 ob = obs[i], d = ds[i];
            const float tmax = (flags & 1u) ? tmaxs[i] : 3.402823466e+38f;
            HitsCursor cur = hits_no_cursor();
            if (flags & 4u) { cur.t = after_t[i]; cur.group = after_group[i]; cur.vertex0 = after_vertex0[i]; }
            if (valid[i]) {
                // ---- the definition
                const f3 qp = ob - (ob + d);
                cand.clear();
                for (uint32_t ti = 0; ti < n_tris; ++ti) {
                    const float4 r0 = tris_in[(size_t)ti * 3], r1 = tris_in[(size_t)ti * 3 + 1], r2 = tris_in[(size_t)ti * 3 + 2];
                    const f3 a = mk3(r0.x, r0.y, r0.z), ab = mk3(r0.w, r1.x, r1.y), ac = mk3(r1.z, r1.w, r2.x), nr = mk3(r2.y, r2.z, r2.w);
                    for (unsigned int side = 0; side < (back_faces ? 2u : 1u); ++side) {
                        float t, dd, v, w;
                        const bool met = side ? tri_geom(ob, qp, a, ac, ab, mk3(-nr.x, -nr.y, -nr.z), t, dd, v, w) : tri_geom(ob, qp, a, ab, ac, nr, t, dd, v, w);
                        if (!met) continue;
                        if (t > 3.402823466e+38f * dd) continue;
                        const float ood = 1.0f / dd;
                        const float th = t * ood;
                        if (!(th < tmax)) continue;
                        Candidate c;
                        c.th = th;
                        c.v = side ? w * ood : v * ood;
                        c.w = side ? v * ood : w * ood;
                        c.group = map_in[ti].x; c.vertex0 = map_in[ti].y; c.back = side;
                        cand.push_back(c);
                    }
                }
                std::sort(cand.begin(), cand.end(), key_less);
                size_t first = 0;
                if (cur.group >= 0) {
                    Candidate c;
                    c.th = cur.t; c.group = (unsigned int)cur.group; c.vertex0 = cur.vertex0;
                    while (first < cand.size() && !key_less(c, cand[first])) ++first;
                    if (cur.t != cur.t) first = cand.size();
                }
                remaining[i] = (uint32_t)(cand.size() - first);
                brute.hit_count[i] = std::min<uint32_t>(k, remaining[i]);
                for (unsigned int s = 0; s < brute.hit_count[i]; ++s) {
                    const Candidate & c = cand[first + s];
                    brute.slot(i, s, c.th, c.v, c.w, c.group, c.vertex0, c.back);
                }
                for (unsigned int s = 0; s < full && first + s < cand.size(); ++s) {
                    const Candidate & c = cand[first + s];
                    full_t[(size_t)i * full + s] = c.th; full_group[(size_t)i * full + s] = (int32_t)c.group;
                    full_vertex0[(size_t)i * full + s] = c.vertex0; full_back[(size_t)i * full + s] = (uint8_t)c.back;
                }
                // ---- the walks, routed as HitsJob::start and k_hits_exact route them
                if (tmax > 0.0f) {
                    unsigned int m;
                    const bool far = fmaxf(fmaxf(fabsf(ob.x), fabsf(ob.y)), fabsf(ob.z)) > replay_beyond;
                    if (ray_overflows(abs_max, ob, d)) {
                        route[i] = 3u;
                        m = back_faces ? hits_scan<GlobalHitList, true, true>(sc, ob, d, tmax, lane.st, glist, k, cur, leaf_map.data())
                                       : hits_scan<GlobalHitList, false, true>(sc, ob, d, tmax, lane.st, glist, k, cur, leaf_map.data());
                    } else if (far) {
                        route[i] = 2u;
                        m = back_faces ? hits_walk<GlobalStack, GlobalHitList, true, true, false>(sc, ob, d, tmax, pad, lane.stk, lane.st, glist, k, cur, leaf_map.data())
                                       : hits_walk<GlobalStack, GlobalHitList, false, true, false>(sc, ob, d, tmax, pad, lane.stk, lane.st, glist, k, cur, leaf_map.data());
                    } else {
                        route[i] = 1u;
                        m = back_faces ? hits_walk<GlobalStack, GlobalHitList, true, true, true>(sc, ob, d, tmax, pad, lane.stk, lane.st, glist, k, cur, leaf_map.data())
                                       : hits_walk<GlobalStack, GlobalHitList, false, true, true>(sc, ob, d, tmax, pad, lane.stk, lane.st, glist, k, cur, leaf_map.data());
                    }
                    walk.take(i, sc, glist, leaf_map.data(), ob, d, m);
                    if (route[i] != 1u) listed[i] = 1u;
                    else {
                        const bool fits = back_faces ? lane_walk<true>(sc, ob, d, tmax, pad, cap, lds, llist, k, cur, leaf_map.data(), m)
                                                     : lane_walk<false>(sc, ob, d, tmax, pad, cap, lds, llist, k, cur, leaf_map.data(), m);
                        if (fits) lanes.take(i, sc, llist, leaf_map.data(), ob, d, m);
                        else listed[i] = 2u;
                    }
                }
            }
            if (!brute.same(i, walk)) {
                if (mismatches < 10) fprintf(stderr, "case %u ray %u: walk %u hits (t0 %.9g), brute force %u (t0 %.9g)\n", ci, i, walk.hit_count[i], walk.t[(size_t)i * k],
                                             brute.hit_count[i], brute.t[(size_t)i * k]);
                mismatches++;
            }
            if (!listed[i] && !brute.same(i, lanes)) {
                if (lane_mismatches < 10) fprintf(stderr, "case %u ray %u: lane %u hits (t0 %.9g), brute force %u (t0 %.9g)\n", ci, i, lanes.hit_count[i],
                                                  lanes.t[(size_t)i * k], brute.hit_count[i], brute.t[(size_t)i * k]);
                lane_mismatches++;
            }
        }
        const int32_t h32[2] = { mismatches, lane_mismatches };
        fwrite(h32, 4, 2, fout);
        const uint64_t h64[2] = { lane.st.nodes, lane.st.tris };
        fwrite(h64, 8, 2, fout);
        brute.write(fout);
        walk.write(fout);
        wr(fout, remaining); wr(fout, route); wr(fout, listed);
        wr(fout, full_t); wr(fout, full_group); wr(fout, full_vertex0); wr(fout, full_back);
        printf("case %u: %u triangles, %u nodes, %u rays, k %u, %d walk and %d lane mismatches, %.1f node visits and %.1f triangle tests per ray\n",
               ci, n_tris, bvh.node_count, n, k, mismatches, lane_mismatches, n ? (double)lane.st.nodes / n : 0.0, n ? (double)lane.st.tris / n : 0.0);
    }
    fclose(fin);
    return fclose(fout) ? 2 : 0;
}
