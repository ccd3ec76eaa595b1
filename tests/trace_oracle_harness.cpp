// trace_oracle_harness.cpp - the CPU oracle's own TraceRay (oracle/prt_oracle.cpp, included unchanged) over a batch of rays:
// the expected answers of prt_trace_rays (include/prt.h) for tests/trace_golden.py's fixtures.
//
//   g++ -O2 -std=c++14 -fPIC -shared -ffp-contract=off -fno-strict-aliasing -pthread -Iinclude tests/trace_oracle_harness.cpp \
//       -o trace_oracle.so
//
// prt_trace_oracle_batch, per ray (origin biased by direction * ray_bias[i], as TraceRay does):
//   CLOSEST   TraceRay's RaycastHit (raytracer.cpp:159-232): t, bw, vertex0, group, position, normal.  A miss is TraceRay's
//             zero-filled record with t = FLT_MAX, except group = -1 and vertex0 = 0xFFFFFFFF (prt.h).
//   OCCLUDED  brute force over every triangle of every group: IntersectRayTriangle against t = FLT_MAX gives a hit with
//             t < tmax (occluded_tmax) / t < FLT_MAX (occluded: no limit).  No visit order is involved.
//   near_tie  1 when the brute-force set of hits has a second member within 2^-19 of the smallest t (the rays the device
//             decides in the reference's visit order, dev_trace_common.h).
//   bf_t      the smallest brute-force t (FLT_MAX: none): the closest hit over ALL triangles, without the sphere tree.
// A ray with a non-finite origin, direction or biased origin component, or a zero direction, is a miss and not occluded.
#include <algorithm>

#include "../oracle/prt_oracle.cpp"

namespace {

bool ray_valid(V3 o, V3 d, V3 ob) {
    const float v[9] = { o.x, o.y, o.z, d.x, d.y, d.z, ob.x, ob.y, ob.z };
    for (float x : v)
        if (!std::isfinite(x)) return false;
    return !(d.x == 0.0f && d.y == 0.0f && d.z == 0.0f);
}

}  // namespace

extern "C" int prt_trace_oracle_batch(const prt_scene_desc * s, const float * origins, const float * dirs, const float * ray_bias,
                                      const float * tmax, uint32_t n, float * t, float * bw, uint32_t * vertex0, int32_t * group,
                                      float * position, float * normal, uint8_t * occluded, uint8_t * occluded_tmax,
                                      uint8_t * near_tie, float * bf_t, int threads) {
    if (!s || !origins || !dirs || !ray_bias || !tmax) return -1;
    if (threads < 1) threads = 1;
    auto work = [&](uint32_t lo, uint32_t hi) {
        Ctx cx;
        memset(&cx, 0, sizeof(cx));
        cx.s = s;
        Counters dbg;
        memset(&dbg, 0, sizeof(dbg));
        for (uint32_t i = lo; i < hi; ++i) {
            Ray ray;
            ray.origin = load3(origins + 3 * (size_t)i);
            ray.direction = load3(dirs + 3 * (size_t)i);
            Ray biased = ray;
            biased.origin = ray.origin + ray.direction * ray_bias[i];      // raytracer.cpp:163
            RaycastHit hit = HitWithT(FLT_MAX);
            bool any = false;
            const bool valid = ray_valid(ray.origin, ray.direction, biased.origin);
            if (valid) {
                cx.p.ray_bias = ray_bias[i];
                any = TraceRay(cx, ray, &hit, &dbg);
            }
            if (!any) {
                hit = HitWithT(FLT_MAX);
                hit.vertex0 = 0xFFFFFFFFu;
                hit.group = -1;
            }
            t[i] = hit.t;
            bw[3 * (size_t)i] = hit.bw.x; bw[3 * (size_t)i + 1] = hit.bw.y; bw[3 * (size_t)i + 2] = hit.bw.z;
            vertex0[i] = hit.vertex0;
            group[i] = hit.group;
            position[3 * (size_t)i] = hit.position.x; position[3 * (size_t)i + 1] = hit.position.y; position[3 * (size_t)i + 2] = hit.position.z;
            normal[3 * (size_t)i] = hit.normal.x; normal[3 * (size_t)i + 1] = hit.normal.y; normal[3 * (size_t)i + 2] = hit.normal.z;
            // brute force: the two smallest t over every front-facing triangle
            float m1 = FLT_MAX, m2 = FLT_MAX;
            bool hit_any = false;
            if (valid) {
                for (uint32_t g = 0; g < s->group_count; ++g) {
                    const prt_group & pg = s->groups[g];
                    const u32 * idx = s->idx_positions + pg.first_index;
                    for (u32 k = 0; k < pg.index_count; k += 3) {
                        RaycastHit h = HitWithT(FLT_MAX);
                        if (!IntersectRayTriangle(biased, load3(s->positions + 3 * (size_t)idx[k]), load3(s->positions + 3 * (size_t)idx[k + 1]),
                                                  load3(s->positions + 3 * (size_t)idx[k + 2]), &h))
                            continue;
                        hit_any = hit_any || h.t < FLT_MAX;
                        if (h.t < m1) { m2 = m1; m1 = h.t; }
                        else if (h.t < m2) m2 = h.t;
                    }
                }
            }
            occluded[i] = hit_any ? 1 : 0;
            occluded_tmax[i] = (hit_any && m1 < tmax[i]) ? 1 : 0;
            near_tie[i] = (m1 < FLT_MAX && m2 < FLT_MAX && m2 * 1.0000019073486328125f >= m1 && m2 <= m1 * 1.0000019073486328125f) ? 1 : 0;
            bf_t[i] = m1;
        }
    };
    std::vector<std::thread> pool;
    const uint32_t per = (n + (uint32_t)threads - 1) / (uint32_t)threads;
    for (int k = 0; k < threads; ++k) {
        const uint32_t lo = std::min(n, per * (uint32_t)k), hi = std::min(n, lo + per);
        if (lo < hi) pool.emplace_back(work, lo, hi);
    }
    for (std::thread & th : pool) th.join();
    return 0;
}
