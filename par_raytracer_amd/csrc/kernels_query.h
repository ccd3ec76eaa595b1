// kernels_query.h - batched ray queries (prt_trace_rays): the reference's TraceRay (raytracer.cpp:159-232) on rays the caller
// supplies, without shading.
//
//   k_query_pad    max |biased origin component| over the batch's valid rays, one word (device entry point only: the host entry
//                  point computes it on the host), for batch_pad.
//   k_query        the wave loop of dev_wave_loop.h over the traversal of dev_trace.h.  CLOSEST: closest hit; OCCLUDED: any hit
//                  below tmax (the best hit starts at tmax: tri_test accepts th < best_t).  A ray that is a miss by definition is
//                  written at once.  Rays that end flagged (a near tie, or a push that did not fit the LDS column) go to a list,
//                  as do CLOSEST rays whose direction is not unit length or whose origin is far from the scene (query_replays),
//                  and OCCLUDED rays from far origins (query_any_unculled), rays whose triangle test overflows (ray_overflows,
//                  dev_trace.h), and CLOSEST hits whose group the reference would
//                  not have scanned (query_hit_stands).
//   k_query_exact  traces the listed rays again on a full-height global stack: trace_ray (near ties decided in the reference's
//                  visit order by resolve_near_ties), the full replay of TraceRay for non-unit directions and for hits that do
//                  not stand, the any-hit walk below tmax, or the scan of every triangle for rays that overflow.
// Directions have any length: every traversal here starts with trav_start<true> (dev_trace.h).
// Only the fields the caller asked for are written (a wave-uniform mask), with plain vector stores.
#pragma once

#include "dev_wave_loop.h"
#include "dev_wave_reduce.h"

namespace prt {

enum { QUERY_CLOSEST = 0, QUERY_OCCLUDED = 1 };
enum { QF_T = 1, QF_BW = 2, QF_VERTEX0 = 4, QF_GROUP = 8, QF_POSITION = 16, QF_NORMAL = 32, QF_OCCLUDED = 64 };

struct QueryArgs : BatchShared {
    const float * origins;           // count x 3
    const float * dirs;              // count x 3
    const float * tmax;              // count, OCCLUDED only; null = no limit
    unsigned int count;
    float ray_bias;
    // outputs (null unless the field's bit is in the mask)
    float * t;
    float * bw;                      // x3
    unsigned int * vertex0;
    int * group;
    float * position;                // x3
    float * normal;                  // x3
    unsigned char * occluded;
    float replay_beyond;             // CLOSEST rays whose biased origin lies further out are replayed (query_replays)
    float scene_max;                 // the scene's largest |coordinate| (ray_overflows)
    const unsigned int * slot_of_rank;      // the inverse of DevScene::tri_rank (scan_closest)
};

// Ray i, origin biased as TraceRay does (raytracer.cpp:163).  False for a ray that is a miss by definition: a non-finite
// origin or direction component, a zero direction.
PRT_D bool query_ray(const QueryArgs & A, unsigned int i, f3 & ob, f3 & d) {
    const f3 o = mk3(A.origins[3u * i], A.origins[3u * i + 1u], A.origins[3u * i + 2u]);
    d = mk3(A.dirs[3u * i], A.dirs[3u * i + 1u], A.dirs[3u * i + 2u]);
    ob = o + d * A.ray_bias;
    const bool finite = isfinite(o.x) && isfinite(o.y) && isfinite(o.z) && isfinite(d.x) && isfinite(d.y) && isfinite(d.z) &&
                        isfinite(ob.x) && isfinite(ob.y) && isfinite(ob.z);
    return finite && !(d.x == 0.0f && d.y == 0.0f && d.z == 0.0f);
}

// The reference's sphere test (IntersectRaySphere, raytracer.cpp:32-60) assumes a unit direction: for other lengths its entry
// distance is not in the units of the ray's t, and TraceRay skips groups whose triangles would give the closest hit.  The fast
// traversal finds the closest hit over all triangles, which is TraceRay's answer only where that test is sound, i.e. for
// (float-normalised) unit directions.  A CLOSEST ray whose |d|^2 is further than 2^-18 from 1 is therefore replayed in full on
// the slow path: resolve_near_ties with an unbounded candidate set offers every triangle the ray's line meets to the
// reference's filter in the reference's visit order, sphere tests included (RefSphereWalk) - TraceRay, step for step.  The same
// holds for an origin far from the scene (beyond 64 x its largest coordinate): there IntersectRaySphere's c = m.m - r^2 cancels
// and the reference drops groups at random.
PRT_D bool query_overflows(const QueryArgs & A, f3 ob, f3 d) { return ray_overflows(A.scene_max, ob, d); }
PRT_D bool query_far(const QueryArgs & A, f3 ob) { return fmaxf(fmaxf(fabsf(ob.x), fabsf(ob.y)), fabsf(ob.z)) > A.replay_beyond; }
PRT_D bool query_replays(const QueryArgs & A, f3 ob, f3 d) {
    const float l2 = dot3(d, d);
    const bool unit = l2 >= 1.0f - 3.814697265625e-6f && l2 <= 1.0f + 3.814697265625e-6f;
    return !unit || query_far(A, ob);
}

// The closest hit over all triangles is TraceRay's hit only if TraceRay scans the hit's group: every sphere on the way down to it
// must pass IntersectRaySphere and be entered no later than the best hit of that moment.  In exact arithmetic a hit lies inside
// its group's sphere; in the reference's float arithmetic a ray through one of the extreme vertices the sphere was built
// through grazes it and can fail the test (an axis-parallel ray up an edge of cornell_box: TraceRay misses the ceiling).  So
// the winner is put to RefSphereWalk with its own t as the best hit: TraceRay's best at that moment is no smaller, so a sphere
// that passes here passes there.  A refusal proves nothing - the ray is then replayed in full, which is TraceRay step for step.
PRT_D bool query_hit_stands(const DevScene & sc, f3 ob, f3 d, const HitRec & h) {
    if (h.tri < 0 || !sc.ref_spheres) return true;
    RefSphereWalk walk;
    walk.reset();
    return walk.offers(sc, ob, d, sc.tri_rank[h.tri], h.t);
}

// The RaycastHit of ray i (raytracer.cpp:20-30, 82-125) into the requested fields.  h.tri < 0: a miss - the reference's
// zero-filled record with t = FLT_MAX, except group = -1 and vertex0 = 0xFFFFFFFF.
template <int MODE>
PRT_D void query_emit(const DevScene & sc, const QueryArgs & A, const uint2 * leaf_map, unsigned int fields, unsigned int i,
                      f3 ob, f3 d, const HitRec & h) {
    const bool hit = h.tri >= 0;
    if (MODE == QUERY_OCCLUDED) {
        if (fields & QF_OCCLUDED) A.occluded[i] = hit ? 1 : 0;
        return;
    }
    if (fields & QF_T) A.t[i] = hit ? h.t : 3.402823466e+38f;
    if (fields & QF_BW) {
        A.bw[3u * i] = hit ? 1.0f - h.v - h.w : 0.0f;                       // raytracer.cpp:120
        A.bw[3u * i + 1u] = hit ? h.v : 0.0f;
        A.bw[3u * i + 2u] = hit ? h.w : 0.0f;
    }
    if (fields & (QF_VERTEX0 | QF_GROUP)) {
        const uint2 m = hit ? leaf_map[h.tri] : make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);      // (group, vertex0)
        if (fields & QF_GROUP) A.group[i] = (int)m.x;
        if (fields & QF_VERTEX0) A.vertex0[i] = m.y;
    }
    if (fields & QF_POSITION) {
        const f3 p = hit ? ob + d * h.t : mk3(0.0f, 0.0f, 0.0f);           // raytracer.cpp:121
        A.position[3u * i] = p.x; A.position[3u * i + 1u] = p.y; A.position[3u * i + 2u] = p.z;
    }
    if (fields & QF_NORMAL) {
        f3 n = mk3(0.0f, 0.0f, 0.0f);
        if (hit) {
            const float4 r2 = sc.tris[3u * (unsigned int)h.tri + 2u];       // (ac.z, n.xyz), n = Cross(ab, ac) from the host
            n = normalize3(mk3(r2.y, r2.z, r2.w));                          // raytracer.cpp:122
        }
        A.normal[3u * i] = n.x; A.normal[3u * i + 1u] = n.y; A.normal[3u * i + 2u] = n.z;
    }
}

// ---------------------------------------------------------------------------------------------------------
// max |biased origin component| of the valid rays -> work[BATCH_W_EXTENT]
__global__ __launch_bounds__(256) void k_query_pad(QueryArgs A) {
    float m = 0.0f;
    for (unsigned int i = blockIdx.x * blockDim.x + threadIdx.x; i < A.count; i += gridDim.x * blockDim.x) {
        f3 ob, d;
        if (query_ray(A, i, ob, d)) m = fmaxf(m, fmaxf(fmaxf(fabsf(ob.x), fabsf(ob.y)), fabsf(ob.z)));
    }
    wave_max_to_word(A.work + BATCH_W_EXTENT, m);
}

// ---------------------------------------------------------------------------------------------------------
// k_query's job for the wave loop: a lane's item is a ray of the batch.
template <int BLOCK, int MODE, bool COUNT>
struct QueryJob : RaySteps<BLOCK, COUNT> {
    const QueryArgs & A;
    const uint2 * leaf_map;
    unsigned int fields;
    PRT_D bool start(unsigned int idx, TravRay & r, const LdsStack<BLOCK> & stack) const {
        f3 ob, d;
        const bool valid = query_ray(A, idx, ob, d);
        if (valid && (query_overflows(A, ob, d) || (MODE == QUERY_CLOSEST ? query_replays(A, ob, d) : query_far(A, ob)))) {
            batch_to_slow_list(A, idx);                                     // scan_* / query_replays / query_any_unculled
        } else if (valid) {
            trav_start<true>(r, ob, d, MODE == QUERY_OCCLUDED ? TRACE_ANY : TRACE_CLOSEST, this->pad, stack);
            if (MODE == QUERY_OCCLUDED && A.tmax) r.best.t = A.tmax[idx];
            return true;
        } else {
            query_emit<MODE>(this->sc, A, leaf_map, fields, idx, ob, d, hit_miss());
        }
        return false;
    }
    PRT_D void finish(unsigned int idx, const TravRay & r, const LdsStack<BLOCK> & stack) const {
        if (trav_needs_slow_path(r, stack) || (MODE == QUERY_CLOSEST && !query_hit_stands(this->sc, r.o, r.d, r.best))) batch_to_slow_list(A, idx);
        else query_emit<MODE>(this->sc, A, leaf_map, fields, idx, r.o, r.d, r.best);       // r.o: the biased origin
    }
};

// Persistent traversal of the batch.  grid = resident blocks; dynamic LDS = stack_lds_entries * BLOCK * 4.
template <int BLOCK, int MODE, bool COUNT>
__global__ __launch_bounds__(BLOCK, 6) void k_query(DevScene sc, QueryArgs A, const uint2 * leaf_map, unsigned int fields,
                                                  int keep_min, int node_min, unsigned int chunk, DevCounters * ctr) {
    extern __shared__ int s_stack[];
    LdsStack<BLOCK> stack;
    stack.attach(s_stack, threadIdx.x);
    stack.cap = A.stack_lds_entries;
    TraceStats st;
    QueryJob<BLOCK, MODE, COUNT> job = { { sc, batch_pad(A) }, A, leaf_map, fields };
    wave_loop<BLOCK, COUNT>(job, stack, st, A.work + BATCH_W_HEAD, A.count, keep_min, node_min, chunk);
    if (COUNT) trace_stats_flush<true>(ctr, st);
}

// ---------------------------------------------------------------------------------------------------------
// Slow path of k_query (exact_list_walk).
template <int MODE, bool COUNT>
__global__ __launch_bounds__(256) void k_query_exact(DevScene sc, QueryArgs A, const uint2 * leaf_map, unsigned int fields,
                                                     DevCounters * ctr) {
    const float pad = batch_pad(A);
    exact_list_walk<COUNT>(A.slow, A.work[BATCH_W_SLOW], A.exact_stack, A.exact_stack_stride, ctr, [&](unsigned int idx, const GlobalStack & slow, TraceStats & st) {
        f3 ob, d;
        (void)query_ray(A, idx, ob, d);                                     // listed rays are valid
        HitRec h;
        if (query_overflows(A, ob, d)) {
            if (MODE == QUERY_OCCLUDED) h = scan_any_below<COUNT>(sc, ob, d, A.tmax ? A.tmax[idx] : 3.402823466e+38f, st);
            else h = scan_closest<COUNT>(sc, A.slot_of_rank, ob, d, st);
        } else if (MODE == QUERY_OCCLUDED && query_far(A, ob))
            h = query_any_unculled<GlobalStack, COUNT>(sc, ob, d, A.tmax ? A.tmax[idx] : 3.402823466e+38f, pad, slow, st);
        else if (MODE == QUERY_OCCLUDED)
            h = query_any_below<GlobalStack, COUNT>(sc, ob, d, A.tmax ? A.tmax[idx] : 3.402823466e+38f, pad, slow, st);
        else {
            bool replay = query_replays(A, ob, d);
            if (!replay) {
                // a miss here is a true miss, or a near tie all of whose members the reference's spheres refused: either way the
                // full replay decides (for a true miss it is one walk that finds no candidate)
                h = trace_ray<GlobalStack, COUNT, true>(sc, ob, d, TRACE_CLOSEST, pad, slow, st);
                replay = h.tri < 0 || !query_hit_stands(sc, ob, d, h);
            }
            if (replay) h = resolve_near_ties<GlobalStack, COUNT, true>(sc, ob, d, pad, 3.402823466e+38f, slow, st);      // bound = inf: every candidate
        }
        query_emit<MODE>(sc, A, leaf_map, fields, idx, ob, d, h);
    });
}

}  // namespace prt
