// kernels_closest.h - nearest surface point for batches of points (prt_closest_points): the walk of dev_closest.h on points the
// caller supplies.
//
//   k_closest_pad    max |component| over the batch's finite points, one word (device entry point only: the host entry point
//                    computes it on the host), for batch_pad.
//   k_closest        the wave loop of dev_wave_loop.h over the walk's node steps and leaf steps.  A point that is a miss by
//                    definition - a non-finite component, max_dist2 negative or NaN - is written at once.  A point whose push
//                    did not fit the LDS column goes to a list.
//   k_closest_exact  walks the listed points again, from the start, on a full-height global stack.
// Only the fields the caller asked for are written (a wave-uniform mask), with plain vector stores.
// prt_signed_distance runs the same two kernels with CF_SIGNED / CF_FEATURE in the mask and the tables of dev_signed.h in the
// arguments: closest_emit then signs the winner (signed_of_winner).  Without those bits nothing of it is read or executed.
#pragma once

#include "dev_signed.h"
#include "dev_wave_loop.h"
#include "dev_wave_reduce.h"

namespace prt {

enum { CF_DIST2 = 1, CF_POINT = 2, CF_BW = 4, CF_VERTEX0 = 8, CF_GROUP = 16, CF_SIGNED = 32, CF_FEATURE = 64 };

struct ClosestArgs : BatchShared {
    const float * points;            // count x 3
    const float * max_dist2;         // count, or null = no limit
    unsigned int count;
    // outputs (null unless the field's bit is in the mask)
    float * dist2;
    float * point;                   // x3
    float * bw;                      // x3
    unsigned int * vertex0;
    int * group;
    // prt_signed_distance (null / unused unless CF_SIGNED or CF_FEATURE is in the mask)
    float * signed_dist;
    unsigned char * feature;
    SignedTables sign;
};

PRT_D bool closest_finite(f3 p) { return isfinite(p.x) && isfinite(p.y) && isfinite(p.z); }

// Point i and its squared radius.  False for a point that is a miss by definition.
PRT_D bool closest_query(const ClosestArgs & A, unsigned int i, f3 & p, float & max_d2) {
    p = mk3(A.points[3u * i], A.points[3u * i + 1u], A.points[3u * i + 2u]);
    max_d2 = A.max_dist2 ? A.max_dist2[i] : 3.402823466e+38f;
    return closest_finite(p) && max_d2 >= 0.0f;                            // NaN fails the comparison
}

// The result of point i into the requested fields.  h.tri < 0: a miss - dist2 = FLT_MAX, zeros, group = -1, vertex0 = 0xFFFFFFFF.
PRT_D void closest_emit(const DevScene & sc, const ClosestArgs & A, const uint2 * leaf_map, unsigned int fields, unsigned int i,
                        const HitRec & h) {
    const bool hit = h.tri >= 0;
    if (fields & CF_DIST2) A.dist2[i] = hit ? h.t : 3.402823466e+38f;
    if (fields & CF_POINT) {
        f3 q = mk3(0.0f, 0.0f, 0.0f);
        if (hit) {
            const float4 * tp = reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(sc.tris) + (unsigned int)h.tri * 48u);
            const float4 r0 = tp[0], r1 = tp[1], r2 = tp[2];
            q = closest_point_of(mk3(r0.x, r0.y, r0.z), mk3(r0.w, r1.x, r1.y), mk3(r1.z, r1.w, r2.x), h.v, h.w);
        }
        A.point[3u * i] = q.x; A.point[3u * i + 1u] = q.y; A.point[3u * i + 2u] = q.z;
    }
    if (fields & CF_BW) {
        A.bw[3u * i] = hit ? 1.0f - h.v - h.w : 0.0f;
        A.bw[3u * i + 1u] = hit ? h.v : 0.0f;
        A.bw[3u * i + 2u] = hit ? h.w : 0.0f;
    }
    if (fields & (CF_VERTEX0 | CF_GROUP)) {
        const uint2 m = hit ? leaf_map[h.tri] : make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);      // (group, vertex0)
        if (fields & CF_GROUP) A.group[i] = (int)m.x;
        if (fields & CF_VERTEX0) A.vertex0[i] = m.y;
    }
    if (fields & (CF_SIGNED | CF_FEATURE)) {
        float sd = 3.402823466e+38f;
        unsigned int feature = 255u;
        if (hit) {
            const float4 * tp = reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(sc.tris) + (unsigned int)h.tri * 48u);
            const float4 r0 = tp[0], r1 = tp[1], r2 = tp[2];
            const f3 p = mk3(A.points[3u * i], A.points[3u * i + 1u], A.points[3u * i + 2u]);
            sd = signed_of_winner(A.sign, (unsigned int)h.tri, p, mk3(r0.x, r0.y, r0.z), mk3(r0.w, r1.x, r1.y), mk3(r1.z, r1.w, r2.x), h.t, feature);
        }
        if (fields & CF_SIGNED) A.signed_dist[i] = sd;
        if (fields & CF_FEATURE) A.feature[i] = (unsigned char)feature;
    }
}

// ---------------------------------------------------------------------------------------------------------
// max |component| of the finite points -> work[BATCH_W_EXTENT]
__global__ __launch_bounds__(256) void k_closest_pad(ClosestArgs A) {
    float m = 0.0f;
    for (unsigned int i = blockIdx.x * blockDim.x + threadIdx.x; i < A.count; i += gridDim.x * blockDim.x) {
        const f3 p = mk3(A.points[3u * i], A.points[3u * i + 1u], A.points[3u * i + 2u]);
        if (closest_finite(p)) m = fmaxf(m, fmaxf(fmaxf(fabsf(p.x), fabsf(p.y)), fabsf(p.z)));
    }
    wave_max_to_word(A.work + BATCH_W_EXTENT, m);
}

// ---------------------------------------------------------------------------------------------------------
// k_closest's job for the wave loop: a lane's item is a point of the batch.
template <int BLOCK, bool COUNT>
struct ClosestJob {
    const DevScene & sc;
    const ClosestArgs & A;
    const uint2 * leaf_map;
    unsigned int fields;
    float pad;
    PRT_D bool start(unsigned int idx, TravRay & r, const LdsStack<BLOCK> & stack) const {
        f3 p;
        float max_d2;
        if (closest_query(A, idx, p, max_d2)) {
            point_init(r, p, max_d2, stack);
            return true;
        }
        closest_emit(sc, A, leaf_map, fields, idx, hit_miss());
        return false;
    }
    PRT_D void node_step(TravRay & r, const LdsStack<BLOCK> & stack, TraceStats & st) const { point_node_step<LdsStack<BLOCK>, COUNT>(sc, r, stack, st, pad); }
    PRT_D bool leaf(TravRay & r, const LdsStack<BLOCK> & stack, TraceStats & st) const {
        point_leaf<LdsStack<BLOCK>, COUNT>(sc, r, stack, st, leaf_map);
        return trav_done(r);
    }
    PRT_D void finish(unsigned int idx, const TravRay & r, const LdsStack<BLOCK> & stack) const {
        if (trav_end_flags(r, stack) & TRAV_FLAG_OVERFLOW) batch_to_slow_list(A, idx);
        else closest_emit(sc, A, leaf_map, fields, idx, r.best);
    }
};

// Persistent walk of the batch.  grid = resident blocks; dynamic LDS = stack_lds_entries * BLOCK * 4 (x2 for the 8-wide tree).
template <int BLOCK, bool COUNT>
__global__ __launch_bounds__(BLOCK) void k_closest(DevScene sc, ClosestArgs A, const uint2 * leaf_map, unsigned int fields,
                                                int keep_min, int node_min, unsigned int chunk, DevCounters * ctr) {
    extern __shared__ int s_stack[];
    LdsStack<BLOCK> stack;
    stack.attach(s_stack, threadIdx.x);
    stack.cap = A.stack_lds_entries;
    TraceStats st;
    ClosestJob<BLOCK, COUNT> job = { sc, A, leaf_map, fields, batch_pad(A) };
    wave_loop<BLOCK, COUNT>(job, stack, st, A.work + BATCH_W_HEAD, A.count, keep_min, node_min, chunk);
    if (COUNT) trace_stats_flush<true>(ctr, st);
}

// ---------------------------------------------------------------------------------------------------------
// Slow path of k_closest (exact_list_walk): the listed points again, from the start.
template <bool COUNT>
__global__ __launch_bounds__(256) void k_closest_exact(DevScene sc, ClosestArgs A, const uint2 * leaf_map, unsigned int fields,
                                                       DevCounters * ctr) {
    const float pad = batch_pad(A);
    exact_list_walk<COUNT>(A.slow, A.work[BATCH_W_SLOW], A.exact_stack, A.exact_stack_stride, ctr, [&](unsigned int idx, const GlobalStack & slow, TraceStats & st) {
        f3 p;
        float max_d2;
        (void)closest_query(A, idx, p, max_d2);                             // listed points are valid
        closest_emit(sc, A, leaf_map, fields, idx, closest_point_walk<GlobalStack, COUNT>(sc, p, max_d2, pad, slow, st, leaf_map));
    });
}

}  // namespace prt
