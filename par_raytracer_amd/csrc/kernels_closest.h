// kernels_closest.h - nearest surface point for batches of points (prt_closest_points): the walk of dev_closest.h on points the
// caller supplies.
//
//   k_closest_pad    max |component| over the batch's finite points, one word (device entry point only: the host entry point
//                    computes it on the host).  pad = 2^-16 x max(scene, points of this batch), section 4.7's rule.
//   k_closest        PERSISTENT waves shaped like k_query: a per-lane LDS stack column, chunked atomic fetch of point indices,
//                    ballot / mbcnt refill of idle lanes under the context's KEEP_MIN / NODE_MIN, node steps and leaf steps in
//                    turn.  A point that is a miss by definition - a non-finite component, max_dist2 negative or NaN - is
//                    written at once.  A point whose push did not fit the LDS column goes to a list.
//   k_closest_exact  walks the listed points again, from the start, on a full-height global stack.
// Only the fields the caller asked for are written (a wave-uniform mask), with plain vector stores.
// prt_signed_distance runs the same two kernels with CF_SIGNED / CF_FEATURE in the mask and the tables of dev_signed.h in the
// arguments: closest_emit then signs the winner (signed_of_winner).  Without those bits nothing of it is read or executed.
#pragma once

#include "dev_signed.h"
#include "kernels_wave.h"            // lane_id

namespace prt {

enum { CF_DIST2 = 1, CF_POINT = 2, CF_BW = 4, CF_VERTEX0 = 8, CF_GROUP = 16, CF_SIGNED = 32, CF_FEATURE = 64 };

struct ClosestArgs {
    const float * points;            // count x 3
    const float * max_dist2;         // count, or null = no limit
    unsigned int count;
    // outputs (null unless the field's bit is in the mask)
    float * dist2;
    float * point;                   // x3
    float * bw;                      // x3
    unsigned int * vertex0;
    int * group;
    // [0] fetch head, [1] length of `slow`, [2] max |point component| as float bits (k_closest_pad)
    unsigned int * work;
    unsigned int * slow;             // point indices for k_closest_exact
    float pad_max;                   // max(scene, points) when the host computed it, else the scene's; pad = 2^-16 x max(this, work[2])
    unsigned int stack_lds_entries;
    int * exact_stack;               // k_closest_exact's full-height global stack columns
    unsigned int exact_stack_stride;
    // prt_signed_distance (null / unused unless CF_SIGNED or CF_FEATURE is in the mask)
    float * signed_dist;
    unsigned char * feature;
    SignedTables sign;
};

PRT_D float closest_pad(const ClosestArgs & A) {
    return fmaxf(A.pad_max, __uint_as_float(A.work[2])) * (1.0f / 65536.0f);
}

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
// max |component| of the finite points -> work[2] (non-negative floats order like their bits: one atomicMax)
__global__ __launch_bounds__(256) void k_closest_pad(ClosestArgs A) {
    float m = 0.0f;
    for (unsigned int i = blockIdx.x * blockDim.x + threadIdx.x; i < A.count; i += gridDim.x * blockDim.x) {
        const f3 p = mk3(A.points[3u * i], A.points[3u * i + 1u], A.points[3u * i + 2u]);
        if (closest_finite(p)) m = fmaxf(m, fmaxf(fmaxf(fabsf(p.x), fabsf(p.y)), fabsf(p.z)));
    }
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
    if ((threadIdx.x & 63u) == 0u && m > 0.0f) atomicMax(A.work + 2, __float_as_uint(m));
}

// ---------------------------------------------------------------------------------------------------------
// Persistent walk of the batch.  grid = resident blocks; dynamic LDS = stack_lds_entries * BLOCK * 4 (x2 for the 8-wide tree).
template <int BLOCK, bool COUNT>
__global__ __launch_bounds__(BLOCK) void k_closest(DevScene sc, ClosestArgs A, const uint2 * leaf_map, unsigned int fields,
                                                int keep_min, int node_min, unsigned int chunk, DevCounters * ctr) {
    extern __shared__ int s_stack[];
    LdsStack<BLOCK> stack;
    stack.attach(s_stack, threadIdx.x);
    stack.cap = A.stack_lds_entries;
    const unsigned int total = A.count;
    const unsigned int lane = lane_id();
    const float pad = closest_pad(A);
    unsigned int * head = A.work;

    TravRay r;
    trav_idle(r);
    int pt = -1;                         // batch index of the lane's point, -1 = idle
    bool exhausted = false;              // wave-uniform: the batch has no more points to hand out
    TraceStats st;

    unsigned int chunk_next = 0, chunk_end = 0;      // wave-uniform: points reserved for this wave, not yet handed out
    for (;;) {
        // ---- refill idle lanes from the wave's reserved chunk (as k_query); a point that is a miss by definition is written at once
        const unsigned long long idle = __ballot(pt < 0);
        if (idle != 0ull && !(exhausted && chunk_next == chunk_end)) {
            if (chunk_next == chunk_end) {
                unsigned int base = 0;
                if (lane == 0) base = atomicAdd(head, chunk);
                base = (unsigned int)__shfl((int)base, 0);
                if (base >= total) {
                    exhausted = true;
                } else {
                    chunk_next = base;
                    chunk_end = base + chunk < total ? base + chunk : total;
                }
            }
            const unsigned int avail = chunk_end - chunk_next;
            if (COUNT && avail && lane == 0) st.wrefills++;
            if (avail) {
                const unsigned int prefix = __builtin_amdgcn_mbcnt_hi((unsigned int)(idle >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)idle, 0u));
                const unsigned int n_idle = (unsigned int)__popcll(idle);
                const unsigned int take = n_idle < avail ? n_idle : avail;
                if (pt < 0 && prefix < take) {
                    const unsigned int idx = chunk_next + prefix;
                    f3 p;
                    float max_d2;
                    if (closest_query(A, idx, p, max_d2)) {
                        point_init(r, p, max_d2, stack);
                        pt = (int)idx;
                    } else {
                        HitRec miss;
                        miss.t = 3.402823466e+38f; miss.v = miss.w = 0.0f; miss.tri = -1;
                        closest_emit(sc, A, leaf_map, fields, idx, miss);
                    }
                }
                chunk_next += take;
            }
        }
        if (__ballot(pt >= 0) == 0ull) {
            if (exhausted && chunk_next == chunk_end) break;
            continue;                    // every point of the refill was a miss by definition: refill again
        }

        // ---- walk until fewer than `leave_below` lanes of the wave are still busy (k_query's loop)
        const int leave_below = (exhausted && chunk_next == chunk_end) ? 1 : keep_min;
        while (pt >= 0) {
            const int walkers = __popcll(__ballot(trav_walking(r)));
            const int nmin = node_min < (walkers >> 1) ? node_min : (walkers >> 1);
            while (trav_walking(r)) {
                point_node_step<LdsStack<BLOCK>, COUNT>(sc, r, stack, st, pad);
                if (__popcll(__ballot(trav_walking(r))) < nmin) break;
            }
            if (!trav_done(r) && !trav_walking(r)) point_leaf<LdsStack<BLOCK>, COUNT>(sc, r, stack, st, leaf_map);
            if (trav_done(r)) {
                if (trav_end_flags(r, stack) & TRAV_FLAG_OVERFLOW) A.slow[atomicAdd(A.work + 1, 1u)] = (unsigned int)pt;
                else closest_emit(sc, A, leaf_map, fields, (unsigned int)pt, r.best);
                pt = -1;
                break;
            }
            if (__popcll(__ballot(true)) < leave_below) break;
        }
    }
    if (COUNT) trace_stats_flush<true>(ctr, st);
}

// ---------------------------------------------------------------------------------------------------------
// Slow path of k_closest (as k_query_exact is k_query's): a small fixed grid that reads the list length on the device.
template <bool COUNT>
__global__ __launch_bounds__(256) void k_closest_exact(DevScene sc, ClosestArgs A, const uint2 * leaf_map, unsigned int fields,
                                                       DevCounters * ctr) {
    const unsigned int gid = blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned int n_slow = A.work[1];
    const float pad = closest_pad(A);
    TraceStats st;
    GlobalStack slow;
    slow.attach(A.exact_stack, gid, A.exact_stack_stride);
    for (unsigned int i = gid; i < n_slow; i += gridDim.x * blockDim.x) {
        const unsigned int idx = A.slow[i];
        f3 p;
        float max_d2;
        (void)closest_query(A, idx, p, max_d2);                             // listed points are valid
        const HitRec h = closest_point_walk<GlobalStack, COUNT>(sc, p, max_d2, pad, slow, st, leaf_map);
        closest_emit(sc, A, leaf_map, fields, idx, h);
    }
    if (COUNT) trace_stats_flush<false>(ctr, st);
}

}  // namespace prt
