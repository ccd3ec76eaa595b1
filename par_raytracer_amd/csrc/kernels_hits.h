// kernels_hits.h - a ray's K nearest hits (prt_trace_hits): the walk of dev_hits.h on rays the caller supplies.
//
//   k_query_pad    (kernels_query.h) the batch's extent for batch_pad, device entry point only: HitsArgs is a QueryArgs.
//   k_hits         the wave loop of dev_wave_loop.h over the node steps of dev_trace.h and the leaf step of dev_hits.h.  A lane's
//                  sorted list lives in a column of the dynamic LDS behind the stack columns, 2 * k words per lane.  A ray that
//                  is a miss by definition, or whose tmax admits nothing (0, negative, NaN), is written at once.  Rays from far
//                  origins (query_far) and rays whose triangle test overflows (ray_overflows) go to a list at the start, a ray
//                  whose push did not fit the LDS stack column at its end.
//   k_hits_exact   the listed rays again, from the start, on a full-height global stack and a global list column: the culled
//                  walk, the walk with boxes culled by geometry only (far origins), or the scan of every record (overflow).
// Only the fields the caller asked for are written (a wave-uniform mask), with plain vector stores.
#pragma once

#include "dev_hits.h"
#include "kernels_query.h"

namespace prt {

enum { HITF_COUNT = 1, HITF_T = 2, HITF_BW = 4, HITF_VERTEX0 = 8, HITF_GROUP = 16, HITF_BACK = 32 };

// QueryArgs' rays (origins, dirs, tmax, count, ray_bias), its t, bw, vertex0 and group - here count x k each - and:
struct HitsArgs : QueryArgs {
    unsigned int k;                  // slots per ray, 1..HITS_MAX
    const float * after_t;           // the cursor, count each; all null or all given
    const int * after_group;
    const unsigned int * after_vertex0;
    unsigned int * hit_count;        // outputs (null unless the field's bit is in the mask)
    unsigned char * back;
    int * exact_lists;               // the exact kernel's list columns, 2 * HITS_MAX words per lane, stride exact_stack_stride
};

PRT_D float hits_tmax(const HitsArgs & A, unsigned int i) { return A.tmax ? A.tmax[i] : 3.402823466e+38f; }
PRT_D HitsCursor hits_cursor(const HitsArgs & A, unsigned int i) {
    HitsCursor c = hits_no_cursor();
    if (A.after_t) { c.t = A.after_t[i]; c.group = A.after_group[i]; c.vertex0 = A.after_vertex0[i]; }
    return c;
}

// Ray i's n entries into the requested fields; slots from n on hold the queries' miss record.
template <class LIST>
PRT_D void hits_emit(const DevScene & sc, const HitsArgs & A, const uint2 * leaf_map, unsigned int fields, unsigned int i, f3 ob, f3 d,
                     const LIST & list, unsigned int n) {
    if (fields & HITF_COUNT) A.hit_count[i] = n;
    if (!(fields & ~(unsigned int)HITF_COUNT)) return;
    const f3 qp = ob - (ob + d);
    for (unsigned int s = 0; s < A.k; ++s) {
        const HitSlot h = s < n ? hits_slot(sc, list, leaf_map, ob, qp, s) : hits_slot_miss();
        const size_t at = (size_t)i * A.k + s;
        if (fields & HITF_T) A.t[at] = h.t;
        if (fields & HITF_BW) {
            A.bw[3u * at] = s < n ? 1.0f - h.v - h.w : 0.0f;               // raytracer.cpp:120
            A.bw[3u * at + 1u] = h.v;
            A.bw[3u * at + 2u] = h.w;
        }
        if (fields & HITF_VERTEX0) A.vertex0[at] = h.m.y;
        if (fields & HITF_GROUP) A.group[at] = (int)h.m.x;
        if (fields & HITF_BACK) A.back[at] = (unsigned char)h.back;
    }
}

// ---------------------------------------------------------------------------------------------------------
// k_hits' job for the wave loop: a lane's item is a ray of the batch.  The item's index rides in best.v (as bits), for the
// cursor's three loads in the leaf step.
template <int BLOCK, bool BACK, bool COUNT>
struct HitsJob : RaySteps<BLOCK, COUNT> {
    const HitsArgs & A;
    const uint2 * leaf_map;
    unsigned int fields;
    LdsHitList<BLOCK> list;
    PRT_D bool start(unsigned int idx, TravRay & r, const LdsStack<BLOCK> & stack) const {
        f3 ob, d;
        const bool valid = query_ray(A, idx, ob, d);
        const float tmax = hits_tmax(A, idx);
        if (valid && tmax > 0.0f && (query_overflows(A, ob, d) || query_far(A, ob))) {
            batch_to_slow_list(A, idx);                                     // hits_scan / the unculled walk
        } else if (valid && tmax > 0.0f) {                                  // (a NaN tmax fails the comparison)
            hits_start(r, ob, d, tmax, this->pad, stack);
            r.best.v = as_f((int)idx);
            return true;
        } else {
            hits_emit(this->sc, A, leaf_map, fields, idx, ob, d, list, 0u);
        }
        return false;
    }
    PRT_D bool leaf(TravRay & r, const LdsStack<BLOCK> & stack, TraceStats & st) const {
        float unused = 0.0f;
        hits_leaf<LdsStack<BLOCK>, LdsHitList<BLOCK>, BACK, COUNT, true>(this->sc, r, stack, st, list, A.k, hits_cursor(A, (unsigned int)as_i(r.best.v)),
                                                                         leaf_map, unused);
        return trav_done(r);
    }
    PRT_D void finish(unsigned int idx, const TravRay & r, const LdsStack<BLOCK> & stack) const {
        if (trav_end_flags(r, stack) & TRAV_FLAG_OVERFLOW) batch_to_slow_list(A, idx);
        else hits_emit(this->sc, A, leaf_map, fields, idx, r.o, r.d, list, (unsigned int)r.best.tri);       // r.o: the biased origin
    }
};

// Persistent walk of the batch.  grid = resident blocks; dynamic LDS = (stack_lds_entries * STACK_ENTRY_INTS + 2 * k) * BLOCK * 4.
template <int BLOCK, bool BACK, bool COUNT>
__global__ __launch_bounds__(BLOCK) void k_hits(DevScene sc, HitsArgs A, const uint2 * leaf_map, unsigned int fields,
                                             int keep_min, int node_min, unsigned int chunk, DevCounters * ctr) {
    extern __shared__ int s_stack[];
    LdsStack<BLOCK> stack;
    stack.attach(s_stack, threadIdx.x);
    stack.cap = A.stack_lds_entries;
    TraceStats st;
    HitsJob<BLOCK, BACK, COUNT> job = { { sc, batch_pad(A) }, A, leaf_map, fields, {} };
    job.list.attach(s_stack + A.stack_lds_entries * (unsigned int)STACK_ENTRY_INTS * (unsigned int)BLOCK, threadIdx.x);
    wave_loop<BLOCK, COUNT>(job, stack, st, A.work + BATCH_W_HEAD, A.count, keep_min, node_min, chunk);
    if (COUNT) trace_stats_flush<true>(ctr, st);
}

// ---------------------------------------------------------------------------------------------------------
// Slow path of k_hits (exact_list_walk): the listed rays again, from the start.
template <bool BACK, bool COUNT>
__global__ __launch_bounds__(256) void k_hits_exact(DevScene sc, HitsArgs A, const uint2 * leaf_map, unsigned int fields,
                                                    DevCounters * ctr) {
    const float pad = batch_pad(A);
    GlobalHitList list;
    list.attach(A.exact_lists, blockIdx.x * blockDim.x + threadIdx.x, A.exact_stack_stride);
    exact_list_walk<COUNT>(A.slow, A.work[BATCH_W_SLOW], A.exact_stack, A.exact_stack_stride, ctr, [&](unsigned int idx, const GlobalStack & slow, TraceStats & st) {
        f3 ob, d;
        (void)query_ray(A, idx, ob, d);                                     // listed rays are valid, and their tmax admits something
        const float tmax = hits_tmax(A, idx);
        const HitsCursor cur = hits_cursor(A, idx);
        unsigned int n;
        if (query_overflows(A, ob, d)) n = hits_scan<GlobalHitList, BACK, COUNT>(sc, ob, d, tmax, st, list, A.k, cur, leaf_map);
        else if (query_far(A, ob)) n = hits_walk<GlobalStack, GlobalHitList, BACK, COUNT, false>(sc, ob, d, tmax, pad, slow, st, list, A.k, cur, leaf_map);
        else n = hits_walk<GlobalStack, GlobalHitList, BACK, COUNT, true>(sc, ob, d, tmax, pad, slow, st, list, A.k, cur, leaf_map);
        hits_emit(sc, A, leaf_map, fields, idx, ob, d, list, n);
    });
}

}  // namespace prt
