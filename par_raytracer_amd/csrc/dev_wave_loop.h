// dev_wave_loop.h - what the persistent traversal kernels (k_trace, k_query, k_closest) and their slow-path kernels share,
// written once: the wave loop, the slow path's skeleton, the counters' flush and a batch's shared words.
//
// wave_loop: PERSISTENT waves pull items (rays, points) through one atomic head word.  A lane that finishes its item goes idle;
// when fewer than KEEP_MIN lanes of a wave are still busy, the wave leaves the walk, compacts its idle lanes with ballot / mbcnt
// and refills them with the next items.  Traversal state (node, stack pointer, best hit) stays in registers + the per-lane LDS
// stack column across refills.  A kernel hands the loop a JOB with what is its own:
//   bool start(idx, r, stack)        item idx becomes the lane's walk (true), or is answered at once and the lane stays idle
//   void node_step(r, stack, st)     one node step of a walking lane
//   bool leaf(r, stack, st)          one leaf step of a lane that holds a leaf; true when the item has ended
//   void finish(idx, r, stack)       the ended item's answer is stored, or its index goes to the slow path's list
#pragma once

#include "dev_trace.h"

namespace prt {

PRT_D unsigned int lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }

// A kernel's TraceStats into the context's counters.  FULL: the persistent kernels' wave-level counters too; else what the
// slow kernels count.  (culled and k_pool's own counters stay with the kernels that report them.)
template <bool FULL>
PRT_D void trace_stats_flush(DevCounters * ctr, const TraceStats & st) {
    atomicAdd(&ctr->node_visits, (unsigned long long)st.nodes);
    atomicAdd(&ctr->tri_tests, (unsigned long long)st.tris);
    if (FULL) {
        atomicAdd(&ctr->wave_node_steps, (unsigned long long)st.wnodes);
        atomicAdd(&ctr->wave_leaf_steps, (unsigned long long)st.wleaves);
        atomicAdd(&ctr->wave_tri_steps, (unsigned long long)st.wtris);
        atomicAdd(&ctr->wave_refills, (unsigned long long)st.wrefills);
        atomicMax(&ctr->max_sp, (unsigned long long)st.max_sp);
    }
    if (st.cone_culls) atomicAdd(&ctr->cone_culled_nodes, (unsigned long long)st.cone_culls);
}

// Items 0 .. total, handed out through *head in chunks.  COUNT: the refills are counted (st.wrefills).
template <int BLOCK, bool COUNT, class Job>
PRT_D void wave_loop(Job & job, const LdsStack<BLOCK> & stack, TraceStats & st, unsigned int * head, unsigned int total, int keep_min,
                     int node_min, unsigned int chunk) {
    const unsigned int lane = lane_id();
    TravRay r;
    trav_idle(r);
    int item = -1;                       // index of the lane's item, -1 = idle
    bool exhausted = false;              // wave-uniform: the head has no more items to hand out
    unsigned int chunk_next = 0, chunk_end = 0;      // wave-uniform: items reserved for this wave, not yet handed out
    for (;;) {
        // ---- refill idle lanes from the wave's reserved chunk; reserve a new chunk when it runs dry.
        // One atomic per CHUNK items, not per refill: the head word is a single address (~90 atomics/us chip-wide).
        const unsigned long long idle = __ballot(item < 0);
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
                if (item < 0 && prefix < take) {
                    const unsigned int idx = chunk_next + prefix;
                    if (job.start(idx, r, stack)) item = (int)idx;
                }
                chunk_next += take;
            }
        }
        if (__ballot(item >= 0) == 0ull) {
            // Every item of the refill was answered at once: refill again.  (A job whose start() always walks, k_trace's, comes
            // here only with avail == 0, which is exhausted with an empty chunk: it leaves.)
            if (exhausted && chunk_next == chunk_end) break;
            continue;
        }

        // ---- walk until fewer than `leave_below` lanes of the wave are still busy
        const int leave_below = (exhausted && chunk_next == chunk_end) ? 1 : keep_min;
        while (item >= 0) {
            // Node phase.  Lanes drop out as they reach a leaf; once fewer than `node_min` lanes are still
            // walking, the stragglers are suspended too (they keep their node) so the wave can run the leaf
            // phase for the majority instead of idling behind the longest walk.
            const int walkers = __popcll(__ballot(trav_walking(r)));
            const int nmin = node_min < (walkers >> 1) ? node_min : (walkers >> 1);
            while (trav_walking(r)) {
                job.node_step(r, stack, st);
                if (__popcll(__ballot(trav_walking(r))) < nmin) break;
            }
            const bool fin = (!trav_done(r) && !trav_walking(r)) ? job.leaf(r, stack, st) : trav_done(r);
            if (fin) {
                job.finish((unsigned int)item, r, stack);
                item = -1;
                break;
            }
            if (__popcll(__ballot(true)) < leave_below) break;
        }
    }
}

// A job's node and leaf steps for rays (k_trace, k_query): the traversal of dev_trace.h under box pad `pad`.
template <int BLOCK, bool COUNT, bool CONES = false>
struct RaySteps {
    const DevScene & sc;
    float pad;
    PRT_D void node_step(TravRay & r, const LdsStack<BLOCK> & stack, TraceStats & st) const { trav_node_step<LdsStack<BLOCK>, COUNT, CONES>(sc, r, stack, st, pad); }
    PRT_D bool leaf(TravRay & r, const LdsStack<BLOCK> & stack, TraceStats & st) const { return trav_leaf<LdsStack<BLOCK>, COUNT>(sc, r, stack, st); }
};

// The slow-path kernels' skeleton (k_trace_exact, k_query_exact, k_closest_exact): a small fixed grid launched after the
// persistent kernel walks list[0 .. n) - n is read on the device, no host round trip, and is normally 0 -, every lane on its own
// full-height global stack column.  body(idx, stack, st) traces item idx again and stores its answer.
template <bool COUNT, class Body>
PRT_D void exact_list_walk(const unsigned int * list, unsigned int n, int * columns, unsigned int stride, DevCounters * ctr, const Body & body) {
    const unsigned int gid = blockIdx.x * blockDim.x + threadIdx.x;
    TraceStats st;
    GlobalStack slow;
    slow.attach(columns, gid, stride);
    for (unsigned int i = gid; i < n; i += gridDim.x * blockDim.x) body(list[i], slow, st);
    if (COUNT) trace_stats_flush<false>(ctr, st);
}

// What the batched queries' argument structs (QueryArgs, ClosestArgs) share: the batch's control words, its slow list and the
// stacks.  The host fills it in one place (run_batch, prt_api.hip).
enum { BATCH_W_HEAD = 0,             // wave_loop's fetch head
       BATCH_W_SLOW = 1,             // length of `slow`
       BATCH_W_EXTENT = 2,           // max |coordinate| of the batch's valid items as float bits (the pad kernels); 0 when the host computed it
       BATCH_WORDS = 4 };
struct BatchShared {
    unsigned int * work;             // BATCH_WORDS control words
    unsigned int * slow;             // item indices for the exact kernel
    float pad_max;                   // max(scene, batch) when the host computed it, else the scene's
    unsigned int stack_lds_entries;
    int * exact_stack;               // the exact kernel's full-height global stack columns
    unsigned int exact_stack_stride;
};
// The box pad of dev_trace_common.h assumes items near the scene; a batch's can be anywhere, so its pad is 2^-16 x the largest
// |coordinate| of the scene and of this batch's valid items.
PRT_D float batch_pad(const BatchShared & S) {
    return fmaxf(S.pad_max, __uint_as_float(S.work[BATCH_W_EXTENT])) * (1.0f / 65536.0f);
}
PRT_D void batch_to_slow_list(const BatchShared & S, unsigned int idx) { S.slow[atomicAdd(S.work + BATCH_W_SLOW, 1u)] = idx; }

}  // namespace prt
