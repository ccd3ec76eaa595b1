// kernels_hemi.h - prt_hemisphere_visibility (include/prt.h): for every point, how many of `samples` rays of the
// cosine lobe around its normal nothing occludes.  The rays are the definition of dev_hemi.h and exist in registers only.
//
//   k_hemi_pad     max |point component| over the pass's valid points, one word (device entry point only), for batch_pad; the
//                  host adds |ray_bias|, since directions are unit length.
//   k_hemi         the wave loop of dev_wave_loop.h over the any-hit traversal of dev_trace.h.  An item is e = i * samples + s:
//                  consecutive lanes share a point and its first node fetches.  start() makes the ray, routes it as k_query
//                  routes an OCCLUDED ray (ray_overflows and far origins go to the slow list) and starts the walk with the best
//                  hit at max_dist[i].  An item's answer is ONE BYTE, flags[e] = 1 for unoccluded: a plain store from the lane
//                  that owns the item, so no two lanes ever write one address.
//   k_hemi_exact   the listed items again on a full-height global stack, by k_query_exact<QUERY_OCCLUDED>'s choice of walk.
//   k_hemi_reduce  a point per lane (samples < 64) or per wave: counts the point's flags, sums the unoccluded directions in
//                  2^-32 fixed point when bent is asked for (the directions are made again, not stored), answers the invalid
//                  points and writes the outputs with plain vector stores.  Integer sums: the same bits under any schedule.
#pragma once

#include "dev_hemi.h"
#include "dev_wave_loop.h"
#include "dev_wave_reduce.h"
#include "kernels_query.h"

namespace prt {

enum { HF_UNOCCLUDED = 1, HF_VISIBILITY = 2, HF_BENT = 4 };
enum { HEMI_INVALID = 0, HEMI_MISS = 1, HEMI_RAY = 2 };
enum { HEMI_WAVE_SAMPLES = 64 };         // from this many samples on a wave reduces a point, below it a lane

// One pass: whole points, count * samples <= 2^30 items.
struct HemiArgs : BatchShared {
    const float * points;            // count x 3, the pass's first point on
    const float * normals;           // count x 3
    const float * max_dist;          // count; null = no limit
    unsigned int count;              // points of the pass
    unsigned int samples;
    unsigned int first;              // the global index of the pass's point 0
    unsigned long long seed;
    float ray_bias;
    unsigned char * flags;           // count x samples: 1 = unoccluded
    unsigned int * unoccluded;       // outputs, the pass's first point on (null unless the field's bit is in the mask)
    float * visibility;
    float * bent;                    // x3
    float replay_beyond;             // origins further out take query_any_unculled (query_far's rule)
    float scene_max;                 // the scene's largest |coordinate| (ray_overflows)
};

PRT_D f3 hemi_ld3(const float * p, unsigned int i) { return mk3(p[3 * (size_t)i], p[3 * (size_t)i + 1], p[3 * (size_t)i + 2]); }

// Sample s of point i of the pass: HEMI_INVALID (no ray: the point is), HEMI_MISS (a miss by definition) or HEMI_RAY with
// the biased origin and the direction.
PRT_D int hemi_item(const DevScene & sc, const HemiArgs & A, unsigned int i, unsigned int s, f3 & ob, f3 & d) {
    const f3 p = hemi_ld3(A.points, i), n = hemi_ld3(A.normals, i);
    if (!hemi_point_valid(p, n)) return HEMI_INVALID;
    const float4 ts = sc.diffuse_dirs[hemi_index(A.seed, A.first + i, s)];
    return hemi_ray(p, n, mk3(ts.x, ts.y, ts.z), A.ray_bias, ob, d) ? HEMI_RAY : HEMI_MISS;
}
PRT_D bool hemi_far(const HemiArgs & A, f3 ob) { return fmaxf(fmaxf(fabsf(ob.x), fabsf(ob.y)), fabsf(ob.z)) > A.replay_beyond; }
PRT_D float hemi_tmax(const HemiArgs & A, unsigned int i) { return A.max_dist ? A.max_dist[i] : 3.402823466e+38f; }

// ---------------------------------------------------------------------------------------------------------
// max |point component| of the valid points -> work[BATCH_W_EXTENT]
__global__ __launch_bounds__(256) void k_hemi_pad(HemiArgs A) {
    float m = 0.0f;
    for (unsigned int i = blockIdx.x * blockDim.x + threadIdx.x; i < A.count; i += gridDim.x * blockDim.x) {
        const f3 p = hemi_ld3(A.points, i), n = hemi_ld3(A.normals, i);
        if (hemi_point_valid(p, n)) m = fmaxf(m, fmaxf(fmaxf(fabsf(p.x), fabsf(p.y)), fabsf(p.z)));
    }
    wave_max_to_word(A.work + BATCH_W_EXTENT, m);
}

// The directions are unit length: a biased origin lies within |ray_bias| of its point.
PRT_D float hemi_pad(const HemiArgs & A) {
    return fmaxf(A.pad_max, __uint_as_float(A.work[BATCH_W_EXTENT]) + fabsf(A.ray_bias)) * (1.0f / 65536.0f);
}

// ---------------------------------------------------------------------------------------------------------
// k_hemi's job for the wave loop: a lane's item is one sample of one point.
template <int BLOCK, bool COUNT>
struct HemiJob : RaySteps<BLOCK, COUNT> {
    const HemiArgs & A;
    PRT_D bool start(unsigned int e, TravRay & r, const LdsStack<BLOCK> & stack) const {
        const unsigned int i = e / A.samples, s = e - i * A.samples;
        f3 ob, d;
        const int kind = hemi_item(this->sc, A, i, s, ob, d);
        if (kind == HEMI_RAY && (ray_overflows(A.scene_max, ob, d) || hemi_far(A, ob))) {
            batch_to_slow_list(A, e);                                       // scan_any_below / query_any_unculled
        } else if (kind == HEMI_RAY) {
            trav_start<true>(r, ob, d, TRACE_ANY, this->pad, stack);
            if (A.max_dist) r.best.t = A.max_dist[i];
            return true;
        } else {
            A.flags[e] = kind == HEMI_MISS ? 1 : 0;
        }
        return false;
    }
    PRT_D void finish(unsigned int e, const TravRay & r, const LdsStack<BLOCK> & stack) const {
        if (trav_needs_slow_path(r, stack)) batch_to_slow_list(A, e);
        else A.flags[e] = r.best.tri < 0 ? 1 : 0;
    }
};

// Persistent traversal of the pass.  grid = resident blocks; dynamic LDS = stack_lds_entries * BLOCK * 4.
template <int BLOCK, bool COUNT>
__global__ __launch_bounds__(BLOCK, 6) void k_hemi(DevScene sc, HemiArgs A, int keep_min, int node_min, unsigned int chunk, DevCounters * ctr) {
    extern __shared__ int s_stack[];
    LdsStack<BLOCK> stack;
    stack.attach(s_stack, threadIdx.x);
    stack.cap = A.stack_lds_entries;
    TraceStats st;
    HemiJob<BLOCK, COUNT> job = { { sc, hemi_pad(A) }, A };
    wave_loop<BLOCK, COUNT>(job, stack, st, A.work + BATCH_W_HEAD, A.count * A.samples, keep_min, node_min, chunk);
    if (COUNT) trace_stats_flush<true>(ctr, st);
}

// Slow path of k_hemi (exact_list_walk): the ray of item e is made again.
template <bool COUNT>
__global__ __launch_bounds__(256) void k_hemi_exact(DevScene sc, HemiArgs A, DevCounters * ctr) {
    const float pad = hemi_pad(A);
    exact_list_walk<COUNT>(A.slow, A.work[BATCH_W_SLOW], A.exact_stack, A.exact_stack_stride, ctr, [&](unsigned int e, const GlobalStack & slow, TraceStats & st) {
        const unsigned int i = e / A.samples, s = e - i * A.samples;
        f3 ob, d;
        (void)hemi_item(sc, A, i, s, ob, d);                                // listed items are rays
        HitRec h;
        if (ray_overflows(A.scene_max, ob, d)) h = scan_any_below<COUNT>(sc, ob, d, hemi_tmax(A, i), st);
        else if (hemi_far(A, ob)) h = query_any_unculled<GlobalStack, COUNT>(sc, ob, d, hemi_tmax(A, i), pad, slow, st);
        else h = query_any_below<GlobalStack, COUNT>(sc, ob, d, hemi_tmax(A, i), pad, slow, st);
        A.flags[e] = h.tri < 0 ? 1 : 0;
    });
}

// ---------------------------------------------------------------------------------------------------------
// The flags of samples s0, s0 + step, ... of point i into the count and, with BENT, the fixed-point sums.
template <bool BENT>
PRT_D void hemi_gather(const DevScene & sc, const HemiArgs & A, unsigned int i, unsigned int s0, unsigned int step, unsigned int & n,
                       long long & bx, long long & by, long long & bz) {
    const unsigned char * f = A.flags + (size_t)i * A.samples;
    for (unsigned int s = s0; s < A.samples; s += step) {
        if (!f[s]) continue;
        n++;
        if (BENT) {
            f3 ob, d;
            (void)hemi_item(sc, A, i, s, ob, d);
            bx += hemi_fix(d.x); by += hemi_fix(d.y); bz += hemi_fix(d.z);
        }
    }
}

PRT_D void hemi_emit(const HemiArgs & A, unsigned int fields, unsigned int i, bool valid, unsigned int n, long long bx, long long by, long long bz) {
    if (fields & HF_UNOCCLUDED) A.unoccluded[i] = valid ? n : 0xFFFFFFFFu;
    if (fields & HF_VISIBILITY) A.visibility[i] = valid ? hemi_visibility(n, A.samples) : 0.0f;
    if (fields & HF_BENT) {
        A.bent[3 * (size_t)i] = valid ? hemi_bent(bx, A.samples) : 0.0f;
        A.bent[3 * (size_t)i + 1] = valid ? hemi_bent(by, A.samples) : 0.0f;
        A.bent[3 * (size_t)i + 2] = valid ? hemi_bent(bz, A.samples) : 0.0f;
    }
}

// WAVE: a wave per point (its lanes stride over the samples), else a lane per point.  The rays cast - valid points x samples -
// go to ctr->ray_count, one add per wave.
template <bool WAVE, bool BENT>
__global__ __launch_bounds__(256) void k_hemi_reduce(DevScene sc, HemiArgs A, unsigned int fields, DevCounters * ctr) {
    const unsigned int gid = blockIdx.x * blockDim.x + threadIdx.x, lanes = gridDim.x * blockDim.x;
    int valid_points = 0;
    if (WAVE) {
        const unsigned int lane = threadIdx.x & 63u;
        for (unsigned int i = gid >> 6; i < A.count; i += lanes >> 6) {
            const bool valid = hemi_point_valid(hemi_ld3(A.points, i), hemi_ld3(A.normals, i));         // wave-uniform
            unsigned int n = 0;
            long long bx = 0, by = 0, bz = 0;
            if (valid) hemi_gather<BENT>(sc, A, i, lane, 64u, n, bx, by, bz);
            for (int off = 32; off > 0; off >>= 1) {
                n += (unsigned int)__shfl_xor((int)n, off);
                if (BENT) { bx += __shfl_xor(bx, off); by += __shfl_xor(by, off); bz += __shfl_xor(bz, off); }
            }
            if (lane == 0) {
                hemi_emit(A, fields, i, valid, n, bx, by, bz);
                valid_points += valid ? 1 : 0;
            }
        }
    } else {
        for (unsigned int i = gid; i < A.count; i += lanes) {
            const bool valid = hemi_point_valid(hemi_ld3(A.points, i), hemi_ld3(A.normals, i));
            unsigned int n = 0;
            long long bx = 0, by = 0, bz = 0;
            if (valid) hemi_gather<BENT>(sc, A, i, 0u, 1u, n, bx, by, bz);
            hemi_emit(A, fields, i, valid, n, bx, by, bz);
            valid_points += valid ? 1 : 0;
        }
    }
    for (int off = 32; off > 0; off >>= 1) valid_points += __shfl_xor(valid_points, off);
    if ((threadIdx.x & 63u) == 0u && valid_points)
        atomicAdd(&ctr->ray_count, (unsigned long long)valid_points * (unsigned long long)A.samples);
}

}  // namespace prt
