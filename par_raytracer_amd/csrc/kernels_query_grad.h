// kernels_query_grad.h - prt_trace_rays_backward on the device: dL/d(vertex positions), dL/d(origins), dL/d(directions) of a
// batch of closest-hit queries, from the gradients of their outputs (dev_query_grad.h has the per-ray step and the fixed point).
//
//   k_qgrad_scan     grid-stride, one lane per ray: resolves the ray's triangle from (group, vertex0), validates the reference,
//                    runs the step and reduces four words - the largest |vertex contribution| of the batch and the counts of
//                    contributing, skipped and invalid rays (one atomic per wave each: dev_wave_reduce.h).  Runs FIRST and
//                    writes only those words; the host reads them and launches nothing else when a reference is invalid, so a
//                    refused call has written none of the caller's outputs.
//   k_qgrad_scatter  reruns the step per ray, writes the ray's origin and direction gradients with plain stores and adds its 9
//                    vertex contributions, in units of 2^u, into 64-bit integer accumulators with no-return relaxed agent-scope
//                    atomics (accum_add's of dev_scene.h).  MERGE: the lanes of a wave that hit the same triangle - camera rays
//                    do, by the dozen - first sum their integers with shuffles, and one lane issues the 9 adds; a lane alone on
//                    its triangle adds directly (qgrad_wave_add9).  The sums are integers, so the merge changes no bit.
//   k_qgrad_resolve  one lane per vertex component: accumulator x 2^u -> the caller's float (overwrites).
//
// No lane waits for another workgroup: no spin loop, no polled flag, no cooperative launch.  The only ordering is that of the
// launches on the context's stream.
#pragma once

#include "dev_query_grad.h"
#include "dev_wave_reduce.h"

namespace prt {

enum { QGRAD_W_MAX = 0, QGRAD_W_HIT = 1, QGRAD_W_SKIPPED = 2, QGRAD_W_INVALID = 3, QGRAD_WORDS = 4 };

struct QGradArgs {
    const float * origins, * dirs;       // count x 3
    const int * group;                   // count: the forward query's hit references
    const unsigned int * vertex0;
    const float * positions;             // position_count x 3: the vertices the forward query saw
    const float * g_t, * g_bw, * g_pos, * g_nrm;      // the output gradients; null = zero
    float * g_origins, * g_dirs;         // count x 3 each; null = not wanted
    float * g_positions;                 // position_count x 3; null = not wanted
    const unsigned int * idx_positions;  // the upload's position index buffer
    const unsigned int * group_runs;     // (first_index, index_count) per group
    long long * acc;                     // position_count x 3 accumulators; null: the scatter adds nothing
    unsigned int * words;                // QGRAD_WORDS control words
    unsigned int count, group_count, position_count;
    float ray_bias;
    int unit_exponent;                   // u (set by the host between the scan and the scatter)
};

PRT_HD f3 qgrad_ld3(const float * p, size_t i) { return p ? mk3(p[3 * i], p[3 * i + 1], p[3 * i + 2]) : mk3(0.0f, 0.0f, 0.0f); }

// Ray i: QGRAD_MISS / QGRAD_INVALID, or QGRAD_HIT with vi = the three position indices and *ok = the step's verdict (false:
// skipped) and *g its result.  Position indices were validated at upload against the position count the entry point insists on.
PRT_HD int qgrad_ray(const QGradArgs & A, unsigned int i, unsigned int * first_corner, unsigned int * vi, bool * ok, QGradOut * g) {
    const int kind = qgrad_reference(A.group[i], A.vertex0[i], A.group_runs, A.group_count, first_corner);
    if (kind != QGRAD_HIT) return kind;
    for (int c = 0; c < 3; ++c) vi[c] = A.idx_positions[*first_corner + c];
    *ok = false;
    if (vi[0] >= A.position_count || vi[1] >= A.position_count || vi[2] >= A.position_count) return QGRAD_HIT;   // (never, after upload)
    *ok = qgrad_step(qgrad_ld3(A.origins, i), qgrad_ld3(A.dirs, i), A.ray_bias, qgrad_ld3(A.positions, vi[0]), qgrad_ld3(A.positions, vi[1]),
                     qgrad_ld3(A.positions, vi[2]), A.g_t ? A.g_t[i] : 0.0f, qgrad_ld3(A.g_bw, i), qgrad_ld3(A.g_pos, i), qgrad_ld3(A.g_nrm, i), g);
    return QGRAD_HIT;
}

// A scan's four words (k_qgrad_scan, k_cgrad_scan) from its lanes' partials.
PRT_D void qgrad_scan_words(unsigned int * words, float m, int hit, int skipped, int invalid) {
    wave_max_to_word(words + QGRAD_W_MAX, m);
    wave_sum_to_word(words + QGRAD_W_HIT, hit);
    wave_sum_to_word(words + QGRAD_W_SKIPPED, skipped);
    wave_sum_to_word(words + QGRAD_W_INVALID, invalid);
}

__global__ __launch_bounds__(256) void k_qgrad_scan(QGradArgs A) {
    float m = 0.0f;
    int hit = 0, skipped = 0, invalid = 0;
    for (unsigned int i = blockIdx.x * blockDim.x + threadIdx.x; i < A.count; i += gridDim.x * blockDim.x) {
        unsigned int first, vi[3];
        bool ok = false;
        QGradOut g;
        const int kind = qgrad_ray(A, i, &first, vi, &ok, &g);
        if (kind == QGRAD_INVALID) ++invalid;
        if (kind == QGRAD_HIT && !ok) ++skipped;
        if (kind == QGRAD_HIT && ok) { ++hit; m = fmaxf(m, qgrad_abs_max(g)); }
    }
    qgrad_scan_words(A.words, m, hit, skipped, invalid);
}

PRT_D void qgrad_add9(long long * acc, const unsigned int * vi, const long long * q) {
    for (int c = 0; c < 3; ++c)
        for (int k = 0; k < 3; ++k)
            __hip_atomic_fetch_add(reinterpret_cast<unsigned long long *>(acc + 3 * (size_t)vi[c] + k), (unsigned long long)q[3 * c + k],
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

PRT_D long long qgrad_shfl_xor64(long long v, int off) {
    const int lo = __shfl_xor((int)(unsigned int)((unsigned long long)v & 0xFFFFFFFFull), off);
    const int hi = __shfl_xor((int)(unsigned int)((unsigned long long)v >> 32), off);
    return (long long)((unsigned long long)(unsigned int)hi << 32 | (unsigned long long)(unsigned int)lo);
}

// The scatter's adds for one wave, written once for k_qgrad_scatter and k_cgrad_scatter (kernels_closest_grad.h).  Every lane of
// the wave calls it together; a live lane holds its triangle's key, its three position indices and its 9 integers.  MERGE: one
// pass per distinct triangle of the wave - the lanes on it sum their integers with xor-shuffles and the first of them issues
// the 9 adds; a lane alone on its triangle adds directly, after the loop, together with the other lone lanes.
template <bool MERGE>
PRT_D void qgrad_wave_add9(long long * acc, unsigned int lane, bool live, unsigned int key, const unsigned int * vi, const long long * q) {
    if (MERGE) {
        bool alone = false;
        unsigned long long todo = __ballot(live);
        while (todo) {                                                // one pass per distinct triangle of the wave
            const int leader = __ffsll((long long)todo) - 1;
            const unsigned int k = (unsigned int)__shfl((int)key, leader);
            const bool mine = live && key == k;
            const unsigned long long same = __ballot(mine);
            if (__popcll(same) == 1) {
                alone = alone || mine;                                // adds with the other lone lanes, after the loop
            } else {
                long long s[9];
                for (int c = 0; c < 9; ++c) {
                    s[c] = mine ? q[c] : 0;
                    for (int off = 32; off > 0; off >>= 1) s[c] += qgrad_shfl_xor64(s[c], off);
                }
                if ((int)lane == leader) qgrad_add9(acc, vi, s);
            }
            todo &= ~same;
        }
        if (alone) qgrad_add9(acc, vi, q);
    } else if (live) {
        qgrad_add9(acc, vi, q);
    }
}

// The loop runs per WAVE (its bound does not depend on the lane), so every lane of a wave reaches the ballots and shuffles of the
// merge together.  blockDim.x is a multiple of 64.
template <bool MERGE>
__global__ __launch_bounds__(256) void k_qgrad_scatter(QGradArgs A) {
    const unsigned int lane = threadIdx.x & 63u;
    for (unsigned int base = blockIdx.x * blockDim.x + (threadIdx.x - lane); base < A.count; base += gridDim.x * blockDim.x) {
        const unsigned int i = base + lane;
        unsigned int key = 0xFFFFFFFFu, vi[3] = { 0u, 0u, 0u };
        long long q[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };
        bool live = false;
        if (i < A.count) {
            QGradOut g;
            bool ok = false;
            const bool adds = qgrad_ray(A, i, &key, vi, &ok, &g) == QGRAD_HIT && ok;
            const f3 go = adds ? g.go : mk3(0.0f, 0.0f, 0.0f), gd = adds ? g.gd : mk3(0.0f, 0.0f, 0.0f);     // a miss, a skipped ray: zeros
            if (A.g_origins) { A.g_origins[3 * (size_t)i] = go.x; A.g_origins[3 * (size_t)i + 1] = go.y; A.g_origins[3 * (size_t)i + 2] = go.z; }
            if (A.g_dirs) { A.g_dirs[3 * (size_t)i] = gd.x; A.g_dirs[3 * (size_t)i + 1] = gd.y; A.g_dirs[3 * (size_t)i + 2] = gd.z; }
            live = adds && A.acc != nullptr;
            if (live) qgrad_fixed9(g, A.unit_exponent, q);
        }
        qgrad_wave_add9<MERGE>(A.acc, lane, live, key, vi, q);
    }
}

__global__ __launch_bounds__(256) void k_qgrad_resolve(QGradArgs A) {
    const unsigned int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 3u * A.position_count) return;
    A.g_positions[i] = qgrad_from_fixed(A.acc[i], A.unit_exponent);
}

}  // namespace prt
