// kernels_sample_grad.h - prt_sample_surface_backward on the device: dL/d(vertex positions) of a batch of surface samples, from
// the gradients of their points and normals (dev_sample_grad.h has the per-sample step; the fixed point, the reference check and
// the wave merge are those of the ray queries' gradients: dev_query_grad.h, kernels_query_grad.h).
//
//   k_sgrad_scan     grid-stride, one lane per sample: resolves the sample's triangle from (group, vertex0), validates the
//                    reference, runs the step and reduces four words - the largest |vertex contribution| of the batch and the
//                    counts of contributing, skipped and invalid samples (qgrad_scan_words).  Runs FIRST and writes only those
//                    words; the host reads them and launches nothing else when a reference is invalid, so a refused call has
//                    written none of the caller's outputs.
//   k_sgrad_scatter  reruns the step per sample and adds its 9 vertex contributions, in units of 2^u, into the 64-bit integer
//                    accumulators.  MERGE: qgrad_wave_add9 - consecutive samples land on the same triangle where it is large.
//   k_qgrad_resolve  (kernels_query_grad.h, as it is) accumulator x 2^u -> the caller's float.
//
// No lane waits for another workgroup: no spin loop, no polled flag, no cooperative launch.  The only ordering is that of the
// launches on the context's stream.
#pragma once

#include "dev_sample_grad.h"
#include "kernels_query_grad.h"

namespace prt {

struct SGradArgs {
    const int * group;                   // count: the forward call's references
    const unsigned int * vertex0;
    const float * bw;                    // count x 3: the forward call's barycentrics
    const float * positions;             // position_count x 3: the vertices the forward call saw
    const float * g_point, * g_normal;   // the output gradients; null = zero
    const unsigned int * idx_positions;  // the upload's position index buffer
    const unsigned int * group_runs;     // (first_index, index_count) per group
    long long * acc;                     // position_count x 3 accumulators; null: the scatter adds nothing
    unsigned int * words;                // QGRAD_WORDS control words
    unsigned int count, group_count, position_count;
    int unit_exponent;                   // u (set by the host between the scan and the scatter)
};

// Sample i: QGRAD_MISS / QGRAD_INVALID, or QGRAD_HIT with vi = the three position indices, *ok = the step's verdict (false:
// skipped) and *g its result.  Position indices were validated at upload against the position count the entry point insists on.
PRT_HD int sgrad_sample(const SGradArgs & A, unsigned int i, unsigned int * first_corner, unsigned int * vi, bool * ok, SGradOut * g) {
    const int kind = qgrad_reference(A.group[i], A.vertex0[i], A.group_runs, A.group_count, first_corner);
    if (kind != QGRAD_HIT) return kind;
    for (int c = 0; c < 3; ++c) vi[c] = A.idx_positions[*first_corner + c];
    *ok = false;
    if (vi[0] >= A.position_count || vi[1] >= A.position_count || vi[2] >= A.position_count) return QGRAD_HIT;   // (never, after upload)
    *ok = sgrad_step(qgrad_ld3(A.positions, vi[0]), qgrad_ld3(A.positions, vi[1]), qgrad_ld3(A.positions, vi[2]), qgrad_ld3(A.bw, i),
                     qgrad_ld3(A.g_point, i), qgrad_ld3(A.g_normal, i), A.g_normal != nullptr, g);
    return QGRAD_HIT;
}

__global__ __launch_bounds__(256) void k_sgrad_scan(SGradArgs A) {
    float m = 0.0f;
    int hit = 0, skipped = 0, invalid = 0;
    for (unsigned int i = blockIdx.x * blockDim.x + threadIdx.x; i < A.count; i += gridDim.x * blockDim.x) {
        unsigned int first, vi[3];
        bool ok = false;
        SGradOut g;
        const int kind = sgrad_sample(A, i, &first, vi, &ok, &g);
        if (kind == QGRAD_INVALID) ++invalid;
        if (kind == QGRAD_HIT && !ok) ++skipped;
        if (kind == QGRAD_HIT && ok) { ++hit; m = fmaxf(m, sgrad_abs_max(g)); }
    }
    qgrad_scan_words(A.words, m, hit, skipped, invalid);
}

// The loop runs per WAVE (its bound does not depend on the lane), so every lane of a wave reaches the ballots and shuffles of the
// merge together.  blockDim.x is a multiple of 64.
template <bool MERGE>
__global__ __launch_bounds__(256) void k_sgrad_scatter(SGradArgs A) {
    const unsigned int lane = threadIdx.x & 63u;
    for (unsigned int base = blockIdx.x * blockDim.x + (threadIdx.x - lane); base < A.count; base += gridDim.x * blockDim.x) {
        const unsigned int i = base + lane;
        unsigned int key = 0xFFFFFFFFu, vi[3] = { 0u, 0u, 0u };
        long long q[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };
        bool live = false;
        if (i < A.count) {
            SGradOut g;
            bool ok = false;
            live = sgrad_sample(A, i, &key, vi, &ok, &g) == QGRAD_HIT && ok && A.acc != nullptr;
            if (live) sgrad_fixed9(g, A.unit_exponent, q);
        }
        qgrad_wave_add9<MERGE>(A.acc, lane, live, key, vi, q);
    }
}

}  // namespace prt
