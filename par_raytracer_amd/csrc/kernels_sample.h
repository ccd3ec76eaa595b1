// kernels_sample.h - prt_sample_surface on the device (dev_sample.h has the definition): the prefix sums of the triangles' fixed-
// point weights, rebuilt from the records as they lie on the device now, and the sampling kernel.
//
// THE TABLE: reduce-then-scan in four launches on the context's stream (prt_api.hip: ensure_sample_table), by the first sampling
// call after an upload or after a prt_update_geometry.  A tile is SAMPLE_TILE = 256 triangles, one per lane of a block.
//   k_sample_weights  grid-stride, one lane per INPUT triangle: reads its record through slot_of_input, writes the double weight and
//                     reduces the largest bit pattern - over the wave with xor-shuffles, then one 64-bit integer atomicMax per wave.
//   k_sample_tiles    grid-stride over tiles: W = the weight in units of 2^u, u from the device-resident maximum; an inclusive scan
//                     inside the block (shuffles inside a wave, the four wave totals through LDS) into C; the tile's total into
//                     tile_sum; the count of W > 0 into the words (one atomic per wave).
//   k_sample_totals   ONE block: an exclusive scan of tile_sum in place, SAMPLE_TILE tiles per pass of its loop with a running
//                     carry (2^26 triangles are 2^18 tiles: 1024 passes); the grand total T into the words.
//   k_sample_offsets  grid-stride, one lane per triangle: C[t] += tile_sum[t / SAMPLE_TILE].
// Integer sums: every scan order gives the same C.  No lane waits for another workgroup: no look-back, no spin loop, no polled
// flag, no cooperative launch; the only ordering is that of the launches on the stream.
//
// k_sample: one lane per sample in a grid-stride loop - seed, three draws, the binary search of C, the record through
// slot_of_input, and plain stores of the requested fields only (the mask is a kernel argument: wave-uniform).
#pragma once

#include "dev_sample.h"

namespace prt {

enum { SAMPLE_TILE = 256 };
enum { SF_POINT = 1, SF_BW = 2, SF_NORMAL = 4, SF_VERTEX0 = 8, SF_GROUP = 16 };
// The table's control words (64-bit each).
enum { SAMPLE_W_MAX = 0, SAMPLE_W_TOTAL = 1, SAMPLE_W_LIVE = 2, SAMPLE_WORDS = 3 };

struct SampleTable {
    const float4 * tris;                 // the records, in leaf-slot order
    const unsigned int * slot_of_input;  // input triangle -> leaf slot
    double * weight;                     // per input triangle
    unsigned long long * C;              // inclusive prefix sums of W, per input triangle
    unsigned long long * tile_sum;       // per tile: its total, then (k_sample_totals) the sum of the tiles before it
    unsigned long long * words;          // SAMPLE_WORDS
    unsigned int n_tris, n_tiles;
};

struct SampleArgs {
    unsigned long long seed, first;      // sample i of the call is sample first + i of the seed
    unsigned int count;
    float * point, * bw, * normal;       // x3 each (null unless the field's bit is in the mask)
    unsigned int * vertex0;
    int * group;
};

PRT_D unsigned long long sample_shfl_xor64(unsigned long long v, int off) {
    const unsigned int lo = (unsigned int)__shfl_xor((int)(unsigned int)(v & 0xFFFFFFFFull), off);
    const unsigned int hi = (unsigned int)__shfl_xor((int)(unsigned int)(v >> 32), off);
    return (unsigned long long)hi << 32 | lo;
}
PRT_D unsigned long long sample_shfl_up64(unsigned long long v, unsigned int off) {
    const unsigned int lo = (unsigned int)__shfl_up((int)(unsigned int)(v & 0xFFFFFFFFull), off);
    const unsigned int hi = (unsigned int)__shfl_up((int)(unsigned int)(v >> 32), off);
    return (unsigned long long)hi << 32 | lo;
}

// Inclusive scan of v over the block's 256 lanes; *total = the block's sum.  lds: 4 words.  Every lane of the block calls it
// together; the closing barrier lets the caller call it again.
PRT_D unsigned long long sample_block_scan(unsigned long long v, unsigned long long * lds, unsigned long long * total) {
    const unsigned int lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (unsigned int off = 1u; off < 64u; off <<= 1) {
        const unsigned long long up = sample_shfl_up64(v, off);
        if (lane >= off) v += up;
    }
    if (lane == 63u) lds[wave] = v;
    __syncthreads();
    unsigned long long before = 0ull, all = 0ull;
    for (unsigned int k = 0u; k < 4u; ++k) {
        const unsigned long long s = lds[k];
        if (k < wave) before += s;
        all += s;
    }
    __syncthreads();
    *total = all;
    return v + before;
}

__global__ __launch_bounds__(256) void k_sample_weights(SampleTable T) {
    unsigned long long m = 0ull;
    for (unsigned int t = blockIdx.x * blockDim.x + threadIdx.x; t < T.n_tris; t += gridDim.x * blockDim.x) {
        const float4 * tp = T.tris + 3u * (size_t)T.slot_of_input[t];
        const float4 r0 = tp[0], r1 = tp[1], r2 = tp[2];
        const double w = sample_weight(mk3(r0.w, r1.x, r1.y), mk3(r1.z, r1.w, r2.x));
        T.weight[t] = w;
        const unsigned long long b = sample_double_bits(w);
        m = b > m ? b : m;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = sample_shfl_xor64(m, off);
        m = o > m ? o : m;
    }
    if ((threadIdx.x & 63u) == 0u && m) atomicMax(T.words + SAMPLE_W_MAX, m);
}

// The loop's bound does not depend on the lane: every lane of the block reaches the scan's shuffles and barriers together.
__global__ __launch_bounds__(256) void k_sample_tiles(SampleTable T) {
    __shared__ unsigned long long lds[4];
    const unsigned long long max_bits = T.words[SAMPLE_W_MAX];
    const int u = sample_unit_exponent(max_bits, T.n_tris);
    unsigned int live = 0u;
    for (unsigned int tile = blockIdx.x; tile < T.n_tiles; tile += gridDim.x) {
        const unsigned int t = tile * (unsigned int)SAMPLE_TILE + threadIdx.x;
        const unsigned long long W = (t < T.n_tris && max_bits) ? sample_to_fixed(T.weight[t], u) : 0ull;
        live += W ? 1u : 0u;
        unsigned long long total;
        const unsigned long long c = sample_block_scan(W, lds, &total);
        if (t < T.n_tris) T.C[t] = c;
        if (threadIdx.x == 0u) T.tile_sum[tile] = total;
    }
    for (int off = 32; off > 0; off >>= 1) live += (unsigned int)__shfl_xor((int)live, off);
    if ((threadIdx.x & 63u) == 0u && live) atomicAdd(T.words + SAMPLE_W_LIVE, (unsigned long long)live);
}

// <<<1, 256>>>
__global__ __launch_bounds__(256) void k_sample_totals(SampleTable T) {
    __shared__ unsigned long long lds[4];
    unsigned long long carry = 0ull;
    for (unsigned int base = 0u; base < T.n_tiles; base += (unsigned int)SAMPLE_TILE) {
        const unsigned int i = base + threadIdx.x;
        const unsigned long long v = i < T.n_tiles ? T.tile_sum[i] : 0ull;
        unsigned long long total;
        const unsigned long long c = sample_block_scan(v, lds, &total);
        if (i < T.n_tiles) T.tile_sum[i] = carry + (c - v);
        carry += total;
    }
    if (threadIdx.x == 0u) T.words[SAMPLE_W_TOTAL] = carry;
}

__global__ __launch_bounds__(256) void k_sample_offsets(SampleTable T) {
    for (unsigned int t = blockIdx.x * blockDim.x + threadIdx.x; t < T.n_tris; t += gridDim.x * blockDim.x)
        T.C[t] += T.tile_sum[t / (unsigned int)SAMPLE_TILE];
}

__global__ __launch_bounds__(256) void k_sample(SampleTable T, SampleArgs A, const uint2 * leaf_map, unsigned int fields) {
    const unsigned long long total = T.words[SAMPLE_W_TOTAL];
    // (a 64-bit index: a count near 2^32 must not wrap the stride)
    for (unsigned long long i = blockIdx.x * blockDim.x + threadIdx.x; i < A.count; i += gridDim.x * blockDim.x) {
        const bool hit = total != 0ull;
        f3 p = mk3(0.0f, 0.0f, 0.0f), b = p, n = p;
        uint2 m = make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);                    // (group, vertex0)
        if (hit) {
            const SampleDraw d = sample_draw(A.seed, A.first + i);
            const unsigned int t = sample_pick(T.C, T.n_tris, sample_mulhi64(d.r0, total));
            const unsigned int slot = T.slot_of_input[t];
            const float4 * tp = T.tris + 3u * (size_t)slot;
            const float4 r0 = tp[0], r1 = tp[1], r2 = tp[2];
            const f3 a = mk3(r0.x, r0.y, r0.z), ab = mk3(r0.w, r1.x, r1.y), ac = mk3(r1.z, r1.w, r2.x);
            p = sample_point(a, ab, ac, d.v, d.w);
            b = sample_bw(d.v, d.w);
            if (fields & SF_NORMAL) n = sample_normal(ab, ac);
            if (fields & (SF_VERTEX0 | SF_GROUP)) m = leaf_map[slot];
        }
        const size_t at = 3u * (size_t)i;
        if (fields & SF_POINT) { A.point[at] = p.x; A.point[at + 1u] = p.y; A.point[at + 2u] = p.z; }
        if (fields & SF_BW) { A.bw[at] = b.x; A.bw[at + 1u] = b.y; A.bw[at + 2u] = b.z; }
        if (fields & SF_NORMAL) { A.normal[at] = n.x; A.normal[at + 1u] = n.y; A.normal[at + 2u] = n.z; }
        if (fields & SF_GROUP) A.group[i] = (int)m.x;
        if (fields & SF_VERTEX0) A.vertex0[i] = m.y;
    }
}

}  // namespace prt
