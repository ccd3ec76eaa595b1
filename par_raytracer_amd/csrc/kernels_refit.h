// kernels_refit.h - prt_update_geometry on the device: the uploaded scene's vertices move, the tree's boxes follow them.
//
//   k_refit_bounds   grid-stride reduction over the positions the triangles reference: max |coordinate| (wave_max_to_word of
//                    dev_wave_reduce.h) and a flag for a coordinate that is not finite or not below 1e18 (the
//                    upload's rule).  Runs FIRST and writes two words of its own; the host reads them and launches nothing else
//                    when the flag is set, so a refused update has modified nothing of the scene.
//   k_refit_records  one lane per leaf slot: gathers the triangle's three positions through the table (dev_refit.h) and writes
//                    the 48 B `tris` record (a, ab, ac, n) in the upload's float expressions and order - the library is built
//                    with -ffp-contract=off, so Cross(ab, ac) gives the host's bits -, the geometric normal in the shade
//                    record, and - when the caller passed them - the vertex normals and tangents.  The material word and the
//                    texture coordinates are not touched.  Plain 16-byte vector stores.
//   k_refit_level    one launch per tree level, deepest first; one lane per node runs refit_step of dev_refit.h (both widths)
//                    and writes back the node's geometry dwords only.
//
// No lane ever waits for another workgroup: there is no spin loop, no polled flag, no cooperative launch.  A level reads the
// exact boxes the level below stored in the scratch array, and the only ordering is that of launches on one stream - which also
// makes the stores of one launch visible to the next.  A few dozen launches of microseconds each; they cannot hang.
//
// The 8-wide slot order (and the 4-wide largest-first order) is NOT re-sorted: it only steers the visiting order (dev_refit.h).
#pragma once

#include "dev_refit.h"
#include "dev_scene.h"
#include "dev_wave_reduce.h"

namespace prt {

struct RefitArgs {
    const float * positions;         // the new positions, xyz (device)
    const float * normals;           // the new normals or null (= keep)
    const float * tangents;          // the new tangents or null; only with normals' indices, only for scenes with bump maps
    const unsigned int * table;      // leaf slot -> three position indices, three normal indices (REFIT_TABLE_WORDS)
    unsigned int n_tris, node_count;
    float4 * nodes, * tris, * shade, * tri_tan;
    RefitBox * boxes;                // scratch: every node's exact box, 24 B per node
    unsigned int * bounds;           // [0] max |coordinate| as float bits, [1] != 0: a coordinate the upload would refuse
};

__global__ __launch_bounds__(256) void k_refit_bounds(RefitArgs A) {
    float m = 0.0f;
    unsigned int bad = 0u;
    const unsigned int total = 3u * A.n_tris;                     // corners
    for (unsigned int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const unsigned int slot = i / 3u, c = i - 3u * slot;
        const float * p = A.positions + 3 * (size_t)A.table[(size_t)slot * REFIT_TABLE_WORDS + c];
        for (int k = 0; k < 3; ++k) {
            const float v = fabsf(p[k]);
            if (!(v < 1e18f)) bad = 1u;                           // NaN, infinity, 1e18 and beyond
            else m = fmaxf(m, v);
        }
    }
    wave_max_to_word(A.bounds, m);
    for (int off = 32; off > 0; off >>= 1) bad |= (unsigned int)__shfl_xor((int)bad, off);
    if ((threadIdx.x & 63u) == 0u && bad) atomicOr(A.bounds + 1, 1u);
}

__global__ __launch_bounds__(256) void k_refit_records(RefitArgs A) {
    const unsigned int slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= A.n_tris) return;
    const unsigned int * t = A.table + (size_t)slot * REFIT_TABLE_WORDS;
    const uint2 i01 = *reinterpret_cast<const uint2 *>(t), i2n0 = *reinterpret_cast<const uint2 *>(t + 2),
                n12 = *reinterpret_cast<const uint2 *>(t + 4);
    const float * pa = A.positions + 3 * (size_t)i01.x, * pb = A.positions + 3 * (size_t)i01.y, * pc = A.positions + 3 * (size_t)i2n0.x;
    const f3 a = mk3(pa[0], pa[1], pa[2]), b = mk3(pb[0], pb[1], pb[2]), c = mk3(pc[0], pc[1], pc[2]);
    const f3 n = tri_record(a, b, c, A.tris + 3 * (size_t)slot);
    float4 * sh = A.shade + 4 * (size_t)slot;
    // (sh[3] - the open-triangle flags of the uploaded geometry and the material index - stays as it is: an update makes the
    // flags stale and no render reads them until the next upload, prt_api.hip shadow_trees_fresh)
    if (A.normals) {
        const float * n0 = A.normals + 3 * (size_t)i2n0.y, * n1 = A.normals + 3 * (size_t)n12.x, * n2 = A.normals + 3 * (size_t)n12.y;
        sh[0] = make_float4(n0[0], n0[1], n0[2], n1[0]);
        sh[1] = make_float4(n1[1], n1[2], n2[0], n2[1]);
        sh[2] = make_float4(n2[2], n.x, n.y, n.z);
    } else {
        sh[2] = make_float4(sh[2].x, n.x, n.y, n.z);              // the third vertex normal's z stays
    }
    if (A.tangents && A.tri_tan) {                                // mesh->tangents[idx_normals[...]], raytracer.cpp:470-473
        const float * g0 = A.tangents + 3 * (size_t)i2n0.y, * g1 = A.tangents + 3 * (size_t)n12.x, * g2 = A.tangents + 3 * (size_t)n12.y;
        float4 * tt = A.tri_tan + 3 * (size_t)slot;
        tt[0] = make_float4(g0[0], g0[1], g0[2], g1[0]);
        tt[1] = make_float4(g1[1], g1[2], g2[0], g2[1]);
        tt[2] = make_float4(g2[2], 0.0f, 0.0f, 0.0f);
    }
}

// Nodes [first, first + count) are one tree level; the level below has been refitted by the previous launch.
template <int WIDTH>
__global__ __launch_bounds__(64) void k_refit_level(RefitArgs A, unsigned int first, unsigned int count) {
    const unsigned int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const unsigned int node = first + i;
    if (node >= A.node_count) return;
    enum { NV = WIDTH == 8 ? 5 : 4 };                             // 16-byte words per node
    uint4 * np = reinterpret_cast<uint4 *>(A.nodes) + (size_t)node * NV;
    unsigned int d[4 * NV];
    for (int k = 0; k < NV; ++k) {
        const uint4 v = np[k];
        d[4 * k] = v.x; d[4 * k + 1] = v.y; d[4 * k + 2] = v.z; d[4 * k + 3] = v.w;
    }
    refit_step<WIDTH>(d, node, A.node_count, A.n_tris, A.table, A.positions, A.boxes);
    unsigned int * nw = reinterpret_cast<unsigned int *>(np);
    if constexpr (WIDTH == 8) {
        np[0] = make_uint4(d[0], d[1], d[2], d[3]);
        *reinterpret_cast<uint2 *>(nw + 6) = make_uint2(d[6], d[7]);      // d4-5 (child_base, tri_base) stay
        np[2] = make_uint4(d[8], d[9], d[10], d[11]);
        np[3] = make_uint4(d[12], d[13], d[14], d[15]);
        np[4] = make_uint4(d[16], d[17], d[18], d[19]);
    } else {
        np[0] = make_uint4(d[0], d[1], d[2], d[3]);
        np[1] = make_uint4(d[4], d[5], d[6], d[7]);
        *reinterpret_cast<uint2 *>(nw + 8) = make_uint2(d[8], d[9]);      // d10-13 (the links) stay
        *reinterpret_cast<uint2 *>(nw + 14) = make_uint2(d[14], d[15]);
    }
}

}  // namespace prt
