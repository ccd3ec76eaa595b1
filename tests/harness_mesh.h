// harness_mesh.h - what the host harnesses (tests/*_host_harness.cpp) do to a mesh before their own query starts: un-index it,
// build the wide tree, lay out the 48-byte triangle records with the product's own tri_record (csrc/dev_math.h) and the
// leaf -> (group, vertex0) table as prt_upload_scene and the queries lay them out, and set up one lane's traversal state.
// (harness_scene.h is something else: the procedural scene of trace_host_harness.cpp.)
#pragma once

#include <cstring>
#include <vector>

#include "dev_trace.h"
#include "bvh_build.h"
#include "prt_options.h"

namespace mesh {

// 9 floats per triangle, in input order.
static std::vector<float> unindexed(const std::vector<float> & pos, const std::vector<uint32_t> & idx) {
    std::vector<float> verts(3 * idx.size());
    for (size_t k = 0; k < idx.size(); ++k) memcpy(&verts[3 * k], &pos[3 * (size_t)idx[k]], 12);
    return verts;
}

// The tree of the width the harness is compiled for: 4-wide by default, -DPRT_BVH8: 8-wide.
static void build_tree(const std::vector<float> & verts, uint32_t n_tris, prt::BvhWide * bvh) {
#if !defined(PRT_BVH8)
    prt::build_bvh_wide(4, verts.data(), n_tris, 4, 2, bvh);
#else
    prt::BvhBuildOptions bopt;
    prt::build_bvh_wide(8, verts.data(), n_tris, 4, 2, bvh, 1.0f, &bopt);
#endif
}

// The n_tris + 1 records (the last one the all-zero dummy): slot i holds input triangle order[i], or i when order is null.
static std::vector<float4> records(const std::vector<float> & verts, uint32_t n_tris, const uint32_t * order) {
    std::vector<float4> rec((size_t)(n_tris + 1) * 3, make_float4(0, 0, 0, 0));
    for (uint32_t slot = 0; slot < n_tris; ++slot) {
        const float * v = &verts[(size_t)(order ? order[slot] : slot) * 9];
        prt::tri_record(prt::mk3(v[0], v[1], v[2]), prt::mk3(v[3], v[4], v[5]), prt::mk3(v[6], v[7], v[8]), &rec[(size_t)slot * 3]);
    }
    return rec;
}

// Slot -> (group, vertex0) from the groups' (first_index, index_count) runs, in the order of records(); the dummy slot and a
// triangle that no group holds map to (0xFFFFFFFF, 0xFFFFFFFF).
static std::vector<uint2> leaf_map(const std::vector<uint32_t> & runs, uint32_t n_groups, uint32_t n_tris, const uint32_t * order) {
    std::vector<uint2> of_input(n_tris, make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu)), map((size_t)n_tris + 1, make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu));
    for (uint32_t g = 0; g < n_groups; ++g)
        for (uint32_t k = 0; k < runs[2 * g + 1] / 3; ++k) of_input[runs[2 * g] / 3 + k] = make_uint2(g, 3u * k);
    for (uint32_t slot = 0; slot < n_tris; ++slot) map[slot] = of_input[order ? order[slot] : slot];
    return map;
}

// One lane's traversal state over a tree and its records: a DevScene that is zero but for nodes, tris and the two counts (the
// harness sets what else its query reads), a global stack of stack_bound + 2 entries attached for one lane, zeroed counters.
struct Walk {
    std::vector<int> stack_mem;
    prt::DevScene sc;
    prt::GlobalStack stk;
    prt::TraceStats st;
    Walk(const uint32_t * nodes, uint32_t node_count, const std::vector<float4> & tris, uint32_t n_tris, uint32_t stack_bound)
        : stack_mem((size_t)(stack_bound + 2) * prt::STACK_ENTRY_INTS, 0) {
        memset(&sc, 0, sizeof(sc));
        sc.nodes = reinterpret_cast<const float4 *>(nodes);
        sc.tris = tris.data();
        sc.tri_count = n_tris;
        sc.node_count = node_count;
        stk.attach(stack_mem.data(), 0, 1);
    }
    Walk(const prt::BvhWide & bvh, const std::vector<float4> & tris, uint32_t n_tris)
        : Walk(bvh.nodes.data(), bvh.node_count, tris, n_tris, bvh.stack_bound) {}
};

}  // namespace mesh
