// bvh_check.cpp - the host's reading of the two node layouts bvh_build.cpp writes, and the two checks built on it: the
// O(nodes) link validation that guards every upload, and the full geometric check of the test-suite.  Host only.
#include "bvh_build.h"
#include "dev_math.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace prt {
namespace {

// One child slot of a node as the traversal will read it.
struct Slot {
    enum Kind { NONE, NODE, LEAF } kind;      // the address it carries: none, internal child `node`, triangles [first, first + count)
    bool empty;                               // holds no child (an empty 4-wide slot still carries a link: the dummy leaf)
    uint32_t qlo[3], qhi[3];                  // quantised planes
    uint32_t node, first, count;
};
struct Node {
    float org[3], scale[3];
    uint32_t n_slots;
    Slot slot[8];
    uint32_t faults;                          // invariants of the layout that do not hold
    const char * unsafe;                      // one of them that makes the node's addresses meaningless, or NULL
};

inline bool power_of_two(uint32_t exponent_dword) { return (exponent_dword & 0x7F800000u) != 0u && !(exponent_dword & 0x80000000u); }

// 4-wide (dev_scene.h): dwords 0-2 origin, 3 / 14 / 15 the grid steps as floats, 4-6 lo planes and 7-9 hi planes (a byte
// per slot), 10-13 links: >= 0 a node, < 0 the complement of first << 2 | count - 1.  Children come first; an empty slot
// has inverted planes on every axis and is linked to the dummy record at n_tris.
void decode4(const uint32_t * d, uint32_t n_tris, Node * n) {
    const int scale_dword[3] = { 3, 14, 15 };
    n->faults = 0;
    n->unsafe = nullptr;
    n->n_slots = 4;
    for (int a = 0; a < 3; ++a) {
        memcpy(&n->org[a], &d[a], 4);
        const uint32_t step = d[scale_dword[a]] & 0xFF800000u;               // the mantissa may hold the node's normal cone (dev_scene.h)
        memcpy(&n->scale[a], &step, 4);
        if (!power_of_two(d[scale_dword[a]])) n->faults++;
    }
    uint32_t used = 0;
    while (used < 4 && !(((d[4] >> (8 * used)) & 0xFFu) == 255u && ((d[7] >> (8 * used)) & 0xFFu) == 0u)) ++used;
    if (used < 1) n->faults++;
    for (uint32_t k = 0; k < 4; ++k) {
        Slot & s = n->slot[k];
        for (int a = 0; a < 3; ++a) { s.qlo[a] = (d[4 + a] >> (8 * k)) & 0xFFu; s.qhi[a] = (d[7 + a] >> (8 * k)) & 0xFFu; }
        const int32_t link = (int32_t)d[10 + k];
        s.kind = link >= 0 ? Slot::NODE : Slot::LEAF;
        s.node = (uint32_t)link;
        s.first = (uint32_t)~link >> 2;
        s.count = ((uint32_t)~link & 3u) + 1u;
        s.empty = k >= used;
        if (s.empty) {
            if (s.kind != Slot::LEAF || s.first != n_tris) n->faults++;
            for (int a = 0; a < 3; ++a) if (s.qlo[a] != 255u || s.qhi[a] != 0u) n->faults++;
        }
    }
}

// 8-wide (bvh_build.h): masks disjoint, counts only on leaf slots, empty slots inverted on every axis; children and
// triangles are addressed implicitly, in slot order from child_base / tri_base.
void decode8(const uint32_t * d, uint32_t, Node * n) {
    const int scale_dword[3] = { 3, 6, 7 };
    n->faults = 0;
    n->n_slots = 8;
    for (int a = 0; a < 3; ++a) {
        const uint32_t sb = d[scale_dword[a]] & 0x7F800000u;
        memcpy(&n->org[a], &d[a], 4);
        memcpy(&n->scale[a], &sb, 4);
        if (!power_of_two(d[scale_dword[a]])) n->faults++;
    }
    const uint32_t imask = d[3] & 0xFFu, lmask = d[3] >> 8 & 0xFFu, c0 = d[6] & 0xFFu, c1 = d[6] >> 8 & 0xFFu;
    n->unsafe = imask & lmask ? "8-wide BVH: a slot is both an internal node and a leaf" : nullptr;
    if (imask & lmask) n->faults++;
    if ((c0 | c1) & ~lmask) n->faults++;
    if (!(imask | lmask)) n->faults++;
    uint32_t next_child = d[4], next_tri = d[5];
    for (uint32_t k = 0; k < 8; ++k) {
        Slot & s = n->slot[k];
        for (int a = 0; a < 3; ++a) {
            s.qlo[a] = d[8 + 2 * a + (k >> 2)] >> (8 * (k & 3u)) & 0xFFu;
            s.qhi[a] = d[14 + 2 * a + (k >> 2)] >> (8 * (k & 3u)) & 0xFFu;
        }
        s.kind = imask >> k & 1u ? Slot::NODE : lmask >> k & 1u ? Slot::LEAF : Slot::NONE;
        s.empty = s.kind == Slot::NONE;
        s.node = s.first = s.count = 0;
        if (s.kind == Slot::NODE) s.node = next_child++;
        if (s.kind == Slot::LEAF) { s.first = next_tri; s.count = 1u + (c0 >> k & 1u) + 2u * (c1 >> k & 1u); next_tri += s.count; }
        if (s.empty) for (int a = 0; a < 3; ++a) if (s.qlo[a] != 255u || s.qhi[a] != 0u) n->faults++;
    }
}

struct Layout {
    void (*decode)(const uint32_t * d, uint32_t n_tris, Node * n);
    bool dummy_in_every_tree;                 // slot n_tris, the uploader's all-zero record, is named by empty slots (4-wide); the
                                              // 8-wide tree names it only as the one leaf of an empty scene
    bool nodes_once;                          // implicit addressing: every node must be reached exactly once
    const char * bad_size, * bad_order, * bad_child, * bad_leaf;
};
const Layout LAYOUT4 = { decode4, true, false,
    "4-wide BVH: node array size does not match the node count", "4-wide BVH: triangle order does not cover the triangles",
    "4-wide BVH: child link out of range (children follow their parent in breadth-first order)", "4-wide BVH: leaf triangle range out of range" };
const Layout LAYOUT8 = { decode8, false, true,
    "8-wide BVH: node array size does not match the node count", "8-wide BVH: triangle order does not cover the triangles",
    "8-wide BVH: child range out of range", "8-wide BVH: leaf triangle range out of range" };

const Layout * layout_of(const BvhWide & bvh) {
    return bvh.node_dwords == BVH4_NODE_DWORDS ? &LAYOUT4 : bvh.node_dwords == BVH8_NODE_DWORDS ? &LAYOUT8 : nullptr;
}

}  // namespace

// A node link or a triangle range outside the arrays would be a wild read on the device - which the runtime reports by
// aborting the process (the round-3 abort) - and is an upload error instead.
const char * validate_bvh_links(const BvhWide & bvh, uint32_t n_tris) {
    const Layout * L = layout_of(bvh);
    if (!L) return "BVH: unknown node size";
    if (bvh.node_count == 0 || bvh.nodes.size() != (size_t)bvh.node_count * bvh.node_dwords) return L->bad_size;
    if (bvh.tri_order.size() != n_tris) return L->bad_order;
    const bool dummy_ok = L->dummy_in_every_tree || n_tris == 0;
    Node n;
    for (uint32_t ni = 0; ni < bvh.node_count; ++ni) {
        L->decode(&bvh.nodes[(size_t)ni * bvh.node_dwords], n_tris, &n);
        if (n.unsafe) return n.unsafe;
        for (uint32_t k = 0; k < n.n_slots; ++k) {
            const Slot & s = n.slot[k];
            if (s.kind == Slot::NODE && (s.node >= bvh.node_count || s.node <= ni)) return L->bad_child;
            if (s.kind == Slot::LEAF && (uint64_t)s.first + s.count > n_tris && !(dummy_ok && s.first == n_tris && s.count == 1)) return L->bad_leaf;
        }
    }
    return nullptr;
}

void check_bvh_wide(const float * verts, uint32_t n_tris, const BvhWide & bvh, uint64_t * out) {
    uint64_t violations = 0, leaves = 0, refs = 0;
    const Layout * L = layout_of(bvh);
    std::vector<uint8_t> seen(std::max(1u, n_tris), 0);
    std::vector<uint8_t> node_seen(std::max(1u, bvh.node_count), 0);
    struct Item { uint32_t node; float lo[3], hi[3]; };
    std::vector<Item> stack;
    Item root;
    root.node = 0;
    for (int a = 0; a < 3; ++a) { root.lo[a] = -3.0e38f; root.hi[a] = 3.0e38f; }
    if (L && bvh.nodes.size() == (size_t)bvh.node_count * bvh.node_dwords && bvh.tri_order.size() == n_tris) stack.push_back(root);
    else violations++;
    const bool dummy_ok = L && (L->dummy_in_every_tree || n_tris == 0);
    Node n;
    while (!stack.empty()) {
        const Item it = stack.back();
        stack.pop_back();
        if (it.node >= bvh.node_count) { violations++; continue; }
        if (node_seen[it.node]++ && L->nodes_once) { violations++; continue; }
        L->decode(&bvh.nodes[(size_t)it.node * bvh.node_dwords], n_tris, &n);
        violations += n.faults;
        for (uint32_t k = 0; k < n.n_slots; ++k) {
            const Slot & s = n.slot[k];
            if (s.empty) continue;
            Item ch;
            for (int a = 0; a < 3; ++a) {
                ch.lo[a] = std::max(it.lo[a], n.org[a] + (float)s.qlo[a] * n.scale[a]);
                ch.hi[a] = std::min(it.hi[a], n.org[a] + (float)s.qhi[a] * n.scale[a]);
            }
            if (s.kind == Slot::NODE) {
                ch.node = s.node;
                stack.push_back(ch);
                continue;
            }
            leaves++;
            for (uint32_t i = 0; i < s.count; ++i) {
                const uint32_t slot = s.first + i;
                if (slot == n_tris && dummy_ok) continue;           // the all-zero dummy triangle
                if (slot >= n_tris) { violations++; continue; }
                refs++;
                if (seen[slot]++) violations++;
                const uint32_t t = bvh.tri_order[slot];
                if (t >= n_tris) { violations++; continue; }
                for (int c = 0; c < 3; ++c)
                    for (int a = 0; a < 3; ++a) {
                        const float v = verts[(size_t)t * 9 + 3 * c + a];
                        // de-quantised planes may round by an ulp of the coordinate; the kernels widen every box
                        // by 2^-16 of the scene extent, far more than that
                        const float tol = 4.0f * 1.1920929e-7f * std::max(1.0f, fabsf(v));
                        if (v < ch.lo[a] - tol || v > ch.hi[a] + tol) violations++;
                    }
            }
        }
    }
    for (uint32_t t = 0; t < n_tris; ++t) if (!seen[t]) violations++;
    if (L && L->nodes_once) for (uint32_t i = 0; i < bvh.node_count; ++i) if (!node_seen[i]) violations++;
    out[0] = violations; out[1] = bvh.node_count; out[2] = bvh.max_depth; out[3] = bvh.stack_bound; out[4] = leaves; out[5] = refs;
}

// Normal cones (bvh_build.h): every (node with a cone, triangle below it) pair whose record normal - computed from the corners
// as the uploader computes it, tri_record - the stored bits do not cover.  A walk from the root with the list of coned
// ancestors: O(triangles x depth).  origin_max as attach_normal_cones got it.
uint64_t check_bvh_cones(const float * verts, uint32_t n_tris, const BvhWide & bvh, double origin_max, uint64_t * coned_nodes) {
    uint64_t violations = 0, coned = 0;
    if (coned_nodes) *coned_nodes = 0;
    if (bvh.node_dwords != BVH4_NODE_DWORDS || validate_bvh_links(bvh, n_tris)) return 0;
    struct Item { uint32_t node, depth; };
    std::vector<Item> stack(1, Item{ 0u, 0u });
    std::vector<uint32_t> above;                       // the coned nodes on the path to the node being visited
    std::vector<uint32_t> above_depth;
    while (!stack.empty()) {
        const Item it = stack.back();
        stack.pop_back();
        while (!above_depth.empty() && above_depth.back() >= it.depth) { above.pop_back(); above_depth.pop_back(); }
        const uint32_t * d = &bvh.nodes[(size_t)it.node * BVH4_NODE_DWORDS];
        if ((d[3] | d[14] | d[15]) & 0x007FFFFFu) { above.push_back(it.node); above_depth.push_back(it.depth); ++coned; }
        for (int k = 0; k < 4; ++k) {
            const int32_t link = (int32_t)d[10 + k];
            if (link >= 0) { stack.push_back(Item{ (uint32_t)link, it.depth + 1u }); continue; }
            const uint32_t first = (uint32_t)~link >> 2, count = ((uint32_t)~link & 3u) + 1u;
            for (uint32_t i = 0; i < count && first + i < n_tris; ++i) {
                const float * v = verts + 9 * (size_t)bvh.tri_order[first + i];
                float4 rec[3];
                tri_record(mk3(v[0], v[1], v[2]), mk3(v[3], v[4], v[5]), mk3(v[6], v[7], v[8]), rec);
                const float n[3] = { rec[2].y, rec[2].z, rec[2].w };
                for (uint32_t a : above) {
                    const uint32_t * c = &bvh.nodes[(size_t)a * BVH4_NODE_DWORDS];
                    if (!cone_covers_normal(c[3], c[14], c[15], n, origin_max)) ++violations;
                }
            }
        }
    }
    if (coned_nodes) *coned_nodes = coned;
    return violations;
}

}  // namespace prt
