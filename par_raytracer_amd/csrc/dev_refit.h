// dev_refit.h - refit of the wide quantised BVH: the step that gives ONE node new boxes after the vertices moved, written once
// for both widths and for host and device (the kernels are in kernels_refit.h; tests/refit_host_harness.cpp runs the same step
// with g++).
//
// The tree's topology stays what the builder made it (bvh_build.cpp finish_wide): which children a node has, which triangles a
// leaf holds, the links, the masks, the 8-wide ordering axis.  Only the geometry follows the vertices: every node is given the
// exact float box of each child - a leaf's from the positions of its 1..4 triangles, an internal child's from the box that
// child stored when its own level was refitted -, unions them, takes the union's lo corner as its grid origin and per axis the
// smallest power-of-two step 2^e with 255 steps spanning the union (bvh_build.cpp Grid), and rounds every child box OUTWARD onto
// that grid (Grid::round_out).  On unmoved vertices the step gives back the builder's node bit for bit.
//
// Not re-sorted: the 8-wide slot order (children ascending along the node's ordering axis).  It only steers the order in which
// a ray visits the children it hits - never which it visits -, check_bvh_wide does not demand it, and every render and query
// result is independent of the visiting order (DESIGN.md sections 2-3).  Likewise the 4-wide largest-first order.
//
// Nodes are numbered breadth-first in both layouts, so a tree level is a contiguous range of nodes and every child lies on
// the level below its parent's: refit_level_table finds the ranges, and the levels are refitted deepest first.
#pragma once

#include "dev_math.h"

#include <vector>

namespace prt {

struct RefitBox { float lo[3], hi[3]; };      // 24 B: an exact float box (the element of the refit's scratch array)

// std::min / std::max as Box::grow of bvh_build.cpp calls them (the first argument unless the second is smaller / larger)
PRT_HD float refit_min(float a, float b) { return b < a ? b : a; }
PRT_HD float refit_max(float a, float b) { return a < b ? b : a; }
PRT_HD void refit_box_reset(RefitBox & b) {
    for (int a = 0; a < 3; ++a) { b.lo[a] = 3.402823466e+38f; b.hi[a] = -3.402823466e+38f; }
}
PRT_HD void refit_box_grow(RefitBox & b, const float * p) {
    for (int a = 0; a < 3; ++a) { b.lo[a] = refit_min(b.lo[a], p[a]); b.hi[a] = refit_max(b.hi[a], p[a]); }
}
PRT_HD void refit_box_grow(RefitBox & b, const RefitBox & c) {
    for (int a = 0; a < 3; ++a) { b.lo[a] = refit_min(b.lo[a], c.lo[a]); b.hi[a] = refit_max(b.hi[a], c.hi[a]); }
}

// One child slot of a node as the refit reads it (layouts: dev_scene.h, bvh_build.h).
enum { REFIT_EMPTY = 0, REFIT_NODE = 1, REFIT_LEAF = 2 };
struct RefitSlot {
    unsigned int kind;
    unsigned int first;       // REFIT_NODE: the child's node index; REFIT_LEAF: leaf-order index of its first triangle
    unsigned int count;       // REFIT_LEAF: triangles, 1..4
};

template <int WIDTH>
PRT_HD void refit_slots(const unsigned int * d, RefitSlot * s) {
    if constexpr (WIDTH == 8) {
        const unsigned int imask = d[3] & 0xFFu, lmask = d[3] >> 8 & 0xFFu, c0 = d[6] & 0xFFu, c1 = d[6] >> 8 & 0xFFu;
        unsigned int next_child = d[4], next_tri = d[5];
        for (unsigned int k = 0; k < 8u; ++k) {
            s[k].kind = imask >> k & 1u ? REFIT_NODE : lmask >> k & 1u ? REFIT_LEAF : REFIT_EMPTY;
            s[k].first = s[k].count = 0u;
            if (s[k].kind == REFIT_NODE) s[k].first = next_child++;
            if (s[k].kind == REFIT_LEAF) { s[k].first = next_tri; s[k].count = 1u + (c0 >> k & 1u) + 2u * (c1 >> k & 1u); next_tri += s[k].count; }
        }
    } else {
        // children fill the slots from 0; an empty slot has lo = 255 > hi = 0 (no box rounds to that) and stays as it is
        bool used = true;
        for (unsigned int k = 0; k < 4u; ++k) {
            used = used && !((d[4] >> (8u * k) & 0xFFu) == 255u && (d[7] >> (8u * k) & 0xFFu) == 0u);
            const int link = (int)d[10 + k];
            s[k].kind = !used ? REFIT_EMPTY : link >= 0 ? REFIT_NODE : REFIT_LEAF;
            s[k].first = link >= 0 ? (unsigned int)link : ~(unsigned int)link >> 2;
            s[k].count = link >= 0 ? 0u : (~(unsigned int)link & 3u) + 1u;
        }
    }
}

PRT_HD double refit_pow2(int e) {               // 2^e as a double, -1022 <= e <= 1023
    const unsigned long long u = (unsigned long long)(e + 1023) << 52;
    double r;
    __builtin_memcpy(&r, &u, 8);
    return r;
}

// Grid of bvh_build.cpp: the smallest e with 255 * 2^e >= extent, clamped to [-100, 100]; -100 for extent 0.
PRT_HD int refit_grid_exponent(double ext) {
    if (!(ext > 0.0)) return -100;
    unsigned long long u;
    __builtin_memcpy(&u, &ext, 8);
    const int k = (int)(u >> 52 & 0x7FFu) - 1023;         // 2^k <= ext < 2^(k+1): a difference of two floats is a normal double
    int e = k - 7;                                        // 255 * 2^(k-8) < 2^k <= ext, and 255 * 2^(k-6) > 2^(k+1) > ext
    if (255.0 * refit_pow2(e) < ext) ++e;
    return e < -100 ? -100 : e > 100 ? 100 : e;
}

// The node step.  d: the node's dwords (16 or 20); slot: refit_slots(d); child[k]: the exact box of used slot k.  Writes the
// node's own exact box to *own and the geometry dwords of d - 4-wide: d0-9 and d14-15 (the links d10-13 stay); 8-wide: d0-2, the
// exponent bytes of d3 / d6 / d7 (their mask / count / axis bits stay) and d8-19 (d4-5 stay).
template <int WIDTH>
PRT_HD void refit_node(unsigned int * d, const RefitSlot * slot, const RefitBox * child, RefitBox * own) {
    RefitBox u;
    refit_box_reset(u);
    for (int k = 0; k < WIDTH; ++k)
        if (slot[k].kind != REFIT_EMPTY) refit_box_grow(u, child[k]);
    *own = u;
    unsigned int ebyte[3];
    double org[3], inv_scale[3];
    for (int a = 0; a < 3; ++a) {
        const int e = refit_grid_exponent((double)u.hi[a] - (double)u.lo[a]);
        ebyte[a] = (unsigned int)(e + 127);
        org[a] = (double)u.lo[a];
        inv_scale[a] = refit_pow2(-e);                    // a division by 2^e is exact, and so is this product
        __builtin_memcpy(&d[a], &u.lo[a], 4);
    }
    if constexpr (WIDTH == 8) { for (int i = 8; i < 20; ++i) d[i] = 0u; }
    else { for (int i = 4; i < 10; ++i) d[i] = 0u; }
    for (int k = 0; k < WIDTH; ++k) {
        unsigned int qlo[3] = { 255u, 255u, 255u }, qhi[3] = { 0u, 0u, 0u };      // empty slot: inverted, can never be hit
        if (slot[k].kind != REFIT_EMPTY)
            for (int a = 0; a < 3; ++a) {
                double lo = floor(((double)child[k].lo[a] - org[a]) * inv_scale[a]);
                double hi = ceil(((double)child[k].hi[a] - org[a]) * inv_scale[a]);
                lo = lo < 0.0 ? 0.0 : lo > 255.0 ? 255.0 : lo;
                hi = hi < 0.0 ? 0.0 : hi > 255.0 ? 255.0 : hi;
                qlo[a] = (unsigned int)lo;
                qhi[a] = (unsigned int)hi;
            }
        for (int a = 0; a < 3; ++a) {
            if constexpr (WIDTH == 8) {
                d[8 + 2 * a + (k >> 2)] |= qlo[a] << (8 * (k & 3));
                d[14 + 2 * a + (k >> 2)] |= qhi[a] << (8 * (k & 3));
            } else {
                d[4 + a] |= qlo[a] << (8 * k);
                d[7 + a] |= qhi[a] << (8 * k);
            }
        }
    }
    if constexpr (WIDTH == 8) {
        d[3] = ebyte[0] << 23 | (d[3] & 0x007FFFFFu);
        d[6] = ebyte[1] << 23 | (d[6] & 0x007FFFFFu);
        d[7] = ebyte[2] << 23 | (d[7] & 0x007FFFFFu);
    } else {
        d[3] = ebyte[0] << 23;
        d[14] = ebyte[1] << 23;
        d[15] = ebyte[2] << 23;
    }
}

// Leaf slot -> vertex indices, 24 B per triangle: the three position indices, then the three normal indices.
enum { REFIT_TABLE_WORDS = 6 };

// One node of the level being refitted: gathers its children's exact boxes - a leaf's as min / max over the positions of its
// triangles, read through the table (never from a + ab, which does not give back b's bits); an internal child's from `boxes`,
// where the level below left it - and runs the node step.  Addresses outside the arrays (no validated tree has them) are
// skipped, not followed.
template <int WIDTH>
PRT_HD void refit_step(unsigned int * d, unsigned int node, unsigned int node_count, unsigned int n_tris,
                       const unsigned int * table, const float * positions, RefitBox * boxes) {
    RefitSlot slot[WIDTH];
    RefitBox child[WIDTH];
    refit_slots<WIDTH>(d, slot);
    for (int k = 0; k < WIDTH; ++k) {
        refit_box_reset(child[k]);
        if (slot[k].kind == REFIT_NODE) {
            if (slot[k].first > node && slot[k].first < node_count) child[k] = boxes[slot[k].first];
        } else if (slot[k].kind == REFIT_LEAF) {
            for (unsigned int i = 0; i < slot[k].count; ++i) {
                const unsigned int ls = slot[k].first + i;
                if (ls >= n_tris) continue;
                for (int c = 0; c < 3; ++c) refit_box_grow(child[k], positions + 3 * (size_t)table[(size_t)ls * REFIT_TABLE_WORDS + c]);
            }
        }
    }
    refit_node<WIDTH>(d, slot, child, &boxes[node]);
}

// Host only.  The first node of every tree level (+ node_count at the end): one O(nodes) walk over the breadth-first array.  False when
// the array is not level-ordered (a child not exactly one level below its parent, or not reached exactly once): such a tree
// cannot be refitted level by level.
template <int WIDTH>
inline bool refit_level_table(const unsigned int * nodes, unsigned int node_count, std::vector<unsigned int> * level_first) {
    const unsigned int nd = WIDTH == 8 ? 20u : 16u;
    level_first->clear();
    if (!node_count) return false;
    std::vector<unsigned int> depth(node_count, 0xFFFFFFFFu);
    depth[0] = 0;
    unsigned int reached = 1;
    for (unsigned int ni = 0; ni < node_count; ++ni) {
        if (depth[ni] == 0xFFFFFFFFu) return false;
        if (ni && depth[ni] < depth[ni - 1]) return false;
        if (!ni || depth[ni] != depth[ni - 1]) level_first->push_back(ni);
        RefitSlot slot[WIDTH];
        refit_slots<WIDTH>(nodes + (size_t)ni * nd, slot);
        for (int k = 0; k < WIDTH; ++k) {
            if (slot[k].kind != REFIT_NODE) continue;
            const unsigned int c = slot[k].first;
            if (c <= ni || c >= node_count || depth[c] != 0xFFFFFFFFu) return false;
            depth[c] = depth[ni] + 1;
            ++reached;
        }
    }
    level_first->push_back(node_count);
    return reached == node_count;
}

}  // namespace prt
