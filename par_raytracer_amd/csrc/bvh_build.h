// bvh_build.h - host-side per-triangle BVH builder and checker for the HIP traversal kernels.
//
// The reference's acceleration structure is a sphere tree over whole OBJ groups with brute force inside
// each leaf (bsphere.cpp:379-444, raytracer.cpp:136-154).  Its RESULT is the exact closest front-facing
// hit over all triangles, so any conservative structure gives the same answer; the
// device uses a binned-SAH binary tree with <= 4 triangles per leaf, collapsed to 4 or 8 children per node
// with the child boxes quantised to 8 bits per plane.  The node layouts are written in bvh_build.cpp (finish_wide),
// decoded on the host in bvh_check.cpp (decode4 / decode8) and traversed in dev_trace4.h / dev_trace8.h.
#pragma once

#include <cstdint>
#include <vector>

namespace prt { struct BvhBuildOptions; }     // prt_options.h: bins, sweep, collapse rule, GPU-builder back end; NULL = defaults

namespace prt {

// A wide quantised BVH of either width.  Every child box is rounded OUTWARD onto its node's own 2^e grid, so the tree
// stays conservative.
struct BvhWide {
    std::vector<uint32_t> nodes;       // node_dwords per node
    std::vector<uint32_t> tri_order;   // tri_order[i] = input triangle stored at leaf-order slot i
    uint32_t node_dwords = 0;          // BVH4_NODE_DWORDS or BVH8_NODE_DWORDS: which layout `nodes` holds
    uint32_t node_count = 0;
    uint32_t max_depth = 0;            // in wide nodes
    uint32_t stack_bound = 0;          // entries a traversal can ever hold (4-wide: 3 per level + sentinel; 8-wide: one group per
                                       // level + the marker)
    float scene_lo[3] = { 0, 0, 0 }, scene_hi[3] = { 0, 0, 0 };
};
enum { BVH4_NODE_DWORDS = 16, BVH8_NODE_DWORDS = 20 };

// 4-wide: 64 B per node (layout in dev_scene.h), explicit links, tri_order in the binary tree's leaf order, an empty
// slot linked to the all-zero dummy record the uploader appends at slot n_tris.  Collapsed largest-area child first.
typedef BvhWide Bvh4Result;

// 8-wide compressed BVH: 80 B per node (5 x dwordx4), child boxes quantised to 8 bits per plane on the node's own
// power-of-two grid, children in slot order sorted along the node's ordering axis, so that a ray visits them front to back in
// ascending or descending slot order by its direction's sign on that axis (no per-step sort), children addressed implicitly
// (internal children consecutive from child_base, leaf triangles consecutive from tri_base, both in slot order).  Layout
// (dwords; dev_trace8.h reads it):
//    0-2   origin xyz (float: lo corner of the union of the children)
//    3     2^e_x as float bits (bits 23-30) | imask (bits 0-7: slot holds an internal node) | lmask << 8 (slot holds a leaf)
//    4     child_base: node index of the first internal child
//    5     tri_base: leaf-order index of the first triangle of the first leaf slot
//    6     2^e_y as float bits | c0 (bits 0-7) | c1 << 8: a leaf slot holds 1 + c0 + 2 c1 triangles (1..4)
//    7     2^e_z as float bits | the ordering axis (bits 0-1)
//    8-9   lo x of slots 0-3, 4-7 (one byte per slot)     10-11 lo y     12-13 lo z
//    14-15 hi x                                            16-17 hi y     18-19 hi z
// An empty slot has lo = 255 > hi = 0 on every axis and is in neither mask.
typedef BvhWide Bvh8Result;

// width: 4 or 8 children per node.  verts: 9 floats per triangle (a, b, c).  leaf_max <= 4 (2 bits in the leaf link).
void build_bvh_wide(int width, const float * verts, uint32_t n_tris, uint32_t leaf_max, uint32_t threads, BvhWide * out,
                    float trav_cost = 1.0f, const BvhBuildOptions * opt = nullptr);

// The same result from a binary radix tree built elsewhere (GPU LBVH, bvh_lbvh.h); see bvh_build.cpp.
void build_bvh_wide_from_radix_tree(int width, uint32_t n_tris, uint32_t leaf_max, const int32_t * left, const int32_t * right,
                                    const uint32_t * first, const uint32_t * last, const float * node_box, const float * leaf_box,
                                    const uint32_t * sorted_ids, BvhWide * out, const BvhBuildOptions * opt = nullptr);

// ---- shadow trees: per directional light, a second tree over the triangles that its shadow rays can hit at all.
//
// The triangle test is single-sided: it leaves at dd = Dot(qp, n) <= 0 with qp = o - (o + d) and n = Cross(ab, ac) as stored
// in the record (dev_trace_common.h tri_test).  All shadow rays of a directional light share d, so a triangle whose dd is
// <= 0 for EVERY origin a render can produce is never hit by them and need not be walked (DESIGN.md section 2 has the
// derivation of the bound below).
//
// shadow_tri_excluded: true when the triangle whose record holds the normal n - the three floats as the uploader STORED them,
// nothing is computed again here - may be left out of the tree of the light whose rays have direction d (the kernels'
// `facing * -1.0f`), for origins with |o_k| <= origin_max on every axis.  Conservative: false for anything it cannot prove -
// a normal that is not finite, is tiny or huge (the float products could under- or overflow), a direction outside
// [2^-20, 2^20], an origin_max that is not finite.
bool shadow_tri_excluded(const float n[3], const float d[3], double origin_max);
// The input triangles that stay: ids ascending.  normals: 3 floats per input triangle, the record normals.
void shadow_occluders(const float * normals, uint32_t n_tris, const float d[3], double origin_max, std::vector<uint32_t> * ids);
// A tree without triangles: one node whose slots are all empty (its 4-wide links name the dummy record at slot 0).
void make_empty_bvh(int width, BvhWide * out);
// Copies sub's nodes to dst (sub.nodes.size() dwords) with every node index moved by node_base and every triangle slot by
// tri_base: the tree as it reads when it lies behind another in the same arrays, rooted at node_base.
void rebase_bvh_nodes(const BvhWide & sub, uint32_t node_base, uint32_t tri_base, uint32_t * dst);

// One light's tree, whole: classify, decide by size, build with the ordinary back end (an empty set: make_empty_bvh) and
// append the nodes - rebased to (node_base, rec_base), the arrays' fill so far - to node_words.  `built` gets the tree as the
// back end made it, before the move: the caller puts it through validate_bvh_links (bvh_check.cpp), over
// r->triangle_count triangles, before anything is uploaded.  rec_tri gets
// the input triangle of every record the caller must append to the record array, in order; the last is 0xFFFFFFFF, the
// tree's own all-zero dummy record.  Not built (r->built = 0, nothing appended): more occluders than ratio_percent hundredths
// of the scene, or an array would pass 2^26 entries (the traversal's 32-bit byte offsets).  Returns NULL, or what is wrong
// with its arguments.
struct ShadowTreeBuild {
    int width = 4;
    uint32_t leaf_max = 4, threads = 1, ratio_percent = 75;
    float trav_cost = 1.0f;
    const BvhBuildOptions * opt = nullptr;
};
struct ShadowTreeResult { uint32_t built = 0, triangle_count = 0, node_count = 0, root = 0, stack_bound = 0; };
// verts: 9 floats per input triangle (the boxes); normals: 3 per input triangle, the stored record normals (the classification).
const char * append_shadow_tree(const ShadowTreeBuild & how, const float * verts, const float * normals, uint32_t n_tris, const float d[3], double origin_max,
                                std::vector<uint32_t> * node_words, uint32_t node_base, uint32_t rec_base,
                                std::vector<uint32_t> * rec_tri, ShadowTreeResult * r, BvhWide * built,
                                const std::vector<uint32_t> * occluders = nullptr);      // shadow_occluders' list, where the caller has it already

// ---- open triangles: per directional light, the triangles on which a shadow ray towards that light can start without any
// possible occluder ahead of it.  Such a ray is unoccluded whatever its exact origin, so a render counts it and adds its
// radiance at the hit instead of tracing it (kernels_wave.h shade_entry_on, include/prt.h "Open triangles").
//
// R is OPEN for direction d when no occluder O (shadow_occluders' list, R itself included when it is on it) has both
//   - its footprint along d within R's lateral margin of R's footprint, and
//   - its largest depth along d at least R's smallest depth minus R's depth margin.
// Footprints are boxes in the plane across d: of R's three corners, and of the eight corners of O's axis-parallel box (the box
// the traversal would have to pass before O is tested at all).  The occluders lie in a uniform grid over that plane, each cell
// holding the largest depth of the occluders that touch it: nothing here depends on a BVH, so both tree widths get the same flags.
//
// The margins (DESIGN.md section 2 has the derivation).  A render uses the flag of a hit only when the hit's distance is below
// `reach` and |Dot(ray direction, unit normal)| is at least 1/8 (ShadowOpenBounds::min_cos); for such a hit of a ray that starts
// within 4 coord_max of the origin on every axis, shadow_open_margins bounds how far from R the shadow ray can start: the
// rounding of the hit distance and of the hit point, the direction the triangle test really uses (o - (o + d), not d), the
// slack of the test at R's edges, the stored normal against the true plane, and the two pushes by ray_bias (|ray_bias| <=
// bias_max).  Everything it cannot bound - a corner that is not finite, a sliver, a scene so large that o + d rounds d away -
// comes back as "not open".
struct ShadowOpenBounds {
    double coord_max = 0.0;        // A: the scene's largest |coordinate|; ray origins (the camera) lie within 4 A on every axis
    double bias_max = 0.0;         // the largest |ray_bias| the flags hold for
    double reach = 0.0;            // the largest hit distance the flags hold for
    static constexpr double min_cos = 0.125;       // the kernels' PRT_SHADOW_OPEN_MIN_COS (dev_scene.h)
};
// The call-independent part of the bounds for a scene: bias_max = 2^-11 A (covers the reference's default ray_bias of 1e-3 from
// A = 2.05 up: every scene of BASELINE.md, the 12-triangle box with A = 4 included), reach = 2 A.  Priced on the 1 M triangle
// terrain (tools/bvh_price.cpp, profiles/shadow_open.txt): 85.1 % of the triangles that face the sun are open; with no bias at
// all it would be 85.8 %, with 2^-9 A 83.0 %, and the reach costs less than a point between A / 2 and 4 A.
ShadowOpenBounds shadow_open_bounds(double coord_max);
// R's two margins; false when R (tri9: its nine floats; n: the stored record normal) or the bounds are outside what the
// argument covers.
bool shadow_open_margins(const float * tri9, const float n[3], const float d[3], const ShadowOpenBounds & b, double * lateral, double * depth);
// open[t] = 1 for every open input triangle t, else 0; returns how many are.  An empty occluder list flags nothing (a ray over a
// scene without occluders is traced, in one node step: tests/test_gpu_shadow_trees.py's flat plane).  occluders: ascending ids.
uint32_t shadow_open_flags(const float * verts, const float * normals, uint32_t n_tris, const float d[3], const std::vector<uint32_t> & occluders,
                           const ShadowOpenBounds & b, uint32_t threads, std::vector<uint8_t> * open);

// ---- normal cones: per node of a 4-wide tree, a cone that bounds the record normals of every triangle below it, in the
// mantissas of the node's three grid steps (layout and predicate: dev_scene.h cone_faces_away).  A closest-hit ray whose
// direction the predicate accepts fails dd = Dot(qp, n) <= 0 on all of those triangles and does not descend.
//
// cone_covers_normal: what the stored bits (the node's dwords 3, 14, 15) promise about ONE triangle below the node, whose record
// holds the normal n - the three floats as stored.  True when every direction d, |d| <= 1 + 2^-20, that the predicate AS THE
// DEVICE EVALUATES IT accepts gives the device's own dd <= 0 for every origin with |o_k| <= origin_max (DESIGN.md section 2
// has the derivation; the dd part is shadow_tri_excluded's bound).  Also true for all-zero bits (no cone) and for a zero normal
// (dd is 0: the test rejects it whatever the ray); false for a normal that is not finite, tiny or huge under a node with bits.
bool cone_covers_normal(uint32_t d3, uint32_t d14, uint32_t d15, const float n[3], double origin_max);
// Writes the cones of a 4-wide tree (an 8-wide tree is left alone), each from the triangles of its node's own range:
// axis = the mean of the unit normals, A = axis / (sin(half angle) + margin) quantised, then shrunk until cone_covers_normal
// holds for every triangle of the range.  No cone (the mantissas stay zero) for a node whose half angle reaches 90 degrees,
// whose triangles are not one run of leaf-order slots, or with a normal that is not finite, tiny or huge below it.
// normals: 3 floats per INPUT triangle, the record normals.  The bits do not depend on `threads`.  Returns the nodes with a cone.
// Not part of build_bvh_wide: a refit reproduces that function's nodes bit for bit, and a refit clears the mantissas.
uint32_t attach_normal_cones(BvhWide & bvh, const float * normals, uint32_t n_tris, double origin_max, uint32_t threads);
// Nodes of a 4-wide node array whose mantissas hold a cone.
uint32_t count_normal_cones(const uint32_t * nodes, uint32_t node_count);

// bvh_check.cpp.  Every address the traversal kernels will form from the tree, checked on the host before the tree is
// uploaded: a message naming the first node link or triangle range outside the arrays, or NULL.  O(nodes), links only.
const char * validate_bvh_links(const BvhWide & bvh, uint32_t n_tris);

// bvh_check.cpp.  The full geometric check: every triangle lies inside the de-quantised box of every ancestor and is
// referenced by exactly one leaf, and the layout's own invariants hold.  out[0] = violations, out[1] = nodes,
// out[2] = depth, out[3] = stack bound, out[4] = leaves, out[5] = triangles referenced.
void check_bvh_wide(const float * verts, uint32_t n_tris, const BvhWide & bvh, uint64_t * out);
// bvh_check.cpp.  The normal cones of a 4-wide tree: the number of (coned node, triangle below it) pairs that
// cone_covers_normal refuses, with the record normal computed from the corners as the uploader does.  (Its own function and
// not a seventh word of check_bvh_wide's output: that function's callers hand it arrays of six.)  *coned_nodes: nodes with a cone.
uint64_t check_bvh_cones(const float * verts, uint32_t n_tris, const BvhWide & bvh, double origin_max, uint64_t * coned_nodes);

}  // namespace prt
