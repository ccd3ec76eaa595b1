// bvh_build.cpp - host BVH builder: a binned surface-area-heuristic binary tree (multi-threaded over subtrees), or a radix
// tree built elsewhere, collapsed to 4 or 8 children per node and quantised (one back end, finish_wide).
#include "bvh_build.h"
#include "prt_options.h"
#include "dev_scene.h"

#include <algorithm>
#include <atomic>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <cstdio>
#include <stdexcept>
#include <thread>

namespace prt {
namespace {

struct Box {
    float lo[3], hi[3];
    void reset() { for (int a = 0; a < 3; ++a) { lo[a] = FLT_MAX; hi[a] = -FLT_MAX; } }
    void grow(const Box & b) { for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], b.lo[a]); hi[a] = std::max(hi[a], b.hi[a]); } }
    void grow(const float * p) { for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], p[a]); hi[a] = std::max(hi[a], p[a]); } }
    float half_area() const {
        float dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
        if (dx < 0.0f) return 0.0f;
        return dx * dy + dy * dz + dz * dx;
    }
};

struct Prim {
    Box box;
    float c[3];
    uint32_t id;
};

struct TmpNode {
    Box box;
    int32_t left, right;        // TmpNode indices, -1 for a leaf
    uint32_t first, count;      // primitive range (leaf)
    uint32_t depth;
};

enum { MAX_BINS = 64, MAX_FORCED_DEPTH = 56 };

struct Builder {
    std::vector<Prim> prims;
    std::vector<TmpNode> pool;
    std::atomic<uint32_t> next_node;
    std::atomic<uint32_t> max_depth;
    std::atomic<int> threads_free;
    uint32_t leaf_max;
    float trav_cost = 1.0f;     // SAH: cost of one traversal step relative to one triangle test
    int BINS = 16;              // SAH bins per axis (PRT_SAH_BINS, <= MAX_BINS)
    uint32_t sweep_max = 0;     // nodes of at most this many triangles try every split position of every axis (PRT_SAH_SWEEP)
    BvhBuildOptions opt;        // how the caller wants the tree built (prt_options.h); defaults when it said nothing
    void configure(const BvhBuildOptions * o) {
        if (o) opt = *o;
        if (opt.sah_bins >= 0) BINS = std::max(4, std::min((int)MAX_BINS, (int)opt.sah_bins));
        if (opt.sah_sweep >= 0) sweep_max = (uint32_t)opt.sah_sweep;
    }

    uint32_t alloc() { return next_node.fetch_add(1); }

    // Builds the subtree over prims[first, first+count) into node `me`.
    void build(uint32_t me, uint32_t first, uint32_t count, uint32_t depth) {
        TmpNode & n = pool[me];
        n.depth = depth;
        Box bounds, cbounds;
        bounds.reset();
        cbounds.reset();
        for (uint32_t i = first; i < first + count; ++i) {
            bounds.grow(prims[i].box);
            cbounds.grow(prims[i].c);
        }
        n.box = bounds;
        n.left = n.right = -1;
        n.first = first;
        n.count = count;

        auto make_leaf = [&]() {
            uint32_t d = max_depth.load();
            while (depth > d && !max_depth.compare_exchange_weak(d, depth)) {}
        };
        if (count == 1) { make_leaf(); return; }

        // --- binned SAH over the three axes
        int best_axis = -1, best_split = -1;
        float best_cost = FLT_MAX;
        float parent_area = bounds.half_area();
        if (depth < MAX_FORCED_DEPTH) {
            // one pass over the triangles fills the bins of all three axes (the array is 40 MB for a million triangles: the
            // passes, not the arithmetic, are what a level costs)
            Box bin_box[3][MAX_BINS];
            uint32_t bin_n[3][MAX_BINS];
            float cmin[3], scale[3];
            bool use[3];
            for (int axis = 0; axis < 3; ++axis) {
                cmin[axis] = cbounds.lo[axis];
                use[axis] = cbounds.hi[axis] > cmin[axis];
                scale[axis] = use[axis] ? (float)BINS / (cbounds.hi[axis] - cmin[axis]) : 0.0f;
                for (int k = 0; k < BINS; ++k) { bin_box[axis][k].reset(); bin_n[axis][k] = 0; }
            }
            for (uint32_t i = first; i < first + count; ++i) {
                const Prim & p = prims[i];
                for (int axis = 0; axis < 3; ++axis) {
                    if (!use[axis]) continue;
                    int k = (int)((p.c[axis] - cmin[axis]) * scale[axis]);
                    k = k < 0 ? 0 : (k >= BINS ? BINS - 1 : k);
                    bin_box[axis][k].grow(p.box);
                    bin_n[axis][k]++;
                }
            }
            for (int axis = 0; axis < 3; ++axis) {
                if (!use[axis]) continue;
                float right_area[MAX_BINS];
                uint32_t right_n[MAX_BINS];
                Box acc;
                acc.reset();
                uint32_t cnt = 0;
                for (int k = BINS - 1; k > 0; --k) {
                    acc.grow(bin_box[axis][k]);
                    cnt += bin_n[axis][k];
                    right_area[k] = acc.half_area();
                    right_n[k] = cnt;
                }
                acc.reset();
                cnt = 0;
                for (int k = 0; k < BINS - 1; ++k) {
                    acc.grow(bin_box[axis][k]);
                    cnt += bin_n[axis][k];
                    if (cnt == 0 || right_n[k + 1] == 0) continue;
                    float cost = acc.half_area() * (float)cnt + right_area[k + 1] * (float)right_n[k + 1];
                    if (cost < best_cost) { best_cost = cost; best_axis = axis; best_split = k; }
                }
            }
        }

        // --- small nodes: every split position of every axis (sorted sweep) instead of the bins
        int sweep_axis = -1;
        uint32_t sweep_left = 0;
        if (count <= sweep_max && depth < MAX_FORCED_DEPTH && count >= 2) {
            std::vector<float> right_area(count);
            for (int axis = 0; axis < 3; ++axis) {
                std::sort(prims.begin() + first, prims.begin() + first + count,
                          [axis](const Prim & a, const Prim & b) { return a.c[axis] < b.c[axis] || (a.c[axis] == b.c[axis] && a.id < b.id); });
                Box acc;
                acc.reset();
                for (uint32_t i = count - 1; i > 0; --i) { acc.grow(prims[first + i].box); right_area[i] = acc.half_area(); }
                acc.reset();
                for (uint32_t i = 0; i + 1 < count; ++i) {
                    acc.grow(prims[first + i].box);
                    float cost = acc.half_area() * (float)(i + 1) + right_area[i + 1] * (float)(count - i - 1);
                    if (cost < best_cost) { best_cost = cost; sweep_axis = axis; sweep_left = i + 1; best_axis = axis; }
                }
            }
            if (sweep_axis >= 0 && sweep_axis != 2)
                std::sort(prims.begin() + first, prims.begin() + first + count,
                          [sweep_axis](const Prim & a, const Prim & b) { return a.c[sweep_axis] < b.c[sweep_axis] || (a.c[sweep_axis] == b.c[sweep_axis] && a.id < b.id); });
        }

        // leaf if allowed and cheaper than splitting (traversal step cost 1, triangle test cost 1)
        if (count <= leaf_max) {
            float split_cost = (best_axis >= 0 && parent_area > 0.0f) ? trav_cost + best_cost / parent_area : FLT_MAX;
            if ((float)count <= split_cost) { make_leaf(); return; }
        }

        uint32_t mid;
        if (sweep_axis >= 0) {
            mid = first + sweep_left;                  // the range is sorted along the winning axis
        } else if (best_axis >= 0) {
            float cmin = cbounds.lo[best_axis];
            float scale = (float)BINS / (cbounds.hi[best_axis] - cmin);
            Prim * b = &prims[first];
            Prim * e = b + count;
            Prim * m = std::partition(b, e, [&](const Prim & p) {
                int bin = (int)((p.c[best_axis] - cmin) * scale);
                bin = bin < 0 ? 0 : (bin >= BINS ? BINS - 1 : bin);
                return bin <= best_split;
            });
            mid = first + (uint32_t)(m - b);
        } else {
            mid = first;
        }
        if (mid == first || mid == first + count) {
            // coincident centroids (or forced depth): median split along the widest centroid axis
            int axis = 0;
            float ext = -1.0f;
            for (int a = 0; a < 3; ++a) {
                float e = cbounds.hi[a] - cbounds.lo[a];
                if (e > ext) { ext = e; axis = a; }
            }
            mid = first + count / 2;
            std::nth_element(prims.begin() + first, prims.begin() + mid, prims.begin() + first + count,
                             [axis](const Prim & a, const Prim & b) { return a.c[axis] < b.c[axis]; });
        }

        uint32_t l = alloc(), r = alloc();
        pool[me].left = (int32_t)l;
        pool[me].right = (int32_t)r;
        uint32_t lcount = mid - first, rcount = count - lcount;
        bool spawn = lcount > 32768 && rcount > 32768 && threads_free.fetch_sub(1) > 0;
        if (spawn) {
            std::thread t([this, l, first, lcount, depth]() { build(l, first, lcount, depth + 1); });
            build(r, mid, rcount, depth + 1);
            t.join();
            threads_free.fetch_add(1);
        } else {
            if (lcount > 32768 && rcount > 32768) threads_free.fetch_add(1);   // undo the failed reservation
            build(l, first, lcount, depth + 1);
            build(r, mid, rcount, depth + 1);
        }
    }
};


// ---------------------------------------------------------------------------------------------------------
// Back end: binary tree (b.pool, root 0; leaves carry [first, first + count) of b.prims) -> wide quantised nodes
// ---------------------------------------------------------------------------------------------------------

inline uint32_t float_bits(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

// Collapse: each wide node adopts up to W binary-tree descendants.
// Every visit of a wide node costs the same (all W boxes are tested), and under the surface-area heuristic a node is
// visited in proportion to the area of its box, so the best collapse of a given binary tree is the one with the smallest
// total area of wide nodes (the leaves stay what they are).  That optimum is a small dynamic programme over the binary
// tree (Ylitie, Karras, Laine 2017, section 3.1, here with fixed leaves):
//   F(m, k) = least area needed below binary node m if it may occupy up to k child slots of its parent
//   F(m, 1) = area(m) + min over i of F(left, i) + F(right, W - i)          (m becomes a wide node; 0 for a leaf)
//   F(m, k) = min(F(m, k - 1), min over i of F(left, i) + F(right, k - i))  (m is dissolved into its parent)
// The other rule is greedy: open the child with the largest box until W are there.
// 4-wide, measured on MI355X: the programme gives 18-20 % fewer wide nodes, but only 1-2 % fewer node visits per frame
// and 2.5 % MORE triangle tests on C4 (the rays of a terrain seen from above are far from the uniform distribution the
// heuristic assumes): frame time unchanged within noise.  So the 4-wide default stays greedy.  8-wide: the greedy rule
// leaves the tree of the 1M-triangle terrain at 3.6 children per node; the programme fills it (tools/bvh_price.cpp) and
// is the default.  The option BVH_COLLAPSE = greedy / dp selects either for both.
struct Collapse {
    struct Dp { float f[7]; uint8_t root_split, split[6]; };   // f[k-1] = F(m, k); split[k-2]: i of the best distribution, 0 = "use k - 1"
    const std::vector<TmpNode> & pool;
    const int W;                                             // children per node, <= 8
    const bool greedy;
    std::vector<Dp> dp;

    bool is_leaf(uint32_t t) const { return pool[t].left < 0; }

    Collapse(const Builder & b, int W_, bool greedy_) : pool(b.pool), W(W_), greedy(greedy_) {
        if (greedy) return;
        const uint32_t n_tmp = b.next_node.load();
        dp.resize(n_tmp);                                    // all zero, which is what a leaf keeps: F = 0, nothing to decide
        for (uint32_t t = n_tmp; t-- > 0;) {                  // children are allocated after their parent: bottom-up
            if (is_leaf(t)) continue;
            Dp & d = dp[t];
            const Dp & l = dp[(uint32_t)pool[t].left], & r = dp[(uint32_t)pool[t].right];
            float best = FLT_MAX;
            d.root_split = 1;
            for (int i = 1; i <= W - 1; ++i) {
                const float c = l.f[i - 1] + r.f[W - 1 - i];
                if (c < best) { best = c; d.root_split = (uint8_t)i; }
            }
            d.f[0] = pool[t].box.half_area() + best;
            for (int k = 2; k <= W - 1; ++k) {
                float bk = d.f[k - 2];
                uint8_t sk = 0;
                for (int i = 1; i < k; ++i) {
                    const float c = l.f[i - 1] + r.f[k - i - 1];
                    if (c < bk) { bk = c; sk = (uint8_t)i; }
                }
                d.f[k - 1] = bk;
                d.split[k - 2] = sk;
            }
        }
    }

    // The binary-tree nodes the wide node rooted at `root` adopts, into kids[0 .. n); returns n.
    uint32_t adopt(uint32_t root, uint32_t * kids) const {
        uint32_t n = 0;
        if (is_leaf(root)) { kids[n++] = root; return n; }
        if (!greedy) {
            // unfold the stored decisions: (node, slots it may occupy)
            struct Todo { uint32_t t; int k; };
            Todo stack[16];
            int sp = 0;
            const int i0 = dp[root].root_split;
            stack[sp++] = Todo{ (uint32_t)pool[root].right, W - i0 };
            stack[sp++] = Todo{ (uint32_t)pool[root].left, i0 };
            while (sp > 0) {
                Todo cur = stack[--sp];
                while (cur.k > 1 && !is_leaf(cur.t) && dp[cur.t].split[cur.k - 2] == 0) cur.k--;      // "use k - 1 slots"
                if (cur.k == 1 || is_leaf(cur.t)) { kids[n++] = cur.t; continue; }
                const int i = dp[cur.t].split[cur.k - 2];
                stack[sp++] = Todo{ (uint32_t)pool[cur.t].right, cur.k - i };
                stack[sp++] = Todo{ (uint32_t)pool[cur.t].left, i };
            }
            return n;
        }
        kids[n++] = (uint32_t)pool[root].left;
        kids[n++] = (uint32_t)pool[root].right;
        while (n < (uint32_t)W) {
            int best = -1;
            float best_area = -1.0f;
            for (uint32_t k = 0; k < n; ++k) {
                if (is_leaf(kids[k])) continue;
                const float a = pool[kids[k]].box.half_area();
                if (a > best_area) { best_area = a; best = (int)k; }
            }
            if (best < 0) break;
            const uint32_t t = kids[best];
            kids[best] = (uint32_t)pool[t].left;
            kids[n++] = (uint32_t)pool[t].right;
        }
        return n;
    }
};

// 8-wide slot order: the children in ascending order of their centres along the node's ordering axis (by default the one
// on which the centres spread most); a ray takes the hit slots in ascending or descending order by the sign of its
// direction on that axis (dev_trace8.h).  (The slot-per-octant order of Ylitie et al. 2017, section 3.2, measured 1.7 %
// more node visits: profiles/r03_ab_bvh8.txt.)  Sorts kids[0 .. n) and returns the axis.
uint32_t sort_along_axis(const Builder & b, uint32_t * kids, uint32_t n) {
    float lo[3] = { FLT_MAX, FLT_MAX, FLT_MAX }, hi[3] = { -FLT_MAX, -FLT_MAX, -FLT_MAX };
    float c[8][3];
    for (uint32_t k = 0; k < n; ++k)
        for (int a = 0; a < 3; ++a) {
            c[k][a] = 0.5f * b.pool[kids[k]].box.lo[a] + 0.5f * b.pool[kids[k]].box.hi[a];
            lo[a] = std::min(lo[a], c[k][a]); hi[a] = std::max(hi[a], c[k][a]);
        }
    int axis = 0;
    for (int a = 1; a < 3; ++a) if (hi[a] - lo[a] > hi[axis] - lo[axis]) axis = a;
    if (b.opt.axis_rule == 1) {
        // experiment: the longest axis of the node's box
        Box u2; u2.reset();
        for (uint32_t k = 0; k < n; ++k) u2.grow(b.pool[kids[k]].box);
        axis = 0;
        for (int a = 1; a < 3; ++a) if (u2.hi[a] - u2.lo[a] > u2.hi[axis] - u2.lo[axis]) axis = a;
    } else if (b.opt.axis_rule == 2) {
        // experiment: the axis along which the children's boxes, sorted by centre, overlap least (sum over all pairs of
        // the overlap of their intervals, relative to the node's extent on that axis)
        float best = FLT_MAX;
        for (int a = 0; a < 3; ++a) {
            float ext = 0.0f, lo_a = FLT_MAX, hi_a = -FLT_MAX;
            for (uint32_t k = 0; k < n; ++k) { lo_a = std::min(lo_a, b.pool[kids[k]].box.lo[a]); hi_a = std::max(hi_a, b.pool[kids[k]].box.hi[a]); }
            ext = hi_a - lo_a;
            if (!(ext > 0.0f)) continue;
            float ov = 0.0f;
            for (uint32_t i = 0; i < n; ++i)
                for (uint32_t j = i + 1; j < n; ++j) {
                    const Box & bi = b.pool[kids[i]].box, & bj = b.pool[kids[j]].box;
                    const float o = std::min(bi.hi[a], bj.hi[a]) - std::max(bi.lo[a], bj.lo[a]);
                    if (o > 0.0f) ov += o / ext;
                }
            if (ov < best) { best = ov; axis = a; }
        }
    }
    uint32_t order[8], sorted[8];
    for (uint32_t k = 0; k < n; ++k) order[k] = k;
    std::sort(order, order + n, [&](uint32_t x, uint32_t y) { return c[x][axis] < c[y][axis]; });
    for (uint32_t k = 0; k < n; ++k) sorted[k] = kids[order[k]];
    for (uint32_t k = 0; k < n; ++k) kids[k] = sorted[k];
    return (uint32_t)axis;
}

// A node's power-of-two grid: origin at the lo corner of the union box `u` of its children, step 2^e per axis with e the
// smallest exponent for which 255 steps span the box.
struct Grid {
    float org[3];
    uint32_t ebyte[3];        // e + 127: the exponent byte of the float 2^e (the traversal multiplies, it does not decode)
    double scale[3];          // 2^e
    explicit Grid(const Box & u) {
        for (int a = 0; a < 3; ++a) {
            const double ext = (double)u.hi[a] - (double)u.lo[a];
            int e = -100;
            if (ext > 0.0) {
                e = (int)std::ceil(std::log2(ext / 255.0));
                while (std::ldexp(255.0, e) < ext) ++e;
                if (e < -100) e = -100;
            }
            if (e > 100) e = 100;
            org[a] = u.lo[a];
            ebyte[a] = (uint32_t)(e + 127);
            scale[a] = std::ldexp(1.0, e);
        }
    }
    // A child's box rounded OUTWARD onto the grid.
    void round_out(const Box & cb, uint32_t * qlo, uint32_t * qhi) const {
        for (int a = 0; a < 3; ++a) {
            double lo = std::floor(((double)cb.lo[a] - (double)org[a]) / scale[a]);
            double hi = std::ceil(((double)cb.hi[a] - (double)org[a]) / scale[a]);
            if (lo < 0.0) lo = 0.0;
            if (lo > 255.0) lo = 255.0;
            if (hi < 0.0) hi = 0.0;
            if (hi > 255.0) hi = 255.0;
            qlo[a] = (uint32_t)lo;
            qhi[a] = (uint32_t)hi;
        }
    }
};

// What differs between the widths is stated here, once each: the default collapse rule, the order of a node's children,
// the order of the triangles, how a node names its children and how its bytes are packed, and the stack bound.
void finish_wide(Builder & b, uint32_t n_tris, int width, BvhWide * out) {
    if (width != 4 && width != 8) throw std::invalid_argument("build_bvh_wide: width must be 4 or 8");
    const auto t0 = std::chrono::steady_clock::now();
    const bool eight = width == 8;
    const bool greedy = eight ? b.opt.collapse == 0 : b.opt.collapse != 1;
    const int W = eight && b.opt.width >= 2 && b.opt.width <= 8 ? (int)b.opt.width : width;   // children per node (experiments: 6 of 8)
    const Collapse collapse(b, W, greedy);
    auto is_leaf = [&](uint32_t t) { return b.pool[t].left < 0; };

    // ---- number the nodes breadth-first: the top of the tree is contiguous (cache / LDS friendly) and the internal
    // children of a node get consecutive indices in slot order.  4-wide: the triangles stay in the binary tree's leaf
    // order and every slot carries a link.  8-wide: the triangles are laid out so that the leaves of a node are
    // consecutive in slot order too; a child is then addressed by the node's base index plus the number of like children
    // in lower slots, and the node needs no links.
    struct WideNode { uint32_t kid[8], n, axis, child_base, tri_base; };   // kid: TmpNode indices, slots n.. are empty
    struct Item { uint32_t tmp, depth; };
    std::vector<WideNode> wide;
    std::vector<Item> work;
    out->tri_order.clear();
    out->tri_order.reserve(n_tris);
    if (!eight) for (uint32_t i = 0; i < n_tris; ++i) out->tri_order.push_back(b.prims[i].id);
    work.push_back(Item{ 0u, 1u });
    uint32_t max_depth = 1;
    for (size_t head = 0; head < work.size(); ++head) {
        const Item it = work[head];
        WideNode w;
        w.n = collapse.adopt(it.tmp, w.kid);
        w.axis = 0;
        if (eight) {
            w.axis = sort_along_axis(b, w.kid, w.n);
        } else if (!greedy) {
            // largest box first: the slot order is the visiting order of equal keys
            for (uint32_t i = 1; i < w.n; ++i)
                for (uint32_t j = i; j > 0 && b.pool[w.kid[j]].box.half_area() > b.pool[w.kid[j - 1]].box.half_area(); --j)
                    std::swap(w.kid[j], w.kid[j - 1]);
        }
        w.child_base = (uint32_t)work.size();
        w.tri_base = (uint32_t)out->tri_order.size();
        for (uint32_t s = 0; s < w.n; ++s) {
            const uint32_t t = w.kid[s];
            if (!is_leaf(t)) {
                work.push_back(Item{ t, it.depth + 1 });
                if (it.depth + 1 > max_depth) max_depth = it.depth + 1;
            } else if (eight) {
                // (an empty scene's root leaf names the all-zero dummy record the uploader appends at slot n_tris = 0)
                for (uint32_t i = 0; i < b.pool[t].count && b.pool[t].first + i < n_tris; ++i)
                    out->tri_order.push_back(b.prims[b.pool[t].first + i].id);
            }
        }
        wide.push_back(w);
    }

    // ---- quantise and pack
    const uint32_t n_nodes = (uint32_t)wide.size();
    out->node_dwords = eight ? BVH8_NODE_DWORDS : BVH4_NODE_DWORDS;
    out->nodes.assign((size_t)n_nodes * out->node_dwords, 0u);
    for (uint32_t ni = 0; ni < n_nodes; ++ni) {
        const WideNode & w = wide[ni];
        Box u;
        u.reset();
        for (uint32_t s = 0; s < w.n; ++s) u.grow(b.pool[w.kid[s]].box);
        const Grid g(u);
        uint32_t * d = &out->nodes[(size_t)ni * out->node_dwords];
        for (int a = 0; a < 3; ++a) d[a] = float_bits(g.org[a]);
        uint32_t imask = 0, lmask = 0, c0 = 0, c1 = 0, next_child = w.child_base;
        for (uint32_t s = 0; s < (uint32_t)width; ++s) {
            uint32_t qlo[3] = { 255, 255, 255 }, qhi[3] = { 0, 0, 0 };      // empty slot: inverted, can never be hit
            const bool used = s < w.n, leaf = used && is_leaf(w.kid[s]);
            if (used) g.round_out(b.pool[w.kid[s]].box, qlo, qhi);
            if (eight) {
                if (leaf) {
                    const uint32_t extra = b.pool[w.kid[s]].count - 1u;          // 0..3
                    lmask |= 1u << s;
                    c0 |= (extra & 1u) << s;
                    c1 |= (extra >> 1) << s;
                } else if (used) {
                    imask |= 1u << s;
                }
                for (int a = 0; a < 3; ++a) {
                    d[8 + 2 * a + (s >> 2)] |= qlo[a] << (8 * (s & 3u));
                    d[14 + 2 * a + (s >> 2)] |= qhi[a] << (8 * (s & 3u));
                }
            } else {
                for (int a = 0; a < 3; ++a) {
                    d[4 + a] |= qlo[a] << (8 * s);
                    d[7 + a] |= qhi[a] << (8 * s);
                }
                // an empty slot is also masked by its link: a 1-triangle leaf naming the all-zero dummy record the uploader
                // appends at slot n_tris (always rejected: d = 0)
                if (!used) d[10 + s] = (uint32_t)~(int32_t)(n_tris << 2);
                else if (leaf) d[10 + s] = (uint32_t)~(int32_t)((b.pool[w.kid[s]].first << 2) | (b.pool[w.kid[s]].count - 1));
                else d[10 + s] = next_child++;
            }
        }
        // the grid steps 2^e as ready-made floats (the exponent byte in place)
        if (eight) {
            d[3] = g.ebyte[0] << 23 | imask | lmask << 8;
            d[4] = w.child_base;
            d[5] = w.tri_base;
            d[6] = g.ebyte[1] << 23 | c0 | c1 << 8;
            d[7] = g.ebyte[2] << 23 | w.axis;
        } else {
            d[3] = g.ebyte[0] << 23;
            d[14] = g.ebyte[1] << 23;
            d[15] = g.ebyte[2] << 23;
        }
    }
    out->node_count = n_nodes;
    out->max_depth = max_depth;
    // 4-wide: 3 unvisited siblings per level + the sentinel; 8-wide: one group of unvisited siblings per level, the bottom
    // marker, one to spare
    out->stack_bound = eight ? max_depth + 2 : 3 * max_depth + 2;
    if (b.opt.debug) fprintf(stderr, "[prt] BVH back end (collapse to %d-wide, quantise, reorder): %.1f ms\n", width, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
}

// Front end shared by the 4- and 8-wide builds: binned-SAH binary tree over the triangles into b.pool (root 0).
void build_sah_binary(Builder & b, const float * verts, uint32_t n_tris, uint32_t leaf_max, uint32_t threads, float trav_cost,
                      float * scene_lo, float * scene_hi) {
    if (leaf_max < 1) leaf_max = 1;
    if (leaf_max > 4) leaf_max = 4;
    b.leaf_max = leaf_max;
    b.trav_cost = trav_cost;
    b.prims.resize(n_tris);
    Box scene;
    scene.reset();
    for (uint32_t i = 0; i < n_tris; ++i) {
        Prim & p = b.prims[i];
        p.box.reset();
        p.box.grow(verts + 9 * (size_t)i);
        p.box.grow(verts + 9 * (size_t)i + 3);
        p.box.grow(verts + 9 * (size_t)i + 6);
        for (int a = 0; a < 3; ++a) p.c[a] = 0.5f * p.box.lo[a] + 0.5f * p.box.hi[a];
        p.id = i;
        scene.grow(p.box);
    }
    for (int a = 0; a < 3; ++a) { scene_lo[a] = n_tris ? scene.lo[a] : 0.0f; scene_hi[a] = n_tris ? scene.hi[a] : 0.0f; }
    b.pool.resize(n_tris ? 2 * (size_t)n_tris : 1);
    b.next_node = 1;
    b.max_depth = 0;
    b.threads_free = (int)(threads > 1 ? threads - 1 : 0);
    const auto t_build = std::chrono::steady_clock::now();
    if (n_tris) {
        b.build(0, 0, n_tris, 0);
    } else {
        TmpNode & n = b.pool[0];
        n.box.reset();
        for (int a = 0; a < 3; ++a) n.box.lo[a] = n.box.hi[a] = 0.0f;
        n.left = n.right = -1;
        n.first = 0;
        n.count = 1;          // the all-zero dummy triangle the uploader always allocates
        n.depth = 0;
    }
    if (b.opt.debug) fprintf(stderr, "[prt] binned-SAH binary build, %u triangles, %u threads: %.1f ms\n", n_tris, threads, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_build).count());
}

}  // namespace

void build_bvh_wide(int width, const float * verts, uint32_t n_tris, uint32_t leaf_max, uint32_t threads, BvhWide * out, float trav_cost,
                    const BvhBuildOptions * opt) {
    *out = BvhWide();
    Builder b;
    b.configure(opt);
    build_sah_binary(b, verts, n_tris, leaf_max, threads, trav_cost, out->scene_lo, out->scene_hi);
    finish_wide(b, n_tris, width, out);
}

// ---- shadow trees (bvh_build.h).  The bound, with u = 2^-24, D = max |d_k|, M = origin_max, N1 = |n_x| + |n_y| + |n_z|:
//   the device forms qp_k = fl(o_k - fl(o_k + d_k)) = -d_k + e_k with |e_k| <= u (M + 2 D) (1 + u) =: E, and
//   dd = fl(Dot(qp, n)) <= Sum qp_k n_k + g3 Sum |qp_k n_k| <= -d.n + N1 (E + g3 (D + E)), g3 = 3 u / (1 - 3 u) < 4 u,
// so dd <= 0 is certain where d.n >= N1 (E + 4 u (D + E)).  d.n is taken in double (the products are exact, the two sums
// cost 2^-52 D N1) and the margin is raised by 2^-20 of itself for its own rounding.  N1 and D are kept inside ranges where
// no product of the float expression can overflow, and where an underflow (or a flushed subnormal, 2^-126 a term) is far
// below the margin: N1 in [2^-60, 2^60], D in [2^-20, 2^20], M <= 2^60.
// The part of that margin that does not depend on the normal, for directions with max |d_k| = D and origins within M:
// E + 4 u (D + E) + 2^-52 D x 4; *E_out gets E.  shadow_tri_excluded and the normal cones (below) both multiply it by N1.
static double dd_margin(double D, double origin_max, double * E_out = nullptr) {
    const double u = 5.9604644775390625e-8;
    const double E = u * (origin_max + 2.0 * D) * (1.0 + u);
    if (E_out) *E_out = E;
    return E + 4.0 * u * (D + E) + D * 8.881784197001252e-16;
}

bool shadow_tri_excluded(const float n[3], const float d[3], double origin_max) {
    const double lo60 = 8.673617379884035e-19, hi60 = 1152921504606846976.0;
    const double D = std::max(std::max(fabs((double)d[0]), fabs((double)d[1])), fabs((double)d[2]));
    const double N1 = fabs((double)n[0]) + fabs((double)n[1]) + fabs((double)n[2]);
    if (!(N1 >= lo60 && N1 <= hi60)) return false;                         // zero area, tiny, huge or not finite: kept
    if (!(D >= 9.5367431640625e-7 && D <= 1048576.0)) return false;
    if (!(origin_max >= 0.0 && origin_max <= hi60)) return false;
    const double margin = N1 * dd_margin(D, origin_max) * (1.0 + 9.5367431640625e-7);
    const double dn = (double)d[0] * (double)n[0] + (double)d[1] * (double)n[1] + (double)d[2] * (double)n[2];
    return dn >= margin;
}

void shadow_occluders(const float * normals, uint32_t n_tris, const float d[3], double origin_max, std::vector<uint32_t> * ids) {
    ids->clear();
    for (uint32_t t = 0; t < n_tris; ++t)
        if (!shadow_tri_excluded(normals + 3 * (size_t)t, d, origin_max)) ids->push_back(t);
}

// ---- normal cones (bvh_build.h).  The stored integers q = (q_x, q_y, q_z), alpha = |q|, a = q / alpha,
// ONE = CONE_ONE, L = 1 + 2^-20 (the longest direction the library normalises), u = 2^-24.
//   the predicate   fl(q.d) = fma(q_z, d_z, fma(q_y, d_y, fl(q_x d_x))) >= ONE.  The converts are exact (|q_k| < 2^22); the three
//       roundings cost at most 4 u alpha |d| together (Cauchy-Schwarz on Sum |q_k d_k|), an underflow 2^-149 a term.  So an
//       accepted d has q.d >= c := ONE - 4 u alpha L - 1e-30 exactly, i.e. a.d >= c / alpha, and |d| >= c / alpha > 2^-11.
//   the region      {d : a.d >= c / alpha, |d| <= L} is convex; d.n is linear and takes its minimum at an extreme point: on the
//       sphere |d| = L, at polar angle 90 deg - beta' from a with sin beta' >= s := c / (alpha L).  For a normal at angle phi from a
//       the smallest d.n / |n| there is L sin(beta' - phi), increasing in beta' up to 90 deg: the minimum is on the rim,
//           min d.n = |n| L (s cos phi - sqrt(1 - s^2) sin phi).
//   the test        dd <= 0 is certain where d.n >= N1 C, C = (E + 4 u (D + E) + 2^-50 D)(1 + 2^-20) with D = L and
//       E = u (M + 2 L)(1 + u): shadow_tri_excluded's margin for the longest direction (its D >= 2^-20 holds: |d| > 2^-11).
// A normal is covered when the minimum is at least that, with 1e-9 of it and 1e-13 to spare for the doubles here.
bool cone_covers_normal(uint32_t d3, uint32_t d14, uint32_t d15, const float n[3], double origin_max) {
    const double q[3] = { (double)cone_component(d3), (double)cone_component(d14), (double)cone_component(d15) };
    if (q[0] == 0.0 && q[1] == 0.0 && q[2] == 0.0) return true;
    const double u = 5.9604644775390625e-8, lo60 = 8.673617379884035e-19, hi60 = 1152921504606846976.0;
    const double m[3] = { (double)n[0], (double)n[1], (double)n[2] };
    const double N1 = fabs(m[0]) + fabs(m[1]) + fabs(m[2]);
    if (N1 == 0.0) return true;                                            // dd = 0: rejected whatever the ray
    if (!(N1 >= lo60 && N1 <= hi60)) return false;
    if (!(origin_max >= 0.0 && origin_max <= hi60)) return false;
    const double L = 1.0 + 9.5367431640625e-7;
    const double C = dd_margin(L, origin_max) * (1.0 + 9.5367431640625e-7);
    const double alpha = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]);
    const double c = (double)CONE_ONE - (4.0 * u * alpha * L + 1e-30);
    if (!(c > 0.0)) return false;
    const double s = c / (alpha * L);
    if (s >= 1.0) return true;                                             // no direction is accepted
    const double nl = sqrt(m[0] * m[0] + m[1] * m[1] + m[2] * m[2]);
    const double x[3] = { q[1] * m[2] - q[2] * m[1], q[2] * m[0] - q[0] * m[2], q[0] * m[1] - q[1] * m[0] };
    const double cos_phi = (q[0] * m[0] + q[1] * m[1] + q[2] * m[2]) / (alpha * nl);
    const double sin_phi = sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]) / (alpha * nl);
    const double least = L * (s * cos_phi - sqrt(1.0 - s * s) * sin_phi);
    return least >= (N1 / nl) * C * (1.0 + 1e-9) + 1e-13;
}

uint32_t count_normal_cones(const uint32_t * nodes, uint32_t node_count) {
    uint32_t n = 0;
    for (uint32_t i = 0; i < node_count; ++i) {
        const uint32_t * d = nodes + (size_t)i * BVH4_NODE_DWORDS;
        if ((d[3] | d[14] | d[15]) & 0x007FFFFFu) ++n;
    }
    return n;
}

uint32_t attach_normal_cones(BvhWide & bvh, const float * normals, uint32_t n_tris, double origin_max, uint32_t threads) {
    const uint32_t nc = bvh.node_count;
    if (bvh.node_dwords != BVH4_NODE_DWORDS || nc == 0 || bvh.nodes.size() != (size_t)nc * BVH4_NODE_DWORDS || bvh.tri_order.size() != n_tris || n_tris == 0) return 0;
    // unit normals in leaf order.  state 0: a zero normal (ignored), 1: usable, 2: not finite, tiny or huge (no cone above it)
    struct Unit { double v[3]; uint32_t state; };
    std::vector<Unit> unit(n_tris);
    for (uint32_t slot = 0; slot < n_tris; ++slot) {
        Unit & un = unit[slot];
        un.v[0] = un.v[1] = un.v[2] = 0.0;
        un.state = 2;
        const uint32_t t = bvh.tri_order[slot];
        if (t >= n_tris) continue;
        const float * n = normals + 3 * (size_t)t;
        const double N1 = fabs((double)n[0]) + fabs((double)n[1]) + fabs((double)n[2]);
        if (N1 == 0.0) { un.state = 0; continue; }
        if (!(N1 >= 8.673617379884035e-19 && N1 <= 1152921504606846976.0)) continue;
        const double l = sqrt((double)n[0] * n[0] + (double)n[1] * n[1] + (double)n[2] * n[2]);
        for (int a = 0; a < 3; ++a) un.v[a] = (double)n[a] / l;
        un.state = 1;
    }
    // every node's triangles, bottom up (children follow their parent in breadth-first order): a run of slots, or no cone
    std::vector<uint32_t> lo(nc, 0xFFFFFFFFu), hi(nc, 0u), cnt(nc, 0u);
    std::vector<uint8_t> bad(nc, 0);
    for (uint32_t ni = nc; ni-- > 0;) {
        const uint32_t * d = &bvh.nodes[(size_t)ni * BVH4_NODE_DWORDS];
        for (int k = 0; k < 4; ++k) {
            const int32_t link = (int32_t)d[10 + k];
            uint32_t f, e, c;
            if (link >= 0) {
                const uint32_t ch = (uint32_t)link;
                if (ch <= ni || ch >= nc || bad[ch]) { bad[ni] = 1; continue; }
                if (!cnt[ch]) continue;
                f = lo[ch]; e = hi[ch]; c = cnt[ch];
            } else {
                f = (uint32_t)~link >> 2;
                c = ((uint32_t)~link & 3u) + 1u;
                if (f >= n_tris) continue;                                  // the dummy record of an empty slot
                if ((uint64_t)f + c > n_tris) { bad[ni] = 1; continue; }
                e = f + c;
            }
            lo[ni] = std::min(lo[ni], f); hi[ni] = std::max(hi[ni], e); cnt[ni] += c;
        }
    }
    const double first_margin = 1.8 * dd_margin(1.0 + 9.5367431640625e-7, origin_max) + 3.0e-4;     // sqrt(3) C, and the axis' own quantisation (0.87 / alpha rad)
    std::vector<uint32_t> words((size_t)nc * 3, 0u);
    auto cone_of = [&](uint32_t ni) -> bool {
        if (bad[ni] || !cnt[ni] || hi[ni] - lo[ni] != cnt[ni]) return false;
        double sum[3] = { 0.0, 0.0, 0.0 };
        uint32_t usable = 0;
        for (uint32_t s = lo[ni]; s < hi[ni]; ++s) {
            if (unit[s].state == 2) return false;
            if (unit[s].state == 1) { for (int a = 0; a < 3; ++a) sum[a] += unit[s].v[a]; ++usable; }
        }
        if (!usable) return false;
        const double len = sqrt(sum[0] * sum[0] + sum[1] * sum[1] + sum[2] * sum[2]);
        if (!(len > 1e-9 * (double)usable)) return false;
        const double axis[3] = { sum[0] / len, sum[1] / len, sum[2] / len };
        double min_cos = 1.0;
        for (uint32_t s = lo[ni]; s < hi[ni]; ++s) {
            if (unit[s].state != 1) continue;
            min_cos = std::min(min_cos, axis[0] * unit[s].v[0] + axis[1] * unit[s].v[1] + axis[2] * unit[s].v[2]);
            if (!(min_cos > 0.0)) return false;                            // half angle of 90 degrees or more
        }
        double denom = sqrt(std::max(0.0, 1.0 - min_cos * min_cos)) + first_margin;
        for (int it = 0; it < 24; ++it) {
            denom = std::max(denom, 1.0e-3);                                // |q_k| <= ONE / 1e-3 < 2^22
            if (denom > 1.0) return false;
            uint32_t w[3];
            for (int a = 0; a < 3; ++a) w[a] = (uint32_t)(int32_t)llround(axis[a] * ((double)CONE_ONE / denom)) & 0x007FFFFFu;
            bool ok = (w[0] | w[1] | w[2]) != 0u;
            for (uint32_t s = lo[ni]; ok && s < hi[ni]; ++s)
                if (unit[s].state == 1) ok = cone_covers_normal(w[0], w[1], w[2], normals + 3 * (size_t)bvh.tri_order[s], origin_max);
            if (ok) { for (int a = 0; a < 3; ++a) words[(size_t)ni * 3 + a] = w[a]; return true; }
            denom = denom * 1.03 + 1.0e-4;
        }
        return false;
    };
    // nodes are independent of each other: whichever thread takes a node writes the same words
    std::atomic<uint32_t> next(0);
    auto worker = [&]() {
        for (;;) {
            const uint32_t base = next.fetch_add(64u);
            if (base >= nc) break;
            for (uint32_t ni = base; ni < std::min(nc, base + 64u); ++ni) cone_of(ni);
        }
    };
    const uint32_t nt = std::max(1u, std::min(threads, 64u));
    std::vector<std::thread> pool;
    for (uint32_t t = 1; t < nt; ++t) pool.emplace_back(worker);
    worker();
    for (std::thread & t : pool) t.join();
    const int scale_dword[3] = { 3, 14, 15 };
    for (uint32_t ni = 0; ni < nc; ++ni)
        for (int a = 0; a < 3; ++a) {
            uint32_t & d = bvh.nodes[(size_t)ni * BVH4_NODE_DWORDS + scale_dword[a]];
            d = (d & 0xFF800000u) | words[(size_t)ni * 3 + a];
        }
    return count_normal_cones(bvh.nodes.data(), nc);
}

// ---- open triangles (bvh_build.h).  How far from R a shadow ray can start, for a hit the render takes the flag for.
// Notation: u = 2^-24, A = coord_max, b = bias_max, all lengths Euclidean.  The hit: a ray (o, r), |o_k| <= 4 A, |r| = 1,
//   ob = fl(o + r bias), qp = fl(ob - fl(ob + r)), ap = fl(ob - a), th = fl(fl(ap.n) / fl(qp.n)), pos = fl(ob + fl(r th)),
// taken only when th < reach and |r.n| / |n| >= min_cos = 1/8 as the device evaluates it.
//   E   |qp_k + r_k| <= u (5 A + 2)(1 + u): the test walks the line ob - s qp, not ob + s r.  sqrt(3) E <= 2^-8 is required (a
//       scene beyond A ~ 2^13 gets no flags), so the true cosine c against that line is above min_cos - 2^-8 - 0.001 (the
//       last for the device's own rounding of the dot product and the normalisation): 1 / c <= 8.3, 1 / c^2 <= 69.
//   P   = reach (1 + 2^-8) + diameter of R: bounds |ap| and the true crossing parameter s.
//   T1  |th - s| <= (1 / c)(6 u P + 4.1 u s) + 2 u s <= (10.1 / c + 2) u P: the numerator's rounding (ap: u per component, the dot
//       product: 4 u |ap| |n|), the denominator's (4 u (1 + E) |n|), the division.
//   T2  |r + qp| s <= sqrt(3) E P: pos is laid out along r, the crossing lies along -qp.
//   T3  the roundings of r th and of the sum: sqrt(3) u (P + 2 A).
//   T4  the slack at R's edges.  Each edge test is a scalar triple product with an edge, off by at most 20 u |edge'| |ap| where
//       edge' is the longest edge the expression handles; the line may pass that much, over |edge x qp| >= |edge| c, outside
//       the edge, and 1 / c again carries it into R's plane: 20 u P ratio / c^2, ratio = perimeter / shortest edge.
//   T5  the record's triangle (a, ab, ac, n as stored) against the input's: the normal is off by an angle of at most
//       11 u L^2 / |n| (L the longest edge), the corners by 2 u L: (11 L^2 / |n| + 2) u L.  L^2 / |n| <= 2^10 is required.
// So pos lies within D = u P (10.1 / c + 2 + 20 ratio / c^2) + sqrt(3) E P + 4 u A + T5 of R.  The shadow ray starts at
// fl(fl(pos + gn bias) + d bias): the first push moves it b sin(angle between n and d) across the light and b along it at the
// most, the second b |d| along it, the two roundings 8 u A.  Both margins are raised by 2^-10 of themselves for their own
// arithmetic.  The occluder's side of the comparison is its axis-parallel box widened by 2^-14 A on every axis, the widest
// padding (box_pad at a camera 4 A out) under which the traversal - which reports no triangle whose leaf box the ray misses -
// is held to find what a loop over all triangles finds; shadow_open_flags adds it.
ShadowOpenBounds shadow_open_bounds(double coord_max) {
    ShadowOpenBounds b;
    b.coord_max = coord_max;
    b.bias_max = coord_max * (1.0 / 2048.0);
    b.reach = coord_max * 2.0;
    return b;
}

bool shadow_open_margins(const float * tri9, const float n[3], const float d[3], const ShadowOpenBounds & b, double * lateral, double * depth) {
    const double u = 5.9604644775390625e-8, lo60 = 8.673617379884035e-19, hi60 = 1152921504606846976.0;
    const double A = b.coord_max;
    if (!(A > 0.0 && A <= 1048576.0 && b.bias_max >= 0.0 && b.bias_max <= A && b.reach > 0.0 && b.reach <= 16.0 * A)) return false;
    const double E = u * (5.0 * A + 2.0) * (1.0 + u);
    if (!(1.7320508075688774 * E <= 0.00390625)) return false;
    double p[9];
    for (int k = 0; k < 9; ++k) { p[k] = (double)tri9[k]; if (!(fabs(p[k]) <= A)) return false; }      // (NaN fails too)
    const double N1 = fabs((double)n[0]) + fabs((double)n[1]) + fabs((double)n[2]);
    if (!(N1 >= lo60 && N1 <= hi60)) return false;
    const double dl = sqrt((double)d[0] * d[0] + (double)d[1] * d[1] + (double)d[2] * d[2]);
    if (!(dl >= 9.5367431640625e-7 && dl <= 1048576.0)) return false;
    double e[3];
    for (int i = 0; i < 3; ++i) {
        const int j = (i + 1) % 3;
        const double x = p[3 * j] - p[3 * i], y = p[3 * j + 1] - p[3 * i + 1], z = p[3 * j + 2] - p[3 * i + 2];
        e[i] = sqrt(x * x + y * y + z * z);
    }
    const double L = std::max(e[0], std::max(e[1], e[2])), s = std::min(e[0], std::min(e[1], e[2]));
    const double nl = sqrt((double)n[0] * n[0] + (double)n[1] * n[1] + (double)n[2] * n[2]);
    if (!(s > 0.0 && nl > 0.0)) return false;
    const double aspect = L * L / nl, ratio = (e[0] + e[1] + e[2]) / s;
    if (!(aspect <= 1024.0 && ratio <= 4096.0)) return false;
    const double P = b.reach * (1.0 + 0.00390625) + L;
    const double T5 = (11.0 * aspect + 2.0) * u * L;
    const double ic = 1.0 / (ShadowOpenBounds::min_cos - 0.00390625 - 0.001);              // 1 / c
    const double D = u * P * (10.1 * ic + 2.0 + 20.0 * ic * ic * ratio) + 1.7320508075688774 * E * P + 4.0 * u * A + T5;
    const double cosnd = std::min(1.0, fabs((double)n[0] * d[0] + (double)n[1] * d[1] + (double)n[2] * d[2]) / (nl * dl));
    const double sinnd = sqrt(std::max(0.0, 1.0 - cosnd * cosnd)) + 1e-6;                     // (+ the stored normal's own angle, amply)
    *lateral = (b.bias_max * std::min(1.0, sinnd) + D + 8.0 * u * A) * (1.0 + 0.0009765625);
    *depth = (b.bias_max * (1.0 + dl) + D + 8.0 * u * A) * (1.0 + 0.0009765625);
    return *lateral < hi60 && *depth < hi60;
}

uint32_t shadow_open_flags(const float * verts, const float * normals, uint32_t n_tris, const float d[3], const std::vector<uint32_t> & occluders,
                           const ShadowOpenBounds & b, uint32_t threads, std::vector<uint8_t> * open) {
    open->assign(n_tris, 0);
    if (occluders.empty() || n_tris == 0) return 0;
    const double dl = sqrt((double)d[0] * d[0] + (double)d[1] * d[1] + (double)d[2] * d[2]);
    if (!(dl >= 9.5367431640625e-7 && dl <= 1048576.0) || !(b.coord_max > 0.0 && b.coord_max <= 1048576.0)) return 0;
    // light space: (e0, e1) span the plane across d, w = d / |d|
    const double w[3] = { d[0] / dl, d[1] / dl, d[2] / dl };
    const int small = fabs(w[0]) <= fabs(w[1]) ? (fabs(w[0]) <= fabs(w[2]) ? 0 : 2) : (fabs(w[1]) <= fabs(w[2]) ? 1 : 2);
    double t[3] = { 0, 0, 0 };
    t[small] = 1.0;
    double e0[3] = { w[1] * t[2] - w[2] * t[1], w[2] * t[0] - w[0] * t[2], w[0] * t[1] - w[1] * t[0] };
    const double l0 = sqrt(e0[0] * e0[0] + e0[1] * e0[1] + e0[2] * e0[2]);
    for (double & x : e0) x /= l0;
    const double e1[3] = { w[1] * e0[2] - w[2] * e0[1], w[2] * e0[0] - w[0] * e0[2], w[0] * e0[1] - w[1] * e0[0] };
    auto to_light = [&](double x, double y, double z, double * q) {
        q[0] = x * e0[0] + y * e0[1] + z * e0[2]; q[1] = x * e1[0] + y * e1[1] + z * e1[2]; q[2] = x * w[0] + y * w[1] + z * w[2];
    };
    // the double arithmetic of the projection (the basis is orthonormal to 2^-52, a coordinate is at most 2 A): 2^-40 A, amply
    const double pad = b.coord_max * (1.0 / 16384.0), slop = b.coord_max * 9.094947017729282e-13;
    // ---- the occluders' footprints: the eight corners of each one's padded axis-parallel box
    const size_t m = occluders.size();
    std::vector<double> foot(m * 5);                  // lo0, hi0, lo1, hi1, largest depth
    double g_lo[2] = { 1e300, 1e300 }, g_hi[2] = { -1e300, -1e300 };
    for (size_t i = 0; i < m; ++i) {
        const float * v = verts + (size_t)occluders[i] * 9;
        double lo[3], hi[3];
        bool finite = true;
        for (int a = 0; a < 3; ++a) {
            lo[a] = std::min((double)v[a], std::min((double)v[3 + a], (double)v[6 + a])) - pad;
            hi[a] = std::max((double)v[a], std::max((double)v[3 + a], (double)v[6 + a])) + pad;
            finite = finite && fabs(lo[a]) <= 4.0 * b.coord_max && fabs(hi[a]) <= 4.0 * b.coord_max;
        }
        if (!finite) return 0;                        // an occluder nobody can place: nothing is provably open
        double * f = &foot[i * 5];
        f[0] = f[2] = 1e300; f[1] = f[3] = f[4] = -1e300;
        for (int c = 0; c < 8; ++c) {
            double q[3];
            to_light(c & 1 ? hi[0] : lo[0], c & 2 ? hi[1] : lo[1], c & 4 ? hi[2] : lo[2], q);
            f[0] = std::min(f[0], q[0]); f[1] = std::max(f[1], q[0]); f[2] = std::min(f[2], q[1]); f[3] = std::max(f[3], q[1]); f[4] = std::max(f[4], q[2]);
        }
        f[0] -= slop; f[1] += slop; f[2] -= slop; f[3] += slop; f[4] += slop;
        g_lo[0] = std::min(g_lo[0], f[0]); g_hi[0] = std::max(g_hi[0], f[1]); g_lo[1] = std::min(g_lo[1], f[2]); g_hi[1] = std::max(g_hi[1], f[3]);
    }
    // ---- the grid: cells the size of the occluders' mean footprint, coarser while filling it would cost more than 2^27 cell writes
    double mean_size = 0.0;
    for (size_t i = 0; i < m; ++i) mean_size += 0.5 * ((foot[i * 5 + 1] - foot[i * 5]) + (foot[i * 5 + 3] - foot[i * 5 + 2]));
    mean_size /= (double)m;
    const double extent = std::max(g_hi[0] - g_lo[0], g_hi[1] - g_lo[1]);
    int G = (int)std::max(1.0, std::min(4096.0, ceil(extent / std::max(mean_size, extent * (1.0 / 4096.0)))));
    double cell[2], inv[2];
    auto span = [&](double lo, double hi, int a, int * c0, int * c1) {     // cells [c0, c1] that [lo, hi] touches; false: none
        if (hi < g_lo[a] || lo > g_hi[a]) return false;
        // (2^-20 of a cell either side: the rounding of the subtraction and the product)
        *c0 = (int)std::max(0.0, std::min((double)(G - 1), floor((lo - g_lo[a]) * inv[a] - 9.5367431640625e-7)));
        *c1 = (int)std::max(0.0, std::min((double)(G - 1), floor((hi - g_lo[a]) * inv[a] + 9.5367431640625e-7)));
        return true;
    };
    for (;;) {
        for (int a = 0; a < 2; ++a) { cell[a] = std::max((g_hi[a] - g_lo[a]) / G, 1e-300); inv[a] = 1.0 / cell[a]; }
        double writes = 0.0;
        for (size_t i = 0; i < m; ++i) {
            int x0, x1, y0, y1;
            if (span(foot[i * 5], foot[i * 5 + 1], 0, &x0, &x1) && span(foot[i * 5 + 2], foot[i * 5 + 3], 1, &y0, &y1)) writes += (double)(x1 - x0 + 1) * (y1 - y0 + 1);
        }
        if (writes <= 134217728.0 || G == 1) break;
        G = std::max(1, G / 2);
    }
    std::vector<double> deepest((size_t)G * G, -1e300);
    for (size_t i = 0; i < m; ++i) {
        int x0, x1, y0, y1;
        if (!span(foot[i * 5], foot[i * 5 + 1], 0, &x0, &x1) || !span(foot[i * 5 + 2], foot[i * 5 + 3], 1, &y0, &y1)) continue;
        for (int y = y0; y <= y1; ++y)
            for (int x = x0; x <= x1; ++x) deepest[(size_t)y * G + x] = std::max(deepest[(size_t)y * G + x], foot[i * 5 + 4]);
    }
    // ---- the receivers: every triangle, in ranges of their own per thread
    auto classify = [&](uint32_t first, uint32_t last) {
        for (uint32_t r = first; r < last; ++r) {
            double lat, dep;
            const float * v = verts + (size_t)r * 9;
            if (!shadow_open_margins(v, normals + (size_t)r * 3, d, b, &lat, &dep)) continue;
            double lo[2] = { 1e300, 1e300 }, hi[2] = { -1e300, -1e300 }, nearest = 1e300;
            for (int c = 0; c < 3; ++c) {
                double q[3];
                to_light(v[3 * c], v[3 * c + 1], v[3 * c + 2], q);
                for (int a = 0; a < 2; ++a) { lo[a] = std::min(lo[a], q[a]); hi[a] = std::max(hi[a], q[a]); }
                nearest = std::min(nearest, q[2]);
            }
            const double floor_depth = nearest - dep - slop;
            int x0, x1, y0, y1;
            bool is_open = true;
            if (span(lo[0] - lat - slop, hi[0] + lat + slop, 0, &x0, &x1) && span(lo[1] - lat - slop, hi[1] + lat + slop, 1, &y0, &y1))
                for (int y = y0; y <= y1 && is_open; ++y)
                    for (int x = x0; x <= x1; ++x)
                        if (deepest[(size_t)y * G + x] >= floor_depth) { is_open = false; break; }
            (*open)[r] = is_open ? 1 : 0;
        }
    };
    const uint32_t n_thr = std::max(1u, std::min(threads, n_tris / 4096u + 1u));
    std::vector<std::thread> pool;
    for (uint32_t k = 0; k < n_thr; ++k) {
        const uint32_t first = (uint32_t)((uint64_t)n_tris * k / n_thr), last = (uint32_t)((uint64_t)n_tris * (k + 1) / n_thr);
        if (k + 1 == n_thr) classify(first, last); else pool.emplace_back(classify, first, last);
    }
    for (std::thread & th : pool) th.join();
    uint32_t count = 0;
    for (uint8_t f : *open) count += f;
    return count;
}

void make_empty_bvh(int width, BvhWide * out) {
    if (width != 4 && width != 8) throw std::invalid_argument("make_empty_bvh: width must be 4 or 8");
    *out = BvhWide();
    const bool eight = width == 8;
    const uint32_t one = 127u << 23;                                       // grid step 2^0
    out->node_dwords = eight ? BVH8_NODE_DWORDS : BVH4_NODE_DWORDS;
    out->nodes.assign(out->node_dwords, 0u);
    uint32_t * d = out->nodes.data();
    if (eight) {
        d[3] = d[6] = d[7] = one;                                          // no mask bit, no count bit
        d[4] = 1u;                                                         // child_base, tri_base: nothing follows
        for (int k = 8; k < 14; ++k) d[k] = 0xFFFFFFFFu;                   // lo = 255 > hi = 0 in every slot
    } else {
        d[3] = d[14] = d[15] = one;
        d[4] = d[5] = d[6] = 0xFFFFFFFFu;
        for (int k = 0; k < 4; ++k) d[10 + k] = (uint32_t)~(int32_t)0;     // the dummy record at slot n_tris = 0
    }
    out->node_count = 1;
    out->max_depth = 1;
    out->stack_bound = eight ? 3 : 5;
}

void rebase_bvh_nodes(const BvhWide & sub, uint32_t node_base, uint32_t tri_base, uint32_t * dst) {
    memcpy(dst, sub.nodes.data(), sub.nodes.size() * sizeof(uint32_t));
    for (uint32_t ni = 0; ni < sub.node_count; ++ni) {
        uint32_t * d = dst + (size_t)ni * sub.node_dwords;
        if (sub.node_dwords == BVH8_NODE_DWORDS) {
            d[4] += node_base;
            d[5] += tri_base;
            continue;
        }
        for (int k = 0; k < 4; ++k) {
            const int32_t link = (int32_t)d[10 + k];
            if (link >= 0) { d[10 + k] = (uint32_t)link + node_base; continue; }
            const uint32_t leaf = (uint32_t)~link;
            d[10 + k] = (uint32_t)~(int32_t)((((leaf >> 2) + tri_base) << 2) | (leaf & 3u));
        }
    }
}

const char * append_shadow_tree(const ShadowTreeBuild & how, const float * verts, const float * normals, uint32_t n_tris, const float d[3], double origin_max,
                                std::vector<uint32_t> * node_words, uint32_t node_base, uint32_t rec_base,
                                std::vector<uint32_t> * rec_tri, ShadowTreeResult * r, BvhWide * built,
                                const std::vector<uint32_t> * occluders) {
    *r = ShadowTreeResult();
    *built = BvhWide();
    rec_tri->clear();
    std::vector<uint32_t> own;
    if (!occluders) shadow_occluders(normals, n_tris, d, origin_max, &own);
    const std::vector<uint32_t> & ids = occluders ? *occluders : own;
    const uint32_t m = (uint32_t)ids.size();
    r->triangle_count = m;
    if ((uint64_t)m * 100u > (uint64_t)n_tris * how.ratio_percent) return nullptr;              // too few left out to pay
    BvhWide sub;
    if (m) {
        std::vector<float> sub_verts((size_t)m * 9);
        for (uint32_t i = 0; i < m; ++i) memcpy(&sub_verts[(size_t)i * 9], verts + (size_t)ids[i] * 9, 36);
        build_bvh_wide(how.width, sub_verts.data(), m, how.leaf_max, how.threads, &sub, how.trav_cost, how.opt);
    } else {
        make_empty_bvh(how.width, &sub);
    }
    if ((uint64_t)node_base + sub.node_count >= (1u << 26) || (uint64_t)rec_base + m + 1u >= (1u << 26)) return nullptr;
    if (node_words->size() != (size_t)node_base * sub.node_dwords) return "shadow tree: the node array does not end at node_base";
    node_words->resize(((size_t)node_base + sub.node_count) * sub.node_dwords);
    rebase_bvh_nodes(sub, node_base, rec_base, &(*node_words)[(size_t)node_base * sub.node_dwords]);
    for (uint32_t slot = 0; slot < m; ++slot) rec_tri->push_back(ids[sub.tri_order[slot]]);
    rec_tri->push_back(0xFFFFFFFFu);
    r->built = 1;
    r->node_count = sub.node_count;
    r->root = node_base;
    r->stack_bound = sub.stack_bound;
    built->nodes.swap(sub.nodes); built->tri_order.swap(sub.tri_order);
    built->node_dwords = sub.node_dwords; built->node_count = sub.node_count; built->max_depth = sub.max_depth; built->stack_bound = sub.stack_bound;
    return nullptr;
}

// Back end for a tree built elsewhere (the GPU LBVH builder, bvh_lbvh.hip): a binary radix tree over the triangles in
// sorted order.  Internal node i has children left[i] / right[i] (>= 0: internal node, < 0: ~sorted position of a
// single triangle), covers sorted positions [first[i], last[i]] and has box node_box[6 i .. 6 i + 5] (lo xyz, hi xyz);
// leaf_box holds the triangles' own boxes in sorted order.  Subtrees of at most leaf_max triangles become leaves.
namespace {
void radix_tree_to_binary(Builder & b, uint32_t n_tris, uint32_t leaf_max, const int32_t * left, const int32_t * right,
                          const uint32_t * first, const uint32_t * last, const float * node_box, const float * leaf_box,
                          const uint32_t * sorted_ids, float * scene_lo, float * scene_hi) {
    if (leaf_max < 1) leaf_max = 1;
    if (leaf_max > 4) leaf_max = 4;
    b.leaf_max = leaf_max;
    b.prims.resize(n_tris);
    Box scene;
    scene.reset();
    for (uint32_t i = 0; i < n_tris; ++i) {
        Prim & p = b.prims[i];
        for (int a = 0; a < 3; ++a) { p.box.lo[a] = leaf_box[6 * (size_t)i + a]; p.box.hi[a] = leaf_box[6 * (size_t)i + 3 + a]; p.c[a] = 0.0f; }
        p.id = sorted_ids[i];
        scene.grow(p.box);
    }
    for (int a = 0; a < 3; ++a) { scene_lo[a] = n_tris ? scene.lo[a] : 0.0f; scene_hi[a] = n_tris ? scene.hi[a] : 0.0f; }
    b.pool.resize(n_tris ? 2 * (size_t)n_tris : 1);
    b.next_node = 1;
    b.max_depth = 0;
    b.threads_free = 0;
    auto make_leaf = [&](TmpNode & n, const Box & box, uint32_t f, uint32_t c, uint32_t depth) {
        n.box = box; n.left = n.right = -1; n.first = f; n.count = c; n.depth = depth;
    };
    if (n_tris == 0) {
        Box zero = { { 0, 0, 0 }, { 0, 0, 0 } };
        make_leaf(b.pool[0], zero, 0, 1, 0);            // the all-zero dummy triangle the uploader always allocates
    } else if (n_tris <= leaf_max || n_tris == 1) {
        make_leaf(b.pool[0], scene, 0, n_tris, 0);
    } else if (b.opt.lbvh_plain) {
        // the radix tree as it is (round 1): fastest back end, 1.6 x slower to traverse than the SAH tree
        struct Todo { uint32_t tmp; int32_t src; uint32_t depth; };
        std::vector<Todo> todo;
        todo.push_back(Todo{ 0u, 0, 0u });
        while (!todo.empty()) {
            const Todo t = todo.back();
            todo.pop_back();
            TmpNode & n = b.pool[t.tmp];
            if (t.src < 0) {                                      // a single triangle
                const uint32_t pos = (uint32_t)~t.src;
                make_leaf(n, b.prims[pos].box, pos, 1, t.depth);
                continue;
            }
            Box box;
            for (int a = 0; a < 3; ++a) { box.lo[a] = node_box[6 * (size_t)t.src + a]; box.hi[a] = node_box[6 * (size_t)t.src + 3 + a]; }
            const uint32_t cnt = last[t.src] - first[t.src] + 1u;
            if (cnt <= leaf_max) { make_leaf(n, box, first[t.src], cnt, t.depth); continue; }
            n.box = box;
            n.depth = t.depth;
            n.first = n.count = 0;
            const uint32_t l = b.alloc(), r = b.alloc();
            n.left = (int32_t)l;
            n.right = (int32_t)r;
            todo.push_back(Todo{ l, left[t.src], t.depth + 1 });
            todo.push_back(Todo{ r, right[t.src], t.depth + 1 });
        }
    } else {
        // Hybrid (default): the device's radix tree only says which triangles belong together - its subtrees of at most
        // `cluster_max` triangles are CLUSTERS, contiguous runs of the Morton order -; the tree itself is surface-area
        // heuristic throughout: binned SAH ACROSS the clusters (a few thousand boxes), and the ordinary SAH builder INSIDE
        // each cluster (independent ranges, built by a pool of threads).  What the Morton order costs is then only where the
        // cluster boundaries lie.
        uint32_t cluster_max = 64;
        if (b.opt.lbvh_cluster >= 0) cluster_max = (uint32_t)std::max(4ll, std::min(1ll << 20, b.opt.lbvh_cluster));
        for (uint32_t i = 0; i < n_tris; ++i)
            for (int a = 0; a < 3; ++a) b.prims[i].c[a] = 0.5f * b.prims[i].box.lo[a] + 0.5f * b.prims[i].box.hi[a];
        struct Cluster { Box box; float c[3]; uint32_t first, count; };
        std::vector<Cluster> clusters;
        {
            std::vector<int32_t> stack;
            stack.push_back(0);
            while (!stack.empty()) {
                const int32_t src = stack.back();
                stack.pop_back();
                Cluster c;
                if (src < 0) {
                    const uint32_t pos = (uint32_t)~src;
                    c.box = b.prims[pos].box; c.first = pos; c.count = 1;
                } else {
                    const uint32_t cnt = last[src] - first[src] + 1u;
                    if (cnt > cluster_max) { stack.push_back(right[src]); stack.push_back(left[src]); continue; }
                    for (int a = 0; a < 3; ++a) { c.box.lo[a] = node_box[6 * (size_t)src + a]; c.box.hi[a] = node_box[6 * (size_t)src + 3 + a]; }
                    c.first = first[src]; c.count = cnt;
                }
                for (int a = 0; a < 3; ++a) c.c[a] = 0.5f * c.box.lo[a] + 0.5f * c.box.hi[a];
                clusters.push_back(c);
            }
        }
        // top tree: binned SAH over the clusters, weighted by their triangle counts; a leaf is one cluster
        struct Job { uint32_t tmp, first, count, depth; };
        std::vector<Job> cluster_jobs;
        std::vector<uint32_t> order(clusters.size());
        for (uint32_t i = 0; i < order.size(); ++i) order[i] = i;
        struct Range { uint32_t tmp, lo, hi, depth; };
        std::vector<Range> ranges;
        ranges.push_back(Range{ 0u, 0u, (uint32_t)order.size(), 0u });
        const int TB = 32;
        while (!ranges.empty()) {
            const Range rg = ranges.back();
            ranges.pop_back();
            if (rg.hi - rg.lo == 1) {
                const Cluster & c = clusters[order[rg.lo]];
                cluster_jobs.push_back(Job{ rg.tmp, c.first, c.count, rg.depth });
                continue;
            }
            Box bounds, cb;
            bounds.reset(); cb.reset();
            for (uint32_t i = rg.lo; i < rg.hi; ++i) { bounds.grow(clusters[order[i]].box); cb.grow(clusters[order[i]].c); }
            int best_axis = -1, best_split = -1;
            float best_cost = FLT_MAX;
            for (int axis = 0; axis < 3; ++axis) {
                const float cmin = cb.lo[axis], cmax = cb.hi[axis];
                if (!(cmax > cmin)) continue;
                const float scale = (float)TB / (cmax - cmin);
                Box bin_box[TB]; float bin_w[TB];
                for (int k = 0; k < TB; ++k) { bin_box[k].reset(); bin_w[k] = 0.0f; }
                for (uint32_t i = rg.lo; i < rg.hi; ++i) {
                    const Cluster & c = clusters[order[i]];
                    int k = (int)((c.c[axis] - cmin) * scale);
                    k = k < 0 ? 0 : (k >= TB ? TB - 1 : k);
                    bin_box[k].grow(c.box); bin_w[k] += (float)c.count;
                }
                float right_area[TB], right_w[TB];
                Box acc; acc.reset(); float w = 0.0f;
                for (int k = TB - 1; k > 0; --k) { acc.grow(bin_box[k]); w += bin_w[k]; right_area[k] = acc.half_area(); right_w[k] = w; }
                acc.reset(); w = 0.0f;
                for (int k = 0; k < TB - 1; ++k) {
                    acc.grow(bin_box[k]); w += bin_w[k];
                    if (w == 0.0f || right_w[k + 1] == 0.0f) continue;
                    const float cost = acc.half_area() * w + right_area[k + 1] * right_w[k + 1];
                    if (cost < best_cost) { best_cost = cost; best_axis = axis; best_split = k; }
                }
            }
            uint32_t mid = rg.lo;
            if (best_axis >= 0) {
                const float cmin = cb.lo[best_axis], scale = (float)TB / (cb.hi[best_axis] - cmin);
                uint32_t * bp = order.data() + rg.lo, * ep = order.data() + rg.hi;
                uint32_t * mp = std::partition(bp, ep, [&](uint32_t ci) {
                    int k = (int)((clusters[ci].c[best_axis] - cmin) * scale);
                    k = k < 0 ? 0 : (k >= TB ? TB - 1 : k);
                    return k <= best_split;
                });
                mid = rg.lo + (uint32_t)(mp - bp);
            }
            // coincident centres - or a run of lopsided splits that has used up the depth budget (the stack bound and the spill
            // areas are sized from the depth): halve the run
            if (mid == rg.lo || mid == rg.hi || rg.depth >= MAX_FORCED_DEPTH) mid = rg.lo + (rg.hi - rg.lo) / 2;
            TmpNode & n = b.pool[rg.tmp];
            n.box = bounds; n.depth = rg.depth; n.first = n.count = 0;
            const uint32_t l = b.alloc(), r = b.alloc();
            b.pool[rg.tmp].left = (int32_t)l;
            b.pool[rg.tmp].right = (int32_t)r;
            ranges.push_back(Range{ l, rg.lo, mid, rg.depth + 1 });
            ranges.push_back(Range{ r, mid, rg.hi, rg.depth + 1 });
        }
        const auto t_bottom = std::chrono::steady_clock::now();
        // bottom trees: the SAH builder on each cluster's range of the (Morton-ordered) triangle array, in parallel
        unsigned int hw = std::thread::hardware_concurrency();
        const unsigned int n_threads = std::max(1u, std::min(16u, hw ? hw : 1u));
        std::atomic<size_t> next_job(0);
        auto work = [&]() {
            for (;;) {
                const size_t k = next_job.fetch_add(1);
                if (k >= cluster_jobs.size()) break;
                const Job & j = cluster_jobs[k];
                b.build(j.tmp, j.first, j.count, j.depth);
            }
        };
        if (n_threads == 1 || cluster_jobs.size() < 64) {
            work();
        } else {
            std::vector<std::thread> pool;
            for (unsigned int t = 0; t < n_threads; ++t) pool.emplace_back(work);
            for (size_t t = 0; t < pool.size(); ++t) pool[t].join();
        }
        if (b.opt.debug) fprintf(stderr, "[prt] LBVH hybrid: %zu clusters (<= %u triangles); SAH inside them on %u threads: %.1f ms\n", clusters.size(), cluster_max, n_threads, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_bottom).count());
    }
}
}  // namespace

void build_bvh_wide_from_radix_tree(int width, uint32_t n_tris, uint32_t leaf_max, const int32_t * left, const int32_t * right,
                                    const uint32_t * first, const uint32_t * last, const float * node_box, const float * leaf_box,
                                    const uint32_t * sorted_ids, BvhWide * out, const BvhBuildOptions * opt) {
    *out = BvhWide();
    Builder b;
    b.configure(opt);
    radix_tree_to_binary(b, n_tris, leaf_max, left, right, first, last, node_box, leaf_box, sorted_ids, out->scene_lo, out->scene_hi);
    finish_wide(b, n_tris, width, out);
}

}  // namespace prt
