// bvh_dump.cpp - one hash per builder configuration, to show that a change to csrc/bvh_build.cpp left every tree byte for
// byte as it was: build this file once against the old bvh_build.cpp and once against the new one, run both ON THE SAME
// MACHINE (log2 / ldexp rounding belongs to the machine's libm, so hashes are not portable) and diff the outputs.
// Host only.
//
//   g++ -O2 -std=c++17 -ffp-contract=off -pthread -I<dir of bvh_build.h> tools/bvh_dump.cpp <dir>/bvh_build.cpp -o /tmp/bvh_dump
//   /tmp/bvh_dump                       the sweep: "<configuration> <FNV-1a 64> <nodes>" per line, about 20 s
//   /tmp/bvh_dump time GRID THREADS     a terrain of 2 GRID^2 triangles through both widths with the builder's debug lines
//                                       (the "[prt] BVH back end" times) on stderr
// -DBVH_DUMP_PER_WIDTH_API builds it against a bvh_build.cpp from before build_bvh_wide (one entry point and result type per
// width).
//
// The hash covers nodes, tri_order, node_count, max_depth, stack_bound and scene_lo / scene_hi.  Scenes: 0, 1, 3 triangles,
// 37 coincident ones, about 2 k and about 90 k (terrain + random soup + coincident copies).  4-wide: collapse {default,
// greedy, dp} x SAH_SWEEP {off, 8}; 8-wide: the same x width {8, 6} x axis rule {0, 1, 2}; all of it x leaf_max {1, 4} x
// threads {1, 8}.  The *_from_radix_tree entry points get a radix tree made here (Morton order of the centroids, split on
// the highest differing bit): LBVH_PLAIN {0, 1} x LBVH_CLUSTER {default, 8}.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <vector>

#include "bvh_build.h"
#include "prt_options.h"

using namespace prt;

#if defined(BVH_DUMP_PER_WIDTH_API)
struct BvhWide {
    std::vector<uint32_t> nodes, tri_order;
    uint32_t node_count, max_depth, stack_bound;
    float scene_lo[3], scene_hi[3];
};
template <class R> static void take(const R & r, BvhWide * o) {
    o->nodes = r.nodes; o->tri_order = r.tri_order; o->node_count = r.node_count; o->max_depth = r.max_depth; o->stack_bound = r.stack_bound;
    memcpy(o->scene_lo, r.scene_lo, 12); memcpy(o->scene_hi, r.scene_hi, 12);
}
static void build_bvh_wide(int width, const float * verts, uint32_t n_tris, uint32_t leaf_max, uint32_t threads, BvhWide * out, float trav_cost,
                           const BvhBuildOptions * opt) {
    if (width == 4) { Bvh4Result r; build_bvh4q(verts, n_tris, leaf_max, threads, &r, trav_cost, opt); take(r, out); }
    else { Bvh8Result r; build_bvh8q(verts, n_tris, leaf_max, threads, &r, trav_cost, opt); take(r, out); }
}
static void build_bvh_wide_from_radix_tree(int width, uint32_t n_tris, uint32_t leaf_max, const int32_t * left, const int32_t * right,
                                           const uint32_t * first, const uint32_t * last, const float * node_box, const float * leaf_box,
                                           const uint32_t * sorted_ids, BvhWide * out, const BvhBuildOptions * opt) {
    if (width == 4) { Bvh4Result r; build_bvh4q_from_radix_tree(n_tris, leaf_max, left, right, first, last, node_box, leaf_box, sorted_ids, &r, opt); take(r, out); }
    else { Bvh8Result r; build_bvh8q_from_radix_tree(n_tris, leaf_max, left, right, first, last, node_box, leaf_box, sorted_ids, &r, opt); take(r, out); }
}
#endif

static uint64_t g_rng = 0x243F6A8885A308D3ull;
static double rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (double)(g_rng >> 11) / 9007199254740992.0; }

typedef std::vector<float> Verts;          // 9 floats per triangle

static void terrain(Verts & v, int grid) {
    auto height = [](float x, float z) { return 0.35f * sinf(x * 0.9f) * cosf(z * 0.7f) + 0.1f * sinf(x * 3.1f + z * 2.3f); };
    for (int i = 0; i < grid; ++i)
        for (int j = 0; j < grid; ++j) {
            const float x0 = i * 0.25f - grid * 0.125f, x1 = x0 + 0.25f, z0 = j * 0.25f - grid * 0.125f, z1 = z0 + 0.25f;
            const float t[18] = { x0, height(x0, z0), z0, x0, height(x0, z1), z1, x1, height(x1, z0), z0,
                                  x1, height(x1, z0), z0, x0, height(x0, z1), z1, x1, height(x1, z1), z1 };
            v.insert(v.end(), t, t + 18);
        }
}

// `n` random triangles above a terrain of `grid` cells a side, every fifth of them twice
static void soup(Verts & v, int grid, int n) {
    const double span = grid * 0.25;
    for (int k = 0; k < n; ++k) {
        const float cx = (float)((rnd() - 0.5) * span), cy = (float)(rnd() * 2 + 0.3), cz = (float)((rnd() - 0.5) * span);
        float t[9];
        for (int q = 0; q < 9; ++q) t[q] = (float)(rnd() - 0.5) * 0.8f + (q % 3 == 0 ? cx : q % 3 == 1 ? cy : cz);
        v.insert(v.end(), t, t + 9);
        if (k % 5 == 0) v.insert(v.end(), t, t + 9);
    }
}

static Verts coincident(int n) {
    Verts v;
    const float t[9] = { 0.5f, 0.25f, -1.0f, 1.5f, 0.25f, -1.0f, 0.5f, 1.0f, -2.0f };
    for (int k = 0; k < n; ++k) v.insert(v.end(), t, t + 9);
    return v;
}

// Binary radix tree over the Morton order of the triangles' centroids, in the arrays build_bvh_wide_from_radix_tree reads.
struct RadixTree {
    std::vector<int32_t> left, right;
    std::vector<uint32_t> first, last, sorted_ids;
    std::vector<float> node_box, leaf_box;
    std::vector<uint64_t> keys;

    // the subtree over sorted positions [lo, hi], lo < hi; returns its node and leaves its box in node_box
    int32_t split(uint32_t lo, uint32_t hi) {
        const int32_t me = (int32_t)left.size();
        left.push_back(0); right.push_back(0); first.push_back(lo); last.push_back(hi);
        node_box.resize(node_box.size() + 6);
        uint32_t mid = lo + (hi - lo + 1) / 2;                          // equal keys: halve the run
        if (keys[lo] != keys[hi]) {
            const uint64_t bit = 1ull << (63 - __builtin_clzll(keys[lo] ^ keys[hi]));
            mid = (uint32_t)(std::partition_point(keys.begin() + lo, keys.begin() + hi + 1, [&](uint64_t k) { return !(k & bit); }) - keys.begin());
        }
        const int32_t l = mid - 1 == lo ? ~(int32_t)lo : split(lo, mid - 1), r = mid == hi ? ~(int32_t)hi : split(mid, hi);
        left[me] = l; right[me] = r;
        for (int a = 0; a < 3; ++a) {
            const float * lb = l < 0 ? &leaf_box[6 * (size_t)~l] : &node_box[6 * (size_t)l], * rb = r < 0 ? &leaf_box[6 * (size_t)~r] : &node_box[6 * (size_t)r];
            node_box[6 * (size_t)me + a] = std::min(lb[a], rb[a]);
            node_box[6 * (size_t)me + 3 + a] = std::max(lb[3 + a], rb[3 + a]);
        }
        return me;
    }

    explicit RadixTree(const Verts & v) {
        const uint32_t n = (uint32_t)(v.size() / 9);
        std::vector<float> box(6 * (size_t)n);
        float lo[3] = { 0, 0, 0 }, hi[3] = { 0, 0, 0 };
        for (uint32_t i = 0; i < n; ++i)
            for (int a = 0; a < 3; ++a) {
                const float p = v[9 * (size_t)i + a], q = v[9 * (size_t)i + 3 + a], r = v[9 * (size_t)i + 6 + a];
                box[6 * (size_t)i + a] = std::min(p, std::min(q, r));
                box[6 * (size_t)i + 3 + a] = std::max(p, std::max(q, r));
                if (i == 0 || box[6 * (size_t)i + a] < lo[a]) lo[a] = box[6 * (size_t)i + a];
                if (i == 0 || box[6 * (size_t)i + 3 + a] > hi[a]) hi[a] = box[6 * (size_t)i + 3 + a];
            }
        std::vector<uint64_t> key(n, 0);
        for (uint32_t i = 0; i < n; ++i)
            for (int a = 0; a < 3; ++a) {
                const double c = 0.5 * box[6 * (size_t)i + a] + 0.5 * box[6 * (size_t)i + 3 + a], ext = (double)hi[a] - lo[a];
                const uint64_t q = ext > 0 ? (uint64_t)std::min(2097151.0, (c - lo[a]) / ext * 2097152.0) : 0;
                for (int bit = 0; bit < 21; ++bit) key[i] |= (q >> bit & 1ull) << (3 * bit + a);
            }
        sorted_ids.resize(n);
        std::iota(sorted_ids.begin(), sorted_ids.end(), 0u);
        std::sort(sorted_ids.begin(), sorted_ids.end(), [&](uint32_t x, uint32_t y) { return key[x] < key[y] || (key[x] == key[y] && x < y); });
        keys.resize(n);
        leaf_box.resize(6 * (size_t)n);
        for (uint32_t i = 0; i < n; ++i) {
            keys[i] = key[sorted_ids[i]];
            memcpy(&leaf_box[6 * (size_t)i], &box[6 * (size_t)sorted_ids[i]], 24);
        }
        if (n >= 2) split(0, n - 1);
    }
};

static uint64_t fnv(uint64_t h, const void * p, size_t n) {
    const unsigned char * b = (const unsigned char *)p;
    for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 0x100000001B3ull; }
    return h;
}

static void print(const char * what, const BvhWide & r) {
    uint64_t h = 0xCBF29CE484222325ull;
    h = fnv(h, r.nodes.data(), r.nodes.size() * 4);
    h = fnv(h, r.tri_order.data(), r.tri_order.size() * 4);
    h = fnv(h, &r.node_count, 4); h = fnv(h, &r.max_depth, 4); h = fnv(h, &r.stack_bound, 4);
    h = fnv(h, r.scene_lo, 12); h = fnv(h, r.scene_hi, 12);
    printf("%s %016llx %u\n", what, (unsigned long long)h, r.node_count);
}

int main(int argc, char ** argv) {
    if (argc == 4 && !strcmp(argv[1], "time")) {
        Verts v;
        terrain(v, atoi(argv[2]));
        BvhBuildOptions opt;
        opt.debug = 1;
        for (int width = 4; width <= 8; width += 4) {
            BvhWide r;
            build_bvh_wide(width, v.data(), (uint32_t)(v.size() / 9), 4, (uint32_t)atoi(argv[3]), &r, 1.0f, &opt);
            char what[64];
            snprintf(what, sizeof(what), "w%d terrain %s", width, argv[2]);
            print(what, r);
        }
        return 0;
    }
    if (argc != 1) { fprintf(stderr, "usage: bvh_dump | bvh_dump time GRID THREADS\n"); return 2; }

    struct Scene { const char * name; Verts v; };
    std::vector<Scene> scenes;
    Verts three;
    soup(three, 8, 3);                                   // its first triangle twice: 4 entries, cut to 3
    three.resize(27);
    Verts k2, k90;
    terrain(k2, 30); soup(k2, 30, 200);
    terrain(k90, 208); soup(k90, 208, 3100);
    scenes.push_back(Scene{ "0", Verts() });
    scenes.push_back(Scene{ "1", coincident(1) });
    scenes.push_back(Scene{ "3", three });
    scenes.push_back(Scene{ "37same", coincident(37) });
    scenes.push_back(Scene{ "2k", k2 });
    scenes.push_back(Scene{ "90k", k90 });

    const char * collapse_name[3] = { "default", "greedy", "dp" };
    char what[160];
    for (const Scene & sc : scenes) {
        const uint32_t n = (uint32_t)(sc.v.size() / 9);
        const RadixTree tree(sc.v);
        for (uint32_t leaf_max = 1; leaf_max <= 4; leaf_max += 3) {
            for (uint32_t threads = 1; threads <= 8; threads += 7)
                for (int collapse = -1; collapse <= 1; ++collapse)
                    for (int sweep = 0; sweep <= 8; sweep += 8)
                        for (int width = 4; width <= 8; width += 4)
                            for (int w = 8; w >= (width == 8 ? 6 : 8); w -= 2)
                                for (int axis = 0; axis <= (width == 8 ? 2 : 0); ++axis) {
                                    BvhBuildOptions opt;
                                    opt.collapse = collapse;
                                    if (sweep) opt.sah_sweep = sweep;
                                    opt.width = w;
                                    opt.axis_rule = axis;
                                    BvhWide r;
                                    build_bvh_wide(width, sc.v.data(), n, leaf_max, threads, &r, 1.0f, &opt);
                                    snprintf(what, sizeof(what), "w%d tris=%s(%u) leaf=%u threads=%u collapse=%s sweep=%d width=%d axis=%d", width, sc.name, n,
                                             leaf_max, threads, collapse_name[collapse + 1], sweep, w, axis);
                                    print(what, r);
                                }
            for (int plain = 0; plain <= 1; ++plain)
                for (int cluster = -1; cluster <= 8; cluster += 9)
                    for (int width = 4; width <= 8; width += 4) {
                        BvhBuildOptions opt;
                        opt.lbvh_plain = plain;
                        opt.lbvh_cluster = cluster;
                        BvhWide r;
                        build_bvh_wide_from_radix_tree(width, n, leaf_max, tree.left.data(), tree.right.data(), tree.first.data(), tree.last.data(),
                                                       tree.node_box.data(), tree.leaf_box.data(), tree.sorted_ids.data(), &r, &opt);
                        snprintf(what, sizeof(what), "w%d radix tris=%s(%u) leaf=%u plain=%d cluster=%d", width, sc.name, n, leaf_max, plain, cluster);
                        print(what, r);
                    }
        }
    }
    return 0;
}
