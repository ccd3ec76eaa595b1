// refit_host_harness.cpp - the refit's node step (par_raytracer_amd/csrc/dev_refit.h) on the host: builds trees of both widths
// over triangle soups of 0, 1, 4, 5, 37 and 1,280 triangles (bvh_build.cpp), refits them level by level, deepest first, with the
// very functions the kernels of kernels_refit.h call, and reports what tests/test_refit_host.py asserts on: the refit of the
// unmoved soup gives back the builder's node array bit for bit; after a move, check_bvh_wide (bvh_check.cpp) finds the tree
// conservative with every triangle referenced once; the level table covers every node once.  One line per (width, soup, move).
// It also runs the three kernels of kernels_refit.h themselves, one lane at a time, on an indexed mesh (kernels_on_the_host).
//
//   g++ -O1 -std=c++17 -ffp-contract=off -Itests/hip_shim -Ipar_raytracer_amd/csrc tests/refit_host_harness.cpp
//       par_raytracer_amd/csrc/bvh_build.cpp par_raytracer_amd/csrc/bvh_check.cpp -pthread -o /tmp/refit_host && /tmp/refit_host
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>            // tests/hip_shim: one lane at a time
// what kernels_refit.h needs beyond the shim (a wave of one lane: a shuffle returns the lane's own value)
static inline uint4 make_uint4(unsigned int x, unsigned int y, unsigned int z, unsigned int w) { uint4 r = { x, y, z, w }; return r; }
static inline float __shfl_xor(float v, int) { return v; }
static inline int __shfl_xor(int v, int) { return v; }
static inline unsigned int __float_as_uint(float f) { unsigned int v; memcpy(&v, &f, 4); return v; }
static inline unsigned int atomicMax(unsigned int * p, unsigned int v) { unsigned int o = *p; if (v > o) *p = v; return o; }
static inline unsigned int atomicOr(unsigned int * p, unsigned int v) { unsigned int o = *p; *p = o | v; return o; }

#include "bvh_build.h"
#include "kernels_refit.h"

using namespace prt;

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static double rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (double)(g_rng >> 11) / 9007199254740992.0; }

static std::vector<float> soup(uint32_t n) {                 // 9 floats per triangle
    std::vector<float> v;
    for (uint32_t t = 0; t < n; ++t) {
        const float c[3] = { (float)(rnd() * 8 - 4), (float)(rnd() * 3 + 0.125), (float)(rnd() * 8 - 4) };
        for (int k = 0; k < 9; ++k) v.push_back(c[k % 3] + (float)(rnd() - 0.5) * 0.75f);
    }
    return v;
}

// The host loop: what prt_update_geometry launches, one level per kernel launch, deepest level first.  A soup is un-indexed:
// its vertices are the positions, and the table of leaf slot s names vertices 3 t, 3 t + 1, 3 t + 2 of t = tri_order[s].
template <int WIDTH>
static bool refit_host(BvhWide & bvh, const std::vector<float> & verts, std::vector<unsigned int> & level_first) {
    const uint32_t n_tris = (uint32_t)(verts.size() / 9);
    if (!refit_level_table<WIDTH>(bvh.nodes.data(), bvh.node_count, &level_first)) return false;
    if (n_tris == 0) return true;                            // a scene of 0 triangles is a no-op (its one leaf is the dummy record)
    std::vector<unsigned int> table((size_t)n_tris * REFIT_TABLE_WORDS, 0u);
    for (uint32_t s = 0; s < n_tris; ++s)
        for (uint32_t c = 0; c < 3; ++c) table[(size_t)s * REFIT_TABLE_WORDS + c] = 3u * bvh.tri_order[s] + c;
    std::vector<RefitBox> boxes(bvh.node_count);
    for (size_t l = level_first.size() - 1; l-- > 0;)
        for (unsigned int ni = level_first[l]; ni < level_first[l + 1]; ++ni)
            refit_step<WIDTH>(&bvh.nodes[(size_t)ni * bvh.node_dwords], ni, bvh.node_count, n_tris, table.data(), verts.data(), boxes.data());
    return true;
}

static void exponents(const BvhWide & bvh, uint32_t ni, int * e) {
    const uint32_t * d = &bvh.nodes[(size_t)ni * bvh.node_dwords];
    const int at[2][3] = { { 3, 14, 15 }, { 3, 6, 7 } };
    for (int a = 0; a < 3; ++a) e[a] = (int)(d[at[bvh.node_dwords == BVH8_NODE_DWORDS][a]] >> 23 & 0xFFu) - 127;
}

// The three kernels of kernels_refit.h, one lane at a time (more blocks than needed: the bounds checks run too), on an INDEXED
// mesh of 777 triangles over 300 positions and 200 normals: the records against the upload's own expressions (prt_upload_scene),
// k_refit_bounds against a host maximum, the refitted nodes against check_bvh_wide, and the links untouched.
template <int WIDTH>
static void kernels_on_the_host() {
    const uint32_t nv = 300, nn = 200, n_tris = 777, n_rec = n_tris + 1;
    std::vector<float> pos(3 * nv), nrm(3 * nn), tan(3 * nn);
    std::vector<uint32_t> ip(3 * n_tris), in(3 * n_tris);
    for (float & v : pos) v = (float)(rnd() * 10 - 5);
    for (float & v : nrm) v = (float)(rnd() * 2 - 1);
    for (float & v : tan) v = (float)(rnd() * 2 - 1);
    for (uint32_t & v : ip) v = (uint32_t)(rnd() * nv);
    for (uint32_t & v : in) v = (uint32_t)(rnd() * nn);
    auto unindexed = [&](const std::vector<float> & P) {
        std::vector<float> v(9 * (size_t)n_tris);
        for (uint32_t t = 0; t < n_tris; ++t) for (int c = 0; c < 3; ++c) memcpy(&v[9 * t + 3 * c], &P[3 * ip[3 * t + c]], 12);
        return v;
    };
    BvhWide bvh;
    build_bvh_wide(WIDTH, unindexed(pos).data(), n_tris, 4, 2, &bvh);
    std::vector<unsigned int> level_first;
    const bool level_ok = refit_level_table<WIDTH>(bvh.nodes.data(), bvh.node_count, &level_first);
    std::vector<float4> tris(3 * n_rec), shade(4 * n_rec, make_float4(7, 7, 7, 7)), ttan(3 * n_rec), nodes4(bvh.nodes.size() / 4);
    memcpy(nodes4.data(), bvh.nodes.data(), bvh.nodes.size() * 4);
    std::vector<unsigned int> table((size_t)REFIT_TABLE_WORDS * n_tris);
    for (uint32_t s = 0; s < n_tris; ++s)
        for (int c = 0; c < 3; ++c) { table[6 * s + c] = ip[3 * bvh.tri_order[s] + c]; table[6 * s + 3 + c] = in[3 * bvh.tri_order[s] + c]; }
    std::vector<float> moved = pos;
    for (float & v : moved) v = v * 1.5f + (float)(rnd() - 0.5);
    std::vector<RefitBox> boxes(bvh.node_count);
    unsigned int bounds[2] = { 0, 0 };
    RefitArgs A;
    memset(&A, 0, sizeof(A));
    A.positions = moved.data(); A.normals = nrm.data(); A.tangents = tan.data(); A.table = table.data();
    A.n_tris = n_tris; A.node_count = bvh.node_count;
    A.nodes = nodes4.data(); A.tris = tris.data(); A.shade = shade.data(); A.tri_tan = ttan.data(); A.boxes = boxes.data(); A.bounds = bounds;
    blockDim.x = 1;
    gridDim.x = 3 * n_tris + 5;
    for (blockIdx.x = 0; blockIdx.x < gridDim.x; ++blockIdx.x) k_refit_bounds(A);
    float abs_max = 0.0f, got_max;
    for (uint32_t i = 0; i < 3 * n_tris; ++i) for (int k = 0; k < 3; ++k) abs_max = std::max(abs_max, fabsf(moved[3 * ip[i] + k]));
    memcpy(&got_max, &bounds[0], 4);
    const bool bounds_ok = got_max == abs_max && bounds[1] == 0;
    std::vector<float> nan_pos = moved;
    nan_pos[3 * ip[11] + 2] = NAN;
    unsigned int nan_bounds[2] = { 0, 0 };
    RefitArgs B = A;
    B.positions = nan_pos.data(); B.bounds = nan_bounds;
    for (blockIdx.x = 0; blockIdx.x < gridDim.x; ++blockIdx.x) k_refit_bounds(B);
    gridDim.x = n_tris + 3;
    for (blockIdx.x = 0; blockIdx.x < gridDim.x; ++blockIdx.x) k_refit_records(A);
    for (size_t l = level_first.size() - 1; level_ok && l-- > 0;) {
        const unsigned int first = level_first[l], count = level_first[l + 1] - first;
        for (blockIdx.x = 0; blockIdx.x < count + 2; ++blockIdx.x) k_refit_level<WIDTH>(A, first, count);
    }
    blockIdx.x = 0;
    uint32_t record_bad = 0;
    // the records written out on purpose, not through tri_record (dev_math.h): the kernel calls it, so this is its test
    for (uint32_t slot = 0; slot < n_tris; ++slot) {              // prt_upload_scene's loop, on the moved positions
        const uint32_t t = bvh.tri_order[slot];
        const float * pa = &moved[3 * ip[3 * t]], * pb = &moved[3 * ip[3 * t + 1]], * pc = &moved[3 * ip[3 * t + 2]];
        const f3 a = mk3(pa[0], pa[1], pa[2]), b = mk3(pb[0], pb[1], pb[2]), c = mk3(pc[0], pc[1], pc[2]);
        const f3 ab = b - a, ac = c - a, n = cross3(ab, ac);
        const float * n0 = &nrm[3 * in[3 * t]], * n1 = &nrm[3 * in[3 * t + 1]], * n2 = &nrm[3 * in[3 * t + 2]];
        const float * g0 = &tan[3 * in[3 * t]], * g1 = &tan[3 * in[3 * t + 1]], * g2 = &tan[3 * in[3 * t + 2]];
        const float4 e[10] = { make_float4(a.x, a.y, a.z, ab.x), make_float4(ab.y, ab.z, ac.x, ac.y), make_float4(ac.z, n.x, n.y, n.z),
                               make_float4(n0[0], n0[1], n0[2], n1[0]), make_float4(n1[1], n1[2], n2[0], n2[1]), make_float4(n2[2], n.x, n.y, n.z),
                               make_float4(7, 7, 7, 7),                  // the material word is not touched
                               make_float4(g0[0], g0[1], g0[2], g1[0]), make_float4(g1[1], g1[2], g2[0], g2[1]), make_float4(g2[2], 0, 0, 0) };
        if (memcmp(&tris[3 * slot], e, 48) || memcmp(&shade[4 * slot], e + 3, 64) || memcmp(&ttan[3 * slot], e + 7, 48)) record_bad++;
    }
    BvhWide t = bvh;
    memcpy(t.nodes.data(), nodes4.data(), t.nodes.size() * 4);
    uint64_t out[6];
    check_bvh_wide(unindexed(moved).data(), n_tris, t, out);
    uint32_t links_changed = 0;
    for (uint32_t ni = 0; ni < t.node_count; ++ni)
        for (uint32_t k = (WIDTH == 8 ? 4u : 10u); k < (WIDTH == 8 ? 6u : 14u); ++k)
            if (t.nodes[(size_t)ni * t.node_dwords + k] != bvh.nodes[(size_t)ni * t.node_dwords + k]) links_changed++;
    printf("kernels width %d | level_ok %d bounds_ok %d nan_flag %u record_bad %u violations %llu refs %llu links_changed %u validate %s\n", WIDTH,
           (int)level_ok, (int)bounds_ok, nan_bounds[1], record_bad, (unsigned long long)out[0], (unsigned long long)out[5], links_changed,
           validate_bvh_links(t, n_tris) ? "bad" : "null");
}

int main() {
    kernels_on_the_host<4>();
    kernels_on_the_host<8>();
    const uint32_t sizes[6] = { 0, 1, 4, 5, 37, 1280 };
    struct Move { const char * name; int shift; };           // shift: what a scale by a power of two adds to every exponent
    const Move moves[5] = { { "identity", 0 }, { "displaced", 0 }, { "flat_y", 0 }, { "scale_1024", 10 }, { "scale_2m20", -20 } };
    for (int width = 4; width <= 8; width += 4)
        for (uint32_t n : sizes) {
            const std::vector<float> a = soup(n);
            BvhWide built;
            build_bvh_wide(width, a.data(), n, 4, 2, &built);
            for (int m = 0; m < 5; ++m) {
                std::vector<float> b = a;
                for (size_t i = 0; i < b.size(); ++i) {
                    if (m == 1) b[i] += (float)(rnd() - 0.5) * 2.0f;
                    if (m == 2 && i % 3 == 1) b[i] = 0.0f;
                    if (m == 3) b[i] *= 1024.0f;
                    if (m == 4) b[i] *= 9.5367431640625e-07f;
                }
                BvhWide t = built;
                std::vector<unsigned int> level_first;
                const bool level_ok = width == 8 ? refit_host<8>(t, b, level_first) : refit_host<4>(t, b, level_first);
                // the level table: every node on exactly one level, every child one level below its parent
                uint32_t covered = 0, child_bad = 0;
                for (size_t l = 0; l + 1 < level_first.size(); ++l) {
                    covered += level_first[l + 1] - level_first[l];
                    for (unsigned int ni = level_first[l]; ni < level_first[l + 1]; ++ni) {
                        RefitSlot s[8];
                        if (width == 8) refit_slots<8>(&t.nodes[(size_t)ni * t.node_dwords], s); else refit_slots<4>(&t.nodes[(size_t)ni * t.node_dwords], s);
                        for (int k = 0; k < width; ++k)
                            if (s[k].kind == REFIT_NODE && !(l + 2 < level_first.size() && s[k].first >= level_first[l + 1] && s[k].first < level_first[l + 2])) child_bad++;
                    }
                }
                uint64_t out[6];
                check_bvh_wide(b.data(), n, t, out);
                const char * bad = validate_bvh_links(t, n);
                // exponents: how many differ from the builder's by anything but the move's shift (an axis of extent 0 stays at -100)
                uint32_t exp_bad = 0, exp_m100 = 0;
                for (uint32_t ni = 0; ni < t.node_count; ++ni) {
                    int e0[3], e1[3];
                    exponents(built, ni, e0);
                    exponents(t, ni, e1);
                    for (int k = 0; k < 3; ++k) {
                        if (e1[k] == -100) exp_m100++;
                        if (e1[k] != (e0[k] == -100 ? -100 : e0[k] + moves[m].shift)) exp_bad++;
                    }
                }
                int root_e[3];
                exponents(t, 0, root_e);
                printf("width %d n %u move %s | level_ok %d levels %zu depth %u covered %u nodes %u child_bad %u identical %d violations %llu refs %llu "
                       "exp_bad %u exp_m100 %u root_e %d %d %d validate %s\n", width, n, moves[m].name, (int)level_ok,
                       level_first.empty() ? (size_t)0 : level_first.size() - 1, t.max_depth, covered, t.node_count, child_bad,
                       (int)(t.nodes == built.nodes), (unsigned long long)out[0], (unsigned long long)out[5], exp_bad, exp_m100,
                       root_e[0], root_e[1], root_e[2], bad ? "bad" : "null");
            }
        }
    return 0;
}
