// query_grad_host_harness.cpp - the gradients of closest-hit queries (par_raytracer_amd/csrc/dev_query_grad.h,
// kernels_query_grad.h) on the host: runs k_qgrad_scan, k_qgrad_scatter and k_qgrad_resolve one lane at a time, in the order and
// with the decisions of prt_trace_rays_backward (csrc/prt_api.hip grad_backward), on the cases tests/test_query_grad_host.py
// writes to a file, and writes the results to another.  No GPU library is involved; the GPU suite compares the device's bits
// with this program's.
//
//   g++ -O1 -std=c++17 -ffp-contract=off -Itests/hip_shim -Ipar_raytracer_amd/csrc tests/query_grad_host_harness.cpp -o qg && ./qg in out
//
// Input: uint32 case count, then per case
//   uint32 count, position_count, index_count, group_count, flags (1 g_t, 2 g_bw, 4 g_position, 8 g_normal present; 16 merge), float ray_bias,
//   origins, directions (count x 3 f32), group (count i32), vertex0 (count u32), positions (position_count x 3 f32),
//   idx_positions (index_count u32), (first_index, index_count) per group, then the gradients present, in flag order.
// Output per case: int32 rc, uint32 hit_rays, skipped_rays, invalid rays, int32 unit_exponent, float max_contribution, then - rc 0
// only - positions gradient (position_count x 3 f32), origins and directions gradients (count x 3), and every ray's own 9
// vertex contributions (count x 9 f32, zeros for a ray that adds nothing).
//
// The wave merge (flag 16): a wave of ONE lane has nothing to merge, so the harness does what k_qgrad_scatter<true> does to a
// wave of 64 with a loop over groups of 64 consecutive rays - per distinct triangle of the group, the lanes' integers are summed
// and added once.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>            // tests/hip_shim: one lane at a time
// what kernels_query_grad.h needs beyond the shim.  A wave of one lane: the other 63 hold what an idle lane holds in the kernels'
// reductions - 0, the neutral element of their sums and of their maximum over non-negative floats.
static inline float __shfl_xor(float, int) { return 0.0f; }
static inline int __shfl_xor(int, int) { return 0; }
static inline int __shfl(int v, int) { return v; }
static inline unsigned int __float_as_uint(float f) { unsigned int v; memcpy(&v, &f, 4); return v; }
static inline unsigned int atomicMax(unsigned int * p, unsigned int v) { unsigned int o = *p; if (v > o) *p = v; return o; }

#include "kernels_query_grad.h"
#include "harness_io.h"

using namespace prt;

template <class K>
static void launch(K kernel, unsigned int grid, const QGradArgs & A) {
    blockDim.x = 1;
    gridDim.x = grid;
    for (blockIdx.x = 0; blockIdx.x < grid; ++blockIdx.x) kernel(A);
    blockIdx.x = 0;
}

int main(int argc, char ** argv) {
    FILE * in, * out;
    if (!open_in_out(argc, argv, "query_grad_host", &in, &out)) return 2;
    const unsigned int n_cases = rd<unsigned int>(in, 1)[0];
    for (unsigned int cs = 0; cs < n_cases; ++cs) {
        const std::vector<unsigned int> h = rd<unsigned int>(in, 5);
        const unsigned int n = h[0], n_pos = h[1], n_idx = h[2], n_groups = h[3], flags = h[4];
        const float ray_bias = rd<float>(in, 1)[0];
        const std::vector<float> origins = rd<float>(in, 3 * (size_t)n), dirs = rd<float>(in, 3 * (size_t)n);
        const std::vector<int> group = rd<int>(in, n);
        const std::vector<unsigned int> vertex0 = rd<unsigned int>(in, n);
        const std::vector<float> positions = rd<float>(in, 3 * (size_t)n_pos);
        const std::vector<unsigned int> idx = rd<unsigned int>(in, n_idx), runs = rd<unsigned int>(in, 2 * (size_t)n_groups);
        const std::vector<float> g_t = rd<float>(in, flags & 1u ? n : 0), g_bw = rd<float>(in, flags & 2u ? 3 * (size_t)n : 0),
                                 g_pos = rd<float>(in, flags & 4u ? 3 * (size_t)n : 0), g_nrm = rd<float>(in, flags & 8u ? 3 * (size_t)n : 0);
        const bool merge = (flags & 16u) != 0;
        // sentinels: what a call must overwrite (positions) or write for every ray (origins, directions)
        std::vector<float> gp(3 * (size_t)n_pos, 7.5f), go(3 * (size_t)n, 7.5f), gd(3 * (size_t)n, 7.5f), contrib(9 * (size_t)n, 0.0f);
        std::vector<long long> acc(3 * (size_t)n_pos + 1, 0);
        unsigned int words[QGRAD_WORDS] = { 0u, 0u, 0u, 0u };
        QGradArgs A;
        memset(&A, 0, sizeof(A));
        A.origins = origins.data(); A.dirs = dirs.data(); A.group = group.data(); A.vertex0 = vertex0.data(); A.positions = positions.data();
        A.g_t = flags & 1u ? g_t.data() : nullptr; A.g_bw = flags & 2u ? g_bw.data() : nullptr;
        A.g_pos = flags & 4u ? g_pos.data() : nullptr; A.g_nrm = flags & 8u ? g_nrm.data() : nullptr;
        A.g_origins = go.data(); A.g_dirs = gd.data(); A.g_positions = gp.data();
        A.idx_positions = idx.data(); A.group_runs = runs.data(); A.words = words;
        A.count = n; A.group_count = n_groups; A.position_count = n_pos; A.ray_bias = ray_bias;
        int rc = 0;
        float m = 0.0f;
        if (n == 0) {
            std::fill(gp.begin(), gp.end(), 0.0f);
        } else {
            launch(k_qgrad_scan, n / 3 + 2, A);                   // fewer blocks than rays: the grid-stride loop runs
            memcpy(&m, &words[QGRAD_W_MAX], 4);
            if (words[QGRAD_W_INVALID]) rc = -1;
        }
        if (n && rc == 0) {
            const bool adds = words[QGRAD_W_HIT] && m > 0.0f;
            A.unit_exponent = m > 0.0f ? qgrad_unit_exponent(m, n) : 0;
            A.acc = adds && !merge ? acc.data() : nullptr;
            if (merge) launch(k_qgrad_scatter<true>, n / 5 + 3, A); else launch(k_qgrad_scatter<false>, n / 5 + 3, A);
            if (adds && merge) {
                for (unsigned int base = 0; base < n; base += 64u) {
                    unsigned int key[64], vi[64][3];
                    long long q[64][9];
                    bool live[64];
                    const unsigned int lanes = n - base < 64u ? n - base : 64u;
                    for (unsigned int l = 0; l < lanes; ++l) {
                        QGradOut g;
                        bool ok = false;
                        live[l] = qgrad_ray(A, base + l, &key[l], vi[l], &ok, &g) == QGRAD_HIT && ok;
                        if (live[l]) qgrad_fixed9(g, A.unit_exponent, q[l]);
                    }
                    for (unsigned int l = 0; l < lanes; ++l) {
                        if (!live[l]) continue;
                        long long s[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };
                        for (unsigned int k = l; k < lanes; ++k)
                            if (live[k] && key[k] == key[l]) { for (int c = 0; c < 9; ++c) s[c] += q[k][c]; if (k != l) live[k] = false; }
                        for (int c = 0; c < 3; ++c) for (int k = 0; k < 3; ++k) acc[3 * (size_t)vi[l][c] + k] += s[3 * c + k];
                    }
                }
            }
            A.acc = acc.data();
            if (adds) launch(k_qgrad_resolve, 3 * n_pos + 2, A);
            else std::fill(gp.begin(), gp.end(), 0.0f);
            for (unsigned int i = 0; i < n; ++i) {
                unsigned int first, vi[3];
                QGradOut g;
                bool ok = false;
                if (qgrad_ray(A, i, &first, vi, &ok, &g) == QGRAD_HIT && ok) {
                    const float c[9] = { g.ga.x, g.ga.y, g.ga.z, g.gb.x, g.gb.y, g.gb.z, g.gc.x, g.gc.y, g.gc.z };
                    memcpy(&contrib[9 * (size_t)i], c, sizeof(c));
                }
            }
        }
        const int unit = rc == 0 ? A.unit_exponent : 0;
        wr(out, &rc, 1); wr(out, &words[QGRAD_W_HIT], 1); wr(out, &words[QGRAD_W_SKIPPED], 1); wr(out, &words[QGRAD_W_INVALID], 1);
        wr(out, &unit, 1); wr(out, &m, 1);
        if (rc == 0) { wr(out, gp.data(), gp.size()); wr(out, go.data(), go.size()); wr(out, gd.data(), gd.size()); wr(out, contrib.data(), contrib.size()); }
    }
    fclose(in);
    if (fclose(out)) return 2;
    return 0;
}
