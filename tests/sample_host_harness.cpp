// sample_host_harness.cpp - the definition of prt_sample_surface and prt_sample_surface_backward (par_raytracer_amd/csrc/dev_sample.h,
// dev_sample_grad.h, kernels_sample_grad.h, include/prt.h), compiled for the host with tests/hip_shim: a brute force in input order.
// The records are laid out as prt_upload_scene lays them out (a, b - a, c - a), slot = input triangle - the answer does not depend
// on the tree, so none is built; the weights, E, unit_exponent, W and C come from the PRT_HD functions of dev_sample.h and plain
// 64-bit integer adds, every sample from sample_draw, sample_pick and the three output expressions; the gradients run
// k_sgrad_scan, k_sgrad_scatter and k_qgrad_resolve one lane at a time, in the order and with the decisions of grad_backward
// (csrc/prt_api.hip).  tests/sample_cases.py writes the cases and reads the results; tests/test_sample_host.py asserts on them,
// tests/test_gpu_sample.py compares the device with them bit for bit.
//
//   g++ -O1 -std=c++17 -ffp-contract=off -Itests/hip_shim -Ipar_raytracer_amd/csrc tests/sample_host_harness.cpp -o sample_host
//       && ./sample_host cases.bin results.bin        (or: ./sample_host --pick lists.bin picks.bin)
//
// cases.bin: u32 case count, then per case 6 x u32 (positions, indices, groups, requests, gradient calls, 0), positions (x3 f32),
// idx_positions (u32), the groups' (first_index, index_count) (2 x u32), per request 3 x u64 (seed, first, count), per gradient
// call 2 x u32 (count, flags: 1 g_point, 2 g_normal present; 16 merge), group (i32), vertex0 (u32), bw (x3 f32), then the
// gradients present (x3 f32 each).
// results.bin, per case: f64 area, u64 total_weight, i32 unit_exponent, u32 live_triangles, W (u64 per input triangle); per
// request point, bw, normal (x3 f32 each), vertex0 (u32), group (i32); per gradient call i32 rc, u32 contributing, skipped,
// invalid samples, i32 unit_exponent, f32 max_contribution and the positions gradient (x3 f32) as the call left it - it starts
// filled with the sentinel 7.5, which a refused call (rc -1) must not have touched.
// --pick: u32 list count, per list 2 x u32 (weights, draws), W (u64 each), r0 (u64 each); out: i64 per draw, the triangle
// sample_pick takes for x = mulhi64(r0, T), -1 when T == 0.
//
// The wave merge (flag 16): a wave of ONE lane has nothing to merge, so the harness does what k_sgrad_scatter<true> does to a
// wave of 64 with a loop over groups of 64 consecutive samples, as tests/closest_grad_host_harness.cpp does.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>            // tests/hip_shim: one lane at a time
using std::isfinite;
// what the kernels need beyond the shim.  A wave of one lane: the other 63 hold the neutral element of the reductions.
static inline float __shfl_xor(float, int) { return 0.0f; }
static inline int __shfl_xor(int, int) { return 0; }
static inline int __shfl(int v, int) { return v; }
static inline unsigned int __float_as_uint(float f) { unsigned int v; memcpy(&v, &f, 4); return v; }
static inline unsigned int atomicMax(unsigned int * p, unsigned int v) { unsigned int o = *p; if (v > o) *p = v; return o; }

#include "kernels_sample_grad.h"
#include "harness_io.h"
#include "harness_mesh.h"

using namespace prt;

template <class K, class ARGS>
static void launch(K kernel, unsigned int grid, const ARGS & A) {
    blockDim.x = 1;
    gridDim.x = grid;
    for (blockIdx.x = 0; blockIdx.x < grid; ++blockIdx.x) kernel(A);
    blockIdx.x = 0;
}

static int pick_mode(FILE * fin, FILE * fout) {
    const uint32_t n_lists = rd<uint32_t>(fin, 1)[0];
    for (uint32_t li = 0; li < n_lists; ++li) {
        const std::vector<uint32_t> hd = rd<uint32_t>(fin, 2);
        const std::vector<unsigned long long> W = rd<unsigned long long>(fin, hd[0]), r0 = rd<unsigned long long>(fin, hd[1]);
        std::vector<unsigned long long> C(W.size());
        unsigned long long total = 0;
        for (size_t t = 0; t < W.size(); ++t) { total += W[t]; C[t] = total; }
        std::vector<long long> out(r0.size());
        for (size_t i = 0; i < r0.size(); ++i)
            out[i] = total ? (long long)sample_pick(C.data(), (unsigned int)C.size(), sample_mulhi64(r0[i], total)) : -1ll;
        wr(fout, out);
    }
    return 0;
}

int main(int argc, char ** argv) {
    const bool pick = argc == 4 && !strcmp(argv[1], "--pick");
    if (argc != 3 && !pick) { fprintf(stderr, "usage: sample_host [--pick] in.bin out.bin\n"); return 2; }
    FILE * fin, * fout;
    if (!open_in_out(argc, argv, "sample_host", &fin, &fout)) return 2;
    if (pick) {
        const int rc = pick_mode(fin, fout);
        fclose(fin);
        return fclose(fout) ? 2 : rc;
    }
    const uint32_t n_cases = rd<uint32_t>(fin, 1)[0];
    for (uint32_t ci = 0; ci < n_cases; ++ci) {
        const std::vector<uint32_t> hd = rd<uint32_t>(fin, 6);
        const uint32_t n_pos = hd[0], n_idx = hd[1], n_groups = hd[2], n_requests = hd[3], n_grads = hd[4], n_tris = n_idx / 3;
        const std::vector<float> pos = rd<float>(fin, 3 * (size_t)n_pos);
        const std::vector<uint32_t> idx = rd<uint32_t>(fin, n_idx);
        const std::vector<uint32_t> runs = rd<uint32_t>(fin, 2 * (size_t)n_groups);

        // the records (slot = input triangle) and the leaf table
        const std::vector<float4> tris = mesh::records(mesh::unindexed(pos, idx), n_tris, nullptr);
        const std::vector<uint2> leaf_map = mesh::leaf_map(runs, n_groups, n_tris, nullptr);
        // the table: what k_sample_weights .. k_sample_offsets build, in input order
        std::vector<double> weight(n_tris);
        unsigned long long max_bits = 0;
        for (uint32_t t = 0; t < n_tris; ++t) {
            const float4 r0 = tris[(size_t)t * 3], r1 = tris[(size_t)t * 3 + 1], r2 = tris[(size_t)t * 3 + 2];
            weight[t] = sample_weight(mk3(r0.w, r1.x, r1.y), mk3(r1.z, r1.w, r2.x));
            const unsigned long long b = sample_double_bits(weight[t]);
            if (b > max_bits) max_bits = b;
        }
        const int unit = sample_unit_exponent(max_bits, n_tris);
        std::vector<unsigned long long> W(n_tris), C(n_tris);
        unsigned long long total = 0;
        uint32_t live = 0;
        for (uint32_t t = 0; t < n_tris; ++t) {
            W[t] = max_bits ? sample_to_fixed(weight[t], unit) : 0ull;
            live += W[t] ? 1u : 0u;
            total += W[t];
            C[t] = total;
        }
        const double area = 0.5 * (double)total * qgrad_pow2(unit);
        wr(fout, &area, 1); wr(fout, &total, 1); wr(fout, &unit, 1); wr(fout, &live, 1); wr(fout, W);

        for (uint32_t rq = 0; rq < n_requests; ++rq) {
            const std::vector<unsigned long long> r = rd<unsigned long long>(fin, 3);
            const unsigned long long seed = r[0], first = r[1];
            const size_t n = (size_t)r[2];
            std::vector<float> point(3 * n, 0.0f), bw(3 * n, 0.0f), normal(3 * n, 0.0f);
            std::vector<unsigned int> vertex0(n, 0xFFFFFFFFu);
            std::vector<int> group(n, -1);
            for (size_t i = 0; i < n && total; ++i) {
                const SampleDraw d = sample_draw(seed, first + i);
                const unsigned int t = sample_pick(C.data(), n_tris, sample_mulhi64(d.r0, total));
                const float4 r0 = tris[(size_t)t * 3], r1 = tris[(size_t)t * 3 + 1], r2 = tris[(size_t)t * 3 + 2];
                const f3 a = mk3(r0.x, r0.y, r0.z), ab = mk3(r0.w, r1.x, r1.y), ac = mk3(r1.z, r1.w, r2.x);
                const f3 p = sample_point(a, ab, ac, d.v, d.w), b = sample_bw(d.v, d.w), nr = sample_normal(ab, ac);
                point[3 * i] = p.x; point[3 * i + 1] = p.y; point[3 * i + 2] = p.z;
                bw[3 * i] = b.x; bw[3 * i + 1] = b.y; bw[3 * i + 2] = b.z;
                normal[3 * i] = nr.x; normal[3 * i + 1] = nr.y; normal[3 * i + 2] = nr.z;
                group[i] = (int)leaf_map[t].x;
                vertex0[i] = leaf_map[t].y;
            }
            wr(fout, point); wr(fout, bw); wr(fout, normal); wr(fout, vertex0); wr(fout, group);
        }

        for (uint32_t gi = 0; gi < n_grads; ++gi) {
            const std::vector<uint32_t> gh = rd<uint32_t>(fin, 2);
            const uint32_t n = gh[0], flags = gh[1];
            const std::vector<int> group = rd<int>(fin, n);
            const std::vector<unsigned int> vertex0 = rd<unsigned int>(fin, n);
            const std::vector<float> bw = rd<float>(fin, 3 * (size_t)n);
            const std::vector<float> g_point = rd<float>(fin, flags & 1u ? 3 * (size_t)n : 0), g_normal = rd<float>(fin, flags & 2u ? 3 * (size_t)n : 0);
            const bool merge = (flags & 16u) != 0;
            std::vector<float> gp(3 * (size_t)n_pos, 7.5f);
            std::vector<long long> acc(3 * (size_t)n_pos + 1, 0);
            unsigned int words[QGRAD_WORDS] = { 0u, 0u, 0u, 0u };
            SGradArgs A;
            memset(&A, 0, sizeof(A));
            A.group = group.data(); A.vertex0 = vertex0.data(); A.bw = bw.data(); A.positions = pos.data();
            A.g_point = flags & 1u ? g_point.data() : nullptr; A.g_normal = flags & 2u ? g_normal.data() : nullptr;
            A.idx_positions = idx.data(); A.group_runs = runs.data(); A.words = words;
            A.count = n; A.group_count = n_groups; A.position_count = n_pos;
            int rc = 0;
            float m = 0.0f;
            if (n == 0) {
                std::fill(gp.begin(), gp.end(), 0.0f);
            } else {
                launch(k_sgrad_scan, n / 3 + 2, A);                   // fewer blocks than samples: the grid-stride loop runs
                memcpy(&m, &words[QGRAD_W_MAX], 4);
                if (words[QGRAD_W_INVALID]) rc = -1;
            }
            if (n && rc == 0) {
                const bool adds = words[QGRAD_W_HIT] && m > 0.0f;
                A.unit_exponent = m > 0.0f ? qgrad_unit_exponent(m, n) : 0;
                A.acc = adds && !merge ? acc.data() : nullptr;
                if (adds && !merge) launch(k_sgrad_scatter<false>, n / 5 + 3, A);
                if (adds && merge) {
                    for (unsigned int base = 0; base < n; base += 64u) {
                        unsigned int key[64], vi[64][3];
                        long long q[64][9];
                        bool lv[64];
                        const unsigned int lanes = n - base < 64u ? n - base : 64u;
                        for (unsigned int l = 0; l < lanes; ++l) {
                            SGradOut g;
                            bool ok = false;
                            lv[l] = sgrad_sample(A, base + l, &key[l], vi[l], &ok, &g) == QGRAD_HIT && ok;
                            if (lv[l]) sgrad_fixed9(g, A.unit_exponent, q[l]);
                        }
                        for (unsigned int l = 0; l < lanes; ++l) {
                            if (!lv[l]) continue;
                            long long s[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };
                            for (unsigned int k = l; k < lanes; ++k)
                                if (lv[k] && key[k] == key[l]) { for (int c = 0; c < 9; ++c) s[c] += q[k][c]; if (k != l) lv[k] = false; }
                            for (int c = 0; c < 3; ++c) for (int k = 0; k < 3; ++k) acc[3 * (size_t)vi[l][c] + k] += s[3 * c + k];
                        }
                    }
                }
                if (adds) {
                    QGradArgs R;                                      // as grad_resolve fills it
                    memset(&R, 0, sizeof(R));
                    R.g_positions = gp.data(); R.acc = acc.data(); R.position_count = n_pos; R.unit_exponent = A.unit_exponent;
                    launch(k_qgrad_resolve, 3 * n_pos + 2, R);
                } else {
                    std::fill(gp.begin(), gp.end(), 0.0f);
                }
            }
            const int u = rc == 0 ? A.unit_exponent : 0;
            wr(fout, &rc, 1); wr(fout, &words[QGRAD_W_HIT], 1); wr(fout, &words[QGRAD_W_SKIPPED], 1); wr(fout, &words[QGRAD_W_INVALID], 1);
            wr(fout, &u, 1); wr(fout, &m, 1); wr(fout, gp);
        }
        printf("case %u: %u triangles, %u live, total %llu, unit 2^%d, %u requests, %u gradient calls\n", ci, n_tris, live, total, unit, n_requests,
               n_grads);
    }
    fclose(fin);
    return fclose(fout) ? 2 : 0;
}
