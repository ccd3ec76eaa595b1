// signed_host_harness.cpp - the definition of prt_signed_distance (par_raytracer_amd/csrc/dev_signed.h, include/prt.h), compiled for
// the host with tests/hip_shim: a brute force over every triangle.  The records are laid out as prt_upload_scene lays them out
// (a, b - a, c - a), in input order - the answer does not depend on the tree, so none is built; the adjacency (position indices and
// edge ids per triangle) comes from the index buffer, the accumulators are filled with the PRT_HD functions of dev_signed.h and
// plain 64-bit integer adds, every point's winner is found with closest_on_triangle and the tie rule (closest_takes) and signed
// with signed_of_winner.  tests/signed_cases.py writes the cases and reads the results; tests/test_signed_host.py asserts on them,
// tests/test_gpu_signed.py compares the device with them bit for bit.
//
//   g++ -O1 -std=c++17 -ffp-contract=off -Itests/hip_shim -Ipar_raytracer_amd/csrc tests/signed_host_harness.cpp -o /tmp/signed_host
//       && /tmp/signed_host cases.bin results.bin
//
// cases.bin: u32 case count, then per case 5 x u32 (points, positions, indices, groups, flags), the points (x3 f32), with flag 1
// max_dist2 (f32 per point), then positions (x3 f32), idx_positions (u32), the groups' (first_index, index_count) (2 x u32).
// With flag 2 the case is a sweep of signed_acos: the 3 x points floats are its arguments, nothing else is read or computed.
// results.bin, per case: dist2, point (x3), bw (x3), vertex0, group, signed_dist (f32), feature (u8) per point, then per input
// triangle its three angles (f32; NaN x3 for a triangle that contributes nothing).  A sweep: 3 x points f32.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>
#include <vector>

#include <hip/hip_runtime.h>            // tests/hip_shim: one lane at a time
using std::isfinite;

#include "dev_signed.h"
#include "harness_io.h"
#include "harness_mesh.h"

using namespace prt;

int main(int argc, char ** argv) {
    FILE * fin, * fout;
    if (!open_in_out(argc, argv, "signed_host", &fin, &fout)) return 2;
    const uint32_t n_cases = rd<uint32_t>(fin, 1)[0];
    for (uint32_t ci = 0; ci < n_cases; ++ci) {
        const std::vector<uint32_t> hd = rd<uint32_t>(fin, 5);
        const uint32_t n = hd[0], n_pos = hd[1], n_idx = hd[2], n_groups = hd[3], flags = hd[4], n_tris = n_idx / 3;
        const std::vector<float> pts = rd<float>(fin, 3 * (size_t)n);
        if (flags & 2u) {                                     // signed_acos alone
            std::vector<float> out(pts.size());
            for (size_t i = 0; i < pts.size(); ++i) out[i] = signed_acos(pts[i]);
            wr(fout, out);
            continue;
        }
        const std::vector<float> radius2 = rd<float>(fin, (flags & 1u) ? n : 0);
        const std::vector<float> pos = rd<float>(fin, 3 * (size_t)n_pos);
        const std::vector<uint32_t> idx = rd<uint32_t>(fin, n_idx);
        const std::vector<uint32_t> runs = rd<uint32_t>(fin, 2 * (size_t)n_groups);

        // the records (slot = input triangle), the leaf table, the adjacency
        const std::vector<float4> tris = mesh::records(mesh::unindexed(pos, idx), n_tris, nullptr);
        const std::vector<uint2> leaf_map = mesh::leaf_map(runs, n_groups, n_tris, nullptr);
        std::map<std::pair<uint32_t, uint32_t>, uint32_t> edge_id;
        std::vector<unsigned int> adj(6 * (size_t)n_tris);
        for (uint32_t t = 0; t < n_tris; ++t) {
            const uint32_t * vi = &idx[3 * (size_t)t];
            const uint32_t pair[3][2] = { { vi[0], vi[1] }, { vi[0], vi[2] }, { vi[1], vi[2] } };          // ab, ac, bc
            for (int k = 0; k < 3; ++k) {
                adj[6 * (size_t)t + k] = vi[k];
                const std::pair<uint32_t, uint32_t> key(std::min(pair[k][0], pair[k][1]), std::max(pair[k][0], pair[k][1]));
                adj[6 * (size_t)t + 3 + k] = edge_id.emplace(key, (uint32_t)edge_id.size()).first->second;
            }
        }
        // the accumulators: what k_signed_normals adds, in input order
        std::vector<long long> acc(3 * ((size_t)n_pos + edge_id.size()), 0);
        std::vector<float> angles(3 * (size_t)n_tris, NAN);
        for (uint32_t t = 0; t < n_tris; ++t) {
            const float4 r0 = tris[(size_t)t * 3], r1 = tris[(size_t)t * 3 + 1], r2 = tris[(size_t)t * 3 + 2];
            f3 nrm;
            float alpha[3];
            if (!signed_triangle_terms(mk3(r0.w, r1.x, r1.y), mk3(r1.z, r1.w, r2.x), nrm, alpha)) continue;
            long long vq[9], eq[3];
            signed_triangle_fixed(nrm, alpha, vq, eq);
            for (int k = 0; k < 3; ++k) {
                angles[3 * (size_t)t + k] = alpha[k];
                for (int c = 0; c < 3; ++c) {
                    acc[3 * (size_t)adj[6 * (size_t)t + k] + c] += vq[3 * k + c];
                    acc[3 * ((size_t)n_pos + adj[6 * (size_t)t + 3 + k]) + c] += eq[c];
                }
            }
        }
        SignedTables T;
        T.adj = adj.data(); T.acc = acc.data(); T.position_count = n_pos; T.edge_count = (unsigned int)edge_id.size();

        std::vector<float> dist2(n), point(3 * (size_t)n), bw(3 * (size_t)n), sd(n);
        std::vector<unsigned int> vertex0(n);
        std::vector<int> group(n);
        std::vector<unsigned char> feature(n);
        for (uint32_t i = 0; i < n; ++i) {
            const f3 p = mk3(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]);
            const float max_d2 = (flags & 1u) ? radius2[i] : 3.402823466e+38f;
            HitRec b;
            b.t = max_d2; b.v = b.w = 0.0f; b.tri = -1;
            if (isfinite(p.x) && isfinite(p.y) && isfinite(p.z) && max_d2 >= 0.0f)
                for (uint32_t slot = 0; slot < n_tris; ++slot) {
                    const float4 r0 = tris[(size_t)slot * 3], r1 = tris[(size_t)slot * 3 + 1], r2 = tris[(size_t)slot * 3 + 2];
                    float d2, v, w;
                    if (closest_on_triangle(p, mk3(r0.x, r0.y, r0.z), mk3(r0.w, r1.x, r1.y), mk3(r1.z, r1.w, r2.x), d2, v, w) &&
                        closest_takes(d2, slot, b, leaf_map.data())) { b.t = d2; b.v = v; b.w = w; b.tri = (int)slot; }
                }
            // closest_emit of kernels_closest.h, field for field
            const bool hit = b.tri >= 0;
            dist2[i] = hit ? b.t : 3.402823466e+38f;
            f3 q = mk3(0.0f, 0.0f, 0.0f);
            sd[i] = 3.402823466e+38f;
            unsigned int feat = 255u;
            if (hit) {
                const float4 r0 = tris[(size_t)b.tri * 3], r1 = tris[(size_t)b.tri * 3 + 1], r2 = tris[(size_t)b.tri * 3 + 2];
                const f3 a = mk3(r0.x, r0.y, r0.z), ab = mk3(r0.w, r1.x, r1.y), ac = mk3(r1.z, r1.w, r2.x);
                q = closest_point_of(a, ab, ac, b.v, b.w);
                sd[i] = signed_of_winner(T, (unsigned int)b.tri, p, a, ab, ac, b.t, feat);
            }
            feature[i] = (unsigned char)feat;
            point[3 * i] = q.x; point[3 * i + 1] = q.y; point[3 * i + 2] = q.z;
            bw[3 * i] = hit ? 1.0f - b.v - b.w : 0.0f; bw[3 * i + 1] = hit ? b.v : 0.0f; bw[3 * i + 2] = hit ? b.w : 0.0f;
            const uint2 m = hit ? leaf_map[(size_t)b.tri] : make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
            group[i] = (int)m.x;
            vertex0[i] = m.y;
        }
        wr(fout, dist2); wr(fout, point); wr(fout, bw); wr(fout, vertex0); wr(fout, group); wr(fout, sd); wr(fout, feature); wr(fout, angles);
        printf("case %u: %u triangles, %u positions, %zu edges, %u points\n", ci, n_tris, n_pos, edge_id.size(), n);
    }
    fclose(fin);
    return fclose(fout) ? 2 : 0;
}
