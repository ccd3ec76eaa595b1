// normal_cones_host_harness.cpp - the normal cones of the 4-wide tree (par_raytracer_amd/csrc/bvh_build.h attach_normal_cones,
// dev_scene.h cone_faces_away) on the host: the builder's and the checker's functions as the upload calls them and the device
// traversal (dev_trace4.h through tests/hip_shim, one lane at a time).  One line per fact; tests/test_normal_cones_host.py asserts.
//   cones      per scene and front end (the SAH build, and the radix tree of tests/lbvh_cases.py through the LBVH back end): coned
//              nodes, the checker's violations before and after one triangle below a coned node is flipped, the bytes under 1, 2
//              and 8 threads, and the mantissas of a coned node after refit_node
//   soundness  per coned node at least 32 directions ON and just inside the cull boundary (bisection on the shared predicate,
//              lengths 1 and 1 + 2^-20), and the direction perpendicular to the widest normal; every direction the predicate accepts
//              is put through the device's own dd = Dot(o - (o + d), n) for EVERY triangle below the node, origins at 0 and at the
//              corners of the origin_max box
//   rays       primary, bounce and shadow rays (axis-parallel ones and ones with a component below 1e-30 among them) walked by
//              trav_node_step / trav_leaf with the cones attached and with the bits cleared: HitRec and the marker's flags bit for
//              bit; culls and triangle tests per class; the same rays with TRACE_NO_CONE and as any-hit rays cull nothing
//   bits       zero words, a NaN direction and a direction of length 0 never cull
// Case file (little endian): u32 cases; per case name[32], u32 n, f32 sun[3], f32 verts[9 n], u32 has_radix, then - if set - the
// arrays of tests/lbvh_backend_harness.cpp: left, right (ni i32), first, last (ni u32), node_box (6 ni f32), leaf_box (6 n f32),
// sorted_ids (n u32), ni = max(n - 1, 1).  A vertex that is not finite is replaced by 0 for the tree alone: the records keep it.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "harness_io.h"
#include "harness_mesh.h"
#include "harness_scene.h"
#include "dev_refit.h"

using namespace prt;

static std::vector<float> stored_normals(const std::vector<float> & verts) {
    std::vector<float> n(verts.size() / 3);
    for (size_t t = 0; t < verts.size() / 9; ++t) {
        float4 rec[3];
        const float * v = &verts[t * 9];
        tri_record(mk3(v[0], v[1], v[2]), mk3(v[3], v[4], v[5]), mk3(v[6], v[7], v[8]), rec);
        n[t * 3] = rec[2].y; n[t * 3 + 1] = rec[2].z; n[t * 3 + 2] = rec[2].w;
    }
    return n;
}

static bool has_cone(const uint32_t * d) { return ((d[3] | d[14] | d[15]) & 0x007FFFFFu) != 0u; }
static bool accepts(const uint32_t * d, f3 dir) { return cone_faces_away(d[3], d[14], d[15], dir); }

// The leaf-order slots below node ni.
static void slots_below(const BvhWide & bvh, uint32_t ni, uint32_t n_tris, std::vector<uint32_t> & out) {
    std::vector<uint32_t> stack(1, ni);
    while (!stack.empty()) {
        const uint32_t * d = &bvh.nodes[(size_t)stack.back() * 16];
        stack.pop_back();
        for (int k = 0; k < 4; ++k) {
            const int32_t link = (int32_t)d[10 + k];
            if (link >= 0) { stack.push_back((uint32_t)link); continue; }
            const uint32_t first = (uint32_t)~link >> 2, count = ((uint32_t)~link & 3u) + 1u;
            for (uint32_t i = 0; i < count && first + i < n_tris; ++i) out.push_back(first + i);
        }
    }
}

static f3 unit_rnd() {
    for (;;) {
        const f3 v = mk3((float)(rnd() * 2 - 1), (float)(rnd() * 2 - 1), (float)(rnd() * 2 - 1));
        const float l = dot3(v, v);
        if (l > 1e-4f && l <= 1.0f) return normalize3(v);
    }
}

struct Sound { unsigned long long nodes = 0, directions = 0, accepted = 0, perpendicular = 0, towards_perpendicular = 0, tests = 0, violations = 0; };

static void soundness(const BvhWide & bvh, const std::vector<float> & normals, uint32_t n_tris, float M, Sound & S) {
    std::vector<uint32_t> below;
    for (uint32_t ni = 0; ni < bvh.node_count; ++ni) {
        const uint32_t * d = &bvh.nodes[(size_t)ni * 16];
        if (!has_cone(d)) continue;
        S.nodes++;
        below.clear();
        slots_below(bvh, ni, n_tris, below);
        const f3 a = normalize3(mk3((float)cone_component(d[3]), (float)cone_component(d[14]), (float)cone_component(d[15])));
        std::vector<f3> dirs;
        for (int k = 0; k < 16; ++k) {
            // the boundary in the plane of a and a random e across it: the largest angle from a that the predicate still accepts
            f3 e = cross3(a, unit_rnd());
            if (dot3(e, e) < 1e-6f) continue;
            e = normalize3(e);
            const float len = k & 1 ? 1.0f + 9.5367431640625e-7f : 1.0f;
            auto at = [&](double th) { return (a * (float)cos(th) + e * (float)sin(th)) * len; };
            double lo = 0.0, hi = 1.5707963267948966;
            if (!accepts(d, at(lo))) continue;                    // (a cone so wide that not even its axis is accepted)
            for (int it = 0; it < 40; ++it) { const double mid = 0.5 * (lo + hi); if (accepts(d, at(mid))) lo = mid; else hi = mid; }
            dirs.push_back(at(lo));                               // on the boundary: the last accepted
            dirs.push_back(at(lo * (1.0 - 1e-6)));                // just inside
            dirs.push_back(at(hi));                               // the first refused (counted, not tested, unless a float quirk accepts it)
        }
        // the direction perpendicular to the widest normal, in the plane of that normal and the axis
        double widest = 2.0; f3 nw = a;
        for (uint32_t s : below) {
            const float * n = &normals[(size_t)bvh.tri_order[s] * 3];
            const f3 nv = mk3(n[0], n[1], n[2]);
            if (dot3(nv, nv) == 0.0f) continue;
            const f3 nu = normalize3(nv);
            if (dot3(a, nu) < widest) { widest = dot3(a, nu); nw = nu; }
        }
        const f3 perp = a - nw * dot3(a, nw);
        if (dot3(perp, perp) > 1e-12f) {
            const f3 pu = normalize3(perp);
            dirs.push_back(pu);
            S.perpendicular++;
            // ... and, since the margin keeps the predicate from accepting it, the accepted direction nearest to it: the boundary on the
            // way from the axis to it, the side on which the widest normal decides
            const f3 ev = normalize3(pu - a * dot3(a, pu));       // across the axis, in the plane of the axis and the widest normal, away from that normal
            auto towards = [&](double th) { return normalize3(a * (float)cos(th) + ev * (float)sin(th)); };
            double lo = 0.0, hi = 1.5707963267948966;
            if (accepts(d, towards(lo)) && !accepts(d, towards(hi))) {
                for (int it = 0; it < 40; ++it) { const double mid = 0.5 * (lo + hi); if (accepts(d, towards(mid))) lo = mid; else hi = mid; }
                dirs.push_back(towards(lo));
                S.towards_perpendicular++;
            }
        }
        for (const f3 & dir : dirs) {
            S.directions++;
            if (!accepts(d, dir)) continue;
            S.accepted++;
            for (uint32_t s : below) {
                const float * n = &normals[(size_t)bvh.tri_order[s] * 3];
                const f3 nv = mk3(n[0], n[1], n[2]);
                for (int c = 0; c < 9; ++c) {
                    const f3 o = c == 8 ? mk3(0, 0, 0) : mk3(c & 1 ? M : -M, c & 2 ? M : -M, c & 4 ? M : -M);
                    const f3 qp = o - (o + dir);                  // raytracer.cpp:88-89, dev_trace4.h trav_leaf
                    S.tests++;
                    if (dot3(qp, nv) > 0.0f) S.violations++;      // tri_test's own expression: dd <= 0 leaves
                }
            }
        }
    }
}

struct Ray { f3 o, d; int cls; };                                  // cls 0 primary, 1 bounce, 2 shadow
struct WalkOut { HitRec h; int flags; unsigned int nodes, tris, culls; };

template <bool CONES>
static WalkOut walk(mesh::Walk & lane, const Ray & ray, int kind, float pad) {
    TraceStats st;
    TravRay r;
    trav_init(r, ray.o, ray.d, kind, pad, lane.stk);
    bool found = false;
    for (;;) {
        while (trav_walking(r)) trav_node_step<GlobalStack, true, CONES>(lane.sc, r, lane.stk, st, pad);
        if (trav_done(r)) break;
        if (trav_leaf<GlobalStack, true>(lane.sc, r, lane.stk, st)) { found = true; break; }
    }
    WalkOut w;
    w.h = r.best;
    w.flags = found ? 0 : trav_end_flags(r, lane.stk);
    w.nodes = st.nodes; w.tris = st.tris; w.culls = st.cone_culls;
    return w;
}

static std::vector<Ray> make_rays(const std::vector<float> & verts, f3 sun, int per_class) {
    const uint32_t n = (uint32_t)(verts.size() / 9);
    f3 lo = mk3(1e30f, 1e30f, 1e30f), hi = lo * -1.0f;
    for (size_t i = 0; i < verts.size(); i += 3) {
        if (!(fabsf(verts[i]) < 1e18f && fabsf(verts[i + 1]) < 1e18f && fabsf(verts[i + 2]) < 1e18f)) continue;
        lo = mk3(fminf(lo.x, verts[i]), fminf(lo.y, verts[i + 1]), fminf(lo.z, verts[i + 2]));
        hi = mk3(fmaxf(hi.x, verts[i]), fmaxf(hi.y, verts[i + 1]), fmaxf(hi.z, verts[i + 2]));
    }
    const f3 mid = (lo + hi) * 0.5f, ext = hi - lo;
    const float size = fmaxf(fmaxf(ext.x, ext.y), fmaxf(ext.z, 1e-3f));
    auto surface = [&](f3 & gn) {
        for (;;) {
            const float * t = &verts[(size_t)(uint32_t)(rnd() * n) * 9];
            const f3 a = mk3(t[0], t[1], t[2]), b = mk3(t[3], t[4], t[5]), c = mk3(t[6], t[7], t[8]);
            const f3 nv = cross3(b - a, c - a);
            if (!(dot3(nv, nv) > 0.0f && dot3(nv, nv) < 1e30f)) continue;
            const float u = (float)rnd(), v = (float)rnd() * (1.0f - u);
            gn = normalize3(nv);
            return a + (b - a) * u + (c - a) * v;
        }
    };
    const f3 axes[6] = { mk3(1, 0, 0), mk3(-1, 0, 0), mk3(0, 1, 0), mk3(0, -1, 0), mk3(0, 0, 1), mk3(0, 0, -1) };
    std::vector<Ray> rays;
    for (int k = 0; k < per_class; ++k) {
        f3 gn;
        const f3 p = surface(gn);
        Ray r;
        // primary: from a camera above and beside the scene towards a point of the surface
        r.cls = 0;
        r.o = mid + mk3((float)(rnd() - 0.5), 0.8f + (float)rnd() * 0.4f, (float)(rnd() - 0.5)) * (1.5f * size);
        r.d = normalize3(p - r.o);
        if (k % 16 == 5) { r.d = axes[k / 16 % 6]; r.o = p - r.d * size; }                   // axis-parallel, through a surface point
        if (k % 16 == 9) { r.d = normalize3(mk3(r.d.x, r.d.y, 1e-35f)); }                    // a component below 1e-30
        rays.push_back(r);
        // bounce: leaves the surface on its front side, cosine-ish
        r.cls = 1;
        r.o = p + gn * 1e-3f;
        f3 dir = gn + unit_rnd() * 0.98f;
        r.d = normalize3(dir);
        if (k % 16 == 5) r.d = axes[k / 16 % 6];
        if (k % 16 == 9) r.d = normalize3(mk3(1e-38f, r.d.y, r.d.z));
        rays.push_back(r);
        // shadow: towards the light, as a point light's closest-hit shadow ray (a directional light's is an any-hit ray: exempt)
        r.cls = 2;
        r.o = p + gn * 1e-3f;
        r.d = normalize3(sun + unit_rnd() * (k % 4 == 0 ? 0.3f : 0.0f));
        rays.push_back(r);
    }
    return rays;
}

int main(int argc, char ** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
    harness_name = "normal_cones_host_harness";
    FILE * f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    const uint32_t n_cases = rd<uint32_t>(f, 1)[0];
    for (uint32_t c = 0; c < n_cases; ++c) {
        const std::vector<char> raw = rd<char>(f, 32);
        const std::string name(raw.data());
        const uint32_t n = rd<uint32_t>(f, 1)[0];
        const std::vector<float> sun3 = rd<float>(f, 3), verts = rd<float>(f, (size_t)n * 9);
        const uint32_t has_radix = rd<uint32_t>(f, 1)[0];
        const size_t ni = n > 1 ? n - 1 : 1;
        std::vector<int32_t> left, right;
        std::vector<uint32_t> first, last, sorted_ids;
        std::vector<float> node_box, leaf_box;
        if (has_radix) {
            left = rd<int32_t>(f, ni); right = rd<int32_t>(f, ni); first = rd<uint32_t>(f, ni); last = rd<uint32_t>(f, ni);
            node_box = rd<float>(f, ni * 6); leaf_box = rd<float>(f, (size_t)n * 6); sorted_ids = rd<uint32_t>(f, n);
        }
        std::vector<float> clean = verts;
        float abs_max = 0.0f;
        for (float & x : clean) { if (!(fabsf(x) < 1e18f)) x = 0.0f; abs_max = fmaxf(abs_max, fabsf(x)); }
        const double M = 32.0 * (double)abs_max;
        const std::vector<float> normals = stored_normals(verts);
        const std::vector<float4> rec_in = mesh::records(verts, n, nullptr);
        for (int front = 0; front < (has_radix ? 2 : 1); ++front) {
            const char * fe = front ? "radix" : "sah";
            BvhWide plain;
            if (front) build_bvh_wide_from_radix_tree(4, n, 4, left.data(), right.data(), first.data(), last.data(), node_box.data(), leaf_box.data(), sorted_ids.data(), &plain);
            else build_bvh_wide(4, clean.data(), n, 4, 2, &plain);
            if (validate_bvh_links(plain, n)) { printf("cones %s %s | broken tree\n", name.c_str(), fe); continue; }
            BvhWide t1 = plain, t2 = plain, t8 = plain;
            const uint32_t coned = attach_normal_cones(t1, normals.data(), n, M, 1);
            attach_normal_cones(t2, normals.data(), n, M, 2);
            attach_normal_cones(t8, normals.data(), n, M, 8);
            const bool same = t1.nodes == t2.nodes && t1.nodes == t8.nodes;
            // outside the mantissas the tree is the builder's
            bool rest_same = true;
            for (size_t i = 0; i < plain.nodes.size(); ++i) {
                const size_t w = i % 16;
                const uint32_t mask = (w == 3 || w == 14 || w == 15) ? 0xFF800000u : 0xFFFFFFFFu;
                rest_same = rest_same && (plain.nodes[i] & mask) == (t1.nodes[i] & mask);
            }
            uint64_t coned_seen = 0, out6[6];
            const uint64_t viol = check_bvh_cones(clean.data(), n, t1, M, &coned_seen);
            check_bvh_wide(clean.data(), n, t1, out6);
            // flip one triangle below a coned node: its record normal turns round
            uint64_t viol_flipped = 0;
            int refit_cleared = -1;
            for (uint32_t nd = 0; nd < t1.node_count; ++nd) {
                uint32_t * d = &t1.nodes[(size_t)nd * 16];
                if (!has_cone(d)) continue;
                std::vector<uint32_t> below;
                slots_below(t1, nd, n, below);
                uint32_t pick = 0xFFFFFFFFu;
                for (uint32_t s : below) { const float * nn = &normals[(size_t)t1.tri_order[s] * 3]; if (nn[0] != 0.0f || nn[1] != 0.0f || nn[2] != 0.0f) { pick = t1.tri_order[s]; break; } }
                if (pick == 0xFFFFFFFFu) continue;
                std::vector<float> flipped = clean;
                for (int k = 0; k < 3; ++k) std::swap(flipped[(size_t)pick * 9 + 3 + k], flipped[(size_t)pick * 9 + 6 + k]);
                viol_flipped = check_bvh_cones(flipped.data(), n, t1, M, nullptr);
                // refit_node on a copy of the node: any boxes will do
                uint32_t copy[16];
                memcpy(copy, d, 64);
                RefitSlot slot[4];
                refit_slots<4>(copy, slot);
                RefitBox child[4], own;
                for (int k = 0; k < 4; ++k) for (int a = 0; a < 3; ++a) { child[k].lo[a] = (float)k; child[k].hi[a] = (float)k + 1.5f; }
                refit_node<4>(copy, slot, child, &own);
                refit_cleared = ((copy[3] | copy[14] | copy[15]) & 0x007FFFFFu) == 0u ? 1 : 0;
                break;
            }
            printf("cones %s %s | tris %u nodes %u coned %u coned_seen %llu violations %llu flipped_violations %llu threads_same %d rest_same %d box_violations %llu refit_cleared %d\n",
                   name.c_str(), fe, n, t1.node_count, coned, (unsigned long long)coned_seen, (unsigned long long)viol, (unsigned long long)viol_flipped,
                   (int)same, (int)rest_same, (unsigned long long)out6[0], refit_cleared);

            Sound S;
            soundness(t1, normals, n, (float)M, S);
            printf("soundness %s %s | nodes %llu directions %llu accepted %llu perpendicular %llu towards_perpendicular %llu dd_tests %llu violations %llu\n", name.c_str(), fe,
                   S.nodes, S.directions, S.accepted, S.perpendicular, S.towards_perpendicular, S.tests, S.violations);

            // ---- bits: zero words, NaN and zero directions
            unsigned long long zero_culls = 0, nan_culls = 0, null_culls = 0;
            const float nanv = nanf("");
            for (uint32_t nd = 0; nd < t1.node_count; ++nd) {
                const uint32_t * d = &t1.nodes[(size_t)nd * 16], * p = &plain.nodes[(size_t)nd * 16];
                for (int k = 0; k < 8; ++k) {
                    const f3 dir = unit_rnd() * (k == 7 ? 1e30f : 1.0f);
                    zero_culls += accepts(p, dir);
                    nan_culls += accepts(d, mk3(k & 1 ? nanv : dir.x, k & 2 ? nanv : dir.y, (k & 3) == 0 || (k & 4) ? nanv : dir.z));
                }
                null_culls += accepts(d, mk3(0.0f, 0.0f, 0.0f)) + accepts(d, mk3(-0.0f, 0.0f, -0.0f));
            }
            printf("bits %s %s | zero_word_culls %llu nan_culls %llu zero_length_culls %llu\n", name.c_str(), fe, zero_culls, nan_culls, null_culls);

            // ---- rays
            std::vector<float4> rec((size_t)(n + 1) * 3, make_float4(0, 0, 0, 0));
            for (uint32_t s = 0; s < n; ++s) memcpy(&rec[(size_t)s * 3], &rec_in[(size_t)t1.tri_order[s] * 3], 48);
            mesh::Walk with(t1, rec, n), without(plain, rec, n);
            const float pad = abs_max * (1.0f / 65536.0f);
            g_rng = 0x9E3779B97F4A7C15ull + c;
            const std::vector<Ray> rays = make_rays(verts, normalize3(mk3(sun3[0], sun3[1], sun3[2])), 7000);
            unsigned long long mism = 0, culls[3] = { 0, 0, 0 }, tris_on[3] = { 0, 0, 0 }, tris_off[3] = { 0, 0, 0 }, nodes_on[3] = { 0, 0, 0 }, nodes_off[3] = { 0, 0, 0 };
            unsigned long long hits = 0, nocone_culls = 0, nocone_tri_diff = 0, any_culls = 0, any_mism = 0, tiny = 0, axis_par = 0;
            for (const Ray & r : rays) {
                const WalkOut a = walk<true>(with, r, TRACE_CLOSEST, pad), b = walk<true>(without, r, TRACE_CLOSEST, pad);
                if (memcmp(&a.h, &b.h, sizeof(HitRec)) || a.flags != b.flags) mism++;
                hits += a.h.tri >= 0;
                culls[r.cls] += a.culls; tris_on[r.cls] += a.tris; tris_off[r.cls] += b.tris; nodes_on[r.cls] += a.nodes; nodes_off[r.cls] += b.nodes;
                const WalkOut nc = walk<true>(with, r, TRACE_CLOSEST | TRACE_NO_CONE, pad);
                nocone_culls += nc.culls; nocone_tri_diff += nc.tris != b.tris || nc.nodes != b.nodes || memcmp(&nc.h, &b.h, sizeof(HitRec)) != 0;
                const WalkOut an = walk<true>(with, r, TRACE_ANY, pad), bn = walk<true>(without, r, TRACE_ANY, pad);
                any_culls += an.culls; any_mism += memcmp(&an.h, &bn.h, sizeof(HitRec)) != 0 || an.nodes != bn.nodes;
                tiny += fabsf(r.d.x) < 1e-30f || fabsf(r.d.y) < 1e-30f || fabsf(r.d.z) < 1e-30f;
                axis_par += (r.d.x == 0.0f) + (r.d.y == 0.0f) + (r.d.z == 0.0f) == 2;
            }
            printf("rays %s %s | rays %zu hits %llu mismatches %llu tiny_component %llu axis_parallel %llu culls_primary %llu culls_bounce %llu culls_shadow %llu "
                   "tris_primary %llu -> %llu tris_bounce %llu -> %llu tris_shadow %llu -> %llu nodes_bounce %llu -> %llu nocone_culls %llu nocone_differs %llu any_culls %llu any_differs %llu\n",
                   name.c_str(), fe, rays.size(), hits, mism, tiny, axis_par, culls[0], culls[1], culls[2], tris_off[0], tris_on[0], tris_off[1], tris_on[1],
                   tris_off[2], tris_on[2], nodes_off[1], nodes_on[1], nocone_culls, nocone_tri_diff, any_culls, any_mism);
            fflush(stdout);
        }
    }
    fclose(f);
    return 0;
}
