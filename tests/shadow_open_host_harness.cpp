// shadow_open_host_harness.cpp - the open triangles of a directional light (par_raytracer_amd/csrc/bvh_build.h) on the host: the
// classification prt_upload_scene runs (pack_scene of scene_pack.cpp, the very function it calls, read back out of the packed
// records) on the scenes of a case file, and a brute-force check of what the flags promise.  It prints one line per fact and
// tests/test_shadow_open_host.py asserts on them:
//   flags    triangles, occluders, triangles facing the light, open ones, a hash of the flags (equal for both tree widths: the
//            classification never sees a tree), the bounds
//   brute    for EVERY open triangle: origins at its corners, edge midpoints and centroid and 4 ulp (of the scene's largest
//            coordinate) outside each edge's midpoint and each corner, pushed as the renderer pushes a hit (pos + gn bias, then
//            + d bias: kernels_wave.h shade_entry_on, dev_trace.h) with bias = +bound, -bound, 0 and 1e-3, each tested against
//            ALL the scene's triangle records with the reference's triangle test (dev_trace_common.h tri_test_ref): hits
//   sanity   open triangles among the occluders (each overlaps itself); open triangles among those that share all three corners
//            with an occluder (a face exported twice, or once more flipped)
//   margin   triangles and bounds outside what the margin's argument covers: unflagged
//
// Case file: u32 scenes; per scene a 32-byte name, u32 n_tris, 3 floats d (towards the light, as the kernels form it: facing
// * -1), 9 n_tris floats.
#include <algorithm>
#include <cfloat>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "harness_mesh.h"
#include "harness_desc.h"
#include "harness_io.h"

using namespace prt;

#if defined(PRT_BVH8)
enum { WIDTH = 8 };
#else
enum { WIDTH = 4 };
#endif

static std::vector<float> stored_normals(const std::vector<float> & verts) {
    std::vector<float> n(verts.size() / 3);
    std::vector<float4> rec(3);
    for (size_t t = 0; t < verts.size() / 9; ++t) {
        const float * v = &verts[t * 9];
        tri_record(mk3(v[0], v[1], v[2]), mk3(v[3], v[4], v[5]), mk3(v[6], v[7], v[8]), rec.data());
        n[t * 3] = rec[2].y; n[t * 3 + 1] = rec[2].z; n[t * 3 + 2] = rec[2].w;
    }
    return n;
}

// Does a shadow ray from `pos` (a point the renderer took for a hit on a triangle of unit normal gn) hit any record?
static bool occluded(const std::vector<float4> & recs, uint32_t n_tris, f3 pos, f3 gn, f3 d, float bias) {
    const f3 hit_p = pos + gn * bias;                        // raytracer.cpp:425
    const f3 ob = hit_p + d * bias;                          // raytracer.cpp:163
    const f3 qp = ob - (ob + d);
    for (uint32_t s = 0; s < n_tris; ++s) {
        const float4 r0 = recs[3 * (size_t)s], r1 = recs[3 * (size_t)s + 1], r2 = recs[3 * (size_t)s + 2];
        float t, v, w;
        if (tri_test_ref(ob, qp, mk3(r0.x, r0.y, r0.z), mk3(r0.w, r1.x, r1.y), mk3(r1.z, r1.w, r2.x), mk3(r2.y, r2.z, r2.w), FLT_MAX, t, v, w)) return true;
    }
    return false;
}

// What prt_upload_scene makes of the triangles under one directional light along d: its host half itself (scene_pack.cpp through
// tests/harness_desc.h pack_as_upload), read back in input order - the flags out of the shading records' spare word, the normals
// out of the triangle records, the occluders out of the light's tree (built whatever its size: ratio 100).
struct Classified {
    std::vector<uint8_t> open;
    std::vector<float> normals;
    std::vector<uint32_t> occ;                                   // ascending
    uint32_t n_open = 0;
    double bias_max = 0.0, reach = 0.0, abs_max = 0.0;
};
static Classified classify(const std::vector<float> & verts, const float d[3], uint32_t threads) {
    OwnedScene owned = flat_scene(verts);
    owned.lights.push_back(light_towards(d));
    BvhBuildOptions bopt;
    ScenePackOptions how;
    how.threads = threads; how.shadow_tree_ratio = 100; how.bvh = &bopt;
    PackedScene P;
    std::vector<float> unindexed;
    std::string error;
    if (pack_as_upload(owned.desc(), WIDTH, how, &P, &unindexed, &error)) { fprintf(stderr, "shadow_open_host_harness: %s\n", error.c_str()); exit(2); }
    const uint32_t n = (uint32_t)(verts.size() / 9);
    Classified c;
    c.open.assign(n, 0);
    c.normals.assign((size_t)n * 3, 0.0f);
    for (uint32_t slot = 0; slot < n; ++slot) {
        const uint32_t t = P.keep.tri_order[slot];
        uint32_t mask;
        memcpy(&mask, &P.shade[(size_t)slot * 4 + 3].x, 4);
        c.open[t] = (uint8_t)(mask & 1u);
        const float4 r2 = P.tris[(size_t)slot * 3 + 2];
        c.normals[(size_t)t * 3] = r2.y; c.normals[(size_t)t * 3 + 1] = r2.z; c.normals[(size_t)t * 3 + 2] = r2.w;
    }
    for (uint32_t t : P.shadow_rec_tri)
        if (t != 0xFFFFFFFFu) c.occ.push_back(t);
    std::sort(c.occ.begin(), c.occ.end());
    const prt_shadow_open_info & oi = P.desc.shadow_open_info[0];
    c.n_open = oi.open_count;
    c.bias_max = oi.bias_max; c.reach = oi.reach; c.abs_max = P.desc.scene_abs_max;
    return c;
}

static void scene(const char * name, const std::vector<float> & verts, const float d[3]) {
    const uint32_t n = (uint32_t)(verts.size() / 9);
    const Classified c4 = classify(verts, d, 4);
    const std::vector<uint8_t> open1 = classify(verts, d, 1).open;                       // the threads change nothing
    const std::vector<uint8_t> & open = c4.open;
    const std::vector<float> & normals = c4.normals;
    const std::vector<uint32_t> & occ = c4.occ;
    const uint32_t n_open = c4.n_open;
    const float A = (float)c4.abs_max;
    struct { double bias_max, reach; } b = { c4.bias_max, c4.reach };
    uint64_t hash = 1469598103934665603ull, facing = 0, facing_open = 0;
    for (uint32_t t = 0; t < n; ++t) {
        hash = (hash ^ open[t]) * 1099511628211ull;
        const float * nn = &normals[(size_t)t * 3];
        if ((double)nn[0] * d[0] + (double)nn[1] * d[1] + (double)nn[2] * d[2] > 0.0) { facing++; facing_open += open[t]; }
    }
    printf("flags %s width %d | triangles %u occluders %zu facing %llu open %u facing_open %llu hash %016llx threads_agree %d bias_max %.17g reach %.17g abs_max %.17g\n",
           name, (int)WIDTH, n, occ.size(), (unsigned long long)facing, n_open, (unsigned long long)facing_open, (unsigned long long)hash,
           (int)(open == open1), b.bias_max, b.reach, (double)A);

    // ---- sanity
    std::vector<uint8_t> is_occ(n, 0);
    for (uint32_t t : occ) is_occ[t] = 1;
    uint64_t occ_open = 0, twin_open = 0, twins = 0;
    for (uint32_t t = 0; t < n; ++t) occ_open += is_occ[t] && open[t];
    auto same_corners = [&](uint32_t a, uint32_t c) {
        int found = 0;
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) found += !memcmp(&verts[(size_t)a * 9 + 3 * i], &verts[(size_t)c * 9 + 3 * j], 12);
        return found >= 3;
    };
    for (uint32_t t = 0; t < n; ++t)
        for (uint32_t o : occ)
            if (o != t && same_corners(t, o)) { twins++; twin_open += open[t]; break; }
    printf("sanity %s width %d | occluders_open %llu twins_of_occluders %llu twins_open %llu\n", name, (int)WIDTH, (unsigned long long)occ_open,
           (unsigned long long)twins, (unsigned long long)twin_open);

    // ---- brute force over every open triangle, the reference's test against every record (input order: no tree)
    const std::vector<float4> recs = mesh::records(verts, n, nullptr);
    const f3 dv = mk3(d[0], d[1], d[2]);
    const float biases[4] = { (float)b.bias_max, -(float)b.bias_max, 0.0f, 1e-3f };
    const float ulp = 4.0f * A * 1.1920929e-7f;
    const unsigned n_thr = 8;
    std::vector<unsigned long long> hits(n_thr, 0), origins(n_thr, 0);
    auto work = [&](unsigned k) {
        for (uint32_t t = k; t < n; t += n_thr) {
            if (!open[t]) continue;
            const float * v = &verts[(size_t)t * 9];
            const f3 c[3] = { mk3(v[0], v[1], v[2]), mk3(v[3], v[4], v[5]), mk3(v[6], v[7], v[8]) };
            const f3 gn = normalize3(mk3(normals[(size_t)t * 3], normals[(size_t)t * 3 + 1], normals[(size_t)t * 3 + 2]));
            const f3 centre = (c[0] + c[1] + c[2]) * (1.0f / 3.0f);
            f3 pts[13];
            int m = 0;
            pts[m++] = centre;
            for (int i = 0; i < 3; ++i) {
                const f3 mid = (c[i] + c[(i + 1) % 3]) * 0.5f;
                pts[m++] = c[i];
                pts[m++] = mid;
                pts[m++] = mid + normalize3(mid - c[(i + 2) % 3]) * ulp;          // a few ulp outside the edge
                pts[m++] = c[i] + normalize3(c[i] - centre) * ulp;                // ... and outside the corner
            }
            for (int i = 0; i < m; ++i)
                for (float bias : biases) {
                    origins[k]++;
                    if (occluded(recs, n, pts[i], gn, dv, bias)) hits[k]++;
                }
        }
    };
    std::vector<std::thread> pool;
    for (unsigned k = 0; k < n_thr; ++k) pool.emplace_back(work, k);
    for (std::thread & th : pool) th.join();
    unsigned long long h = 0, o = 0;
    for (unsigned k = 0; k < n_thr; ++k) { h += hits[k]; o += origins[k]; }
    // (the check can see a hit at all: the same origins on the triangles that are NOT open, a few of them)
    unsigned long long closed_hits = 0, closed = 0;
    for (uint32_t t = 0; t < n && closed < 400; ++t) {
        if (open[t] || is_occ[t]) continue;
        const float * v = &verts[(size_t)t * 9];
        const f3 centre = (mk3(v[0], v[1], v[2]) + mk3(v[3], v[4], v[5]) + mk3(v[6], v[7], v[8])) * (1.0f / 3.0f);
        const f3 gn = normalize3(mk3(normals[(size_t)t * 3], normals[(size_t)t * 3 + 1], normals[(size_t)t * 3 + 2]));
        closed++;
        closed_hits += occluded(recs, n, centre, gn, dv, 1e-3f);
    }
    printf("brute %s width %d | open %u origins %llu hits %llu closed_tried %llu closed_hits %llu\n", name, (int)WIDTH, n_open, o, h, closed, closed_hits);
}

// Inputs outside what the margin's argument covers leave a triangle unflagged: one occluder high above a floor of receivers,
// off to the side, so that every well-formed receiver is open - and the odd ones among them must not be.
static void margin_cases() {
    const float d[3] = { 0.0f, 1.0f, 0.0f };
    struct Case { const char * name; float v[9]; };
    const float inf = INFINITY, nan = NAN;
    const Case cases[] = {
        { "plain", { 0, 0, 0,  0, 0, 1,  1, 0, 0 } },
        { "zero_area_point", { 2, 0, 2,  2, 0, 2,  2, 0, 2 } },
        { "zero_area_line", { 0, 0, 0,  1, 0, 1,  2, 0, 2 } },
        { "sliver", { 0, 0, 0,  0, 0, 3,  1e-6f, 0, 1.5f } },
        { "tiny", { 0, 0, 0,  0, 0, 1e-25f,  1e-25f, 0, 0 } },
        { "inf_corner", { 0, 0, 0,  0, 0, inf,  1, 0, 0 } },
        { "nan_corner", { 0, 0, 0,  0, 0, 1,  nan, 0, 0 } },
        { "beyond_extent", { 0, 0, 0,  0, 0, 100,  100, 0, 0 } },
    };
    for (const Case & c : cases) {
        std::vector<float> verts(c.v, c.v + 9);
        const float occ[9] = { 3, 2, 3,  4, 2, 3,  3, 2, 4 };                  // faces down: an occluder for light from above
        verts.insert(verts.end(), occ, occ + 9);
        const std::vector<float> normals = stored_normals(verts);
        std::vector<uint32_t> ids = { 1u };
        std::vector<uint8_t> open;
        const ShadowOpenBounds b = shadow_open_bounds(4.0);
        shadow_open_flags(verts.data(), normals.data(), 2, d, ids, b, 1, &open);
        printf("margin %s | open %d occluder_open %d\n", c.name, (int)open[0], (int)open[1]);
    }
    // a face exported once more with its winding flipped: the copy faces away from the light, is an occluder, and lies in the
    // receiver's own plane on top of it - the receiver is not open, and no longer so with the copy moved aside (the control)
    {
        const float twin[18] = { 0, 0, 0,  0, 0, 1,  1, 0, 0,   0, 0, 0,  1, 0, 0,  0, 0, 1 };
        const float aside[18] = { 0, 0, 0,  0, 0, 1,  1, 0, 0,   3, 0, 0,  4, 0, 0,  3, 0, 1 };
        for (int k = 0; k < 2; ++k) {
            const std::vector<float> verts(k ? aside : twin, (k ? aside : twin) + 18);
            const std::vector<float> normals = stored_normals(verts);
            std::vector<uint32_t> ids;
            shadow_occluders(normals.data(), 2, d, 32.0 * 4.0, &ids);
            std::vector<uint8_t> open;
            shadow_open_flags(verts.data(), normals.data(), 2, d, ids, shadow_open_bounds(4.0), 1, &open);
            printf("margin %s | open %d occluder_open %d occluders %zu\n", k ? "flipped_copy_aside" : "flipped_twin", (int)open[0], (int)open[1], ids.size());
        }
    }
    // bounds and directions the argument does not cover: nothing is open
    const float plain[18] = { 0, 0, 0,  0, 0, 1,  1, 0, 0,   3, 2, 3,  4, 2, 3,  3, 2, 4 };
    const std::vector<float> verts(plain, plain + 18);
    const std::vector<float> normals = stored_normals(verts);
    const std::vector<uint32_t> ids = { 1u };
    struct Bound { const char * name; double A, bias, reach; float d[3]; };
    const Bound bounds[] = {
        { "good", 4.0, 4.0 / 2048, 8.0, { 0, 1, 0 } },
        { "huge_extent", 1e9, 1e9 / 2048, 2e9, { 0, 1, 0 } },               // o + d rounds d away
        { "extent_2_pow_14", 16384.0, 8.0, 32768.0, { 0, 1, 0 } },          // sqrt(3) E above 2^-8
        { "nan_extent", (double)nan, 0.0, 1.0, { 0, 1, 0 } },
        { "negative_bias", 4.0, -1.0, 8.0, { 0, 1, 0 } },
        { "nan_bias", 4.0, (double)nan, 8.0, { 0, 1, 0 } },
        { "zero_reach", 4.0, 4.0 / 2048, 0.0, { 0, 1, 0 } },
        { "inf_reach", 4.0, 4.0 / 2048, (double)inf, { 0, 1, 0 } },
        { "zero_direction", 4.0, 4.0 / 2048, 8.0, { 0, 0, 0 } },
        { "nan_direction", 4.0, 4.0 / 2048, 8.0, { 0, nan, 0 } },
        { "huge_direction", 4.0, 4.0 / 2048, 8.0, { 0, 1e30f, 0 } },
    };
    for (const Bound & bd : bounds) {
        ShadowOpenBounds b;
        b.coord_max = bd.A; b.bias_max = bd.bias; b.reach = bd.reach;
        std::vector<uint8_t> open;
        const uint32_t k = shadow_open_flags(verts.data(), normals.data(), 2, bd.d, ids, b, 1, &open);
        printf("bounds %s | open %u\n", bd.name, k);
    }
    // no occluder at all: nothing is flagged (the rays are traced, one node step each)
    {
        std::vector<uint8_t> open;
        const float up[3] = { 0, 1, 0 };
        const uint32_t k = shadow_open_flags(verts.data(), normals.data(), 2, up, std::vector<uint32_t>(), shadow_open_bounds(4.0), 1, &open);
        printf("bounds empty_set | open %u\n", k);
    }
}

int main(int argc, char ** argv) {
    // `flags cases.bin results.bin`: only the flags of every scene, one byte per input triangle behind a u32 count (what a GPU
    // test needs to know which triangles a render takes for open)
    if (argc == 4 && !strcmp(argv[1], "flags")) {
        FILE * fin, * fout;
        if (!open_in_out(argc, argv, "shadow_open_host_harness", &fin, &fout)) return 2;
        const uint32_t scenes = rd<uint32_t>(fin, 1)[0];
        for (uint32_t s = 0; s < scenes; ++s) {
            rd<char>(fin, 32);
            const uint32_t n = rd<uint32_t>(fin, 1)[0];
            const std::vector<float> d = rd<float>(fin, 3);
            const std::vector<float> verts = rd<float>(fin, (size_t)n * 9);
            wr(fout, &n, 1);
            wr(fout, classify(verts, d.data(), 2).open);
        }
        fclose(fin);
        fclose(fout);
        return 0;
    }
    if (argc < 2) { fprintf(stderr, "usage: shadow_open_host_harness [flags] cases.bin [results.bin]\n"); return 2; }
    harness_name = "shadow_open_host_harness";
    FILE * f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    const uint32_t scenes = rd<uint32_t>(f, 1)[0];
    for (uint32_t s = 0; s < scenes; ++s) {
        std::vector<char> name = rd<char>(f, 32);
        name[31] = 0;
        const uint32_t n = rd<uint32_t>(f, 1)[0];
        const std::vector<float> d = rd<float>(f, 3);
        const std::vector<float> verts = rd<float>(f, (size_t)n * 9);
        scene(name.data(), verts, d.data());
    }
    fclose(f);
    margin_cases();
    return 0;
}
