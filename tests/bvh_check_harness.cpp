// bvh_check_harness.cpp - the guard in front of every upload, shown to fire: builds trees of both widths with both collapse
// rules (par_raytracer_amd/csrc/bvh_build.cpp), hands them to validate_bvh_links() and check_bvh_wide() (bvh_check.cpp) as they
// are, and then again with one edit each that the guard must catch.  Host arrays handed to host functions: nothing is uploaded.
// Prints one line per tree; tests/test_bvh_check.py builds it, runs it and asserts on the lines.
//
//   g++ -O1 -std=c++17 -ffp-contract=off -Ipar_raytracer_amd/csrc tests/bvh_check_harness.cpp
//       par_raytracer_amd/csrc/bvh_build.cpp par_raytracer_amd/csrc/bvh_check.cpp -pthread -o /tmp/bvh_check && /tmp/bvh_check
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "bvh_build.h"
#include "prt_options.h"
#include "harness_scene.h"

using namespace prt;

static void report(const std::string & what, const std::vector<float> & verts, const BvhWide & bvh) {
    const uint32_t n_tris = (uint32_t)(verts.size() / 9);
    const char * bad = validate_bvh_links(bvh, n_tris);
    uint64_t out[6];
    check_bvh_wide(verts.data(), n_tris, bvh, out);
    printf("%s | n_tris %u violations %llu nodes %llu depth %llu stack_bound %llu leaves %llu refs %llu | validate: %s\n", what.c_str(), n_tris,
           (unsigned long long)out[0], (unsigned long long)out[1], (unsigned long long)out[2], (unsigned long long)out[3],
           (unsigned long long)out[4], (unsigned long long)out[5], bad ? bad : "null");
}

// The test's own reading of a slot (layouts: dev_scene.h, bvh_build.h): is slot k of node d a leaf with triangles, and where
// is the byte of its upper x plane?
static bool leaf_slot(int width, const uint32_t * d, uint32_t k, uint32_t n_tris) {
    if (width == 8) return d[3] >> (8 + k) & 1u;
    return (int32_t)d[10 + k] < 0 && (~d[10 + k] >> 2) < n_tris;
}
static uint32_t * qhi_x(int width, uint32_t * d, uint32_t k, uint32_t * shift) {
    *shift = 8 * (k & 3u);
    return width == 8 ? &d[14 + (k >> 2)] : &d[7];
}

int main() {
    struct Scene { const char * name; std::vector<float> verts; };
    const float one[9] = { 0.5f, 0.25f, -1.0f, 1.5f, 0.25f, -1.0f, 0.5f, 1.0f, -2.0f };
    std::vector<Scene> scenes(3);
    scenes[0].name = "grid12";
    scenes[0].verts = harness_scene(12);
    scenes[1].name = "one";
    scenes[1].verts.assign(one, one + 9);
    scenes[2].name = "same37";
    for (int k = 0; k < 37; ++k) scenes[2].verts.insert(scenes[2].verts.end(), one, one + 9);

    for (int width = 4; width <= 8; width += 4)
        for (int collapse = 0; collapse <= 1; ++collapse) {
            const std::string tag = "width " + std::to_string(width) + (collapse ? " dp " : " greedy ");
            BvhBuildOptions opt;
            opt.collapse = collapse;
            BvhWide good;
            for (const Scene & sc : scenes) {
                build_bvh_wide(width, sc.verts.data(), (uint32_t)(sc.verts.size() / 9), 4, 2, &good, 1.0f, &opt);
                report(tag + sc.name + " good", sc.verts, good);
            }
            // ---- one edit each to a copy of the grid12 tree
            const std::vector<float> & verts = scenes[0].verts;
            const uint32_t n_tris = (uint32_t)(verts.size() / 9), nd = good.node_dwords;
            build_bvh_wide(width, verts.data(), n_tris, 4, 2, &good, 1.0f, &opt);
            uint32_t leaf_node = 0, leaf_k = 0, shift = 0;        // the first leaf slot whose upper x plane can go down by 8
            auto editable = [&]() {
                for (leaf_node = 0; leaf_node < good.node_count; ++leaf_node)
                    for (leaf_k = 0; leaf_k < (uint32_t)width; ++leaf_k) {
                        uint32_t * d = &good.nodes[(size_t)leaf_node * nd];
                        if (leaf_slot(width, d, leaf_k, n_tris) && (*qhi_x(width, d, leaf_k, &shift) >> shift & 0xFFu) >= 8u) return true;
                    }
                return false;
            };
            if (!editable()) { printf("%sgrid12: no leaf slot to edit\n", tag.c_str()); return 1; }

            BvhWide t = good;                                     // the root's (first) child: node_count
            if (width == 8) t.nodes[4] = t.node_count;
            else for (uint32_t k = 0; k < 4; ++k) if ((int32_t)t.nodes[10 + k] >= 0) { t.nodes[10 + k] = t.node_count; break; }
            report(tag + "grid12 edit child", verts, t);

            t = good;                                             // a leaf's triangles: past n_tris
            if (width == 8) t.nodes[(size_t)leaf_node * nd + 5] = n_tris;
            else t.nodes[(size_t)leaf_node * nd + 10 + leaf_k] = ~((n_tris - 1u) << 2 | 3u);
            report(tag + "grid12 edit leaf_range", verts, t);

            t = good;                                             // a leaf's upper x plane: 8 grid steps down
            *qhi_x(width, &t.nodes[(size_t)leaf_node * nd], leaf_k, &shift) -= 8u << shift;
            report(tag + "grid12 edit qhi", verts, t);

            t = good;                                             // the last slot holds the first slot's triangle
            t.tri_order[n_tris - 1] = t.tri_order[0];
            report(tag + "grid12 edit tri_order", verts, t);

            if (width == 8) {
                t = good;                                         // the root's internal children are leaves as well
                t.nodes[3] |= (t.nodes[3] & 0xFFu) << 8;
                report(tag + "grid12 edit masks", verts, t);
            }
        }
    return 0;
}
