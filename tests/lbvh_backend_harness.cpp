// lbvh_backend_harness.cpp - the host back end of the GPU LBVH builder (par_raytracer_amd/csrc/bvh_build.cpp
// build_bvh_wide_from_radix_tree) on radix trees written by tests/lbvh_cases.py's reference: both widths, and the back-end settings
// plain, cluster 4, cluster 64 (the default) and cluster 2^20, each result handed to validate_bvh_links() and check_bvh_wide()
// (bvh_check.cpp).  Host arrays handed to host functions: no GPU library is involved.  Prints one line per tree;
// tests/test_lbvh_cases_host.py builds it (with the address and undefined-behaviour sanitizers), runs it and asserts on the lines.
//
//   g++ -O1 -std=c++17 -ffp-contract=off -Ipar_raytracer_amd/csrc tests/lbvh_backend_harness.cpp
//       par_raytracer_amd/csrc/bvh_build.cpp par_raytracer_amd/csrc/bvh_check.cpp -pthread -o /tmp/lbvh_backend && /tmp/lbvh_backend trees.bin
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "bvh_build.h"
#include "prt_options.h"

using namespace prt;

template <class T> static bool read_array(FILE * f, std::vector<T> & v, size_t count) {
    v.resize(count);
    return fread(v.data(), sizeof(T), count, f) == count;
}

int main(int argc, char ** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s trees.bin\n", argv[0]); return 2; }
    FILE * f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    uint32_t n_cases = 0;
    if (fread(&n_cases, 4, 1, f) != 1) return 2;
    struct Setting { const char * name; long long plain, cluster; };
    const Setting settings[4] = { { "plain", 1, -1 }, { "cluster4", 0, 4 }, { "cluster64", 0, -1 }, { "cluster1048576", 0, 1ll << 20 } };
    for (uint32_t c = 0; c < n_cases; ++c) {
        uint32_t len = 0, n = 0;
        if (fread(&len, 4, 1, f) != 1 || len > 256) return 2;
        std::string name(len, ' ');
        if (fread(&name[0], 1, len, f) != len || fread(&n, 4, 1, f) != 1 || n == 0) return 2;
        const size_t ni = n > 1 ? n - 1 : 1;
        std::vector<float> verts, node_box, leaf_box;
        std::vector<int32_t> left, right;
        std::vector<uint32_t> first, last, sorted_ids;
        if (!read_array(f, verts, (size_t)n * 9) || !read_array(f, left, ni) || !read_array(f, right, ni) || !read_array(f, first, ni) ||
            !read_array(f, last, ni) || !read_array(f, node_box, ni * 6) || !read_array(f, leaf_box, (size_t)n * 6) || !read_array(f, sorted_ids, n)) {
            fprintf(stderr, "%s: short file\n", name.c_str());
            return 2;
        }
        for (int width = 4; width <= 8; width += 4)
            for (const Setting & s : settings) {
                BvhBuildOptions opt;
                opt.lbvh_plain = s.plain;
                opt.lbvh_cluster = s.cluster;
                BvhWide bvh;
                build_bvh_wide_from_radix_tree(width, n, 4, left.data(), right.data(), first.data(), last.data(), node_box.data(), leaf_box.data(),
                                               sorted_ids.data(), &bvh, &opt);
                const char * bad = validate_bvh_links(bvh, n);
                uint64_t out[6];
                check_bvh_wide(verts.data(), n, bvh, out);
                printf("%s width %d %s | n_tris %u violations %llu nodes %llu depth %llu stack_bound %llu leaves %llu refs %llu | validate: %s\n", name.c_str(),
                       width, s.name, n, (unsigned long long)out[0], (unsigned long long)out[1], (unsigned long long)out[2], (unsigned long long)out[3],
                       (unsigned long long)out[4], (unsigned long long)out[5], bad ? bad : "null");
                fflush(stdout);
            }
    }
    fclose(f);
    return 0;
}
