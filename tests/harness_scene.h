// harness_scene.h - the scene of the host harnesses (trace_host_harness.cpp, bvh_check_harness.cpp): a wavy height field of
// 2 grid^2 triangles plus 300 floating triangles, every fifth of them twice (coincident copies), and 40 coplanar
// overlapping patches.  rnd() goes on from where the scene left it.
#pragma once

#include <cmath>
#include <cstdint>
#include <vector>

static uint64_t g_rng = 0x243F6A8885A308D3ull;
static double rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (double)(g_rng >> 11) / 9007199254740992.0; }

static std::vector<float> harness_scene(int grid) {       // 9 floats per triangle
    std::vector<float> verts;
    auto tri = [&](float ax, float ay, float az, float bx, float by, float bz, float cx, float cy, float cz) {
        const float v[9] = { ax, ay, az, bx, by, bz, cx, cy, cz };
        verts.insert(verts.end(), v, v + 9);
    };
    auto height = [](float x, float z) { return 0.35f * sinf(x * 0.9f) * cosf(z * 0.7f) + 0.1f * sinf(x * 3.1f + z * 2.3f); };
    for (int i = 0; i < grid; ++i)
        for (int j = 0; j < grid; ++j) {
            const float x0 = i * 0.25f - grid * 0.125f, x1 = x0 + 0.25f, z0 = j * 0.25f - grid * 0.125f, z1 = z0 + 0.25f;
            tri(x0, height(x0, z0), z0, x0, height(x0, z1), z1, x1, height(x1, z0), z0);            // counter-clockwise seen from +y
            tri(x1, height(x1, z0), z0, x0, height(x0, z1), z1, x1, height(x1, z1), z1);
        }
    for (int k = 0; k < 300; ++k) {                          // floating triangles, some of them twice (coincident copies)
        const float cx = (float)(rnd() * 8 - 4), cy = (float)(rnd() * 2 + 0.3), cz = (float)(rnd() * 8 - 4);
        float p[9];
        for (int q = 0; q < 9; ++q) p[q] = (float)(rnd() - 0.5) * 0.8f;
        tri(cx + p[0], cy + p[1], cz + p[2], cx + p[3], cy + p[4], cz + p[5], cx + p[6], cy + p[7], cz + p[8]);
        if (k % 5 == 0) tri(cx + p[0], cy + p[1], cz + p[2], cx + p[3], cy + p[4], cz + p[5], cx + p[6], cy + p[7], cz + p[8]);
    }
    for (int k = 0; k < 40; ++k) {                           // coplanar overlapping patches at y = 1.5 (decals)
        const float cx = (float)(rnd() * 6 - 3), cz = (float)(rnd() * 6 - 3), s = (float)(rnd() * 0.8 + 0.2);
        tri(cx, 1.5f, cz, cx, 1.5f, cz + s, cx + s, 1.5f, cz);
    }
    return verts;
}
