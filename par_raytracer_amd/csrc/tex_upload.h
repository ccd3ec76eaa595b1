// tex_upload.h - what prt_upload_scene turns a scene's textures into (host code): the RGBA8 texel pool and texture table of
// dev_texture.h, and the 256-entry sRGB -> linear table.  A header of its own so that tests/texture_host_harness.cpp feeds
// dev_texture.h, compiled for the host, with exactly what the upload feeds the device.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "dev_scene.h"

namespace prt {

// textures: RGBA8 by GetTexel's channel rules (texture.cpp:27-41).  A texture no material can use (no texels, under 2 x 2, not
// 1..4 channels) keeps an all-zero record.  False: more than 2^32 texels.
inline bool tex_expand_rgba8(const prt_texture * textures, uint32_t texture_count, std::vector<DevTexture> & dev_tex,
                             std::vector<unsigned int> & texel_pool) {
    dev_tex.resize(texture_count);
    for (uint32_t ti = 0; ti < texture_count; ++ti) {
        const prt_texture & t = textures[ti];
        DevTexture & d = dev_tex[ti];
        memset(&d, 0, sizeof(d));
        if (!t.texels || t.size_x < 2 || t.size_y < 2 || t.channels < 1 || t.channels > 4) continue;     // unreferenced and unusable
        const size_t n = (size_t)t.size_x * t.size_y;
        if (texel_pool.size() + n >= (1ull << 32)) return false;
        d.first_texel = (unsigned int)texel_pool.size();
        d.size_x = t.size_x;
        d.size_y = t.size_y;
        texel_pool.resize(texel_pool.size() + n);
        unsigned int * out = texel_pool.data() + d.first_texel;
        for (size_t i = 0; i < n; ++i) {
            const uint8_t * px = t.texels + i * t.channels;
            unsigned int r = px[0], g = t.channels >= 2 ? px[1] : 0u, b = t.channels >= 3 ? px[2] : 0u, a = t.channels >= 4 ? px[3] : 255u;
            if (t.channels == 1) b = g = r;
            out[i] = r | g << 8 | b << 16 | a << 24;
        }
    }
    return true;
}

// A triangle's records of the texture path (dev_scene.h): 2 x float4 of texture coordinates, 3 x float4 of vertex tangents
// (packed like the normals in `shade`), from the three corners' values.
inline void tex_pack_uv(const float * u0, const float * u1, const float * u2, float4 * out2) {
    out2[0] = make_float4(u0[0], u0[1], u1[0], u1[1]);
    out2[1] = make_float4(u2[0], u2[1], 0.0f, 0.0f);
}
inline void tex_pack_tangents(const float * g0, const float * g1, const float * g2, float4 * out3) {
    out3[0] = make_float4(g0[0], g0[1], g0[2], g1[0]);
    out3[1] = make_float4(g1[1], g1[2], g2[0], g2[1]);
    out3[2] = make_float4(g2[2], 0.0f, 0.0f, 0.0f);
}
// A material's texture slots, two 16-bit texture numbers per word (DevMaterial::tex)
inline void tex_pack_material_slots(const prt_material & pm, DevMaterial & d) {
    auto slot16 = [](int32_t v) { return v < 0 ? (unsigned int)DEV_TEX_NONE : (unsigned int)v; };
    d.tex[0] = slot16(pm.ambient_texture) | slot16(pm.diffuse_texture) << 16;
    d.tex[1] = slot16(pm.specular_texture) | slot16(pm.alpha_texture) << 16;
    d.tex[2] = slot16(pm.bump_texture) | (unsigned int)DEV_TEX_NONE << 16;
}

// the 256 values Color_SRGBToLinear can take, by this machine's powf
inline void tex_fill_srgb_lut(std::vector<float> & lut) {
    lut.resize(256);
    const float one_over_255 = 1.0f / 255.0f;                  // texture.cpp:15
    for (int i = 0; i < 256; ++i) {
        const float srgb = (float)i * one_over_255;
        lut[i] = srgb <= 0.04045f ? srgb / 12.92f : powf((srgb + 0.055f) / 1.055f, 2.4f);     // color.h:13-21
    }
}

}  // namespace prt
