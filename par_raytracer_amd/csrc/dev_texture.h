// dev_texture.h - texture lookups of the shading path (texture.cpp:5-83, raytracer.cpp:439-502).
//
// Layout: every texture is expanded on the host to RGBA8 with GetTexel's channel rules (texture.cpp:27-41:
// missing alpha = 255, one-channel maps are grey, two-channel maps are (r, g, 0)), so a texel is ONE 4-byte load.
// The per-texel sRGB -> linear powf of the reference (texture.cpp:44-48) only ever sees 256 different inputs
// (u8 * (1/255)): the host evaluates them once with its own powf into srgb_lut and the device does table
// lookups, which is exact.  Everything else - wrap, v flip, the (size - 2) scale, clamp, floor, the order of the
// three lerps - is restated expression by expression; lerp stays a + (b - a) * t (mathlib.h:10), unfused.
#pragma once

#include "dev_scene.h"

namespace prt {

PRT_D float tex_wrap(float uv) {                               // texture.cpp:5-13; fmodf(x, 1) == x - trunc(x), exactly
    const float frac = uv - truncf(uv);
    return uv >= 0.0f ? frac : 1.0f + frac;
}

struct TexTap {                                                // the 2x2 footprint of one lookup
    const unsigned int * px;                                   // texture's first texel
    unsigned int i00, i01, i10, i11;                           // texel indices: (x0,y0) (x0,y1) (x1,y0) (x1,y1)
    float fx, fy;
};

PRT_D TexTap tex_tap(const DevScene & sc, unsigned int tex, float u, float v) {
    const DevTexture t = sc.textures[tex];
    u = tex_wrap(u);
    v = 1.0f - tex_wrap(v);
    const float sx = (float)(t.size_x - 2u), sy = (float)(t.size_y - 2u);
    const float tx = ref_min(ref_max(u * sx, 0.0f), sx);       // Clamp = Min(Max(n, a), b), mathlib.h:7-9
    const float ty = ref_min(ref_max(v * sy, 0.0f), sy);
    const unsigned int tx0 = (unsigned int)floorf(tx), ty0 = (unsigned int)floorf(ty);
    TexTap k;
    k.px = sc.texels + t.first_texel;
    k.i00 = ty0 * t.size_x + tx0;
    k.i01 = k.i00 + t.size_x;
    k.i10 = k.i00 + 1u;
    k.i11 = k.i01 + 1u;
    k.fx = tx - (float)tx0;
    k.fy = ty - (float)ty0;
    return k;
}

PRT_D float tex_lerp(float a, float b, float t) { return a + (b - a) * t; }

// One channel (0 = r .. 3 = a) of Texture_SampleBilinear: Lerp(Lerp(s00, s01, fy), Lerp(s10, s11, fy), fx).
PRT_D float tex_channel(const DevScene & sc, const TexTap & k, unsigned int t00, unsigned int t01, unsigned int t10, unsigned int t11,
                        int shift) {
    const float s00 = sc.srgb_lut[(t00 >> shift) & 255u], s01 = sc.srgb_lut[(t01 >> shift) & 255u];
    const float s10 = sc.srgb_lut[(t10 >> shift) & 255u], s11 = sc.srgb_lut[(t11 >> shift) & 255u];
    return tex_lerp(tex_lerp(s00, s01, k.fy), tex_lerp(s10, s11, k.fy), k.fx);
}

PRT_D f3 tex_sample_rgb(const DevScene & sc, unsigned int tex, float u, float v) {
    const TexTap k = tex_tap(sc, tex, u, v);
    const unsigned int t00 = k.px[k.i00], t01 = k.px[k.i01], t10 = k.px[k.i10], t11 = k.px[k.i11];
    return mk3(tex_channel(sc, k, t00, t01, t10, t11, 0), tex_channel(sc, k, t00, t01, t10, t11, 8),
               tex_channel(sc, k, t00, t01, t10, t11, 16));
}

PRT_D float tex_sample_r(const DevScene & sc, unsigned int tex, float u, float v) {
    const TexTap k = tex_tap(sc, tex, u, v);
    return tex_channel(sc, k, k.px[k.i00], k.px[k.i01], k.px[k.i10], k.px[k.i11], 0);
}

// What the textures of a hit change (raytracer.cpp:439-502): colours, alpha, the shading normal.  The functions below are the
// textured-hit block of shade_entry_on (kernels_wave.h), which calls them in this order with its alpha early-out between
// textured_hit_alpha and textured_hit_colours; KAT_TEXTURED_HIT (kernels_debug.h) fills the struct with them.
struct TexturedHit {
    float tu, tv;                      // the hit's texture coordinates (0, 0 for a material without maps)
    float alpha;
    bool alpha_tested;                 // raytracer.cpp:443: alpha <= 1 or an alpha map
    f3 ambient, diffuse, specular;
    f3 normal;                         // interpolated, then bump-mapped (not renormalised)
};

PRT_D bool textured_hit_any(const DevMaterial & mat) { return (mat.tex[0] & mat.tex[1] & mat.tex[2]) != 0xFFFFFFFFu; }

PRT_D void textured_hit_uv(const DevScene & sc, int tri, float bwx, float bwy, float bwz, float & tu, float & tv) {
    const float4 * up = sc.tri_uv + 2 * (size_t)tri;
    const float4 u01 = up[0], u2 = up[1];
    tu = 0.0f + u01.x * bwx; tv = 0.0f + u01.y * bwx;                   // raytracer.cpp:439-442
    tu = tu + u01.z * bwy; tv = tv + u01.w * bwy;
    tu = tu + u2.x * bwz; tv = tv + u2.y * bwz;
}

PRT_D void textured_hit_alpha(const DevScene & sc, const DevMaterial & mat, float tu, float tv, float & alpha, bool & alpha_tested) {
    const unsigned int alpha_tex = mat.tex[1] >> 16;
    if (alpha_tex != DEV_TEX_NONE) {                                    // raytracer.cpp:444-446
        alpha *= tex_sample_r(sc, alpha_tex, tu, tv);
        alpha_tested = true;
    }
}

// raytracer.cpp:455-462.  KD, KS: f3, or the frame's f3 stand-ins that shade_entry_on keeps its colours in
template <class KD, class KS>
PRT_D void textured_hit_colours(const DevScene & sc, const DevMaterial & mat, float tu, float tv, f3 & ka, KD & kd, KS & ks) {
    const unsigned int t_ka = mat.tex[0] & 0xFFFFu, t_kd = mat.tex[0] >> 16, t_ks = mat.tex[1] & 0xFFFFu;
    if (t_ka != DEV_TEX_NONE) ka = ka * tex_sample_rgb(sc, t_ka, tu, tv);
    if (t_kd != DEV_TEX_NONE) kd = kd * tex_sample_rgb(sc, t_kd, tu, tv);
    if (t_ks != DEV_TEX_NONE) ks = tex_sample_rgb(sc, t_ks, tu, tv);      // replaces Ks
}

// s0, s1, s2: the first three float4 of the triangle's shading record (dev_scene.h `shade`)
// N: f3, or the frame's f3 stand-in (the normal is written where shade_entry_on keeps it, and read back from there)
template <bool TEX, class N>
PRT_D void textured_hit_normal(const DevScene & sc, const DevMaterial & mat, int tri, float4 s0, float4 s1, float4 s2, float bwx, float bwy,
                               float bwz, float tu, float tv, N & hit_n) {
    f3 interp = mk3(0.0f, 0.0f, 0.0f);                                  // raytracer.cpp:464-467
    interp = interp + mk3(s0.x, s0.y, s0.z) * bwx;
    interp = interp + mk3(s0.w, s1.x, s1.y) * bwy;
    interp = interp + mk3(s1.z, s1.w, s2.x) * bwz;
    hit_n = normalize3(interp);
    if (TEX && (mat.tex[2] & 0xFFFFu) != DEV_TEX_NONE) {                // raytracer.cpp:468-502
        const float4 * tp = sc.tri_tan + 3 * (size_t)tri;
        const float4 t0 = tp[0], t1 = tp[1], t2 = tp[2];
        f3 tangent = mk3(0.0f, 0.0f, 0.0f);
        tangent = tangent + mk3(t0.x, t0.y, t0.z) * bwx;
        tangent = tangent + mk3(t0.w, t1.x, t1.y) * bwy;
        tangent = tangent + mk3(t1.z, t1.w, t2.x) * bwz;
        tangent = normalize3(tangent);
        const f3 bitangent = normalize3(cross3(hit_n, tangent));
        const f3 smp = tex_sample_rgb(sc, mat.tex[2] & 0xFFFFu, tu, tv);
        const f3 sn = smp * 2.0f - mk3(1.0f, 1.0f, 1.0f);
        // world_from_tangent_space * sn, columns (tangent, bitangent, normal), mathlib.h:697-709; not renormalised
        const f3 nn = hit_n;
        hit_n = mk3((tangent.x * sn.x + bitangent.x * sn.y) + nn.x * sn.z,
                    (tangent.y * sn.x + bitangent.y * sn.y) + nn.y * sn.z,
                    (tangent.z * sn.x + bitangent.z * sn.y) + nn.z * sn.z);
    }
}

// A hit at barycentrics (1 - v - w, v, w) of triangle record `tri` as shade_entry_on treats it, without its alpha early-out.
// Test hook: KAT_TEXTURED_HIT (kernels_debug.h) on the device, tests/texture_host_harness.cpp on the host.
PRT_D TexturedHit textured_hit_at(const DevScene & sc, unsigned int tri, float v, float w) {
    const float4 * sp = sc.shade + 4 * (size_t)tri;
    const float4 s0 = sp[0], s1 = sp[1], s2 = sp[2], s3 = sp[3];
    const DevMaterial mat = sc.materials[__float_as_int(s3.w)];
    const float bwy = v, bwz = w;
    const float bwx = 1.0f - bwy - bwz;                                 // raytracer.cpp:120
    TexturedHit h;
    h.tu = 0.0f; h.tv = 0.0f;
    h.alpha = mat.alpha;
    h.alpha_tested = mat.alpha <= 1.0f;                                 // raytracer.cpp:443
    h.ambient = mk3(mat.ambient[0], mat.ambient[1], mat.ambient[2]);
    h.diffuse = mk3(mat.diffuse[0], mat.diffuse[1], mat.diffuse[2]);
    h.specular = mk3(mat.specular[0], mat.specular[1], mat.specular[2]);
    if (textured_hit_any(mat)) {
        textured_hit_uv(sc, (int)tri, bwx, bwy, bwz, h.tu, h.tv);
        textured_hit_alpha(sc, mat, h.tu, h.tv, h.alpha, h.alpha_tested);
        textured_hit_colours(sc, mat, h.tu, h.tv, h.ambient, h.diffuse, h.specular);
    }
    textured_hit_normal<true>(sc, mat, (int)tri, s0, s1, s2, bwx, bwy, bwz, h.tu, h.tv, h.normal);
    return h;
}

}  // namespace prt
