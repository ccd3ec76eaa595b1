// texture_host_harness.cpp - the texture lookups of the shading path (par_raytracer_amd/csrc/dev_texture.h) compiled for the host
// with tests/hip_shim, fed with what prt_upload_scene feeds the device: the RGBA8 texel pool, the texture table and the sRGB table
// of csrc/tex_upload.h.  tests/texture_cases.py writes the cases and reads the results; tests/test_texture_host.py compares them,
// bit for bit, with what the reference's own Texture_SampleBilinear returned (tests/golden/kat_texture.npz).
//
//   g++ -O1 -std=c++17 -ffp-contract=off -Itests/hip_shim -Ipar_raytracer_amd/csrc tests/texture_host_harness.cpp -o /tmp/texture_host
//       && /tmp/texture_host cases.bin results.bin
//
// cases.bin starts with a u32 mode.  A texture table is: u32 texture count, per texture 3 x u32 (size_x, size_y, channels), u32 byte
// count, the textures' texel bytes one after the other.
// Mode 0 (samples): a texture table, u32 record count, per record 3 x f32 (texture index, u, v).
//   results.bin: the 256 f32 of the sRGB table, then per record 5 x f32: tex_sample_rgb's x, y, z, tex_sample_r, and the sample's
//   fourth channel by tex_channel.
// Mode 1 (textured hits): u32 scene count, per scene a texture table, one prt_material (include/prt.h), the three corners' normals
//   (9 f32), texture coordinates (6 f32) and tangents (9 f32), u32 record count, per record 2 x f32 (v, w).
//   results.bin: per record 16 x f32: tu tv alpha alpha_tested ka(3) kd(3) ks(3) shading normal(3), as KAT_TEXTURED_HIT gives them.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include <hip/hip_runtime.h>            // tests/hip_shim: one lane at a time

#include "tex_upload.h"
#include "dev_texture.h"
#include "harness_io.h"

using namespace prt;

// A texture table as the cases file holds it, and what prt_upload_scene makes of it (csrc/tex_upload.h).
struct Tables {
    uint32_t n_tex = 0;
    std::vector<uint32_t> dims;
    std::vector<uint8_t> bytes;
    std::vector<prt_texture> textures;
    std::vector<DevTexture> dev_tex;
    std::vector<unsigned int> texel_pool;
    std::vector<float> lut;
    void read(FILE * fin) {
        n_tex = rd<uint32_t>(fin, 1)[0];
        dims = rd<uint32_t>(fin, 3 * (size_t)n_tex);
        bytes = rd<uint8_t>(fin, rd<uint32_t>(fin, 1)[0]);
        textures.resize(n_tex);
        size_t at = 0;
        for (uint32_t t = 0; t < n_tex; ++t) {
            textures[t].size_x = dims[3 * t]; textures[t].size_y = dims[3 * t + 1]; textures[t].channels = dims[3 * t + 2];
            textures[t].texels = bytes.data() + at;
            at += (size_t)dims[3 * t] * dims[3 * t + 1] * dims[3 * t + 2];
        }
        if (at != bytes.size()) { fprintf(stderr, "texture_host: the texel bytes do not match the sizes\n"); exit(2); }
        if (!tex_expand_rgba8(textures.data(), n_tex, dev_tex, texel_pool)) { fprintf(stderr, "texture_host: too many texels\n"); exit(2); }
        tex_fill_srgb_lut(lut);
    }
};

// Mode 1: scenes of one triangle and one material; per record (v, w) what textured_hit_at (csrc/dev_texture.h) makes of a hit there.
// The triangle's records are laid out as prt_upload_scene lays them out: tri_uv, tri_tan and the material's texture slots by the
// functions of csrc/tex_upload.h that the upload calls, the shading record and the material's other fields restated here.
static void run_hits(FILE * fin, FILE * fout) {
    const uint32_t n_scenes = rd<uint32_t>(fin, 1)[0];
    for (uint32_t si = 0; si < n_scenes; ++si) {
        Tables T;
        T.read(fin);
        const prt_material pm = rd<prt_material>(fin, 1)[0];
        const std::vector<float> nrm = rd<float>(fin, 9), uv = rd<float>(fin, 6), tan = rd<float>(fin, 9);
        const uint32_t n = rd<uint32_t>(fin, 1)[0];
        const std::vector<float> rec = rd<float>(fin, 2 * (size_t)n);
        const int32_t slots[5] = { pm.ambient_texture, pm.diffuse_texture, pm.specular_texture, pm.alpha_texture, pm.bump_texture };
        bool textured = false;
        for (int k = 0; k < 5; ++k) {
            if (slots[k] < 0) continue;
            textured = true;
            if ((uint32_t)slots[k] >= T.n_tex || T.dev_tex[slots[k]].size_x < 2) { fprintf(stderr, "texture_host: scene %u names no usable texture\n", si); exit(2); }
        }
        const bool bumped = pm.bump_texture >= 0;
        DevMaterial d;
        memset(&d, 0, sizeof(d));
        for (int k = 0; k < 3; ++k) { d.ambient[k] = pm.ambient_color[k]; d.diffuse[k] = pm.diffuse_color[k]; d.specular[k] = pm.specular_color[k]; }
        d.specular_intensity = pm.specular_intensity;
        d.index_of_refraction = pm.index_of_refraction;
        d.alpha = pm.alpha;
        tex_pack_material_slots(pm, d);
        float4 shade[4], tri_uv[2], tri_tan[3];
        shade[0] = make_float4(nrm[0], nrm[1], nrm[2], nrm[3]);
        shade[1] = make_float4(nrm[4], nrm[5], nrm[6], nrm[7]);
        shade[2] = make_float4(nrm[8], 0.0f, 0.0f, 1.0f);                  // (the geometric normal: not read here)
        shade[3] = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(0));       // material 0
        tex_pack_uv(&uv[0], &uv[2], &uv[4], tri_uv);
        tex_pack_tangents(&tan[0], &tan[3], &tan[6], tri_tan);
        DevScene sc;
        memset(&sc, 0, sizeof(sc));
        sc.shade = shade;
        sc.materials = &d;
        sc.material_count = 1;
        sc.tri_count = 1;
        if (textured) { sc.textures = T.dev_tex.data(); sc.texels = T.texel_pool.data(); sc.srgb_lut = T.lut.data(); sc.tri_uv = tri_uv; }
        if (bumped) sc.tri_tan = tri_tan;
        std::vector<float> out(16 * (size_t)n);
        for (uint32_t i = 0; i < n; ++i) {
            const TexturedHit h = textured_hit_at(sc, 0u, rec[2 * (size_t)i], rec[2 * (size_t)i + 1]);
            float * q = &out[16 * (size_t)i];
            q[0] = h.tu; q[1] = h.tv; q[2] = h.alpha; q[3] = h.alpha_tested ? 1.0f : 0.0f;
            q[4] = h.ambient.x; q[5] = h.ambient.y; q[6] = h.ambient.z;
            q[7] = h.diffuse.x; q[8] = h.diffuse.y; q[9] = h.diffuse.z;
            q[10] = h.specular.x; q[11] = h.specular.y; q[12] = h.specular.z;
            q[13] = h.normal.x; q[14] = h.normal.y; q[15] = h.normal.z;
        }
        wr(fout, out);
        printf("scene %u: %u textures, %u records\n", si, T.n_tex, n);
    }
}

int main(int argc, char ** argv) {
    FILE * fin, * fout;
    if (!open_in_out(argc, argv, "texture_host", &fin, &fout)) return 2;
    const uint32_t mode = rd<uint32_t>(fin, 1)[0];
    if (mode == 1) {
        run_hits(fin, fout);
        fclose(fin);
        return fclose(fout) ? 2 : 0;
    }
    Tables T;
    T.read(fin);
    const uint32_t n_tex = T.n_tex;
    const std::vector<DevTexture> & dev_tex = T.dev_tex;
    const std::vector<unsigned int> & texel_pool = T.texel_pool;
    const std::vector<float> & lut = T.lut;
    const uint32_t n = rd<uint32_t>(fin, 1)[0];
    const std::vector<float> rec = rd<float>(fin, 3 * (size_t)n);
    DevScene sc;
    memset(&sc, 0, sizeof(sc));
    sc.textures = dev_tex.data();
    sc.texels = texel_pool.data();
    sc.srgb_lut = lut.data();

    std::vector<float> out(5 * (size_t)n);
    for (uint32_t i = 0; i < n; ++i) {
        const float ti = rec[3 * (size_t)i], u = rec[3 * (size_t)i + 1], v = rec[3 * (size_t)i + 2];
        if (!(ti >= 0.0f && ti < (float)n_tex) || dev_tex[(size_t)ti].size_x < 2) { fprintf(stderr, "texture_host: record %u names no usable texture\n", i); return 2; }
        const f3 c = tex_sample_rgb(sc, (unsigned int)ti, u, v);
        out[5 * (size_t)i] = c.x; out[5 * (size_t)i + 1] = c.y; out[5 * (size_t)i + 2] = c.z;
        out[5 * (size_t)i + 3] = tex_sample_r(sc, (unsigned int)ti, u, v);
        // the fourth channel of the expanded texels: no kernel reads it, the reference's sample has it
        const TexTap k = tex_tap(sc, (unsigned int)ti, u, v);
        out[5 * (size_t)i + 4] = tex_channel(sc, k, k.px[k.i00], k.px[k.i01], k.px[k.i10], k.px[k.i11], 24);
    }
    wr(fout, lut);
    wr(fout, out);
    printf("%u textures, %zu texels, %u records\n", n_tex, texel_pool.size(), n);
    fclose(fin);
    return fclose(fout) ? 2 : 0;
}
