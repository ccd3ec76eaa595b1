// hammersley.h - the reference's Hammersley set and the cosine lobe built on it, on the HOST: the functions prt_upload_scene
// fills DevScene::diffuse_dirs with.  A header of their own so that a host harness (tests/hemi_host_harness.cpp) computes the
// table with the very text the library compiles; the table's bits are part of prt_hemisphere_visibility's definition.
#pragma once

#include <cmath>
#include <cstdint>

namespace prt {

// raytracer.cpp:273-288 on the host.
inline float radical_inverse_vdc(uint32_t bits) {
    bits = (bits << 16u) | (bits >> 16u);
    bits = ((bits & 0x55555555u) << 1u) | ((bits & 0xAAAAAAAAu) >> 1u);
    bits = ((bits & 0x33333333u) << 2u) | ((bits & 0xCCCCCCCCu) >> 2u);
    bits = ((bits & 0x0F0F0F0Fu) << 4u) | ((bits & 0xF0F0F0F0u) >> 4u);
    bits = ((bits & 0x00FF00FFu) << 8u) | ((bits & 0xFF00FF00u) >> 8u);
    return (float)(bits * 2.3283064365386963e-10);
}

const float kPi32 = 3.1415927f;

// Tangent-space direction of GetDiffuseReflectionRay for Xi = Hammersley(i, 1024) (raytracer.cpp:322-328).
// Host libm: the same cosf / sinf the reference's CPU path calls.
inline float4 diffuse_tangent_dir(uint32_t i) {
    float xi_x = (float)i / (float)1024u;
    float xi_y = radical_inverse_vdc(i);
    float phi = xi_y * 2.0f * kPi32;
    float cp = cosf(phi);
    float sp = sinf(phi);
    float ct = sqrtf(1.0f - xi_x);
    float st = sqrtf(1.0f - ct * ct);
    return make_float4(cp * st, sp * st, ct, 0.0f);
}

}  // namespace prt
