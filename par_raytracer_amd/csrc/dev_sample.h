// dev_sample.h - area-weighted points on the uploaded surface (prt_sample_surface): the definition, written once for host and
// device.  The kernels are in kernels_sample.h; tests/sample_host_harness.cpp compiles this file with g++ through tests/hip_shim
// and every function below gives the same bits on both sides - plain float32 in a fixed expression order (+ - x / sqrtf only,
// compiled without contraction), one rint per triangle and integer sums.
//
// THE DEFINITION (include/prt.h).  Everything is a pure function of (the 48-byte records as they lie on
// the device, seed, sample index j): no tree, launch shape, batch split or run changes a bit.
//   ORDER    input order: triangle t is index triple t of the position index buffer (group g's run starts at first_index / 3).
//            The records lie in leaf-slot order; slot_of_input[t] (the inverse of the upload's slot -> t table) finds them.
//   WEIGHT   of a record (a, ab, ac): k = the exponent of the largest |component| of ab and ac (pow2_of, dev_closest.h),
//            A = sqrtf(length_sq(cross(ab x 2^-k, ac x 2^-k))) in float32; the weight is A x 2^(2k) - twice the area - held in a
//            double (sample_weight), which is exact: A has 24 bits and |2k| <= 252.  A zero or non-finite A: weight 0, never drawn.
//   FIXED    E: 2^(E-1) <= max weight < 2^E, from the largest bit pattern of the non-negative doubles (an integer max: the same
//            for every order); L: the smallest integer with n_tris <= 2^L; unit_exponent u = E + L - 62 (the rule of
//            qgrad_unit_exponent); W_t = (uint64)rint(weight_t x 2^-u) < 2^(62-L);
//            C_t = W_0 + .. + W_t, T = C_(n-1) < 2^62.  Integer sums: any scan gives the same C.  With L = 20 the largest
//            triangle keeps 42 bits, so float32's 24 bits survive for triangles down to 2^-18 of the largest area; below that a
//            weight loses bits and below 2^-42 it rounds to 0.
//   SAMPLE   j: rng_seed(prt_sample_key(seed, j >> 16, j & 0xFFFF)) (the key's packed word is j itself, j < 2^48), three draws of
//            rng_next<false>: r0 raw, u1 = rng_to_float01, u2 = rng_to_float01.  x = mulhi64(r0, T); the triangle is the smallest t
//            with C_t > x (zero-weight triangles are skipped by construction).  v = u1, w = u2, and both are mirrored (1 - v, 1 - w)
//            when v + w > 1; bw = (fmaxf(0, (1 - v) - w), v, w); point = (a + ab v) + ac w (closest_point_of's expression);
//            normal = normalize3(cross3(ab x 2^-k, ac x 2^-k)) - PRT_QUERY_CLOSEST's expression on the scaled edges.
//   MISS     T == 0 (no triangle, or none with area): zeros, group -1, vertex0 0xFFFFFFFF.
#pragma once

#include "../../include/prt_key.h"
#include "dev_closest.h"
#include "dev_query_grad.h"
#include "dev_rng.h"

namespace prt {

// The scale of a record's edges: 2^-k and 2^k of the largest |component| of ab and ac, and k itself (clamped as pow2_of clamps).
PRT_HD Pow2 sample_scale(f3 ab, f3 ac, int & k) {
    const float m = __builtin_fmaxf(abs_max3(ab), abs_max3(ac));
    unsigned int be = (__builtin_bit_cast(unsigned int, m) >> 23) & 0xFFu;
    be = be < 1u ? 1u : (be > 253u ? 253u : be);
    k = (int)be - 127;
    return pow2_of(m);
}

// The weight of a record: twice its area, exactly A x 2^(2k).  0 for a triangle that is never drawn.
PRT_HD double sample_weight(f3 ab, f3 ac) {
    int k;
    const Pow2 s = sample_scale(ab, ac, k);
    const f3 n = cross3(ab * s.down, ac * s.down);
    const float A = sqrtf(dot3(n, n));
    if (!(A > 0.0f) || !qgrad_finite(A)) return 0.0;
    return (double)A * qgrad_pow2(2 * k);
}

PRT_HD unsigned long long sample_double_bits(double w) {
    unsigned long long u;
    __builtin_memcpy(&u, &w, 8);
    return u;
}

// E of the largest weight's bit pattern (0 for no weight at all) and L of the triangle count.
PRT_HD int sample_exponent(unsigned long long max_bits) { return max_bits ? (int)(max_bits >> 52 & 0x7FFu) - 1022 : 0; }
PRT_HD int sample_log2_count(unsigned int n_tris) {
    int l = 0;
    while ((1ull << l) < (unsigned long long)n_tris) ++l;
    return l;
}
PRT_HD int sample_unit_exponent(unsigned long long max_bits, unsigned int n_tris) {
    return max_bits ? sample_exponent(max_bits) + sample_log2_count(n_tris) - 62 : 0;
}
// W_t: the weight in units of 2^u.  The scaling by a power of two is exact, rint rounds ties to even.
PRT_HD unsigned long long sample_to_fixed(double weight, int u) { return (unsigned long long)rint(weight * qgrad_pow2(-u)); }

PRT_HD unsigned long long sample_mulhi64(unsigned long long a, unsigned long long b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (unsigned long long)(((unsigned __int128)a * (unsigned __int128)b) >> 64);
#endif
}

// The smallest t with C[t] > x.  n >= 1 and x < C[n - 1] (x = mulhi64(r0, T) < T).
PRT_HD unsigned int sample_pick(const unsigned long long * C, unsigned int n, unsigned long long x) {
    unsigned int lo = 0u, hi = n - 1u;
    while (lo < hi) {
        const unsigned int mid = lo + (hi - lo) / 2u;
        if (C[mid] > x) hi = mid; else lo = mid + 1u;
    }
    return lo;
}

struct SampleDraw { unsigned long long r0; float v, w; };

// The three draws of sample j, and its barycentrics.
PRT_HD SampleDraw sample_draw(unsigned long long seed, unsigned long long j) {
    Rng r;
    rng_seed(r, prt_sample_key(seed, (uint32_t)(j >> 16), (uint32_t)(j & 0xFFFFull)));
    SampleDraw d;
    d.r0 = rng_next<false>(r, nullptr, 0);
    d.v = rng_to_float01(rng_next<false>(r, nullptr, 0));
    d.w = rng_to_float01(rng_next<false>(r, nullptr, 0));
    if (d.v + d.w > 1.0f) { d.v = 1.0f - d.v; d.w = 1.0f - d.w; }
    return d;
}

PRT_HD f3 sample_bw(float v, float w) { return mk3(__builtin_fmaxf(0.0f, (1.0f - v) - w), v, w); }
PRT_HD f3 sample_point(f3 a, f3 ab, f3 ac, float v, float w) { return (a + ab * v) + ac * w; }
PRT_HD f3 sample_normal(f3 ab, f3 ac) {
    int k;
    const Pow2 s = sample_scale(ab, ac, k);
    return normalize3(cross3(ab * s.down, ac * s.down));
}

}  // namespace prt
