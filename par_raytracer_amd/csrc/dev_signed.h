// dev_signed.h - the sign of a closest-point answer (prt_signed_distance): the angle-weighted pseudonormal of Baerentzen &
// Aanaes, "Signed distance computation using the angle weighted pseudonormal" (2005), on the feature that closest_region_walk
// (dev_closest.h) names.  Host and device: tests/signed_host_harness.cpp compiles this file with g++ through tests/hip_shim, and
// every function below gives the same bits on both sides - plain float32 in a fixed expression order (+ - x / sqrtf only, this
// translation unit is compiled without contraction), one rint per contribution component and integer sums.
//
// THE DEFINITION (include/prt.h).  For the winner (leaf slot, d2) of a point p: R = the region of
// closest_region_walk on the slot's 48-byte record, q = closest_point_of, e = p - q, and
//     N = cross(ab, ac) x 2^-2k, unnormalised             R = interior
//     N = the edge's accumulator x 2^-32                  R = an edge
//     N = the vertex's accumulator x 2^-32                R = a vertex
//     s = dot3(e x 2^-k, N)                               k: the walk's scale (closest_scale) - only the sign of s is read
//     signed_dist = s < 0 ? -sqrtf(d2) : sqrtf(d2)         (NaN, s == 0, d2 == 0: the non-negative branch)
// THE ACCUMULATORS.  Every triangle record (a, ab, ac) gives n = normalize3(cross(ab, ac)) and its three interior angles; the
// vertex accumulator of corner k gets angle_k x n, the accumulator of each of its three edges gets n; a triangle whose n or
// angles are not all finite gives nothing.  Each component is rounded once to a multiple of 2^-32 (signed_to_fixed) and added
// as a 64-bit integer: the sum does not depend on the order of the adds (the device of section 4.9).  |component| < 4 and fewer
// than 3 x 2^26 incident corners (prt_upload_scene refuses 2^26 triangles) keep every sum below 2^62.
// THE TABLES (built by prt_api.hip):  adj[6 slot + 0..2] = the position indices of the record's corners a, b, c;
// adj[6 slot + 3..5] = the ids of its edges ab, ac, bc (an edge is an unordered pair of position indices);
// acc[3 i + 0..2] = vertex i's accumulator, acc[3 (position_count + j) + 0..2] = edge j's.
#pragma once

#include "dev_closest.h"

namespace prt {

struct SignedTables {
    const unsigned int * adj;            // 6 words per leaf slot
    long long * acc;                     // (position_count + edge_count) x 3
    unsigned int position_count;
    unsigned int edge_count;
};

// acos(x) for x in [-1, 1] from + - x / sqrtf alone: Abramowitz & Stegun 4.4.46, sqrt(1 - |x|) times a polynomial of degree 7 in
// |x| (Horner, highest power first), mirrored as pi - . for x < 0.  An x outside [-1, 1] by rounding is clamped; NaN stays NaN.
// The measured error against float64 acos is in DESIGN.md section 4.12 (tests/test_signed_host.py prints and bounds it).
PRT_HD float signed_acos(float x) {
    const float t = x < 0.0f ? -x : x;
    const float c = t > 1.0f ? 1.0f : t;
    float r = -0.0012624911f;
    r = r * c + 0.0066700901f;
    r = r * c + -0.0170881256f;
    r = r * c + 0.0308918810f;
    r = r * c + -0.0501743046f;
    r = r * c + 0.0889789874f;
    r = r * c + -0.2145988016f;
    r = r * c + 1.5707963050f;
    r = r * sqrtf(1.0f - c);
    return x < 0.0f ? 3.14159265358979323846f - r : r;
}

// The angle between u and v: signed_acos of the normalised dot product.  A zero-length side gives 0 / 0 = NaN.
PRT_HD float signed_angle(f3 u, f3 v) { return signed_acos(dot3(u, v) / sqrtf(dot3(u, u) * dot3(v, v))); }

PRT_HD bool signed_finite(float x) { return x - x == 0.0f; }            // false for NaN and +-inf

// One record's contributions: the unit normal and the interior angles at a, b, c.  False: the triangle contributes nothing.
// Both are free of scale, and both square an area (length_sq of the cross product, dot3(u, u) * dot3(v, v)): they are computed on
// (ab, ac) x 2^-k, k = the exponent of the largest |component| of the two edges (pow2_of, dev_closest.h) - the same bits wherever
// the unscaled products stayed in range.
PRT_HD bool signed_triangle_terms(f3 ab0, f3 ac0, f3 & n, float * alpha) {
    const Pow2 k = pow2_of(__builtin_fmaxf(abs_max3(ab0), abs_max3(ac0)));
    const f3 ab = ab0 * k.down, ac = ac0 * k.down;
    n = normalize3(cross3(ab, ac));
    const f3 bc = ac - ab;
    alpha[0] = signed_angle(ab, ac);
    alpha[1] = signed_angle(mk3(0.0f, 0.0f, 0.0f) - ab, bc);
    alpha[2] = signed_angle(ac, bc);
    return signed_finite(n.x) && signed_finite(n.y) && signed_finite(n.z) && signed_finite(alpha[0]) && signed_finite(alpha[1]) &&
           signed_finite(alpha[2]);
}

// A contribution component in units of 2^-32: the scaling is exact, rint rounds ties to even.
PRT_HD long long signed_to_fixed(float c) { return (long long)rint((double)c * 4294967296.0); }
PRT_HD float signed_from_fixed(long long a) { return (float)a * 2.3283064365386962890625e-10f; }      // x 2^-32, exact

// The 9 vertex integers (corner-major) and the 3 edge integers (the same for every edge) of one record.
PRT_HD void signed_triangle_fixed(f3 n, const float * alpha, long long * vq, long long * eq) {
    for (int k = 0; k < 3; ++k) {
        vq[3 * k + 0] = signed_to_fixed(alpha[k] * n.x);
        vq[3 * k + 1] = signed_to_fixed(alpha[k] * n.y);
        vq[3 * k + 2] = signed_to_fixed(alpha[k] * n.z);
    }
    eq[0] = signed_to_fixed(n.x); eq[1] = signed_to_fixed(n.y); eq[2] = signed_to_fixed(n.z);
}

// The column of adj that a vertex or edge region reads: CLOSEST_VERTEX_A, _B, EDGE_AB, VERTEX_C, EDGE_AC, EDGE_BC -> 0, 1, 3, 2, 4, 5.
PRT_HD unsigned int signed_adj_column(int region) { return (0x542310u >> (4u * (unsigned int)region)) & 7u; }

// N of the definition for leaf slot `slot` in region R; (ab, ac): the record's edges x 2^-k.
PRT_D f3 signed_normal_of(const SignedTables & T, unsigned int slot, int region, f3 ab, f3 ac) {
    if (region == CLOSEST_INTERIOR) return cross3(ab, ac);
    const unsigned int col = signed_adj_column(region);
    const size_t at = (size_t)T.adj[6u * (size_t)slot + col] + (col >= 3u ? (size_t)T.position_count : (size_t)0);
    const long long * a = T.acc + 3u * at;
    return mk3(signed_from_fixed(a[0]), signed_from_fixed(a[1]), signed_from_fixed(a[2]));
}

// signed_dist and the deciding region for the winner (slot, d2) of p; (a, ab, ac) is the slot's record.
PRT_D float signed_of_winner(const SignedTables & T, unsigned int slot, f3 p, f3 a, f3 ab, f3 ac, float d2, unsigned int & feature) {
    float d2r, v, w;
    ClosestTerms t;
    const int region = closest_region_walk(p, a, ab, ac, d2r, v, w, t);
    const Pow2 k = closest_scale(t.ap, ab, ac);
    const f3 e = (p - closest_point_of(a, ab, ac, v, w)) * k.down;
    const float s = dot3(e, signed_normal_of(T, slot, region, ab * k.down, ac * k.down));
    const float d = sqrtf(d2);
    feature = (unsigned int)region;
    return (s < 0.0f && d2 > 0.0f) ? -d : d;              // (d2 rounded to 0 below 2^-149 while s, on the scaled e, is not: +0, never -0)
}

}  // namespace prt
