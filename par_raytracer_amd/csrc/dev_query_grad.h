// dev_query_grad.h - gradients of a closest-hit query: the reverse-mode step of ONE ray, written once for host and device (the
// kernels are in kernels_query_grad.h; tests/query_grad_host_harness.cpp runs the same step with g++), and the fixed-point
// conversion that makes the vertex gradient's bits independent of the order in which rays arrive.
//
// The function that is differentiated is the real-valued one behind tri_test and query_emit (dev_trace_common.h,
// kernels_query.h), on the triangle (a, b, c) the forward query reported:
//     ob = o + d * ray_bias     ab = b - a     ac = c - a     n = cross(ab, ac)     qp = -d     dd = dot(qp, n)
//     ap = ob - a               e = cross(qp, ap)
//     t = dot(ap, n) / dd       v = dot(ac, e) / dd            w = -dot(ab, e) / dd
//     bw = (1 - v - w, v, w)    position = ob + d * t          normal = n / |n|
// for any length of d.  Smooth on the reported triangle; a change of visibility (a silhouette) is not modelled.
//
// float32 throughout, and - like the rest of the library - compiled with -ffp-contract=off, so the host harness and the device
// give the same bits.
#pragma once

#include "dev_math.h"

namespace prt {

struct QGradOut { f3 ga, gb, gc, go, gd; };   // dL/da, dL/db, dL/dc (the three corners), dL/do, dL/dd

PRT_HD bool qgrad_finite(float x) { return x - x == 0.0f; }      // false for NaN and the infinities
PRT_HD bool qgrad_finite3(f3 a) { return qgrad_finite(a.x) && qgrad_finite(a.y) && qgrad_finite(a.z); }

// The reverse-mode step.  g_t, g_bw, g_pos, g_nrm: dL/dt, dL/dbw, dL/dposition, dL/dnormal of this ray (zero where the caller
// has none).  Returns false - the ray is SKIPPED, it contributes nothing - when the named triangle does not face the ray
// (dd <= 0: the forward test would not have reported it) or when any of the 15 gradient components is not finite (a grazing hit
// that overflows, a NaN vertex or ray).  *out is only meaningful when the step returns true.
PRT_HD bool qgrad_step(f3 o, f3 d, float ray_bias, f3 a, f3 b, f3 c, float g_t, f3 g_bw, f3 g_pos, f3 g_nrm, QGradOut * out) {
    // ---- forward, in the forward's association
    const f3 ob = o + d * ray_bias;
    const f3 ab = b - a, ac = c - a;
    const f3 n = cross3(ab, ac);
    const f3 qp = mk3(-d.x, -d.y, -d.z);
    const float dd = dot3(qp, n);
    if (!(dd > 0.0f)) return false;
    const f3 ap = ob - a;
    const f3 e = cross3(qp, ap);
    const float t = dot3(ap, n) / dd;
    const float v = dot3(ac, e) / dd;
    const float w = -dot3(ab, e) / dd;
    const float n_len = sqrtf(dot3(n, n));
    const f3 nrm = n / n_len;
    // ---- reverse
    const float gv = g_bw.y - g_bw.x, gw = g_bw.z - g_bw.x;       // bw = (1 - v - w, v, w)
    f3 g_ob = g_pos;                                               // position = ob + d * t
    f3 g_d = g_pos * t;
    const float gt = g_t + dot3(g_pos, d);
    f3 g_n = (g_nrm - nrm * dot3(nrm, g_nrm)) / n_len;             // normal = n / |n|
    const float g_tn = gt / dd, g_vn = gv / dd, g_wn = gw / dd;    // the three quotients
    const float g_dd = -(g_tn * t + g_vn * v + g_wn * w);
    f3 g_ap = n * g_tn;                                            // dot(ap, n)
    g_n = g_n + ap * g_tn;
    f3 g_ac = e * g_vn;                                            // dot(ac, e)
    f3 g_ab = e * -g_wn;                                           // -dot(ab, e)
    const f3 g_e = ac * g_vn - ab * g_wn;
    f3 g_qp = cross3(ap, g_e);                                     // e = cross(qp, ap)
    g_ap = g_ap + cross3(g_e, qp);
    g_qp = g_qp + n * g_dd;                                        // dd = dot(qp, n)
    g_n = g_n + qp * g_dd;
    g_ab = g_ab + cross3(ac, g_n);                                 // n = cross(ab, ac)
    g_ac = g_ac + cross3(g_n, ab);
    g_ob = g_ob + g_ap;                                            // ap = ob - a
    g_d = g_d - g_qp;                                              // qp = -d
    out->ga = mk3(0.0f, 0.0f, 0.0f) - g_ap - g_ab - g_ac;          // ab = b - a, ac = c - a
    out->gb = g_ab;
    out->gc = g_ac;
    out->go = g_ob;                                                // ob = o + d * ray_bias
    out->gd = g_d + g_ob * ray_bias;
    return qgrad_finite3(out->ga) && qgrad_finite3(out->gb) && qgrad_finite3(out->gc) && qgrad_finite3(out->go) && qgrad_finite3(out->gd);
}

PRT_HD float qgrad_abs_max3(f3 a) {
    const float x = fabsf(a.x), y = fabsf(a.y), z = fabsf(a.z);
    const float m = x > y ? x : y;
    return m > z ? m : z;
}
// The largest |component| of a ray's 9 vertex contributions.
PRT_HD float qgrad_abs_max(const QGradOut & g) {
    const float p = qgrad_abs_max3(g.ga), q = qgrad_abs_max3(g.gb), r = qgrad_abs_max3(g.gc);
    const float m = p > q ? p : q;
    return m > r ? m : r;
}

// ---- fixed point.  The vertex gradient is a sum over rays; float additions would make its last bits depend on the order in
// which the rays' atomics arrive.  Every contribution is instead rounded ONCE to a multiple of the batch's unit 2^u and added as
// a 64-bit integer - integer addition is associative, so the sum is the same bits for every launch shape and ray order - with
//     u = E + L - 62,    2^(E-1) <= M < 2^E (M: the largest |contribution| of the batch),    L: the smallest integer with
//     3 * count <= 2^L (a vertex can receive at most three contributions per ray).
// |c / 2^u| <= 2^(62 - L), so at most 2^L of them sum to less than 2^62 in magnitude: no overflow.  The rounding error per
// contribution is half a unit = 2^(L - 63) of M at most - for 2^30 rays, 2^-31 of M: far below a float32 ulp of M.
PRT_HD double qgrad_pow2(int e) {                // 2^e as a double, -1022 <= e <= 1023
    const unsigned long long u = (unsigned long long)(e + 1023) << 52;
    double r;
    __builtin_memcpy(&r, &u, 8);
    return r;
}
// E of a finite M > 0 (denormal floats included: the float is widened first).
PRT_HD int qgrad_exponent(float m) {
    const double w = (double)m;
    unsigned long long u;
    __builtin_memcpy(&u, &w, 8);
    return (int)(u >> 52 & 0x7FFu) - 1022;
}
PRT_HD int qgrad_log2_slots(unsigned int count) {
    const unsigned long long need = 3ull * count;
    int l = 0;
    while ((1ull << l) < need) ++l;
    return l;
}
PRT_HD int qgrad_unit_exponent(float m, unsigned int count) { return qgrad_exponent(m) + qgrad_log2_slots(count) - 62; }
// A contribution in units of 2^u: the scaling by a power of two is exact, rint rounds ties to even.
PRT_HD long long qgrad_to_fixed(float c, int u) { return (long long)rint((double)c * qgrad_pow2(-u)); }
PRT_HD float qgrad_from_fixed(long long acc, int u) { return (float)((double)acc * qgrad_pow2(u)); }
PRT_HD void qgrad_fixed9(const QGradOut & g, int u, long long * q) {
    q[0] = qgrad_to_fixed(g.ga.x, u); q[1] = qgrad_to_fixed(g.ga.y, u); q[2] = qgrad_to_fixed(g.ga.z, u);
    q[3] = qgrad_to_fixed(g.gb.x, u); q[4] = qgrad_to_fixed(g.gb.y, u); q[5] = qgrad_to_fixed(g.gb.z, u);
    q[6] = qgrad_to_fixed(g.gc.x, u); q[7] = qgrad_to_fixed(g.gc.y, u); q[8] = qgrad_to_fixed(g.gc.z, u);
}

// A ray's hit reference, as prt_trace_rays reports it: (group, vertex0) names corners first_index + vertex0 + 0..2 of the position
// index buffer.
enum { QGRAD_MISS = 0, QGRAD_HIT = 1, QGRAD_INVALID = 2 };
PRT_HD int qgrad_reference(int group, unsigned int vertex0, const unsigned int * group_runs, unsigned int group_count, unsigned int * first_corner) {
    if (group < 0) return QGRAD_MISS;
    if ((unsigned int)group >= group_count) return QGRAD_INVALID;
    const unsigned int first = group_runs[2 * group], run = group_runs[2 * group + 1];
    if (vertex0 % 3u != 0u || vertex0 >= run || run - vertex0 <= 2u) return QGRAD_INVALID;      // vertex0 + 2 >= index_count, without overflow
    *first_corner = first + vertex0;
    return QGRAD_HIT;
}

}  // namespace prt
