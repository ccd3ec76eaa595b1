// dev_closest_grad.h - gradients of a closest-point query: the reverse-mode step of ONE point, written once for host and device
// (the kernels are in kernels_closest_grad.h; tests/closest_grad_host_harness.cpp runs the same step with g++).  The fixed point
// that makes the vertex gradient's bits independent of the order of the points is dev_query_grad.h's, unchanged.
//
// The function that is differentiated is the real-valued one behind closest_on_triangle (dev_closest.h) on the triangle
// (a, b, c) the forward query reported, inside the region R its walk takes for p in float32 (closest_region_walk: recomputed
// here, never passed in):
//     ab = b - a    ac = c - a    ap = p - a    bp = ap - ab    cp = ap - ac
//     d1 = ab.ap    d2 = ac.ap    d3 = ab.bp    d4 = ac.bp      d5 = ab.cp    d6 = ac.cp
//     vc = d1 d4 - d3 d2          vb = d5 d2 - d1 d6            va = d3 d6 - d5 d4
//     R  region      v                          w
//     0  vertex a    0                          0
//     1  vertex b    1                          0
//     2  edge ab     d1 / (d1 - d3)             0
//     3  vertex c    0                          1
//     4  edge ac     0                          d2 / (d2 - d6)
//     5  edge bc     1 - w                      (d4 - d3) / ((d4 - d3) + (d5 - d6))
//     6  interior    vb / ((va + vb) + vc)      vc / ((va + vb) + vc)
//     point = q = (a + ab v) + ac w             dist2 = Dot(p - q, p - q)                 bw = (1 - v - w, v, w)
// The constants 0 and 1 have zero derivative.  A change of region, or of the winning triangle, is not modelled - the stance
// dev_query_grad.h takes on silhouettes.
//
// float32 throughout, and - like the rest of the library - compiled with -ffp-contract=off, so the host harness and the device
// give the same bits.
#pragma once

#include "dev_closest.h"
#include "dev_query_grad.h"

namespace prt {

struct CGradOut { f3 ga, gb, gc, gp; int region; };   // dL/da, dL/db, dL/dc (the three corners), dL/dp; the region R of p

// The reverse-mode step.  g_dist2, g_point, g_bw: dL/ddist2, dL/dpoint, dL/dbw of this point (zero where the caller has none).
// Returns false - the point is SKIPPED, it contributes nothing - when the named triangle is no candidate for p (d2, v or w not
// finite: the forward query would not have reported it) or when any of the 12 gradient components is not finite (a NaN vertex or
// point, a NaN in the output gradients, an overflow).  out->region is set in every case; the rest of *out is only meaningful
// when the step returns true.
PRT_HD bool cgrad_step(f3 p, f3 a, f3 b, f3 c, float g_dist2, f3 g_point, f3 g_bw, CGradOut * out) {
    // ---- forward, as the upload forms the record and the walk reads it
    const f3 ab = b - a, ac = c - a;
    float dist2, v, w;
    ClosestTerms t;
    const int region = closest_region_walk(p, a, ab, ac, dist2, v, w, t);
    out->region = region;
    if (!(qgrad_finite(dist2) && qgrad_finite(v) && qgrad_finite(w))) return false;
    const f3 q = (a + ab * v) + ac * w;
    const f3 e = p - q;
    // ---- reverse
    const f3 g_e = e * (2.0f * g_dist2);                           // dist2 = dot(e, e)
    const f3 g_q = g_point - g_e;                                  // e = p - q
    f3 g_p = g_e;
    f3 g_a = g_q;                                                  // q = (a + ab v) + ac w
    f3 g_ab = g_q * v;
    f3 g_ac = g_q * w;
    const float gv = dot3(g_q, ab) + (g_bw.y - g_bw.x);            // bw = (1 - v - w, v, w)
    const float gw = dot3(g_q, ac) + (g_bw.z - g_bw.x);
    float g1 = 0.0f, g2 = 0.0f, g3 = 0.0f, g4 = 0.0f, g5 = 0.0f, g6 = 0.0f;       // dL/dd1 .. dL/dd6
    if (region == CLOSEST_EDGE_AB) {                               // v = d1 / (d1 - d3)
        const float s = gv / (t.d1 - t.d3);
        g3 = s * v;
        g1 = s - g3;
    } else if (region == CLOSEST_EDGE_AC) {                        // w = d2 / (d2 - d6)
        const float s = gw / (t.d2 - t.d6);
        g6 = s * w;
        g2 = s - g6;
    } else if (region == CLOSEST_EDGE_BC) {                        // w = x / (x + y), x = d4 - d3, y = d5 - d6; v = 1 - w
        const float s = (gw - gv) / ((t.d4 - t.d3) + (t.d5 - t.d6));
        const float gy = -(s * w), gx = s + gy;
        g4 = gx; g3 = -gx;
        g5 = gy; g6 = -gy;
    } else if (region == CLOSEST_INTERIOR) {                       // v = vb r, w = vc r, r = 1 / ((va + vb) + vc)
        const float r = 1.0f / ((t.va + t.vb) + t.vc);
        const float g_va = -((gv * v + gw * w) * r);
        const float g_vb = gv * r + g_va, g_vc = gw * r + g_va;
        g1 = g_vc * t.d4 - g_vb * t.d6;                            // vc = d1 d4 - d3 d2, vb = d5 d2 - d1 d6, va = d3 d6 - d5 d4
        g2 = g_vb * t.d5 - g_vc * t.d3;
        g3 = g_va * t.d6 - g_vc * t.d2;
        g4 = g_vc * t.d1 - g_va * t.d5;
        g5 = g_vb * t.d2 - g_va * t.d4;
        g6 = g_va * t.d3 - g_vb * t.d1;
    }
    g_ab = g_ab + (t.ap * g1 + t.bp * g3 + t.cp * g5);             // d1 = ab.ap, d3 = ab.bp, d5 = ab.cp
    g_ac = g_ac + (t.ap * g2 + t.bp * g4 + t.cp * g6);             // d2 = ac.ap, d4 = ac.bp, d6 = ac.cp
    const f3 g_bp = ab * g3 + ac * g4, g_cp = ab * g5 + ac * g6;
    const f3 g_ap = (ab * g1 + ac * g2) + (g_bp + g_cp);           // bp = ap - ab, cp = ap - ac
    g_ab = g_ab - g_bp;
    g_ac = g_ac - g_cp;
    g_p = g_p + g_ap;                                              // ap = p - a
    g_a = g_a - g_ap;
    out->ga = g_a - g_ab - g_ac;                                   // ab = b - a, ac = c - a
    out->gb = g_ab;
    out->gc = g_ac;
    out->gp = g_p;
    return qgrad_finite3(out->ga) && qgrad_finite3(out->gb) && qgrad_finite3(out->gc) && qgrad_finite3(out->gp);
}

// The largest |component| of a point's 9 vertex contributions.
PRT_HD float cgrad_abs_max(const CGradOut & g) {
    const float p = qgrad_abs_max3(g.ga), q = qgrad_abs_max3(g.gb), r = qgrad_abs_max3(g.gc);
    const float m = p > q ? p : q;
    return m > r ? m : r;
}
PRT_HD void cgrad_fixed9(const CGradOut & g, int u, long long * q) {
    q[0] = qgrad_to_fixed(g.ga.x, u); q[1] = qgrad_to_fixed(g.ga.y, u); q[2] = qgrad_to_fixed(g.ga.z, u);
    q[3] = qgrad_to_fixed(g.gb.x, u); q[4] = qgrad_to_fixed(g.gb.y, u); q[5] = qgrad_to_fixed(g.gb.z, u);
    q[6] = qgrad_to_fixed(g.gc.x, u); q[7] = qgrad_to_fixed(g.gc.y, u); q[8] = qgrad_to_fixed(g.gc.z, u);
}

}  // namespace prt
