// dev_sample_grad.h - gradients of a surface sample (prt_sample_surface_backward): the reverse-mode step of ONE sample, written
// once for host and device (the kernels are in kernels_sample_grad.h; tests/sample_host_harness.cpp runs the same step with g++).
// The fixed point that makes the vertex gradient's bits independent of the order of the samples is dev_query_grad.h's, unchanged.
//
// What is differentiated is the real-valued function behind dev_sample.h on the triangle (a, b, c) the forward call reported, with
// the sample's barycentrics bw held fixed:
//     point = bw0 a + bw1 b + bw2 c            normal = N / |N|,  N = cross(ab, ac),  ab = b - a,  ac = c - a
// The choice of the triangle is not differentiated: there is no gradient through the area weights (the stance dev_query_grad.h
// takes on silhouettes and dev_closest_grad.h on regions).
//
// float32 throughout, and - like the rest of the library - compiled with -ffp-contract=off, so the host harness and the device
// give the same bits.
#pragma once

#include "dev_sample.h"

namespace prt {

struct SGradOut { f3 ga, gb, gc; };   // dL/da, dL/db, dL/dc (the three corners)

// The derivative of normalize(cross(ab, ac)): from g = dL/dnormal to dL/dab and dL/dac, with dL/da = -(dL/dab + dL/dac) left to
// the caller.  Evaluated on the edges x 2^-k (sample_scale), so that |N| - an area - stays in range at every scale:
//     n = N / |N|     gN = (g - n (n.g)) / |N|     dL/dab = ac x gN     dL/dac = gN x ab
// and one exact product with 2^-k takes the two results back to the units of the unscaled edges.  False: the triangle has no
// finite normal (zero area, a NaN corner).
PRT_HD bool sgrad_normal(f3 ab0, f3 ac0, f3 g, f3 & g_ab, f3 & g_ac) {
    int k;
    const Pow2 s = sample_scale(ab0, ac0, k);
    const f3 ab = ab0 * s.down, ac = ac0 * s.down;
    const f3 N = cross3(ab, ac);
    const float len = sqrtf(dot3(N, N));
    const f3 n = N / len;
    if (!qgrad_finite3(n)) return false;
    const f3 gN = (g - n * dot3(n, g)) / len;
    g_ab = cross3(ac, gN) * s.down;
    g_ac = cross3(gN, ab) * s.down;
    return true;
}

// The reverse-mode step.  g_point, g_normal: dL/dpoint, dL/dnormal of this sample (zero where the caller has none); with_normal:
// the caller gave normal gradients at all.  Returns false - the sample is SKIPPED, it contributes nothing - when its triangle has
// no finite normal while normal gradients are given, or when any of the 9 gradient components is not finite (a NaN vertex, a NaN
// in bw or in the output gradients, an overflow).  *out is only meaningful when the step returns true.
PRT_HD bool sgrad_step(f3 a, f3 b, f3 c, f3 bw, f3 g_point, f3 g_normal, bool with_normal, SGradOut * out) {
    f3 ga = g_point * bw.x, gb = g_point * bw.y, gc = g_point * bw.z;
    if (with_normal) {
        f3 g_ab, g_ac;
        if (!sgrad_normal(b - a, c - a, g_normal, g_ab, g_ac)) return false;
        ga = ga - (g_ab + g_ac);
        gb = gb + g_ab;
        gc = gc + g_ac;
    }
    out->ga = ga; out->gb = gb; out->gc = gc;
    return qgrad_finite3(ga) && qgrad_finite3(gb) && qgrad_finite3(gc);
}

// The largest |component| of a sample's 9 vertex contributions.
PRT_HD float sgrad_abs_max(const SGradOut & g) {
    const float p = qgrad_abs_max3(g.ga), q = qgrad_abs_max3(g.gb), r = qgrad_abs_max3(g.gc);
    const float m = p > q ? p : q;
    return m > r ? m : r;
}
PRT_HD void sgrad_fixed9(const SGradOut & g, int u, long long * q) {
    q[0] = qgrad_to_fixed(g.ga.x, u); q[1] = qgrad_to_fixed(g.ga.y, u); q[2] = qgrad_to_fixed(g.ga.z, u);
    q[3] = qgrad_to_fixed(g.gb.x, u); q[4] = qgrad_to_fixed(g.gb.y, u); q[5] = qgrad_to_fixed(g.gb.z, u);
    q[6] = qgrad_to_fixed(g.gc.x, u); q[7] = qgrad_to_fixed(g.gc.y, u); q[8] = qgrad_to_fixed(g.gc.z, u);
}

}  // namespace prt
