// dev_closest.h - nearest surface point of a point (prt_closest_points): the definition, and the walk that finds it.
// PRT_D code that also compiles with g++ through tests/hip_shim (tests/closest_host_harness.cpp), as dev_trace*.h does.
//
// THE DEFINITION.  closest_on_triangle(p, a, ab, ac) is the region walk of Ericson, Real-Time Collision Detection, 5.1.5 - the
// three vertex regions, the three edge regions, then the interior - on the 48-byte record's own a, ab, ac (bp and cp are formed
// as ap - ab and ap - ac: the record is the only input), in plain float32 and the expression order written below, compiled like
// tri_geom without contraction: host and device give the same bits.  It yields the barycentrics (v, w) of the nearest point
// q = (a + ab * v) + ac * w and d2 = Dot(p - q, p - q).  The tests and d2 are evaluated on the vectors times an exact power of
// two (THE SCALE, below): the same bits at ordinary scale, and right from 2^-45 to 2^58, where the unscaled products left the
// float32 range.  Both sides of a triangle count; there is no facing test.  A triangle
// whose d2, v or w is not finite is not a candidate (a zero-area record with collinear corners divides by zero in the interior
// branch: it drops out instead of poisoning the point).
// The answer for p: among the triangles with finite d2 <= max_dist2 (FLT_MAX when no radius is given) the one with the
// smallest d2; among equal d2 bits the one with the smallest (group, vertex0), compared lexicographically (closest_takes).
// That is a total order on the candidates, so the answer is a pure function of (scene, point): it does not depend on the tree,
// the visit order, the launch shape or the run.
//
// THE WALK culls boxes by a lower bound of the distance from p instead of a ray's slab interval.  Per child box and axis the
// gap is max(lo - p, p - hi, 0); every gap is shrunk by `pad` before it is squared, and the sum of the squares is rounded down
// by 2^-21 (closest_bound).  A child is entered when its bound does not exceed the best d2 so far - equality enters, because
// an equal d2 may still win by the tie rule.  Why no box that holds a candidate with d2 <= best is ever culled (u = 2^-23,
// E = max(scene |coordinate|, batch |coordinate|), pad = 2^-16 E = 128 u E; DESIGN.md section 4.10 has the long form):
//   * the builder and the refit round every child box outward in double, so in exact arithmetic the de-quantised box contains
//     its triangles; what the walk computes per plane is fl(p - origin), fl(. +- pad) and one FMA, each within u E: the
//     computed gap exceeds the true gap to the triangle's extent by less than 4 u E;
//   * sqrt(d2) as closest_on_triangle computes it is within 64 u E of the true distance (the bound the CPU tests enforce on the
//     measured error: tests/test_closest_host.py), and the true distance is at least the norm of the true gaps;
//   * gaps shrunk by c = 128 u E - 4 u E > 64 u E have a norm of at most (norm of the true gaps) - c, so the exact sum of the
//     shrunk squares is <= the computed d2 of every triangle in the box; three products and two sums add at most 3 x 2^-24
//     relative, which the factor 1 - 2^-21 removes.  (Sums below the smallest normal float are outside the argument: scenes
//     whose extent is below 2^-40 are not supported by it.)
// An empty child slot has lo = 255 > hi = 0 on every axis, which is what the ray walk relies on; a point's gap to such a slot
// is positive but need not exceed the best d2, so the walk tests lo > hi itself (4-wide) or the node's slot masks (8-wide).
// FAR POINTS.  The pad grows with the batch's largest coordinate, and for a point far from the scene the bounds of all boxes
// differ by less than the pad: almost every bound ties and the walk visits much of the tree.  That cost is accepted - slow
// but exact.
// The walk keeps its state in a TravRay (r.o = the point, r.best.t = the best d2, r.best.v / w / tri; the ray's direction
// fields are unused and cost no register) so that the stacks, the marker, the leaf ranges and the end-of-walk flags of
// dev_trace4.h / dev_trace8.h serve it unchanged.
#pragma once

#include "dev_trace.h"

namespace prt {

// The regions of the walk, in the order of its tests.
enum { CLOSEST_VERTEX_A = 0, CLOSEST_VERTEX_B = 1, CLOSEST_EDGE_AB = 2, CLOSEST_VERTEX_C = 3, CLOSEST_EDGE_AC = 4, CLOSEST_EDGE_BC = 5,
       CLOSEST_INTERIOR = 6 };

// The six dot products and three areas of Ericson 5.1.5 on (a, ab, ac), for the walk below and for its derivative
// (dev_closest_grad.h).
struct ClosestTerms { f3 ap, bp, cp; float d1, d2, d3, d4, d5, d6, va, vb, vc; };

// THE SCALE of a record and a point ("Scale").  The areas va, vb, vc are products of four lengths: with
// edges above 2^31 or below 2^-31 they leave the float32 range, although v, w and the region depend on ratios of lengths alone.
// So the walk runs on (p - a, ab, ac) x 2^-k, k = the exponent of the largest |component| of the three vectors: the largest
// component then lies in [1, 2), and the four-fold products within 2^-126 .. 2^11 unless one vector is below 2^-31 of another.
// A product with a power of two is exact (the one exception: a component below 2^-126 x 2^k, which no longer matters to the
// largest one), so v, w, the region and - after the two exact products that undo the scale - d2 and the terms are the bits of the
// unscaled walk wherever that one stayed in range.  k is clamped to -126 .. 126 so that both powers are normal floats.
struct Pow2 { float down, up; };                         // 2^-k and 2^k

PRT_HD Pow2 pow2_of(float m) {
    unsigned int be = (__builtin_bit_cast(unsigned int, m) >> 23) & 0xFFu;
    be = be < 1u ? 1u : (be > 253u ? 253u : be);
    Pow2 s;
    s.down = __builtin_bit_cast(float, (254u - be) << 23);
    s.up = __builtin_bit_cast(float, be << 23);
    return s;
}

PRT_HD float abs_max3(f3 a) { return __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(a.x), __builtin_fabsf(a.y)), __builtin_fabsf(a.z)); }

PRT_HD Pow2 closest_scale(f3 ap, f3 ab, f3 ac) { return pow2_of(__builtin_fmaxf(__builtin_fmaxf(abs_max3(ap), abs_max3(ab)), abs_max3(ac))); }

// Ericson 5.1.5 on (a, ab, ac): v, w, d2 and the region (CLOSEST_*) whose branch produced them.  Host and device: the gradient's
// step and its host harness recompute the region with it.  The tests run on the scaled vectors; q is formed from the record
// itself (closest_point_of), e = p - q is scaled, squared and scaled back; the terms come back in the record's own units.
PRT_HD int closest_region_walk(f3 p, f3 a, f3 ab, f3 ac, float & d2, float & v, float & w, ClosestTerms & t) {
    const f3 ap0 = p - a;
    const Pow2 k = closest_scale(ap0, ab, ac);
    const f3 ap = ap0 * k.down, sab = ab * k.down, sac = ac * k.down;
    const float d1 = dot3(sab, ap), d2_ = dot3(sac, ap);
    const f3 bp = ap - sab;
    const float d3 = dot3(sab, bp), d4 = dot3(sac, bp);
    const f3 cp = ap - sac;
    const float d5 = dot3(sab, cp), d6 = dot3(sac, cp);
    const float vc = d1 * d4 - d3 * d2_;
    const float vb = d5 * d2_ - d1 * d6;
    const float va = d3 * d6 - d5 * d4;
    int region;
    if (d1 <= 0.0f && d2_ <= 0.0f) { v = 0.0f; w = 0.0f; region = CLOSEST_VERTEX_A; }
    else if (d3 >= 0.0f && d4 <= d3) { v = 1.0f; w = 0.0f; region = CLOSEST_VERTEX_B; }
    else if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) { v = d1 / (d1 - d3); w = 0.0f; region = CLOSEST_EDGE_AB; }
    else if (d6 >= 0.0f && d5 <= d6) { v = 0.0f; w = 1.0f; region = CLOSEST_VERTEX_C; }
    else if (vb <= 0.0f && d2_ >= 0.0f && d6 <= 0.0f) { v = 0.0f; w = d2_ / (d2_ - d6); region = CLOSEST_EDGE_AC; }
    else if (va <= 0.0f && (d4 - d3) >= 0.0f && (d5 - d6) >= 0.0f) {
        w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
        v = 1.0f - w;
        region = CLOSEST_EDGE_BC;
    } else {
        const float denom = 1.0f / ((va + vb) + vc);
        v = vb * denom;
        w = vc * denom;
        region = CLOSEST_INTERIOR;
    }
    const f3 q = (a + ab * v) + ac * w;
    const f3 e = (p - q) * k.down;
    d2 = (dot3(e, e) * k.up) * k.up;
    const float u2 = k.up * k.up;                        // the terms of the gradient: inf above 2^64, where it is not defined
    t.ap = ap0; t.bp = bp * k.up; t.cp = cp * k.up;
    t.d1 = d1 * u2; t.d2 = d2_ * u2; t.d3 = d3 * u2; t.d4 = d4 * u2; t.d5 = d5 * u2; t.d6 = d6 * u2;
    t.va = (va * u2) * u2; t.vb = (vb * u2) * u2; t.vc = (vc * u2) * u2;
    return region;
}

// Ericson 5.1.5 on (a, ab, ac).  Returns false when d2, v or w is not finite.
PRT_D bool closest_on_triangle(f3 p, f3 a, f3 ab, f3 ac, float & d2, float & v, float & w) {
    ClosestTerms t;
    closest_region_walk(p, a, ab, ac, d2, v, w, t);
    return isfinite(d2) && isfinite(v) && isfinite(w);
}

// The nearest point itself, from the winner's record: the expression closest_on_triangle measured d2 to.
PRT_D f3 closest_point_of(f3 a, f3 ab, f3 ac, float v, float w) { return (a + ab * v) + ac * w; }

// Does the candidate (d2, leaf slot ti) replace the best so far?  best.tri < 0: nothing found yet, best.t = max_dist2.
// leaf_map: leaf slot -> (group, vertex0); read only on equal d2 bits (d2 is a sum of squares: never -0).
PRT_D bool closest_takes(float d2, unsigned int ti, const HitRec & best, const uint2 * leaf_map) {
    if (d2 < best.t) return true;
    if (d2 != best.t) return false;
    if (best.tri < 0) return true;
    const uint2 c = leaf_map[ti], b = leaf_map[best.tri];
    return c.x < b.x || (c.x == b.x && c.y < b.y);
}

// The lower bound of d2 over a box from its three gaps, already shrunk by the pad: rounded down past the rounding of the sum.
PRT_D float closest_bound(float gx, float gy, float gz) {
    return __builtin_fmaf(gz, gz, __builtin_fmaf(gy, gy, gx * gx)) * 0.999999523162841796875f;          // 1 - 2^-21
}

// A point at the root.  max_d2 >= 0 (or +inf); the caller has sorted out invalid points.
template <class STK>
PRT_D void point_init(TravRay & r, f3 p, float max_d2, const STK & stk) {
    trav_idle(r);
    r.o = p;
    r.d = mk3(0.0f, 0.0f, 0.0f);
    r.best.t = max_d2;
    r.best.v = r.best.w = 0.0f;
    r.best.tri = -1;
    r.kind = TRACE_CLOSEST;
#if defined(PRT_BVH8)
    stk.put(0, make_int2(TRAV_SENTINEL, 0));
#else
    stk.push(0, TRAV_SENTINEL);
#endif
    r.sp = 1;
    r.node = 0;
}

#if !defined(PRT_BVH8)

// One 4-wide node (layout: dev_scene.h): the bound of every child box, the children sorted by it, descend into the nearest and
// push the others farthest first.  A child whose bound exceeds the best d2, and an empty slot, get the key +inf.
//   lo - p - pad = q_lo * 2^e - ((p - origin) + pad)        p - hi - pad = ((p - origin) - pad) - q_hi * 2^e
template <class STK, bool COUNT>
PRT_D void point_node_step(const DevScene & sc, TravRay & r, const STK & stk, TraceStats & st, float pad) {
    const uint4 * np = reinterpret_cast<const uint4 *>(reinterpret_cast<const char *>(sc.nodes) + ((unsigned int)r.node << 6));
    const uint4 w0 = np[0], w1 = np[1], w2 = np[2], w3 = np[3];
    if (COUNT) { st.nodes++; if (first_active_lane()) st.wnodes++; if ((unsigned int)r.sp > st.max_sp) st.max_sp = (unsigned int)r.sp; }
    const float sx = __uint_as_float(node_grid_step(w0.w)), sy = __uint_as_float(node_grid_step(w3.z)), sz = __uint_as_float(node_grid_step(w3.w));      // (the mantissas may hold a normal cone: dev_scene.h)
    const float ex = r.o.x - __uint_as_float(w0.x), ey = r.o.y - __uint_as_float(w0.y), ez = r.o.z - __uint_as_float(w0.z);
    const float lx = -(ex + pad), ly = -(ey + pad), lz = -(ez + pad);
    const float hx = ex - pad, hy = ey - pad, hz = ez - pad;
    float key[4];
    int link[4] = { (int)w2.z, (int)w2.w, (int)w3.x, (int)w3.y };
    const float inf = __uint_as_float(0x7F800000u);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned int qlx = (w1.x >> (8 * k)) & 0xFFu, qhx = (w1.w >> (8 * k)) & 0xFFu;
        const float gx = fmaxf(fmaxf(__builtin_fmaf((float)qlx, sx, lx), __builtin_fmaf(-(float)qhx, sx, hx)), 0.0f);
        const float gy = fmaxf(fmaxf(__builtin_fmaf((float)((w1.y >> (8 * k)) & 0xFFu), sy, ly),
                                     __builtin_fmaf(-(float)((w2.x >> (8 * k)) & 0xFFu), sy, hy)), 0.0f);
        const float gz = fmaxf(fmaxf(__builtin_fmaf((float)((w1.z >> (8 * k)) & 0xFFu), sz, lz),
                                     __builtin_fmaf(-(float)((w2.y >> (8 * k)) & 0xFFu), sz, hz)), 0.0f);
        const float b = closest_bound(gx, gy, gz);
        key[k] = (qlx <= qhx && b <= r.best.t) ? b : inf;
    }
    cswap(key[0], key[1], link[0], link[1]);
    cswap(key[2], key[3], link[2], link[3]);
    cswap(key[0], key[2], link[0], link[2]);
    cswap(key[1], key[3], link[1], link[3]);
    cswap(key[1], key[2], link[1], link[2]);
    if (key[0] < inf) {
        if (COUNT && first_active_lane()) st.wdescend++;
        if (key[3] < inf) trav_push(r, stk, link[3]);
        if (key[2] < inf) trav_push(r, stk, link[2]);
        if (key[1] < inf) trav_push(r, stk, link[1]);
        r.node = link[0];
    } else {
        if (COUNT && r.best.tri >= 0) st.culled++;
        if (COUNT && first_active_lane()) st.wpop++;
        trav_pop(r, stk);
    }
}

#else

// One 8-wide node (layout: bvh_build.h): the bound of every slot, the passing leaf slots noted for the leaf phase, and - the
// one-entry-per-node form of dev_trace8.h - the passing internal children left on the stack as one group.  Slot order: the
// slots are sorted along the node's ordering axis, so the bounds of the passing internal slots are roughly monotone in the
// slot number; the group is taken from the end whose slot has the smaller bound (bit 16 of the group word: descending).
// The order is a matter of speed only.
template <class STK, bool COUNT>
PRT_D void point_node_step(const DevScene & sc, TravRay & r, const STK & stk, TraceStats & st, float pad) {
    const uint4 * np = reinterpret_cast<const uint4 *>(reinterpret_cast<const char *>(sc.nodes) + (unsigned int)r.node * (unsigned int)BVH_NODE_BYTES);
    const uint4 q0 = np[0], q1 = np[1], q2 = np[2], q3 = np[3], q4 = np[4];
    if (COUNT) { st.nodes++; if (first_active_lane()) st.wnodes++; if ((unsigned int)r.sp > st.max_sp) st.max_sp = (unsigned int)r.sp; }
    const float sx = __uint_as_float(q0.w & 0x7F800000u), sy = __uint_as_float(q1.z & 0x7F800000u), sz = __uint_as_float(q1.w & 0x7F800000u);
    const float ex = r.o.x - __uint_as_float(q0.x), ey = r.o.y - __uint_as_float(q0.y), ez = r.o.z - __uint_as_float(q0.z);
    const float lx = -(ex + pad), ly = -(ey + pad), lz = -(ez + pad);
    const float hx = ex - pad, hy = ey - pad, hz = ez - pad;
    const unsigned int qlx[2] = { q2.x, q2.y }, qly[2] = { q2.z, q2.w }, qlz[2] = { q3.x, q3.y };
    const unsigned int qhx[2] = { q3.z, q3.w }, qhy[2] = { q4.x, q4.y }, qhz[2] = { q4.z, q4.w };
    const unsigned int imask = q0.w & 0xFFu, valid = imask | ((q0.w >> 8) & 0xFFu);
    unsigned int m = 0u;
    float k_low = 0.0f, k_high = 0.0f;                  // bounds of the lowest / highest passing internal slot
    bool any = false;
#pragma unroll
    for (int j = 7; j >= 0; --j) {
        const int h = j >> 2, k = j & 3;
        const float gx = fmaxf(fmaxf(__builtin_fmaf((float)((qlx[h] >> (8 * k)) & 0xFFu), sx, lx),
                                     __builtin_fmaf(-(float)((qhx[h] >> (8 * k)) & 0xFFu), sx, hx)), 0.0f);
        const float gy = fmaxf(fmaxf(__builtin_fmaf((float)((qly[h] >> (8 * k)) & 0xFFu), sy, ly),
                                     __builtin_fmaf(-(float)((qhy[h] >> (8 * k)) & 0xFFu), sy, hy)), 0.0f);
        const float gz = fmaxf(fmaxf(__builtin_fmaf((float)((qlz[h] >> (8 * k)) & 0xFFu), sz, lz),
                                     __builtin_fmaf(-(float)((qhz[h] >> (8 * k)) & 0xFFu), sz, hz)), 0.0f);
        const float b = closest_bound(gx, gy, gz);
        const bool pass = ((valid >> j) & 1u) != 0u && b <= r.best.t;
        m |= pass ? (1u << j) : 0u;
        if (pass && ((imask >> j) & 1u)) {
            k_low = b;
            if (!any) k_high = b;
            any = true;
        }
    }
    // the node's passing leaves wait for the leaf phase
    r.tbase = q1.y;
    r.tbits = (m & ~imask) | (q0.w & 0xFF00u) | (q1.z << 16);
    // the next node: from this node's passing internal children, else from the group on top of the stack
    const unsigned int mi = m & imask;
    unsigned int gbase = q1.x, gbits = imask | mi << 8 | (k_high < k_low ? 0x10000u : 0u);
    int at = r.sp;
    if (COUNT) {
        const unsigned long long down = __ballot(mi != 0u), all = __ballot(true);
        if (first_active_lane()) { st.wdescend += down != 0ull; st.wpop += down != all; }
    }
    if (mi == 0u) {
        if (COUNT && r.best.tri >= 0 && (m & ~imask) == 0u) st.culled++;
        at = r.sp - 1;
        const int2 e = stk.get(at);
        if (e.x <= TRAV_SENTINEL_LAST) {                // the marker: no node is left (the pending leaves still are)
            r.node = TRAV_SENTINEL;
            r.sp = at;
            return;
        }
        gbase = (unsigned int)e.x;
        gbits = (unsigned int)e.y;
    }
    const unsigned int rest8 = (gbits >> 8) & 0xFFu;
    const unsigned int s = (gbits & 0x10000u) ? 31u - (unsigned int)__clz((int)rest8) : (unsigned int)(__ffs((int)rest8) - 1);
    r.node = (int)(gbase + (unsigned int)__popc(gbits & ((1u << s) - 1u) & 0xFFu));
    gbits &= ~(0x100u << s);
    if ((gbits >> 8) & 0xFFu) {
        if (stk.put(at, make_int2((int)gbase, (int)gbits))) r.sp = at + 1;
        else { stk.flag(TRAV_FLAG_OVERFLOW); r.sp = at; }
    } else {
        r.sp = at;
    }
}

#endif

// The leaf the walk holds: every triangle through closest_on_triangle and the tie rule, then on to the next entry.
template <class STK, bool COUNT>
PRT_D void point_leaf(const DevScene & sc, TravRay & r, const STK & stk, TraceStats & st, const uint2 * leaf_map) {
    unsigned int first, count;
    trav_leaf_range(r, first, count);
    if (COUNT) { if (first_active_lane()) st.wleaves++; }
    for (unsigned int i = 0; i < count; ++i) {
        const unsigned int ti = first + i;
        const float4 * tp = reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(sc.tris) + ti * 48u);
        const float4 r0 = tp[0], r1 = tp[1], r2 = tp[2];
        if (COUNT) { st.tris++; if (first_active_lane()) st.wtris++; }
        float d2, v, w;
        // (ti < tri_count: the all-zero dummy record behind the last triangle, which a tree of 0 triangles links, is no candidate)
        if (closest_on_triangle(r.o, mk3(r0.x, r0.y, r0.z), mk3(r0.w, r1.x, r1.y), mk3(r1.z, r1.w, r2.x), d2, v, w) && ti < sc.tri_count &&
            closest_takes(d2, ti, r.best, leaf_map)) {
            r.best.t = d2;
            r.best.v = v;
            r.best.w = w;
            r.best.tri = (int)ti;
        }
    }
    trav_leaf_next(r, stk);
}

// Whole-point walk on a stack that cannot overflow (the slow path, and the host harness).
template <class STK, bool COUNT>
PRT_D HitRec closest_point_walk(const DevScene & sc, f3 p, float max_d2, float pad, const STK & stk, TraceStats & st, const uint2 * leaf_map) {
    TravRay r;
    point_init(r, p, max_d2, stk);
    for (;;) {
        while (trav_walking(r)) point_node_step<STK, COUNT>(sc, r, stk, st, pad);
        if (trav_done(r)) break;
        point_leaf<STK, COUNT>(sc, r, stk, st, leaf_map);
    }
    return r.best;
}

}  // namespace prt
