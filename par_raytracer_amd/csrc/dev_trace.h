// dev_trace.h - the traversal the library is built with.
//   default     dev_trace4.h: 4-wide quantised BVH (64 B nodes), children sorted by entry distance at every step
//   -DPRT_BVH8  dev_trace8.h: 8-wide compressed BVH (80 B nodes), children ordered along one axis, no per-step sort (built in
//               round 3; 1 - 2 % behind the 4-wide tree on the headline frame, ahead on deep bounce trees: profiles/r03_ab_bvh8.txt)
// Both implement one interface, and everything below the #include is written against it once:
//   TravRay; LdsStack<BLOCK>, LdsSpillStack<BLOCK>, GlobalStack; StackEntry, STACK_ENTRY_INTS, BVH_NODE_BYTES
//   trav_idle(r), trav_init(r, o, d, kind, pad, stk, root = 0)                no ray / a ray at the root of a tree
//   trav_start<ANY_LENGTH>(r, o, d, kind, pad, stk)                           the same, for directions of any length (below)
//   trav_walking(r), trav_done(r)                                             wants a node step / ended; neither: holds a leaf
//   trav_node_step<STK, COUNT, CONES = false>(sc, r, stk, st, pad), trav_leaf<STK, COUNT>(sc, r, stk, st)
//   trav_leaf_range(r, first, count), trav_leaf_next(r, stk)                  the held leaf's triangles, and the step past it
//   trav_cone_kind(P)                                                         what a call ors into its closest-hit rays' kind
//   trav_wants_resolve(r, stk), trav_needs_slow_path(r, stk)                  what the marker says after the end
// Code outside the two traversal files never reads r.node itself.
#pragma once

#if defined(PRT_BVH8)
#include "dev_trace8.h"
#else
#include "dev_trace4.h"
#endif

namespace prt {

// ---------------------------------------------------------------------------------------------------------------------
// trav_init walks the boxes along the direction it is given and clamps its components away from 0 at an ABSOLUTE 1e-30: sound
// for a unit direction from an origin near the scene, which is all the render kernels ever trace.  A query's origin and
// direction are anything (include/prt.h), and two things then part the box test from the triangle test:
//   * IntersectRayTriangle does not test the ray o + t d but o + t w, w = (o + d) - o as floats (qp = o - (o + d),
//     raytracer.cpp:88-89).  For a unit direction in a scene scaled by 2^20, w is d rounded to quarters: another ray.
//     trav_start<true> - the query paths - walks the boxes along w.  (w = 0: no triangle can be hit; any walk will do.)
//   * the clamp is absolute.  At |d| = 1e-29 it is a tenth of the ray and bends it out of the boxes its triangles lie in; in a
//     scene of coordinates beyond 3e8 the clamped component's 1 / 1e-30 times a coordinate is inf, and inf - inf = NaN culls
//     the box.  trav_start<true> clamps at 2^-40 of the direction's largest component m instead (across the whole scene a
//     2^-22th of the pad; 1 / component times a coordinate stays finite up to coordinates of 2^67 m), after bringing m into
//     [1, 2) where it is below 2^-20, by a power of two, which is exact.  The box parameters of such a short direction then
//     come out 2^k times too SMALL beside the ray's own t (the best hit, tmax), so a box is culled against the best hit later
//     than it could be and never sooner: conservative.  Unit directions are walked as they are.
// The triangle tests see the caller's direction, bit for bit.  trav_start<false> is trav_init.
template <bool ANY_LENGTH, class STK>
PRT_D void trav_start(TravRay & r, f3 o, f3 d, int kind, float pad, const STK & stk, int root = 0) {
    if (ANY_LENGTH) {
        f3 w = (o + d) - o;
        if (w.x == 0.0f && w.y == 0.0f && w.z == 0.0f) w = d;
        float m = fmaxf(fmaxf(fabsf(w.x), fabsf(w.y)), fabsf(w.z));
        if (m < 9.5367431640625e-7f) {                                      // 2^-20
            const int k = -ilogbf(m);
            w = mk3(ldexpf(w.x, k), ldexpf(w.y, k), ldexpf(w.z, k));
            m = ldexpf(m, k);
        }
        const float tiny = m * 9.094947017729282e-13f;                      // 2^-40
        if (fabsf(w.x) < tiny) w.x = copysignf(tiny, w.x);
        if (fabsf(w.y) < tiny) w.y = copysignf(tiny, w.y);
        if (fabsf(w.z) < tiny) w.z = copysignf(tiny, w.z);
        trav_init(r, o, w, kind, pad, stk, root);
        r.d = d;
        return;
    }
    trav_init(r, o, d, kind, pad, stk, root);
}

// ---------------------------------------------------------------------------------------------------------------------
// Near ties: the reference's answer for a ray whose closest hit has company within a few ulp.
//
// The reference keeps `best` (FLT_MAX at first) and offers it every triangle in ITS visit order - sphere tree depth first,
// c1 before c0, groups in leaf order, triangles in index order (raytracer.cpp:136, 208-209); a triangle replaces best iff
// !(t > best * d) and t / d < best (:104, :149, :220).  Far from best both comparisons say the same; within an ulp or two
// they need not, so which of several near-coincident hits survives depends on the order.  What cannot depend on it:
// let N be the candidates with t <= bound, where no candidate lies in the "moat" (bound, bound * (1 + 2^-20)].  Then
//   - every member of N beats any best that is not in N on both comparisons with room to spare, so the first member the
//     reference meets is accepted whatever came before it;
//   - from then on best <= bound, and nothing outside N can pass `t / d < best`.
// Hence the reference's final hit is its own filter run over N alone, in its visit order, from FLT_MAX.  That is what this
// function does: N's members are fetched one by one in visit order (tri_rank) - each fetch a traversal bounded by `bound`,
// no storage needed - and put through tri_test_ref.  If the moat turns out to be occupied the bound is widened and the
// replay starts over; after sc.tie_widen_max widenings the replay is finished over the set as it stands and the event is
// counted (DevScene::near_tie_unresolved: the render call then fails - it has never been seen to happen).
// The reference also skips a whole GROUP whose bounding sphere it enters later than its best hit so far
// (raytracer.cpp:176-181): RefSphereWalk (dev_trace_common.h) replays that on the uploaded sphere tree.
template <class STK, bool COUNT, bool ANY_LENGTH = false>
PRT_D HitRec resolve_near_ties(const DevScene & sc, f3 o, f3 d, float pad, float min_t, const STK & stk, TraceStats & st) {
    TravRay r;
    HitRec result = hit_miss();
    const f3 qp = o - (o + d);
    float bound = min_t * PRT_TIE_NEAR;
    for (unsigned int widen = 0; ; ++widen) {
        const bool last = widen >= sc.tie_widen_max;
        const float moat = bound * 1.00000095367431640625f;          // 1 + 2^-20
        bool occupied = false;
        float best = 3.402823466e+38f;                              // the reference's best_hit.t, replayed
        result.tri = -1;
        unsigned int next_rank = 0;                                 // candidates of rank >= next_rank are still to come
        RefSphereWalk walk;
        walk.reset();
        for (;;) {
            // the member of N with the smallest rank >= next_rank
            unsigned int c_rank = 0xFFFFFFFFu;
            int c_tri = -1;
            trav_start<ANY_LENGTH>(r, o, d, TRACE_CLOSEST, pad, stk);
            r.best.t = moat;                                        // the boxes are culled against the moat's far side
            for (;;) {
                while (trav_walking(r)) trav_node_step<STK, COUNT>(sc, r, stk, st, pad);
                if (trav_done(r)) break;
                unsigned int first, count;
                trav_leaf_range(r, first, count);
                for (unsigned int i = 0; i < count; ++i) {
                    const unsigned int ti = first + i;
                    const float4 * tp = sc.tris + 3 * (size_t)ti;
                    const float4 r0 = tp[0], r1 = tp[1], r2 = tp[2];
                    float t, dd, v, w;
                    if (!tri_geom(o, qp, mk3(r0.x, r0.y, r0.z), mk3(r0.w, r1.x, r1.y), mk3(r1.z, r1.w, r2.x), mk3(r2.y, r2.z, r2.w), t, dd, v, w)) continue;
                    const float th = t * (1.0f / dd);
                    if (th > bound) { if (th <= moat) occupied = true; continue; }
                    const unsigned int rk = sc.tri_rank[ti];
                    if (rk >= next_rank && rk < c_rank) { c_rank = rk; c_tri = (int)ti; }
                }
                trav_leaf_next(r, stk);
            }
            if (c_tri < 0 || (occupied && !last)) break;
            const float4 * tp = sc.tris + 3 * (size_t)c_tri;
            const float4 r0 = tp[0], r1 = tp[1], r2 = tp[2];
            float t, v, w;
            if (walk.offers(sc, o, d, c_rank, best) &&
                tri_test_ref(o, qp, mk3(r0.x, r0.y, r0.z), mk3(r0.w, r1.x, r1.y), mk3(r1.z, r1.w, r2.x), mk3(r2.y, r2.z, r2.w), best, t, v, w)) {
                best = t;
                result.t = t; result.v = v; result.w = w; result.tri = c_tri;
            }
            next_rank = c_rank + 1u;
        }
        if (!occupied) break;
        if (last) {                                                 // gave up widening: the replay ran over the set as it stood
            if (sc.near_tie_unresolved) atomicAdd(sc.near_tie_unresolved, 1ull);
            break;
        }
        bound = moat * PRT_TIE_NEAR;                                // take the moat's occupants in and try again
    }
    return result;
}

// Whole-ray traversal, "while-while" (Aila & Laine): every lane first walks internal nodes until it holds a leaf (or runs out
// of work), and only then does the wave run the triangle code.  With 64 lanes a fused node-or-leaf loop would execute the (4x
// longer) leaf body in almost every iteration.  Near ties are decided on the spot: this is the form for the slow paths, on a
// stack that cannot overflow.  ANY_LENGTH: the queries' form (trav_start).  root: where an any-hit ray starts (a closest-hit
// ray's near ties are replayed over the scene's tree: it always starts at 0).  CONES: the walk takes the nodes' normal cones
// (the render kernels' slow paths; the replay of near ties never does - it only meets triangles the cones leave alone).
template <class STK, bool COUNT, bool ANY_LENGTH = false, bool CONES = false>
PRT_D HitRec trace_ray(const DevScene & sc, f3 o, f3 d, int kind, float pad, const STK & stk, TraceStats & st, int root = 0) {
    TravRay r;
    trav_start<ANY_LENGTH>(r, o, d, kind, pad, stk, root);
    for (;;) {
        while (trav_walking(r)) trav_node_step<STK, COUNT, CONES>(sc, r, stk, st, pad);
        if (trav_done(r)) break;
        if (trav_leaf<STK, COUNT>(sc, r, stk, st)) return r.best;           // any-hit ray: found its occluder
    }
    if (trav_wants_resolve(r, stk)) return resolve_near_ties<STK, COUNT, ANY_LENGTH>(sc, o, d, pad, r.best.t, stk, st);
    return r.best;
}

// ---------------------------------------------------------------------------------------------------------------------
// Rays whose triangle test overflows.  IntersectRayTriangle multiplies the direction, the origin's distance from a vertex and the
// triangle's edges (raytracer.cpp:82-125): where such a product passes FLT_MAX the sums behind it are inf - inf = NaN, every
// comparison with a NaN is false, and the reference ACCEPTS a triangle the ray's line is nowhere near (a direction of length
// 2^120 from 10^4 scene extents away).  No box test can find such a hit, so a query traces these rays without one:
// ray_overflows is true when a bound of the products' exponents - s: the scene's largest |coordinate| -
//     |qp| < 2^ed   |ap| < 2^eo   |ab|, |ac| < 2^(es + 1)   |n| < 2^(2 es + 3)
//     dd < 2^(ed + 2 es + 5)   t < 2^(eo + 2 es + 5)   |e| < 2^(ed + eo + 1)   v, w < 2^(ed + eo + es + 4)
// reaches 2^127; scan_closest is then TraceRay as written - every triangle in the reference's visit order (slot_of_rank: the
// inverse of tri_rank) through RefSphereWalk and the reference's filter - and scan_any_below the brute-force rule of OCCLUDED.
// Linear in the scene per ray; unit directions near the scene never come here.
PRT_D bool ray_overflows(float scene_max, f3 o, f3 d) {
    const float D = fmaxf(fmaxf(fabsf(d.x), fabsf(d.y)), fabsf(d.z)), O = fmaxf(fmaxf(fabsf(o.x), fabsf(o.y)), fabsf(o.z));
    const float s = fmaxf(scene_max, 1.17549435e-38f);
    const int es = ilogbf(s) + 1, eo = ilogbf(fmaxf(O, s)) + 2;
    const int ed = ilogbf(fmaxf(fmaxf(D, O * 1.1920929e-7f), 1.17549435e-38f)) + 2;          // qp = o - (o + d): d, or the rounding of o + d
    const int top = (ed > eo ? ed : eo) + 2 * es + 5, mixed = ed + eo + es + 4;
    return (top > mixed ? top : mixed) >= 127;
}

template <bool COUNT>
PRT_D HitRec scan_closest(const DevScene & sc, const unsigned int * slot_of_rank, f3 o, f3 d, TraceStats & st) {
    const f3 qp = o - (o + d);
    HitRec h = hit_miss();
    RefSphereWalk walk;
    walk.reset();
    for (unsigned int rank = 0; rank < sc.tri_count; ++rank) {
        if (!walk.offers(sc, o, d, rank, h.t)) {
            if (walk.skip_until > rank) rank = walk.skip_until - 1u;        // the refused sphere's range ends there
            continue;
        }
        const unsigned int ti = slot_of_rank[rank];
        const float4 * tp = sc.tris + 3 * (size_t)ti;
        const float4 r0 = tp[0], r1 = tp[1], r2 = tp[2];
        float t, v, w;
        if (COUNT) st.tris++;
        if (tri_test_ref(o, qp, mk3(r0.x, r0.y, r0.z), mk3(r0.w, r1.x, r1.y), mk3(r1.z, r1.w, r2.x), mk3(r2.y, r2.z, r2.w), h.t, t, v, w)) {
            h.t = t; h.v = v; h.w = w; h.tri = (int)ti;
        }
    }
    return h;
}

template <bool COUNT>
PRT_D HitRec scan_any_below(const DevScene & sc, f3 o, f3 d, float tmax, TraceStats & st) {
    const f3 qp = o - (o + d);
    HitRec h = hit_miss();
    for (unsigned int ti = 0; ti < sc.tri_count; ++ti) {
        const float4 * tp = sc.tris + 3 * (size_t)ti;
        const float4 r0 = tp[0], r1 = tp[1], r2 = tp[2];
        float t, dd, v, w;
        if (COUNT) st.tris++;
        if (!tri_geom(o, qp, mk3(r0.x, r0.y, r0.z), mk3(r0.w, r1.x, r1.y), mk3(r1.z, r1.w, r2.x), mk3(r2.y, r2.z, r2.w), t, dd, v, w)) continue;
        if (t > 3.402823466e+38f * dd) continue;                            // raytracer.cpp:104 against FLT_MAX
        const float th = t * (1.0f / dd);
        if (th < tmax) { h.t = th; h.tri = (int)ti; return h; }
    }
    return h;
}

// The any-hit walks of the OCCLUDED rule's slow path (k_query_exact, k_hemi_exact; the host harnesses run them too).
// Any hit below tmax on a stack that cannot overflow (trace_ray's walk with the best hit started at tmax).
template <class STK, bool COUNT>
PRT_D HitRec query_any_below(const DevScene & sc, f3 o, f3 d, float tmax, float pad, const STK & stk, TraceStats & st) {
    TravRay r;
    trav_start<true>(r, o, d, TRACE_ANY, pad, stk);
    r.best.t = tmax;
    for (;;) {
        while (trav_walking(r)) trav_node_step<STK, COUNT>(sc, r, stk, st, pad);
        if (trav_done(r)) break;
        if (trav_leaf<STK, COUNT>(sc, r, stk, st)) break;                   // found its occluder
    }
    return r.best;
}

// OCCLUDED for an origin far from the scene (query_far): there the triangle test's t carries a rounding error (ap = o - a is
// large and cancels in Dot(ap, n)) that can exceed the box pad, so a box culled against tmax could hold a triangle whose
// computed t is below tmax.  This walk culls boxes by geometry only and applies the rule itself to every triangle the ray's
// line meets: IntersectRayTriangle against FLT_MAX and t < tmax.
template <class STK, bool COUNT>
PRT_D HitRec query_any_unculled(const DevScene & sc, f3 o, f3 d, float tmax, float pad, const STK & stk, TraceStats & st) {
    TravRay r;
    trav_start<true>(r, o, d, TRACE_ANY, pad, stk);
    r.best.t = __uint_as_float(0x7F800000u);
    const f3 qp = o - (o + d);                                              // raytracer.cpp:88-89
    HitRec h = hit_miss();
    for (;;) {
        while (trav_walking(r)) trav_node_step<STK, COUNT>(sc, r, stk, st, pad);
        if (trav_done(r)) break;
        unsigned int first, count;
        trav_leaf_range(r, first, count);
        for (unsigned int i = 0; i < count; ++i) {
            const float4 * tp = sc.tris + 3 * (size_t)(first + i);
            const float4 r0 = tp[0], r1 = tp[1], r2 = tp[2];
            float t, dd, v, w;
            if (COUNT) st.tris++;
            if (!tri_geom(o, qp, mk3(r0.x, r0.y, r0.z), mk3(r0.w, r1.x, r1.y), mk3(r1.z, r1.w, r2.x), mk3(r2.y, r2.z, r2.w), t, dd, v, w)) continue;
            if (t > 3.402823466e+38f * dd) continue;                        // raytracer.cpp:104 against FLT_MAX
            const float th = t * (1.0f / dd);
            if (th < tmax) { h.t = th; h.tri = (int)(first + i); return h; }
        }
        trav_leaf_next(r, stk);
    }
    return h;
}

}  // namespace prt
