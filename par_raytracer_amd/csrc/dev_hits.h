// dev_hits.h - a ray's K nearest hits, both sides, resumable (prt_trace_hits): the definition, the sorted list and the walks.
// PRT_D code that also compiles with g++ through tests/hip_shim (tests/hits_host_harness.cpp), as dev_closest.h does.
//
// THE DEFINITION (include/prt.h has it word for word).  For the biased origin o, the direction d as given and qp = o - (o + d),
// a record (a, ab, ac, n) is a FRONT candidate when PRT_QUERY_OCCLUDED's rule accepts it: tri_geom true, !(t > FLT_MAX * dd),
// th = t * (1 / dd) < tmax.  With BACK it is also a BACK candidate when the same rule accepts (a, ac, ab, -n); dd decides which of
// the two a record can be (hits_side).  A candidate's key is (th, group, vertex0), compared lexicographically (hits_key_less);
// a cursor leaves the candidates whose key is strictly greater; the answer is the k smallest in key order.  The rule does not
// depend on the visit order, so there are no near-tie replays and no sphere walk: the answer is a pure function of the records
// and the ray.
//
// THE LIST.  Up to k entries (th, leaf slot << 1 | back), ascending in key order, in storage the caller supplies: a column of the
// workgroup's LDS behind the stack columns (LdsHitList: word j of lane l at col[j * BLOCK + l], as LdsStack lays its entries
// out), or a global column (GlobalHitList, the exact kernel and the host harness).  v, w, group and vertex0 are not stored:
// hits_slot recomputes them from the winner's record with the expressions of the leaf step.  The entry count and the cull
// bound are two scalars the caller keeps - the walks keep them in the TravRay they carry anyway: best.tri is the count (the
// traversal reads best.tri only for closest-hit rays with a near-tie flag, which nothing here raises, and for any-hit rays,
// which these are not) and best.t the bound: the effective tmax until the list is full, then the last entry's th.
//
// CULLING.  trav_node_step enters a child when its entry distance does not exceed min(exit distance, best.t) - equality enters -
// on boxes widened by the batch pad; DESIGN.md section 4.17 has the argument why a candidate with th <= bound is never hidden.
// Rays from far origins (query_far) are walked with the boxes culled by geometry only (best.t stays +inf, the bound lives in a
// local), rays whose triangle test overflows (ray_overflows) meet every record (hits_scan).
#pragma once

#include "dev_trace.h"

namespace prt {

enum { HITS_MAX = 16 };

template <int BLOCK>
struct LdsHitList {
    int * col;
    PRT_D void attach(int * lds, unsigned int tid) { col = lds + tid; }
    PRT_D float t(unsigned int s) const { return as_f(col[(2u * s) * BLOCK]); }
    PRT_D unsigned int id(unsigned int s) const { return (unsigned int)col[(2u * s + 1u) * BLOCK]; }
    PRT_D void set(unsigned int s, float t, unsigned int id) const { col[(2u * s) * BLOCK] = as_i(t); col[(2u * s + 1u) * BLOCK] = (int)id; }
};

struct GlobalHitList {
    int * col;
    size_t stride;
    PRT_D void attach(int * base, size_t lane, size_t lanes) { col = base + lane; stride = lanes; }
    PRT_D float t(unsigned int s) const { return as_f(col[(size_t)(2u * s) * stride]); }
    PRT_D unsigned int id(unsigned int s) const { return (unsigned int)col[(size_t)(2u * s + 1u) * stride]; }
    PRT_D void set(unsigned int s, float t, unsigned int id) const { col[(size_t)(2u * s) * stride] = as_i(t); col[(size_t)(2u * s + 1u) * stride] = (int)id; }
};

// A ray's cursor: only candidates whose key is strictly greater remain.  group < 0: no cursor.
struct HitsCursor {
    float t;
    int group;
    unsigned int vertex0;
};
PRT_D HitsCursor hits_no_cursor() {
    HitsCursor c;
    c.t = 0.0f; c.group = -1; c.vertex0 = 0u;
    return c;
}

// (ta, group a, vertex0 a) < (tb, group b, vertex0 b).  t is compared as a float: a NaN on either side is false both ways.
PRT_D bool hits_key_less(float ta, uint2 a, float tb, uint2 b) {
    if (ta < tb) return true;
    if (ta != tb) return false;
    return a.x < b.x || (a.x == b.x && a.y < b.y);
}

PRT_D bool hits_after_cursor(const HitsCursor & c, float th, uint2 m) {
    if (c.group < 0) return true;
    return hits_key_less(c.t, make_uint2((unsigned int)c.group, c.vertex0), th, m);
}

// The record of leaf slot ti as the side the ray can meet it from: the record itself, or with BACK and dd < 0 the record
// (a, ac, ab, -n).  (dd = 0 and a NaN dd: neither side is a candidate, either form rejects.)
template <bool BACK>
PRT_D bool hits_side(const DevScene & sc, unsigned int ti, f3 qp, f3 & a, f3 & ab, f3 & ac, f3 & n) {
    const float4 * tp = reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(sc.tris) + ti * 48u);
    const float4 r0 = tp[0], r1 = tp[1], r2 = tp[2];
    a = mk3(r0.x, r0.y, r0.z); ab = mk3(r0.w, r1.x, r1.y); ac = mk3(r1.z, r1.w, r2.x); n = mk3(r2.y, r2.z, r2.w);
    if (BACK && dot3(qp, n) < 0.0f) {
        const f3 sw = ab;
        ab = ac; ac = sw;
        n = mk3(-n.x, -n.y, -n.z);
        return true;
    }
    return false;
}

// One record against the rule and into the list.  n: the entries so far, bound: tmax while n < k, then the last entry's th.
template <class LIST, bool BACK>
PRT_D void hits_offer(const DevScene & sc, const LIST & list, unsigned int k, unsigned int & n, float & bound, const HitsCursor & cur,
                      const uint2 * leaf_map, f3 o, f3 qp, unsigned int ti) {
    f3 a, ab, ac, nr;
    const bool back = hits_side<BACK>(sc, ti, qp, a, ab, ac, nr);
    float t, dd, v, w;
    if (!tri_geom(o, qp, a, ab, ac, nr, t, dd, v, w)) return;
    if (t > 3.402823466e+38f * dd) return;                                  // raytracer.cpp:104 against FLT_MAX
    const float th = t * (1.0f / dd);
    const bool full = n == k;
    // not full: the rule's th < tmax.  Full: the last entry is below tmax, and a candidate beyond it cannot enter; one that
    // equals it in th may, by the tie key
    if (full ? th > bound : !(th < bound)) return;
    const unsigned int id = ti << 1 | (back ? 1u : 0u);
    uint2 m = make_uint2(0u, 0u);
    bool have_m = false;
    if (cur.group >= 0) {
        m = leaf_map[ti]; have_m = true;
        if (!hits_after_cursor(cur, th, m)) return;
    }
    if (full && !(th < bound)) {                                            // th == bound
        if (!have_m) { m = leaf_map[ti]; have_m = true; }
        if (!hits_key_less(th, m, bound, leaf_map[list.id(k - 1u) >> 1])) return;
    }
    // the candidate's slot: behind every entry whose key is not greater.  An entry with the candidate's own key is the candidate
    // itself, met before - a walk may offer a record twice (the 8-wide tree under a wide pad: a node's empty slot passes the
    // box test and names the first triangle behind the node's own) - and the list holds a candidate once.
    const unsigned int end = full ? k - 1u : n;
    unsigned int s = end;
    while (s > 0u) {
        const float pt = list.t(s - 1u);
        if (pt < th) break;
        if (pt == th) {
            const unsigned int pid = list.id(s - 1u);
            if (pid == id) return;
            if (!have_m) { m = leaf_map[ti]; have_m = true; }
            if (!hits_key_less(th, m, pt, leaf_map[pid >> 1])) break;
        }
        --s;
    }
    // insert in order: entries above the candidate move up one slot, the last one of a full list drops out
    for (unsigned int j = end; j > s; --j) list.set(j, list.t(j - 1u), list.id(j - 1u));
    list.set(s, th, id);
    if (!full) ++n;
    if (n == k) bound = list.t(k - 1u);
}

// A ray at the root, as a closest-hit ray that takes no cones: best.t = the effective tmax, best.tri = 0 entries.
template <class STK>
PRT_D void hits_start(TravRay & r, f3 ob, f3 d, float tmax, float pad, const STK & stk) {
    trav_start<true>(r, ob, d, TRACE_CLOSEST | TRACE_NO_CONE, pad, stk);
    r.best.t = tmax;
    r.best.tri = 0;
}

// The leaf the walk holds, every triangle through hits_offer, then on to the next entry.  CULL: the bound is r.best.t, which
// the node steps cull against; else r.best.t stays where the caller put it (+inf) and the bound is `loose_bound`.
template <class STK, class LIST, bool BACK, bool COUNT, bool CULL>
PRT_D void hits_leaf(const DevScene & sc, TravRay & r, const STK & stk, TraceStats & st, const LIST & list, unsigned int k,
                     const HitsCursor & cur, const uint2 * leaf_map, float & loose_bound) {
    const f3 qp = r.o - (r.o + r.d);                 // raytracer.cpp:88-89, not bitwise -d
    unsigned int first, count;
    trav_leaf_range(r, first, count);
    if (COUNT) { if (first_active_lane()) st.wleaves++; }
    unsigned int n = (unsigned int)r.best.tri;
    for (unsigned int i = 0; i < count; ++i) {
        if (COUNT) { st.tris++; if (first_active_lane()) st.wtris++; }
        hits_offer<LIST, BACK>(sc, list, k, n, CULL ? r.best.t : loose_bound, cur, leaf_map, r.o, qp, first + i);
    }
    r.best.tri = (int)n;
    trav_leaf_next(r, stk);
}

// Whole-ray walk on a stack that cannot overflow (the slow path, and the host harness); returns the entries.
// CULL false: query_far's form, boxes culled by geometry only (query_any_unculled).
template <class STK, class LIST, bool BACK, bool COUNT, bool CULL>
PRT_D unsigned int hits_walk(const DevScene & sc, f3 ob, f3 d, float tmax, float pad, const STK & stk, TraceStats & st, const LIST & list,
                             unsigned int k, const HitsCursor & cur, const uint2 * leaf_map) {
    TravRay r;
    hits_start(r, ob, d, tmax, pad, stk);
    float loose = tmax;
    if (!CULL) r.best.t = __uint_as_float(0x7F800000u);
    for (;;) {
        while (trav_walking(r)) trav_node_step<STK, COUNT>(sc, r, stk, st, pad);
        if (trav_done(r)) break;
        hits_leaf<STK, LIST, BACK, COUNT, CULL>(sc, r, stk, st, list, k, cur, leaf_map, loose);
    }
    return (unsigned int)r.best.tri;
}

// Every record (ray_overflows, as scan_any_below); returns the entries.
template <class LIST, bool BACK, bool COUNT>
PRT_D unsigned int hits_scan(const DevScene & sc, f3 ob, f3 d, float tmax, TraceStats & st, const LIST & list, unsigned int k,
                             const HitsCursor & cur, const uint2 * leaf_map) {
    const f3 qp = ob - (ob + d);
    unsigned int n = 0u;
    float bound = tmax;
    for (unsigned int ti = 0; ti < sc.tri_count; ++ti) {
        if (COUNT) st.tris++;
        hits_offer<LIST, BACK>(sc, list, k, n, bound, cur, leaf_map, ob, qp, ti);
    }
    return n;
}

// What a slot reports.  hits_slot(s < n): the list's th, and v, w, group, vertex0 recomputed from the entry's record with the
// leaf step's expressions; a back hit's barycentrics in the order of the real corners.
struct HitSlot {
    float t, v, w;
    uint2 m;                         // (group, vertex0)
    unsigned int back;
};
PRT_D HitSlot hits_slot_miss() {
    HitSlot h;
    h.t = 3.402823466e+38f; h.v = h.w = 0.0f; h.m = make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu); h.back = 0u;
    return h;
}
template <class LIST>
PRT_D HitSlot hits_slot(const DevScene & sc, const LIST & list, const uint2 * leaf_map, f3 o, f3 qp, unsigned int s) {
    HitSlot h;
    const unsigned int id = list.id(s), ti = id >> 1;
    h.t = list.t(s);
    h.back = id & 1u;
    h.m = leaf_map[ti];
    f3 a, ab, ac, nr;
    const bool back = hits_side<true>(sc, ti, qp, a, ab, ac, nr);
    float t = 0.0f, dd = 1.0f, v = 0.0f, w = 0.0f;
    (void)tri_geom(o, qp, a, ab, ac, nr, t, dd, v, w);                      // true: the entry passed it in the leaf step
    const float ood = 1.0f / dd;
    h.v = back ? w * ood : v * ood;
    h.w = back ? v * ood : w * ood;
    return h;
}

}  // namespace prt
