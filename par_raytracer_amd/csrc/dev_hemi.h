// dev_hemi.h - the definition of prt_hemisphere_visibility (include/prt.h), written once for the kernels
// (kernels_hemi.h) and for the host (tests/hemi_host_harness.cpp, through tests/hip_shim).
//
//   SAMPLE (j, s)  of point j = first + i (j < 2^32), s < samples <= 65535:
//                  rng_seed(prt_sample_key(seed, j, s)); k = rng_next<false>() % 1024           hemi_index
//                  dir = tangent_to_world(normal, diffuse_dirs[k].xyz), the normal AS GIVEN     hemi_ray
//                  the ray (point, dir, ray_bias): its origin is biased as TraceRay biases it, point + dir * ray_bias, and it
//                  is a miss by definition under prt_trace_rays' rule (a non-finite component, a zero direction) - hemi_ray
//                  is then false and the sample counts as unoccluded.
//   POINT          invalid when a component of the point or of the normal is not finite, or the normal is all zeros
//                  (hemi_point_valid): no ray is cast.
//   SUMS           unoccluded = the number of s whose ray PRT_QUERY_OCCLUDED answers 0; B_c = the sum over those s of
//                  hemi_fix(dir_c) = (int64)rint((double)dir_c * 2^32), 0 for a component that is not finite (only a ray that
//                  is a miss by definition has one).  Integers: no order of summation changes them.
//   OUTPUTS        visibility = (float)unoccluded / (float)samples   hemi_visibility
//                  bent_c = (float)(((double)B_c * 2^-32) / (double)samples)   hemi_bent
#pragma once

#include "../../include/prt_key.h"
#include "dev_rng.h"
#include "dev_shade.h"

namespace prt {

// The table entry of sample s of point j: the first draw of the sample's own generator, modulo the table's 1024 entries.
PRT_HD unsigned int hemi_index(u64 seed, u32 j, u32 s) {
    Rng r;
    rng_seed(r, prt_sample_key(seed, j, s));
    return (unsigned int)(rng_next<false>(r, nullptr, 0) % 1024ull);
}

PRT_HD bool hemi_point_valid(f3 p, f3 n) {
    const bool finite = isfinite(p.x) && isfinite(p.y) && isfinite(p.z) && isfinite(n.x) && isfinite(n.y) && isfinite(n.z);
    return finite && !(n.x == 0.0f && n.y == 0.0f && n.z == 0.0f);
}

// The ray of (point, normal, table entry ts): d the direction, ob the origin biased as TraceRay does (raytracer.cpp:163).
// False for a ray that is a miss by definition (query_ray's rule, kernels_query.h).
PRT_D bool hemi_ray(f3 p, f3 n, f3 ts, float ray_bias, f3 & ob, f3 & d) {
    d = tangent_to_world(n, ts);
    ob = p + d * ray_bias;
    const bool finite = isfinite(d.x) && isfinite(d.y) && isfinite(d.z) && isfinite(ob.x) && isfinite(ob.y) && isfinite(ob.z);
    return finite && !(d.x == 0.0f && d.y == 0.0f && d.z == 0.0f);
}

// A direction component in 2^-32 fixed point: exact in the double, rounded to an integer once.
PRT_HD long long hemi_fix(float c) { return isfinite(c) ? (long long)rint((double)c * 4294967296.0) : 0ll; }

PRT_HD float hemi_visibility(unsigned int unoccluded, unsigned int samples) { return (float)unoccluded / (float)samples; }
PRT_HD float hemi_bent(long long B, unsigned int samples) { return (float)(((double)B * (1.0 / 4294967296.0)) / (double)samples); }

// One pass of a call holds whole points, at most `pass_items` samples of them (option HEMI_PASS_ITEMS, at least one point).
PRT_HD unsigned int hemi_pass_points(unsigned long long pass_items, unsigned int samples) {
    const unsigned long long cap = 1ull << 30;                              // wave_loop's item index is an int
    const unsigned long long items = pass_items < samples ? samples : pass_items > cap ? cap : pass_items;
    return (unsigned int)(items / samples);
}

}  // namespace prt
