// kernels_rays.h - prt_render_rays on the device: the wavefront pipeline fed from the caller's rays instead of the camera.
//
//   k_rays_check     grid-stride reduction over the batch's rays, run FIRST: the largest |origin component| of the rays inside the
//                    domain (wave_max_to_word of dev_wave_reduce.h), the number of rays outside it and the first such ray's index
//                    - one atomic per wave each.  The host reads the three words and launches nothing else when a ray is outside
//                    (the stance of k_refit_bounds): a refused batch has rendered nothing.
//   k_raygen_rays    beside k_raygen (kernels_wave.h): one lane per ray.  Seeds the ray's generator with the key prt_render gives
//                    sample s of pixel first + i, makes - with PRT_RAYS_CAMERA_STREAM - the two draws RenderPixel spends on the
//                    jitter (main.cpp:238) and drops them, loads the caller's ray and writes the chain's first closest-hit queue
//                    and RNG state exactly as k_raygen does.  k_trace, k_trace_exact, k_shade and the resolve kernels take it from
//                    there; none of them knows where a primary ray came from.
//
// The DOMAIN (include/prt.h): every component of origin, direction and biased origin finite; |Dot(d, d) - 1| <= 2^-18 (k_query's
// criterion for the walk that is the reference's sphere-tree TraceRay, kernels_query.h query_replays); every |origin component|
// <= 64 x the scene's largest |coordinate| (its replay_beyond).  The directions are used as given.
//
// A ray's index in the caller's arrays is 64 bits wide everywhere: count x spp can pass 2^32.
#pragma once

#include "../../include/prt_key.h"
#include "dev_wave_reduce.h"
#include "wave_buffers.h"

namespace prt {

enum { RAYS_W_EXTENT = 0, RAYS_W_OUTSIDE = 1, RAYS_W_FIRST = 2, RAYS_WORDS = 3 };

struct RaysArgs {
    const float * origins;           // rays x 3 (device); ray e = i * spp + s is sample s of output i
    const float * directions;        // rays x 3
    unsigned long long n_rays;       // of the whole call
    float ray_bias;
    float origin_max;                // 64 x the scene's largest |coordinate|
    // [RAYS_W_EXTENT] low word: max |origin component| of the rays inside the domain, as float bits; [RAYS_W_OUTSIDE] rays outside
    // the domain; [RAYS_W_FIRST] the smallest index among them (the host sets it to all ones)
    unsigned long long * words;
    // k_raygen_rays
    unsigned int first;              // the key's pixel word of output 0 (the batch's `first`, below 2^32 whenever there is a ray)
    unsigned int camera_stream;      // PRT_RAYS_CAMERA_STREAM
};

// |v| is a finite number (false for NaN and the infinities)
PRT_HD bool rays_finite(float v) { return fabsf(v) <= 3.402823466e+38f; }

// Ray e as the caller gave it; true when it lies inside the domain.
PRT_HD bool rays_load(const RaysArgs & A, unsigned long long e, f3 & o, f3 & d) {
    const float * po = A.origins + 3ull * e, * pd = A.directions + 3ull * e;
    o = mk3(po[0], po[1], po[2]);
    d = mk3(pd[0], pd[1], pd[2]);
    const f3 ob = o + d * A.ray_bias;                                               // raytracer.cpp:163
    const bool finite = rays_finite(o.x) && rays_finite(o.y) && rays_finite(o.z) && rays_finite(d.x) && rays_finite(d.y) && rays_finite(d.z) &&
                        rays_finite(ob.x) && rays_finite(ob.y) && rays_finite(ob.z);
    const float l2 = dot3(d, d);
    const bool unit = l2 >= 1.0f - 3.814697265625e-6f && l2 <= 1.0f + 3.814697265625e-6f;      // query_replays' test
    const bool near = fmaxf(fmaxf(fabsf(o.x), fabsf(o.y)), fabsf(o.z)) <= A.origin_max;
    return finite && unit && near;
}

__global__ __launch_bounds__(256) void k_rays_check(RaysArgs A) {
    float m = 0.0f;
    unsigned int outside = 0u;
    unsigned long long first_bad = ~0ull;
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long e = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; e < A.n_rays; e += stride) {
        f3 o, d;
        if (rays_load(A, e, o, d)) {
            m = fmaxf(m, fmaxf(fmaxf(fabsf(o.x), fabsf(o.y)), fabsf(o.z)));
        } else {
            outside++;
            if (e < first_bad) first_bad = e;
        }
    }
    wave_max_to_word(reinterpret_cast<unsigned int *>(A.words + RAYS_W_EXTENT), m);
    for (int off = 32; off > 0; off >>= 1) {
        outside += (unsigned int)__shfl_xor((int)outside, off);
        const unsigned long long other = __shfl_xor(first_bad, off);
        if (other < first_bad) first_bad = other;
    }
    if ((threadIdx.x & 63u) == 0u && outside) {
        atomicAdd(A.words + RAYS_W_OUTSIDE, (unsigned long long)outside);
        atomicMin(A.words + RAYS_W_FIRST, first_bad);
    }
}

// ray_base: the index, in the caller's arrays, of the chain's sample 0 - (the pass's first output) x spp + the chain's first
// sample within the pass (B.sample_base).  Item order is ray order: no tiling, no work-order options, no pixel list.
template <bool RING>
__global__ __launch_bounds__(256) void k_raygen_rays(RaysArgs A, DevParams P, WaveBuffers B, unsigned long long ray_base) {
    const unsigned int sid = blockIdx.x * blockDim.x + threadIdx.x;
    if (sid >= B.n_samples) return;
    const unsigned long long e = ray_base + sid;
    if (e >= A.n_rays) return;                                     // never: the chains of a call cover its rays exactly
    const unsigned int pixel = A.first + (unsigned int)(e / P.spp);
    const unsigned int samp = (unsigned int)(e % P.spp);
    Rng rng;
    rng_seed(rng, prt_sample_key(P.seed, pixel, samp));
    u64 * ring = RING ? B.ring + (size_t)sid * B.ring_step : nullptr;
    if (A.camera_stream) {
        // Vector2 sample_offset(NextFloat11, NextFloat11) of RenderPixel: made through the ring, so that draw 16 finds draw 0's
        // word where it looks for it, and dropped
        (void)rng_float11<RING>(rng, ring, B.ring_stride);
        (void)rng_float11<RING>(rng, ring, B.ring_stride);
    }
    f3 o, d;
    (void)rays_load(A, e, o, d);
    B.rng[sid] = make_ulonglong2(rng.chain, rng.prev);
    if (RING) B.rng_aux[sid] = make_ulonglong2(rng.seed0, (u64)rng.k);
    B.rq_o[0][sid] = make_float4(o.x, o.y, o.z, __int_as_float((int)sid));
    B.rq_d[0][sid] = make_float4(d.x, d.y, d.z, __int_as_float((int)WF_PENDING_FRESH_BIT << 8));
    B.rq_t[0][sid] = make_float4(1.0f, 1.0f, 1.0f, 0.0f);
}

}  // namespace prt
