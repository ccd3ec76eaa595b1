// wave_buffers.h - the wavefront pipeline's per-chain arrays and the words its queue entries carry: what kernels_wave.h and
// kernels_rays.h (ray generation from the caller's arrays) both write.  Nothing here needs a device: tests compile it with g++.
#pragma once

#include "dev_rng.h"
#include "dev_scene.h"

namespace prt {

enum { WF_KIND_CLOSEST = 0, WF_KIND_SHADOW_ANY = 1, WF_KIND_SHADOW_DIST = 2 };
enum { WF_STAGE_REFL = 0, WF_STAGE_SPEC = 1, WF_STAGE_ALPHA = 2, WF_STAGE_DONE = 3 };
// In a closest-hit list entry's `pending` field (24 bits; the low 17 are the levels with a parked frame): this is the FIRST
// closest-hit ray of its sample, so the sample's radiance record holds nothing yet - the shading lane does not read it and
// writes it whatever it adds (no zero fill when the sample is fetched, no read at its first hit: 56 bytes per sample).
enum { WF_PENDING_FRESH_BIT = 0x400000 };
// ... and: this ray is a LEAF that flies beside its sample's walk (emitters with FORKS, see shade_entry_on's fork step).  It
// entered at the last level, so its hit spawns nothing and draws nothing: its shade event adds its radiance and ends.  The bit
// travels with the entry through the trace phase, the park list and the adopting launch (0x800000 is k_pool's
// POOL_SPEC_PENDING_BIT, bits 0..16 the level mask).
enum { WF_PENDING_LEAF_BIT = 0x200000 };

struct WaveBuffers {
    Accum * accum;               // [N] per-sample radiance (xyz), fixed point (dev_scene.h)
    ulonglong2 * rng;            // [N] (chain, prev)
    ulonglong2 * rng_aux;        // [N] (seed0, k)            RING only
    u64 * ring;                  // RING only: a sample's 16 slots at ring[sample * ring_step + slot * ring_stride].  Fixed spp:
                                 // [16][N] (step 1, stride N) - the lanes of a wave are consecutive samples making the same
                                 // draw, one run of 8-byte words.  Adaptive mode: [N][16] (step 16, stride 1) - the lanes are
                                 // pixels at different draws, and a pixel's slots share one 128-byte line
                                 // (profiles/r02_experiments.txt item 17)
    unsigned int ring_step, ring_stride;
    float4 * frames;             // [levels][FR4][N] pending frames
    float4 * rq_o[2];            // closest-hit queues, double buffered: (o.xyz, sample)
    float4 * rq_d[2];            //                                      (d.xyz, level | pending_mask << 8)
    float4 * rq_t[2];            //                                      (throughput.xyz, -)
    float4 * hits;               // [N] (t, v, w, tri) by queue position
    float4 * sq_o;               // shadow queue: (o.xyz, sample)
    float4 * sq_c;               //               (radiance if unoccluded .xyz, w): w >= 0: point light, w = distance^2 to
                                 //               it (raytracer.cpp:393-396); w < 0: directional light number -w - 1, whose
                                 //               direction comes from the light table - no per-ray copy of a constant
    float4 * sq_d;               //               (d.xyz, -)   written and read for point lights only
    unsigned int * counts;       // [0] next closest count, [1] next shadow count, [2] trace fetch head, [3] rays handed to k_trace_exact, [4] shadow rays of this round's hits that were counted, not traced
    unsigned int * overflow;     // ray indices whose hit has a near tie or whose stack overflowed (traced again, exactly, by k_trace_exact)
    unsigned int n_samples;      // samples of THIS chain (all per-sample arrays are indexed 0 .. n_samples)
    unsigned int sample_base;    // global id of its first sample (pixel / key derivation only)
};

}  // namespace prt
