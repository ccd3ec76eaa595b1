// rays_host_harness.cpp - the two kernels of par_raytracer_amd/csrc/kernels_rays.h on the host, one lane at a time, before they
// ever run on a card: a stand-alone program built with g++ and -fsanitize=address,undefined through tests/hip_shim
// (tests/test_radiance_host.py builds and runs it).  Every array has exactly the size its owner would give it, so an index that is
// off by a pass's or a chain's base reads or writes outside a heap block and the sanitizer stops the program.
//
//   k_rays_check    over a valid batch and over one with rays outside the domain at known places: the three words.
//   k_raygen_rays   over a batch of 534 outputs x 3 rays in 3 passes (192, 192, 150 outputs) x 2 chains of uneven size (384 + 192,
//                   384 + 192, 384 + 66 samples - the split render_wavefront makes: chains start on a multiple of spp x 64), with and
//                   without the draw ring, with and without PRT_RAYS_CAMERA_STREAM: every queue entry is the caller's ray of the
//                   GLOBAL index, every generator the one seeded with (first + output, sample) and advanced as asked, and the
//                   lanes past the chain's end write nothing.
//
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -Itests/hip_shim -Ipar_raytracer_amd/csrc
//       tests/rays_host_harness.cpp -o /tmp/rays_host && /tmp/rays_host
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>            // tests/hip_shim: one lane at a time
// what kernels_rays.h needs beyond the shim (a wave of one lane: a shuffle returns what a lane with nothing to say holds - the
// identity of the reduction that type is used for: 0 for the maximum and the sum, all ones for the minimum)
static inline float __shfl_xor(float, int) { return 0.0f; }
static inline int __shfl_xor(int, int) { return 0; }
static inline unsigned long long __shfl_xor(unsigned long long, int) { return ~0ull; }
static inline unsigned int __float_as_uint(float f) { unsigned int v; memcpy(&v, &f, 4); return v; }
static inline unsigned int atomicMax(unsigned int * p, unsigned int v) { unsigned int o = *p; if (v > o) *p = v; return o; }
static inline unsigned long long atomicMin(unsigned long long * p, unsigned long long v) { unsigned long long o = *p; if (v < o) *p = v; return o; }

#include "kernels_rays.h"

using namespace prt;

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static double rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (double)(g_rng >> 11) / 9007199254740992.0; }

static void make_batch(size_t n_rays, std::vector<float> & o, std::vector<float> & d) {
    o.resize(3 * n_rays); d.resize(3 * n_rays);
    for (size_t e = 0; e < n_rays; ++e) {
        double v[3] = { rnd() - 0.5, rnd() - 0.5, rnd() - 0.5 };
        const double l = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        for (int k = 0; k < 3; ++k) { d[3 * e + k] = (float)(v[k] / l); o[3 * e + k] = (float)(rnd() * 20 - 10); }
    }
}

static void run_check(const RaysArgs & A, unsigned long long * words) {
    words[RAYS_W_EXTENT] = 0; words[RAYS_W_OUTSIDE] = 0; words[RAYS_W_FIRST] = ~0ull;
    blockDim.x = 1;
    gridDim.x = 5;                                    // a grid-stride loop of 5 one-lane waves
    for (blockIdx.x = 0; blockIdx.x < gridDim.x; ++blockIdx.x) k_rays_check(A);
    blockIdx.x = 0; gridDim.x = 1;
}

static int check_kernel() {
    const size_t n = 1001;
    std::vector<float> o, d;
    make_batch(n, o, d);
    unsigned long long words[RAYS_WORDS];
    RaysArgs A;
    memset(&A, 0, sizeof(A));
    A.origins = o.data(); A.directions = d.data(); A.n_rays = n; A.ray_bias = 0.001f; A.origin_max = 64.0f * 5.0f; A.words = words;
    run_check(A, words);
    float want = 0.0f, got;
    for (float v : o) want = std::max(want, fabsf(v));
    const unsigned int bits = (unsigned int)words[RAYS_W_EXTENT];
    memcpy(&got, &bits, 4);
    const bool clean_ok = got == want && words[RAYS_W_OUTSIDE] == 0 && words[RAYS_W_FIRST] == ~0ull && (words[RAYS_W_EXTENT] >> 32) == 0;
    // rays outside the domain: NaN origin, infinite direction, a direction too long and one too short, an origin too far
    std::vector<float> o2 = o, d2 = d;
    o2[3 * 777 + 1] = NAN;
    d2[3 * 500 + 0] = INFINITY;
    for (int k = 0; k < 3; ++k) { d2[3 * 333 + k] *= 1.00001f; d2[3 * 999 + k] *= 0.9999f; }
    o2[3 * 400 + 2] = 321.0f;
    A.origins = o2.data(); A.directions = d2.data();
    run_check(A, words);
    const bool bad_ok = words[RAYS_W_OUTSIDE] == 5 && words[RAYS_W_FIRST] == 333;
    // 320 = 64 x 5 itself is inside; the extent then reports it
    std::vector<float> o3 = o;
    o3[3 * 12] = -320.0f;
    A.origins = o3.data(); A.directions = d.data();
    run_check(A, words);
    const unsigned int bits3 = (unsigned int)words[RAYS_W_EXTENT];
    memcpy(&got, &bits3, 4);
    const bool edge_ok = words[RAYS_W_OUTSIDE] == 0 && got == 320.0f;
    A.ray_bias = INFINITY;                              // every component of o and d is finite, none of o + d * bias
    run_check(A, words);
    const bool bias_ok = words[RAYS_W_OUTSIDE] == n && words[RAYS_W_FIRST] == 0;
    printf("check | clean_ok %d bad_ok %d edge_ok %d bias_ok %d\n", (int)clean_ok, (int)bad_ok, (int)edge_ok, (int)bias_ok);
    return clean_ok && bad_ok && edge_ok && bias_ok ? 0 : 1;
}

// One chain of one pass, as chain_setup sizes it: every per-sample array holds exactly n_samples entries.
template <bool RING>
static unsigned int raygen_chain(const RaysArgs & A, const DevParams & P, unsigned int pass_base_px, unsigned int chain_base, unsigned int n_samples,
                                 unsigned long long * checked) {
    std::vector<ulonglong2> rng(RING ? 2 * (size_t)n_samples : n_samples, make_ulonglong2(7, 7));
    std::vector<u64> ring(RING ? 16 * (size_t)n_samples : 0, 0x77ull);
    std::vector<float4> q(3 * (size_t)n_samples, make_float4(-7, -7, -7, -7));
    WaveBuffers B;
    memset(&B, 0, sizeof(B));
    B.n_samples = n_samples; B.sample_base = chain_base;
    B.rng = rng.data(); B.rng_aux = RING ? rng.data() + n_samples : nullptr;
    B.ring = RING ? ring.data() : nullptr; B.ring_step = 1; B.ring_stride = n_samples;
    B.rq_o[0] = q.data(); B.rq_d[0] = q.data() + n_samples; B.rq_t[0] = q.data() + 2 * (size_t)n_samples;
    const unsigned long long ray_base = (unsigned long long)pass_base_px * P.spp + chain_base;
    blockDim.x = 1;
    gridDim.x = (n_samples + 255u) / 256u * 256u;       // the launch's lanes, the idle ones of the last block included
    for (blockIdx.x = 0; blockIdx.x < gridDim.x; ++blockIdx.x) k_raygen_rays<RING>(A, P, B, ray_base);
    blockIdx.x = 0; gridDim.x = 1;
    unsigned int bad = 0;
    for (unsigned int sid = 0; sid < n_samples; ++sid) {
        const unsigned long long e = ray_base + sid;
        Rng r;
        rng_seed(r, prt_sample_key(P.seed, A.first + (unsigned int)(e / P.spp), (unsigned int)(e % P.spp)));
        u64 slots[16];
        for (u64 & s : slots) s = 0x77ull;
        if (A.camera_stream) { (void)rng_float11<RING>(r, RING ? slots : nullptr, 1); (void)rng_float11<RING>(r, RING ? slots : nullptr, 1); }
        bool ok = rng[sid].x == r.chain && rng[sid].y == r.prev;
        if (RING) {
            ok = ok && rng[n_samples + sid].x == r.seed0 && rng[n_samples + sid].y == r.k;
            for (int k = 0; k < 16; ++k) ok = ok && ring[(size_t)k * n_samples + sid] == slots[k];
        }
        const float4 ro = q[sid], rd = q[n_samples + sid], rt = q[2 * (size_t)n_samples + sid];
        ok = ok && !memcmp(&ro, A.origins + 3 * e, 12) && !memcmp(&rd, A.directions + 3 * e, 12);
        ok = ok && __float_as_int(ro.w) == (int)sid && __float_as_int(rd.w) == ((int)WF_PENDING_FRESH_BIT << 8);
        ok = ok && rt.x == 1.0f && rt.y == 1.0f && rt.z == 1.0f && rt.w == 0.0f;
        if (!ok) bad++;
        ++*checked;
    }
    return bad;
}

template <bool RING>
static unsigned int raygen_batch(unsigned int camera_stream, unsigned long long * checked) {
    const unsigned int count = 534, spp = 3, pass_pixels = 192, n_chains = 2;
    std::vector<float> o, d;
    make_batch((size_t)count * spp, o, d);
    RaysArgs A;
    memset(&A, 0, sizeof(A));
    A.origins = o.data(); A.directions = d.data(); A.n_rays = (unsigned long long)count * spp;
    A.first = 0xFFFFFFFFu - count + 1u;                   // first + count = 2^32
    A.camera_stream = camera_stream;
    DevParams P;
    memset(&P, 0, sizeof(P));
    P.spp = spp; P.seed = 99;
    unsigned int bad = 0, uneven = 0;
    for (unsigned int p0 = 0; p0 < count; p0 += pass_pixels) {                // render_pixels_once's pass loop
        const unsigned int n_samples = std::min(pass_pixels, count - p0) * spp;
        const unsigned int unit = spp * 64u;                                    // render_wavefront's split
        const unsigned int per = (unsigned int)((((unsigned long long)n_samples + n_chains - 1) / n_chains + unit - 1) / unit * unit);
        unsigned int base = 0;
        for (unsigned int c = 0; c < n_chains; ++c) {
            const unsigned int n = c + 1 == n_chains ? n_samples - base : std::min(per, n_samples - base);
            if (c && n != base) uneven++;
            bad += raygen_chain<RING>(A, P, p0, base, n, checked);
            base += n;
        }
    }
    return bad + (uneven == 3 ? 0u : 1000000u);
}

int main() {
    int rc = check_kernel();
    for (unsigned int cs = 0; cs < 2; ++cs) {
        unsigned long long n0 = 0, n1 = 0;
        const unsigned int b0 = raygen_batch<false>(cs, &n0), b1 = raygen_batch<true>(cs, &n1);
        printf("raygen camera_stream %u | plain bad %u of %llu ring bad %u of %llu\n", cs, b0, n0, b1, n1);
        if (b0 || b1 || n0 != 1602 || n1 != 1602) rc = 1;
    }
    return rc;
}
