// radiance_oracle_harness.cpp - the CPU oracle's own TraceRayColor (oracle/prt_oracle.cpp, included unchanged) along a batch of
// the caller's rays: the expected answers of prt_render_rays (include/prt.h) for tests/radiance_cases.py's fixtures.
//
//   g++ -O2 -std=c++14 -fPIC -shared -ffp-contract=off -fno-strict-aliasing -pthread -Iinclude tests/radiance_oracle_harness.cpp \
//       -o radiance_oracle.so
//
// prt_radiance_oracle_batch   THE DEFINITION of prt.h: output i (global index first + i) owns rays i * spp .. i * spp + spp - 1; for
//     sample s: Random_Seed(prt_sample_key(seed, (uint32)(first + i), s)), with camera_stream two Random_NextFloat11 made and
//     dropped, then TraceRayColor(ray as given, bounce_depth, rng).  rgba_out[i] = (sum in sample order / spp, 1) as RenderPixel
//     divides.  Per output also the number of TraceRay calls its rays made (ray_count) and of hits TraceRayColor shaded
//     (shaded_hits: CountWalk below, which returns -2 unless it made TraceRayColor's TraceRay calls and triangle tests), per ray
//     whether the primary ray hit (primary_hit) and whether its walk crossed a hit that is not opaque - alpha below 1 after the
//     alpha map (translucent).
// prt_radiance_camera_rays    RenderPixel's jittered rays (main.cpp:237-240) of pixels [p0, p0 + n) of a width-wide frame, spp
//     samples each: Random_NextFloat11 twice, y first, then MakeCameraRay.
#include <algorithm>

#include "../oracle/prt_oracle.cpp"

namespace {

// TraceRayColor's CONTROL FLOW restated with the oracle's own functions - the roulette, TraceRay, the alpha test, ShadeLight, the
// children in their order - without its colours: what the oracle does not count (the hits TraceRayColor shades: prt_counters'
// shaded_hits) is counted here.  It proves itself on every output: its TraceRay calls must number what TraceRayColor's did.
struct Walk { uint64_t shaded; bool primary_known, primary_hit, translucent; };
void CountWalk(const Ctx & cx, Ray ray, s32 iters, Counters * dbg, RandomState * rng, Walk * w) {
    if (iters < 0 || (iters != (s32)cx.p.bounce_depth && Random_NextFloat01(rng) < 0.5f)) return;
    RaycastHit hit;
    const bool any = TraceRay(cx, ray, &hit, dbg);
    if (!w->primary_known) { w->primary_known = true; w->primary_hit = any; }
    if (!any) return;
    w->shaded++;
    const prt_scene_desc * s = cx.s;
    const prt_group & g = s->groups[hit.group];
    const prt_material & mat = s->materials[g.material];
    V3 hit_p = hit.position + hit.normal * cx.p.ray_bias;
    u32 idx = g.first_index + hit.vertex0;
    TexturedHit th;
    TexturedHitAlpha(s, mat, idx, hit.bw, th);
    if (th.alpha < 1.0f) w->translucent = true;
    if (th.alpha_tested && th.alpha <= 0.05f) {
        ray.origin = hit.position + ray.direction * cx.p.ray_bias * 2.0f;
        CountWalk(cx, ray, iters, dbg, rng, w);
        return;
    }
    TexturedHitShading(s, mat, idx, hit.bw, th);
    for (u32 i = 0; i < s->light_count; ++i) (void)ShadeLight(cx, s->lights[i], ray, th.normal, hit_p, mat.specular_intensity, dbg);
    if (iters > 0) {
        for (u32 samp = 0; samp < cx.p.reflection_samples; ++samp) {
            u32 series_i = (u32)(Random_Next(rng) % 1024);
            CountWalk(cx, GetDiffuseReflectionRay(hit_p, th.normal, Hammersley(series_i, 1024)), iters - 1, dbg, rng, w);
        }
        for (u32 samp = 0; samp < cx.p.spec_samples; ++samp)
            CountWalk(cx, GetSpecularReflectionRay(hit_p, th.normal, mat.specular_intensity, Hammersley(samp, cx.p.spec_samples)), iters - 1, dbg, rng, w);
    }
    if (th.alpha < 1.0f) {
        ray.origin = hit.position + ray.direction * cx.p.ray_bias * 2.0f;
        CountWalk(cx, ray, iters - 1, dbg, rng, w);
    }
}

void seed_ray(RandomState * rng, const prt_params * params, uint64_t first, uint32_t i, uint32_t samp, int camera_stream) {
    Random_Seed(rng, prt_sample_key(params->seed, (uint32_t)(first + i), samp));
    if (camera_stream) {
        (void)Random_NextFloat11(rng);
        (void)Random_NextFloat11(rng);
    }
}

}  // namespace

extern "C" int prt_radiance_oracle_batch(const prt_scene_desc * s, const prt_params * params, const float * origins, const float * dirs,
                                         uint32_t count, uint64_t first, int camera_stream, float * rgba_out, uint64_t * ray_count,
                                         uint64_t * shaded_hits, uint8_t * primary_hit, uint8_t * translucent, int threads) {
    if (!s || !params || !origins || !dirs || !rgba_out || !ray_count || !shaded_hits || !primary_hit || !translucent || !params->spp) return -1;
    std::vector<int> disagree((size_t)std::max(threads, 1), 0);
    if (threads < 1) threads = 1;
    const uint32_t spp = params->spp;
    auto work = [&](uint32_t lo, uint32_t hi, int tid) {
        Ctx cx;
        memset(&cx, 0, sizeof(cx));
        cx.s = s;
        cx.p = *params;
        for (uint32_t i = lo; i < hi; ++i) {
            Counters dbg, dbg_walk;
            memset(&dbg, 0, sizeof(dbg));
            memset(&dbg_walk, 0, sizeof(dbg_walk));
            uint64_t shaded = 0;
            V4 color = v4(0, 0, 0, 0);
            for (uint32_t samp = 0; samp < spp; ++samp) {
                const size_t e = (size_t)i * spp + samp;
                RandomState rng;
                seed_ray(&rng, params, first, i, samp, camera_stream);
                Ray ray;
                ray.origin = load3(origins + 3 * e);
                ray.direction = load3(dirs + 3 * e);
                color = color + TraceRayColor(cx, ray, (s32)params->bounce_depth, &dbg, &rng);
                seed_ray(&rng, params, first, i, samp, camera_stream);
                Walk w = { 0, false, false, false };
                CountWalk(cx, ray, (s32)params->bounce_depth, &dbg_walk, &rng, &w);
                primary_hit[e] = w.primary_hit ? 1 : 0;
                translucent[e] = w.translucent ? 1 : 0;
                shaded += w.shaded;
            }
            color = color / (float)spp;
            color.w = 1.0f;
            rgba_out[4 * (size_t)i] = color.x; rgba_out[4 * (size_t)i + 1] = color.y; rgba_out[4 * (size_t)i + 2] = color.z; rgba_out[4 * (size_t)i + 3] = color.w;
            ray_count[i] = dbg.ray_count;
            shaded_hits[i] = shaded;
            if (dbg_walk.ray_count != dbg.ray_count || dbg_walk.tri_tests != dbg.tri_tests) disagree[tid] = 1;
        }
    };
    std::vector<std::thread> pool;
    const uint32_t per = (count + (uint32_t)threads - 1) / (uint32_t)threads;
    for (int k = 0; k < threads; ++k) {
        const uint32_t lo = std::min(count, per * (uint32_t)k), hi = std::min(count, lo + per);
        if (lo < hi) pool.emplace_back(work, lo, hi, k);
    }
    for (std::thread & th : pool) th.join();
    for (int v : disagree)
        if (v) return -2;                              // CountWalk is not TraceRayColor's walk: its counts mean nothing
    return 0;
}

extern "C" int prt_radiance_camera_rays(const prt_camera * cam, uint64_t seed, uint32_t width, uint32_t p0, uint32_t n, uint32_t spp,
                                        float * origins, float * dirs) {
    if (!cam || !width || !spp || !origins || !dirs) return -1;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t pixel = p0 + i, x = pixel % width, y = pixel / width;
        for (uint32_t samp = 0; samp < spp; ++samp) {
            RandomState rng;
            Random_Seed(&rng, prt_sample_key(seed, pixel, samp));
            float off_y = Random_NextFloat11(&rng);               // main.cpp:238: the first draw lands in .y
            float off_x = Random_NextFloat11(&rng);
            V2 p = { (float)x + off_x * 0.5f, (float)y + off_y * 0.5f };
            const Ray ray = MakeCameraRay(cam, p);
            const size_t e = (size_t)i * spp + samp;
            origins[3 * e] = ray.origin.x; origins[3 * e + 1] = ray.origin.y; origins[3 * e + 2] = ray.origin.z;
            dirs[3 * e] = ray.direction.x; dirs[3 * e + 1] = ray.direction.y; dirs[3 * e + 2] = ray.direction.z;
        }
    }
    return 0;
}
