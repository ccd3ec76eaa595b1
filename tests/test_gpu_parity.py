"""GPU parity: the HIP path (through the C ABI) against the reference's golden pixels and the CPU oracle.

Bar (BASELINE.json north_star): integer ray counts EQUAL, per-pixel RGB within 1e-4 of the reference CPU
renderer on the same scene / seed.  The tolerance exists only for device powf in the Phong highlight
(raytracer.cpp:388) - every control-flow decision is reproduced bit for bit.
"""
from __future__ import annotations

import numpy as np
import pytest

from conftest import camera_and_params, host_scene, load_golden

pytestmark = pytest.mark.gpu

TOL = 1e-4      # north_star: "per-pixel RGB within 1e-4 of the reference"

SMALL = ["c1_sphere_plane_256", "c2_cornell_128", "c2_cornell_512_l4", "cornell_point_light_d5",
         "icosphere_l3_two_lights", "terrain64_d3", "terrain192_d2", "many_materials_two_lights",
         # coplanar patches of different groups, decals 1-4 ulp off their wall, doubled faces, shared edges hit head-on: the
         # reference's sequential filter in ITS visit order decides these hits (raytracer.cpp:104, 149, 208-209, 220)
         "coincident_192x144_d3", "coincident_two_lights"]
BIG = ["c3_icosphere_1080p_l24", "c4_terrain1m_1080p_l40", "c5_terrain1m_4k_l120"]
TEXTURED = ["gallery_160x120", "gallery_two_lights_d4", "jpeg_gallery_128x96", "png_gallery_128x96", "bmp_gallery_128x96", "tga_gallery_128x96", "gif_gallery_128x96", "psd_gallery_128x96", "hdr_gallery_128x96", "pic_gallery_128x96",       # row N1: ambient / diffuse / specular / alpha / bump maps
            # the texture path at its edges (tests/texture_fixtures.py texture_edges): a 2 x 2 map, integer and negative texture
            # coordinates, alpha x texel across 0.05 and 1 (the holes decide the ray count), a two-channel Ks map, a tiled bump map
            "texture_edges_64x48", "texture_edges_point_light_64x48"]
ADAPTIVE = ["cornell_adaptive_4_16", "gallery_adaptive_10_50", "terrain64_adaptive_3_12_d4", "c4_terrain1m_adaptive_l60"]   # row N4


def _render_fixture(gpu_renderer_factory, name, pipeline=0):
    g = load_golden(name)
    r = gpu_renderer_factory(str(g["scene"]), int(g["light_mode"]))
    cam, p = camera_and_params(g, pipeline)
    img, ctr = r.render_lattice(cam, p, int(g["width"]), int(g["height"]), int(g["lattice"]))
    return g, img, ctr


PIPELINES = {"wavefront": 2, "pool": 4}


@pytest.mark.parametrize("pipeline", sorted(PIPELINES))
@pytest.mark.parametrize("name", SMALL + BIG)
def test_matches_reference_golden(gpu_renderer_factory, name, pipeline):
    g, img, ctr = _render_fixture(gpu_renderer_factory, name, PIPELINES[pipeline])
    ref = g["rgb"]
    assert img.shape[:2] == ref.shape[:2]
    assert np.all(img[:, :, 3] == 1.0)
    diff = np.abs(img[:, :, :3] - ref)
    n_bad = int((diff.max(axis=2) > TOL).sum())
    assert ctr.ray_count == int(g["ray_count"]), "ray_count %d != reference %d (max|d|=%g, %d px over tol)" % (
        ctr.ray_count, int(g["ray_count"]), diff.max(), n_bad)
    assert n_bad == 0 and diff.max() <= TOL, "max|dRGB| = %g, %d pixels over %g" % (diff.max(), n_bad, TOL)


@pytest.mark.parametrize("pipeline", ["wavefront", "pool"])
@pytest.mark.parametrize("name", TEXTURED)
def test_textured_scene_matches_reference_golden(gpu_renderer_factory, name, pipeline):
    """The texture path against the unmodified reference: bilinear lookups with the (size - 2) scale and flipped v,
    sRGB decode of all four channels, the specular map REPLACING Ks, alpha maps (holes pass the ray through with
    its bounce budget, the rest blends), bump-mapped normals that are not renormalised."""
    g, img, ctr = _render_fixture(gpu_renderer_factory, name, PIPELINES[pipeline])
    ref = g["rgb"]
    diff = np.abs(img[:, :, :3] - ref)
    n_bad = int((diff.max(axis=2) > TOL).sum())
    assert ctr.ray_count == int(g["ray_count"]), "ray_count %d != reference %d (max|d|=%g, %d px over tol)" % (
        ctr.ray_count, int(g["ray_count"]), diff.max(), n_bad)
    assert n_bad == 0 and diff.max() <= TOL, "max|dRGB| = %g, %d pixels over %g" % (diff.max(), n_bad, TOL)
    assert np.all(img[:, :, 3] == 1.0)


@pytest.mark.parametrize("name", ADAPTIVE)
def test_adaptive_sampling_matches_reference_golden(gpu_renderer_factory, name):
    """RenderPixel's adaptive loop (main.cpp:245-258) as the unmodified reference runs it, one RNG stream per pixel:
    equal ray counts mean every pixel took the same number of samples as on the CPU (the stopping rule compares a
    float variance with 0.01, so this also pins the per-sample colours to well inside the tolerance)."""
    g, img, ctr = _render_fixture(gpu_renderer_factory, name)
    assert ctr.pipeline == PIPELINES["pool"]
    ref = g["rgb"]
    diff = np.abs(img[:, :, :3] - ref)
    n_bad = int((diff.max(axis=2) > TOL).sum())
    assert ctr.ray_count == int(g["ray_count"]), "ray_count %d != reference %d (max|d|=%g, %d px over tol)" % (
        ctr.ray_count, int(g["ray_count"]), diff.max(), n_bad)
    assert n_bad == 0 and diff.max() <= TOL, "max|dRGB| = %g, %d pixels over %g" % (diff.max(), n_bad, TOL)
    assert np.all(img[:, :, 3] == 1.0)
    # verdicts of the stopping rule within 0.1 % of the threshold are the only ones the device's last bits could turn (include/prt.h
    # prt_params): rare - none on three of the fixtures, 2 of ~10^5 on the gallery - and not turned where they occur
    r = gpu_renderer_factory(str(g["scene"]), int(g["light_mode"]))
    assert r.render_stats().variance_close_calls <= 4


def test_adaptive_close_calls_are_counted():
    """prt_render_stats::variance_close_calls: a stopping-rule verdict whose variance lies within 0.1 % of the threshold (+1e-7) is
    counted.  A threshold of 1e-30 makes every pixel that sees only sky (all samples the background colour, variance exactly 0)
    such a verdict (at least one per sky pixel); the reference's 0.01 makes next to none; fixed spp has no verdicts at all."""
    from conftest import host_scene, scene_dir
    from par_raytracer_amd import api
    import oracle_py as orc
    s, _ = scene_dir("sphere_plane")
    hs = host_scene("sphere_plane", 0)
    w, h = 64, 48
    cam = api.make_camera(s.fov, w, h, s.camera_position, s.camera_facing)
    r = api.Renderer(0)
    try:
        r.upload(hs)
        calls = {}
        for thr in (1e-30, 0.01):
            p = api.default_params(3, 5, pipeline=PIPELINES["pool"], max_spp=9, variance_threshold=thr)
            ref, c_ref = orc.render(hs.desc, cam, p, w, h, 1, 8)
            img, c = r.render(cam, p, w, h)
            assert c.ray_count == c_ref.ray_count
            calls[thr] = int(r.render_stats().variance_close_calls)
        # (ref is the 0.01 render; the image's first pixel is sky: n + 1 samples of the background colour summed and divided by
        # n, main.cpp:253-262 - a multiple of it)
        bg = np.array(list(p.background_color)[:3], dtype=np.float32)
        ratio = ref[0, 0, :3] / bg
        assert ratio.max() - ratio.min() < 1e-5 and ratio[0] > 1.0
        sky = int((np.abs(ref[:, :, :3] - ref[0, 0, :3]).max(axis=2) < 1e-6).sum())
        assert sky > 50, "the camera was meant to see sky"
        assert calls[1e-30] >= sky and calls[0.01] <= 4, calls          # (at 0.01 one of this image's ~15,000 verdicts happens to be that close)
        img, c = r.render(cam, api.default_params(3, 5, pipeline=PIPELINES["pool"]), w, h)
        assert r.render_stats().variance_close_calls == 0
    finally:
        r.close()


def test_adaptive_sampling_shards_passes_and_refusals(gpu_renderer_factory, monkeypatch):
    g = load_golden("terrain64_adaptive_3_12_d4")
    r = gpu_renderer_factory(str(g["scene"]), int(g["light_mode"]))
    w, h = int(g["width"]), int(g["height"])
    cam, p = camera_and_params(g)
    full, c = r.render(cam, p, w, h)
    assert c.ray_count == int(g["ray_count"])
    from par_raytracer_amd import sharding
    frame = np.zeros((h, w, 4), dtype=np.float32)
    rays = 0
    for k in range(3):
        part, ck = r.render_shard(cam, p, w, h, 8, k, 3)
        frame[sharding.shard_row_list(h, 8, k, 3)] = part
        rays += ck.ray_count
    assert rays == c.ray_count
    # two lights: the two shadow contributions of a hit land in either order - the fixed-point accumulator does not care
    assert np.array_equal(frame.view(np.uint32), full.reshape(h, w, 4).view(np.uint32))
    r.set_option("PASS_SAMPLES", "700")
    again, c2 = r.render(cam, p, w, h)
    r.set_option("PASS_SAMPLES", None)
    assert c2.ray_count == c.ray_count and c2.trace_kernel_launches > 1
    assert np.array_equal(again.view(np.uint32), full.view(np.uint32))
    cam, p_wave = camera_and_params(g, PIPELINES["wavefront"])
    with pytest.raises(RuntimeError, match="adaptive sampling"):
        r.render(cam, p_wave, 16, 16)


def test_textured_scene_shards_passes_and_pipelines_agree(gpu_renderer_factory, monkeypatch):
    g = load_golden("gallery_160x120")
    r = gpu_renderer_factory(str(g["scene"]), 0)
    w, h = int(g["width"]), int(g["height"])
    cam, p_wave = camera_and_params(g, PIPELINES["wavefront"])
    cam, p_pool = camera_and_params(g, PIPELINES["pool"])
    a, ca = r.render(cam, p_wave, w, h)
    b, cb = r.render(cam, p_pool, w, h)
    assert ca.ray_count == cb.ray_count == int(g["ray_count"])
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "single light: both pipelines add in the same order"
    from par_raytracer_amd import sharding
    frame = np.zeros((h, w, 4), dtype=np.float32)
    for k in range(3):
        frame[sharding.shard_row_list(h, 8, k, 3)] = r.render_shard(cam, p_pool, w, h, 8, k, 3)[0]
    assert np.array_equal(frame.view(np.uint32), a.reshape(h, w, 4).view(np.uint32))
    r.set_option("PASS_SAMPLES", "2051")
    c, cc = r.render(cam, p_wave, w, h)
    r.set_option("PASS_SAMPLES", None)
    assert np.array_equal(a.view(np.uint32), c.view(np.uint32)) and cc.ray_count == ca.ray_count


def test_textured_scene_is_refused_by_the_experimental_pipelines(gpu_renderer_factory):
    from par_raytracer_amd import capi
    g = load_golden("gallery_160x120")
    r = gpu_renderer_factory(str(g["scene"]), 0)
    # MEGAKERNEL (1) and PERSISTENT (3) are reserved values of removed pipelines: the library refuses them
    for pipeline in (capi.PIPELINE_MEGAKERNEL, capi.PIPELINE_PERSISTENT):
        cam, p = camera_and_params(g, pipeline)
        with pytest.raises(RuntimeError, match="not built into this library"):
            r.render(cam, p, 16, 16)


@pytest.mark.parametrize("name", ["c2_cornell_128", "terrain64_d3"])
def test_full_frame_equals_pixel_list(gpu_renderer_factory, name):
    """prt_render (contiguous range) and prt_render_pixel_list give bit-identical pixels: a pixel's value
    is a pure function of (scene, camera, params, seed, pixel index)."""
    g = load_golden(name)
    if int(g["lattice"]) != 1:
        pytest.skip("needs a full-frame fixture")
    r = gpu_renderer_factory(str(g["scene"]), int(g["light_mode"]))
    cam, p = camera_and_params(g)
    w, h = int(g["width"]), int(g["height"])
    full, c1 = r.render(cam, p, w, h)
    lat, c2 = r.render_lattice(cam, p, w, h, 1)
    assert np.array_equal(full.reshape(h, w, 4).view(np.uint32), lat.view(np.uint32))
    assert c1.ray_count == c2.ray_count
    # split ranges reproduce the same bits
    half = (w * h) // 2 + 7
    a, ca = r.render(cam, p, w, h, 0, half)
    b, cb = r.render(cam, p, w, h, half, w * h)
    assert np.array_equal(np.concatenate([a, b]).view(np.uint32), full.view(np.uint32))
    assert ca.ray_count + cb.ray_count == c1.ray_count


def test_shards_reassemble_bit_identical(gpu_renderer_factory):
    """1-, 2-, 3- and 8-way interleaved row-block sharding reproduces the single-GPU frame bit for bit."""
    g = load_golden("c2_cornell_128")
    r = gpu_renderer_factory(str(g["scene"]), 0)
    cam, p = camera_and_params(g)
    w, h = int(g["width"]), int(g["height"])
    full, c_full = r.render(cam, p, w, h)
    full = full.reshape(h, w, 4)
    for nranks, block_rows in ((1, 8), (2, 8), (3, 5), (8, 8)):
        frame = np.zeros_like(full)
        rays = 0
        for rank in range(nranks):
            shard, c = r.render_shard(cam, p, w, h, block_rows, rank, nranks)
            rays += c.ray_count
            row = 0
            b = rank
            while b * block_rows < h:
                y0 = b * block_rows
                rows = min(block_rows, h - y0)
                frame[y0:y0 + rows] = shard[row:row + rows]
                row += rows
                b += nranks
            assert row == shard.shape[0]
        assert np.array_equal(frame.view(np.uint32), full.view(np.uint32)), "nranks=%d" % nranks
        assert rays == c_full.ray_count


def test_counting_variant_same_pixels(gpu_renderer_factory):
    from par_raytracer_amd import capi
    g = load_golden("terrain64_d3")
    r = gpu_renderer_factory(str(g["scene"]), 0)
    w, h = int(g["width"]), int(g["height"])
    cam, p = camera_and_params(g)
    a, ca = r.render(cam, p, w, h)
    cam, p2 = camera_and_params(g, pipeline=capi.FLAG_COUNT_VISITS)
    b, cb = r.render(cam, p2, w, h)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert ca.ray_count == cb.ray_count and cb.node_visits > 0 and cb.tri_tests > 0 and ca.node_visits == 0


@pytest.mark.parametrize("pipeline", sorted(PIPELINES))
def test_multi_pass_rendering_is_invisible(gpu_renderer_factory, pipeline, monkeypatch):
    """Calls whose per-sample workspace would not fit are rendered in passes of whole pixels (4K x 64 spp = 530 M
    samples needs them); forced here with a tiny pass size: full frame, a row shard and a pixel list must not change."""
    g = load_golden("terrain64_d3")
    r = gpu_renderer_factory(str(g["scene"]), 0)
    cam, p = camera_and_params(g, PIPELINES[pipeline])
    w, h = int(g["width"]), int(g["height"])
    px = np.arange(7, w * h, 13, dtype=np.uint32)
    ref, c_ref = r.render(cam, p, w, h)
    ref_shard, cs_ref = r.render_shard(cam, p, w, h, 8, 1, 3)
    ref_px, cp_ref = r.render_pixels(cam, p, w, h, px)
    r.set_option("PASS_SAMPLES", str(150 * int(p.spp) + 3))
    got, c_got = r.render(cam, p, w, h)
    got_shard, cs_got = r.render_shard(cam, p, w, h, 8, 1, 3)
    got_px, cp_got = r.render_pixels(cam, p, w, h, px)
    r.set_option("PASS_SAMPLES", None)
    assert len(px) > 300, "several passes of 128 pixels each, also for the pixel list"
    assert np.array_equal(ref.view(np.uint32), got.view(np.uint32)) and c_ref.ray_count == c_got.ray_count
    assert np.array_equal(ref_shard.view(np.uint32), got_shard.view(np.uint32)) and cs_ref.ray_count == cs_got.ray_count
    assert np.array_equal(ref_px.view(np.uint32), got_px.view(np.uint32)) and cp_ref.ray_count == cp_got.ray_count
    assert c_got.shaded_hits == c_ref.shaded_hits
    if pipeline != "wavefront":
        assert c_got.trace_kernel_launches > c_ref.trace_kernel_launches == 1


@pytest.mark.parametrize("name", ["cornell_box", "sphere_plane", "icosphere_l3", "terrain_64", "terrain_192", "textured_gallery"])
def test_gpu_lbvh_tree_is_conservative_and_complete(name):
    """Row N3: the radix tree built on the device (Morton sort + Karras hierarchy + bottom-up fit), pushed through the same
    4-wide / quantise back end: every triangle inside every ancestor's box and in exactly one leaf."""
    import ctypes as C
    from conftest import host_scene
    from par_raytracer_amd import api, capi
    hs = host_scene(name)
    r = api.Renderer(0)
    try:
        out = (C.c_uint64 * 6)()
        assert capi.hip_lib().prt_debug_check_bvh_lbvh(r._ctx, hs.desc, out) == 0, capi.hip_lib().prt_last_error(r._ctx)
        violations, nodes, depth, bound, leaves, refs = list(out)
        assert violations == 0
        assert refs == hs.n_tris and leaves >= hs.n_tris / 4
    finally:
        r.close()


@pytest.mark.parametrize("name", ["terrain64_d3", "gallery_160x120", "many_materials_two_lights", "c2_cornell_128"])
def test_gpu_lbvh_renders_the_same_image(name, monkeypatch):
    """Any conservative tree gives the same closest hits: with PRT_BVH_BUILDER=lbvh the fixtures still match the reference."""
    from conftest import host_scene
    from par_raytracer_amd import api
    g = load_golden(name)
    hs = host_scene(str(g["scene"]), int(g["light_mode"]))
    monkeypatch.setenv("PRT_BVH_BUILDER", "lbvh")
    r = api.Renderer(0)
    try:
        r.upload(hs)
        monkeypatch.delenv("PRT_BVH_BUILDER")
        cam, p = camera_and_params(g)
        img, ctr = r.render_lattice(cam, p, int(g["width"]), int(g["height"]), int(g["lattice"]))
    finally:
        r.close()
    assert ctr.ray_count == int(g["ray_count"])
    assert np.abs(img[:, :, :3] - g["rgb"]).max() <= TOL


@pytest.mark.parametrize("rule", ["dp", "greedy"])
@pytest.mark.parametrize("name", ["terrain192_d2", "gallery_160x120", "icosphere_l3_two_lights", "c2_cornell_128"])
def test_either_collapse_rule_renders_the_same_image(name, rule, monkeypatch):
    """PRT_BVH_COLLAPSE=dp / greedy (the binary tree collapsed into wide nodes by dynamic programming, the 8-wide tree's default,
    or by opening the largest child first): two conservative trees over the same triangles, so the fixtures match the reference
    either way, on both production pipelines."""
    from conftest import host_scene
    from par_raytracer_amd import api
    g = load_golden(name)
    hs = host_scene(str(g["scene"]), int(g["light_mode"]))
    monkeypatch.setenv("PRT_BVH_COLLAPSE", rule)
    r = api.Renderer(0)
    try:
        info = r.upload(hs)
        monkeypatch.delenv("PRT_BVH_COLLAPSE")
        for pl in (PIPELINES["pool"], PIPELINES["wavefront"]):
            cam, p = camera_and_params(g, pl)
            img, ctr = r.render_lattice(cam, p, int(g["width"]), int(g["height"]), int(g["lattice"]))
            assert ctr.ray_count == int(g["ray_count"])
            assert np.abs(img[:, :, :3] - g["rgb"]).max() <= TOL
    finally:
        r.close()


def _random_configs():
    rng = np.random.default_rng(20241003)
    scenes_ = ["cornell_box", "sphere_plane", "icosphere_l3", "terrain_64", "many_materials", "textured_gallery"]
    out = []
    for i in range(18):
        sc = scenes_[i % len(scenes_)]
        cfg = dict(scene=sc, light_mode=int(rng.integers(0, 3)), depth=int(rng.integers(0, 7)), rs=int(rng.integers(0, 4)),
                   ss=int(rng.integers(0, 4)), spp=int(rng.integers(1, 6)), seed=int(rng.integers(0, 2 ** 62)),
                   w=int(rng.integers(17, 70)), h=int(rng.integers(11, 50)), adaptive=int(rng.integers(0, 3) == 0))
        out.append(cfg)
    return out


@pytest.mark.parametrize("cfg", _random_configs(), ids=lambda c: "%s-d%d-r%d-s%d-l%d-%s" % (c["scene"], c["depth"], c["rs"], c["ss"], c["light_mode"], "adapt" if c["adaptive"] else "fixed"))
def test_random_configurations_against_the_oracle(cfg):
    """Parameter corners the fixtures do not visit (depth 0..6, 0..3 diffuse / specular bounce samples, odd image sizes,
    point lights, adaptive mode with arbitrary bounds): every production pipeline that accepts the configuration must give
    the oracle's ray count and colours."""
    import oracle_py as orc
    from conftest import host_scene, scene_dir
    from par_raytracer_amd import api
    s, _ = scene_dir(cfg["scene"])
    hs = host_scene(cfg["scene"], cfg["light_mode"])
    cam = api.make_camera(s.fov, cfg["w"], cfg["h"], s.camera_position, s.camera_facing)
    max_spp = cfg["spp"] + 5 if cfg["adaptive"] else 0
    def params(pipeline):
        return api.default_params(cfg["spp"], cfg["seed"], bounce_depth=cfg["depth"], reflection_samples=cfg["rs"],
                                  spec_samples=cfg["ss"], pipeline=pipeline, max_spp=max_spp)
    ref, c_ref = orc.render(hs.desc, cam, params(0), cfg["w"], cfg["h"], 1, 8)
    r = api.Renderer(0)
    try:
        r.upload(hs)
        for name in (["pool"] if cfg["adaptive"] else ["pool", "wavefront"]):
            img, c = r.render(cam, params(PIPELINES[name]), cfg["w"], cfg["h"])
            assert c.ray_count == c_ref.ray_count, "%s: ray count %d != oracle %d" % (name, c.ray_count, c_ref.ray_count)
            d = np.abs(img.reshape(cfg["h"], cfg["w"], 4)[:, :, :3] - ref[:, :, :3])
            assert d.max() <= TOL, "%s: max|dRGB| = %g" % (name, d.max())
    finally:
        r.close()


@pytest.mark.parametrize("scene", ["cornell_box", "terrain_64", "many_materials"])      # the last one has translucent materials: the general adaptive kernel
def test_adaptive_stopping_rule_at_thresholds_among_the_pixels_variances(scene):
    """The stopping rule (main.cpp:190-222, 253-257) is decided from a lower bound on the variance where that bound clears the
    threshold, and by the reference's loop over the stored samples otherwise (kernels_pool.h finalise step).  Thresholds
    spread over the range of the pixels' variances put pixels on either side of it and close to it: every verdict shows in
    the ray count, which must be the oracle's."""
    import oracle_py as orc
    from conftest import host_scene, scene_dir
    from par_raytracer_amd import api
    s, _ = scene_dir(scene)
    hs = host_scene(scene, 0)
    w, h = 48, 36
    cam = api.make_camera(s.fov, w, h, s.camera_position, s.camera_facing)
    r = api.Renderer(0)
    try:
        r.upload(hs)
        stopped_early = []
        for thr in (1e-4, 0.01, 0.1, 0.5, 2.0, 8.0, 40.0, 1e4):
            p = api.default_params(3, 77, pipeline=PIPELINES["pool"], max_spp=14, variance_threshold=thr)
            ref, c_ref = orc.render(hs.desc, cam, p, w, h, 1, 8)
            img, c = r.render(cam, p, w, h)
            assert c.ray_count == c_ref.ray_count, "threshold %g: ray count %d != oracle %d" % (thr, c.ray_count, c_ref.ray_count)
            assert np.abs(img.reshape(h, w, 4)[:, :, :3] - ref[:, :, :3]).max() <= TOL
            stopped_early.append(c.ray_count)
        assert len(set(stopped_early)) >= 4, "the thresholds were meant to split the pixels differently: %r" % (stopped_early,)
    finally:
        r.close()


def test_default_pipeline_try_out_is_invisible(gpu_renderer_factory):
    """PRT_PIPELINE_DEFAULT is the pool pipeline.  With PRT_FLAG_TRYOUT, between 1 M and 64 M samples the first DEFAULT
    call of a configuration renders the frame with both production pipelines and keeps the faster one: the image is the
    same whichever wins, later calls stick to it."""
    g = load_golden("terrain192_d2")
    r = gpu_renderer_factory(str(g["scene"]), 0)
    w, h = 640, 480                                               # x 4 spp = 1.23 M samples
    from par_raytracer_amd import api, capi
    cam = api.make_camera(float(g["fov"]), w, h, g["camera_position"], g["camera_facing"])
    plain, c0 = r.render(cam, api.default_params(4, 99), w, h)
    assert c0.pipeline == PIPELINES["pool"], "without the flag DEFAULT is the pool pipeline"
    p0 = api.default_params(4, 99, pipeline=capi.FLAG_TRYOUT)
    first, c1 = r.render(cam, p0, w, h)
    second, c2 = r.render(cam, p0, w, h)
    assert c1.pipeline in (PIPELINES["pool"], PIPELINES["wavefront"]) and c2.pipeline in (PIPELINES["pool"], PIPELINES["wavefront"])
    third, c3 = r.render(cam, p0, w, h)
    assert c3.pipeline == c2.pipeline, "the choice is kept"
    for name in ("pool", "wavefront"):
        img, c = r.render(cam, api.default_params(4, 99, pipeline=PIPELINES[name]), w, h)
        assert c.ray_count == c0.ray_count == c1.ray_count == c2.ray_count
        for other in (plain, first, second, third):
            assert np.array_equal(img.view(np.uint32), other.view(np.uint32))


@pytest.mark.parametrize("pipeline", sorted(PIPELINES))
def test_many_lights_and_materials_against_the_oracle(pipeline):
    """More lights (7) and materials (42) than the shading kernels stage in LDS (4 / 32), directional and point lights
    mixed: the global-table paths, one shadow queue slot per light, atomics for the shadow contributions.  The
    reference's InitScene only ever enables two lights, so this compares with the CPU oracle, which is pinned to the
    reference bit for bit on the one- and two-light fixtures of the same scene."""
    import ctypes as C
    import oracle_py as orc
    from conftest import host_scene
    from par_raytracer_amd import api, capi
    g = load_golden("many_materials_two_lights")
    hs = host_scene("many_materials", 1)
    base = hs.desc.contents
    n = 7
    lights = (capi.PrtLight * n)()
    rng = np.random.default_rng(3)
    for i in range(n):
        l = lights[i]
        l.type = i % 2                                        # directional, point, directional, ...
        col = rng.uniform(0.3, 1.0, size=3) * (1.5 if i % 2 == 0 else 6.0)
        l.color = (C.c_float * 4)(float(col[0]), float(col[1]), float(col[2]), 1.0)
        f = rng.normal(size=3); f[1] = -abs(f[1]) - 0.5; f /= np.linalg.norm(f)
        l.facing = (C.c_float * 3)(*[float(np.float32(v)) for v in f])
        l.position = (C.c_float * 3)(float(rng.uniform(-4, 4)), float(rng.uniform(3, 7)), float(rng.uniform(-2, 6)))
        l.falloff = float(rng.uniform(2.0, 5.0))
    desc = capi.PrtSceneDesc()
    C.memmove(C.byref(desc), C.byref(base), C.sizeof(desc))
    desc.lights = C.cast(lights, C.POINTER(capi.PrtLight))
    desc.light_count = n
    w, h = 64, 48
    cam, p = camera_and_params(g, PIPELINES[pipeline])
    cam = api.make_camera(float(g["fov"]), w, h, g["camera_position"], g["camera_facing"])
    ref, c_ref = orc.render(C.pointer(desc), cam, p, w, h, 1, 8)
    r = api.Renderer(0)
    try:
        r.upload(C.pointer(desc))
        img, ctr = r.render(cam, p, w, h)
        again, ctr2 = r.render(cam, p, w, h)
        other, ctr3 = r.render(cam, camera_and_params(g, PIPELINES["wavefront" if pipeline != "wavefront" else "pool"])[1], w, h)
    finally:
        r.close()
    assert ctr.ray_count == c_ref.ray_count
    diff = np.abs(img.reshape(h, w, 4)[:, :, :3] - ref[:, :, :3])
    assert diff.max() <= TOL, "max|dRGB| = %g" % diff.max()
    assert c_ref.ray_count > 10 * w * h, "seven shadow rays per hit"
    # The image is a pure function of (scene, seed, pixel) (include/prt.h): seven shadow rays per hit finish in any order and
    # their radiance lands in a fixed-point accumulator, so a second run gives the same bits, and so does the other
    # production pipeline, which processes the samples in a completely different order.
    assert ctr2.ray_count == ctr.ray_count == ctr3.ray_count
    assert np.array_equal(img.view(np.uint32), again.view(np.uint32))
    if pipeline in ("pool", "wavefront"):
        assert np.array_equal(img.view(np.uint32), other.view(np.uint32))


def test_default_pipeline_picks_by_size_and_both_agree(gpu_renderer_factory, monkeypatch):
    """PRT_PIPELINE_DEFAULT: the single-launch pool pipeline for small calls, the wavefront pipeline for large ones
    (prt_counters.pipeline says which ran); single-light scenes come out bit-identical either way."""
    g = load_golden("terrain64_d3")
    r = gpu_renderer_factory(str(g["scene"]), 0)
    w, h = int(g["width"]), int(g["height"])
    cam, p = camera_and_params(g)
    a, ca = r.render(cam, p, w, h)
    assert ca.pipeline == PIPELINES["pool"]
    r.set_option("POOL_MAX_SAMPLES", "0")
    b, cb = r.render(cam, p, w, h)
    r.set_option("POOL_MAX_SAMPLES", None)
    assert cb.pipeline == PIPELINES["wavefront"]
    assert ca.ray_count == cb.ray_count == int(g["ray_count"])
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("pipeline", sorted(PIPELINES))
def test_stack_overflow_falls_back_to_the_slow_stack(gpu_renderer_factory, pipeline, monkeypatch):
    """PRT_STACK_CAP=2 leaves room for the sentinel and one entry, so nearly every ray drops a push, is flagged
    and re-traced on the global stack: results must not change."""
    g = load_golden("terrain64_d3")
    r = gpu_renderer_factory(str(g["scene"]), 0)
    cam, p = camera_and_params(g, PIPELINES[pipeline])
    w, h = int(g["width"]), int(g["height"])
    ref, c_ref = r.render(cam, p, w, h)
    r.set_option("STACK_CAP", 2)
    got, c_got = r.render(cam, p, w, h)
    r.set_option("STACK_CAP", None)
    assert np.array_equal(ref.view(np.uint32), got.view(np.uint32))
    assert c_ref.ray_count == c_got.ray_count == int(g["ray_count"])


@pytest.mark.parametrize("name", ["terrain64_adaptive_3_12_d4", "cornell_adaptive_4_16", "gallery_adaptive_10_50"])
def test_adaptive_sampling_slow_paths(gpu_renderer_factory, name, monkeypatch):
    """Adaptive mode where nearly every ray takes the slow route (stack columns of two entries: closest-hit rays AND shadow
    rays are parked, so finalise steps are deferred to the EXACT launch and camera rays started ahead are called off), with
    park lists that start far too short, and with the EXACT kernel doing everything: always the reference's pixels and the
    reference's sample counts (equal ray counts)."""
    g = load_golden(name)
    r = gpu_renderer_factory(str(g["scene"]), int(g["light_mode"]))
    w, h, lat = int(g["width"]), int(g["height"]), int(g["lattice"])
    cam, p = camera_and_params(g)
    ref, c_ref = r.render_lattice(cam, p, w, h, lat)
    assert c_ref.ray_count == int(g["ray_count"])
    results = []
    r.set_option("STACK_CAP", 2)
    results.append(r.render_lattice(cam, p, w, h, lat))
    r.set_option("STACK_CAP", None)
    r.set_option("POOL_EXACT", 1)
    results.append(r.render_lattice(cam, p, w, h, lat))
    r.set_option("POOL_EXACT", None)
    for img, c in results:
        assert c.ray_count == c_ref.ray_count
        assert np.array_equal(img.view(np.uint32), ref.view(np.uint32))


def test_near_ties_park_lists_grow_and_the_exact_kernel_agrees(monkeypatch):
    """Coincident geometry on the pool pipeline: the fast kernel parks every ray whose hit has company within a few ulp and
    the EXACT launch that follows decides them by the reference's visit order (dev_trace.h).  Three ways to the same bits:
    the normal route; park lists that start far too short (the frame is rendered again with longer ones); the EXACT kernel
    rendering everything by itself.  And with stack columns of two entries nearly every ray of the frame - shadow rays
    included - takes the slow route."""
    from par_raytracer_amd import api
    g = load_golden("coincident_192x144_d3")
    w, h = int(g["width"]), int(g["height"])
    cam, p = camera_and_params(g, PIPELINES["pool"])
    hs = host_scene(str(g["scene"]), 0)

    def render():
        r = api.Renderer(0)
        try:
            r.upload(hs)
            return r.render(cam, p, w, h)
        finally:
            r.close()

    ref, c_ref = render()
    assert c_ref.ray_count == int(g["ray_count"])
    assert np.abs(ref.reshape(h, w, 4)[:, :, :3] - g["rgb"]).max() <= TOL
    monkeypatch.setenv("PRT_POOL_PARK_CAP", "8")
    small, c_small = render()
    monkeypatch.setenv("PRT_STACK_CAP", "2")
    tiny, c_tiny = render()
    monkeypatch.delenv("PRT_STACK_CAP")
    monkeypatch.delenv("PRT_POOL_PARK_CAP")
    monkeypatch.setenv("PRT_POOL_EXACT", "1")
    exact, c_exact = render()
    monkeypatch.delenv("PRT_POOL_EXACT")
    for img, c in ((small, c_small), (tiny, c_tiny), (exact, c_exact)):
        assert c.ray_count == c_ref.ray_count
        assert np.array_equal(img.view(np.uint32), ref.view(np.uint32))


@pytest.mark.parametrize("pipeline", ["wavefront", "pool"])
@pytest.mark.parametrize("scene,frame", [("cornell_box", "c2_cornell_128"), ("textured_gallery", "gallery_160x120"),
                                         ("terrain_64", "terrain64_d3")])
def test_level1_dropin_reference_flattened_scene(scene, frame, pipeline):
    """The level-1 drop-in: a scene parsed, decoded and linked by the REFERENCE and flattened
    inside it by include/prt_flatten_ref.h (tests/golden/desc_<scene>.npz holds the resulting prt_scene_desc arrays,
    texels included) goes through prt_upload_scene / prt_render and must give the reference's own frame.  Nothing of this
    repository's loader, decoders or host mirror is involved."""
    from par_raytracer_amd import api
    d = load_golden("desc_" + scene)
    g = load_golden(frame)
    fd = api.FlatDesc({k: d[k] for k in d.files})
    r = api.Renderer(0)
    try:
        info = r.upload(fd)
        assert info.triangle_count == int(g["triangles"])
        cam, p = camera_and_params(g, PIPELINES[pipeline])
        img, ctr = r.render_lattice(cam, p, int(g["width"]), int(g["height"]), int(g["lattice"]))
    finally:
        r.close()
    diff = np.abs(img[:, :, :3] - g["rgb"])
    assert ctr.ray_count == int(g["ray_count"]), "ray_count %d != reference %d" % (ctr.ray_count, int(g["ray_count"]))
    assert diff.max() <= TOL, "max|dRGB| = %g" % diff.max()
