"""Normal cones on the GPU (include/prt.h "Normal cones", option NORMAL_CONES, read at upload): a closest-hit ray does not
descend into a 4-wide node whose triangles all face away from it.  Nothing that is rendered or counted may change, so every case
renders on TWO renderers, one uploaded with NORMAL_CONES=1 and one with 0, plain and counting: the frames must be the same bits,
ray_count and shaded_hits equal, cone_culled_nodes 0 with the option off; where nodes were culled tri_tests must be strictly lower
and node_visits no higher, where none were both must be equal (so that no case passes because the switch does nothing).

Scenes: terrain_64, icosphere_l3, the Cornell box, `coincident`, and the textured gallery.  Schedules: those of
tests/test_gpu_shadow_trees.py and POOL_FORK=0; depth 8; adaptive.  Then the queries (which ignore cones), prt_render_rays with
the longest directions its domain admits, a directional light whose facing has length 2, calls outside the bounds, prt_update_geometry, and the
module once more on the 8-wide library, which carries no cones."""
from __future__ import annotations

import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, host_scene, scene_dir
from test_gpu_shadow_trees import SCHEDULES, POOL, WAVEFRONT, upload_desc

#         id            scene key    w    h  spp depth
CASES = [("terrain", "terrain_64", 320, 180, 2, 2),
         ("icosphere", "icosphere_l3", 160, 120, 2, 2),
         ("box", "cornell_box", 128, 128, 2, 2),
         ("ties", "coincident", 128, 72, 2, 2),
         ("gallery", "gallery_two_lights", 96, 72, 2, 2),
         ("terrain_deep", "terrain_64", 64, 36, 2, 8),
         ("icosphere_deep", "icosphere_l3", 64, 36, 2, 8)]
MUST_CULL = ("terrain_64", "icosphere_l3")
ALL_SCHEDULES = dict(SCHEDULES, pool_nofork=(POOL, {"POOL_FORK": 0}))
BVH8 = os.environ.get("PRT_HIP_LIB", "") == "libprt_hip_bvh8.so"          # the 8-wide library: no cones, the same frames

_RENDERERS = {}


@pytest.fixture(scope="module")
def renderers_of():
    """key -> ((renderer with cones, renderer without), ObjScene)."""
    from par_raytracer_amd import api

    def get(key):
        if key not in _RENDERERS:
            desc, s = upload_desc(key)
            pair = []
            for cones in (1, 0):
                r = api.Renderer(0)
                r.set_option("NORMAL_CONES", cones)
                r.upload(desc)
                pair.append(r)
            info = [r.normal_cones()["coned_nodes"] for r in pair]
            assert info[1] == 0 and (info[0] > 0) == (not BVH8), (key, info)
            _RENDERERS[key] = (tuple(pair), s)
        return _RENDERERS[key]

    yield get
    for pair, _ in _RENDERERS.values():
        for r in pair:
            r.close()
    _RENDERERS.clear()


def render_both(pair, render, pipeline, options, **kw):
    """{(cones, counting): (pixel bits, counters, render stats)}; render(r, params) -> (image, counters)."""
    from par_raytracer_amd import api, capi
    out = {}
    for cones, r in zip((1, 0), pair):
        try:
            for k, v in options.items():
                r.set_option(k, v)
            for counting in (False, True):
                p = api.default_params(pipeline=pipeline | (capi.FLAG_COUNT_VISITS if counting else 0), **kw)
                img, c = render(r, p)
                assert c.pipeline == pipeline
                out[cones, counting] = (np.ascontiguousarray(img).view(np.uint32).copy(), c, r.render_stats() if counting else None)
        finally:
            for k in options:
                r.set_option(k, None)
    return out


def assert_identical(got, what, must_cull=False, expect_none=False, same_tree=True):
    """The contract of the module's docstring; returns cone_culled_nodes of the counting render with cones.  same_tree=False: the
    two renderers walk different trees (a refitted one and a fresh build), so their visit counts say nothing about each other."""
    off = got[0, False]
    for k in got:
        assert np.array_equal(got[k][0], off[0]), "%s: frame of (NORMAL_CONES, counting) = %s differs" % (what, k)
        assert got[k][1].ray_count == off[1].ray_count > 0 and got[k][1].shaded_hits == off[1].shaded_hits, (what, k)
    (_, con, son), (_, coff, soff) = got[1, True], got[0, True]
    print(what, "culled", son.cone_culled_nodes, "node_visits off/on", coff.node_visits, con.node_visits, "tri_tests off/on", coff.tri_tests, con.tri_tests)
    assert soff.cone_culled_nodes == 0, what
    if not same_tree:
        pass
    elif son.cone_culled_nodes > 0:
        # (strictly fewer triangle tests where the scene must cull; elsewhere a handful of culled nodes may all have been nodes
        # whose leaves the ray would have missed anyway)
        assert con.tri_tests <= coff.tri_tests and con.node_visits <= coff.node_visits, (what, con.tri_tests, coff.tri_tests, con.node_visits, coff.node_visits)
        assert con.tri_tests < coff.tri_tests or not must_cull, (what, con.tri_tests, coff.tri_tests)
    else:
        assert con.tri_tests == coff.tri_tests and con.node_visits == coff.node_visits, what
    if must_cull and not BVH8:
        assert son.cone_culled_nodes > 0, what
    if expect_none or BVH8:
        assert son.cone_culled_nodes == 0, what
    return son.cone_culled_nodes


@pytest.mark.gpu
@pytest.mark.parametrize("schedule", list(ALL_SCHEDULES))
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_a_render_with_normal_cones_is_the_render_without(renderers_of, case, schedule):
    from par_raytracer_amd import api
    cid, key, w, h, spp, depth = case
    pair, s = renderers_of(key)
    cam = api.make_camera(s.fov, w, h, s.camera_position, s.camera_facing)
    pipeline, options = ALL_SCHEDULES[schedule]
    got = render_both(pair, lambda r, p: r.render(cam, p, w, h), pipeline, options, spp=spp, seed=77, bounce_depth=depth)
    assert_identical(got, "%s %s" % (cid, schedule), must_cull=key in MUST_CULL)


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["terrain_64", "icosphere_l3"])
def test_adaptive_sampling_with_normal_cones(renderers_of, key):
    from par_raytracer_amd import api
    pair, s = renderers_of(key)
    cam = api.make_camera(s.fov, 64, 64, s.camera_position, s.camera_facing)
    got = render_both(pair, lambda r, p: r.render(cam, p, 64, 64), POOL, {}, spp=10, seed=77, bounce_depth=2, max_spp=50)
    assert_identical(got, "%s adaptive 10..50" % key, must_cull=True)


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["terrain_64", "icosphere_l3", "coincident"])
def test_the_queries_ignore_the_cones(renderers_of, key):
    """prt_trace_rays, prt_closest_points and prt_signed_distance read the grid steps through the mask and never test a cone: the
    results and the node visits are those of the renderer without."""
    import radiance_cases as R
    pair, s = renderers_of(key)
    o, d, _ = R.make_rays(host_scene(key).arrays(), 512, 4, 909)
    o, d = np.ascontiguousarray(o.reshape(-1, 3)), np.ascontiguousarray(d.reshape(-1, 3))
    ext = float(np.abs(s.positions).max())
    pts = np.ascontiguousarray((o + d * np.float32(0.37 * ext)).astype(np.float32))
    for name, call in (("trace closest", lambda r: r.trace_rays(o, d, count_visits=True)),
                       ("trace occluded", lambda r: r.trace_rays(o, d, mode="occluded", count_visits=True)),
                       ("closest points", lambda r: r.closest_points(pts, count_visits=True)),
                       ("signed distance", lambda r: r.signed_distance(pts, count_visits=True))):
        a, b = call(pair[0]), call(pair[1])
        assert a["counters"].node_visits == b["counters"].node_visits > 0 and a["counters"].tri_tests == b["counters"].tri_tests, (key, name)
        for f in a:
            if isinstance(a[f], np.ndarray):
                assert np.array_equal(np.ascontiguousarray(a[f]).view(np.uint8), np.ascontiguousarray(b[f]).view(np.uint8)), (key, name, f)


@pytest.mark.gpu
def test_render_rays_along_the_longest_directions_the_domain_admits_takes_no_cone(renderers_of):
    """The caller's directions are used as given, and the domain admits |Dot(d, d) - 1| <= 2^-18: longer than the 1 + 2^-20 the
    cones' margin assumes of a direction the library normalised.  Such a call leaves the cones alone, whole.  (A direction of
    length 3 is outside the domain: the library refuses the batch, on either renderer.  prt_render_rays runs on the wavefront
    pipeline only.)"""
    pipeline = WAVEFRONT
    import radiance_cases as R
    from par_raytracer_amd import api
    pair, _ = renderers_of("terrain_64")
    o, d, _ = R.make_rays(host_scene("terrain_64").arrays(), 257, 4, 505)
    o = np.ascontiguousarray(o)
    with pytest.raises(RuntimeError, match="outside the domain"):
        pair[0].render_rays(o, np.ascontiguousarray((d * np.float32(3.0)).astype(np.float32)), api.default_params(spp=4, seed=77, pipeline=pipeline), first=3)
    d = np.ascontiguousarray((d * np.float32(1.0 + 1.5e-6)).astype(np.float32))
    got = render_both(pair, lambda r, p: r.render_rays(o, d, p, first=3), pipeline, {}, spp=4, seed=77, bounce_depth=2)
    assert_identical(got, "terrain render_rays, pipeline %d" % pipeline, expect_none=True)


@pytest.mark.gpu
def test_a_directional_light_whose_facing_has_length_2():
    """Its shadow rays run along facing * -1 as it stands: any-hit rays, which never take a cone - with SHADOW_TREES=0 they walk
    the scene's tree, cones and all."""
    from par_raytracer_amd import api, capi
    name = "terrain_64"
    s, _ = scene_dir(name)
    a = dict(api.desc_arrays(host_scene(name, 0).desc))
    lights = np.array(a["lights"], copy=True)
    sun = capi.PrtLight.from_buffer_copy(lights[:48].tobytes())
    assert sun.type == 0
    for k in range(3):
        sun.facing[k] *= 2.0
    lights[:48] = np.frombuffer(bytes(sun), dtype=np.uint8)
    a["lights"] = lights
    pair = (api.Renderer(0), api.Renderer(0))
    try:
        for cones, r in zip((1, 0), pair):
            r.set_option("NORMAL_CONES", cones)
            r.upload(api.FlatDesc(a))
        cam = api.make_camera(s.fov, 96, 54, s.camera_position, s.camera_facing)
        for pipeline in (POOL, WAVEFRONT):
            got = render_both(pair, lambda r, p: r.render(cam, p, 96, 54), pipeline, {"SHADOW_TREES": 0}, spp=2, seed=77, bounce_depth=2)
            assert_identical(got, "facing x2, pipeline %d" % pipeline, must_cull=True)
    finally:
        for r in pair:
            r.close()


@pytest.mark.gpu
def test_a_call_outside_the_bounds_takes_no_cone(renderers_of):
    """|ray_bias| beyond the scene's extent, or a camera more than 4 extents out: the margin of the cones does not cover the call's
    ray origins, and no node is culled."""
    from par_raytracer_amd import api
    pair, s = renderers_of("terrain_64")
    ext = float(np.abs(s.positions).max())
    near = api.make_camera(s.fov, 64, 36, s.camera_position, s.camera_facing)
    far_pos = [float(v) for v in (np.asarray(s.camera_position, dtype=np.float64) + np.array([0.0, 1.0, 0.0]) * 6.0 * ext)]
    far = api.make_camera(s.fov, 64, 36, far_pos, (0.0, -1.0, 0.05))

    def both(cam, bias):
        def render(r, p):
            if bias is not None:
                p.ray_bias = bias
            return r.render(cam, p, 64, 36)
        return render_both(pair, render, POOL, {}, spp=2, seed=77, bounce_depth=2)

    assert_identical(both(near, None), "near", must_cull=True)
    assert_identical(both(near, ext), "bias at the bound", must_cull=True)
    assert_identical(both(near, 1.5 * ext), "bias beyond the bound", expect_none=True)
    assert_identical(both(far, None), "camera 6 extents up", expect_none=True)


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["terrain_64", "icosphere_l3"])
def test_the_device_built_tree_takes_cones_too(key):
    """BVH_BUILDER=lbvh: the radix tree of the GPU builder goes through the same wide back end, and pack_scene attaches the cones
    to it like to the SAH tree's.  The frames are the cone-less renderer's, nodes are culled, and the queries agree."""
    from par_raytracer_amd import api
    desc, s = upload_desc(key)
    pair = (api.Renderer(0), api.Renderer(0))
    try:
        for cones, r in zip((1, 0), pair):
            r.set_option("BVH_BUILDER", "lbvh")
            r.set_option("NORMAL_CONES", cones)
            r.upload(desc)
        assert pair[1].normal_cones()["coned_nodes"] == 0 and (pair[0].normal_cones()["coned_nodes"] > 0) == (not BVH8)
        cam = api.make_camera(s.fov, 160, 90, s.camera_position, s.camera_facing)
        for pipeline in (POOL, WAVEFRONT):
            got = render_both(pair, lambda r, p: r.render(cam, p, 160, 90), pipeline, {}, spp=2, seed=77, bounce_depth=2)
            assert_identical(got, "%s lbvh, pipeline %d" % (key, pipeline), must_cull=True)
    finally:
        for r in pair:
            r.close()


@pytest.mark.gpu
def test_an_update_clears_the_cones():
    """prt_update_geometry refits every node and writes its grid steps afresh, mantissas zero: the frame equals a fresh upload's,
    nothing is culled on the updated scene, and the fresh upload has cones again."""
    from par_raytracer_amd import api
    name = "terrain_64"
    s, _ = scene_dir(name)
    a = dict(api.desc_arrays(host_scene(name, 0).desc))
    p = a["positions"].reshape(-1, 3).copy()
    ext = float((p.max(0) - p.min(0)).max())
    p = (p + np.float32(0.03 * ext) * np.sin(p[:, [1, 2, 0]] * np.float32(2.0 * np.pi / ext) + np.float32(0.7))).astype(np.float32)
    a["positions"] = p.reshape(-1)
    a["spheres"], a["sphere_group"] = np.zeros(0, np.uint8), np.zeros(0, np.int32)
    ra, rb = api.Renderer(0), api.Renderer(0)
    try:
        ra.upload(host_scene(name, 0))
        assert (ra.normal_cones()["coned_nodes"] > 0) == (not BVH8)
        ra.update_geometry(a["positions"])
        assert ra.normal_cones()["coned_nodes"] == 0
        rb.upload(api.FlatDesc(a))
        cam = api.make_camera(s.fov, 96, 54, s.camera_position, s.camera_facing)
        for pipeline in (POOL, WAVEFRONT):
            got = render_both((rb, ra), lambda r, q: r.render(cam, q, 96, 54), pipeline, {}, spp=2, seed=77, bounce_depth=2)
            assert_identical(got, "fresh upload against the updated scene, pipeline %d" % pipeline, must_cull=True, same_tree=False)
    finally:
        ra.close()
        rb.close()


@pytest.mark.gpu
def test_normal_cones_on_the_8_wide_library():
    """The module's render checks once more, in a child process that loads the 8-wide library (one library per process): the same
    frames, and no node culled."""
    if BVH8:
        return                                              # this IS that child
    if os.environ.get("PRT_HIP_LIB"):
        pytest.skip("the suite runs against %s: one library per process" % os.environ["PRT_HIP_LIB"])
    if not os.path.exists(os.path.join(ROOT, "par_raytracer_amd", "libprt_hip_bvh8.so")):
        pytest.skip("libprt_hip_bvh8.so not built (make hip-bvh8)")
    env = dict(os.environ, PRT_HIP_LIB="libprt_hip_bvh8.so")
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", "-k", "render_with_normal_cones or adaptive or update or device_built",
                          os.path.abspath(__file__)], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    tail = out.stdout.decode()[-3000:]
    assert out.returncode == 0 and " passed" in tail and "failed" not in tail, tail
