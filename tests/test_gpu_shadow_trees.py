"""Shadow trees on the GPU (include/prt.h "Shadow trees", option SHADOW_TREES): a directional light's any-hit shadow rays start
at a second tree that holds only the triangles they can hit.  Nothing that is rendered or counted may change, so every case
renders with SHADOW_TREES=1 and SHADOW_TREES=0 on ONE renderer: the frames must be the same bits, ray_count and shaded_hits
equal, and - counting renders - the elided shadow rays equal; node_visits must be strictly lower where the upload built a tree
(and equal where it built none, so that no case passes because the switch does nothing).

(Where the scene's own tree is a single node - the 12-triangle box on the 8-wide library - a walk cannot be shorter than its one
step: there node_visits must be equal and tri_tests strictly lower.)

Scenes: terrain_64 (slopes facing away from the sun; once more with the sun 7 degrees above the horizon), the Cornell box (6 of its 12 triangles face away), the box with two
directional lights and a point light, the textured gallery with two directional lights, a flat plane (the empty set: a tree of
one node), and `coincident` with its doubled and coplanar faces (near ties).  Schedules: the pool pipeline with block-shared
pools, with wave-private pools and with its EXACT kernel, the wavefront pipeline, and the pool pipeline with two-entry stack
columns and 8-entry park lists, where dropped pushes send shadow rays through k_pool_parked_shadows.  One adaptive case; one
case in which prt_update_geometry makes the trees stale; and the whole module once more on the 8-wide library."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, host_scene, scene_dir

POOL, WAVEFRONT = 4, 2

#         id            scene key    w    h  spp depth
CASES = [("terrain", "terrain_64", 320, 180, 2, 2),
         ("low_sun", "terrain_low_sun", 320, 180, 2, 2),
         ("box", "cornell_box", 128, 128, 4, 2),
         ("three_lights", "box_three_lights", 96, 96, 2, 2),
         ("gallery_two_lights", "gallery_two_lights", 96, 72, 2, 2),
         ("plane", "flat_plane", 160, 90, 2, 2),
         ("ties", "coincident", 128, 72, 2, 2)]
SCHEDULES = {
    "pool_shared": (POOL, {"POOL_SHARED": 1}),
    "pool_private": (POOL, {"POOL_SHARED": 0}),
    "pool_exact": (POOL, {"POOL_EXACT": 1}),
    "wavefront": (WAVEFRONT, {}),
    "pool_parked": (POOL, {"STACK_CAP": 2, "POOL_PARK_CAP": 8}),
}
# lights whose shadow rays must have a tree of their own, per scene key (light order: InitScene's)
# (None: whatever the size rule says; the box's third light is the point light.  The gallery's two lights have 188 and 190 of its
# 372 triangles as possible occluders, about half: both under the rule's 75 %)
BUILT = {"terrain_64": [1], "terrain_low_sun": [1], "cornell_box": [1], "box_three_lights": [1, None, 0], "gallery_two_lights": [1, 1], "flat_plane": [1], "coincident": [1]}


def _lights(*recs):
    from par_raytracer_amd import capi
    return np.concatenate([np.frombuffer(bytes(r), dtype=np.uint8) if isinstance(r, capi.PrtLight) else r for r in recs])


def upload_desc(key):
    """What Renderer.upload takes for a scene key, and the ObjScene its camera comes from."""
    from par_raytracer_amd import api, capi
    if key == "box_three_lights":
        # the two directional lights of light mode 1 and the point light of light mode 2
        a = dict(api.desc_arrays(host_scene("cornell_box", 1).desc))
        point = api.desc_arrays(host_scene("cornell_box", 2).desc)["lights"][-48:]
        a["lights"] = _lights(a["lights"], point)
        return api.FlatDesc(a), scene_dir("cornell_box")[0]
    if key == "terrain_low_sun":
        # the sun 7 degrees above the horizon: long shadows, and unoccluded shadow rays that skim over slopes facing away from it
        a = dict(api.desc_arrays(host_scene("terrain_64", 0).desc))
        sun = capi.PrtLight.from_buffer_copy(a["lights"][:48].tobytes())
        f = np.array([1.0, -0.12, 0.25]) / np.linalg.norm([1.0, -0.12, 0.25])
        sun.facing[0], sun.facing[1], sun.facing[2] = (float(np.float32(v)) for v in f)
        a["lights"] = _lights(sun)
        return api.FlatDesc(a), scene_dir("terrain_64")[0]
    if key == "gallery_two_lights":
        return host_scene("textured_gallery", 1), scene_dir("textured_gallery")[0]
    if key == "flat_plane":
        # terrain_64 pressed flat: every triangle faces the sun, no triangle can occlude (spheres of the old shape: dropped).
        # Tilted by 0.3 rad about z, so that the boxes of the scene's tree have a height and a shadow ray that starts on the
        # plane starts inside them: in the scene's tree it walks several levels, in the light's one node
        a = dict(api.desc_arrays(host_scene("terrain_64", 0).desc))
        p = a["positions"].reshape(-1, 3).copy()
        p[:, 1] = p[:, 0] * np.float32(np.sin(0.3))
        p[:, 0] = p[:, 0] * np.float32(np.cos(0.3))
        a["positions"] = p.reshape(-1)
        a["spheres"], a["sphere_group"] = np.zeros(0, np.uint8), np.zeros(0, np.int32)
        return api.FlatDesc(a), scene_dir("terrain_64")[0]
    return host_scene(key, 0), scene_dir(key)[0]


_RENDERERS = {}


@pytest.fixture(scope="module")
def renderer_of():
    from par_raytracer_amd import api

    def get(key):
        if key not in _RENDERERS:
            desc, s = upload_desc(key)
            r = api.Renderer(0)
            r.upload(desc)
            _RENDERERS[key] = (r, s, desc)
        return _RENDERERS[key][:2]

    yield get
    for r, _, _ in _RENDERERS.values():
        r.close()
    _RENDERERS.clear()


def render_both(r, cam, w, h, pipeline, options, **kw):
    """{(trees, counting): (pixel bits, counters, elided shadow rays, parked shadow rays)} for SHADOW_TREES 1 / 0, plain and counting."""
    from par_raytracer_amd import api, capi
    out = {}
    try:
        for k, v in options.items():
            r.set_option(k, v)
        for trees in (1, 0):
            r.set_option("SHADOW_TREES", trees)
            for counting in (False, True):
                p = api.default_params(pipeline=pipeline | (capi.FLAG_COUNT_VISITS if counting else 0), **kw)
                img, c = r.render(cam, p, w, h)
                assert c.pipeline == pipeline
                st = r.render_stats()
                out[trees, counting] = (img.view(np.uint32).copy(), c, st.elided_shadow_rays if counting else None,
                                        st.parked_shadow_rays if counting else None)
    finally:
        for k in list(options) + ["SHADOW_TREES"]:
            r.set_option(k, None)
    return out


def assert_identical(got, built, what, one_node=False):
    on, off = got[1, False], got[0, False]
    for k in got:
        assert np.array_equal(got[k][0], off[0]), "%s: frame of (SHADOW_TREES, counting) = %s differs" % (what, k)
        assert got[k][1].ray_count == off[1].ray_count > 0 and got[k][1].shaded_hits == off[1].shaded_hits > 0, (what, k)
    assert on[1].render_ms > 0
    con, coff = got[1, True], got[0, True]
    assert con[2] == coff[2], (what, "elided shadow rays", con[2], coff[2])
    print(what, "node_visits off/on", coff[1].node_visits, con[1].node_visits, "tri_tests off/on", coff[1].tri_tests, con[1].tri_tests,
          "parked shadow rays off/on", coff[3], con[3])
    if built and one_node:
        assert con[1].node_visits == coff[1].node_visits and con[1].tri_tests < coff[1].tri_tests, (what, con[1].tri_tests, coff[1].tri_tests)
    elif built:
        assert con[1].node_visits < coff[1].node_visits, (what, con[1].node_visits, coff[1].node_visits)
        assert con[1].tri_tests <= coff[1].tri_tests, what
    else:
        assert con[1].node_visits == coff[1].node_visits and con[1].tri_tests == coff[1].tri_tests, what


def check_trees(r, key):
    """The getter against the scene: one entry per light, trees only for directional lights, roots behind the scene's nodes."""
    trees = r.shadow_trees()
    info = r.scene_info()
    roots = [t.root for t in trees if t.built]
    for t in trees:
        assert t.active == t.built
        if t.built:
            assert t.root >= info.bvh_node_count and t.node_count >= 1 and t.device_bytes > 0 and t.stack_bound >= 2
            assert t.triangle_count * 100 <= info.triangle_count * 75
        else:
            assert t.root == 0 and t.node_count == 0 and t.device_bytes == 0
    assert len(set(roots)) == len(roots)
    if BUILT[key] is not None:
        assert len(trees) == len(BUILT[key]) and all(b is None or t.built == b for t, b in zip(trees, BUILT[key])), (key, [t.as_dict() for t in trees])
    if key == "flat_plane":
        assert trees[0].triangle_count == 0 and trees[0].node_count == 1
    # a walk is never shorter than one node step: where the scene's own tree is a single node (the box on the 8-wide library)
    # the light's tree cannot save a visit, only triangle tests
    return any(t.built for t in trees), info.bvh_node_count == 1


@pytest.mark.gpu
@pytest.mark.parametrize("schedule", list(SCHEDULES))
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_a_render_with_shadow_trees_is_the_render_without(renderer_of, case, schedule):
    from par_raytracer_amd import api, capi
    cid, key, w, h, spp, depth = case
    r, s = renderer_of(key)
    built, one_node = check_trees(r, key)
    cam = api.make_camera(s.fov, w, h, s.camera_position, s.camera_facing)
    pipeline, options = SCHEDULES[schedule]
    got = render_both(r, cam, w, h, pipeline, options, spp=spp, seed=77, bounce_depth=depth)
    assert_identical(got, built, "%s %s" % (cid, schedule), one_node)
    # (the 8-wide tree's stack entries are whole groups of siblings: two of them hold these walks, and nothing is parked there)
    if schedule == "pool_parked" and cid == "gallery_two_lights" and capi.hip_lib().prt_build_flags() & capi.BUILD_BVH4:
        assert got[1, True][3] > 0 and got[0, True][3] > 0, "no shadow ray was parked: k_pool_parked_shadows did not run"


@pytest.mark.gpu
def test_adaptive_sampling_with_shadow_trees(renderer_of):
    from par_raytracer_amd import api
    r, s = renderer_of("terrain_64")
    cam = api.make_camera(s.fov, 64, 64, s.camera_position, s.camera_facing)
    got = render_both(r, cam, 64, 64, POOL, {}, spp=10, seed=77, bounce_depth=2, max_spp=50)
    assert_identical(got, True, "terrain adaptive 10..50")


@pytest.mark.gpu
def test_a_call_outside_the_bound_uses_the_scenes_tree(renderer_of):
    """|ray_bias| beyond the scene's extent, or a camera more than 4 extents out: the upload's exclusion bound does not cover the
    call's shadow-ray origins, and the call walks the scene's tree whatever SHADOW_TREES says - the same node_visits either way."""
    from par_raytracer_amd import api, capi
    r, s = renderer_of("cornell_box")
    ext = float(np.abs(s.positions).max())
    far = [float(v) for v in (np.asarray(s.camera_position, dtype=np.float64) + np.array([0.0, 0.0, 1.0]) * 6.0 * ext)]
    for what, cam, bias in (("far camera", api.make_camera(s.fov, 64, 64, far, s.camera_facing), None),
                            ("large bias", api.make_camera(s.fov, 64, 64, s.camera_position, s.camera_facing), 2.0 * ext)):
        visits = {}
        for trees in (1, 0):
            r.set_option("SHADOW_TREES", trees)
            p = api.default_params(spp=2, seed=77, bounce_depth=1, pipeline=POOL | capi.FLAG_COUNT_VISITS)
            if bias is not None:
                p.ray_bias = bias
            img, c = r.render(cam, p, 64, 64)
            visits[trees] = (c.node_visits, c.ray_count, img.view(np.uint32).copy())
        r.set_option("SHADOW_TREES", None)
        assert visits[1][0] == visits[0][0] > 0 and visits[1][1] == visits[0][1], what
        assert np.array_equal(visits[1][2], visits[0][2]), what


@pytest.mark.gpu
def test_an_update_makes_the_trees_stale():
    """After prt_update_geometry the trees are of another geometry: the getter reports them as not active, a render equals a
    fresh upload's render and walks the scene's tree (SHADOW_TREES changes nothing); the next upload has trees again."""
    from par_raytracer_amd import api, capi
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
        assert [(t.built, t.active) for t in ra.shadow_trees()] == [(1, 1)]
        ra.update_geometry(a["positions"])
        assert [(t.built, t.active) for t in ra.shadow_trees()] == [(1, 0)]
        rb.upload(api.FlatDesc(a))
        assert [(t.built, t.active) for t in rb.shadow_trees()] == [(1, 1)]
        cam = api.make_camera(s.fov, 96, 54, s.camera_position, s.camera_facing)
        for pipeline in (POOL, WAVEFRONT):
            fresh = render_both(rb, cam, 96, 54, pipeline, {}, spp=2, seed=77, bounce_depth=2)
            assert_identical(fresh, True, "fresh upload, pipeline %d" % pipeline)
            stale = render_both(ra, cam, 96, 54, pipeline, {}, spp=2, seed=77, bounce_depth=2)
            assert_identical(stale, False, "after the update, pipeline %d" % pipeline)
            assert np.array_equal(stale[1, False][0], fresh[1, False][0])
            assert stale[1, False][1].ray_count == fresh[1, False][1].ray_count and stale[1, False][1].shaded_hits == fresh[1, False][1].shaded_hits
        ra.upload(api.FlatDesc(a))
        assert [(t.built, t.active) for t in ra.shadow_trees()] == [(1, 1)]
    finally:
        ra.close()
        rb.close()


@pytest.mark.gpu
def test_shadow_trees_on_the_8_wide_library():
    """The module's other tests once more, in a child process that loads the 8-wide library (one library per process)."""
    if os.environ.get("PRT_HIP_LIB"):
        return                                              # this IS that child
    assert os.path.exists(os.path.join(ROOT, "par_raytracer_amd", "libprt_hip_bvh8.so")), "libprt_hip_bvh8.so not built (make hip-bvh8)"
    env = dict(os.environ, PRT_HIP_LIB="libprt_hip_bvh8.so")
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__)],
                         cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    tail = out.stdout.decode()[-3000:]
    assert out.returncode == 0 and " passed" in tail and "failed" not in tail, tail
