"""Open triangles on the GPU (include/prt.h "Open triangles", option SHADOW_OPEN): a directional light's shadow ray that starts
on a triangle the upload found open for that light is counted and credited at the hit, not traced.  Nothing that is rendered or
counted may change, so every case renders with SHADOW_OPEN=1 and SHADOW_OPEN=0 on ONE renderer, plain and counting: the frames
must be the same bits, ray_count and shaded_hits equal, elided(1) - elided(0) == open_shadow_rays(1), open_shadow_rays(0) == 0;
where rays were elided by a flag node_visits must be strictly lower and tri_tests no higher, where none were both must be equal
(so that no case passes because the switch does nothing).  On the pool pipeline ray_count - elided keeps matching the region
table's refill lanes, as tests/test_gpu_regions.py requires.

Scenes: terrain_64 (once more with the sun 7 degrees above the horizon: few open triangles), the Cornell box (none), icosphere_l3,
`coincident` (no possible occluder at all: the exception, nothing flagged), the box with two directional lights and a point light
(a bit per light next to a light without one) and the textured gallery with two lights (on the pool pipeline a textured render
runs a kernel variant that leaves the flags alone: there the counters must be equal).  Schedules: those of
tests/test_gpu_shadow_trees.py.  Then the flags against the device's own occlusion query, an adaptive case, a prt_render_rays case,
TRACE_DEAD_SHADOW_RAYS, calls outside the bounds, staleness after prt_update_geometry, and the module once more on the 8-wide
library."""
from __future__ import annotations

import os
import subprocess
import sys

import numpy as np
import pytest

import harness
from conftest import ROOT, host_scene, scene_dir
from test_gpu_shadow_trees import SCHEDULES, POOL, WAVEFRONT, upload_desc

#         id            scene key    w    h  spp depth
CASES = [("terrain", "terrain_64", 320, 180, 2, 2),
         ("low_sun", "terrain_low_sun", 320, 180, 2, 2),
         ("box", "cornell_box", 128, 128, 4, 2),
         ("icosphere", "icosphere_l3", 160, 120, 2, 2),
         ("ties", "coincident", 128, 72, 2, 2),
         ("three_lights", "box_three_lights", 96, 96, 2, 2),
         ("gallery_two_lights", "gallery_two_lights", 96, 72, 2, 2)]
MUST_ELIDE = ("terrain_64", "icosphere_l3")

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


def render_both(r, render, pipeline, options, **kw):
    """{(open, counting): (pixel bits, counters, render stats, region table)} for SHADOW_OPEN 1 / 0, plain and counting.
    render(params) -> (image, counters)."""
    from par_raytracer_amd import api, capi
    out = {}
    try:
        for k, v in options.items():
            r.set_option(k, v)
        for open_ in (1, 0):
            r.set_option("SHADOW_OPEN", open_)
            for counting in (False, True):
                p = api.default_params(pipeline=pipeline | (capi.FLAG_COUNT_VISITS if counting else 0), **kw)
                img, c = render(p)
                assert c.pipeline == pipeline
                out[open_, counting] = (np.ascontiguousarray(img).view(np.uint32).copy(), c, r.render_stats() if counting else None,
                                        r.region_stats() if counting and pipeline == POOL else None)
    finally:
        for k in list(options) + ["SHADOW_OPEN"]:
            r.set_option(k, None)
    return out


def assert_identical(got, what, must_elide=False, expect_none=False, regions=True):
    """The contract of the module's docstring; returns open_shadow_rays of the SHADOW_OPEN=1 counting render.  regions=False:
    an adaptive render, whose refill lanes include the camera rays it started ahead and called off - traced, never counted
    (kernels_pool.h POOL_JOB_SPEC_FLYING) -, so the region identity of tests/test_gpu_regions.py, a fixed-spp one, has no upper end."""
    off = got[0, False]
    for k in got:
        assert np.array_equal(got[k][0], off[0]), "%s: frame of (SHADOW_OPEN, counting) = %s differs" % (what, k)
        assert got[k][1].ray_count == off[1].ray_count > 0 and got[k][1].shaded_hits == off[1].shaded_hits > 0, (what, k)
    (_, con, son, ton), (_, coff, soff, toff) = got[1, True], got[0, True]
    print(what, "open", son.open_shadow_rays, "elided off/on", soff.elided_shadow_rays, son.elided_shadow_rays,
          "node_visits off/on", coff.node_visits, con.node_visits, "tri_tests off/on", coff.tri_tests, con.tri_tests)
    assert soff.open_shadow_rays == 0, what
    assert son.elided_shadow_rays - soff.elided_shadow_rays == son.open_shadow_rays, (what, son.elided_shadow_rays, soff.elided_shadow_rays, son.open_shadow_rays)
    if son.open_shadow_rays > 0:
        assert con.node_visits < coff.node_visits and con.tri_tests <= coff.tri_tests, (what, con.node_visits, coff.node_visits, con.tri_tests, coff.tri_tests)
    else:
        assert con.node_visits == coff.node_visits and con.tri_tests == coff.tri_tests, what
    if must_elide:
        assert son.open_shadow_rays > 0, what
    if expect_none:
        assert son.open_shadow_rays == 0, what
    for c, st, t in ((con, son, ton), (coff, soff, toff)):
        if t is not None:                                      # tests/test_gpu_regions.py: one finish block per ray that was traced
            traced = c.ray_count - st.elided_shadow_rays
            assert t["refill"][1] == t["finish"][1] and 0 <= t["refill"][1] - traced, (what, t["refill"], traced)
            assert not regions or t["refill"][1] - traced <= st.parked_rays, (what, t["refill"], traced, st.parked_rays)
    return son.open_shadow_rays


def check_info(r, key):
    """The getter against the scene: one entry per light, classified only for directional lights among the first four."""
    from par_raytracer_amd import capi
    infos, trees, n_tris = r.shadow_open(), r.shadow_trees(), r.scene_info().triangle_count
    assert len(infos) == len(trees)
    for l, (o, t) in enumerate(zip(infos, trees)):
        directional = t.triangle_count > 0 or t.built                      # (a point light has neither)
        assert o.classified <= (1 if l < capi.MAX_SHADOW_TREES else 0)
        assert o.open_count <= n_tris - t.triangle_count and o.active == (1 if o.open_count else 0)
        if not directional or t.triangle_count == 0:
            assert o.open_count == 0, (key, l)                             # a point light; the empty occluder set
        assert o.classify_ms >= 0.0
    return infos


@pytest.mark.gpu
@pytest.mark.parametrize("schedule", list(SCHEDULES))
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_a_render_with_open_flags_is_the_render_without(renderer_of, case, schedule):
    from par_raytracer_amd import api
    cid, key, w, h, spp, depth = case
    r, s = renderer_of(key)
    infos = check_info(r, key)
    cam = api.make_camera(s.fov, w, h, s.camera_position, s.camera_facing)
    pipeline, options = SCHEDULES[schedule]
    got = render_both(r, lambda p: r.render(cam, p, w, h), pipeline, options, spp=spp, seed=77, bounce_depth=depth)
    assert_identical(got, "%s %s" % (cid, schedule), must_elide=key in MUST_ELIDE, expect_none=not any(o.open_count for o in infos))
    if key == "box_three_lights":
        assert infos[2].classified == 0 and infos[2].open_count == 0          # the point light


@pytest.mark.gpu
def test_adaptive_sampling_with_open_flags(renderer_of):
    from par_raytracer_amd import api
    r, s = renderer_of("terrain_64")
    cam = api.make_camera(s.fov, 64, 64, s.camera_position, s.camera_facing)
    got = render_both(r, lambda p: r.render(cam, p, 64, 64), POOL, {}, spp=10, seed=77, bounce_depth=2, max_spp=50)
    # (adaptive renders run k_pool's general-RNG variants, which leave the flags alone: kernels_pool.h PoolEmit::TAKES_OPEN)
    assert_identical(got, "terrain adaptive 10..50", regions=False)


@pytest.mark.gpu
def test_render_rays_with_open_flags(renderer_of):
    """prt_render_rays shares the shading code: the caller's rays, 257 outputs x 8 rays from inside and outside the scene's box."""
    import radiance_cases as R
    r, _ = renderer_of("terrain_64")
    o, d, _ = R.make_rays(host_scene("terrain_64").arrays(), 257, 8, 505)
    o, d = np.ascontiguousarray(o), np.ascontiguousarray(d)
    got = render_both(r, lambda p: r.render_rays(o, d, p, first=3), WAVEFRONT, {}, spp=8, seed=77, bounce_depth=2)
    assert_identical(got, "terrain render_rays", must_elide=True)


@pytest.mark.gpu
@pytest.mark.parametrize("pipeline", [POOL, WAVEFRONT])
def test_tracing_dead_shadow_rays_traces_the_open_ones_too(renderer_of, pipeline):
    """TRACE_DEAD_SHADOW_RAYS=1 keeps meaning "every ray is traced": nothing is elided, by a flag or otherwise, and the frame is
    the frame."""
    from par_raytracer_amd import api, capi
    r, s = renderer_of("terrain_64")
    cam = api.make_camera(s.fov, 96, 54, s.camera_position, s.camera_facing)
    p = api.default_params(spp=2, seed=77, bounce_depth=2, pipeline=pipeline | capi.FLAG_COUNT_VISITS)
    ref, cref = r.render(cam, p, 96, 54)
    assert r.render_stats().open_shadow_rays > 0
    try:
        r.set_option("TRACE_DEAD_SHADOW_RAYS", 1)
        img, c = r.render(cam, p, 96, 54)
        st = r.render_stats()
        assert st.elided_shadow_rays == 0 and st.open_shadow_rays == 0
        assert np.array_equal(img.view(np.uint32), ref.view(np.uint32)) and c.ray_count == cref.ray_count and c.shaded_hits == cref.shaded_hits
    finally:
        r.set_option("TRACE_DEAD_SHADOW_RAYS", None)


@pytest.mark.gpu
def test_a_call_outside_the_bounds_elides_nothing_by_flag(renderer_of):
    """|ray_bias| above the upload's bound (2^-11 of the scene's largest |coordinate|), or a camera beyond the trees' guard (4 x
    that coordinate): the flags were not computed for the call's shadow-ray origins and it traces them all."""
    from par_raytracer_amd import api, capi
    r, s = renderer_of("terrain_64")
    ext = float(np.abs(s.positions).max())
    near = api.make_camera(s.fov, 64, 64, s.camera_position, s.camera_facing)
    far_pos = [float(v) for v in (np.asarray(s.camera_position, dtype=np.float64) + np.array([0.0, 1.0, 0.0]) * 6.0 * ext)]
    far = api.make_camera(s.fov, 64, 64, far_pos, (0.0, -1.0, 0.05))
    bound = ext / 2048.0

    def opened(cam, bias):
        # depth 2: the far camera's primary hits lie beyond the flags' reach anyway, its bounce hits do not - only the camera
        # guard keeps those from taking a flag
        p = api.default_params(spp=2, seed=77, bounce_depth=2, pipeline=POOL | capi.FLAG_COUNT_VISITS)
        if bias is not None:
            p.ray_bias = bias
        _, c = r.render(cam, p, 64, 64)
        assert c.shaded_hits > 0
        return r.render_stats().open_shadow_rays

    assert opened(near, None) > 0
    assert opened(near, bound) > 0 and opened(near, -bound) > 0                      # at the bound: covered
    assert opened(near, float(np.nextafter(np.float32(bound), np.float32(1e9)))) == 0
    assert opened(near, -2.0 * bound) == 0
    assert opened(far, None) == 0
    # ... and it is the guard: just inside it (3.9 extents up, as far beyond the reach) bounce hits do take flags
    inside = [float(v) for v in (np.asarray(s.camera_position, dtype=np.float64) * np.array([1.0, 0.0, 1.0]) + np.array([0.0, 1.0, 0.0]) * 3.9 * ext)]
    assert opened(api.make_camera(s.fov, 64, 64, inside, (0.0, -1.0, 0.05)), None) > 0
    infos = r.shadow_open()
    assert infos[0].bias_max == np.float32(bound) and infos[0].reach == np.float32(2.0 * ext)


@pytest.mark.gpu
def test_an_update_makes_the_flags_stale():
    """After prt_update_geometry the flags are of another geometry: the getter reports them as not active and no ray is elided by
    one - the frame equals a fresh upload's, which has flags again."""
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
        assert [(o.classified, o.active) for o in ra.shadow_open()] == [(1, 1)] and ra.shadow_open()[0].open_count > 0
        ra.update_geometry(a["positions"])
        assert [(o.classified, o.active) for o in ra.shadow_open()] == [(1, 0)]
        rb.upload(api.FlatDesc(a))
        assert [(o.classified, o.active) for o in rb.shadow_open()] == [(1, 1)]
        cam = api.make_camera(s.fov, 96, 54, s.camera_position, s.camera_facing)
        for pipeline in (POOL, WAVEFRONT):
            fresh = render_both(rb, lambda q: rb.render(cam, q, 96, 54), pipeline, {}, spp=2, seed=77, bounce_depth=2)
            assert_identical(fresh, "fresh upload, pipeline %d" % pipeline, must_elide=True)
            stale = render_both(ra, lambda q: ra.render(cam, q, 96, 54), pipeline, {}, spp=2, seed=77, bounce_depth=2)
            assert_identical(stale, "after the update, pipeline %d" % pipeline, expect_none=True)
            assert np.array_equal(stale[1, False][0], fresh[1, False][0])
            assert stale[1, False][1].ray_count == fresh[1, False][1].ray_count and stale[1, False][1].shaded_hits == fresh[1, False][1].shaded_hits
        ra.upload(api.FlatDesc(a))
        assert [(o.classified, o.active) for o in ra.shadow_open()] == [(1, 1)]
    finally:
        ra.close()
        rb.close()


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["terrain_64", "icosphere_l3"])
def test_the_flags_against_the_devices_own_occlusion_query(renderer_of, key, tmp_path):
    """A few thousand points on open triangles (the flags as tests/shadow_open_host_harness.cpp computes them with the upload's
    functions; the upload's own count must agree), pushed as a render pushes a hit with its bias: prt_trace_rays in mode
    "occluded", towards the light with that bias, finds every one of them unoccluded."""
    from test_shadow_open_host import scene_case
    r, _ = renderer_of(key)
    verts, direction = scene_case(key)
    cases, results = harness.case_files(tmp_path, "cases.bin", "flags.bin")
    with open(cases, "wb") as f:
        harness.put(f, ([1], np.uint32))
        f.write(key.encode().ljust(32, b"\0"))
        harness.put(f, ([len(verts)], np.uint32), (direction, np.float32), (verts, np.float32))
    exe = harness.build("shadow_open_host_harness.cpp", tmp_path, "so_flags", sources=("scene_pack.cpp", "bvh_build.cpp", "bvh_check.cpp"), flags=("-O2",))
    harness.run(exe, "flags", cases, results)
    rd = harness.Reader.of_file(results)
    (n,) = rd.unpack("<I")
    flags = rd.take(n, np.uint8)
    rd.done()
    assert n == len(verts) and int(flags.sum()) == r.shadow_open()[0].open_count > 0
    rng = np.random.default_rng(9)
    tri = verts[np.nonzero(flags)[0]].reshape(-1, 3, 3)
    tri = tri[rng.integers(0, len(tri), 4096)]
    u = rng.random(4096).astype(np.float32)
    v = (rng.random(4096).astype(np.float32) * (np.float32(1.0) - u)).astype(np.float32)
    u[:64], v[:64] = 0.0, 0.0                                                    # corners and edges among them
    u[64:128], v[64:128] = 1.0, 0.0
    v[128:192] = 0.0
    a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
    pos = (a + (b - a) * u[:, None] + (c - a) * v[:, None]).astype(np.float32)
    nrm = np.cross((b - a).astype(np.float32), (c - a).astype(np.float32)).astype(np.float32)
    gn = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True).astype(np.float32)).astype(np.float32)
    bound = float(np.abs(verts).max()) / 2048.0
    dirs = np.ascontiguousarray(np.broadcast_to(direction.astype(np.float32), pos.shape))
    for bias in (1e-3, bound, -bound, 0.0):
        origins = np.ascontiguousarray((pos + gn * np.float32(bias)).astype(np.float32))          # raytracer.cpp:425; the query pushes by d * bias
        res = r.trace_rays(origins, dirs, mode="occluded", ray_bias=bias)
        assert int(res["occluded"].sum()) == 0, (key, bias, int(res["occluded"].sum()))


@pytest.mark.gpu
def test_open_flags_on_the_8_wide_library():
    """The module's other tests once more, in a child process that loads the 8-wide library (one library per process)."""
    if os.environ.get("PRT_HIP_LIB"):
        return                                              # this IS that child
    assert os.path.exists(os.path.join(ROOT, "par_raytracer_amd", "libprt_hip_bvh8.so")), "libprt_hip_bvh8.so not built (make hip-bvh8)"
    env = dict(os.environ, PRT_HIP_LIB="libprt_hip_bvh8.so")
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__)],
                         cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    tail = out.stdout.decode()[-3000:]
    assert out.returncode == 0 and " passed" in tail and "failed" not in tail, tail
