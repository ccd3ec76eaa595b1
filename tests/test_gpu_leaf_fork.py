"""Leaf rays beside the bounce walk (option POOL_FORK; kernels_wave.h shade_entry_on's fork step, kernels_pool.h FORKS).

A ray that enters at the last bounce level draws nothing and spawns nothing in an opaque scene, so the pool pipeline lets it fly
beside its sample's walk, marked, instead of making the walk wait a round for it.  Nothing that is rendered or counted may
change: every case renders with POOL_FORK=1 and POOL_FORK=0 on one renderer and with the wavefront pipeline, and the three
frames must be the same bits, with the same ray_count and shaded_hits.  So that no case passes because nothing forked, a
counting render of both modes must show leaf rays made with forking on and none with it off, the same child rays in total, and
no more frames saved.

The near-tie scene `coincident` carries a translucent patch, so it renders with the kernel that keeps its draw ring in memory,
which is no forking kernel: a leaf could draw there.  Its cases (the plain one, POOL_PARK_CAP=8, STACK_CAP=4) are kept and
must show what a translucent scene has to show - POOL_FORK=1 changes neither the frame nor a row of the region table.  What
they were meant to reach - marked leaves that are parked, park lists that grow, a frame rendered again, leaves adopted by the
EXACT launch - is reached on an opaque scene instead: terrain_64 with two-entry stack columns, where dropped pushes park
nearly every ray, with and without park lists that start at 8 entries.
"""
from __future__ import annotations

import numpy as np
import pytest

from conftest import host_scene, scene_dir

pytestmark = pytest.mark.gpu

# the pool's schedules: block-shared pools (the default kernel), wave-private pools, the EXACT kernel rendering everything, and
# pools so small, with so little room for leaves, that forking and non-forking passes mix in one frame
SCHEDULES = {
    "shared": {"POOL_SHARED": 1},
    "private": {"POOL_SHARED": 0},
    "exact": {"POOL_EXACT": 1},
    "mixed_shared": {"POOL_SHARED": 1, "POOL_CAP": 64, "POOL_FORK_ROOM": 1},
    "mixed_private": {"POOL_SHARED": 0, "POOL_CAP": 64, "POOL_FORK_ROOM": 1},
}
MIXED_OF = {"mixed_shared": "shared", "mixed_private": "private"}

#        id                scene          w    h   spp depth  R     extra options
CASES = [("box_d2", "cornell_box", 96, 96, 4, 2, None, {}),
         ("box_d1", "cornell_box", 96, 96, 4, 1, None, {}),          # every child is a leaf, the walk ends at the primary hit
         ("box_d0", "cornell_box", 96, 96, 4, 0, None, {}),          # no children at all: forking is a no-op
         ("terrain_d2", "terrain_64", 160, 90, 4, 2, None, {}),
         ("terrain_r2_d1", "terrain_64", 160, 90, 4, 1, 2, {}),      # three leaves per event, 7 draws
         ("ties_d2", "coincident", 128, 72, 2, 2, None, {}),
         ("ties_park8", "coincident", 128, 72, 2, 2, None, {"POOL_PARK_CAP": 8}),     # leaves get parked, lists grow, the frame is rendered again
         ("ties_stack4", "coincident", 128, 72, 2, 2, None, {"STACK_CAP": 4}),
         # an opaque scene whose rays are parked: dropped pushes park leaves; lists that grow, the frame rendered again
         ("terrain_stack2", "terrain_64", 160, 90, 4, 2, None, {"STACK_CAP": 2}),
         ("terrain_stack2_park8", "terrain_64", 160, 90, 4, 2, None, {"STACK_CAP": 2, "POOL_PARK_CAP": 8})]
TRANSLUCENT = ("coincident", "many_materials")        # scenes of the draw-ring kernel: nothing forks

_RENDERERS = {}


@pytest.fixture(scope="module")
def renderer_of():
    from par_raytracer_amd import api

    def get(scene):
        if scene not in _RENDERERS:
            r = api.Renderer(0)
            r.upload(host_scene(scene, 0))
            _RENDERERS[scene] = r
        return _RENDERERS[scene]

    yield get
    for r in _RENDERERS.values():
        r.close()
    _RENDERERS.clear()


def _render_all(r, cam, w, h, spp, depth, refl, options):
    """Frames and counters of POOL_FORK 0 / 1 under `options`, then the region tables of a counting render of each."""
    from par_raytracer_amd import api, capi
    kw = dict(bounce_depth=depth)
    if refl is not None:
        kw["reflection_samples"] = refl
    out = {}
    try:
        for k, v in options.items():
            r.set_option(k, v)
        for fork in (0, 1):
            r.set_option("POOL_FORK", fork)
            out["img", fork], out["ctr", fork] = r.render(cam, api.default_params(spp, 77, pipeline=capi.PIPELINE_POOL, **kw), w, h)
        for fork in (0, 1):
            r.set_option("POOL_FORK", fork)
            img, c = r.render(cam, api.default_params(spp, 77, pipeline=capi.PIPELINE_POOL | capi.FLAG_COUNT_VISITS, **kw), w, h)
            out["table", fork] = r.region_stats()
            out["parked", fork] = r.render_stats().parked_rays
            # counting changes nothing either
            assert np.array_equal(img.view(np.uint32), out["img", fork].view(np.uint32))
            assert c.ray_count == out["ctr", fork].ray_count
    finally:
        for k in list(options) + ["POOL_FORK"]:
            r.set_option(k, None)
    return out


_WAVEFRONT = {}


def _wavefront(r, key, cam, w, h, spp, depth, refl):
    """The reference frame of a case, rendered once and shared by its schedules."""
    from par_raytracer_amd import api, capi
    if key not in _WAVEFRONT:
        kw = dict(bounce_depth=depth)
        if refl is not None:
            kw["reflection_samples"] = refl
        img, c = r.render(cam, api.default_params(spp, 77, pipeline=capi.PIPELINE_WAVEFRONT, **kw), w, h)
        _WAVEFRONT[key] = (img.view(np.uint32).copy(), c.ray_count, c.shaded_hits)
    return _WAVEFRONT[key]


_FULL_LEAVES = {}


@pytest.mark.parametrize("schedule", list(SCHEDULES))
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_forked_render_is_the_unforked_render(renderer_of, case, schedule):
    from par_raytracer_amd import api
    cid, scene, w, h, spp, depth, refl, extra = case
    s, _ = scene_dir(scene)
    r = renderer_of(scene)
    cam = api.make_camera(s.fov, w, h, s.camera_position, s.camera_facing)
    want, want_rays, want_hits = _wavefront(r, cid, cam, w, h, spp, depth, refl)
    got = _render_all(r, cam, w, h, spp, depth, refl, dict(SCHEDULES[schedule], **extra))
    for fork in (0, 1):
        assert np.array_equal(got["img", fork].view(np.uint32), want), "POOL_FORK=%d" % fork
        assert got["ctr", fork].ray_count == want_rays > 0 and got["ctr", fork].shaded_hits == want_hits > 0
    off, on = got["table", 0], got["table", 1]
    print(cid, schedule, "leaf_ray", on["leaf_ray"], "walk_child_ray off/on", off["walk_child_ray"], on["walk_child_ray"],
          "frame_save off/on", off["frame_save"][1], on["frame_save"][1], "shade_pass off/on", off["shade_pass"][0], on["shade_pass"][0])
    assert off["leaf_ray"] == (0, 0)
    if scene in TRANSLUCENT:
        assert on["leaf_ray"] == (0, 0)
        for name in ("shade_pass", "walk_child_ray", "frame_save", "frame_load", "outputs", "walk_loop", "radiance_store"):
            assert off[name][1] == on[name][1], name
        return
    if depth == 0:
        assert on["leaf_ray"] == (0, 0) and on["walk_child_ray"][1] == 0
    else:
        assert on["leaf_ray"][1] > 0
    if "STACK_CAP" in extra and schedule != "exact":
        assert got["parked", 1] > 0                                  # (the EXACT kernel's stack spills to memory: it parks nothing)
    # the same rays are made, whichever event makes them; and no frame is saved that was not saved before
    assert on["leaf_ray"][1] + on["walk_child_ray"][1] == off["walk_child_ray"][1]
    assert on["frame_save"][1] <= off["frame_save"][1]
    if schedule in ("shared", "private"):
        _FULL_LEAVES[cid, schedule] = on["leaf_ray"][1]
    if schedule in MIXED_OF and depth > 0:
        # forking and non-forking passes in one frame: some leaves fly marked, not all that could
        if (cid, MIXED_OF[schedule]) not in _FULL_LEAVES:           # (that schedule of the case was not selected: render it here)
            full = _render_all(r, cam, w, h, spp, depth, refl, dict(SCHEDULES[MIXED_OF[schedule]], **extra))
            _FULL_LEAVES[cid, MIXED_OF[schedule]] = full["table", 1]["leaf_ray"][1]
        if "STACK_CAP" in extra:
            # nearly every ray is parked and forks in the adopting launch, a few entries per wave: room is no constraint there
            assert on["leaf_ray"][1] > 0
        else:
            assert 0 < on["leaf_ray"][1] < _FULL_LEAVES[cid, MIXED_OF[schedule]]


def test_translucent_scene_does_not_fork(renderer_of):
    """many_materials has translucent clusters: its kernel keeps a draw ring in memory and is no forking kernel, so POOL_FORK=1
    must change nothing - neither the frame nor one row of the region table."""
    from par_raytracer_amd import api, capi
    w, h = 96, 64
    s, _ = scene_dir("many_materials")
    r = renderer_of("many_materials")
    cam = api.make_camera(s.fov, w, h, s.camera_position, s.camera_facing)
    want, want_rays, want_hits = _wavefront(r, "many_materials", cam, w, h, 2, 2, None)
    got = _render_all(r, cam, w, h, 2, 2, None, {})
    for fork in (0, 1):
        assert np.array_equal(got["img", fork].view(np.uint32), want)
        assert got["ctr", fork].ray_count == want_rays and got["ctr", fork].shaded_hits == want_hits
    assert got["table", 1]["leaf_ray"] == (0, 0)
    for name in ("shade_pass", "walk_child_ray", "frame_save", "frame_load", "outputs", "walk_loop"):
        assert got["table", 0][name][1] == got["table", 1][name][1], name
