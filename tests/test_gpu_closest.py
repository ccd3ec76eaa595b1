"""prt_closest_points on the GPU against the brute force of tests/closest_host_harness.cpp (closest_on_triangle over every triangle
with the tie rule, built here with g++): every field bit for bit through the host entry point (numpy) and the device entry point
(torch), on the SAH tree, the LBVH tree, the 8-wide library and a refitted tree; radii, invalid points, mixed waves, permutations,
more points than one pass of the grid, the stack overflow path, the empty scene, the errors, and that the walk culls."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import closest_cases as K
from conftest import ROOT, host_scene

SEEDS = {name: 100 + i for i, name in enumerate(K.FIXTURES)}


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("closest_gpu")


@pytest.fixture(scope="module")
def brute(workdir):
    """brute(mesh, points, max_dist2=None) -> the harness's brute-force answers {field: array}."""
    exe = K.build_harness(workdir)

    def run(mesh, points, max_dist2=None):
        return K.run_harness(exe, [K.case(mesh, points, max_dist2)], workdir)[0]["brute"]
    return run


@pytest.fixture(scope="module")
def reference(brute):
    """name -> (mesh, points, kind, brute-force answers) of the four fixtures' recipe points, computed once."""
    cache = {}

    def get(name):
        if name not in cache:
            mesh = K.scene_mesh(name)
            pts, kind = K.recipe_points(mesh, K.RECIPE_POINTS, SEEDS[name])
            cache[name] = (mesh, pts, kind, brute(mesh, pts))
        return cache[name]
    return get


@pytest.fixture(scope="module")
def renderers():
    from par_raytracer_amd import api
    out = {}

    def get(name, builder="sah"):
        if (name, builder) not in out:
            r = api.Renderer(0)
            if builder != "sah":
                r.set_option("BVH_BUILDER", builder)
            r.upload(host_scene(name, 0))
            out[(name, builder)] = r
        return out[(name, builder)]
    yield get
    for r in out.values():
        r.close()


def both_paths(r, pts, what, expect, max_dist=None):
    """The batch through the numpy and the torch path; every field of both equals `expect`."""
    import torch
    res = r.closest_points(pts, max_dist=max_dist)
    assert res["counters"].ray_count == len(pts) and res["counters"].pipeline == 0
    K.assert_same_bits(res, expect, what + " (numpy)")
    miss = expect["group"] < 0
    assert np.all(np.isinf(res["distance"][miss])) and np.array_equal(res["distance"][~miss], np.sqrt(expect["dist2"][~miss]))
    dev = torch.device("cuda", r.device_id)
    res_t = r.closest_points(torch.from_numpy(pts).to(dev), max_dist=None if max_dist is None else torch.from_numpy(max_dist).to(dev))
    K.assert_same_bits(K.to_numpy(res_t), expect, what + " (torch)")


def raw_call(r, pts, max_dist2, device=False):
    """prt_closest_points through the C ABI with squared radii as given; returns {field: array}."""
    from par_raytracer_amd import capi
    n = len(pts)
    out = dict(dist2=np.empty(n, np.float32), point=np.empty((n, 3), np.float32), bw=np.empty((n, 3), np.float32),
               vertex0=np.empty(n, np.uint32), group=np.empty(n, np.int32))
    batch = capi.PrtPointBatch(pts.ctypes.data, None if max_dist2 is None else max_dist2.ctypes.data, n)
    cb = capi.PrtClosestBuffers(*[out[k].ctypes.data for k in K.FIELDS])
    assert capi.hip_lib().prt_closest_points(r._ctx, C.byref(batch), C.byref(cb), 0, None) == 0
    return out


@pytest.mark.gpu
def test_wave_boundaries_on_one_triangle(brute):
    from par_raytracer_amd import api
    mesh = K.one_triangle()
    r = api.Renderer(0)
    try:
        r.upload(K.flat_desc(mesh))
        for n in (1, 64, 65):
            pts, _ = K.recipe_points(mesh, max(n, 8), 40 + n)
            pts = np.ascontiguousarray(pts[:n])
            both_paths(r, pts, "one triangle, %d points" % n, brute(mesh, pts))
    finally:
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", K.FIXTURES)
@pytest.mark.parametrize("builder", ["sah", "lbvh"])
def test_fixtures_equal_the_brute_force(renderers, reference, name, builder):
    mesh, pts, kind, expect = reference(name)
    both_paths(renderers(name, builder), pts, "%s / %s" % (name, builder), expect)


CHILD = r"""
import os, sys, tempfile
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, "tests")); sys.path.insert(0, os.path.join(%(root)r, "oracle"))
import numpy as np
from conftest import host_scene
import closest_cases as K
from test_gpu_closest import SEEDS, both_paths
from par_raytracer_amd import api, capi
lib = capi.hip_lib()
assert os.path.basename(lib._name) == "libprt_hip_bvh8.so" and not (lib.prt_build_flags() & capi.BUILD_BVH4)
d = tempfile.mkdtemp(prefix="prt_closest8_")
exe = K.build_harness(d)
meshes = {name: K.scene_mesh(name) for name in K.FIXTURES}
points = {name: K.recipe_points(meshes[name], K.RECIPE_POINTS, SEEDS[name])[0] for name in K.FIXTURES}
results = K.run_harness(exe, [K.case(meshes[name], points[name]) for name in K.FIXTURES], d)
for name, res in zip(K.FIXTURES, results):
    r = api.Renderer(0)
    r.upload(host_scene(name, 0))
    both_paths(r, points[name], name + " / 8-wide", res["brute"])
    print(name, "equal", flush=True)
    r.close()
print("bvh8 closest points ok")
"""


@pytest.mark.gpu
def test_fixtures_on_the_8_wide_library():
    if not os.path.exists(os.path.join(ROOT, "par_raytracer_amd", "libprt_hip_bvh8.so")):
        pytest.skip("libprt_hip_bvh8.so not built (make hip-bvh8)")
    env = dict(os.environ)
    env["PRT_HIP_LIB"] = "libprt_hip_bvh8.so"
    out = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         timeout=600)
    assert out.returncode == 0 and b"bvh8 closest points ok" in out.stdout, (out.returncode, out.stdout.decode()[-1500:],
                                                                             out.stderr.decode()[-3000:])


@pytest.mark.gpu
def test_radius(renderers, reference, brute):
    mesh, pts, kind, free = reference("icosphere_l3")
    r = renderers("icosphere_l3")
    n = 6 * 128
    pts, d2 = np.ascontiguousarray(pts[:n]), free["dist2"][:n]
    cls = np.arange(n) % 6                 # 0: d2 itself, 1: the next float below, 2: +inf, 3: negative, 4: NaN, 5: d2 itself
    below = np.nextafter(d2, np.float32(-np.inf))
    radius2 = np.select([cls == 1, cls == 2, cls == 3, cls == 4], [below, np.float32(np.inf), np.float32(-1.0), np.float32(np.nan)],
                        d2).astype(np.float32)
    expect = brute(mesh, pts, radius2)
    got = raw_call(r, pts, radius2)
    K.assert_same_bits(got, expect, "radii")
    hit = np.isin(cls, (0, 2, 5))
    assert np.all(got["group"][hit] >= 0) and np.array_equal(K.bits(got["dist2"][hit]), K.bits(d2[hit])), "equal bits and +inf must hit"
    assert np.all(got["group"][~hit] == -1) and np.all(got["dist2"][~hit] == K.FLT_MAX) and np.all(got["vertex0"][~hit] == 0xFFFFFFFF)
    assert np.all(got["point"][~hit] == 0) and np.all(got["bw"][~hit] == 0)
    for k in K.FIELDS:                      # the hits are what they are without a radius: their neighbours did not disturb them
        assert np.array_equal(K.bits(got[k][hit]), K.bits(free[k][:n][hit])), k
    K.assert_same_bits(raw_call(r, pts, None), {k: v[:n] for k, v in free.items()}, "NULL radii")
    # radius 0 finds points that lie on the surface, and only those
    on = np.nonzero(free["dist2"] == 0)[0]
    assert on.size > 0
    sel = np.concatenate([on[:64], np.nonzero(free["dist2"] > 0)[0][:64]])
    zero = raw_call(r, np.ascontiguousarray(reference("icosphere_l3")[1][sel]), np.zeros(len(sel), np.float32))
    assert np.array_equal(zero["group"] >= 0, free["dist2"][sel] == 0)
    # the wrapper takes distances and squares them in float32
    dist = np.sqrt(d2).astype(np.float32) * np.float32(1.5)
    both_paths(r, pts, "max_dist", brute(mesh, pts, (dist * dist).astype(np.float32)), max_dist=dist)


@pytest.mark.gpu
def test_non_finite_points_are_misses_and_disturb_nothing(renderers, reference, brute):
    mesh, pts, kind, free = reference("coincident")
    r = renderers("coincident")
    pts = pts[:512].copy()
    bad = np.array([0, 5, 63, 64, 65, 200, 511])
    for i, (j, val) in enumerate(zip(bad, (np.nan, np.inf, -np.inf, np.nan, np.inf, -np.inf, np.nan))):
        pts[j, i % 3] = val
    expect = brute(mesh, pts)
    both_paths(r, pts, "non-finite points", expect)
    good = np.setdiff1d(np.arange(512), bad)
    assert np.all(expect["group"][bad] == -1) and np.all(expect["dist2"][bad] == K.FLT_MAX)
    for k in K.FIELDS:
        assert np.array_equal(K.bits(expect[k][good]), K.bits(free[k][:512][good])), k


@pytest.mark.gpu
def test_mixed_waves_equal_the_batch_sorted_by_kind(renderers, reference):
    mesh, pts, kind, free = reference("icosphere_l3")
    r = renderers("icosphere_l3")
    per = 128
    groups = [np.nonzero(kind == K.KIND_NEAR)[0][:per], np.nonzero(kind == K.KIND_FAR)[0][:per], np.nonzero(kind == K.KIND_ON)[0][:per]]
    assert all(len(g) == per for g in groups)
    sorted_pts = np.concatenate([pts[g] for g in groups] + [np.full((per, 3), np.nan, np.float32)]).astype(np.float32)
    mix = (np.arange(4 * per) % 4) * per + np.arange(4 * per) // 4      # near, far, on the surface, invalid, near, ...
    mixed = r.closest_points(np.ascontiguousarray(sorted_pts[mix]))
    by_kind = r.closest_points(sorted_pts)
    K.assert_same_bits(mixed, {k: by_kind[k][mix] for k in K.FIELDS}, "mixed waves")
    assert np.all(by_kind["group"][3 * per:] == -1) and np.all(by_kind["group"][:3 * per] >= 0)
    K.assert_same_bits({k: by_kind[k][:3 * per] for k in K.FIELDS}, {k: free[k][np.concatenate(groups)] for k in K.FIELDS}, "sorted by kind")


@pytest.mark.gpu
def test_permutation_and_repetition(renderers, reference):
    mesh, pts, kind, free = reference("coincident")
    r = renderers("coincident")
    perm = np.random.default_rng(11).permutation(len(pts))
    K.assert_same_bits(r.closest_points(np.ascontiguousarray(pts[perm])), {k: free[k][perm] for k in K.FIELDS}, "permuted")
    first, second = r.closest_points(pts), r.closest_points(pts)
    K.assert_same_bits(second, first, "the same batch twice")


@pytest.mark.gpu
def test_more_points_than_one_pass_of_the_grid(renderers, brute):
    mesh = K.scene_mesh("cornell_box")
    n = (1 << 19) + 5
    pts, _ = K.recipe_points(mesh, n, 77)
    res = renderers("cornell_box").closest_points(pts)
    K.assert_same_bits(res, brute(mesh, pts), "2^19 + 5 points")


@pytest.mark.gpu
def test_stack_overflow_path(reference):
    from par_raytracer_amd import api
    mesh, pts, kind, free = reference("terrain_64")
    near = np.ascontiguousarray(pts[kind == K.KIND_NEAR])
    expect = {k: free[k][kind == K.KIND_NEAR] for k in K.FIELDS}
    r = api.Renderer(0)
    try:
        r.upload(host_scene("terrain_64", 0))
        plain = r.closest_points(near, count_visits=True)
        r.set_option("STACK_CAP", 2)        # the marker and one entry: nearly every push is dropped, the points go to the slow list
        capped = r.closest_points(near, count_visits=True)
        r.set_option("STACK_CAP", None)
    finally:
        r.close()
    K.assert_same_bits(plain, expect, "default stack")
    K.assert_same_bits(capped, expect, "STACK_CAP=2")
    # a listed point is walked twice (the dropped walk, then the whole one): the visit count tells
    assert capped["counters"].node_visits != plain["counters"].node_visits


@pytest.mark.gpu
def test_moved_scene_equals_a_fresh_upload_and_the_brute_force(brute):
    from par_raytracer_amd import api
    p, idx, runs = K.scene_mesh("icosphere_l3")
    shear = np.array([[1.25, 0.0, 0.0], [0.5, 0.75, 0.0], [-0.25, 0.125, 1.5]], np.float32)
    moved = np.ascontiguousarray((p @ shear).astype(np.float32))
    pts, _ = K.recipe_points((moved, idx, runs), 1024, 55)
    r, fresh = api.Renderer(0), api.Renderer(0)
    try:
        r.upload(K.flat_desc((p, idx, runs)))
        for positions in (moved, p):                      # there, and back again
            mesh = (positions, idx, runs)
            r.update_geometry(positions)
            fresh.upload(K.flat_desc(mesh))
            expect = brute(mesh, pts)
            K.assert_same_bits(r.closest_points(pts), expect, "refitted tree")
            K.assert_same_bits(fresh.closest_points(pts), expect, "fresh upload")
    finally:
        r.close()
        fresh.close()


@pytest.mark.gpu
def test_empty_scene_and_errors():
    from par_raytracer_amd import api, capi
    lib = capi.hip_lib()
    p, idx, runs = K.one_triangle()
    pts = np.array([[0.5, 0.5, 0.5], [3.0, -1.0, 2.0], [np.nan, 0.0, 0.0]], np.float32)
    d2 = np.full(3, 7.5, np.float32)
    batch = capi.PrtPointBatch(pts.ctypes.data, None, 3)
    out = capi.PrtClosestBuffers(d2.ctypes.data, None, None, None, None)
    r = api.Renderer(0)
    try:
        for entry in (lib.prt_closest_points, lib.prt_closest_points_device):
            assert entry(r._ctx, C.byref(batch), C.byref(out), 0, None) == -2, "no scene"
        r.upload(K.flat_desc((p, np.zeros(0, np.uint32), np.zeros((0, 2), np.uint32))))
        assert r.scene_info().triangle_count == 0
        res = r.closest_points(pts)
        assert np.all(res["group"] == -1) and np.all(res["vertex0"] == 0xFFFFFFFF) and np.all(res["dist2"] == K.FLT_MAX)
        assert np.all(res["point"] == 0) and np.all(res["bw"] == 0) and np.all(np.isinf(res["distance"]))
        r.upload(K.flat_desc((p, idx, runs)))
        ctr = capi.PrtCounters()
        for entry in (lib.prt_closest_points, lib.prt_closest_points_device):
            null_points = capi.PrtPointBatch(None, None, 3)
            assert entry(r._ctx, C.byref(null_points), C.byref(out), 0, None) == -1
            assert entry(r._ctx, None, C.byref(out), 0, None) == -1 and entry(r._ctx, C.byref(batch), None, 0, None) == -1
            empty = capi.PrtPointBatch(None, None, 0)
            assert entry(r._ctx, C.byref(empty), C.byref(out), 0, C.byref(ctr)) == 0 and ctr.ray_count == 0
        assert np.all(d2 == 7.5), "nothing was written"
        # only the requested field is written
        assert lib.prt_closest_points(r._ctx, C.byref(batch), C.byref(out), 0, C.byref(ctr)) == 0 and ctr.ray_count == 3
        assert d2[0] < K.FLT_MAX and d2[1] < K.FLT_MAX and d2[2] == K.FLT_MAX
    finally:
        r.close()


@pytest.mark.gpu
def test_the_walk_culls(renderers, reference):
    """tri_tests per near-surface point below 1/16 of terrain_64's 8,192 triangles: a walk that culls sits orders of magnitude
    under that (the host walk: 15 per point), one that does not sits at 1."""
    mesh, pts, kind, free = reference("terrain_64")
    near = np.ascontiguousarray(pts[kind == K.KIND_NEAR])
    n_tris = mesh[1].size // 3
    ctr = renderers("terrain_64").closest_points(near, count_visits=True)["counters"]
    print("terrain_64: %.1f triangle tests and %.1f node visits per near-surface point" % (ctr.tri_tests / len(near), ctr.node_visits / len(near)))
    assert n_tris == 8192 and ctr.node_visits > 0 and ctr.render_ms > 0 and ctr.trace_kernel_ms > 0
    assert ctr.tri_tests / len(near) < n_tris / 16
