"""prt_signed_distance on the GPU against the brute force of tests/signed_host_harness.cpp (the definition with the PRT_HD functions of
csrc/dev_signed.h and integer accumulators, built here with g++): signed_distance, feature and the five closest fields bit for bit,
through the host entry point (numpy) and the device entry point (torch), on the SAH tree, the LBVH tree, the 8-wide library, the
stack overflow path and a refitted tree; eight scales from 2^-45 to 2^58 against float64; open, unwelded, non-manifold, cancelling,
degenerate and multi-group meshes, each moved and moved back; permutations, contention at a vertex of 200 triangles, radii, invalid points, the empty
scene, the errors, and signed_distance_differentiable."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import closest_cases as K
import signed_cases as S
from conftest import ROOT

NAMES = ("cube", "l_prism", "torus", "fan") + S.GPU_FIXTURES


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("signed_gpu")


@pytest.fixture(scope="module")
def brute(workdir):
    """brute(mesh, points, max_dist2=None) -> the harness's answers {field: array}."""
    exe = S.build_harness(workdir)

    def run(mesh, points, max_dist2=None):
        return S.run_harness(exe, [S.case(mesh, points, max_dist2)], workdir)[0]
    return run


@pytest.fixture(scope="module")
def reference(brute):
    """name -> (mesh, points, harness answers) of a mesh's recipe points, computed once."""
    cache = {}

    def get(name):
        if name not in cache:
            mesh = S.mesh_of(name)
            pts = S.recipe_points(mesh, S.POINTS, S.SEEDS[name])
            cache[name] = (mesh, pts, brute(mesh, pts))
        return cache[name]
    return get


def upload(r, name):
    from conftest import host_scene
    r.upload(host_scene(name, 0) if name in S.GPU_FIXTURES else S.flat_desc(S.mesh_of(name)))


@pytest.fixture(scope="module")
def renderers():
    from par_raytracer_amd import api
    out = {}

    def get(name, builder="sah"):
        if (name, builder) not in out:
            r = api.Renderer(0)
            if builder != "sah":
                r.set_option("BVH_BUILDER", builder)
            upload(r, name)
            out[(name, builder)] = r
        return out[(name, builder)]
    yield get
    for r in out.values():
        r.close()


def both_paths(r, pts, what, expect, max_dist=None):
    """The batch through the numpy and the torch path: the seven fields of both equal `expect`, and the five closest fields equal
    prt_closest_points on the same context."""
    import torch
    res = r.signed_distance(pts, max_dist=max_dist)
    assert res["counters"].ray_count == len(pts) and res["counters"].pipeline == 0
    S.assert_same_bits(res, expect, what + " (numpy)")
    miss = expect["group"] < 0
    assert np.array_equal(res["inside"], expect["signed_distance"] < 0) and not np.any(res["inside"][miss])
    assert np.all(res["feature"][miss] == 255) and np.all(res["signed_distance"][miss] == S.FLT_MAX) and np.all(res["feature"][~miss] <= 6)
    K.assert_same_bits(r.closest_points(pts, max_dist=max_dist), res, what + " (prt_closest_points)")
    dev = torch.device("cuda", r.device_id)
    pts_t = torch.from_numpy(pts).to(dev)
    dist_t = None if max_dist is None else torch.from_numpy(max_dist).to(dev)
    res_t = r.signed_distance(pts_t, max_dist=dist_t)
    S.assert_same_bits(S.to_numpy(res_t), expect, what + " (torch)")
    assert res_t["feature"].dtype == torch.uint8 and res_t["inside"].dtype == torch.bool
    K.assert_same_bits(K.to_numpy(r.closest_points(pts_t, max_dist=dist_t)), expect, what + " (prt_closest_points_device)")


@pytest.mark.gpu
def test_wave_boundaries_on_the_tetrahedron(brute):
    from par_raytracer_amd import api
    mesh = S.tetrahedron()
    r = api.Renderer(0)
    try:
        r.upload(S.flat_desc(mesh))
        for n in (1, 64, 65):
            pts = np.ascontiguousarray(S.recipe_points(mesh, 128, 40 + n)[:n])
            both_paths(r, pts, "tetrahedron, %d points" % n, brute(mesh, pts))
        on = S.surface_points(mesh, 65, 3)                        # vertices and edge midpoints: d2 == 0, the non-negative branch
        expect = brute(mesh, on)
        assert np.all(expect["dist2"] == 0) and not np.any(np.signbit(expect["signed_distance"]))
        both_paths(r, on, "tetrahedron, points on the surface", expect)
    finally:
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("builder", ["sah", "lbvh"])
def test_meshes_equal_the_brute_force(renderers, reference, name, builder):
    mesh, pts, expect = reference(name)
    both_paths(renderers(name, builder), pts, "%s / %s" % (name, builder), expect)
    if name != "cornell_box":                                   # (open: a side, not an occupancy)
        assert set(np.unique(expect["feature"])) >= set(range(7)), "every region occurs"


def signed_sweep(exe, directory, name, what):
    """One closed mesh of the float64 sweep (K.SWEEP_EXPONENTS) on contexts of its own, one per builder, uploaded once per exponent:
    the harness's bits on all seven fields at the default stack and at STACK_CAP=2 through both entry points, and conditions a, b
    and c on the harness's and on the device's own answers (tests/test_signed_host.py proves the cases)."""
    import torch
    from par_raytracer_amd import api
    from test_closest_host import LIMIT_UNITS
    mesh, pts = K.sweep_mesh(name), K.sweep_points(name)
    best = K.true_distance(mesh, pts)
    ref_sd = S.reference(mesh, pts)[0]
    cases = [K.sweep_case(mesh, pts, best, e) for e in K.SWEEP_EXPONENTS]
    expects = S.run_harness(exe, [S.case(big, big_pts) for big, big_pts, keep in cases], directory)

    def conditions(res, keep, e, who):
        K.assert_sweep_answers(res, mesh, pts[keep], best[keep], e, LIMIT_UNITS, who)
        assert S.assert_sweep_signs(res["signed_distance"], name, mesh, pts[keep], ref_sd[keep], who) >= 0.9 * keep.sum()
    made = {builder: api.Renderer(0) for builder in ("sah", "lbvh")}
    try:
        for builder, r in made.items():
            r.set_option("BVH_BUILDER", builder)
            dev = torch.device("cuda", r.device_id)
            for e, (big, big_pts, keep), expect in zip(K.SWEEP_EXPONENTS, cases, expects):
                who = "%s x 2^%d / %s / %s" % (name, e, builder, what)
                assert keep.mean() >= 7.0 / 8.0, who
                conditions(expect, keep, e, who + ", brute force")
                S.assert_sweep_angles(expect["angles"], mesh, who)
                r.upload(S.flat_desc(big))
                for cap in (None, 2):
                    r.set_option("STACK_CAP", cap)
                    both_paths(r, big_pts, "%s / STACK_CAP=%s" % (who, cap), expect)
                    conditions(r.signed_distance(big_pts), keep, e, who + ", device (numpy)")
                    conditions(S.to_numpy(r.signed_distance(torch.from_numpy(big_pts).to(dev))), keep, e, who + ", device (torch)")
                r.set_option("STACK_CAP", None)
    finally:
        for r in made.values():
            r.close()


def topology_round_trip(exe, directory, name, builders, what):
    """One mesh of S.TOPOLOGIES: the harness's bits on all seven fields through both entry points, then after an update_geometry
    to the sheared mirror image and after one back, each time on the moved context and on a fresh upload."""
    from par_raytracer_amd import api
    mesh, pts = S.topology_case(name)
    moved, pts_moved = S.sheared_mirror(mesh), S.sheared_mirror_points(pts)
    here, there = S.run_harness(exe, [S.case(mesh, pts), S.case(moved, pts_moved)], directory)
    for builder in builders:
        r = api.Renderer(0)
        try:
            if builder != "sah":
                r.set_option("BVH_BUILDER", builder)
            r.upload(S.flat_desc(mesh))
            both_paths(r, pts, "%s / %s / %s" % (name, builder, what), here)
            for at, at_pts, expect, step in ((moved, pts_moved, there, "moved"), (mesh, pts, here, "moved back")):
                r.update_geometry(at[0])
                both_paths(r, at_pts, "%s / %s / %s, %s" % (name, builder, what, step), expect)
                fresh = api.Renderer(0)
                try:
                    if builder != "sah":
                        fresh.set_option("BVH_BUILDER", builder)
                    fresh.upload(S.flat_desc(at))
                    S.assert_same_bits(fresh.signed_distance(at_pts), expect, "%s / %s / %s, %s, fresh upload" % (name, builder, what, step))
                finally:
                    fresh.close()
        finally:
            r.close()
    return here


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(S.TOPOLOGIES))
def test_topologies_equal_the_brute_force(workdir, name):
    """Boundary edges, unwelded vertices, an edge of three triangles, accumulators that cancel, zero-area records that win ties,
    unused positions and three shuffled groups (tests/test_signed_host.py proves the cases and what their signs mean)."""
    expect = topology_round_trip(S.build_harness(workdir), workdir, name, ("sah", "lbvh"), "4-wide")
    if name == "back_to_back":
        assert not np.any(expect["signed_distance"][expect["feature"] <= 5] < 0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", K.SWEEP_CLOSED)
def test_float64_truth_at_every_scale(workdir, name):
    signed_sweep(S.build_harness(workdir), workdir, name, "4-wide")


@pytest.mark.gpu
def test_the_bounds_of_dist2(brute):
    """The cube x 2^58 with its whole batch (the far points' dist2 overflows: misses) and x 2^-70 (dist2 subnormal or 0: +0, never
    -0) - the harness's bits, which tests/test_signed_host.py holds against the unscaled cube."""
    from par_raytracer_amd import api
    mesh, pts = K.sweep_mesh("cube"), K.sweep_points("cube")
    for e in (58, -70):
        big, big_pts = K.scaled(mesh, e), np.ldexp(pts, e).astype(np.float32)
        expect = brute(big, big_pts)
        assert (expect["group"] < 0).any() == (e == 58) and not np.any(np.signbit(expect["signed_distance"][expect["dist2"] == 0]))
        r = api.Renderer(0)
        try:
            r.upload(S.flat_desc(big))
            both_paths(r, big_pts, "cube x 2^%d" % e, expect)
        finally:
            r.close()


CHILD = r"""
import os, sys, tempfile
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, "tests")); sys.path.insert(0, os.path.join(%(root)r, "oracle"))
import numpy as np
import signed_cases as S
import closest_cases as K
from test_gpu_signed import NAMES, both_paths, signed_sweep, topology_round_trip, upload
from par_raytracer_amd import api, capi
lib = capi.hip_lib()
assert os.path.basename(lib._name) == "libprt_hip_bvh8.so" and not (lib.prt_build_flags() & capi.BUILD_BVH4)
d = tempfile.mkdtemp(prefix="prt_signed8_")
exe = S.build_harness(d)
meshes = {name: S.mesh_of(name) for name in NAMES}
points = {name: S.recipe_points(meshes[name], S.POINTS, S.SEEDS[name]) for name in NAMES}
results = S.run_harness(exe, [S.case(meshes[name], points[name]) for name in NAMES], d)
for name, res in zip(NAMES, results):
    r = api.Renderer(0)
    upload(r, name)
    both_paths(r, points[name], name + " / 8-wide", res)
    print(name, "equal", flush=True)
    r.close()
for name in S.TOPOLOGIES:
    topology_round_trip(exe, d, name, ("sah",), "8-wide")
    print(name, "topology ok", flush=True)
for name in K.SWEEP_CLOSED:
    signed_sweep(exe, d, name, "8-wide")
    print(name, "sweep ok", flush=True)
print("bvh8 signed distance ok")
"""


@pytest.mark.gpu
def test_meshes_on_the_8_wide_library():
    assert os.path.exists(os.path.join(ROOT, "par_raytracer_amd", "libprt_hip_bvh8.so")), "libprt_hip_bvh8.so not built (make hip-bvh8)"
    env = dict(os.environ)
    env["PRT_HIP_LIB"] = "libprt_hip_bvh8.so"
    out = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         timeout=600)
    assert out.returncode == 0 and b"bvh8 signed distance ok" in out.stdout, (out.returncode, out.stdout.decode()[-1500:],
                                                                              out.stderr.decode()[-3000:])


@pytest.mark.gpu
def test_stack_overflow_path(reference):
    from par_raytracer_amd import api
    mesh, pts, expect = reference("icosphere_l3")
    r = api.Renderer(0)
    try:
        upload(r, "icosphere_l3")
        plain = r.signed_distance(pts, count_visits=True)
        r.set_option("STACK_CAP", 2)        # the marker and one entry: nearly every push is dropped, the points go to k_closest_exact
        capped = r.signed_distance(pts, count_visits=True)
        r.set_option("STACK_CAP", None)
    finally:
        r.close()
    S.assert_same_bits(plain, expect, "default stack")
    S.assert_same_bits(capped, expect, "STACK_CAP=2")
    assert capped["counters"].node_visits != plain["counters"].node_visits      # a listed point is walked twice


@pytest.mark.gpu
def test_permutation_and_repetition(renderers, reference):
    mesh, pts, expect = reference("torus")
    r = renderers("torus")
    perm = np.random.default_rng(11).permutation(len(pts))
    S.assert_same_bits(r.signed_distance(np.ascontiguousarray(pts[perm])), {k: expect[k][perm] for k in S.FIELDS}, "permuted")
    S.assert_same_bits(r.signed_distance(pts), r.signed_distance(pts), "the same batch twice")
    only = r.signed_distance(pts, fields=("feature",))
    assert set(only) == {"feature", "counters"} and np.array_equal(only["feature"], expect["feature"])


@pytest.mark.gpu
def test_fan_from_two_fresh_contexts(reference):
    """200 triangles add to the apex's and to the base centre's accumulator at once: the integer sums do not depend on the order."""
    from par_raytracer_amd import api
    mesh, pts, expect = reference("fan")
    got = []
    for _ in range(2):
        r = api.Renderer(0)
        try:
            upload(r, "fan")
            got.append(r.signed_distance(pts))
        finally:
            r.close()
    S.assert_same_bits(got[0], got[1], "two fresh contexts")
    S.assert_same_bits(got[0], expect, "fan")
    assert (expect["feature"] == 0).sum() > 0 and (expect["signed_distance"] < 0).sum() > 0


@pytest.mark.gpu
def test_moved_scene_equals_a_fresh_upload_and_the_brute_force(brute, reference):
    """Query, move the geometry to a sheared and mirrored copy (the winding stays, so every normal and every sign flips), query
    again: accumulators left over from before the update would give the old signs."""
    from par_raytracer_amd import api
    mesh, pts, before = reference("torus")
    moved = S.sheared_mirror(mesh)
    pts_moved = S.sheared_mirror_points(pts)
    expect = brute(moved, pts_moved)
    r, fresh = api.Renderer(0), api.Renderer(0)
    try:
        r.upload(S.flat_desc(mesh))
        S.assert_same_bits(r.signed_distance(pts), before, "before the update")
        r.update_geometry(moved[0])
        fresh.upload(S.flat_desc(moved))
        S.assert_same_bits(r.signed_distance(pts_moved), expect, "refitted tree")
        S.assert_same_bits(fresh.signed_distance(pts_moved), expect, "fresh upload")
        r.update_geometry(mesh[0])                                # and back again
        S.assert_same_bits(r.signed_distance(pts), before, "moved back")
    finally:
        r.close()
        fresh.close()
    clear = (np.abs(before["signed_distance"]) > 0.01) & (np.abs(expect["signed_distance"]) > 0.01)
    assert clear.sum() > len(pts) // 4 and np.all((before["signed_distance"][clear] < 0) != (expect["signed_distance"][clear] < 0))


@pytest.mark.gpu
def test_radii_invalid_points_and_the_empty_scene(renderers, reference, brute):
    from par_raytracer_amd import api
    mesh, pts, free = reference("icosphere_l3")
    r = renderers("icosphere_l3")
    n = 512
    pts = pts[:n].copy()
    dist = (np.sqrt(free["dist2"][:n]) * np.where(np.arange(n) % 2 == 0, 0.5, 1.5)).astype(np.float32)
    dist[free["dist2"][:n] == 0] = 0.0
    bad = np.array([0, 5, 63, 64, 65, 200, 511])
    for i, (j, val) in enumerate(zip(bad, (np.nan, np.inf, -np.inf, np.nan, np.inf, -np.inf, np.nan))):
        pts[j, i % 3] = val
    dist[[7, 9]] = np.nan
    expect = brute(mesh, pts, (dist * dist).astype(np.float32))
    both_paths(r, pts, "radii and invalid points", expect, max_dist=dist)
    miss = expect["group"] < 0
    assert np.all(miss[bad]) and np.all(miss[[7, 9]]) and miss.sum() > n // 4 and (~miss).sum() > n // 4
    for k in S.FIELDS:
        assert np.all(expect[k][miss] == S.MISS[k]), k
    hit = ~miss
    for k in S.FIELDS:                      # the hits are what they are without a radius
        assert np.array_equal(K.bits(expect[k][hit]) if k != "feature" else expect[k][hit],
                              K.bits(free[k][:n][hit]) if k != "feature" else free[k][:n][hit]), k
    p = mesh[0]
    e = api.Renderer(0)
    try:
        e.upload(S.flat_desc((p, np.zeros(0, np.uint32), np.zeros((0, 2), np.uint32))))
        assert e.scene_info().triangle_count == 0
        res = e.signed_distance(np.ascontiguousarray(pts[:70]))
        for k in S.FIELDS:
            assert np.all(res[k] == S.MISS[k]), k
        assert not np.any(res["inside"])
    finally:
        e.close()


@pytest.mark.gpu
def test_errors_and_count_zero():
    from par_raytracer_amd import api, capi
    lib = capi.hip_lib()
    mesh = S.tetrahedron()
    pts = np.array([[0.1, 0.1, 0.1], [3.0, -1.0, 2.0], [np.nan, 0.0, 0.0]], np.float32)
    sd = np.full(3, 7.5, np.float32)
    feature = np.full(3, 77, np.uint8)
    batch = capi.PrtPointBatch(pts.ctypes.data, None, 3)
    out = capi.PrtSignedBuffers(capi.PrtClosestBuffers(None, None, None, None, None), sd.ctypes.data, feature.ctypes.data)
    r = api.Renderer(0)
    try:
        for entry in (lib.prt_signed_distance, lib.prt_signed_distance_device):
            assert entry(r._ctx, C.byref(batch), C.byref(out), 0, None) == -2, "no scene"
            assert entry(None, C.byref(batch), C.byref(out), 0, None) == -1
        r.upload(S.flat_desc(mesh))
        ctr = capi.PrtCounters()
        for entry in (lib.prt_signed_distance, lib.prt_signed_distance_device):
            null_points = capi.PrtPointBatch(None, None, 3)
            assert entry(r._ctx, C.byref(null_points), C.byref(out), 0, None) == -1
            assert entry(r._ctx, None, C.byref(out), 0, None) == -1 and entry(r._ctx, C.byref(batch), None, 0, None) == -1
            empty = capi.PrtPointBatch(None, None, 0)
            ctr.ray_count = 99
            assert entry(r._ctx, C.byref(empty), C.byref(out), 0, C.byref(ctr)) == 0 and ctr.ray_count == 0
        assert np.all(sd == 7.5) and np.all(feature == 77), "nothing was written"
        assert lib.prt_signed_distance(r._ctx, C.byref(batch), C.byref(out), 0, C.byref(ctr)) == 0 and ctr.ray_count == 3
        assert sd[0] < 0 and 0 < sd[1] < S.FLT_MAX and sd[2] == S.FLT_MAX and list(feature[:2] <= 6) == [True, True] and feature[2] == 255
        with pytest.raises(ValueError):
            r.signed_distance(pts, fields=("sign",))
    finally:
        r.close()


@pytest.fixture(scope="module")
def cube_gradient(reference):
    """signed_distance_differentiable on the cube's recipe points (the first eight moved onto the vertices), its sum back-propagated
    to the points; the same with a radius of 1e-6 that makes most points miss.  Computed once for the two tests below."""
    import torch
    from par_raytracer_amd import api, autograd
    mesh, pts, _ = reference("cube")
    pts = pts.copy()
    pts[:8] = mesh[0]                                            # exactly on the eight vertices
    r = api.Renderer(0)
    try:
        r.upload(S.flat_desc(mesh))
        dev = torch.device("cuda", r.device_id)
        positions = torch.from_numpy(mesh[0]).to(dev)
        p = torch.from_numpy(pts).to(dev).requires_grad_(True)
        sd = autograd.signed_distance_differentiable(r, positions, p)
        res = S.to_numpy(r.signed_distance(p.detach()))
        sd.sum().backward()
        grad = p.grad.cpu().numpy()
        far = autograd.signed_distance_differentiable(r, positions, p, max_dist=torch.full((len(pts),), 1e-6, device=dev), update_geometry=False)
        p.grad = None
        far.sum().backward()
        out = dict(mesh=mesh, pts=pts, res=res, sd=sd.detach().cpu().numpy(), grad=grad, far=far.detach().cpu().numpy(), far_grad=p.grad.cpu().numpy())
    finally:
        r.close()
    e = (pts - res["point"]).astype(np.float64)                   # p - q as the library forms it, in float32
    dist = np.sqrt(res["dist2"].astype(np.float64))
    out["dist"] = dist
    out["want"] = np.where(res["signed_distance"] < 0, -1.0, 1.0)[:, None] * e / dist[:, None].clip(1e-300)
    return out


@pytest.mark.gpu
def test_signed_distance_differentiable_on_the_cube(cube_gradient):
    """The values are Renderer.signed_distance's bits, also under a radius that makes most points miss; the gradient is finite,
    zero on a miss and zero on the surface (the eight vertices)."""
    g = cube_gradient
    res, grad, pts = g["res"], g["grad"], g["pts"]
    assert np.array_equal(K.bits(g["sd"]), K.bits(res["signed_distance"]))
    missed = g["far"] == S.FLT_MAX
    assert missed.sum() > len(pts) // 2 and np.all(g["far_grad"][missed] == 0) and np.all(np.isfinite(g["far_grad"]))
    assert np.array_equal(K.bits(g["far"][~missed]), K.bits(res["signed_distance"][~missed]))
    assert np.all(np.isfinite(grad))
    on = res["dist2"] == 0
    assert np.all(on[:8]) and np.all(grad[on] == 0), "zero gradient on the surface"


@pytest.mark.gpu
def test_point_gradient_equals_the_returned_fields_to_four_ulps(cube_gradient):
    """The gradient with respect to the points equals sign x (p - q) / dist from the returned fields, to 4 float32 ulps of the
    point's largest gradient component: p - q in float32 as the library forms it, then a square root, a division and two products."""
    g = cube_gradient
    res, grad, want = g["res"], g["grad"], g["want"]
    live = res["dist2"] > 0
    tol = 4.0 * 2.0 ** -23 * np.abs(want).max(1, keepdims=True)
    ratio = np.where(live, (np.abs(grad - want) / tol.clip(1e-300)).max(1), 0.0)
    for region in range(7):
        sel = live & (res["feature"] == region)
        print("region %d: %d points, worst %.2f x the tolerance" % (region, sel.sum(), ratio[sel].max() if sel.any() else 0.0))
        assert sel.sum() > 0
    assert ratio.max() <= 1.0
