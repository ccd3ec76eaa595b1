"""prt_closest_points without a GPU: the walk of csrc/dev_closest.h against a brute force of the same function over every triangle
(tests/closest_host_harness.cpp, both tree widths, the SAH builder - the LBVH builder runs on the device only), the function against
a float64 yardstick, one triangle region by region, the harness under the address and undefined-behaviour sanitizers, and the entry
points' argument checks."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import closest_cases as K

# |sqrt(d2) - dist64| in units of 2^-23 x M, M the largest |coordinate| of the point and the three corners: the largest value over
# the four fixtures' recipe points (seeds 100..103), each against the triangle that wins it and three random ones, was measured
# as 1.588 (terrain_64, a near-surface point; cornell_box 1.114, icosphere_l3 1.151, coincident 1.179).  The fixtures only sample the
# error, hence the factor 4.  The culling argument of DESIGN.md section 4.10 needs the limit below 64 units.
MEASURED_MAX_UNITS = 1.588
LIMIT_UNITS = 4.0 * MEASURED_MAX_UNITS
SEEDS = {name: 100 + i for i, name in enumerate(K.FIXTURES)}


@pytest.fixture(scope="module")
def meshes():
    return {name: K.scene_mesh(name) for name in K.FIXTURES}


@pytest.fixture(scope="module")
def points(meshes):
    return {name: K.recipe_points(meshes[name], K.RECIPE_POINTS, SEEDS[name]) for name in K.FIXTURES}


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("closest_host")


@pytest.fixture(scope="module")
def harness4(workdir):
    return K.build_harness(workdir)


@pytest.mark.parametrize("width", [4, 8])
def test_walk_equals_brute_force_bit_for_bit(meshes, points, workdir, harness4, width):
    exe = harness4 if width == 4 else K.build_harness(workdir, bvh8=True)
    near = points["terrain_64"][0][points["terrain_64"][1] == K.KIND_NEAR]
    cases = [K.case(meshes[name], points[name][0]) for name in K.FIXTURES] + [K.case(meshes["terrain_64"], near)]
    results = K.run_harness(exe, cases, workdir)
    for name, r in zip(K.FIXTURES + ("terrain_64 near",), results):
        print(width, name, "mismatches", r["mismatches"], "tie points", r["tie_points"], "tri tests per point",
              r["tri_tests"] / len(r["brute"]["group"]))
        assert r["mismatches"] == 0, (width, name)
        K.assert_same_bits(r["walk"], r["brute"], "%d-wide %s" % (width, name))
        assert np.all(r["brute"]["group"] >= 0), "no radius: every point has an answer"
    assert results[K.FIXTURES.index("coincident")]["tie_points"] > 0, "coincident: no point was decided by the tie rule"
    # the culling condition of the GPU suite, on the host walk first: below 1/16 of the triangles per near-surface point
    n_tris = meshes["terrain_64"][1].size // 3
    assert results[-1]["tri_tests"] / len(near) < n_tris / 16


def test_function_against_the_float64_yardstick(meshes, points, workdir, harness4):
    assert LIMIT_UNITS < 64.0, "the limit must stay below half of what the 2^-16 pad grants, or the culling argument is void"
    rng = np.random.default_rng(7)
    winners = K.run_harness(harness4, [K.case(meshes[name], points[name][0]) for name in K.FIXTURES], workdir)
    cases, tris, pts = [], [], []
    for name, r in zip(K.FIXTURES, winners):
        m, P = meshes[name], points[name][0]
        win = K.input_triangle(m, r["brute"]["group"], r["brute"]["vertex0"])
        tri = np.concatenate([win] + [rng.integers(0, m[1].size // 3, len(P)) for _ in range(3)])
        tris.append(tri)
        pts.append(np.concatenate([P] * 4))
        cases.append(K.case(m, pts[-1], pair_tri=tri))
    worst = 0.0
    for name, tri, PP, r in zip(K.FIXTURES, tris, pts, K.run_harness(harness4, cases, workdir)):
        a, b, c = K.corners(meshes[name], tri)
        dist, v, w, region = K.yardstick(PP, a, b, c)
        assert np.all(r["ok"] == 1), "%s: a fixture triangle is no candidate" % name
        M = np.max(np.abs(np.concatenate([PP, a, b, c], axis=1)), axis=1).astype(np.float64)
        units = np.abs(np.sqrt(r["d2"].astype(np.float64)) - dist) / (2.0 ** -23 * M)
        print("%s: max |sqrt(d2) - dist64| = %.4f units of 2^-23 M (limit %.3f)" % (name, units.max(), LIMIT_UNITS))
        worst = max(worst, float(units.max()))
    print("largest over the fixtures: %.4f units; measured when the limit was set: %.3f" % (worst, MEASURED_MAX_UNITS))
    assert worst <= LIMIT_UNITS


def _region_of(v, w):
    """Region from the barycentrics closest_on_triangle returned (the order of K.yardstick)."""
    if v == 0 and w == 0:
        return 0
    if v == 1 and w == 0:
        return 1
    if w == 0:
        return 2
    if v == 0 and w == 1:
        return 3
    if v == 0:
        return 4
    if v == np.float32(1) - w:
        return 5
    return 6


def test_one_triangle_all_seven_regions(workdir, harness4):
    # legs 2 and 4 along x and y: every dot product below is a short dyadic number and |ab x ac|^2 = 64, so the points placed ON
    # the triangle come out with d2 == 0 exactly
    a, ab, ac = np.array([0.5, -1.0, 2.0]), np.array([2.0, 0.0, 0.0]), np.array([0.0, 4.0, 0.0])
    mesh = (np.array([a, a + ab, a + ac], np.float32), np.array([0, 1, 2], np.uint32), np.array([[0, 3]], np.uint32))
    b, c, nrm = a + ab, a + ac, np.array([0.0, 0.0, 1.0])
    centroid = (a + b + c) / 3
    anchors = {0: a + (a - centroid) * 0.5, 1: b + (b - centroid) * 0.5, 3: c + (c - centroid) * 0.5,
               2: (a + b) / 2 + np.array([0.0, -0.75, 0.0]), 4: (a + c) / 2 + np.array([-0.75, 0.0, 0.0]),
               5: (b + c) / 2 + np.array([0.5, 0.25, 0.0]) * 1.5, 6: a + ab * 0.3 + ac * 0.45}
    pts, expect = [], []
    for region, p in anchors.items():
        for h in (0.375, -0.375, 0.0):                    # both sides of the plane, and in it
            pts.append(p + nrm * h)
            expect.append(region)
    on = {0: a, 2: a + ab * 0.5, 6: a + ab * 0.25 + ac * 0.25, 1: b, 3: c, 4: a + ac * 0.375, 5: b * 0.5 + c * 0.5}
    n_off = len(pts)
    for region, p in on.items():
        pts.append(p)
        expect.append(region)
    pts = np.array(pts, np.float32)
    r = K.run_harness(harness4, [K.case(mesh, pts, pair_tri=np.zeros(len(pts), np.uint32))], workdir)[0]
    dist, v64, w64, region64 = K.yardstick(pts, *K.corners(mesh, np.zeros(len(pts), np.int64)))
    M = np.max(np.abs(np.concatenate([pts, mesh[0].reshape(1, 9).repeat(len(pts), 0)], axis=1)), axis=1).astype(np.float64)
    for i in range(len(pts)):
        assert r["ok"][i] == 1
        if i < n_off:
            assert region64[i] == expect[i], "the construction missed its region"
            assert _region_of(r["v"][i], r["w"][i]) == expect[i], (i, expect[i], r["v"][i], r["w"][i])
        # 16 float32 ulps of 1 on the barycentrics (a handful of roundings on well-conditioned quotients), the suite's limit on the distance
        assert abs(float(r["v"][i]) - v64[i]) <= 2.0 ** -19 and abs(float(r["w"][i]) - w64[i]) <= 2.0 ** -19, i
        assert abs(np.sqrt(float(r["d2"][i])) - dist[i]) <= LIMIT_UNITS * 2.0 ** -23 * M[i], i
        if i >= n_off:
            assert r["d2"][i] == 0.0 and dist[i] == 0.0, (i, r["d2"][i])
    assert sorted(set(expect[:n_off])) == list(range(7))


def test_sanitized_harness_on_icosphere(meshes, points, workdir):
    exe = K.build_harness(workdir, sanitize=True)
    r = K.run_harness(exe, [K.case(meshes["icosphere_l3"], points["icosphere_l3"][0])], workdir)[0]
    assert r["mismatches"] == 0


def test_entry_points_without_a_gpu():
    from par_raytracer_amd import capi
    lib = capi.hip_lib()
    assert lib.prt_abi_version() == 5
    assert "prt_closest_points" in capi.PRT_SYMBOLS and "prt_closest_points_device" in capi.PRT_SYMBOLS
    pts = np.zeros((4, 3), np.float32)
    d2 = np.zeros(4, np.float32)
    batch = capi.PrtPointBatch(pts.ctypes.data, None, 4)
    out = capi.PrtClosestBuffers(d2.ctypes.data, None, None, None, None)
    assert lib.prt_closest_points(None, C.byref(batch), C.byref(out), 0, None) == -1
    assert lib.prt_closest_points_device(None, C.byref(batch), C.byref(out), 0, None) == -1
