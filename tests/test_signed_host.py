"""The definition of prt_signed_distance on the host (tests/signed_host_harness.cpp: a float32 brute force with the PRT_HD functions of
csrc/dev_signed.h and integer accumulators, built here with g++): its sign against the analytic inside tests of the cube and the
L-prism, against a float64 numpy reference with true arccos and against the smooth torus; the angle function against float64 acos;
and the harness once under the address and undefined-behaviour sanitizers."""
from __future__ import annotations


import numpy as np
import pytest

import closest_cases as K
import signed_cases as S


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("signed_host")


@pytest.fixture(scope="module")
def results(workdir):
    """name -> (mesh, points, harness answers) of the five meshes' recipe points, computed in one run."""
    exe = S.build_harness(workdir)
    meshes = {name: S.mesh_of(name) for name in S.MESHES}
    points = {name: S.recipe_points(meshes[name], S.POINTS, S.SEEDS[name]) for name in S.MESHES}
    out = S.run_harness(exe, [S.case(meshes[name], points[name]) for name in S.MESHES], workdir)
    return {name: (meshes[name], points[name], res) for name, res in zip(S.MESHES, out)}


def test_meshes_are_closed_and_consistently_wound():
    sizes = {"tetrahedron": 4, "cube": 12, "l_prism": 20, "torus": 576, "fan": 400}
    for name, n_tris in sizes.items():
        p, idx, runs = S.mesh_of(name)
        tri = idx.reshape(-1, 3).astype(np.int64)
        assert len(tri) == n_tris, name
        directed = np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]])
        keys = set(map(tuple, directed))
        assert len(keys) == len(directed), name + ": a directed edge occurs twice"
        assert all((b, a) in keys for a, b in keys), name + ": an edge without its opposite"
        P = p.astype(np.float64)
        volume = (P[tri[:, 0]] * np.cross(P[tri[:, 1]], P[tri[:, 2]])).sum() / 6.0
        assert volume > 0, name + ": inward winding"
    apex = (S.fan()[1] == 0).sum()
    assert apex == 200


def test_every_region_occurs_in_every_batch(results):
    for name, (mesh, pts, res) in results.items():
        assert set(np.unique(res["feature"])) >= set(range(7)), (name, np.unique(res["feature"]))
        assert np.all(res["group"] == 0)
        assert np.array_equal(np.abs(res["signed_distance"]), np.sqrt(res["dist2"]))


def test_points_on_the_surface_take_the_non_negative_branch(workdir):
    """Vertices and float32 edge midpoints: d2 == 0 gives +0, never -0.  (Within an ulp of the coordinates of the surface p - q is
    rounding noise, so the sign of a midpoint that rounding moved off its edge is not compared with anything.)"""
    exe = S.build_harness(workdir)
    names = ("cube", "l_prism", "torus")
    meshes = [S.mesh_of(name) for name in names]
    out = S.run_harness(exe, [S.case(mesh, S.surface_points(mesh, 128, 7)) for mesh in meshes], workdir)
    for name, res in zip(names, out):
        on = res["dist2"] == 0
        assert on.sum() >= 64, name                              # every vertex, and the midpoints that are exact
        assert np.all(res["signed_distance"][on] == 0) and not np.any(np.signbit(res["signed_distance"][on])), name
        assert np.all(res["feature"] <= 6) and np.array_equal(np.abs(res["signed_distance"]), np.sqrt(res["dist2"])), name
    assert np.all(out[0]["dist2"] == 0) and np.all(out[1]["dist2"] == 0), "the cube's and the prism's midpoints are exact"


@pytest.mark.parametrize("name,inside", [("cube", S.inside_cube), ("l_prism", S.inside_l_prism)])
def test_sign_equals_the_analytic_inside_test(results, name, inside):
    """Every point at least 1e-4 x extent from the surface (by the float64 reference's distance) is checked: no wrong sign; at
    least 95 % of the points are checked."""
    mesh, pts, res = results[name]
    extent = K.mesh_extent(mesh)[2]
    ref_sd, _, _ = S.reference(mesh, pts)
    checked = np.abs(ref_sd) >= 1e-4 * extent
    wrong = (res["signed_distance"] < 0) != inside(pts)
    print("%s: %d of %d points checked (%.1f %%), %d wrong signs" % (name, checked.sum(), len(pts), 100.0 * checked.mean(), (wrong & checked).sum()))
    assert checked.mean() >= 0.95
    assert not np.any(wrong & checked), np.nonzero(wrong & checked)[0][:10]


def test_torus_sign_equals_the_float64_reference(results):
    """On every point of the torus batch the harness's sign is the float64 reference's, also where float32 takes another region."""
    mesh, pts, res = results["torus"]
    ref_sd, ref_region, _ = S.reference(mesh, pts)
    wrong = (res["signed_distance"] < 0) != (ref_sd < 0)
    print("torus: %d wrong signs against the float64 reference (largest |reference distance| among them %.3e), %d points in another "
          "region than the reference's" % (wrong.sum(), np.abs(ref_sd[wrong]).max() if wrong.any() else 0.0, (res["feature"] != ref_region).sum()))
    assert not np.any(wrong), (np.nonzero(wrong)[0][:10], res["signed_distance"][wrong][:10], ref_sd[wrong][:10])


def test_torus_sign_equals_the_smooth_torus(results):
    mesh, pts, res = results["torus"]
    sdf = S.torus_sdf(pts)
    far = np.abs(sdf) >= 0.05
    print("torus: %d of %d points at least 0.05 from the smooth torus" % (far.sum(), len(pts)))
    assert far.sum() >= len(pts) // 8
    assert not np.any(((res["signed_distance"] < 0) != (sdf < 0)) & far)


def test_angle_function_against_float64_acos(workdir, results):
    """signed_acos over a dense sweep of [-1, 1] against float64 acos of the same float32 argument, and the harness's angles of
    every test mesh against the float64 angles (atan2 of the cross and dot products of the float32 corners).  The largest errors
    are printed; DESIGN.md section 4.12 records them.  The bounds: the polynomial of Abramowitz & Stegun 4.4.46 is within 2e-8 of
    acos, its float32 evaluation (8 Horner steps on values <= pi / 2, one sqrtf, one product, one subtraction from pi) adds a few
    ulps of pi: 2^-20 (9.5e-7) covers both.  A mesh angle also carries the rounding of its float32 argument
    x = dot(u, v) / sqrtf(dot(u, u) * dot(v, v)): three roundings in each dot product, one each in the product, the square root (halved)
    and the division, at most 8 x 2^-24 in x, which acos magnifies by 1 / sin(angle).  The test meshes' angles lie between 0.015 and
    pi - 0.015 (asserted), so a mesh angle is within 8 x 2^-24 / sin(0.015) + 2^-20 = 3.3e-5."""
    exe = S.build_harness(workdir)
    n = 3 * (1 << 18)
    x = np.concatenate([np.linspace(-1.0, 1.0, n - 6), [-1.0, 1.0, 0.0, -0.0, np.nextafter(np.float32(1), np.float32(0)),
                                                         np.nextafter(np.float32(-1), np.float32(0))]]).astype(np.float32)
    got = S.run_harness(exe, [S.sweep(x)], workdir)[0]["acos"]
    err = np.abs(got.astype(np.float64) - np.arccos(x.astype(np.float64)))
    print("signed_acos: largest error over %d arguments in [-1, 1]: %.3e at x = %r" % (x.size, err.max(), float(x[err.argmax()])))
    assert err.max() <= 2.0 ** -20
    worst = 0.0
    for name, (mesh, pts, res) in results.items():
        alpha, keep = S.mesh_angle_cosines(mesh)
        assert keep.all() and alpha.min() > 0.015 and alpha.max() < np.pi - 0.015, name
        e = np.abs(res["angles"].astype(np.float64) - alpha).max()
        print("%s: largest angle error %.3e (angles %.4f .. %.4f)" % (name, e, alpha.min(), alpha.max()))
        worst = max(worst, e)
    assert worst <= 8.0 * 2.0 ** -24 / np.sin(0.015) + 2.0 ** -20


def test_harness_under_the_sanitizers(workdir):
    exe = S.build_harness(workdir, sanitize=True)
    mesh = S.l_prism()
    pts = S.recipe_points(mesh, 256, 5)
    bad = pts.copy()
    bad[::7, 1] = np.nan
    radius2 = np.full(256, 0.01, np.float32)
    empty = (mesh[0], np.zeros(0, np.uint32), np.zeros((0, 2), np.uint32))
    out = S.run_harness(exe, [S.case(mesh, pts), S.case(mesh, bad, radius2), S.case(empty, pts[:8]), S.sweep(np.linspace(-1, 1, 30))], workdir)
    assert np.all(out[2]["feature"] == 255) and np.all(out[2]["signed_distance"] == S.FLT_MAX)
    assert np.all(out[1]["feature"][::7] == 255)
    plain = S.run_harness(S.build_harness(workdir), [S.case(mesh, pts)], workdir)[0]
    S.assert_same_bits(out[0], plain, "sanitized and plain harness")
