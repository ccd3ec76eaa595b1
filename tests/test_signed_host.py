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
    # the scale sweep (the exponent arithmetic of pow2_of, up to both ends of its clamp) and the topologies
    cases = []
    for name in K.SWEEP_CLOSED:
        m, p = K.sweep_mesh(name), K.sweep_points(name)[:256]
        best = K.true_distance(m, p)
        cases += [S.case(*K.sweep_case(m, p, best, e)[:2]) for e in K.SWEEP_EXPONENTS]
    cases.append(S.case((np.ldexp(S.cube()[0], -140).astype(np.float32),) + S.cube()[1:], np.ldexp(K.sweep_points("cube")[:256], -140).astype(np.float32)))
    cases.append(S.case((np.ldexp(S.cube()[0], 126).astype(np.float32),) + S.cube()[1:], np.ldexp(K.sweep_points("cube")[:256], 100).astype(np.float32)))
    n_sweep = len(cases) - 2
    for name in S.TOPOLOGIES:
        m, p = S.topology_case(name)
        cases.append(S.case(m, p[:256]))
    out = S.run_harness(exe, cases, workdir)
    assert all(np.all(res["group"] >= 0) for res in out[:n_sweep])


# ---- float64 truth at every scale (closest_cases.SWEEP_EXPONENTS)

@pytest.fixture(scope="module")
def sweep(workdir):
    """(name, e) -> (mesh, kept points, float64 minimum, reference signed distance and region - all unscaled - and the harness's
    answers on mesh x 2^e and points x 2^e), and name -> the share of the batch that the filter keeps per exponent."""
    exe = S.build_harness(workdir)
    keys, cases, truth, shares = [], [], {}, {}
    for name in K.SWEEP_CLOSED:
        mesh, pts = K.sweep_mesh(name), K.sweep_points(name)
        best = K.true_distance(mesh, pts)
        ref_sd, ref_region, _ = S.reference(mesh, pts)
        for e in K.SWEEP_EXPONENTS:
            big, big_pts, keep = K.sweep_case(mesh, pts, best, e)
            keys.append((name, e))
            cases.append(S.case(big, big_pts))
            truth[name, e] = (mesh, pts[keep], best[keep], ref_sd[keep], ref_region[keep])
            shares.setdefault(name, {})[e] = float(keep.mean())
    out = S.run_harness(exe, cases, workdir)
    return {k: truth[k] + (res,) for k, res in zip(keys, out)}, shares


def test_the_sweeps_filter_keeps_seven_eighths_of_every_batch(sweep):
    for name, per in sweep[1].items():
        print(name, "kept:", ", ".join("2^%d %.4f" % (e, s) for e, s in per.items()))
        assert min(per.values()) >= 7.0 / 8.0, (name, per)
        assert per[0] == 1.0, (name, per)                     # the 2^0 batch holds every other batch's points


@pytest.mark.parametrize("name", K.SWEEP_CLOSED)
def test_signed_distance_against_float64_at_every_scale(sweep, name):
    """Conditions a to d of the sweep on the harness, and the two reported counts (e)."""
    from test_closest_host import LIMIT_UNITS
    base = sweep[0][name, 0][5]
    for e in K.SWEEP_EXPONENTS:
        mesh, pts, best, ref_sd, ref_region, res = sweep[0][name, e]
        what = "%s x 2^%d" % (name, e)
        excess, root = K.assert_sweep_answers(res, mesh, pts, best, e, LIMIT_UNITS, what)
        checked = S.assert_sweep_signs(res["signed_distance"], name, mesh, pts, ref_sd, what)
        angle = S.assert_sweep_angles(res["angles"], mesh, what)
        assert np.array_equal(np.abs(res["signed_distance"]), np.sqrt(res["dist2"])), what
        # e: reported only.  The 2^0 batch holds every point of the others (the filter keeps all of it), in the same order
        at = np.nonzero(K.sweep_keep(sweep[0][name, 0][2], e))[0]
        inexact = int((np.ldexp(base["signed_distance"][at].astype(np.float64), e) != res["signed_distance"]).sum() +
                      (base["feature"][at] != res["feature"]).sum()) if len(at) == len(pts) else -1
        print("%s: %d points, %d signs checked, excess %.3f and sqrt(d2) %.3f units (limit %.3f), angle error %.2e, %d regions other than "
              "float64's, %d answers not 2^e x the 2^0 answer" % (what, len(pts), checked, excess, root, LIMIT_UNITS, angle,
                                                                  int((res["feature"] != ref_region).sum()), inexact))


# ---- the topologies of the definition (signed_cases.TOPOLOGIES)

@pytest.fixture(scope="module")
def topologies(workdir):
    """name -> (mesh, points, harness answers); also "torus" on multi_group's points and "cube" on degenerate's."""
    exe = S.build_harness(workdir)
    cases = {name: S.topology_case(name) for name in S.TOPOLOGIES}
    cases["torus"] = (S.torus(), cases["multi_group"][1])
    cases["cube"] = (S.cube(), cases["degenerate"][1])
    out = S.run_harness(exe, [S.case(mesh, pts) for mesh, pts in cases.values()], workdir)
    return {name: cases[name] + (res,) for name, res in zip(cases, out)}


def edge_uses(mesh):
    """How many triangles use each undirected edge of position indices (zero-length edges (a, a) left out)."""
    tri = mesh[1].reshape(-1, 3).astype(np.int64)
    pairs = np.sort(np.concatenate([tri[:, [0, 1]], tri[:, [0, 2]], tri[:, [1, 2]]]), axis=1)
    return np.unique(pairs[pairs[:, 0] != pairs[:, 1]], axis=0, return_counts=True)[1]


def test_topologies_are_what_their_names_say():
    for name in S.TOPOLOGIES:
        mesh = S.TOPOLOGIES[name]()
        assert mesh[1].size // 3 <= 2000 and mesh[2][:, 1].sum() == mesh[1].size, name
    uses = edge_uses(S.open_sheet())
    assert (uses == 1).sum() == 4 * 16 and set(uses) == {1, 2}, "the rim's edges have one triangle"
    p, idx, runs = S.unwelded(S.cube())
    assert len(p) == 36 and np.all(edge_uses((p, idx, runs)) == 1) and len(np.unique(p, axis=0)) == 8
    assert sorted(edge_uses(S.non_manifold())) == [1] * 9 + [2] * 3 + [3]
    p, idx, runs = S.back_to_back()
    tri = idx.reshape(-1, 3)
    assert np.array_equal(tri[128:], tri[:128][:, [0, 2, 1]]) and np.all(edge_uses((p, idx, runs)) % 2 == 0)
    p, idx, runs = S.unreferenced_and_repeated()
    assert sorted(set(range(len(p))) - set(idx.tolist())) == [0, 9, 10] and idx.reshape(-1, 3)[-1].tolist() == [1, 1, 8]
    p, idx, runs = S.multi_group(S.torus())
    assert runs[:, 0].tolist() == [384 * 3, 0, 192 * 3] and np.all(runs[:, 1] == 192 * 3)
    key = lambda t: sorted(map(tuple, t.reshape(-1, 3).tolist()))       # noqa: E731
    assert key(idx) == key(S.torus()[1]) and np.array_equal(p, S.torus()[0])


def test_every_region_occurs_on_every_topology(topologies):
    """Every region code in every batch - but one: on with_degenerates(cube) edge bc never wins.  Its 128 zero-area records
    (a, b, midpoint) and (a, a, b) on random vertex pairs cover all 28 pairs of the cube's 8 vertices (asserted), so on every edge of
    the cube a record of group 0 ties with the real triangles, wins by group order, and names the edge ab or ac."""
    for name in S.TOPOLOGIES:
        mesh, pts, res = topologies[name]
        seen = set(np.unique(res["feature"]))
        print(name, "points per region:", np.bincount(res["feature"], minlength=7).tolist(), "negative:", int((res["signed_distance"] < 0).sum()))
        assert len(pts) == S.TOPOLOGY_POINTS and np.all(res["group"] >= 0)
        assert seen >= set(range(7)) - ({5} if name == "degenerate" else set()), (name, seen)
        assert np.array_equal(np.abs(res["signed_distance"]), np.sqrt(res["dist2"])), name
    mesh = S.degenerate_cube()
    flat = mesh[1].reshape(-1, 3)[:2 * K.DEGENERATE_PER_FORM]
    pairs = {tuple(sorted((int(t[0]), int(t[1]) if t[1] != t[0] else int(t[2])))) for t in flat}
    assert len(pairs) == 28


def test_signs_on_the_topologies(topologies):
    """open, non_manifold, unwelded, unreferenced, multi_group: the float64 reference's sign at every point 1e-4 extents off the
    surface.  back_to_back: the accumulators cancel to exactly 0, so no vertex or edge answer is negative; an interior answer is
    signed by the winner's own cross product - and the two copies of a triangle round d2 differently (ab and ac change places), so
    which copy wins, and with it the interior sign, is decided by the last bit of d2: the sign is the winner's side, no more.  multi_group: the one-group torus's signed_distance bits.
    degenerate: how many signs differ from the plain cube's analytic inside test - a property of the definition that
    DESIGN.md section 4.12 records, not a gate."""
    for name in ("open", "non_manifold", "unwelded", "unreferenced", "multi_group"):
        mesh, pts, res = topologies[name]
        ref_sd = S.reference(mesh, pts)[0]
        checked = S.assert_sweep_signs(res["signed_distance"], name, mesh, pts, ref_sd, name)
        assert checked >= 0.95 * len(pts), (name, checked)
    mesh, pts, res = topologies["back_to_back"]
    edge = res["feature"] <= 5
    assert edge.sum() > 200 and not np.any(res["signed_distance"][edge] < 0) and not np.any(np.signbit(res["signed_distance"][edge]))
    tri = K.input_triangle(mesh, res["group"], res["vertex0"])
    print("back_to_back: %d of %d answers name a reversed copy" % ((tri >= mesh[1].size // 6).sum(), len(tri)))
    a, b, c = (x.astype(np.float64) for x in K.corners(mesh, tri))
    side = ((pts - res["point"].astype(np.float64)) * np.cross(b - a, c - a)).sum(1)
    inner = ~edge & (np.sqrt(res["dist2"]) >= S.OFF_SURFACE * K.mesh_extent(mesh)[2])
    assert inner.sum() > 500 and np.array_equal(res["signed_distance"][inner] < 0, side[inner] < 0)
    assert (res["signed_distance"][inner] < 0).sum() > 100
    S.assert_same_bits(topologies["multi_group"][2], topologies["torus"][2], "three shuffled groups and one", ("dist2", "signed_distance"))
    mesh, pts, res = topologies["degenerate"]
    inside = S.inside_cube(pts)
    assert not np.any((topologies["cube"][2]["signed_distance"] < 0) != inside)
    changed = (res["signed_distance"] < 0) != inside
    print("with_degenerates(cube): %d of %d points take another sign than the plain cube's inside test (%d answers name a zero-area record, "
          "%d triangles contribute nothing)" % (changed.sum(), len(pts), (res["group"] == 0).sum(), np.isnan(res["angles"]).any(1).sum()))
    assert np.all(inside[changed]) and not np.any(res["signed_distance"][res["group"] == 0] < 0), "a zero-area record has no normal: never negative"


def test_signed_distance_at_the_bounds_of_dist2(workdir):
    """The documented range is that of dist2 (include/prt.h).  Above: the cube x 2^58 with its whole batch - the points whose true
    dist2 reaches 2^128 miss (FLT_MAX, feature 255), the others keep their sign.  Below: the cube x 2^-70 - nearly every dist2 is
    subnormal or 0, signed_distance is +-sqrtf of it, +0 where it is 0, and the sign of every point whose dist2 is still a
    positive float is the unscaled cube's."""
    exe = S.build_harness(workdir)
    mesh, pts = K.sweep_mesh("cube"), K.sweep_points("cube")
    best = K.true_distance(mesh, pts)
    ref_sd = S.reference(mesh, pts)[0]
    up, down = (S.case(K.scaled(mesh, e), np.ldexp(pts, e).astype(np.float32)) for e in (58, -70))
    big, small = S.run_harness(exe, [up, down], workdir)
    over = (best * 2.0 ** 58) ** 2 >= 2.0 ** 128
    margin = np.abs(np.log2(np.maximum(best, 1e-300)) - 6.0) > 0.01           # not within rounding of the bound 2^64 / 2^58
    missed = big["group"] < 0
    assert over.sum() > 16 and np.array_equal(missed[margin], over[margin])
    assert np.all(big["signed_distance"][missed] == S.FLT_MAX) and np.all(big["feature"][missed] == 255)
    S.assert_sweep_signs(big["signed_distance"][~missed], "cube", mesh, pts[~missed], ref_sd[~missed], "cube x 2^58, every point that hits")
    tiny = small["dist2"] < np.float32(2.0 ** -126)                         # all but the far points: subnormal, or rounded to 0
    assert np.all(small["group"] >= 0) and tiny.sum() > 800 and (tiny & (small["dist2"] > 0)).sum() > 200
    assert np.array_equal(np.abs(small["signed_distance"]), np.sqrt(small["dist2"]))
    zero = small["dist2"] == 0
    assert not np.any(np.signbit(small["signed_distance"][zero]))
    S.assert_sweep_signs(small["signed_distance"][~zero], "cube", mesh, pts[~zero], ref_sd[~zero], "cube x 2^-70, dist2 > 0")
