"""The case builders of tests/closest_cases.py without a GPU: what tests/test_gpu_closest_schedules.py relies on is proved here
first, on tests/closest_host_harness.cpp (both tree widths unless said) - the walk gives the brute force's bits on degenerate
records, on scenes of every scale and far from the origin; the answers on identical stacked records satisfy expectations that do
not call the tie rule; the batches' expected rows are the brute force's; the stack caps list as many points as the GPU tests
need (the harness walks every point as one lane of k_closest does); and the far point of far_tail changes what is culled."""
from __future__ import annotations

import numpy as np
import pytest

import closest_cases as K
from test_closest_host import LIMIT_UNITS

EXACT_LANES = 64 * 256                   # k_closest_exact's grid (launch_walk)
SCALE_POINTS = 1024
MID_CAP = K.MID_CAP                      # the intermediate caps and their measured shares: tests/closest_cases.py
DEFAULT_CAP = {4: 24, 8: 13}


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("closest_cases_host")


@pytest.fixture(scope="module")
def harness(workdir):
    made = {}

    def get(width):
        if width not in made:
            made[width] = K.build_harness(workdir, bvh8=width == 8)
        return made[width]
    return get


def scale_cases():
    """name -> (mesh, points): the meshes of device test (h) and SCALE_POINTS recipe points on each (K.scale_meshes)."""
    return {name: (mesh, K.recipe_points(mesh, SCALE_POINTS, K.SCALE_SEED)[0]) for name, mesh in K.scale_meshes().items()}


@pytest.mark.parametrize("width", [4, 8])
def test_walk_equals_brute_force_on_every_scale_and_on_degenerate_records(workdir, harness, width):
    cases = scale_cases()
    results = K.run_harness(harness(width), [K.case(m, p, stack_cap=2) for m, p in cases.values()], workdir)
    for name, r in zip(cases, results):
        misses = int((r["brute"]["group"] < 0).sum())
        print(width, name, "mismatches", r["mismatches"], "ties", r["tie_points"], "misses", misses, "listed at cap 2", int(r["listed"].sum()),
              "node visits per point %.1f" % (r["node_visits"] / SCALE_POINTS))
        assert r["mismatches"] == 0, (width, name)
        K.assert_same_bits(r["walk"], r["brute"], "%d-wide %s" % (width, name))
        if name == "2^62":                                    # d2 overflows for the far points: a miss without a radius
            assert 0.05 * SCALE_POINTS < misses < 0.5 * SCALE_POINTS, misses
            assert np.all(r["brute"]["dist2"][r["brute"]["group"] < 0] == K.FLT_MAX)
        elif name == "2^58":                                  # what the device can upload: measured 74 of 1,024
            assert misses > 0 and float(np.abs(cases[name][0][0]).max()) < 1.0e18
        else:
            assert misses == 0, (name, misses)
        assert int(r["listed"].sum()) > 0.75 * (SCALE_POINTS - misses), "device test (h) at STACK_CAP=2 would not use the slow path"
    d2 = results[list(cases).index("2^-70")]["brute"]["dist2"]
    assert np.any((d2 > 0) & (d2 < np.float32(2.0 ** -126))), "2^-70: no subnormal d2"
    assert results[list(cases).index("degenerate")]["brute"]["group"].tolist().count(0) > 0, "no zero-area record wins a point"
    n_tris = cases["+1e6"][0][1].size // 3
    assert n_tris <= 2048 and results[list(cases).index("+1e6")]["tri_tests"] == n_tris * SCALE_POINTS      # every bound ties
    # stacked_copies: the tie rule's answers against expectations that do not call it
    mesh, pts = cases["stacked"]
    r = results[list(cases).index("stacked")]
    assert r["tie_points"] == SCALE_POINTS
    excess = K.assert_stacked_expectations(r["brute"], K.stacked_base(), K.stacked_perm(), pts, LIMIT_UNITS, "%d-wide brute force" % width)
    print("stacked copies: worst excess over the float64 minimum %.3f units (limit %.3f)" % (excess, LIMIT_UNITS))


def test_zero_area_records_are_candidates_in_some_regions_only(workdir, harness):
    """Both behaviours of a zero-area record, on the function alone: rejected (the interior branch divides by zero) for some
    points, a candidate (a vertex or edge region) for others - per form of degenerate triangle."""
    mesh, pts = scale_cases()["degenerate"]
    n_deg = int(mesh[2][0, 1]) // 3
    assert n_deg == 4 * K.DEGENERATE_PER_FORM
    tri = (np.arange(len(pts)) * 7) % n_deg
    r = K.run_harness(harness(4), [K.case(mesh, pts, pair_tri=tri)], workdir)[0]
    form = tri // K.DEGENERATE_PER_FORM
    counts = [(int((r["ok"][form == f] == 1).sum()), int((r["ok"][form == f] == 0).sum())) for f in range(4)]
    print("(candidate, rejected) per form - midpoint, doubled corner, point, sliver:", counts)
    assert (r["ok"] == 0).any() and (r["ok"] == 1).any()
    a, b, c = K.corners(mesh, tri)
    assert not np.cross(b.astype(np.float64) - a, c.astype(np.float64) - a)[form != 0].any(), "forms 1 to 3 have no area at all"


@pytest.mark.parametrize("name", ["icosphere_l3", "terrain_64"])
def test_batches_expected_rows_are_the_brute_forces(workdir, harness, name):
    """sorted_by_kind, its shuffle, tiled and radius_mix: the rows the GPU tests expect, picked from the unique points' brute
    force, are what the brute force gives for the batch itself."""
    mesh = K.scene_mesh(name)
    pts, kind = K.recipe_points(mesh, K.RECIPE_POINTS, K.SCHEDULE_SEEDS[name])
    batch, shuffled = K.sorted_by_kind(pts, kind)
    n = 5 * K.PER
    assert K.PER % 64 == 0 and K.PER > 128 and K.PER % 128 != 0          # whole waves, boundaries of the default chunk inside a run
    assert len(batch["index"]) == n and np.all(batch["index"][4 * K.PER:] == -1) and np.all(batch["index"][:4 * K.PER] >= 0)
    assert np.array_equal(kind[batch["index"][:4 * K.PER]], np.repeat([K.KIND_NEAR, K.KIND_BOX, K.KIND_FAR, K.KIND_ON], K.PER))
    bad_p, bad_r = batch["points"][4 * K.PER:], batch["max_dist2"][4 * K.PER:]
    ways = [np.isnan(bad_p).any(1), np.isposinf(bad_p).any(1), np.isneginf(bad_p).any(1), bad_r < 0, np.isnan(bad_r)]
    assert np.all(np.sum(ways, axis=0) == 1) and all(int(w.sum()) >= K.PER // 5 for w in ways)
    assert np.array_equal(np.sort(shuffled["index"]), np.sort(batch["index"])) and not np.array_equal(shuffled["index"], batch["index"])
    t_pts, t_index = K.tiled(pts, 5000)
    assert len(t_pts) == 5000 and np.array_equal(K.bits(t_pts), K.bits(pts[np.arange(5000) % len(pts)]))
    free, sorted_r, shuffled_r, tiled_r = K.run_harness(harness(4), [
        K.case(mesh, pts), K.case(mesh, batch["points"], batch["max_dist2"]), K.case(mesh, shuffled["points"], shuffled["max_dist2"]),
        K.case(mesh, t_pts)], workdir)
    K.assert_same_bits(sorted_r["brute"], K.rows(free["brute"], batch["index"]), name + " sorted by kind")
    K.assert_same_bits(shuffled_r["brute"], K.rows(free["brute"], shuffled["index"]), name + " shuffled")
    K.assert_same_bits(tiled_r["brute"], K.rows(free["brute"], t_index), name + " tiled")
    # radius_mix: classes 1 and 3 keep the free answer, 0 too; 2, 4 and 5 miss (the next float below d2 excludes the winner)
    r2 = K.radius_mix(free["brute"]["dist2"])
    mixed = K.run_harness(harness(4), [K.case(mesh, pts, r2)], workdir)[0]
    cls = np.arange(len(pts)) % 6
    keep = np.isin(cls, (0, 1, 3))
    K.assert_same_bits(mixed["brute"], K.rows(free["brute"], np.where(keep, np.arange(len(pts)), -1)), name + " radius_mix")
    assert mixed["mismatches"] == 0
    spoiled = K.run_harness(harness(4), [K.case(mesh, *K.spoil_points(300)), K.case(mesh, *K.spoil_points(300, radii=False)),
                                         K.case(mesh, *K.spoil_points(300, pts))], workdir)
    assert np.all(spoiled[0]["brute"]["group"] == -1) and np.all(spoiled[1]["brute"]["group"] == -1) and np.all(spoiled[2]["brute"]["group"] >= 0)


@pytest.mark.parametrize("width", [4, 8])
def test_stack_caps_list_what_the_gpu_tests_need(workdir, harness, width):
    """The harness walks every point as one lane of k_closest does, on an LDS stack of the given cap.  The device's tree may differ
    from the harness's (builder threads, the cost option): conditions with margin, not equalities."""
    exe = harness(width)
    terrain, coincident = K.scene_mesh("terrain_64"), K.scene_mesh("coincident")
    t_pts = K.recipe_points(terrain, K.RECIPE_POINTS, K.SCHEDULE_SEEDS["terrain_64"])[0]
    c_pts = K.recipe_points(coincident, K.RECIPE_POINTS, K.SCHEDULE_SEEDS["coincident"])[0]
    r2 = K.radius_mix(K.run_harness(exe, [K.case(terrain, t_pts)], workdir)[0]["brute"]["dist2"])
    t2, t_mid, t_def, t_r2, c_mid = K.run_harness(exe, [
        K.case(terrain, t_pts, stack_cap=2), K.case(terrain, t_pts, stack_cap=MID_CAP[width]), K.case(terrain, t_pts, stack_cap=DEFAULT_CAP[width]),
        K.case(terrain, t_pts, r2, stack_cap=2), K.case(coincident, c_pts, stack_cap=MID_CAP[width])], workdir)
    n = K.RECIPE_POINTS
    listed = {k: int(r["listed"].sum()) for k, r in dict(cap2=t2, mid=t_mid, default=t_def, cap2_radii=t_r2, coincident_mid=c_mid).items()}
    print("%d-wide, of %d points: %s; caps in effect: mid %d, default %d" % (width, n, listed, t_mid["stack_cap"], t_def["stack_cap"]))
    # the long list of device test (d): terrain_64's recipe tiled to LONG_LIST points at STACK_CAP=2
    index = K.tiled(t_pts, K.LONG_LIST)[1]
    assert K.LONG_LIST < 21000 and int(t2["listed"][index].sum()) > 1.2 * EXACT_LANES
    # a radius on a listed point: the lanes of radius_mix that stay valid and keep their winner are listed with their radius
    cls = np.arange(n) % 6
    assert int(t_r2["listed"][cls == 1].sum()) > 0.25 * int((cls == 1).sum()) and not t_r2["listed"][cls >= 4].any()
    # the intermediate cap: waves with listed and unlisted lanes
    assert t_mid["stack_cap"] == MID_CAP[width] and c_mid["stack_cap"] == MID_CAP[width], "the tree's stack_bound clips the cap"
    if width == 4:
        assert min(listed["mid"], n - listed["mid"]) >= n // 4, listed
    else:                                                     # see MID_CAP: the quarter on each side is coincident's
        assert min(listed["mid"], n - listed["mid"]) >= 8 and min(listed["coincident_mid"], n - listed["coincident_mid"]) >= n // 4, listed
    # the default caps, clipped to the tree's stack_bound: nothing is listed
    assert t_def["stack_cap"] <= DEFAULT_CAP[width] and listed["default"] == 0, listed


@pytest.mark.parametrize("width", [4, 8])
def test_far_tail_changes_what_is_culled(workdir, harness, width):
    """The far point of far_tail grows the pad 2^-16 x max |coordinate| of the whole batch, and with it the other points' walks:
    the visits with it exceed the control's by more than its own walk could account for - a walk visits a node at most once, a
    wide tree has fewer nodes than triangles, and a walk tests a triangle at most once.  The NaN point changes nothing."""
    mesh, near = K.far_tail_scene()
    n_tris = mesh[1].size // 3
    ft = K.far_tail(near, K.PAD_LANES)
    u = len(near)
    assert len(ft["far"]) > K.PAD_LANES and len(ft["far"]) == len(ft["control"])
    differ = np.nonzero(ft["index_far"] != ft["index_control"])[0]
    assert len(differ) == 1 and differ[0] > K.PAD_LANES and ft["index_far"][differ[0]] == u
    far_pt = ft["unique"][u]
    assert far_pt[1] < 0 and abs(far_pt[1]) == np.abs(ft["far"][np.isfinite(ft["far"]).all(1)]).max()
    nan_at = np.nonzero(ft["index_control"] == u + 1)[0]
    assert len(nan_at) == 1 and nan_at[0] > K.PAD_LANES and np.isnan(ft["unique"][u + 1, 0]) and np.abs(ft["unique"][u + 1, 1:]).min() > abs(far_pt[1])
    assert set(ft["index_control"]) == set(range(u)) | {u + 1}
    plain, with_nan, with_far = K.run_harness(harness(width), [K.case(mesh, near), K.case(mesh, ft["unique"][np.r_[0:u, u + 1]]),
                                                               K.case(mesh, ft["unique"])], workdir)
    print("%d-wide far_tail: node visits %d -> %d, triangle tests %d -> %d with the far point (%d triangles)" % (
        width, plain["node_visits"], with_far["node_visits"], plain["tri_tests"], with_far["tri_tests"], n_tris))
    assert with_far["mismatches"] == 0 and with_nan["mismatches"] == 0
    assert with_nan["node_visits"] == plain["node_visits"] and with_nan["tri_tests"] == plain["tri_tests"]
    assert with_far["node_visits"] - plain["node_visits"] > n_tris and with_far["tri_tests"] - plain["tri_tests"] > n_tris
    K.assert_same_bits({k: v[:u] for k, v in with_far["brute"].items()}, plain["brute"], "the answers do not depend on the pad")


def test_sanitized_harness_on_the_new_cases(workdir):
    """The capped lane walk on the 8-wide tree's two-word stack entries, the degenerate records and the extreme scales under the
    address and undefined-behaviour sanitizers (the 4-wide harness: tests/test_closest_host.py)."""
    exe = K.build_harness(workdir, sanitize=True, bvh8=True)
    cases = scale_cases()
    picked = [("degenerate", 2), ("degenerate", MID_CAP[8]), ("2^-70", 2), ("2^62", 3), ("stacked", DEFAULT_CAP[8])]
    results = K.run_harness(exe, [K.case(cases[name][0], cases[name][1][:256], stack_cap=cap) for name, cap in picked], workdir)
    assert all(r["mismatches"] == 0 for r in results)
    assert int(results[0]["listed"].sum()) > 0
    # the scale sweep: the exponent arithmetic of pow2_of at both ends of its clamp and in between
    sweep = []
    for name in SWEEP_MESHES:
        mesh, pts = K.sweep_mesh(name), K.sweep_points(name)[:256]
        best = K.true_distance(mesh, pts)
        sweep += [K.sweep_case(mesh, pts, best, e)[:2] for e in K.SWEEP_EXPONENTS]
    tiny = (np.ldexp(K.sweep_mesh("cube")[0], -140).astype(np.float32),) + K.sweep_mesh("cube")[1:]          # subnormal coordinates: k clamps at -126
    sweep.append((tiny, np.ldexp(K.sweep_points("cube")[:256], -140).astype(np.float32)))
    results = K.run_harness(exe, [K.case(mesh, pts, stack_cap=2) for mesh, pts in sweep], workdir)
    assert all(r["mismatches"] == 0 for r in results) and all(np.all(r["brute"]["group"] >= 0) for r in results[:-1])


# ---- float64 truth at every scale (closest_cases.SWEEP_EXPONENTS)

SWEEP_MESHES = K.SWEEP_CLOSED + ("height_field",)


@pytest.fixture(scope="module")
def sweep_truth():
    """name -> (mesh, points, float64 minimum distance), unscaled."""
    out = {}
    for name in SWEEP_MESHES:
        mesh, pts = K.sweep_mesh(name), K.sweep_points(name)
        out[name] = (mesh, pts, K.true_distance(mesh, pts))
    return out


def test_the_sweeps_filter_keeps_seven_eighths_of_every_batch(sweep_truth):
    for name, (mesh, pts, best) in sweep_truth.items():
        shares = {e: float(K.sweep_keep(best, e).mean()) for e in K.SWEEP_EXPONENTS}
        print(name, "kept:", ", ".join("2^%d %.4f" % (e, s) for e, s in shares.items()))
        assert min(shares.values()) >= 7.0 / 8.0 and shares[0] == 1.0, (name, shares)
        assert shares[58] < 1.0, name + ": no far point is dropped at 2^58"


@pytest.mark.parametrize("width", [4, 8])
def test_closest_points_against_float64_at_every_scale(workdir, harness, sweep_truth, width):
    """Conditions a and b of the sweep on the brute force, the walk's bits against it, and how many answers are not the exact
    2^e multiple of the 2^0 answer (reported)."""
    keys, cases = [], []
    for name, (mesh, pts, best) in sweep_truth.items():
        for e in K.SWEEP_EXPONENTS:
            big, big_pts, keep = K.sweep_case(mesh, pts, best, e)
            keys.append((name, e, keep))
            cases.append(K.case(big, big_pts, stack_cap=2))
    results = dict(((name, e), (keep, r)) for (name, e, keep), r in zip(keys, K.run_harness(harness(width), cases, workdir)))
    for (name, e), (keep, r) in results.items():
        mesh, pts, best = sweep_truth[name]
        what = "%d-wide %s x 2^%d" % (width, name, e)
        assert r["mismatches"] == 0, what
        K.assert_same_bits(r["walk"], r["brute"], what)
        excess, root = K.assert_sweep_answers(r["brute"], mesh, pts[keep], best[keep], e, LIMIT_UNITS, what)
        base = results[name, 0][1]["brute"]
        inexact = int((np.ldexp(base["dist2"][keep].astype(np.float64), 2 * e) != r["brute"]["dist2"]).sum() +
                      np.any(base["bw"][keep] != r["brute"]["bw"], axis=1).sum())
        print("%s: %d points, excess %.3f and sqrt(d2) %.3f units (limit %.3f), %d listed at cap 2, %d answers not 2^e x the 2^0 answer" % (
            what, int(keep.sum()), excess, root, LIMIT_UNITS, int(r["listed"].sum()), inexact))
