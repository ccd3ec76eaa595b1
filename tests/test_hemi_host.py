"""The definition of prt_hemisphere_visibility on the host (tests/hemi_host_harness.cpp: the functions of csrc/dev_hemi.h and
csrc/hammersley.h, built here with g++): the device traversal compiled for the host against a brute force over every triangle, ray
by ray, on the 4-wide and on the 8-wide tree; hemi_index against a plain restatement of the key, the seed and the first draw; the
table's bytes against the formula as it stood before it moved; the counts, sums and outputs against the rays' flags; the input mix
the GPU tests rely on; invalid points, max_dist at its edges, far points and the scene of no triangles."""
from __future__ import annotations

import numpy as np
import pytest

import closest_cases as K
import hemi_cases as H
import signed_cases as S

SCENES = ("torus", "cube", "cornell_box")
N_POINTS, SAMPLES = 257, 100


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("hemi_host")


@pytest.fixture(scope="module")
def exes(workdir):
    return {4: H.build_harness(workdir), 8: H.build_harness(workdir, bvh8=True)}


def scene_case(name, **kw):
    mesh = S.mesh_of(name)
    pts, nrm = H.mixed_points(mesh, N_POINTS, S.SEEDS.get(name, 77))
    return H.case(mesh, pts, nrm, SAMPLES, seed=11, first=5, **kw)


@pytest.fixture(scope="module")
def results(exes, workdir):
    """width -> scene -> the harness's result; computed once."""
    cases = [scene_case(name) for name in SCENES]
    return {w: dict(zip(SCENES, H.run_harness(exe, cases, workdir, tag="scenes%d" % w))) for w, exe in exes.items()}


@pytest.mark.parametrize("width", [4, 8])
@pytest.mark.parametrize("name", SCENES)
def test_walk_equals_brute_force_ray_by_ray(results, name, width):
    res = results[width][name]
    assert res["brute"].shape == (N_POINTS, SAMPLES)
    diff = np.argwhere(res["brute"] != res["walk"])
    assert len(diff) == 0, (name, width, len(diff), diff[:5].tolist())
    assert res["cast"] == N_POINTS * SAMPLES


@pytest.mark.parametrize("name", SCENES)
def test_trees_agree_and_inputs_are_mixed(results, name):
    """Both widths give the same bits, and the scene's points see the whole range: at least three distinct counts, one of them
    strictly between 0 and samples.  The torus's inner ring and the box's furniture give the partial ones; the test is
    single-sided, so a point inside the outward-wound cube sees back faces only and stays unoccluded."""
    a, b = results[4][name], results[8][name]
    for f in H.FIELDS + ("sums", "k", "dirs", "brute"):
        assert np.array_equal(np.ascontiguousarray(a[f]).view(np.uint8), np.ascontiguousarray(b[f]).view(np.uint8)), (name, f)
    H.assert_input_mix(a, SAMPLES, name)


def test_points_inside_the_cube_are_unoccluded(exes, workdir):
    mesh = S.cube()
    rng = np.random.default_rng(3)
    pts = rng.uniform(0.1, 0.9, (64, 3)).astype(np.float32)
    nrm = np.tile(np.array([[0, 0, 1]], np.float32), (64, 1))
    res = H.run_harness(exes[4], [H.case(mesh, pts, nrm, 64, seed=2)], workdir, tag="inside")[0]
    assert (res["unoccluded"] == 64).all()
    assert (res["visibility"] == 1.0).all()


def test_hemi_index_against_a_plain_restatement(results):
    """k of every ray of the torus case against prt_sample_key, Random_Seed and the first Random_Next in Python integers, at
    first = 5; and the key's own corner cases through a one-point case each."""
    res = results[4]["torus"]
    for i in (0, 1, 100, N_POINTS - 1):
        expect = [H.hemi_index(11, 5 + i, s) for s in range(SAMPLES)]
        assert res["k"][i].tolist() == expect, i
    assert len(np.unique(res["k"])) > 900, "the draws cover the table"


def test_hemi_index_at_the_key_edges(exes, workdir):
    mesh = S.cube()
    pts, nrm = np.array([[0.5, 0.5, 2.0]], np.float32), np.array([[0, 0, 1]], np.float32)
    firsts = (0, 65535, 65536, 2 ** 32 - 1)
    seeds = (0, 1, 2 ** 64 - 1)
    cases = [H.case(mesh, pts, nrm, 65535 if j == 0 else 3, seed=seed, first=j) for j in firsts for seed in seeds]
    res = H.run_harness(exes[4], cases, workdir, tag="keys")
    for c, r in zip(cases, res):
        s = np.array([0, 1, c["samples"] - 1])
        assert r["k"][0, s].tolist() == [H.hemi_index(c["seed"], c["first"], int(x)) for x in s], (c["seed"], c["first"])


def test_table_keeps_its_bytes(exes, workdir):
    """csrc/hammersley.h gives, with the host's libm, the bytes of the formula as csrc/prt_api.hip held it."""
    got, expect = H.harness_table(exes[4], workdir), H.table_before_the_move()
    assert got.dtype == expect.dtype and got.shape == expect.shape == (1024, 4)
    assert np.array_equal(got.view(np.uint32), expect.view(np.uint32)), np.argwhere(got.view(np.uint32) != expect.view(np.uint32))[:5]
    ln = np.linalg.norm(got[:, :3].astype(np.float64), axis=1)
    assert np.abs(ln - 1.0).max() < 1e-6 and (got[:, 2] > 0).all() and (got[:, 3] == 0).all()


@pytest.mark.parametrize("name", SCENES)
def test_outputs_follow_from_the_flags(results, name):
    """unoccluded, the sums, visibility and bent restated in numpy from the harness's rays and flags."""
    res = results[4][name]
    free = res["brute"].astype(bool)
    assert np.array_equal(res["unoccluded"], free.sum(1).astype(np.uint32))
    fix = np.rint(res["dirs"].astype(np.float64) * 2.0 ** 32).astype(np.int64)
    sums = (fix * free[:, :, None]).sum(1)
    assert np.array_equal(res["sums"], sums)
    vis = (res["unoccluded"].astype(np.float32) / np.float32(SAMPLES)).astype(np.float32)
    assert np.array_equal(res["visibility"].view(np.uint32), vis.view(np.uint32))
    bent = ((sums.astype(np.float64) * 2.0 ** -32) / float(SAMPLES)).astype(np.float32)
    assert np.array_equal(res["bent"].view(np.uint32), bent.view(np.uint32))
    # directions are unit length and lie in the normal's hemisphere (up to rounding)
    ln = np.linalg.norm(res["dirs"].astype(np.float64), axis=2)
    assert np.abs(ln - 1.0).max() < 1e-6
    mesh = S.mesh_of(name)
    _pts, nrm = H.mixed_points(mesh, N_POINTS, S.SEEDS.get(name, 77))
    assert ((res["dirs"].astype(np.float64) * nrm[:, None, :]).sum(2) > -1e-6).all()


def test_edges(exes, workdir):
    """Invalid points, max_dist at its edges, a far point and the scene of no triangles - on both trees."""
    mesh = S.torus()
    pts, nrm = H.surface_points(mesh, 16, 9)
    pts, nrm = np.tile(pts, (2, 1)), np.tile(nrm, (2, 1))              # 32 points: the second half gets the edge values
    md = np.full(32, np.inf, np.float32)
    bad = dict(p_nan=16, p_inf=17, n_nan=18, n_inf=19, n_zero=20)
    pts[16, 1], pts[17, 0] = np.nan, np.inf
    nrm[18, 2], nrm[19, 0] = np.nan, -np.inf
    nrm[20] = 0
    md[21], md[22], md[23], md[24] = 0.0, -1.0, np.nan, np.inf
    md[:16] = 0.3                                                        # a reach inside the torus's extent
    extent = K.mesh_extent(mesh)[2]
    pts[25] = np.array([100.0 * extent, 0.0, 0.0], np.float32)           # query_far: looks back at the torus
    nrm[25] = np.array([-1.0, 0.0, 0.0], np.float32)
    empty = (mesh[0], np.zeros(0, np.uint32), np.zeros((1, 2), np.uint32))
    for w, exe in exes.items():
        full, lim, none = H.run_harness(exe, [H.case(mesh, pts, nrm, 64, seed=4), H.case(mesh, pts, nrm, 64, seed=4, max_dist=md),
                                              H.case(empty, pts, nrm, 64, seed=4)], workdir, tag="edges%d" % w)
        for res in (full, lim, none):
            assert np.array_equal(res["brute"], res["walk"]), w
            for i in bad.values():
                assert res["unoccluded"][i] == H.INVALID and res["visibility"][i] == 0 and not res["bent"][i].any()
                assert not res["brute"][i].any()
            assert res["cast"] == (32 - len(bad)) * 64
        for i in (21, 22, 23):
            assert lim["unoccluded"][i] == 64, "nothing occludes below a max_dist of 0, -1 or NaN"
        assert lim["unoccluded"][24] == full["unoccluded"][24]
        assert (lim["unoccluded"][:16] >= full["unoccluded"][:16]).all() and (lim["unoccluded"][:16] > full["unoccluded"][:16]).any()
        assert full["unoccluded"][25] <= 64                              # (routed through query_any_unculled: walk == brute above)
        valid = np.setdiff1d(np.arange(32), list(bad.values()))
        assert (none["unoccluded"][valid] == 64).all() and (none["visibility"][valid] == 1.0).all()
