"""The cases and the reference of tests/lbvh_cases.py, proven without a GPU: every case has the property it is named for; the
top-down reference tree equals a lane-by-lane port of k_hierarchy (par_raytracer_amd/csrc/bvh_lbvh.h); the comparison the GPU test
makes fails under four edits of a right tree; and the host back end (bvh_build.cpp build_bvh_wide_from_radix_tree), built with
g++ under the address and undefined-behaviour sanitizers as a program of its own, turns every reference tree into a valid wide tree
of both widths under the settings plain, cluster 4, cluster 64 and cluster 2^20.

Distinct keys / longest run of equal keys, as the reference computes them: same_centre_1000 1 / 1,000; same_centre_1024 1 / 1,024;
runs 7 / 300; identical 1 / 37; flat_3 1 / 300; every other case (counts_*, flat_1, flat_2, tiny_extent, far_and_thin 1,024, large
131,073) one key per triangle.  The four edits: a delta without the position tie-break changes first and last on same_centre_1000,
runs and identical (and nothing where all keys differ); swapped children show in left and right, a shifted `last` in last, a
box one ulp short in node_box - each in no other array.  209 tests, 14 s, nearly all of it the sanitized
harness's build and run."""
from __future__ import annotations

import re

import numpy as np
import pytest

import harness
import lbvh_cases as L

SMALL = [n for n in L.case_names() if n != "large"]


def runs_of_equal_keys(sorted_keys):
    edges = np.nonzero(np.diff(sorted_keys) != 0)[0] + 1
    return np.diff(np.concatenate([[0], edges, [len(sorted_keys)]]))


# ---- the cases are what they are named for

@pytest.mark.parametrize("n", L.COUNTS)
def test_counts_fall_on_the_stated_side_of_a_block(n):
    """k_prims and k_fit launch (n + 255) / 256 blocks, k_hierarchy (n - 1 + 255) / 256: the counts put the last lane of a block on
    either side of the arrays' ends, and below one wave there is 1 (no hierarchy at all), 2 (one node), 3, 4, 5."""
    mesh = L.case("counts_%d" % n)
    assert mesh[1].size == 3 * n
    side = {1: (1, 0), 2: (2, 1), 3: (3, 2), 4: (4, 3), 5: (5, 4),
            255: (255, 254),                     # both kernels: one block, its last lane idle
            256: (0, 255),                       # the triangles fill a block exactly; the nodes end one lane short
            257: (1, 0),                         # one triangle in a second block; the nodes fill one block exactly
            258: (2, 1),                         # one node in a second block
            513: (1, 0)}[n]                      # three blocks of triangles, two full blocks of nodes
    assert (n % 256, (n - 1) % 256) == side
    r = L.case_reference("counts_%d" % n)
    assert len(np.unique(r["sorted_keys"])) == n, "a random soup has distinct keys"


@pytest.mark.parametrize("name", ["same_centre_1000", "same_centre_1024"])
def test_same_centre_has_one_key_and_no_coplanar_pair(name):
    p, idx, _ = L.case(name)
    n = idx.size // 3
    assert n == int(name.split("_")[2])
    units = np.rint(p.astype(np.float64) / L.GRID)
    assert np.array_equal(units * L.GRID, p.astype(np.float64)) and np.abs(units).max() < 64 * 1024          # on the 2^-10 grid below 64
    u = units.astype(np.int64).reshape(n, 3, 3)
    assert np.all(u.min(1) + u.max(1) == 2 * np.array([24 * 1024, 17 * 1024 + 512, 40 * 1024 + 256]))
    r = L.case_reference(name)
    assert len(np.unique(r["sorted_keys"])) == L.DISTINCT_KEYS[name] == 1
    assert np.array_equal(r["sorted_ids"], np.arange(n))                                 # a stable sort leaves equal keys alone
    # exact integer test: two triangles are coplanar when their normals are parallel and one's corner lies in the other's plane
    nrm = np.cross(u[:, 1] - u[:, 0], u[:, 2] - u[:, 0])
    assert np.abs(nrm).max() < 2 ** 26 and np.all(np.any(nrm != 0, axis=1))
    parallel = np.all(np.cross(nrm[:, None, :], nrm[None, :, :]) == 0, axis=2)
    in_plane = np.einsum("ik,ijk->ij", nrm, u[None, :, 0, :] - u[:, None, 0, :]) == 0
    assert int((parallel & in_plane).sum()) == n                                          # only each triangle with itself


def test_runs_have_the_stated_lengths_and_reach_both_ends_of_the_grid():
    mesh, run = L.runs_case()
    r = L.case_reference("runs")
    assert len(run) == sum(L.RUN_LENGTHS) == 624
    assert len(np.unique(r["sorted_keys"])) == L.DISTINCT_KEYS["runs"] == 7
    assert sorted(runs_of_equal_keys(r["sorted_keys"])) == sorted(L.RUN_LENGTHS)
    assert np.all(r["sorted_keys"][1:] >= r["sorted_keys"][:-1])
    by_run = run[r["sorted_ids"]]
    for k in range(7):
        at = np.nonzero(by_run == k)[0]
        assert at[-1] - at[0] + 1 == L.RUN_LENGTHS[k]                                     # a run of the construction is a run of the keys
        assert np.all(np.diff(r["sorted_ids"][at].astype(np.int64)) > 0)                  # ... in input order
    assert np.all(r["q"][by_run == 0] == 0) and r["sorted_keys"][0] == 0
    assert np.all(r["q"][by_run == 1] == L.QMAX) and r["sorted_keys"][-1] == 2 ** 63 - 1
    assert by_run[0] == 0 and np.all(by_run[-2:] == 1)


def test_identical_is_one_triangle_37_times():
    p, idx, _ = L.case("identical")
    assert idx.size == 3 * 37 and np.all(p.reshape(37, 9) == np.asarray(L.ONE, np.float32))
    r = L.case_reference("identical")
    assert len(np.unique(r["sorted_keys"])) == L.DISTINCT_KEYS["identical"] == 1 and np.array_equal(r["sorted_ids"], np.arange(37))


@pytest.mark.parametrize("axes", [1, 2, 3])
def test_flat_scenes_have_extent_zero_and_scale_zero(axes):
    mesh = L.case("flat_%d" % axes)
    p = mesh[0]
    assert mesh[1].size == 900
    ext = p.max(0) - p.min(0)
    assert int((ext == 0).sum()) == axes
    keys, q, _, scale = L.reference_keys(L.verts9(mesh))
    assert np.all(scale[ext == 0] == 0) and np.all(scale[ext > 0] > 0)
    assert np.all(q[:, ext == 0] == 0)
    if axes == 3:
        assert len(np.unique(keys)) == L.DISTINCT_KEYS["flat_3"] == 1
    else:
        assert len(np.unique(keys)) > 250


def test_tiny_extent_has_an_infinite_scale_and_both_ends_of_the_clamp():
    mesh = L.case("tiny_extent")
    p = mesh[0]
    assert mesh[1].size == 900 and p[:, 2].min() == 0 and p[:, 2].max() == np.float32(L.TINY) > np.finfo(np.float32).tiny
    keys, q, boxes, scale = L.reference_keys(L.verts9(mesh))
    assert np.isinf(scale[2]) and np.all(np.isfinite(scale[:2]))
    at_zero = boxes[:, 5] == 0                               # all three corners at z = 0: 0 * inf, a NaN that becomes 0
    assert 30 <= at_zero.sum() < 60
    assert np.all(q[at_zero, 2] == 0) and np.all(q[~at_zero, 2] == L.QMAX)
    assert len(np.unique(keys)) == 300


def test_far_and_thin_merges_centres_that_exact_arithmetic_tells_apart():
    mesh = L.case("far_and_thin")
    p, idx, _ = mesh
    n = idx.size // 3
    assert n == 1024 and p.min() == L.FAR and np.float32(p[:, 2].max() - p[:, 2].min()) == np.float32(L.STEP)
    assert np.array_equal(np.unique(p[:, 2]), np.array([L.FAR, L.FAR + L.STEP], np.float32))
    v = p.reshape(n, 3, 3).astype(np.float64)
    exact = 0.5 * (v.min(1) + v.max(1))
    keys, q, boxes, _ = L.reference_keys(L.verts9(mesh))
    centre32 = np.float32(0.5) * (boxes[:, :3] + boxes[:, 3:])
    straddle = v[:, :, 2].min(1) != v[:, :, 2].max(1)
    assert 0.5 * n < straddle.sum() < n
    assert len(np.unique(exact[:, 2])) == 3 and len(np.unique(centre32[:, 2])) == 2
    assert np.all(centre32[straddle, 2] == np.float32(L.FAR))                             # round to even: down into the lower plane
    assert np.array_equal(np.unique(q[:, 2]), [0, L.QMAX])
    assert len(np.unique(keys)) == L.DISTINCT_KEYS["far_and_thin"] == 1024       # x and y tell every cell apart


# ---- the reference against the second construction

@pytest.mark.parametrize("name", SMALL)
def test_reference_tree_equals_the_port_of_k_hierarchy(name):
    r = L.case_reference(name)
    n = len(r["sorted_ids"])
    assert np.all(r["sorted_keys"][1:] >= r["sorted_keys"][:-1])
    port = dict(zip(("left", "right", "first", "last"), L.port_hierarchy(r["sorted_keys"])))
    if n > 1:
        for k, v in port.items():
            assert np.array_equal(v, r[k]) and v.dtype == r[k].dtype, (name, k)
        # and it is a tree: every node but the root and every leaf is the child of exactly one node
        kids = np.concatenate([r["left"], r["right"]])
        assert sorted(kids[kids >= 0]) == list(range(1, n - 1)) and sorted(~kids[kids < 0]) == list(range(n))
    assert L.differences(port, r) == []


def test_reference_tree_of_the_large_case_on_4096_nodes_and_their_ancestors():
    r = L.case_reference("large")
    n = len(r["sorted_ids"])
    assert n == L.LARGE_N == 2 ** 17 + 1
    up = L.parents(r["left"], r["right"])
    assert up[0] == -1 and np.all(up[1:] >= 0)
    rng = np.random.default_rng(5)
    lanes = set()
    for node in rng.choice(n - 1, 4096, replace=False):
        while node >= 0 and node not in lanes:
            lanes.add(int(node))
            node = up[node]
    assert 0 in lanes
    lanes = np.array(sorted(lanes))
    port = dict(zip(("left", "right", "first", "last"), L.port_hierarchy(r["sorted_keys"], lanes)))
    assert L.differences(port, r, nodes=lanes) == []
    # the boxes: a node's box is the union of its children's (the reference took it from the leaves of [first, last])
    child = lambda c: np.where((c < 0)[:, None], r["leaf_box"][np.where(c < 0, ~c, 0)], r["node_box"][np.where(c < 0, 0, c)])     # noqa: E731
    lb, rb = child(r["left"]), child(r["right"])
    assert np.array_equal(r["node_box"][:, :3], np.minimum(lb[:, :3], rb[:, :3])) and np.array_equal(r["node_box"][:, 3:], np.maximum(lb[:, 3:], rb[:, 3:]))


# ---- the comparison sees a wrong tree

def _copy(r):
    return {k: np.array(r[k]) for k in L.TREE_ARRAYS}


@pytest.mark.parametrize("name", ["same_centre_1000", "runs", "identical"])
def test_a_delta_without_the_position_tie_break_is_seen(name):
    r = L.case_reference(name)
    got = _copy(r)
    got["left"], got["right"], got["first"], got["last"] = L.port_hierarchy(r["sorted_keys"], tie_break=False)
    assert set(L.differences(got, r)) >= {"first", "last"}


def test_a_delta_without_the_tie_break_is_right_where_no_keys_are_equal():
    r = L.case_reference("counts_513")
    got = _copy(r)
    got["left"], got["right"], got["first"], got["last"] = L.port_hierarchy(r["sorted_keys"], tie_break=False)
    assert L.differences(got, r) == []


@pytest.mark.parametrize("name", ["counts_2", "counts_257", "same_centre_1024", "runs"])
def test_swapped_children_a_shifted_range_and_a_box_one_ulp_short_are_seen(name):
    r = L.case_reference(name)
    assert L.differences(_copy(r), r) == []
    n = len(r["sorted_ids"])
    node = 0 if n == 2 else (n - 1) // 3
    got = _copy(r)
    got["left"][node], got["right"][node] = r["right"][node], r["left"][node]
    assert L.differences(got, r) == ["left", "right"]
    got = _copy(r)
    got["last"][node] += 1
    assert L.differences(got, r) == ["last"]
    # an upper node: the root's larger child, or the root - a box the default back end never reads
    upper = 0 if n == 2 else int(max((c for c in (r["left"][0], r["right"][0]) if c >= 0), key=lambda c: r["last"][c] - r["first"][c]))
    for column in (0, 4):                                    # lo x one ulp up, hi y one ulp down: the box no longer holds its triangles
        got = _copy(r)
        x = got["node_box"][upper, column]
        got["node_box"][upper, column] = np.nextafter(x, np.float32(np.inf if column < 3 else -np.inf), dtype=np.float32)
        assert got["node_box"][upper, column] != x
        assert L.differences(got, r) == ["node_box"]


def test_one_triangle_leaves_the_node_arrays_out():
    r = L.case_reference("counts_1")
    got = _copy(r)
    for k in ("left", "right", "first", "last"):
        got[k][:] = 12345
    got["node_box"][:] = 7.5
    assert L.differences(got, r) == []
    got["leaf_box"][0, 0] += 1
    assert L.differences(got, r) == ["leaf_box"]


def test_a_zero_of_either_sign_is_the_same_box():
    r = L.case_reference("counts_3")
    got = _copy(r)
    got["leaf_box"][0, 0] = 0.0
    ref = dict(r)
    ref["leaf_box"] = np.array(r["leaf_box"])
    ref["leaf_box"][0, 0] = -0.0
    assert L.differences(got, ref) == []


# ---- the host back end on the reference's trees

LINE = re.compile(r"(\w+) width (\d) (\w+) \| n_tris (\d+) violations (\d+) nodes (\d+) depth (\d+) stack_bound (\d+) leaves (\d+) refs (\d+) "
                  r"\| validate: (.*)")


@pytest.fixture(scope="module")
def backend(tmp_path_factory):
    d = tmp_path_factory.mktemp("lbvh_backend")
    exe = L.build_backend_harness(d, sanitize=True)
    path = str(d / "trees.bin")
    L.write_trees(path, L.case_names())
    out = harness.run(exe, path)
    found = {}
    for line in out.splitlines():
        m = LINE.fullmatch(line)
        assert m, line
        found[(m.group(1), int(m.group(2)), m.group(3))] = dict(n_tris=int(m.group(4)), violations=int(m.group(5)), refs=int(m.group(10)),
                                                               validate=m.group(11))
    return found


@pytest.mark.parametrize("setting", [b[0] for b in L.BACKENDS])
@pytest.mark.parametrize("width", [4, 8])
@pytest.mark.parametrize("name", L.case_names())
def test_the_host_back_end_makes_a_valid_tree_of_every_reference_tree(backend, name, width, setting):
    t = backend[(name, width, setting)]
    n = L.case(name)[1].size // 3
    assert t["validate"] == "null"
    assert t["violations"] == 0
    assert t["n_tris"] == n and t["refs"] == n
