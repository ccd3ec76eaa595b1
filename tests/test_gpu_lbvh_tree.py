"""The GPU LBVH builder's own output (par_raytracer_amd/csrc/bvh_lbvh.h: k_prims, the device radix sort, k_hierarchy, k_fit), read
back through prt_debug_lbvh_tree and held against the numpy reference of tests/lbvh_cases.py element by element, with == : sorted
keys, order, links, ranges and every box, upper nodes included - which the default back end never reads.  Then the trees in use: the
host back end's four settings on every case (the geometric check), and rays and closest points on uploads of those four settings
against the SAH upload, bit for bit.  tests/test_lbvh_cases_host.py proves the cases and the reference without a GPU.

Measured on an MI355X (52 tests, 6.1 s alone of which 0.3 s is the process's first GPU use): the 8-wide child 1.9 s; queries on
`large` 0.56 s, on the other cases 0.18 - 0.22 s each; back ends on `large` 0.32 s, on the others <= 0.06 s; the tree of `large`
0.13 s (5.9 ms in the library), three builds of it 0.02 s; every other tree comparison <= 0.01 s.

What each device-side revert of bvh_lbvh.h turns red (each built apart and run once; none can change a link):
  clamp at 2097152.0f in k_prims       the tree of tiny_extent only - the one case whose scale is inf; on every other case
                                       (c - lo) * s stays below 2097151.25, so that clamp end decides nothing
  hi for lo in k_prims' centre         the tree of every case but flat_3, and the three builds
  fmaxf for fminf in k_fit's merge     the tree of every case whose boxes are not all one box (not counts_1, identical, flat_3), the
                                       three builds, the back ends of those cases from 5 triangles on, all nine query cases
  sorted_ids from the unsorted buffer  the tree of every case whose order is not the identity (not counts_1, counts_3, same_centre,
                                       identical, flat_3), the three builds, those cases' back ends from 5 triangles on and queries
The device's keys equal the float32 restatement on every case, far_and_thin and tiny_extent included: k_prims' centre needs no
pinning against contraction."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from conftest import ROOT

import lbvh_cases as L

CLOSEST = ("t", "bw", "vertex0", "group", "position", "normal")
POINT_FIELDS = ("dist2", "point", "bw", "vertex0", "group")
SETTINGS = (("default", {}), ("plain", {"LBVH_PLAIN": "1"}), ("cluster4", {"LBVH_CLUSTER": "4"}), ("cluster1048576", {"LBVH_CLUSTER": "1048576"}))


@pytest.fixture(scope="module")
def renderer():
    from par_raytracer_amd import api
    r = api.Renderer(0)
    yield r
    r.close()


def explain(got, ref):
    """The first differing element of every array that differs."""
    out = []
    for k in L.differences(got, ref):
        a, b = np.asarray(got[k]), np.asarray(ref[k])
        if a.shape != b.shape or a.dtype != b.dtype:
            out.append("%s: %s %s, expected %s %s" % (k, a.dtype, a.shape, b.dtype, b.shape))
            continue
        rows = np.nonzero((a != b).reshape(len(a), -1).any(1))[0]
        out.append("%s: %d of %d differ, first at %d: got %r, expected %r" % (k, rows.size, len(a), rows[0], a[rows[0]], b[rows[0]]))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", L.case_names())
def test_device_tree_equals_the_reference(renderer, name):
    ref = L.case_reference(name)
    v = L.verts9(L.case(name))
    t0 = time.perf_counter()
    got = renderer.lbvh_tree(v)
    print("%s: %d triangles, prt_debug_lbvh_tree %.1f ms" % (name, len(v), 1e3 * (time.perf_counter() - t0)))
    assert set(got) == set(L.TREE_ARRAYS)
    assert explain(got, ref) == []
    without = renderer.lbvh_tree(v, keys=False)                    # the keys are optional; the rest does not depend on asking for them
    assert "sorted_keys" not in without and explain(without, ref) == []


@pytest.mark.gpu
def test_three_builds_of_the_large_case_are_identical(renderer):
    """k_fit's cross-lane reads: every block of the second and third build meets memory the builds before it left behind."""
    big, small = L.verts9(L.case("large")), L.verts9(L.case("counts_257"))
    builds = []
    for k in range(3):
        builds.append(renderer.lbvh_tree(big))
        assert explain(renderer.lbvh_tree(small), L.case_reference("counts_257")) == []
    bits = lambda a: a.view(np.uint32) if a.dtype == np.float32 else a                                  # noqa: E731
    for b in builds:
        assert set(b) == set(L.TREE_ARRAYS) and len(b["node_box"]) == len(big) - 1
    for b in builds[1:]:
        for k in L.TREE_ARRAYS:
            assert np.array_equal(bits(b[k]), bits(builds[0][k])), k
    assert explain(builds[2], L.case_reference("large")) == []


def set_backend(r, options):
    r.set_option("BVH_BUILDER", "lbvh")
    for k in ("LBVH_PLAIN", "LBVH_CLUSTER"):
        r.set_option(k, options.get(k))


def check_backends(r, name):
    """prt_debug_check_bvh_lbvh on the case under the four back-end settings; returns the checks' outputs."""
    import query_grad_cases as Q
    from par_raytracer_amd import capi
    lib = capi.hip_lib()
    mesh = L.case(name)
    desc = Q.flat_desc(mesh)
    n = mesh[1].size // 3
    found = {}
    for setting, options in SETTINGS:
        set_backend(r, options)
        out = (C.c_uint64 * 6)()
        assert lib.prt_debug_check_bvh_lbvh(r._ctx, desc.desc, out) == 0, (name, setting, lib.prt_last_error(r._ctx))
        assert out[0] == 0, "%s %s: %d violations" % (name, setting, out[0])
        assert out[5] == n, "%s %s: %d of %d triangles referenced" % (name, setting, out[5], n)
        found[setting] = tuple(int(x) for x in out)
    return found


@pytest.mark.gpu
@pytest.mark.parametrize("name", L.case_names())
def test_every_back_end_makes_a_conservative_and_complete_tree(name):
    from par_raytracer_amd import api
    r = api.Renderer(0)
    try:
        found = check_backends(r, name)
        n = L.case(name)[1].size // 3
        if n > 64:                                             # the settings are in effect: they give different trees
            assert found["plain"][1] != found["default"][1] or found["cluster4"][1] != found["default"][1], found
    finally:
        r.close()


def upload(name, options):
    """A context with the case uploaded: options None = the SAH builder, else the LBVH builder with that back end."""
    import query_grad_cases as Q
    from par_raytracer_amd import api
    r = api.Renderer(0)
    try:
        if options is not None:
            set_backend(r, options)
        info = r.upload(Q.flat_desc(L.case(name)))
        assert info.triangle_count == L.case(name)[1].size // 3
    except Exception:
        r.close()
        raise
    return r


def all_queries(r, o, d, tmax, pts):
    """Every field of closest hits, occlusion without and with a limit, and closest points, as bit patterns."""
    res = r.trace_rays(o, d)
    out = {k: np.ascontiguousarray(res[k]).view(np.uint32).copy() for k in CLOSEST}
    out["occluded"] = r.trace_rays(o, d, mode="occluded")["occluded"].copy()
    out["occluded_tmax"] = r.trace_rays(o, d, mode="occluded", tmax=tmax)["occluded"].copy()
    cp = r.closest_points(pts)
    for k in POINT_FIELDS:
        out["cp_" + k] = np.ascontiguousarray(cp[k]).view(np.uint32).copy()
    return out


def compare_queries(name, keys=None):
    """The case's rays and points on the four LBVH uploads against the SAH upload; `keys`: compare only these.  Returns (hits, rays, the
    SAH upload's results)."""
    o, d, pts = L.queries(name)
    rng = np.random.default_rng(71)
    sah = upload(name, None)
    try:
        t = sah.trace_rays(o, d, fields=("t",))["t"]
        # a limit on either side of each ray's own hit (a miss keeps FLT_MAX): both answers of OCCLUDED below tmax occur
        with np.errstate(over="ignore"):
            tmax = np.minimum(t * rng.uniform(0.5, 1.5, len(t)).astype(np.float32), np.float32(3.0e38)).astype(np.float32)
        exp = all_queries(sah, o, d, tmax, pts)
    finally:
        sah.close()
    for setting, options in SETTINGS:
        r = upload(name, options)
        try:
            got = all_queries(r, o, d, tmax, pts)
        finally:
            r.close()
        for k in (keys or exp):
            bad = np.nonzero(np.any((got[k] != exp[k]).reshape(len(exp[k]), -1), axis=1))[0]
            assert bad.size == 0, "%s, LBVH %s: %s differs from the SAH upload on %d of %d, first %d: %r / %r" % (
                name, setting, k, bad.size, len(exp[k]), bad[0], got[k][bad[0]], exp[k][bad[0]])
    hits = int((exp["group"].view(np.int32) >= 0).sum())
    assert np.all(exp["cp_group"].view(np.int32) >= 0)
    return hits, len(o), exp


@pytest.mark.gpu
@pytest.mark.parametrize("name", L.QUERY_CASES)
def test_queries_on_every_back_end_equal_the_sah_upload(name):
    t0 = time.perf_counter()
    hits, rays, exp = compare_queries(name)
    print("%s: %d of %d rays hit, %d occluded, %d below tmax; %.2f s" % (name, hits, rays, int(exp["occluded"].sum()), int(exp["occluded_tmax"].sum()),
                                                                          time.perf_counter() - t0))
    assert rays == 4096 and len(exp["cp_group"]) == 2048
    assert hits >= 0.9 * rays                                     # the equality is not between misses
    assert 0 < exp["occluded_tmax"].sum() < exp["occluded"].sum()


@pytest.mark.gpu
def test_queries_on_identical_copies():
    """37 copies of one triangle: which copy wins is not the subject here - the distances and the occlusion are."""
    hits, rays, exp = compare_queries("identical", keys=("t", "occluded", "occluded_tmax", "cp_dist2"))
    assert hits >= 0.9 * rays


CHILD = r"""
import os, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, "tests")); sys.path.insert(0, os.path.join(%(root)r, "oracle"))
import numpy as np
import lbvh_cases as L
from test_gpu_lbvh_tree import check_backends, compare_queries, explain
from par_raytracer_amd import api, capi
lib = capi.hip_lib()
assert os.path.basename(lib._name) == "libprt_hip_bvh8.so" and not (lib.prt_build_flags() & capi.BUILD_BVH4)
for name in ("same_centre_1000", "same_centre_1024", "runs", "counts_257"):
    r = api.Renderer(0)
    assert explain(r.lbvh_tree(L.verts9(L.case(name))), L.case_reference(name)) == []
    check_backends(r, name)
    r.close()
    hits, rays, _ = compare_queries(name)
    assert hits >= 0.9 * rays
    print(name, hits, "of", rays, "rays hit", flush=True)
print("bvh8 lbvh ok")
"""


@pytest.mark.gpu
def test_on_the_8_wide_library():
    if not os.path.exists(os.path.join(ROOT, "par_raytracer_amd", "libprt_hip_bvh8.so")):
        pytest.skip("libprt_hip_bvh8.so not built (make hip-bvh8)")
    env = dict(os.environ)
    env["PRT_HIP_LIB"] = "libprt_hip_bvh8.so"
    out = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0 and b"bvh8 lbvh ok" in out.stdout, (out.returncode, out.stdout.decode()[-1500:], out.stderr.decode()[-3000:])
