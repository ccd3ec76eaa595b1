"""prt_hemisphere_visibility on the GPU against tests/hemi_host_harness.cpp (the definition with the functions of csrc/dev_hemi.h
and csrc/hammersley.h, every ray answered by a brute force over all triangles, built here with g++): unoccluded, visibility and
bent bit for bit, through the host entry point (numpy) and the device entry point (torch); point counts around the wave and the
block, sample counts on both sides of the reduce kernel's threshold, past one pass of an 8-compute-unit grid; every subset of the
fields; the composition with trace_rays(mode="occluded") ray by ray; purity in the split of a batch, in HEMI_PASS_ITEMS, in
STACK_CAP, in the builder, in the tree's width and after update_geometry; the edges and the refusals.

The inputs are mixed by construction and checked to be (hemi_cases.assert_input_mix): each scene's expected counts take at least
three values and some point is partly occluded.  The OCCLUDED rule is single-sided, so the torus's inner ring and the box's
furniture give the partial counts, while points inside the outward-wound cube see back faces only and stay unoccluded."""
from __future__ import annotations

import ctypes as C
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import closest_cases as K
import hemi_cases as H
import signed_cases as S
from conftest import ROOT

SCENES = ("torus", "cube", "cornell_box")
COUNTS = (1, 63, 64, 65, 257)
SAMPLES = (1, 7, 64, 100)                  # csrc/kernels_hemi.h: a lane reduces a point below HEMI_WAVE_SAMPLES = 64, a wave from it on
SEED, FIRST = 11, 5


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("hemi_gpu")


@pytest.fixture(scope="module")
def harness(workdir):
    exe = H.build_harness(workdir)

    def run(cases):
        return H.run_harness(exe, cases, workdir)
    return run


def scene_points(name, n=257):
    mesh = S.mesh_of(name)
    return (mesh,) + H.mixed_points(mesh, n, S.SEEDS.get(name, 77))


def query(r, c, fields=None, torch_path=False, count_visits=False, rows=slice(None), first=None):
    """The case's call (or its rows) on the GPU, as numpy arrays."""
    pts, nrm, md = c["points"][rows], c["normals"][rows], None if c["max_dist"] is None else c["max_dist"][rows]
    if torch_path:
        import torch
        pts, nrm = torch.from_numpy(pts).to("cuda:0"), torch.from_numpy(nrm).to("cuda:0")
        md = None if md is None else torch.from_numpy(md).to("cuda:0")
    else:
        pts, nrm = np.ascontiguousarray(pts), np.ascontiguousarray(nrm)
        md = None if md is None else np.ascontiguousarray(md)
    res = r.hemisphere_visibility(pts, nrm, samples=c["samples"], seed=c["seed"], first=c["first"] if first is None else first,
                                  max_dist=md, ray_bias=float(c["ray_bias"]), fields=fields, count_visits=count_visits)
    return H.to_numpy(res)


def check(r, c, exp, what):
    for torch_path in (False, True):
        res = query(r, c, torch_path=torch_path)
        H.assert_same_bits(res, exp, "%s (%s)" % (what, "torch" if torch_path else "numpy"))
        assert res["counters"].ray_count == exp["cast"], (what, res["counters"].ray_count, exp["cast"])
        assert res["counters"].pipeline == 0 and res["counters"].render_ms >= res["counters"].trace_kernel_ms > 0


def shape_cases(name):
    mesh, pts, nrm = scene_points(name)
    return [H.case(mesh, pts[:n], nrm[:n], s, seed=SEED, first=FIRST) for n in COUNTS for s in SAMPLES]


# ---- shapes, entry points, fields

@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_counts_and_samples_against_the_harness(harness, name):
    from par_raytracer_amd import api
    cases = shape_cases(name)
    expect = harness(cases)
    H.assert_input_mix(expect[-1], SAMPLES[-1], name)
    r = api.Renderer(0)
    try:
        r.upload(S.flat_desc(cases[0]["mesh"]))
        for c, exp in zip(cases, expect):
            check(r, c, exp, "%s, %d points x %d" % (name, c["points"].shape[0], c["samples"]))
        res = query(r, cases[-1], count_visits=True)
        H.assert_same_bits(res, expect[-1], name + ", counted")
        assert res["counters"].node_visits > 0 and res["counters"].tri_tests > 0
    finally:
        r.close()


@pytest.mark.gpu
def test_past_one_pass_of_a_small_grid(harness):
    """320 points x 64 = 20,480 items: more than the 16,384 lanes of an 8-compute-unit grid, so waves refill from the head."""
    from par_raytracer_amd import api
    mesh, pts, nrm = scene_points("torus", 320)
    c = H.case(mesh, pts, nrm, 64, seed=3)
    assert pts.shape[0] * 64 == 20480
    exp = harness([c])[0]
    H.assert_input_mix(exp, 64, "torus")
    r = api.Renderer(0)
    try:
        r.upload(S.flat_desc(mesh))
        check(r, c, exp, "20480 items")
    finally:
        r.close()


@pytest.mark.gpu
def test_every_subset_of_the_fields(harness):
    import torch
    from par_raytracer_amd import api
    mesh, pts, nrm = scene_points("torus", 65)
    cases = [H.case(mesh, pts, nrm, s, seed=9, first=1) for s in (7, 64)]
    expect = harness(cases)
    r = api.Renderer(0)
    try:
        r.upload(S.flat_desc(mesh))
        for c, exp in zip(cases, expect):
            for size in range(len(H.FIELDS) + 1):
                for fields in itertools.combinations(H.FIELDS, size):
                    for torch_path in (False, True):
                        res = query(r, c, fields=fields, torch_path=torch_path)
                        assert set(res) == set(fields) | {"counters"}
                        H.assert_same_bits(res, exp, "fields %r" % (fields,), fields)
        t = r.hemisphere_visibility(torch.from_numpy(pts).to("cuda:0"), torch.from_numpy(nrm).to("cuda:0"), samples=7)
        assert t["unoccluded"].dtype == torch.int32 and t["unoccluded"].device.type == "cuda" and t["bent"].shape == (65, 3)
        with pytest.raises(ValueError, match="unknown hemisphere-visibility field 'occluded'"):
            r.hemisphere_visibility(pts, nrm, fields=("occluded",))
        with pytest.raises(ValueError):
            r.hemisphere_visibility(pts, nrm[:5])
    finally:
        r.close()


# ---- the public rule

@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_composition_with_occluded_queries(harness, name):
    """The harness's rays through trace_rays(mode="occluded") on the same context: 1 - occluded summed per point is unoccluded,
    with and without a reach."""
    from par_raytracer_amd import api
    mesh, pts, nrm = scene_points(name, 65)
    reach = np.linspace(0.05, 2.0, 65).astype(np.float32) * np.float32(K.mesh_extent(mesh)[2])
    reach[::7] = np.inf
    cases = [H.case(mesh, pts, nrm, 100, seed=21, first=2 ** 32 - 65), H.case(mesh, pts, nrm, 100, seed=21, first=2 ** 32 - 65, max_dist=reach)]
    expect = harness(cases)
    assert (expect[1]["unoccluded"] != expect[0]["unoccluded"]).any(), "the reach matters"
    r = api.Renderer(0)
    try:
        r.upload(S.flat_desc(mesh))
        for c, exp in zip(cases, expect):
            origins = np.ascontiguousarray(np.repeat(pts, 100, axis=0))
            dirs = np.ascontiguousarray(exp["dirs"].reshape(-1, 3))
            tmax = None if c["max_dist"] is None else np.ascontiguousarray(np.repeat(c["max_dist"], 100))
            occ = r.trace_rays(origins, dirs, mode="occluded", tmax=tmax, ray_bias=float(c["ray_bias"]))["occluded"]
            by_rays = (1 - occ.reshape(65, 100).astype(np.int64)).sum(1)
            got = query(r, c)
            assert np.array_equal(by_rays, got["unoccluded"].astype(np.int64)), name
            assert np.array_equal(1 - occ.reshape(65, 100), exp["brute"]), name
            H.assert_same_bits(got, exp, name)
    finally:
        r.close()


# ---- purity

@pytest.fixture(scope="module")
def purity_case(harness):
    mesh, pts, nrm = scene_points("torus")
    c = H.case(mesh, pts, nrm, 100, seed=31, first=1000)
    return c, harness([c])[0]


@pytest.mark.gpu
def test_a_batch_in_parts_and_in_passes(purity_case):
    """Split at arbitrary points with `first` moved along; passes of 4096 items (40 points each) and of one point each."""
    from par_raytracer_amd import api
    c, exp = purity_case
    r = api.Renderer(0)
    try:
        r.upload(S.flat_desc(c["mesh"]))
        for torch_path in (False, True):
            parts = [query(r, c, torch_path=torch_path, rows=slice(a, b), first=1000 + a) for a, b in ((0, 1), (1, 100), (100, 257))]
            H.assert_same_bits({f: np.concatenate([p[f] for p in parts]) for f in H.FIELDS}, exp, "three calls")
            assert sum(p["counters"].ray_count for p in parts) == exp["cast"]
        for items in (4096, 100, 1):                           # 1: clamped to one point
            r.set_option("HEMI_PASS_ITEMS", items)
            check(r, c, exp, "HEMI_PASS_ITEMS=%d" % items)
        r.set_option("HEMI_PASS_ITEMS", None)
        check(r, c, exp, "default passes")
    finally:
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("option", [("STACK_CAP", 2), ("BVH_BUILDER", "lbvh")])
def test_same_bits_under_other_schedules_and_trees(harness, purity_case, option):
    """STACK_CAP=2: the smallest LDS column, every walk that pushes more goes to the slow list and k_hemi_exact."""
    from par_raytracer_amd import api
    c, exp = purity_case
    box = scene_points("cornell_box")
    cb = H.case(box[0], box[1], box[2], 64, seed=5)
    expb = harness([cb])[0]
    r = api.Renderer(0)
    try:
        r.set_option(*option)
        for case, e in ((c, exp), (cb, expb)):
            r.upload(S.flat_desc(case["mesh"]))
            check(r, case, e, "%s=%s" % option)
    finally:
        r.close()


CHILD = r"""
import os, sys, tempfile
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, "tests")); sys.path.insert(0, os.path.join(%(root)r, "oracle"))
import numpy as np
import hemi_cases as H
import signed_cases as S
from test_gpu_hemi import check, scene_points
from par_raytracer_amd import api, capi
lib = capi.hip_lib()
assert os.path.basename(lib._name) == "libprt_hip_bvh8.so" and not (lib.prt_build_flags() & capi.BUILD_BVH4)
d = tempfile.mkdtemp(prefix="prt_hemi8_")
exe = H.build_harness(d)
for name in ("torus", "cornell_box"):
    mesh, pts, nrm = scene_points(name)
    cases = [H.case(mesh, pts, nrm, s, seed=31, first=1000) for s in (7, 100)]
    expect = H.run_harness(exe, cases, d)
    r = api.Renderer(0)
    r.upload(S.flat_desc(mesh))
    for c, e in zip(cases, expect):
        check(r, c, e, name + " / 8-wide")
    r.set_option("STACK_CAP", 2)
    check(r, cases[1], expect[1], name + " / 8-wide, STACK_CAP=2")
    r.close()
    print(name, "equal", flush=True)
print("bvh8 hemisphere visibility ok")
"""


@pytest.mark.gpu
def test_same_bits_on_the_8_wide_library():
    assert os.path.exists(os.path.join(ROOT, "par_raytracer_amd", "libprt_hip_bvh8.so")), "libprt_hip_bvh8.so not built (make hip-bvh8)"
    env = dict(os.environ)
    env["PRT_HIP_LIB"] = "libprt_hip_bvh8.so"
    out = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         timeout=600)
    assert out.returncode == 0 and b"bvh8 hemisphere visibility ok" in out.stdout, (out.returncode, out.stdout.decode()[-1500:],
                                                                                    out.stderr.decode()[-3000:])


@pytest.mark.gpu
def test_visibility_follows_the_geometry(harness):
    """After update_geometry to the sheared mirror image: the harness's bits on the moved mesh, and those of a fresh upload of it."""
    from par_raytracer_amd import api
    mesh = S.torus()
    moved = S.sheared_mirror(mesh)
    pts, nrm = H.mixed_points(moved, 257, 41)
    here, there = H.case(mesh, pts, nrm, 64, seed=8), H.case(moved, pts, nrm, 64, seed=8)
    e_here, e_there = harness([here, there])
    assert (e_here["unoccluded"] != e_there["unoccluded"]).any(), "the move matters"
    H.assert_input_mix(e_there, 64, "moved torus")
    r, fresh = api.Renderer(0), api.Renderer(0)
    try:
        r.upload(S.flat_desc(mesh))
        check(r, here, e_here, "before the move")
        r.update_geometry(moved[0])
        check(r, there, e_there, "moved")
        fresh.upload(S.flat_desc(moved))
        H.assert_same_bits(query(r, there), query(fresh, there), "moved against a fresh upload")
        r.update_geometry(mesh[0])
        check(r, here, e_here, "moved back")
    finally:
        r.close()
        fresh.close()


# ---- edges

def edge_inputs(mesh):
    pts, nrm = H.surface_points(mesh, 16, 9)
    pts, nrm = np.tile(pts, (2, 1)), np.tile(nrm, (2, 1))              # 32 points: the second half gets the edge values
    md = np.full(32, np.inf, np.float32)
    bad = (16, 17, 18, 19, 20)
    pts[16, 1], pts[17, 0] = np.nan, np.inf
    nrm[18, 2], nrm[19, 0] = np.nan, -np.inf
    nrm[20] = 0
    md[21], md[22], md[23], md[24] = 0.0, -1.0, np.nan, np.inf
    md[:16] = 0.3
    pts[25] = np.array([100.0 * K.mesh_extent(mesh)[2], 0.0, 0.0], np.float32)      # query_far
    nrm[25] = np.array([-1.0, 0.0, 0.0], np.float32)
    return pts, nrm, md, bad


@pytest.mark.gpu
def test_edges(harness):
    """NaN and inf in a point or a normal, a zero normal; max_dist 0, negative, NaN and +inf; a point 100 extents away; the scene
    of no triangles; count == 0; ray_count = valid points x samples."""
    from par_raytracer_amd import api
    mesh = S.torus()
    pts, nrm, md, bad = edge_inputs(mesh)
    empty = (mesh[0], np.zeros(0, np.uint32), np.zeros((0, 2), np.uint32))
    cases = [H.case(mesh, pts, nrm, s, seed=4, max_dist=m) for s in (7, 64) for m in (None, md)]
    none = [H.case(empty, pts, nrm, s, seed=4) for s in (7, 64)]
    expect, e_none = harness(cases), harness(none)
    for e in expect + e_none:
        assert e["cast"] == (32 - len(bad)) * e["brute"].shape[1] and (e["unoccluded"][list(bad)] == H.INVALID).all()
    assert (expect[3]["unoccluded"][21:24] == 64).all()
    valid = np.setdiff1d(np.arange(32), bad)
    r = api.Renderer(0)
    try:
        r.upload(S.flat_desc(mesh))
        for c, e in zip(cases, expect):
            check(r, c, e, "edges, %d samples%s" % (c["samples"], "" if c["max_dist"] is None else ", max_dist"))
        for torch_path in (False, True):
            res = query(r, H.case(mesh, pts[:0], nrm[:0], 64), torch_path=torch_path)
            assert all(len(res[f]) == 0 for f in H.FIELDS) and res["counters"].ray_count == 0
        r.upload(S.flat_desc(empty))
        for c, e in zip(none, e_none):
            check(r, c, e, "no triangles")
            assert (e["unoccluded"][valid] == c["samples"]).all()
    finally:
        r.close()


# ---- refusals

@pytest.mark.gpu
def test_refusals():
    """Each refusal's code and text, through both entry points; nothing is written."""
    from par_raytracer_amd import api, capi
    lib = capi.hip_lib()
    mesh = S.tetrahedron()
    pts = np.array([[0, 0, 2], [0, 0, 3], [0, 0, 4], [0, 0, 5]], np.float32)
    nrm = np.tile(np.array([[0, 0, -1]], np.float32), (4, 1))
    un, vis = np.full(4, 77, np.uint32), np.full(4, 7.5, np.float32)
    out = capi.PrtHemiBuffers(un.ctypes.data, vis.ctypes.data, None)

    def batch(points=pts.ctypes.data, normals=nrm.ctypes.data, count=4, samples=8, first=0):
        return capi.PrtHemiBatch(points, normals, None, count, samples, 1, first, 0.0)
    r = api.Renderer(0)

    def last():
        return lib.prt_last_error(r._ctx).decode()
    try:
        for entry in (lib.prt_hemisphere_visibility, lib.prt_hemisphere_visibility_device):
            assert entry(None, C.byref(batch()), C.byref(out), 0, None) == -1
            assert entry(r._ctx, C.byref(batch()), C.byref(out), 0, None) == -2
            assert last() == "prt_hemisphere_visibility: no scene uploaded"
        with pytest.raises(RuntimeError, match=r"prt_hemisphere_visibility failed \(-2\): prt_hemisphere_visibility: no scene uploaded"):
            r.hemisphere_visibility(pts, nrm)
        r.upload(S.flat_desc(mesh))
        counters = capi.PrtCounters()
        for entry in (lib.prt_hemisphere_visibility, lib.prt_hemisphere_visibility_device):
            assert entry(r._ctx, None, C.byref(out), 0, None) == -1 and last() == "prt_hemisphere_visibility: null batch or buffers"
            assert entry(r._ctx, C.byref(batch()), None, 0, None) == -1 and last() == "prt_hemisphere_visibility: null batch or buffers"
            for b in (batch(points=None), batch(normals=None)):
                assert entry(r._ctx, C.byref(b), C.byref(out), 0, None) == -1 and last() == "prt_hemisphere_visibility: null points or normals"
            for s in (0, 65536, 2 ** 32 - 1):
                assert entry(r._ctx, C.byref(batch(samples=s)), C.byref(out), 0, None) == -1, s
                assert last() == "prt_hemisphere_visibility: samples must be in 1..65535 (prt_key.h packs the sample in 16 bits)"
            for first, count in ((2 ** 32 - 3, 4), (2 ** 32 + 1, 0), (2 ** 64 - 1, 4)):
                assert entry(r._ctx, C.byref(batch(first=first, count=count)), C.byref(out), 0, None) == -1, (first, count)
                assert last() == "prt_hemisphere_visibility: first + count exceeds 2^32 (the point index is the key's pixel word)"
            # count == 0: nothing is written, the counters are zeroed; null arrays are then fine
            counters.ray_count = 99
            assert entry(r._ctx, C.byref(batch(points=None, normals=None, count=0, first=2 ** 32)), C.byref(out), 0, C.byref(counters)) == 0
            assert counters.ray_count == 0
        assert np.all(un == 77) and np.all(vis == 7.5), "nothing was written"
        with pytest.raises(RuntimeError, match=r"\(-1\): prt_hemisphere_visibility: samples must be in 1\.\.65535"):
            r.hemisphere_visibility(pts, nrm, samples=0)
        with pytest.raises(RuntimeError, match=r"\(-1\): prt_hemisphere_visibility: first \+ count exceeds 2\^32"):
            r.hemisphere_visibility(pts, nrm, first=2 ** 32 - 3)
        assert lib.prt_hemisphere_visibility(r._ctx, C.byref(batch(first=2 ** 32 - 4, samples=65535)), C.byref(out), 0, C.byref(counters)) == 0
        assert counters.ray_count == 4 * 65535 and np.all(un <= 65535) and np.all(vis != 7.5)
    finally:
        r.close()
