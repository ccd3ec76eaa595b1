"""prt_sample_surface and prt_sample_surface_backward on the GPU against the brute force of tests/sample_host_harness.cpp (the
definition with the PRT_HD functions of csrc/dev_sample.h and csrc/dev_sample_grad.h, built here with g++): every field and the
info integers bit for bit, through the host entry point (numpy) and the device entry point (torch), on the SAH tree, the LBVH tree
and the 8-wide library; sample counts around the wave and the grid, every subset of the fields, triangle counts around the scan
kernels' tile and pass sizes, moved geometry, purity in `first`, in the split of a batch, in the context and in the grid; the empty
and the all-degenerate scene, the refusals; the backward call's bits, its info and its refusals; and
sample_surface_differentiable."""
from __future__ import annotations

import ctypes as C
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import closest_cases as K
import sample_cases as M
import signed_cases as S
from conftest import ROOT

COUNTS = (1, 63, 64, 65, 257, 20480)       # around a wave, past a block, and past one pass of an 8-compute-unit grid (16,384 lanes)
INTS = ("total_weight", "unit_exponent", "live_triangles")


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("sample_gpu")


@pytest.fixture(scope="module")
def harness(workdir):
    exe = M.build_harness(workdir)

    def run(mesh, requests=(), grads=()):
        return M.run_harness(exe, [M.case(mesh, requests, grads)], workdir)[0]
    return run


def sample(r, count, seed, first=0, fields=None, torch_path=False):
    res = r.sample_surface(count, seed=seed, first=first, fields=fields, out="torch" if torch_path else "numpy")
    return M.to_numpy(res)


def assert_info(info, expect, what):
    for k in INTS:
        assert getattr(info, k) == expect[k], (what, k, getattr(info, k), expect[k])
    assert info.area == expect["area"], (what, info.area, expect["area"])
    assert info.device_ms >= info.table_ms >= 0.0, what


def check_counts(r, mesh, harness, what, seed=7):
    """COUNTS samples through both entry points against the harness."""
    expect = harness(mesh, [M.request(seed, 0, n) for n in COUNTS])
    for n, exp in zip(COUNTS, expect["samples"]):
        for torch_path in (False, True):
            res = sample(r, n, seed, torch_path=torch_path)
            M.assert_same_bits(res, exp, "%s, %d samples (%s)" % (what, n, "torch" if torch_path else "numpy"))
            assert_info(res["info"], expect, what)
    return expect


# ---- sample counts, trees, fields

@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cube", "torus"])
@pytest.mark.parametrize("builder", ["sah", "lbvh"])
def test_sample_counts_around_the_wave_and_the_grid(harness, name, builder):
    from par_raytracer_amd import api
    mesh = S.mesh_of(name)
    r = api.Renderer(0)
    try:
        if builder != "sah":
            r.set_option("BVH_BUILDER", builder)
        r.upload(S.flat_desc(mesh))
        expect = check_counts(r, mesh, harness, "%s / %s" % (name, builder))
        assert expect["live_triangles"] == mesh[1].size // 3
        big = expect["samples"][-1]
        assert len(np.unique(K.input_triangle(mesh, big["group"], big["vertex0"]))) == mesh[1].size // 3, "every triangle is drawn"
    finally:
        r.close()


@pytest.mark.gpu
def test_every_subset_of_the_fields(harness):
    import torch
    from par_raytracer_amd import api
    mesh = S.torus()
    n = 257
    expect = harness(mesh, [M.request(3, 5, n)])["samples"][0]
    r = api.Renderer(0)
    try:
        r.upload(S.flat_desc(mesh))
        for size in range(len(M.FIELDS) + 1):
            for fields in itertools.combinations(M.FIELDS, size):
                for torch_path in (False, True):
                    res = r.sample_surface(n, seed=3, first=5, fields=fields, out="torch" if torch_path else "numpy")
                    assert set(res) == set(fields) | {"info"}
                    M.assert_same_bits(M.to_numpy(res), expect, "fields %r" % (fields,), fields)
                    if torch_path and "vertex0" in fields:
                        assert res["vertex0"].dtype == torch.int32 and res["vertex0"].device.type == "cuda"
        with pytest.raises(ValueError):
            r.sample_surface(4, fields=("dist2",))
        with pytest.raises(ValueError):
            r.sample_surface(4, out="cupy")
    finally:
        r.close()


CHILD = r"""
import os, sys, tempfile
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, "tests")); sys.path.insert(0, os.path.join(%(root)r, "oracle"))
import numpy as np
import sample_cases as M
import signed_cases as S
from test_gpu_sample import check_counts, backward_against_the_harness
from par_raytracer_amd import api, capi
lib = capi.hip_lib()
assert os.path.basename(lib._name) == "libprt_hip_bvh8.so" and not (lib.prt_build_flags() & capi.BUILD_BVH4)
d = tempfile.mkdtemp(prefix="prt_sample8_")
exe = M.build_harness(d)
harness = lambda mesh, requests=(), grads=(): M.run_harness(exe, [M.case(mesh, requests, grads)], d)[0]
for name in ("cube", "torus"):
    mesh = S.mesh_of(name)
    r = api.Renderer(0)
    r.upload(S.flat_desc(mesh))
    check_counts(r, mesh, harness, name + " / 8-wide")
    moved = S.sheared_mirror(mesh)
    r.update_geometry(moved[0])
    check_counts(r, moved, harness, name + " / 8-wide, moved")
    r.close()
    print(name, "equal", flush=True)
backward_against_the_harness(harness, "fan")
print("bvh8 surface samples ok")
"""


@pytest.mark.gpu
def test_meshes_on_the_8_wide_library():
    assert os.path.exists(os.path.join(ROOT, "par_raytracer_amd", "libprt_hip_bvh8.so")), "libprt_hip_bvh8.so not built (make hip-bvh8)"
    env = dict(os.environ)
    env["PRT_HIP_LIB"] = "libprt_hip_bvh8.so"
    out = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         timeout=600)
    assert out.returncode == 0 and b"bvh8 surface samples ok" in out.stdout, (out.returncode, out.stdout.decode()[-1500:],
                                                                               out.stderr.decode()[-3000:])


# ---- the scan's boundaries

# csrc/kernels_sample.h: a tile is SAMPLE_TILE = 256 triangles (one block of k_sample_tiles), and one pass of k_sample_totals' loop
# scans SAMPLE_TILE tiles = 65,536 triangles.  1 and 2 triangles; 255, 256, 257: one tile short, full, and a second tile of one
# triangle; 65,535, 65,536, 65,537: one pass short, full, and a second pass of one tile of one triangle; height_field(182, 2)
# whole: 66,248 triangles, a second pass of three tiles.
SCAN_COUNTS = (1, 2, M.SAMPLE_TILE - 1, M.SAMPLE_TILE, M.SAMPLE_TILE + 1, M.TOTALS_PASS - 1, M.TOTALS_PASS, M.TOTALS_PASS + 1, 2 * 182 * 182)


@pytest.mark.gpu
@pytest.mark.parametrize("n_tris", SCAN_COUNTS)
def test_scan_boundaries(harness, n_tris):
    """C through total_weight and through 20,480 samples: a wrong tile offset moves every later triangle's interval."""
    from par_raytracer_amd import api
    assert M.SAMPLE_TILE == 256 and M.TOTALS_PASS == 65536 and SCAN_COUNTS[-1] == 66248 >= 2 ** 16 + 1
    mesh = M.height_field_of(n_tris)
    assert mesh[1].size == 3 * n_tris
    n = 20480
    expect = harness(mesh, [M.request(13, 0, n)])
    assert expect["live_triangles"] == n_tris
    r = api.Renderer(0)
    try:
        r.upload(S.flat_desc(mesh))
        res = sample(r, n, 13)
        assert_info(res["info"], expect, "%d triangles" % n_tris)
        assert res["info"].table_ms > 0
        M.assert_same_bits(res, expect["samples"][0], "%d triangles" % n_tris)
        t = K.input_triangle(mesh, res["group"], res["vertex0"])
        assert t.max() >= min(n_tris - 1, (n_tris * 3) // 4), "the samples reach the last tiles"
    finally:
        r.close()


# ---- geometry

@pytest.mark.gpu
def test_samples_follow_the_geometry(harness):
    """Query, update_geometry to sheared_mirror(mesh), query, and back: each time the harness's bits on the mesh as it is now and
    those of a fresh upload of it.  The shear changes the ratios of the areas, so a stale C draws other triangles.  table_ms > 0
    on exactly the first call after each move."""
    from par_raytracer_amd import api
    mesh = S.torus()
    moved = S.sheared_mirror(mesh)
    n = 4096
    here, there = harness(mesh, [M.request(17, 0, n)]), harness(moved, [M.request(17, 0, n)])
    assert here["total_weight"] != there["total_weight"]
    assert not np.array_equal(here["samples"][0]["vertex0"], there["samples"][0]["vertex0"]), "the shear moves the intervals"
    r = api.Renderer(0)
    try:
        r.upload(S.flat_desc(mesh))
        for at, expect, step in ((mesh, here, "uploaded"), (moved, there, "moved"), (mesh, here, "moved back")):
            if step != "uploaded":
                r.update_geometry(at[0])
            first = sample(r, n, 17)
            again = sample(r, n, 17, torch_path=True)
            for res in (first, again):
                M.assert_same_bits(res, expect["samples"][0], step)
                assert_info(res["info"], expect, step)
            assert first["info"].table_ms > 0 and again["info"].table_ms == 0, step
            fresh = api.Renderer(0)
            try:
                fresh.upload(S.flat_desc(at))
                res = sample(fresh, n, 17)
                M.assert_same_bits(res, first, step + ", fresh upload")
                assert_info(res["info"], expect, step + ", fresh upload")
            finally:
                fresh.close()
    finally:
        r.close()


# ---- purity

@pytest.mark.gpu
def test_samples_are_a_function_of_their_index(harness, monkeypatch):
    """The values of `first` at which the key's packing crosses its fields; a batch split into two calls; two fresh contexts; and a
    context of 8 compute units (PRT_RESERVE_CUS = the device's count - 8, as tests/test_gpu_signed_schedules.py reserves them):
    its grids are at most 64 blocks, so k_sample strides over 20,480 samples and the table's kernels over height_field(96, 5)'s
    18,432 triangles = 72 tiles."""
    import torch
    from par_raytracer_amd import api
    mesh = K.height_field(96, 5)
    n = 20480
    assert mesh[1].size // 3 == 18432 > 64 * M.SAMPLE_TILE and n > 8 * 8 * 256
    expect = harness(mesh, [M.request(19, f, 64) for f in M.FIRSTS] + [M.request(19, 0, n)])
    assert not os.environ.get("PRT_RESERVE_CUS")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert cus > 16
    monkeypatch.setenv("PRT_RESERVE_CUS", str(cus - 8))
    small = api.Renderer(0)
    monkeypatch.delenv("PRT_RESERVE_CUS")
    assert not os.environ.get("PRT_RESERVE_CUS")
    one, two = api.Renderer(0), api.Renderer(0)
    try:
        for r in (small, one, two):
            r.upload(S.flat_desc(mesh))
        for f, exp in zip(M.FIRSTS, expect["samples"]):
            for torch_path in (False, True):
                M.assert_same_bits(sample(one, 64, 19, first=f, torch_path=torch_path), exp, "first = %d" % f)
        whole = expect["samples"][-1]
        M.assert_same_bits(sample(one, n, 19), whole, "one call")
        M.assert_same_bits(sample(two, n, 19, torch_path=True), whole, "another context")
        cut = 7777
        head, tail = sample(two, cut, 19), sample(two, n - cut, 19, first=cut)
        M.assert_same_bits({k: np.concatenate([head[k], tail[k]]) for k in M.FIELDS}, whole, "a batch in two calls")
        # (the host entry point alone: a context with a CU mask has blocking streams, which torch's null stream would join)
        res = sample(small, n, 19)
        M.assert_same_bits(res, whole, "8 compute units")
        assert_info(res["info"], expect, "8 compute units")
        moved = S.sheared_mirror(mesh)
        small.update_geometry(moved[0])
        there = harness(moved, [M.request(19, 0, n)])
        res = sample(small, n, 19)
        M.assert_same_bits(res, there["samples"][0], "8 compute units, moved")
        assert_info(res["info"], there, "8 compute units, moved")
    finally:
        for r in (small, one, two):
            r.close()


# ---- edges

@pytest.mark.gpu
def test_scenes_without_area_miss_everywhere():
    from par_raytracer_amd import api
    empty = (np.zeros((3, 3), np.float32), np.zeros(0, np.uint32), np.zeros((0, 2), np.uint32))
    for mesh, what in ((empty, "the empty scene"), (M.all_degenerate(), "the all-degenerate scene")):
        r = api.Renderer(0)
        try:
            r.upload(S.flat_desc(mesh))
            for torch_path in (False, True):
                res = sample(r, 130, 1, torch_path=torch_path)
                M.assert_all_miss(res, what)
                info = res["info"]
                assert (info.total_weight, info.unit_exponent, info.live_triangles, info.area) == (0, 0, 0, 0.0), what
            back = r.sample_surface_backward(res["group"], res["vertex0"], res["bw"], mesh[0], grad_point=np.ones((130, 3), np.float32))
            assert np.all(back["positions"] == 0) and back["info"].hit_rays == 0 and back["info"].skipped_rays == 0
        finally:
            r.close()


@pytest.mark.gpu
def test_errors_and_count_zero():
    from par_raytracer_amd import api, capi
    lib = capi.hip_lib()
    mesh = S.tetrahedron()
    point = np.full((4, 3), 7.5, np.float32)
    group = np.full(4, 77, np.int32)
    out = capi.PrtSampleBuffers(point.ctypes.data, None, None, None, group.ctypes.data)
    rq = capi.PrtSampleRequest(1, 0, 4)
    info = capi.PrtSampleInfo()
    r = api.Renderer(0)

    def last():
        return lib.prt_last_error(r._ctx).decode()
    try:
        for entry in (lib.prt_sample_surface, lib.prt_sample_surface_device):
            assert entry(r._ctx, C.byref(rq), C.byref(out), None) == -2 and "no scene uploaded" in last()
            assert entry(None, C.byref(rq), C.byref(out), None) == -1
        with pytest.raises(RuntimeError, match=r"prt_sample_surface failed \(-2\): prt_sample_surface: no scene uploaded"):
            r.sample_surface(4)
        r.upload(S.flat_desc(mesh))
        for entry in (lib.prt_sample_surface, lib.prt_sample_surface_device):
            assert entry(r._ctx, None, C.byref(out), None) == -1 and "null request or buffers" in last()
            assert entry(r._ctx, C.byref(rq), None, C.byref(info)) == -1 and "null request or buffers" in last()
            for first, count in ((2 ** 48 - 3, 4), (2 ** 48 + 1, 0), (2 ** 64 - 1, 4)):
                far = capi.PrtSampleRequest(1, first, count)
                assert entry(r._ctx, C.byref(far), C.byref(out), None) == -1 and "first + count exceeds 2^48" in last(), (first, count)
            info.total_weight = 99
            assert entry(r._ctx, C.byref(capi.PrtSampleRequest(1, 2 ** 48, 0)), C.byref(out), C.byref(info)) == 0 and info.total_weight == 0
        assert np.all(point == 7.5) and np.all(group == 77), "nothing was written"
        with pytest.raises(RuntimeError, match=r"\(-1\): prt_sample_surface: first \+ count exceeds 2\^48"):
            r.sample_surface(4, first=2 ** 48 - 3)
        assert lib.prt_sample_surface(r._ctx, C.byref(capi.PrtSampleRequest(1, 2 ** 48 - 4, 4)), C.byref(out), C.byref(info)) == 0
        assert np.all(group == 0) and np.all(point != 7.5) and info.live_triangles == 4 and info.table_ms > 0
        for k in (0, 1):
            res = r.sample_surface(0, out=("numpy", "torch")[k])
            assert all(len(res[f]) == 0 for f in M.FIELDS)
    finally:
        r.close()


# ---- backward

def backward(r, smp, positions, gp, gn, torch_path, merge=None):
    r.set_option("QGRAD_MERGE", merge)
    try:
        if torch_path:
            import torch
            dev = torch.device("cuda", r.device_id)
            t = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)         # noqa: E731
            res = r.sample_surface_backward(t(smp["group"]), t(smp["vertex0"].view(np.int32)), t(smp["bw"]), t(positions), grad_point=t(gp),
                                            grad_normal=t(gn))
            return dict(positions=res["positions"].cpu().numpy(), info=res["info"])
        return r.sample_surface_backward(smp["group"], smp["vertex0"], smp["bw"], positions, grad_point=gp, grad_normal=gn)
    finally:
        r.set_option("QGRAD_MERGE", None)


def assert_grad(res, exp, what):
    assert np.array_equal(res["positions"].view(np.uint32), exp["positions"].view(np.uint32)), what
    info = res["info"]
    assert (info.hit_rays, info.skipped_rays, info.unit_exponent, info.max_contribution) == (exp["hit"], exp["skipped"], exp["unit_exponent"],
                                                                                              exp["max_contribution"]), what
    assert info.device_ms > 0, what


def backward_against_the_harness(harness, name):
    """The device's own forward samples, then the backward call's bits against the harness's: with both, one and no output gradient,
    permuted samples, QGRAD_MERGE both ways, numpy and torch."""
    from par_raytracer_amd import api
    mesh = S.mesh_of(name)
    n = 4096 + 37
    r = api.Renderer(0)
    try:
        r.upload(S.flat_desc(mesh))
        smp = sample(r, n, 23)
        gp, gn = M.random_grads(n, 24)
        perm = np.random.default_rng(25).permutation(n)
        shuffled = {k: np.ascontiguousarray(smp[k][perm]) for k in M.FIELDS}
        calls = [M.grad_call(smp["group"], smp["vertex0"], smp["bw"], a, b) for a, b in ((gp, gn), (gp, None), (None, gn), (None, None))]
        exp = harness(mesh, grads=calls)["grads"]
        assert exp[0]["hit"] == n and exp[0]["max_contribution"] > 0 and exp[3]["max_contribution"] == 0 and np.all(exp[3]["positions"] == 0)
        for (a, b), e, what in zip(((gp, gn), (gp, None), (None, gn), (None, None)), exp, ("point + normal", "point", "normal", "none")):
            for torch_path in (False, True):
                for merge in (0, 1):
                    assert_grad(backward(r, smp, mesh[0], a, b, torch_path, merge), e, "%s, %s, merge %d" % (name, what, merge))
        for merge in (0, 1):
            res = backward(r, shuffled, mesh[0], gp[perm], gn[perm], merge == 1, merge)
            assert_grad(res, exp[0], "%s, permuted, merge %d" % (name, merge))
        M.check_grad_against_yardstick(mesh, calls[0], res["positions"], name)
    finally:
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["torus", "fan"])
def test_backward_equals_the_harness(harness, name):
    backward_against_the_harness(harness, name)


@pytest.mark.gpu
def test_backward_skips_and_refusals(harness):
    """The skipped classes (a miss, a NaN in gout, a zero-area reference together with a normal gradient) against the harness, and
    the refusals: an invalid reference is refused before anything is written, and the text of prt_last_error says why."""
    from par_raytracer_amd import api, capi
    lib = capi.hip_lib()
    mesh = S.degenerate_cube()
    n = 256
    r = api.Renderer(0)
    try:
        r.upload(S.flat_desc(mesh))
        smp = sample(r, n, 41)
        gp, gn = M.random_grads(n, 42)
        group, vertex0, bw = smp["group"].copy(), smp["vertex0"].copy(), smp["bw"].copy()
        group[:16], vertex0[:16] = -1, 0xFFFFFFFF
        gp[16:32, 1] = np.nan
        group[32:48], vertex0[32:48] = 0, (3 * np.arange(16)).astype(np.uint32)          # group 0: the zero-area triangles
        bent = dict(group=group, vertex0=vertex0, bw=bw)
        exp = harness(mesh, grads=[M.grad_call(group, vertex0, bw, gp, gn), M.grad_call(group, vertex0, bw, gp, None)])["grads"]
        assert (exp[0]["hit"], exp[0]["skipped"]) == (n - 48, 32) and (exp[1]["hit"], exp[1]["skipped"]) == (n - 32, 16)
        for torch_path in (False, True):
            assert_grad(backward(r, bent, mesh[0], gp, gn, torch_path), exp[0], "skipped classes")
            assert_grad(backward(r, bent, mesh[0], gp, None, torch_path), exp[1], "skipped classes, point only")
        # refusals, through the C ABI: the output keeps its sentinel
        gin = np.full(mesh[0].shape, 7.5, np.float32)
        go = capi.PrtSampleGrads(gp.ctypes.data, gn.ctypes.data)
        info = capi.PrtGradInfo()
        ptr = lambda a: a.ctypes.data                                                      # noqa: E731

        def call(g, v, n_pos=len(mesh[0]), count=n, b=bw):
            return lib.prt_sample_surface_backward(r._ctx, count, ptr(g), ptr(v), None if b is None else ptr(b), ptr(mesh[0]), n_pos, C.byref(go), ptr(gin),
                                                   C.byref(info))
        for g, v in ((3, 0), (1, 1), (1, 36), (1, 0xFFFFFFFC)):
            gg, vv = group.copy(), vertex0.copy()
            gg[100], vv[100] = g, v
            assert call(gg, vv) == -1 and "1 samples name a triangle the scene does not have" in lib.prt_last_error(r._ctx).decode(), (g, v)
        assert call(group, vertex0, n_pos=len(mesh[0]) - 1) == -1 and "position_count differs" in lib.prt_last_error(r._ctx).decode()
        assert call(group, vertex0, b=None) == -1 and "null group, vertex0, bw or positions" in lib.prt_last_error(r._ctx).decode()
        assert np.all(gin == 7.5), "a refused call wrote to its output"
        assert call(group, vertex0, count=0) == 0 and np.all(gin == 0), "count == 0 zeroes the gradient"
        gin[:] = 7.5
        assert call(group, vertex0) == 0 and np.array_equal(gin.view(np.uint32), exp[0]["positions"].view(np.uint32))
        fresh = api.Renderer(0)
        try:
            assert lib.prt_sample_surface_backward(fresh._ctx, n, ptr(group), ptr(vertex0), ptr(bw), ptr(mesh[0]), len(mesh[0]), C.byref(go), ptr(gin),
                                                   None) == -2
        finally:
            fresh.close()
    finally:
        r.close()


# ---- autograd

@pytest.mark.gpu
def test_sample_surface_differentiable():
    """On the cube: the outputs are the library's bits; torch.autograd.grad of point.sum() and of (normal * c).sum() equals
    sample_surface_backward; and for a one-sided chamfer term - 4,096 samples against a fixed cloud - the float32 gradient is
    within 4 x 2^-23 x its largest component of a float64 torch restatement of the same sum."""
    import torch
    from par_raytracer_amd import api
    from par_raytracer_amd.autograd import sample_surface_differentiable
    mesh = S.cube()
    dev = torch.device("cuda", 0)
    n = 4096
    r = api.Renderer(0)
    try:
        r.upload(S.flat_desc(mesh))
        start = (mesh[0] + np.random.default_rng(5).uniform(-0.05, 0.05, mesh[0].shape)).astype(np.float32)
        pos = torch.from_numpy(start).to(dev).requires_grad_(True)
        point, normal, bw, group, vertex0 = sample_surface_differentiable(r, pos, n, seed=29)
        assert point.requires_grad and normal.requires_grad and not bw.requires_grad and not group.requires_grad and not vertex0.requires_grad
        direct = r.sample_surface(n, seed=29, out="torch")
        for k, t in (("point", point), ("normal", normal), ("bw", bw), ("group", group), ("vertex0", vertex0)):
            assert torch.equal(t.detach(), direct[k]), k
        c = torch.from_numpy(np.random.default_rng(6).standard_normal((n, 3)).astype(np.float32)).to(dev)
        g_point, = torch.autograd.grad(point.sum(), pos, retain_graph=True)
        g_normal, = torch.autograd.grad((normal * c).sum(), pos, retain_graph=True)
        ones = torch.ones_like(point)
        back = r.sample_surface_backward(group, vertex0, bw, pos.detach(), grad_point=ones)
        assert torch.equal(g_point, back["positions"]) and back["info"].hit_rays == n
        back = r.sample_surface_backward(group, vertex0, bw, pos.detach(), grad_normal=c)
        assert torch.equal(g_normal, back["positions"]) and float(g_normal.abs().max()) > 0
        # every sample's point gradient spreads bw over three corners: the columns sum to n
        assert abs(float(g_point.sum()) - 3.0 * n) <= 3.0 * n * 2.0 ** -20
        # a one-sided chamfer term: each sample to its nearest point of a fixed cloud (the pairing is fixed, as the triangles are).
        # The cloud is a scan of the cube inflated to [-0.25, 1.25]^3 - 2,048 points on its faces -, so that a vertex's residuals
        # point the same way and its gradient is not what is left of a cancellation.
        rng = np.random.default_rng(7)
        scan = rng.uniform(-0.25, 1.25, (2048, 3))
        scan[np.arange(2048), rng.integers(0, 3, 2048)] = rng.choice([-0.25, 1.25], 2048)
        cloud = torch.from_numpy(scan.astype(np.float32)).to(dev)
        with torch.no_grad():
            near = torch.cdist(point.detach().double(), cloud.double()).argmin(1)
        loss = ((point - cloud[near]) ** 2).sum(1).mean()
        g32, = torch.autograd.grad(loss, pos)
        # the float64 restatement: point = bw0 a + bw1 b + bw2 c on the same triangles, the same barycentrics, the same pairs
        idx = torch.from_numpy(mesh[1].astype(np.int64)).to(dev)
        corner = torch.from_numpy(mesh[2][:, 0].astype(np.int64)).to(dev)[group.long()] + (vertex0.long() & 0xFFFFFFFF)
        p64 = pos.detach().double().requires_grad_(True)
        a, b, cc = (p64[idx[corner + k]] for k in range(3))
        w = bw.double()
        point64 = a * w[:, :1] + b * w[:, 1:2] + cc * w[:, 2:]
        loss64 = ((point64 - cloud[near].double()) ** 2).sum(1).mean()
        g64, = torch.autograd.grad(loss64, p64)
        err = float((g32.double() - g64).abs().max())
        bound = 4.0 * 2.0 ** -23 * float(g64.abs().max())
        print("chamfer term: max |g32 - g64| = %.3g, bound %.3g" % (err, bound))
        assert err <= bound
        # update_geometry=False on the geometry already moved gives the same samples
        again = sample_surface_differentiable(r, pos, n, seed=29, update_geometry=False)
        assert torch.equal(again[0].detach(), point.detach())
    finally:
        r.close()
