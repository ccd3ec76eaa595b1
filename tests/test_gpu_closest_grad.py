"""prt_closest_points_backward on the GPU: the device's bits against the host harness's (tests/closest_grad_host_harness.cpp runs the
same kernels lane by lane) with the references of the device's own forward prt_closest_points call, the accuracy yardstick (torch CPU
autograd in float64, tests/closest_grad_cases.py), independence of point order, of the run and of QGRAD_MERGE, the mixed-wave and
repeated-point cases tests/test_closest_grad_host.py proves on the CPU, subsets and refusals, a moved scene, torch autograd through
par_raytracer_amd.autograd, ten steps of gradient descent, and the 8-wide library.  The backward call reads no tree, so small batches
reach everything: wave boundaries, the merge and one wrap of the capped grid."""
from __future__ import annotations

import os
import subprocess
import sys

import numpy as np
import pytest

import closest_cases as C
import closest_grad_cases as G
from closest_grad_cases import bits
from conftest import ROOT, host_scene

N = C.RECIPE_POINTS


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("closest_grad_gpu")
    exe = G.build_harness(d, sanitize=False)
    return lambda cases: G.run_harness(exe, cases, d)


@pytest.fixture(scope="module")
def scenes():
    """name -> (Renderer, mesh), uploaded once."""
    from par_raytracer_amd import api
    out = {}

    def get(name):
        if name not in out:
            r = api.Renderer(0)
            if name == "one_triangle":
                mesh = G.one_triangle()
                r.upload(G.flat_desc(mesh))
            else:
                mesh = G.scene_mesh(name)
                r.upload(host_scene(name, 0))
            out[name] = (r, mesh)
        return out[name]
    yield get
    for r, _ in out.values():
        r.close()


def forward(r, pts):
    """The device's own references for pts: (group, vertex0), every point a hit."""
    res = r.closest_points(pts, fields=("group", "vertex0"))
    assert np.all(res["group"] >= 0)
    return np.ascontiguousarray(res["group"]), np.ascontiguousarray(res["vertex0"])


def backward(r, pts, group, vertex0, p, g, torch_path, want=G.GRADS, merge=None):
    r.set_option("QGRAD_MERGE", merge)
    try:
        if torch_path:
            import torch
            cv = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
            res = r.closest_points_backward(cv(pts), cv(group), cv(vertex0.view(np.int32)), cv(p), grad_dist2=cv(g.get("dist2")),
                                            grad_point=cv(g.get("point")), grad_bw=cv(g.get("bw")), want=want)
            return {k: (v.cpu().numpy() if k != "info" else v) for k, v in res.items()}
        return r.closest_points_backward(pts, group, vertex0, p, grad_dist2=g.get("dist2"), grad_point=g.get("point"), grad_bw=g.get("bw"),
                                         want=want)
    finally:
        r.set_option("QGRAD_MERGE", None)


def same_as_harness(res, h):
    assert h["rc"] == 0
    for k in G.GRADS:
        assert np.array_equal(bits(res[k]), bits(h[k])), k
    info = res["info"]
    assert (info.hit_rays, info.skipped_rays, info.unit_exponent) == (h["hit_rays"], h["skipped_rays"], h["unit_exponent"])
    assert bits(np.float32(info.max_contribution)) == bits(h["max_contribution"])


def recipe(mesh, name):
    return C.recipe_points(mesh, N, 100 + ("cornell_box", "icosphere_l3").index(name))


@pytest.mark.gpu
@pytest.mark.parametrize("name,n", [("one_triangle", 1), ("one_triangle", 64), ("one_triangle", 65), ("cornell_box", N), ("icosphere_l3", N)])
def test_device_bits_equal_the_host_harness(scenes, harness, name, n):
    r, mesh = scenes(name)
    built = None
    if name == "one_triangle":
        pts, built = (G.points_over(mesh, [0], 1), np.array([6], np.int32)) if n == 1 else G.region_points(n)
    else:
        pts = recipe(mesh, name)[0]
    group, vertex0 = forward(r, pts)
    g = G.random_grads(n, 41)
    h = harness([G.case(mesh, pts, group, vertex0, g)])[0]
    assert h["hit_rays"] + h["skipped_rays"] == n
    if built is not None:                                  # every region occurs, where the builder put it
        assert np.array_equal(h["region"], built) and (n == 1 or set(h["region"]) == set(range(7)))
    for torch_path in (False, True):
        same_as_harness(backward(r, pts, group, vertex0, mesh[0], g, torch_path), h)


@pytest.mark.gpu
def test_yardstick_on_the_icosphere(scenes, harness):
    """The gate of tests/test_closest_grad_host.py on the device's results: NEAR + BOX + ON together, FAR alone."""
    r, mesh = scenes("icosphere_l3")
    for label, c in G.accuracy_cases(mesh, 1, lambda pts: dict(zip(("group", "vertex0"), forward(r, pts)))):
        if "dist2+point+bw" not in label:
            continue
        res = backward(r, c["points"], c["group"], c["vertex0"], mesh[0], c["gout"], torch_path=True)
        assert res["info"].hit_rays == len(c["group"]) and res["info"].skipped_rays == 0
        region = harness([c])[0]["region"]
        G.check_against_yardstick(mesh, c["points"], c["group"], c["vertex0"], region, c["gout"], res, "icosphere_l3 on the device, " + label)


@pytest.mark.gpu
def test_the_same_bits_twice_for_a_permuted_batch_and_for_both_merges(scenes):
    r, mesh = scenes("icosphere_l3")
    pts = recipe(mesh, "icosphere_l3")[0]
    group, vertex0 = forward(r, pts)
    g = G.random_grads(N, 61)
    first = backward(r, pts, group, vertex0, mesh[0], g, torch_path=True)
    again = backward(r, pts, group, vertex0, mesh[0], g, torch_path=True)
    p = np.random.default_rng(62).permutation(N)
    perm = backward(r, pts[p], group[p], vertex0[p], mesh[0], G.take(g, p), torch_path=True)
    assert np.abs(first["positions"]).max() > 0
    for k in G.GRADS:
        assert np.array_equal(bits(first[k]), bits(again[k])), k
    assert np.array_equal(bits(first["positions"]), bits(perm["positions"]))
    assert np.array_equal(bits(first["points"][p]), bits(perm["points"]))
    for merge in (0, 1):                                  # both forms of the scatter kernel
        res = backward(r, pts, group, vertex0, mesh[0], g, torch_path=True, merge=merge)
        for k in G.GRADS:
            assert np.array_equal(bits(first[k]), bits(res[k])), (k, merge)


# ---- the shared cases of tests/closest_grad_cases.py, which carry their own references and are proven on the CPU first

def backward_case(r, c, torch_path, merge=None):
    return backward(r, c["points"], c["group"], c["vertex0"], c["mesh"][0], c["gout"], torch_path, merge=merge)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell_box", "icosphere_l3"])
def test_mixed_waves_equal_the_host_harness(scenes, harness, name):
    r, mesh = scenes(name)
    c = G.wave_layout_case(mesh, 200, False)
    h = harness([c])[0]
    expect = G.exact_integer_sum(mesh, c, h)
    assert (h["hit_rays"], h["skipped_rays"]) == (c["hit_rays"], c["skipped_rays"])
    for merge in (0, 1):
        for torch_path in (False, True):
            res = backward_case(r, c, torch_path, merge)
            same_as_harness(res, h)
            assert np.array_equal(bits(res["positions"]), bits(expect)), (merge, torch_path)
            assert np.all(bits(res["points"][~c["contributing"]]) == 0)


@pytest.mark.gpu
def test_a_repeated_point_past_one_grid_pass(scenes, harness):
    """grad_backward caps the grid at 8 * cu_count blocks of 256: this batch is two full passes of it, three waves and 37 lanes."""
    import torch
    # the context's cu_count starts as the device's multiprocessor count; PRT_RESERVE_CUS can only lower it, which shortens a pass
    assert not os.environ.get("PRT_RESERVE_CUS")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    count = 2 * 8 * cus * 256 + 3 * 64 + 37
    assert count > 8 * cus * 256 and count % 64 == 37
    r, mesh = scenes("cornell_box")
    rep = G.repeated_point_case(mesh, count)
    h = harness([rep])[0]
    assert h["hit_rays"] == count
    expect, top_bits = G.repeated_point_expectation(mesh, rep, h)
    assert 59 <= top_bits <= 62
    for merge in (0, 1):                                  # merge 0: every point's 9 adds land on the same 9 words
        res = backward_case(r, rep, True, merge)
        same_as_harness(res, h)
        assert np.array_equal(bits(res["positions"]), bits(expect)), merge


@pytest.mark.gpu
def test_subsets_and_refusals(scenes):
    import ctypes as Ct
    from par_raytracer_amd import api, capi
    r, mesh = scenes("cornell_box")
    p, idx, runs = mesh
    lib = capi.hip_lib()
    pts = np.ascontiguousarray(recipe(mesh, "cornell_box")[0][:512])
    group, vertex0 = forward(r, pts)
    n = len(group)
    g = G.random_grads(n, 71)
    full = backward(r, pts, group, vertex0, p, g, torch_path=False)
    for want in (("positions",), ("points",), ()):
        for torch_path in (False, True):
            res = backward(r, pts, group, vertex0, p, g, torch_path, want=want)
            assert set(res) == set(want) | {"info"} and res["info"].hit_rays == full["info"].hit_rays
            for k in want:
                assert np.array_equal(bits(res[k]), bits(full[k])), (want, k)
    # refusals: -1, and the sentinel-filled outputs stay untouched
    batch = capi.PrtPointBatch(pts.ctypes.data, None, n)
    gout = capi.PrtClosestGrads(g["dist2"].ctypes.data, g["point"].ctypes.data, g["bw"].ctypes.data)
    outs = [np.full((p.shape[0], 3), 7.5, np.float32), np.full((n, 3), 7.5, np.float32)]
    gin = capi.PrtPointGrads(*[a.ctypes.data for a in outs])
    info = capi.PrtGradInfo()

    def call(grp, v0, ctx=None, count=None):
        return lib.prt_closest_points_backward(ctx or r._ctx, Ct.byref(batch), grp.ctypes.data, v0.ctypes.data, p.ctypes.data,
                                               p.shape[0] if count is None else count, Ct.byref(gout), Ct.byref(gin), Ct.byref(info))
    for g_bad, v_bad in ((runs.shape[0], 0), (int(group[5]), 1), (int(group[5]), int(runs[group[5], 1])), (int(group[5]), 0xFFFFFFFC)):
        g2, v2 = group.copy(), vertex0.copy()
        g2[5], v2[5] = g_bad, v_bad
        assert call(g2, v2) == -1
        assert all(np.all(a == 7.5) for a in outs)
    assert call(group, vertex0, count=p.shape[0] + 1) == -1 and all(np.all(a == 7.5) for a in outs)
    r2 = api.Renderer(0)
    assert call(group, vertex0, ctx=r2._ctx) == -2                # no scene
    r2.close()
    assert all(np.all(a == 7.5) for a in outs)
    assert call(group, vertex0) == 0 and np.array_equal(bits(outs[0]), bits(full["positions"])) and np.array_equal(bits(outs[1]), bits(full["points"]))
    empty = capi.PrtPointBatch(None, None, 0)                     # count = 0: a zero vertex gradient
    assert lib.prt_closest_points_backward(r._ctx, Ct.byref(empty), None, None, None, p.shape[0], None, Ct.byref(gin), Ct.byref(info)) == 0
    assert np.all(bits(outs[0]) == 0) and info.hit_rays == 0


@pytest.mark.gpu
def test_a_moved_scene(harness):
    from par_raytracer_amd import api
    name = "icosphere_l3"
    r = api.Renderer(0)                                           # its own context: the scene is moved
    r.upload(host_scene(name, 0))
    p, idx, runs = G.scene_mesh(name)
    moved = np.ascontiguousarray(p + np.random.default_rng(80).uniform(-0.02, 0.02, p.shape).astype(np.float32))
    r.update_geometry(moved)
    mesh = (moved, idx, runs)
    pts = recipe(mesh, name)[0]
    group, vertex0 = forward(r, pts)
    g = G.random_grads(N, 82)
    new = backward(r, pts, group, vertex0, moved, g, torch_path=True)
    old = backward(r, pts, group, vertex0, p, g, torch_path=True)
    r.close()
    same_as_harness(new, harness([G.case(mesh, pts, group, vertex0, g)])[0])
    assert not np.array_equal(bits(new["positions"]), bits(old["positions"]))


# Ten steps of plain gradient descent, vertices <- vertices - STEP * d(mean dist2)/d(vertices).  d(mean dist2)/d(vertex) =
# (2 / n) * sum over the points of bw * (q - p): with STEP = n / 8 a vertex moves by a quarter of its points' weighted residuals,
# well inside the step 1 / (2 * sum of weights / n) at which a vertex's own quadratic stops contracting.  Chosen on the CPU first:
# with the float64 yardstick's gradient and the brute-force forward the loss went 0.0485, 0.0309, 0.0183, 0.0113, 0.0072, 0.0047,
# 0.0032, 0.0022, 0.0016, 0.0011, 0.0008 (STEP = n / 32 also falls at every step, four times slower).
DESCENT_STEP_OVER_N = 1.0 / 8.0


@pytest.mark.gpu
def test_autograd_equals_the_direct_call_and_descends(scenes):
    import torch
    from par_raytracer_amd import api
    from par_raytracer_amd.autograd import closest_points_differentiable
    r, mesh = scenes("icosphere_l3")
    pts, kind = recipe(mesh, "icosphere_l3")
    g = G.random_grads(N, 91, ("dist2", "bw"))
    tq, tp = (torch.from_numpy(a).cuda().requires_grad_(True) for a in (pts, mesh[0]))
    d2, q, bw, grp, v0 = closest_points_differentiable(r, tp, tq)
    assert not grp.requires_grad and not v0.requires_grad and d2.requires_grad and q.requires_grad and bw.requires_grad
    loss = (d2 * torch.from_numpy(g["dist2"]).cuda()).sum() + (bw * torch.from_numpy(g["bw"]).cuda()).sum()
    got = torch.autograd.grad(loss, (tp, tq))
    direct = backward(r, pts, grp.cpu().numpy(), v0.cpu().numpy().view(np.uint32), mesh[0], g, torch_path=True)
    for k, x in zip(G.GRADS, got):
        assert np.array_equal(bits(x.cpu().numpy()), bits(direct[k])), k
    (only_points,) = torch.autograd.grad((closest_points_differentiable(r, tp.detach(), tq, update_geometry=False)[0]).sum(), (tq,))
    assert np.array_equal(bits(only_points.cpu().numpy()), bits(backward(r, pts, grp.cpu().numpy(), v0.cpu().numpy().view(np.uint32), mesh[0],
                                                                          dict(dist2=np.ones(N, np.float32)), True, want=("points",))["points"]))
    # descent, on a context of its own: the scene is moved
    rd = api.Renderer(0)
    rd.upload(host_scene("icosphere_l3", 0))
    target = torch.from_numpy(np.ascontiguousarray(pts[kind == C.KIND_ON])).cuda()
    n = target.shape[0]
    P = torch.from_numpy(np.ascontiguousarray(mesh[0] * np.float32(1.1))).cuda().requires_grad_(True)
    losses = []
    for step in range(11):
        loss = closest_points_differentiable(rd, P, target)[0].mean()
        losses.append(float(loss))
        (gp,) = torch.autograd.grad(loss, (P,))
        P = (P.detach() - gp * (DESCENT_STEP_OVER_N * n)).requires_grad_(True)
    rd.close()
    print("n %d, losses %s" % (n, ["%.4g" % x for x in losses]))
    assert n == N // 8 and losses[0] > 0 and all(b < a for a, b in zip(losses, losses[1:])), losses


CHILD = r"""
import os, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, "tests")); sys.path.insert(0, os.path.join(%(root)r, "oracle"))
import numpy as np
import closest_grad_cases as G
from conftest import host_scene
from test_gpu_closest_grad import backward, backward_case, forward, recipe, same_as_harness
from par_raytracer_amd import api, capi
lib = capi.hip_lib()
assert os.path.basename(lib._name) == "libprt_hip_bvh8.so" and not (lib.prt_build_flags() & capi.BUILD_BVH4)
mesh = G.scene_mesh("cornell_box")
r = api.Renderer(0)
r.upload(host_scene("cornell_box", 0))
pts = recipe(mesh, "cornell_box")[0]
group, vertex0 = forward(r, pts)
g = G.random_grads(len(group), 41)
exe = G.build_harness(%(tmp)r, sanitize=False)
h = G.run_harness(exe, [G.case(mesh, pts, group, vertex0, g)], %(tmp)r)[0]
for torch_path in (False, True):
    same_as_harness(backward(r, pts, group, vertex0, mesh[0], g, torch_path), h)
c = G.wave_layout_case(mesh, 200, False)                      # the mixed waves: the gradient kernels read nothing of the tree
h = G.run_harness(exe, [c], %(tmp)r)[0]
res = backward_case(r, c, True)
same_as_harness(res, h)
assert np.array_equal(G.bits(res["positions"]), G.bits(G.exact_integer_sum(mesh, c, h)))
r.close()
print("bvh8 closest gradients ok")
"""


@pytest.mark.gpu
def test_closest_gradients_on_the_8_wide_library(tmp_path):
    assert os.path.exists(os.path.join(ROOT, "par_raytracer_amd", "libprt_hip_bvh8.so")), "libprt_hip_bvh8.so not built (make hip-bvh8)"
    env = dict(os.environ)
    env["PRT_HIP_LIB"] = "libprt_hip_bvh8.so"
    out = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "tmp": str(tmp_path)}], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         timeout=600)
    assert out.returncode == 0 and b"bvh8 closest gradients ok" in out.stdout, (out.returncode, out.stdout.decode()[-1500:],
                                                                               out.stderr.decode()[-3000:])
