"""prt_trace_rays_backward on the GPU: the device's bits against the host harness's (tests/query_grad_host_harness.cpp runs the same
kernels lane by lane), the accuracy yardstick (torch CPU autograd in float64, tests/query_grad_cases.py), independence of ray order
and of the run, subsets and refusals, a moved scene, torch autograd through par_raytracer_amd.autograd, and the 8-wide library.
Those tests feed the forward call's own (group, vertex0) to the backward call.  The tests of mixed waves, of batches past one pass of
the capped grid and of the fixed point's extremes take the cases of tests/query_grad_cases.py, which carry their own references."""
from __future__ import annotations

import os
import subprocess
import sys

import numpy as np
import pytest

import query_grad_cases as Q
from conftest import ROOT, camera_and_params, host_scene, load_golden
from query_grad_cases import bits

N = 2048


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("query_grad_gpu")
    exe = Q.build_harness(d, sanitize=False)
    return lambda cases: Q.run_harness(exe, cases, d)


@pytest.fixture(scope="module")
def scenes():
    """name -> (Renderer, mesh), uploaded once."""
    from par_raytracer_amd import api
    out = {}

    def get(name):
        if name not in out:
            r = api.Renderer(0)
            if name in ("one_triangle", "quad"):
                mesh = Q.one_triangle() if name == "one_triangle" else Q.quad()
                desc = Q.flat_desc(mesh)
                r.upload(desc)
            else:
                mesh = Q.scene_mesh(name)
                r.upload(host_scene(name, 0))
            out[name] = (r, mesh)
        return out[name]
    yield get
    for r, _ in out.values():
        r.close()


def forward(r, mesh, n, seed):
    """Recipe rays traced by the library; returns o, d, group, vertex0 (the forward call's own) of the rays kept: hits whose
    -dot(d, normal) is at least 0.05.  Fails if that drops more than 10 %."""
    o, d, _, _ = Q.recipe_rays(mesh, n, seed)
    res = r.trace_rays(o, d, ray_bias=0.0)
    keep = (res["group"] >= 0) & (-(d * res["normal"]).sum(1) >= 0.05)
    assert keep.sum() >= 0.9 * n, "%d of %d recipe rays dropped" % (n - keep.sum(), n)
    if n in (1, 64, 65):
        assert keep.all()
    k = np.nonzero(keep)[0]
    return (np.ascontiguousarray(o[k]), np.ascontiguousarray(d[k]), np.ascontiguousarray(res["group"][k]), np.ascontiguousarray(res["vertex0"][k]))


def backward(r, o, d, group, vertex0, p, ray_bias, g, torch_path, want=Q.GRADS):
    kw = dict(ray_bias=ray_bias, want=want)
    if torch_path:
        import torch
        cv = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
        res = r.trace_rays_backward(cv(o), cv(d), cv(group), cv(vertex0.view(np.int32)), cv(p), grad_t=cv(g.get("t")), grad_bw=cv(g.get("bw")),
                                    grad_position=cv(g.get("position")), grad_normal=cv(g.get("normal")), **kw)
        return {k: (v.cpu().numpy() if k != "info" else v) for k, v in res.items()}
    return r.trace_rays_backward(o, d, group, vertex0, p, grad_t=g.get("t"), grad_bw=g.get("bw"), grad_position=g.get("position"),
                                 grad_normal=g.get("normal"), **kw)


def same_as_harness(res, h):
    assert h["rc"] == 0
    for k in Q.GRADS:
        assert np.array_equal(bits(res[k]), bits(h[k])), k
    info = res["info"]
    assert (info.hit_rays, info.skipped_rays, info.unit_exponent) == (h["hit_rays"], h["skipped_rays"], h["unit_exponent"])
    assert bits(np.float32(info.max_contribution)) == bits(h["max_contribution"])


@pytest.mark.gpu
@pytest.mark.parametrize("name,n", [("one_triangle", 1), ("one_triangle", 64), ("one_triangle", 65), ("cornell_box", N), ("icosphere_l3", N)])
def test_device_bits_equal_the_host_harness(scenes, harness, name, n):
    r, mesh = scenes(name)
    o, d, group, vertex0 = forward(r, mesh, n, seed=40 + n)
    g = Q.random_grads(len(group), 41)
    h = harness([Q.case(mesh, o, d, group, vertex0, 1e-3, g)])[0]
    for torch_path in (False, True):
        same_as_harness(backward(r, o, d, group, vertex0, mesh[0], 1e-3, g, torch_path), h)


@pytest.mark.gpu
def test_yardstick_on_the_icosphere(scenes):
    r, mesh = scenes("icosphere_l3")
    o, d, group, vertex0 = forward(r, mesh, N, seed=50)
    g = Q.random_grads(len(group), 51)
    res = backward(r, o, d, group, vertex0, mesh[0], 0.0, g, torch_path=True)
    assert res["info"].hit_rays == len(group) and res["info"].skipped_rays == 0
    Q.check_against_yardstick(mesh, o, d, group, vertex0, 0.0, g, res, "icosphere_l3 on the device")


@pytest.mark.gpu
def test_the_same_bits_twice_and_for_a_permuted_batch(scenes):
    r, mesh = scenes("icosphere_l3")
    o, d, group, vertex0 = forward(r, mesh, N, seed=60)
    g = Q.random_grads(len(group), 61)
    first = backward(r, o, d, group, vertex0, mesh[0], 1e-3, g, torch_path=True)
    again = backward(r, o, d, group, vertex0, mesh[0], 1e-3, g, torch_path=True)
    p = np.random.default_rng(62).permutation(len(group))
    perm = backward(r, o[p], d[p], group[p], vertex0[p], mesh[0], 1e-3, {k: v[p] for k, v in g.items()}, torch_path=True)
    assert np.abs(first["positions"]).max() > 0
    for k in Q.GRADS:
        assert np.array_equal(bits(first[k]), bits(again[k])), k
    assert np.array_equal(bits(first["positions"]), bits(perm["positions"]))
    assert np.array_equal(bits(first["origins"][p]), bits(perm["origins"])) and np.array_equal(bits(first["directions"][p]), bits(perm["directions"]))
    for merge in (0, 1):                                  # both forms of the scatter kernel
        r.set_option("QGRAD_MERGE", merge)
        res = backward(r, o, d, group, vertex0, mesh[0], 1e-3, g, torch_path=True)
        for k in Q.GRADS:
            assert np.array_equal(bits(first[k]), bits(res[k])), (k, merge)
    r.set_option("QGRAD_MERGE", None)


@pytest.mark.gpu
def test_subsets_and_refusals(scenes):
    import ctypes as C
    from par_raytracer_amd import api, capi
    r, mesh = scenes("cornell_box")
    p, idx, runs = mesh
    lib = capi.hip_lib()
    o, d, group, vertex0 = forward(r, mesh, 512, seed=70)
    n = len(group)
    g = Q.random_grads(n, 71)
    full = backward(r, o, d, group, vertex0, p, 0.0, g, torch_path=False)
    for want in (("positions",), ("origins",), ("directions",), ("origins", "positions")):
        for torch_path in (False, True):
            res = backward(r, o, d, group, vertex0, p, 0.0, g, torch_path, want=want)
            assert set(res) == set(want) | {"info"}
            for k in want:
                assert np.array_equal(bits(res[k]), bits(full[k])), (want, k)
    # refusals: -1, and the sentinel-filled outputs stay untouched
    batch = capi.PrtRayBatch(o.ctypes.data, d.ctypes.data, None, n, 0.0)
    gout = capi.PrtHitGrads(g["t"].ctypes.data, g["bw"].ctypes.data, g["position"].ctypes.data, g["normal"].ctypes.data)
    outs = [np.full((p.shape[0], 3), 7.5, np.float32), np.full((n, 3), 7.5, np.float32), np.full((n, 3), 7.5, np.float32)]
    gin = capi.PrtQueryGrads(*[a.ctypes.data for a in outs])
    info = capi.PrtGradInfo()

    def call(grp, v0, ctx=None, count=None):
        return lib.prt_trace_rays_backward(ctx or r._ctx, C.byref(batch), grp.ctypes.data, v0.ctypes.data, p.ctypes.data,
                                           p.shape[0] if count is None else count, C.byref(gout), C.byref(gin), C.byref(info))
    for g_bad, v_bad in ((runs.shape[0], 0), (int(group[5]), 1), (int(group[5]), int(runs[group[5], 1]))):
        g2, v2 = group.copy(), vertex0.copy()
        g2[5], v2[5] = g_bad, v_bad
        assert call(g2, v2) == -1
        assert all(np.all(a == 7.5) for a in outs)
    assert call(group, vertex0, count=p.shape[0] + 1) == -1 and all(np.all(a == 7.5) for a in outs)
    r2 = api.Renderer(0)
    assert call(group, vertex0, ctx=r2._ctx) == -2                # no scene
    r2.close()
    assert all(np.all(a == 7.5) for a in outs)
    assert call(group, vertex0) == 0 and np.array_equal(bits(outs[0]), bits(full["positions"]))
    empty = capi.PrtRayBatch(None, None, None, 0, 0.0)            # count = 0: a zero vertex gradient
    assert lib.prt_trace_rays_backward(r._ctx, C.byref(empty), None, None, None, p.shape[0], None, C.byref(gin), C.byref(info)) == 0
    assert np.all(bits(outs[0]) == 0) and info.hit_rays == 0


@pytest.mark.gpu
def test_a_moved_scene_and_renders_left_alone():
    from par_raytracer_amd import api, capi
    gold = load_golden("c2_cornell_128")
    name = str(gold["scene"])
    r = api.Renderer(0)                                           # its own context: the scene is moved
    r.upload(host_scene(name, 0))
    p, idx, runs = Q.scene_mesh(name)
    rng = np.random.default_rng(80)
    moved = np.ascontiguousarray(p + rng.uniform(-0.02, 0.02, p.shape).astype(np.float32))
    r.update_geometry(moved)
    mesh = (moved, idx, runs)
    cam, prm = camera_and_params(gold, capi.PIPELINE_WAVEFRONT)
    w, h = int(gold["width"]), int(gold["height"])
    before, c0 = r.render(cam, prm, w, h)
    o, d, group, vertex0 = forward(r, mesh, N, seed=81)
    g = Q.random_grads(len(group), 82)
    res = backward(r, o, d, group, vertex0, moved, 0.0, g, torch_path=True)
    after, c1 = r.render(cam, prm, w, h)
    r.close()
    assert np.array_equal(before.view(np.uint32), after.view(np.uint32)) and c0.ray_count == c1.ray_count
    Q.check_against_yardstick(mesh, o, d, group, vertex0, 0.0, g, res, "moved %s" % name)


@pytest.mark.gpu
def test_autograd_equals_the_direct_call_and_descends(scenes):
    import torch
    from par_raytracer_amd.autograd import trace_rays_differentiable
    r, mesh = scenes("icosphere_l3")
    o, d, group, vertex0 = forward(r, mesh, N, seed=90)
    g = Q.random_grads(len(group), 91, ("t", "normal"))
    to, td, tp = (torch.from_numpy(a).cuda().requires_grad_(True) for a in (o, d, mesh[0]))
    t, bw, pos, nrm, grp, v0 = trace_rays_differentiable(r, tp, to, td, ray_bias=1e-3)
    assert not grp.requires_grad and not v0.requires_grad and t.requires_grad and nrm.requires_grad
    loss = (t * torch.from_numpy(g["t"]).cuda()).sum() + (nrm * torch.from_numpy(g["normal"]).cuda()).sum()
    got = torch.autograd.grad(loss, (tp, to, td))
    direct = backward(r, o, d, grp.cpu().numpy(), v0.cpu().numpy().view(np.uint32), mesh[0], 1e-3, g, torch_path=True)
    for k, x in zip(Q.GRADS, got):
        assert np.array_equal(bits(x.cpu().numpy()), bits(direct[k])), k
    # descent: a quad facing a 16 x 16 grid of parallel rays; loss = sum((t - target)^2); step 1 / (2 * rays) - a rigid shift
    # along the normal changes every t equally, so plain gradient descent on the vertices is a contraction
    rq, quad = scenes("quad")
    xs = (np.arange(16, dtype=np.float32) + 0.5) / 8 - 1
    grid = np.stack(np.meshgrid(xs * 0.9, xs * 0.8 + 0.013, indexing="ij"), -1).reshape(-1, 2).astype(np.float32)   # no ray on the diagonal edge
    qo = torch.from_numpy(np.concatenate([grid, np.full((256, 1), 2.0, np.float32)], 1)).cuda()
    qd = torch.tensor([[0.0, 0.0, -1.0]], device="cuda").repeat(256, 1).contiguous()
    P = torch.from_numpy(quad[0]).cuda().requires_grad_(True)
    target, losses = 1.5, []
    for step in range(11):
        t = trace_rays_differentiable(rq, P, qo, qd)[0]
        loss = ((t - target) ** 2).sum()
        losses.append(float(loss))
        (gp,) = torch.autograd.grad(loss, (P,))
        P = (P.detach() - gp / (2 * 256)).requires_grad_(True)
    assert losses[0] > 0 and all(b < a for a, b in zip(losses, losses[1:])), losses
    rq.update_geometry(quad[0])                                   # leave the cached scene as it was uploaded


# ---- mixed waves, batches past one pass of the capped grid, the fixed point's extremes.  The backward call does not trace: the
# cases of tests/query_grad_cases.py carry their own references and are the ones tests/test_query_grad_host.py proves on the CPU.

def backward_case(r, c, torch_path, merge=None):
    r.set_option("QGRAD_MERGE", merge)
    try:
        return backward(r, c["o"], c["d"], c["group"], c["vertex0"], c["mesh"][0], c["ray_bias"], c["gout"], torch_path)
    finally:
        r.set_option("QGRAD_MERGE", None)


def backward_with_live_rows_behind(r, c, merge):
    """The device entry point on tensors that are the first `count` rows of longer ones, whose next 64 rows hold contributing rays
    of the same batch: a lane at or past `count` that was not held back would read a live ray there and add it."""
    import torch
    n = len(c["group"])
    live = np.nonzero(c["contributing"])[0][:64]
    assert live.size == 64 and n % 64 != 0
    cv = lambda a: torch.from_numpy(np.ascontiguousarray(np.concatenate([a, a[live]]))).cuda()[:n]      # noqa: E731
    g = c["gout"]
    r.set_option("QGRAD_MERGE", merge)
    try:
        res = r.trace_rays_backward(cv(c["o"]), cv(c["d"]), cv(c["group"]), cv(c["vertex0"].view(np.int32)),
                                    torch.from_numpy(c["mesh"][0]).cuda(), ray_bias=c["ray_bias"], grad_t=cv(g["t"]), grad_bw=cv(g["bw"]),
                                    grad_position=cv(g["position"]), grad_normal=cv(g["normal"]))
    finally:
        r.set_option("QGRAD_MERGE", None)
    return {k: (v.cpu().numpy() if k != "info" else v) for k, v in res.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell_box", "icosphere_l3"])
def test_mixed_waves_equal_the_host_harness(scenes, harness, name):
    r, mesh = scenes(name)
    c = Q.wave_layout_case(mesh, 200, False)
    h = harness([c])[0]
    expect = Q.exact_integer_sum(mesh, c, h)
    assert (h["hit_rays"], h["skipped_rays"]) == (c["hit_rays"], c["skipped_rays"])
    for merge in (0, 1):
        for torch_path in (False, True):
            res = backward_case(r, c, torch_path, merge)
            same_as_harness(res, h)
            assert (res["info"].hit_rays, res["info"].skipped_rays) == (c["hit_rays"], c["skipped_rays"]), (merge, torch_path)
            assert np.array_equal(bits(res["positions"]), bits(expect)), (merge, torch_path)
            assert np.all(bits(res["origins"][~c["contributing"]]) == 0) and np.all(bits(res["directions"][~c["contributing"]]) == 0)
        same_as_harness(backward_with_live_rows_behind(r, c, merge), h)


@pytest.mark.gpu
def test_batches_past_one_grid_pass(scenes, harness):
    """grad_backward caps the grid at 8 * cu_count blocks of 256: this batch is two full passes of it, three waves and 37 lanes."""
    import time
    import torch
    # The context's own cu_count is not exported.  It starts as hipGetDeviceProperties' multiProcessorCount - the figure torch
    # reports - and PRT_RESERVE_CUS can only lower it, which makes a pass shorter: the second pass is reached either way.
    assert not os.environ.get("PRT_RESERVE_CUS")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    count = 2 * 8 * cus * 256 + 3 * 64 + 37
    assert count > 8 * cus * 256 and count % 64 == 37
    r, mesh = scenes("cornell_box")
    t0 = time.perf_counter()
    o, d, group, vertex0 = Q.recipe_rays(mesh, count, 600)
    rand = Q.case(mesh, o, d, group, vertex0, 1e-3, Q.random_grads(count, 601))
    rep = Q.repeated_ray_case(mesh, count)
    h_rand, h_rep = harness([rand, rep])
    t1 = time.perf_counter()
    assert h_rand["hit_rays"] == count and h_rep["hit_rays"] == count
    expect_rand = Q.exact_integer_sum(mesh, rand, h_rand)
    expect_rep, top_bits = Q.repeated_ray_expectation(mesh, rep, h_rep)
    first = None
    for merge in (0, 1):
        res = backward_case(r, rand, True, merge)
        same_as_harness(res, h_rand)
        assert np.array_equal(bits(res["positions"]), bits(expect_rand)), merge
        first = res
        res = backward_case(r, rep, True, merge)              # merge 0: every ray's 9 adds land on the same 9 words
        same_as_harness(res, h_rep)
        assert np.array_equal(bits(res["positions"]), bits(expect_rep)), merge
    same_as_harness(backward_case(r, rand, False), h_rand)    # the host entry point
    p = np.random.default_rng(602).permutation(count)
    perm = backward_case(r, Q.case(mesh, o[p], d[p], group[p], vertex0[p], 1e-3, {k: v[p] for k, v in rand["gout"].items()}), True)
    assert np.array_equal(bits(perm["positions"]), bits(first["positions"]))
    assert np.array_equal(bits(perm["origins"]), bits(first["origins"][p]))
    t2 = time.perf_counter()
    print("CUs %d, count %d, the repeated ray's largest accumulator has %d bits; cases and harness %.2f s, device calls and checks %.2f s"
          % (cus, count, top_bits, t1 - t0, t2 - t1))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell_box", "icosphere_l3"])
def test_fixed_point_extremes_on_the_device(scenes, harness, name):
    r, mesh = scenes(name)
    cases = [Q.scaled_grads_case(mesh, e) for e in Q.SCALED_EXPONENTS]
    n = Q.LAYOUT_RAYS
    for e, c, h in zip(Q.SCALED_EXPONENTS, cases, harness(cases)):
        m = float(h["max_contribution"])
        print("%s 2^%d: M %.3g, unit exponent %d, hit %d, skipped %d" % (name, e, m, h["unit_exponent"], h["hit_rays"], h["skipped_rays"]))
        # the regimes, from the harness: a denormal M, a positive unit exponent, a batch skipped in part, a sum that is +-inf
        if e == -140:
            assert 0 < m < 2.0 ** -126 and h["skipped_rays"] == 0 and np.abs(h["positions"]).max() > 0
        if e == 100:
            assert h["unit_exponent"] > 0
        if (e, name) in ((122, "icosphere_l3"), (124, "cornell_box")):
            assert 0 < h["skipped_rays"] < n
        if (e, name) == (124, "cornell_box"):
            assert np.isinf(h["positions"]).any()
        expect = Q.exact_integer_sum(mesh, c, h)
        for merge in (0, 1):
            for torch_path in (False, True):
                res = backward_case(r, c, torch_path, merge)
                same_as_harness(res, h)
                assert np.array_equal(bits(res["positions"]), bits(expect)), (e, merge, torch_path)


CHILD = r"""
import os, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, "tests")); sys.path.insert(0, os.path.join(%(root)r, "oracle"))
import numpy as np
import query_grad_cases as Q
from conftest import host_scene
from test_gpu_query_grad import N, backward, forward, same_as_harness
from par_raytracer_amd import api, capi
lib = capi.hip_lib()
assert os.path.basename(lib._name) == "libprt_hip_bvh8.so" and not (lib.prt_build_flags() & capi.BUILD_BVH4)
mesh = Q.scene_mesh("cornell_box")
r = api.Renderer(0)
r.upload(host_scene("cornell_box", 0))
o, d, group, vertex0 = forward(r, mesh, N, seed=40 + N)
g = Q.random_grads(len(group), 41)
exe = Q.build_harness(%(tmp)r, sanitize=False)
h = Q.run_harness(exe, [Q.case(mesh, o, d, group, vertex0, 1e-3, g)], %(tmp)r)[0]
for torch_path in (False, True):
    same_as_harness(backward(r, o, d, group, vertex0, mesh[0], 1e-3, g, torch_path), h)
c = Q.wave_layout_case(mesh, 200, False)                      # the mixed waves: the gradient kernels read nothing of the tree
h = Q.run_harness(exe, [c], %(tmp)r)[0]
res = backward(r, c["o"], c["d"], c["group"], c["vertex0"], mesh[0], c["ray_bias"], c["gout"], True)
same_as_harness(res, h)
assert (res["info"].hit_rays, res["info"].skipped_rays) == (c["hit_rays"], c["skipped_rays"])
assert np.array_equal(Q.bits(res["positions"]), Q.bits(Q.exact_integer_sum(mesh, c, h)))
r.close()
print("bvh8 query gradients ok")
"""


@pytest.mark.gpu
def test_query_gradients_on_the_8_wide_library(tmp_path):
    if not os.path.exists(os.path.join(ROOT, "par_raytracer_amd", "libprt_hip_bvh8.so")):
        pytest.skip("libprt_hip_bvh8.so not built (make hip-bvh8)")
    env = dict(os.environ)
    env["PRT_HIP_LIB"] = "libprt_hip_bvh8.so"
    out = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "tmp": str(tmp_path)}], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         timeout=600)
    assert out.returncode == 0 and b"bvh8 query gradients ok" in out.stdout, (out.returncode, out.stdout.decode()[-1500:],
                                                                             out.stderr.decode()[-3000:])
