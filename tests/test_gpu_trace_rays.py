"""prt_trace_rays on the GPU against the CPU oracle's own TraceRay (tests/golden/trace_*.npz, tests/trace_golden.py):
every hit field bit for bit in CLOSEST mode, near ties included, and OCCLUDED with and without tmax - through the host entry
point (numpy) and the device entry point (torch tensors), on the SAH tree, the LBVH tree and the 8-wide library; plus the edges of
the call (field subsets, empty batches, invalid rays, errors) and the promise that a query leaves renders alone."""
from __future__ import annotations

import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, camera_and_params, host_scene, load_golden

SCENES = ["cornell_box", "coincident", "icosphere_l3", "terrain_1m"]
CLOSEST = ("t", "bw", "vertex0", "group", "position", "normal")
FLT_MAX = np.float32(3.4028234663852886e38)


def _fixture(name):
    return np.load(os.path.join(GOLDEN, "trace_%s.npz" % name), allow_pickle=False)


def _bits(a):
    """The array's bits, every NaN as one pattern: which NaN an invalid operation gives is the hardware's choice (the oracle's CPU
    raises the negative one, the GPU the positive one), and TraceRay's barycentrics are NaN where its triangle test overflows."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.float32:
        return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))
    return a.view(np.uint32) if a.dtype == np.int32 else a


def check_fixture(r, g, torch_path: bool, count_visits: bool = False):
    """Every ray of fixture g (or of a case of tests/trace_cases.py, as_fixture) through Renderer r, one call per distinct
    ray_bias; returns the number of rays compared.  count_visits: the calls run the counting instantiations of the kernels."""
    if torch_path:
        import torch
        dev = torch.device("cuda", r.device_id)
        conv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)       # noqa: E731
        back = lambda t: t.cpu().numpy()                                          # noqa: E731
    else:
        conv = lambda a: np.ascontiguousarray(a)                                  # noqa: E731
        back = lambda a: a                                                        # noqa: E731
    n = 0
    for bias in np.unique(g["ray_bias"]):
        sel = np.nonzero(g["ray_bias"] == bias)[0]
        o, d, tm = conv(g["origins"][sel]), conv(g["directions"][sel]), conv(g["tmax"][sel])
        res = r.trace_rays(o, d, ray_bias=float(bias), count_visits=count_visits)
        assert res["counters"].ray_count == len(sel) and res["counters"].pipeline == 0
        for k in CLOSEST:
            got = back(res[k])
            if k == "vertex0":
                got = got.view(np.uint32)                                          # torch: int32 with the same bits
            exp = g[k][sel]
            bad = np.nonzero(np.any((_bits(got) != _bits(exp)).reshape(len(sel), -1), axis=1))[0]
            assert bad.size == 0, ("%s: field %s differs on %d of %d rays (bias %g), first ray %d: got %r, expected %r, near tie %d" % (
                str(g["scene"]), k, bad.size, len(sel), bias, sel[bad[0]], got[bad[0]], exp[bad[0]], int(g["near_tie"][sel[bad[0]]])))
        occ = back(r.trace_rays(o, d, mode="occluded", ray_bias=float(bias), count_visits=count_visits)["occluded"])
        assert np.array_equal(occ, g["occluded"][sel]), (str(g["scene"]), "occluded", int((occ != g["occluded"][sel]).sum()))
        occ_t = back(r.trace_rays(o, d, mode="occluded", tmax=tm, ray_bias=float(bias), count_visits=count_visits)["occluded"])
        bad = np.nonzero(occ_t != g["occluded_tmax"][sel])[0]
        assert bad.size == 0, [(str(g["scene"]), "occluded below tmax", int(sel[i]), float(g["tmax"][sel[i]]), float(g["t"][sel[i]]),
                                int(occ_t[i]), int(g["occluded_tmax"][sel[i]]), int(g["near_tie"][sel[i]]), float(bias),
                                g["directions"][sel[i]].tolist(), int(g["family"][sel[i]])) for i in bad[:4]]
        n += len(sel)
    return n


@pytest.fixture(scope="module")
def renderers():
    from par_raytracer_amd import api
    out = {}

    def get(name, builder="sah"):
        if (name, builder) not in out:
            out[(name, builder)] = _make(api, name, builder)
        return out[(name, builder)]
    yield get
    for r in out.values():
        r.close()


def _make(api, name, builder):
    r = api.Renderer(0)
    if builder != "sah":
        r.set_option("BVH_BUILDER", builder)
    r.upload(host_scene(name, 0))
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("builder", ["sah", "lbvh"])
def test_queries_equal_the_oracles_trace_ray(renderers, name, builder):
    g = _fixture(name)
    r = renderers(name, builder)
    assert check_fixture(r, g, torch_path=False) == g["origins"].shape[0]
    assert check_fixture(r, g, torch_path=True) == g["origins"].shape[0]


CHILD = r"""
import os, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, "tests")); sys.path.insert(0, os.path.join(%(root)r, "oracle"))
import numpy as np
from conftest import host_scene
from test_gpu_trace_rays import SCENES, _fixture, check_fixture
from par_raytracer_amd import api, capi
lib = capi.hip_lib()
assert os.path.basename(lib._name) == "libprt_hip_bvh8.so" and not (lib.prt_build_flags() & capi.BUILD_BVH4)
for name in SCENES:
    r = api.Renderer(0)
    r.upload(host_scene(name, 0))
    n = check_fixture(r, _fixture(name), torch_path=False)
    n += check_fixture(r, _fixture(name), torch_path=True)
    print(name, n, "rays equal", flush=True)
    r.close()
print("bvh8 queries ok")
"""


@pytest.mark.gpu
def test_queries_on_the_8_wide_library():
    if not os.path.exists(os.path.join(ROOT, "par_raytracer_amd", "libprt_hip_bvh8.so")):
        pytest.skip("libprt_hip_bvh8.so not built (make hip-bvh8)")
    env = dict(os.environ)
    env["PRT_HIP_LIB"] = "libprt_hip_bvh8.so"
    out = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         timeout=900)
    assert out.returncode == 0 and b"bvh8 queries ok" in out.stdout, (out.returncode, out.stdout.decode()[-1500:],
                                                                     out.stderr.decode()[-3000:])


@pytest.mark.gpu
def test_field_subsets_empty_batches_invalid_rays_and_errors(renderers):
    import ctypes as C
    from par_raytracer_amd import api, capi
    g = _fixture("cornell_box")
    r = renderers("cornell_box")
    lib = capi.hip_lib()
    sel = np.nonzero(g["ray_bias"] == 0)[0][:512]
    o, d = np.ascontiguousarray(g["origins"][sel]), np.ascontiguousarray(g["directions"][sel])
    n = len(sel)
    # only t and group requested: the other buffers keep their sentinels
    bufs = {k: np.full((n, 3), 7.5, np.float32) for k in ("bw", "position", "normal")}
    bufs["t"] = np.full(n, 7.5, np.float32)
    bufs["vertex0"] = np.full(n, 12345, np.uint32)
    bufs["group"] = np.full(n, 777, np.int32)
    bufs["occluded"] = np.full(n, 9, np.uint8)
    batch = capi.PrtRayBatch(o.ctypes.data, d.ctypes.data, None, n, 0.0)
    hb = capi.PrtHitBuffers(bufs["t"].ctypes.data, None, None, bufs["group"].ctypes.data, None, None, bufs["occluded"].ctypes.data)
    ctr = capi.PrtCounters()
    assert lib.prt_trace_rays(r._ctx, capi.QUERY_CLOSEST, C.byref(batch), C.byref(hb), 0, C.byref(ctr)) == 0
    assert np.array_equal(_bits(bufs["t"]), _bits(g["t"][sel])) and np.array_equal(bufs["group"], g["group"][sel])
    assert np.all(bufs["bw"] == 7.5) and np.all(bufs["position"] == 7.5) and np.all(bufs["normal"] == 7.5)
    assert np.all(bufs["vertex0"] == 12345) and np.all(bufs["occluded"] == 9)          # CLOSEST does not write occluded
    assert ctr.ray_count == n
    # count = 0 is a no-op
    empty = capi.PrtRayBatch(None, None, None, 0, 0.0)
    assert lib.prt_trace_rays(r._ctx, capi.QUERY_CLOSEST, C.byref(empty), C.byref(hb), 0, C.byref(ctr)) == 0 and ctr.ray_count == 0
    assert lib.prt_trace_rays_device(r._ctx, capi.QUERY_OCCLUDED, C.byref(empty), None, 0, C.byref(ctr)) == 0
    # null origins -> -1, unknown mode -> -1
    bad = capi.PrtRayBatch(None, d.ctypes.data, None, n, 0.0)
    assert lib.prt_trace_rays(r._ctx, capi.QUERY_CLOSEST, C.byref(bad), C.byref(hb), 0, None) == -1
    assert lib.prt_trace_rays(r._ctx, 7, C.byref(batch), C.byref(hb), 0, None) == -1
    # no scene -> -2
    r2 = api.Renderer(0)
    assert lib.prt_trace_rays(r2._ctx, capi.QUERY_CLOSEST, C.byref(batch), C.byref(hb), 0, None) == -2
    r2.close()
    # non-finite and zero-direction rays are misses and leave their neighbours alone
    o2, d2 = o.copy(), d.copy()
    o2[1, 0] = np.nan; d2[3, 2] = np.inf; d2[5] = 0.0; o2[7, 1] = -np.inf
    for torch_path in (False, True):
        if torch_path:
            import torch
            res = r.trace_rays(torch.from_numpy(o2).cuda(), torch.from_numpy(d2).cuda())
            res = {k: (v.cpu().numpy() if k != "counters" else v) for k, v in res.items()}
            occ = r.trace_rays(torch.from_numpy(o2).cuda(), torch.from_numpy(d2).cuda(), mode="occluded")["occluded"].cpu().numpy()
        else:
            res = r.trace_rays(o2, d2)
            occ = r.trace_rays(o2, d2, mode="occluded")["occluded"]
        bad_rays = np.array([1, 3, 5, 7])
        good = np.setdiff1d(np.arange(n), bad_rays)
        assert np.all(res["group"][bad_rays] == -1) and np.all(res["t"][bad_rays] == FLT_MAX) and np.all(occ[bad_rays] == 0)
        assert np.all(res["position"][bad_rays] == 0) and np.all(res["normal"][bad_rays] == 0) and np.all(res["bw"][bad_rays] == 0)
        assert np.array_equal(_bits(res["t"][good]), _bits(g["t"][sel][good]))
        assert np.array_equal(res["group"][good], g["group"][sel][good])
        assert np.array_equal(occ[good], g["occluded"][sel][good])
    # count_visits fills the traversal counters
    ctr = r.trace_rays(o, d, count_visits=True)["counters"]
    assert ctr.node_visits > 0 and ctr.tri_tests > 0 and ctr.render_ms > 0 and ctr.trace_kernel_ms > 0


@pytest.mark.gpu
def test_four_million_rays_closest_and_occluded_agree(renderers):
    """A batch of 4 M rays on the 1M-triangle scene, built on the device: every ray's OCCLUDED (no limit) is its CLOSEST hit's
    existence."""
    import torch
    r = renderers("terrain_1m")
    g = _fixture("terrain_1m")
    n = 1 << 22
    gen = torch.Generator(device="cuda").manual_seed(5)
    p = g["position"][g["group"] >= 0]                       # points on the terrain: its extent
    lo = torch.from_numpy(p.min(0)).cuda()
    hi = torch.from_numpy(p.max(0)).cuda()
    o = lo + (hi - lo) * torch.rand((n, 3), device="cuda", generator=gen)
    o[:, 1] = hi[1] + 5.0                                     # above it
    o = o.contiguous()
    d = torch.randn((n, 3), device="cuda", generator=gen)
    d[:, 1] = -d[:, 1].abs()                                  # mostly downwards, onto the terrain
    d = (d / d.norm(dim=1, keepdim=True)).contiguous()
    res = r.trace_rays(o, d, fields=("t", "group"))
    occ = r.trace_rays(o, d, mode="occluded")["occluded"]
    hit = res["group"] >= 0
    assert res["counters"].ray_count == n
    assert int(hit.sum()) > n // 4
    assert torch.equal(occ.bool(), hit)
    assert torch.equal(hit, res["t"] < float(FLT_MAX))


@pytest.mark.gpu
def test_queries_leave_renders_and_render_stats_alone(renderers):
    from par_raytracer_amd import capi
    gold = load_golden("c2_cornell_128")
    r = renderers(str(gold["scene"]))
    cam, p = camera_and_params(gold, capi.PIPELINE_WAVEFRONT)
    p.pipeline |= capi.FLAG_COUNT_VISITS
    w, h = int(gold["width"]), int(gold["height"])
    before, c0 = r.render(cam, p, w, h)
    s0 = r.render_stats()
    g = _fixture(str(gold["scene"]))
    r.trace_rays(np.ascontiguousarray(g["origins"]), np.ascontiguousarray(g["directions"]), count_visits=True)
    r.trace_rays(np.ascontiguousarray(g["origins"]), np.ascontiguousarray(g["directions"]), mode="occluded", count_visits=True)
    s1 = r.render_stats()
    assert bytes(s0) == bytes(s1)
    after, c1 = r.render(cam, p, w, h)
    assert np.array_equal(before.view(np.uint32), after.view(np.uint32)) and c0.ray_count == c1.ray_count
