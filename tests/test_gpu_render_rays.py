"""prt_render_rays on the GPU (include/prt.h "radiance along the caller's rays").

1. Against tests/radiance_oracle_harness.cpp - the CPU oracle's own TraceRayColor along the same rays: RGB within the parity
   tolerance, ray_count and shaded_hits equal, for 1..257 outputs x 1, 3, 8 rays, both entry points, two values of `first`.
2. Composition: RenderPixel's rays with PRT_RAYS_CAMERA_STREAM and first = p0 are prt_render's pixels bit for bit, on both of
   its pipelines.
3. Purity: the same bits for every split of a batch, CHAINS, PASS_SAMPLES, STACK_CAP, builder, SHADOW_TREES, tree width, after
   update_geometry, and for origins beyond the shadow trees' guard.
4. Refusals: code, text, and an output buffer nobody touched.

Scenes: cornell_box, many_materials (translucent: the general RNG), coincident (near ties: k_trace_exact) and textured_gallery
(alpha maps).  tests/test_radiance_host.py proves the yardstick and that the batches are mixed."""
from __future__ import annotations

import ctypes as C
import hashlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import radiance_cases as R
from conftest import ROOT, host_scene, scene_dir

COUNTS = (1, 63, 64, 65, 257)
SPPS = (1, 3, 8)                           # launch_resolve: k_resolve for 1 and 3, k_resolve_pow2 for 8
SEED = 5


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def params_for(spp, **kw):
    from par_raytracer_amd import api
    return api.default_params(spp, SEED, **kw)


def call(r, o, d, params, first=0, camera_stream=False, torch_path=False):
    """One render_rays call; (rgba as numpy, counters)."""
    if torch_path:
        import torch
        rgba, ctr = r.render_rays(torch.from_numpy(np.ascontiguousarray(o)).to("cuda:0"), torch.from_numpy(np.ascontiguousarray(d)).to("cuda:0"),
                                  params, first=first, camera_stream=camera_stream)
        assert rgba.device.type == "cuda" and tuple(rgba.shape) == (o.shape[0], 4)
        return rgba.cpu().numpy(), ctr
    rgba, ctr = r.render_rays(np.ascontiguousarray(o), np.ascontiguousarray(d), params, first=first, camera_stream=camera_stream)
    return rgba, ctr


_RAYS = {}


def scene_rays(name):
    """(arrays, origins, directions) of the scene's fixture batch: 257 outputs x 8 rays; fewer of either are its leading part."""
    if name not in _RAYS:
        arrays = host_scene(name).arrays()
        o, d, _ = R.make_rays(arrays, 257, 8, R.SEEDS[name])
        _RAYS[name] = (arrays, o, d)
    return _RAYS[name]


_EXPECT = {}


def expected(name, spp, first):
    """The harness's answers for the scene's 257 x spp batch (computed once; output i of a shorter batch is output i of this)."""
    key = (name, spp, first)
    if key not in _EXPECT:
        _, o, d = scene_rays(name)
        o, d = o[:, :spp], d[:, :spp]
        exp = R.oracle_batch(host_scene(name).desc, params_for(spp), o, d, first=first)
        _EXPECT[key] = exp
    return _EXPECT[key]


# ---- 1. against the harness

@pytest.mark.gpu
@pytest.mark.parametrize("name", R.SCENES)
def test_radiance_against_the_harness(gpu_renderer_factory, name, capsys):
    from par_raytracer_amd import capi
    r = gpu_renderer_factory(name)
    _, o, d = scene_rays(name)
    worst = 0.0
    for spp in SPPS:
        p = params_for(spp)
        for first, counts in ((5, COUNTS), (2 ** 32 - 257, (257,))):
            exp = expected(name, spp, first)
            for n in counts:
                for torch_path in (False, True):
                    rgba, ctr = call(r, o[:n, :spp], d[:n, :spp], p, first=first, torch_path=torch_path)
                    what = "%s: %d x %d, first %d, %s" % (name, n, spp, first, "torch" if torch_path else "numpy")
                    diff = float(np.abs(rgba[:, :3] - exp["rgba"][:n, :3]).max())
                    worst = max(worst, diff)
                    assert diff <= R.TOL, (what, diff)
                    assert np.all(rgba[:, 3] == 1.0), what
                    assert ctr.ray_count == int(exp["rays_per_output"][:n].sum()), (what, ctr.ray_count)
                    assert ctr.shaded_hits == int(exp["shaded_per_output"][:n].sum()), (what, ctr.shaded_hits)
                    assert ctr.pipeline == capi.PIPELINE_WAVEFRONT and ctr.render_ms > 0 and ctr.trace_kernel_launches > 0, what
    # counted renders give the same image and counters, plus visits; PRT_FLAG_TRYOUT is ignored
    p = params_for(3)
    plain, c0 = call(r, o[:, :3], d[:, :3], p, first=5)
    counted, c1 = call(r, o[:, :3], d[:, :3], params_for(3, pipeline=capi.PIPELINE_WAVEFRONT | capi.FLAG_COUNT_VISITS | capi.FLAG_TRYOUT), first=5)
    assert np.array_equal(bits(plain), bits(counted)) and c0.ray_count == c1.ray_count and c0.shaded_hits == c1.shaded_hits > 0
    assert c1.node_visits > 0 and c1.tri_tests > 0 and c0.node_visits == 0
    assert r.render_stats().stack_bound > 0
    with capsys.disabled():
        print("\n[render_rays] %s: largest |dRGB| against the harness %.3g" % (name, worst))


# ---- 2. composition with prt_render

@pytest.mark.gpu
@pytest.mark.parametrize("name", R.SCENES)
def test_camera_rays_compose_to_prt_render(gpu_renderer_factory, name):
    from par_raytracer_amd import api, capi
    r = gpu_renderer_factory(name)
    s, _ = scene_dir(name)
    w, h, p0 = 64, 48, 1000
    cam = api.make_camera(s.fov, w, h, s.camera_position, s.camera_facing)
    for spp in (3, 8):
        for n in (65, 257):
            o, d = R.camera_rays(cam, SEED, w, p0, n, spp)
            rgba, ctr = call(r, o, d, params_for(spp), first=p0, camera_stream=True)
            for pipeline in (capi.PIPELINE_WAVEFRONT, capi.PIPELINE_POOL):
                img, ictr = r.render(cam, params_for(spp, pipeline=pipeline), w, h, p0, p0 + n)
                what = "%s: %d x %d against pipeline %d" % (name, n, spp, pipeline)
                assert ictr.pipeline == pipeline, what
                assert np.array_equal(bits(rgba), bits(img)), (what, float(np.abs(rgba - img).max()))
                assert ctr.ray_count == ictr.ray_count and ctr.shaded_hits == ictr.shaded_hits, what
            t_rgba, t_ctr = call(r, o, d, params_for(spp), first=p0, camera_stream=True, torch_path=True)
            assert np.array_equal(bits(t_rgba), bits(rgba)) and t_ctr.ray_count == ctr.ray_count
            # without the flag the stream is another one: the image differs (the rays are the same)
            other, _ = call(r, o, d, params_for(spp), first=p0, camera_stream=False)
            assert not np.array_equal(bits(other), bits(rgba)), name


# ---- 3. purity

PURITY_SCENES = ("many_materials", "coincident")


def purity_batch(name):
    _, o, d = scene_rays(name)
    return o[:, :3], d[:, :3]


def digest(rgba, ctr):
    return hashlib.sha256(bits(rgba).tobytes()).hexdigest() + " %d %d" % (ctr.ray_count, ctr.shaded_hits)


@pytest.fixture(scope="module")
def purity_base(gpu_renderer_factory):
    base = {}
    for name in PURITY_SCENES:
        o, d = purity_batch(name)
        base[name] = call(gpu_renderer_factory(name), o, d, params_for(3), first=1000)
    return base


def same(got, want, what):
    assert np.array_equal(bits(got[0]), bits(want[0])), what
    assert got[1].ray_count == want[1].ray_count and got[1].shaded_hits == want[1].shaded_hits, what


@pytest.mark.gpu
@pytest.mark.parametrize("name", PURITY_SCENES)
def test_a_batch_in_three_calls(gpu_renderer_factory, purity_base, name):
    r = gpu_renderer_factory(name)
    o, d = purity_batch(name)
    for torch_path in (False, True):
        parts = [call(r, o[a:b], d[a:b], params_for(3), first=1000 + a, torch_path=torch_path) for a, b in ((0, 64), (64, 65), (65, 257))]
        assert np.array_equal(bits(np.concatenate([p[0] for p in parts])), bits(purity_base[name][0])), name
        assert sum(p[1].ray_count for p in parts) == purity_base[name][1].ray_count
        assert sum(p[1].shaded_hits for p in parts) == purity_base[name][1].shaded_hits
    flat, _ = call(r, o.reshape(-1, 3), d.reshape(-1, 3), params_for(3), first=1000)             # (count * spp, 3) is the same batch
    assert np.array_equal(bits(flat), bits(purity_base[name][0]))


@pytest.mark.gpu
@pytest.mark.parametrize("option", [("CHAINS", 2), ("PASS_SAMPLES", 192), ("PASS_SAMPLES", 3), ("STACK_CAP", 2), ("SHADOW_TREES", 0)])
@pytest.mark.parametrize("name", PURITY_SCENES)
def test_same_bits_under_other_schedules(gpu_renderer_factory, purity_base, name, option):
    """CHAINS=2: two chains of 576 + 195 samples; PASS_SAMPLES=192: five passes of 64 outputs; 3: one output per pass; STACK_CAP=2:
    nearly every walk overflows its LDS column and goes to k_trace_exact; SHADOW_TREES=0: every shadow ray starts at the root."""
    r = gpu_renderer_factory(name)
    o, d = purity_batch(name)
    r.set_option(*option)
    try:
        for torch_path in (False, True):
            same(call(r, o, d, params_for(3), first=1000, torch_path=torch_path), purity_base[name], "%s, %s=%s" % ((name,) + option))
    finally:
        r.set_option(option[0], None)
    r.set_option("CHAINS", 2)
    r.set_option("PASS_SAMPLES", 192 * 2)
    try:
        same(call(r, o, d, params_for(3), first=1000), purity_base[name], name + ", passes x chains")
    finally:
        r.set_option("CHAINS", None)
        r.set_option("PASS_SAMPLES", None)


@pytest.mark.gpu
@pytest.mark.parametrize("name", PURITY_SCENES)
def test_same_bits_on_an_lbvh_tree(purity_base, name):
    from par_raytracer_amd import api
    o, d = purity_batch(name)
    r = api.Renderer(0)
    try:
        r.set_option("BVH_BUILDER", "lbvh")
        r.upload(host_scene(name))
        same(call(r, o, d, params_for(3), first=1000), purity_base[name], name + ", lbvh")
    finally:
        r.close()


CHILD = r"""
import os, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, "tests")); sys.path.insert(0, os.path.join(%(root)r, "oracle"))
import conftest
from test_gpu_render_rays import PURITY_SCENES, call, digest, params_for, purity_batch
from par_raytracer_amd import api, capi
lib = capi.hip_lib()
assert os.path.basename(lib._name) == "libprt_hip_bvh8.so" and not (lib.prt_build_flags() & capi.BUILD_BVH4)
for name in PURITY_SCENES:
    o, d = purity_batch(name)
    r = api.Renderer(0)
    r.upload(conftest.host_scene(name))
    print("digest", name, digest(*call(r, o, d, params_for(3), first=1000)), flush=True)
    r.close()
print("bvh8 render_rays ok")
"""


@pytest.mark.gpu
def test_same_bits_on_the_8_wide_library(purity_base):
    assert os.path.exists(os.path.join(ROOT, "par_raytracer_amd", "libprt_hip_bvh8.so")), "libprt_hip_bvh8.so not built (make hip-bvh8)"
    env = dict(os.environ)
    env["PRT_HIP_LIB"] = "libprt_hip_bvh8.so"
    out = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    text = out.stdout.decode()
    assert out.returncode == 0 and "bvh8 render_rays ok" in text, (out.returncode, text[-1500:], out.stderr.decode()[-3000:])
    for name in PURITY_SCENES:
        assert "digest %s %s" % (name, digest(*purity_base[name])) in text, (name, text)


@pytest.mark.gpu
def test_radiance_follows_the_geometry():
    """After update_geometry: the bits of a fresh upload of the moved scene; moved back: the bits from before the move."""
    from par_raytracer_amd import api
    name = "cornell_box"
    arrays, o, d = scene_rays(name)
    o, d = o[:, :3], d[:, :3]

    full = api.desc_arrays(host_scene(name).desc)

    def desc(positions):
        a = dict(full)
        a["positions"] = positions
        a["spheres"], a["sphere_group"] = np.zeros(0, np.uint8), np.zeros(0, np.int32)      # an update keeps no hierarchy either
        return api.FlatDesc(a)
    here = full["positions"].copy()
    there = here.reshape(-1, 3).copy()
    there[:, 1] = there[:, 1] * np.float32(0.75) + there[:, 0] * np.float32(0.125)            # squashed and sheared
    there = np.ascontiguousarray(there.reshape(-1))
    r, fresh = api.Renderer(0), api.Renderer(0)
    try:
        keep_here, keep_there = desc(here), desc(there)
        r.upload(keep_here)
        before = call(r, o, d, params_for(3), first=7)
        r.update_geometry(there)
        moved = call(r, o, d, params_for(3), first=7)
        fresh.upload(keep_there)
        same(moved, call(fresh, o, d, params_for(3), first=7), "moved against a fresh upload")
        assert not np.array_equal(bits(moved[0]), bits(before[0])), "the move matters"
        r.update_geometry(here)
        same(call(r, o, d, params_for(3), first=7), before, "moved back")
    finally:
        r.close()
        fresh.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("cornell_box", "many_materials"))
def test_origins_beyond_the_shadow_trees_guard(gpu_renderer_factory, name):
    """Origins at 10 x the scene's extent: inside the domain (64 x), outside the bound within which a call may use the shadow trees
    (4 x).  The harness's radiance, and the bits of SHADOW_TREES=0."""
    r = gpu_renderer_factory(name)
    arrays, _, _ = scene_rays(name)
    o, d = R.far_rays(arrays, 65, 3, 9, 10.0)
    am = R.scene_abs_max(arrays)
    assert (np.abs(o).max(-1) > np.float32(4.0) * am).all() and R.in_domain(o, d, params_for(3).ray_bias, am).all()
    exp = R.oracle_batch(host_scene(name).desc, params_for(3), o, d, first=3)
    assert exp["primary_hit"].any()
    got = call(r, o, d, params_for(3), first=3)
    diff = float(np.abs(got[0][:, :3] - exp["rgba"][:, :3]).max())
    assert diff <= R.TOL and got[1].ray_count == exp["ray_count"], (name, diff, got[1].ray_count, exp["ray_count"])
    assert got[1].shaded_hits == exp["shaded_hits"], name
    r.set_option("SHADOW_TREES", 0)
    try:
        same(call(r, o, d, params_for(3), first=3), got, name + ", far, SHADOW_TREES=0")
    finally:
        r.set_option("SHADOW_TREES", None)


# ---- 4. refusals

def violations(abs_max):
    """name -> (what to do to ray 100 of a valid 65 x 3 batch, ray_bias or None)."""
    f = np.float32

    def set_o(k, v):
        def edit(o, d):
            o.reshape(-1, 3)[100, k] = v
        return edit

    def set_d(k, v):
        def edit(o, d):
            d.reshape(-1, 3)[100, k] = v
        return edit

    def scale_d(s):
        def edit(o, d):
            d.reshape(-1, 3)[100] *= f(s)
        return edit
    return {"nan origin": (set_o(1, np.nan), None), "inf origin": (set_o(0, -np.inf), None), "nan direction": (set_d(2, np.nan), None),
            "inf direction": (set_d(0, np.inf), None), "zero direction": (scale_d(0.0), None),
            "long direction": (scale_d(np.sqrt(1.0 + 2.0 ** -16)), None), "short direction": (scale_d(np.sqrt(1.0 - 2.0 ** -16)), None),
            "twice the length": (scale_d(2.0), None), "far origin": (set_o(2, f(65.0) * abs_max), None),
            "infinite bias": (lambda o, d: None, np.inf), "nan bias": (lambda o, d: None, np.nan)}


@pytest.mark.gpu
def test_domain_violations_refuse_the_whole_batch(gpu_renderer_factory):
    import torch
    from par_raytracer_amd import capi
    lib = capi.hip_lib()
    name = "cornell_box"
    r = gpu_renderer_factory(name)
    arrays, o0, d0 = scene_rays(name)
    am = R.scene_abs_max(arrays)
    for what, (edit, bias) in violations(am).items():
        o, d = np.ascontiguousarray(o0[:65, :3]).copy(), np.ascontiguousarray(d0[:65, :3]).copy()
        edit(o, d)
        p = params_for(3)
        if bias is not None:
            p.ray_bias = bias
        ok = R.in_domain(o, d, p.ray_bias, am)
        n_bad, first_bad = int((~ok).sum()), int(np.argmin(ok))
        assert n_bad == (195 if bias is not None else 1) and first_bad == (0 if bias is not None else 100), what
        text = r"prt_render_rays: %d of 195 rays lie outside the domain .*the first is ray %d$" % (n_bad, first_bad)
        # host entry point
        out = np.full((65, 4), 7.5, np.float32)
        ctr = capi.PrtCounters()
        ctr.ray_count = 99
        b = capi.PrtRadianceBatch(o.ctypes.data, d.ctypes.data, 65, 0, 5)
        assert lib.prt_render_rays(r._ctx, C.byref(b), C.byref(p), out.ctypes.data, C.byref(ctr)) == -1, what
        assert re.search(text, lib.prt_last_error(r._ctx).decode()), (what, lib.prt_last_error(r._ctx).decode())
        assert np.all(out == 7.5) and ctr.ray_count == 99, what
        # device entry point
        to, td = torch.from_numpy(o).to("cuda:0"), torch.from_numpy(d).to("cuda:0")
        tout = torch.full((65, 4), 7.5, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        b = capi.PrtRadianceBatch(to.data_ptr(), td.data_ptr(), 65, 0, 5)
        assert lib.prt_render_rays_device(r._ctx, C.byref(b), C.byref(p), tout.data_ptr(), C.byref(ctr)) == -1, what
        assert re.search(text, lib.prt_last_error(r._ctx).decode()), what
        assert bool((tout == 7.5).all()), what
        with pytest.raises(RuntimeError, match=r"prt_render_rays failed \(-1\): prt_render_rays: %d of 195 rays lie outside the domain" % n_bad):
            r.render_rays(o, d, p, first=5)
    # the bounds themselves are inside: |d|^2 within 2^-20 of 1, an origin at 63 x the extent; the call then renders
    o, d = np.ascontiguousarray(o0[:65, :3]).copy(), np.ascontiguousarray(d0[:65, :3]).copy()
    d.reshape(-1, 3)[100] *= np.float32(np.sqrt(1.0 + 2.0 ** -20))
    o.reshape(-1, 3)[7, 0] = np.float32(63.0) * am
    assert R.in_domain(o, d, params_for(3).ray_bias, am).all()
    rgba, ctr = r.render_rays(o, d, params_for(3), first=5)
    assert np.all(rgba[:, 3] == 1.0) and ctr.ray_count >= 195


@pytest.mark.gpu
def test_argument_refusals():
    """Each refusal's code and text, through both entry points; nothing is written."""
    from par_raytracer_amd import api, capi
    lib = capi.hip_lib()
    _, o0, d0 = scene_rays("cornell_box")
    o, d = np.ascontiguousarray(o0[:4, :3]), np.ascontiguousarray(d0[:4, :3])
    out = np.full((4, 4), 7.5, np.float32)

    def batch(origins=o.ctypes.data, directions=d.ctypes.data, count=4, flags=0, first=0):
        return capi.PrtRadianceBatch(origins, directions, count, flags, first)
    r = api.Renderer(0)

    def last():
        return lib.prt_last_error(r._ctx).decode()
    good = params_for(3)
    try:
        for entry in (lib.prt_render_rays, lib.prt_render_rays_device):
            assert entry(None, C.byref(batch()), C.byref(good), out.ctypes.data, None) == -1
            assert entry(r._ctx, C.byref(batch()), C.byref(good), out.ctypes.data, None) == -2
            assert last() == "prt_render_rays: no scene uploaded"
        with pytest.raises(RuntimeError, match=r"prt_render_rays failed \(-2\): prt_render_rays: no scene uploaded"):
            r.render_rays(o, d, good)
        r.upload(host_scene("cornell_box"))
        ctr = capi.PrtCounters()
        for entry in (lib.prt_render_rays, lib.prt_render_rays_device):
            def refused(b, p, text, o_ptr=out.ctypes.data):
                assert entry(r._ctx, b if b is None else C.byref(b), p if p is None else C.byref(p), o_ptr, None) == -1, text
                assert last() == text
            refused(None, good, "prt_render_rays: null batch or params")
            refused(batch(), None, "prt_render_rays: null batch or params")
            for b in (batch(origins=None), batch(directions=None)):
                refused(b, good, "prt_render_rays: null origins, directions or output")
            refused(batch(), good, "prt_render_rays: null origins, directions or output", None)
            for flags in (2, 3, 0x80000000):
                refused(batch(flags=flags), good, "prt_render_rays: unknown flag")
            for spp in (0, 65536):
                refused(batch(), params_for(spp), "prt_render_rays: spp must be in 1..65535 (prt_key.h packs the sample in 16 bits)")
            refused(batch(), params_for(3, bounce_depth=17), "prt_render_rays: bounce_depth > 16 not supported")
            for first, count in ((2 ** 32 - 3, 4), (2 ** 32 + 1, 0), (2 ** 64 - 1, 4)):
                refused(batch(first=first, count=count), good, "prt_render_rays: first + count exceeds 2^32 (the output index is the key's pixel word)")
            refused(batch(), params_for(3, max_spp=4), "prt_render_rays: adaptive sampling (max_spp > spp) is not supported for caller rays")
            for pipeline in (capi.PIPELINE_POOL, capi.PIPELINE_MEGAKERNEL, capi.PIPELINE_POOL | capi.FLAG_COUNT_VISITS):
                refused(batch(), params_for(3, pipeline=pipeline), "prt_render_rays: runs on PRT_PIPELINE_WAVEFRONT (or DEFAULT) only")
            # count == 0: nothing is written, the counters are zeroed; null arrays and a null output are then fine
            ctr.ray_count = 99
            assert entry(r._ctx, C.byref(batch(origins=None, directions=None, count=0, first=2 ** 32)), C.byref(good), None, C.byref(ctr)) == 0
            assert ctr.ray_count == 0
        assert np.all(out == 7.5), "nothing was written"
        empty, ectr = r.render_rays(np.zeros((0, 3, 3), np.float32), np.zeros((0, 3, 3), np.float32), good)
        assert empty.shape == (0, 4) and ectr.ray_count == 0
        with pytest.raises(ValueError, match="not a multiple of params.spp"):
            r.render_rays(np.zeros((4, 3), np.float32), np.zeros((4, 3), np.float32), good)
        with pytest.raises(ValueError):
            r.render_rays(o, d[:3], good)
        with pytest.raises(RuntimeError, match=r"\(-1\): prt_render_rays: first \+ count exceeds 2\^32"):
            r.render_rays(o, d, good, first=2 ** 32 - 3)
        # the last output index there is: first + count = 2^32
        rgba, c = r.render_rays(o, d, good, first=2 ** 32 - 4)
        assert np.all(rgba[:, 3] == 1.0) and c.ray_count >= 12
    finally:
        r.close()
