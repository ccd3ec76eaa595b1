#!/usr/bin/env python3
"""Ray-query rates (prt_trace_rays) on the C4 scene (terrain_1m).

    python tools/trace_rays_rate.py [--reps N]

1. 1920 x 1080 pixel-centre camera rays, CLOSEST: k_query's time (counters.trace_kernel_ms: k_query + k_query_exact) against
   k_trace's in a WAVEFRONT render that traces camera rays only (spp 1, bounce_depth 0, the scene without its light), whose
   ray_count must be 2,073,600.  Same traversal code; the render's k_trace also runs the wavefront's queue plumbing.
2. Incoherent rays: origins at the first hits of (1), cosine-distributed directions about the hit normal from a host RNG,
   CLOSEST and OCCLUDED.
3. A 64 k-ray batch (the first rays of (2)): fixed overhead.
Median of --reps calls each (after one warm-up call); the line before each result gives the kernels' min and median, for A/B runs.  Mrays/s = rays / trace_kernel_ms and rays / render_ms (the whole call).
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from par_raytracer_amd import api, capi, scenes  # noqa: E402


def camera_rays(s, w, h):
    """Pixel-centre camera rays (MakeCameraRay, main.cpp:165-176, without the jitter), float32 unit directions."""
    cam = api.make_camera(s.fov, w, h, s.camera_position, s.camera_facing)
    f = np.array(cam.forward, np.float64)
    rs = np.array(cam.right, np.float64) * cam.tan_a2 * cam.aspect
    us = np.array(cam.up, np.float64) * cam.tan_a2
    x = (np.arange(w) + 0.5) * cam.inv_width * 2.0 - 1.0
    y = 1.0 - (np.arange(h) + 0.5) * cam.inv_height * 2.0
    d = f[None, None] + x[None, :, None] * rs[None, None] + y[:, None, None] * us[None, None]
    d = d.reshape(-1, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = np.repeat(np.array(s.camera_position, np.float32)[None], w * h, 0)
    return np.ascontiguousarray(o), np.ascontiguousarray(d.astype(np.float32)), cam


def timed(fn, reps):
    fn()
    runs = [fn() for _ in range(reps)]
    ker = float(np.median([c.trace_kernel_ms for c in runs]))
    call = float(np.median([c.render_ms for c in runs]))
    print("    [kernels min %.3f median %.3f ms over %d calls]" % (min(c.trace_kernel_ms for c in runs), ker, reps))
    return runs[-1], ker, call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    s = scenes.make_scene("terrain_1m")
    d = tempfile.mkdtemp(prefix="prt_rate_")
    scenes.write_obj(s, d, "scene.obj")
    hs = api.HostScene(d, "scene.obj", 0, s.camera_position)
    # the same scene without its light: a bounce_depth 0 render then traces camera rays and nothing else
    dark = capi.PrtSceneDesc()
    C.memmove(C.byref(dark), hs.desc, C.sizeof(capi.PrtSceneDesc))
    dark.light_count = 0
    r = api.Renderer(0)
    r.upload(C.pointer(dark))
    w, h = 1920, 1080
    o, dirs, cam = camera_rays(s, w, h)
    print("C4 scene: %d triangles, %s" % (r.scene_info().triangle_count, "8-wide tree" if not capi.hip_lib().prt_build_flags() & capi.BUILD_BVH4 else "4-wide tree"))

    p = api.default_params(1, 1234, bounce_depth=0, pipeline=capi.PIPELINE_WAVEFRONT)
    ctr, ker, call = timed(lambda: r.render(cam, p, w, h)[1], a.reps)
    assert ctr.ray_count == w * h, ctr.ray_count
    print("render WAVEFRONT spp 1 depth 0, no light: ray_count %d, k_trace %.3f ms (%.0f Mrays/s), whole call %.3f ms" % (
        ctr.ray_count, ker, w * h / ker / 1e3, call))
    k_trace = ker

    to, td = torch.from_numpy(o).cuda(), torch.from_numpy(dirs).cuda()
    res = None

    def q_closest():
        nonlocal res
        res = r.trace_rays(to, td)
        return res["counters"]
    ctr, ker, call = timed(q_closest, a.reps)
    assert ctr.ray_count == w * h
    print("query CLOSEST, camera rays: k_query %.3f ms (%.0f Mrays/s), whole call %.3f ms; k_query / k_trace = %.3f" % (
        ker, w * h / ker / 1e3, call, ker / k_trace))
    vis = r.trace_rays(to, td, count_visits=True)["counters"]
    print("    per ray: %.2f node visits, %.2f triangle tests" % (vis.node_visits / (w * h), vis.tri_tests / (w * h)))
    p_cnt = api.default_params(1, 1234, bounce_depth=0, pipeline=capi.PIPELINE_WAVEFRONT | capi.FLAG_COUNT_VISITS)
    rc = r.render(cam, p_cnt, w, h)[1]
    st = r.render_stats()
    print("    render, per ray: %.2f node visits, %.2f triangle tests; wave node steps %d" % (
        rc.node_visits / (w * h), rc.tri_tests / (w * h), st.wave_node_steps))

    # incoherent rays from the first hits
    hit = (res["group"] >= 0).cpu().numpy()
    pos = res["position"].cpu().numpy()[hit]
    nrm = res["normal"].cpu().numpy()[hit]
    rng = np.random.default_rng(11)
    u1, u2 = rng.random(len(pos)), rng.random(len(pos))
    rr, phi = np.sqrt(u1), 2 * np.pi * u2
    t1 = np.cross(nrm, np.where(np.abs(nrm[:, :1]) > 0.9, [[0.0, 1.0, 0.0]], [[1.0, 0.0, 0.0]]))
    t1 /= np.linalg.norm(t1, axis=1, keepdims=True)
    t2 = np.cross(nrm, t1)
    dd = (t1 * (rr * np.cos(phi))[:, None] + t2 * (rr * np.sin(phi))[:, None] + nrm * np.sqrt(1 - u1)[:, None])
    dd /= np.linalg.norm(dd, axis=1, keepdims=True)
    io, idr = torch.from_numpy(np.ascontiguousarray(pos)).cuda(), torch.from_numpy(np.ascontiguousarray(dd.astype(np.float32))).cuda()
    n = len(pos)
    for mode in ("closest", "occluded"):
        ctr, ker, call = timed(lambda: r.trace_rays(io, idr, mode=mode, ray_bias=1e-3, fields=("t",) if mode == "closest" else None)["counters"], a.reps)
        print("query %s, %d incoherent rays: %.3f ms kernels (%.0f Mrays/s), whole call %.3f ms (%.0f Mrays/s)" % (
            mode.upper(), n, ker, n / ker / 1e3, call, n / call / 1e3))
    m = 1 << 16
    so, sd = io[:m].contiguous(), idr[:m].contiguous()
    ctr, ker, call = timed(lambda: r.trace_rays(so, sd, ray_bias=1e-3, fields=("t",))["counters"], a.reps)
    print("query CLOSEST, 64 k incoherent rays: %.3f ms kernels (%.0f Mrays/s), whole call %.3f ms (%.0f Mrays/s)" % (
        ker, m / ker / 1e3, call, m / call / 1e3))
    r.close()


if __name__ == "__main__":
    main()
