#!/usr/bin/env python3
"""K-nearest-hits rates (prt_trace_hits) on the C4 scene (terrain_1m).

    python tools/trace_hits_rate.py [--reps N] [--append profiles/trace_hits.txt]

The rays of tools/trace_rays_rate.py: 1920 x 1080 pixel-centre camera rays, and incoherent rays from their first hits (cosine
lobes about the hit normals, ray_bias 1e-3).  On each set PRT_QUERY_CLOSEST (field t) first, then prt_trace_hits at k = 1, 4 and
16, front only and both sides (fields hit_count and t), in the same run on the same device arrays.  Median of --reps calls each
after one warm-up call; Mrays/s = rays / trace_kernel_ms (the two kernels) and rays / render_ms (the whole call).  --append adds
the lines it prints to that file.
"""
from __future__ import annotations

import argparse
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from par_raytracer_amd import api, capi, scenes  # noqa: E402
from trace_rays_rate import camera_rays, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--append", default=None)
    a = ap.parse_args()
    import torch
    lines = []

    def say(text):
        print(text)
        lines.append(text)
    s = scenes.make_scene("terrain_1m")
    d = tempfile.mkdtemp(prefix="prt_rate_")
    scenes.write_obj(s, d, "scene.obj")
    hs = api.HostScene(d, "scene.obj", 0, s.camera_position)
    r = api.Renderer(0)
    r.upload(hs)
    w, h = 1920, 1080
    o, dirs, _ = camera_rays(s, w, h)
    say("C4 scene: %d triangles, %s, %d reps" % (r.scene_info().triangle_count,
                                                 "8-wide tree" if not capi.hip_lib().prt_build_flags() & capi.BUILD_BVH4 else "4-wide tree", a.reps))
    to, td = torch.from_numpy(o).cuda(), torch.from_numpy(dirs).cuda()
    first = r.trace_rays(to, td)
    hit = (first["group"] >= 0).cpu().numpy()
    pos, nrm = first["position"].cpu().numpy()[hit], first["normal"].cpu().numpy()[hit]
    rng = np.random.default_rng(11)
    u1, u2 = rng.random(len(pos)), rng.random(len(pos))
    rr, phi = np.sqrt(u1), 2 * np.pi * u2
    t1 = np.cross(nrm, np.where(np.abs(nrm[:, :1]) > 0.9, [[0.0, 1.0, 0.0]], [[1.0, 0.0, 0.0]]))
    t1 /= np.linalg.norm(t1, axis=1, keepdims=True)
    t2 = np.cross(nrm, t1)
    dd = (t1 * (rr * np.cos(phi))[:, None] + t2 * (rr * np.sin(phi))[:, None] + nrm * np.sqrt(1 - u1)[:, None])
    dd /= np.linalg.norm(dd, axis=1, keepdims=True)
    io, idr = torch.from_numpy(np.ascontiguousarray(pos)).cuda(), torch.from_numpy(np.ascontiguousarray(dd.astype(np.float32))).cuda()

    for what, ro, rd, bias in (("camera rays", to, td, 0.0), ("incoherent rays", io, idr, 1e-3)):
        n = int(ro.shape[0])
        ctr, ker, call = timed(lambda: r.trace_rays(ro, rd, ray_bias=bias, fields=("t",))["counters"], a.reps)
        say("%s, %d: CLOSEST %.3f ms kernels (%.0f Mrays/s), whole call %.3f ms" % (what, n, ker, n / ker / 1e3, call))
        closest = ker
        for back in (False, True):
            for k in (1, 4, 16):
                res = None

                def q():
                    nonlocal res
                    res = r.trace_hits(ro, rd, k, ray_bias=bias, back_faces=back, fields=("hit_count", "t"))
                    return res["counters"]
                ctr, ker, call = timed(q, a.reps)
                say("%s, %d: hits k=%-2d %s %.3f ms kernels (%.0f Mrays/s, %.2f x CLOSEST), whole call %.3f ms, %.2f hits per ray" % (
                    what, n, k, "both sides" if back else "front only", ker, n / ker / 1e3, ker / closest, call,
                    float(res["hit_count"].float().mean())))
    r.close()
    if a.append:
        with open(a.append, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
