#!/usr/bin/env python3
"""Closest-point rates (prt_closest_points) on the C4 scene (terrain_1m).

    python tools/closest_points_rate.py [--reps N] [--out FILE]

1. 2^20 points near the surface: random barycentric points on random triangles, displaced along +- the normal by up to 1 % of the
   scene's extent.
2. 2^20 points uniform in the scene's bounding box.
Device entry point (torch tensors), fields dist2 and group.  Median and min of --reps calls each after one warm-up call, kernels
(counters.trace_kernel_ms: k_closest + k_closest_exact) and whole call (render_ms); node visits and triangle tests per point from
one more call with count_visits.  The lines go to stdout and to --out (default profiles/r06_closest_points.txt).
"""
from __future__ import annotations

import argparse
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from par_raytracer_amd import api, capi, scenes  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r06_closest_points.txt"))
    a = ap.parse_args()
    import torch
    s = scenes.make_scene("terrain_1m")
    d = tempfile.mkdtemp(prefix="prt_rate_")
    scenes.write_obj(s, d, "scene.obj")
    hs = api.HostScene(d, "scene.obj", 0, s.camera_position)
    arr = hs.arrays()
    r = api.Renderer(0)
    r.upload(hs)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
    wide = "8-wide tree" if not capi.hip_lib().prt_build_flags() & capi.BUILD_BVH4 else "4-wide tree"
    say("closest points on the C4 scene: %d triangles, %s" % (r.scene_info().triangle_count, wide))

    n = 1 << 20
    rng = np.random.default_rng(21)
    P = np.asarray(arr["positions"], np.float64).reshape(-1, 3)
    idx = np.asarray(arr["idx_positions"]).reshape(-1, 3)
    lo, hi = P[idx.reshape(-1)].min(0), P[idx.reshape(-1)].max(0)
    extent = float((hi - lo).max())
    tri = rng.integers(0, len(idx), n)
    pa, pb, pc = P[idx[tri, 0]], P[idx[tri, 1]], P[idx[tri, 2]]
    bw = rng.uniform(0.0, 1.0, (n, 3))
    bw /= bw.sum(1, keepdims=True)
    nrm = np.cross(pb - pa, pc - pa)
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-300)
    near = bw[:, :1] * pa + bw[:, 1:2] * pb + bw[:, 2:] * pc + nrm * rng.uniform(-0.01, 0.01, (n, 1)) * extent
    box = lo + (hi - lo) * rng.uniform(0.0, 1.0, (n, 3))
    for what, pts in (("near the surface (within 1 % of the extent)", near), ("uniform in the bounding box", box)):
        t = torch.from_numpy(np.ascontiguousarray(pts.astype(np.float32))).cuda()
        call = lambda **kw: r.closest_points(t, fields=("dist2", "group"), **kw)     # noqa: E731
        call()
        runs = [call()["counters"] for _ in range(a.reps)]
        ker = [c.trace_kernel_ms for c in runs]
        whole = [c.render_ms for c in runs]
        vis = call(count_visits=True)["counters"]
        say("%d points %s: kernels median %.3f min %.3f ms (%.1f Mpoints/s at the median), whole call median %.3f min %.3f ms, over %d calls; "
            "per point %.1f node visits, %.1f triangle tests" % (n, what, float(np.median(ker)), min(ker), n / float(np.median(ker)) / 1e3,
                                                                 float(np.median(whole)), min(whole), a.reps, vis.node_visits / n, vis.tri_tests / n))
    r.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
