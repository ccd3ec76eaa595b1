#!/usr/bin/env python3
"""Signed-distance rates (prt_signed_distance) against prt_closest_points on the C4 scene (terrain_1m).

    python tools/signed_distance_rate.py [--reps N] [--out FILE]

2^20 points near the surface: random barycentric points on random triangles, displaced along +- the normal by up to 1 % of the
scene's extent.  Device entry points (torch tensors); prt_closest_points with the fields dist2 and group, prt_signed_distance with
those and signed_distance and feature, on the same context and batch.  The walk is shared, so the number of interest is the ratio
of the two rates.  Median, min and max of --reps calls each after one warm-up call, the two calls taken in turn, kernels (counters.trace_kernel_ms: k_closest +
k_closest_exact) and whole call (render_ms).  The table build: render_ms of a 64-point signed query right after prt_update_geometry
(it refills the accumulators with k_signed_normals) minus the median render_ms of the three that follow, median of --reps
updates; and the one-off host build of the adjacency, as wall time of the first signed query after the upload minus a later call's.
The lines go to stdout and to --out (default profiles/signed_distance.txt).
"""
from __future__ import annotations

import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from par_raytracer_amd import api, capi, scenes  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "signed_distance.txt"))
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
    say("signed distances on the C4 scene: %d triangles, %d positions, %s" % (r.scene_info().triangle_count, len(arr["positions"]), wide))

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
    t = torch.from_numpy(np.ascontiguousarray(near.astype(np.float32))).cuda()
    signed = lambda: r.signed_distance(t, fields=("dist2", "group", "signed_distance", "feature"))     # noqa: E731
    closest = lambda: r.closest_points(t, fields=("dist2", "group"))                                    # noqa: E731

    t0 = time.perf_counter()
    signed()                                                # builds the adjacency on the host, fills the accumulators
    first_wall = time.perf_counter() - t0
    t0 = time.perf_counter()
    signed()
    later_wall = time.perf_counter() - t0
    closest()
    rate = {}
    calls = (("prt_signed_distance", signed), ("prt_closest_points", closest))
    runs = {what: [] for what, _ in calls}
    for _ in range(a.reps):                                 # the two calls in turn: a drift of the machine reaches both alike
        for what, call in calls:
            runs[what].append(call()["counters"])
    for what, _ in calls:
        ker = [c.trace_kernel_ms for c in runs[what]]
        whole = [c.render_ms for c in runs[what]]
        rate[what] = n / float(np.median(ker)) / 1e3
        say("%s, %d points near the surface (within 1 %% of the extent): kernels median %.3f min %.3f max %.3f ms (%.1f Mpoints/s at the "
            "median), whole call median %.3f min %.3f ms, over %d calls" % (what, n, float(np.median(ker)), min(ker), max(ker), rate[what],
                                                                          float(np.median(whole)), min(whole), a.reps))
    say("prt_signed_distance / prt_closest_points: %.3f of the rate" % (rate["prt_signed_distance"] / rate["prt_closest_points"]))

    # the refill alone: a batch of 64 points, whose walk is small beside it
    positions = torch.from_numpy(np.ascontiguousarray(arr["positions"], np.float32)).cuda()
    few = t[:64].contiguous()
    small = lambda: r.signed_distance(few, fields=("signed_distance", "feature"))["counters"].render_ms     # noqa: E731
    small()
    fills = []
    for k in range(a.reps):
        r.update_geometry(positions)
        after = small()
        fills.append(after - float(np.median([small() for _ in range(3)])))
    say("table build after an update (k_signed_normals: zero and fill, on the device; render_ms of a 64-point signed query right after "
        "prt_update_geometry minus the median of the next three): median %.3f min %.3f max %.3f ms over %d updates" % (
            float(np.median(fills)), min(fills), max(fills), a.reps))
    say("adjacency build at the first signed query after the upload (host, once per upload): %.1f ms" % (1e3 * (first_wall - later_wall)))
    r.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
