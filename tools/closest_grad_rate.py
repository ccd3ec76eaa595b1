#!/usr/bin/env python3
"""What the gradients of a closest-point query cost (prt_closest_points_backward) on the C4 scene (terrain_1m):
2^20 points, twice.

    python tools/closest_grad_rate.py [--reps N] [--out profiles/closest_grad.txt]

1. scan-like: 16 random barycentric points on each of 2^16 random triangles, displaced along +- the normal by up to 1 % of the
   scene's extent, in the order of a sweep over the surface (sorted by triangle) - a scan denser than the mesh: lanes of a wave
   share triangles;
2. uniform: points uniform in the scene's bounding box, in random order - a wave's lanes on 64 different triangles as a rule.
For each: prt_grad_info.device_ms of the backward call (all three output gradients random, both input gradients wanted) with the
wave merge of k_cgrad_scatter on and off (option QGRAD_MERGE; the two give the same bits, which the tool checks), the number of
distinct triangles per wave of 64 points, and render_ms of the forward prt_closest_points_device call on the same batch.  One
warm-up call, then the median (and min) of --reps calls each, the two settings interleaved.  Output goes to stdout and to --out."""
from __future__ import annotations

import argparse
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from par_raytracer_amd import api, capi, scenes  # noqa: E402

N = 1 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "closest_grad.txt"))
    a = ap.parse_args()
    import torch
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    s = scenes.make_scene("terrain_1m")
    d = tempfile.mkdtemp(prefix="prt_cgrad_rate_")
    scenes.write_obj(s, d, "scene.obj")
    hs = api.HostScene(d, "scene.obj", 0, s.camera_position)
    arr = hs.arrays()
    r = api.Renderer(0)
    r.upload(hs)
    P32 = np.ascontiguousarray(np.asarray(arr["positions"], np.float32).reshape(-1, 3))
    P = P32.astype(np.float64)
    idx = np.asarray(arr["idx_positions"]).reshape(-1, 3)
    say("prt_closest_points_backward, %d points on the C4 scene (%d triangles, %d positions), %s; median (min) of %d calls after one warm-up" % (
        N, len(idx), P.shape[0], "8-wide tree" if not capi.hip_lib().prt_build_flags() & capi.BUILD_BVH4 else "4-wide tree", a.reps))
    rng = np.random.default_rng(23)
    lo, hi = P[idx.reshape(-1)].min(0), P[idx.reshape(-1)].max(0)
    extent = float((hi - lo).max())
    tri = np.repeat(np.sort(rng.integers(0, len(idx), N // 16)), 16)
    pa, pb, pc = P[idx[tri, 0]], P[idx[tri, 1]], P[idx[tri, 2]]
    bw = rng.uniform(0.0, 1.0, (N, 3))
    bw /= bw.sum(1, keepdims=True)
    nrm = np.cross(pb - pa, pc - pa)
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-300)
    scan = bw[:, :1] * pa + bw[:, 1:2] * pb + bw[:, 2:] * pc + nrm * rng.uniform(-0.01, 0.01, (N, 1)) * extent
    box = lo + (hi - lo) * rng.uniform(0.0, 1.0, (N, 3))
    tp = torch.from_numpy(P32).cuda()
    gen = torch.Generator(device="cuda").manual_seed(7)
    g_d2 = torch.randn((N,), device="cuda", generator=gen)
    g_pt, g_bw = (torch.randn((N, 3), device="cuda", generator=gen) for _ in range(2))
    for what, pts in (("scan-like, near the surface", scan), ("uniform in the bounding box", box)):
        t = torch.from_numpy(np.ascontiguousarray(pts.astype(np.float32))).cuda()
        r.closest_points(t, fields=("group", "vertex0"))
        fwd = [r.closest_points(t, fields=("group", "vertex0")) for _ in range(a.reps)]
        res = fwd[-1]
        f_ms = [f["counters"].render_ms for f in fwd]
        key = (res["group"].to(torch.int64) << 32 | (res["vertex0"].to(torch.int64) & 0xFFFFFFFF)).cpu().numpy().reshape(-1, 64)
        per_wave = float(np.mean([len(np.unique(row)) for row in key[::64]]))

        def back(merge):
            r.set_option("QGRAD_MERGE", merge)
            return r.closest_points_backward(t, res["group"], res["vertex0"], tp, grad_dist2=g_d2, grad_point=g_pt, grad_bw=g_bw)
        ms = {0: [], 1: []}
        first = {m: back(m) for m in (0, 1)}                  # warm-up, and the bits
        same = all(torch.equal(first[0][k].view(torch.int32), first[1][k].view(torch.int32)) for k in ("positions", "points"))
        for _ in range(a.reps):
            for m in (0, 1):
                ms[m].append(back(m)["info"].device_ms)
        r.set_option("QGRAD_MERGE", None)
        info = first[1]["info"]
        say("%s: %d contributing, %d skipped, %.1f distinct triangles per wave (every 64th wave); unit 2^%d, largest contribution %.6g" % (
            what, info.hit_rays, info.skipped_rays, per_wave, info.unit_exponent, info.max_contribution))
        say("    backward device_ms: merge on %.3f (min %.3f), merge off %.3f (min %.3f); bits %s" % (
            float(np.median(ms[1])), min(ms[1]), float(np.median(ms[0])), min(ms[0]), "equal" if same else "DIFFER"))
        say("    forward prt_closest_points_device render_ms: %.3f (min %.3f)" % (float(np.median(f_ms)), min(f_ms)))
    r.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
