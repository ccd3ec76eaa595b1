#!/usr/bin/env python3
"""What the gradients of a closest-hit query cost (prt_trace_rays_backward): 2^20 rays, twice.

    python tools/query_grad_rate.py [--reps N] [--out profiles/r09_query_grad.txt]

1. coherent: a 1024 x 1024 grid of pixel-centre camera rays on cornell_box - dozens of lanes of a wave on one triangle;
2. incoherent: random rays from above terrain_1m, mostly downwards - a wave's lanes on 64 different triangles.
For each: prt_grad_info.device_ms of the backward call (all four output gradients random, all three input gradients wanted) with the
wave merge of k_qgrad_scatter on and off (option QGRAD_MERGE; the two give the same bits, which the tool checks), and render_ms of
the forward prt_trace_rays_device call on the same batch.  One warm-up call, then the median (and min) of --reps calls each, the
two settings interleaved.  Output goes to stdout and to --out."""
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


def load(name):
    s = scenes.make_scene(name)
    d = tempfile.mkdtemp(prefix="prt_qgrad_rate_")
    scenes.write_obj(s, d, "scene.obj")
    hs = api.HostScene(d, "scene.obj", 0, s.camera_position)
    return s, hs


def camera_grid(s, side):
    cam = api.make_camera(s.fov, side, side, s.camera_position, s.camera_facing)
    f = np.array(cam.forward, np.float64)
    rs = np.array(cam.right, np.float64) * cam.tan_a2 * cam.aspect
    us = np.array(cam.up, np.float64) * cam.tan_a2
    x = (np.arange(side) + 0.5) * cam.inv_width * 2.0 - 1.0
    y = 1.0 - (np.arange(side) + 0.5) * cam.inv_height * 2.0
    d = (f[None, None] + x[None, :, None] * rs[None, None] + y[:, None, None] * us[None, None]).reshape(-1, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = np.repeat(np.array(s.camera_position, np.float32)[None], side * side, 0)
    return np.ascontiguousarray(o), np.ascontiguousarray(d.astype(np.float32))


def random_rays(positions, n):
    rng = np.random.default_rng(5)
    lo, hi = positions.min(0), positions.max(0)
    o = (lo + (hi - lo) * rng.random((n, 3))).astype(np.float32)
    o[:, 1] = hi[1] + 5.0
    d = rng.standard_normal((n, 3))
    d[:, 1] = -np.abs(d[:, 1])
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.ascontiguousarray(o), np.ascontiguousarray(d.astype(np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_query_grad.txt"))
    a = ap.parse_args()
    import torch
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say("prt_trace_rays_backward, %d rays, %s; median (min) of %d calls after one warm-up" % (
        N, "8-wide tree" if not capi.hip_lib().prt_build_flags() & capi.BUILD_BVH4 else "4-wide tree", a.reps))
    for name, kind in (("cornell_box", "coherent"), ("terrain_1m", "incoherent")):
        s, hs = load(name)
        arrays = api.desc_arrays(hs.desc)
        P = np.ascontiguousarray(arrays["positions"].reshape(-1, 3))
        o, d = camera_grid(s, 1024) if kind == "coherent" else random_rays(P, N)
        r = api.Renderer(0)
        r.upload(hs)
        to, td, tp = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda(), torch.from_numpy(P).cuda()
        gen = torch.Generator(device="cuda").manual_seed(7)
        g_t = torch.randn((N,), device="cuda", generator=gen)
        g_bw, g_pos, g_nrm = (torch.randn((N, 3), device="cuda", generator=gen) for _ in range(3))
        r.trace_rays(to, td)
        fwd = [r.trace_rays(to, td) for _ in range(a.reps)]
        res = fwd[-1]
        f_ms = [f["counters"].render_ms for f in fwd]
        hits = int((res["group"] >= 0).sum())

        def back(merge):
            r.set_option("QGRAD_MERGE", merge)
            return r.trace_rays_backward(to, td, res["group"], res["vertex0"], tp, grad_t=g_t, grad_bw=g_bw, grad_position=g_pos,
                                         grad_normal=g_nrm)
        ms = {0: [], 1: []}
        first = {m: back(m) for m in (0, 1)}                  # warm-up, and the bits
        same = all(torch.equal(first[0][k].view(torch.int32), first[1][k].view(torch.int32)) for k in ("positions", "origins", "directions"))
        for _ in range(a.reps):
            for m in (0, 1):
                ms[m].append(back(m)["info"].device_ms)
        info = first[1]["info"]
        say("%s (%s, %d triangles, %d positions): %d hits, %d contributing, %d skipped; unit 2^%d, largest contribution %.6g" % (
            name, kind, arrays["idx_positions"].size // 3, P.shape[0], hits, info.hit_rays, info.skipped_rays, info.unit_exponent,
            info.max_contribution))
        say("    backward device_ms: merge on %.3f (min %.3f), merge off %.3f (min %.3f); bits %s" % (
            float(np.median(ms[1])), min(ms[1]), float(np.median(ms[0])), min(ms[0]), "equal" if same else "DIFFER"))
        say("    forward prt_trace_rays_device render_ms: %.3f (min %.3f)" % (float(np.median(f_ms)), min(f_ms)))
        r.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
