#!/usr/bin/env python3
"""prt_hemisphere_visibility against the composition it replaces on the C4 scene (terrain_1m).

    python tools/hemi_visibility_rate.py [--reps N] [--points LOG2] [--samples S] [--out FILE]

2^18 surface samples (sample_surface: point and normal) x 64 rays, ray_bias 1e-3, device entry points (torch tensors).
  fused         prt_hemisphere_visibility_device, all three fields and `unoccluded` alone: prt_counters.render_ms.
  composition   prt_trace_rays_device(PRT_QUERY_OCCLUDED) on the same 2^24 rays, already lying on the device as 24 bytes each:
                prt_counters.render_ms, which leaves out making the rays and reducing the answers.
The rays of the composition are made here in numpy from the definition (include/prt.h) - the key, the generator's first draw, the
table with the host's libm, tangent_to_world in float32 - so its answers, summed per point, must equal the fused call's counts:
that is asserted.  --reps calls each after one warm-up call, the three taken in turn; the series, their medians and the scratch
bytes go to stdout and to --out (default profiles/hemi_visibility.txt).
"""
from __future__ import annotations

import argparse
import ctypes
import ctypes.util
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from par_raytracer_amd import api, capi, scenes  # noqa: E402

U = np.uint64
F = np.float32


def sample_keys(seed, j, s):
    """include/prt_key.h on uint64 arrays (the arithmetic wraps)."""
    z = U(seed) + U(0x9E3779B97F4A7C15) * (((j.astype(U) << U(16)) | s.astype(U)) + U(1))
    z = (z ^ (z >> U(30))) * U(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> U(27))) * U(0x94D049BB133111EB)
    return z ^ (z >> U(31))


def first_draws(key):
    """The reference generator seeded with `key`, its first draw (csrc/dev_rng.h)."""
    def chain_step(x):
        x = x ^ (x >> U(12))
        x = x ^ (x >> U(25))
        return x ^ (x >> U(27))
    key = np.where(key == U(0), U(0x5555555555555555), key)
    c0 = chain_step(key)
    s0 = c0 * U(2685821657736338717)
    s1 = chain_step(c0) * U(2685821657736338717)
    s1 = s1 ^ (s1 << U(31))
    s1 = s1 ^ (s1 >> U(11))
    s0 = s0 & (s0 >> U(30))
    return (s0 ^ s1) * U(1181783497276652981)


def lobe_table():
    """csrc/hammersley.h in float32, cosf and sinf from the host's libm: (1024, 3)."""
    lm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    for name in ("cosf", "sinf"):
        getattr(lm, name).restype = ctypes.c_float
        getattr(lm, name).argtypes = [ctypes.c_float]
    i = np.arange(1024, dtype=np.uint32)
    bits = np.array([int("{:032b}".format(int(x))[::-1], 2) for x in i], np.uint32)
    xi_y = (bits.astype(np.float64) * 2.3283064365386963e-10).astype(F)
    phi = xi_y * F(2.0) * F(3.1415927)
    cp, sp = np.array([lm.cosf(float(x)) for x in phi], F), np.array([lm.sinf(float(x)) for x in phi], F)
    ct = np.sqrt(F(1.0) - i.astype(F) / F(1024))
    st = np.sqrt(F(1.0) - ct * ct)
    return np.stack([cp * st, sp * st, ct], -1)


def dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - b[:, 1] * a[:, 2], a[:, 2] * b[:, 0] - b[:, 2] * a[:, 0], a[:, 0] * b[:, 1] - b[:, 0] * a[:, 1]], -1)


def normalize(a):
    l2 = dot(a, a)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where((l2 == 0)[:, None], a, a / np.sqrt(l2)[:, None])


def tangent_to_world(n, ts):
    """csrc/dev_shade.h in float32 arrays."""
    up = np.where((np.abs(n[:, 2]) < F(0.9999))[:, None], np.array([0, 0, 1], F), np.array([1, 0, 0], F))
    tangent = normalize(cross(up, n))
    bitangent = normalize(cross(n, tangent))
    return normalize((tangent * ts[:, :1] + bitangent * ts[:, 1:2]) + n * ts[:, 2:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--points", type=int, default=18, help="log2 of the point count")
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hemi_visibility.txt"))
    a = ap.parse_args()
    import torch
    s = scenes.make_scene("terrain_1m")
    d = tempfile.mkdtemp(prefix="prt_rate_")
    scenes.write_obj(s, d, "scene.obj")
    hs = api.HostScene(d, "scene.obj", 0, s.camera_position)
    r = api.Renderer(0)
    r.upload(hs)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
    wide = "8-wide tree" if not capi.hip_lib().prt_build_flags() & capi.BUILD_BVH4 else "4-wide tree"
    n, spp, seed, bias = 1 << a.points, a.samples, 7, 1e-3
    say("hemisphere visibility on the C4 scene: %d triangles, %s; %d surface samples x %d rays = %d rays, ray_bias %g" % (
        r.scene_info().triangle_count, wide, n, spp, n * spp, bias))
    smp = r.sample_surface(n, seed=1, fields=("point", "normal"), out="torch")
    points, normals = smp["point"], smp["normal"]

    # the composition's rays, from the definition
    nrm = normals.cpu().numpy()
    j = np.repeat(np.arange(n, dtype=np.uint32), spp)
    k = (first_draws(sample_keys(seed, j, np.tile(np.arange(spp, dtype=np.uint32), n))) % U(1024)).astype(np.int64)
    dirs = tangent_to_world(np.repeat(nrm, spp, axis=0), lobe_table()[k])
    assert dirs.dtype == F
    d_dirs = torch.from_numpy(np.ascontiguousarray(dirs)).cuda()
    d_origins = points.repeat_interleave(spp, dim=0).contiguous()

    fused_all = lambda: r.hemisphere_visibility(points, normals, samples=spp, seed=seed, ray_bias=bias)                              # noqa: E731
    fused_one = lambda: r.hemisphere_visibility(points, normals, samples=spp, seed=seed, ray_bias=bias, fields=("unoccluded",))     # noqa: E731
    composed = lambda: r.trace_rays(d_origins, d_dirs, mode="occluded", ray_bias=bias)                                                # noqa: E731
    calls = (("fused, all three fields", fused_all), ("fused, unoccluded only", fused_one), ("composition (trace_rays occluded)", composed))
    first = [call() for _, call in calls]                   # the warm-up calls, and the check
    by_rays = (1 - first[2]["occluded"].reshape(n, spp).to(torch.int32)).sum(1)
    assert torch.equal(by_rays, first[0]["unoccluded"]) and torch.equal(by_rays, first[1]["unoccluded"]), "the composition's counts differ"
    u = first[0]["unoccluded"]
    say("counts equal the composition's ray by ray sums; mean visibility %.4f, %d points partly occluded, %d fully" % (
        float(first[0]["visibility"].mean()), int(((u > 0) & (u < spp)).sum()), int((u == 0).sum())))
    assert first[0]["counters"].ray_count == n * spp
    runs = {what: [] for what, _ in calls}
    for _ in range(a.reps):                                 # in turn: a drift of the machine reaches all alike
        for what, call in calls:
            runs[what].append(call()["counters"].render_ms)
    for what, _ in calls:
        ms = runs[what]
        say("%s: render_ms %s; median %.3f min %.3f max %.3f (%.0f Mrays/s at the median), over %d calls" % (
            what, ", ".join("%.3f" % x for x in ms), float(np.median(ms)), min(ms), max(ms), n * spp / float(np.median(ms)) / 1e3, a.reps))
    comp = runs[calls[2][0]]
    say("fused / composition at the medians: %.3f (all fields), %.3f (unoccluded only); the composition's own spread (max - min): %.3f ms" % (
        float(np.median(runs[calls[0][0]])) / float(np.median(comp)), float(np.median(runs[calls[1][0]])) / float(np.median(comp)), max(comp) - min(comp)))
    say("memory: fused reads %d B of points and normals and writes %d B; its scratch is 5 B per ray of a pass = %d B (flags %d B, slow list %d B); "
        "the composition reads %d B of rays and writes %d B of answers" % (24 * n, 20 * n, 5 * n * spp, n * spp, 4 * n * spp, 24 * n * spp, n * spp))
    say("result scheme: one flag byte per ray (plain stores) and k_hemi_reduce; no atomics on the outputs")
    r.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
