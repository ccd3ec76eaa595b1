#!/usr/bin/env python3
"""Surface-sampling rates (prt_sample_surface, prt_sample_surface_backward) on the C4 scene (terrain_1m).

    python tools/sample_surface_rate.py [--reps N] [--out FILE]

Device entry points (torch tensors).  2^20 samples with all five fields and with `point` alone: median, min and max of
prt_sample_info.device_ms over --reps calls each after one warm-up call, the two taken in turn.  The table: table_ms of the first
sampling call after each of --reps prt_update_geometry calls (the four launches of kernels_sample.h, on the device), and the
one-off host build of the input -> leaf table as wall time of the first call after the upload minus a later call's.  The backward
call: prt_grad_info.device_ms for 2^20 samples with point and normal gradients, QGRAD_MERGE on (the default) and off.
The lines go to stdout and to --out (default profiles/sample_surface.txt).
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_surface.txt"))
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
    say("surface samples on the C4 scene: %d triangles, %d positions, %s" % (r.scene_info().triangle_count, np.asarray(arr["positions"]).reshape(-1, 3).shape[0], wide))

    n = 1 << 20
    every = lambda: r.sample_surface(n, seed=1, out="torch")                               # noqa: E731
    point = lambda: r.sample_surface(n, seed=1, fields=("point",), out="torch")            # noqa: E731
    t0 = time.perf_counter()
    first = every()                                         # builds the input -> leaf table on the host and the prefix sums on the device
    first_wall = time.perf_counter() - t0
    t0 = time.perf_counter()
    every()
    later_wall = time.perf_counter() - t0
    info = first["info"]
    say("table: total_weight %d, unit 2^%d, %d live triangles, area %.9g; first build %.3f ms on the device" % (
        info.total_weight, info.unit_exponent, info.live_triangles, info.area, info.table_ms))
    point()
    calls = (("all five fields", every), ("point only", point))
    runs = {what: [] for what, _ in calls}
    for _ in range(a.reps):                                 # the two calls in turn: a drift of the machine reaches both alike
        for what, call in calls:
            res = call()["info"]
            assert res.table_ms == 0.0
            runs[what].append(res.device_ms)
    for what, _ in calls:
        ms = runs[what]
        say("prt_sample_surface_device, %d samples, %s: device_ms median %.3f min %.3f max %.3f (%.1f Msamples/s at the median), over %d calls" % (
            n, what, float(np.median(ms)), min(ms), max(ms), n / float(np.median(ms)) / 1e3, a.reps))

    positions = torch.from_numpy(np.ascontiguousarray(arr["positions"], np.float32).reshape(-1, 3)).cuda()
    builds = []
    for _ in range(a.reps):
        r.update_geometry(positions)
        builds.append(r.sample_surface(64, seed=1, fields=("point",), out="torch")["info"].table_ms)
    say("table_ms of the first call after prt_update_geometry (k_sample_weights, k_sample_tiles, k_sample_totals, k_sample_offsets): "
        "%s; median %.3f ms over %d updates" % (", ".join("%.3f" % b for b in builds), float(np.median(builds)), a.reps))
    say("input -> leaf table at the first call after the upload (host, once per upload): %.1f ms" % (1e3 * (first_wall - later_wall) - info.table_ms))

    smp = every()
    g_point = torch.randn((n, 3), device="cuda", dtype=torch.float32, generator=torch.Generator("cuda").manual_seed(3))
    g_normal = torch.randn((n, 3), device="cuda", dtype=torch.float32, generator=torch.Generator("cuda").manual_seed(4))
    for merge in (None, 0):
        r.set_option("QGRAD_MERGE", merge)
        back = lambda: r.sample_surface_backward(smp["group"], smp["vertex0"], smp["bw"], positions, grad_point=g_point,     # noqa: E731
                                                 grad_normal=g_normal)["info"]
        back()
        ms = [back().device_ms for _ in range(a.reps)]
        say("prt_sample_surface_backward_device, %d samples, point and normal gradients, QGRAD_MERGE %s: device_ms median %.3f min %.3f max %.3f "
            "(%.1f Msamples/s at the median), over %d calls" % (n, "default (on)" if merge is None else "off", float(np.median(ms)), min(ms), max(ms),
                                                              n / float(np.median(ms)) / 1e3, a.reps))
    r.set_option("QGRAD_MERGE", None)
    r.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
