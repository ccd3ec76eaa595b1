#!/usr/bin/env python3
"""What a geometry update costs and what a refitted tree costs to traverse (prt_update_geometry), on the C4 scene
(terrain_1m).

    python tools/refit_rate.py [--reps N] [--parent-lib libprt_hip_parent.so] [--out profiles/r07_refit.txt]

For both builders (BVH_BUILDER sah, lbvh) and two moves - a small displacement (1 % of the extent, along y) and a large one (x
scaled by 3) -:
1. the update: prt_update_info.device_ms and the wall time of the call (median of --reps), against the wall time of a fresh
   prt_upload_scene of the same moved scene.  --parent-lib names a library of the PARENT commit inside par_raytracer_amd/ (build
   it there with `make hip` and copy it); its upload is then timed in a child process (PRT_HIP_LIB), which is the fair
   yardstick.  Without it the upload of this library is timed, and the output says so.
2. a C4 frame (1920 x 1080, 8 spp) on the refitted tree against the fresh tree: render_ms (median of --reps) and node_visits.
   The two frames must be bit-equal; the tool checks that too.
The moved scenes carry no sphere hierarchy (spheres NULL on both sides).  Output goes to stdout and to --out."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from par_raytracer_amd import api, capi, scenes  # noqa: E402

W, H, SPP = 1920, 1080, 8


def scene_arrays():
    s = scenes.make_scene("terrain_1m")
    d = tempfile.mkdtemp(prefix="prt_refit_rate_")
    scenes.write_obj(s, d, "scene.obj")
    hs = api.HostScene(d, "scene.obj", 0, s.camera_position)
    a = api.desc_arrays(hs.desc)
    a["spheres"], a["sphere_group"] = np.zeros(0, np.uint8), np.zeros(0, np.int32)
    return s, a


def move(a, cam_pos, which):
    P = a["positions"].reshape(-1, 3).copy()
    cam = np.array(cam_pos, np.float32)
    ext = float((P.max(0) - P.min(0)).max())
    if which == "small":
        P[:, 1] += np.float32(0.01 * ext) * np.sin(P[:, 0] * np.float32(40.0 / ext) + P[:, 2] * np.float32(25.0 / ext))
    else:
        P[:, 0] *= np.float32(3.0)
        cam[0] *= np.float32(3.0)
    return np.ascontiguousarray(P.reshape(-1).astype(np.float32)), cam


def time_upload(a, positions, builder, reps):
    r = api.Renderer(0)
    if builder != "sah":
        r.set_option("BVH_BUILDER", builder)
    fd = api.FlatDesc(dict(a, positions=positions))
    ts = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        r.upload(fd)
        ts.append((time.perf_counter() - t0) * 1e3)
    r.close()
    return float(np.median(ts[1:]))


def child(args):
    s, a = scene_arrays()
    out = {}
    for which in ("small", "large"):
        P, _ = move(a, s.camera_position, which)
        for builder in ("sah", "lbvh"):
            out["%s/%s" % (builder, which)] = time_upload(a, P, builder, args.reps)
    print("UPLOAD_MS " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_refit.txt"))
    ap.add_argument("--child-upload", action="store_true")
    args = ap.parse_args()
    if args.child_upload:
        return child(args)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    parent_ms = None
    if args.parent_lib:
        env = dict(os.environ, PRT_HIP_LIB=args.parent_lib)
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-upload", "--reps", str(args.reps)], env=env,
                             stdout=subprocess.PIPE, check=True).stdout.decode()
        parent_ms = json.loads([ln for ln in out.splitlines() if ln.startswith("UPLOAD_MS ")][-1][len("UPLOAD_MS "):])
    s, a = scene_arrays()
    say("terrain_1m: %d triangles, %s; fresh upload timed on %s" % (
        a["idx_positions"].size // 3, "8-wide tree" if not capi.hip_lib().prt_build_flags() & capi.BUILD_BVH4 else "4-wide tree",
        "the parent commit's library (%s)" % args.parent_lib if parent_ms else "THIS library (no --parent-lib given)"))
    p = api.default_params(SPP, 1234)
    p_cnt = api.default_params(SPP, 1234, pipeline=capi.FLAG_COUNT_VISITS)
    for builder in ("sah", "lbvh"):
        for which in ("small", "large"):
            P, cam_pos = move(a, s.camera_position, which)
            cam = api.make_camera(s.fov, W, H, [float(v) for v in cam_pos], s.camera_facing)
            ra, rb = api.Renderer(0), api.Renderer(0)
            if builder != "sah":
                ra.set_option("BVH_BUILDER", builder)
                rb.set_option("BVH_BUILDER", builder)
            ra.upload(api.FlatDesc(a))
            dev, wall = [], []
            for k in range(args.reps + 1):                 # (the first call builds the table: reported apart)
                t0 = time.perf_counter()
                info = ra.update_geometry(P)
                wall.append((time.perf_counter() - t0) * 1e3)
                dev.append(info.device_ms)
            up = parent_ms["%s/%s" % (builder, which)] if parent_ms else time_upload(a, P, builder, args.reps)
            say("%s, %s move: update device %.3f ms, wall %.3f ms (first call, with the table: %.1f ms), %d levels, %d nodes; fresh upload %.1f ms wall" % (
                builder, which, float(np.median(dev[1:])), float(np.median(wall[1:])), wall[0], info.levels, info.node_count, up))
            rb.upload(api.FlatDesc(dict(a, positions=P)))
            res = {}
            for tag, r in (("refitted", ra), ("fresh", rb)):
                r.render(cam, p, W, H)
                runs = [r.render(cam, p, W, H) for _ in range(args.reps)]
                img, c = r.render(cam, p_cnt, W, H)
                res[tag] = (float(np.median([c2.render_ms for _, c2 in runs])), c.node_visits, c.tri_tests, img, c.ray_count)
            same = np.array_equal(res["refitted"][3].view(np.uint32), res["fresh"][3].view(np.uint32)) and res["refitted"][4] == res["fresh"][4]
            say("    C4 frame: refitted %.3f ms, %d node visits, %d triangle tests; fresh %.3f ms, %d node visits, %d triangle tests; frames %s" % (
                res["refitted"][0], res["refitted"][1], res["refitted"][2], res["fresh"][0], res["fresh"][1], res["fresh"][2],
                "bit-equal" if same else "DIFFER"))
            ra.close()
            rb.close()
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
