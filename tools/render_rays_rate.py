#!/usr/bin/env python3
"""prt_render_rays_device against prt_render_device on the frame both can make: the C4 scene (terrain_1m),
1920x1080, 8 spp.

    python tools/render_rays_rate.py [--reps N] [--width W --height H --spp S] [--parent-lib libprt_hip_parent.so] [--out FILE]

The frame's 16.6 M camera rays are made here in numpy from the definition - the key of include/prt_key.h, the generator's first two
draws (csrc/dev_rng.h), RenderPixel's jitter, cameras.pinhole_rays - and lie on the device as 24 bytes each.
  rays      prt_render_rays_device on them with PRT_RAYS_CAMERA_STREAM: prt_counters.render_ms (the domain check included).
  camera    prt_render_device of the same frame with PRT_PIPELINE_WAVEFRONT: prt_counters.render_ms.
First the two images are compared: they must be the same bits, with the same ray_count (asserted).  Then --reps calls each after a
warm-up call, taken in turn; the series, medians and the spread go to stdout and to --out (default profiles/render_rays.txt).
--parent-lib names a build of an earlier commit's library inside the package directory (PRT_HIP_LIB): a child process renders the
same frame with its prt_render_device, --reps calls after a warm-up, before and after this process's series; its image must be
the same bits too.  The requirement - the new call's median is at most a camera series' median plus that series' own max - min - is
stated against every series of five.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from par_raytracer_amd import api, cameras, capi, scenes  # noqa: E402

U = np.uint64
F = np.float32
SEED = 1234


def sample_keys(seed, pixel, s):
    """include/prt_key.h on uint64 arrays (the arithmetic wraps)."""
    z = U(seed) + U(0x9E3779B97F4A7C15) * (((pixel.astype(U) << U(16)) | s.astype(U)) + U(1))
    z = (z ^ (z >> U(30))) * U(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> U(27))) * U(0x94D049BB133111EB)
    return z ^ (z >> U(31))


def first_two_float11(key):
    """The reference generator seeded with `key` (csrc/dev_rng.h): NextFloat11 of its first two draws."""
    def chain_step(x):
        x = x ^ (x >> U(12))
        x = x ^ (x >> U(25))
        return x ^ (x >> U(27))
    mul = U(2685821657736338717)
    key = np.where(key == U(0), U(0x5555555555555555), key)
    chain = chain_step(key)
    prev = chain * mul
    out = []
    for _ in range(2):
        chain = chain_step(chain)
        s1 = chain * mul
        s1 = s1 ^ (s1 << U(31))
        s1 = s1 ^ (s1 >> U(11))
        s0 = prev & (prev >> U(30))
        prev = s0 ^ s1
        v = (prev * U(1181783497276652981)).astype(F) * F(2.0 ** -64)
        out.append(np.clip(v, F(0), F(1)) * F(2.0) - F(1.0))
    return out


def frame_rays(cam, width, height, spp, seed):
    """RenderPixel's rays (main.cpp:237-240) of the whole frame: (origins, directions), (width * height * spp, 3) float32."""
    n = width * height
    pixel = np.repeat(np.arange(n, dtype=np.uint32), spp)
    samp = np.tile(np.arange(spp, dtype=np.uint32), n)
    off_y, off_x = first_two_float11(sample_keys(seed, pixel, samp))             # the first draw lands in .y
    xy = np.stack([(pixel % np.uint32(width)).astype(F) + off_x * F(0.5), (pixel // np.uint32(width)).astype(F) + off_y * F(0.5)], -1)
    return cameras.pinhole_rays(cam, xy)


def make_frame(a):
    s = scenes.make_scene("terrain_1m")
    d = tempfile.mkdtemp(prefix="prt_rate_")
    scenes.write_obj(s, d, "scene.obj")
    hs = api.HostScene(d, "scene.obj", 0, s.camera_position)
    cam = api.make_camera(s.fov, a.width, a.height, s.camera_position, s.camera_facing)
    r = api.Renderer(0)
    r.upload(hs)
    return r, cam


def camera_series(r, cam, a, out):
    """1 + reps calls of prt_render_device (wavefront); returns the series after the warm-up."""
    import torch
    p = api.default_params(a.spp, SEED, pipeline=capi.PIPELINE_WAVEFRONT)
    ms = []
    for _ in range(a.reps + 1):
        torch.cuda.synchronize()
        ms.append(r.render_device(cam, p, a.width, a.height, 0, a.width * a.height, out.data_ptr()).render_ms)
    return ms[1:]


def child(a):
    """--parent-lib's process: this commit's Python over the named library."""
    import torch
    r, cam = make_frame(a)
    out = torch.zeros((a.width * a.height, 4), dtype=torch.float32, device="cuda:0")
    ms = camera_series(r, cam, a, out)
    print("CHILD " + json.dumps({"render_ms": ms, "sha": hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest(),
                                 "lib": os.path.basename(capi.hip_lib()._name)}), flush=True)
    r.close()


def run_child(a):
    env = dict(os.environ)
    env["PRT_HIP_LIB"] = a.parent_lib
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--width", str(a.width), "--height", str(a.height),
           "--spp", str(a.spp)]
    proc = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    if proc.returncode != 0:
        raise RuntimeError("the --parent-lib process failed (%d): %s" % (proc.returncode, proc.stderr.decode()[-2000:]))
    line = [x for x in proc.stdout.decode().splitlines() if x.startswith("CHILD ")][-1]
    return json.loads(line[6:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_rays.txt"))
    a = ap.parse_args()
    if a.child:
        return child(a)
    import torch
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
    before = run_child(a) if a.parent_lib else None
    r, cam = make_frame(a)
    n, spp = a.width * a.height, a.spp
    wide = "8-wide tree" if not capi.hip_lib().prt_build_flags() & capi.BUILD_BVH4 else "4-wide tree"
    say("radiance along caller rays on the C4 scene: %d triangles, %s; %dx%d x %d spp = %d rays (%d MB of rays on the device)" % (
        r.scene_info().triangle_count, wide, a.width, a.height, spp, n * spp, 24 * n * spp >> 20))
    o, d = frame_rays(cam, a.width, a.height, spp, SEED)
    d_o, d_d = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    del o, d
    p_rays = api.default_params(spp, SEED)
    out = torch.zeros((n, 4), dtype=torch.float32, device="cuda:0")
    image, c_rays = r.render_rays(d_o, d_d, p_rays, first=0, camera_stream=True)                 # warm-up, and the check
    c_cam = r.render_device(cam, api.default_params(spp, SEED, pipeline=capi.PIPELINE_WAVEFRONT), a.width, a.height, 0, n, out.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(image.view(torch.int32), out.view(torch.int32)), "the two images differ"
    assert c_rays.ray_count == c_cam.ray_count and c_rays.shaded_hits == c_cam.shaded_hits
    sha = hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest()
    say("identity: prt_render_rays_device(camera rays, PRT_RAYS_CAMERA_STREAM) and prt_render_device(WAVEFRONT) give the same bits "
        "(sha256 %s...), ray_count %d and shaded_hits %d" % (sha[:16], c_rays.ray_count, c_rays.shaded_hits))
    runs = {"rays": [], "camera": []}
    pw = api.default_params(spp, SEED, pipeline=capi.PIPELINE_WAVEFRONT)
    for _ in range(a.reps):                                 # in turn: a drift of the machine reaches both alike
        runs["rays"].append(r.render_rays(d_o, d_d, p_rays, first=0, camera_stream=True)[1].render_ms)
        torch.cuda.synchronize()
        runs["camera"].append(r.render_device(cam, pw, a.width, a.height, 0, n, out.data_ptr()).render_ms)
    r.close()
    after = run_child(a) if a.parent_lib else None

    def show(what, ms):
        say("%s: render_ms %s; median %.3f min %.3f max %.3f (%.0f Mrays/s at the median)" % (
            what, ", ".join("%.3f" % x for x in ms), float(np.median(ms)), min(ms), max(ms), c_rays.ray_count / float(np.median(ms)) / 1e3))
    show("prt_render_rays_device (this library)", runs["rays"])
    show("prt_render_device, WAVEFRONT (this library, taken in turn)", runs["camera"])
    series = [("this library's camera path, taken in turn", runs["camera"])]
    if a.parent_lib:
        for when, c in (("before", before), ("after", after)):
            assert c["sha"] == sha, "the image of %s differs" % a.parent_lib
            show("prt_render_device, WAVEFRONT (%s, its own process, %s)" % (c["lib"], when), c["render_ms"])
            series.append(("%s, %s" % (c["lib"], when), c["render_ms"]))
        say("the images of %s are the same bits" % a.parent_lib)
    med = float(np.median(runs["rays"]))
    for what, ref in series:                                # every series of five is its own yardstick: median + (max - min)
        bound = float(np.median(ref)) + (max(ref) - min(ref))
        say("requirement against %s: median %.3f ms <= %.3f + %.3f = %.3f ms: %s (the new call costs %+.3f ms)" % (
            what, med, float(np.median(ref)), max(ref) - min(ref), bound, "met" if med <= bound else "MISSED", med - float(np.median(ref))))
    say("extra work of the new call: %d B of rays read by the check kernel and again by ray generation" % (24 * n * spp))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
