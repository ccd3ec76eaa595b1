"""bench.py without --full: only the headline is measured, and --dump-outputs writes what the timed path computed.

The dumped frame of the last timed step must be the frame prt_render gives for the same scene, camera and parameters, bit
for bit, with the same ray count: two builds of the project can then be compared output for output.
"""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import scene_dir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_bench_run_dumps_the_last_timed_frame(tmp_path, gpu_renderer_factory):
    from par_raytracer_amd import api
    import bench

    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "tiny", "--steps", "3",
                          "--warmup", "1", "--dump-outputs", str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0, out.stderr.decode()[-3000:]
    line = json.loads(out.stdout.decode().strip().splitlines()[-1])
    assert line["full"] is False and line["steps"] == 3 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["unit"] == "Mrays/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["roofline"] is None and line["cpu_baseline"] is None and line["parity"] is None
    assert line["extra"] == {"other_workloads": None, "two_frames_in_flight_one_gpu": None}
    assert sorted(os.listdir(tmp_path)) == ["framebuffer.npy", "ray_count.npy"]

    scene_name, w, h, spp, depth, _ = bench.WORKLOADS["tiny"]
    s, _ = scene_dir(scene_name)
    r = gpu_renderer_factory(scene_name)
    cam = api.make_camera(s.fov, w, h, s.camera_position, s.camera_facing)
    img, ctr = r.render(cam, api.default_params(spp, bench.SEED, bounce_depth=depth), w, h)
    fb = np.load(tmp_path / "framebuffer.npy")
    rays = np.load(tmp_path / "ray_count.npy")
    assert fb.dtype == np.float32 and fb.shape == (h, w, 4) and rays.dtype == np.float64
    assert np.array_equal(fb.view(np.uint32), img.reshape(h, w, 4).view(np.uint32))
    assert rays.tolist() == [float(ctr.ray_count)] and line["config"]["rays_per_frame"] == ctr.ray_count
