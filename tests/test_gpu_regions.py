"""prt_get_region_stats (include/prt.h): the region table of k_pool's COUNT variants, which tools/valu_budget.py joins with
the kernel's static instruction counts.  The table must be consistent with the counters that existed before it, and counting
must not change what is rendered.
"""
from __future__ import annotations

import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, host_scene, scene_dir

pytestmark = pytest.mark.gpu


def _check(r, cam, w, h, spp, seed):
    from par_raytracer_amd import api, capi
    plain, cp = r.render(cam, api.default_params(spp, seed, pipeline=capi.PIPELINE_POOL), w, h)
    shipped_table = r.region_stats()
    img, c = r.render(cam, api.default_params(spp, seed, pipeline=capi.PIPELINE_POOL | capi.FLAG_COUNT_VISITS), w, h)
    st = r.render_stats()
    t = r.region_stats()
    # the COUNT kernel and the shipped kernel: same frame, same counts
    assert np.array_equal(img.view(np.uint32), plain.view(np.uint32))
    assert c.ray_count == cp.ray_count > 0 and c.shaded_hits == cp.shaded_hits > 0
    # a render without the flag leaves an empty table
    assert all(v == (0, 0) for v in shipped_table.values())
    # the steps that had counters before: the table's rows are those counters
    assert t["node_step"] == (st.wave_node_steps, st.node_visits) and st.wave_node_steps > 0
    assert t["tri"] == (st.wave_tri_steps, st.tri_tests) and st.wave_tri_steps > 0
    assert t["leaf"][0] == st.wave_leaf_visits
    assert 0 < t["refill"][0] <= st.wave_refills         # (wave_refills also counts a refill that found the block's shared list handed out)
    # the shade passes: the lanes that shaded a hit sum to shaded_hits, and with the misses to every entry a pass held
    assert t["shade_hit"][1] == c.shaded_hits
    assert t["shade_pass"][1] == t["shade_hit"][1] + t["shade_miss"][1]
    assert t["shade_pass"][0] >= max(t["shade_hit"][0], t["shade_miss"][0])
    # one finish block per ray a refill handed out; those are the rays of ray_count that were traced, and once more the
    # closest-hit rays that were parked (the adopting launch traces them again and does not count them again)
    traced = c.ray_count - st.elided_shadow_rays
    assert t["refill"][1] == t["finish"][1]
    assert 0 <= t["refill"][1] - traced <= st.parked_rays
    # every node step either goes down or pops, lane by lane; at wave level a step can do both
    assert t["node_descend"][0] + t["node_pop"][0] >= t["node_step"][0] >= max(t["node_descend"][0], t["node_pop"][0])
    # the bounce walk: every pass of its loop runs at least one step, every hit starts a walk
    steps = t["walk_next_child"][0] + t["walk_enter"][0] + t["walk_return_up"][0]
    assert t["walk_loop"][0] <= steps <= 3 * t["walk_loop"][0]
    assert t["walk_next_child"][1] >= c.shaded_hits
    assert t["frame_load"][1] <= t["frame_save"][1]
    assert t["walk_child_ray"][1] <= t["outputs"][1] and t["walk_child_ray"][0] <= t["shade_pass"][0]
    assert t["park"][0] <= t["finish"][0] and t["node_push"][0] <= 3 * t["node_step"][0]
    # a wave-level execution has 1..64 lanes
    for name, (n, lanes) in t.items():
        if name not in ("leaf", "node_descend", "node_pop", "node_push"):             # (rows without a lane count)
            assert n <= lanes <= 64 * n, name
    assert t["wave"][0] > 0 and t["round"][0] >= t["wave"][0]
    return t


def test_region_table_of_a_counting_render(gpu_renderer_factory):
    from par_raytracer_amd import api
    for name, w, h, spp in (("terrain_64", 160, 90, 4), ("cornell_box", 96, 96, 4)):
        s, _ = scene_dir(name)
        cam = api.make_camera(s.fov, w, h, s.camera_position, s.camera_facing)
        _check(gpu_renderer_factory(name, 0), cam, w, h, spp, 11)


_CHILD = """
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import test_gpu_regions as T
from conftest import host_scene, scene_dir
from par_raytracer_amd import api, capi
assert not (capi.hip_lib().prt_build_flags() & capi.BUILD_BVH4)
s, _ = scene_dir("terrain_64")
r = api.Renderer(0); r.upload(host_scene("terrain_64", 0))
T._check(r, api.make_camera(s.fov, 160, 90, s.camera_position, s.camera_facing), 160, 90, 4, 11)
r.close()
print("REGIONS_OK")
"""


def test_region_table_of_the_8_wide_library():
    """The same checks on libprt_hip_bvh8.so, in a process of its own (a process loads one library)."""
    lib = os.path.join(ROOT, "par_raytracer_amd", "libprt_hip_bvh8.so")
    assert os.path.exists(lib), "libprt_hip_bvh8.so not built (make hip-bvh8)"
    env = dict(os.environ)
    env["PRT_HIP_LIB"] = "libprt_hip_bvh8.so"
    p = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, os.path.join(ROOT, "tests"))], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=600)
    out = p.stdout.decode(errors="replace")
    assert p.returncode == 0 and "REGIONS_OK" in out, out[-3000:]
