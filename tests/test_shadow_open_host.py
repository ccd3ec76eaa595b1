"""Open triangles on the host (par_raytracer_amd/csrc/bvh_build.h, include/prt.h "Open triangles"): the per-light flag that lets
a render count a directional light's shadow ray and credit it at the hit instead of tracing it.
tests/shadow_open_host_harness.cpp - g++, bvh_build.cpp and the device's triangle test through tests/hip_shim, once per tree width -
calls the functions the upload calls and prints one line per fact; the assertions are here.

The property the images rest on: a shadow ray that starts on an open triangle hits nothing.  The harness checks it by brute force
for EVERY open triangle of every scene - origins at the corners, edge midpoints and centroid and a few ulp outside each edge and
corner, pushed as the renderer pushes a hit with ray_bias at +bound, -bound, 0 and the reference's default 1e-3, each tested
against all triangle records with the reference's triangle test.  Nothing here is fitted to what the code gives: the shares of
open triangles are printed, not pinned."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import harness
from conftest import ROOT, host_scene

WIDTHS = [4, 8]
SCENES = ["terrain_64", "terrain_low_sun", "cornell_box", "icosphere_l3", "coincident"]


def scene_case(key):
    """(9 floats per triangle, d = facing * -1 of the scene's first light) as prt_upload_scene sees them."""
    from par_raytracer_amd import api, capi
    a = api.desc_arrays(host_scene("terrain_64" if key == "terrain_low_sun" else key, 0).desc)
    verts = a["positions"].reshape(-1, 3)[a["idx_positions"]].reshape(-1, 9).astype(np.float32)
    sun = capi.PrtLight.from_buffer_copy(a["lights"][:48].tobytes())
    assert sun.type == 0
    facing = np.array([sun.facing[0], sun.facing[1], sun.facing[2]], dtype=np.float32)
    if key == "terrain_low_sun":                        # the sun 7 degrees above the horizon (tests/test_gpu_shadow_trees.py)
        facing = (np.array([1.0, -0.12, 0.25]) / np.linalg.norm([1.0, -0.12, 0.25])).astype(np.float32)
    return verts, facing * np.float32(-1.0)


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    d = tmp_path_factory.mktemp("shadow_open")
    cases = os.path.join(str(d), "cases.bin")
    with open(cases, "wb") as f:
        harness.put(f, ([len(SCENES)], np.uint32))
        for key in SCENES:
            verts, direction = scene_case(key)
            f.write(key.encode().ljust(32, b"\0"))
            harness.put(f, ([len(verts)], np.uint32), (direction, np.float32), (verts, np.float32))
    out = {}
    for width in WIDTHS:
        exe = harness.build("shadow_open_host_harness.cpp", d, "so%d" % width, bvh8=width == 8, sources=("scene_pack.cpp", "bvh_build.cpp", "bvh_check.cpp"), flags=("-O2",))
        out[width] = harness.run(exe, cases, timeout=300).splitlines()
    print("\n".join(ln for ln in out[4] if ln.startswith(("flags", "brute"))))          # the recorded shares (pytest -s shows them)
    return out


def fields(line):
    words = line.split("|", 1)[1].split()
    return dict(zip(words[0::2], words[1::2]))


def pick(lines, prefix):
    got = [ln for ln in lines if ln.startswith(prefix)]
    assert len(got) == 1, "%d lines start with %r" % (len(got), prefix)
    return fields(got[0])


@pytest.mark.parametrize("scene", SCENES)
@pytest.mark.parametrize("width", WIDTHS)
def test_no_shadow_ray_from_an_open_triangle_hits_anything(lines, width, scene):
    f = pick(lines[width], "brute %s width %d |" % (scene, width))
    assert int(f["hits"]) == 0, f
    assert int(f["origins"]) == 13 * 4 * int(f["open"]), f
    # the check is able to see a hit: shadow rays from triangles that are not open do get occluded, where the scene has shadows
    if scene in ("terrain_64", "terrain_low_sun"):
        assert int(f["closed_tried"]) > 0 and int(f["closed_hits"]) > 0, f


@pytest.mark.parametrize("scene", SCENES)
def test_the_flags_do_not_depend_on_the_tree_width_or_the_threads(lines, scene):
    a, b = (pick(lines[w], "flags %s width %d |" % (scene, w)) for w in WIDTHS)
    assert a["hash"] == b["hash"] and a["open"] == b["open"] and a["occluders"] == b["occluders"]
    assert a["threads_agree"] == b["threads_agree"] == "1"


@pytest.mark.parametrize("scene", SCENES)
@pytest.mark.parametrize("width", WIDTHS)
def test_no_occluder_and_no_twin_of_an_occluder_is_open(lines, width, scene):
    """An occluder overlaps itself; a face that shares its three corners with an occluder (exported twice, or flipped) lies in
    that occluder's plane, on top of it."""
    f = pick(lines[width], "sanity %s width %d |" % (scene, width))
    assert int(f["occluders_open"]) == 0 and int(f["twins_open"]) == 0, f
    g = pick(lines[width], "flags %s width %d |" % (scene, width))
    assert int(g["facing_open"]) == int(g["open"]) <= int(g["facing"]), g       # only triangles that face the light are open


@pytest.mark.parametrize("scene", ["terrain_64", "terrain_low_sun"])
def test_both_terrains_have_open_and_shadowed_triangles(lines, scene):
    """The shares are recorded in the test's output, not pinned: some light-facing triangles are open, some are not."""
    f = pick(lines[4], "flags %s width 4 |" % scene)
    print("%s: %s of %s light-facing triangles open (%.1f %%)" % (scene, f["facing_open"], f["facing"], 100.0 * int(f["facing_open"]) / int(f["facing"])))
    assert 0 < int(f["facing_open"]) < int(f["facing"]), f


def test_the_bias_bound_covers_the_default_ray_bias_on_every_scene(lines):
    for scene in SCENES:
        f = pick(lines[4], "flags %s width 4 |" % scene)
        assert float(f["bias_max"]) >= 1e-3 and float(f["bias_max"]) == float(f["abs_max"]) / 2048.0 and float(f["reach"]) == 2.0 * float(f["abs_max"]), f


def test_inputs_outside_the_margins_argument_stay_unflagged(lines):
    tri = {ln.split()[1]: fields(ln) for ln in lines[4] if ln.startswith("margin ")}
    assert tri["plain"]["open"] == "1"                                   # the set-up can flag a triangle
    for name in ("zero_area_point", "zero_area_line", "sliver", "tiny", "inf_corner", "nan_corner", "beyond_extent"):
        assert tri[name]["open"] == "0", (name, tri[name])
    assert all(f["occluder_open"] == "0" for f in tri.values())
    # a flipped copy on top of a light-facing triangle is an occluder in its plane: not open; with the copy aside it is
    assert tri["flipped_twin"]["open"] == "0" and tri["flipped_twin"]["occluders"] == "1"
    assert tri["flipped_copy_aside"]["open"] == "1" and tri["flipped_copy_aside"]["occluders"] == "1"
    bounds = {ln.split()[1]: fields(ln) for ln in lines[4] if ln.startswith("bounds ")}
    assert bounds["good"]["open"] == "1"
    for name in ("huge_extent", "extent_2_pow_14", "nan_extent", "negative_bias", "nan_bias", "zero_reach", "inf_reach", "zero_direction",
                 "nan_direction", "huge_direction", "empty_set"):
        assert bounds[name]["open"] == "0", (name, bounds[name])


def test_the_getter_the_option_and_the_stats_field_are_declared_and_bound():
    from par_raytracer_amd import capi
    assert "prt_get_shadow_open" in capi.PRT_SYMBOLS and hasattr(capi.hip_lib(), "prt_get_shadow_open")
    assert capi.PrtShadowOpenInfo.classify_ms.offset == 16 and C.sizeof(capi.PrtShadowOpenInfo) == 32 and capi.PrtRenderStats.open_shadow_rays.offset == capi.PrtRenderStats.stack_bound.offset + 4
    with open(os.path.join(ROOT, "include", "prt.h")) as f:
        header = f.read()
    assert re.search(r"int prt_get_shadow_open\(const prt_ctx \* ctx, prt_shadow_open_info \* out, uint32_t cap\);", header)
    assert re.search(r"uint64_t open_shadow_rays;", header)
    with open(os.path.join(ROOT, "par_raytracer_amd", "csrc", "prt_options.h")) as f:
        assert '"SHADOW_OPEN"' in f.read()
