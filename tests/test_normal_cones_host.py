"""Normal cones on the host (par_raytracer_amd/csrc/bvh_build.h attach_normal_cones, dev_scene.h cone_faces_away, include/prt.h
"Normal cones"): the cone in the mantissas of a 4-wide node's grid steps that lets a closest-hit ray skip a subtree whose triangles
all face away from it.  tests/normal_cones_host_harness.cpp - g++ with the address and undefined-behaviour sanitizers, the builder, the
checker and the device's traversal through tests/hip_shim - prints one line per fact; the assertions are here.

The property the images rest on: a direction the predicate accepts gives the device's own dd <= 0 on every triangle below the node,
for every origin inside the bound.  The harness checks it on and just inside the cull boundary of every coned node, and walks 21,000
rays per scene with the cones attached and with the bits cleared.  Nothing here is fitted to what the code gives: the culls and the
triangle tests are printed, and only their signs are pinned."""
import os

import numpy as np
import pytest

import harness
import lbvh_cases
from conftest import host_scene

REAL = ["terrain_64", "terrain_low_sun", "cornell_box", "icosphere_l3", "coincident"]
SMALL = ["flat_plane", "one_triangle", "five_triangles", "degenerate"]
SCENES = REAL + SMALL
FRONTS = ["sah", "radix"]


def scene_case(key):
    """(9 floats per triangle, the direction towards the light) of the case."""
    if key == "flat_plane":                                  # 2 triangles, every normal equal
        return np.array([[-1, 0, -1, -1, 0, 1, 1, 0, -1], [1, 0, -1, -1, 0, 1, 1, 0, 1]], np.float32), np.array([0.3, 1.0, 0.2], np.float32)
    if key == "one_triangle":
        return np.array([[0, 0, 0, 0, 0.5, 1, 1, 0.25, 0]], np.float32), np.array([0.0, 1.0, 0.0], np.float32)
    if key == "five_triangles":                              # the smallest tree with an inner child
        t = np.array([[0, 0, 0, 0, 0.1, 1, 1, 0, 0]], np.float32)
        return np.concatenate([t + np.float32(2 * k) * np.array([1, 0.05 * k, 0] * 3, np.float32) for k in range(5)]), np.array([0.2, 1.0, 0.1], np.float32)
    if key == "degenerate":                                  # a zero-area triangle, and a triangle with a NaN vertex
        v = np.array([[0, 0, 0, 0, 0, 1, 1, 0, 0], [2, 0, 0, 2, 0, 1, 3, 0.2, 0], [1, 1, 1, 1, 1, 1, 1, 1, 1], [4, 0, 0, 4, 0, 1, 5, 0, 0],
                      [6, 0, 0, 6, 0, 1, 7, 0.1, 0], [8, 0, 0, 8, 0, 1, 9, 0, 0]], np.float32)
        v[3, 4] = np.nan
        return v, np.array([0.0, 1.0, 0.0], np.float32)
    from par_raytracer_amd import api, capi
    a = api.desc_arrays(host_scene("terrain_64" if key == "terrain_low_sun" else key, 0).desc)
    verts = a["positions"].reshape(-1, 3)[a["idx_positions"]].reshape(-1, 9).astype(np.float32)
    sun = capi.PrtLight.from_buffer_copy(a["lights"][:48].tobytes())
    facing = np.array([sun.facing[0], sun.facing[1], sun.facing[2]], dtype=np.float32)
    if sun.type != 0:                                        # a point light: towards it from the origin
        facing = -np.array([sun.position[0], sun.position[1], sun.position[2]], dtype=np.float32)
    if key == "terrain_low_sun":                             # the sun 7 degrees above the horizon (tests/test_gpu_shadow_trees.py)
        facing = (np.array([1.0, -0.12, 0.25]) / np.linalg.norm([1.0, -0.12, 0.25])).astype(np.float32)
    return verts, facing * np.float32(-1.0)


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    d = tmp_path_factory.mktemp("normal_cones")
    cases = os.path.join(str(d), "cases.bin")
    with open(cases, "wb") as f:
        harness.put(f, ([len(SCENES)], np.uint32))
        for key in SCENES:
            verts, direction = scene_case(key)
            f.write(key.encode().ljust(32, b"\0"))
            harness.put(f, ([len(verts)], np.uint32), (direction, np.float32), (verts, np.float32))
            radix = bool(np.all(np.isfinite(verts)))         # the radix front end takes finite soups only (the upload refuses the rest)
            harness.put(f, ([1 if radix else 0], np.uint32))
            if radix:
                r = lbvh_cases.reference(lbvh_cases.soup(verts.reshape(-1, 3)))
                harness.put(f, (r["left"], np.int32), (r["right"], np.int32), (r["first"], np.uint32), (r["last"], np.uint32),
                            (r["node_box"], np.float32), (r["leaf_box"], np.float32), (r["sorted_ids"], np.uint32))
    exe = harness.build("normal_cones_host_harness.cpp", d, "nc", sanitize=True, sources=("bvh_build.cpp", "bvh_check.cpp"), flags=("-O2",))
    out = harness.run(exe, cases, timeout=600).splitlines()
    print("\n".join(out))                                    # the recorded counts (pytest -s shows them)
    return out


def pick(lines, what, scene, front):
    got = [ln for ln in lines if ln.startswith("%s %s %s |" % (what, scene, front))]
    assert len(got) == 1, "%d lines start with %r" % (len(got), (what, scene, front))
    words = got[0].split("|", 1)[1].replace("->", " ").split()
    out, k = {}, 0
    while k < len(words):                                    # name value [value]
        vals = []
        j = k + 1
        while j < len(words) and words[j].lstrip("-").isdigit():
            vals.append(int(words[j]))
            j += 1
        out[words[k]] = vals[0] if len(vals) == 1 else tuple(vals)
        k = j
    return out


def fronts_of(scene):
    return ["sah"] if scene == "degenerate" else FRONTS


CASES = [(s, fe) for s in SCENES for fe in fronts_of(s)]


@pytest.mark.parametrize("scene,front", CASES)
def test_no_accepted_direction_meets_a_front_face_below_its_node(lines, scene, front):
    f = pick(lines, "soundness", scene, front)
    assert f["violations"] == 0, f
    c = pick(lines, "cones", scene, front)
    assert f["nodes"] == c["coned"] == c["coned_seen"], (f, c)
    if c["coned"]:
        assert f["directions"] >= 32 * f["nodes"] and f["accepted"] >= 16 * f["nodes"] and f["dd_tests"] > 0, f
    if scene in ("terrain_64", "terrain_low_sun", "icosphere_l3", "flat_plane", "five_triangles"):
        assert c["coned"] > 0, c
    # the direction perpendicular to the widest normal, and the accepted direction nearest to it, wherever a node's normals differ
    assert f["towards_perpendicular"] <= f["perpendicular"] <= f["nodes"], f
    if scene in ("terrain_64", "terrain_low_sun", "icosphere_l3"):
        assert f["perpendicular"] == f["nodes"] and f["towards_perpendicular"] >= 0.9 * f["nodes"], f


@pytest.mark.parametrize("scene,front", CASES)
def test_rays_find_the_same_hits_with_and_without_cones(lines, scene, front):
    f = pick(lines, "rays", scene, front)
    assert f["rays"] >= 20000 and f["mismatches"] == 0, f
    assert f["tiny_component"] > 0 and f["axis_parallel"] > 0, f
    assert f["nocone_culls"] == 0 and f["nocone_differs"] == 0, f          # the no-cone bit
    assert f["any_culls"] == 0 and f["any_differs"] == 0, f                # any-hit rays are exempt
    for cls in ("primary", "bounce", "shadow"):
        off, on = f["tris_" + cls]
        assert on <= off, (cls, f)
    if scene in ("terrain_64", "terrain_low_sun", "icosphere_l3"):
        assert f["hits"] > 0 and f["culls_primary"] + f["culls_bounce"] + f["culls_shadow"] > 0, f
        assert f["tris_bounce"][1] < f["tris_bounce"][0] and f["nodes_bounce"][1] <= f["nodes_bounce"][0], f


@pytest.mark.parametrize("scene,front", CASES)
def test_zero_words_and_nan_and_null_directions_never_cull(lines, scene, front):
    f = pick(lines, "bits", scene, front)
    assert f["zero_word_culls"] == 0 and f["nan_culls"] == 0 and f["zero_length_culls"] == 0, f


@pytest.mark.parametrize("scene,front", CASES)
def test_the_checker_counts_cone_violations_and_a_refit_clears_the_cone(lines, scene, front):
    c = pick(lines, "cones", scene, front)
    assert c["violations"] == 0 and c["box_violations"] == 0 and c["rest_same"] == 1, c
    if c["coned"]:
        assert c["flipped_violations"] > 0 and c["refit_cleared"] == 1, c


@pytest.mark.parametrize("scene,front", CASES)
def test_the_bits_do_not_depend_on_the_thread_count(lines, scene, front):
    assert pick(lines, "cones", scene, front)["threads_same"] == 1


def test_a_bad_normal_below_a_node_leaves_it_without_a_cone(lines):
    c = pick(lines, "cones", "degenerate", "sah")
    assert 0 < c["coned"] < c["nodes"], c                    # the root holds the NaN normal; a subtree without it keeps its cone


def test_the_c_abi_reports_the_cones():
    import ctypes as C
    from par_raytracer_amd import capi
    lib = capi.hip_lib()
    out = (C.c_uint64 * 2)()
    assert lib.prt_debug_check_cones(host_scene("terrain_64", 0).desc, out) == 0
    assert out[0] == 0 and out[1] > 0
    assert capi.PrtRenderStats.cone_culled_nodes.offset == capi.PrtRenderStats.open_shadow_rays.offset + 8
    assert C.sizeof(capi.PrtNormalConeInfo) == 16 and lib.prt_abi_version() == 5
