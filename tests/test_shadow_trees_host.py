"""Shadow trees on the host (par_raytracer_amd/csrc/bvh_build.h, include/prt.h "Shadow trees"): the classification of the
triangles a directional light's shadow rays can hit, and the trees prt_upload_scene appends behind the scene's for them.
tests/shadow_trees_host_harness.cpp - g++, scene_pack.cpp + bvh_build.cpp + bvh_check.cpp + the device traversal through
tests/hip_shim, both tree widths - calls the function the upload calls (pack_scene) and prints one line per fact; the assertions are here.

The exclusion property is the one the images rest on: a triangle may be left out only if the device's own expression
dd = Dot(o - (o + d), n) is <= 0 for every origin a render can produce.  The bound is derived in DESIGN.md section 2; nothing
here is fitted to what the code gives - the harness evaluates the device expression itself, in float, on origins inside the
bounds, on the surface, 4 x outside, at the bound and next to powers of two, for the scene at 2^-20 .. 2^20 times its size, the
scales 2^10 and 2^14 among them, where the rounding of o + d decides who stays; and on synthetic normals swept through the margin
itself with origins at the bound.  The normal is always the one read back out of the record, as the upload classifies it."""
import os
import re

import pytest

import harness
from harness import ROOT

WIDTHS = [4, 8]


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    out = {}
    for width in WIDTHS:
        exe = harness.build("shadow_trees_host_harness.cpp", tmp_path_factory.mktemp("shadow_trees"), "st%d" % width, bvh8=width == 8,
                            sources=("scene_pack.cpp", "bvh_build.cpp", "bvh_check.cpp"))
        out[width] = harness.run(exe, timeout=120).splitlines()
    return out


def fields(line):
    """'k v k v ...' after the bar -> dict (values stay strings)."""
    words = line.split("|", 1)[1].split()
    return dict(zip(words[0::2], words[1::2]))


def pick(lines, prefix):
    got = [ln for ln in lines if ln.startswith(prefix)]
    assert got, "no line starts with %r" % prefix
    return got


@pytest.mark.parametrize("scale", [-20, 0, 10, 14, 17, 20])
@pytest.mark.parametrize("light", ["sun", "low", "axis"])
@pytest.mark.parametrize("width", WIDTHS)
def test_no_excluded_triangle_can_ever_pass_the_devices_facing_test(lines, width, light, scale):
    (ln,) = pick(lines[width], "exclusion %s scale 2^%d |" % (light, scale))
    f = fields(ln)
    assert int(f["violations"]) == 0, ln
    if scale <= 14:
        # the rule must be doing something where the float expression still sees the direction: most of a terrain lit from
        # above faces its light
        assert int(f["excluded"]) > int(f["triangles"]) // 2 and int(f["origins"]) >= 64 * int(f["excluded"]), ln
    else:
        # from 2^17 times the size on, o + d rounds d away (32 extents are 2^24 and more: an ulp of such an origin is 1 and more):
        # nothing is provable, everything stays
        assert int(f["excluded"]) == 0, ln
    if scale in (10, 14):
        # here the margin's M-dependent term decides membership: some of the triangles left out would stay were it 4 x larger,
        # so these scales pass on the strength of u (M + 2 D) and its constant 32 A, not beside it
        assert int(f["decided"]) > 0, ln


@pytest.mark.parametrize("M", ["128", "22656", "4e+06"])
@pytest.mark.parametrize("light", ["sun", "low", "axis"])
@pytest.mark.parametrize("width", WIDTHS)
def test_normals_swept_through_the_margin_with_origins_at_the_bound(lines, width, light, M):
    (ln,) = pick(lines[width], "margin %s M %s |" % (light, M))
    f = fields(ln)
    # the boundary lies inside the sweep (both verdicts occur), no normal that was left out passes the device's test at +-M, and
    # the sweep reaches normals that do pass it (so the origins are able to show a violation)
    assert int(f["excluded"]) > 300 and int(f["kept"]) > 300 and int(f["origins"]) == 64 * int(f["excluded"]), ln
    assert int(f["violations"]) == 0, ln
    assert int(f["kept_alive"]) > 0, ln


@pytest.mark.parametrize("width", WIDTHS)
def test_edge_on_degenerate_and_non_finite_triangles_are_kept_or_dead(lines, width):
    cases = {ln.split()[1]: fields(ln) for ln in pick(lines[width], "edge ")}
    must_stay = ["edge_on_x", "edge_on_skew", "edge_on_minus_ulp", "edge_on_plus_ulp", "zero_area_point", "zero_area_line", "huge_normal",
                 "inf_normal", "nan_normal", "tiny_normal", "faces_away"]
    for name in must_stay:
        assert cases[name]["excluded"] == "0", (name, cases[name])
    assert cases["faces_light"]["excluded"] == "1"
    for name, f in cases.items():                       # kept, or dead for every origin tried
        assert f["excluded"] == "0" or int(f["alive_origins"]) == 0, (name, f)
    # the cases are what they are named: one ulp either side of edge-on is alive on one side only, facing away always
    assert int(cases["edge_on_minus_ulp"]["alive_origins"]) > 0 and int(cases["faces_away"]["alive_origins"]) == 4000


@pytest.mark.parametrize("scene,lights", [("one", 1), ("two", 2), ("plane", 1)])
@pytest.mark.parametrize("width", WIDTHS)
def test_hit_or_miss_of_the_lights_tree_equals_a_loop_over_every_triangle(lines, width, scene, lights):
    got = pick(lines[width], "brute %s width %d light " % (scene, width))
    assert len(got) == lights
    for ln in got:
        f = fields(ln)
        assert int(f["rays"]) >= 500 and int(f["tree_mismatches"]) == 0 and int(f["scene_mismatches"]) == 0, ln
        before, after = int(ln.split("node_visits")[1].split()[0]), int(ln.split("->")[1])
        assert after < before, ln
        if scene == "plane":
            assert int(f["hits"]) == 0 and after == int(f["rays"]), ln      # the empty set: one node step per ray, no hit
        else:
            assert 100 < int(f["hits"]) < int(f["rays"]) - 100, ln           # both answers occur


@pytest.mark.parametrize("width", WIDTHS)
def test_appended_trees_pass_the_link_and_box_checks(lines, width):
    ls = lines[width]
    for scene, n_lights in [("none", 0), ("one", 1), ("two", 2), ("ratio", 1), ("plane", 1)]:
        (head,) = pick(ls, "links %s width %d lights %d |" % (scene, width, n_lights))
        assert head.endswith("scene validate null")
        per_light = pick(ls, "links %s width %d light " % (scene, width)) if n_lights else []
        assert len(per_light) == n_lights
        roots = []
        for ln in per_light:
            f = fields(ln)
            assert f["append"] == "null", ln
            if scene == "ratio":                        # 256 of 1552 is more than the 10 % this upload allowed: no tree, root 0
                assert f["built"] == "0" and f["root"] == "0" and f["nodes"] == "0", ln
                continue
            assert f["built"] == "1" and f["reread"] == "null" and f["violations"] == "0", ln
            assert int(f["refs"]) == int(f["occluders"]), ln
            assert int(f["root"]) > 0 and int(f["root"]) not in roots, ln
            roots.append(int(f["root"]))
            if scene == "plane":
                assert int(f["occluders"]) == 0 and int(f["nodes"]) == 1, ln
    two = [fields(ln) for ln in pick(ls, "links two width %d light " % width)]
    assert int(two[1]["root"]) == int(two[0]["root"]) + int(two[0]["nodes"])      # one behind the other


def test_the_getter_is_declared_and_bound():
    from par_raytracer_amd import capi
    assert "prt_get_shadow_trees" in capi.PRT_SYMBOLS
    assert capi.PrtShadowTreeInfo.build_ms.offset == 32 and capi.MAX_SHADOW_TREES == 4
    with open(os.path.join(ROOT, "include", "prt.h")) as f:
        header = f.read()
    assert re.search(r"int prt_get_shadow_trees\(const prt_ctx \* ctx, prt_shadow_tree_info \* out, uint32_t cap\);", header)
    assert "PRT_MAX_SHADOW_TREES = 4" in header
