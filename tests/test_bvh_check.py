"""The guard in front of every upload, shown to fire.  par_raytracer_amd/csrc/bvh_check.cpp holds validate_bvh_links() - what
prt_upload_scene asks before it uploads a tree (the round-3 abort) - and check_bvh_wide(), the geometric check
behind prt_debug_check_bvh.  tests/bvh_check_harness.cpp, built with g++ from bvh_build.cpp + bvh_check.cpp alone, hands them
trees of both widths and both collapse rules as the builder made them, and then copies with one edit each; it prints a line per
tree and the assertions are here.  No GPU library is involved, so the 8-wide checker runs whichever library is loaded."""
import re

import pytest

import harness

LINE = re.compile(r"width (\d) (\w+) (\w+) (good|edit \w+) \| n_tris (\d+) violations (\d+) nodes (\d+) depth (\d+) stack_bound (\d+) "
                  r"leaves (\d+) refs (\d+) \| validate: (.*)")


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    exe = harness.build("bvh_check_harness.cpp", tmp_path_factory.mktemp("bvh_check"), "bvh_check", sources=("bvh_build.cpp", "bvh_check.cpp"))
    out = harness.run(exe, timeout=120)
    found = {}
    for line in out.splitlines():
        m = LINE.fullmatch(line)
        assert m, line
        keys = ("n_tris", "violations", "nodes", "depth", "stack_bound", "leaves", "refs")
        rec = dict(zip(keys, (int(v) for v in m.groups()[4:11])))
        rec["validate"] = m.group(12)
        found[(int(m.group(1)), m.group(2), m.group(3), m.group(4))] = rec
    return found


WIDTHS = [4, 8]
RULES = ["greedy", "dp"]


@pytest.mark.parametrize("scene,n_tris", [("grid12", 688), ("one", 1), ("same37", 37)])
@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("width", WIDTHS)
def test_a_built_tree_passes_both_checks(trees, width, rule, scene, n_tris):
    t = trees[(width, rule, scene, "good")]
    assert t["validate"] == "null"
    assert t["violations"] == 0
    assert t["n_tris"] == n_tris and t["refs"] == n_tris
    assert t["stack_bound"] == (3 * t["depth"] + 2 if width == 4 else t["depth"] + 2)


@pytest.mark.parametrize("edit,names", [("child", "child"), ("leaf_range", "leaf triangle range")])
@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("width", WIDTHS)
def test_an_address_outside_the_arrays_is_named_before_upload(trees, width, rule, edit, names):
    t = trees[(width, rule, "grid12", "edit " + edit)]
    assert t["validate"].startswith("%d-wide BVH: " % width) and names in t["validate"] and "out of range" in t["validate"]


@pytest.mark.parametrize("edit", ["qhi", "tri_order"])
@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("width", WIDTHS)
def test_a_triangle_outside_its_box_is_counted(trees, width, rule, edit):
    t = trees[(width, rule, "grid12", "edit " + edit)]
    assert t["validate"] == "null"            # the addresses are all in range: only the geometric check can see it
    assert t["violations"] > 0


@pytest.mark.parametrize("rule", RULES)
def test_a_slot_in_both_masks_is_flagged_by_both(trees, rule):
    t = trees[(8, rule, "grid12", "edit masks")]
    assert t["validate"] == "8-wide BVH: a slot is both an internal node and a leaf"
    assert t["violations"] > 0
