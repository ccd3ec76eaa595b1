"""The host half of prt_upload_scene without a GPU (par_raytracer_amd/csrc/scene_pack.cpp: the description's checks, the
un-indexing, the layout of every array the upload puts on the device).  tests/scene_pack_host_harness.cpp - g++ with ASan and
UBSan, scene_pack.cpp + bvh_build.cpp + bvh_check.cpp through tests/hip_shim, once per tree width - calls the functions the upload
calls, in its order, and compares what they lay out with an independent copy: tests/harness_mesh.h's records() and leaf_map(), the
description's own normals, groups and lights, the classification called on the independent records' normals, and the two tree
checkers on every tree read back out of the packed arrays.  It prints one line per fact; the assertions are here.

The scenes are the smallest at which each branch is taken: no triangle; one; a cube in two groups with two materials, the
reference's sphere tree, a directional and a point light; a textured and bump-mapped quad; a seeded closed mesh of 288 triangles
under two directional lights, where shadow trees are built and triangles are open."""
import pytest

import harness

WIDTHS = [4, 8]
CASES = ["empty", "one_triangle", "cube", "textured_quad", "closed_mesh"]

# every refusal of the description: name -> the message prt_upload_scene gives (all with return code -1)
REFUSALS = {
    "null_scene": "null scene or index_count not a multiple of 3",
    "index_count": "null scene or index_count not a multiple of 3",
    "no_material": "at least one material is required",
    "triangle_cap": "2^26 triangles or more (the traversal addresses nodes and triangles by 32-bit byte offsets)",
    "group_first": "group index range is not a whole run of triangles inside the index buffers",
    "group_count": "group index range is not a whole run of triangles inside the index buffers",
    "group_past_end": "group index range is not a whole run of triangles inside the index buffers",
    "group_wraps": "group index range is not a whole run of triangles inside the index buffers",
    "material_negative": "group material out of range",
    "material_past_end": "group material out of range",
    "uncovered": "triangle not covered by any group",
    "position_index": "vertex index out of range (the reference would read out of bounds here)",
    "normal_index": "vertex index out of range (the reference would read out of bounds here)",
    "texcoord_index": "vertex index out of range (the reference would read out of bounds here)",
    "texture_slot_no_table": "material texture slot out of range",
    "texture_slot_past_end": "material texture slot out of range",
    "texture_no_texels": "texture needs texels, 1..4 channels and at least 2 x 2 texels",
    "texture_one_row": "texture needs texels, 1..4 channels and at least 2 x 2 texels",
    "texture_no_channels": "texture needs texels, 1..4 channels and at least 2 x 2 texels",
    "texture_five_channels": "texture needs texels, 1..4 channels and at least 2 x 2 texels",
    "texture_count": "more than 65534 textures",
    "bump_without_tangents": "a material has a bump map but the scene has no tangents",
    "coordinate_inf": "vertex coordinate is not finite or exceeds 1e18",
    "coordinate_nan": "vertex coordinate is not finite or exceeds 1e18",
    "coordinate_1e18": "vertex coordinate is not finite or exceeds 1e18",
}
CONTROLS = ["control_cube", "control_quad", "control_9e17"]


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    d = tmp_path_factory.mktemp("scene_pack")
    out = {}
    for width in WIDTHS:
        exe = harness.build("scene_pack_host_harness.cpp", d, "sp%d" % width, sanitize=True, bvh8=width == 8,
                            sources=("scene_pack.cpp", "bvh_build.cpp", "bvh_check.cpp"))
        out[width] = harness.run(exe, timeout=120).splitlines()
    return out


def fields(line):
    words = line.split("|", 1)[1].split()
    return dict(zip(words[0::2], words[1::2]))


def pick(lines, prefix):
    got = [ln for ln in lines if ln.startswith(prefix)]
    assert len(got) == 1, "%d lines start with %r" % (len(got), prefix)
    return got[0]


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("width", WIDTHS)
def test_every_packed_array_is_what_the_independent_copy_says(lines, width, case):
    ln = pick(lines[width], "case %s width %d |" % (case, width))
    f = fields(ln)
    assert f["rc"] == "0", ln
    # the triangle records bit for bit and the all-zero dummy; normals, stored geometric normal and material bits of the shading
    # records; bit l of the spare word = light l's open flag; the leaf map; the ranks; the trees' roots in the first light
    # table's pad and 0 in the second's
    for k in ("records_diff", "dummy_nonzero", "shade_diff", "open_diff", "leaf_map_diff", "rank_diff", "pad_diff"):
        assert f[k] == "0", (k, ln)
    # the scene's tree, and every appended tree moved home again: links, boxes, every occluder referenced once
    assert f["validate"] == "null" and f["reread_bad"] == "0" and f["box_violations"] == "0" and f["refs_diff"] == "0", ln
    # device_bytes is the sum of the array sizes; the same input packs to the same bytes
    assert f["bytes_diff"] == "0" and f["repack_same"] == "1", ln


@pytest.mark.parametrize("width", WIDTHS)
def test_each_case_takes_the_branch_it_is_there_for(lines, width):
    f = {case: fields(pick(lines[width], "case %s width %d |" % (case, width))) for case in CASES}
    assert [int(f[c]["triangles"]) for c in CASES] == [0, 1, 12, 2, 288]
    # no light: no tree; the cube's one directional light and the quad's get one each, the point light none
    assert f["empty"]["trees"] == f["one_triangle"]["trees"] == "0" and f["cube"]["trees"] == "1" and f["textured_quad"]["trees"] == "1"
    assert f["cube"]["point_lights"] == "1" and f["cube"]["translucent"] == "1" and f["closed_mesh"]["translucent"] == "0"
    # the cube's sphere tree is usable: 3 spheres x 2 records, c1's group first - group 0's first triangle ranks behind group
    # 1's seven -, so every slot's rank differs from its input index
    assert f["cube"]["spheres"] == "6" and f["cube"]["rank_of_first"] == "7" and f["cube"]["rank_moved"] == "12"
    assert f["closed_mesh"]["spheres"] == "0" and f["closed_mesh"]["rank_moved"] == "0"
    # the texture path's arrays exist for the quad alone: 2 x float4 of uv and 3 of tangents per record (2 triangles + the dummy)
    assert f["textured_quad"]["textured"] == f["textured_quad"]["bumped"] == "1" and f["textured_quad"]["textures"] == "2"
    assert f["textured_quad"]["uv"] == "6" and f["textured_quad"]["tan"] == "9"
    for c in ("empty", "one_triangle", "cube", "closed_mesh"):
        assert f[c]["textured"] == f[c]["bumped"] == "0" and f[c]["uv"] == f[c]["tan"] == "0", c
    # the closed mesh cannot go vacuous: shadow trees are built under the default size rule, and triangles are open
    assert int(f["closed_mesh"]["trees"]) >= 1 and int(f["closed_mesh"]["open"]) >= 1, f["closed_mesh"]


def test_neither_the_open_flags_nor_the_ranks_depend_on_the_tree_width(lines):
    for case in CASES:
        a, b = (fields(pick(lines[w], "case %s width %d |" % (case, w))) for w in WIDTHS)
        assert a["open"] == b["open"] and a["rank_of_first"] == b["rank_of_first"] and a["trees"] == b["trees"], case


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_a_refused_description_keeps_its_message_and_code_and_leaves_the_output_untouched(lines, name):
    for width in WIDTHS:
        ln = pick(lines[width], "refusal %s |" % name)
        assert ln == "refusal %s | rc -1 untouched 1 message prt_upload_scene: %s" % (name, REFUSALS[name]), ln


def test_the_refusals_are_the_edits_fault(lines):
    """The scenes the refusals edit pass unedited, and so does a coordinate just inside the 1e18 rule."""
    for name in CONTROLS:
        assert pick(lines[4], "refusal %s |" % name) == "refusal %s | rc 0 untouched 0 message untouched" % name
    assert len([ln for ln in lines[4] if ln.startswith("refusal ")]) == len(REFUSALS) + len(CONTROLS)
