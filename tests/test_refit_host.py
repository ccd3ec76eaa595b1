"""The refit's node step on the CPU.  par_raytracer_amd/csrc/dev_refit.h holds what one lane of k_refit_level does to one node -
read the children's exact boxes, union them, re-derive the node's power-of-two grid, round every child box outward onto it - as
__host__ __device__ code; tests/refit_host_harness.cpp, a stand-alone program built with g++ (and AddressSanitizer / UBSan,
through tests/hip_shim) from bvh_build.cpp + bvh_check.cpp + that header, runs it level by level, deepest first, over trees of
both widths and prints one line per (width, soup, move); the assertions are here.  No GPU library is involved."""
import re

import pytest

import harness

LINE = re.compile(r"width (\d) n (\d+) move (\w+) \| level_ok (\d) levels (\d+) depth (\d+) covered (\d+) nodes (\d+) child_bad (\d+) "
                  r"identical (\d) violations (\d+) refs (\d+) exp_bad (\d+) exp_m100 (\d+) root_e (-?\d+) (-?\d+) (-?\d+) validate (\w+)")
KERNELS = re.compile(r"kernels width (\d) \| level_ok (\d) bounds_ok (\d) nan_flag (\d+) record_bad (\d+) violations (\d+) refs (\d+) "
                     r"links_changed (\d+) validate (\w+)")
KERNEL_KEYS = ("level_ok", "bounds_ok", "nan_flag", "record_bad", "violations", "refs", "links_changed", "validate")
KEYS = ("level_ok", "levels", "depth", "covered", "nodes", "child_bad", "identical", "violations", "refs", "exp_bad", "exp_m100")


@pytest.fixture(scope="module")
def refits(tmp_path_factory):
    exe = harness.build("refit_host_harness.cpp", tmp_path_factory.mktemp("refit_host"), "refit_host", sanitize=True,
                        sources=("bvh_build.cpp", "bvh_check.cpp"))
    out = harness.run(exe, timeout=120)
    found = {}
    for line in out.splitlines():
        k = KERNELS.fullmatch(line)
        if k:
            found[("kernels", int(k.group(1)))] = dict(zip(KERNEL_KEYS, k.groups()[1:]))
            continue
        m = LINE.fullmatch(line)
        assert m, line
        rec = dict(zip(KEYS, (int(v) for v in m.groups()[3:14])))
        rec["root_e"] = tuple(int(v) for v in m.groups()[14:17])
        rec["validate"] = m.group(18)
        found[(int(m.group(1)), int(m.group(2)), m.group(3))] = rec
    return found


WIDTHS = [4, 8]
SIZES = [0, 1, 4, 5, 37, 1280]
MOVES = ["identity", "displaced", "flat_y", "scale_1024", "scale_2m20"]


def test_every_case_ran(refits):
    assert set(refits) == {(w, n, m) for w in WIDTHS for n in SIZES for m in MOVES} | {("kernels", w) for w in WIDTHS}


@pytest.mark.parametrize("width", WIDTHS)
def test_the_kernels_run_lane_by_lane_on_the_host_write_the_uploads_records(refits, width):
    """k_refit_bounds, k_refit_records and k_refit_level themselves, compiled with g++ through tests/hip_shim: the maximum and the
    NaN flag, every tris / shade / tangent record bit for bit as prt_upload_scene's expressions give it (the material word kept),
    a conservative tree, and no link touched."""
    k = refits[("kernels", width)]
    assert k == dict(level_ok="1", bounds_ok="1", nan_flag="1", record_bad="0", violations="0", refs="777", links_changed="0", validate="null")


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("width", WIDTHS)
def test_identity_refit_gives_back_the_builders_nodes_bit_for_bit(refits, width, n):
    t = refits[(width, n, "identity")]
    assert t["identical"] == 1 and t["violations"] == 0 and t["refs"] == n


@pytest.mark.parametrize("move", MOVES)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("width", WIDTHS)
def test_a_refitted_tree_is_conservative_and_references_every_triangle_once(refits, width, n, move):
    t = refits[(width, n, move)]
    assert t["validate"] == "null"
    assert t["violations"] == 0 and t["refs"] == n


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("width", WIDTHS)
def test_the_level_table_covers_every_node_once_with_children_one_level_below(refits, width, n):
    t = refits[(width, n, "identity")]
    assert t["level_ok"] == 1 and t["covered"] == t["nodes"] and t["child_bad"] == 0
    assert t["levels"] == t["depth"]
    if n <= 4:
        assert t["nodes"] == 1 and t["levels"] == 1           # the root is a single leaf (n = 0: the dummy record's)


@pytest.mark.parametrize("n", [1, 4, 5, 37, 1280])
@pytest.mark.parametrize("width", WIDTHS)
def test_an_axis_of_extent_zero_gets_the_smallest_exponent(refits, width, n):
    t = refits[(width, n, "flat_y")]
    assert t["root_e"][1] == -100
    assert t["exp_m100"] == t["nodes"]                        # every node's y axis, and no other
    assert refits[(width, n, "identity")]["exp_m100"] == 0


@pytest.mark.parametrize("move,shift", [("scale_1024", 10), ("scale_2m20", -20)])
@pytest.mark.parametrize("n", [1, 4, 5, 37, 1280])
@pytest.mark.parametrize("width", WIDTHS)
def test_a_power_of_two_scale_shifts_every_exponent(refits, width, n, move, shift):
    t, base = refits[(width, n, move)], refits[(width, n, "identity")]
    assert t["exp_bad"] == 0                                  # every exponent of every node is the builder's + shift
    assert t["root_e"] == tuple(e + shift for e in base["root_e"])
    assert t["identical"] == 0


def test_null_handles_are_refused_without_a_gpu():
    import ctypes as C
    import sys
    sys.path.insert(0, harness.ROOT)
    from par_raytracer_amd import capi
    lib = capi.hip_lib()
    u, info, out = capi.PrtGeometryUpdate(), capi.PrtUpdateInfo(), (C.c_uint64 * 6)()
    assert lib.prt_update_geometry(None, C.byref(u), C.byref(info)) == -1
    assert lib.prt_update_geometry_device(None, None, None) == -1
    assert lib.prt_multi_update_geometry(None, C.byref(u)) == -1
    assert lib.prt_debug_check_refit(None, None, out) == -1
    assert C.sizeof(capi.PrtGeometryUpdate) == 64 and C.sizeof(capi.PrtUpdateInfo) == 24
