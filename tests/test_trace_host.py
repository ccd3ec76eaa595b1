"""The device traversal code on the host: par_raytracer_amd/csrc/dev_trace*.h compiled with g++ against tests/hip_shim and run
one lane at a time (tests/trace_host_harness.cpp).  For thousands of rays over a scene with doubled and coplanar triangles the
hit trace_ray() returns - through the BVH the library builds and, where hits are near-tied, through resolve_near_ties() - must be
the hit of the reference's own sequential filter over every triangle in visit order (raytracer.cpp:104, 149, 208-220), bit for
bit; any-hit rays must agree on occluded / unoccluded.  Both traversal flavours the sources can be built as."""
import pytest

import harness


@pytest.mark.parametrize("flavour", ["bvh8", "bvh4"])
def test_device_traversal_equals_the_references_filter_on_the_host(flavour, tmp_path):
    exe = harness.build("trace_host_harness.cpp", tmp_path, "trace_host_" + flavour, bvh8=flavour == "bvh8", sources=("bvh_build.cpp",))
    out = harness.run(exe, 32, 8000, timeout=300)
    assert "closest-hit mismatches 0, any-hit mismatches 0, unresolved near ties 0" in out
    assert " 0 with a near tie" not in out, "the scene is meant to exercise resolve_near_ties: " + out
