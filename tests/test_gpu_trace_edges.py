"""prt_trace_rays on the GPU against the CPU oracle on the cases of tests/trace_edge_cases.py: axis-parallel rays with signed
zeros, rays in a wall's plane and through vertices, direction components around 1e-30, directions of length 2^-120 to 2^120,
scenes scaled by 2^-45 to 2^30 and moved 10^3 and 10^6 away, scenes of one to five triangles, a flat one, one with zero-area
records.  Every case runs on the SAH and on the LBVH tree, through the numpy and the torch entry point (which computes the box pad
on the device), and is compared by tests/test_gpu_trace_rays.check_fixture: CLOSEST's six fields, OCCLUDED and OCCLUDED below
tmax, every ray bit for bit with the oracle's answer on the very desc that was uploaded.  No ray is left out and nothing has a
tolerance.  tests/test_trace_edges_host.py proves the cases on the CPU."""
from __future__ import annotations

import os
import subprocess
import sys

import pytest

import trace_edge_cases as E
from conftest import ROOT
from test_gpu_trace_rays import check_fixture
from test_gpu_trace_rays_schedules import options


def renderer(scene, builder="sah"):
    from par_raytracer_amd import api
    r = api.Renderer(0)
    if builder != "sah":
        r.set_option("BVH_BUILDER", builder)
    r.upload(scene.obj)
    return r


def check(r, cid):
    c = E.case(cid)
    fx = E.as_fixture(c)
    n = len(c["origins"])
    assert check_fixture(r, fx, torch_path=False) == n
    assert check_fixture(r, fx, torch_path=True) == n
    return n


def run_case(cid, builder="sah", **knobs):
    r = renderer(E.case(cid)["scene"], builder)
    try:
        assert r.scene_info().triangle_count == len(E.case(cid)["scene"].tri)
        with options(r, **knobs):
            return check(r, cid)
    finally:
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("builder", ["sah", "lbvh"])
@pytest.mark.parametrize("cid", E.CASES)
def test_edge_cases_equal_the_oracles_trace_ray(cid, builder):
    run_case(cid, builder)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ["axis-icosphere_l3", "plane-icosphere_l3", "flat-grid"])
def test_edge_cases_through_the_exact_kernel(cid):
    """STACK_CAP = 2: the marker and one entry - the rays overflow the LDS stack and k_query_exact traces them again."""
    run_case(cid, STACK_CAP=2)


@pytest.mark.gpu
def test_a_refit_to_the_shifted_scene_gives_the_shifted_cases_answers():
    """cornell_box uploaded, then moved by + 10^3 in place with the moved desc's spheres: the queries answer as on a fresh upload
    of the moved desc, which is what the oracle traced."""
    moved = E.case("shift-cornell_box@1000")["scene"]
    r = renderer(E.base_scene("cornell_box"))
    try:
        r.update_geometry(moved.positions, spheres=moved.arrays["spheres"], sphere_group=moved.arrays["sphere_group"])
        check(r, "shift-cornell_box@1000")
    finally:
        r.close()


CHILD = r"""
import os, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, "tests")); sys.path.insert(0, os.path.join(%(root)r, "oracle"))
import conftest
import trace_edge_cases as E
import test_gpu_trace_edges as G
from par_raytracer_amd import capi
lib = capi.hip_lib()
assert os.path.basename(lib._name) == "libprt_hip_bvh8.so" and not (lib.prt_build_flags() & capi.BUILD_BVH4)
n = sum(G.run_case(cid) for cid in E.CASES)
n += sum(G.run_case(cid, STACK_CAP=2) for cid in ("axis-icosphere_l3", "flat-grid"))
print("bvh8 edges ok", n, "rays")
"""


@pytest.mark.gpu
def test_edge_cases_on_the_8_wide_library():
    if not os.path.exists(os.path.join(ROOT, "par_raytracer_amd", "libprt_hip_bvh8.so")):
        pytest.skip("libprt_hip_bvh8.so not built (make hip-bvh8)")
    env = dict(os.environ)
    env["PRT_HIP_LIB"] = "libprt_hip_bvh8.so"
    out = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         timeout=300)
    assert out.returncode == 0 and b"bvh8 edges ok" in out.stdout, (out.returncode, out.stdout.decode()[-1500:],
                                                                   out.stderr.decode()[-3000:])
