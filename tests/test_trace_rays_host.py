"""prt_trace_rays without a GPU: the entry points exist in both libraries, the null-handle paths, and the fixtures of
tests/golden/trace_*.npz reproduce bit for bit from the CPU oracle's own TraceRay (tests/trace_oracle_harness.cpp, which
#includes oracle/prt_oracle.cpp unchanged).  The GPU side of the same fixtures: tests/test_gpu_trace_rays.py."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import trace_golden
from conftest import GOLDEN, ROOT, host_scene
from par_raytracer_amd import capi

FIELDS = ("t", "bw", "vertex0", "group", "position", "normal", "occluded", "occluded_tmax", "near_tie")


def test_both_libraries_export_the_query_entry_points():
    lib = capi.hip_lib()
    for n in ("prt_trace_rays", "prt_trace_rays_device"):
        assert hasattr(lib, n) and n in capi.PRT_SYMBOLS
    bvh8 = os.path.join(ROOT, "par_raytracer_amd", "libprt_hip_bvh8.so")
    if not os.path.exists(bvh8):
        subprocess.run(["make", "-C", ROOT, "hip-bvh8"], check=True, stdout=subprocess.DEVNULL)
    code = ("import ctypes; lib = ctypes.CDLL(%r)\n"
            "assert hasattr(lib, 'prt_trace_rays') and hasattr(lib, 'prt_trace_rays_device')\nprint('exported')\n") % bvh8
    out = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert out.returncode == 0 and b"exported" in out.stdout, out.stderr.decode()[-2000:]


def test_query_entry_points_refuse_a_null_context():
    lib = capi.hip_lib()
    o = np.zeros((1, 3), np.float32)
    b = capi.PrtRayBatch(o.ctypes.data, o.ctypes.data, None, 1, 0.0)
    for entry in (lib.prt_trace_rays, lib.prt_trace_rays_device):
        assert entry(None, capi.QUERY_CLOSEST, C.byref(b), None, 0, None) == -1
        assert entry(None, capi.QUERY_OCCLUDED, None, None, 0, None) == -1


def _fixture(name):
    path = os.path.join(GOLDEN, "trace_%s.npz" % name)
    assert os.path.exists(path), "missing fixture %s (python tests/trace_golden.py)" % path
    return np.load(path, allow_pickle=False)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


@pytest.mark.parametrize("name", [
    "cornell_box", "coincident", "icosphere_l3",
    pytest.param("terrain_1m", marks=pytest.mark.slow),          # 1,024 rays x 1M triangles of brute force: ~10^9 tests
])
def test_oracle_harness_reproduces_the_fixture(name):
    g = _fixture(name)
    assert str(g["scene"]) == name
    hs = host_scene(name, int(g["light_mode"]))
    out = trace_golden.oracle_batch(hs.desc, g["origins"], g["directions"], g["ray_bias"], g["tmax"])
    for k in FIELDS:
        assert np.array_equal(_bits(out[k]), _bits(g[k])), (name, k)
    n = g["origins"].shape[0]
    hit = g["group"] >= 0
    assert 1000 <= n <= 4096 and hit.any() and (~hit).any()
    assert np.all(g["vertex0"][~hit] == 0xFFFFFFFF) and np.all(g["t"][~hit] == np.float32(3.4028234663852886e38))
    assert np.all(g["vertex0"][hit] % 3 == 0)
    assert len(np.unique(g["ray_bias"])) >= 2 and np.any(g["ray_bias"] != 0)
    lengths = np.linalg.norm(g["directions"].astype(np.float64), axis=1)
    assert np.any(np.abs(lengths - 1.0) > 0.5)                          # non-unit directions are in
    # OCCLUDED without a limit is TraceRay(...) == true for the rays whose closest hit the reference finds
    assert np.all(g["occluded"][hit] == 1)


def test_coincident_fixture_holds_near_tied_rays():
    g = _fixture("coincident")
    assert int(g["near_tie"].sum()) > 0
    assert int((g["near_tie"].astype(bool) & (g["group"] >= 0)).sum()) > 100
