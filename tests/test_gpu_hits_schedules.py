"""prt_trace_hits on the GPU under every schedule: a ray's answer is a function of (scene, ray, ray_bias, tmax, k, flags, cursor) alone,
whatever else is in the batch and however the kernels hand the work out.  Every expected row is the brute force's of
tests/hits_host_harness.cpp.  What varies is the schedule (KEEP_MIN, NODE_MIN, CHUNK_MIN, TRACE_BLOCKS_PER_CU, the counting
kernels), the LDS stack (STACK_CAP: rays that overflow it are walked again by k_hits_exact), the length of the slow list (more
listed rays than k_hits_exact has lanes) and the library (the 8-wide tree, in a child process).  check() is tests/test_gpu_hits.py's:
both entry points, each after a spoil batch of the same shape."""
from __future__ import annotations

import os
import subprocess
import sys

import numpy as np
import pytest

import hits_cases as H
from conftest import ROOT
from test_gpu_hits import Oracle, check, oracle, query, renderers, upload       # noqa: F401  (oracle, renderers: the module-scoped fixtures)
from test_gpu_trace_rays_schedules import KNOBS, options

EXACT_LANES = 64 * 256                 # k_hits_exact's grid (launch_walk)


# ---- the cases, as functions of a renderer getter and the oracle: the tests below and the 8-wide child process run the same ones

def knobs(get, orc, name, kw, count_visits):
    mesh, o, d, tmax, _ = orc.scene(name)
    if ("knobs", name) not in orc.cache:
        orc.cache[("knobs", name)] = orc.run([H.case(mesh, o, d, 8, back_faces=True), H.case(mesh, o, d, 3, tmax=tmax)])
    free, limited = orc.cache[("knobs", name)]
    with options(get(name), **kw) as r:
        check(r, free["brute"], o, d, 8, "%s %s" % (name, kw), count_visits=count_visits, back_faces=True)
        check(r, limited["brute"], o, d, 3, "%s %s below tmax" % (name, kw), count_visits=count_visits, tmax=tmax)


def overflow_route(get, orc, name, cap, four_wide=True):
    """STACK_CAP = 2 is the marker and one entry, 3 one more: pushes are dropped, the ray is listed and k_hits_exact walks it again
    from the start.  A listed ray is walked twice: the visit counts differ from the default stack's (asserted for the 4-wide tree,
    whose lanes the host harness walks under the same cap; the 8-wide tree's stack is as deep as the tree)."""
    mesh, o, d, _, _ = orc.scene(name)
    res = orc.run([H.case(mesh, o, d, 16, back_faces=True, stack_cap=cap)])[0]
    assert (res["listed"] == 2).sum() > 0, "no lane of the host harness dropped a push under this cap"
    r = get(name)
    plain = query(r, o, d, 16, False, back_faces=True, count_visits=True)["counters"].node_visits
    with options(r, STACK_CAP=cap):
        check(r, res["brute"], o, d, 16, "%s STACK_CAP=%d" % (name, cap), back_faces=True)
        capped = check(r, res["brute"], o, d, 16, "%s STACK_CAP=%d counted" % (name, cap), count_visits=True, back_faces=True)
    print("%s STACK_CAP=%d node visits: default %d, capped %s" % (name, cap, plain, capped))
    assert plain > 0 and (not four_wide or all(c != plain for c in capped))


def long_list(get, orc):
    """The plates' 16 far-origin rays tiled to more than k_hits_exact has lanes, a near ray after every 16: every far ray is
    listed at the start, and the exact kernel's lanes take more than one each."""
    mesh, o, d, _, kind = orc.scene("plates")
    far = np.nonzero(kind == "far")[0]
    near = np.nonzero(kind == "axis")[0][:1]
    unit = np.concatenate([far, near])
    expect = orc.brute(mesh, o[unit], d[unit], 4, back_faces=True)
    n = EXACT_LANES * len(unit) // len(far) + 1000
    sel = np.arange(n) % len(unit)
    assert n < 20000 and int((sel < len(far)).sum()) > EXACT_LANES
    check(get("plates"), {f: expect[f][sel] for f in H.FIELDS}, np.ascontiguousarray(o[unit][sel]), np.ascontiguousarray(d[unit][sel]), 4,
          "long list", back_faces=True)
    return n


# ---- schedule knobs

@pytest.mark.gpu
@pytest.mark.parametrize("count_visits", [False, True], ids=["plain", "counted"])
@pytest.mark.parametrize("kw", KNOBS, ids=lambda kw: ",".join("%s=%s" % kv for kv in kw.items()))
def test_hits_do_not_depend_on_how_the_waves_are_tuned(renderers, oracle, kw, count_visits):       # noqa: F811
    for name in ("plates", "coincident"):
        knobs(renderers, oracle, name, kw, count_visits)


@pytest.mark.gpu
def test_counting_kernels_count(renderers, oracle):                               # noqa: F811
    mesh, o, d, _, _ = oracle.scene("coincident")
    r = renderers("coincident")
    plain, counted = query(r, o, d, 4, False), query(r, o, d, 4, False, count_visits=True)
    assert plain["counters"].node_visits == 0 and counted["counters"].node_visits > 0 and counted["counters"].tri_tests > 0
    H.assert_same_bits(counted, plain, "counted against plain")


# ---- the LDS stack overflow route and the list

@pytest.mark.gpu
@pytest.mark.parametrize("name", ["icosphere_l3", "coincident"])
@pytest.mark.parametrize("cap", [2, 3])
def test_rays_that_overflow_the_lds_stack(renderers, oracle, name, cap):          # noqa: F811
    overflow_route(renderers, oracle, name, cap)


@pytest.mark.gpu
def test_stack_overflow_with_every_lane_kept_and_the_smallest_chunk(renderers, oracle):       # noqa: F811
    mesh, o, d, _, _ = oracle.scene("coincident")
    with options(renderers("coincident"), STACK_CAP=2, KEEP_MIN=64, CHUNK_MIN=64) as r:
        check(r, oracle.brute(mesh, o, d, 16, back_faces=True), o, d, 16, "cap 2, every lane kept", back_faces=True)


@pytest.mark.gpu
def test_a_list_longer_than_the_exact_kernels_grid(renderers, oracle):            # noqa: F811
    print("long list: %d rays" % long_list(renderers, oracle))


# ---- the 8-wide library

CHILD = r"""
import os, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, "tests")); sys.path.insert(0, os.path.join(%(root)r, "oracle"))
import hits_cases as H
import test_gpu_hits as G
import test_gpu_hits_schedules as S
from par_raytracer_amd import api, capi
lib = capi.hip_lib()
assert os.path.basename(lib._name) == "libprt_hip_bvh8.so" and not (lib.prt_build_flags() & capi.BUILD_BVH4)
orc = G.Oracle(%(dir)r)
made = {}
def get(name):
    if name not in made:
        made[name] = G.upload(api.Renderer(0), name)
    return made[name]
def every_field(name):
    mesh, o, d, tmax, _ = orc.scene(name)
    for back in (False, True):
        for k, res in zip(H.KS, orc.run([H.case(mesh, o, d, k, back_faces=back) for k in H.KS])):
            G.check(get(name), res["brute"], o, d, k, "%%s k=%%d back=%%d" %% (name, k, back), back_faces=back)
steps = [lambda: every_field("plates"), lambda: every_field("coincident"), lambda: every_field("icosphere_l3"),
         lambda: S.knobs(get, orc, "coincident", dict(CHUNK_MIN=64, KEEP_MIN=64), True),
         lambda: S.overflow_route(get, orc, "coincident", 2, False), lambda: S.overflow_route(get, orc, "icosphere_l3", 2, False),
         lambda: S.long_list(get, orc)]
for i, step in enumerate(steps):
    step()
    print("step", i, "ok", flush=True)
for r in made.values():
    r.close()
print("bvh8 hits ok")
"""


@pytest.mark.gpu
def test_hits_on_the_8_wide_library(oracle):                                      # noqa: F811
    assert os.path.exists(os.path.join(ROOT, "par_raytracer_amd", "libprt_hip_bvh8.so")), "libprt_hip_bvh8.so not built (make hip-bvh8)"
    env = dict(os.environ)
    env["PRT_HIP_LIB"] = "libprt_hip_bvh8.so"
    out = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "dir": oracle.dir}], env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 0 and b"bvh8 hits ok" in out.stdout, (out.returncode, out.stdout.decode()[-1500:], out.stderr.decode()[-3000:])
