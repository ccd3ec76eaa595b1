"""prt_trace_rays on the GPU under every schedule: a ray's answer is a function of (scene, ray, ray_bias, tmax) alone, whatever else
is in the batch and however the kernels hand the work out.  Every ray is a row of the committed fixtures tests/golden/trace_*.npz
(or one of the invalid rays of tests/trace_cases.py) and every expected value is the CPU oracle's: the fixture's own rows, or, for
the tmax specials, tests/trace_oracle_harness.cpp at test time.  What varies is the batch (its length, its order, whole waves and
chunks of one kind of ray, more rays than one pass of each grid), the schedule (KEEP_MIN, NODE_MIN, CHUNK_MIN, TRACE_BLOCKS_PER_CU,
the counting kernels), the LDS stack (STACK_CAP: rays that overflow it are traced again by k_query_exact) and the tree (a second
upload, the leaf table built by prt_closest_points, no triangles, the 8-wide library).

Every comparison is check_fixture's of tests/test_gpu_trace_rays.py: the six CLOSEST fields bit for bit, OCCLUDED without a limit
and below tmax, over every ray of the batch, through the numpy and the torch entry point.  Before each of them `spoil` runs a batch
of the same length with other answers through the same path, so that a ray the kernels never write shows a stale miss (or a stale
hit) in the reused buffers rather than the right answer of an earlier identical call.

tests/test_trace_cases_host.py proves the cases on the CPU (class sizes, uniform runs, the oracle reproduces the expected rows)."""
from __future__ import annotations

import contextlib
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import closest_cases as K
import trace_cases as T
from conftest import ROOT, host_scene
from test_gpu_trace_rays import check_fixture, renderers       # noqa: F401  (renderers: the module-scoped fixture)

PER = 192
EXACT_LANES = 64 * 256                 # k_query_exact's grid (launch_walk)
PAD_LANES = 1024 * 256                 # k_query_pad's grid (run_batch)
KNOBS = [dict(KEEP_MIN=1), dict(KEEP_MIN=64), dict(NODE_MIN=0), dict(NODE_MIN=64), dict(CHUNK_MIN=64, KEEP_MIN=64), dict(CHUNK_MIN=512),
         dict(TRACE_BLOCKS_PER_CU=1)]


@contextlib.contextmanager
def options(r, **kw):
    """The context's options set for the block, and restored whatever happens in it."""
    try:
        for k, v in kw.items():
            r.set_option(k, v)
        yield r
    finally:
        for k in kw:
            r.set_option(k, None)


def _call(r, case, torch_path, **kw):
    """One trace_rays call on the case's rays; numpy results either way."""
    o, d = case["origins"], case["directions"]
    if "tmax" in kw:
        kw["tmax"] = case["tmax"]
    if torch_path:
        import torch
        dev = torch.device("cuda", r.device_id)
        kw = {k: (torch.from_numpy(v).to(dev) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
        res = r.trace_rays(torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev), **kw)
        return {k: (v if k == "counters" else (v.cpu().numpy().view(np.uint32) if k == "vertex0" else v.cpu().numpy())) for k, v in res.items()}
    return r.trace_rays(o, d, **kw)


def spoil(r, g, n, torch_path, valid=False):
    """Fill the buffers the next calls of this length reuse (the context's staging buffer, torch's cached blocks) with other
    answers: n invalid rays - every one written at once as a miss / not occluded - or, ahead of a batch that expects misses, the
    fixture's rays from the 8th on, most of which hit."""
    case = T.rows(g, T.bias0(g)[(np.arange(n) + 7) % T.BIAS0_RAYS]) if valid else T.invalid_rays(g, n)
    _call(r, case, torch_path)
    _call(r, case, torch_path, mode="occluded")
    _call(r, case, torch_path, mode="occluded", tmax=True)


def check(r, g, case, count_visits=False, spoil_with_hits=False):
    """The case through both entry points against its expected rows; every ray is compared."""
    fx = T.as_fixture(case, g)
    n = len(case["origins"])
    for torch_path in (False, True):
        spoil(r, g, n, torch_path, valid=spoil_with_hits)
        assert check_fixture(r, fx, torch_path, count_visits) == n


# ---- the cases, as functions of a renderer getter: the tests below and the 8-wide child process run the same ones

def whole_waves_of_one_kind(get):
    for name in ("coincident", "icosphere_l3"):
        g = T.fixture(name)
        case = T.sorted_by_kind(g, PER)
        check(get(name), g, case)
        check(get(name), g, T.take(case, np.random.default_rng(17).permutation(len(case["kind"]))))


def stack_cap_2(get):
    for name in ("icosphere_l3", "coincident"):
        g = T.fixture(name)
        with options(get(name), STACK_CAP=2) as r:
            check(r, g, T.rows(g, T.bias0(g)))


def long_list(get):
    """24 x 2300 rays of cornell_box: 24 x 731 = 17,544 of them are replayed, more than k_query_exact has lanes."""
    g = T.fixture("cornell_box")
    case = T.tiled(g, 24 * T.BIAS0_RAYS)
    assert int(np.isin(case["index"], T.classes(g)["replay"]).sum()) > EXACT_LANES
    check(get("cornell_box"), g, case)
    return len(case["index"])


def tmax_specials(get, caps=(None, 2)):
    for name in ("coincident", "icosphere_l3"):
        g = T.fixture(name)
        case = T.expect_from_oracle(T.tmax_specials(g), host_scene(name, 0).desc)
        for cap in caps:
            with options(get(name), STACK_CAP=cap) as r:
                check(r, g, case)


def mixed_130(g):
    """130 rays, every fifth invalid, with the documented miss expected of all of them (a scene without triangles)."""
    case = T.invalid_rays(g, 130)
    sel = T.bias0(g)[:130]
    keep = np.arange(130) % 5 != 0
    for k in T.RAYS:
        case[k][keep] = g[k][sel][keep]
    case["index"] = np.where(keep, sel, -1)
    return case


def empty_scene():
    from par_raytracer_amd import api
    g = T.fixture("cornell_box")
    case = mixed_130(g)
    p = K.one_triangle()[0]
    r = api.Renderer(0)
    try:
        # hits of the same length first, on the same context and through torch's allocator: what the misses must overwrite
        r.upload(host_scene("cornell_box", 0))
        for torch_path in (False, True):
            spoil(r, g, 130, torch_path, valid=True)
        r.upload(K.flat_desc((p, np.zeros(0, np.uint32), np.zeros((0, 2), np.uint32))))
        assert r.scene_info().triangle_count == 0
        for torch_path in (False, True):
            assert check_fixture(r, T.as_fixture(case, g), torch_path) == 130        # asserts ray_count == 130
            res = _call(r, case, torch_path)
            assert np.all(res["group"] == -1) and np.all(res["t"] == T.FLT_MAX) and np.all(res["vertex0"] == 0xFFFFFFFF)
            assert not _call(r, case, torch_path, mode="occluded")["occluded"].any()
    finally:
        r.close()


# ---- a. wave boundaries

@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 257])
def test_batches_around_the_wave_size(renderers, n):                             # noqa: F811
    """The first n rays alone: another box pad than the whole fixture's (its origins' extent), the same answers."""
    g = T.fixture("cornell_box")
    check(renderers("cornell_box"), g, T.rows(g, T.bias0(g)[:n]))


# ---- b. whole waves and chunks of one kind

@pytest.mark.gpu
def test_whole_waves_of_one_kind_and_the_same_rays_shuffled(renderers):           # noqa: F811
    whole_waves_of_one_kind(renderers)


@pytest.mark.gpu
def test_a_batch_of_invalid_rays_only(renderers):                                # noqa: F811
    """Every chunk of every wave is written at the refill: nothing is ever traversed (k_query's `continue`)."""
    g = T.fixture("cornell_box")
    check(renderers("cornell_box"), g, T.invalid_rays(g, 200), spoil_with_hits=True)          # check_fixture asserts ray_count == 200


@pytest.mark.gpu
@pytest.mark.parametrize("name", T.FIXTURES)
def test_a_batch_of_replayed_rays_only(renderers, name):                          # noqa: F811
    """CLOSEST: every ray of every refill goes to the list, k_query traverses nothing and k_query_exact everything."""
    g = T.fixture(name)
    check(renderers(name), g, T.rows(g, T.classes(g)["replay"]))


# ---- c. schedule knobs

@pytest.mark.gpu
@pytest.mark.parametrize("name", ["coincident", "icosphere_l3"])
@pytest.mark.parametrize("knobs", KNOBS, ids=lambda kw: ",".join("%s=%s" % kv for kv in kw.items()))
def test_queries_do_not_depend_on_how_the_waves_are_tuned(renderers, name, knobs):      # noqa: F811
    g = T.fixture(name)
    with options(renderers(name), **knobs) as r:
        check(r, g, T.rows(g, T.bias0(g)))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["coincident", "icosphere_l3"])
def test_counting_kernels_give_the_same_bits(renderers, name):                    # noqa: F811
    g = T.fixture(name)
    r = renderers(name)
    case = T.rows(g, T.bias0(g))
    check(r, g, case, count_visits=True)
    for torch_path in (False, True):
        for kw in (dict(), dict(mode="occluded"), dict(mode="occluded", tmax=True)):
            plain, counted = _call(r, case, torch_path, **kw), _call(r, case, torch_path, count_visits=True, **kw)
            assert counted["counters"].node_visits > 0 and plain["counters"].node_visits == 0
            for k in plain:
                if k != "counters":
                    assert T.differing(counted[k], plain[k]).size == 0, (k, kw)


# ---- d. the LDS stack overflow route and the list

@pytest.mark.gpu
@pytest.mark.parametrize("name", ["icosphere_l3", "coincident"])
@pytest.mark.parametrize("cap", [2, 3])
def test_rays_that_overflow_the_lds_stack(renderers, name, cap):                  # noqa: F811
    """STACK_CAP = 2 is the marker and one entry, 3 one more: pushes are dropped, the ray is listed and k_query_exact traces it
    again - in OCCLUDED mode from tmax.  A listed ray is walked twice: the visit counts differ from the default stack's."""
    g = T.fixture(name)
    r = renderers(name)
    case = T.rows(g, T.bias0(g))
    modes = (dict(), dict(mode="occluded"), dict(mode="occluded", tmax=True))
    plain = [_call(r, case, False, count_visits=True, **kw)["counters"].node_visits for kw in modes]
    with options(r, STACK_CAP=cap):
        check(r, g, case)
        check(r, g, case, count_visits=True)
        capped = [_call(r, case, False, count_visits=True, **kw)["counters"].node_visits for kw in modes]
    print("%s STACK_CAP=%d node visits (closest, occluded, below tmax): default %s, capped %s" % (name, cap, plain, capped))
    assert all(a != b for a, b in zip(plain, capped)), (plain, capped)


@pytest.mark.gpu
def test_stack_overflow_with_every_lane_kept_and_the_smallest_chunk(renderers):   # noqa: F811
    for name in ("icosphere_l3", "coincident"):
        g = T.fixture(name)
        with options(renderers(name), STACK_CAP=2, KEEP_MIN=64, CHUNK_MIN=64) as r:
            check(r, g, T.rows(g, T.bias0(g)))


@pytest.mark.gpu
def test_a_list_longer_than_the_exact_kernels_grid(renderers):                    # noqa: F811
    t0 = time.perf_counter()
    n = long_list(renderers)
    print("long list: %d rays, %.2f s" % (n, time.perf_counter() - t0))


# ---- e. past one pass of every grid

@pytest.mark.gpu
@pytest.mark.parametrize("per_cu", [None, 1])
def test_more_rays_than_one_pass_of_the_grids(renderers, per_cu):                 # noqa: F811
    """2^19 + 5 rays: k_query's waves fetch chunk after chunk, k_query_pad (torch path) strides over its 262,144 lanes twice and
    k_query_exact over its 16,384 ten times.  With TRACE_BLOCKS_PER_CU = 1 the persistent grid is at most one block of 256 lanes
    per compute unit - the context's cu_count is the device's multiProcessorCount, which PRT_RESERVE_CUS can only lower - so
    the batch is more than twice its lanes."""
    import torch
    assert not os.environ.get("PRT_RESERVE_CUS")
    n = (1 << 19) + 5
    lanes = torch.cuda.get_device_properties(0).multi_processor_count * 256
    assert n > 4 * lanes and n > PAD_LANES and n % 64 == 5
    g = T.fixture("cornell_box")
    case = T.tiled(g, n)
    assert int(np.isin(case["index"], T.classes(g)["replay"]).sum()) > 10 * EXACT_LANES
    t0 = time.perf_counter()
    with options(renderers("cornell_box"), TRACE_BLOCKS_PER_CU=per_cu) as r:
        check(r, g, case)
    print("%d rays, TRACE_BLOCKS_PER_CU=%s: %.2f s" % (n, per_cu, time.perf_counter() - t0))


# ---- f. tmax specials

@pytest.mark.gpu
def test_tmax_inf_zero_negative_and_nan(renderers):                               # noqa: F811
    """+inf and FLT_MAX: no limit; 0, -1, NaN, -inf: not occluded (t < tmax never holds); the lanes between keep the fixture's
    tmax and its answers - against the oracle harness's brute force, at the default stack and through the overflow route."""
    tmax_specials(renderers)


# ---- g. uploads and the leaf table the two kinds of query share

@pytest.mark.gpu
def test_a_second_and_a_third_upload_on_one_context():
    from par_raytracer_amd import api
    r = api.Renderer(0)
    try:
        counts = []
        for name in ("coincident", "icosphere_l3", "coincident"):
            g = T.fixture(name)
            counts.append(r.upload(host_scene(name, 0)).triangle_count)
            check(r, g, T.rows(g, T.bias0(g)))
        assert counts[0] != counts[1] and counts[0] == counts[2]
    finally:
        r.close()


@pytest.mark.gpu
def test_the_leaf_table_built_by_either_kind_of_query(tmp_path):
    from par_raytracer_amd import api
    name = "icosphere_l3"
    g = T.fixture(name)
    rays = T.rows(g, T.bias0(g))
    mesh = K.scene_mesh(name)
    pts, _ = K.recipe_points(mesh, 512, 29)
    brute = K.run_harness(K.build_harness(tmp_path), [K.case(mesh, pts)], tmp_path)[0]["brute"]
    r = api.Renderer(0)
    try:
        for points_first in (True, False):
            r.upload(host_scene(name, 0))                                         # drops the table
            if points_first:
                K.assert_same_bits(r.closest_points(pts), brute, "points before rays")
            check(r, g, rays)
            K.assert_same_bits(r.closest_points(pts), brute, "points after rays")
    finally:
        r.close()


# ---- h. no triangles

@pytest.mark.gpu
def test_a_scene_without_triangles_is_all_misses():
    empty_scene()


# ---- i. the 8-wide library

CHILD = r"""
import os, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, "tests")); sys.path.insert(0, os.path.join(%(root)r, "oracle"))
from conftest import host_scene
import test_gpu_trace_rays_schedules as S
from par_raytracer_amd import api, capi
lib = capi.hip_lib()
assert os.path.basename(lib._name) == "libprt_hip_bvh8.so" and not (lib.prt_build_flags() & capi.BUILD_BVH4)
made = {}
def get(name):
    if name not in made:
        made[name] = api.Renderer(0)
        made[name].upload(host_scene(name, 0))
    return made[name]
for step in (S.whole_waves_of_one_kind, S.stack_cap_2, S.long_list, S.tmax_specials):
    step(get)
    print(step.__name__, "ok", flush=True)
for r in made.values():
    r.close()
S.empty_scene()
print("bvh8 schedules ok")
"""


@pytest.mark.gpu
def test_schedules_on_the_8_wide_library():
    if not os.path.exists(os.path.join(ROOT, "par_raytracer_amd", "libprt_hip_bvh8.so")):
        pytest.skip("libprt_hip_bvh8.so not built (make hip-bvh8)")
    env = dict(os.environ)
    env["PRT_HIP_LIB"] = "libprt_hip_bvh8.so"
    out = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         timeout=300)
    assert out.returncode == 0 and b"bvh8 schedules ok" in out.stdout, (out.returncode, out.stdout.decode()[-1500:],
                                                                       out.stderr.decode()[-3000:])


# ---- j. near ties given up

@pytest.mark.gpu
def test_near_ties_without_widening():
    """TIE_WIDEN_MAX = 0 on the coincident scene.  A render of it fails there with "near-tied hits could not be resolved"
    (tests/test_gpu_edges.py): some pixel's candidate set has a neighbour in the band above it.  No ray of the fixture has - measured on
    the device: none of its 3,072 rays, 1,478 of them near ties, at any of its three ray_bias values, and none of the other two fixtures'
    either - so no query of it can raise error -8.  What the rays can show is asserted instead: resolved at the first attempt, the
    replay gives the oracle's bits, for every ray of the fixture, and again once the option is restored."""
    from par_raytracer_amd import api
    g = T.fixture("coincident")
    n = g["origins"].shape[0]
    r = api.Renderer(0)
    try:
        r.upload(host_scene("coincident", 0))
        with options(r, TIE_WIDEN_MAX=0):
            assert check_fixture(r, g, torch_path=False) == n and check_fixture(r, g, torch_path=True) == n
        check(r, g, T.rows(g, T.bias0(g)))
    finally:
        r.close()
