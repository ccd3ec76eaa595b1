"""prt_closest_points on the GPU under every schedule: a point's answer is a function of (scene, point, max_dist2) alone, whatever
else is in the batch and however the kernels hand the work out.  Every expected row is the brute force's of
tests/closest_host_harness.cpp on the batch's unique points; tests/test_closest_cases_host.py proves the cases on the CPU first
(the rows of the built batches, how many points each stack cap lists, that far_tail's far point changes what is culled).  What
varies is the batch (its length, its order, whole waves and chunks of one kind of point, more points than one pass of each grid,
a far point that only k_closest_pad's second stride pass sees), the schedule (KEEP_MIN, NODE_MIN, CHUNK_MIN, TRACE_BLOCKS_PER_CU,
the counting kernels), the LDS stack (STACK_CAP: points that overflow it are walked again by k_closest_exact, with their radius),
the requested fields, and the scene (zero-area records, identical stacked records, scales from 2^-70 to 2^58 - eight of them
against float64 as well - offsets to 1e6, a refitted tree, the 8-wide library).

Every comparison is assert_same_bits on all requested fields over every point of the batch, through the host entry point (numpy)
and the device entry point (torch).  Before each of them a spoil batch of the same length, radii and fields runs through the same
path, so that a point the kernels never write shows a stale answer in the reused buffers rather than the right one of an earlier
identical call."""
from __future__ import annotations

import ctypes as C
import itertools
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import closest_cases as K
from conftest import ROOT, host_scene
from test_closest_host import LIMIT_UNITS
from test_gpu_closest import renderers                              # noqa: F401  (the module-scoped fixture)
from test_gpu_trace_rays_schedules import KNOBS, options

EXACT_LANES = 64 * 256                 # k_closest_exact's grid (launch_walk)
DTYPES = dict(dist2=(1, np.float32), point=(3, np.float32), bw=(3, np.float32), vertex0=(1, np.uint32), group=(1, np.int32))


class Oracle:
    """The brute force of tests/closest_host_harness.cpp, and the fixtures' recipe points with their answers, computed once."""

    def __init__(self, directory):
        self.dir = str(directory)
        exe = os.path.join(self.dir, "closest_host")
        self.exe = exe if os.path.exists(exe) else K.build_harness(self.dir)
        self.cache = {}

    def brute(self, mesh, points, max_dist2=None):
        return K.run_harness(self.exe, [K.case(mesh, points, max_dist2)], self.dir)[0]["brute"]

    def fixture(self, name):
        """(mesh, points, kind, answers without a radius) of the fixture's recipe."""
        if name not in self.cache:
            mesh = K.scene_mesh(name)
            pts, kind = K.recipe_points(mesh, K.RECIPE_POINTS, K.SCHEDULE_SEEDS[name])
            self.cache[name] = (mesh, pts, kind, self.brute(mesh, pts))
        return self.cache[name]

    def with_radii(self, name, n=K.RECIPE_POINTS):
        """(points, radius_mix radii, answers) of the fixture's first n recipe points."""
        if (name, n) not in self.cache:
            mesh, pts, kind, free = self.fixture(name)
            pts, r2 = np.ascontiguousarray(pts[:n]), K.radius_mix(free["dist2"][:n])
            self.cache[(name, n)] = (pts, r2, self.brute(mesh, pts, r2))
        return self.cache[(name, n)]


@pytest.fixture(scope="module")
def oracle(tmp_path_factory):
    return Oracle(tmp_path_factory.mktemp("closest_schedules"))


def query(r, pts, r2, torch_path, fields=K.FIELDS, count_visits=False):
    """One call; numpy results and "counters" either way.  Without radii through Renderer.closest_points; with radii through the
    C ABI, because the squares go in as given (the wrapper takes distances and squares them: no negative square, no exact d2)."""
    if r2 is None:
        if not torch_path:
            return r.closest_points(pts, fields=fields, count_visits=count_visits)
        import torch
        return K.to_numpy(r.closest_points(torch.from_numpy(pts).to(torch.device("cuda", r.device_id)), fields=fields, count_visits=count_visits))
    from par_raytracer_amd import capi
    n = len(pts)
    shape = lambda k: (n, 3) if DTYPES[k][0] == 3 else (n,)           # noqa: E731
    ctr = capi.PrtCounters()
    flags = capi.FLAG_COUNT_VISITS if count_visits else 0
    if torch_path:
        import torch
        dev = torch.device("cuda", r.device_id)
        tp, tr = torch.from_numpy(pts).to(dev), torch.from_numpy(r2).to(dev)
        out = {k: torch.empty(shape(k), dtype=torch.float32 if DTYPES[k][1] == np.float32 else torch.int32, device=dev) for k in fields}
        torch.cuda.current_stream(dev).synchronize()                   # the library's stream is not ordered against torch's
        ptr, entry = (lambda x: x.data_ptr()), capi.hip_lib().prt_closest_points_device
    else:
        tp, tr = pts, r2
        out = {k: np.empty(shape(k), DTYPES[k][1]) for k in fields}
        ptr, entry = (lambda x: x.ctypes.data), capi.hip_lib().prt_closest_points
    batch = capi.PrtPointBatch(ptr(tp), ptr(tr), n)
    cb = capi.PrtClosestBuffers(*[ptr(out[k]) if k in out else None for k in K.FIELDS])
    rc = entry(r._ctx, C.byref(batch), C.byref(cb), flags, C.byref(ctr))
    assert rc == 0, (rc, capi.hip_lib().prt_last_error(r._ctx))
    res = K.to_numpy(out) if torch_path else out
    res["counters"] = ctr
    return res


def check(r, pts, r2, expect, what, count_visits=False, fields=K.FIELDS, spoil_hits=None):
    """The batch through both entry points, each after a spoil batch through the same path; every point is compared.  Returns the
    two calls' (node_visits, tri_tests)."""
    n = len(pts)
    seen = []
    for torch_path in (False, True):
        query(r, *K.spoil_points(n, spoil_hits, radii=r2 is not None), torch_path, fields)
        res = query(r, pts, r2, torch_path, fields, count_visits)
        assert res["counters"].ray_count == n and set(res) == set(fields) | {"counters"} | ({"distance"} if r2 is None and "dist2" in fields else set())
        K.assert_same_bits(res, expect, "%s (%s)" % (what, "torch" if torch_path else "numpy"), fields)
        seen.append((res["counters"].node_visits, res["counters"].tri_tests))
    return seen


# ---- the cases, as functions of a renderer getter and the oracle: the tests below and the 8-wide child process run the same ones

def whole_waves_of_one_kind(get, orc):
    for name in ("icosphere_l3", "terrain_64"):
        mesh, pts, kind, free = orc.fixture(name)
        for batch in K.sorted_by_kind(pts, kind):
            check(get(name), batch["points"], batch["max_dist2"], K.rows(free, batch["index"]), name + " by kind")


def invalid_points_only(get, orc):
    """200 invalid queries after 200 hits: every chunk of every wave is written at the refill, nothing is ever walked."""
    mesh, pts, kind, free = orc.fixture("icosphere_l3")
    bad, r2 = K.invalid_points(200)
    check(get("icosphere_l3"), bad, r2, K.rows(free, np.full(200, -1)), "invalid points only", spoil_hits=pts)


def two_invalid_chunks_first(get, orc):
    """The first two default chunks (2 x 128 points) hold invalid queries only; 300 valid points follow."""
    mesh, pts, kind, free = orc.fixture("icosphere_l3")
    bad, bad_r2 = K.invalid_points(256)
    batch = np.ascontiguousarray(np.concatenate([bad, pts[:300]]))
    r2 = np.concatenate([bad_r2, np.full(300, K.FLT_MAX, np.float32)])
    check(get("icosphere_l3"), batch, r2, K.rows(free, np.concatenate([np.full(256, -1), np.arange(300)])), "two invalid chunks first", spoil_hits=pts)


def overflow_route(get, orc, width, name):
    """STACK_CAP 2 (the marker and one entry), 3 and the intermediate cap, with radius_mix radii and without: dropped pushes, the
    list and k_closest_exact's walk from the start, under the listed point's own radius.  A listed point is walked twice: the
    visit counts differ from the default stack's."""
    mesh, pts, kind, free = orc.fixture(name)
    _, r2, limited = orc.with_radii(name)
    r = get(name)
    plain = [query(r, pts, rr, False, count_visits=True)["counters"].node_visits for rr in (None, r2)]
    for cap in (2, 3, K.MID_CAP[width]):
        with options(r, STACK_CAP=cap):
            check(r, pts, None, free, "%s STACK_CAP=%d" % (name, cap))
            capped = [check(r, pts, None, free, "%s STACK_CAP=%d counting" % (name, cap), count_visits=True)[0][0],
                      check(r, pts, r2, limited, "%s STACK_CAP=%d radii" % (name, cap), count_visits=True)[0][0]]
        print("%s STACK_CAP=%d node visits (no radius, radii): default %s, capped %s" % (name, cap, plain, capped))
        assert all(a != b for a, b in zip(plain, capped)), (cap, plain, capped)


def overflow_with_every_lane_kept(get, orc):
    for name in ("terrain_64", "coincident"):
        pts, r2, limited = orc.with_radii(name)
        with options(get(name), STACK_CAP=2, KEEP_MIN=64, CHUNK_MIN=64) as r:
            check(r, pts, r2, limited, name + " STACK_CAP=2 KEEP_MIN=64 CHUNK_MIN=64")


def long_list(get, orc):
    """terrain_64's recipe tiled to 20,480 points at STACK_CAP=2: every valid point is listed (tests/test_closest_cases_host.py),
    more than k_closest_exact has lanes - its loop strides, and a lane's global stack column serves a second point."""
    mesh, pts, kind, free = orc.fixture("terrain_64")
    batch, index = K.tiled(pts, K.LONG_LIST)
    assert len(batch) > 1.2 * EXACT_LANES
    with options(get("terrain_64"), STACK_CAP=2) as r:
        check(r, batch, None, K.rows(free, index), "long list")
    return len(batch)


def past_one_pass(get, orc, per_cu, cap):
    import torch
    assert not os.environ.get("PRT_RESERVE_CUS")
    n = (1 << 19) + 5
    lanes = torch.cuda.get_device_properties(0).multi_processor_count * 256
    assert n > 4 * lanes and n > K.PAD_LANES and n % 64 == 5
    mesh, pts, kind, free = orc.fixture("cornell_box")
    batch, index = K.tiled(pts, n)
    with options(get("cornell_box"), TRACE_BLOCKS_PER_CU=per_cu, STACK_CAP=cap) as r:
        check(r, batch, None, K.rows(free, index), "2^19 + 5 points")
    return n


def field_subsets(get, orc):
    pts, r2, limited = orc.with_radii("coincident", 130)
    assert (limited["group"] >= 0).any() and (limited["group"] < 0).any()
    r = get("coincident")
    subsets = [s for k in range(1, 6) for s in itertools.combinations(K.FIELDS, k)]
    assert len(subsets) == 31
    for fields in subsets:
        check(r, pts, r2, limited, "fields " + "+".join(fields), fields=fields)


def scale_and_degenerates(orc, name, width):
    """One mesh of K.scale_meshes on contexts of its own: both builders, the default stack and STACK_CAP=2."""
    from par_raytracer_amd import api
    mesh = K.scale_meshes()[name]
    pts = K.recipe_points(mesh, 1024, K.SCALE_SEED)[0]
    expect = orc.brute(mesh, pts)
    if name == "stacked":
        K.assert_stacked_expectations(expect, K.stacked_base(), K.stacked_perm(), pts, LIMIT_UNITS, "brute force")
    for builder in ("sah", "lbvh"):
        r = api.Renderer(0)
        try:
            r.set_option("BVH_BUILDER", builder)
            if name == "2^62":                                # beyond the upload's rule (|coordinate| < 1e18): refused, not answered
                with pytest.raises(RuntimeError, match="exceeds 1e18"):
                    r.upload(K.flat_desc(mesh))
                continue
            r.upload(K.flat_desc(mesh))
            for cap in (None, 2):
                with options(r, STACK_CAP=cap):
                    check(r, pts, None, expect, "%s / %s / STACK_CAP=%s" % (name, builder, cap))
                    if name == "stacked":                     # on the device's own answers, whatever the brute force says
                        for torch_path in (False, True):
                            got = query(r, pts, None, torch_path)
                            K.assert_stacked_expectations(got, K.stacked_base(), K.stacked_perm(), pts, LIMIT_UNITS, "device, " + builder)
        finally:
            r.close()
    return int((expect["group"] < 0).sum())


def scale_sweep(orc, name, width):
    """One mesh of the float64 sweep (K.SWEEP_EXPONENTS) on contexts of its own, one per builder, uploaded once per exponent: the
    harness's bits at the default stack and at STACK_CAP=2 through both entry points, and conditions a and b on the harness's and
    on the device's own answers."""
    from par_raytracer_amd import api
    mesh, pts = K.sweep_mesh(name), K.sweep_points(name)
    best = K.true_distance(mesh, pts)
    cases = [K.sweep_case(mesh, pts, best, e) for e in K.SWEEP_EXPONENTS]
    expects = [x["brute"] for x in K.run_harness(orc.exe, [K.case(big, big_pts) for big, big_pts, keep in cases], orc.dir)]
    made = {builder: api.Renderer(0) for builder in ("sah", "lbvh")}
    try:
        for builder, r in made.items():
            r.set_option("BVH_BUILDER", builder)
            for e, (big, big_pts, keep), expect in zip(K.SWEEP_EXPONENTS, cases, expects):
                what = "%d-wide %s x 2^%d / %s" % (width, name, e, builder)
                assert keep.mean() >= 7.0 / 8.0, what
                K.assert_sweep_answers(expect, mesh, pts[keep], best[keep], e, LIMIT_UNITS, what + ", brute force")
                r.upload(K.flat_desc(big))
                for cap in (None, 2):
                    with options(r, STACK_CAP=cap):
                        check(r, big_pts, None, expect, "%s / STACK_CAP=%s" % (what, cap))
                        for torch_path in (False, True):
                            K.assert_sweep_answers(query(r, big_pts, None, torch_path), mesh, pts[keep], best[keep], e, LIMIT_UNITS, what + ", device")
    finally:
        for r in made.values():
            r.close()


# ---- a. around the wave size

@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 257])
def test_batches_around_the_wave_size(renderers, oracle, n):                     # noqa: F811
    """The first n points alone: another pad than the whole recipe's (their own extent), the same answers."""
    mesh, pts, kind, free = oracle.fixture("coincident")
    check(renderers("coincident"), np.ascontiguousarray(pts[:n]), None, K.rows(free, np.arange(n)), "%d points" % n)
    pts, r2, limited = oracle.with_radii("coincident")
    check(renderers("coincident"), np.ascontiguousarray(pts[:n]), np.ascontiguousarray(r2[:n]), K.rows(limited, np.arange(n)), "%d points, radii" % n)


# ---- b. whole waves and chunks of one kind

@pytest.mark.gpu
def test_whole_waves_of_one_kind_and_the_same_points_shuffled(renderers, oracle):  # noqa: F811
    whole_waves_of_one_kind(renderers, oracle)


@pytest.mark.gpu
def test_a_batch_of_invalid_points_only(renderers, oracle):                      # noqa: F811
    invalid_points_only(renderers, oracle)


@pytest.mark.gpu
def test_two_chunks_of_invalid_points_ahead_of_valid_ones(renderers, oracle):    # noqa: F811
    two_invalid_chunks_first(renderers, oracle)


# ---- c. schedule knobs and the counting kernels

@pytest.mark.gpu
@pytest.mark.parametrize("name", ["coincident", "terrain_64"])
def test_answers_and_counters_do_not_depend_on_how_the_waves_are_tuned(renderers, oracle, name):      # noqa: F811
    """The counters of a counting call are a function of (tree, batch, cap, pad): equal under every knob and between the entry
    points.  The counting kernels give the plain kernels' bits; the plain kernels report no visits."""
    pts, r2, limited = oracle.with_radii(name)
    r = renderers(name)
    base = check(r, pts, r2, limited, name + " counting", count_visits=True)
    assert base[0] == base[1] and base[0][0] > 0 and base[0][1] > 0, base
    assert check(r, pts, r2, limited, name + " plain") == [(0, 0), (0, 0)]
    for knobs in KNOBS:
        with options(r, **knobs):
            assert check(r, pts, r2, limited, "%s %s" % (name, knobs), count_visits=True) == base, knobs
            check(r, pts, r2, limited, "%s %s plain" % (name, knobs))


# ---- d. the LDS stack overflow route and the list

@pytest.mark.gpu
@pytest.mark.parametrize("name", ["terrain_64", "coincident"])
def test_points_that_overflow_the_lds_stack(renderers, oracle, name):            # noqa: F811
    overflow_route(renderers, oracle, 4, name)


@pytest.mark.gpu
def test_stack_overflow_with_every_lane_kept_and_the_smallest_chunk(renderers, oracle):       # noqa: F811
    overflow_with_every_lane_kept(renderers, oracle)


@pytest.mark.gpu
def test_a_list_longer_than_the_exact_kernels_grid(renderers, oracle):           # noqa: F811
    t0 = time.perf_counter()
    n = long_list(renderers, oracle)
    print("long list: %d points, %.2f s" % (n, time.perf_counter() - t0))


# ---- e. past one pass of every grid

@pytest.mark.gpu
@pytest.mark.parametrize("per_cu,cap", [(None, None), (None, 2), (1, 2)])
def test_more_points_than_one_pass_of_the_grids(renderers, oracle, per_cu, cap):   # noqa: F811
    """2^19 + 5 points: k_closest's waves fetch chunk after chunk, k_closest_pad (torch path) strides over its 262,144 lanes twice
    and, at STACK_CAP=2, k_closest_exact over its 16,384 thirty-two times (every point of cornell_box's recipe is listed at that
    cap on the 4-wide tree).  With TRACE_BLOCKS_PER_CU = 1 the persistent grid is at most one block of 256 lanes per compute
    unit, so the batch is more than four times its lanes."""
    t0 = time.perf_counter()
    n = past_one_pass(renderers, oracle, per_cu, cap)
    print("%d points, TRACE_BLOCKS_PER_CU=%s, STACK_CAP=%s: %.2f s" % (n, per_cu, cap, time.perf_counter() - t0))


# ---- f. k_closest_pad

@pytest.mark.gpu
def test_the_pad_reduced_on_the_device(oracle):
    """far_tail: the batch's largest |coordinate| is a negative y above index 262,144, next to a NaN point with larger components.
    The answers do not depend on the pad; the counters do (tests/test_closest_cases_host.py), so the device entry point's equal the
    host entry point's only if k_closest_pad found that point - in its second stride pass, through fabsf, past the NaN point.
    The control batch lacks the far point and visits strictly less, also right after the far batch on the same context."""
    from par_raytracer_amd import api
    mesh, near = K.far_tail_scene()
    ft = K.far_tail(near, K.PAD_LANES)
    assert len(ft["far"]) > K.PAD_LANES
    unique = oracle.brute(mesh, ft["unique"])
    r = api.Renderer(0)
    try:
        r.upload(K.flat_desc(mesh))
        assert unique["group"][len(near)] >= 0 and unique["group"][len(near) + 1] == -1       # the far point hits, the NaN point misses
        control = check(r, ft["control"], None, K.rows(unique, ft["index_control"]), "control", count_visits=True)
        far = check(r, ft["far"], None, K.rows(unique, ft["index_far"]), "far tail", count_visits=True)
        again = [tuple(getattr(query(r, ft["control"], None, torch_path, count_visits=True)["counters"], k) for k in ("node_visits", "tri_tests"))
                 for torch_path in (False, True)]
    finally:
        r.close()
    print("(node visits, triangle tests) numpy, torch: control %s, far tail %s, control again %s" % (control, far, again))
    assert far[0] == far[1] and control[0] == control[1], "the device's pad is not the host's"
    assert control[0][0] < far[0][0] and control[0][1] < far[0][1]
    assert again == control, "a pad was left over"


# ---- g. field subsets

@pytest.mark.gpu
def test_every_subset_of_the_fields(renderers, oracle):                          # noqa: F811
    field_subsets(renderers, oracle)


# ---- h. scale and degenerate geometry

@pytest.mark.gpu
@pytest.mark.parametrize("name", list(K.scale_meshes()))
def test_scales_offsets_and_degenerate_records(oracle, name):
    misses = scale_and_degenerates(oracle, name, 4)
    assert (misses > 0) == (name in ("2^58", "2^62"))       # d2 overflows for the far points: misses without a radius


@pytest.mark.gpu
@pytest.mark.parametrize("name", K.SWEEP_CLOSED + ("height_field",))
def test_float64_truth_at_every_scale(oracle, name):
    """2^-45 to 2^58: no valid point misses and the answer is within LIMIT_UNITS of the float64 minimum over all triangles - on
    the device's own answers, which are also the harness's bits (tests/test_closest_cases_host.py proves the cases)."""
    t0 = time.perf_counter()
    scale_sweep(oracle, name, 4)
    print("%s: %d exponents, %.2f s" % (name, len(K.SWEEP_EXPONENTS), time.perf_counter() - t0))


# ---- i. a moved scene on the slow path

@pytest.mark.gpu
def test_a_moved_scene_on_the_slow_path(oracle):
    from par_raytracer_amd import api
    p, idx, runs = K.scene_mesh("icosphere_l3")
    shear = np.array([[1.25, 0.0, 0.0], [0.5, 0.75, 0.0], [-0.25, 0.125, 1.5]], np.float32)
    moved = (np.ascontiguousarray((p @ shear).astype(np.float32)), idx, runs)
    pts, _ = K.recipe_points(moved, 1024, 55)
    r2 = K.radius_mix(oracle.brute(moved, pts)["dist2"])
    expect = oracle.brute(moved, pts, r2)
    assert (expect["group"] >= 0).sum() > 256
    r, fresh = api.Renderer(0), api.Renderer(0)
    try:
        r.upload(K.flat_desc((p, idx, runs)))
        r.update_geometry(moved[0])
        fresh.upload(K.flat_desc(moved))
        for ctx, what in ((r, "refitted tree"), (fresh, "fresh upload")):
            plain = query(ctx, pts, r2, False, count_visits=True)["counters"].node_visits
            with options(ctx, STACK_CAP=2):
                capped = check(ctx, pts, r2, expect, what + ", STACK_CAP=2", count_visits=True)
            assert capped[0][0] != plain
    finally:
        r.close()
        fresh.close()


# ---- the 8-wide library: b, d, e, g and h

CHILD = r"""
import os, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, "tests")); sys.path.insert(0, os.path.join(%(root)r, "oracle"))
from conftest import host_scene
import closest_cases as K
import test_gpu_closest_schedules as S
from par_raytracer_amd import api, capi
lib = capi.hip_lib()
assert os.path.basename(lib._name) == "libprt_hip_bvh8.so" and not (lib.prt_build_flags() & capi.BUILD_BVH4)
orc = S.Oracle(%(dir)r)
made = {}
def get(name):
    if name not in made:
        made[name] = api.Renderer(0)
        made[name].upload(host_scene(name, 0))
    return made[name]
steps = [lambda: S.whole_waves_of_one_kind(get, orc), lambda: S.invalid_points_only(get, orc), lambda: S.two_invalid_chunks_first(get, orc),
         lambda: S.overflow_route(get, orc, 8, "terrain_64"), lambda: S.overflow_route(get, orc, 8, "coincident"),
         lambda: S.overflow_with_every_lane_kept(get, orc), lambda: S.long_list(get, orc),
         lambda: S.past_one_pass(get, orc, None, 2), lambda: S.past_one_pass(get, orc, 1, 2), lambda: S.field_subsets(get, orc)]
steps += [lambda name=name: S.scale_and_degenerates(orc, name, 8) for name in K.scale_meshes()]
steps += [lambda name=name: S.scale_sweep(orc, name, 8) for name in K.SWEEP_CLOSED + ("height_field",)]
for i, step in enumerate(steps):
    step()
    print("step", i, "ok", flush=True)
for r in made.values():
    r.close()
print("bvh8 closest schedules ok")
"""


@pytest.mark.gpu
def test_schedules_on_the_8_wide_library(oracle):
    if not os.path.exists(os.path.join(ROOT, "par_raytracer_amd", "libprt_hip_bvh8.so")):
        pytest.skip("libprt_hip_bvh8.so not built (make hip-bvh8)")
    env = dict(os.environ)
    env["PRT_HIP_LIB"] = "libprt_hip_bvh8.so"
    out = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "dir": oracle.dir}], env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0 and b"bvh8 closest schedules ok" in out.stdout, (out.returncode, out.stdout.decode()[-1500:],
                                                                                 out.stderr.decode()[-3000:])
