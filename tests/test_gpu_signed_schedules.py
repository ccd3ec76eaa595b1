"""prt_signed_distance on the GPU under every schedule: a point's seven fields are a function of (scene, point, max_dist2) alone,
whatever else is in the batch and however the kernels hand the work out - the suite of tests/test_gpu_closest_schedules.py for
the signed query.  Every expected row is the brute force's of tests/signed_host_harness.cpp on the batch's unique points; the
batches are the ones tests/test_closest_cases_host.py proves (their rows, how many points each stack cap lists).  What varies is
the batch (its length around the wave size, whole waves of one kind of point, invalid points only, a list longer than
k_closest_exact's grid), the schedule (KEEP_MIN, NODE_MIN, CHUNK_MIN, TRACE_BLOCKS_PER_CU, the counting kernels), the LDS stack
(STACK_CAP), the requested fields (all 127 subsets), the grid of k_signed_normals (a context of 8 compute units, so that both of
its phases stride) and what the context held before (another scene, other geometry).

Every comparison is on all requested fields over every point of the batch, through the host entry point (numpy) and the device
entry point (torch), and follows a spoil batch of the same length, radii and fields through the same path.  A signed query after
prt_multi_update_geometry goes through the C ABI on the handle's own contexts (prt_multi_context), host entry point."""
from __future__ import annotations

import ctypes as C
import itertools
import os
import time

import numpy as np
import pytest

import closest_cases as K
import signed_cases as S
from conftest import host_scene
from test_gpu_trace_rays_schedules import KNOBS, options

EXACT_LANES = 64 * 256                 # k_closest_exact's grid (launch_walk)
DTYPES = dict(dist2=(1, np.float32), point=(3, np.float32), bw=(3, np.float32), vertex0=(1, np.uint32), group=(1, np.int32),
              signed_distance=(1, np.float32), feature=(1, np.uint8))
SCENES = ("coincident", "icosphere_l3", "terrain_64")


class Oracle:
    """The brute force of tests/signed_host_harness.cpp, and the fixtures' recipe points (closest_cases.recipe_points with the seeds
    of the closest-point schedule tests) with their answers, computed once."""

    def __init__(self, directory):
        self.dir = str(directory)
        self.exe = S.build_harness(self.dir)
        self.cache = {}

    def brute(self, mesh, points, max_dist2=None):
        return S.run_harness(self.exe, [S.case(mesh, points, max_dist2)], self.dir)[0]

    def fixture(self, name):
        """(mesh, points, kind, answers without a radius)."""
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
    return Oracle(tmp_path_factory.mktemp("signed_schedules"))


@pytest.fixture(scope="module")
def renderers():
    from par_raytracer_amd import api
    made = {}

    def get(name):
        if name not in made:
            made[name] = api.Renderer(0)
            made[name].upload(host_scene(name, 0))
        return made[name]
    yield get
    for r in made.values():
        r.close()


def rows(expect, index):
    """Expected rows of a batch built from unique points: row index[i] of `expect`, the documented miss where index[i] < 0."""
    index = np.asarray(index)
    out = {}
    for k in S.FIELDS:
        picked = np.asarray(expect[k])[np.maximum(index, 0)].copy()
        picked[index < 0] = S.MISS[k]
        out[k] = picked
    return out


def query(r, pts, r2, torch_path, fields=S.FIELDS, count_visits=False):
    """One call through the C ABI, as Renderer.signed_distance makes it, with the squared radii as given; numpy results and
    "counters" either way."""
    from par_raytracer_amd import capi
    n = len(pts)
    shape = lambda k: (n, 3) if DTYPES[k][0] == 3 else (n,)           # noqa: E731
    ctr = capi.PrtCounters()
    if torch_path:
        import torch
        dev = torch.device("cuda", r.device_id)
        kinds = {np.float32: torch.float32, np.uint32: torch.int32, np.int32: torch.int32, np.uint8: torch.uint8}
        tp, tr = torch.from_numpy(pts).to(dev), None if r2 is None else torch.from_numpy(r2).to(dev)
        out = {k: torch.empty(shape(k), dtype=kinds[DTYPES[k][1]], device=dev) for k in fields}
        torch.cuda.current_stream(dev).synchronize()                   # the library's stream is not ordered against torch's
        ptr, entry = (lambda x: None if x is None else x.data_ptr()), capi.hip_lib().prt_signed_distance_device
    else:
        tp, tr = pts, r2
        out = {k: np.empty(shape(k), DTYPES[k][1]) for k in fields}
        ptr, entry = (lambda x: None if x is None else x.ctypes.data), capi.hip_lib().prt_signed_distance
    batch = capi.PrtPointBatch(ptr(tp), ptr(tr), n)
    sb = capi.PrtSignedBuffers(capi.PrtClosestBuffers(*[ptr(out.get(k)) for k in K.FIELDS]), ptr(out.get("signed_distance")), ptr(out.get("feature")))
    rc = entry(r._ctx, C.byref(batch), C.byref(sb), capi.FLAG_COUNT_VISITS if count_visits else 0, C.byref(ctr))
    assert rc == 0, (rc, capi.hip_lib().prt_last_error(r._ctx))
    res = S.to_numpy(out) if torch_path else out
    res["counters"] = ctr
    return res


def check(r, pts, r2, expect, what, count_visits=False, fields=S.FIELDS, spoil_hits=None):
    """The batch through both entry points, each after a spoil batch through the same path; every point is compared.  Returns the
    two calls' (node_visits, tri_tests)."""
    n = len(pts)
    seen = []
    for torch_path in (False, True):
        query(r, *K.spoil_points(n, spoil_hits, radii=r2 is not None), torch_path, fields)
        res = query(r, pts, r2, torch_path, fields, count_visits)
        assert res["counters"].ray_count == n and set(res) == set(fields) | {"counters"}
        S.assert_same_bits(res, expect, "%s (%s)" % (what, "torch" if torch_path else "numpy"), fields)
        seen.append((res["counters"].node_visits, res["counters"].tri_tests))
    return seen


# ---- a. around the wave size

@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 128, 129, 257])
def test_batches_around_the_wave_size(renderers, oracle, n):
    mesh, pts, kind, free = oracle.fixture("coincident")
    check(renderers("coincident"), np.ascontiguousarray(pts[:n]), None, rows(free, np.arange(n)), "%d points" % n)
    pts, r2, limited = oracle.with_radii("coincident")
    check(renderers("coincident"), np.ascontiguousarray(pts[:n]), np.ascontiguousarray(r2[:n]), rows(limited, np.arange(n)), "%d points, radii" % n)


# ---- b. whole waves of one kind, invalid points only

@pytest.mark.gpu
@pytest.mark.parametrize("name", ["icosphere_l3", "terrain_64"])
def test_whole_waves_of_one_kind_and_the_same_points_shuffled(renderers, oracle, name):
    mesh, pts, kind, free = oracle.fixture(name)
    assert set(np.unique(free["feature"])) >= set(range(7)), "every region occurs"
    for batch in K.sorted_by_kind(pts, kind):
        check(renderers(name), batch["points"], batch["max_dist2"], rows(free, batch["index"]), name + " by kind")


@pytest.mark.gpu
def test_a_batch_of_invalid_points_only(renderers, oracle):
    """200 invalid queries after 200 hits: nothing is walked and nothing is signed; every field is the documented miss."""
    mesh, pts, kind, free = oracle.fixture("icosphere_l3")
    bad, r2 = K.invalid_points(200)
    check(renderers("icosphere_l3"), bad, r2, rows(free, np.full(200, -1)), "invalid points only", spoil_hits=pts)


# ---- c. schedule knobs and the counting kernels

@pytest.mark.gpu
def test_answers_and_counters_do_not_depend_on_how_the_waves_are_tuned(renderers, oracle):
    pts, r2, limited = oracle.with_radii("coincident")
    r = renderers("coincident")
    base = check(r, pts, r2, limited, "counting", count_visits=True)
    assert base[0] == base[1] and base[0][0] > 0 and base[0][1] > 0, base
    assert check(r, pts, r2, limited, "plain") == [(0, 0), (0, 0)]
    for knobs in KNOBS:
        with options(r, **knobs):
            assert check(r, pts, r2, limited, "%s" % knobs, count_visits=True) == base, knobs
            check(r, pts, r2, limited, "%s plain" % knobs)


# ---- d. the LDS stack overflow route and the list

@pytest.mark.gpu
@pytest.mark.parametrize("name", ["terrain_64", "coincident"])
def test_points_that_overflow_the_lds_stack(renderers, oracle, name):
    """STACK_CAP 2, 3 and the intermediate cap, with radius_mix radii and without: a listed point is walked again by
    k_closest_exact and signed from that walk's winner - the visit counts differ from the default stack's."""
    mesh, pts, kind, free = oracle.fixture(name)
    _, r2, limited = oracle.with_radii(name)
    r = renderers(name)
    plain = [query(r, pts, rr, False, count_visits=True)["counters"].node_visits for rr in (None, r2)]
    for cap in (2, 3, K.MID_CAP[4]):
        with options(r, STACK_CAP=cap):
            capped = [check(r, pts, None, free, "%s STACK_CAP=%d" % (name, cap), count_visits=True)[0][0],
                      check(r, pts, r2, limited, "%s STACK_CAP=%d radii" % (name, cap), count_visits=True)[0][0]]
        print("%s STACK_CAP=%d node visits (no radius, radii): default %s, capped %s" % (name, cap, plain, capped))
        assert all(a != b for a, b in zip(plain, capped)), (cap, plain, capped)


@pytest.mark.gpu
def test_a_list_longer_than_the_exact_kernels_grid(renderers, oracle):
    """terrain_64's recipe tiled to 20,480 points at STACK_CAP=2: every valid point is listed (tests/test_closest_cases_host.py),
    more than k_closest_exact has lanes."""
    mesh, pts, kind, free = oracle.fixture("terrain_64")
    batch, index = K.tiled(pts, K.LONG_LIST)
    assert len(batch) > 1.2 * EXACT_LANES
    t0 = time.perf_counter()
    with options(renderers("terrain_64"), STACK_CAP=2) as r:
        check(r, batch, None, rows(free, index), "long list")
    print("long list: %d points, %.2f s" % (len(batch), time.perf_counter() - t0))


# ---- e. field subsets

@pytest.mark.gpu
def test_every_subset_of_the_fields(renderers, oracle):
    """All 127: signed_distance without dist2 and feature alone among them."""
    pts, r2, limited = oracle.with_radii("coincident", 130)
    assert (limited["group"] >= 0).any() and (limited["group"] < 0).any()
    r = renderers("coincident")
    subsets = [s for k in range(1, 8) for s in itertools.combinations(S.FIELDS, k)]
    assert len(subsets) == 127 and ("signed_distance",) in subsets and ("feature",) in subsets
    for fields in subsets:
        check(r, pts, r2, limited, "fields " + "+".join(fields), fields=fields)


# ---- f. k_signed_normals past one pass of both phases

@pytest.mark.gpu
def test_the_accumulators_on_a_grid_that_strides(oracle, monkeypatch):
    """A context of 8 compute units (PRT_RESERVE_CUS = the device's count - 8): k_signed_normals' grid is at most 64 blocks = 16,384
    lanes, fewer than height_field(96, 5)'s 18,432 triangles (phase 1) and a sixth of its accumulator words (phase 0).  The answers
    are the harness's and those of a context on every compute unit, also after an update_geometry - for which phase 0 must have
    zeroed every word."""
    import torch
    from par_raytracer_amd import api
    assert not os.environ.get("PRT_RESERVE_CUS")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    mesh = K.height_field(96, 5)
    n_tris = mesh[1].size // 3
    words = 3 * (len(mesh[0]) + (3 * n_tris + 4 * 96) // 2)          # positions + edges (each inner edge twice, the rim's once)
    lanes = 8 * 8 * 256
    assert cus > 16 and n_tris == 18432 and n_tris > lanes and words > 100000 and words > 6 * lanes
    pts = S.recipe_points(mesh, 1024, 77)
    moved, pts_moved = S.sheared_mirror(mesh), S.sheared_mirror_points(pts)
    here, there = S.run_harness(oracle.exe, [S.case(mesh, pts), S.case(moved, pts_moved)], oracle.dir)
    assert set(np.unique(here["feature"])) >= set(range(7))
    monkeypatch.setenv("PRT_RESERVE_CUS", str(cus - 8))
    small = api.Renderer(0)
    monkeypatch.delenv("PRT_RESERVE_CUS")
    assert not os.environ.get("PRT_RESERVE_CUS")
    whole = api.Renderer(0)
    try:
        for r in (small, whole):
            r.upload(K.flat_desc(mesh))
        for at, at_pts, expect, step in ((mesh, pts, here, "uploaded"), (moved, pts_moved, there, "moved"), (mesh, pts, here, "moved back")):
            if step != "uploaded":
                small.update_geometry(at[0])
                whole.update_geometry(at[0])
            # (the host entry point alone: a context with a CU mask has blocking streams, which torch's null stream would join)
            query(small, *K.spoil_points(len(at_pts), radii=False), False)
            got = query(small, at_pts, None, False)
            S.assert_same_bits(got, expect, "8 compute units, " + step)
            check(whole, at_pts, None, got, "every compute unit, " + step)
    finally:
        small.close()
        whole.close()
    clear = (np.abs(here["signed_distance"]) > 0.01) & (np.abs(there["signed_distance"]) > 0.01)
    flipped = (here["signed_distance"][clear] < 0) != (there["signed_distance"][clear] < 0)
    assert clear.sum() > 256 and flipped.mean() > 0.75, "the mirror image turns the sheet over: stale accumulators would keep the old signs"


# ---- g. a second upload on one context

@pytest.mark.gpu
def test_a_second_upload_on_one_context(oracle):
    """The torus, then the cube: the adjacency and the accumulators of the old scene (288 positions, 864 edges) must not survive."""
    from par_raytracer_amd import api
    r = api.Renderer(0)
    try:
        for name in ("torus", "cube", "torus"):
            mesh = S.mesh_of(name)
            pts = S.recipe_points(mesh, 1024, S.SEEDS[name])
            r.upload(S.flat_desc(mesh))
            check(r, pts, None, oracle.brute(mesh, pts), "second upload: " + name)
    finally:
        r.close()


# ---- h. several devices behind one handle

class MultiContext:
    """Device i's context of a prt_multi handle, with what query() reads of a Renderer."""

    def __init__(self, lib, m, i):
        self._ctx, self.device_id = lib.prt_multi_context(m, i), 0
        assert self._ctx


@pytest.mark.gpu
def test_a_signed_query_after_a_multi_device_update(oracle):
    """Two contexts on device 0 behind one handle: the torus, a signed query on each (the tables are built), prt_multi_update_geometry
    to the sheared mirror image and back - after each the accumulators of both contexts are refilled from the moved records."""
    from par_raytracer_amd import capi
    lib = capi.hip_lib()
    mesh = S.torus()
    pts = S.recipe_points(mesh, 1024, S.SEEDS["torus"])
    moved, pts_moved = S.sheared_mirror(mesh), S.sheared_mirror_points(pts)
    here, there = S.run_harness(oracle.exe, [S.case(mesh, pts), S.case(moved, pts_moved)], oracle.dir)
    desc = S.flat_desc(mesh)
    m = lib.prt_multi_create((C.c_int * 2)(0, 0), 2)
    assert m
    try:
        assert lib.prt_multi_upload_scene(m, desc.desc) == 0, lib.prt_multi_last_error(m)
        contexts = [MultiContext(lib, m, i) for i in range(2)]
        for at, at_pts, expect, step in ((mesh, pts, here, "uploaded"), (moved, pts_moved, there, "moved"), (mesh, pts, here, "moved back")):
            if step != "uploaded":
                pos = np.ascontiguousarray(at[0])
                u = capi.PrtGeometryUpdate()
                u.positions, u.position_count = pos.ctypes.data, pos.size // 3
                assert lib.prt_multi_update_geometry(m, C.byref(u)) == 0, lib.prt_multi_last_error(m)
            for i, ctx in enumerate(contexts):
                query(ctx, *K.spoil_points(len(at_pts), radii=False), False)
                S.assert_same_bits(query(ctx, at_pts, None, False), expect, "device %d of the handle, %s" % (i, step))
    finally:
        lib.prt_multi_destroy(m)
