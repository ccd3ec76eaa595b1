"""prt_trace_hits on the GPU against the definition: every expected row is the brute force's of tests/hits_host_harness.cpp over all
records in input order (tests/test_hits_host.py proves the walk against it on the CPU first).  Every comparison is
assert_same_bits on all requested fields over every ray, through the host entry point (numpy) and the device entry point (torch),
each after a spoil batch of the same shape through the same path, so that a slot the kernels never write shows a stale record in
the reused buffers rather than the right one of an earlier identical call."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import pytest

import hits_cases as H
import trace_cases as T
from conftest import host_scene

SCENES = ("plates",) + T.FIXTURES


class Oracle:
    """The brute force of tests/hits_host_harness.cpp; meshes and rays per scene, computed once."""

    def __init__(self, directory):
        self.dir = str(directory)
        exe = os.path.join(self.dir, "hits_host")
        self.exe = exe if os.path.exists(exe) else H.build_harness(self.dir)
        self.cache = {}

    def scene(self, name):
        """(mesh, origins, directions, tmax, kind): the plates with their rays and the tmax specials, or a fixture with its bias-0 rays."""
        if name not in self.cache:
            if name == "plates":
                o, d, kind = H.plate_rays()
                self.cache[name] = (H.plates(), o, d, H.tmax_specials(len(o))[0], kind)
            else:
                self.cache[name] = (H.scene_mesh(name),) + H.fixture_rays(name) + (None,)
        return self.cache[name]

    def run(self, cases):
        return H.run_harness(self.exe, cases, self.dir)

    def brute(self, mesh, o, d, k, **kw):
        return self.run([H.case(mesh, o, d, k, **kw)])[0]["brute"]


@pytest.fixture(scope="module")
def oracle(tmp_path_factory):
    return Oracle(tmp_path_factory.mktemp("gpu_hits"))


def upload(r, name):
    r.upload(H.flat_desc(H.plates()) if name == "plates" else host_scene(name, 0))
    return r


@pytest.fixture(scope="module")
def renderers():
    from par_raytracer_amd import api
    out = {}

    def get(name, builder="sah"):
        if (name, builder) not in out:
            r = api.Renderer(0)
            if builder != "sah":
                r.set_option("BVH_BUILDER", builder)
            out[(name, builder)] = upload(r, name)
        return out[(name, builder)]
    yield get
    for r in out.values():
        r.close()


def query(r, o, d, k, torch_path, **kw):
    """One trace_hits call; numpy results and "counters" either way."""
    if not torch_path:
        return r.trace_hits(o, d, k, **kw)
    import torch
    dev = torch.device("cuda", r.device_id)
    conv = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32) if a.dtype == np.uint32 else np.ascontiguousarray(a)).to(dev)   # noqa: E731
    for key in ("tmax",):
        if kw.get(key) is not None:
            kw[key] = conv(kw[key])
    if isinstance(kw.get("after"), dict):
        kw["after"] = {f: conv(v) for f, v in kw["after"].items() if f != "counters"}
    elif kw.get("after") is not None:
        kw["after"] = tuple(conv(a) for a in kw["after"])
    return H.to_numpy(r.trace_hits(conv(o), conv(d), k, **kw))


def spoil(r, n, k, torch_path, fields=H.FIELDS, hits=None):
    """Fill the buffers the next call of this shape reuses with other answers: n rays that are misses by definition, or - ahead
    of a batch that expects misses - `hits`, (origins, directions) of rays that hit."""
    if hits is not None:
        o, d = (np.ascontiguousarray(a[np.arange(n) % len(a)]) for a in hits)
    else:
        o, d = np.full((n, 3), np.nan, np.float32), np.tile(np.float32([0, 0, 1]), (n, 1))
    query(r, o, d, k, torch_path, fields=fields, back_faces=True)


def check(r, expect, o, d, k, what, fields=H.FIELDS, count_visits=False, spoil_hits=None, **kw):
    """The batch through both entry points against the expected rows; returns the two calls' node_visits."""
    n, seen = len(o), []
    for torch_path in (False, True):
        spoil(r, n, k, torch_path, fields, spoil_hits)
        res = query(r, o, d, k, torch_path, fields=fields, count_visits=count_visits, **dict(kw))
        assert res["counters"].ray_count == n and res["counters"].pipeline == 0 and set(res) == set(fields) | {"counters"}
        H.assert_same_bits(res, expect, "%s (%s)" % (what, "torch" if torch_path else "numpy"), fields)
        seen.append(res["counters"].node_visits)
    return seen


# ---- every field against the brute force

@pytest.mark.gpu
@pytest.mark.parametrize("back", [False, True], ids=["front", "both"])
@pytest.mark.parametrize("name", SCENES)
def test_every_field_equals_the_brute_force(renderers, oracle, name, back):
    mesh, o, d, tmax, _ = oracle.scene(name)
    cases = [H.case(mesh, o, d, k, back_faces=back) for k in H.KS] + [H.case(mesh, o, d, 3, tmax=tmax, back_faces=back)]
    results = oracle.run(cases)
    r = renderers(name)
    for k, res in zip(H.KS, results):
        assert res["brute"]["hit_count"].max() == min(k, res["remaining"].max())
        check(r, res["brute"], o, d, k, "%s k=%d back=%d" % (name, k, back), back_faces=back)
    check(r, results[-1]["brute"], o, d, 3, "%s below tmax back=%d" % (name, back), back_faces=back, tmax=tmax)


@pytest.mark.gpu
def test_a_biased_batch(renderers, oracle):
    mesh, o, d, _, kind = oracle.scene("plates")
    near = kind != "overflow"                             # (their biased origins lie 2^117 out, and a batch's pad follows its largest origin)
    o, d = np.ascontiguousarray(o[near]), np.ascontiguousarray(d[near])
    check(renderers("plates"), oracle.brute(mesh, o, d, 8, back_faces=True, ray_bias=0.125), o, d, 8, "ray_bias 0.125", back_faces=True, ray_bias=0.125)


# ---- field masks

@pytest.mark.gpu
def test_single_fields_and_none(renderers, oracle):
    mesh, o, d, _, _ = oracle.scene("plates")
    expect = oracle.brute(mesh, o, d, 3, back_faces=True)
    r = renderers("plates")
    for fields in [(f,) for f in H.FIELDS] + [(), ("hit_count", "back"), ("t", "group")]:
        check(r, expect, o, d, 3, "fields %s" % (fields,), fields=fields, back_faces=True)


# ---- batch lengths

@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_batch_lengths(renderers, oracle, n):
    """The first n rays (the plates' rays repeated past their end): another pad than the whole batch's wherever the far and the
    overflow rays fall away, the same answers."""
    mesh, o, d, _, _ = oracle.scene("plates")
    expect = oracle.brute(mesh, o, d, 8, back_faces=True)
    sel = np.arange(n) % len(o)
    check(renderers("plates"), {f: expect[f][sel] for f in H.FIELDS}, np.ascontiguousarray(o[sel]), np.ascontiguousarray(d[sel]), 8, "n=%d" % n,
          back_faces=True)


@pytest.mark.gpu
def test_a_batch_longer_than_one_pass_of_the_grid(renderers, oracle):
    """One block per compute unit and the smallest chunks: the persistent grid has at most cu_count x 256 lanes, the batch more."""
    import torch
    from test_gpu_trace_rays_schedules import options
    lanes = torch.cuda.get_device_properties(0).multi_processor_count * 256
    n = lanes + 4097
    mesh, o, d, _, _ = oracle.scene("plates")
    expect = oracle.brute(mesh, o, d, 2, back_faces=True)
    sel = np.arange(n) % len(o)
    with options(renderers("plates"), TRACE_BLOCKS_PER_CU=1, CHUNK_MIN=64) as r:
        check(r, {f: expect[f][sel] for f in H.FIELDS}, np.ascontiguousarray(o[sel]), np.ascontiguousarray(d[sel]), 2, "n=%d" % n, back_faces=True)


# ---- resume

@pytest.mark.gpu
@pytest.mark.parametrize("torch_path", [False, True], ids=["numpy", "torch"])
def test_pages_of_three_reproduce_the_list(renderers, oracle, torch_path):
    """Pages of k = 3 chained through `after` (the previous result) until no ray fills its page: laid end to end they are the
    harness's full sorted list - 24 and more entries on the axis rays - and one k = 16 call where a ray has no more than 16."""
    mesh, o, d, _, kind = oracle.scene("plates")
    whole = oracle.run([H.case(mesh, o, d, 16, back_faces=True, full=H.FULL)])[0]
    assert whole["remaining"][kind == "axis"].min() >= 24 and whole["remaining"].max() <= H.FULL
    r = renderers("plates")
    pages, after = [], None
    for _ in range(H.FULL // 3 + 2):
        spoil(r, len(o), 3, torch_path)
        page = query(r, o, d, 3, torch_path, back_faces=True, after=after)
        pages.append(page)
        if not (page["hit_count"] == 3).any():
            break
        after = page
    else:
        raise AssertionError("the pages never ran dry")
    assert 3 * len(pages) >= whole["remaining"].max()
    assert np.array_equal(sum(p["hit_count"].astype(np.int64) for p in pages), whole["remaining"])
    laid = {f: np.concatenate([p[f] for p in pages], axis=1) for f in ("t", "bw", "vertex0", "group", "back")}
    m = min(laid["t"].shape[1], H.FULL)
    H.assert_same_bits({f: laid[f][:, :m] for f in ("t", "vertex0", "group", "back")}, {f: whole["full"][f][:, :m] for f in ("t", "vertex0", "group", "back")},
                       "pages against the full list", ("t", "vertex0", "group", "back"))
    one = query(r, o, d, 16, torch_path, back_faces=True)
    H.assert_same_bits(one, whole["brute"], "k = 16", H.FIELDS)
    few = whole["remaining"] <= 16
    assert few.sum() > 64
    H.assert_same_bits({f: laid[f][few][:, :16] for f in laid}, {f: one[f][few] for f in laid}, "pages against k = 16", tuple(laid))
    # a triple instead of a result: the same second page
    second = query(r, o, d, 3, torch_path, back_faces=True, after=H.last_filled(pages[0]))
    H.assert_same_bits(second, pages[1], "cursor as a triple", H.FIELDS)


# ---- compositions with prt_trace_rays

@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_compositions_with_trace_rays(renderers, oracle, name):
    """hit_count > 0 (front only, no cursor) exactly when OCCLUDED with the same tmax; slot 0's t <= CLOSEST's t, equal in bits
    wherever both name the same (group, vertex0)."""
    mesh, o, d, tmax, _ = oracle.scene(name)
    r = renderers(name)
    free, limited = r.trace_hits(o, d, 1), r.trace_hits(o, d, 1, tmax=tmax)
    assert np.array_equal(free["hit_count"] > 0, r.trace_rays(o, d, mode="occluded")["occluded"] != 0)
    assert np.array_equal(limited["hit_count"] > 0, r.trace_rays(o, d, mode="occluded", tmax=tmax)["occluded"] != 0)
    assert (limited["hit_count"] > 0).any() and (limited["hit_count"] < free["hit_count"]).any()
    closest = r.trace_rays(o, d)
    assert np.all(free["t"][:, 0] <= closest["t"])
    same = (free["group"][:, 0] == closest["group"]) & (free["vertex0"][:, 0] == closest["vertex0"]) & (closest["group"] >= 0)
    # (where CLOSEST hits, slot 0 names its triangle unless a tie on t is decided the other way: the reference's visit order there, the key here)
    assert same.sum() > 0 and same.sum() >= (closest["group"] >= 0).sum() // 2
    assert np.array_equal(free["t"][same, 0].view(np.uint32), closest["t"][same].view(np.uint32))


# ---- other trees

@pytest.mark.gpu
@pytest.mark.parametrize("name", ["plates", "coincident"])
def test_the_lbvh_tree(renderers, oracle, name):
    mesh, o, d, _, _ = oracle.scene(name)
    check(renderers(name, "lbvh"), oracle.brute(mesh, o, d, 8, back_faces=True), o, d, 8, name + " lbvh", back_faces=True)


@pytest.mark.gpu
def test_a_refitted_tree(oracle):
    """prt_update_geometry moves the vertices under the tree: the expected rows are the brute force's over the moved mesh."""
    from par_raytracer_amd import api
    p, idx, runs = H.scene_mesh("icosphere_l3")
    o, d, _ = H.fixture_rays("icosphere_l3")
    shear = np.array([[1.25, 0.0, 0.0], [0.5, 0.75, 0.0], [-0.25, 0.125, 1.5]], np.float32)
    moved = (np.ascontiguousarray((p @ shear).astype(np.float32)), idx, runs)
    still, expect = (res["brute"] for res in oracle.run([H.case(m, o, d, 8, back_faces=True) for m in ((p, idx, runs), moved)]))
    assert T.differing(still["t"], expect["t"]).size > len(o) // 4
    r = api.Renderer(0)
    try:
        r.upload(H.flat_desc((p, idx, runs)))
        check(r, still, o, d, 8, "before the move", back_faces=True)
        r.update_geometry(moved[0])
        check(r, expect, o, d, 8, "refitted tree", back_faces=True)
    finally:
        r.close()


# ---- refusals

@pytest.mark.gpu
def test_refusals(renderers):
    from par_raytracer_amd import api, capi
    lib = capi.hip_lib()
    r = renderers("plates")
    o, d, _ = H.plate_rays()
    n = len(o)
    count, aft, afg, afv = np.full(n, 77, np.uint32), np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros(n, np.uint32)

    def call(ctx, rq, out, entry=lib.prt_trace_hits):
        ctr = capi.PrtCounters()
        ctr.ray_count = 99
        rc = entry(ctx, C.byref(rq) if rq is not None else None, C.byref(out) if out is not None else None, 0, C.byref(ctr))
        return rc, lib.prt_last_error(ctx).decode(), ctr

    def request(k=3, flags=0, after=(None, None, None), origins=o, directions=d, n_rays=n):
        ptr = lambda a: a.ctypes.data if a is not None else None             # noqa: E731
        return capi.PrtHitsRequest(capi.PrtRayBatch(ptr(origins), ptr(directions), None, n_rays, 0.0), k, flags, *[ptr(a) for a in after])
    out = capi.PrtHitsBuffers(count.ctypes.data, None, None, None, None, None)
    for entry in (lib.prt_trace_hits, lib.prt_trace_hits_device):
        for rq, ob, text in ((None, out, "null request or buffers"), (request(), None, "null request or buffers"),
                             (request(origins=None), out, "null origins or directions"), (request(directions=None), out, "null origins or directions"),
                             (request(k=0), out, "k must be 1..16"), (request(k=17), out, "k must be 1..16"), (request(flags=2), out, "unknown flag"),
                             (request(after=(aft, None, None)), out, "must all be given, or none"),
                             (request(after=(aft, afg, None)), out, "must all be given, or none"),
                             (request(after=(None, afg, afv)), out, "must all be given, or none")):
            rc, err, _ = call(r._ctx, rq, ob, entry)
            assert rc == -1 and text in err and err.startswith("prt_trace_hits: "), (rc, err, text)
        # count == 0 writes nothing, zeroes the counters and returns 0 - whatever else the request holds
        rc, _, ctr = call(r._ctx, request(n_rays=0, origins=None, directions=None), out, entry)
        assert rc == 0 and ctr.ray_count == 0 and np.all(count == 77)
    bare = api.Renderer(0)
    try:
        for entry in (lib.prt_trace_hits, lib.prt_trace_hits_device):
            rc, err, _ = call(bare._ctx, request(), out, entry)
            assert rc == -2 and err == "prt_trace_hits: no scene uploaded"
    finally:
        bare.close()
    assert np.all(count == 77)
    for k in (0, 17):
        with pytest.raises(RuntimeError, match="k must be 1..16"):
            r.trace_hits(o, d, k)
    with pytest.raises(ValueError, match="unknown hits field"):
        r.trace_hits(o, d, 2, fields=("position",))


@pytest.mark.gpu
def test_a_scene_without_triangles(oracle):
    from par_raytracer_amd import api
    from query_grad_cases import one_triangle
    mesh, o, d, _, _ = oracle.scene("plates")
    n = len(o)
    miss = dict(hit_count=np.zeros(n, np.uint32), t=np.full((n, 4), H.FLT_MAX, np.float32), bw=np.zeros((n, 4, 3), np.float32),
                vertex0=np.full((n, 4), 0xFFFFFFFF, np.uint32), group=np.full((n, 4), -1, np.int32), back=np.zeros((n, 4), np.uint8))
    r = api.Renderer(0)
    try:
        for torch_path in (False, True):
            # hits of the same shape first, on the same context and through the same allocator: what the misses must overwrite
            upload(r, "plates")
            assert query(r, o, d, 4, torch_path, back_faces=True)["hit_count"].max() == 4
            r.upload(H.flat_desc((one_triangle()[0], np.zeros(0, np.uint32), np.zeros((0, 2), np.uint32))))
            assert r.scene_info().triangle_count == 0
            res = query(r, o, d, 4, torch_path, back_faces=True)
            assert res["counters"].ray_count == n
            H.assert_same_bits(res, miss, "no triangles (%s)" % ("torch" if torch_path else "numpy"))
    finally:
        r.close()
