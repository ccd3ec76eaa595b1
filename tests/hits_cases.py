"""Shared by tests/test_hits_host.py, tests/test_gpu_hits.py and tests/test_gpu_hits_schedules.py: the plates scene and its rays, the
fixtures' rays, the runner of tests/hits_host_harness.cpp (the definition of prt_trace_hits as a brute force over every record, and
the walks of csrc/dev_hits.h, one lane at a time on the host) and the classes of rays a batch must hold.  numpy only, seeded."""
from __future__ import annotations

import struct

import numpy as np

import harness
import trace_cases as T
from query_grad_cases import flat_desc, scene_mesh       # noqa: F401  (re-exported)

FIELDS = ("hit_count", "t", "bw", "vertex0", "group", "back")
DTYPES = dict(hit_count=np.uint32, t=np.float32, bw=np.float32, vertex0=np.uint32, group=np.int32, back=np.uint8)
FLT_MAX = np.float32(3.4028234663852886e38)
MAX_HITS = 16
KS = (1, 2, 3, 8, 16)
PLATES = 24
PLATE_STEP = 0.25
DOUBLED = (3, 10, 17)                   # the plates that lie in group 1 as well, with the same corner order: their keys tie on t
FULL = 64                               # candidates per ray the harness lists in key order (the plates hold 54 records)
ROUTE_NONE, ROUTE_WALK, ROUTE_FAR, ROUTE_OVERFLOW = 0, 1, 2, 3


# ---- the plates scene

def plates():
    """24 parallel quads of 2 triangles, [-1, 1]^2 at z = 0.25 j, facing +z for even j and -z for odd j; group 0 holds all of them,
    group 1 the plates of DOUBLED again."""
    corners = np.array([[-1, -1], [1, -1], [1, 1], [-1, 1]], np.float32)
    p = np.concatenate([np.concatenate([corners, np.full((4, 1), PLATE_STEP * j, np.float32)], axis=1) for j in range(PLATES)]).astype(np.float32)

    def quad(j):
        b = 4 * j
        return [b, b + 1, b + 2, b, b + 2, b + 3] if j % 2 == 0 else [b, b + 2, b + 1, b, b + 3, b + 2]
    g0 = [i for j in range(PLATES) for i in quad(j)]
    g1 = [i for j in DOUBLED for i in quad(j)]
    return (np.ascontiguousarray(p), np.array(g0 + g1, np.uint32), np.array([[0, len(g0)], [len(g0), len(g1)]], np.uint32))


def plate_rays(seed=5):
    """(origins, directions, kind): rays down and up the axis from outside the stack, through the quads' shared diagonal,
    obliquely from a sphere around the stack, from between the plates, from a far origin, with a direction whose products
    overflow, and rays that are misses by definition."""
    rng = np.random.default_rng(seed)
    top = PLATE_STEP * (PLATES - 1)
    o, d, kind = [], [], []

    def add(oo, dd, name):
        o.append(np.asarray(oo, np.float32).reshape(-1, 3)); d.append(np.asarray(dd, np.float32).reshape(-1, 3))
        kind.extend([name] * len(o[-1]))
    for sign in (-1.0, 1.0):
        xy = rng.uniform(-0.9, 0.9, (64, 2))
        z = np.full((64, 1), top + 2.25 if sign < 0 else -3.0)
        add(np.concatenate([xy, z], 1), np.tile([0.0, 0.0, sign], (64, 1)), "axis")
        u = rng.uniform(-0.9, 0.9, (32, 1)).astype(np.float32)
        add(np.concatenate([u, u, z[:32]], 1), np.tile([0.0, 0.0, sign], (32, 1)), "diagonal")
    centre = np.array([0.0, 0.0, top / 2])
    v = rng.standard_normal((256, 3))
    src = centre + 8.0 * v / np.linalg.norm(v, axis=1, keepdims=True)
    dst = np.concatenate([rng.uniform(-1.0, 1.0, (256, 2)), rng.uniform(0.0, top, (256, 1))], 1)
    dirs = dst - src
    add(src, dirs / np.linalg.norm(dirs, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, (256, 1)), "oblique")
    v = rng.standard_normal((64, 3))
    add(np.concatenate([rng.uniform(-0.8, 0.8, (64, 2)), rng.uniform(0.0, top, (64, 1))], 1), v / np.linalg.norm(v, axis=1, keepdims=True), "between")
    xy = rng.uniform(-0.9, 0.9, (16, 2))
    add(np.concatenate([xy, np.full((16, 1), 2000.0)], 1), np.tile([0.0, 0.0, -1.0], (16, 1)), "far")
    xy = rng.uniform(-0.9, 0.9, (16, 2))
    add(np.concatenate([xy, np.full((16, 1), 5.0e4)], 1), np.tile([0.0, 0.0, -(2.0 ** 120)], (16, 1)), "overflow")
    bad_o = np.tile([0.1, 0.2, 8.0], (8, 1)).astype(np.float32)
    bad_d = np.tile([0.0, 0.0, -1.0], (8, 1)).astype(np.float32)
    bad_o[0, 0] = np.nan; bad_d[1, 2] = np.inf; bad_d[2] = 0.0; bad_o[3, 1] = -np.inf
    bad_o[4, 2] = np.nan; bad_d[5, 0] = -np.inf; bad_d[6] = 0.0; bad_d[7, 1] = np.nan
    add(bad_o, bad_d, "invalid")
    return np.ascontiguousarray(np.concatenate(o)), np.ascontiguousarray(np.concatenate(d)), np.array(kind)


TMAX_LANES = ("own", "inf", "zero", "negative", "nan", "-inf", "flt_max", "own")


def tmax_specials(n, seed=9, lo=1.0, hi=12.0):
    """(tmax, lane): by ray i % 8 a limit of its own (uniform in lo..hi), +inf, 0, -1, NaN, -inf, FLT_MAX, a limit of its own."""
    lane = np.arange(n) % 8
    special = np.array([0.0, np.inf, 0.0, -1.0, np.nan, -np.inf, FLT_MAX, 0.0], np.float32)[lane]
    own = np.random.default_rng(seed).uniform(lo, hi, n).astype(np.float32)
    return np.where((lane == 0) | (lane == 7), own, special).astype(np.float32), lane


def fixture_rays(name):
    """The bias-0 rays of the committed ray fixture, with the fixture's tmax."""
    g = T.fixture(name)
    sel = T.bias0(g)
    return (np.ascontiguousarray(g["origins"][sel], np.float32), np.ascontiguousarray(g["directions"][sel], np.float32),
            np.ascontiguousarray(g["tmax"][sel], np.float32))


# ---- the host harness

def build_harness(directory, sanitize=False, bvh8=False):
    return harness.build("hits_host_harness.cpp", directory, "hits_host" + ("8" if bvh8 else "") + ("_san" if sanitize else ""),
                         sanitize=sanitize, bvh8=bvh8, sources=("bvh_build.cpp",))


def case(mesh, origins, directions, k, tmax=None, back_faces=False, after=None, ray_bias=0.0, full=0, stack_cap=0):
    """after: (after_t, after_group, after_vertex0) per ray, or None."""
    return dict(mesh=mesh, origins=np.ascontiguousarray(origins, np.float32), directions=np.ascontiguousarray(directions, np.float32), k=int(k),
                tmax=tmax, back_faces=bool(back_faces), after=after, ray_bias=float(ray_bias), full=int(full), stack_cap=int(stack_cap))


def run_harness(exe, cases, directory):
    """Every case through the harness in one run.  Per case a dict: mismatches, lane_mismatches, node_visits, tri_tests, "brute" and
    "walk" ({field: array}, shaped (n,), (n, k) and (n, k, 3)), remaining, route, listed (per ray) and, with full > 0, "full": t, group,
    vertex0, back of the first `full` remaining candidates in key order, (n, full) each."""
    fin, fout = harness.case_files(directory, "hits_cases.bin", "hits_results.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for c in cases:
            p, idx, runs = c["mesh"]
            n = c["origins"].shape[0]
            flags = (1 if c["tmax"] is not None else 0) | (2 if c["back_faces"] else 0) | (4 if c["after"] is not None else 0)
            f.write(struct.pack("<8If", n, p.shape[0], idx.size, runs.shape[0], flags, c["k"], c["full"], c["stack_cap"], c["ray_bias"]))
            harness.put(f, (c["origins"], np.float32), (c["directions"], np.float32))
            if c["tmax"] is not None:
                harness.put(f, (c["tmax"], np.float32))
            if c["after"] is not None:
                harness.put(f, (c["after"][0], np.float32), (c["after"][1], np.int32), (c["after"][2], np.uint32))
            harness.put(f, (p, np.float32), (idx, np.uint32), (runs, np.uint32))
    harness.run(exe, fin, fout)
    r, out = harness.Reader.of_file(fout), []
    for c in cases:
        n, k, full = c["origins"].shape[0], c["k"], c["full"]
        mism, lane_mism, nodes, tris = r.unpack("<iiQQ")
        res = dict(mismatches=mism, lane_mismatches=lane_mism, node_visits=nodes, tri_tests=tris)
        for which in ("brute", "walk"):
            res[which] = dict(hit_count=r.take(n, np.uint32), t=r.take(n * k, np.float32, (n, k)), bw=r.take(3 * n * k, np.float32, (n, k, 3)),
                              vertex0=r.take(n * k, np.uint32, (n, k)), group=r.take(n * k, np.int32, (n, k)), back=r.take(n * k, np.uint8, (n, k)))
        res["remaining"], res["route"], res["listed"] = r.take(n, np.uint32), r.take(n, np.uint32), r.take(n, np.uint32)
        res["full"] = dict(t=r.take(n * full, np.float32, (n, full)), group=r.take(n * full, np.int32, (n, full)),
                           vertex0=r.take(n * full, np.uint32, (n, full)), back=r.take(n * full, np.uint8, (n, full)))
        out.append(res)
    r.done()
    return out


def assert_same_bits(got, expect, what, fields=FIELDS):
    harness.assert_same_bits(got, expect, what, fields)


def to_numpy(res):
    """A trace_hits result with torch tensors -> numpy arrays (hit_count and vertex0 back to uint32)."""
    return harness.to_numpy(res, ("vertex0", "hit_count"))


def last_filled(res):
    """The cursor that continues behind a result: (t, group, vertex0) of each ray's last filled slot; a ray without a hit gets
    (+inf, 0, 0), behind which nothing remains (every accepted t is finite)."""
    n, k = res["t"].shape
    count = np.asarray(res["hit_count"]).astype(np.int64)
    at = np.maximum(count - 1, 0)
    rows = np.arange(n)
    some = count > 0
    return (np.where(some, res["t"][rows, at], np.float32(np.inf)).astype(np.float32), np.where(some, res["group"][rows, at], 0).astype(np.int32),
            np.where(some, res["vertex0"][rows, at], 0).astype(np.uint32))


# ---- the classes a set of cases must hold (asserted from the brute force's own output)

CLASSES = ("fewer than k", "exactly k", "more than k", "equal t across the cut", "equal t inside the list", "back between fronts",
           "miss by definition", "far origin", "overflow")


def classes_of(c, r):
    """{class: number of rays} of case c with harness result r (full >= k + 1 for the cut class)."""
    b, k = r["brute"], c["k"]
    o, d = c["origins"].astype(np.float32), c["directions"].astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        ob = o + d * np.float32(c["ray_bias"])
        invalid = ~(np.isfinite(o).all(1) & np.isfinite(d).all(1) & np.isfinite(ob).all(1)) | (d == 0).all(1)
    rem = r["remaining"].astype(np.int64)
    out = {"fewer than k": int(((rem < k) & (rem > 0)).sum()), "exactly k": int((rem == k).sum()), "more than k": int((rem > k).sum()),
           "miss by definition": int(invalid.sum()), "far origin": int((r["route"] == ROUTE_FAR).sum()),
           "overflow": int((r["route"] == ROUTE_OVERFLOW).sum())}
    assert not np.any(b["hit_count"][invalid]) and not np.any(r["route"][invalid])
    cut = np.zeros(len(rem), bool)
    if c["full"] > k:
        cut = (rem > k) & (r["full"]["t"][:, k - 1].view(np.uint32) == r["full"]["t"][:, k].view(np.uint32))
    out["equal t across the cut"] = int(cut.sum())
    slot = np.arange(k)[None, :]
    filled = slot < b["hit_count"][:, None]
    tb = b["t"].view(np.uint32)
    inside = (tb[:, :-1] == tb[:, 1:]) & filled[:, 1:] if k > 1 else np.zeros((len(rem), 0), bool)
    out["equal t inside the list"] = int(inside.any(1).sum())
    if k > 2:
        mid = (b["back"][:, :-2] == 0) & (b["back"][:, 1:-1] == 1) & (b["back"][:, 2:] == 0) & filled[:, 2:]
        out["back between fronts"] = int(mid.any(1).sum())
    else:
        out["back between fronts"] = 0
    return out
