"""Shared by tests/test_trace_cases_host.py and tests/test_gpu_trace_rays_schedules.py: batches cut from the committed ray fixtures
(tests/golden/trace_*.npz) that put prt_trace_rays' scheduling under test - whole waves and chunks of one kind of ray, batches
longer than one pass of the grids, special tmax values - each with the answers the fixture (that is: the CPU oracle) already holds
for its rays.  numpy only.  No ray is made up here except the invalid ones (a miss by definition, include/prt.h).

Every builder works on the rays of a fixture whose ray_bias is 0, so that a case is one call, and returns a dict: origins, directions,
tmax, the expected fields (CLOSEST's six, occluded = no limit, occluded_tmax = below tmax) and, where it applies, a label per ray."""
from __future__ import annotations

import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FLT_MAX = np.float32(3.4028234663852886e38)
CLOSEST = ("t", "bw", "vertex0", "group", "position", "normal")
EXPECTED = CLOSEST + ("occluded", "occluded_tmax")
RAYS = ("origins", "directions", "tmax")
FIXTURES = ("cornell_box", "coincident", "icosphere_l3")
BIAS0_RAYS = 2300                      # of the 3,072 rays of each of FIXTURES
CLASSES = ("replay", "near_tie", "plain_hit", "miss")
INVALID = "invalid"
# k_query sends a CLOSEST ray to the replay list when its float32 |d|^2 is further than 2^-18 from 1 (kernels_query.h
# query_replays).  Any float32 evaluation of d.d is within 3 x 2^-24 of the exact one, so a ray whose |d.d - 1| here is above
# 2^-17 is listed and one below 2^-19 is not, however the device rounds; what lies between is class "rest".
REPLAY_ABOVE = np.float32(2.0 ** -17)
UNIT_BELOW = np.float32(2.0 ** -19)


def fixture(name):
    return np.load(os.path.join(GOLDEN, "trace_%s.npz" % name), allow_pickle=False)


def bias0(g):
    """Indices of the fixture's rays with ray_bias == 0, in the fixture's order."""
    return np.nonzero(g["ray_bias"] == 0)[0]


def rows(g, sel):
    """Rays `sel` of fixture g and the fixture's answers for them, as a case."""
    out = {k: np.ascontiguousarray(g[k][sel]) for k in RAYS + EXPECTED}
    out["index"] = np.asarray(sel)
    return out


def classes(g):
    """{class: indices into the fixture} over the bias-0 rays, by the route k_query sends a CLOSEST ray: `replay` (far family, or a
    direction that is not unit length), `near_tie`, `plain_hit`, `miss`, and `rest` - the rays the margins leave undecided."""
    sel = bias0(g)
    d = g["directions"][sel].astype(np.float32)
    off = np.abs((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] - np.float32(1.0))
    far = g["family"][sel] == list(g["family_names"]).index("far")
    replay = far | (off > REPLAY_ABOVE)
    unit = ~replay & (off < UNIT_BELOW)
    tie = g["near_tie"][sel] != 0
    hit = g["group"][sel] >= 0
    out = {"replay": sel[replay], "near_tie": sel[unit & tie], "plain_hit": sel[unit & ~tie & hit], "miss": sel[unit & ~tie & ~hit],
           "rest": sel[~replay & ~unit]}
    assert sum(len(v) for v in out.values()) == len(sel)
    return out


def invalid_rays(g, n):
    """n rays that are misses by definition: the first bias-0 rays with, cycling, a NaN origin component, an infinite direction
    component, a zero direction, a -inf origin component - and the documented miss as their expected rows."""
    base = bias0(g)[np.arange(n) % len(bias0(g))]
    o, d = g["origins"][base].copy(), g["directions"][base].copy()
    kind = np.arange(n) % 4
    o[kind == 0, 0] = np.nan
    d[kind == 1, 2] = np.inf
    d[kind == 2] = 0.0
    o[kind == 3, 1] = -np.inf
    return {"origins": o, "directions": d, "tmax": np.ascontiguousarray(g["tmax"][base]), "t": np.full(n, FLT_MAX, np.float32),
            "bw": np.zeros((n, 3), np.float32), "vertex0": np.full(n, 0xFFFFFFFF, np.uint32), "group": np.full(n, -1, np.int32),
            "position": np.zeros((n, 3), np.float32), "normal": np.zeros((n, 3), np.float32), "occluded": np.zeros(n, np.uint8),
            "occluded_tmax": np.zeros(n, np.uint8), "index": np.full(n, -1)}


def concat(cases):
    return {k: np.ascontiguousarray(np.concatenate([c[k] for c in cases])) for k in RAYS + EXPECTED + ("index",)}


def take(case, order):
    """The case's rays in another order (or a subset), every array alike."""
    return {k: np.ascontiguousarray(v[order]) for k, v in case.items()}


def sorted_by_kind(g, per=192):
    """`per` rays of each class of CLASSES that has that many, then `per` invalid rays: whole waves and (at the default 128-ray
    chunks) whole chunks of one kind, the class boundaries inside a chunk.  case["kind"]: the class name per ray."""
    cls = classes(g)
    used = [c for c in CLASSES if len(cls[c]) >= per]
    parts = [rows(g, cls[c][:per]) for c in used] + [invalid_rays(g, per)]
    case = concat(parts)
    case["kind"] = np.repeat(np.array(used + [INVALID]), per)
    return case


def tiled(g, n):
    """The bias-0 rays repeated cyclically to n rays."""
    sel = bias0(g)
    return rows(g, sel[np.arange(n) % len(sel)])


def tmax_specials(g, n=1024):
    """The first n bias-0 rays with tmax by lane i % 8: the fixture's, +inf, 0, -1, NaN, -inf, FLT_MAX, the fixture's.
    Only the rays: the expected answers are the oracle harness's (expect_from_oracle)."""
    sel = bias0(g)[:n]
    lane = np.arange(len(sel)) % 8
    special = np.array([0.0, np.inf, 0.0, -1.0, np.nan, -np.inf, FLT_MAX, 0.0], np.float32)[lane]
    tmax = np.where((lane == 0) | (lane == 7), g["tmax"][sel], special).astype(np.float32)
    return {"origins": np.ascontiguousarray(g["origins"][sel]), "directions": np.ascontiguousarray(g["directions"][sel]), "tmax": tmax,
            "index": sel, "lane": lane}


def expect_from_oracle(case, desc):
    """The case with its expected fields filled in by tests/trace_oracle_harness.cpp (TraceRay; brute force `t < tmax`)."""
    import trace_golden
    n = len(case["origins"])
    out = trace_golden.oracle_batch(desc, case["origins"], case["directions"], np.zeros(n, np.float32), case["tmax"])
    full = dict(case)
    full.update({k: out[k] for k in EXPECTED})
    return full


def as_fixture(case, g):
    """The case with the keys of a fixture file, for helpers that take one (test_gpu_trace_rays.check_fixture): ray_bias 0
    everywhere, and the fixture's scene, near_tie and family per ray (0 for the invalid rays, which the fixture does not hold)."""
    idx = case["index"]
    known = idx >= 0
    out = dict(case)
    out["scene"] = g["scene"]
    out["ray_bias"] = np.zeros(len(idx), np.float32)
    for k in ("near_tie", "family"):
        out[k] = np.where(known, g[k][np.where(known, idx, 0)], 0).astype(g[k].dtype)
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype in (np.float32, np.int32) else a


def differing(got, expect):
    """Indices of the rays on which `got` and `expect` differ in any bit."""
    got, expect = bits(got), bits(expect)
    assert got.shape == expect.shape and got.dtype == expect.dtype, (got.shape, expect.shape, got.dtype, expect.dtype)
    return np.nonzero(np.any((got != expect).reshape(len(expect), -1), axis=1))[0]
