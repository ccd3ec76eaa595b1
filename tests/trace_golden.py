"""Fixtures of prt_trace_rays (include/prt.h): rays and the CPU oracle's answers, tests/golden/trace_<scene>.npz.

    python tests/trace_golden.py [scene ...]        (default: every scene of SCENES below)

The answers come from tests/trace_oracle_harness.cpp, which runs oracle/prt_oracle.cpp's own TraceRay (CLOSEST) and a brute-force
IntersectRayTriangle over every triangle (OCCLUDED, and the per-ray near-tie flag).  Ray families, seeded: camera-like rays,
random origins in the bounding box with random directions, rays aimed at vertices and edge midpoints, rays aimed at points of
random triangles from their front side (on the coincident scene: the coplanar and ulp-lifted patches), misses, non-unit
directions, far-away origins aimed at triangles, non-zero ray_bias.  tests/test_trace_rays_host.py checks that the harness
reproduces every fixture; tests/test_gpu_trace_rays.py checks the device against them.
"""
from __future__ import annotations

import ctypes as C
import os
import sys
import tempfile

import numpy as np

import harness
from harness import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden")
FLT_MAX = np.float32(3.4028234663852886e38)

# scene -> rays; terrain_1m's brute force tests every one of its 1M triangles per ray
SCENES = {"cornell_box": 3072, "coincident": 3072, "icosphere_l3": 3072, "terrain_1m": 1024}
# origins of the far family lie this many scene extents from their target (there the reference's sphere test,
# raytracer.cpp:32-60, cancels and drops groups: the fixtures record TraceRay's answer, which the device replays)
FAR_EXTENTS = 1.0e4

_LIB = None


def harness_lib(out_dir: str = None) -> C.CDLL:
    """tests/trace_oracle_harness.cpp compiled with g++ (once per process)."""
    global _LIB
    if _LIB is None:
        lib = C.CDLL(harness.build_shared("trace_oracle_harness.cpp", out_dir or tempfile.mkdtemp(prefix="prt_trace_oracle_"), "trace_oracle.so"))
        lib.prt_trace_oracle_batch.restype = C.c_int
        lib.prt_trace_oracle_batch.argtypes = [C.c_void_p] + [C.c_void_p] * 4 + [C.c_uint32] + [C.c_void_p] * 10 + [C.c_int]
        _LIB = lib
    return _LIB


def oracle_batch(desc, origins, directions, ray_bias, tmax, threads: int = 0) -> dict:
    """The harness's answers for one batch (desc: a prt_scene_desc pointer)."""
    n = origins.shape[0]
    o = np.ascontiguousarray(origins, dtype=np.float32)
    d = np.ascontiguousarray(directions, dtype=np.float32)
    b = np.ascontiguousarray(ray_bias, dtype=np.float32)
    tm = np.ascontiguousarray(tmax, dtype=np.float32)
    out = {"t": np.zeros(n, np.float32), "bw": np.zeros((n, 3), np.float32), "vertex0": np.zeros(n, np.uint32),
           "group": np.zeros(n, np.int32), "position": np.zeros((n, 3), np.float32), "normal": np.zeros((n, 3), np.float32),
           "occluded": np.zeros(n, np.uint8), "occluded_tmax": np.zeros(n, np.uint8), "near_tie": np.zeros(n, np.uint8),
           "bf_t": np.zeros(n, np.float32)}
    threads = threads or min(16, os.cpu_count() or 1)
    rc = harness_lib().prt_trace_oracle_batch(
        C.cast(desc, C.c_void_p), o.ctypes.data, d.ctypes.data, b.ctypes.data, tm.ctypes.data, n,
        *[out[k].ctypes.data for k in ("t", "bw", "vertex0", "group", "position", "normal", "occluded", "occluded_tmax",
                                       "near_tie", "bf_t")], threads)
    assert rc == 0
    return out


def host_scene(name: str):
    """(ObjScene, HostScene) of scenes.SCENES[name], written to a temporary directory and loaded by the host library."""
    sys.path.insert(0, ROOT)
    from par_raytracer_amd import api, scenes
    s = scenes.make_scene(name)
    d = tempfile.mkdtemp(prefix="prt_trace_%s_" % name)
    scenes.write_obj(s, d, "scene.obj")
    return s, api.HostScene(d, "scene.obj", 0, s.camera_position)


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def make_rays(s, arrays: dict, n: int, seed: int):
    """(origins, directions, ray_bias, family) - float32, `n` rays of the families listed in the module docstring."""
    rng = np.random.default_rng(seed)
    P = arrays["positions"].astype(np.float64)
    tri = P[arrays["idx_positions"].astype(np.int64).reshape(-1, 3)]
    lo, hi = P.min(0), P.max(0)
    ext = float((hi - lo).max())
    centre = (lo + hi) / 2
    cam = np.array(s.camera_position, dtype=np.float64)
    facing = _unit(np.array(s.camera_facing, dtype=np.float64))
    fam_names = ["camera", "box", "vertex", "front", "miss", "far"]
    share = np.array([0.2, 0.2, 0.2, 0.25, 0.075, 0.075])
    counts = np.floor(share * n).astype(int)
    counts[3] += n - counts.sum()
    O, D, F = [], [], []

    def point_on_triangles(k):
        t = tri[rng.integers(0, len(tri), k)]
        uv = rng.uniform(0, 1, (k, 2))
        flip = uv.sum(1) > 1
        uv[flip] = 1 - uv[flip]
        p = t[:, 0] + uv[:, :1] * (t[:, 1] - t[:, 0]) + uv[:, 1:] * (t[:, 2] - t[:, 0])
        nrm = _unit(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]))
        return p, nrm

    # camera-like: from the scene's camera, spread around its facing
    k = counts[0]
    O.append(np.repeat(cam[None], k, 0)); D.append(_unit(facing[None] + rng.uniform(-0.6, 0.6, (k, 3)))); F += [0] * k
    # random origins in the bounding box, random directions
    k = counts[1]
    O.append(rng.uniform(lo, hi, (k, 3))); D.append(_unit(rng.normal(size=(k, 3)))); F += [1] * k
    # aimed at vertices and edge midpoints (shared edges and corners hit head-on), from the camera or from inside the box
    k = counts[2]
    t = tri[rng.integers(0, len(tri), k)]
    c = rng.integers(0, 3, k)
    mid = rng.uniform(0, 1, k) < 0.5
    target = np.where(mid[:, None], (t[np.arange(k), c] + t[np.arange(k), (c + 1) % 3]) / 2, t[np.arange(k), c])
    target = target.astype(np.float32).astype(np.float64)
    src = np.where((rng.uniform(0, 1, k) < 0.5)[:, None], cam[None], rng.uniform(lo, hi, (k, 3)))
    O.append(src); D.append(target - src); F += [2] * k
    # aimed at points of random triangles from their front side (the coplanar / lifted patches of the coincident scene)
    k = counts[3]
    p, nrm = point_on_triangles(k)
    src = p + nrm * rng.uniform(0.02, 0.5, (k, 1)) * ext + rng.normal(size=(k, 3)) * 0.1 * ext
    O.append(src); D.append(p - src); F += [3] * k
    # misses: from outside the box, pointing away from it
    k = counts[4]
    u = _unit(rng.normal(size=(k, 3)))
    src = centre[None] + u * 2.0 * ext
    O.append(src); D.append(_unit(u + rng.normal(size=(k, 3)) * 0.2)); F += [4] * k
    # far away origins aimed at triangles
    k = counts[5]
    p, nrm = point_on_triangles(k)
    dirn = _unit(-nrm + rng.normal(size=(k, 3)) * 0.3)
    src = p - dirn * FAR_EXTENTS * ext
    O.append(src); D.append(p - src); F += [5] * k

    origins = np.concatenate(O).astype(np.float32)
    directions = _unit(np.concatenate(D))
    # non-unit directions: a quarter of the rays scaled by 10^[-3, 3] (TraceRay's sphere test assumes unit length: the device
    # replays those rays in the reference's visit order, kernels_query.h query_replays)
    scale = np.where(rng.uniform(0, 1, n) < 0.25, 10.0 ** rng.uniform(-3, 3, n), 1.0)
    directions = (directions * scale[:, None]).astype(np.float32)
    # non-zero ray_bias on a quarter of the rays (two values; prt_trace_rays takes one bias per call)
    bias_values = np.array([0.0, 1e-3, 0.02], dtype=np.float32)
    ray_bias = bias_values[np.where(rng.uniform(0, 1, n) < 0.75, 0, rng.integers(1, 3, n))]
    perm = rng.permutation(n)
    return origins[perm], directions[perm], ray_bias[perm], np.array(F, dtype=np.uint8)[perm], fam_names


def generate(name: str, n: int, seed: int = 20261016) -> dict:
    s, hs = host_scene(name)
    arrays = hs.arrays()
    origins, directions, ray_bias, family, fam_names = make_rays(s, arrays, n, seed)
    first = oracle_batch(hs.desc, origins, directions, ray_bias, np.full(n, FLT_MAX, np.float32))
    # tmax around the brute-force closest t: below it, exactly it (t < tmax is false there), the next float up, above it
    rng = np.random.default_rng(seed + 1)
    bf = first["bf_t"]
    pick = rng.integers(0, 4, n)
    with np.errstate(over="ignore"):
        tmax = np.where(pick == 0, bf * np.float32(0.5), np.where(pick == 1, bf, np.where(pick == 2, np.nextafter(bf, np.float32(np.inf)),
                                                                                               bf * np.float32(2.0))))
    miss = bf >= FLT_MAX
    tmax = np.where(miss, rng.uniform(0.1, 100.0, n).astype(np.float32), tmax).astype(np.float32)
    out = oracle_batch(hs.desc, origins, directions, ray_bias, tmax)
    fx = {"scene": np.array(name), "light_mode": np.array(0), "origins": origins, "directions": directions,
          "ray_bias": ray_bias, "tmax": tmax, "family": family, "family_names": np.array(fam_names)}
    for k in ("t", "bw", "vertex0", "group", "position", "normal", "occluded", "occluded_tmax", "near_tie"):
        fx[k] = out[k]
    hit = out["group"] >= 0
    lost = hit != (out["bf_t"] < FLT_MAX)
    unit = np.abs((directions.astype(np.float64) ** 2).sum(1) - 1.0) <= 2.0 ** -18
    print("%s: %d rays, %d hits, %d occluded below tmax, %d near ties, %d where TraceRay and the brute force disagree on hit / miss "
          "(%d of them with a unit direction)" % (name, n, int(hit.sum()), int(out["occluded_tmax"].sum()), int(out["near_tie"].sum()),
                                                   int(lost.sum()), int((lost & unit).sum())))
    for f, fname in enumerate(fam_names):
        m = family == f
        print("    %-7s %5d rays, %5d hits, %4d near ties, %d disagree" % (fname, int(m.sum()), int(hit[m].sum()), int(out["near_tie"][m].sum()),
                                                                          int(lost[m].sum())))
    return fx


def main(argv):
    names = argv or list(SCENES)
    for name in names:
        fx = generate(name, SCENES[name])
        path = os.path.join(GOLDEN, "trace_%s.npz" % name)
        np.savez_compressed(path, **fx)
        print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main(sys.argv[1:])
