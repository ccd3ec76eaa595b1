"""What the tests of prt_render_rays (include/prt.h) share: the CPU yardstick, the rays, the domain.

tests/radiance_oracle_harness.cpp includes oracle/prt_oracle.cpp unchanged and runs THE DEFINITION of prt.h with the oracle's own
Random_Seed, Random_NextFloat11 and TraceRayColor (oracle_batch), and makes RenderPixel's jittered camera rays (camera_rays).
tests/test_radiance_host.py proves the yardstick against oracle_py.render; tests/test_gpu_render_rays.py holds the device to it.

Rays (make_rays): per output `spp` rays of one family - random origins in the scene's bounding box with random unit directions,
origins outside the box aimed at a point inside it, and origins outside it pointing away (misses).  in_domain restates the
library's domain test in numpy, float32 operation by float32 operation.
"""
from __future__ import annotations

import ctypes as C
import os
import tempfile

import numpy as np

import harness

SCENES = ("cornell_box", "many_materials", "coincident", "textured_gallery")
# RGB against the harness: what tests/test_gpu_parity.py applies against the reference (README "Parity")
TOL = 1e-4
SEEDS = {"cornell_box": 101, "many_materials": 202, "coincident": 303, "textured_gallery": 404}

_LIB = None


def harness_lib() -> C.CDLL:
    """tests/radiance_oracle_harness.cpp compiled with g++ (once per process)."""
    global _LIB
    if _LIB is None:
        lib = C.CDLL(harness.build_shared("radiance_oracle_harness.cpp", tempfile.mkdtemp(prefix="prt_radiance_oracle_"), "radiance_oracle.so"))
        lib.prt_radiance_oracle_batch.restype = C.c_int
        lib.prt_radiance_oracle_batch.argtypes = [C.c_void_p] * 4 + [C.c_uint32, C.c_uint64, C.c_int] + [C.c_void_p] * 5 + [C.c_int]
        lib.prt_radiance_camera_rays.restype = C.c_int
        lib.prt_radiance_camera_rays.argtypes = [C.c_void_p, C.c_uint64] + [C.c_uint32] * 4 + [C.c_void_p] * 2
        _LIB = lib
    return _LIB


def oracle_batch(desc, params, origins, directions, first: int = 0, camera_stream: bool = False) -> dict:
    """The definition on the CPU.  origins, directions: (count, spp, 3).  Returns rgba (count, 4), ray_count and shaded_hits (sums over
    the batch), rays_per_output and shaded_per_output, primary_hit and translucent (count, spp)."""
    o = np.ascontiguousarray(origins, dtype=np.float32)
    d = np.ascontiguousarray(directions, dtype=np.float32)
    count, spp = o.shape[0], int(params.spp)
    assert o.shape == (count, spp, 3) and d.shape == o.shape
    rgba = np.zeros((count, 4), np.float32)
    rays, shaded = np.zeros(count, np.uint64), np.zeros(count, np.uint64)
    hit, tr = np.zeros((count, spp), np.uint8), np.zeros((count, spp), np.uint8)
    rc = harness_lib().prt_radiance_oracle_batch(C.cast(desc, C.c_void_p), C.cast(C.pointer(params), C.c_void_p), o.ctypes.data, d.ctypes.data,
                                                 count, int(first), int(bool(camera_stream)), rgba.ctypes.data, rays.ctypes.data,
                                                 shaded.ctypes.data, hit.ctypes.data, tr.ctypes.data, min(16, os.cpu_count() or 1))
    assert rc == 0, rc
    return {"rgba": rgba, "ray_count": int(rays.sum()), "rays_per_output": rays, "shaded_hits": int(shaded.sum()), "shaded_per_output": shaded,
            "primary_hit": hit, "translucent": tr}


def camera_rays(cam, seed: int, width: int, p0: int, n: int, spp: int):
    """RenderPixel's jittered rays of pixels [p0, p0 + n): (origins, directions), each (n, spp, 3)."""
    o, d = np.zeros((n, spp, 3), np.float32), np.zeros((n, spp, 3), np.float32)
    rc = harness_lib().prt_radiance_camera_rays(C.cast(C.pointer(cam), C.c_void_p), int(seed), int(width), int(p0), int(n), int(spp),
                                                o.ctypes.data, d.ctypes.data)
    assert rc == 0
    return o, d


def scene_abs_max(arrays: dict) -> np.float32:
    """The largest |coordinate| of a triangle corner: the library's extent of the scene."""
    P = arrays["positions"].reshape(-1, 3)[arrays["idx_positions"].astype(np.int64).reshape(-1)]
    return np.float32(np.abs(P.astype(np.float32)).max())


def in_domain(origins, directions, ray_bias, abs_max) -> np.ndarray:
    """The DOMAIN of include/prt.h, per ray, in float32 as the library computes it."""
    f = np.float32
    o, d = np.asarray(origins, f).reshape(-1, 3), np.asarray(directions, f).reshape(-1, 3)
    with np.errstate(all="ignore"):
        ob = o + d * f(ray_bias)
        finite = np.isfinite(o).all(1) & np.isfinite(d).all(1) & np.isfinite(ob).all(1)
        l2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]             # Dot, mathlib.h:236
        unit = (l2 >= f(1.0) - f(2.0 ** -18)) & (l2 <= f(1.0) + f(2.0 ** -18))
        near = np.abs(o).max(1) <= f(64.0) * f(abs_max)
    return finite & unit & near


def unit32(v) -> np.ndarray:
    """float32 directions of unit length as the domain wants it: normalised in float64, rounded once."""
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


def make_rays(arrays: dict, count: int, spp: int, seed: int, scale: float = 1.0):
    """(origins, directions, family): (count, spp, 3) float32 twice and (count,) uint8 - 0 box, 1 aimed from outside, 2 miss.
    scale: how far, in scene extents, the outside origins lie from the centre."""
    rng = np.random.default_rng(seed)
    P = arrays["positions"].reshape(-1, 3)[arrays["idx_positions"].astype(np.int64).reshape(-1)].astype(np.float64)
    lo, hi = P.min(0), P.max(0)
    ext = float((hi - lo).max())
    centre = (lo + hi) / 2
    family = (np.arange(count) % 4 % 3).astype(np.uint8)             # 0 1 2 0 | 0 1 2 0 ...: half box, a quarter each of the others
    rng.shuffle(family)
    fam = np.repeat(family[:, None], spp, 1)
    n = count * spp
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    box_o = rng.uniform(lo, hi, (n, 3))
    out_o = centre[None] + u * 1.5 * ext * scale
    target = rng.uniform(lo + 0.1 * (hi - lo), hi - 0.1 * (hi - lo), (n, 3))
    v = rng.normal(size=(n, 3))
    f = fam.reshape(-1)[:, None]
    origins = np.where(f == 0, box_o, out_o).astype(np.float32)
    dirs = np.where(f == 0, v, np.where(f == 1, target - origins.astype(np.float64), u + 0.2 * v))
    return origins.reshape(count, spp, 3), unit32(dirs).reshape(count, spp, 3), family


def far_rays(arrays: dict, count: int, spp: int, seed: int, factor: float):
    """Rays from `factor` times the scene's largest |coordinate| away from the world's origin, aimed into the scene's box."""
    rng = np.random.default_rng(seed)
    P = arrays["positions"].reshape(-1, 3)[arrays["idx_positions"].astype(np.int64).reshape(-1)].astype(np.float64)
    lo, hi = P.min(0), P.max(0)
    n = count * spp
    u = np.sign(rng.normal(size=(n, 3))) * rng.uniform(0.8, 1.0, (n, 3))
    u /= np.abs(u).max(1, keepdims=True)                             # the largest |component| is exactly the factor
    origins = (u * factor * float(scene_abs_max(arrays)) * 0.999).astype(np.float32)
    target = rng.uniform(lo + 0.1 * (hi - lo), hi - 0.1 * (hi - lo), (n, 3))
    return origins.reshape(count, spp, 3), unit32(target - origins.astype(np.float64)).reshape(count, spp, 3)


def assert_mixed(exp: dict, name: str, want_translucent: bool = False) -> None:
    """The batch exercises what it is meant to: hits and misses among the primary rays, bounce and shadow rays behind them, at
    least three output colours, and - where asked - a sample whose walk crossed a translucent hit."""
    hit = exp["primary_hit"]
    assert hit.any() and not hit.all(), name
    assert exp["ray_count"] > hit.size, name
    assert len(np.unique(exp["rgba"][:, :3].view(np.uint32), axis=0)) >= 3, name
    if want_translucent:
        assert exp["translucent"].any(), name
