"""Shared by tests/test_hemi_host.py and tests/test_gpu_hemi.py: the runner of tests/hemi_host_harness.cpp (the definition of
prt_hemisphere_visibility with the functions of csrc/dev_hemi.h and csrc/hammersley.h, every ray answered by a brute force over all
triangles and by the device traversal compiled for the host), the point sets, and plain numpy restatements of the pieces the
definition names: prt_sample_key, the generator's seed and first draw, and the cosine lobe's table as it was written before it
moved into csrc/hammersley.h."""
from __future__ import annotations

import ctypes
import ctypes.util
import os
import struct

import numpy as np

import closest_cases as K
import harness
import signed_cases as S

FIELDS = ("unoccluded", "visibility", "bent")
INVALID = np.uint32(0xFFFFFFFF)
RAY_BIAS = np.float32(1e-3)


def build_harness(directory, bvh8=False):
    return harness.build("hemi_host_harness.cpp", directory, "hemi_host" + ("_bvh8" if bvh8 else ""), bvh8=bvh8, sources=("bvh_build.cpp",))


def case(mesh, points, normals, samples, seed=0, first=0, ray_bias=RAY_BIAS, max_dist=None):
    points, normals = np.ascontiguousarray(points, np.float32), np.ascontiguousarray(normals, np.float32)
    assert points.shape == normals.shape and points.ndim == 2 and points.shape[1] == 3
    if max_dist is not None:
        max_dist = np.ascontiguousarray(max_dist, np.float32)
        assert max_dist.shape == (points.shape[0],)
    return dict(mesh=mesh, points=points, normals=normals, samples=int(samples), seed=int(seed), first=int(first),
                ray_bias=np.float32(ray_bias), max_dist=max_dist)


def run_harness(exe, cases, directory, tag="hemi"):
    """Every case through the harness in one run.  Per case a dict: per ray "k" (n, samples), "dirs" (n, samples, 3), "brute" and
    "walk" (n, samples: 1 = unoccluded); per point the three FIELDS and "sums" (n, 3 int64); "cast" = the rays cast."""
    fin, fout = harness.case_files(directory, tag + "_cases.bin", tag + "_results.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for c in cases:
            p, idx, runs = c["mesh"]
            n = c["points"].shape[0]
            f.write(struct.pack("<8I", p.shape[0], idx.size, n, c["samples"], 1 if c["max_dist"] is not None else 0, 0, 0, 0))
            f.write(struct.pack("<2Q2f", c["seed"], c["first"], float(c["ray_bias"]), 0.0))
            harness.put(f, (p, np.float32), (idx, np.uint32))
            f.write(c["points"].tobytes() + c["normals"].tobytes())
            if c["max_dist"] is not None:
                f.write(c["max_dist"].tobytes())
    harness.run(exe, fin, fout)
    r, out = harness.Reader.of_file(fout), []
    for c in cases:
        n, s = c["points"].shape[0], c["samples"]
        out.append(dict(k=r.take(n * s, np.uint32, (n, s)), dirs=r.take(3 * n * s, np.float32, (n, s, 3)),
                        brute=r.take(n * s, np.uint8, (n, s)), walk=r.take(n * s, np.uint8, (n, s)),
                        unoccluded=r.take(n, np.uint32), visibility=r.take(n, np.float32), bent=r.take(3 * n, np.float32, (n, 3)),
                        sums=r.take(3 * n, np.int64, (n, 3)), cast=r.unpack("<Q")[0]))
    r.done()
    return out


def harness_table(exe, directory):
    """The 1024 entries of DevScene::diffuse_dirs as csrc/hammersley.h computes them with the host's libm: (1024, 4) float32."""
    fout = os.path.join(str(directory), "hemi_table.bin")
    harness.run(exe, "--table", fout)
    r = harness.Reader.of_file(fout)
    table = r.take(4096, np.float32, (1024, 4))
    r.done()
    return table


def assert_same_bits(got, expect, what, fields=FIELDS):
    """Every field of `got` ({field: numpy array}) equals `expect` bit for bit."""
    harness.assert_same_bits(got, expect, what, fields)


def to_numpy(res):
    """A hemisphere_visibility result with torch tensors -> numpy arrays (unoccluded back to uint32)."""
    return harness.to_numpy(res, ("unoccluded",))


# ---- the definition's pieces in plain numpy (uint64 arithmetic wraps)

M64 = (1 << 64) - 1


def sample_key(seed, pixel, sample):
    """include/prt_key.h in Python integers."""
    z = (seed + 0x9E3779B97F4A7C15 * ((((pixel & 0xFFFFFFFF) << 16) | (sample & 0xFFFF)) + 1)) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def first_draw(key):
    """The reference generator (random.h) seeded with `key`, its first draw, in Python integers: Random_Seed's xorshift chain
    (three right shifts) gives the state words, the draw mixes words 0 and 1."""
    def chain_step(x):
        x ^= x >> 12
        x ^= x >> 25
        x ^= x >> 27
        return x
    if key == 0:
        key = 0x5555555555555555
    c0 = chain_step(key)
    s0 = (c0 * 2685821657736338717) & M64                   # state[0]
    s1 = (chain_step(c0) * 2685821657736338717) & M64       # state[1]
    s1 ^= (s1 << 31) & M64
    s1 ^= s1 >> 11
    s0 &= s0 >> 30                                          # (sic)
    return ((s0 ^ s1) * 1181783497276652981) & M64


def hemi_index(seed, j, s):
    return first_draw(sample_key(seed, j, s)) % 1024


def libm():
    lib = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    for name in ("cosf", "sinf"):
        getattr(lib, name).restype = ctypes.c_float
        getattr(lib, name).argtypes = [ctypes.c_float]
    return lib


def table_before_the_move():
    """The table as csrc/prt_api.hip computed it before the functions moved (radical_inverse_vdc and diffuse_tangent_dir, pasted
    here as numpy float32 arithmetic; cosf and sinf are the host's libm, called through ctypes): (1024, 4) float32."""
    f32 = np.float32
    lm = libm()
    i = np.arange(1024, dtype=np.uint32)
    bits = i.copy()
    bits = (bits << np.uint32(16)) | (bits >> np.uint32(16))
    bits = ((bits & np.uint32(0x55555555)) << np.uint32(1)) | ((bits & np.uint32(0xAAAAAAAA)) >> np.uint32(1))
    bits = ((bits & np.uint32(0x33333333)) << np.uint32(2)) | ((bits & np.uint32(0xCCCCCCCC)) >> np.uint32(2))
    bits = ((bits & np.uint32(0x0F0F0F0F)) << np.uint32(4)) | ((bits & np.uint32(0xF0F0F0F0)) >> np.uint32(4))
    bits = ((bits & np.uint32(0x00FF00FF)) << np.uint32(8)) | ((bits & np.uint32(0xFF00FF00)) >> np.uint32(8))
    xi_y = (bits.astype(np.float64) * 2.3283064365386963e-10).astype(f32)
    xi_x = i.astype(f32) / f32(1024)
    phi = xi_y * f32(2.0) * f32(3.1415927)
    assert phi.dtype == f32
    cp = np.array([lm.cosf(float(x)) for x in phi], f32)
    sp = np.array([lm.sinf(float(x)) for x in phi], f32)
    ct = np.sqrt(f32(1.0) - xi_x)
    st = np.sqrt(f32(1.0) - ct * ct)
    assert ct.dtype == f32 and st.dtype == f32
    return np.stack([cp * st, sp * st, ct, np.zeros(1024, f32)], -1)


# ---- point sets: (points, normals), float32

def face_normals(mesh):
    p, idx, runs = mesh
    tri = idx.reshape(-1, 3).astype(np.int64)
    P = p.astype(np.float64)
    cr = np.cross(P[tri[:, 1]] - P[tri[:, 0]], P[tri[:, 2]] - P[tri[:, 0]])
    return cr / np.linalg.norm(cr, axis=1, keepdims=True)


def surface_points(mesh, n, seed):
    """n points on random triangles (random barycentrics, kept off the edges) with the faces' unit normals."""
    p, idx, runs = mesh
    rng = np.random.default_rng(seed)
    tri = idx.reshape(-1, 3).astype(np.int64)
    t = rng.integers(0, tri.shape[0], n)
    bw = rng.uniform(0.05, 1.0, (n, 3))
    bw /= bw.sum(1, keepdims=True)
    P = p.astype(np.float64)
    pts = (bw[:, :, None] * P[tri[t]]).sum(1)
    nrm = face_normals(mesh)[t].astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True).astype(np.float32)
    return np.ascontiguousarray(pts, np.float32), np.ascontiguousarray(nrm, np.float32)


def off_surface_points(mesh, n, seed):
    """n points in 1.5 x the bounding box (same centre) with random unit normals."""
    rng = np.random.default_rng(seed)
    lo, hi, _ = K.mesh_extent(mesh)
    pts = 0.5 * (lo + hi) + rng.uniform(-0.75, 0.75, (n, 3)) * (hi - lo)
    nrm = rng.standard_normal((n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm = nrm.astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True).astype(np.float32)
    return np.ascontiguousarray(pts, np.float32), np.ascontiguousarray(nrm, np.float32)


def mixed_points(mesh, n, seed):
    """Half on the surface, half off it (at least one of each from n = 2 on), interleaved."""
    n_on = (n + 1) // 2
    a, an = surface_points(mesh, n_on, seed)
    b, bn = off_surface_points(mesh, n - n_on, seed + 1)
    pts, nrm = np.empty((n, 3), np.float32), np.empty((n, 3), np.float32)
    pts[0::2], nrm[0::2] = a, an
    pts[1::2], nrm[1::2] = b, bn
    return pts, nrm


def assert_input_mix(expect, samples, what):
    """The condition on a scene's inputs: the expected counts of its valid points take at least three distinct values, and some
    point is partly occluded."""
    u = expect["unoccluded"][expect["unoccluded"] != INVALID]
    assert len(np.unique(u)) >= 3, (what, np.unique(u))
    assert ((u > 0) & (u < samples)).any(), (what, np.unique(u))
