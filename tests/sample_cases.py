"""Shared by tests/test_sample_host.py and tests/test_gpu_sample.py: the runner of tests/sample_host_harness.cpp (a brute force of the
definition of prt_sample_surface and prt_sample_surface_backward in input order, with the PRT_HD functions of csrc/dev_sample.h
and csrc/dev_sample_grad.h), the meshes of tests/signed_cases.py and tests/closest_cases.py cut to the triangle counts the scan
kernels care about, and float64 numpy yardsticks: the area, the gradient, the statistic's gate."""
from __future__ import annotations

import struct

import numpy as np

import closest_cases as K
import harness
import signed_cases as S

FIELDS = ("point", "bw", "normal", "vertex0", "group")
INFO = ("area", "total_weight", "unit_exponent", "live_triangles")
SENTINEL = np.float32(7.5)
# the values of `first` at which the key's packing (pixel = j >> 16, sample = j & 0xFFFF, 32 + 16 bits) crosses its fields
FIRSTS = (0, 1, 65535, 65536, 2 ** 32 - 1, 2 ** 32, 2 ** 48 - 64)
# csrc/kernels_sample.h: a scan tile is SAMPLE_TILE triangles, and one pass of k_sample_totals' loop covers SAMPLE_TILE tiles
SAMPLE_TILE = 256
TOTALS_PASS = SAMPLE_TILE * SAMPLE_TILE


def build_harness(directory, sanitize=False):
    return harness.build("sample_host_harness.cpp", directory, "sample_host" + ("_san" if sanitize else ""), sanitize=sanitize)


def request(seed, first, count):
    return (int(seed), int(first), int(count))


def grad_call(group, vertex0, bw, grad_point=None, grad_normal=None, merge=False):
    f32 = lambda x: None if x is None else np.ascontiguousarray(x, np.float32)       # noqa: E731
    return dict(group=np.ascontiguousarray(group, np.int32), vertex0=np.ascontiguousarray(vertex0).view(np.uint32),
                bw=f32(bw), grad_point=f32(grad_point), grad_normal=f32(grad_normal), merge=bool(merge))


def case(mesh, requests=(), grads=()):
    return dict(mesh=mesh, requests=list(requests), grads=list(grads))


def run_harness(exe, cases, directory, tag="sample"):
    """Every case through the harness in one run.  Per case a dict: the four INFO entries, "W" (uint64 per input triangle),
    "samples" (per request {field: array}) and "grads" (per gradient call rc, hit, skipped, invalid, unit_exponent,
    max_contribution, positions)."""
    fin, fout = harness.case_files(directory, tag + "_cases.bin", tag + "_results.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for c in cases:
            p, idx, runs = c["mesh"]
            f.write(struct.pack("<6I", p.shape[0], idx.size, runs.shape[0], len(c["requests"]), len(c["grads"]), 0))
            harness.put(f, (p, np.float32), (idx, np.uint32), (runs, np.uint32))
            for seed, first, count in c["requests"]:
                f.write(struct.pack("<3Q", seed, first, count))
            for g in c["grads"]:
                flags = (1 if g["grad_point"] is not None else 0) | (2 if g["grad_normal"] is not None else 0) | (16 if g["merge"] else 0)
                f.write(struct.pack("<2I", len(g["group"]), flags))
                f.write(g["group"].tobytes() + g["vertex0"].tobytes() + g["bw"].tobytes())
                for key in ("grad_point", "grad_normal"):
                    if g[key] is not None:
                        f.write(g[key].tobytes())
    harness.run(exe, fin, fout)
    r, out = harness.Reader.of_file(fout), []
    for c in cases:
        n_pos, n_tris = c["mesh"][0].shape[0], c["mesh"][1].size // 3
        area, total, unit, live = r.unpack("<dQiI")
        res = dict(area=area, total_weight=total, unit_exponent=unit, live_triangles=live, W=r.take(n_tris, np.uint64), samples=[], grads=[])
        for _seed, _first, n in c["requests"]:
            res["samples"].append(dict(point=r.take(3 * n, np.float32, (n, 3)), bw=r.take(3 * n, np.float32, (n, 3)),
                                       normal=r.take(3 * n, np.float32, (n, 3)), vertex0=r.take(n, np.uint32), group=r.take(n, np.int32)))
        for _g in c["grads"]:
            rc, hit, skipped, invalid, unit, m = r.unpack("<5if")
            res["grads"].append(dict(rc=rc, hit=hit, skipped=skipped, invalid=invalid, unit_exponent=unit, max_contribution=m,
                                     positions=r.take(3 * n_pos, np.float32, (n_pos, 3))))
        out.append(res)
    r.done()
    return out


def run_pick(exe, lists, directory):
    """lists: [(weights, r0 values)] of Python integers -> per list the int64 array of the triangles picked (-1: a miss)."""
    fin, fout = harness.case_files(directory, "pick_lists.bin", "pick_out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<I", len(lists)))
        for w, r in lists:
            f.write(struct.pack("<2I", len(w), len(r)))
            f.write(np.array(w, np.uint64).tobytes() + np.array(r, np.uint64).tobytes())
    harness.run(exe, "--pick", fin, fout)
    blob = harness.Reader.of_file(fout)
    out = [blob.take(len(r), np.int64) for _, r in lists]
    blob.done()
    return out


def pick_by_integers(weights, r0):
    """The definition in Python integers: x = floor(r0 * T / 2^64), the smallest t with C_t > x; -1 when T == 0."""
    total = sum(weights)
    if total == 0:
        return -1
    x, c = (r0 * total) >> 64, 0
    for t, w in enumerate(weights):
        c += w
        if c > x:
            return t
    raise AssertionError("x < T must hold")


def boundary_draws(weights):
    """r0 = 0, 2^64 - 1 and, for every boundary value b of x (a prefix sum 0 < b < T), the largest r0 with x = b - 1 and the
    smallest with x = b."""
    total = sum(weights)
    out, c = [0, 2 ** 64 - 1], 0
    for w in weights[:-1]:
        c += w
        if 0 < c < total:
            r = -((-c << 64) // total)                              # the smallest r0 with r0 * T >= c * 2^64
            assert (r * total) >> 64 == c and ((r - 1) * total) >> 64 == c - 1
            out += [r - 1, r]
    return sorted(set(out))


def assert_same_bits(got, expect, what, fields=FIELDS):
    """Every field of `got` ({field: numpy array}) equals `expect` bit for bit."""
    harness.assert_same_bits(got, expect, what, fields)


def to_numpy(res):
    """A sample_surface result with torch tensors -> numpy arrays (vertex0 back to uint32)."""
    return harness.to_numpy(res, ("vertex0",))


def assert_all_miss(res, what, fields=FIELDS):
    """Every sample is a miss: +0 in point, bw and normal, group -1, vertex0 0xFFFFFFFF."""
    miss = dict(point=0, bw=0, normal=0, vertex0=0xFFFFFFFF, group=0xFFFFFFFF)
    for f in fields:
        a = np.ascontiguousarray(res[f])
        assert np.all(a.view(np.uint32) == miss[f]), (what, f)


# ---- meshes

def truncated(mesh, n_tris):
    """The first n_tris triangles of a one-group mesh (positions that no triangle uses any more stay)."""
    p, idx, runs = mesh
    assert runs.shape[0] == 1 and idx.size >= 3 * n_tris
    return p, np.ascontiguousarray(idx[:3 * n_tris]), np.array([[0, 3 * n_tris]], np.uint32)


def height_field_of(n_tris, seed=2):
    """height_field(n, seed) with the smallest n that has n_tris triangles, cut to n_tris."""
    n = 1
    while 2 * n * n < n_tris:
        n += 1
    return truncated(K.height_field(n, seed), n_tris)


def size_ratio_mesh():
    """Two right triangles in the plane z = 0 whose areas differ by 2^30: legs 2^15 and legs 1, apart from each other."""
    big = 2.0 ** 15
    p = np.array([[0, 0, 0], [big, 0, 0], [0, big, 0], [-4, -4, 0], [-3, -4, 0], [-4, -3, 0]], np.float32)
    return p, np.arange(6, dtype=np.uint32), np.array([[0, 6]], np.uint32)


def all_degenerate():
    """Four zero-area triangles: (a, a, a), (a, a, b), collinear corners, and a repeated index."""
    p = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [0.5, 0, 0]], np.float32)
    tri = np.array([[0, 0, 0], [0, 0, 1], [0, 1, 2], [1, 3, 1]], np.uint32)
    return p, np.ascontiguousarray(tri.reshape(-1)), np.array([[0, tri.size]], np.uint32)


# ---- float64 yardsticks

def triangle_corners64(mesh):
    p, idx, runs = mesh
    tri = idx.reshape(-1, 3).astype(np.int64)
    P = p.astype(np.float64)
    return P[tri[:, 0]], P[tri[:, 1]], P[tri[:, 2]]


def area64(mesh):
    a, b, c = triangle_corners64(mesh)
    return float(0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1).sum())


def wilson_hilferty(k, z=3.0902):
    """The 99.9 % quantile of chi-square with k degrees of freedom by Wilson and Hilferty."""
    return k * (1.0 - 2.0 / (9.0 * k) + z * np.sqrt(2.0 / (9.0 * k))) ** 3


def pearson(mesh, samples, W):
    """Pearson's statistic of the samples' triangle counts against N W_t / T over the triangles with W_t > 0, and the degrees of freedom."""
    t = K.input_triangle(mesh, samples["group"], samples["vertex0"])
    n = len(t)
    counts = np.bincount(t, minlength=len(W)).astype(np.float64)
    w = W.astype(np.float64)
    live = w > 0
    assert counts[~live].sum() == 0, "a zero-weight triangle was drawn"
    expect = n * w[live] / w.sum()
    return float(((counts[live] - expect) ** 2 / expect).sum()), int(live.sum()) - 1


def grad_yardstick(mesh, group, vertex0, bw, grad_point, grad_normal, dtype=np.float64):
    """dL/dpositions of the table of csrc/dev_sample_grad.h in `dtype` (numpy, np.add.at), on the float32 inputs widened exactly:
    the point term g bw_k per corner, and the normal term through n = N / |N|.  Samples with group < 0 are left out."""
    p, idx, runs = mesh
    live = np.nonzero(group >= 0)[0]
    corner = runs[group[live], 0].astype(np.int64) + vertex0[live].astype(np.int64)
    vi = [idx[corner + k].astype(np.int64) for k in range(3)]
    P = p.astype(dtype)
    a, b, c = (P[v] for v in vi)
    g = [np.zeros((len(live), 3), dtype) for _ in range(3)]
    if grad_point is not None:
        gp = grad_point[live].astype(dtype)
        for k in range(3):
            g[k] = g[k] + gp * bw[live, k:k + 1].astype(dtype)
    if grad_normal is not None:
        ab, ac = b - a, c - a
        N = np.cross(ab, ac)
        ln = np.sqrt((N * N).sum(1, keepdims=True))
        n = N / ln
        gn = grad_normal[live].astype(dtype)
        gN = (gn - n * (n * gn).sum(1, keepdims=True)) / ln
        g_ab, g_ac = np.cross(ac, gN), np.cross(gN, ab)
        g[0] = g[0] - (g_ab + g_ac)
        g[1] = g[1] + g_ab
        g[2] = g[2] + g_ac
    out = np.zeros(P.shape, dtype)
    for k in range(3):
        np.add.at(out, vi[k], g[k])
    return out.astype(np.float64)


FLOOR = 2.0 ** -22           # closest_grad_cases.FLOOR: four float32 ulps of an array's largest entry


def check_grad_against_yardstick(mesh, call, ours, what=""):
    """The rule of closest_grad_cases.check_against_yardstick: err(X) = max |X - X64| / max |X64|; the gate is
    err(ours) <= 4 * max(err(X32), 2^-22).  Returns (err ours, err float32)."""
    args = (mesh, call["group"], call["vertex0"], call["bw"], call["grad_point"], call["grad_normal"])
    x64, x32 = grad_yardstick(*args, dtype=np.float64), grad_yardstick(*args, dtype=np.float32)
    scale = np.abs(x64).max()
    assert scale > 0
    e_ours, e_32 = np.abs(np.asarray(ours, np.float64) - x64).max() / scale, np.abs(x32 - x64).max() / scale
    print("%s positions: err ours %.3g, err numpy float32 %.3g, gate %.3g" % (what, e_ours, e_32, 4 * max(e_32, FLOOR)))
    assert e_ours <= 4 * max(e_32, FLOOR), "%s: err %.3g above 4 * max(%.3g, 2^-22)" % (what, e_ours, e_32)
    return float(e_ours), float(e_32)


def random_grads(n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, 3)).astype(np.float32), rng.standard_normal((n, 3)).astype(np.float32)


def upload_mesh(api, mesh, device=0, lbvh=False):
    """A Renderer with the mesh uploaded the way tests/test_gpu_signed.py uploads its meshes."""
    r = api.Renderer(device)
    if lbvh:
        r.set_option("BVH_BUILDER", "lbvh")
    flat = S.flat_desc(mesh)
    r.upload(flat)
    return r, flat
