"""Shared by tests/test_lbvh_cases_host.py and tests/test_gpu_lbvh_tree.py: seeded triangle soups at the sizes and shapes where the
GPU LBVH builder's three kernels (par_raytracer_amd/csrc/bvh_lbvh.h: k_prims, k_hierarchy, k_fit) can go wrong, and a plain numpy
statement of what the builder must return for them - every array has exactly one right answer, so the comparison is ==.

  keys       k_prims and build_lbvh_tree's scale, restated in float32 expression by expression (reference_keys)
  order      stable argsort of the keys
  tree       top-down: a range splits at the highest differing bit of key << 32 | position (reference_tree)
  boxes      float32 min / max of the corners; a node's box is the min / max over [first, last]

port_hierarchy() is a second construction of the tree, k_hierarchy lane by lane; the host test holds the two against each other
and shows that the comparison (differences) sees a broken tie-break, swapped children, a shifted range and a box one ulp short.

Every case is a soup (positions (P, 3) f32, idx u32, runs) - the mesh format of tests/query_grad_cases.py - in which triangle t
owns vertices 3 t .. 3 t + 2."""
from __future__ import annotations

import bisect
import struct

import numpy as np

import harness

QMAX = 2097151                                   # 2^21 - 1: the Morton grid per axis
TREE_ARRAYS = ("sorted_keys", "sorted_ids", "left", "right", "first", "last", "leaf_box", "node_box")


def soup(corners):
    c = np.ascontiguousarray(corners, np.float32).reshape(-1, 3)
    assert c.shape[0] % 3 == 0 and np.all(np.isfinite(c))
    return c, np.arange(c.shape[0], dtype=np.uint32), np.array([[0, c.shape[0]]], np.uint32)


def verts9(mesh):
    p, idx, _ = mesh
    return np.ascontiguousarray(p[idx.astype(np.int64)].reshape(-1, 9), np.float32)


# ---- the reference

def spread21(v):
    x = v.astype(np.uint64) & np.uint64(0x1FFFFF)
    for shift, mask in ((32, 0x1F00000000FFFF), (16, 0x1F0000FF0000FF), (8, 0x100F00F00F00F00F), (4, 0x10C30C30C30C30C3), (2, 0x1249249249249249)):
        x = (x | x << np.uint64(shift)) & np.uint64(mask)
    return x


def reference_keys(v9):
    """(keys u64 (n,), q u32 (n, 3), leaf boxes f32 (n, 6), scale f32 (3,)) in input order: the float32 arithmetic of the upload's
    scene bounds, build_lbvh_tree's scale and k_prims, one numpy operation per C operation."""
    v = np.ascontiguousarray(v9, np.float32).reshape(-1, 3, 3)
    f32 = np.float32
    scene_lo, scene_hi = v.reshape(-1, 3).min(0), v.reshape(-1, 3).max(0)
    ext = scene_hi - scene_lo
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        scale = np.where(ext > f32(0), f32(QMAX) / ext, f32(0)).astype(f32)
        lo = np.fmin(np.fmin(v[:, 0], v[:, 1]), v[:, 2])
        hi = np.fmax(np.fmax(v[:, 0], v[:, 1]), v[:, 2])
        c = (f32(0.5) * (lo + hi) - scene_lo) * scale
        assert c.dtype == np.float32
        q = np.fmin(np.fmax(c, f32(0)), f32(QMAX)).astype(np.uint32)
    keys = spread21(q[:, 0]) | spread21(q[:, 1]) << np.uint64(1) | spread21(q[:, 2]) << np.uint64(2)
    return keys, q, np.concatenate([lo, hi], 1), scale


def reference_tree(sorted_keys):
    """left, right (i32), first, last (u32) of the radix tree over (key, position), in the kernel's numbering; arrays of length
    max(n - 1, 1), all zero for n = 1.  Top-down with an explicit stack."""
    keys = [int(k) for k in sorted_keys]
    n = len(keys)
    ni = max(n - 1, 1)
    left, right = np.zeros(ni, np.int32), np.zeros(ni, np.int32)
    first, last = np.zeros(ni, np.uint32), np.zeros(ni, np.uint32)
    stack = [(0, 0, n - 1)] if n > 1 else []
    while stack:
        node, lo, hi = stack.pop()
        if keys[lo] != keys[hi]:
            b = (keys[lo] ^ keys[hi]).bit_length() - 1                  # the highest differing bit of the keys ...
            gamma = bisect.bisect_left(keys, ((keys[lo] >> b) + 1) << b, lo, hi + 1) - 1
        else:
            b = (lo ^ hi).bit_length() - 1                              # ... or, keys equal, of the positions
            gamma = ((hi >> b) << b) - 1
        assert lo <= gamma < hi
        first[node], last[node] = lo, hi
        if lo == gamma:
            left[node] = ~gamma
        else:
            left[node] = gamma
            stack.append((gamma, lo, gamma))
        if hi == gamma + 1:
            right[node] = ~(gamma + 1)
        else:
            right[node] = gamma + 1
            stack.append((gamma + 1, gamma + 1, hi))
    return left, right, first, last


def range_boxes(leaf_box, first, last):
    """min of lo / max of hi over [first[i], last[i]] for every i, straight from the leaf boxes."""
    pad = np.concatenate([leaf_box, leaf_box[-1:]], 0)
    at = np.stack([first.astype(np.int64), last.astype(np.int64) + 1], 1).reshape(-1)
    return np.concatenate([np.minimum.reduceat(pad[:, :3], at, axis=0)[::2], np.maximum.reduceat(pad[:, 3:], at, axis=0)[::2]], 1)


def reference(mesh):
    """Everything prt_debug_lbvh_tree returns for the soup, plus "q" (n, 3) in sorted order."""
    keys, q, boxes, _ = reference_keys(verts9(mesh))
    order = np.argsort(keys, kind="stable")
    sk = keys[order]
    left, right, first, last = reference_tree(sk)
    leaf_box = np.ascontiguousarray(boxes[order])
    n = len(sk)
    node_box = range_boxes(leaf_box, first, last) if n > 1 else np.zeros((1, 6), np.float32)
    return dict(sorted_keys=sk, sorted_ids=order.astype(np.uint32), left=left, right=right, first=first, last=last, leaf_box=leaf_box,
                node_box=np.ascontiguousarray(node_box, np.float32), q=q[order])


def differences(got, ref, nodes=None):
    """Names of the arrays of TREE_ARRAYS in which `got` differs from `ref` (boxes as values: -0 == +0).  For one triangle the
    per-node arrays are unspecified and left out.  nodes: compare only these rows of the per-node arrays."""
    n = len(ref["sorted_ids"])
    bad = []
    for k in TREE_ARRAYS:
        if k not in got:
            continue
        per_node = k in ("left", "right", "first", "last", "node_box")
        if per_node and n == 1:
            continue
        a, b = np.asarray(got[k]), np.asarray(ref[k])
        if per_node and nodes is not None:
            a, b = a[nodes], b[nodes]
        if a.shape != b.shape or a.dtype != b.dtype or not np.array_equal(a, b):
            bad.append(k)
    return bad


# ---- the second construction: k_hierarchy, lane by lane

def port_hierarchy(sorted_keys, lanes=None, tie_break=True):
    """What lane i of k_hierarchy writes, for every i (or the lanes named), with Python integers.  tie_break=False leaves the
    positions out of delta (equal keys share 64 bits and no more) - the edit the host test shows to be visible."""
    keys = [int(k) for k in sorted_keys]
    n = len(keys)
    ni = max(n - 1, 1)
    left, right = np.zeros(ni, np.int32), np.zeros(ni, np.int32)
    first, last = np.zeros(ni, np.uint32), np.zeros(ni, np.uint32)

    def delta(i, j):
        if j < 0 or j >= n:
            return -1
        a, b = keys[i], keys[j]
        if a != b:
            return 64 - (a ^ b).bit_length()
        return 64 + 32 - (i ^ j).bit_length() if tie_break else 64

    for i in (range(n - 1) if lanes is None else lanes):
        d = 1 if delta(i, i + 1) - delta(i, i - 1) >= 0 else -1
        dmin = delta(i, i - d)
        lmax = 2
        while delta(i, i + lmax * d) > dmin:
            lmax *= 2
        l, t = 0, lmax // 2
        while t >= 1:
            if delta(i, i + (l + t) * d) > dmin:
                l += t
            t //= 2
        j = i + l * d
        dnode = delta(i, j)
        s, t = 0, (l + 1) // 2
        while True:
            if delta(i, i + (s + t) * d) > dnode:
                s += t
            if t <= 1:                                                   # (the kernel tests t == 1: l >= 1 there, so t never is 0)
                break
            t = (t + 1) // 2
        gamma = i + s * d + (-1 if d < 0 else 0)
        lo, hi = min(i, j), max(i, j)
        left[i] = ~gamma if lo == gamma else gamma
        right[i] = ~(gamma + 1) if hi == gamma + 1 else gamma + 1
        first[i], last[i] = lo, hi
    return left, right, first, last


def parents(left, right):
    p = np.full(len(left), -1, np.int64)
    for child in (left, right):
        at = np.nonzero(child >= 0)[0]
        p[child[at]] = at
    return p


# ---- the cases

GRID = 2.0 ** -10


def _centred_shapes(rng, count, centre_units, half=2048):
    """`count` random triangles in integer units whose box centre is exactly centre_units (integers): corners uniform within
    +-half, moved so that lo + hi = 2 * centre on every axis; returns (count, 3, 3) int64."""
    v = rng.integers(-half, half + 1, (count, 3, 3))
    lo, hi = v.min(1), v.max(1)
    odd = (lo + hi) % 2 != 0
    top = v.argmax(1)                                                    # (count, 3): the corner holding hi, per axis
    for a in range(3):
        v[np.arange(count), top[:, a], a] += odd[:, a]
    lo, hi = v.min(1), v.max(1)
    assert np.all((lo + hi) % 2 == 0)
    return v - ((lo + hi) // 2)[:, None, :] + np.asarray(centre_units, np.int64)[None, None, :]


def random_soup(n, seed):
    """n small triangles of random orientation, centres uniform in a cube with about one triangle per unit volume."""
    rng = np.random.default_rng(seed)
    side = max(1.0, float(n) ** (1.0 / 3.0))
    centre = rng.uniform(0.0, side, (n, 1, 3))
    return soup(centre + rng.uniform(-0.3, 0.3, (n, 3, 3)))


def same_centre(n, seed):
    """n random shapes whose box centre is the one grid point (24, 17.5, 40.25): one key, no two triangles coplanar."""
    rng = np.random.default_rng(seed)
    units = _centred_shapes(rng, n, (24 * 1024, 17 * 1024 + 512, 40 * 1024 + 256))
    return soup(units * GRID)


RUN_LENGTHS = (1, 2, 63, 64, 65, 300, 129)
RUN_CENTRES = ((4, 4, 4), (60, 36, 32), (8, 9, 10), (24, 12, 26), (16, 28, 12), (27, 20, 21), (12, 16, 27.5))


def runs_case(seed=31):
    """Seven box centres, RUN_LENGTHS triangles on each, in shuffled input order.  The first two centres are the scene's own corners:
    a box centre can only lie there if the triangle has no extent, so those three triangles are points - they quantise to 0 and
    to 2097151 on every axis; the other five runs are random shapes built as same_centre's, strictly inside.  Returns the soup and
    the run (0..6) of every triangle."""
    rng = np.random.default_rng(seed)
    parts, run = [], []
    for k, (count, c) in enumerate(zip(RUN_LENGTHS, RUN_CENTRES)):
        cu = [int(round(x * 1024)) for x in c]
        units = np.tile(np.asarray(cu, np.int64), (count, 3, 1)) if k < 2 else _centred_shapes(rng, count, cu)
        parts.append(units)
        run += [k] * count
    order = rng.permutation(len(run))
    return soup(np.concatenate(parts, 0)[order] * GRID), np.asarray(run)[order]


ONE = (0.5, 0.25, -1.0, 1.5, 0.25, -1.0, 0.5, 1.0, -2.0)           # tests/bvh_check_harness.cpp's triangle


def identical(count=37):
    return soup(np.tile(np.asarray(ONE, np.float32), count))


def flat(axes, n=300, seed=41):
    """n triangles in a scene of extent exactly 0 on `axes` of its axes: 1 - non-overlapping triangles in the plane z = 0.75, one
    per cell of a jittered grid, facing +z; 2 - collinear corners along x; 3 - n points at one place."""
    rng = np.random.default_rng(seed + axes)
    if axes == 1:
        side = int(np.ceil(np.sqrt(n)))
        cell = np.arange(n)
        centre = np.stack([cell % side + 0.5, cell // side + 0.5], 1) + rng.uniform(-0.1, 0.1, (n, 2))
        angle = rng.uniform(0, 2 * np.pi, n)[:, None] + np.array([0.0, 2.1, 4.2])[None, :]
        radius = rng.uniform(0.15, 0.3, (n, 3))
        xy = centre[:, None, :] + np.stack([radius * np.cos(angle), radius * np.sin(angle)], 2)
        c = np.concatenate([xy, np.full((n, 3, 1), 0.75)], 2)
    elif axes == 2:
        c = np.concatenate([rng.uniform(0.0, 50.0, (n, 3, 1)), np.full((n, 3, 1), -1.5), np.full((n, 3, 1), 0.375)], 2)
    else:
        c = np.tile(np.array([1.25, -2.5, 3.0]), (n, 3, 1))
    return soup(c)


TINY = 2.0 ** -110                               # 2097151 / TINY is above FLT_MAX: the scale of an axis of this extent is inf


def tiny_extent(n=300, seed=47):
    """flat(1)'s triangles with every corner's z drawn from 0, TINY / 2 and TINY - normal floats, and the scale of z is inf.
    (centre - lo) * inf is inf, clamped to 2097151, and NaN = 0 * inf where all three corners have z = 0, which fmaxf(NaN, 0)
    turns into 0: the one case here in which the upper end of k_prims' clamp decides a key."""
    rng = np.random.default_rng(seed)
    c = flat(1, n, seed)[0].reshape(n, 3, 3).astype(np.float64)
    c[:, :, 2] = rng.integers(0, 3, (n, 3)) * (TINY / 2)
    c[: n // 10, :, 2] = 0.0
    return soup(c)


FAR, STEP = 2.0 ** 20, 2.0 ** -3                 # float32's spacing at 2^20 is 2^-3


def far_and_thin(n=1024, seed=51):
    """A soup at offset 2^20 on every axis whose z extent is 2^-3, one float32 step: every corner has z = 2^20 or 2^20 + 2^-3.  One
    triangle per cell (4 x 4, 32 steps a side) of a square grid, corners on the float grid inside the cell, counter-clockwise seen
    from +z.  A triangle with corners in both planes has its centre between two floats: 0.5f * (lo + hi) rounds it into the lower
    plane, so three z centres become two keys' worth."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(n)))
    cell = np.arange(n)
    angle = rng.uniform(0, 2 * np.pi, n)[:, None] + np.array([0.0, 2.1, 4.2])[None, :]
    radius = rng.uniform(6.0, 11.0, (n, 3))
    xy = np.rint(16.0 + np.stack([radius * np.cos(angle), radius * np.sin(angle)], 2)).astype(np.int64)       # steps, 5 .. 27
    xy += 32 * np.stack([cell % side, cell // side], 1)[:, None, :]
    z = rng.integers(0, 2, (n, 3, 1))
    c = FAR + STEP * np.concatenate([xy, z], 2).astype(np.float64)
    return soup(c)


COUNTS = (1, 2, 3, 4, 5, 255, 256, 257, 258, 513)
LARGE_N = 2 ** 17 + 1

_CASES = {}


def case_names():
    return (["counts_%d" % n for n in COUNTS] + ["same_centre_1000", "same_centre_1024", "runs", "identical", "flat_1", "flat_2", "flat_3",
                                                  "tiny_extent", "far_and_thin", "large"])


def case(name):
    """The soup of a case, built once."""
    if name not in _CASES:
        if name.startswith("counts_"):
            n = int(name.split("_")[1])
            m = random_soup(n, 100 + n)
        elif name.startswith("same_centre_"):
            m = same_centre(int(name.split("_")[2]), 21)
        elif name == "runs":
            m = runs_case()[0]
        elif name == "identical":
            m = identical()
        elif name.startswith("flat_"):
            m = flat(int(name.split("_")[1]))
        elif name == "tiny_extent":
            m = tiny_extent()
        elif name == "far_and_thin":
            m = far_and_thin()
        elif name == "large":
            m = random_soup(LARGE_N, 7)
        else:
            raise KeyError(name)
        _CASES[name] = m
    return _CASES[name]


_REFS = {}


def case_reference(name):
    """reference(case(name)), computed once and handed out read-only."""
    if name not in _REFS:
        r = reference(case(name))
        for v in r.values():
            v.setflags(write=False)
        _REFS[name] = r
    return _REFS[name]


# distinct keys of the cases that are about them (the host test asserts the figures); every other case has one key per triangle
DISTINCT_KEYS = {"same_centre_1000": 1, "same_centre_1024": 1, "runs": 7, "identical": 1, "flat_3": 1, "far_and_thin": 1024}
QUERY_CASES = ("counts_5", "counts_257", "counts_513", "same_centre_1000", "same_centre_1024", "runs", "flat_1", "far_and_thin", "large")


def query_targets(name):
    """Triangles a ray can be aimed at: all of them, but not the point triangles of `runs`."""
    if name == "runs":
        return np.nonzero(runs_case()[1] >= 2)[0]
    return np.arange(case(name)[1].size // 3)


def queries(name, n_rays=4096, n_points=2048, seed=61):
    """(origins, directions, points): recipe rays of tests/query_grad_cases.py aimed at random triangles, and points one tenth
    of sqrt(area) off random places of the surface, on either side."""
    import query_grad_cases as Q
    mesh = case(name)
    p, idx, _ = mesh
    rng = np.random.default_rng(seed)
    targets = query_targets(name)
    o, d, _, _ = Q.recipe_rays(mesh, n_rays, seed + 1, triangles=targets[rng.integers(0, len(targets), n_rays)])
    tri = targets[rng.integers(0, len(targets), n_points)]
    a, b, c = (p[idx[3 * tri + k]].astype(np.float64) for k in range(3))
    w = rng.uniform(0.05, 1.0, (n_points, 3))
    w /= w.sum(1, keepdims=True)
    cr = np.cross(b - a, c - a)
    area2 = np.linalg.norm(cr, axis=1, keepdims=True)
    pts = w[:, :1] * a + w[:, 1:2] * b + w[:, 2:] * c + cr / area2 * 0.1 * np.sqrt(area2) * rng.choice([-1.0, 1.0], (n_points, 1))
    return o, d, np.ascontiguousarray(pts, np.float32)


# ---- the host back end on the reference's trees (tests/lbvh_backend_harness.cpp)

BACKENDS = (("plain", 1, -1), ("cluster4", 0, 4), ("cluster64", 0, -1), ("cluster1048576", 0, 1 << 20))       # name, LBVH_PLAIN, LBVH_CLUSTER


def build_backend_harness(directory, sanitize=True):
    return harness.build("lbvh_backend_harness.cpp", directory, "lbvh_backend" + ("_san" if sanitize else ""), sanitize=sanitize,
                         sources=("bvh_build.cpp", "bvh_check.cpp"))


def write_trees(path, names):
    """The cases' triangles and reference trees in the harness's input format (little endian): u32 case count, then per case
    u32 name length, the name, u32 n and the arrays verts (9 n f32), left, right (ni i32), first, last (ni u32), node_box (6 ni f32),
    leaf_box (6 n f32), sorted_ids (n u32), ni = max(n - 1, 1)."""
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(names)))
        for name in names:
            r, v = case_reference(name), verts9(case(name))
            f.write(struct.pack("<I", len(name)) + name.encode() + struct.pack("<I", v.shape[0]))
            harness.put(f, (v, np.float32), (r["left"], np.int32), (r["right"], np.int32), (r["first"], np.uint32), (r["last"], np.uint32),
                        (r["node_box"], np.float32), (r["leaf_box"], np.float32), (r["sorted_ids"], np.uint32))
