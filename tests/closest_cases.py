"""Shared by tests/test_closest_host.py, tests/test_closest_cases_host.py, tests/test_gpu_closest.py and
tests/test_gpu_closest_schedules.py: meshes, the point recipe, the float64 yardstick of closest_on_triangle, the runner of
tests/closest_host_harness.cpp (the walk of csrc/dev_closest.h and a brute force of the same function over every triangle, one lane
at a time on the host) and the case builders of the schedule tests (pure numpy, seeded)."""
from __future__ import annotations

import struct

import numpy as np

import harness
from query_grad_cases import bits, flat_desc, one_triangle, scene_mesh       # noqa: F401  (re-exported)

FIXTURES = ("cornell_box", "icosphere_l3", "coincident", "terrain_64")
RECIPE_POINTS = 2048
FIELDS = ("dist2", "point", "bw", "vertex0", "group")
FLT_MAX = np.float32(3.4028234663852886e38)
KIND_NEAR, KIND_BOX, KIND_FAR, KIND_ON = 0, 1, 2, 3


# ---- the point recipe

def mesh_extent(mesh):
    """(lo, hi, largest side) of the referenced positions' bounding box, float64."""
    p, idx, runs = mesh
    used = p[idx].astype(np.float64)
    lo, hi = used.min(0), used.max(0)
    return lo, hi, float((hi - lo).max())


def recipe_points(mesh, n, seed):
    """n float32 points, seeded.  n/2: random barycentric points on random triangles, displaced along +- the normal by up to 5 %
    of the extent (the box's largest side); n/4: uniform in twice the bounding box (same centre); n/8: at 1 to 1e4 x the extent
    from the box's centre, log-uniform, in random directions; n/8: exactly on vertices (the first half) and on edge midpoints
    ((a + b) * 0.5 in float32).  Returns (points (n, 3), kind (n,) of KIND_*), shuffled together."""
    p, idx, runs = mesh
    rng = np.random.default_rng(seed)
    n_tris = idx.size // 3
    lo, hi, extent = mesh_extent(mesh)
    centre = 0.5 * (lo + hi)
    P = p.astype(np.float64)
    n_near, n_box, n_far = n // 2, n // 4, n // 8
    n_on = n - n_near - n_box - n_far
    out, kind = [], []
    # near the surface
    tri = rng.integers(0, n_tris, n_near)
    a, b, c = (P[idx[3 * tri + k]] for k in range(3))
    bw = rng.uniform(0.0, 1.0, (n_near, 3))
    bw /= bw.sum(1, keepdims=True)
    on = bw[:, :1] * a + bw[:, 1:2] * b + bw[:, 2:] * c
    cr = np.cross(b - a, c - a)
    ln = np.linalg.norm(cr, axis=1, keepdims=True)
    nrm = np.where(ln > 0, cr / np.where(ln > 0, ln, 1.0), 0.0)
    out.append(on + nrm * rng.uniform(-0.05, 0.05, (n_near, 1)) * extent)
    kind.append(np.full(n_near, KIND_NEAR))
    # in twice the box
    half = (hi - lo)
    out.append(centre + rng.uniform(-1.0, 1.0, (n_box, 3)) * half)
    kind.append(np.full(n_box, KIND_BOX))
    # far away
    d = rng.standard_normal((n_far, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    out.append(centre + d * extent * 10.0 ** rng.uniform(0.0, 4.0, (n_far, 1)))
    kind.append(np.full(n_far, KIND_FAR))
    pts = np.concatenate(out).astype(np.float32)
    # on vertices and edge midpoints, in float32
    tri = rng.integers(0, n_tris, n_on)
    corner = rng.integers(0, 3, n_on)
    va = p[idx[3 * tri + corner]]
    vb = p[idx[3 * tri + (corner + 1) % 3]]
    on_pts = va.copy()
    mid = np.arange(n_on) >= n_on // 2
    on_pts[mid] = ((va[mid] + vb[mid]) * np.float32(0.5)).astype(np.float32)
    pts = np.concatenate([pts, on_pts]).astype(np.float32)
    kind = np.concatenate(kind + [np.full(n_on, KIND_ON)])
    order = rng.permutation(n)
    return np.ascontiguousarray(pts[order]), kind[order]


# ---- the yardstick: Ericson 5.1.5 in float64 on the float32 corners

def yardstick(p, a, b, c):
    """Region walk in float64, vectorised: returns (dist, v, w, region) with region 0..6 = vertex a, b, edge ab, vertex c, edge ac,
    edge bc, interior (the order of the tests in closest_on_triangle)."""
    p, a, b, c = (np.asarray(x, np.float64) for x in (p, a, b, c))
    dot = lambda x, y: (x * y).sum(-1)            # noqa: E731
    ab, ac, ap = b - a, c - a, p - a
    d1, d2 = dot(ab, ap), dot(ac, ap)
    bp = p - b
    d3, d4 = dot(ab, bp), dot(ac, bp)
    cp = p - c
    d5, d6 = dot(ab, cp), dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    with np.errstate(divide="ignore", invalid="ignore"):
        conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0)]
        wbc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        den = 1.0 / (va + vb + vc)
        vs = [np.zeros_like(d1), np.ones_like(d1), d1 / (d1 - d3), np.zeros_like(d1), np.zeros_like(d1), 1.0 - wbc, vb * den]
        ws = [np.zeros_like(d1), np.zeros_like(d1), np.zeros_like(d1), np.ones_like(d1), d2 / (d2 - d6), wbc, vc * den]
    region = np.full(d1.shape, 6)
    for k in range(5, -1, -1):
        region = np.where(conds[k], k, region)
    v = np.choose(region, vs)
    w = np.choose(region, ws)
    q = a + ab * v[..., None] + ac * w[..., None]
    return np.sqrt(dot(p - q, p - q)), v, w, region


def corners(mesh, tri):
    p, idx, runs = mesh
    return tuple(p[idx[3 * np.asarray(tri) + k]] for k in range(3))


def input_triangle(mesh, group, vertex0):
    """Input triangle index of the hit reference (group, vertex0)."""
    p, idx, runs = mesh
    return (runs[group, 0].astype(np.int64) + vertex0.astype(np.int64)) // 3


# ---- the host harness

def build_harness(directory, sanitize=False, bvh8=False):
    return harness.build("closest_host_harness.cpp", directory, "closest_host" + ("8" if bvh8 else "") + ("_san" if sanitize else ""),
                         sanitize=sanitize, bvh8=bvh8, sources=("bvh_build.cpp",))


def case(mesh, points, max_dist2=None, pair_tri=None, stack_cap=None):
    """stack_cap: also walk every valid point as one lane of k_closest does, on an LDS stack of that many entries ("listed")."""
    return dict(mesh=mesh, points=np.ascontiguousarray(points, np.float32), max_dist2=max_dist2, pair_tri=pair_tri, stack_cap=stack_cap)


def run_harness(exe, cases, directory):
    """Every case through the harness in one run.  Per case a dict: walked cases - mismatches, tie_points, node_visits, tri_tests,
    "brute" and "walk" ({field: array}), with a stack cap also stack_cap (the cap in effect: clamped to 2..40 and to the tree's
    stack_bound) and listed (u32 per point: the capped walk dropped a push); pair cases - d2, v, w, ok."""
    fin, fout = harness.case_files(directory, "closest_cases.bin", "closest_results.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for c in cases:
            p, idx, runs = c["mesh"]
            n = c["points"].shape[0]
            cap = c.get("stack_cap")
            flags = (1 if c["max_dist2"] is not None else 0) | (2 if c["pair_tri"] is not None else 0) | (4 if cap is not None else 0)
            f.write(struct.pack("<6I", n, p.shape[0], idx.size, runs.shape[0], flags, cap or 0))
            f.write(c["points"].tobytes())
            if c["max_dist2"] is not None:
                harness.put(f, (c["max_dist2"], np.float32))
            if c["pair_tri"] is not None:
                harness.put(f, (c["pair_tri"], np.uint32))
            harness.put(f, (p, np.float32), (idx, np.uint32), (runs, np.uint32))
    harness.run(exe, fin, fout)
    r, out = harness.Reader.of_file(fout), []
    for c in cases:
        n = c["points"].shape[0]
        mism, ties, nodes, tris = r.unpack("<iIQQ")
        if c["pair_tri"] is not None:
            out.append(dict(d2=r.take(n, np.float32), v=r.take(n, np.float32), w=r.take(n, np.float32), ok=r.take(n, np.uint32)))
            continue
        res = dict(mismatches=mism, tie_points=ties, node_visits=nodes, tri_tests=tris)
        for which in ("brute", "walk"):
            res[which] = dict(dist2=r.take(n, np.float32), point=r.take(3 * n, np.float32, (n, 3)), bw=r.take(3 * n, np.float32, (n, 3)),
                              vertex0=r.take(n, np.uint32), group=r.take(n, np.int32))
        if c.get("stack_cap") is not None:
            res["stack_cap"] = int(r.take(1, np.uint32)[0])
            res["listed"] = r.take(n, np.uint32)
        out.append(res)
    r.done()
    return out


def assert_same_bits(got, expect, what, fields=FIELDS):
    """Every field of `got` ({field: numpy array}) equals `expect` bit for bit."""
    harness.assert_same_bits(got, expect, what, fields)


def to_numpy(res):
    """A closest_points result with torch tensors -> numpy arrays (vertex0 back to uint32)."""
    return harness.to_numpy(res, ("vertex0",))


# ---- case builders of the schedule tests (tests/test_closest_cases_host.py proves them, tests/test_gpu_closest_schedules.py runs them)

MISS = dict(dist2=FLT_MAX, point=np.zeros(3, np.float32), bw=np.zeros(3, np.float32), vertex0=np.uint32(0xFFFFFFFF), group=np.int32(-1))
DEGENERATE_PER_FORM = 64
PER = 192                                # three waves; one and a half default chunks


def height_field(n, seed):
    """(n + 1)^2 vertices on a regular grid over [-1, 1]^2 with z = 0.2 x a standard normal, two triangles per cell, one group."""
    rng = np.random.default_rng(seed)
    g = np.linspace(-1.0, 1.0, n + 1)
    x, y = np.meshgrid(g, g, indexing="xy")
    p = np.stack([x, y, 0.2 * rng.standard_normal((n + 1, n + 1))], axis=-1).reshape(-1, 3).astype(np.float32)
    i, j = (a.reshape(-1) for a in np.meshgrid(np.arange(n), np.arange(n), indexing="ij"))
    v00 = i * (n + 1) + j
    v01, v10, v11 = v00 + 1, v00 + n + 1, v00 + n + 2
    idx = np.stack([v00, v01, v11, v00, v11, v10], axis=1).reshape(-1).astype(np.uint32)
    return np.ascontiguousarray(p), idx, np.array([[0, idx.size]], np.uint32)


def with_degenerates(mesh, seed):
    """Three groups: 0 - 4 x 64 zero-area triangles on random vertices a != b of the mesh: (a, b, midpoint of ab), (a, a, b),
    (a, a, a) and a collinear sliver (a, a + 0.5 z, a + 1.0 z) standing out of the surface; 1 - the mesh; 2 - the mesh's triangles
    in reversed order."""
    p, idx, runs = mesh
    rng = np.random.default_rng(seed)
    m = DEGENERATE_PER_FORM
    tri = idx.reshape(-1, 3)
    ia = rng.integers(0, p.shape[0], 4 * m)
    ib = (ia + 1 + rng.integers(0, p.shape[0] - 1, 4 * m)) % p.shape[0]
    a, b = p[ia], p[ib]
    z = np.array([0.0, 0.0, 1.0], np.float32)
    new = np.concatenate([((a[:m] + b[:m]) * np.float32(0.5)).astype(np.float32), a[3 * m:] + np.float32(0.5) * z, a[3 * m:] + z]).astype(np.float32)
    at = p.shape[0] + np.arange(3 * m).reshape(3, m)
    deg = np.concatenate([np.stack([ia[:m], ib[:m], at[0]], 1), np.stack([ia[m:2 * m], ia[m:2 * m], ib[m:2 * m]], 1),
                          np.stack([ia[2 * m:3 * m]] * 3, 1), np.stack([ia[3 * m:], at[1], at[2]], 1)])
    all_idx = np.concatenate([deg, tri, tri[::-1]]).reshape(-1).astype(np.uint32)
    firsts = np.cumsum([0, deg.size, tri.size])
    return (np.ascontiguousarray(np.concatenate([p, new]), np.float32), all_idx,
            np.array([[firsts[0], deg.size], [firsts[1], tri.size], [firsts[2], tri.size]], np.uint32))


def stacked_copies(mesh, seed):
    """Three groups of the same triangles with the same corner order - the 48-byte records are identical, every candidate ties
    with its two copies: group 0 in reversed order, group 1 forward, group 2 permuted.  Returns (mesh, perm): triangle k of group 2
    is triangle perm[k] of the input."""
    p, idx, runs = mesh
    tri = idx.reshape(-1, 3)
    perm = np.random.default_rng(seed).permutation(len(tri))
    all_idx = np.concatenate([tri[::-1], tri, tri[perm]]).reshape(-1).astype(np.uint32)
    return (p, all_idx, np.array([[k * tri.size, tri.size] for k in range(3)], np.uint32)), perm


def source_triangle(perm, group, vertex0):
    """The input triangle behind the copy (group, vertex0) of stacked_copies, from index arithmetic alone."""
    k = np.asarray(vertex0).astype(np.int64) // 3
    return np.select([np.asarray(group) == 0, np.asarray(group) == 1], [len(perm) - 1 - k, k], perm[k])


def expected_copy(perm, group, vertex0):
    """The smallest (group, vertex0) among the three copies of the triangle that (group, vertex0) names: group 0 holds every
    triangle, in reversed order."""
    t = source_triangle(perm, group, vertex0)
    return np.zeros(len(t), np.int32), (3 * (len(perm) - 1 - t)).astype(np.uint32)


def scaled(mesh, e):
    """The mesh times 2^e, exact in float32 (asserted: no position leaves the normal range)."""
    p, idx, runs = mesh
    q = np.ldexp(p, e).astype(np.float32)
    assert np.array_equal(np.ldexp(q.astype(np.float64), -e), p.astype(np.float64))
    return np.ascontiguousarray(q), idx, runs


def shifted(mesh, off):
    """The mesh plus a float32 offset (a scalar, or one per axis), rounded to float32."""
    p, idx, runs = mesh
    return np.ascontiguousarray((p + np.asarray(off, np.float32)).astype(np.float32)), idx, runs


def tiled(points, n):
    """The unique points repeated to length n: (points, index into the unique ones)."""
    index = np.arange(n) % len(points)
    return np.ascontiguousarray(points[index]), index


def invalid_points(n, radii=True):
    """n invalid queries, cycling through a NaN component, +inf, -inf and - with radii - a negative and a NaN squared radius:
    (points, max_dist2 or None)."""
    way = np.arange(n) % (5 if radii else 3)
    pts = np.full((n, 3), 0.25, np.float32)
    pts[way == 0, 1] = np.nan
    pts[way == 1, 0] = np.inf
    pts[way == 2, 2] = -np.inf
    if not radii:
        return pts, None
    return pts, np.select([way == 3, way == 4], [np.float32(-1.0), np.float32(np.nan)], FLT_MAX).astype(np.float32)


def sorted_by_kind(points, kind, per=PER, seed=17):
    """Runs of `per` points of one kind each - NEAR, BOX, FAR, ON, then invalid_points - as dict(points, max_dist2, index), index
    into `points` or -1 for an invalid query; and the same batch shuffled.  The valid queries carry FLT_MAX: no radius."""
    runs = [np.nonzero(kind == k)[0][:per] for k in (KIND_NEAR, KIND_BOX, KIND_FAR, KIND_ON)]
    assert all(len(r) == per for r in runs)
    bad_pts, bad_r2 = invalid_points(per)
    index = np.concatenate(runs + [np.full(per, -1)])
    batch = dict(points=np.ascontiguousarray(np.concatenate([points[np.concatenate(runs)], bad_pts]), np.float32),
                 max_dist2=np.concatenate([np.full(4 * per, FLT_MAX, np.float32), bad_r2]), index=index)
    perm = np.random.default_rng(seed).permutation(len(index))
    return batch, {k: np.ascontiguousarray(v[perm]) for k, v in batch.items()}


def rows(expect, index):
    """Expected rows of a batch built from unique points: row index[i] of `expect`, the documented miss where index[i] < 0."""
    index = np.asarray(index)
    out = {}
    for k in FIELDS:
        picked = np.asarray(expect[k])[np.maximum(index, 0)].copy()
        picked[index < 0] = MISS[k]
        out[k] = picked
    return out


def radius_mix(d2):
    """A squared radius per point in a cycle of period 6: FLT_MAX (as none), d2 itself, the next float below d2, +inf, -1, NaN."""
    d2 = np.asarray(d2, np.float32)
    c = np.arange(len(d2)) % 6
    return np.select([c == 0, c == 1, c == 2, c == 3, c == 4], [FLT_MAX, d2, np.nextafter(d2, np.float32(-np.inf)), np.float32(np.inf),
                                                                 np.float32(-1.0)], np.float32(np.nan)).astype(np.float32)


FAR_Y = np.float32(-3.0e4)


def far_tail(points, lanes, n=None):
    """A batch of n > lanes + 64 points (default lanes + 1000 + 5) and its control.  Both tile `points`; both hold, above index
    `lanes`, one NaN point whose other components are larger than anything else in the batch.  The far batch alone holds, also
    above `lanes`, one point whose y = FAR_Y is negative and by far the batch's largest |coordinate|: it sets the pad.  Returns
    dict(far, control, unique, index_far, index_control): the batches, the unique points (`points`, then the far point, then the
    NaN point) and each batch's index into them."""
    u = len(points)
    n = lanes + 1005 if n is None else n
    far_at, nan_at = lanes + 17, lanes + 40
    assert n > nan_at and float(np.abs(points).max()) < 0.01 * abs(float(FAR_Y))
    unique = np.concatenate([points, [[0.5, FAR_Y, -0.25]], [[np.nan, 1.0e6, -1.0e7]]]).astype(np.float32)
    index_control = np.arange(n) % u
    index_control[nan_at] = u + 1
    index_far = index_control.copy()
    index_far[far_at] = u
    return dict(far=np.ascontiguousarray(unique[index_far]), control=np.ascontiguousarray(unique[index_control]), unique=unique,
                index_far=index_far, index_control=index_control)


def spoil_points(n, hits=None, radii=True):
    """A batch of length n with other answers than the one that follows: (points, max_dist2 or None - as the batch that follows
    has radii or not, so that both lay their buffers out alike).  By default every query is invalid, so every field comes back as
    a miss; ahead of a batch that expects misses pass `hits`, valid points of the scene."""
    if hits is None:
        return invalid_points(n, radii)
    return np.ascontiguousarray(hits[(np.arange(n) + 7) % len(hits)]), (np.full(n, FLT_MAX, np.float32) if radii else None)


def assert_stacked_expectations(answers, base_mesh, perm, points, limit_units, what):
    """The three expectations of stacked_copies that share nothing with closest_takes: every answer is in group 0; it is the
    smallest copy of the triangle it names; and the float64 yardstick's distance to that triangle is within limit_units x 2^-23 M
    (M: the largest |coordinate| of the point and the three corners) of the float64 minimum over all triangles.  Returns the
    largest excess in those units."""
    group, vertex0 = np.asarray(answers["group"]), np.asarray(answers["vertex0"])
    assert np.all(group == 0), "%s: %d answers outside group 0" % (what, int((group != 0).sum()))
    eg, ev = expected_copy(perm, group, vertex0)
    assert np.array_equal(eg, group) and np.array_equal(ev, vertex0), what
    tri = source_triangle(perm, group, vertex0)
    a, b, c = corners(base_mesh, tri)
    answered = yardstick(points, a, b, c)[0]
    aa, bb, cc = corners(base_mesh, np.arange(len(perm)))
    best = yardstick(points[:, None, :], aa[None], bb[None], cc[None])[0].min(1)
    M = np.max(np.abs(np.concatenate([points, a, b, c], axis=1)), axis=1).astype(np.float64)
    excess = float(((answered - best) / (2.0 ** -23 * M)).max())
    assert excess <= limit_units, (what, excess)
    return excess


# ---- the fixed choices the host proofs and the GPU tests share

SCHEDULE_SEEDS = {name: 100 + i for i, name in enumerate(FIXTURES)}       # the recipe seeds of tests/test_gpu_closest.py
PAD_LANES = 1024 * 256                   # k_closest_pad's grid (run_batch)
LONG_LIST = 10 * RECIPE_POINTS           # terrain_64's recipe tiled: at STACK_CAP=2 more points are listed than k_closest_exact has lanes
SCALE_SEED = 21
# The intermediate stack cap of the overflow tests, per tree width, with the number of terrain_64's 2,048 recipe points (seed 103)
# that the host walk lists at it.  4-wide: 17 -> 2,045, 18 -> 1,973, 19 -> 908, 20 -> 200, 21 -> 61, 23 -> 0; coincident at 19:
# 1,291.  8-wide: 3 -> 2,048, 4 -> 2,023, 5 -> 0 - there is no cap at which a quarter of terrain_64's points falls on each side,
# so the 8-wide cap is the one at which coincident's recipe splits (4: 1,468 listed, 580 not) and terrain_64 still has points on
# both sides.  tests/test_closest_cases_host.py asserts the shares.
MID_CAP = {4: 19, 8: 4}


def stacked_base():
    return height_field(16, 2)


def stacked_perm():
    return stacked_copies(stacked_base(), 4)[1]


def scale_meshes():
    """name -> mesh of the scale and degenerate cases: height_field(16, 2) with its zero-area records and reversed duplicate (1,280
    triangles) as it is, times 2^-70, 2^-45, 2^40, 2^58 and 2^62, moved by 1e3 and 1e6, and the stacked copies of
    height_field(16, 2).  2^62 is beyond what prt_upload_scene accepts (|coordinate| < 1e18): the host harness walks it, the device
    refuses it; 2^58 is the largest power of two that keeps this mesh below the limit, and the recipe's far points still lie
    more than 2^64 away, where d2 overflows."""
    base = with_degenerates(height_field(16, 2), 3)
    out = {"degenerate": base}
    for e in (-70, -45, 40, 58, 62):
        out["2^%d" % e] = scaled(base, e)
    out["+1e3"] = shifted(base, 1.0e3)
    out["+1e6"] = shifted(base, 1.0e6)
    out["stacked"] = stacked_copies(stacked_base(), 4)[0]
    return out


def far_tail_scene():
    """(mesh, points) of the far_tail tests: height_field(32, 1) and the 512 near-surface points of a 1,024-point recipe."""
    mesh = height_field(32, 1)
    pts, kind = recipe_points(mesh, 1024, 9)
    return mesh, np.ascontiguousarray(pts[kind == KIND_NEAR])


# ---- the scale sweep: float64 truth at every scale (tests/test_closest_cases_host.py and tests/test_signed_host.py prove it on the
# harnesses, tests/test_gpu_closest_schedules.py and tests/test_gpu_signed.py assert it on the device's own answers)

SWEEP_EXPONENTS = (-45, -34, -30, 0, 31, 34, 40, 58)
SWEEP_POINTS = 1024
SWEEP_CLOSED = ("cube", "l_prism", "torus")              # signed_cases.MESHES: the signed sweep, and with "height_field" the unsigned one


def sweep_mesh(name):
    import signed_cases
    return height_field(16, 2) if name == "height_field" else signed_cases.mesh_of(name)


def sweep_points(name):
    """The SWEEP_POINTS recipe points of a sweep mesh at 2^0: the signed recipe on the closed meshes, the closest recipe on the
    height field."""
    import signed_cases
    if name == "height_field":
        return recipe_points(sweep_mesh(name), SWEEP_POINTS, SCALE_SEED)[0]
    return signed_cases.recipe_points(sweep_mesh(name), SWEEP_POINTS, signed_cases.SEEDS[name])


def true_distance(mesh, points):
    """The float64 minimum over all triangles of the yardstick's distance, per point."""
    a, b, c = corners(mesh, np.arange(mesh[1].size // 3))
    with np.errstate(invalid="ignore", divide="ignore"):
        dist, v, w, _ = yardstick(np.asarray(points, np.float64)[:, None, :], a[None], b[None], c[None])
    return np.where(np.isfinite(dist) & np.isfinite(v) & np.isfinite(w), dist, np.inf).min(1)


def sweep_keep(best, e):
    """The points whose true squared distance times 2^2e is a normal float32, or exactly 0."""
    d2 = (np.asarray(best, np.float64) * 2.0 ** e) ** 2
    return (best == 0) | ((d2 > 2.0 ** -126) & (d2 < 2.0 ** 127))


def sweep_case(mesh, points, best, e):
    """(mesh x 2^e, kept points x 2^e, keep): both scaled exactly (asserted), every squared edge length a normal float32."""
    keep = sweep_keep(best, e)
    big = scaled(mesh, e)
    tri = big[0].astype(np.float64)[big[1].reshape(-1, 3).astype(np.int64)]
    edge2 = np.concatenate([((tri[:, i] - tri[:, j]) ** 2).sum(1) for i, j in ((0, 1), (0, 2), (1, 2))])
    edge2 = edge2[edge2 > 0]
    assert edge2.min() > 2.0 ** -126 and edge2.max() < 2.0 ** 127, e
    pts = np.ldexp(points[keep], e).astype(np.float32)
    assert np.array_equal(np.ldexp(pts.astype(np.float64), -e), points[keep].astype(np.float64)) and np.all(np.isfinite(pts))
    return big, np.ascontiguousarray(pts), keep


def assert_sweep_answers(answers, mesh, points, best, e, limit_units, what):
    """Conditions a and b of the sweep on the five closest-point fields of `answers` (for mesh x 2^e and points x 2^e; mesh, points
    and the float64 minimum `best` are the unscaled ones): no point misses; the float64 yardstick's distance to the reported
    triangle is within limit_units x 2^-23 M of `best` (M: the largest |coordinate| of the point and the three corners), and
    sqrt(dist2) x 2^-e is within the same limit of that distance.  Returns the two largest errors in those units."""
    group, vertex0 = np.asarray(answers["group"]), np.asarray(answers["vertex0"])
    missed = np.nonzero(group < 0)[0]
    assert missed.size == 0, "%s: %d of %d valid points miss, first %d" % (what, missed.size, len(group), missed[0])
    a, b, c = corners(mesh, input_triangle(mesh, group, vertex0))
    answered = yardstick(points, a, b, c)[0]
    unit = 2.0 ** -23 * np.max(np.abs(np.concatenate([points, a, b, c], axis=1)), axis=1).astype(np.float64)
    excess = (answered - best) / unit
    root = np.abs(np.ldexp(np.sqrt(np.asarray(answers["dist2"], np.float64)), -e) - answered) / unit
    assert excess.max() <= limit_units, "%s: the reported triangle is %.3g units farther than the nearest (point %d)" % (what, excess.max(), excess.argmax())
    assert root.max() <= limit_units, "%s: sqrt(dist2) is %.3g units off the distance to the reported triangle (point %d)" % (what, root.max(), root.argmax())
    return float(excess.max()), float(root.max())
