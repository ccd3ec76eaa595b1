"""Shared by tests/test_signed_host.py and tests/test_gpu_signed.py: closed meshes with shared vertices and outward winding, the
point recipe, a float64 numpy reference of the definition of prt_signed_distance (include/prt.h, csrc/dev_signed.h) with true
arccos, the analytic inside tests, and the runner of tests/signed_host_harness.cpp (a float32 brute force of the definition with
the PRT_HD functions of csrc/dev_signed.h and integer accumulators)."""
from __future__ import annotations

import struct

import numpy as np

import closest_cases as K
import harness
from closest_cases import bits, flat_desc, scene_mesh                       # noqa: F401  (re-exported)

POINTS = 2048
FIELDS = K.FIELDS + ("signed_distance", "feature")
FLT_MAX = K.FLT_MAX
MISS = dict(K.MISS, signed_distance=FLT_MAX, feature=np.uint8(255))
GPU_FIXTURES = ("icosphere_l3", "cornell_box", "coincident")
SEEDS = {name: 300 + i for i, name in enumerate(("tetrahedron", "cube", "l_prism", "torus", "fan") + GPU_FIXTURES)}
TORUS_R, TORUS_r = 1.0, 0.4


# ---- meshes: (positions (P, 3) f32, idx_positions u32, runs (G, 2) u32), one group, every vertex shared, outward winding

def _mesh(p, tri):
    tri = np.asarray(tri, np.uint32)
    return np.ascontiguousarray(p, np.float32), np.ascontiguousarray(tri.reshape(-1)), np.array([[0, tri.size]], np.uint32)


def _outward_from(p, tri, inner):
    """The triangles with their last two corners swapped where the normal points towards `inner` (one point per triangle)."""
    tri = np.asarray(tri, np.int64).copy()
    P = np.asarray(p, np.float64)
    a, b, c = P[tri[:, 0]], P[tri[:, 1]], P[tri[:, 2]]
    flip = (np.cross(b - a, c - a) * ((a + b + c) / 3.0 - inner)).sum(1) < 0
    tri[flip] = tri[flip][:, [0, 2, 1]]
    return tri


def tetrahedron():
    p = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float32)
    return _mesh(p, _outward_from(p, [[0, 1, 2], [0, 1, 3], [0, 2, 3], [1, 2, 3]], np.zeros(3)))


def cube():
    """[0, 1]^3: 8 vertices, 12 triangles."""
    p = np.array([[x, y, z] for z in (0, 1) for y in (0, 1) for x in (0, 1)], np.float32)
    quads = [[0, 1, 3, 2], [4, 5, 7, 6], [0, 1, 5, 4], [2, 3, 7, 6], [0, 2, 6, 4], [1, 3, 7, 5]]
    tri = [t for q in quads for t in ([q[0], q[1], q[2]], [q[0], q[2], q[3]])]
    return _mesh(p, _outward_from(p, tri, np.full(3, 0.5)))


L_POLYGON = np.array([[0, 0], [2, 0], [2, 1], [1, 1], [1, 2], [0, 2]], np.float64)     # counter-clockwise; reflex at (1, 1)


def l_prism():
    """The L-shaped hexagon [0, 2] x [0, 1] + [0, 1] x [0, 2] extruded over z in [0, 1]: 12 vertices, 20 triangles, one reflex edge."""
    p = np.concatenate([np.c_[L_POLYGON, np.zeros(6)], np.c_[L_POLYGON, np.ones(6)]]).astype(np.float32)
    cap = [[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 5]]                  # a fan from (0, 0): every triangle lies inside the L
    tri = [[a + 6, b + 6, c + 6] for a, b, c in cap] + [[a, c, b] for a, b, c in cap]
    for i in range(6):
        j = (i + 1) % 6
        tri += [[i, j, j + 6], [i, j + 6, i + 6]]
    return _mesh(p, tri)


def torus(n_major=24, n_minor=12):
    u = 2.0 * np.pi * np.arange(n_major) / n_major
    v = 2.0 * np.pi * np.arange(n_minor) / n_minor
    uu, vv = np.meshgrid(u, v, indexing="ij")
    ring = TORUS_R + TORUS_r * np.cos(vv)
    p = np.stack([ring * np.cos(uu), ring * np.sin(uu), TORUS_r * np.sin(vv)], -1).reshape(-1, 3).astype(np.float32)
    at = lambda i, j: (i % n_major) * n_minor + (j % n_minor)          # noqa: E731
    tri = []
    for i in range(n_major):
        for j in range(n_minor):
            tri += [[at(i, j), at(i + 1, j), at(i + 1, j + 1)], [at(i, j), at(i + 1, j + 1), at(i, j + 1)]]
    tri = np.array(tri)
    c = p.astype(np.float64)[tri].mean(1)
    ang = np.arctan2(c[:, 1], c[:, 0])
    inner = np.stack([TORUS_R * np.cos(ang), TORUS_R * np.sin(ang), np.zeros(len(c))], -1)      # the tube's centre line
    return _mesh(p, _outward_from(p, tri, inner))


def fan(n=200):
    """A cone over a regular n-gon, closed by a fan from the base's centre: the apex and the centre have n incident triangles each."""
    t = 2.0 * np.pi * np.arange(n) / n
    p = np.concatenate([[[0, 0, 1], [0, 0, 0]], np.stack([np.cos(t), np.sin(t), np.zeros(n)], -1)]).astype(np.float32)
    tri = [[0, 2 + i, 2 + (i + 1) % n] for i in range(n)] + [[1, 2 + (i + 1) % n, 2 + i] for i in range(n)]
    return _mesh(p, _outward_from(p, tri, np.array([0.0, 0.0, 0.25])))


MESHES = {"tetrahedron": tetrahedron, "cube": cube, "l_prism": l_prism, "torus": torus, "fan": fan}


def mesh_of(name):
    return MESHES[name]() if name in MESHES else scene_mesh(name)


SHEAR_MIRROR = np.array([[-1.25, 0.0, 0.0], [0.5, 0.75, 0.0], [-0.25, 0.125, 1.5]], np.float32)


def sheared_mirror(mesh):
    """The mesh sheared and mirrored in x (float32): the winding stays, so every normal - and every sign - flips."""
    p, idx, runs = mesh
    return sheared_mirror_points(p), idx, runs


def sheared_mirror_points(points):
    return np.ascontiguousarray((points @ SHEAR_MIRROR).astype(np.float32))


# ---- the analytic inside tests (float64, of float32 points)

def inside_cube(q):
    q = np.asarray(q, np.float64)
    return np.all((q > 0) & (q < 1), axis=1)


def inside_l_prism(q):
    q = np.asarray(q, np.float64)
    box = lambda lo, hi: np.all((q > lo) & (q < hi), axis=1)             # noqa: E731
    return box(np.array([0, 0, 0]), np.array([2, 1, 1])) | box(np.array([0, 0, 0]), np.array([1, 2, 1]))


def torus_sdf(q):
    q = np.asarray(q, np.float64)
    return np.sqrt((np.sqrt(q[:, 0] ** 2 + q[:, 1] ** 2) - TORUS_R) ** 2 + q[:, 2] ** 2) - TORUS_r


# ---- the point recipe

def recipe_points(mesh, n, seed):
    """n float32 points, seeded: closest_cases.recipe_points(mesh, n, seed), and for half of the points a displacement of 10^-3 to
    10^-1 x the extent (log-uniform) in a random direction from a vertex or an edge point.  The displaced half: every point the
    base recipe put on a vertex or an edge midpoint (n/8; displaced from where it is) and 3n/8 of the others, replaced by a random
    vertex (half of them) or a random point of a random edge, displaced.  Every region code occurs in every batch.  The order is
    the base recipe's."""
    p, idx, runs = mesh
    rng = np.random.default_rng(seed + 1000)
    pts, kind = K.recipe_points(mesh, n, seed)
    pts = pts.astype(np.float64)
    on = np.nonzero(kind == K.KIND_ON)[0]
    others = rng.permutation(np.nonzero(kind != K.KIND_ON)[0])[: n // 2 - len(on)]
    m = len(others)
    tri = rng.integers(0, idx.size // 3, m)
    corner = rng.integers(0, 3, m)
    a = p[idx[3 * tri + corner]].astype(np.float64)
    b = p[idx[3 * tri + (corner + 1) % 3]].astype(np.float64)
    t = rng.uniform(0.0, 1.0, (m, 1))
    t[: m // 2] = 0.0
    pts[others] = a + (b - a) * t
    moved = np.concatenate([on, others])
    d = rng.standard_normal((len(moved), 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    pts[moved] += d * K.mesh_extent(mesh)[2] * 10.0 ** rng.uniform(-3.0, -1.0, (len(moved), 1))
    return np.ascontiguousarray(pts.astype(np.float32))


def surface_points(mesh, n, seed):
    """n float32 points on vertices and edge midpoints ((a + b) * 0.5 in float32): the ones closest_cases.recipe_points makes."""
    pts, kind = K.recipe_points(mesh, 8 * n, seed)
    return np.ascontiguousarray(pts[kind == K.KIND_ON][:n])


# ---- the float64 reference of the definition: true arccos, float sums

def reference(mesh, points):
    """signed distance (float64, nan for no candidate), region and input triangle of every point by the definition evaluated in
    float64: Ericson's walk over every triangle (closest_cases.yardstick), the smallest distance (the first triangle among equal
    ones), N = cross(ab, ac), the sum of the unit normals over the edge's triangles, or the angle-weighted sum over the vertex's."""
    p, idx, runs = mesh
    P = p.astype(np.float64)
    tri = idx.reshape(-1, 3).astype(np.int64)
    a, b, c = P[tri[:, 0]], P[tri[:, 1]], P[tri[:, 2]]
    cr = np.cross(b - a, c - a)
    with np.errstate(divide="ignore", invalid="ignore"):
        nh = cr / np.linalg.norm(cr, axis=1, keepdims=True)

        def angle(u, v):
            return np.arccos(np.clip((u * v).sum(1) / (np.linalg.norm(u, axis=1) * np.linalg.norm(v, axis=1)), -1.0, 1.0))
        alpha = np.stack([angle(b - a, c - a), angle(a - b, c - b), angle(a - c, b - c)], 1)
    ok = np.all(np.isfinite(nh), axis=1) & np.all(np.isfinite(alpha), axis=1)
    vert_n = np.zeros((len(P), 3))
    edge_n = {}
    for t in np.nonzero(ok)[0]:
        for k in range(3):
            vert_n[tri[t, k]] += alpha[t, k] * nh[t]
        for i, j in ((0, 1), (0, 2), (1, 2)):
            key = (min(tri[t, i], tri[t, j]), max(tri[t, i], tri[t, j]))
            edge_n[key] = edge_n.get(key, np.zeros(3)) + nh[t]
    pts = np.asarray(points, np.float64)
    with np.errstate(invalid="ignore"):
        dist, v, w, region = K.yardstick(pts[:, None, :], a[None], b[None], c[None])
    dist = np.where(np.isfinite(dist) & np.isfinite(v) & np.isfinite(w), dist, np.inf)
    win = dist.argmin(1)
    rows = np.arange(len(pts))
    d, v, w, region = dist[rows, win], v[rows, win], w[rows, win], region[rows, win]
    q = a[win] + (b[win] - a[win]) * v[:, None] + (c[win] - a[win]) * w[:, None]
    N = cr[win].copy()
    corner_of = {0: 0, 1: 1, 3: 2}
    edge_of = {2: (0, 1), 4: (0, 2), 5: (1, 2)}
    for i in np.nonzero(region != 6)[0]:
        r, t = int(region[i]), win[i]
        if r in corner_of:
            N[i] = vert_n[tri[t, corner_of[r]]]
        else:
            e0, e1 = tri[t, edge_of[r][0]], tri[t, edge_of[r][1]]
            N[i] = edge_n.get((min(e0, e1), max(e0, e1)), np.zeros(3))
    s = ((pts - q) * N).sum(1)
    # a distance within float64 rounding of the coordinates is a point of the surface: d2 == 0, the non-negative branch
    scale = max(float(np.abs(P[tri]).max()) if len(tri) else 0.0, 1e-300)
    s = np.where(d <= 2.0 ** -48 * np.maximum(scale, np.abs(pts).max(1)), 0.0, s)
    return np.where(np.isfinite(d), np.where(s < 0, -d, d), np.nan), region, win


def mesh_angle_cosines(mesh):
    """The float64 interior angles of every non-degenerate triangle of the float32 mesh, (n, 3) at corners a, b, c, and the rows kept."""
    p, idx, runs = mesh
    P = p.astype(np.float64)
    tri = idx.reshape(-1, 3)
    a, b, c = P[tri[:, 0]], P[tri[:, 1]], P[tri[:, 2]]

    def angle(u, v):
        return np.arctan2(np.linalg.norm(np.cross(u, v), axis=1), (u * v).sum(1))
    alpha = np.stack([angle(b - a, c - a), angle(a - b, c - b), angle(a - c, b - c)], 1)
    keep = np.linalg.norm(np.cross(b - a, c - a), axis=1) > 0
    return alpha, keep


# ---- the host harness

def build_harness(directory, sanitize=False):
    return harness.build("signed_host_harness.cpp", directory, "signed_host" + ("_san" if sanitize else ""), sanitize=sanitize)


def case(mesh, points, max_dist2=None):
    return dict(mesh=mesh, points=np.ascontiguousarray(points, np.float32), max_dist2=max_dist2)


def sweep(x):
    """A case that evaluates signed_acos on the float32 array x (its length a multiple of 3)."""
    x = np.ascontiguousarray(x, np.float32)
    assert x.size % 3 == 0
    return dict(sweep=x)


def run_harness(exe, cases, directory):
    """Every case through the harness in one run.  Per case a dict {field: array} of the seven fields plus "angles" (n_tris, 3); a
    sweep gives {"acos": array}."""
    fin, fout = harness.case_files(directory, "signed_cases.bin", "signed_results.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for c in cases:
            if "sweep" in c:
                f.write(struct.pack("<5I", c["sweep"].size // 3, 0, 0, 0, 2))
                f.write(c["sweep"].tobytes())
                continue
            p, idx, runs = c["mesh"]
            n = c["points"].shape[0]
            f.write(struct.pack("<5I", n, p.shape[0], idx.size, runs.shape[0], 1 if c["max_dist2"] is not None else 0))
            f.write(c["points"].tobytes())
            if c["max_dist2"] is not None:
                harness.put(f, (c["max_dist2"], np.float32))
            harness.put(f, (p, np.float32), (idx, np.uint32), (runs, np.uint32))
    harness.run(exe, fin, fout)
    r, out = harness.Reader.of_file(fout), []
    for c in cases:
        if "sweep" in c:
            out.append(dict(acos=r.take(c["sweep"].size, np.float32)))
            continue
        n, n_tris = c["points"].shape[0], c["mesh"][1].size // 3
        out.append(dict(dist2=r.take(n, np.float32), point=r.take(3 * n, np.float32, (n, 3)), bw=r.take(3 * n, np.float32, (n, 3)),
                        vertex0=r.take(n, np.uint32), group=r.take(n, np.int32), signed_distance=r.take(n, np.float32),
                        feature=r.take(n, np.uint8), angles=r.take(3 * n_tris, np.float32, (n_tris, 3))))
    r.done()
    return out


def assert_same_bits(got, expect, what, fields=FIELDS):
    """Every field of `got` equals `expect` bit for bit."""
    harness.assert_same_bits(got, expect, what, fields)


def to_numpy(res):
    """A signed_distance result with torch tensors -> numpy arrays (vertex0 back to uint32)."""
    return K.to_numpy(res)


# ---- the scale sweep (closest_cases.SWEEP_EXPONENTS): conditions c and d on the unscaled mesh

ANGLE_GATE = 8.0 * 2.0 ** -24 / np.sin(0.015) + 2.0 ** -20            # DESIGN.md section 4.12; argued in tests/test_signed_host.py
OFF_SURFACE = 1e-4                                                    # x extent: closer points' signs are rounding noise
INSIDE = {"cube": inside_cube, "l_prism": inside_l_prism}


def assert_sweep_signs(signed_distance, name, mesh, points, ref_sd, what):
    """Condition c: the sign is the float64 reference's on the unscaled mesh for every point at least OFF_SURFACE extents off the
    surface, and on the cube and the L-prism the analytic inside test's.  Returns the number of points checked."""
    negative = np.asarray(signed_distance) < 0
    checked = np.abs(ref_sd) >= OFF_SURFACE * K.mesh_extent(mesh)[2]
    wrong = (negative != (ref_sd < 0)) & checked
    assert not wrong.any(), "%s: %d of %d checked signs differ from the float64 reference, first %d" % (what, wrong.sum(), checked.sum(), np.nonzero(wrong)[0][0])
    if name in INSIDE:
        wrong = (negative != INSIDE[name](points)) & checked
        assert not wrong.any(), "%s: %d of %d checked signs differ from the analytic inside test" % (what, wrong.sum(), checked.sum())
    return int(checked.sum())


def assert_sweep_angles(angles, mesh, what):
    """Condition d: every non-degenerate triangle has its three angles, each within ANGLE_GATE of float64."""
    alpha, keep = mesh_angle_cosines(mesh)
    got = np.asarray(angles, np.float64)
    assert np.all(np.isfinite(got[keep])), "%s: %d non-degenerate triangles without angles" % (what, (~np.isfinite(got[keep]).all(1)).sum())
    err = float(np.abs(got[keep] - alpha[keep]).max())
    assert err <= ANGLE_GATE, "%s: angle error %.3e" % (what, err)
    return err


# ---- the topologies the definition speaks of: boundary edges, unwelded vertices, edges of three triangles,
# accumulators that cancel, records that contribute nothing, positions nobody uses, several groups.  TOPOLOGY_POINTS recipe points each.

TOPOLOGY_POINTS = 1024


def open_sheet():
    """height_field(16, 2): 512 triangles, the rim's edges have one triangle each."""
    return K.height_field(16, 2)


def unwelded(mesh):
    """Every triangle owns its three positions: equal coordinates under different indices, every edge a boundary edge."""
    p, idx, runs = mesh
    return np.ascontiguousarray(p[idx]), np.arange(idx.size, dtype=np.uint32), runs.copy()


def non_manifold():
    """Three quads around the edge (0, 0, 0) - (0, 0, 1), at 0, 100 and 230 degrees: 8 positions, 6 triangles, one edge of six
    triangle sides."""
    p = [[0, 0, 0], [0, 0, 1]]
    tri = []
    for k, deg in enumerate((0.0, 100.0, 230.0)):
        c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
        p += [[c, s, 0], [c, s, 1]]
        lo, hi = 2 + 2 * k, 3 + 2 * k
        tri += [list(np.roll([0, lo, hi], k)), list(np.roll([0, hi, 1], k))]     # the shared edge is ab, ca or bc: a quad each
    return _mesh(np.array(p, np.float32), tri)


def back_to_back():
    """height_field(8, 5) and its copy with reversed winding on the same indices: every accumulator cancels to exactly 0."""
    p, idx, runs = K.height_field(8, 5)
    tri = idx.reshape(-1, 3)
    return _mesh(p, np.concatenate([tri, tri[:, [0, 2, 1]]]))


def degenerate_cube():
    return K.with_degenerates(cube(), 3)


def unreferenced_and_repeated():
    """The cube, three positions that no triangle uses (one of them far away) and a triangle (a, a, b) on the diagonal 0 - 7."""
    p, idx, runs = cube()
    p = np.concatenate([[[9.0, 9.0, 9.0]], p, [[0.5, 0.5, 0.5], [-3.0, 0.25, 0.75]]]).astype(np.float32)
    tri = np.concatenate([idx.reshape(-1, 3).astype(np.int64) + 1, [[1, 1, 8]]])
    return _mesh(p, tri)


def multi_group(mesh, seed=8):
    """The mesh's triangles shuffled and split over three groups that lie in the index buffer in the order 2, 0, 1."""
    p, idx, runs = mesh
    tri = idx.reshape(-1, 3)[np.random.default_rng(seed).permutation(idx.size // 3)]
    third = 3 * (len(tri) // 3)
    first = [0, third, 2 * third, 3 * len(tri)]
    order = (2, 0, 1)
    return p, np.ascontiguousarray(tri.reshape(-1)), np.array([[first[k], first[k + 1] - first[k]] for k in order], np.uint32)


TOPOLOGIES = {"open": open_sheet, "unwelded": lambda: unwelded(cube()), "non_manifold": non_manifold, "back_to_back": back_to_back,
              "degenerate": degenerate_cube, "unreferenced": unreferenced_and_repeated, "multi_group": lambda: multi_group(torus())}
TOPOLOGY_SEEDS = {name: 330 + i for i, name in enumerate(TOPOLOGIES)}


def topology_case(name):
    """(mesh, its TOPOLOGY_POINTS recipe points); multi_group: the points of the one-group torus, whose sums it must repeat."""
    mesh = TOPOLOGIES[name]()
    if name == "multi_group":
        return mesh, recipe_points(torus(), TOPOLOGY_POINTS, SEEDS["torus"])
    return mesh, recipe_points(mesh, TOPOLOGY_POINTS, TOPOLOGY_SEEDS[name])
