"""Shared by tests/test_trace_edges_host.py and tests/test_gpu_trace_edges.py: ray queries on the inputs the committed fixtures
(tests/trace_golden.py: six ray families, lengths 10^+-3, four ordinary scenes) never produce - directions with exact zeros of
either sign, rays in the plane of a wall and through vertices, components around trav_init's 1e-30 clamp, directions of length
2^-120 to 2^120, scenes scaled by 2^-45 to 2^30 or moved 10^6 away, scenes of one to five triangles, a flat one, one with
zero-area records.  numpy only.

A case is a scene (an object with .desc: the one prt_scene_desc that goes to the CPU oracle and to Renderer.upload, spheres
included - TraceRay walks them), rays and one ray_bias (0).  Nothing is expected from a file: the answers are the oracle's on
that desc at test time (tests/trace_oracle_harness.cpp: TraceRay; brute force for OCCLUDED, bf_t and near_tie), with tmax set
around the brute-force closest t as trace_golden.generate sets it.  Every recipe is seeded.  case(id) builds a case once per
process; CASES lists the ids.  Meta arrays per ray, for the host test that proves the cases are what they claim: kind (the
recipe), axis (the +-1 axis of an `axis` ray, the zero axis of a `plane` ray), aimed and target (the vertex or float32 edge
midpoint an aimed ray shares coordinates with)."""
from __future__ import annotations

import os
import tempfile

import numpy as np

import closest_cases as K
import trace_cases as T
import trace_golden
from conftest import host_scene

FLT_MAX = T.FLT_MAX
BASE = ("cornell_box", "icosphere_l3", "coincident")
TWO = ("cornell_box", "icosphere_l3")
CLAMP = np.float32(1e-30)
CLAMP_VALUES = np.array([2.0 ** -149, 2.0 ** -126, np.nextafter(CLAMP, np.float32(0)), CLAMP, np.nextafter(CLAMP, np.float32(1)),
                         2.0 ** -99, 2.0 ** -64], np.float32)
LENGTH_EXPONENTS = (-120, -110, -100, -95, -60, 60, 100, 120)
SCALE_ORIGINS_ONLY = (-45, -20, 20)            # origins scaled, directions as they are
SCALE_SIMILAR = (-30, 30)                      # directions scaled too: an exact similarity, the same t
SHIFTS = (1.0e3, 1.0e6)
TINY = ("1", "2", "3", "4", "5", "5x2")        # triangles (x groups)
SPHERE_SLACK = np.float32(1.0 + 2.0 ** -10)    # a moved scene's radii: its positions are rounded again


class Scene:
    """What a case traces: obj.desc for the oracle and the upload, and the triangles as arrays."""

    def __init__(self, obj):
        from par_raytracer_amd import api
        self.obj = obj
        self.arrays = api.desc_arrays(obj.desc)
        self.positions = self.arrays["positions"].reshape(-1, 3)
        self.tri = self.arrays["idx_positions"].astype(np.int64).reshape(-1, 3)

    @property
    def desc(self):
        return self.obj.desc

    def box(self):
        used = self.positions[np.unique(self.tri)]
        return used.min(0), used.max(0)


_SCENES = {}


def _cached(key, make):
    if key not in _SCENES:
        _SCENES[key] = make()
    return _SCENES[key]


def base_scene(name):
    return _cached(name, lambda: Scene(host_scene(name, 0)))


def box_centre(name):
    lo, hi = base_scene(name).box()
    return ((lo + hi) * np.float32(0.5)).astype(np.float32)


def transformed(name, e=0, shift=0.0):
    """The base scene times 2^e (exact) plus `shift` (a scalar or one float per axis; rounded to float32), spheres along: centres
    and radii scaled; for a shift the centres moved and the radii widened by 2^-10."""
    def make():
        from par_raytracer_amd import api
        a = dict(base_scene(name).arrays)
        off = np.asarray(shift, np.float32)
        moved = bool(np.any(off != 0))
        p = np.ldexp(a["positions"].reshape(-1, 3), e).astype(np.float32)
        assert np.array_equal(np.ldexp(p.astype(np.float64), -e), a["positions"].reshape(-1, 3).astype(np.float64))
        sph = a["spheres"].copy().view(np.float32).reshape(-1, 6)                 # centre, radius, (c0, c1 as bits)
        sph[:, :4] = np.ldexp(sph[:, :4], e)
        if moved:
            p = (p + off).astype(np.float32)
            sph[:, :3] = sph[:, :3] + off
            sph[:, 3] = sph[:, 3] * SPHERE_SLACK
        a["positions"] = np.ascontiguousarray(p.reshape(-1))
        a["spheres"] = np.ascontiguousarray(sph.reshape(-1)).view(np.uint8)
        return Scene(api.FlatDesc(a))
    return _cached((name, e, tuple(np.broadcast_to(np.asarray(shift, np.float32), 3).tolist())), make)


def centred(name):
    """The scene moved by minus its float32 box centre: the origin 0 lies inside."""
    return transformed(name, 0, -box_centre(name))


def write_obj(directory, mesh, name="scene.obj"):
    """A (positions, indices, runs) mesh of tests/closest_cases.py as OBJ text, a group per run."""
    p, idx, runs = mesh
    lines = ["v %.9g %.9g %.9g" % tuple(float(x) for x in v) for v in p] + ["vt 0 0", "vn 0 0 1"]
    for g, (first, count) in enumerate(np.asarray(runs).tolist()):
        lines.append("g g%d" % g)
        lines += ["f %d/1/1 %d/1/1 %d/1/1" % tuple(int(i) + 1 for i in t) for t in idx[first:first + count].reshape(-1, 3)]
    with open(os.path.join(directory, name), "w") as f:
        f.write("\n".join(lines) + "\n")


def obj_scene(key, mesh):
    def make():
        from par_raytracer_amd import api
        d = tempfile.mkdtemp(prefix="prt_edge_%s_" % key)
        write_obj(d, mesh)
        return Scene(api.HostScene(d, "scene.obj", 0, (0.0, 0.0, 0.0)))
    return _cached(("obj", key), make)


def tiny_mesh(which):
    """1 to 5 random triangles in the unit cube, one group; "5x2": five in two groups (2 + 3)."""
    n = int(which[0])
    rng = np.random.default_rng(40 + n)
    p = rng.uniform(0, 1, (3 * n, 3)).astype(np.float32)
    idx = np.arange(3 * n, dtype=np.uint32)
    runs = [[0, 3 * n]] if which == str(n) else [[0, 6], [6, 3 * n - 6]]
    return p, idx, np.array(runs, np.uint32)


def flat_mesh(n=8):
    """n x n cells, two triangles each, in the plane y = 0.5, facing +y: the scene's extent on y is 0."""
    g = np.linspace(0.0, 1.0, n + 1)
    x, z = np.meshgrid(g, g, indexing="xy")
    p = np.stack([x, np.full_like(x, 0.5), z], axis=-1).reshape(-1, 3).astype(np.float32)
    i, j = (a.reshape(-1) for a in np.meshgrid(np.arange(n), np.arange(n), indexing="ij"))
    v00 = i * (n + 1) + j
    v01, v10, v11 = v00 + 1, v00 + n + 1, v00 + n + 2
    idx = np.stack([v00, v11, v01, v00, v10, v11], axis=1).reshape(-1).astype(np.uint32)
    return p, idx, np.array([[0, idx.size]], np.uint32)


def degenerate_mesh():
    return K.with_degenerates(K.height_field(16, 2), 3)


# ---- ray recipes: (scene, n, rng) -> dict of per-ray arrays

def _blank(n, kind):
    return {"origins": np.zeros((n, 3), np.float32), "directions": np.zeros((n, 3), np.float32), "kind": np.full(n, kind, "U5"),
            "axis": np.full(n, -1, np.int8), "aimed": np.zeros(n, bool), "target": np.zeros((n, 3), np.float32)}


def _targets(sc, n, rng):
    """n vertices or float32 edge midpoints (a + b) * 0.5f of random triangles."""
    t = sc.positions[sc.tri[rng.integers(0, len(sc.tri), n)]]
    c = rng.integers(0, 3, n)
    a, b = t[np.arange(n), c], t[np.arange(n), (c + 1) % 3]
    mid = ((a + b) * np.float32(0.5)).astype(np.float32)
    return np.where((rng.uniform(0, 1, n) < 0.5)[:, None], mid, a).astype(np.float32)


def _extent(sc):
    lo, hi = sc.box()
    return lo, hi, np.float32((hi - lo).max())


def axis_rays(sc, n, rng):
    """+-unit along one axis, the other two components +0.0 or -0.0 (pair i % 4); odd rays share two coordinates bitwise with a
    vertex or an edge midpoint and start 0.1 to 0.9 extents before it, even rays start anywhere in the box."""
    out = _blank(n, "axis")
    lo, hi, ext = _extent(sc)
    ax = rng.integers(0, 3, n)
    sign = np.where(rng.uniform(0, 1, n) < 0.5, np.float32(-1), np.float32(1))
    i = np.arange(n)
    d = out["directions"]
    d[i, (ax + 1) % 3] = np.where(i % 4 & 1, np.float32(-0.0), np.float32(0.0))
    d[i, (ax + 2) % 3] = np.where(i % 4 & 2, np.float32(-0.0), np.float32(0.0))
    d[i, ax] = sign
    o = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    aimed = i % 2 == 1
    target = _targets(sc, n, rng)
    back = (target[i, ax] - sign * (rng.uniform(0.1, 0.9, n).astype(np.float32) * ext)).astype(np.float32)
    o[aimed] = target[aimed]
    o[i[aimed], ax[aimed]] = back[aimed]
    out.update(origins=o, axis=ax.astype(np.int8), aimed=aimed, target=np.where(aimed[:, None], target, 0).astype(np.float32))
    return out


def plane_rays(sc, n, rng):
    """One component +-0.0 (sign by ray parity), the other two random and normalised in float32.  The ray runs, in the plane
    that fixes its origin's coordinate on the zero axis, towards a point of the scene from 0.2 to 1.5 extents away: a random
    point of a random triangle, or (odd pairs, `aimed`) a vertex, whose coordinate on the zero axis the origin then shares bit
    for bit.  Every fourth ray starts anywhere in the box grown by half an extent instead."""
    out = _blank(n, "plane")
    _, _, ext = _extent(sc)
    ax = rng.integers(0, 3, n)
    i = np.arange(n)
    v = rng.normal(size=(n, 2)).astype(np.float32)
    v = (v / np.sqrt(v[:, :1] * v[:, :1] + v[:, 1:] * v[:, 1:])).astype(np.float32)
    d = out["directions"]
    d[i, ax] = np.where(i % 2 == 1, np.float32(-0.0), np.float32(0.0))
    d[i, (ax + 1) % 3], d[i, (ax + 2) % 3] = v[:, 0], v[:, 1]
    aimed = (i // 2) % 2 == 1
    t = sc.positions[sc.tri[rng.integers(0, len(sc.tri), n)]]
    uv = rng.uniform(0, 1, (n, 2)).astype(np.float32)
    flip = uv.sum(1) > 1
    uv[flip] = 1 - uv[flip]
    inner = (t[:, 0] + uv[:, :1] * (t[:, 1] - t[:, 0]) + uv[:, 1:] * (t[:, 2] - t[:, 0])).astype(np.float32)
    target = np.where(aimed[:, None], t[i, rng.integers(0, 3, n)], inner).astype(np.float32)
    o = (target - d * (rng.uniform(0.2, 1.5, (n, 1)).astype(np.float32) * ext)).astype(np.float32)
    o[i, ax] = target[i, ax]
    lo, hi, _ = _extent(sc)
    loose = i % 4 == 0                                    # a quarter starts anywhere around the scene: most of these miss
    o[loose] = rng.uniform(lo - 0.5 * ext, hi + 0.5 * ext, (n, 3)).astype(np.float32)[loose]
    out.update(origins=o, axis=ax.astype(np.int8), aimed=aimed, target=np.where(aimed[:, None], target, 0).astype(np.float32))
    return out


def front_rays(sc, n, rng):
    """trace_golden's family `front`: aimed at points of random triangles from their front side, unit length."""
    out = _blank(n, "front")
    _, _, ext = _extent(sc)
    t = sc.positions[sc.tri[rng.integers(0, len(sc.tri), n)]].astype(np.float64)
    uv = rng.uniform(0, 1, (n, 2))
    flip = uv.sum(1) > 1
    uv[flip] = 1 - uv[flip]
    p = t[:, 0] + uv[:, :1] * (t[:, 1] - t[:, 0]) + uv[:, 1:] * (t[:, 2] - t[:, 0])
    nrm = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    length = np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm = np.where(length > 0, nrm / np.where(length > 0, length, 1), [0.0, 0.0, 1.0])       # a zero-area record has no front
    src = p + nrm * rng.uniform(0.02, 0.5, (n, 1)) * float(ext) + rng.normal(size=(n, 3)) * 0.1 * float(ext)
    d = p - src
    out.update(origins=src.astype(np.float32), directions=(d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32))
    return out


def clamp_rays(sc, n, rng):
    """`front` rays whose smallest component (odd rays: smallest two) is replaced by +- a value of CLAMP_VALUES; slot and value
    record which and what (-1 / 0: untouched)."""
    out = front_rays(sc, n, rng)
    out["kind"][:] = "clamp"
    d = out["directions"]
    i = np.arange(n)
    order = np.argsort(np.abs(d), axis=1)
    slot = np.stack([order[:, 0], np.where(i % 2 == 1, order[:, 1], -1)], 1).astype(np.int8)
    value = np.stack([CLAMP_VALUES[i % 7] * np.where(i // 7 % 2, np.float32(-1), np.float32(1)),
                      CLAMP_VALUES[(i // 14) % 7] * np.where(i // 2 % 2, np.float32(-1), np.float32(1))], 1).astype(np.float32)
    value[slot[:, 1] < 0, 1] = 0
    d[i, slot[:, 0]] = value[:, 0]
    two = slot[:, 1] >= 0
    d[i[two], slot[two, 1]] = value[two, 1]
    out.update(slot=slot, value=value)
    return out


def length_directions(n, rng):
    """Random unit vectors x 2^k, k = LENGTH_EXPONENTS[i * 8 // n]; ray i % 4 == 1: one component further x 1e-3, i % 4 == 2:
    another x 1e-2 (exponent: k per ray)."""
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    i = np.arange(n)
    c = rng.integers(0, 3, n)
    u[i, c] *= np.where(i % 4 == 1, 1e-3, 1.0)
    u[i, (c + 1) % 3] *= np.where(i % 4 == 2, 1e-2, 1.0)
    k = np.array(LENGTH_EXPONENTS)[i * len(LENGTH_EXPONENTS) // n]
    return np.ldexp(u, k[:, None]).astype(np.float32), k


def fixture_rays(name, n=1024):
    g = T.fixture(name)
    sel = T.bias0(g)[:n]
    return np.ascontiguousarray(g["origins"][sel]), np.ascontiguousarray(g["directions"][sel])


def _concat(parts):
    return {k: np.ascontiguousarray(np.concatenate([p[k] for p in parts])) for k in parts[0]}


def _mixed(sc, n, rng, recipes):
    per = [n // len(recipes) + (1 if k < n % len(recipes) else 0) for k in range(len(recipes))]
    return _concat([f(sc, m, rng) for f, m in zip(recipes, per)])


# ---- the cases

def _ids():
    ids = ["axis-" + s for s in BASE] + ["plane-" + s for s in BASE] + ["clamp-icosphere_l3"] + ["length-" + s for s in TWO + ("flat_grid",)]
    ids += ["scale-%s@%d" % (s, e) for s in TWO for e in SCALE_ORIGINS_ONLY + SCALE_SIMILAR]
    ids += ["shift-%s@%g" % (s, off) for s in TWO for off in SHIFTS]
    return ids + ["tiny-" + t for t in TINY] + ["flat-grid", "degenerate-field"]


CASES = _ids()
# the device traversal on the host runs these (all of them: the box test walks another ray than the triangle test where o + d
# rounds, which the scaled and shifted scenes show)
HOST_WALK_FAMILIES = ("axis", "plane", "clamp", "length", "scale", "shift", "tiny", "flat", "degenerate")
_BUILT = {}


def build(cid):
    """(scene, rays) of case `cid`, before the oracle."""
    family, _, rest = cid.partition("-")
    rng = np.random.default_rng(7000 + CASES.index(cid))
    if family == "axis":
        sc = base_scene(rest)
        return sc, axis_rays(sc, 8192 if rest == "cornell_box" else 1536, rng)
    if family == "plane":
        sc = base_scene(rest)
        return sc, plane_rays(sc, 1536, rng)
    if family == "clamp":
        sc = base_scene(rest)
        return sc, clamp_rays(sc, 1024, rng)
    if family == "length":
        d, k = length_directions(1024, rng)
        rays = _concat([_blank(1024, "len0"), _blank(1024, "lenfx")])
        rays["directions"] = np.concatenate([d, d])
        if rest == "flat_grid":
            # from the origin 0, every ray of cornell_box starts inside every box of its two-node tree and every ray of
            # icosphere_l3 faces the sphere's back: neither can show a bent ray.  The flat grid's 128 triangles lie a twentieth
            # below the origin and face it; the second batch starts on a grid of points above them.
            p, idx, runs = flat_mesh()
            sc = obj_scene("flat_below", ((p - np.array([0.5, 0.55, 0.5], np.float32)).astype(np.float32), idx, runs))
            rays["origins"][1024:] = rng.uniform([-0.5, 0.0, -0.5], [0.5, 1.0, 0.5], (1024, 3)).astype(np.float32)
        else:
            sc = centred(rest)
            rays["origins"][1024:] = (fixture_rays(rest)[0] - box_centre(rest)).astype(np.float32)
        rays["exponent"] = np.concatenate([k, k])
        return sc, rays
    if family == "scale":
        name, e = rest.split("@")[0], int(rest.split("@")[1])
        sc = transformed(name, e)
        o, d = fixture_rays(name)
        rays = _blank(len(o), "scale")
        rays["origins"] = np.ldexp(o, e).astype(np.float32)
        rays["directions"] = np.ldexp(d, e).astype(np.float32) if e in SCALE_SIMILAR else d
        return sc, rays
    if family == "shift":
        name, off = rest.split("@")
        sc = transformed(name, 0, float(off))
        o, d = fixture_rays(name)
        rays = _blank(len(o), "shift")
        rays["origins"] = (o + np.float32(float(off))).astype(np.float32)
        rays["directions"] = d
        return sc, rays
    if family == "tiny":
        sc = obj_scene("tiny" + rest, tiny_mesh(rest))
        return sc, _mixed(sc, 256, rng, (axis_rays, plane_rays, front_rays))
    if family == "flat":
        sc = obj_scene("flat", flat_mesh())
        return sc, _mixed(sc, 512, rng, (axis_rays, plane_rays, front_rays))
    assert family == "degenerate", cid
    sc = obj_scene("degenerate", degenerate_mesh())
    return sc, _mixed(sc, 1024, rng, (axis_rays, front_rays))


def tmax_around(bf, seed):
    """trace_golden.generate's tmax: half the brute-force closest t, exactly it, the next float up, twice it (a miss: anything)."""
    rng = np.random.default_rng(seed)
    n = len(bf)
    pick = rng.integers(0, 4, n)
    with np.errstate(over="ignore"):
        tmax = np.where(pick == 0, bf * np.float32(0.5), np.where(pick == 1, bf, np.where(pick == 2, np.nextafter(bf, np.float32(np.inf)),
                                                                                               bf * np.float32(2.0))))
    return np.where(bf >= FLT_MAX, rng.uniform(0.1, 100.0, n).astype(np.float32), tmax).astype(np.float32)


def case(cid):
    """Case `cid` with the oracle's answers: the rays and meta of build(), tmax, T.EXPECTED, near_tie and bf_t; "scene": the Scene."""
    if cid not in _BUILT:
        sc, rays = build(cid)
        n = len(rays["origins"])
        zero = np.zeros(n, np.float32)
        first = trace_golden.oracle_batch(sc.desc, rays["origins"], rays["directions"], zero, np.full(n, FLT_MAX, np.float32))
        out = dict(rays)
        out["tmax"] = tmax_around(first["bf_t"], 9000 + CASES.index(cid))
        out.update(trace_golden.oracle_batch(sc.desc, out["origins"], out["directions"], zero, out["tmax"]))
        out["scene"] = sc
        out["id"] = cid
        _BUILT[cid] = out
    return _BUILT[cid]


def as_fixture(c):
    """The case with the keys test_gpu_trace_rays.check_fixture reads off a fixture file."""
    n = len(c["origins"])
    out = {k: c[k] for k in T.RAYS + T.EXPECTED + ("near_tie",)}
    out.update(scene=np.array(c["id"]), ray_bias=np.zeros(n, np.float32), family=np.zeros(n, np.uint8))
    return out


def summary(c):
    """rays, hits, near ties, and the rays on which TraceRay's answer is not the brute-force closest hit (all / without a near tie)."""
    hit = c["group"] >= 0
    parts = np.where(hit, c["t"], FLT_MAX) != c["bf_t"]
    return {"rays": len(hit), "hits": int(hit.sum()), "near_ties": int(c["near_tie"].sum()), "parts": int(parts.sum()),
            "parts_no_tie": int((parts & (c["near_tie"] == 0)).sum()), "occluded_tmax": int(c["occluded_tmax"].sum())}
