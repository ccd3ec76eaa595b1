"""Shared by tests/test_closest_grad_host.py and tests/test_gpu_closest_grad.py: the runner of tests/closest_grad_host_harness.cpp,
the forward references (the float32 brute force of tests/closest_host_harness.cpp), the accuracy yardstick (torch CPU autograd of
the per-region function of csrc/dev_closest_grad.h, in float64 and float32, each region's formula evaluated on that region's
points only) and the case builders both suites use (pure numpy, seeded)."""
from __future__ import annotations

import struct

import numpy as np

import closest_cases as C
import harness
import query_grad_cases as Q
from query_grad_cases import bits, flat_desc, one_triangle, scene_mesh       # noqa: F401  (re-exported)

GRADS = ("positions", "points")
GOUT_KEYS = ("dist2", "point", "bw")
FLOOR = Q.FLOOR             # 2^-22: four float32 ulps of an array's largest entry
WAVE = 64
LAYOUT_POINTS = 32 * WAVE + 37                   # 33 waves, the last one partial
GRID_PASS_POINTS = 2 * 8 * 256 * 256 + 3 * 64 + 37      # past one pass of the capped grid on a 256-CU part
SENTINEL = np.float32(7.5)                      # what the harness fills both output buffers with before the call
REGION_NAMES = ("vertex a", "vertex b", "edge ab", "vertex c", "edge ac", "edge bc", "interior")


# ---- the host harness

def build_harness(directory, sanitize):
    return harness.build("closest_grad_host_harness.cpp", directory, "closest_grad_host" + ("_san" if sanitize else ""), sanitize=sanitize)


def case(mesh, points, group, vertex0, gout=None, merge=False):
    return dict(mesh=mesh, points=np.ascontiguousarray(points, np.float32), group=np.ascontiguousarray(group, np.int32),
                vertex0=np.ascontiguousarray(vertex0, np.uint32), gout=gout or {}, merge=merge)


def run_harness(exe, cases, directory):
    """Every case through the harness in one run; returns per case a dict: rc, hit_rays, skipped_rays, invalid, unit_exponent,
    max_contribution, positions and points (the output buffers as the call left them: the sentinel SENTINEL everywhere after a
    refusal) and - rc 0 - contrib (n, 9), region (n,)."""
    fin, fout = harness.case_files(directory, "cg_cases.bin", "cg_results.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for c in cases:
            p, idx, runs = c["mesh"]
            n = len(c["group"])
            flags = sum(1 << i for i, k in enumerate(GOUT_KEYS) if c["gout"].get(k) is not None) | (16 if c["merge"] else 0)
            f.write(struct.pack("<5I", n, p.shape[0], idx.size, runs.shape[0], flags))
            harness.put(f, (c["points"], np.float32), (c["group"], np.int32), (c["vertex0"], np.uint32), (p, np.float32), (idx, np.uint32),
                        (runs, np.uint32), *((c["gout"][k], np.float32) for k in GOUT_KEYS if c["gout"].get(k) is not None))
    harness.run(exe, fin, fout, timeout=300)
    blob, out = harness.Reader.of_file(fout), []
    for c in cases:
        rc, hit, skipped, invalid, unit, m = blob.unpack("<iIIIif")
        r = dict(rc=rc, hit_rays=hit, skipped_rays=skipped, invalid=invalid, unit_exponent=unit, max_contribution=np.float32(m))
        n, n_pos = len(c["group"]), c["mesh"][0].shape[0]
        fields = (("positions", (n_pos, 3), np.float32), ("points", (n, 3), np.float32))       # written on a refusal too
        if rc == 0:
            fields += (("contrib", (n, 9), np.float32), ("region", (n,), np.int32))
        for k, shape, dt in fields:
            r[k] = blob.take(np.prod(shape), dt, shape)
        out.append(r)
    blob.done()
    return out


# ---- forward references: the float32 brute force over all triangles with closest_on_triangle and the tie rule

def forward_references(closest_exe, queries, directory):
    """queries: [(mesh, points)].  Returns per query the brute force's {dist2, point, bw, vertex0, group}."""
    res = C.run_harness(closest_exe, [C.case(mesh, pts) for mesh, pts in queries], directory)
    for r in res:
        assert r["mismatches"] == 0
    return [r["brute"] for r in res]


def random_grads(n, seed, which=GOUT_KEYS):
    rng = np.random.default_rng(seed)
    full = dict(dist2=rng.standard_normal(n).astype(np.float32), point=rng.standard_normal((n, 3)).astype(np.float32),
                bw=rng.standard_normal((n, 3)).astype(np.float32))
    return {k: (full[k] if k in which else None) for k in full}


def take(gout, sel):
    return {k: (None if v is None else np.ascontiguousarray(v[sel])) for k, v in gout.items()}


# ---- the yardstick

def yardstick(mesh, pts, group, vertex0, region, gout, dtype):
    """torch CPU autograd of the table of csrc/dev_closest_grad.h in `dtype` on the float32 inputs widened exactly, with every
    point's region fixed to `region`; each region's formula runs on that region's points only (a stacked "all branches, then
    gather" form puts 0 x inf = NaN into the gradient).  Points with group < 0 are left out.  Returns {positions, points} as
    float64 numpy arrays."""
    import torch
    p, idx, runs = mesh
    P = torch.tensor(p, dtype=dtype, requires_grad=True)
    X = torch.tensor(pts, dtype=dtype, requires_grad=True)
    dot = lambda x, y: (x * y).sum(1)              # noqa: E731
    loss = torch.zeros((), dtype=dtype)
    for r in range(7):
        sel = np.nonzero((group >= 0) & (region == r))[0]
        if sel.size == 0:
            continue
        corner = runs[group[sel], 0].astype(np.int64) + vertex0[sel].astype(np.int64)
        a, b, c = (P[torch.from_numpy(idx[corner + k].astype(np.int64))] for k in range(3))
        x = X[torch.from_numpy(sel)]
        ab, ac, ap = b - a, c - a, x - a
        bp, cp = ap - ab, ap - ac
        d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
        zero, one = torch.zeros_like(d1), torch.ones_like(d1)
        if r == 0:
            v, w = zero, zero
        elif r == 1:
            v, w = one, zero
        elif r == 2:
            v, w = d1 / (d1 - d3), zero
        elif r == 3:
            v, w = zero, one
        elif r == 4:
            v, w = zero, d2 / (d2 - d6)
        elif r == 5:
            w = (d4 - d3) / ((d4 - d3) + (d5 - d6))
            v = 1 - w
        else:
            vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
            v, w = vb / ((va + vb) + vc), vc / ((va + vb) + vc)
        q = (a + ab * v[:, None]) + ac * w[:, None]
        e = x - q
        outs = dict(dist2=dot(e, e), point=q, bw=torch.stack((1 - v - w, v, w), 1))
        for key in GOUT_KEYS:
            if gout.get(key) is not None:
                loss = loss + (outs[key] * torch.tensor(gout[key][sel], dtype=dtype)).sum()
    if not loss.requires_grad:
        return {k: np.zeros(x.shape) for k, x in zip(GRADS, (p, pts))}
    g = torch.autograd.grad(loss, (P, X), allow_unused=True)
    return {k: (np.zeros(x.shape) if gi is None else gi.double().numpy()) for k, gi, x in zip(GRADS, g, (p, pts))}


def check_against_yardstick(mesh, pts, group, vertex0, region, gout, ours, what=""):
    """err(X) = max |X - X64| / max |X64| per output array; the gate is err(ours) <= 4 * max(err(X32), 2^-22).  Returns the
    figures (name -> (err ours, err X32)) after asserting."""
    import torch
    x64 = yardstick(mesh, pts, group, vertex0, region, gout, torch.float64)
    x32 = yardstick(mesh, pts, group, vertex0, region, gout, torch.float32)
    figures = {}
    for k in GRADS:
        if k not in ours:
            continue
        scale = np.abs(x64[k]).max() if x64[k].size else 0.0
        got = np.asarray(ours[k], np.float64)
        if scale == 0.0:
            assert np.all(got == 0.0), "%s %s: the exact gradient is zero, ours is not" % (what, k)
            figures[k] = (0.0, 0.0)
            continue
        e_ours, e_32 = np.abs(got - x64[k]).max() / scale, np.abs(x32[k] - x64[k]).max() / scale
        figures[k] = (float(e_ours), float(e_32))
        print("%s %s: err ours %.3g, err torch float32 %.3g, gate %.3g" % (what, k, e_ours, e_32, 4 * max(e_32, FLOOR)))
    for k, (e_ours, e_32) in figures.items():
        assert e_ours <= 4 * max(e_32, FLOOR), "%s %s: err %.3g above 4 * max(%.3g, 2^-22)" % (what, k, e_ours, e_32)
    return figures


ACCURACY_VARIANTS = (GOUT_KEYS,) + tuple((k,) for k in GOUT_KEYS)
ACCURACY_GROUPS = (("near+box+on", (C.KIND_NEAR, C.KIND_BOX, C.KIND_ON)), ("far", (C.KIND_FAR,)))


def accuracy_cases(mesh, fixture_index, ref_of):
    """The accuracy cases of one fixture: closest_cases.recipe_points(mesh, 2048, 100 + fixture index), split into the groups
    NEAR + BOX + ON and FAR (a far point's gradient would otherwise set the array's scale and hide the rest), each with all three
    output gradients random and with one at a time.  ref_of(points) -> the forward references.  Returns [(label, case)]."""
    pts, kind = C.recipe_points(mesh, C.RECIPE_POINTS, 100 + fixture_index)
    ref = ref_of(pts)
    out = []
    for gi, (gname, kinds) in enumerate(ACCURACY_GROUPS):
        sel = np.nonzero(np.isin(kind, kinds))[0]
        for vi, which in enumerate(ACCURACY_VARIANTS):
            g = random_grads(len(sel), 1000 * fixture_index + 10 * gi + vi, which)
            out.append(("%s grads %s" % (gname, "+".join(which)), case(mesh, pts[sel], ref["group"][sel], ref["vertex0"][sel], g)))
    return out


# ---- points built for a triangle and a region

def reference_of(mesh, tri):
    """(group, vertex0) of the input triangles `tri`."""
    p, idx, runs = mesh
    first = runs[:, 0].astype(np.int64)
    tri = np.asarray(tri, np.int64)
    group = (np.searchsorted(first, 3 * tri, side="right") - 1).astype(np.int32)
    return group, (3 * tri - first[group]).astype(np.uint32)


def points_over(mesh, tri, seed):
    """One point per entry of `tri`: a barycentric point of that triangle (weights uniform in [0.1, 0.8], normalised) lifted along
    the normal by 0.05 to 0.25 x sqrt(|cross(ab, ac)|), either side.  It lies in the triangle's interior region; the reference
    names that triangle (which need not be the scene's nearest: the backward call differentiates the triangle it is given)."""
    p, idx, runs = mesh
    rng = np.random.default_rng(seed)
    tri = np.asarray(tri)
    P = p.astype(np.float64)
    a, b, c = (P[idx[3 * tri + k]] for k in range(3))
    bw = rng.uniform(0.1, 0.8, (len(tri), 3))
    bw /= bw.sum(1, keepdims=True)
    cr = np.cross(b - a, c - a)
    area2 = np.linalg.norm(cr, axis=1, keepdims=True)
    lift = rng.uniform(0.05, 0.25, (len(tri), 1)) * rng.choice([-1.0, 1.0], (len(tri), 1))
    pts = bw[:, :1] * a + bw[:, 1:2] * b + bw[:, 2:] * c + cr / area2 * lift * np.sqrt(area2)
    return np.ascontiguousarray(pts, np.float32)


def region_points(n):
    """n points around Q.one_triangle() that cycle through the seven regions: point i is built for region i % 7 from the triangle's
    own geometry in float64 - beyond a corner along the outward bisector, beyond an edge's middle stretch along the in-plane
    outward normal, or over the interior - with a seeded lift off the plane.  Returns (points, region built for)."""
    p, idx, runs = one_triangle()
    rng = np.random.default_rng(77)
    a, b, c = p.astype(np.float64)
    nrm = np.cross(b - a, c - a)
    nrm /= np.linalg.norm(nrm)
    centre = (a + b + c) / 3.0
    unit = lambda x: x / np.linalg.norm(x)                     # noqa: E731
    pts, want = [], []
    for i in range(n):
        r = i % 7
        s, lift = rng.uniform(0.2, 1.5), rng.uniform(-0.5, 0.5)
        if r in (0, 1, 3):
            corner = {0: a, 1: b, 3: c}[r]
            x = corner + unit(corner - centre) * s
        elif r in (2, 4, 5):
            e0, e1 = {2: (a, b), 4: (a, c), 5: (b, c)}[r]
            t = rng.uniform(0.2, 0.8)
            on = e0 + (e1 - e0) * t
            outward = np.cross(e1 - e0, nrm)
            outward = unit(outward) * (1.0 if np.dot(outward, on - centre) > 0 else -1.0)
            x = on + outward * s
        else:
            bw = rng.uniform(0.1, 0.8, 3)
            bw /= bw.sum()
            x = bw[0] * a + bw[1] * b + bw[2] * c
        pts.append(x + nrm * lift)
        want.append(r)
    return np.ascontiguousarray(pts, np.float32), np.array(want, np.int32)


# ---- cases for the wave merge, the capped grid and the fixed point, with a reference that shares nothing with the kernels' sum

exact_integer_sum = Q.exact_integer_sum          # reads mesh, case["group"], case["vertex0"], result["contrib"], result["unit_exponent"]


def _case_with_dead_classes(mesh, pts, group, vertex0, g, miss, nan, inf, merge):
    """Turns the masked points into the classes that add nothing - a miss, a NaN point, an infinite output gradient - and returns
    case(...) with "hit_rays", "skipped_rays" and the masks "contributing", "skipped" from this bookkeeping.  A miss wins over the
    skipped classes (the kernels look at the reference first)."""
    group[miss] = -1
    vertex0[miss] = 0xFFFFFFFF
    pts[nan, 1] = np.nan
    g["dist2"][inf] = np.inf
    skipped = (nan | inf) & ~miss
    contributing = ~miss & ~skipped
    c = case(mesh, pts, group, vertex0, g, merge)
    c.update(hit_rays=int(contributing.sum()), skipped_rays=int(skipped.sum()), contributing=contributing, skipped=skipped)
    return c


def wave_layout_case(mesh, seed, merge):
    """LAYOUT_POINTS points laid out by wave (64 consecutive points) and lane for k_cgrad_scatter<true>.  Waves not named below:
    random triangles; point i is a miss when i % 5 == 0, has a NaN component when i % 11 == 5 and g_dist2 = inf when i % 13 == 7 -
    the strides are coprime to 64, so the dead lanes move from wave to wave.  The named waves are clean except where said:
        3   64 misses                       5   lane 0 is the only live lane      6   lane 63 is the only live lane
        7   64 lanes on one triangle        8   lanes 2k, 2k + 1 on triangle k (mod the mesh's count: 32 pairs where it has 32)
        9   lane 0 alone on its triangle, the lanes after it in groups of three on others
        32  (37 lanes) ten groups of three, two lone lanes, then a miss, a NaN point, an inf gradient and two misses."""
    p, idx, runs = mesh
    n, n_tris = LAYOUT_POINTS, idx.size // 3
    assert n_tris >= 12
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    wave, lane = i // WAVE, i % WAVE
    tri = rng.integers(0, n_tris, n)
    special = np.isin(wave, (3, 5, 6, 7, 8, 9, 32))
    miss, nan, inf = (~special & (i % m == r) for m, r in ((5, 0), (11, 5), (13, 7)))
    miss |= (wave == 3) | ((wave == 5) & (lane != 0)) | ((wave == 6) & (lane != 63))
    tri[wave == 7] = tri[7 * WAVE]
    tri[wave == 8] = (lane[wave == 8] // 2) % n_tris
    tri[wave == 9] = np.where(lane[wave == 9] == 0, 0, 1 + ((lane[wave == 9] - 1) // 3) % (n_tris - 1))
    last = lane[wave == 32]
    tri[wave == 32] = np.where(last < 30, last // 3, np.minimum(last, 31) - 20)      # groups on 0..9, lone lanes on 10 and 11
    for m, l in ((miss, 32), (nan, 33), (inf, 34), (miss, 35), (miss, 36)):
        m[32 * WAVE + l] = True
    group, vertex0 = reference_of(mesh, tri)
    return _case_with_dead_classes(mesh, points_over(mesh, tri, seed + 1), group, vertex0, random_grads(n, seed + 2), miss, nan, inf, merge)


SCALED_EXPONENTS = (-140, 100, 124)


def scaled_grads_case(mesh, exponent, merge=False):
    """LAYOUT_POINTS clean points over random triangles whose three output gradients are standard normal times 2^exponent, rounded
    to float32 (at -140 they are denormal floats).  -140: the largest contribution is a denormal float; +100: a positive unit
    exponent; +124: finite contributions whose sum leaves float32."""
    n = LAYOUT_POINTS
    tri = np.random.default_rng(400).integers(0, mesh[1].size // 3, n)
    group, vertex0 = reference_of(mesh, tri)
    g = {k: np.ldexp(v.astype(np.float64), exponent).astype(np.float32) for k, v in random_grads(n, 401).items()}
    assert all(np.all(np.isfinite(v)) for v in g.values())
    return case(mesh, points_over(mesh, tri, 402), group, vertex0, g, merge)


def repeated_point_case(mesh, count, merge=False):
    """One point over a triangle and its output gradients, `count` times: every accumulator holds count times the point's integer."""
    tri = np.array([5])
    group, vertex0 = reference_of(mesh, tri)
    pts, g = points_over(mesh, tri, 500), random_grads(1, 501)
    rep = lambda a: np.ascontiguousarray(np.repeat(a, count, axis=0))          # noqa: E731
    return case(mesh, rep(pts), rep(group), rep(vertex0), {k: rep(v) for k, v in g.items()}, merge)


repeated_point_expectation = Q.repeated_ray_expectation      # count x q per corner component as Python integers
