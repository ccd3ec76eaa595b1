"""Shared by tests/test_query_grad_host.py and tests/test_gpu_query_grad.py: meshes, the ray recipe, the accuracy yardstick (torch
CPU autograd of the hit arithmetic, in float64 and float32) and the runner of tests/query_grad_host_harness.cpp."""
from __future__ import annotations

import struct

import numpy as np

import harness

GRADS = ("positions", "origins", "directions")
FLOOR = 2.0 ** -22          # four float32 ulps of an array's largest entry


# ---- meshes: (positions (P, 3) f32, idx_positions u32, runs (G, 2) u32 = first_index, index_count per group)

def scene_mesh(name):
    from conftest import host_scene
    a = host_scene(name, 0).arrays()
    return (np.ascontiguousarray(a["positions"], np.float32), np.ascontiguousarray(a["idx_positions"], np.uint32),
            np.ascontiguousarray(a["groups"][:, :2], np.uint32))


def one_triangle():
    p = np.array([[0.25, -0.5, 1.0], [2.0, 0.125, 0.75], [0.5, 1.75, -0.25]], np.float32)
    return p, np.array([0, 1, 2], np.uint32), np.array([[0, 3]], np.uint32)


def quad(z=0.0):
    """Two triangles in the plane z, facing +z."""
    p = np.array([[-1, -1, z], [1, -1, z], [1, 1, z], [-1, 1, z]], np.float32)
    return p, np.array([0, 1, 2, 0, 2, 3], np.uint32), np.array([[0, 6]], np.uint32)


def flat_desc(mesh):
    """An api.FlatDesc of a bare mesh: one normal, one texture coordinate, one material, no lights, no sphere tree."""
    import ctypes as C
    from par_raytracer_amd import api, capi
    p, idx, runs = mesh
    groups = (capi.PrtGroup * len(runs))(*[capi.PrtGroup(int(f), int(c), 0) for f, c in runs])
    mat = capi.PrtMaterial()
    mat.alpha = 1.0
    mat.ambient_texture = mat.diffuse_texture = mat.specular_texture = mat.alpha_texture = mat.bump_texture = -1
    raw = lambda x: np.frombuffer(bytes(x), np.uint8).copy()                       # noqa: E731
    z32, zu8 = np.zeros(0, np.float32), np.zeros(0, np.uint8)
    return api.FlatDesc(dict(positions=p.reshape(-1), normals=np.array([0, 0, 1], np.float32), texcoords=np.zeros(2, np.float32), tangents=z32,
                             idx_positions=idx, idx_texcoords=np.zeros_like(idx), idx_normals=np.zeros_like(idx), groups=raw(groups),
                             materials=raw(mat), lights=zu8, spheres=zu8, sphere_group=np.zeros(0, np.int32),
                             texture_dims=np.zeros(0, np.uint32), texture_bytes=zu8))


# ---- the ray recipe

def recipe_rays(mesh, n, seed, triangles=None):
    """n rays, each aimed at a triangle of the mesh: barycentrics uniform in [0.1, 0.8] then normalised, direction
    -cos * normal + sin * tangent with cos uniform in [0.2, 1], origin = hit - d * 0.25 * sqrt(|cross(ab, ac)|).
    Returns origins, directions (unit), group, vertex0 of the targets."""
    p, idx, runs = mesh
    rng = np.random.default_rng(seed)
    n_tris = idx.size // 3
    tri = rng.integers(0, n_tris, n) if triangles is None else np.asarray(triangles)
    P = p.astype(np.float64)
    a, b, c = (P[idx[3 * tri + k]] for k in range(3))
    bw = rng.uniform(0.1, 0.8, (n, 3))
    bw /= bw.sum(1, keepdims=True)
    hit = bw[:, :1] * a + bw[:, 1:2] * b + bw[:, 2:] * c
    ab, ac = b - a, c - a
    cr = np.cross(ab, ac)
    area2 = np.linalg.norm(cr, axis=1, keepdims=True)
    nrm = cr / area2
    t1 = ab / np.linalg.norm(ab, axis=1, keepdims=True)
    t2 = np.cross(nrm, t1)
    phi = rng.uniform(0, 2 * np.pi, (n, 1))
    cos = rng.uniform(0.2, 1.0, (n, 1))
    d = -cos * nrm + np.sqrt(1 - cos * cos) * (np.cos(phi) * t1 + np.sin(phi) * t2)
    o = hit - d * 0.25 * np.sqrt(area2)
    first = runs[:, 0].astype(np.int64)
    group = (np.searchsorted(first, 3 * tri, side="right") - 1).astype(np.int32)
    vertex0 = (3 * tri - first[group]).astype(np.uint32)
    return (np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32), group, vertex0)


def random_grads(n, seed, which=("t", "bw", "position", "normal")):
    rng = np.random.default_rng(seed)
    full = dict(t=rng.standard_normal(n).astype(np.float32), bw=rng.standard_normal((n, 3)).astype(np.float32),
                position=rng.standard_normal((n, 3)).astype(np.float32), normal=rng.standard_normal((n, 3)).astype(np.float32))
    return {k: (full[k] if k in which else None) for k in full}


# ---- the yardstick

def yardstick(mesh, o, d, group, vertex0, ray_bias, gout, dtype):
    """torch CPU autograd of the hit arithmetic in `dtype` on the float32 inputs widened exactly; rays with group < 0 are left
    out.  Returns {positions, origins, directions} as float64 numpy arrays."""
    import torch
    p, idx, runs = mesh
    sel = np.nonzero(group >= 0)[0]
    corner = runs[group[sel], 0].astype(np.int64) + vertex0[sel].astype(np.int64)
    vi = [torch.from_numpy(idx[corner + k].astype(np.int64)) for k in range(3)]
    P = torch.tensor(p, dtype=dtype, requires_grad=True)
    O = torch.tensor(o, dtype=dtype, requires_grad=True)
    D = torch.tensor(d, dtype=dtype, requires_grad=True)
    s = torch.from_numpy(sel)
    oo, dd_ = O[s], D[s]
    a, b, c = P[vi[0]], P[vi[1]], P[vi[2]]
    ob = oo + dd_ * torch.tensor(float(np.float32(ray_bias)), dtype=dtype)
    ab, ac = b - a, c - a
    n = torch.cross(ab, ac, dim=1)
    qp = -dd_
    den = (qp * n).sum(1)
    ap = ob - a
    e = torch.cross(qp, ap, dim=1)
    t = (ap * n).sum(1) / den
    v = (ac * e).sum(1) / den
    w = -(ab * e).sum(1) / den
    bw = torch.stack((1 - v - w, v, w), 1)
    pos = ob + dd_ * t[:, None]
    nrm = n / n.norm(dim=1, keepdim=True)
    loss = torch.zeros((), dtype=dtype)
    for out, key in ((t, "t"), (bw, "bw"), (pos, "position"), (nrm, "normal")):
        if gout.get(key) is not None:
            loss = loss + (out * torch.tensor(gout[key][sel], dtype=dtype)).sum()
    if not loss.requires_grad:
        return {k: np.zeros(x.shape) for k, x in zip(GRADS, (p, o, d))}
    g = torch.autograd.grad(loss, (P, O, D), allow_unused=True)
    return {k: (np.zeros(x.shape) if gi is None else gi.double().numpy()) for k, gi, x in zip(GRADS, g, (p, o, d))}


def check_against_yardstick(mesh, o, d, group, vertex0, ray_bias, gout, ours, what=""):
    """err(X) = max |X - X64| / max |X64| per output array; the gate is err(ours) <= 4 * max(err(X32), 2^-22).  Returns the
    figures (name -> (err ours, err X32)) after asserting."""
    import torch
    x64 = yardstick(mesh, o, d, group, vertex0, ray_bias, gout, torch.float64)
    x32 = yardstick(mesh, o, d, group, vertex0, ray_bias, gout, torch.float32)
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


# ---- the host harness

def build_harness(directory, sanitize):
    return harness.build("query_grad_host_harness.cpp", directory, "query_grad_host", sanitize=sanitize)


def case(mesh, o, d, group, vertex0, ray_bias=0.0, gout=None, merge=False):
    return dict(mesh=mesh, o=o, d=d, group=group, vertex0=vertex0, ray_bias=ray_bias, gout=gout or {}, merge=merge)


def run_harness(exe, cases, directory):
    """Every case through the harness in one run; returns per case a dict: rc, hit_rays, skipped_rays, invalid, unit_exponent,
    max_contribution and - rc 0 - positions, origins, directions, contrib (n, 9)."""
    fin, fout = harness.case_files(directory, "cases.bin", "results.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for c in cases:
            p, idx, runs = c["mesh"]
            n = len(c["group"])
            keys = ("t", "bw", "position", "normal")
            flags = sum(1 << i for i, k in enumerate(keys) if c["gout"].get(k) is not None) | (16 if c["merge"] else 0)
            f.write(struct.pack("<5If", n, p.shape[0], idx.size, runs.shape[0], flags, c["ray_bias"]))
            harness.put(f, (c["o"], np.float32), (c["d"], np.float32), (c["group"], np.int32), (c["vertex0"], np.uint32), (p, np.float32),
                        (idx, np.uint32), (runs, np.uint32), *((c["gout"][k], np.float32) for k in keys if c["gout"].get(k) is not None))
    harness.run(exe, fin, fout, timeout=300)
    blob, out = harness.Reader.of_file(fout), []
    for c in cases:
        rc, hit, skipped, invalid, unit, m = blob.unpack("<iIIIif")
        r = dict(rc=rc, hit_rays=hit, skipped_rays=skipped, invalid=invalid, unit_exponent=unit, max_contribution=np.float32(m))
        if rc == 0:
            n, n_pos = len(c["group"]), c["mesh"][0].shape[0]
            for k, shape in (("positions", (n_pos, 3)), ("origins", (n, 3)), ("directions", (n, 3)), ("contrib", (n, 9))):
                r[k] = blob.take(np.prod(shape), np.float32, shape)
        out.append(r)
    blob.done()
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- cases for the wave merge, the capped grid and the fixed point, with a reference that shares nothing with the kernels' sum

WAVE = 64
LAYOUT_RAYS = 32 * WAVE + 37                     # 33 waves, the last one partial


def exact_integer_sum(mesh, case, result):
    """The vertex gradient from the harness's per-ray contributions and unit exponent alone: rint(contrib * 2^-u) as int64,
    scatter-added through idx_positions, float32(float64(acc) * 2^u).  Independent of the kernels' accumulation and merge."""
    p, idx, runs = mesh
    u = int(result["unit_exponent"])
    contrib = np.asarray(result["contrib"], np.float64)
    q = np.rint(np.ldexp(contrib, -u))                        # the scaling by a power of two is exact, rint rounds ties to even
    group = np.asarray(case["group"])
    sel = np.nonzero((group >= 0) & np.any(contrib != 0.0, axis=1))[0]
    corner = runs[group[sel], 0].astype(np.int64) + np.asarray(case["vertex0"])[sel].astype(np.int64)
    acc = np.zeros((p.shape[0], 3), np.int64)
    load = np.zeros((p.shape[0], 3), np.float64)              # sum of |q|: below 2^63 it proves that acc did not wrap
    for c in range(3):
        vi = idx[corner + c].astype(np.int64)
        for k in range(3):
            np.add.at(acc[:, k], vi, q[sel, 3 * c + k].astype(np.int64))
            np.add.at(load[:, k], vi, np.abs(q[sel, 3 * c + k]))
    assert load.max(initial=0.0) < 2.0 ** 63 and np.abs(acc).max(initial=0) < 2 ** 62
    with np.errstate(over="ignore"):
        return np.ldexp(acc.astype(np.float64), u).astype(np.float32)


def _case_with_dead_classes(mesh, o, d, group, vertex0, g, miss, back, nan, inf, merge):
    """Turns the masked rays into the four classes that add nothing and returns Q.case(...) with "hit_rays", "skipped_rays" and
    the masks "contributing", "skipped" from this bookkeeping.  A miss wins over the three skipped classes (the kernels look at the
    reference first)."""
    group[miss] = -1
    vertex0[miss] = 0xFFFFFFFF
    d[back] = -d[back]                                        # the reference stays: dd <= 0, the step refuses the ray
    o[nan, 1] = np.nan
    g["t"][inf] = np.inf
    skipped = (back | nan | inf) & ~miss
    contributing = ~miss & ~skipped
    c = case(mesh, o, d, group, vertex0, 1e-3, g, merge)
    c.update(hit_rays=int(contributing.sum()), skipped_rays=int(skipped.sum()), contributing=contributing, skipped=skipped)
    return c


def wave_layout_case(mesh, seed, merge):
    """LAYOUT_RAYS rays laid out by wave (64 consecutive rays) and lane for k_qgrad_scatter<true>.  Waves not named below: random
    triangles; ray i is a miss when i % 5 == 0, back-facing when i % 7 == 3, has a NaN origin when i % 11 == 5 and g_t = inf when
    i % 13 == 7 - the strides are coprime to 64, so the dead lanes move from wave to wave.  The named waves are clean except where
    said:
        3   64 misses                       5   lane 0 is the only live lane      6   lane 63 is the only live lane
        7   64 lanes on one triangle        8   lanes 2k, 2k + 1 on triangle k (mod the mesh's count: 32 pairs where it has 32)
        9   lane 0 alone on its triangle, the lanes after it in groups of three on others
        32  (37 lanes) ten groups of three, two lone lanes, then a miss, a back-facing, a NaN, an inf ray and a miss.
    Returns Q.case(...) with "hit_rays", "skipped_rays" and the masks "contributing", "skipped" from the builder's own bookkeeping."""
    p, idx, runs = mesh
    n, n_tris = LAYOUT_RAYS, idx.size // 3
    assert n_tris >= 12
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    wave, lane = i // WAVE, i % WAVE
    tri = rng.integers(0, n_tris, n)
    special = np.isin(wave, (3, 5, 6, 7, 8, 9, 32))
    miss, back, nan, inf = (~special & (i % m == r) for m, r in ((5, 0), (7, 3), (11, 5), (13, 7)))
    miss |= (wave == 3) | ((wave == 5) & (lane != 0)) | ((wave == 6) & (lane != 63))
    tri[wave == 7] = tri[7 * WAVE]
    tri[wave == 8] = (lane[wave == 8] // 2) % n_tris
    tri[wave == 9] = np.where(lane[wave == 9] == 0, 0, 1 + ((lane[wave == 9] - 1) // 3) % (n_tris - 1))
    last = lane[wave == 32]
    tri[wave == 32] = np.where(last < 30, last // 3, np.minimum(last, 31) - 20)      # groups on 0..9, lone lanes on 10 and 11
    for m, l in ((miss, 32), (back, 33), (nan, 34), (inf, 35), (miss, 36)):
        m[32 * WAVE + l] = True
    o, d, group, vertex0 = recipe_rays(mesh, n, seed + 1, triangles=tri)
    return _case_with_dead_classes(mesh, o, d, group, vertex0, random_grads(n, seed + 2), miss, back, nan, inf, merge)


def regular_case(mesh, seed=300, merge=False, n=LAYOUT_RAYS):
    """n recipe rays on random triangles; a miss every fifth ray and wave 3 entirely, the three skipped classes on strides 7, 11
    and 13 (as wave_layout_case's unnamed waves)."""
    i = np.arange(n)
    miss, back, nan, inf = (i % m == r for m, r in ((5, 0), (7, 3), (11, 5), (13, 7)))
    miss = miss | (i // WAVE == 3)
    o, d, group, vertex0 = recipe_rays(mesh, n, seed)
    return _case_with_dead_classes(mesh, o, d, group, vertex0, random_grads(n, seed + 1), miss, back, nan, inf, merge)


SCALED_EXPONENTS = (-140, 100, 122, 124)


def scaled_grads_case(mesh, exponent, merge=False):
    """LAYOUT_RAYS clean recipe rays whose four output gradients are standard normal times 2^exponent, rounded to float32 (at -140
    they are denormal floats).  -140: the largest contribution is a denormal float; +100: a positive unit exponent; +122, +124:
    part of the rays' contributions overflow float32 and are skipped - how many, the harness says."""
    n = LAYOUT_RAYS
    o, d, group, vertex0 = recipe_rays(mesh, n, 400)
    g = {k: np.ldexp(v.astype(np.float64), exponent).astype(np.float32) for k, v in random_grads(n, 401).items()}
    assert all(np.all(np.isfinite(v)) for v in g.values())
    return case(mesh, o, d, group, vertex0, 1e-3, g, merge)


def repeated_ray_case(mesh, count, merge=False):
    """One recipe ray and its output gradients, `count` times: every accumulator holds count times the ray's integer."""
    o, d, group, vertex0 = recipe_rays(mesh, 1, 500)
    g = random_grads(1, 501)
    rep = lambda a: np.ascontiguousarray(np.repeat(a, count, axis=0))          # noqa: E731
    return case(mesh, rep(o), rep(d), rep(group), rep(vertex0), 1e-3, {k: rep(v) for k, v in g.items()}, merge)


def repeated_ray_expectation(mesh, c, result):
    """count x q per corner component as Python integers, from the harness's contribution of ray 0 and its unit exponent."""
    p, idx, runs = mesh
    count, u = len(c["group"]), int(result["unit_exponent"])
    corner = int(runs[c["group"][0], 0]) + int(c["vertex0"][0])
    expect = np.zeros((p.shape[0], 3), np.float32)
    top = 0
    for cn in range(3):
        for k in range(3):
            total = count * int(np.rint(np.ldexp(np.float64(result["contrib"][0, 3 * cn + k]), -u)))
            top = max(top, abs(total))
            expect[idx[corner + cn], k] = np.float32(np.ldexp(np.float64(total), u))
    assert top < 2 ** 62
    return expect, top.bit_length()
