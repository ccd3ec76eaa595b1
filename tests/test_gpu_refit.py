"""prt_update_geometry on the GPU: after an update every render and every query gives the BITS a fresh prt_upload_scene of the
moved scene gives (include/prt.h) - pixels, ray_count, shaded_hits and every hit field; only node_visits and
tri_tests may differ.  The fresh upload is the yardstick throughout; one test also holds the refitted scene against the CPU
oracle, and prt_debug_check_refit is the geometric proof that the refitted tree is conservative.

Scene A is one of the suite's small scenes; B is A with moved positions, written as OBJ and loaded again (so that B has its own
sphere hierarchy), with the precondition that the loader gives B the index buffers, groups, normals and lights of A.  The
reference of a comparison is always A's description with exactly the fields replaced that the update passes."""
from __future__ import annotations

import ctypes as C
import dataclasses
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, host_scene, load_golden, scene_dir

SCENES = ["cornell_box", "coincident", "icosphere_l3", "terrain_64", "textured_gallery"]
MOVES = {name: (["rigid"] if name == "coincident" else ["smooth"]) + ["flat", "scale1000"] for name in SCENES}
W, H, SPP, DEPTH = 48, 36, 2, 3
POOL, WAVEFRONT = 4, 2

_A, _B = {}, {}


def arrays_a(name):
    from par_raytracer_amd import api
    if name not in _A:
        _A[name] = api.desc_arrays(host_scene(name, 0).desc)
    return _A[name]


def _move(s, move):
    """(moved positions, camera position) of ObjScene s."""
    P = s.positions.astype(np.float32).copy()
    cam = np.array(s.camera_position, dtype=np.float32)
    lo, hi = P.min(0), P.max(0)
    ext = float((hi - lo).max())
    if move == "smooth":
        k = np.float32(2.0 * np.pi / ext)
        P = (P + np.float32(0.03 * ext) * np.sin(P[:, [1, 2, 0]] * k + np.float32(0.7))).astype(np.float32)
    elif move == "rigid":                                    # near ties survive a translation; the ranks decide them
        t = np.array([0.5, 0.25, -0.75], dtype=np.float32)
        P, cam = (P + t).astype(np.float32), cam + t
    elif move == "flat":                                     # the first group that is not flat already, onto its lowest y
        for g in s.groups:
            idx = np.unique(np.asarray(g.faces)[:, :, 0])
            if P[idx, 1].max() > P[idx, 1].min():
                P[idx, 1] = P[idx, 1].min()
                break
        else:
            raise AssertionError("no group to flatten")
    elif move == "scale1000":                                # the box pad changes with the extent
        P, cam = (P * np.float32(1000.0)).astype(np.float32), cam * np.float32(1000.0)
    else:
        raise KeyError(move)
    return P, cam


def moved(name, move):
    """B = scene `name` after `move`: {"positions", "spheres", "sphere_group", "camera", "host" (its HostScene)}; checked on the
    CPU: the loader gives B the topology, normals and lights of A and the moved positions bit for bit."""
    from par_raytracer_amd import api, scenes
    if (name, move) not in _B:
        s, _ = scene_dir(name)
        P, cam = _move(s, move)
        d = tempfile.mkdtemp(prefix="prt_refit_%s_%s_" % (name, move))
        scenes.write_obj(dataclasses.replace(s, positions=P), d, "scene.obj")
        hs = api.HostScene(d, "scene.obj", 0, s.camera_position)
        b, a = api.desc_arrays(hs.desc), arrays_a(name)
        for key in ("idx_positions", "idx_texcoords", "idx_normals", "groups", "normals", "texcoords", "materials", "lights"):
            assert np.array_equal(a[key], b[key]), (name, move, key)
        assert np.array_equal(b["positions"].view(np.uint32), P.reshape(-1).view(np.uint32)), (name, move)
        _B[(name, move)] = {"positions": b["positions"], "spheres": b["spheres"], "sphere_group": b["sphere_group"],
                            "camera": cam, "host": hs}
    return _B[(name, move)]


def flat_desc(name, **replace):
    """A's description with some arrays replaced (spheres=None: without a hierarchy)."""
    from par_raytracer_amd import api
    a = dict(arrays_a(name))
    for k, v in replace.items():
        a[k] = v
    if a.get("spheres") is None:
        a["spheres"], a["sphere_group"] = np.zeros(0, np.uint8), np.zeros(0, np.int32)
    return api.FlatDesc(a)


def camera(name, cam_pos, w=W, h=H):
    from par_raytracer_amd import api
    s, _ = scene_dir(name)
    return api.make_camera(s.fov, w, h, [float(v) for v in cam_pos], s.camera_facing)


def frames(r, cam, w=W, h=H, **kw):
    """{pipeline: (pixel bits, ray_count, shaded_hits)} of one small frame on both pipelines."""
    from par_raytracer_amd import api
    out = {}
    for pipe in (POOL, WAVEFRONT):
        p = api.default_params(pipeline=pipe, **(kw or dict(spp=SPP, seed=77, bounce_depth=DEPTH)))
        img, c = r.render(cam, p, w, h)
        assert c.pipeline == pipe
        out[pipe] = (img.view(np.uint32).copy(), c.ray_count, c.shaded_hits)
        if kw:
            break                                            # adaptive sampling runs on POOL only
    return out


def assert_same(got, exp, what):
    assert got.keys() == exp.keys()
    for pipe in got:
        assert got[pipe][1] == exp[pipe][1] and got[pipe][2] == exp[pipe][2], (what, pipe, "ray_count / shaded_hits", got[pipe][1:], exp[pipe][1:])
        bad = int(np.any(got[pipe][0] != exp[pipe][0], axis=1).sum())
        assert bad == 0, "%s, pipeline %d: %d of %d pixels differ from the fresh upload" % (what, pipe, bad, got[pipe][0].shape[0])


def make_renderer(builder="sah"):
    from par_raytracer_amd import api
    r = api.Renderer(0)
    if builder != "sah":
        r.set_option("BVH_BUILDER", builder)
    return r


def render_equality(name, builder):
    """Check 1 for one scene and builder: A uploaded once, then every move of the scene as an update - with B's own spheres and
    without -, each against a fresh upload of the same description.  Returns the number of frames compared."""
    ra, rb = make_renderer(builder), make_renderer(builder)
    n = 0
    try:
        ra.upload(host_scene(name, 0))
        for move in MOVES[name]:
            b = moved(name, move)
            cam = camera(name, b["camera"])
            for own_spheres in (True, False):
                sp = (b["spheres"], b["sphere_group"]) if own_spheres else (None, None)
                info = ra.update_geometry(b["positions"], spheres=sp[0], sphere_group=sp[1])
                assert info.levels >= 1 and info.node_count == ra.scene_info().bvh_node_count and info.device_ms > 0
                assert info.levels <= ra.scene_info().bvh_max_depth
                assert info.abs_max == np.abs(b["positions"][arrays_a(name)["idx_positions"].astype(np.int64)[:, None] * 3 + np.arange(3)]).max()
                fresh = flat_desc(name, positions=b["positions"], spheres=sp[0], sphere_group=sp[1])
                rb.upload(fresh)
                what = "%s %s %s spheres=%s" % (name, builder, move, own_spheres)
                assert_same(frames(ra, cam), frames(rb, cam), what)
                chk = ra.check_refit(fresh)
                assert chk["violations"] == 0 and chk["refs"] == ra.scene_info().triangle_count, (what, chk)
                n += 2
    finally:
        ra.close()
        rb.close()
    return n


@pytest.mark.gpu
@pytest.mark.parametrize("builder", ["sah", "lbvh"])
@pytest.mark.parametrize("name", SCENES)
def test_a_refitted_scene_renders_the_bits_of_a_fresh_upload(name, builder):
    assert render_equality(name, builder) == 4 * len(MOVES[name])


@pytest.mark.gpu
def test_adaptive_sampling_on_a_refitted_scene():
    g = load_golden("cornell_adaptive_4_16")
    name = str(g["scene"])
    b = moved(name, "smooth")
    ra, rb = make_renderer(), make_renderer()
    try:
        ra.upload(host_scene(name, 0))
        ra.update_geometry(b["positions"], spheres=b["spheres"], sphere_group=b["sphere_group"])
        rb.upload(flat_desc(name, positions=b["positions"], spheres=b["spheres"], sphere_group=b["sphere_group"]))
        kw = dict(spp=int(g["spp"]), seed=int(g["seed"]), bounce_depth=int(g["bounce_depth"]), max_spp=int(g["max_spp"]))
        cam = camera(name, b["camera"], 64, 48)
        assert_same(frames(ra, cam, 64, 48, **kw), frames(rb, cam, 64, 48, **kw), "adaptive")
    finally:
        ra.close()
        rb.close()


CHILD = r"""
import os, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, "tests")); sys.path.insert(0, os.path.join(%(root)r, "oracle"))
from test_gpu_refit import MOVES, render_equality, query_equality
from par_raytracer_amd import capi
lib = capi.hip_lib()
assert os.path.basename(lib._name) == "libprt_hip_bvh8.so" and not (lib.prt_build_flags() & capi.BUILD_BVH4)
for name in ("coincident", "icosphere_l3", "textured_gallery"):
    print(name, render_equality(name, "sah"), "frames equal", flush=True)
print("coincident", query_equality("coincident", "rigid"), "rays equal", flush=True)
print("bvh8 refit ok")
"""


@pytest.mark.gpu
def test_refit_on_the_8_wide_library():
    if not os.path.exists(os.path.join(ROOT, "par_raytracer_amd", "libprt_hip_bvh8.so")):
        pytest.skip("libprt_hip_bvh8.so not built (make hip-bvh8)")
    env = dict(os.environ)
    env["PRT_HIP_LIB"] = "libprt_hip_bvh8.so"
    out = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0 and b"bvh8 refit ok" in out.stdout, (out.returncode, out.stdout.decode()[-1500:], out.stderr.decode()[-3000:])


# ---- 2. queries ------------------------------------------------------------------------------------------------------------

CLOSEST = ("t", "bw", "vertex0", "group", "position", "normal")


def _queries(r, g, torch_path):
    """Every field of every ray of fixture g, closest and occluded (with and without tmax), as bit patterns."""
    o, d, tm = (np.ascontiguousarray(g[k]) for k in ("origins", "directions", "tmax"))
    if torch_path:
        import torch
        dev = torch.device("cuda", r.device_id)
        o, d, tm = (torch.from_numpy(x).to(dev) for x in (o, d, tm))
        back = lambda t: t.cpu().numpy()                                          # noqa: E731
    else:
        back = lambda a: a                                                        # noqa: E731
    bias = float(g["ray_bias"].max())
    res = r.trace_rays(o, d, ray_bias=bias)
    out = {k: np.ascontiguousarray(back(res[k])).view(np.uint32).copy() for k in CLOSEST}
    out["occluded"] = back(r.trace_rays(o, d, mode="occluded", ray_bias=bias)["occluded"]).copy()
    out["occluded_tmax"] = back(r.trace_rays(o, d, mode="occluded", tmax=tm, ray_bias=bias)["occluded"]).copy()
    return out


def query_equality(name, move, builder="sah"):
    g = np.load(os.path.join(GOLDEN, "trace_%s.npz" % name), allow_pickle=False)
    b = moved(name, move)
    ra, rb = make_renderer(builder), make_renderer(builder)
    try:
        ra.upload(host_scene(name, 0))
        before = _queries(ra, g, False)                          # builds q_leaf_map before the update (it depends on topology only)
        ra.update_geometry(b["positions"], spheres=b["spheres"], sphere_group=b["sphere_group"])
        rb.upload(flat_desc(name, positions=b["positions"], spheres=b["spheres"], sphere_group=b["sphere_group"]))
        for torch_path in (False, True):
            got, exp = _queries(ra, g, torch_path), _queries(rb, g, torch_path)
            for k in exp:
                bad = np.nonzero(np.any((got[k] != exp[k]).reshape(len(exp[k]), -1), axis=1))[0]
                assert bad.size == 0, "%s %s: field %s differs from the fresh upload on %d rays, first %d (torch %s)" % (
                    name, move, k, bad.size, bad[0], torch_path)
        hits = int((_queries(rb, g, False)["group"].view(np.int32) >= 0).sum())
        assert hits > 0 and any(np.any(before[k] != exp[k]) for k in CLOSEST), "the move was meant to change the hits"
        return len(g["origins"])
    finally:
        ra.close()
        rb.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,move", [("cornell_box", "smooth"), ("coincident", "rigid"), ("icosphere_l3", "smooth"), ("icosphere_l3", "scale1000")])
def test_queries_on_a_refitted_scene_equal_a_fresh_uploads(name, move):
    assert query_equality(name, move) > 0


@pytest.mark.gpu
def test_queries_on_a_refitted_lbvh_tree():
    assert query_equality("coincident", "rigid", "lbvh") > 0


# ---- 3. the CPU oracle on the moved scene ----------------------------------------------------------------------------------

@pytest.mark.gpu
def test_a_refitted_scene_matches_the_cpu_oracle_on_the_moved_scene():
    """B written as OBJ and loaded with HostScene IS a scene the oracle renders; the precondition - B's index arrays, groups,
    normals and lights equal A's, so that the update passes everything in which B differs - is asserted in moved()."""
    from par_raytracer_amd import api
    import oracle_py as orc
    name = "cornell_box"
    b = moved(name, "smooth")
    w, h, lattice = 96, 72, 3
    cam = camera(name, b["camera"], w, h)
    r = make_renderer()
    try:
        r.upload(host_scene(name, 0))
        r.update_geometry(b["positions"], spheres=b["spheres"], sphere_group=b["sphere_group"])
        for pipe in (POOL, WAVEFRONT):
            p = api.default_params(4, 1234, bounce_depth=DEPTH, pipeline=pipe)
            gpu, ctr = r.render_lattice(cam, p, w, h, lattice)
            cpu, octr = orc.render(b["host"].desc, cam, p, w, h, lattice=lattice, threads=4)
            assert ctr.ray_count == octr.ray_count
            assert float(np.abs(gpu[:, :, :3] - cpu[:, :, :3]).max()) <= 1e-4
    finally:
        r.close()


# ---- 4. conservativeness, composition --------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", ["icosphere_l3", "terrain_64"])
def test_updates_compose_and_the_tree_stays_conservative(name):
    a = arrays_a(name)
    b = moved(name, "smooth")
    s, _ = scene_dir(name)
    cam_a, cam_b = camera(name, s.camera_position), camera(name, b["camera"])
    r = make_renderer()
    try:
        r.upload(host_scene(name, 0))
        n = r.scene_info().triangle_count
        original = frames(r, cam_a)
        for _ in range(2):                                   # A -> B -> A -> B -> A
            r.update_geometry(b["positions"], spheres=b["spheres"], sphere_group=b["sphere_group"])
            chk = r.check_refit(flat_desc(name, positions=b["positions"]))
            assert chk["violations"] == 0 and chk["refs"] == n, chk
            assert r.check_refit(host_scene(name, 0))["violations"] > 0       # ... and it is B's tree now, not A's
            frames(r, cam_b)
            r.update_geometry(a["positions"], spheres=a["spheres"], sphere_group=a["sphere_group"])
            chk = r.check_refit(host_scene(name, 0))
            assert chk["violations"] == 0 and chk["refs"] == n, chk
            assert_same(frames(r, cam_a), original, name + " back to A")
    finally:
        r.close()


# ---- 5. normals and tangents, 6. the device entry point --------------------------------------------------------------------

def _turned(v, seed):
    """Unit vectors near the rows of flat xyz array v."""
    rng = np.random.default_rng(seed)
    x = v.reshape(-1, 3).astype(np.float64) + rng.normal(0.0, 0.15, (v.size // 3, 3))
    return np.ascontiguousarray((x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32).reshape(-1))


@pytest.mark.gpu
@pytest.mark.parametrize("name,torch_path", [("icosphere_l3", False), ("textured_gallery", False), ("textured_gallery", True)])
def test_new_normals_and_tangents_equal_a_fresh_upload_with_them(name, torch_path):
    a = arrays_a(name)
    b = moved(name, "smooth")
    nrm = _turned(a["normals"], 3)
    tan = _turned(a["tangents"], 4) if a["tangents"].size else None
    if name == "textured_gallery":
        assert tan is not None, "the gallery was meant to have bump maps"
    cam = camera(name, b["camera"])
    ra, rb = make_renderer(), make_renderer()
    try:
        ra.upload(host_scene(name, 0))
        keep = frames(ra, cam)
        args = [b["positions"], nrm, tan]
        if torch_path:
            import torch
            args = [None if x is None else torch.from_numpy(x).to(torch.device("cuda", ra.device_id)) for x in args]
        ra.update_geometry(args[0], normals=args[1], tangents=args[2])
        repl = dict(positions=b["positions"], normals=nrm, spheres=None)
        if tan is not None:
            repl["tangents"] = tan
        rb.upload(flat_desc(name, **repl))
        got, exp = frames(ra, cam), frames(rb, cam)
        assert_same(got, exp, name + " normals")
        assert any(np.any(got[p][0] != keep[p][0]) for p in got)
        # normals = None keeps them
        ra.update_geometry(arrays_a(name)["positions"])
        rb.upload(flat_desc(name, normals=nrm, spheres=None, **({"tangents": tan} if tan is not None else {})))
        s, _ = scene_dir(name)
        cam_a = camera(name, s.camera_position)
        assert_same(frames(ra, cam_a), frames(rb, cam_a), name + " normals kept")
    finally:
        ra.close()
        rb.close()


@pytest.mark.gpu
def test_torch_tensors_give_the_bits_numpy_arrays_give():
    import torch
    name = "terrain_64"
    b = moved(name, "smooth")
    cam = camera(name, b["camera"])
    ra, rb = make_renderer(), make_renderer()
    try:
        for r in (ra, rb):
            r.upload(host_scene(name, 0))
        i0 = ra.update_geometry(b["positions"], spheres=b["spheres"], sphere_group=b["sphere_group"])
        t = torch.from_numpy(b["positions"]).to(torch.device("cuda", rb.device_id)).reshape(-1, 3)
        i1 = rb.update_geometry(t, spheres=b["spheres"], sphere_group=b["sphere_group"])
        assert i0.abs_max == i1.abs_max and i0.levels == i1.levels
        assert_same(frames(rb, cam), frames(ra, cam), "device entry point")
    finally:
        ra.close()
        rb.close()


# ---- 7. errors -------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_refused_updates_write_nothing():
    from par_raytracer_amd import api, capi
    lib = capi.hip_lib()
    name = "icosphere_l3"
    a = arrays_a(name)
    s, _ = scene_dir(name)
    cam = camera(name, s.camera_position)
    r = make_renderer()
    try:
        good = np.ascontiguousarray(moved(name, "smooth")["positions"])
        n = good.size // 3

        def call(positions, count, entry=lib.prt_update_geometry):
            u = capi.PrtGeometryUpdate()
            u.positions, u.position_count = positions, count
            info = capi.PrtUpdateInfo()
            return entry(r._ctx, C.byref(u), C.byref(info))

        assert call(good.ctypes.data, n) == -2 and lib.prt_last_error(r._ctx)          # no scene
        r.upload(host_scene(name, 0))
        before = frames(r, cam)
        nan = good.copy()
        nan[3 * int(a["idx_positions"][5]) + 1] = np.nan
        huge = good.copy()
        huge[3 * int(a["idx_positions"][7])] = 2e18
        import torch
        nan_dev = torch.from_numpy(nan).cuda()
        for what, rc in (("count", call(good.ctypes.data, n - 1)), ("null positions", call(None, n)),
                         ("null update", lib.prt_update_geometry(r._ctx, None, None)),
                         ("nan", call(nan.ctypes.data, n)), ("1e18", call(huge.ctypes.data, n)),
                         ("nan, device", call(nan_dev.data_ptr(), n, lib.prt_update_geometry_device))):
            assert rc == -1, (what, rc)
            assert lib.prt_last_error(r._ctx).decode().startswith("prt_update_geometry"), what
            assert_same(frames(r, cam), before, "after a refused update (%s)" % what)
        # normals of the wrong count
        u = capi.PrtGeometryUpdate()
        u.positions, u.position_count, u.normals, u.normal_count = good.ctypes.data, n, good.ctypes.data, a["normals"].size // 3 + 1
        assert lib.prt_update_geometry(r._ctx, C.byref(u), None) == -1
        assert_same(frames(r, cam), before, "after a refused update (normal count)")
        assert lib.prt_update_geometry(None, C.byref(u), None) == -1
        # a scene of 0 triangles updates successfully (nothing references a position)
        empty = dict(a)
        for k in ("idx_positions", "idx_texcoords", "idx_normals"):
            empty[k] = np.zeros(0, np.uint32)
        empty["groups"], empty["spheres"], empty["sphere_group"] = np.zeros(0, np.uint8), np.zeros(0, np.uint8), np.zeros(0, np.int32)
        r.upload(api.FlatDesc(empty))
        assert r.scene_info().triangle_count == 0
        info = r.update_geometry(good)
        assert info.node_count == 1 and info.levels == 1
    finally:
        r.close()


# ---- 7b. more corners than one pass of k_refit_bounds' capped grid ----------------------------------------------------------

def triangle_soup(n_tris, seed):
    """n_tris small triangles, one per cell of a jittered square grid of unit cells, each owning its three vertices (so every
    vertex is exactly one corner of k_refit_bounds' loop); all face +z, none touches another.  A mesh of tests/query_grad_cases.py."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(n_tris)))
    cell = np.arange(n_tris)
    centre = np.stack([cell % side + 0.5, cell // side + 0.5, np.zeros(n_tris)], 1) + rng.uniform(-0.1, 0.1, (n_tris, 3))
    angle = rng.uniform(0, 2 * np.pi, n_tris)[:, None] + np.array([0.0, 2.1, 4.2])[None, :]          # counter-clockwise seen from +z
    radius = rng.uniform(0.15, 0.3, (n_tris, 3))
    corners = centre[:, None, :] + np.stack([radius * np.cos(angle), radius * np.sin(angle), rng.uniform(-0.05, 0.05, (n_tris, 3))], 2)
    p = np.ascontiguousarray(corners.reshape(-1, 3), np.float32)
    return p, np.arange(3 * n_tris, dtype=np.uint32), np.array([[0, 3 * n_tris]], np.uint32)


@pytest.mark.gpu
def test_a_soup_larger_than_one_pass_of_the_bounds_kernel():
    """update_geometry caps k_refit_bounds' grid at 8 * cu_count blocks of 256 lanes; this soup has one and a half times as many
    corners, plus 111.  Single-vertex probes spread over the index range - a third of them in the second pass - must each be seen
    by the reduction: 1e6 is the new abs_max, NaN refuses the update."""
    import time
    import torch
    import query_grad_cases as Q
    from par_raytracer_amd import capi
    lib = capi.hip_lib()
    # The context's own cu_count is not exported.  It starts as hipGetDeviceProperties' multiProcessorCount - the figure torch
    # reports - and PRT_RESERVE_CUS can only lower it, which makes a pass shorter: the second pass is reached either way.
    assert not os.environ.get("PRT_RESERVE_CUS")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    one_pass = 8 * cus * 256
    T = one_pass // 2 + 37
    assert one_pass < 3 * T < 2 * one_pass and (3 * T) % 64 != 0
    t0 = time.perf_counter()
    mesh = triangle_soup(T, 7)
    p, idx, runs = mesh
    ext = float(p.max())
    k = np.float32(2.0 * np.pi / ext)
    moved_p = np.ascontiguousarray((p + np.float32(0.02 * ext) * np.sin(p[:, [1, 2, 0]] * k + np.float32(0.7))).astype(np.float32))
    moved_mesh = (moved_p, idx, runs)
    rng = np.random.default_rng(9)
    target = rng.integers(0, T, 4096)
    o, d, _, _ = Q.recipe_rays(moved_mesh, 4096, 8, triangles=target)
    a, b, c = (moved_p[3 * target + j].astype(np.float64) for j in range(3))
    reach = 0.25 * np.sqrt(np.linalg.norm(np.cross(b - a, c - a), axis=1))       # the recipe's distance to its target: tmax on both sides of it
    g = {"origins": o, "directions": d, "tmax": (reach * rng.uniform(0.25, 2.0, 4096)).astype(np.float32), "ray_bias": np.zeros(4096, np.float32)}
    ra, rb = make_renderer("lbvh"), make_renderer("lbvh")
    try:
        ra.upload(Q.flat_desc(mesh))
        assert ra.scene_info().triangle_count == T
        before = _queries(ra, g, False)
        t1 = time.perf_counter()
        info = ra.update_geometry(moved_p)
        assert info.abs_max == np.abs(moved_p).max()
        fresh = Q.flat_desc(moved_mesh)
        rb.upload(fresh)
        chk = ra.check_refit(fresh)
        assert chk["violations"] == 0 and chk["refs"] == T, chk
        t2 = time.perf_counter()
        got, exp = _queries(ra, g, False), _queries(rb, g, False)
        for key in exp:
            assert np.array_equal(got[key], exp[key]), key
        hits = int((exp["group"].view(np.int32) >= 0).sum())
        assert hits >= 0.9 * 4096 and 0 < exp["occluded_tmax"].sum() < exp["occluded"].sum()
        assert any(np.any(before[key] != exp[key]) for key in CLOSEST), "the move was meant to change the hits"

        def refused(positions):
            u = capi.PrtGeometryUpdate()
            u.positions, u.position_count = positions.ctypes.data, positions.size // 3
            return lib.prt_update_geometry(ra._ctx, C.byref(u), None)

        # k_refit_bounds walks the leaf slots of the LBVH tree, not the vertex index: which probes fall into the second pass (slots
        # from one_pass / 3 on, the last third) depends on the builder's order, which no call exports, so the test cannot name
        # them.  The tree is built over Morton codes of the grid; vertices spread evenly over the row-major index cover every
        # row of it, and only a builder that put all 32 into the first two thirds of its order would hide a dropped pass.
        t3 = time.perf_counter()
        for vertex in np.linspace(0, 3 * T - 1, 32).astype(np.int64):
            probe = moved_p.copy()
            probe[vertex, 2] = 1e6
            assert ra.update_geometry(probe).abs_max == np.float32(1e6), vertex
            kept = _queries(ra, g, False)
            probe[vertex, 2] = np.nan
            assert refused(probe) == -1, vertex
            assert lib.prt_last_error(ra._ctx).decode().startswith("prt_update_geometry"), vertex
            after = _queries(ra, g, False)
            for key in kept:
                assert np.array_equal(after[key], kept[key]), (vertex, key)
        t4 = time.perf_counter()
        print("CUs %d, T %d, %d corners; soup, upload and first queries %.2f s, update, fresh upload and check %.2f s, "
              "queries %.2f s, 32 probes %.2f s" % (cus, T, 3 * T, t1 - t0, t2 - t1, t3 - t2, t4 - t3))
    finally:
        ra.close()
        rb.close()


# ---- 8. several devices behind one handle ----------------------------------------------------------------------------------

@pytest.mark.gpu
def test_multi_update_reaches_every_device_and_every_lane():
    from par_raytracer_amd import api, capi
    lib = capi.hip_lib()
    name = "coincident"
    b = moved(name, "rigid")
    cam = camera(name, b["camera"], 48, 40)
    p = api.default_params(SPP, 77, bounce_depth=DEPTH)
    rb = make_renderer()
    m = lib.prt_multi_create((C.c_int * 2)(0, 0), 2)
    assert m
    try:
        rb.upload(flat_desc(name, positions=b["positions"], spheres=b["spheres"], sphere_group=b["sphere_group"]))
        fresh, cf = rb.render(cam, p, 48, 40)
        assert lib.prt_multi_upload_scene(m, host_scene(name, 0).desc) == 0
        assert lib.prt_multi_depth(m) >= 2
        warm = np.empty((48 * 40, 4), np.float32)              # both lanes render A first (their workspaces and tables exist)
        for _ in range(2):
            assert lib.prt_multi_render(m, C.byref(cam), C.byref(p), 48, 40, warm.ctypes.data_as(C.c_void_p), None) == 0
        assert not np.array_equal(warm.view(np.uint32), fresh.view(np.uint32))
        pos = np.ascontiguousarray(b["positions"])
        sp, sg = np.ascontiguousarray(b["spheres"]), np.ascontiguousarray(b["sphere_group"])
        u = capi.PrtGeometryUpdate()
        u.positions, u.position_count = pos.ctypes.data, pos.size // 3
        u.spheres, u.sphere_group, u.sphere_count = sp.ctypes.data_as(C.POINTER(capi.PrtBSphere)), sg.ctypes.data_as(C.POINTER(C.c_int32)), sg.size
        assert lib.prt_multi_update_geometry(m, C.byref(u)) == 0, lib.prt_multi_last_error(m)
        out = [np.empty((48 * 40, 4), np.float32) for _ in range(2)]
        tickets = [C.c_uint64(0), C.c_uint64(0)]
        ctr = capi.PrtCounters()
        for k in range(2):                                    # two frames in flight: one per lane
            assert lib.prt_multi_submit(m, C.byref(cam), C.byref(p), 48, 40, out[k].ctypes.data_as(C.c_void_p), C.byref(tickets[k])) == 0
        assert lib.prt_multi_update_geometry(m, C.byref(u)) == -11        # refused while a ticket is open
        assert b"in flight" in lib.prt_multi_last_error(m)
        for k in range(2):
            assert lib.prt_multi_wait(m, tickets[k], C.byref(ctr)) == 0, lib.prt_multi_last_error(m)
            assert ctr.ray_count == cf.ray_count and ctr.shaded_hits == cf.shaded_hits
            assert np.array_equal(out[k].view(np.uint32), fresh.view(np.uint32)), "lane of frame %d" % k
    finally:
        lib.prt_multi_destroy(m)
        rb.close()


# ---- 9. queries and renders around an update -------------------------------------------------------------------------------

@pytest.mark.gpu
def test_queries_before_and_after_an_update_leave_renders_alone():
    name = "cornell_box"
    g = np.load(os.path.join(GOLDEN, "trace_%s.npz" % name), allow_pickle=False)
    b = moved(name, "smooth")
    cam = camera(name, b["camera"])
    ra, rb = make_renderer(), make_renderer()
    try:
        ra.upload(host_scene(name, 0))
        q0 = _queries(ra, g, False)                              # q_leaf_map is built here, before the update
        ra.update_geometry(b["positions"], spheres=b["spheres"], sphere_group=b["sphere_group"])
        rb.upload(flat_desc(name, positions=b["positions"], spheres=b["spheres"], sphere_group=b["sphere_group"]))
        f0 = frames(ra, cam)
        q1, qb = _queries(ra, g, False), _queries(rb, g, False)
        for k in qb:
            assert np.array_equal(q1[k], qb[k]), k
        assert_same(frames(ra, cam), f0, "render after queries")
        assert_same(f0, frames(rb, cam), "render of the refitted scene")
    finally:
        ra.close()
        rb.close()
