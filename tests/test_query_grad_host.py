"""Gradients of closest-hit queries on the CPU.  par_raytracer_amd/csrc/dev_query_grad.h holds the reverse-mode step of one ray
and the fixed-point conversion as __host__ __device__ code, kernels_query_grad.h the three kernels; tests/query_grad_host_harness.cpp,
a stand-alone program built with g++ (and AddressSanitizer / UBSan, through tests/hip_shim), runs them lane by lane in the order of
prt_trace_rays_backward on the cases written here.  The yardstick for accuracy is torch CPU autograd of the same formulas in
float64 (tests/query_grad_cases.py); the gate, computed at run time, is err <= 4 * max(err of torch float32, 2^-22).  No GPU library
runs a kernel here."""
import numpy as np
import pytest

import query_grad_cases as Q
from query_grad_cases import bits

ALL = ("t", "bw", "position", "normal")
N = 2048


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("query_grad_host")
    exe = Q.build_harness(d, sanitize=True)
    return lambda cases: Q.run_harness(exe, cases, d)


@pytest.fixture(scope="module")
def meshes():
    return {"one_triangle": Q.one_triangle(), "cornell_box": Q.scene_mesh("cornell_box"), "icosphere_l3": Q.scene_mesh("icosphere_l3")}


def test_accuracy_against_float64_autograd(harness, meshes):
    """One triangle with one ray, cornell_box and icosphere_l3 with 2,048 recipe rays each; ray_bias 0 and 1e-3; directions scaled
    by 2.5; all four output gradients random, and one at a time."""
    cases, labels = [], []
    for si, (name, mesh) in enumerate(meshes.items()):
        n = 1 if name == "one_triangle" else N
        o, d, group, vertex0 = Q.recipe_rays(mesh, n, seed=100 + si)
        variants = [(0.0, 1.0, ALL), (1e-3, 2.5, ALL)] + [(1e-3, 1.0, (k,)) for k in ALL]
        for vi, (bias, scale, which) in enumerate(variants):
            dd = np.ascontiguousarray(d * np.float32(scale))
            cases.append(Q.case(mesh, o, dd, group, vertex0, bias, Q.random_grads(n, 7 * si + vi, which)))
            labels.append("%s bias %g scale %g grads %s" % (name, bias, scale, "+".join(which)))
    for c, r, label in zip(cases, harness(cases), labels):
        assert r["rc"] == 0 and r["hit_rays"] == len(c["group"]) and r["skipped_rays"] == 0, label
        Q.check_against_yardstick(c["mesh"], c["o"], c["d"], c["group"], c["vertex0"], c["ray_bias"], c["gout"], r, label)


def test_the_vertex_gradient_does_not_depend_on_the_order_of_the_rays(harness, meshes):
    mesh = meshes["icosphere_l3"]
    o, d, group, vertex0 = Q.recipe_rays(mesh, N, seed=3)
    g = Q.random_grads(N, 4)
    orders = [np.arange(N), np.arange(N)[::-1], np.random.default_rng(5).permutation(N)]
    cases = [Q.case(mesh, o[p], d[p], group[p], vertex0[p], 1e-3, {k: v[p] for k, v in g.items()}, merge) for merge in (False, True) for p in orders]
    res = harness(cases)
    assert np.abs(res[0]["positions"]).max() > 0
    for r, p in zip(res, orders * 2):
        assert r["rc"] == 0 and r["unit_exponent"] == res[0]["unit_exponent"] and bits(r["max_contribution"]) == bits(res[0]["max_contribution"])
        assert np.array_equal(bits(r["positions"]), bits(res[0]["positions"]))
        for k in ("origins", "directions"):
            assert np.array_equal(bits(r[k]), bits(res[0][k][p]))


def test_misses_nan_rays_and_empty_batches_give_zeros(harness, meshes):
    mesh = meshes["cornell_box"]
    n = 200
    o, d, group, vertex0 = Q.recipe_rays(mesh, n, seed=8)
    g = Q.random_grads(n, 9)
    miss, nan = np.arange(0, n, 5), np.arange(1, n, 7)
    group2, vertex2, o2 = group.copy(), vertex0.copy(), o.copy()
    group2[miss] = -1
    vertex2[miss] = 0xFFFFFFFF
    o2[nan, 1] = np.nan
    all_miss = np.full(n, -1, np.int32)
    z = np.zeros((0, 3), np.float32)
    res = harness([Q.case(mesh, o2, d, group2, vertex2, 0.0, g), Q.case(mesh, o, d, all_miss, vertex2, 0.0, g),
                   Q.case(mesh, z, z, np.zeros(0, np.int32), np.zeros(0, np.uint32), 0.0, {})])
    dead = np.union1d(miss, nan)
    r = res[0]
    n_skipped = len(np.setdiff1d(nan, miss))
    assert r["rc"] == 0 and r["skipped_rays"] == n_skipped and r["hit_rays"] == n - len(dead)
    assert np.all(r["origins"][dead] == 0) and np.all(r["directions"][dead] == 0) and np.all(r["contrib"][dead] == 0)
    live = np.setdiff1d(np.arange(n), dead)
    assert np.all(np.isfinite(r["positions"])) and np.all(np.any(r["origins"][live] != 0, axis=1))
    for r in res[1:]:
        assert r["rc"] == 0 and r["hit_rays"] == 0 and r["skipped_rays"] == 0 and r["unit_exponent"] == 0 and r["max_contribution"] == 0
        assert np.all(bits(r["positions"]) == 0) and np.all(bits(r["origins"]) == 0) and np.all(bits(r["directions"]) == 0)


def test_a_nan_vertex_skips_exactly_the_rays_on_its_triangles(harness, meshes):
    mesh = meshes["icosphere_l3"]
    p, idx, runs = mesh
    o, d, group, vertex0 = Q.recipe_rays(mesh, N, seed=11)
    g = Q.random_grads(N, 12)
    corner = runs[group, 0].astype(np.int64) + vertex0
    bad_vertex = int(idx[corner[17]])                            # a vertex some ray's triangle uses
    uses = np.any(np.stack([idx[corner + k] for k in range(3)], 1) == bad_vertex, axis=1)
    assert 0 < uses.sum() < N // 4
    p_nan = p.copy()
    p_nan[bad_vertex, 2] = np.nan
    group_removed, vertex_removed = group.copy(), vertex0.copy()
    group_removed[uses] = -1                                      # the same batch with those rays turned into misses: count stays
    vertex_removed[uses] = 0xFFFFFFFF
    a, b = harness([Q.case((p_nan, idx, runs), o, d, group, vertex0, 1e-3, g), Q.case(mesh, o, d, group_removed, vertex_removed, 1e-3, g)])
    assert a["rc"] == 0 and b["rc"] == 0
    assert a["skipped_rays"] == int(uses.sum()) and a["hit_rays"] == N - int(uses.sum()) == b["hit_rays"] and b["skipped_rays"] == 0
    assert a["unit_exponent"] == b["unit_exponent"]
    for k in Q.GRADS:
        assert np.array_equal(bits(a[k]), bits(b[k])), k
    assert np.all(a["origins"][uses] == 0) and np.all(a["directions"][uses] == 0)


@pytest.mark.parametrize("merge", [False, True])
def test_65_rays_on_one_triangle_sum_as_python_integers(harness, meshes, merge):
    mesh = meshes["one_triangle"]
    n = 65
    o, d, group, vertex0 = Q.recipe_rays(mesh, n, seed=21)
    r = harness([Q.case(mesh, o, d, group, vertex0, 1e-3, Q.random_grads(n, 22), merge)])[0]
    assert r["rc"] == 0 and r["hit_rays"] == n
    u = int(r["unit_exponent"])
    m = float(np.abs(r["contrib"]).max())
    assert np.float32(m) == r["max_contribution"]
    e = int(np.floor(np.log2(m))) + 1
    assert 2.0 ** (e - 1) <= m < 2.0 ** e and u == e + 8 - 62                 # 3 * 65 = 195 <= 2^8
    expect = np.zeros((3, 3), np.float32)
    for corner in range(3):
        for k in range(3):
            total = sum(round(float(c) * 2.0 ** -u) for c in r["contrib"][:, 3 * corner + k])     # exact scaling; round() ties to even
            assert abs(total) < 2 ** 62
            expect[corner, k] = np.float32(float(total) * 2.0 ** u)
    assert np.array_equal(bits(r["positions"]), bits(expect))


def test_invalid_references_are_refused_before_anything_is_written(harness, meshes):
    mesh = meshes["cornell_box"]
    p, idx, runs = mesh
    o, d, group, vertex0 = Q.recipe_rays(mesh, 64, seed=31)
    cases = []
    for ray, (g_bad, v_bad) in enumerate(((runs.shape[0], 0), (0, 1), (0, int(runs[0, 1])), (0, 0xFFFFFFFC))):
        g2, v2 = group.copy(), vertex0.copy()
        g2[ray], v2[ray] = g_bad, v_bad
        cases.append(Q.case(mesh, o, d, g2, v2, 0.0, Q.random_grads(64, 32)))
    for r in harness(cases):
        assert r["rc"] == -1 and r["invalid"] == 1


def test_the_library_refuses_null_handles_without_a_gpu():
    import ctypes as C
    from par_raytracer_amd import capi
    lib = capi.hip_lib()
    batch, gout, gin, info = capi.PrtRayBatch(), capi.PrtHitGrads(), capi.PrtQueryGrads(), capi.PrtGradInfo()
    assert lib.prt_trace_rays_backward(None, C.byref(batch), None, None, None, 0, C.byref(gout), C.byref(gin), C.byref(info)) == -1
    assert lib.prt_trace_rays_backward_device(None, None, None, None, None, 0, None, None, None) == -1
    assert "prt_trace_rays_backward" in capi.PRT_SYMBOLS and "prt_trace_rays_backward_device" in capi.PRT_SYMBOLS
    assert lib.prt_abi_version() == 5
    assert C.sizeof(capi.PrtHitGrads) == 32 and C.sizeof(capi.PrtQueryGrads) == 24 and C.sizeof(capi.PrtGradInfo) == 24
