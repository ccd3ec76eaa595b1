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


# ---- the shared cases of the GPU suite (tests/query_grad_cases.py), proven here before a device sees them

def both_merges_against_the_integer_sum(run, mesh, build):
    """build(merge) -> case.  The harness with and without the merge gives the same bits, the vertex gradient equals
    exact_integer_sum, rays that add nothing get zero origin and direction gradients.  Returns the merge-off result."""
    cases = [build(False), build(True)]
    off, on = run(cases)
    assert off["rc"] == 0 and on["rc"] == 0
    for k in Q.GRADS + ("contrib",):
        assert np.array_equal(bits(off[k]), bits(on[k])), k
    for k in ("hit_rays", "skipped_rays", "unit_exponent"):
        assert off[k] == on[k], k
    assert bits(off["max_contribution"]) == bits(on["max_contribution"])
    assert np.array_equal(bits(off["positions"]), bits(Q.exact_integer_sum(mesh, cases[0], off)))
    dead = ~np.any(off["contrib"] != 0, axis=1)
    assert int((~dead).sum()) == off["hit_rays"]
    assert np.all(bits(off["origins"][dead]) == 0) and np.all(bits(off["directions"][dead]) == 0)
    return cases[0], off


@pytest.mark.parametrize("name", ["cornell_box", "icosphere_l3"])
@pytest.mark.parametrize("layout", ["waves", "regular"])
def test_mixed_wave_layouts_sum_as_integers(harness, meshes, name, layout):
    mesh = meshes[name]
    build = (lambda m: Q.wave_layout_case(mesh, 200, m)) if layout == "waves" else (lambda m: Q.regular_case(mesh, merge=m))
    c, r = both_merges_against_the_integer_sum(harness, mesh, build)
    n = len(c["group"])
    assert n == Q.LAYOUT_RAYS == 2085 and n % 64 == 37
    assert (r["hit_rays"], r["skipped_rays"]) == (c["hit_rays"], c["skipped_rays"])
    assert 0 < c["hit_rays"] and 0 < c["skipped_rays"] and c["hit_rays"] + c["skipped_rays"] < n
    assert np.array_equal(np.any(r["contrib"] != 0, axis=1), c["contributing"])
    assert np.all(np.any(r["origins"][c["contributing"]] != 0, axis=1)) and np.abs(r["positions"]).max() > 0
    if layout == "waves":                                      # the layout is what its docstring says
        live = c["contributing"].reshape(-1)
        w = lambda k: live[64 * k:64 * k + 64]                                    # noqa: E731
        key = c["mesh"][2][np.maximum(c["group"], 0), 0].astype(np.int64) + c["vertex0"]
        assert not w(3).any() and list(np.nonzero(w(5))[0]) == [0] and list(np.nonzero(w(6))[0]) == [63]
        assert w(7).all() and len(set(key[64 * 7:64 * 8])) == 1
        assert w(8).all() and np.array_equal(key[64 * 8:64 * 9:2], key[64 * 8 + 1:64 * 9:2])
        if name == "icosphere_l3":
            assert len(set(key[64 * 8:64 * 9])) == 32
        k9 = key[64 * 9:64 * 10]
        assert w(9).all() and (k9 == k9[0]).sum() == 1 and all((k9 == k).sum() >= 3 for k in k9[1:])
        last, kl = w(32), key[64 * 32:]
        assert last.size == 37 and last[:32].all() and not last[32:].any()
        assert all((kl[:32] == k).sum() == 3 for k in kl[:30]) and all((kl[:32] == k).sum() == 1 for k in kl[30:32])


@pytest.mark.parametrize("name", ["cornell_box", "icosphere_l3"])
@pytest.mark.parametrize("exponent", Q.SCALED_EXPONENTS)
def test_fixed_point_extremes(harness, meshes, name, exponent):
    mesh = meshes[name]
    c, r = both_merges_against_the_integer_sum(harness, mesh, lambda m: Q.scaled_grads_case(mesh, exponent, m))
    n = len(c["group"])
    m = float(r["max_contribution"])
    print("%s 2^%d: M %.3g, unit exponent %d, hit %d, skipped %d, %d non-finite entries" % (
        name, exponent, m, r["unit_exponent"], r["hit_rays"], r["skipped_rays"], int((~np.isfinite(r["positions"])).sum())))
    assert r["hit_rays"] + r["skipped_rays"] == n and np.float32(np.abs(r["contrib"]).max()) == r["max_contribution"]
    if exponent == -140:
        assert 0 < m < 2.0 ** -126 and r["skipped_rays"] == 0 and r["unit_exponent"] < -149
        assert np.abs(r["positions"]).max() > 0
    if exponent == 100:
        assert r["unit_exponent"] > 0 and r["skipped_rays"] == 0
    if (exponent, name) in ((122, "icosphere_l3"), (124, "cornell_box")):
        assert 0 < r["skipped_rays"] < n
    if (exponent, name) == (124, "cornell_box"):              # finite contributions whose exact sum exceeds float32: +-inf
        assert np.all(np.isfinite(r["contrib"])) and np.isinf(r["positions"]).any() and not np.isnan(r["positions"]).any()


@pytest.fixture(scope="module")
def plain_harness(tmp_path_factory):
    """Without the sanitizers, for the half million rays of the batch that passes the capped grid on the device."""
    d = tmp_path_factory.mktemp("query_grad_host_plain")
    exe = Q.build_harness(d, sanitize=False)
    return lambda cases: Q.run_harness(exe, cases, d)


def test_a_repeated_ray_sums_to_count_times_its_integer(harness, plain_harness, meshes):
    """At 2,085 rays on the sanitized harness, and at 2 * 8 * 256 * 256 + 3 * 64 + 37 = 1,048,805 - the device suite's batch on a
    256-CU part - on the plain one."""
    mesh = meshes["cornell_box"]
    for run, count in ((harness, Q.LAYOUT_RAYS), (plain_harness, 2 * 8 * 256 * 256 + 3 * 64 + 37)):
        c, r = both_merges_against_the_integer_sum(run, mesh, lambda m: Q.repeated_ray_case(mesh, count, m))
        expect, top_bits = Q.repeated_ray_expectation(mesh, c, r)
        print("count %d: the largest accumulator has %d bits" % (count, top_bits))
        # the largest |q| is at least 2^(61 - L) and count > 2^L / 6, so the largest accumulator is at least 2^61 / 6 > 2^58
        assert r["hit_rays"] == count and 59 <= top_bits <= 62
        assert np.array_equal(bits(r["positions"]), bits(expect))
        assert np.all(bits(r["origins"]) == bits(r["origins"][0])) and np.all(bits(r["directions"]) == bits(r["directions"][0]))


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
