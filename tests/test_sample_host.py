"""The definition of prt_sample_surface and prt_sample_surface_backward on the host (tests/sample_host_harness.cpp: a brute force in
input order with the PRT_HD functions of csrc/dev_sample.h and csrc/dev_sample_grad.h, built here with g++): the selection at its
edges against Python integers, uniformity by area (Pearson's statistic, 16 seeds on three meshes), the barycentrics, the area
against float64, the scale sweep, degenerate and multi-group meshes, purity in `first`, the gradient against a float64 yardstick,
and the harness once under the address and undefined-behaviour sanitizers."""
from __future__ import annotations

import numpy as np
import pytest

import closest_cases as K
import sample_cases as M
import signed_cases as S

N_STAT = 1 << 18
STAT_SEEDS = tuple(range(1, 17))
STAT_MESHES = ("torus", "fan", "cube")


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("sample_host")


@pytest.fixture(scope="module")
def exe(workdir):
    return M.build_harness(workdir)


@pytest.fixture(scope="module")
def run(exe, workdir):
    def go(cases):
        return M.run_harness(exe, cases, workdir)
    return go


# ---- selection

def test_selection_at_its_edges(exe, workdir):
    """sample_pick on x = mulhi64(r0, T) against Python integers: zero weights at the front, in the middle and at the end with
    r0 = 0, 2^64 - 1 and the two values on either side of every boundary of x; one weight, which takes every r0; all weights
    zero, a miss; and a list of fixed-point size (weights near 2^42, T near 2^45)."""
    lists = [[0, 0, 5, 0, 3, 0], [7], [0, 0, 0], [2 ** 61], [1, 0, 2 ** 42, 3, 0, 0, 2 ** 42 - 1, 1], [1] * 9, [0, 1]]
    draws = []
    for w in lists:
        r = M.boundary_draws(w) if sum(w) else [0, 1, 2 ** 63, 2 ** 64 - 1]
        draws.append(sorted(set(r + [1, 2 ** 32, 2 ** 63, 2 ** 64 - 2])))
    assert len(draws[0]) >= 2 + 2 + 4                               # 0, 2^64 - 1 and both sides of the one inner boundary (x = 5)
    got = M.run_pick(exe, list(zip(lists, draws)), workdir)
    for w, r, g in zip(lists, draws, got):
        expect = [M.pick_by_integers(w, x) for x in r]
        assert list(g) == expect, (w, [hex(x) for x in r], list(g), expect)
        assert all(t < 0 or w[t] > 0 for t in g), "a zero weight was picked"
    assert set(got[0]) == {2, 4} and set(got[1]) == {0} and set(got[2]) == {-1}
    assert got[0][0] == 2 and got[0][-1] == 4                        # r0 = 0 and r0 = 2^64 - 1


# ---- uniform by area, barycentrics

@pytest.fixture(scope="module")
def statistics(exe, workdir):
    """(mesh name, seed) -> the figures of 2^18 samples: Pearson's statistic and its degrees of freedom, the smallest bw
    component, the largest |bw0 + bw1 + bw2 - 1|, the three means, the largest distance from the float64 triangle in units of
    2^-23 M."""
    out = {}
    for name in STAT_MESHES:
        mesh = S.mesh_of(name)
        a, b, c = M.triangle_corners64(mesh)
        for seed in STAT_SEEDS:
            res = M.run_harness(exe, [M.case(mesh, [M.request(seed, 0, N_STAT)])], workdir, tag="stat")[0]
            smp = res["samples"][0]
            t = K.input_triangle(mesh, smp["group"], smp["vertex0"])
            bw = smp["bw"].astype(np.float64)
            dist = K.yardstick(smp["point"], a[t], b[t], c[t])[0]
            big = np.maximum(np.abs(smp["point"]).max(1), np.maximum(np.abs(a[t]).max(1), np.maximum(np.abs(b[t]).max(1), np.abs(c[t]).max(1))))
            # the point is the barycentric combination of the float64 corners, too
            comb = bw[:, :1] * a[t] + bw[:, 1:2] * b[t] + bw[:, 2:] * c[t]
            stat, dof = M.pearson(mesh, smp, res["W"])
            out[name, seed] = dict(stat=stat, dof=dof, bw_min=float(smp["bw"].min()), sum_err=float(np.abs(bw.sum(1) - 1.0).max()),
                                   mean=bw.mean(0), units=float((dist / (2.0 ** -23 * big)).max()),
                                   comb_units=float((np.linalg.norm(comb - smp["point"], axis=1) / (2.0 ** -23 * big)).max()))
    return out


@pytest.mark.parametrize("name,dof,gate", [("torus", 575, 685.5), ("fan", 399, 492.0), ("cube", 11, 31.4)])
def test_uniform_by_area(statistics, name, dof, gate):
    """Pearson's statistic of the triangle counts of 2^18 samples against N W_t / T, seeds 1..16: every one below the 99.9 %
    quantile of chi-square by Wilson and Hilferty (685.5, 492.0, 31.4 for 575, 399 and 11 degrees of freedom)."""
    assert abs(M.wilson_hilferty(dof) - gate) < 0.05
    stats = [statistics[name, seed]["stat"] for seed in STAT_SEEDS]
    print("%s: Pearson's statistic over seeds 1..16: %.1f .. %.1f (gate %.1f, %d degrees of freedom)" % (name, min(stats), max(stats), gate, dof))
    for seed in STAT_SEEDS:
        assert statistics[name, seed]["dof"] == dof
        assert statistics[name, seed]["stat"] <= M.wilson_hilferty(dof), (name, seed, statistics[name, seed]["stat"])


@pytest.mark.parametrize("name", STAT_MESHES)
def test_barycentrics(statistics, name):
    """Over the same samples: every component >= 0, |bw0 + bw1 + bw2 - 1| <= 2^-22, every component's mean within 4 sigma of 1/3
    (sigma = sqrt(1 / (18 N)): the variance of a barycentric of a uniform point is 1/18), and the point on its float64 triangle
    within the distance limit of tests/test_closest_host.py."""
    from test_closest_host import LIMIT_UNITS
    sigma = np.sqrt(1.0 / (18.0 * N_STAT))
    worst_mean = worst_units = 0.0
    for seed in STAT_SEEDS:
        s = statistics[name, seed]
        assert s["bw_min"] >= 0.0, (name, seed)
        assert s["sum_err"] <= 2.0 ** -22, (name, seed, s["sum_err"])
        dev = np.abs(s["mean"] - 1.0 / 3.0).max() / sigma
        assert dev <= 4.0, (name, seed, s["mean"])
        assert s["units"] <= LIMIT_UNITS and s["comb_units"] <= LIMIT_UNITS, (name, seed, s["units"], s["comb_units"])
        worst_mean, worst_units = max(worst_mean, dev), max(worst_units, s["units"], s["comb_units"])
    print("%s: means within %.2f sigma of 1/3, points within %.3f units of 2^-23 M of their triangles (limit %.3f)" % (name, worst_mean, worst_units,
                                                                                                               LIMIT_UNITS))


# ---- area

def test_area_against_float64(run):
    """info.area against the float64 numpy area: relative error <= 2^-20 (float32 cross products of well-shaped triangles hold
    about 2^-22; the fixed point adds less: half a unit of 2^-(62 - L) of the largest weight per triangle)."""
    meshes = {"cube": S.cube(), "torus": S.torus(), "height_field(16, 2)": K.height_field(16, 2)}
    for (name, mesh), res in zip(meshes.items(), run([M.case(m) for m in meshes.values()])):
        truth = M.area64(mesh)
        err = abs(res["area"] - truth) / truth
        print("%s: area %.9g, float64 %.9g, relative error %.3g = 2^%.1f" % (name, res["area"], truth, err, np.log2(max(err, 1e-300))))
        assert err <= 2.0 ** -20, name
        assert res["live_triangles"] == mesh[1].size // 3
        assert res["area"] == 0.5 * res["total_weight"] * 2.0 ** res["unit_exponent"]
        assert res["total_weight"] == int(res["W"].astype(object).sum()) < 2 ** 62


# ---- scale

def test_scale_sweep(run):
    """closest_cases.scaled(mesh, e) over closest_cases.SWEEP_EXPONENTS: group, vertex0, bw, normal, total_weight and
    live_triangles are those of scale 1, point is 2^e times the point of scale 1, unit_exponent moves by 2e."""
    n = 4096
    for name in ("cube", "torus", "fan"):
        mesh = S.mesh_of(name)
        out = run([M.case(K.scaled(mesh, e), [M.request(5, 0, n)]) for e in K.SWEEP_EXPONENTS])
        base = out[K.SWEEP_EXPONENTS.index(0)]
        for e, res in zip(K.SWEEP_EXPONENTS, out):
            what = "%s x 2^%d" % (name, e)
            M.assert_same_bits(res["samples"][0], base["samples"][0], what, ("group", "vertex0", "bw", "normal"))
            assert res["total_weight"] == base["total_weight"] and res["live_triangles"] == base["live_triangles"], what
            assert np.array_equal(res["W"], base["W"]), what
            assert res["unit_exponent"] == base["unit_exponent"] + 2 * e, what
            assert np.array_equal(res["samples"][0]["point"].astype(np.float64), np.ldexp(base["samples"][0]["point"].astype(np.float64), e)), what


# ---- degenerates and order

def test_degenerates_are_never_drawn(run):
    """with_degenerates(cube): 256 zero-area triangles in group 0, the cube's 12 in group 1 and again, reversed, in group 2 - so 24
    triangles live, each cube triangle twice -, and no zero-area record is ever returned."""
    mesh = S.degenerate_cube()
    res = run([M.case(mesh, [M.request(3, 0, 1 << 16)])])[0]
    assert res["live_triangles"] == 2 * 12 and (res["W"] > 0).sum() == 24
    assert np.all(res["W"][:4 * K.DEGENERATE_PER_FORM] == 0)
    smp = res["samples"][0]
    assert set(np.unique(smp["group"])) == {1, 2}
    t = K.input_triangle(mesh, smp["group"], smp["vertex0"])
    assert np.all(res["W"][t] > 0) and len(np.unique(t)) == 24
    assert abs(res["area"] - 2 * 6.0) <= 12.0 * 2.0 ** -20


def test_multi_group_names_the_input_triangle(run):
    """multi_group(torus): the groups lie in the index buffer in the order 2, 0, 1.  Sample j's draws are those of the one-group
    torus with the same triangles in the same index-buffer order, so its (group, vertex0) must name the same index triple."""
    mesh = S.multi_group(S.torus())
    p, idx, runs = mesh
    flat = (p, idx, np.array([[0, idx.size]], np.uint32))
    multi, one = run([M.case(mesh, [M.request(9, 0, 1 << 14)]), M.case(flat, [M.request(9, 0, 1 << 14)])])
    assert np.array_equal(multi["W"], one["W"])
    t_multi = K.input_triangle(mesh, multi["samples"][0]["group"], multi["samples"][0]["vertex0"])
    t_one = K.input_triangle(flat, one["samples"][0]["group"], one["samples"][0]["vertex0"])
    assert np.array_equal(t_multi, t_one)
    assert set(np.unique(multi["samples"][0]["group"])) == {0, 1, 2}
    M.assert_same_bits(multi["samples"][0], one["samples"][0], "multi_group", ("point", "bw", "normal"))


def test_unreferenced_positions_and_a_repeated_corner(run):
    mesh = S.unreferenced_and_repeated()
    res = run([M.case(mesh, [M.request(4, 0, 1 << 14)])])[0]
    assert res["live_triangles"] == 12 and res["W"][12] == 0
    smp = res["samples"][0]
    assert np.all(smp["vertex0"] < 36) and np.all(smp["point"] >= 0) and np.all(smp["point"] <= 1)
    assert abs(res["area"] - 6.0) <= 6.0 * 2.0 ** -20


def test_a_triangle_of_2_to_the_minus_30_keeps_its_weight(run):
    mesh = M.size_ratio_mesh()
    res = run([M.case(mesh, [M.request(1, 0, 16)])])[0]
    assert res["live_triangles"] == 2 and res["W"][0] == res["W"][1] << 30 and res["W"][1] > 0
    print("weights of the 2^30 pair: %d and %d (unit 2^%d)" % (res["W"][0], res["W"][1], res["unit_exponent"]))


def test_no_area_is_a_miss(run):
    empty = (np.zeros((1, 3), np.float32), np.zeros(0, np.uint32), np.zeros((0, 2), np.uint32))
    for mesh in (M.all_degenerate(), empty):
        res = run([M.case(mesh, [M.request(1, 0, 65)])])[0]
        assert res["total_weight"] == 0 and res["live_triangles"] == 0 and res["area"] == 0.0 and res["unit_exponent"] == 0
        M.assert_all_miss(res["samples"][0], "no area")


# ---- purity

def test_samples_are_a_function_of_their_index(run):
    """Samples [first, first + count) equal rows first .. of a call from 0 - checked directly for the small values of `first`, and
    for the large ones by overlapping windows: the key's packing crosses its fields at 65,535 / 65,536 and at 2^32 - 1 / 2^32."""
    mesh = S.torus()
    requests = [M.request(11, 0, 65536 + 64)] + [M.request(11, f, 64) for f in M.FIRSTS] + [M.request(11, f - 32, 64) for f in M.FIRSTS[4:]]
    requests.append(M.request(12, 0, 64))
    res = run([M.case(mesh, requests)])[0]["samples"]
    base, other = res[0], res[-1]
    for k, f in enumerate(M.FIRSTS[:4]):
        M.assert_same_bits(res[1 + k], {key: base[key][f:f + 64] for key in M.FIELDS}, "first = %d" % f)
    for k, f in enumerate(M.FIRSTS[4:]):
        at, before = res[1 + 4 + k], res[1 + len(M.FIRSTS) + k]                  # [f, f + 64) and [f - 32, f + 32)
        M.assert_same_bits({key: before[key][32:] for key in M.FIELDS}, {key: at[key][:32] for key in M.FIELDS}, "first = %d" % f)
        assert not np.array_equal(at["bw"], base["bw"][:64])
    assert not np.array_equal(other["bw"], base["bw"][:64]), "the seed matters"
    assert len(np.unique(base["bw"][:, 1])) > 65000, "the samples differ from each other"


# ---- gradient

def forward(run, mesh, seed, n):
    return run([M.case(mesh, [M.request(seed, 0, n)])])[0]["samples"][0]


@pytest.mark.parametrize("name", ["torus", "fan"])
def test_gradient_against_the_float64_yardstick(run, name):
    mesh = S.mesh_of(name)
    n = 4096
    smp = forward(run, mesh, 21, n)
    gp, gn = M.random_grads(n, 22)
    calls = [M.grad_call(smp["group"], smp["vertex0"], smp["bw"], gp, gn), M.grad_call(smp["group"], smp["vertex0"], smp["bw"], gp, None),
             M.grad_call(smp["group"], smp["vertex0"], smp["bw"], None, gn)]
    for call, res, what in zip(calls, run([M.case(mesh, grads=calls)])[0]["grads"], ("point + normal", "point", "normal")):
        assert res["rc"] == 0 and res["hit"] == n and res["skipped"] == 0 and res["invalid"] == 0
        assert res["max_contribution"] > 0
        M.check_grad_against_yardstick(mesh, call, res["positions"], "%s, %s" % (name, what))


def test_gradient_bits_do_not_depend_on_the_order(run):
    """On the fan 200 triangles share the apex: its gradient - every vertex's - is the same bits under a permutation of the
    samples and with the wave merge on and off."""
    mesh = S.fan()
    n = 4096
    smp = forward(run, mesh, 31, n)
    gp, gn = M.random_grads(n, 32)
    perm = np.random.default_rng(33).permutation(n)
    calls = [M.grad_call(smp["group"], smp["vertex0"], smp["bw"], gp, gn, merge=False), M.grad_call(smp["group"], smp["vertex0"], smp["bw"], gp, gn, merge=True),
             M.grad_call(smp["group"][perm], smp["vertex0"][perm], smp["bw"][perm], gp[perm], gn[perm], merge=False),
             M.grad_call(smp["group"][perm], smp["vertex0"][perm], smp["bw"][perm], gp[perm], gn[perm], merge=True)]
    out = run([M.case(mesh, grads=calls)])[0]["grads"]
    apex_samples = (mesh[1].reshape(-1, 3)[K.input_triangle(mesh, smp["group"], smp["vertex0"])] == 0).any(1).sum()
    assert apex_samples > n // 4, "the apex is contended"
    for res in out[1:]:
        assert res["rc"] == 0 and np.array_equal(res["positions"].view(np.uint32), out[0]["positions"].view(np.uint32))
        assert (res["hit"], res["unit_exponent"], res["max_contribution"]) == (out[0]["hit"], out[0]["unit_exponent"], out[0]["max_contribution"])
    assert np.abs(out[0]["positions"][0]).max() > 0


def test_skipped_samples_and_refused_references(run):
    """The skipped classes - a miss, a NaN in gout, a zero-area reference together with a normal gradient - add nothing and are
    counted; an invalid reference refuses the call with nothing written."""
    mesh = S.degenerate_cube()
    n = 256
    smp = forward(run, mesh, 41, n)
    gp, gn = M.random_grads(n, 42)
    group, vertex0, bw = smp["group"].copy(), smp["vertex0"].copy(), smp["bw"].copy()
    miss, nan, flat = np.arange(0, 16), np.arange(16, 32), np.arange(32, 48)
    group[miss], vertex0[miss] = -1, 0xFFFFFFFF
    gp = gp.copy()
    gp[nan, 1] = np.nan
    group[flat], vertex0[flat] = 0, (3 * np.arange(len(flat))).astype(np.uint32)       # group 0: the zero-area triangles
    keep = np.setdiff1d(np.arange(n), np.concatenate([miss, nan, flat]))
    calls = [M.grad_call(group, vertex0, bw, gp, gn), M.grad_call(group[keep], vertex0[keep], bw[keep], gp[keep], gn[keep]),
             M.grad_call(group, vertex0, bw, gp, None)]
    bad = []
    for g, v in ((3, 0), (1, 1), (1, 36), (1, 0xFFFFFFFC)):            # group out of range, vertex0 not a multiple of 3, past the run
        gg, vv = group.copy(), vertex0.copy()
        gg[100], vv[100] = g, v
        bad.append(M.grad_call(gg, vv, bw, gp, gn))
    out = run([M.case(mesh, grads=calls + bad)])[0]["grads"]
    full, kept, point_only = out[:3]
    assert (full["rc"], full["hit"], full["skipped"], full["invalid"]) == (0, n - 48, 32, 0)
    assert np.array_equal(full["positions"].view(np.uint32), kept["positions"].view(np.uint32)), "the skipped samples added nothing"
    # without a normal gradient a zero-area reference has a gradient: g bw per corner
    assert (point_only["rc"], point_only["hit"], point_only["skipped"]) == (0, n - 32, 16)
    for res in out[3:]:
        assert res["rc"] == -1 and res["invalid"] == 1
        assert np.all(res["positions"] == M.SENTINEL), "a refused call wrote to its output"


def test_harness_under_the_sanitizers(workdir):
    exe = M.build_harness(workdir, sanitize=True)
    mesh = S.degenerate_cube()
    smp_case = M.case(mesh, [M.request(1, 2 ** 48 - 64, 64), M.request(2, 0, 1000)])
    res = M.run_harness(exe, [smp_case, M.case(M.all_degenerate(), [M.request(1, 0, 3)])], workdir, tag="san")
    smp = res[0]["samples"][1]
    gp, gn = M.random_grads(1000, 5)
    out = M.run_harness(exe, [M.case(mesh, grads=[M.grad_call(smp["group"], smp["vertex0"], smp["bw"], gp, gn, merge=m) for m in (False, True)])],
                        workdir, tag="san")[0]["grads"]
    assert out[0]["rc"] == 0 and np.array_equal(out[0]["positions"].view(np.uint32), out[1]["positions"].view(np.uint32))
    got = M.run_pick(exe, [([0, 0, 5, 0, 3, 0], M.boundary_draws([0, 0, 5, 0, 3, 0])), ([0, 0], [0, 2 ** 64 - 1])], workdir)
    assert set(got[0]) == {2, 4} and set(got[1]) == {-1}
