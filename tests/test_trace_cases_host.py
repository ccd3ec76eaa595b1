"""The case builders of tests/trace_cases.py without a GPU: the batches are what tests/test_gpu_trace_rays_schedules.py relies on
(class sizes, uniform runs, a replay list longer than k_query_exact's grid), and their expected rows reproduce bit for bit from
the CPU oracle's TraceRay and brute force (tests/trace_oracle_harness.cpp) - the fixture's rows in another order are still the
oracle's answers, and the tmax specials mean what include/prt.h says."""
from __future__ import annotations

import numpy as np
import pytest

import trace_cases as T
import trace_golden
from conftest import host_scene

PER = 192
SORTED_SCENES = {"coincident": T.CLASSES, "icosphere_l3": ("replay", "plain_hit", "miss")}


@pytest.fixture(scope="module")
def oracle():
    """oracle(name, case) -> the harness's answers for the case's rays and tmax."""
    def run(name, case):
        n = len(case["origins"])
        return trace_golden.oracle_batch(host_scene(name, 0).desc, case["origins"], case["directions"], np.zeros(n, np.float32), case["tmax"])
    return run


def assert_rows_are_the_oracles(case, out, what):
    for k in T.EXPECTED:
        bad = T.differing(out[k], case[k])
        assert bad.size == 0, (what, k, bad.size, bad[:4])


@pytest.mark.parametrize("name", T.FIXTURES)
def test_classes_partition_the_bias_0_rays(name):
    g = T.fixture(name)
    cls = T.classes(g)
    sel = T.bias0(g)
    assert len(sel) == T.BIAS0_RAYS
    assert np.array_equal(np.sort(np.concatenate(list(cls.values()))), sel)
    sizes = {k: len(v) for k, v in cls.items()}
    print(name, sizes)
    assert sizes["rest"] < 0.01 * len(sel), sizes
    assert sizes["replay"] >= 700                            # 731 without margins
    for c in SORTED_SCENES.get(name, ()):
        assert sizes[c] >= PER, (c, sizes)
    if name == "icosphere_l3":
        assert sizes["near_tie"] < PER                      # why it takes part without that class
    # the classes are what their names say
    d = g["directions"].astype(np.float64)
    off = np.abs((d * d).sum(1) - 1.0)
    far = g["family"] == list(g["family_names"]).index("far")
    assert np.all(far[cls["replay"]] | (off[cls["replay"]] > 2.0 ** -18))
    for c in ("near_tie", "plain_hit", "miss"):
        assert np.all(~far[cls[c]] & (off[cls[c]] < 2.0 ** -18)), c
    assert np.all(g["near_tie"][cls["near_tie"]] == 1) and np.all(g["near_tie"][cls["plain_hit"]] == 0)
    assert np.all(g["group"][cls["plain_hit"]] >= 0) and np.all(g["group"][cls["miss"]] == -1) and np.all(g["near_tie"][cls["miss"]] == 0)


@pytest.mark.parametrize("name", sorted(SORTED_SCENES))
def test_sorted_by_kind_has_uniform_runs_and_the_oracles_rows(name, oracle):
    g = T.fixture(name)
    case = T.sorted_by_kind(g, PER)
    kinds = SORTED_SCENES[name] + (T.INVALID,)
    n = PER * len(kinds)
    assert all(len(case[k]) == n for k in T.RAYS + T.EXPECTED + ("kind", "index"))
    assert np.array_equal(case["kind"], np.repeat(np.array(kinds), PER))          # runs of exactly PER, in this order
    assert PER % 64 == 0 and PER > 128 and PER % 128 != 0                         # whole waves, whole default chunks, boundaries inside one
    cls = T.classes(g)
    for i, c in enumerate(SORTED_SCENES[name]):
        run = case["index"][i * PER:(i + 1) * PER]
        assert np.all(np.isin(run, cls[c])) and len(np.unique(run)) == PER
    valid = np.nonzero(case["kind"] != T.INVALID)[0]
    for k in T.RAYS + T.EXPECTED:                                                 # the valid part: rows of the fixture, untouched
        assert np.array_equal(T.bits(case[k][valid]), T.bits(g[k][case["index"][valid]])), k
    assert np.all(g["ray_bias"][case["index"][valid]] == 0)
    # invalid rays: each of the four ways, and the documented miss
    inv = T.take(case, np.nonzero(case["kind"] == T.INVALID)[0])
    o, d = inv["origins"], inv["directions"]
    ways = [np.isnan(o).any(1), np.isposinf(d).any(1), (d == 0).all(1), np.isneginf(o).any(1)]
    assert all(int(w.sum()) == PER // 4 for w in ways) and np.all(np.sum(ways, axis=0) == 1)
    assert np.all(inv["t"] == T.FLT_MAX) and np.all(inv["group"] == -1) and np.all(inv["vertex0"] == 0xFFFFFFFF)
    assert not inv["bw"].any() and not inv["position"].any() and not inv["normal"].any()
    assert not inv["occluded"].any() and not inv["occluded_tmax"].any()
    # the oracle harness gives these rows for this batch, invalid rays included, and for a shuffle of it
    assert_rows_are_the_oracles(case, oracle(name, case), name + " sorted by kind")
    shuffled = T.take(case, np.random.default_rng(3).permutation(n))
    assert_rows_are_the_oracles(shuffled, oracle(name, shuffled), name + " shuffled")


@pytest.mark.parametrize("name", T.FIXTURES)
def test_tiled_rows_are_the_oracles(name, oracle):
    g = T.fixture(name)
    case = T.tiled(g, 5000)
    sel = T.bias0(g)
    assert len(case["origins"]) == 5000 and np.array_equal(case["index"], sel[np.arange(5000) % len(sel)])
    assert_rows_are_the_oracles(case, oracle(name, case), name + " tiled")


def test_the_long_list_is_longer_than_the_exact_kernels_grid():
    """Device test (d): tiled(cornell_box, 24 x 2300) lists more rays than k_query_exact has lanes (64 blocks of 256)."""
    g = T.fixture("cornell_box")
    case = T.tiled(g, 24 * T.BIAS0_RAYS)
    listed = int(np.isin(case["index"], T.classes(g)["replay"]).sum())
    print("replay rays:", listed)
    assert listed == 24 * len(T.classes(g)["replay"]) and listed > 64 * 256


@pytest.mark.parametrize("name", ["coincident", "icosphere_l3"])
def test_tmax_specials_mean_what_the_header_says(name, oracle):
    g = T.fixture(name)
    rays = T.tmax_specials(g)
    n = len(rays["origins"])
    assert n == 1024 and np.array_equal(rays["index"], T.bias0(g)[:n])
    lane, tm = rays["lane"], rays["tmax"]
    assert np.all(np.isposinf(tm[lane == 1])) and np.all(tm[lane == 2] == 0) and np.all(tm[lane == 3] == -1) and np.all(np.isnan(tm[lane == 4]))
    assert np.all(np.isneginf(tm[lane == 5])) and np.all(tm[lane == 6] == T.FLT_MAX)
    plain = (lane == 0) | (lane == 7)
    assert np.array_equal(T.bits(tm[plain]), T.bits(g["tmax"][rays["index"]][plain]))
    case = T.expect_from_oracle(rays, host_scene(name, 0).desc)
    fx = T.rows(g, rays["index"])
    for k in T.CLOSEST + ("occluded",):                       # tmax touches neither CLOSEST nor the no-limit answer
        assert T.differing(case[k], fx[k]).size == 0, k
    occ = case["occluded_tmax"]
    no_limit = (lane == 1) | (lane == 6)
    assert np.array_equal(occ[no_limit], fx["occluded"][no_limit]) and occ[no_limit].any()
    assert not occ[(lane >= 2) & (lane <= 5)].any()          # 0, negative, NaN, -inf: t < tmax never holds
    assert np.array_equal(occ[plain], fx["occluded_tmax"][plain]) and occ[plain].any() and not occ[plain].all()
    print(name, "occluded at no limit:", int(occ[no_limit].sum()), "plain lanes:", int(occ[plain].sum()))
