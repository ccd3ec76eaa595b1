"""prt_trace_hits without a GPU: the walks of csrc/dev_hits.h - as k_hits_exact routes a ray, and as one lane of k_hits walks it on
LDS columns - against the definition of include/prt.h as a brute force over every record (tests/hits_host_harness.cpp, both tree
widths, the SAH builder), bit for bit on every field; that the batches hold every class of ray on which the walk can go wrong,
counted from the brute force's own output; paging with the cursor; the harness under the address and undefined-behaviour
sanitizers; and the entry points' argument checks."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import closest_cases as K
import hits_cases as H
import trace_cases as T


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("hits_host")


@pytest.fixture(scope="module")
def scenes():
    """{name: (mesh, origins, directions, tmax or None)}: the plates, the three ray fixtures, and icosphere_l3 with zero-area
    triangles and every triangle stacked on a copy of itself (closest_cases.with_degenerates)."""
    out = {}
    o, d, kind = H.plate_rays()
    out["plates"] = (H.plates(), o, d, None)
    out["plates_kind"] = kind
    for name in T.FIXTURES:
        out[name] = (H.scene_mesh(name),) + H.fixture_rays(name)
    out["degenerate"] = (K.with_degenerates(H.scene_mesh("icosphere_l3"), 41),) + H.fixture_rays("icosphere_l3")
    return out


def all_cases(scenes):
    """(label, case) for one harness run: every k of H.KS on the plates, front only and both sides; the tmax specials; the fixtures
    and the degenerate mesh at two k, without a limit and with the fixture's tmax; the smallest LDS stack."""
    mesh, o, d, _ = scenes["plates"]
    tm, _ = H.tmax_specials(len(o))
    out = []
    for back in (False, True):
        for k in H.KS + (7,):
            out.append(("plates k=%d back=%d" % (k, back), H.case(mesh, o, d, k, back_faces=back, full=H.FULL)))
        out.append(("plates tmax back=%d" % back, H.case(mesh, o, d, 3, tmax=tm, back_faces=back, full=H.FULL)))
    out.append(("plates cap 2", H.case(mesh, o, d, 16, back_faces=True, stack_cap=2)))
    # (without the overflow rays: their biased origins lie 2^117 out, and the pad of a batch follows its largest origin)
    near = scenes["plates_kind"] != "overflow"
    out.append(("plates biased", H.case(mesh, o[near], d[near], 8, back_faces=True, ray_bias=0.125)))
    for name in T.FIXTURES + ("degenerate",):
        mesh, o, d, tmax = scenes[name]
        out.append((name + " k=2", H.case(mesh, o, d, 2, full=4)))
        out.append((name + " k=8 back", H.case(mesh, o, d, 8, back_faces=True, full=16)))
        out.append((name + " k=16 back tmax", H.case(mesh, o, d, 16, tmax=tmax, back_faces=True)))
        out.append((name + " k=3 back cap 3", H.case(mesh, o, d, 3, back_faces=True, stack_cap=3)))
    return out


@pytest.mark.parametrize("width", [4, 8])
def test_walk_and_lane_equal_the_brute_force_bit_for_bit(scenes, workdir, width):
    exe = H.build_harness(workdir, bvh8=width == 8)
    labelled = all_cases(scenes)
    results = H.run_harness(exe, [c for _, c in labelled], workdir)
    seen = {k: 0 for k in H.CLASSES}
    lanes_listed = 0
    for (label, c), r in zip(labelled, results):
        cls = H.classes_of(c, r)
        print(width, label, "mismatches", r["mismatches"], r["lane_mismatches"], cls)
        assert r["mismatches"] == 0 and r["lane_mismatches"] == 0, (width, label)
        H.assert_same_bits(r["walk"], r["brute"], "%d-wide %s" % (width, label))
        for k, v in cls.items():
            seen[k] += v
        lanes_listed += int((r["listed"] == 2).sum())
        filled = np.arange(c["k"])[None, :] < r["brute"]["hit_count"][:, None]
        assert np.all(r["brute"]["group"][~filled] == -1) and np.all(r["brute"]["t"][~filled] == H.FLT_MAX)
        assert np.all(r["brute"]["hit_count"] == np.minimum(r["remaining"], c["k"]))
        if not c["back_faces"]:
            assert not r["brute"]["back"].any()
    print(width, "classes over all cases:", seen, "lanes that dropped a push:", lanes_listed)
    for k in H.CLASSES:
        assert seen[k] > 0, "no ray of class %r in any case" % k
    assert lanes_listed > 0, "no lane overflowed the capped LDS stack"


def test_every_tmax_special_has_rays_and_its_answer(scenes, workdir):
    mesh, o, d, _ = scenes["plates"]
    tm, lane = H.tmax_specials(len(o))
    exe = H.build_harness(workdir)
    limited, free = H.run_harness(exe, [H.case(mesh, o, d, 16, tmax=tm, back_faces=True), H.case(mesh, o, d, 16, back_faces=True)], workdir)
    assert limited["mismatches"] == 0 and free["mismatches"] == 0
    count, free_count = limited["brute"]["hit_count"], free["brute"]["hit_count"]
    for i, name in enumerate(H.TMAX_LANES):
        rays = lane == i
        assert rays.sum() > 0 and free_count[rays].sum() > 0, name
        if name in ("inf", "flt_max"):
            for f in H.FIELDS:
                assert np.array_equal(limited["brute"][f][rays].view(np.uint8), free["brute"][f][rays].view(np.uint8)), (name, f)
        elif name == "own":
            assert np.any(count[rays] < free_count[rays]) and np.any(count[rays] > 0), name
            filled = np.arange(16)[None, :] < count[rays][:, None]
            assert np.all(limited["brute"]["t"][rays][filled] < np.repeat(tm[rays][:, None], 16, 1)[filled])
        else:
            assert not count[rays].any(), name


def test_pages_through_the_cursor_reproduce_the_whole_list(scenes, workdir):
    """Pages of k = 3 chained through the last filled slot until every ray runs dry: the pages laid end to end are the harness's
    full sorted list, and a ray without a cursor (group < 0) or with a NaN cursor is answered as the definition says."""
    mesh, o, d, _ = scenes["plates"]
    exe = H.build_harness(workdir)
    whole = H.run_harness(exe, [H.case(mesh, o, d, 1, back_faces=True, full=H.FULL)], workdir)[0]
    assert whole["remaining"].max() > 24 and whole["remaining"].max() <= H.FULL
    after, pages = None, []
    for _ in range(H.FULL // 3 + 2):
        r = H.run_harness(exe, [H.case(mesh, o, d, 3, back_faces=True, after=after)], workdir)[0]
        assert r["mismatches"] == 0 and r["lane_mismatches"] == 0
        pages.append(r["brute"])
        if not (r["brute"]["hit_count"] == 3).any():
            break
        after = H.last_filled(r["brute"])
    else:
        raise AssertionError("the pages never ran dry")
    for f in ("t", "group", "vertex0", "back"):
        # page p's slot s is entry 3 p + s; a page that ran dry holds the miss record, as the full list's tail does
        laid = np.concatenate([p[f] for p in pages], axis=1)
        m = min(laid.shape[1], H.FULL)
        assert 3 * len(pages) >= whole["remaining"].max()
        assert np.array_equal(np.ascontiguousarray(laid[:, :m]).view(np.uint8), np.ascontiguousarray(whole["full"][f][:, :m]).view(np.uint8)), f
    total = sum(p["hit_count"].astype(np.int64) for p in pages)
    assert np.array_equal(total, whole["remaining"])
    # no cursor for every other ray, a NaN cursor for every fifth
    first = pages[0]
    t, g, v0 = H.last_filled(first)
    g = np.where(np.arange(len(g)) % 2 == 0, -1, g).astype(np.int32)
    t = np.where(np.arange(len(t)) % 5 == 0, np.float32(np.nan), t).astype(np.float32)
    r = H.run_harness(exe, [H.case(mesh, o, d, 3, back_faces=True, after=(t, g, v0))], workdir)[0]
    assert r["mismatches"] == 0 and r["lane_mismatches"] == 0
    none = g < 0
    for f in H.FIELDS:
        assert np.array_equal(r["brute"][f][none].view(np.uint8), first[f][none].view(np.uint8)), f
    assert not r["brute"]["hit_count"][~none & np.isnan(t)].any() and (~none & np.isnan(t) & (first["hit_count"] > 0)).any()


def test_sanitized_harness_on_the_plates(scenes, workdir):
    mesh, o, d, _ = scenes["plates"]
    exe = H.build_harness(workdir, sanitize=True)
    first = H.run_harness(exe, [H.case(mesh, o, d, 16, back_faces=True, full=H.FULL)], workdir)[0]
    tm, _ = H.tmax_specials(len(o))
    rest = H.run_harness(exe, [H.case(mesh, o, d, 16, back_faces=True, after=H.last_filled(first["brute"]), stack_cap=2),
                               H.case(mesh, o, d, 1, tmax=tm)], workdir)
    for r in [first] + rest:
        assert r["mismatches"] == 0 and r["lane_mismatches"] == 0


def test_entry_points_without_a_gpu():
    from par_raytracer_amd import capi
    lib = capi.hip_lib()
    assert lib.prt_abi_version() == 5
    assert "prt_trace_hits" in capi.PRT_SYMBOLS and "prt_trace_hits_device" in capi.PRT_SYMBOLS
    assert capi.MAX_HITS == 16 and capi.HITS_BACK_FACES == 1
    o = np.zeros((4, 3), np.float32)
    count = np.zeros(4, np.uint32)
    rq = capi.PrtHitsRequest(capi.PrtRayBatch(o.ctypes.data, o.ctypes.data, None, 4, 0.0), 3, 0, None, None, None)
    out = capi.PrtHitsBuffers(count.ctypes.data, None, None, None, None, None)
    assert lib.prt_trace_hits(None, C.byref(rq), C.byref(out), 0, None) == -1
    assert lib.prt_trace_hits_device(None, C.byref(rq), C.byref(out), 0, None) == -1
