"""The cases of tests/trace_edge_cases.py without a GPU: they are what they claim (exact zeros and their signs, coordinates shared
bit for bit with vertices, the listed component values, exact scalings), none passes by containing nothing (by the oracle alone:
hits, misses, both answers of OCCLUDED below tmax), the cornell_box axis case holds rays on which TraceRay's answer is not the
closest hit over all triangles although nothing ties with it (a grazed group sphere), and the device traversal compiled for the
host (tests/trace_host_harness.cpp --file, both tree widths) returns the brute-force filter's hit on every case - which places
a box-test failure here, without a GPU.  The length case on the flat grid fails that check through the renders' start of a
traversal (trav_init's absolute 1e-30 clamp: 35 of 2,048 rays) and passes through the queries' (trav_start<true>)."""
from __future__ import annotations

import re
import subprocess

import numpy as np
import pytest

import harness as H                                         # (the fixture below is called harness)
import trace_cases as T
import trace_edge_cases as E


def of_family(family):
    return [c for c in E.CASES if c.split("-")[0] == family]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def vertex_and_midpoint_rows(sc):
    t = sc.positions[sc.tri]
    mids = [((t[:, c] + t[:, (c + 1) % 3]) * np.float32(0.5)).astype(np.float32) for c in range(3)]
    return {r.tobytes() for r in np.concatenate([sc.positions] + mids)}


def check_axis(c, sel):
    sc = c["scene"]
    o, d, ax, target = c["origins"][sel], c["directions"][sel], c["axis"][sel].astype(int), c["target"][sel]
    i = np.arange(len(ax))
    assert np.all(np.abs(d[i, ax]) == 1) and (d[i, ax] > 0).any() and (d[i, ax] < 0).any()
    z1, z2 = d[i, (ax + 1) % 3], d[i, (ax + 2) % 3]
    assert np.all(z1 == 0) and np.all(z2 == 0)
    pairs = set(zip(np.signbit(z1).tolist(), np.signbit(z2).tolist()))
    assert len(pairs) == 4, pairs                                             # +0 +0, -0 +0, +0 -0, -0 -0
    aimed = c["aimed"][sel]
    assert abs(int(aimed.sum()) * 2 - len(i)) <= 1
    known = vertex_and_midpoint_rows(sc)
    assert all(r.tobytes() in known for r in target[aimed])
    for k in (1, 2):                                                          # the other two coordinates: the target's bits
        assert np.array_equal(bits(o[i, (ax + k) % 3])[aimed], bits(target[i, (ax + k) % 3])[aimed])
    lo, hi = sc.box()
    ext = float((hi - lo).max())
    before = ((target[i, ax] - o[i, ax]) * d[i, ax])[aimed] / ext             # 0.1 to 0.9 extents before it, along the axis
    assert before.min() > 0.099 and before.max() < 0.901, (before.min(), before.max())
    assert np.all((o[~aimed] >= lo) & (o[~aimed] <= hi))


def check_plane(c, sel):
    sc = c["scene"]
    o, d, ax, target = c["origins"][sel], c["directions"][sel], c["axis"][sel].astype(int), c["target"][sel]
    i = np.arange(len(ax))
    z = d[i, ax]
    assert np.all(z == 0) and np.signbit(z).any() and not np.signbit(z).all()
    a, b = d[i, (ax + 1) % 3].astype(np.float64), d[i, (ax + 2) % 3].astype(np.float64)
    assert np.abs(a * a + b * b - 1).max() < 2.0 ** -22
    aimed = c["aimed"][sel]
    assert abs(int(aimed.sum()) * 2 - len(i)) <= 2
    coords = [set(bits(sc.positions[:, k]).tolist()) for k in range(3)]
    assert all(int(w) in coords[k] for w, k in zip(bits(o[i, ax])[aimed], ax[aimed]))
    assert np.array_equal(bits(o[i, ax])[aimed], bits(target[i, ax])[aimed])
    assert len(set(ax.tolist())) == 3


@pytest.mark.parametrize("cid", of_family("axis") + of_family("plane") + of_family("tiny") + of_family("flat") + of_family("degenerate"))
def test_axis_and_plane_rays_are_what_they_claim(cid):
    c = E.case(cid)
    kinds = set(c["kind"].tolist())
    assert kinds == {"axis": {"axis"}, "plane": {"plane"}, "degenerate": {"axis", "front"}}.get(cid.split("-")[0], {"axis", "plane", "front"})
    assert len(c["kind"]) == {"axis-cornell_box": 8192, "tiny": 256, "flat": 512, "degenerate": 1024}.get(
        cid if cid == "axis-cornell_box" else cid.split("-")[0], 1536)
    if "axis" in kinds:
        check_axis(c, np.nonzero(c["kind"] == "axis")[0])
    if "plane" in kinds:
        check_plane(c, np.nonzero(c["kind"] == "plane")[0])
    if cid == "plane-cornell_box":                                            # a pinned ray lies in the plane of an axis-aligned wall
        sc = c["scene"]
        t = sc.positions[sc.tri]
        walls = {(k, float(t[j, 0, k])) for j in range(len(t)) for k in range(3) if np.all(t[j, :, k] == t[j, 0, k])}
        ax = c["axis"].astype(int)
        in_wall = [(int(k), float(x)) in walls for k, x in zip(ax, c["origins"][np.arange(len(ax)), ax])]
        print(cid, "rays in the plane of a wall:", sum(in_wall))
        assert sum(in_wall) >= 256
    if cid == "flat-grid":
        sc = c["scene"]
        assert np.all(sc.positions[:, 1] == 0.5) and len(sc.tri) == 128
        plane = np.nonzero((c["kind"] == "plane") & (c["axis"] == 1) & (c["origins"][:, 1] == 0.5))[0]
        print(cid, "rays in the scene's plane:", len(plane))
        assert len(plane) >= 8 and not (c["group"][plane] >= 0).any()         # they lie in it: facing no triangle
    if cid.startswith("tiny"):
        sc = c["scene"]
        which = cid.split("-")[1]
        assert len(sc.tri) == int(which[0]) and len(sc.arrays["groups"]) // 12 == (2 if which.endswith("x2") else 1)
    if cid.startswith("degenerate"):
        sc = c["scene"]
        t = sc.positions[sc.tri].astype(np.float64)
        area = np.linalg.norm(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), axis=1)
        assert int((area == 0).sum()) >= 192 and len(sc.arrays["groups"]) // 12 == 3


def test_clamp_rays_hold_every_listed_value_with_both_signs():
    c = E.case("clamp-icosphere_l3")
    d, slot, value = c["directions"], c["slot"], c["value"]
    n = len(d)
    assert n == 1024 and np.all(slot[:, 0] >= 0)
    i = np.arange(n)
    assert np.array_equal(bits(d[i, slot[:, 0]]), bits(value[:, 0]))
    two = slot[:, 1] >= 0
    assert abs(int(two.sum()) * 2 - n) <= 1 and np.array_equal(bits(d[i[two], slot[two, 1]]), bits(value[two, 1]))
    listed = np.array([2.0 ** -149, 2.0 ** -126, np.nextafter(np.float32(1e-30), np.float32(0)), np.float32(1e-30),
                       np.nextafter(np.float32(1e-30), np.float32(1)), 2.0 ** -99, 2.0 ** -64], np.float32)
    assert listed[2] < listed[3] < listed[4] and len(set(bits(listed).tolist())) == 7
    for col, rows in ((0, i), (1, i[two])):
        for v in listed:
            for s in (np.float32(1), np.float32(-1)):
                assert (bits(value[rows, col]) == bits(np.float32(v * s))).any(), (col, v, s)
    rest = np.ones((n, 3), bool)                                              # the untouched components are the larger ones
    rest[i, slot[:, 0]] = False
    rest[i[two], slot[two, 1]] = False
    assert np.abs(d[rest]).min() > 2.0 ** -30


@pytest.mark.parametrize("cid", of_family("length"))
def test_length_rays_start_at_zero_and_span_2_pow_240(cid):
    c = E.case(cid)
    o, d, k = c["origins"], c["directions"], c["exponent"]
    assert len(o) == 2048 and not o[:1024].any() and not np.signbit(o[:1024]).any()
    assert np.array_equal(bits(d[:1024]), bits(d[1024:])) and o[1024:].any()
    i = np.arange(1024)
    assert np.array_equal(k[:1024], np.array(E.LENGTH_EXPONENTS)[i * 8 // 1024]) and [int((k[:1024] == e).sum()) for e in E.LENGTH_EXPONENTS] == [128] * 8
    unit = np.ldexp(d[:1024].astype(np.float64), -k[:1024, None])             # exact: back to length <= 1
    norm = np.linalg.norm(unit, axis=1)
    assert norm.max() < 1 + 1e-6 and norm[i % 4 == 0].min() > 1 - 1e-6 and norm[i % 4 == 3].min() > 1 - 1e-6
    assert (norm[i % 4 == 1] < 1 - 1e-9).any() and (norm[i % 4 == 2] < 1 - 1e-9).any()
    assert (np.abs(d[d != 0]) < 2.0 ** -126).any()                            # subnormal components among them
    lo, hi = c["scene"].box()
    if cid == "length-flat_grid":
        assert lo[1] == hi[1] == np.float32(0.5) - np.float32(0.55) and np.all(lo[[0, 2]] < 0) and np.all(hi[[0, 2]] > 0)       # the origin 0 lies above it, on its front side
    else:
        assert np.all(lo < 0) and np.all(hi > 0)                              # the origin 0 lies inside


@pytest.mark.parametrize("cid", of_family("scale") + of_family("shift"))
def test_scaled_and_shifted_cases_are_exact(cid):
    c = E.case(cid)
    family, rest = cid.split("-", 1)
    name, arg = rest.split("@")
    base = E.base_scene(name)
    o0, d0 = E.fixture_rays(name)
    sc = c["scene"]
    assert len(o0) == 1024 and sc.obj is not base.obj and np.array_equal(sc.tri, base.tri)
    sph, sph0 = (s.arrays["spheres"].view(np.float32).reshape(-1, 6) for s in (sc, base))
    assert np.array_equal(bits(sph[:, 4:]), bits(sph0[:, 4:]))
    if family == "scale":
        e = int(arg)
        for got, was in ((sc.positions, base.positions), (c["origins"], o0), (sph[:, :4], sph0[:, :4])):
            assert np.array_equal(np.ldexp(got.astype(np.float64), -e), was.astype(np.float64))
        similar = e in E.SCALE_SIMILAR
        assert np.array_equal(np.ldexp(c["directions"].astype(np.float64), -e if similar else 0), d0.astype(np.float64))
        if similar:                                                           # reported, not required: the same answers as the base case
            g = T.fixture(name)
            sel = T.bias0(g)[:1024]
            same = [int((bits(c[k]).reshape(1024, -1) == bits(g[k][sel]).reshape(1024, -1)).all(1).sum()) for k in ("group", "vertex0", "bw")]
            print("%s: rays with the base case's group %d, vertex0 %d, bw %d of 1024" % (cid, *same))
    else:
        off = np.float32(float(arg))
        assert np.array_equal(bits(sc.positions), bits((base.positions + off).astype(np.float32)))
        assert np.array_equal(bits(c["origins"]), bits((o0 + off).astype(np.float32))) and np.array_equal(bits(c["directions"]), bits(d0))
        assert np.array_equal(bits(sph[:, 3]), bits(sph0[:, 3] * np.float32(1 + 2.0 ** -10)))


@pytest.mark.parametrize("cid", E.CASES)
def test_no_case_passes_by_containing_nothing(cid):
    c = E.case(cid)
    s = E.summary(c)
    print("%-26s %5d triangles, %5d rays, %5d hits, %4d near ties, %4d rays where TraceRay is not the brute-force closest hit (%d without "
          "a near tie), %5d occluded below tmax" % (cid, len(c["scene"].tri), s["rays"], s["hits"], s["near_ties"], s["parts"],
                                                   s["parts_no_tie"], s["occluded_tmax"]))
    n = s["rays"]
    if not cid.startswith("tiny"):
        assert s["hits"] * 5 >= n and (n - s["hits"]) * 10 >= n, s
    assert 0 < s["occluded_tmax"] < int(c["occluded"].sum()), s              # both answers below tmax, among the occluded rays
    assert np.all(c["occluded_tmax"] <= c["occluded"])


def test_the_cornell_box_axis_case_holds_grazed_spheres():
    """Rays on which TraceRay differs from the closest hit over all triangles with no second hit within 2^-19: the reference's
    IntersectRaySphere rejects a group whose sphere the ray grazes at one of the vertices it was built through."""
    c = E.case("axis-cornell_box")
    s = E.summary(c)
    print("axis-cornell_box: %d rays part from the brute force, %d of them without a near tie" % (s["parts"], s["parts_no_tie"]))
    assert s["parts_no_tie"] >= 16


# ---- the device traversal on the host

@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    made = {}

    def get(flavour):
        if flavour not in made:
            made[flavour] = H.build("trace_host_harness.cpp", tmp_path_factory.mktemp("edges"), "trace_host_" + flavour,
                                    bvh8=flavour == "bvh8", sources=("bvh_build.cpp",))
        return made[flavour]
    return get


def write_case(c, path):
    sc = c["scene"]
    verts = np.ascontiguousarray(sc.positions[sc.tri], np.float32)
    with open(path, "wb") as f:
        f.write(np.array([len(sc.tri), len(c["origins"])], np.uint32).tobytes())
        for a in (verts, c["origins"], c["directions"]):
            f.write(np.ascontiguousarray(a, np.float32).tobytes())


def mismatches(exe, mode, path):
    run = subprocess.run([exe, mode, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = run.stdout.decode()
    m = re.search(r"closest-hit mismatches (\d+), any-hit mismatches (\d+), unresolved near ties (\d+)", out)
    assert m, out
    return tuple(int(x) for x in m.groups()), run.returncode, out


@pytest.mark.parametrize("flavour", ["bvh4", "bvh8"])
@pytest.mark.parametrize("cid", [c for c in E.CASES if c.split("-")[0] in E.HOST_WALK_FAMILIES])
def test_device_traversal_on_the_host_equals_the_brute_force_filter(harness, tmp_path, cid, flavour):
    c = E.case(cid)
    path = str(tmp_path / "case.bin")
    write_case(c, path)
    counts, rc, out = mismatches(harness(flavour), "--file", path)
    assert counts == (0, 0, 0) and rc == 0, out
    if cid.startswith("length"):                                              # what the family is for: the absolute clamp bends these rays
        plain, rc, out = mismatches(harness(flavour), "--file-plain", path)
        print(cid, flavour, "through trav_init's absolute clamp: closest-hit, any-hit mismatches", plain[:2])
        if cid == "length-flat_grid":                                         # (the other two scenes cannot show it: trace_edge_cases.build)
            assert plain[0] > 0 and plain[1] > 0 and rc == 1, out
