"""The texture path on the host, bit for bit.  Lookups against the reference's own Texture_SampleBilinear
(tests/golden/kat_texture.npz): the float32 numpy restatement of tests/texture_cases.py, what the golden's records cover, and
csrc/dev_texture.h itself, compiled for the host with tests/hip_shim and fed by csrc/tex_upload.h (tests/texture_host_harness.cpp).
The textured-hit functions of csrc/dev_texture.h, compiled the same way, against the function the oracle's TraceRayColor calls."""
from __future__ import annotations

import numpy as np
import pytest

import texture_cases as T


@pytest.fixture(scope="module")
def gold():
    return T.golden()


@pytest.fixture(scope="module")
def restated(gold):
    """(rgba, tx0, ty0, fx, fy) of every golden record by the numpy restatement with the golden's own sRGB table."""
    rec = gold["tex_in"]
    return T.bilinear_f32(gold["srgb_lut"], gold["texture_dims"], gold["texture_bytes"], rec[:, 0], rec[:, 1], rec[:, 2])


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("texture_host")


@pytest.fixture(scope="module")
def exe(workdir):
    return T.build_harness(workdir)


@pytest.fixture(scope="module")
def harness(gold, exe, workdir):
    return T.run_harness(exe, gold["texture_dims"], gold["texture_bytes"], gold["tex_in"], workdir)


@pytest.fixture(scope="module")
def hits(exe, workdir):
    """(records, {scene name: scene}, {scene name: the host harness's (n, 16)}, {scene name: the oracle's}), one harness run."""
    rec = T.hit_records()
    scenes = {name: T.hit_scene(name) for name in T.HIT_SCENES}
    got = T.run_hit_harness(exe, list(scenes.values()), rec, workdir)
    return rec, scenes, dict(zip(scenes, got)), {name: T.oracle_hits(s, rec) for name, s in scenes.items()}


def test_numpy_restatement_equals_the_reference(gold, restated):
    assert gold["tex_out"].shape == (len(gold["tex_in"]), 4) and np.all(np.isfinite(gold["tex_in"]))
    T.assert_same_bits(restated[0], gold["tex_out"], "bilinear_f32 against Texture_SampleBilinear")


def test_golden_records_reach_the_edges(gold, restated):
    """Computed from tex_in with the restatement (which the test above holds to the reference's bits): the vectors reach the
    first and the last texel pair, exact texel boundaries and interior points on every axis with more than two texels, the wrap
    of a tiny negative coordinate to exactly 1, coordinates past 2^24, every sRGB table entry, and the 2 x 2 textures' only tap."""
    _, tx0, ty0, fx, fy = restated
    rec = gold["tex_in"]
    dims = gold["texture_dims"].reshape(-1, 3).astype(np.int64)
    tex = rec[:, 0].astype(np.int64)
    assert len(dims) == 9 and set(np.unique(tex)) == set(range(9))
    for t, (sx, sy, ch) in enumerate(dims):
        of = tex == t
        for axis, size, t0, f in (("x", sx, tx0, fx), ("y", sy, ty0, fy)):
            if size > 2:
                counts = [int((of & (t0 == 0)).sum()), int((of & (t0 == size - 2)).sum()), int((of & (f == 0)).sum()),
                          int((of & (f > 0) & (f < 1)).sum())]
                assert min(counts) >= 8, (t, axis, counts)
            else:
                assert np.all(t0[of] == 0) and np.all(f[of] == 0), (t, axis)
        if sx == 2 and sy == 2:
            assert np.all(tx0[of] == 0) and np.all(ty0[of] == 0) and np.all(fx[of] == 0) and np.all(fy[of] == 0), t
    u, v = rec[:, 1], rec[:, 2]
    tiny_u, tiny_v = (u < 0) & (u > -1e-6), (v < 0) & (v > -1e-6)
    assert int((tiny_u & (T.wrap_f32(u) == 1.0)).sum()) >= 20 and int((tiny_v & (T.wrap_f32(v) == 1.0)).sum()) >= 20
    assert int((np.abs(u) >= 2.0 ** 24).sum()) >= 20
    seen = T.tapped_byte_values(gold["texture_dims"], gold["texture_bytes"], tex, tx0, ty0)
    assert seen.all(), np.nonzero(~seen)[0]
    # the ramp alone reads every table entry, the sRGB knee (bytes 10 and 11: 10 / 255 <= 0.04045 < 11 / 255) included
    ramp = tex == 8
    assert T.tapped_byte_values(gold["texture_dims"], gold["texture_bytes"], tex[ramp], tx0[ramp], ty0[ramp]).all()
    lut = gold["srgb_lut"]
    assert lut[10] == np.float32(10) * (np.float32(1) / np.float32(255)) / np.float32(12.92) and lut[0] == 0 and lut[255] == 1


def test_device_header_on_the_host_equals_the_reference(gold, harness):
    """csrc/dev_texture.h (g++ -O1 -ffp-contract=off) on csrc/tex_upload.h's tables: tex_sample_rgb's three channels are the
    reference's bits, tex_sample_r is the red channel's.  The sRGB table is this machine's powf: where it is not the golden's (a
    different C library), the expected values are the restatement's with this machine's table, and the entries are printed."""
    lut, got = harness
    expect = gold["tex_out"]
    differ = np.nonzero(T.bits(lut) != T.bits(gold["srgb_lut"]))[0]
    if differ.size:
        print("sRGB table: entries %s differ from the golden's (this machine's powf)" % differ.tolist())
        rec = gold["tex_in"]
        expect = T.bilinear_f32(lut, gold["texture_dims"], gold["texture_bytes"], rec[:, 0], rec[:, 1], rec[:, 2])[0]
    assert np.array_equal(T.bits(lut), T.bits(T.machine_srgb_lut())), "tex_fill_srgb_lut against powf through ctypes"
    T.assert_same_bits(got[:, :3], expect[:, :3], "tex_sample_rgb on the host")
    T.assert_same_bits(got[:, 3], got[:, 0], "tex_sample_r against tex_sample_rgb's x")
    T.assert_same_bits(got[:, 4], expect[:, 3], "the fourth channel of the expanded texels")


def test_hit_records_reach_the_block_s_branches(hits):
    """From the records and the oracle's answers alone: corners, a zero on each barycentric, 1 - v - w a tiny negative, and, in the
    scenes made for it, alpha x texel on both sides of 0.05 and of 1."""
    rec, scenes, _, oracle = hits
    v, w = rec[:, 0], rec[:, 1]
    bwx = (np.float32(1) - v - w).astype(np.float32)
    assert len(rec) >= 300 and {(0.0, 0.0), (1.0, 0.0), (0.0, 1.0)} <= set(map(tuple, rec.tolist()))
    assert (v == 0).sum() >= 10 and (w == 0).sum() >= 10 and (bwx == 0).sum() >= 10
    assert ((bwx < 0) & (bwx > -1e-6)).sum() >= 10 and bwx[-241] == np.float32(-2.0 ** -23)
    assert ((bwx > 0) & (v > 0) & (w > 0)).sum() >= 200
    a = oracle["alpha_1p5_with_map"]
    assert np.all(a[:, 3] == 1) and (a[:, 2] <= 0.05).sum() >= 5 and ((a[:, 2] > 0.05) & (a[:, 2] < 1)).sum() >= 20 and (a[:, 2] > 1).sum() >= 20
    b = oracle["alpha_1_map_below_0p05"]
    assert np.all(b[:, 3] == 1) and (b[:, 2] <= 0.05).sum() >= 5 and (b[:, 2] > 0.05).sum() >= 100
    assert np.all(oracle["alpha_0p9_without_map"][:, 2:4] == np.float32([0.9, 1.0]))
    assert np.all(oracle["no_maps"][:, 2:4] == np.float32([1, 1]))
    uv = oracle["map_kd"][:, :2]
    assert (uv < 0).any() and (uv > 1).any() and np.array_equal(uv[:3], T.HIT_TEXCOORDS)      # the corners: integer, negative, past 1
    n = oracle["bump_three_normals_and_tangents"][:, 13:16]
    assert np.all(np.isfinite(n)) and np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1).max() > 1e-3, "the bumped normal is not unit length"


@pytest.mark.parametrize("name", list(T.HIT_SCENES))
def test_textured_hit_on_the_host_equals_the_oracle(hits, name):
    """The textured-hit functions of csrc/dev_texture.h (textured_hit_at: what shade_entry_on does with a hit, without its alpha
    early-out), compiled for the host, against the function the oracle's TraceRayColor calls: sixteen floats per record."""
    _, _, got, oracle = hits
    T.assert_same_hits(got[name], oracle[name], name, compare_uv=T.has_maps(name))
