"""The device's texture path function by function (csrc/dev_texture.h through prt_debug_device_kat, csrc/kernels_debug.h), bit for
bit, on tables and records built by prt_upload_scene: the lookups against the reference's own Texture_SampleBilinear
(tests/golden/kat_texture.npz), the textured-hit functions shade_entry_on calls against the function the oracle's TraceRayColor
calls (scenes and records: tests/texture_cases.py)."""
from __future__ import annotations

import numpy as np
import pytest

import texture_cases as T

pytestmark = pytest.mark.gpu

KAT_TEXTURE, KAT_TEXTURED_HIT = 8, 9


@pytest.fixture(scope="module")
def gold():
    return T.golden()


def test_device_texture_samples_match_reference(gold):
    """One upload (a one-triangle scene whose texture table is the golden's), one launch over every golden record.  The sRGB table
    is computed at upload by this machine's powf: where that is the golden's table (expected), the device must return the
    reference's bits; where it is not, the expected values are the numpy restatement's with this machine's table, and the entries
    that differ are printed - the kernel is held to bits either way."""
    from par_raytracer_amd import api
    rec = np.ascontiguousarray(gold["tex_in"], np.float32)
    lut = T.machine_srgb_lut()
    differ = np.nonzero(T.bits(lut) != T.bits(gold["srgb_lut"]))[0]
    expect = gold["tex_out"]
    if differ.size:
        print("sRGB table: entries %s differ from the golden's (this machine's powf)" % differ.tolist())
        expect = T.bilinear_f32(lut, gold["texture_dims"], gold["texture_bytes"], rec[:, 0], rec[:, 1], rec[:, 2])[0]
    scene = T.one_triangle_scene(gold["texture_dims"], gold["texture_bytes"])
    r = api.Renderer(0)
    try:
        r.upload(scene)
        got = r.device_kat(KAT_TEXTURE, rec, (len(rec), 4), np.float32)
    finally:
        r.close()
    T.assert_same_bits(got[:, :3], expect[:, :3], "tex_sample_rgb on the device")
    T.assert_same_bits(got[:, 3], got[:, 0], "tex_sample_r against tex_sample_rgb's x")


@pytest.fixture(scope="module")
def renderer():
    from par_raytracer_amd import api
    r = api.Renderer(0)
    yield r
    r.close()


@pytest.mark.parametrize("name", list(T.HIT_SCENES))
def test_device_textured_hit_matches_oracle(renderer, name):
    """KAT_TEXTURED_HIT - the functions shade_entry_on calls for a textured hit, on the records prt_upload_scene packed (tri_uv,
    tri_tan, the shading record, the material's texture slots; one triangle, so its record is slot 0) - against the function the
    oracle's TraceRayColor calls, whose frames tests/test_oracle_golden.py holds to the reference's bits: sixteen floats per (v, w)."""
    scene = T.hit_scene(name)
    rec = T.hit_records()
    renderer.upload(scene)
    dev_in = np.concatenate([np.zeros((len(rec), 1), np.float32), rec], axis=1)
    got = renderer.device_kat(KAT_TEXTURED_HIT, dev_in, (len(rec), 16), np.float32)
    T.assert_same_hits(got, T.oracle_hits(scene, rec), name, compare_uv=T.has_maps(name))
