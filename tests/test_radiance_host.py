"""prt_render_rays without a GPU: the CPU yardstick of tests/radiance_cases.py is proved against RenderPixel, its fixture batches
are shown to be mixed, the domain function and par_raytracer_amd/cameras.py are checked, and the two kernels of
csrc/kernels_rays.h run lane by lane on the host in a stand-alone program built with AddressSanitizer and UBSan
(tests/rays_host_harness.cpp, through tests/hip_shim) over a batch of 3 passes x 2 chains of uneven size."""
from __future__ import annotations

import ctypes as C
import re

import numpy as np
import pytest

import harness
import radiance_cases as R
from conftest import host_scene, scene_dir

F = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("name", ["cornell_box", "many_materials"])
@pytest.mark.parametrize("spp", [3, 8])
def test_camera_rays_with_the_camera_stream_are_render_pixel(name, spp):
    """The yardstick: RenderPixel's own rays through the harness's definition, keyed with first = p0, give oracle_py.render's
    pixels bit for bit and its ray count."""
    import oracle_py as orc
    from par_raytracer_amd import api
    s, _ = scene_dir(name)
    hs = host_scene(name)
    w, h = 24, 16
    cam = api.make_camera(s.fov, w, h, s.camera_position, s.camera_facing)
    params = api.default_params(spp, 77)
    frame, octr = orc.render(hs.desc, cam, params, w, h, lattice=1, threads=4)
    frame = frame.reshape(w * h, 4)
    o, d = R.camera_rays(cam, 77, w, 0, w * h, spp)
    assert R.in_domain(o, d, params.ray_bias, R.scene_abs_max(hs.arrays())).all()
    whole = R.oracle_batch(hs.desc, params, o, d, first=0, camera_stream=True)
    assert np.array_equal(bits(whole["rgba"]), bits(frame))
    assert whole["ray_count"] == octr.ray_count
    p0, n = 100, 65
    part = R.oracle_batch(hs.desc, params, o[p0:p0 + n], d[p0:p0 + n], first=p0, camera_stream=True)
    assert np.array_equal(bits(part["rgba"]), bits(frame[p0:p0 + n]))
    # the flag and `first` matter: without either the stream is another one
    plain = R.oracle_batch(hs.desc, params, o[p0:p0 + n], d[p0:p0 + n], first=p0, camera_stream=False)
    moved = R.oracle_batch(hs.desc, params, o[p0:p0 + n], d[p0:p0 + n], first=p0 + 1, camera_stream=True)
    assert not np.array_equal(bits(plain["rgba"]), bits(part["rgba"])) and not np.array_equal(bits(moved["rgba"]), bits(part["rgba"]))


@pytest.mark.parametrize("name", R.SCENES)
def test_the_fixture_batches_are_mixed(name):
    from par_raytracer_amd import api
    hs = host_scene(name)
    arrays = hs.arrays()
    o, d, family = R.make_rays(arrays, 257, 8, R.SEEDS[name])
    assert set(family.tolist()) == {0, 1, 2}
    assert R.in_domain(o, d, api.default_params(8).ray_bias, R.scene_abs_max(arrays)).all()
    for spp in (1, 3, 8):
        exp = R.oracle_batch(hs.desc, api.default_params(spp, 5), o[:, :spp], d[:, :spp], first=5)
        R.assert_mixed(exp, "%s x %d" % (name, spp), want_translucent=name == "many_materials")
        hit = exp["primary_hit"].astype(bool)
        assert hit[family == 0].any() and hit[family == 1].any() and not hit[family == 2].any(), name
    far_o, far_d = R.far_rays(arrays, 65, 3, 9, 10.0)
    am = R.scene_abs_max(arrays)
    assert R.in_domain(far_o, far_d, 0.001, am).all() and (np.abs(far_o).max(-1) > F(4.0) * am).all()


def test_the_domain_function():
    am = F(2.5)
    o = np.zeros((12, 3), F)
    d = np.tile(np.array([[0.0, 0.0, 1.0]], F), (12, 1))
    want = np.ones(12, bool)
    o[1, 0], want[1] = np.nan, False
    o[2, 2], want[2] = np.inf, False
    d[3, 1], want[3] = np.nan, False
    d[4, 0], want[4] = -np.inf, False
    d[5], want[5] = 0.0, False                                              # the zero direction is not unit length
    # |d|^2 = 1 +- 2^-17 is outside, 1 +- 2^-20 inside (2^-18 is the bound)
    for row, l2, ok in ((6, 1.0 + 2.0 ** -17, False), (7, 1.0 - 2.0 ** -17, False), (8, 1.0 + 2.0 ** -20, True), (9, 1.0 - 2.0 ** -20, True)):
        d[row, 2] = F(np.sqrt(l2))
        got = F(d[row, 2] * d[row, 2])
        assert (abs(float(got) - 1.0) <= 2.0 ** -18) == ok, (row, got)
        want[row] = ok
    o[10, 1], want[10] = F(63.0) * am, True
    o[11, 1], want[11] = -F(65.0) * am, False
    assert np.array_equal(R.in_domain(o, d, 0.001, am), want)
    o64 = np.zeros((2, 3), F)
    o64[0, 0], o64[1, 0] = F(64.0) * am, np.nextafter(F(64.0) * am, F(np.inf))
    assert R.in_domain(o64, d[:2], 0.0, am).tolist() == [True, False]
    # a bias that is not finite makes the biased origin not finite, whatever the ray
    assert not R.in_domain(o[:1], d[:1], np.inf, am).any() and not R.in_domain(o[:1], d[:1], np.nan, am).any()
    assert R.in_domain(o[:1], d[:1], 0.001, am).all()


def test_pinhole_rays_are_make_camera_ray_bit_for_bit():
    import oracle_py as orc
    from par_raytracer_amd import api, cameras
    s, _ = scene_dir("cornell_box")
    cam = api.make_camera(s.fov, 160, 90, s.camera_position, s.camera_facing)
    rng = np.random.default_rng(3)
    xy = np.concatenate([rng.uniform(-1, 161, (500, 2)), [[0, 0], [159.5, 89.5], [79.5, 44.5]]]).astype(F)
    o, d = cameras.pinhole_rays(cam, xy)
    assert o.dtype == F and d.dtype == F and o.shape == d.shape == (503, 3)
    want = np.zeros(3, F)
    for k in range(xy.shape[0]):
        orc.lib().prt_oracle_camera_ray(C.cast(C.pointer(cam), C.c_void_p), float(xy[k, 0]), float(xy[k, 1]), want.ctypes.data)
        assert np.array_equal(bits(d[k]), bits(want)), (k, xy[k])
    assert np.array_equal(o, np.tile(np.array(list(cam.position), F), (503, 1)))
    assert R.in_domain(o, d, 0.001, F(max(abs(v) for v in cam.position))).all()


def test_the_other_cameras_make_unit_rays_inside_the_domain():
    from par_raytracer_amd import cameras
    rng = np.random.default_rng(4)
    uv = rng.uniform(0, 1, (4096, 2)).astype(F)
    uv[:4] = [[0, 0], [1, 1], [0.5, 0.5], [0.25, 0.0]]
    o, d = cameras.equirect_rays((1.0, 2.0, 3.0), uv)
    assert o.dtype == F and d.dtype == F and R.in_domain(o, d, 0.001, F(3.0)).all()
    assert np.allclose(d[2], [0, 0, -1], atol=1e-6) and np.allclose(d[0], [0, 1, 0], atol=1e-6) and np.allclose(d[1], [0, -1, 0], atol=1e-6)
    o2, d2 = cameras.equirect_rays((0, 0, 0), np.array([[0.75, 0.5]], F))
    assert np.allclose(d2[0], [1, 0, 0], atol=1e-6)                        # a quarter turn to the right of -z, y up
    # every direction of the sphere is reached
    assert (d.min(0) < -0.95).all() and (d.max(0) > 0.95).all()
    oo, od = cameras.orthographic_rays((0.0, 1.0, 5.0), (0.0, 0.0, -2.0), 2.0, 1.0, uv * 2 - 1)
    assert oo.dtype == F and od.dtype == F and R.in_domain(oo, od, 0.0, F(5.0)).all()
    assert np.array_equal(od, np.tile(np.array([[0, 0, -1]], F), (4096, 1)))
    assert np.allclose(oo[:, 2], 5.0) and oo[:, 0].min() >= -2.0 and oo[:, 0].max() <= 2.0 and oo[:, 1].min() >= 0.0 and oo[:, 1].max() <= 2.0
    assert np.allclose(oo[1], [2.0, 2.0, 5.0])                              # (u, v) = (1, 1): right and up


def test_the_kernels_run_lane_by_lane_under_the_sanitizers(tmp_path):
    """k_rays_check's three words and k_raygen_rays's queue entries and generators over 3 passes x 2 chains of uneven size, in a
    stand-alone program with its own main: a wrong base is an out-of-bounds access there, not a fault on a card."""
    exe = harness.build("rays_host_harness.cpp", tmp_path, "rays_host", sanitize=True)
    lines = harness.run(exe, timeout=120).splitlines()
    assert lines[0] == "check | clean_ok 1 bad_ok 1 edge_ok 1 bias_ok 1"
    for cs in (0, 1):
        m = re.fullmatch(r"raygen camera_stream (\d) \| plain bad (\d+) of (\d+) ring bad (\d+) of (\d+)", lines[1 + cs])
        assert m and [int(v) for v in m.groups()] == [cs, 0, 1602, 0, 1602], lines[1 + cs]


def test_the_symbols_are_exported_and_null_handles_refused_without_a_gpu():
    from par_raytracer_amd import api, capi
    lib = capi.hip_lib()
    b, p = capi.PrtRadianceBatch(), api.default_params(1)
    assert lib.prt_render_rays(None, C.byref(b), C.byref(p), None, None) == -1
    assert lib.prt_render_rays_device(None, None, None, None, None) == -1
    assert C.sizeof(capi.PrtRadianceBatch) == 32 and capi.RAYS_CAMERA_STREAM == 1
    assert {"prt_render_rays", "prt_render_rays_device"} <= set(capi.PRT_SYMBOLS)
