"""Host logic on CPU: OBJ/MTL loader, sphere hierarchy, flattening, tone map + PNG, C ABI surface, BVH builder.

No compute call needs a GPU here: prt_create must fail cleanly without one, and everything else is host code.
"""
from __future__ import annotations

import ctypes as C
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

import texture_fixtures
from conftest import ROOT, host_scene, load_golden, scene_dir

from par_raytracer_amd import api, capi, scenes


# ---- the C ABI: every symbol the headers declare is exported ----------------------------------------------

def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(prt_[a-z0-9_]+)\s*\(", text)))


def test_hip_library_exports_every_declared_symbol():
    lib = capi.hip_lib()
    names = _declared("prt.h")
    assert set(names) == set(capi.PRT_SYMBOLS), "capi.PRT_SYMBOLS out of sync with include/prt.h"
    for n in names:
        assert hasattr(lib, n), "libprt_hip.so does not export %s" % n
    assert lib.prt_abi_version() == 5


def test_host_library_exports_every_declared_symbol():
    lib = capi.host_lib()
    names = _declared("prt_host.h")
    assert set(names) == set(capi.PRT_HOST_SYMBOLS)
    for n in names:
        assert hasattr(lib, n), "libprt_host.so does not export %s" % n


def test_public_headers_are_plain_c(tmp_path):
    """include/*.h is the drop-in boundary: it must compile as C99 (no C++, no torch types) and a C program must link
    against the library with nothing but the header."""
    import shutil
    import subprocess
    if not shutil.which("gcc"):
        pytest.skip("no C compiler")
    src = tmp_path / "abi.c"
    src.write_text('#include "prt.h"\n#include "prt_host.h"\n#include "prt_key.h"\n#include <stdio.h>\n'
                   'int main(void) {\n'
                   '    prt_params p; prt_camera c; prt_counters k; prt_scene_desc d;\n'
                   '    (void)p; (void)c; (void)k; (void)d;\n'
                   '    printf("%d %u\\n", prt_abi_version(), (unsigned)prt_shard_rows(1080, 8, 3, 8));\n'
                   '    return prt_last_error(0) ? 0 : 1;\n}\n')
    pkg = os.path.join(ROOT, "par_raytracer_amd")
    exe = tmp_path / "abi"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-L", pkg, "-lprt_hip", "-Wl,-rpath," + pkg], check=True)
    out = subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE).stdout.decode().split()
    assert int(out[0]) == capi.hip_lib().prt_abi_version() and int(out[1]) == 136          # 17 of the 135 row blocks: 16 x 8 + 8 rows


def test_struct_sizes_match_the_reference_layouts():
    # SURVEY.md §8a A19 [probed] sizes of the reference structs these mirror
    assert C.sizeof(capi.PrtBSphere) == 24          # BoundingSphere
    assert C.sizeof(capi.PrtCamera) == 64           # Camera
    assert C.sizeof(capi.PrtLight) == 48            # LightSource


def test_error_paths_without_a_gpu_or_scene():
    lib = capi.hip_lib()
    import torch
    if not torch.cuda.is_available():
        assert not lib.prt_create(0)
        assert b"no HIP device" in lib.prt_last_error(None)
    assert lib.prt_upload_scene(None, None) == -1
    assert lib.prt_render(None, None, None, 1, 1, 0, 1, None, None) == -1
    assert lib.prt_shard_rows(1080, 8, 0, 0) == 0 and lib.prt_shard_rows(1080, 0, 0, 1) == 0
    # the n-device handle and the option call: null handles are errors, never crashes
    import ctypes as C
    assert not lib.prt_multi_create(None, 0)
    assert b"no devices" in lib.prt_multi_last_error(None)
    if not torch.cuda.is_available():
        assert not lib.prt_multi_create((C.c_int * 2)(0, 1), 2)
        assert b"no HIP device" in lib.prt_multi_last_error(None)
    assert lib.prt_multi_device_count(None) == 0 and not lib.prt_multi_context(None, 0)
    assert lib.prt_multi_upload_scene(None, None) == -1
    assert lib.prt_multi_render(None, None, None, 1, 1, None, None) == -1
    lib.prt_multi_destroy(None)
    assert lib.prt_set_option(None, b"STACK_CAP", b"2") == -1
    assert lib.prt_build_flags() & ~capi.BUILD_BVH4 == 0
    # the two-deep form of the n-device handle
    assert lib.prt_multi_depth(None) == 0
    assert lib.prt_multi_submit(None, None, None, 1, 1, None, None) == -1
    assert lib.prt_multi_wait(None, 1, None) == -1


def test_no_cpp_exception_leaves_an_entry_point():
    """include/prt.h: "nothing aborts".  The libraries are C++ (std::vector, std::string, std::thread, new) behind extern "C":
    an exception that left an entry point would be std::terminate in the CALLER's process - round 3 lost a GPU test run to an
    abort whose message pytest's capture swallowed.  Every entry point that can allocate now runs under a
    guard; the hook throws inside one - std::bad_alloc, a REAL std::length_error from a vector asked for more than max_size,
    std::runtime_error, a non-std exception - and must come back with PRT_ERR_EXCEPTION (-12) and a message, in both
    libraries.  Run in a child process as well: if the guard were missing this is the test that would abort."""
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from par_raytracer_amd import capi\n"
            "hip, host = capi.hip_lib(), capi.host_lib()\n"
            "host.prt_host_last_error.restype = __import__('ctypes').c_char_p\n"
            "for kind, word in ((1, b'bad_alloc'), (2, b'C++ exception'), (3, b'thrown on request'), (4, b'unknown C++ exception')):\n"
            "    assert hip.prt_debug_throw(None, kind) == -12, kind\n"
            "    assert word in hip.prt_last_error(None), (kind, hip.prt_last_error(None))\n"
            "    assert host.prt_host_debug_throw(kind) == -12, kind\n"
            "    assert word in host.prt_host_last_error(), (kind, host.prt_host_last_error())\n"
            "assert hip.prt_debug_throw(None, 0) == 0 and host.prt_host_debug_throw(0) == 0\n"
            "print('guarded')\n") % ROOT
    out = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert out.returncode == 0 and b"guarded" in out.stdout, (out.returncode, out.stderr.decode()[-2000:])
    # and in this process
    lib = capi.hip_lib()
    assert lib.prt_debug_throw(None, 1) == -12 and b"bad_alloc" in lib.prt_last_error(None)


def test_every_extern_c_function_with_a_body_is_guarded():
    """Source-level check that goes with the test above: in csrc/prt_api.hip and host/host_capi.cpp every extern "C" function
    whose body is more than a one-line accessor opens with the guard macro."""
    def bodies(path, prefix):
        text = open(path).read()
        out = {}
        for m in re.finditer(r"^[A-Za-z_][\w \*]*\b(%s\w+)\(" % prefix, text, flags=re.M):
            i = text.index("(", m.start())
            depth = 0
            while True:
                depth += {"(": 1, ")": -1}.get(text[i], 0)
                if depth == 0:
                    break
                i += 1
            rest = text[i + 1:].lstrip()
            if not rest.startswith("{"):
                continue                                        # a declaration
            out[m.group(1)] = rest[1:200]
        return out
    hip = bodies(os.path.join(ROOT, "par_raytracer_amd", "csrc", "prt_api.hip"), "prt_")
    host = bodies(os.path.join(ROOT, "par_raytracer_amd", "host", "host_capi.cpp"), "prt_host_")
    accessors = {"prt_abi_version", "prt_build_flags", "prt_last_error", "prt_shard_rows", "prt_multi_last_error", "prt_multi_device_count",
                 "prt_multi_depth", "prt_multi_context", "prt_host_last_error", "prt_host_scene_desc", "prt_host_scene_id",
                 "prt_host_scene_hierarchy_seconds", "prt_host_scene_parse_seconds", "prt_host_free_texture"}
    assert len(hip) >= 24 and len(host) >= 8
    for name, body in list(hip.items()) + list(host.items()):
        if name in accessors:
            continue
        assert body.lstrip().startswith(("PRT_API_TRY", "HOST_API_TRY")), "%s has no exception guard" % name


def test_shard_rows_partition_the_frame():
    lib = capi.hip_lib()
    for h, br, n in ((1080, 8, 8), (1080, 8, 3), (17, 8, 2), (5, 8, 8), (2160, 8, 8), (100, 7, 4)):
        rows = [lib.prt_shard_rows(h, br, r, n) for r in range(n)]
        assert sum(rows) == h
        # python mirror of the block walk used by bench.py
        for r in range(n):
            mine, b = 0, r
            while b * br < h:
                mine += min(br, h - b * br)
                b += n
            assert mine == rows[r]


# ---- loader + hierarchy against the reference's parse of the same files ------------------------------------

def _load_texture(lib, path):
    """prt_host_load_texture -> uint8 array [h, w, c] or None."""
    import ctypes as C
    sx, sy, ch = C.c_uint32(), C.c_uint32(), C.c_uint32()
    ptr = lib.prt_host_load_texture(path.encode(), C.byref(sx), C.byref(sy), C.byref(ch))
    if not ptr:
        return None
    out = np.ctypeslib.as_array(ptr, shape=(sy.value, sx.value, ch.value)).copy()
    lib.prt_host_free_texture(ptr)
    return out


def _sums(a):
    a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    return np.array([a.size, int(a.astype(np.uint64).sum()),
                     int((a.astype(np.uint64) * (np.arange(a.size, dtype=np.uint64) % 251 + 1)).sum() % (1 << 62))], dtype=np.uint64)


@pytest.mark.parametrize("name", ["c1_sphere_plane_256", "c2_cornell_128", "icosphere_l3_two_lights", "terrain64_d3",
                                  "terrain192_d2", "c3_icosphere_1080p_l24"])
def test_loader_and_hierarchy_bit_identical_to_reference(name):
    g = load_golden(name)
    hs = host_scene(str(g["scene"]), int(g["light_mode"]))
    a = hs.arrays()
    for k in ("positions", "texcoords", "normals", "idx_positions", "idx_texcoords", "idx_normals"):
        assert np.array_equal(_sums(a[k]), g["sum_" + k]), k
    assert np.array_equal(a["spheres"].view(np.uint32), g["spheres"].view(np.uint32)), "sphere tree differs from the reference"
    assert np.array_equal(a["sphere_children"], g["sphere_children"])
    assert np.array_equal(a["sphere_group"], g["sphere_group"])
    assert np.array_equal(a["groups"][:, 1].astype(np.uint32), g["group_index_counts"])
    assert hs.n_tris == int(g["triangles"])


def test_texture_decoders_and_tangents_bit_identical_to_reference():
    """Row N1: the 14 texture files of the gallery scene (8/16-bit PNG in grey, RGB, RGBA, palette, palette + tRNS
    with all five scanline filters and split IDAT; TGA raw / run-length / top-down, grey / BGR / BGRA; 24-bit BMP;
    binary PGM / PPM) decode to the bytes the reference's decoder produced, the height maps convert to the same
    normal maps (texture.cpp:102-143) and CalculateTangents (mesh.h:59-130) gives the same vectors."""
    g = load_golden("gallery_160x120")
    hs = host_scene("textured_gallery")
    a = hs.arrays()
    assert np.array_equal(a["group_texture_dims"], g["group_texture_dims"])
    assert np.array_equal(_sums(a["group_texture_bytes"]), g["sum_group_texture_bytes"])
    assert np.array_equal(_sums(a["tangents"]), g["sum_tangents"])
    assert np.abs(a["tangents"]).sum() > 100.0, "floor and ball have real tangents"
    for k in ("positions", "texcoords", "normals", "idx_positions", "idx_texcoords", "idx_normals"):
        assert np.array_equal(_sums(a[k]), g["sum_" + k]), k
    dims = a["group_texture_dims"].reshape(-1, 5, 3)
    assert (dims[:, :, 0] > 0).sum() == 14 and set(np.unique(dims[:, :, 2])) == {0, 1, 2, 3, 4}


def test_jpeg_decoder_bit_identical_to_reference():
    """The 16 JPEG files of the jpeg_gallery scene - baseline grey, 4:4:4, 4:2:2, 4:4:0, 4:2:0, 4:1:1, restart intervals,
    one scan per component, RGB component ids; progressive (spectral selection + successive approximation, ten scans)
    4:4:4, 4:2:0, 4:2:2 with restarts, grey; sizes that are not multiples of the MCU - decode to the bytes the
    reference's decoder produced (its inverse DCT, chroma upsampling filter and YCbCr arithmetic), grey files to 1
    channel, colour files to 3; the bump map converts to the same normal map."""
    g = load_golden("jpeg_gallery_128x96")
    hs = host_scene("jpeg_gallery")
    a = hs.arrays()
    assert np.array_equal(a["group_texture_dims"], g["group_texture_dims"])
    assert np.array_equal(_sums(a["group_texture_bytes"]), g["sum_group_texture_bytes"])
    dims = a["group_texture_dims"].reshape(-1, 5, 3)
    assert (dims[:, :, 0] > 0).sum() == 16 and set(np.unique(dims[:, :, 2])) == {0, 1, 3}


def test_png_corner_cases_bit_identical_to_reference():
    """The 13 files of the png_gallery scene - Adam7 interlaced 8- and 16-bit, 1 / 2 / 4-bit grey (scaled to 0..255), 4- and
    1-bit palettes (one with tRNS, interlaced), colour-key tRNS on grey / RGB / 16-bit RGB / 2-bit grey - decode to the
    bytes AND the channel counts the reference's decoder reported."""
    g = load_golden("png_gallery_128x96")
    hs = host_scene("png_gallery")
    a = hs.arrays()
    assert np.array_equal(a["group_texture_dims"], g["group_texture_dims"])
    assert np.array_equal(_sums(a["group_texture_bytes"]), g["sum_group_texture_bytes"])
    dims = a["group_texture_dims"].reshape(-1, 5, 3)
    assert (dims[:, :, 0] > 0).sum() == 13 and set(np.unique(dims[:, :, 2])) == {0, 1, 3, 4}


def test_bmp_flavours_bit_identical_to_reference():
    """The 12 files of the bmp_gallery scene - 24-bit bottom-up / top-down, OS/2 headers, 8- and 4-bit palettes, 16-bit
    5-5-5 and 5-6-5 BITFIELDS (read twelve bytes late, like the reference's decoder does), 32-bit with a real and with an
    all-zero alpha channel, a 108-byte header with A-R-G-B masks - decode to the reference's bytes and channel counts."""
    g = load_golden("bmp_gallery_128x96")
    hs = host_scene("bmp_gallery")
    a = hs.arrays()
    assert np.array_equal(a["group_texture_dims"], g["group_texture_dims"])
    assert np.array_equal(_sums(a["group_texture_bytes"]), g["sum_group_texture_bytes"])
    dims = a["group_texture_dims"].reshape(-1, 5, 3)
    assert (dims[:, :, 0] > 0).sum() == 12 and set(np.unique(dims[:, :, 2])) == {0, 3, 4}


def test_tga_corner_cases_bit_identical_to_reference_and_round_trip(tmp_path):
    """The 8 files of the tga_gallery scene - 5-5-5 pixels raw and run-length, 16-bit grey + alpha, colour maps with 24-,
    32- and 15-bit entries, 16-bit indices, image ids, non-zero first-entry fields - decode to the reference's bytes; and
    every flavour returns what was written (5-5-5 as c * 255 / 31)."""
    g = load_golden("tga_gallery_128x96")
    hs = host_scene("tga_gallery")
    a = hs.arrays()
    assert np.array_equal(a["group_texture_dims"], g["group_texture_dims"])
    assert np.array_equal(_sums(a["group_texture_bytes"]), g["sum_group_texture_bytes"])
    dims = a["group_texture_dims"].reshape(-1, 5, 3)
    assert (dims[:, :, 0] > 0).sum() == 8 and set(np.unique(dims[:, :, 2])) == {0, 2, 3, 4}
    from par_raytracer_amd import scenes
    lib = capi.host_lib()
    rng = np.random.default_rng(12)
    rgb = rng.integers(0, 256, size=(9, 11, 3), dtype=np.uint8)
    rgb[2:5, 3:9] = rgb[2, 3]
    few = (rng.integers(0, 3, size=(9, 11, 3), dtype=np.uint8) * 100 + 20).astype(np.uint8)
    few[4:7, 2:8] = few[4, 2]
    few_a = np.concatenate([few, few[:, :, :1] // 2 + 60], axis=2).astype(np.uint8)
    ga = rng.integers(0, 256, size=(9, 11, 2), dtype=np.uint8)
    q = (rgb >> 3).astype(np.uint32)
    for enc, img, expect in (("tga16", rgb, (q * 255 // 31).astype(np.uint8)), ("tga16_rle", rgb, (q * 255 // 31).astype(np.uint8)), ("tga_ga", ga, ga),
                             ("tga_map24", few, few), ("tga_map32_rle", few_a, few_a), ("tga_map24_i16", rgb, rgb),
                             ("tga_map16", few, ((few >> 3).astype(np.uint32) * 255 // 31).astype(np.uint8))):
        path = str(tmp_path / ("t_%s.tga" % enc))
        texture_fixtures.write_texture(path, img, enc)
        got = _load_texture(lib, path)
        assert got is not None and got.shape == expect.shape and np.array_equal(got, expect), enc


def test_gif_bit_identical_to_reference_and_round_trip(tmp_path):
    """The 7 files of the gif_gallery scene decode to the reference's bytes: always RGBA, the first image on the logical
    screen, background and transparent pixels with alpha 0, interlaced rows back in place, local colour tables, an LZW
    stream long enough to fill the code table.  And what was written comes back."""
    g = load_golden("gif_gallery_128x96")
    hs = host_scene("gif_gallery")
    a = hs.arrays()
    assert np.array_equal(a["group_texture_dims"], g["group_texture_dims"])
    assert np.array_equal(_sums(a["group_texture_bytes"]), g["sum_group_texture_bytes"])
    dims = a["group_texture_dims"].reshape(-1, 5, 3)
    assert (dims[:, :, 0] > 0).sum() == 7 and set(np.unique(dims[:, :, 2])) == {0, 4}
    from par_raytracer_amd import scenes
    lib = capi.host_lib()
    rng = np.random.default_rng(5)
    img = (rng.integers(0, 6, size=(23, 31, 3)) * 45 + 10).astype(np.uint8)
    img[5:12, 4:20] = img[0, 0]
    key = (img == img[0, 0]).all(axis=2)
    for enc in ("gif", "gif_i", "gif_t", "gif_local_i_t"):
        path = str(tmp_path / ("t_%s.gif" % enc))
        texture_fixtures.write_texture(path, img, enc)
        got = _load_texture(lib, path)
        assert got is not None and got.shape == (23, 31, 4), enc
        if "t" in enc.split("_", 1)[-1] and enc != "gif_i":
            assert np.array_equal(got[:, :, :3][~key], img[~key]) and np.all(got[:, :, 3][~key] == 255) and np.all(got[:, :, 3][key] == 0), enc
        else:
            assert np.array_equal(got[:, :, :3], img) and np.all(got[:, :, 3] == 255), enc
    path = str(tmp_path / "canvas.gif")
    texture_fixtures.write_texture(path, img, "gif_canvas")
    got = _load_texture(lib, path)
    assert got is not None and got.shape == (28, 38, 4)
    assert np.array_equal(got[2:25, 3:34, :3], img) and np.all(got[2:25, 3:34, 3] == 255)
    outside = np.ones((28, 38), dtype=bool)
    outside[2:25, 3:34] = False
    assert np.all(got[:, :, 3][outside] == 0)


def test_psd_bit_identical_to_reference_and_round_trip(tmp_path):
    """The 6 composites of the psd_gallery scene (raw / PackBits, 16-bit, RGBA with every alpha value) decode to the
    reference's bytes - always four channels, colours un-blended from the white matte in float - and opaque / fully
    transparent pixels come back as written."""
    g = load_golden("psd_gallery_128x96")
    hs = host_scene("psd_gallery")
    a = hs.arrays()
    assert np.array_equal(a["group_texture_dims"], g["group_texture_dims"])
    assert np.array_equal(_sums(a["group_texture_bytes"]), g["sum_group_texture_bytes"])
    from par_raytracer_amd import scenes
    lib = capi.host_lib()
    rng = np.random.default_rng(5)
    rgb = rng.integers(0, 256, size=(9, 13, 3), dtype=np.uint8)
    rgb[3:6, 2:11] = rgb[3, 2]
    rgba = np.concatenate([rgb, np.where(rng.integers(0, 2, size=(9, 13, 1)) > 0, 255, 0).astype(np.uint8)], axis=2)
    for enc, img in (("psd", rgb), ("psd_rle", rgb), ("psd16", rgb), ("psd", rgba), ("psd_rle", rgba)):
        path = str(tmp_path / ("t_%s.psd" % enc))
        texture_fixtures.write_texture(path, img, enc)
        got = _load_texture(lib, path)
        assert got is not None and got.shape == (9, 13, 4) and np.array_equal(got[:, :, :img.shape[2]], img), enc
        if img.shape[2] == 3:
            assert np.all(got[:, :, 3] == 255)


def test_hdr_bit_identical_to_reference(tmp_path):
    """The 5 Radiance files of the hdr_gallery scene (run-length scanlines, flat pixels in a wide file, a file narrower
    than 8 pixels, zero exponents, several decades of radiance) come back as the reference's decoder tone-maps them:
    three channels, pow(v, 1 / 2.2) x 255 + 0.5 truncated.  A written picture comes back within the RGBE mantissa's
    precision of the analytic tone map."""
    g = load_golden("hdr_gallery_128x96")
    hs = host_scene("hdr_gallery")
    a = hs.arrays()
    assert np.array_equal(a["group_texture_dims"], g["group_texture_dims"])
    assert np.array_equal(_sums(a["group_texture_bytes"]), g["sum_group_texture_bytes"])
    from par_raytracer_amd import scenes
    lib = capi.host_lib()
    yy, xx = np.mgrid[0:12, 0:20]
    rad = np.stack([0.02 + xx / 10.0, 0.5 + 0.4 * np.sin(yy * 0.9), np.full(xx.shape, 0.25)], axis=2)
    want = (np.clip(rad, 0, None) ** (1 / 2.2) * 255 + 0.5).clip(0, 255)
    for enc in ("hdr", "hdr_flat"):
        path = str(tmp_path / ("t_%s.hdr" % enc))
        texture_fixtures.write_texture(path, rad, enc)
        got = _load_texture(lib, path)
        assert got is not None and got.shape == (12, 20, 3), enc
        assert np.abs(got.astype(np.float64) - want).max() <= 5.0, enc         # the 8-bit shared-exponent mantissa truncates


def test_pic_bit_identical_to_reference_and_round_trip(tmp_path):
    """The 7 Softimage files of the pic_gallery scene (raw, pure and mixed run-length packets, a separate alpha packet, a
    300-pixel run with a 16-bit count) decode to the reference's bytes and channel counts; what was written comes back."""
    g = load_golden("pic_gallery_128x96")
    hs = host_scene("pic_gallery")
    a = hs.arrays()
    assert np.array_equal(a["group_texture_dims"], g["group_texture_dims"])
    assert np.array_equal(_sums(a["group_texture_bytes"]), g["sum_group_texture_bytes"])
    from par_raytracer_amd import scenes
    lib = capi.host_lib()
    rng = np.random.default_rng(5)
    rgb = rng.integers(0, 256, size=(9, 300, 3), dtype=np.uint8)
    rgb[3:6, 2:290] = rgb[3, 2]
    rgba = np.concatenate([rgb, rng.integers(0, 256, size=(9, 300, 1), dtype=np.uint8)], axis=2)
    rgba[4, :, 3] = 77
    for enc in ("pic", "pic_raw", "pic_pure"):
        for img in (rgb, rgba):
            path = str(tmp_path / ("t_%s_%d.pic" % (enc, img.shape[2])))
            texture_fixtures.write_texture(path, img, enc)
            got = _load_texture(lib, path)
            assert got is not None and got.shape == img.shape and np.array_equal(got, img), (enc, img.shape)


def test_bmp_flavours_round_trip(tmp_path):
    """What was written comes back: exactly for palettes, 24- and 32-bit; within the 5-bit quantisation (top bits repeated
    into the low ones) for 16-bit 5-5-5; a 32-bit file whose alpha bytes are all 0 comes back opaque."""
    from par_raytracer_amd import scenes
    lib = capi.host_lib()
    rng = np.random.default_rng(8)
    rgb = rng.integers(0, 256, size=(9, 7, 3), dtype=np.uint8)
    rgba = np.concatenate([rgb, rng.integers(1, 256, size=(9, 7, 1), dtype=np.uint8)], axis=2)
    few = (rng.integers(0, 2, size=(9, 7, 3), dtype=np.uint8) * 200 + 20).astype(np.uint8)
    for enc, img in (("bmp", rgb), ("bmp_top", rgb), ("bmp_os2", rgb), ("bmp_os2_8", few), ("bmp8", few), ("bmp4", few), ("bmp32", rgba), ("bmp32_v4", rgba)):
        path = str(tmp_path / ("t_%s.bmp" % enc))
        texture_fixtures.write_texture(path, img, enc)
        got = _load_texture(lib, path)
        assert got is not None and got.shape == img.shape and np.array_equal(got, img), enc
    path = str(tmp_path / "t16.bmp")
    texture_fixtures.write_texture(path, rgb, "bmp16")
    got = _load_texture(lib, path)
    q = rgb >> 3
    assert got is not None and np.array_equal(got, ((q << 3) | (q >> 2)).astype(np.uint8))
    texture_fixtures.write_texture(path, rgb, "bmp32")                          # alpha bytes all 0
    got = _load_texture(lib, path)
    assert got is not None and got.shape == (9, 7, 4) and np.array_equal(got[:, :, :3], rgb) and np.all(got[:, :, 3] == 255)


def test_png_variants_round_trip_with_every_filter(tmp_path):
    """Adam7, sub-byte depths and colour keys against what was written, at sizes that leave interlace passes empty, with
    all five scanline filters (the fixture above can only use None / Sub on sub-byte images: the reference's decoder reads
    the previous row of those at the wrong offset).  A colour key comes back the way the reference's decoder hands it
    over: the (channels + 1)-interleaved pixels cut off at width x height x channels bytes (image_in.cpp DecodePng)."""
    from par_raytracer_amd import scenes
    lib = capi.host_lib()
    rng = np.random.default_rng(3)
    allf = (0, 1, 2, 3, 4)

    def check(img, expect, **kw):
        path = str(tmp_path / "v.png")
        texture_fixtures.write_png(path, img, filters=allf, **kw)
        got = _load_texture(lib, path)
        assert got is not None and got.shape == expect.shape and np.array_equal(got, expect), (img.shape, kw)

    def keyed(expect_with_alpha):                                       # what the reference sees of an image with a colour key
        h, w, c1 = expect_with_alpha.shape
        return expect_with_alpha.reshape(-1)[:h * w * (c1 - 1)].reshape(h, w, c1 - 1)

    for hh, ww in ((13, 7), (1, 1), (3, 5), (9, 1), (2, 17), (8, 8), (16, 33)):
        rgb = rng.integers(0, 256, size=(hh, ww, 3), dtype=np.uint8)
        rgba = rng.integers(0, 256, size=(hh, ww, 4), dtype=np.uint8)
        check(rgb, rgb, interlace=True)
        check(rgba, rgba, interlace=True, sixteen_bit=True)
        for bits, scale in ((1, 255), (2, 85), (4, 17)):
            gl = rng.integers(0, 1 << bits, size=(hh, ww), dtype=np.uint8)
            for il in (False, True):
                check(gl, (gl * scale)[:, :, None].astype(np.uint8), bits=bits, interlace=il)
            k = np.stack([gl * scale, np.where(gl == gl[0, 0], 0, 255)], axis=2).astype(np.uint8)
            check(gl, keyed(k), bits=bits, key=[int(gl[0, 0])])
        p4 = (rng.integers(0, 2, size=(hh, ww, 3), dtype=np.uint8) * 120 + 7).astype(np.uint8)          # 8 colours
        check(p4, p4, palette=True, bits=4, interlace=True)
        p1 = np.where(rng.integers(0, 2, size=(hh, ww, 1)) > 0, np.array([10, 200, 30, 128], dtype=np.uint8),
                      np.array([250, 0, 90, 255], dtype=np.uint8)).astype(np.uint8)
        if len(np.unique(p1.reshape(-1, 4), axis=0)) == 2:
            check(p1, p1, palette=True, palette_alpha=True, bits=1)
        ka = np.concatenate([rgb, np.where((rgb == rgb[0, 0]).all(axis=2, keepdims=True), 0, 255).astype(np.uint8)], axis=2)
        check(rgb, keyed(ka), key=rgb[0, 0])
        check(rgb, keyed(ka), key=rgb[0, 0], sixteen_bit=True, interlace=True)


def test_jpeg_files_decode_close_to_what_was_encoded(tmp_path):
    """texture_fixtures.write_jpeg is a real (lossy) encoder: what comes back is the picture that went in, within the quantisation
    error, for every layout - so the bit-identity test above is about pictures, not about noise."""
    from par_raytracer_amd import scenes
    lib = capi.host_lib()
    yy, xx = np.mgrid[0:45, 0:70]
    img = np.stack([128 + 100 * np.sin(xx * 0.21) * np.cos(yy * 0.17), 128 + 90 * np.cos(yy * 0.3), 40 + 2.5 * xx], axis=2).clip(0, 255).astype(np.uint8)
    for enc in ("jpg", "jpg422", "jpg440", "jpg420", "jpg411", "jpg420_rst", "jpg_scans", "jpg_rgb", "jpg_prog", "jpg_prog420", "jpg_prog422_rst"):
        path = str(tmp_path / ("t_%s.jpg" % enc))
        texture_fixtures.write_texture(path, img, enc)
        got = _load_texture(lib, path)
        assert got is not None and got.shape == img.shape, enc
        err = np.abs(got.astype(np.int32) - img.astype(np.int32))
        assert err.mean() < 6.0 and np.percentile(err, 99) < 40, (enc, err.mean(), err.max())
    path = str(tmp_path / "grey.jpg")
    for enc in ("jpg", "jpg_prog"):
        texture_fixtures.write_texture(path, img[:, :, 0], enc)
        got = _load_texture(lib, path)
        assert got is not None and got.shape == (45, 70, 1), enc
        assert np.abs(got[:, :, 0].astype(np.int32) - img[:, :, 0].astype(np.int32)).mean() < 4.0, enc


def test_texture_writers_round_trip_through_the_loader(tmp_path):
    """Every encoding of texture_fixtures.write_texture decodes to the array that was written (16-bit PNG keeps the high
    byte; palette images come back as RGB / RGBA)."""
    from par_raytracer_amd import scenes
    rng = np.random.default_rng(5)
    lib = capi.host_lib()
    cases = [("png", 1), ("png", 2), ("png", 3), ("png", 4), ("png16", 1), ("png16", 3), ("png16", 4), ("tga", 1), ("tga", 3),
             ("tga", 4), ("tga_top", 3), ("tga_rle", 1), ("tga_rle", 3), ("tga_rle", 4), ("bmp", 3), ("pnm", 1), ("pnm", 3)]
    for enc, ch in cases:
        img = rng.integers(0, 256, size=(13, 7, ch), dtype=np.uint8)
        img[3:9, 1:6] = img[3, 1]                                   # runs, so the run-length packets are exercised
        path = str(tmp_path / ("t_%s_%d.img" % (enc, ch)))
        texture_fixtures.write_texture(path, img, enc)
        got = _load_texture(lib, path)
        assert got is not None, (enc, ch)
        assert got.shape == img.shape and np.array_equal(got, img), (enc, ch)
    few = (rng.integers(0, 4, size=(9, 11, 4), dtype=np.uint8) * 80).astype(np.uint8)
    for enc, ch in (("png_palette", 3), ("png_palette_alpha", 4)):
        path = str(tmp_path / ("p_%s.png" % enc))
        texture_fixtures.write_texture(path, few[:, :, :ch], enc)
        got = _load_texture(lib, path)
        assert got is not None and np.array_equal(got, few[:, :, :ch]), enc


def test_unsupported_images_leave_the_slot_empty_like_a_decoder_failure(tmp_path):
    """obj_parser.cpp:201-204: a file the decoder rejects prints a message and yields no texture.  Same here for
    arithmetic-coded JPEG, truncated files and missing files - no crash, and the material simply has no map."""
    lib = capi.host_lib()
    bad = tmp_path / "x.jpg"
    bad.write_bytes(b"\xff\xd8\xff\xe0" + b"\0" * 64)
    assert _load_texture(lib, str(bad)) is None
    from par_raytracer_amd import scenes as _scenes
    prog = tmp_path / "arithmetic.jpg"
    texture_fixtures.write_texture(str(prog), np.full((16, 16, 3), 90, dtype=np.uint8), "jpg")
    raw = bytearray(prog.read_bytes())
    raw[raw.index(b"\xff\xc0") + 1] = 0xC9                    # SOF0 -> SOF9: arithmetic coding, which the reference's decoder rejects too
    prog.write_bytes(bytes(raw))
    assert _load_texture(lib, str(prog)) is None
    cut = tmp_path / "cut.jpg"
    texture_fixtures.write_texture(str(cut), np.full((24, 24, 3), 90, dtype=np.uint8), "jpg420")
    cut.write_bytes(cut.read_bytes()[:150])
    assert _load_texture(lib, str(cut)) is None
    trunc = tmp_path / "t.png"
    from par_raytracer_amd import scenes
    texture_fixtures.write_texture(str(trunc), np.zeros((8, 8, 3), dtype=np.uint8), "png")
    trunc.write_bytes(trunc.read_bytes()[:40])
    assert _load_texture(lib, str(trunc)) is None
    assert _load_texture(lib, str(tmp_path / "missing.tga")) is None
    # a material whose map is missing still loads, untextured
    (tmp_path / "scene.obj").write_text("mtllib scene.mtl\nv 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nvn 0 0 1\ng a\nusemtl m\nf 1/1/1 2/1/1 3/1/1\n")
    (tmp_path / "scene.mtl").write_text("newmtl m\nd 1\nKd 1 1 1\nmap_Kd nothing.png\nmap_bump nothing.tga\n")
    hs = api.HostScene(str(tmp_path), "scene.obj")
    assert hs.desc.contents.texture_count == 0 and hs.n_tris == 1


def test_malformed_obj_and_image_files_fail_cleanly(tmp_path):
    """Found by fuzzing the loader under AddressSanitizer (tools/fuzz_obj_loader.py, tools/fuzz_image_decoders.py): face
    indices past the vertex arrays (a wild read in the reference's CalculateTangents / BuildHierarchy), a face record cut
    off at the end of the file, an image header that promises 4 Gpixels."""
    base = "v 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nvn 0 0 1\ng a\n"
    (tmp_path / "range.obj").write_text(base + "f 1/1/1 2/1/1 9/1/1\n")
    with pytest.raises(RuntimeError):
        api.HostScene(str(tmp_path), "range.obj")
    (tmp_path / "cut.obj").write_text(base + "f 1/1/1 2/1/1 3/1/1\nf 1/1/1 2/1/1 3/")           # no newline, truncated corner
    hs = api.HostScene(str(tmp_path), "cut.obj")
    assert hs.n_tris == 1
    (tmp_path / "later.obj").write_text("vt 0 0\nvn 0 0 1\ng a\nf 1/1/1 2/1/1 3/1/1\nv 0 0 0\nv 1 0 0\nv 0 1 0\n")   # vertices after the face: fine
    assert api.HostScene(str(tmp_path), "later.obj").n_tris == 1
    png = bytearray()
    texture_fixtures.write_texture(str(tmp_path / "ok.png"), np.zeros((4, 4, 3), dtype=np.uint8), "png")
    png = bytearray((tmp_path / "ok.png").read_bytes())
    png[16:24] = b"\xff\xff\xff\xf0\xff\xff\xff\xf0"                                            # IHDR width / height
    (tmp_path / "huge.png").write_bytes(bytes(png))
    assert _load_texture(capi.host_lib(), str(tmp_path / "huge.png")) is None
    tga = bytearray(18); tga[2] = 10; tga[12:16] = b"\xff\xff\xff\xff"; tga[16] = 24                  # 65535 x 65535 run-length TGA, no data
    (tmp_path / "huge.tga").write_bytes(bytes(tga))
    assert _load_texture(capi.host_lib(), str(tmp_path / "huge.tga")) is None


def test_loader_matches_generator_arrays():
    s, d = scene_dir("cornell_box")
    hs = host_scene("cornell_box")
    a = hs.arrays()
    assert np.array_equal(a["positions"], s.positions) and np.array_equal(a["normals"], s.normals)
    faces = np.concatenate([g.faces for g in s.groups]).reshape(-1, 3)
    assert np.array_equal(a["idx_positions"], faces[:, 0].astype(np.uint32))
    # material 0 is the scene default (main.cpp:579), MTL materials follow in first-use order
    m = a["materials"]
    assert np.allclose(m[0, :3], [10.0, 1.5, 1.0]) and np.allclose(m[0, 3:7], [0.75, 0.5, 0.75, 1.0])
    names = [g.material for g in s.groups]
    by_name = {mm.name: mm for mm in s.materials}
    for gi, nm in enumerate(names):
        row = m[a["groups"][gi, 2]]
        assert np.allclose(row[:3], [by_name[nm].Ns, by_name[nm].Ni, by_name[nm].d])
        assert np.allclose(row[7:10], by_name[nm].Kd)


def test_obj_quirks(tmp_path):
    """Format behaviour of obj_parser.cpp the loader preserves."""
    (tmp_path / "q.mtl").write_text("newmtl a\nNs 5\nNi 1.2\nd 0.5\nKa 1 0 0\nKd 0 1 0\nKs 0 0 1\n\nnewmtl b\nKd 0.5 0.5 0.5\n")
    (tmp_path / "q.obj").write_text(
        "mtllib q.mtl\nv 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nv 0 0 1\nvt 0 0\nvn 0 0 1\n"
        "g quad\nusemtl a\nf 1/1/1 2/1/1 3/1/1 4/1/1\n"          # 4 corners -> fan of 2 triangles
        "usemtl b\nf -5/-1/-1 -4/-1/-1 -1/-1/-1\n"                # second usemtl splits the group; negative = relative
        "g nomat\nf 1/1/1 2/1/1 5/1/1\n")
    hs = api.HostScene(str(tmp_path), "q.obj")
    a = hs.arrays()
    assert hs.n_tris == 4
    assert a["groups"].shape[0] == 3                                    # quad, quad (split), nomat
    assert list(a["idx_positions"][:6]) == [0, 1, 2, 0, 2, 3]           # fan around corner 0
    assert list(a["idx_positions"][6:9]) == [0, 1, 4]                   # -5,-4,-1 of 5 positions
    m = a["materials"]
    mat_a = m[a["groups"][0, 2]]
    mat_b = m[a["groups"][1, 2]]
    assert np.allclose(mat_a[:3], [5, 1.2, 0.5]) and np.allclose(mat_a[3:7], [1, 0, 0, 1])
    assert np.allclose(mat_b[:3], [0, 0, 0]), "materials start zeroed: missing d means alpha 0 (obj_parser.cpp:255)"
    assert a["groups"][2, 2] == 0                                        # group without usemtl -> default material


def test_missing_file_is_an_error_not_a_crash(tmp_path):
    with pytest.raises(RuntimeError):
        api.HostScene(str(tmp_path), "does_not_exist.obj")


# ---- acceleration structure (host-only check of what upload builds) -----------------------------------------

@pytest.mark.parametrize("name", ["cornell_box", "sphere_plane", "icosphere_l3", "terrain_64", "terrain_192"])
def test_bvh_is_conservative_and_complete(name):
    hs = host_scene(name)
    out = (C.c_uint64 * 6)()
    assert capi.hip_lib().prt_debug_check_bvh(hs.desc, out) == 0
    violations, nodes, depth, bound, leaves, refs = list(out)
    assert violations == 0
    assert refs == hs.n_tris and leaves >= hs.n_tris / 4
    bvh4 = bool(capi.hip_lib().prt_build_flags() & capi.BUILD_BVH4)
    assert bound == (3 * depth + 2 if bvh4 else depth + 2)      # 4-wide: three links per level; 8-wide: one group per level


@pytest.mark.parametrize("name", ["cornell_box", "icosphere_l3", "terrain_64", "textured_gallery"])
def test_area_optimal_collapse_is_conservative_and_smaller(name, monkeypatch):
    """PRT_BVH_COLLAPSE=dp: same leaves, every triangle still inside every ancestor's box, never more wide nodes than the
    greedy collapse of the same binary tree."""
    hs = host_scene(name)
    out = (C.c_uint64 * 6)()
    monkeypatch.setenv("PRT_BVH_COLLAPSE", "greedy")
    assert capi.hip_lib().prt_debug_check_bvh(hs.desc, out) == 0
    greedy = list(out)
    assert greedy[0] == 0
    monkeypatch.setenv("PRT_BVH_COLLAPSE", "dp")
    assert capi.hip_lib().prt_debug_check_bvh(hs.desc, out) == 0
    violations, nodes, depth, bound, leaves, refs = list(out)
    assert violations == 0 and refs == hs.n_tris
    assert leaves == greedy[4] and nodes <= greedy[1]


def test_bvh_degenerate_scenes(tmp_path):
    # one triangle, and many coincident triangles (all centroids equal -> median splits)
    (tmp_path / "one.obj").write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nvn 0 0 1\ng t\nf 1/1/1 2/1/1 3/1/1\n")
    lines = "v 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nvn 0 0 1\ng t\n" + "f 1/1/1 2/1/1 3/1/1\n" * 37
    (tmp_path / "many.obj").write_text(lines)
    for f, n in (("one.obj", 1), ("many.obj", 37)):
        hs = api.HostScene(str(tmp_path), f)
        out = (C.c_uint64 * 6)()
        assert capi.hip_lib().prt_debug_check_bvh(hs.desc, out) == 0
        assert out[0] == 0 and out[5] == n


# ---- tone map + PNG -------------------------------------------------------------------------------------------

def _decode_png(path):
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    off, chunks = 8, {}
    idat = b""
    while off < len(data):
        n, tag = struct.unpack(">I4s", data[off:off + 8])
        body = data[off + 8:off + 8 + n]
        crc, = struct.unpack(">I", data[off + 8 + n:off + 12 + n])
        assert crc == (zlib.crc32(tag + body) & 0xFFFFFFFF)
        if tag == b"IDAT":
            idat += body
        chunks[tag] = body
        off += 12 + n
    w, h, depth, ctype = struct.unpack(">IIBB", chunks[b"IHDR"][:10])
    raw = zlib.decompress(idat)
    rows = [raw[(w * 4 + 1) * y + 1:(w * 4 + 1) * (y + 1)] for y in range(h)]
    assert all(raw[(w * 4 + 1) * y] == 0 for y in range(h))
    return w, h, depth, ctype, np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(h, w, 4)


@pytest.mark.parametrize("fixture", ["c1_sphere_plane_256", "c2_cornell_128", "gallery_160x120"])
def test_output_path_is_the_references_byte_for_byte(fixture, tmp_path):
    """LogAverageLuma + the tone-map loop + Color_Pack (main.cpp:78-127, color.h:105-111) and the PNG behind them.  The
    fixture holds what the REFERENCE's own WriteFramebufferImage made of its own frame: the float LogAverageLuma returned
    (bit pattern) and the RGBA8 pixels of the PNG file it wrote.  prt_host_tonemap must return that float and those bytes
    exactly - the log sum is sequential in row-major order and the pack truncates, so nothing here has a tolerance - and
    the file prt_host_write_image writes must decode to the same pixels."""
    g = load_golden(fixture)
    if "rgba8" not in g:
        pytest.skip("fixture without the reference's output bytes")
    rgb = g["rgb"]
    h, w = rgb.shape[:2]
    rgba = np.concatenate([rgb, np.ones((h, w, 1), dtype=np.float32)], axis=2).astype(np.float32)
    lib = capi.host_lib()
    out8 = np.zeros((h, w, 4), dtype=np.uint8)
    luma = lib.prt_host_tonemap(rgba.ctypes.data_as(C.c_void_p), w, h, out8.ctypes.data_as(C.c_void_p))
    assert np.float32(luma).view(np.uint32) == np.uint32(g["scene_luma_bits"]), "LogAverageLuma differs from the reference's"
    assert np.array_equal(out8, g["rgba8"]), "%d bytes differ from the reference's PNG" % int((out8 != g["rgba8"]).sum())
    assert np.all(out8[:, :, 3] == 255) and out8[:, :, :3].max() > 40
    path = str(tmp_path / "o.png")
    assert lib.prt_host_write_image(rgba.ctypes.data_as(C.c_void_p), w, h, path.encode()) == 0
    pw, ph, depth, ctype, px = _decode_png(path)
    assert (pw, ph, depth, ctype) == (w, h, 8, 6)
    assert np.array_equal(px, g["rgba8"])


# ---- level-1 drop-in: FlattenReferenceScene over the reference's own scene graph --------------------------------------

@pytest.mark.parametrize("scene", ["cornell_box", "textured_gallery", "terrain_64"])
def test_flattened_reference_scene_equals_the_host_mirrors(scene):
    """tests/golden/desc_<scene>.npz is include/prt_flatten_ref.h run INSIDE the reference (oracle/ref_harness --dump-desc:
    its OBJ / MTL / texture loaders, its Scene -> SceneObject -> MeshGroup graph, its sphere tree).  Every array must be
    byte for byte what this repository's loader + host mirror hand to prt_upload_scene for the same files."""
    from par_raytracer_amd import api
    g = load_golden("desc_" + scene)
    mine = api.desc_arrays(host_scene(scene, 0).desc)
    assert sorted(mine) == sorted(g.files)
    for k in g.files:
        want, got = g[k], mine[k]
        assert want.dtype == got.dtype and want.shape == got.shape, k
        assert np.array_equal(want.view(np.uint8), got.view(np.uint8)), "%s: %d differing bytes" % (k, int((want.view(np.uint8) != got.view(np.uint8)).sum()))
    # and the arrays make a scene the CPU restatement renders to the reference's own pixels
    fd = api.FlatDesc({k: g[k] for k in g.files})
    frame = {"cornell_box": "c2_cornell_128", "textured_gallery": "gallery_160x120", "terrain_64": "terrain64_d3"}[scene]
    gf = load_golden(frame)
    from conftest import camera_and_params
    import oracle_py as orc
    cam, p = camera_and_params(gf)
    img, ctr = orc.render(fd.desc, cam, p, int(gf["width"]), int(gf["height"]), 1, 4)
    assert ctr.ray_count == int(gf["ray_count"])
    assert np.array_equal(img[:, :, :3].view(np.uint32), gf["rgb"].view(np.uint32))


# ---- driver binary ------------------------------------------------------------------------------------------------

def test_driver_reports_missing_scene(tmp_path):
    exe = os.path.join(ROOT, "par_raytracer_amd", "prt_main")
    if not os.path.exists(exe):
        pytest.skip("prt_main not built")
    p = subprocess.run([exe, "-d", str(tmp_path), "--obj", "nope.obj", "-w", "8", "-h", "8"], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 1 and b"Cannot load" in p.stderr


def test_bench_folds_its_own_pmc_passes_into_bytes_per_launch(tmp_path, monkeypatch):
    """bench.py measures roofline.traffic in the run that prints it: two `rocprofv3 --pmc` child passes of itself (FETCH_SIZE,
    WRITE_SIZE; counters only) whose counter files it folds into bytes per launch of every kernel - corrected = 2 x FETCH + WRITE
    (KiB units), as the gfx950 guide prescribes.  Here with a stand-in for the profiler that writes the files such a pass writes:
    the command line must be a plain `rocprofv3 --pmc <one counter> ... -- python bench.py ... --no-live-traffic` (no tracing
    beside the counters, no recursion), and a failing pass must give None, not an exception."""
    import importlib.util, stat, sys
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    fake = tmp_path / "bin"
    fake.mkdir()
    log = tmp_path / "calls.txt"
    script = fake / "rocprofv3"
    script.write_text("""#!/usr/bin/env python3
import os, sys
a = sys.argv[1:]
open(%r, "a").write(" ".join(a) + "\\n")
if os.environ.get("FAKE_ROCPROF_FAILS"): sys.exit(3)
counter, out = a[a.index("--pmc") + 1], a[a.index("-d") + 1]
d = os.path.join(out, "host", "runc"); os.makedirs(d)
rows = {"FETCH_SIZE": [("void prt::k_pool<256, 5, false>(prt::PoolArgs const*)", 1000.0), ("void prt::k_pool<256, 5, false>(prt::PoolArgs const*)", 3000.0), ("void prt::k_pool<256, 5, true>(prt::PoolArgs const*)", 9000.0)],
        "WRITE_SIZE": [("void prt::k_pool<256, 5, false>(prt::PoolArgs const*)", 500.0), ("void prt::k_pool<256, 5, false>(prt::PoolArgs const*)", 700.0), ("void prt::k_pool<256, 5, true>(prt::PoolArgs const*)", 100.0)]}[counter]
with open(os.path.join(d, "1_counter_collection.csv"), "w") as f:
    f.write("Kernel_Name,Counter_Name,Counter_Value\\n")
    for k, v in rows: f.write('"%%s",%%s,%%s\\n' %% (k, counter, v))
""" % str(log))
    script.chmod(script.stat().st_mode | stat.S_IEXEC)
    monkeypatch.setenv("PATH", str(fake) + os.pathsep + os.environ["PATH"])
    res, note = bench.measure_traffic_live("C4", 0)
    fast, counting = res["k_pool<256, 5, false>"], res["k_pool<256, 5, true>"]
    assert fast["launches"] == 2 and fast["bytes_raw"] == int((2000.0 + 600.0) * 1024) and fast["bytes_corrected"] == int((2 * 2000.0 + 600.0) * 1024)
    assert counting["launches"] == 1 and counting["bytes_corrected"] == int((2 * 9000.0 + 100.0) * 1024)
    calls = log.read_text().splitlines()
    assert len(calls) == 2 and "--pmc FETCH_SIZE" in calls[0] and "--pmc WRITE_SIZE" in calls[1]
    for c in calls:
        assert "--no-live-traffic" in c and "--no-cpu-baseline" in c and "bench.py" in c.split(" -- ")[1]
        assert not any(t in c.split(" -- ")[0] for t in ("--kernel-trace", "--sys-trace", "--hip-trace", "--stats", "-r ", "-s "))
    monkeypatch.setenv("FAKE_ROCPROF_FAILS", "1")
    res, note = bench.measure_traffic_live("C4", 0)
    assert res is None and "failed" in note
