#!/usr/bin/env python3
"""Generate tests/golden/*.npz from the compiled, unmodified reference (oracle/_ref/ref_harness).

Run in the build container only (needs /root/reference):  python oracle/gen_golden.py [--only NAME ...]

Each fixture is DATA: the inputs (scene name -> par_raytracer_amd.scenes generator, camera, params, seed,
lattice) and the reference's outputs (float RGB at the lattice pixels, the three DebugCounters).  Pixels are
independently seeded (include/prt_key.h), so any pixel subset of a frame is a valid fixture; the big
configs are sampled on a sparse lattice to keep fixtures small.
`kat.npz` holds per-function known-answer vectors (PRNG, Hammersley, bounce directions, Fresnel,
ray/triangle, ray/sphere, camera rays) produced by calling the reference's own functions; `kat_texture.npz` the
same for Texture_SampleBilinear on a table of small in-memory textures (its own file and its own random stream, so
kat.npz never has to be regenerated for it).
"""
from __future__ import annotations

import argparse
import os
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import oracle_py as orc                                  # noqa: E402
from par_raytracer_amd import scenes                     # noqa: E402
sys.path.insert(0, os.path.join(ROOT, "tests"))
import texture_fixtures                                   # noqa: E402,F401  (registers the textured gallery scenes)

GOLDEN = os.path.join(ROOT, "tests", "golden")

# name -> dict(scene, width, height, spp, lattice, depth, light_mode, rs, ss, seed)
FIXTURES = {
    # BASELINE configs (C1 full frame; C2 full small frame + lattice of the 512^2 frame; C3-C5 sparse lattices)
    "c1_sphere_plane_256": dict(scene="sphere_plane", width=256, height=256, spp=1, lattice=1, png=True),
    "c2_cornell_128": dict(scene="cornell_box", width=128, height=128, spp=4, lattice=1, png=True),
    "c2_cornell_512_l4": dict(scene="cornell_box", width=512, height=512, spp=4, lattice=4),
    "c3_icosphere_1080p_l24": dict(scene="icosphere_l6", width=1920, height=1080, spp=8, lattice=24),
    "c4_terrain1m_1080p_l40": dict(scene="terrain_1m", width=1920, height=1080, spp=8, lattice=40),
    "c5_terrain1m_4k_l120": dict(scene="terrain_1m", width=3840, height=2160, spp=64, lattice=120, depth=8),
    # code-path coverage: two lights, point light (inverted occlusion test), deeper trees, multi-sample bounces
    "cornell_point_light_d5": dict(scene="cornell_box", width=48, height=48, spp=2, lattice=1, depth=5, light_mode=2, rs=2, ss=2),
    "icosphere_l3_two_lights": dict(scene="icosphere_l3", width=64, height=48, spp=2, lattice=1, light_mode=1),
    "terrain64_d3": dict(scene="terrain_64", width=80, height=60, spp=2, lattice=1, depth=3),
    "terrain192_d2": dict(scene="terrain_192", width=160, height=90, spp=4, lattice=1),
    "many_materials_two_lights": dict(scene="many_materials", width=96, height=72, spp=2, lattice=1, depth=3, light_mode=1),
    # near-coincident hits: the reference's visit order decides (raytracer.cpp:104, 149, 208-209, 220)
    "coincident_192x144_d3": dict(scene="coincident", width=192, height=144, spp=4, lattice=1, depth=3, png=True),
    "coincident_two_lights": dict(scene="coincident", width=96, height=72, spp=2, lattice=1, depth=2, light_mode=2),
    # row N1: texture / alpha / bump path (14 texture files in 9 encodings; alpha holes, translucency, bump frames)
    "gallery_160x120": dict(scene="textured_gallery", width=160, height=120, spp=4, lattice=1, png=True),
    "gallery_two_lights_d4": dict(scene="textured_gallery", width=96, height=72, spp=2, lattice=1, depth=4, light_mode=1, rs=2, ss=2),
    # JPEG textures: 12 baseline files of every sampling layout (grey, 4:4:4 ... 4:1:1, restart intervals, one scan per
    # component, RGB ids) as diffuse / bump / alpha maps; pins the decoder's IDCT, upsampling and colour arithmetic
    "jpeg_gallery_128x96": dict(scene="jpeg_gallery", width=128, height=96, spp=4, lattice=1),
    # the PNG corners of the loader: Adam7, 1 / 2 / 4-bit grey and palettes, colour-key tRNS (with the reference decoder's
    # channel-count quirk), 16-bit interlaced
    "png_gallery_128x96": dict(scene="png_gallery", width=128, height=96, spp=4, lattice=1),
    # every BMP flavour the reference's decoder accepts (palettes, 16 / 24 / 32-bit, OS/2 and V4 headers, masks, alpha rules)
    "bmp_gallery_128x96": dict(scene="bmp_gallery", width=128, height=96, spp=4, lattice=1),
    # the TGA corners: 5-5-5 pixels, grey + alpha, colour maps with 15 / 24 / 32-bit entries and 8 / 16-bit indices
    "tga_gallery_128x96": dict(scene="tga_gallery", width=128, height=96, spp=4, lattice=1),
    # GIF as the reference's decoder reads it: first image, RGBA, background / transparent pixels with alpha 0
    "gif_gallery_128x96": dict(scene="gif_gallery", width=128, height=96, spp=4, lattice=1),
    # Photoshop composites: raw / PackBits, 16-bit, RGBA with every alpha value (float un-blending from white)
    "psd_gallery_128x96": dict(scene="psd_gallery", width=128, height=96, spp=4, lattice=1),
    # Radiance .hdr through the 8-bit entry point: RGBE -> float -> the decoder's gamma-2.2 tone map
    "hdr_gallery_128x96": dict(scene="hdr_gallery", width=128, height=96, spp=4, lattice=1),
    # Softimage PIC: raw / pure / mixed run-length packets, separate alpha packet, 16-bit run counts
    "pic_gallery_128x96": dict(scene="pic_gallery", width=128, height=96, spp=4, lattice=1),
    # the texture path at its edges: a 2 x 2 map under texture coordinates from -2.5 to 3.5, corners exactly 0 and 1, d 1.5 with an
    # alpha ramp (alpha x texel crosses 0.05 and 1), a two-channel Ks map, a non-square bump map tiled from a negative origin
    "texture_edges_64x48": dict(scene="texture_edges", width=64, height=48, spp=2, lattice=1, depth=2),
    "texture_edges_point_light_64x48": dict(scene="texture_edges", width=64, height=48, spp=2, lattice=1, depth=2, light_mode=2),
    # row N4: the reference's adaptive loop (main.cpp:245-258), one RNG stream per pixel; spp = min_samples
    "cornell_adaptive_4_16": dict(scene="cornell_box", width=96, height=72, spp=4, max_spp=16, lattice=1),
    "gallery_adaptive_10_50": dict(scene="textured_gallery", width=64, height=48, spp=10, max_spp=50, lattice=1),      # reference defaults
    "terrain64_adaptive_3_12_d4": dict(scene="terrain_64", width=80, height=60, spp=3, max_spp=12, lattice=1, depth=4, light_mode=1),
    "c4_terrain1m_adaptive_l60": dict(scene="terrain_1m", width=1920, height=1080, spp=10, max_spp=50, lattice=60),
    # tests/test_oracle_golden.py::test_live_against_compiled_reference: odd sizes, depths, light modes and sample counts
    "live_cornell_box_40x30": dict(scene="cornell_box", width=40, height=30, spp=3, lattice=1, depth=4, light_mode=1, rs=1, ss=2, seed=99),
    "live_sphere_plane_48x48": dict(scene="sphere_plane", width=48, height=48, spp=2, lattice=1, depth=2, light_mode=2, rs=2, ss=1, seed=7),
    "live_terrain_64_32x24": dict(scene="terrain_64", width=32, height=24, spp=2, lattice=1, depth=6, light_mode=0, rs=1, ss=1, seed=424242),
    "live_textured_gallery_56x40": dict(scene="textured_gallery", width=56, height=40, spp=3, lattice=1, depth=5, light_mode=2, rs=1, ss=2,
                                        seed=31337),
    "live_coincident_64x48": dict(scene="coincident", width=64, height=48, spp=3, lattice=1, depth=4, light_mode=1, rs=1, ss=1, seed=2025),
}


def generate(name: str, cfg: dict, scene_cache: dict) -> None:
    scene_name = cfg["scene"]
    if scene_name not in scene_cache:
        d = tempfile.mkdtemp(prefix="prt_golden_%s_" % scene_name)
        s = scenes.make_scene(scene_name)
        scenes.write_obj(s, d, "scene.obj")
        scene_cache[scene_name] = (s, d)
    s, d = scene_cache[scene_name]
    seed = cfg.get("seed", 1234)
    t0 = time.time()
    want_dump = s.n_tris <= 100000
    ref = orc.run_reference(d, "scene.obj", cfg["width"], cfg["height"], cfg["spp"], seed, s.camera_position,
                            s.camera_facing, s.fov, bounce_depth=cfg.get("depth", 2),
                            reflection_samples=cfg.get("rs", 1), spec_samples=cfg.get("ss", 1),
                            lattice=cfg["lattice"], light_mode=cfg.get("light_mode", 0), dump_scene=want_dump,
                            timeout=6 * 3600, adaptive_max=cfg.get("max_spp", 0), write_png=bool(cfg.get("png")))
    st = ref["stats"]
    out = dict(
        scene=scene_name, width=cfg["width"], height=cfg["height"], spp=cfg["spp"], lattice=cfg["lattice"],
        bounce_depth=cfg.get("depth", 2), light_mode=cfg.get("light_mode", 0), reflection_samples=cfg.get("rs", 1),
        spec_samples=cfg.get("ss", 1), seed=seed, max_spp=cfg.get("max_spp", 0),
        camera_position=np.array(s.camera_position, dtype=np.float64), camera_facing=np.array(s.camera_facing, dtype=np.float64),
        fov=float(s.fov),
        rgb=ref["pixels"][:, :, :3].copy(),
        ray_count=np.uint64(st["ray_count"]), sphere_check_count=np.uint64(st["sphere_check_count"]),
        mesh_check_count=np.uint64(st["mesh_check_count"]), triangles=st["triangles"], groups=st["groups"],
        reference_render_seconds=st["render_seconds"], reference_hierarchy_seconds=st["hierarchy_seconds"],
    )
    assert np.all(ref["pixels"][:, :, 3] == 1.0)
    if ref.get("png"):
        # the output path (main.cpp:78-131): bytes of the PNG the reference's own WriteFramebufferImage wrote for this frame,
        # and the float LogAverageLuma returned
        out["rgba8"] = orc.decode_png_rgba8(ref["png"])
        out["scene_luma_bits"] = np.uint32(st["scene_luma_bits"])
    if want_dump:
        sc = ref["scene"]
        out["spheres"] = np.frombuffer(sc["spheres"], dtype=np.float32).reshape(-1, 4).copy()
        out["sphere_children"] = np.frombuffer(sc["sphere_children"], dtype=np.uint32).reshape(-1, 2).copy()
        out["sphere_group"] = np.frombuffer(sc["sphere_group"], dtype=np.int32).copy()
        out["group_index_counts"] = np.frombuffer(sc["group_index_counts"], dtype=np.uint32).copy()
        # loader check without storing the whole mesh: exact byte sums of what the reference parsed
        if len(sc.get("group_texture_bytes", b"")):
            out["group_texture_dims"] = np.frombuffer(sc["group_texture_dims"], dtype=np.uint32).copy()
        for k in ("positions", "texcoords", "normals", "idx_positions", "idx_texcoords", "idx_normals", "group_materials",
                  "tangents", "group_texture_bytes"):
            if k not in sc:
                continue
            a = np.frombuffer(sc[k], dtype=np.uint8)
            out["sum_" + k] = np.array([a.size, int(a.astype(np.uint64).sum()),
                                        int((a.astype(np.uint64) * (np.arange(a.size, dtype=np.uint64) % 251 + 1)).sum() % (1 << 62))],
                                       dtype=np.uint64)
    os.makedirs(GOLDEN, exist_ok=True)
    np.savez_compressed(os.path.join(GOLDEN, name + ".npz"), **out)
    print("%-28s %7d tris  %dx%d spp %d lattice %d  rays %d  ref %.1fs  (total %.1fs)" % (
        name, st["triangles"], cfg["width"], cfg["height"], cfg["spp"], cfg["lattice"], st["ray_count"],
        st["render_seconds"], time.time() - t0), flush=True)


# Scenes whose prt_scene_desc - FlattenReferenceScene (include/prt_flatten_ref.h) run inside ref_harness over the REFERENCE's
# own scene graph - is stored whole: tests/golden/desc_<scene>.npz.  The CPU tests compare it byte for byte with the host
# mirror's flattening; the GPU tests upload it through prt_upload_scene (the level-1 drop-in: the reference's loader, graph
# and decoded textures feeding the HIP path) and match the frame fixture named here.
DESC_FIXTURES = {
    "cornell_box": "c2_cornell_128",
    "textured_gallery": "gallery_160x120",
    "terrain_64": "terrain64_d3",
}


def generate_desc(scene_name: str, scene_cache: dict) -> None:
    if scene_name not in scene_cache:
        d = tempfile.mkdtemp(prefix="prt_golden_%s_" % scene_name)
        s = scenes.make_scene(scene_name)
        scenes.write_obj(s, d, "scene.obj")
        scene_cache[scene_name] = (s, d)
    s, d = scene_cache[scene_name]
    ref = orc.run_reference(d, "scene.obj", 16, 16, 1, 1234, s.camera_position, s.camera_facing, s.fov, render=False,
                            dump_desc=True)
    raw = ref["desc"]
    f32 = ("positions", "normals", "texcoords", "tangents")
    u32 = ("idx_positions", "idx_texcoords", "idx_normals", "texture_dims")
    out = {}
    for k, v in raw.items():
        dt = np.float32 if k in f32 else np.uint32 if k in u32 else np.int32 if k == "sphere_group" else np.uint8
        out[k] = np.frombuffer(v, dtype=dt).copy()
    np.savez_compressed(os.path.join(GOLDEN, "desc_%s.npz" % scene_name), **out)
    print("desc_%s.npz: %d triangles, %d groups, %d materials, %d textures (%d texel bytes)" % (
        scene_name, out["idx_positions"].size // 3, out["groups"].size // 12, out["materials"].size // 80,
        out["texture_dims"].size // 3, out["texture_bytes"].size))


def generate_kat(scene_cache: dict) -> None:
    s = scenes.make_scene("sphere_plane")
    d = tempfile.mkdtemp(prefix="prt_golden_kat_")
    scenes.write_obj(s, d, "scene.obj")
    ref = orc.run_reference(d, "scene.obj", 256, 256, 1, 1234, s.camera_position, s.camera_facing, s.fov,
                            render=False, kat=True)
    k = ref["kat"]
    u64 = ("rng_seed", "rng_state", "rng_next", "key_1234")
    out = {}
    for name, raw in k.items():
        out[name] = np.frombuffer(raw, dtype=np.uint64 if name in u64 else np.float32).copy()
    np.savez_compressed(os.path.join(GOLDEN, "kat.npz"), **out)
    print("kat.npz: %s" % ", ".join(sorted(out)))


def generate_kat_texture() -> None:
    """kat_texture.npz: the reference's Texture_SampleBilinear on a table of in-memory textures (ref_harness --kat-texture)."""
    k = orc.run_reference_kat_texture()
    out = {
        "texture_dims": np.frombuffer(k["texture_dims"], dtype=np.uint32).copy(),
        "texture_bytes": np.frombuffer(k["texture_bytes"], dtype=np.uint8).copy(),
        "tex_in": np.frombuffer(k["tex_in"], dtype=np.float32).reshape(-1, 3).copy(),
        "tex_out": np.frombuffer(k["tex_out"], dtype=np.float32).reshape(-1, 4).copy(),
        "srgb_lut": np.frombuffer(k["srgb_lut"], dtype=np.float32).copy(),
    }
    np.savez_compressed(os.path.join(GOLDEN, "kat_texture.npz"), **out)
    print("kat_texture.npz: %d textures (%d texel bytes), %d records" % (out["texture_dims"].size // 3, out["texture_bytes"].size,
                                                                          len(out["tex_in"])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", default=None)
    args = ap.parse_args()
    if not orc.have_reference():
        raise SystemExit("oracle/_ref/ref_harness missing: run `make -C oracle ref` in the build container")
    cache = {}
    names = args.only if args.only else ["kat", "kat_texture"] + list(FIXTURES) + ["desc_" + k for k in DESC_FIXTURES]
    for n in names:
        if n == "kat":
            generate_kat(cache)
        elif n == "kat_texture":
            generate_kat_texture()
        elif n.startswith("desc_"):
            generate_desc(n[5:], cache)
        else:
            generate(n, FIXTURES[n], cache)


if __name__ == "__main__":
    main()
