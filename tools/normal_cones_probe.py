"""The C4 frame (terrain_1m, 1920x1080, 8 spp, depth 2, pool pipeline) with the library PRT_HIP_LIB names: frame times, the frame's
counts and hash, the upload's times, and - on a library that has the option - a counting render with NORMAL_CONES 1 and 0, each
from an upload of its own, since the option is read there (profiles/normal_cones.txt).

    python tools/normal_cones_probe.py [frames [what ...]]      what: frame adaptive c5 counting upload  (default: frame upload)
"""
import hashlib, os, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from par_raytracer_amd import api, scenes, capi

frames = int(sys.argv[1]) if len(sys.argv) > 1 else 15
what = sys.argv[2:] or ["frame", "upload"]
tag = os.environ.get("PRT_HIP_LIB", "libprt_hip.so")
s = scenes.make_scene("terrain_1m"); d = tempfile.mkdtemp(); scenes.write_obj(s, d, "scene.obj")
hs = api.HostScene(d, "scene.obj", 0, s.camera_position)
r = api.Renderer(0)
t0 = time.perf_counter(); info = r.upload(hs); upload_s = time.perf_counter() - t0
has_cones = hasattr(capi.hip_lib(), "prt_get_normal_cones")
w, h = 1920, 1080
cam = api.make_camera(s.fov, w, h, s.camera_position, s.camera_facing)
buf = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda"); torch.cuda.synchronize()


def run(n, p, width=w, height=h, camera=cam):
    c = r.render_device(camera, p, width, height, 0, width * height, buf.data_ptr(), True)             # warm-up
    ms = []
    for _ in range(n):
        c = r.render_device(camera, p, width, height, 0, width * height, buf.data_ptr(), True)
        ms.append(c.render_ms)
    torch.cuda.synchronize()
    ms.sort()
    return ms, c, hashlib.sha1(buf[:height, :width].cpu().numpy().view(np.uint32).tobytes()).hexdigest()[:16]


if "upload" in what:
    print("%-24s upload %.3f s wall, scene tree %.1f ms, normal cones %s" % (
        tag, upload_s, info.bvh_build_ms, "%(coned_nodes)d nodes, %(attach_ms).1f ms" % r.normal_cones() if has_cones else "-"), flush=True)
if "frame" in what:
    ms, c, hx = run(frames, api.default_params(8, 1234, pipeline=capi.PIPELINE_POOL))
    print("%-24s C4 min %.3f median %.3f max %.3f ms  rays %d  shaded %d  image %s" % (tag, ms[0], ms[len(ms) // 2], ms[-1], c.ray_count, c.shaded_hits, hx), flush=True)
if "adaptive" in what:                      # the reference's default sampling, 10..50 spp: k_pool's adaptive variant
    ms, c, hx = run(frames, api.default_params(10, 1234, pipeline=capi.PIPELINE_POOL, max_spp=50))
    print("%-24s C4 adaptive 10..50 min %.3f median %.3f max %.3f ms  rays %d  image %s" % (tag, ms[0], ms[len(ms) // 2], ms[-1], c.ray_count, hx), flush=True)
if "c5" in what:                            # deep bounce trees: the kernel with the draw ring in memory (bench.py's C5 shape at 1080p and 16 spp)
    ms, c, hx = run(frames, api.default_params(16, 1234, pipeline=capi.PIPELINE_POOL, bounce_depth=8))
    print("%-24s depth 8, 1920x1080, 16 spp min %.3f median %.3f max %.3f ms  rays %d  image %s" % (tag, ms[0], ms[len(ms) // 2], ms[-1], c.ray_count, hx), flush=True)
if "counting" in what:
    for v in ((1, 0) if has_cones else (None,)):
        if v is not None:
            r.set_option("NORMAL_CONES", v)
            r.upload(hs)
        ms, c, hx = run(1, api.default_params(8, 1234, pipeline=capi.PIPELINE_POOL | capi.FLAG_COUNT_VISITS))
        st = r.render_stats()
        print("%-24s counting NORMAL_CONES=%s: node visits %d  tri tests %d  wave node steps %d  wave tri steps %d  leaf visits %d  culled %d  coned nodes %s  rays %d  shaded %d  image %s" % (
            tag, v, c.node_visits, c.tri_tests, st.wave_node_steps, st.wave_tri_steps, st.wave_leaf_visits,
            st.cone_culled_nodes if has_cones else 0, r.normal_cones()["coned_nodes"] if has_cones else "-", c.ray_count, c.shaded_hits, hx), flush=True)
r.close()
