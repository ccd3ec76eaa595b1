"""The C4 frame (terrain_1m, 1920x1080, 8 spp, depth 2, pool pipeline) with the library PRT_HIP_LIB names: frame times, the frame's
counts and hash, the upload's times, and - on a library that has the option - SHADOW_OPEN 1 / 0 in one process and a counting
render of each (profiles/shadow_open.txt).

    python tools/shadow_open_probe.py [frames [what ...]]      what: frame adaptive switch counting upload  (default: frame upload)
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
has_open = hasattr(capi.hip_lib(), "prt_get_shadow_open")
w, h = 1920, 1080
cam = api.make_camera(s.fov, w, h, s.camera_position, s.camera_facing)
buf = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda"); torch.cuda.synchronize()


def run(n, counting=False):
    p = api.default_params(8, 1234, pipeline=capi.PIPELINE_POOL | (capi.FLAG_COUNT_VISITS if counting else 0))
    c = r.render_device(cam, p, w, h, 0, w * h, buf.data_ptr(), True)             # warm-up
    ms = []
    for _ in range(n):
        c = r.render_device(cam, p, w, h, 0, w * h, buf.data_ptr(), True)
        ms.append(c.render_ms)
    torch.cuda.synchronize()
    ms.sort()
    return ms, c, hashlib.sha1(buf.cpu().numpy().view(np.uint32).tobytes()).hexdigest()[:16]


if "upload" in what:
    trees = [t.as_dict() for t in r.shadow_trees()]
    print("%-24s upload %.3f s wall, scene tree %.1f ms, shadow trees %s" % (tag, upload_s, info.bvh_build_ms, ["%.1f ms" % t["build_ms"] for t in trees]), flush=True)
    if has_open:
        print("%-24s open triangles %s" % (tag, [(o.open_count, "%.1f ms" % o.classify_ms, o.active) for o in r.shadow_open()]), flush=True)
if "frame" in what:
    ms, c, hx = run(frames)
    print("%-24s C4 min %.3f median %.3f max %.3f ms  rays %d  shaded %d  image %s" % (tag, ms[0], ms[len(ms) // 2], ms[-1], c.ray_count, c.shaded_hits, hx), flush=True)
if "adaptive" in what:                      # the reference's default sampling, 10..50 spp: k_pool's adaptive variant
    p = api.default_params(10, 1234, pipeline=capi.PIPELINE_POOL, max_spp=50)
    ms = []
    for k in range(frames + 1):
        c = r.render_device(cam, p, w, h, 0, w * h, buf.data_ptr(), True)
        if k:
            ms.append(c.render_ms)
    ms.sort()
    print("%-24s C4 adaptive 10..50 min %.3f median %.3f max %.3f ms  rays %d" % (tag, ms[0], ms[len(ms) // 2], ms[-1], c.ray_count), flush=True)
if "switch" in what and has_open:
    for v in (1, 0, 1, 0):
        r.set_option("SHADOW_OPEN", v)
        ms, c, hx = run(frames)
        print("%-24s SHADOW_OPEN=%d min %.3f median %.3f max %.3f ms  rays %d  image %s" % (tag, v, ms[0], ms[len(ms) // 2], ms[-1], c.ray_count, hx), flush=True)
    r.set_option("SHADOW_OPEN", None)
if "counting" in what:
    for v in ((1, 0) if has_open else (None,)):
        if v is not None:
            r.set_option("SHADOW_OPEN", v)
        ms, c, hx = run(1, True)
        st = r.render_stats()
        print("%-24s counting SHADOW_OPEN=%s: node visits %d  tri tests %d  wave node steps %d  wave tri steps %d  leaf visits %d  elided %d  open %d  rays %d  shaded %d  image %s" % (
            tag, v, c.node_visits, c.tri_tests, st.wave_node_steps, st.wave_tri_steps, st.wave_leaf_visits, st.elided_shadow_rays,
            st.open_shadow_rays, c.ray_count, c.shaded_hits, hx), flush=True)
    if has_open:
        r.set_option("SHADOW_OPEN", None)
r.close()
