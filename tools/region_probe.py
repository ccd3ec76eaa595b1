#!/usr/bin/env python3
"""One C4 frame (terrain_1m, 1920x1080, 8 spp, depth 2; pool pipeline, or --pipeline wavefront, whose traversal kernel is k_trace)
with the library PRT_HIP_LIB names: frame times, ray count, shaded hits and a hash of the frame's words - one process per library
and round gives the interleaved A/B protocol of profiles/r05_valu_budget.txt section 3 - and, with --regions (pool only), the
region table of a COUNT render of the same frame as JSON for tools/valu_budget.py --regions.

    python tools/region_probe.py [--pipeline pool|wavefront] [--frames N] [--regions OUT.json] [--tag NAME]
"""
import hashlib, json, os, sys, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from par_raytracer_amd import api, scenes, capi


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


frames = int(arg("--frames", "15"))
out = arg("--regions", None)
pipeline = {"pool": capi.PIPELINE_POOL, "wavefront": capi.PIPELINE_WAVEFRONT}[arg("--pipeline", "pool")]
if out and pipeline != capi.PIPELINE_POOL:
    sys.exit("--regions: the region table is k_pool's")
tag = arg("--tag", os.environ.get("PRT_HIP_LIB", "libprt_hip.so"))
s = scenes.make_scene("terrain_1m"); d = tempfile.mkdtemp(); scenes.write_obj(s, d, "scene.obj")
hs = api.HostScene(d, "scene.obj", 0, s.camera_position)
r = api.Renderer(0); r.upload(hs)
w, h = 1920, 1080
cam = api.make_camera(s.fov, w, h, s.camera_position, s.camera_facing)
buf = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda"); torch.cuda.synchronize()


def sha(t):
    torch.cuda.synchronize()
    return hashlib.sha1(t.cpu().numpy().view(np.uint32).tobytes()).hexdigest()[:16]


p = api.default_params(8, 1234, pipeline=pipeline)
r.render_device(cam, p, w, h, 0, w * h, buf.data_ptr(), True)          # warm-up
ms = []
for _ in range(frames):
    c = r.render_device(cam, p, w, h, 0, w * h, buf.data_ptr(), True)
    ms.append(c.render_ms)
ms.sort()
image = sha(buf)
print("%-24s C4 min %.3f median %.3f max %.3f ms  rays %d  shaded %d  image %s" % (
    tag, ms[0], ms[len(ms) // 2], ms[-1], c.ray_count, c.shaded_hits, image), flush=True)
if out:
    buf.zero_()
    pc = api.default_params(8, 1234, pipeline=capi.PIPELINE_POOL | capi.FLAG_COUNT_VISITS)
    cc = r.render_device(cam, pc, w, h, 0, w * h, buf.data_ptr(), True)
    st = r.render_stats()
    table = r.region_stats()
    same = sha(buf) == image and cc.ray_count == c.ray_count and cc.shaded_hits == c.shaded_hits
    print("%-24s COUNT render %.2f ms: image and counts %s" % (tag, cc.render_ms, "IDENTICAL" if same else "DIFFER"), flush=True)
    table["_frame"] = {"ray_count": int(cc.ray_count), "shaded_hits": int(cc.shaded_hits), "image": image,
                       "wave_node_steps": int(st.wave_node_steps), "wave_tri_steps": int(st.wave_tri_steps),
                       "wave_refills": int(st.wave_refills), "elided_shadow_rays": int(st.elided_shadow_rays)}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    json.dump(table, open(out, "w"), indent=1)
    for k in capi.REGION_NAMES:
        n, lanes = table[k]
        print("   %-18s %12d executions %14d lanes (%.1f each)" % (k, n, lanes, lanes / n if n else 0.0))
r.close()
