"""Thin Python objects over the C ABI: HostScene (reference-style host pipeline) and Renderer (prt_ctx).

Mirrors the reference driver's call sequence (main.cpp:537-612) so tests read like the reference's
own main(): load OBJ -> hierarchy -> scene -> camera -> Render -> image.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np

from . import capi
from .capi import PrtCamera, PrtCounters, PrtParams, PrtSceneDesc, PrtGradInfo, PrtSceneInfo, PrtUpdateInfo


class HostScene:
    """ParseOBJ + CalculateTangents + BuildHierarchy + InitScene + object list, flattened."""

    def __init__(self, directory: str, obj_name: str = "sponza.obj", light_mode: int = 0,
                 camera_position: Sequence[float] = (0.0, 0.0, 0.0)):
        lib = capi.host_lib()
        cp = (C.c_float * 3)(*[float(v) for v in camera_position])
        self._lib = lib
        self._h = lib.prt_host_load_obj(directory.encode(), obj_name.encode(), int(light_mode), cp)
        if not self._h:
            raise RuntimeError("prt_host_load_obj failed: %s" % lib.prt_host_last_error().decode())

    @property
    def handle(self):
        return self._h

    @property
    def desc(self) -> "C.POINTER(PrtSceneDesc)":
        return self._lib.prt_host_scene_desc(self._h)

    @property
    def hierarchy_seconds(self) -> float:
        return self._lib.prt_host_scene_hierarchy_seconds(self._h)

    @property
    def parse_seconds(self) -> float:
        return self._lib.prt_host_scene_parse_seconds(self._h)

    @property
    def n_tris(self) -> int:
        return self.desc.contents.index_count // 3

    def arrays(self) -> dict:
        """numpy copies of the flattened scene (for tests)."""
        d = self.desc.contents
        f = capi.np_from_ptr
        out = {
            "positions": f(d.positions, d.position_count * 3, np.float32).reshape(-1, 3),
            "normals": f(d.normals, d.normal_count * 3, np.float32).reshape(-1, 3),
            "texcoords": f(d.texcoords, d.texcoord_count * 2, np.float32).reshape(-1, 2),
            "idx_positions": f(d.idx_positions, d.index_count, np.uint32),
            "idx_texcoords": f(d.idx_texcoords, d.index_count, np.uint32),
            "idx_normals": f(d.idx_normals, d.index_count, np.uint32),
            "groups": np.array([(d.groups[i].first_index, d.groups[i].index_count, d.groups[i].material)
                                for i in range(d.group_count)], dtype=np.int64).reshape(-1, 3),
            "spheres": np.array([(tuple(d.spheres[i].center) + (d.spheres[i].radius,)) for i in range(d.sphere_count)],
                                dtype=np.float32).reshape(-1, 4),
            "sphere_children": np.array([(d.spheres[i].c0, d.spheres[i].c1) for i in range(d.sphere_count)],
                                        dtype=np.uint32).reshape(-1, 2),
            "sphere_group": f(d.sphere_group, d.sphere_count, np.int32),
            "materials": np.array([[m.specular_intensity, m.index_of_refraction, m.alpha] + list(m.ambient_color) +
                                   list(m.diffuse_color) + list(m.specular_color)
                                   for m in (d.materials[i] for i in range(d.material_count))], dtype=np.float32),
        }
        out["tangents"] = (f(d.tangents, d.normal_count * 3, np.float32).reshape(-1, 3) if d.tangents
                           else np.zeros((0, 3), dtype=np.float32))
        # texture slots per group, in the reference's slot order (ambient, diffuse, specular, alpha, bump)
        dims, blobs = [], []
        for g in range(d.group_count):
            m = d.materials[d.groups[g].material]
            for slot in (m.ambient_texture, m.diffuse_texture, m.specular_texture, m.alpha_texture, m.bump_texture):
                if slot < 0:
                    dims += [0, 0, 0]
                else:
                    t = d.textures[slot]
                    dims += [t.size_x, t.size_y, t.channels]
                    blobs.append(np.ctypeslib.as_array(t.texels, shape=(t.size_x * t.size_y * t.channels,)).copy())
        out["group_texture_dims"] = np.array(dims, dtype=np.uint32)
        out["group_texture_bytes"] = np.concatenate(blobs) if blobs else np.zeros(0, dtype=np.uint8)
        return out

    def close(self):
        if self._h:
            self._lib.prt_host_free_scene(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- prt_scene_desc <-> flat arrays (the level-1 drop-in's data: what FlattenReferenceScene hands to prt_upload_scene) ---

DESC_F32 = ("positions", "normals", "texcoords", "tangents")
DESC_U32 = ("idx_positions", "idx_texcoords", "idx_normals", "texture_dims")


def desc_arrays(desc_ptr) -> dict:
    """Every array a prt_scene_desc points to, as flat numpy copies: float / index arrays as such, the record arrays
    (prt_group 12 B, prt_material 80 B, prt_light 48 B, prt_bsphere 24 B) as raw bytes, textures as (size_x, size_y,
    channels) triples + the concatenated texel bytes - the layout of oracle/ref_harness --dump-desc."""
    d = desc_ptr.contents
    f = capi.np_from_ptr

    def raw(ptr, count, size):
        return f(C.cast(ptr, C.POINTER(C.c_uint8)), count * size, np.uint8) if count else np.zeros(0, dtype=np.uint8)

    out = {
        "positions": f(d.positions, d.position_count * 3, np.float32),
        "normals": f(d.normals, d.normal_count * 3, np.float32),
        "texcoords": f(d.texcoords, d.texcoord_count * 2, np.float32),
        "tangents": f(d.tangents, d.normal_count * 3, np.float32) if d.tangents else np.zeros(0, dtype=np.float32),
        "idx_positions": f(d.idx_positions, d.index_count, np.uint32),
        "idx_texcoords": f(d.idx_texcoords, d.index_count, np.uint32),
        "idx_normals": f(d.idx_normals, d.index_count, np.uint32),
        "groups": raw(d.groups, d.group_count, C.sizeof(capi.PrtGroup)),
        "materials": raw(d.materials, d.material_count, C.sizeof(capi.PrtMaterial)),
        "lights": raw(d.lights, d.light_count, C.sizeof(capi.PrtLight)),
        "spheres": raw(d.spheres, d.sphere_count, C.sizeof(capi.PrtBSphere)),
        "sphere_group": f(d.sphere_group, d.sphere_count, np.int32) if d.sphere_count else np.zeros(0, dtype=np.int32),
    }
    dims, blobs = [], []
    for i in range(d.texture_count):
        t = d.textures[i]
        dims += [t.size_x, t.size_y, t.channels]
        blobs.append(np.ctypeslib.as_array(t.texels, shape=(t.size_x * t.size_y * t.channels,)).copy())
    out["texture_dims"] = np.array(dims, dtype=np.uint32)
    out["texture_bytes"] = np.concatenate(blobs) if blobs else np.zeros(0, dtype=np.uint8)
    return out


class FlatDesc:
    """A prt_scene_desc built from the arrays of desc_arrays() / a tests/golden/desc_*.npz fixture.  Keeps the arrays
    alive; `.desc` is what Renderer.upload() and the oracle take."""

    def __init__(self, arrays: dict):
        a = {k: np.ascontiguousarray(np.asarray(v)) for k, v in arrays.items()}
        self._keep = a
        d = capi.PrtSceneDesc()

        def ptr(key, ctype):
            arr = a[key]
            return arr.ctypes.data_as(C.POINTER(ctype)) if arr.size else C.cast(None, C.POINTER(ctype))

        d.positions = ptr("positions", C.c_float); d.position_count = a["positions"].size // 3
        d.normals = ptr("normals", C.c_float); d.normal_count = a["normals"].size // 3
        d.texcoords = ptr("texcoords", C.c_float); d.texcoord_count = a["texcoords"].size // 2
        d.tangents = ptr("tangents", C.c_float)
        d.idx_positions = ptr("idx_positions", C.c_uint32)
        d.idx_texcoords = ptr("idx_texcoords", C.c_uint32)
        d.idx_normals = ptr("idx_normals", C.c_uint32)
        d.index_count = a["idx_positions"].size
        d.groups = ptr("groups", capi.PrtGroup); d.group_count = a["groups"].size // C.sizeof(capi.PrtGroup)
        d.materials = ptr("materials", capi.PrtMaterial); d.material_count = a["materials"].size // C.sizeof(capi.PrtMaterial)
        d.lights = ptr("lights", capi.PrtLight); d.light_count = a["lights"].size // C.sizeof(capi.PrtLight)
        d.spheres = ptr("spheres", capi.PrtBSphere); d.sphere_count = a["spheres"].size // C.sizeof(capi.PrtBSphere)
        d.sphere_group = ptr("sphere_group", C.c_int32)
        dims = a["texture_dims"].reshape(-1, 3)
        self._tex = (capi.PrtTexture * max(1, len(dims)))()
        off = 0
        base = a["texture_bytes"].ctypes.data
        for i, (sx, sy, ch) in enumerate(dims):
            self._tex[i].size_x, self._tex[i].size_y, self._tex[i].channels = int(sx), int(sy), int(ch)
            self._tex[i].texels = C.cast(base + off, C.POINTER(C.c_uint8))
            off += int(sx) * int(sy) * int(ch)
        d.textures = C.cast(self._tex, C.POINTER(capi.PrtTexture)) if len(dims) else C.cast(None, C.POINTER(capi.PrtTexture))
        d.texture_count = len(dims)
        self._desc = d

    @property
    def desc(self):
        return C.pointer(self._desc)


def make_camera(fov: float, width: int, height: int, position: Sequence[float], facing: Sequence[float]) -> PrtCamera:
    cam = PrtCamera()
    p = (C.c_float * 3)(*[float(v) for v in position])
    f = (C.c_float * 3)(*[float(v) for v in facing])
    capi.host_lib().prt_host_make_camera(float(fov), int(width), int(height), p, f, C.byref(cam))
    return cam


def default_params(spp: int, seed: int = 1234, bounce_depth: Optional[int] = None, reflection_samples: Optional[int] = None,
                   spec_samples: Optional[int] = None, pipeline: int = 0, max_spp: int = 0,
                   variance_threshold: float = 0.0) -> PrtParams:
    """`max_spp` > spp turns on the reference's adaptive loop (main.cpp:245-258): spp fixed samples, then up to max_spp."""
    p = PrtParams()
    capi.host_lib().prt_host_default_params(int(spp), int(seed), C.byref(p))
    if bounce_depth is not None:
        p.bounce_depth = int(bounce_depth)
    if reflection_samples is not None:
        p.reflection_samples = int(reflection_samples)
    if spec_samples is not None:
        p.spec_samples = int(spec_samples)
    p.pipeline = int(pipeline)
    p.max_spp = int(max_spp)
    p.variance_threshold = float(variance_threshold)
    return p


class Renderer:
    """prt_ctx: one HIP device, one uploaded scene."""

    def __init__(self, device_id: int = 0):
        lib = capi.hip_lib()
        self._lib = lib
        self._ctx = lib.prt_create(int(device_id))
        if not self._ctx:
            raise RuntimeError("prt_create(%d) failed: %s" % (device_id, lib.prt_last_error(None).decode()))
        self.device_id = device_id

    def _check(self, rc: int, what: str):
        if rc != 0:
            raise RuntimeError("%s failed (%d): %s" % (what, rc, self._lib.prt_last_error(self._ctx).decode()))

    def set_option(self, name: str, value=None) -> None:
        """prt_set_option: one entry of the context's option table (csrc/prt_options.h); value None restores the default.
        The environment (PRT_<NAME>) is only read when the context is created."""
        v = None if value is None else str(value).encode()
        self._check(self._lib.prt_set_option(self._ctx, name.encode(), v), "prt_set_option(%s)" % name)

    def upload(self, scene) -> PrtSceneInfo:
        desc = scene.desc if isinstance(scene, (HostScene, FlatDesc)) else scene
        self._check(self._lib.prt_upload_scene(self._ctx, desc), "prt_upload_scene")
        return self.scene_info()

    def scene_info(self) -> PrtSceneInfo:
        info = PrtSceneInfo()
        self._check(self._lib.prt_get_scene_info(self._ctx, C.byref(info)), "prt_get_scene_info")
        return info

    def shadow_trees(self) -> list:
        """One capi.PrtShadowTreeInfo per light of the uploaded scene (include/prt.h "Shadow trees")."""
        n = self._lib.prt_get_shadow_trees(self._ctx, None, 0)
        if n < 0:
            self._check(n, "prt_get_shadow_trees")
        out = (capi.PrtShadowTreeInfo * max(1, n))()
        self._check(min(0, self._lib.prt_get_shadow_trees(self._ctx, out, n)), "prt_get_shadow_trees")
        return [out[i] for i in range(n)]

    def shadow_open(self) -> list:
        """One capi.PrtShadowOpenInfo per light of the uploaded scene (include/prt.h "Open triangles")."""
        n = self._lib.prt_get_shadow_open(self._ctx, None, 0)
        if n < 0:
            self._check(n, "prt_get_shadow_open")
        out = (capi.PrtShadowOpenInfo * max(1, n))()
        self._check(min(0, self._lib.prt_get_shadow_open(self._ctx, out, n)), "prt_get_shadow_open")
        return [out[i] for i in range(n)]

    def normal_cones(self) -> dict:
        """The scene's normal cones (include/prt.h "Normal cones"): nodes that carried one at upload, and the host time of attaching them."""
        out = capi.PrtNormalConeInfo()
        self._check(self._lib.prt_get_normal_cones(self._ctx, C.byref(out)), "prt_get_normal_cones")
        return out.as_dict()

    def render_stats(self) -> "capi.PrtRenderStats":
        """Diagnostics of the last render made with FLAG_COUNT_VISITS (lane utilisation, phase times, parked rays)."""
        st = capi.PrtRenderStats()
        self._check(self._lib.prt_get_render_stats(self._ctx, C.byref(st)), "prt_get_render_stats")
        return st

    def region_stats(self) -> dict:
        """k_pool's region table of the last render made with FLAG_COUNT_VISITS: {region: (wave-level executions, active lanes)}."""
        n = 2 * len(capi.REGION_NAMES)
        out = (C.c_uint64 * n)()
        got = self._lib.prt_get_region_stats(self._ctx, out, n)
        if got != n:
            raise RuntimeError("prt_get_region_stats: the library has %d words, capi.REGION_NAMES %d" % (got, n))
        return {name: (int(out[2 * k]), int(out[2 * k + 1])) for k, name in enumerate(capi.REGION_NAMES)}

    def render(self, cam: PrtCamera, params: PrtParams, width: int, height: int, start_idx: int = 0,
               end_idx: Optional[int] = None) -> Tuple[np.ndarray, PrtCounters]:
        if end_idx is None:
            end_idx = width * height
        out = np.empty((end_idx - start_idx, 4), dtype=np.float32)
        counters = PrtCounters()
        self._check(self._lib.prt_render(self._ctx, C.byref(cam), C.byref(params), width, height, start_idx, end_idx,
                                         out.ctypes.data_as(C.c_void_p), C.byref(counters)), "prt_render")
        return out, counters

    def render_pixels(self, cam: PrtCamera, params: PrtParams, width: int, height: int, pixel_ids) -> Tuple[np.ndarray, PrtCounters]:
        ids = np.ascontiguousarray(pixel_ids, dtype=np.uint32).reshape(-1)
        out = np.empty((ids.size, 4), dtype=np.float32)
        counters = PrtCounters()
        self._check(self._lib.prt_render_pixel_list(self._ctx, C.byref(cam), C.byref(params), width, height,
                                                    ids.ctypes.data_as(C.c_void_p), ids.size,
                                                    out.ctypes.data_as(C.c_void_p), C.byref(counters)), "prt_render_pixel_list")
        return out, counters

    def render_lattice(self, cam, params, width: int, height: int, lattice: int) -> Tuple[np.ndarray, PrtCounters]:
        """Pixels (x % lattice == 0, y % lattice == 0), returned as [lh, lw, 4] like the oracle's lattice output."""
        xs = np.arange(0, width, lattice, dtype=np.uint32)
        ys = np.arange(0, height, lattice, dtype=np.uint32)
        ids = (ys[:, None] * np.uint32(width) + xs[None, :]).reshape(-1)
        out, ctr = self.render_pixels(cam, params, width, height, ids)
        return out.reshape(len(ys), len(xs), 4), ctr

    def render_device(self, cam, params, width, height, start_idx, end_idx, d_ptr: int,
                      want_counters: bool = True) -> Optional[PrtCounters]:
        counters = PrtCounters() if want_counters else None
        self._check(self._lib.prt_render_device(self._ctx, C.byref(cam), C.byref(params), width, height, start_idx,
                                                end_idx, C.c_void_p(d_ptr),
                                                C.byref(counters) if want_counters else None), "prt_render_device")
        return counters

    def shard_rows(self, height: int, block_rows: int, rank: int, nranks: int) -> int:
        return int(self._lib.prt_shard_rows(height, block_rows, rank, nranks))

    def render_shard_device(self, cam, params, width, height, block_rows, rank, nranks, d_ptr: int,
                            want_counters: bool = True) -> Optional[PrtCounters]:
        counters = PrtCounters() if want_counters else None
        self._check(self._lib.prt_render_shard_device(self._ctx, C.byref(cam), C.byref(params), width, height,
                                                      block_rows, rank, nranks, C.c_void_p(d_ptr),
                                                      C.byref(counters) if want_counters else None),
                    "prt_render_shard_device")
        return counters

    def render_shard(self, cam, params, width, height, block_rows, rank, nranks) -> Tuple[np.ndarray, PrtCounters]:
        rows = self.shard_rows(height, block_rows, rank, nranks)
        out = np.empty((rows, width, 4), dtype=np.float32)
        counters = PrtCounters()
        self._check(self._lib.prt_render_shard(self._ctx, C.byref(cam), C.byref(params), width, height, block_rows,
                                               rank, nranks, out.ctypes.data_as(C.c_void_p), C.byref(counters)),
                    "prt_render_shard")
        return out, counters

    def device_kat(self, kind: int, records: np.ndarray, out_shape, out_dtype, cam: Optional[PrtCamera] = None) -> np.ndarray:
        """Run one device function on `records` (see csrc/kernels_debug.h); test hook."""
        rec = np.ascontiguousarray(records)
        out = np.zeros(out_shape, dtype=out_dtype)
        self._check(self._lib.prt_debug_device_kat(self._ctx, int(kind), rec.ctypes.data_as(C.c_void_p), rec.nbytes,
                                                   out.ctypes.data_as(C.c_void_p), out.nbytes, rec.shape[0],
                                                   C.byref(cam) if cam is not None else None), "prt_debug_device_kat")
        return out

    def _arrays(self, first):
        """What the batched queries do to their arrays, decided by the call's first one: numpy arrays go to the host entry points,
        torch tensors on this context's device to the `_device` ones.  Returns (check, empty, ptr, sync, suffix):
        check(x, what, shape, dtypes=(np.float32,)) returns x as a contiguous array or tensor of that shape (None in it: any
        length) or raises ValueError, empty(shape, dtype) allocates an output where the inputs live, ptr(x) is its address (None
        for None), sync() orders the library's stream behind torch's, suffix names the entry point.  dtypes are numpy's; torch
        has no uint32 and carries those bits as int32 (vertex0: a miss, 0xFFFFFFFF, reads -1)."""
        def fits(got, shape):
            return len(got) == len(shape) and all(s is None or s == g for g, s in zip(got, shape))

        def shown(shape):
            return "(%s)" % ", ".join("n" if s is None else str(s) for s in shape) if None in shape else str(shape)
        if type(first).__module__.split(".")[0] == "torch":
            import torch
            tdt = {np.float32: torch.float32, np.uint32: torch.int32, np.int32: torch.int32, np.uint8: torch.uint8}

            def check(x, what, shape, dtypes=(np.float32,)):
                names = " or ".join(str(d) for d in dict.fromkeys(tdt[d] for d in dtypes))
                if not isinstance(x, torch.Tensor) or x.dtype not in [tdt[d] for d in dtypes] or not x.is_contiguous():
                    raise ValueError("%s must be a contiguous %s torch tensor" % (what, names))
                if x.device.type != "cuda" or (x.device.index or 0) != self.device_id:
                    raise ValueError("%s must live on this context's device (cuda:%d)" % (what, self.device_id))
                if not fits(tuple(x.shape), shape):
                    raise ValueError("%s has shape %s, not %s" % (what, tuple(x.shape), shown(shape)))
                return x
            empty = lambda shape, dtype=np.float32: torch.empty(shape, dtype=tdt[dtype], device=first.device)    # noqa: E731
            ptr = lambda x: x.data_ptr() if x is not None else None                                             # noqa: E731
            # the library's stream is not ordered against torch's: whatever torch still has queued on the inputs must be done
            sync = lambda: torch.cuda.current_stream(first.device).synchronize()                                # noqa: E731
            return check, empty, ptr, sync, "_device"

        def check(x, what, shape, dtypes=(np.float32,)):
            a = np.asarray(x)
            if a.dtype not in dtypes or not a.flags["C_CONTIGUOUS"]:
                raise ValueError("%s must be a contiguous %s array" % (what, " or ".join(np.dtype(d).name for d in dtypes)))
            if not fits(a.shape, shape):
                raise ValueError("%s has shape %s, not %s" % (what, a.shape, shown(shape)))
            return a
        empty = lambda shape, dtype=np.float32: np.empty(shape, dtype=dtype)    # noqa: E731
        ptr = lambda x: x.ctypes.data if x is not None else None                # noqa: E731
        return check, empty, ptr, lambda: None, ""

    # (name, components per ray, numpy dtype) of prt_hit_buffers' fields
    HIT_FIELDS = (("t", 1, np.float32), ("bw", 3, np.float32), ("vertex0", 1, np.uint32), ("group", 1, np.int32),
                  ("position", 3, np.float32), ("normal", 3, np.float32), ("occluded", 1, np.uint8))
    CLOSEST_FIELDS = ("t", "bw", "vertex0", "group", "position", "normal")

    def trace_rays(self, origins, directions, *, mode: str = "closest", tmax=None, ray_bias: float = 0.0,
                   fields: Optional[Sequence[str]] = None, count_visits: bool = False) -> dict:
        """The reference's TraceRay on n rays against the uploaded scene (prt_trace_rays, include/prt.h).

        origins, directions: float32 (n, 3), contiguous - numpy arrays (host entry point, numpy results) or torch tensors on
        this context's device (device entry point, tensors on that device).  mode "closest" returns the closest hit's fields
        (default all of t, bw, vertex0, group, position, normal), "occluded" the field `occluded` (1 when some front-facing
        triangle is hit below tmax; tmax None = no limit).  Returns {field: array} plus "counters" (PrtCounters)."""
        modes = {"closest": capi.QUERY_CLOSEST, "occluded": capi.QUERY_OCCLUDED}
        if mode not in modes:
            raise ValueError("mode must be 'closest' or 'occluded', not %r" % (mode,))
        m = modes[mode]
        if fields is None:
            fields = self.CLOSEST_FIELDS if m == capi.QUERY_CLOSEST else ("occluded",)
        spec = {name: (k, dt) for name, k, dt in self.HIT_FIELDS}
        for f in fields:
            if f not in spec:
                raise ValueError("unknown hit field %r" % (f,))
            if (f == "occluded") != (m == capi.QUERY_OCCLUDED):
                raise ValueError("field %r is not written in mode %r" % (f, mode))
        check, empty, ptr, sync, suffix = self._arrays(origins)
        origins = check(origins, "origins", (None, 3))
        n = int(origins.shape[0])
        directions = check(directions, "directions", (n, 3))
        if tmax is not None:
            tmax = check(tmax, "tmax", (n,))
        out = {f: empty((n, spec[f][0]) if spec[f][0] > 1 else (n,), spec[f][1]) for f in fields}
        sync()
        batch = capi.PrtRayBatch(ptr(origins), ptr(directions), ptr(tmax) if m == capi.QUERY_OCCLUDED else None, n,
                                 float(ray_bias))
        hb = capi.PrtHitBuffers(*[ptr(out[name]) if name in out else None for name, _, _ in self.HIT_FIELDS])
        counters = PrtCounters()
        flags = capi.FLAG_COUNT_VISITS if count_visits else 0
        name = "prt_trace_rays" + suffix
        self._check(getattr(self._lib, name)(self._ctx, m, C.byref(batch), C.byref(hb), flags, C.byref(counters)), name)
        out["counters"] = counters
        return out

    # (name, components per slot, numpy dtype) of prt_hits_buffers' fields; hit_count is per ray
    HITS_FIELDS = (("hit_count", 0, np.uint32), ("t", 1, np.float32), ("bw", 3, np.float32), ("vertex0", 1, np.uint32), ("group", 1, np.int32),
                   ("back", 1, np.uint8))

    def trace_hits(self, origins, directions, k: int, *, tmax=None, ray_bias: float = 0.0, back_faces: bool = False, after=None,
                   fields: Optional[Sequence[str]] = None, count_visits: bool = False) -> dict:
        """The k nearest hits of n rays in key order (t, group, vertex0), front faces or both sides (prt_trace_hits, include/prt.h).

        origins, directions: float32 (n, 3), contiguous - numpy arrays (host entry point, numpy results) or torch tensors on this
        context's device (device entry point, tensors on that device).  k: slots per ray, 1..16.  tmax: None, or float32 (n,).
        after: None, a previous result of this call (it then needs hit_count, t, group and vertex0: the cursor is each ray's last
        filled slot, and a ray that had no hit gets nothing again), or a (t, group, vertex0) triple of float32, int32 and uint32
        (torch: int32) arrays of shape (n,); group < 0 means no cursor for that ray.  fields: any of hit_count, t, bw, vertex0, group,
        back (default all).  Returns {field: array} shaped (n,) for hit_count, (n, k) and (n, k, 3) for the others, plus
        "counters" (PrtCounters).  Slots from hit_count on hold the miss record."""
        spec = {name: (c, dt) for name, c, dt in self.HITS_FIELDS}
        if fields is None:
            fields = tuple(spec)
        for f in fields:
            if f not in spec:
                raise ValueError("unknown hits field %r" % (f,))
        k = int(k)
        check, empty, ptr, sync, suffix = self._arrays(origins)
        origins = check(origins, "origins", (None, 3))
        n = int(origins.shape[0])
        directions = check(directions, "directions", (n, 3))
        if tmax is not None:
            tmax = check(tmax, "tmax", (n,))
        cursor = (None, None, None)
        if isinstance(after, dict):
            for f in ("hit_count", "t", "group", "vertex0"):
                if f not in after:
                    raise ValueError("after: a previous result needs the field %r" % (f,))
            count, kk = after["hit_count"], int(after["t"].shape[1]) if len(after["t"].shape) == 2 else 0
            check(after["t"], "after['t']", (n, kk)), check(count, "after['hit_count']", (n,), (np.uint32,))
            if suffix:
                import torch
                rows = torch.arange(n, device=origins.device)
                at = (count.long() - 1).clamp(min=0)
                some = count > 0
                cursor = (torch.where(some, after["t"][rows, at], torch.full_like(after["t"][:, 0], float("inf"))).contiguous(),
                          torch.where(some, after["group"][rows, at], torch.zeros_like(after["group"][:, 0])).contiguous(),
                          torch.where(some, after["vertex0"][rows, at], torch.zeros_like(after["vertex0"][:, 0])).contiguous())
            else:
                rows = np.arange(n)
                at = np.maximum(count.astype(np.int64) - 1, 0)
                some = count > 0
                cursor = (np.ascontiguousarray(np.where(some, after["t"][rows, at], np.float32(np.inf)), np.float32),
                          np.ascontiguousarray(np.where(some, after["group"][rows, at], 0), np.int32),
                          np.ascontiguousarray(np.where(some, after["vertex0"][rows, at], 0), np.uint32))
        elif after is not None:
            if len(after) != 3:
                raise ValueError("after must be a previous result or a (t, group, vertex0) triple")
            cursor = (check(after[0], "after t", (n,)), check(after[1], "after group", (n,), (np.int32,)),
                      check(after[2], "after vertex0", (n,), (np.uint32,)))
        shape = lambda c: (n,) if c == 0 else ((n, k) if c == 1 else (n, k, c))    # noqa: E731
        out = {f: empty(shape(spec[f][0]), spec[f][1]) for f in fields} if 1 <= k <= capi.MAX_HITS else {}
        sync()
        rq = capi.PrtHitsRequest(capi.PrtRayBatch(ptr(origins), ptr(directions), ptr(tmax), n, float(ray_bias)), k,
                                 capi.HITS_BACK_FACES if back_faces else 0, *[ptr(c) for c in cursor])
        hb = capi.PrtHitsBuffers(*[ptr(out[name]) if name in out else None for name, _, _ in self.HITS_FIELDS])
        counters = PrtCounters()
        flags = capi.FLAG_COUNT_VISITS if count_visits else 0
        name = "prt_trace_hits" + suffix
        self._check(getattr(self._lib, name)(self._ctx, C.byref(rq), C.byref(hb), flags, C.byref(counters)), name)
        out["counters"] = counters
        return out

    # (name, components per point, numpy dtype) of prt_closest_buffers' fields
    CLOSEST_POINT_FIELDS = (("dist2", 1, np.float32), ("point", 3, np.float32), ("bw", 3, np.float32), ("vertex0", 1, np.uint32),
                            ("group", 1, np.int32))

    def closest_points(self, points, *, max_dist=None, fields: Optional[Sequence[str]] = None, count_visits: bool = False) -> dict:
        """The nearest point of the uploaded surface for n points (prt_closest_points, include/prt.h).

        points: float32 (n, 3), contiguous - a numpy array (host entry point, numpy results) or a torch tensor on this context's
        device (device entry point, tensors on that device).  max_dist: None, or float32 (n,) DISTANCES: the wrapper squares them
        in float32 (max_dist * max_dist, rounded once) and passes the squares as max_dist2; a triangle is a candidate when its
        squared distance is <= that square.  fields: any of dist2, point, bw, vertex0, group (default all).  Returns {field: array}
        plus "distance" = sqrt(dist2) when dist2 is among the fields - inf on a miss - and "counters" (PrtCounters)."""
        return self._point_query(points, max_dist, fields, count_visits, False)

    # prt_signed_buffers' own fields, behind prt_closest_buffers'
    SIGNED_DISTANCE_FIELDS = (("signed_distance", 1, np.float32), ("feature", 1, np.uint8))

    def signed_distance(self, points, *, max_dist=None, fields: Optional[Sequence[str]] = None, count_visits: bool = False) -> dict:
        """The nearest point of the uploaded surface and the side of it that n points lie on (prt_signed_distance, include/prt.h).

        points, max_dist, count_visits: as closest_points takes them.  fields: any of closest_points' fields, signed_distance and
        feature (default all).  Returns what closest_points returns plus "signed_distance" (+-sqrt(dist2), FLT_MAX on a miss),
        "feature" (uint8: the region 0..6 whose normal decided the sign, 255 on a miss) and, with signed_distance among the
        fields, "inside" = signed_distance < 0 (bool).  On a closed, consistently wound mesh inside is containment; on an open
        mesh it is the side of the nearest surface element."""
        return self._point_query(points, max_dist, fields, count_visits, True)

    def _point_query(self, points, max_dist, fields, count_visits, signed) -> dict:
        """closest_points and signed_distance: the same batch and buffers, one of the two entry points."""
        all_fields = self.CLOSEST_POINT_FIELDS + (self.SIGNED_DISTANCE_FIELDS if signed else ())
        spec = {name: (k, dt) for name, k, dt in all_fields}
        if fields is None:
            fields = tuple(spec)
        for f in fields:
            if f not in spec:
                raise ValueError("unknown %s field %r" % ("signed-distance" if signed else "closest-point", f))
        check, empty, ptr, sync, suffix = self._arrays(points)
        points = check(points, "points", (None, 3))
        n = int(points.shape[0])
        max_d2 = None
        if max_dist is not None:
            max_dist = check(max_dist, "max_dist", (n,))
            if suffix:
                max_d2 = (max_dist * max_dist).contiguous()
            else:
                with np.errstate(over="ignore"):
                    max_d2 = np.ascontiguousarray(max_dist * max_dist, np.float32)
        out = {f: empty((n, spec[f][0]) if spec[f][0] > 1 else (n,), spec[f][1]) for f in fields}
        sync()
        name = ("prt_signed_distance" if signed else "prt_closest_points") + suffix
        batch = capi.PrtPointBatch(ptr(points), ptr(max_d2), n)
        cb = capi.PrtClosestBuffers(*[ptr(out[f]) if f in out else None for f, _, _ in self.CLOSEST_POINT_FIELDS])
        if signed:
            cb = capi.PrtSignedBuffers(cb, *[ptr(out[f]) if f in out else None for f, _, _ in self.SIGNED_DISTANCE_FIELDS])
        counters = PrtCounters()
        flags = capi.FLAG_COUNT_VISITS if count_visits else 0
        self._check(getattr(self._lib, name)(self._ctx, C.byref(batch), C.byref(cb), flags, C.byref(counters)), name)
        if "dist2" in out:
            d2 = out["dist2"]
            if suffix:
                import torch
                out["distance"] = torch.where(d2 < 3.4028234663852886e38, d2.sqrt(), torch.full_like(d2, float("inf")))
            else:
                out["distance"] = np.where(d2 < np.float32(3.4028234663852886e38), np.sqrt(d2), np.float32(np.inf)).astype(np.float32)
        if "signed_distance" in out:
            out["inside"] = out["signed_distance"] < 0
        out["counters"] = counters
        return out

    GRAD_NAMES = ("positions", "origins", "directions")

    def trace_rays_backward(self, origins, directions, group, vertex0, positions, *, ray_bias: float = 0.0, grad_t=None, grad_bw=None,
                            grad_position=None, grad_normal=None, want: Sequence[str] = ("positions", "origins", "directions")) -> dict:
        """Gradients of a closest-hit query (prt_trace_rays_backward, include/prt.h): from dL/dt, dL/dbw, dL/dposition, dL/dnormal
        of n rays (None = zero) to dL/dpositions (summed over the rays; the same bits for every order of the rays), dL/dorigins and
        dL/ddirections - whichever `want` names.

        origins, directions, ray_bias, group, vertex0: the forward trace_rays call's inputs and hit references (vertex0 uint32, or
        int32 holding the same bits); positions: float32 (P, 3), the vertices that call saw.  numpy arrays go to the host entry
        point, torch tensors on this context's device to the device entry point.  Returns {name: array} plus "info" (PrtGradInfo)."""
        for w in want:
            if w not in self.GRAD_NAMES:
                raise ValueError("unknown gradient %r" % (w,))
        check, empty, ptr, sync, suffix = self._arrays(origins)
        name = "prt_trace_rays_backward" + suffix
        if getattr(origins, "ndim", 0) != 2:
            raise ValueError("origins must have shape (n, 3)")
        n = int(origins.shape[0])
        if getattr(positions, "ndim", 0) != 2:
            raise ValueError("positions must have shape (P, 3)")
        n_pos = int(positions.shape[0])
        origins = check(origins, "origins", (n, 3))
        directions = check(directions, "directions", (n, 3))
        group = check(group, "group", (n,), (np.int32,))
        vertex0 = check(vertex0, "vertex0", (n,), (np.int32, np.uint32))
        positions = check(positions, "positions", (n_pos, 3))
        gouts = [None if g is None else check(g, what, shape) for g, what, shape in
                 ((grad_t, "grad_t", (n,)), (grad_bw, "grad_bw", (n, 3)), (grad_position, "grad_position", (n, 3)),
                  (grad_normal, "grad_normal", (n, 3)))]
        out = {w: empty((n_pos, 3) if w == "positions" else (n, 3)) for w in want}
        sync()
        batch = capi.PrtRayBatch(ptr(origins), ptr(directions), None, n, float(ray_bias))
        go = capi.PrtHitGrads(*[ptr(g) for g in gouts])
        gi = capi.PrtQueryGrads(*[ptr(out.get(w)) for w in self.GRAD_NAMES])
        info = PrtGradInfo()
        self._check(getattr(self._lib, name)(self._ctx, C.byref(batch), ptr(group), ptr(vertex0), ptr(positions), n_pos, C.byref(go),
                                             C.byref(gi), C.byref(info)), name)
        out["info"] = info
        return out

    POINT_GRAD_NAMES = ("positions", "points")

    def closest_points_backward(self, points, group, vertex0, positions, *, grad_dist2=None, grad_point=None, grad_bw=None,
                                want: Sequence[str] = ("positions", "points")) -> dict:
        """Gradients of a closest-point query (prt_closest_points_backward, include/prt.h): from dL/ddist2, dL/dpoint, dL/dbw of n
        points (None = zero) to dL/dpositions (summed over the points; the same bits for every order of the points) and
        dL/dpoints - whichever `want` names.

        points, group, vertex0: the forward closest_points call's input and references (vertex0 uint32, or int32 holding the same
        bits); positions: float32 (P, 3), the vertices that call saw.  numpy arrays go to the host entry point, torch tensors on
        this context's device to the device entry point.  Returns {name: array} plus "info" (PrtGradInfo)."""
        for w in want:
            if w not in self.POINT_GRAD_NAMES:
                raise ValueError("unknown gradient %r" % (w,))
        check, empty, ptr, sync, suffix = self._arrays(points)
        name = "prt_closest_points_backward" + suffix
        if getattr(points, "ndim", 0) != 2:
            raise ValueError("points must have shape (n, 3)")
        n = int(points.shape[0])
        if getattr(positions, "ndim", 0) != 2:
            raise ValueError("positions must have shape (P, 3)")
        n_pos = int(positions.shape[0])
        points = check(points, "points", (n, 3))
        group = check(group, "group", (n,), (np.int32,))
        vertex0 = check(vertex0, "vertex0", (n,), (np.int32, np.uint32))
        positions = check(positions, "positions", (n_pos, 3))
        gouts = [None if g is None else check(g, what, shape) for g, what, shape in
                 ((grad_dist2, "grad_dist2", (n,)), (grad_point, "grad_point", (n, 3)), (grad_bw, "grad_bw", (n, 3)))]
        out = {w: empty((n_pos, 3) if w == "positions" else (n, 3)) for w in want}
        sync()
        batch = capi.PrtPointBatch(ptr(points), None, n)
        go = capi.PrtClosestGrads(*[ptr(g) for g in gouts])
        gi = capi.PrtPointGrads(*[ptr(out.get(w)) for w in self.POINT_GRAD_NAMES])
        info = PrtGradInfo()
        self._check(getattr(self._lib, name)(self._ctx, C.byref(batch), ptr(group), ptr(vertex0), ptr(positions), n_pos, C.byref(go),
                                             C.byref(gi), C.byref(info)), name)
        out["info"] = info
        return out

    # (name, components per sample, numpy dtype) of prt_sample_buffers' fields
    SAMPLE_FIELDS = (("point", 3, np.float32), ("bw", 3, np.float32), ("normal", 3, np.float32), ("vertex0", 1, np.uint32),
                     ("group", 1, np.int32))

    def sample_surface(self, count: int, *, seed: int = 0, first: int = 0, fields: Optional[Sequence[str]] = None, out: str = "numpy") -> dict:
        """`count` points on the uploaded surface, drawn uniformly by area (prt_sample_surface, include/prt.h): samples
        first .. first + count - 1 of `seed`, a pure function of (scene as it lies on the device, seed, sample index).

        fields: any of point, bw, normal, vertex0, group (default all).  out: "numpy" (host entry point, numpy results) or
        "torch" (device entry point, tensors on this context's device; vertex0 carries its bits as int32).  Returns
        {field: array} plus "info" (PrtSampleInfo: area, total_weight, unit_exponent, live_triangles, device_ms, table_ms)."""
        spec = {name: (k, dt) for name, k, dt in self.SAMPLE_FIELDS}
        if fields is None:
            fields = tuple(spec)
        for f in fields:
            if f not in spec:
                raise ValueError("unknown sample field %r" % (f,))
        if out not in ("numpy", "torch"):
            raise ValueError("out must be 'numpy' or 'torch', not %r" % (out,))
        n = int(count)
        if n < 0 or n >= 1 << 32 or int(first) < 0 or int(seed) < 0:
            raise ValueError("count must be in 0 .. 2^32 - 1, first and seed non-negative")
        if out == "torch":
            import torch
            like = torch.empty(0, device="cuda:%d" % self.device_id)
        else:
            like = np.empty(0, np.float32)
        _check, empty, ptr, sync, suffix = self._arrays(like)
        res = {f: empty((n, spec[f][0]) if spec[f][0] > 1 else (n,), spec[f][1]) for f in fields}
        sync()
        name = "prt_sample_surface" + suffix
        rq = capi.PrtSampleRequest(int(seed) & 0xFFFFFFFFFFFFFFFF, int(first), n)
        sb = capi.PrtSampleBuffers(*[ptr(res[f]) if f in res else None for f, _, _ in self.SAMPLE_FIELDS])
        info = capi.PrtSampleInfo()
        self._check(getattr(self._lib, name)(self._ctx, C.byref(rq), C.byref(sb), C.byref(info)), name)
        res["info"] = info
        return res

    # (name, components per point, numpy dtype) of prt_hemi_buffers' fields
    HEMI_FIELDS = (("unoccluded", 1, np.uint32), ("visibility", 1, np.float32), ("bent", 3, np.float32))

    def hemisphere_visibility(self, points, normals, *, samples: int = 64, seed: int = 0, first: int = 0, max_dist=None,
                              ray_bias: float = 0.0, fields: Optional[Sequence[str]] = None, count_visits: bool = False) -> dict:
        """Which part of a cosine lobe around n points' normals is unoccluded (prt_hemisphere_visibility, include/prt.h).

        points, normals: float32 (n, 3), contiguous, the normals unit length - numpy arrays (host entry point, numpy results) or
        torch tensors on this context's device (device entry point, tensors on that device).  samples rays are cast per point,
        drawn from the reference's 1024-direction lobe by (seed, first + i, s); max_dist: None, or float32 (n,), the rays' reach.
        fields: any of unoccluded (uint32, int32 in torch: the rays nothing occludes, 0xFFFFFFFF for an invalid point), visibility
        (unoccluded / samples) and bent (n, 3: the mean unoccluded direction); default all.  Returns {field: array} plus "counters"
        (PrtCounters)."""
        spec = {name: (k, dt) for name, k, dt in self.HEMI_FIELDS}
        if fields is None:
            fields = tuple(spec)
        for f in fields:
            if f not in spec:
                raise ValueError("unknown hemisphere-visibility field %r" % (f,))
        check, empty, ptr, sync, suffix = self._arrays(points)
        points = check(points, "points", (None, 3))
        n = int(points.shape[0])
        normals = check(normals, "normals", (n, 3))
        if max_dist is not None:
            max_dist = check(max_dist, "max_dist", (n,))
        out = {f: empty((n, spec[f][0]) if spec[f][0] > 1 else (n,), spec[f][1]) for f in fields}
        sync()
        if not 0 <= int(samples) < 1 << 32 or not 0 <= int(first) < 1 << 64 or int(seed) < 0:
            raise ValueError("samples must be in 0 .. 2^32 - 1, first in 0 .. 2^64 - 1 and seed non-negative")
        # what the C types hold goes to the library as given: its refusals (samples, first + count) are the check
        batch = capi.PrtHemiBatch(ptr(points), ptr(normals), ptr(max_dist), n, int(samples), int(seed) & 0xFFFFFFFFFFFFFFFF, int(first),
                                  float(ray_bias))
        hb = capi.PrtHemiBuffers(*[ptr(out[name]) if name in out else None for name, _, _ in self.HEMI_FIELDS])
        counters = PrtCounters()
        flags = capi.FLAG_COUNT_VISITS if count_visits else 0
        name = "prt_hemisphere_visibility" + suffix
        self._check(getattr(self._lib, name)(self._ctx, C.byref(batch), C.byref(hb), flags, C.byref(counters)), name)
        out["counters"] = counters
        return out

    def render_rays(self, origins, directions, params: PrtParams, *, first: int = 0, camera_stream: bool = False):
        """The radiance TraceRayColor returns along the caller's rays (prt_render_rays, include/prt.h): lights, shadow rays,
        textures, alpha maps and the bounce tree, for rays that are no pinhole pixel's.  par_raytracer_amd.cameras makes rays.

        origins, directions: float32, contiguous, (count, spp, 3) or (count * spp, 3) with spp = params.spp - numpy arrays (host
        entry point, a numpy result) or torch tensors on this context's device (device entry point, a tensor on that device).  Ray
        i * spp + s is sample s of output first + i and draws from the stream prt_render gives sample s of pixel first + i;
        camera_stream first drops the two draws RenderPixel spends on the jitter.  The directions must be unit length and are used
        as given; a ray outside the domain makes the library refuse the whole batch.  Returns (rgba (count, 4), PrtCounters)."""
        spp = int(params.spp)
        check, empty, ptr, sync, suffix = self._arrays(origins)
        if len(origins.shape) == 3:
            origins = check(origins, "origins", (None, spp, 3))
            count = int(origins.shape[0])
            directions = check(directions, "directions", (count, spp, 3))
        else:
            origins = check(origins, "origins", (None, 3))
            rays = int(origins.shape[0])
            if spp < 1 or rays % spp:
                raise ValueError("origins holds %d rays, not a multiple of params.spp = %d" % (rays, spp))
            count = rays // spp
            directions = check(directions, "directions", (rays, 3))
        if not 0 <= int(first) < 1 << 64:
            raise ValueError("first must be in 0 .. 2^64 - 1")
        out = empty((count, 4))
        sync()
        # what the C types hold goes to the library as given: its refusals (spp, first + count, the domain) are the check
        batch = capi.PrtRadianceBatch(ptr(origins), ptr(directions), count, capi.RAYS_CAMERA_STREAM if camera_stream else 0, int(first))
        counters = PrtCounters()
        name = "prt_render_rays" + suffix
        self._check(getattr(self._lib, name)(self._ctx, C.byref(batch), C.byref(params), ptr(out), C.byref(counters)), name)
        return out, counters

    def sample_surface_backward(self, group, vertex0, bw, positions, *, grad_point=None, grad_normal=None) -> dict:
        """Gradients of surface samples (prt_sample_surface_backward, include/prt.h): from dL/dpoint and dL/dnormal of n samples
        (None = zero) to dL/dpositions, summed over the samples - the same bits for every order of the samples.

        group, vertex0, bw: the forward sample_surface call's outputs (vertex0 uint32, or int32 holding the same bits);
        positions: float32 (P, 3), the vertices that call saw.  numpy arrays go to the host entry point, torch tensors on this
        context's device to the device entry point (decided by `group`).  Returns {"positions": array, "info": PrtGradInfo}."""
        check, empty, ptr, sync, suffix = self._arrays(group)
        name = "prt_sample_surface_backward" + suffix
        if getattr(group, "ndim", 0) != 1:
            raise ValueError("group must have shape (n,)")
        n = int(group.shape[0])
        if getattr(positions, "ndim", 0) != 2:
            raise ValueError("positions must have shape (P, 3)")
        n_pos = int(positions.shape[0])
        group = check(group, "group", (n,), (np.int32,))
        vertex0 = check(vertex0, "vertex0", (n,), (np.int32, np.uint32))
        bw = check(bw, "bw", (n, 3))
        positions = check(positions, "positions", (n_pos, 3))
        gouts = [None if g is None else check(g, what, (n, 3)) for g, what in ((grad_point, "grad_point"), (grad_normal, "grad_normal"))]
        out = {"positions": empty((n_pos, 3))}
        sync()
        go = capi.PrtSampleGrads(*[ptr(g) for g in gouts])
        info = PrtGradInfo()
        self._check(getattr(self._lib, name)(self._ctx, n, ptr(group), ptr(vertex0), ptr(bw), ptr(positions), n_pos, C.byref(go),
                                             ptr(out["positions"]), C.byref(info)), name)
        out["info"] = info
        return out

    def update_geometry(self, positions, normals=None, tangents=None, spheres=None, sphere_group=None) -> PrtUpdateInfo:
        """Move the uploaded scene's vertices in place and refit the tree on the device (prt_update_geometry, include/prt.h):
        afterwards renders and queries give the bits a fresh upload of the moved scene would.

        positions (and optionally normals, tangents): float32 (n, 3) or flat, contiguous, with the uploaded scene's counts - numpy
        arrays (host entry point) or torch tensors on this context's device (device entry point).  spheres, sphere_group: the
        reference's hierarchy of the MOVED scene as HOST data - the raw prt_bsphere bytes and int32 groups of api.desc_arrays(),
        or ctypes pointers with a count as (pointer, count) - or None (ranks in input order, as an upload without spheres)."""
        is_torch = type(positions).__module__.split(".")[0] == "torch"
        keep = []
        if is_torch:
            import torch

            def conv(x, what):
                if x is None:
                    return None, 0
                if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or not x.is_contiguous():
                    raise ValueError("%s must be a contiguous float32 torch tensor" % what)
                if x.device.type != "cuda" or (x.device.index or 0) != self.device_id:
                    raise ValueError("%s must live on this context's device (cuda:%d)" % (what, self.device_id))
                if x.numel() % 3:
                    raise ValueError("%s has %d floats, not a multiple of 3" % (what, x.numel()))
                keep.append(x)
                return x.data_ptr(), x.numel() // 3
            # the library's stream is not ordered against torch's: whatever torch still has queued on the inputs must be done
            torch.cuda.current_stream(positions.device).synchronize()
            entry, name = self._lib.prt_update_geometry_device, "prt_update_geometry_device"
        else:
            def conv(x, what):
                if x is None:
                    return None, 0
                a = np.asarray(x)
                if a.dtype != np.float32 or not a.flags["C_CONTIGUOUS"]:
                    raise ValueError("%s must be a contiguous float32 array" % what)
                if a.size % 3:
                    raise ValueError("%s has %d floats, not a multiple of 3" % (what, a.size))
                keep.append(a)
                return a.ctypes.data, a.size // 3
            entry, name = self._lib.prt_update_geometry, "prt_update_geometry"
        u = capi.PrtGeometryUpdate()
        u.positions, u.position_count = conv(positions, "positions")
        u.normals, u.normal_count = conv(normals, "normals")
        u.tangents, n_tan = conv(tangents, "tangents")
        if tangents is not None and normals is not None and n_tan != u.normal_count:
            raise ValueError("tangents come one per normal")
        if spheres is not None and sphere_group is not None:
            if isinstance(spheres, tuple):
                (sp, count), sg = spheres, sphere_group
                u.spheres, u.sphere_group, u.sphere_count = sp, sg, int(count)
            else:
                sp = np.ascontiguousarray(np.asarray(spheres)).view(np.uint8).reshape(-1)
                sg = np.ascontiguousarray(np.asarray(sphere_group), dtype=np.int32).reshape(-1)
                if sp.size != sg.size * C.sizeof(capi.PrtBSphere):
                    raise ValueError("spheres holds %d bytes for %d sphere groups" % (sp.size, sg.size))
                keep += [sp, sg]
                if sg.size:
                    u.spheres = sp.ctypes.data_as(C.POINTER(capi.PrtBSphere))
                    u.sphere_group = sg.ctypes.data_as(C.POINTER(C.c_int32))
                    u.sphere_count = sg.size
        info = PrtUpdateInfo()
        self._check(entry(self._ctx, C.byref(u), C.byref(info)), name)
        return info

    def check_refit(self, moved_scene) -> dict:
        """prt_debug_check_refit: the geometric BVH check on the tree as it lies on the device now, against moved_scene's triangles."""
        desc = moved_scene.desc if isinstance(moved_scene, (HostScene, FlatDesc)) else moved_scene
        out = (C.c_uint64 * 6)()
        self._check(self._lib.prt_debug_check_refit(self._ctx, desc, out), "prt_debug_check_refit")
        return dict(zip(("violations", "nodes", "depth", "stack_bound", "leaves", "refs"), (int(v) for v in out)))

    def lbvh_tree(self, verts9, keys: bool = True) -> dict:
        """prt_debug_lbvh_tree: the GPU builder's radix tree over the un-indexed triangles verts9 (float32, n x 9 or n x 3 x 3), as the
        device made it: left, right, first, last, node_box (ni, 6), leaf_box (n, 6), sorted_ids and - keys=True - sorted_keys
        (uint64).  ni = max(n - 1, 1); for n = 1 the per-node arrays are unspecified (include/prt.h)."""
        v = np.ascontiguousarray(verts9, np.float32).reshape(-1, 9)
        n = v.shape[0]
        ni = max(n - 1, 1)
        out = dict(left=np.zeros(ni, np.int32), right=np.zeros(ni, np.int32), first=np.zeros(ni, np.uint32), last=np.zeros(ni, np.uint32),
                   node_box=np.zeros((ni, 6), np.float32), leaf_box=np.zeros((n, 6), np.float32), sorted_ids=np.zeros(n, np.uint32))
        if keys:
            out["sorted_keys"] = np.zeros(n, np.uint64)
        names = ("left", "right", "first", "last", "node_box", "leaf_box", "sorted_ids", "sorted_keys")
        self._check(self._lib.prt_debug_lbvh_tree(self._ctx, n, v.ctypes.data, *[out[k].ctypes.data if k in out else None for k in names]),
                    "prt_debug_lbvh_tree")
        return out

    def close(self):
        if self._ctx:
            self._lib.prt_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
