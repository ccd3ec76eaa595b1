"""What the ten batched-query entry points answer when they refuse a call: the return code, the exact bytes of prt_last_error, and
that no output of the caller's was written.  The texts are literal copies of the library's source as of the commit that wrote the
queries' host path once; a text that changes is a change of behaviour and belongs in this table.  Two quirks are pinned as they
are: the signed-distance calls refuse under prt_closest_points' name, and every _device form under its host form's name.

Scene: the 4-triangle tetrahedron of signed_cases.py; batches of 3 items."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import signed_cases as S

pytestmark = pytest.mark.gpu

N = 3
SENTINEL = 0xA5
INVALID = (b" name a triangle the scene does not have (group out of range, vertex0 not a multiple of 3 or past its "
           b"group's run)")

# case -> (return code, prt_last_error); None: the context is null, nothing can hold a text
RAYS = {
    "null context": (-1, None),
    "unknown mode": (-1, b"prt_trace_rays: unknown mode"),
    "null batch": (-1, b"prt_trace_rays: null batch"),
    "null array": (-1, b"prt_trace_rays: null origins or directions"),
    "no scene": (-2, b"prt_trace_rays: no scene uploaded"),
}
POINTS = {
    "null context": (-1, None),
    "null batch": (-1, b"prt_closest_points: null batch or buffers"),
    "null array": (-1, b"prt_closest_points: null points"),
    "null output": (-1, b"prt_closest_points: null batch or buffers"),
    "no scene": (-2, b"prt_closest_points: no scene uploaded"),
}
RAYS_BACKWARD = {
    "null context": (-1, None),
    "null batch": (-1, b"prt_trace_rays_backward: null batch"),
    "null array": (-1, b"prt_trace_rays_backward: null origins, directions, group, vertex0 or positions"),
    "no scene": (-2, b"prt_trace_rays_backward: no scene uploaded"),
    "position_count": (-1, b"prt_trace_rays_backward: position_count differs from the uploaded scene's"),
    "group 99": (-1, b"prt_trace_rays_backward: 1 rays" + INVALID),
}
POINTS_BACKWARD = {
    "null context": (-1, None),
    "null batch": (-1, b"prt_closest_points_backward: null batch"),
    "null array": (-1, b"prt_closest_points_backward: null points, group, vertex0 or positions"),
    "no scene": (-2, b"prt_closest_points_backward: no scene uploaded"),
    "position_count": (-1, b"prt_closest_points_backward: position_count differs from the uploaded scene's"),
    "group 99": (-1, b"prt_closest_points_backward: 1 points" + INVALID),
}
ENTRY_POINTS = (("prt_trace_rays", RAYS), ("prt_closest_points", POINTS), ("prt_signed_distance", POINTS),
                ("prt_trace_rays_backward", RAYS_BACKWARD), ("prt_closest_points_backward", POINTS_BACKWARD))


class Arrays:
    """A call's arrays where the entry point wants them: numpy arrays (host form) or torch tensors on device 0 (device form)."""

    def __init__(self, device):
        self.device = device
        self.outputs = []

    def put(self, a):
        a = np.ascontiguousarray(a)
        if not self.device:
            return a
        import torch
        return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to("cuda:0")

    def out(self, items=3 * N):
        """A sentinel-filled output of `items` 4-byte words, remembered for untouched()."""
        x = self.put(np.full(4 * items, SENTINEL, np.uint8))
        self.outputs.append(x)
        return x

    def ptr(self, x):
        return None if x is None else x.data_ptr() if self.device else x.ctypes.data

    def untouched(self):
        return all(bool(((x.cpu().numpy() if self.device else x) == SENTINEL).all()) for x in self.outputs)


def mark(r):
    """Leaves a known other text in prt_last_error, so that the text found after a refusal is that refusal's."""
    with pytest.raises(RuntimeError, match="unknown option"):
        r.set_option("NO_SUCH_OPTION", 1)
    return r._lib.prt_last_error(r._ctx)


def refuse(r, bare, name, case, device):
    """Calls entry point `name` with arguments that are valid but for `case`; returns (rc, the call's Arrays)."""
    from par_raytracer_amd import capi
    a = Arrays(device)
    ctx = None if case == "null context" else r._ctx
    entry = getattr(r._lib, name)
    pts = a.put(np.array([[0.1, 0.2, 0.3], [2.0, 0.0, 0.0], [0.0, -3.0, 0.5]], np.float32))
    dirs = a.put(np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0]], np.float32))
    first = None if case == "null array" else pts
    counters = capi.PrtCounters()
    if bare == "prt_trace_rays":
        batch = capi.PrtRayBatch(a.ptr(first), a.ptr(dirs), None, N, 0.0)
        hb = capi.PrtHitBuffers(*[a.ptr(a.out()) for _ in range(6)], None)
        mode = 7 if case == "unknown mode" else capi.QUERY_CLOSEST
        return entry(ctx, mode, None if case == "null batch" else C.byref(batch), C.byref(hb), 0, C.byref(counters)), a
    if bare in ("prt_closest_points", "prt_signed_distance"):
        batch = capi.PrtPointBatch(a.ptr(first), None, N)
        cb = capi.PrtClosestBuffers(*[a.ptr(a.out()) for _ in range(5)])
        if bare == "prt_signed_distance":
            cb = capi.PrtSignedBuffers(cb, a.ptr(a.out()), a.ptr(a.out()))
        return entry(ctx, None if case == "null batch" else C.byref(batch), None if case == "null output" else C.byref(cb), 0,
                     C.byref(counters)), a
    # the gradient calls: items 0 and 1 name triangles of the tetrahedron, item 2 is a miss - or names group 99
    group = a.put(np.array([0, 0, 99 if case == "group 99" else -1], np.int32))
    vertex0 = a.put(np.array([0, 3, 0 if case == "group 99" else 0xFFFFFFFF], np.uint32))
    positions = a.put(S.tetrahedron()[0])
    n_pos = 5 if case == "position_count" else 4
    info = capi.PrtGradInfo()
    if bare == "prt_trace_rays_backward":
        batch = capi.PrtRayBatch(a.ptr(first), a.ptr(dirs), None, N, 0.0)
        go = capi.PrtHitGrads(*[a.ptr(a.put(np.ones(k, np.float32))) for k in (N, 3 * N, 3 * N, 3 * N)])
        gi = capi.PrtQueryGrads(a.ptr(a.out(3 * 4)), a.ptr(a.out()), a.ptr(a.out()))
    else:
        batch = capi.PrtPointBatch(a.ptr(first), None, N)
        go = capi.PrtClosestGrads(*[a.ptr(a.put(np.ones(k, np.float32))) for k in (N, 3 * N, 3 * N)])
        gi = capi.PrtPointGrads(a.ptr(a.out(3 * 4)), a.ptr(a.out()))
    return entry(ctx, None if case == "null batch" else C.byref(batch), a.ptr(group), a.ptr(vertex0), a.ptr(positions), n_pos, C.byref(go),
                 C.byref(gi), C.byref(info)), a


def test_refusals_code_text_and_untouched_outputs():
    from par_raytracer_amd import api
    with_scene, without = api.Renderer(0), api.Renderer(0)
    try:
        assert with_scene.upload(S.flat_desc(S.tetrahedron())).triangle_count == 4
        checked = 0
        for bare, cases in ENTRY_POINTS:
            for device in (False, True):
                name = bare + ("_device" if device else "")
                for case, (code, text) in cases.items():
                    r = without if case == "no scene" else with_scene
                    marked = mark(r)
                    rc, arrays = refuse(r, bare, name, case, device)
                    what = "%s, %s" % (name, case)
                    assert rc == code, what
                    assert r._lib.prt_last_error(r._ctx) == (marked if text is None else text), what
                    assert arrays.untouched(), what
                    checked += 1
        assert checked == 2 * (len(RAYS) + 2 * len(POINTS) + len(RAYS_BACKWARD) + len(POINTS_BACKWARD))
    finally:
        with_scene.close()
        without.close()
