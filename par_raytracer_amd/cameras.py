"""Ray makers for Renderer.render_rays (prt_render_rays, include/prt.h): pure numpy, float32, no random numbers.

Each returns (origins, directions), float32 arrays of shape (n, 3) with the directions normalised in float32 the way the
reference normalises (mathlib.h:253-262: every component divided by sqrtf(Dot(d, d))) - unit length inside the call's domain.
Sub-pixel positions are the caller's: for `spp` samples per output, pass n = count x spp positions, sample-major per output
(ray i * spp + s is sample s of output i), and jitter them as you like.
"""
from __future__ import annotations

import numpy as np

F = np.float32


def _f3(v) -> np.ndarray:
    return np.asarray(v, dtype=F).reshape(3)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]          # Dot, mathlib.h:236


def _normalize(d: np.ndarray) -> np.ndarray:
    d = np.ascontiguousarray(d, dtype=F)
    l2 = _dot(d, d)
    length = np.sqrt(l2, dtype=F)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where((l2 == 0)[..., None], d, d / length[..., None]).astype(F)


def _basis(facing, up=(0.0, 1.0, 0.0)):
    """(forward, right, up): the reference's camera frame (main.cpp:152-158: right = Cross(forward, up), up = Cross(right, forward))."""
    f = _normalize(_f3(facing))
    r = _normalize(np.cross(f, _f3(up)).astype(F))
    u = np.cross(r, f).astype(F)
    return f, r, u


def pinhole_rays(cam, pixel_xy):
    """MakeCameraRay (main.cpp:164-177) at the caller's sub-pixel positions.  cam: a PrtCamera (api.make_camera); pixel_xy: (n, 2)
    positions in pixels - pixel (x, y)'s centre is (x, y), RenderPixel jitters it by +-0.5.  The expression order is the
    reference's, so the directions are prt_render's bit for bit."""
    p = np.asarray(pixel_xy, dtype=F).reshape(-1, 2)
    nx = F(2.0) * (p[:, 0] + F(0.5)) * F(cam.inv_width) - F(1.0)
    ny = F(1.0) - F(2.0) * (p[:, 1] + F(0.5)) * F(cam.inv_height)
    fwd, right, up = (np.array(list(v), dtype=F) for v in (cam.forward, cam.right, cam.up))
    rs = right * F(cam.tan_a2) * F(cam.aspect)
    us = up * F(cam.tan_a2)
    d = (fwd[None] + rs[None] * nx[:, None]) + us[None] * ny[:, None]
    o = np.tile(np.array(list(cam.position), dtype=F)[None], (p.shape[0], 1))
    return np.ascontiguousarray(o), _normalize(d)


def orthographic_rays(position, facing, half_width: float, half_height: float, uv, up=(0.0, 1.0, 0.0)):
    """Parallel rays along `facing` from a window of 2 half_width x 2 half_height world units centred at `position`.
    uv: (n, 2) window coordinates in [-1, 1] x [-1, 1], +v up."""
    uv = np.asarray(uv, dtype=F).reshape(-1, 2)
    f, r, u = _basis(facing, up)
    o = _f3(position)[None] + r[None] * (uv[:, :1] * F(half_width)) + u[None] * (uv[:, 1:] * F(half_height))
    return np.ascontiguousarray(o, dtype=F), np.ascontiguousarray(np.tile(f[None], (uv.shape[0], 1)))


def equirect_rays(position, uv, facing=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0)):
    """A 360 x 180 degree panorama around `position`.  uv: (n, 2) in [0, 1] x [0, 1]: u runs over the longitude (0.5 looks along
    `facing`, growing to the right), v over the latitude from straight up (0) to straight down (1)."""
    uv = np.asarray(uv, dtype=F).reshape(-1, 2)
    f, r, u = _basis(facing, up)
    lon = (uv[:, 0] - F(0.5)) * F(2.0 * np.pi)
    lat = (F(0.5) - uv[:, 1]) * F(np.pi)
    cl = np.cos(lat, dtype=F)
    d = f[None] * (cl * np.cos(lon, dtype=F))[:, None] + r[None] * (cl * np.sin(lon, dtype=F))[:, None] + u[None] * np.sin(lat, dtype=F)[:, None]
    o = np.tile(_f3(position)[None], (uv.shape[0], 1))
    return np.ascontiguousarray(o), _normalize(d)
