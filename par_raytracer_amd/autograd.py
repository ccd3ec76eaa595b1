"""Closest-hit queries and closest-point queries as differentiable torch operations.

`trace_rays_differentiable` ties Renderer.update_geometry, Renderer.trace_rays and Renderer.trace_rays_backward into one
torch.autograd.Function, so that a loss over t, bw, position and normal of a batch of rays can be back-propagated to the vertex
positions, the ray origins and the ray directions - the optimisation loop over vertex positions that prt_update_geometry and
prt_trace_rays were added for (include/prt.h).  The gradient is that of the hit arithmetic on the triangle each ray reported; changes
of visibility at silhouettes are not modelled.

`closest_points_differentiable` does the same for Renderer.closest_points and Renderer.closest_points_backward: a loss over
dist2, point and bw of a batch of points - a point-to-surface or chamfer loss when a mesh is fitted to scanned points - is
back-propagated to the vertex positions and the points.  The gradient is that of the region walk on the triangle and in the region
each point reported; a change of region or of the winning triangle is not modelled.

`signed_distance_differentiable` puts the sign of Renderer.signed_distance on the distance of `closest_points_differentiable`: a
signed distance whose gradient is that of the unsigned distance times the sign.  A gradient of the sign itself is not modelled.

`sample_surface_differentiable` ties Renderer.update_geometry, Renderer.sample_surface and Renderer.sample_surface_backward together:
points drawn uniformly by area on the mesh - the mesh -> scan side of a chamfer loss - whose positions and normals are
differentiable with respect to the vertex positions.  The choice of the triangle is not differentiated.

torch is imported when a function is first called: importing the package stays torch-free.
"""
from __future__ import annotations

_FUNCTION = None
_POINT_FUNCTION = None
_SAMPLE_FUNCTION = None


def _function():
    global _FUNCTION
    if _FUNCTION is not None:
        return _FUNCTION
    import torch

    class TraceRays(torch.autograd.Function):
        @staticmethod
        def forward(ctx, renderer, positions, origins, directions, ray_bias, update_geometry):
            p, o, d = (x.detach().contiguous() for x in (positions, origins, directions))
            if update_geometry:
                renderer.update_geometry(p)
            res = renderer.trace_rays(o, d, ray_bias=ray_bias)
            ctx.renderer, ctx.ray_bias = renderer, ray_bias
            ctx.set_materialize_grads(False)              # an output the loss does not use arrives as None = zero, and is not read
            ctx.save_for_backward(p, o, d, res["group"], res["vertex0"])
            ctx.mark_non_differentiable(res["group"], res["vertex0"])
            return res["t"], res["bw"], res["position"], res["normal"], res["group"], res["vertex0"]

        @staticmethod
        def backward(ctx, g_t, g_bw, g_position, g_normal, _g_group, _g_vertex0):
            p, o, d, group, vertex0 = ctx.saved_tensors
            names = ("positions", "origins", "directions")
            want = tuple(n for n, needed in zip(names, ctx.needs_input_grad[1:4]) if needed)
            if not want:
                return (None,) * 6
            grads = [None if g is None else g.contiguous() for g in (g_t, g_bw, g_position, g_normal)]
            res = ctx.renderer.trace_rays_backward(o, d, group, vertex0, p, ray_bias=ctx.ray_bias, grad_t=grads[0], grad_bw=grads[1],
                                                   grad_position=grads[2], grad_normal=grads[3], want=want)
            return (None,) + tuple(res.get(n) for n in names) + (None, None)

    _FUNCTION = TraceRays
    return _FUNCTION


def trace_rays_differentiable(renderer, positions, origins, directions, *, ray_bias: float = 0.0, update_geometry: bool = True):
    """Closest hits of the rays (origins, directions) against the renderer's scene with its vertices at `positions`.

    positions (P, 3), origins and directions (n, 3): float32 torch tensors on the renderer's device.  With update_geometry (the
    default) the scene's vertices are first moved to `positions` (Renderer.update_geometry: P must be the uploaded scene's
    count); without it `positions` must be what the scene holds already.  Returns (t, bw, position, normal, group, vertex0) as
    Renderer.trace_rays does; the first four are differentiable with respect to whichever of positions, origins and directions
    require a gradient, group and vertex0 are not."""
    return _function().apply(renderer, positions, origins, directions, float(ray_bias), bool(update_geometry))


def _point_function():
    global _POINT_FUNCTION
    if _POINT_FUNCTION is not None:
        return _POINT_FUNCTION
    import torch

    class ClosestPoints(torch.autograd.Function):
        @staticmethod
        def forward(ctx, renderer, positions, points, max_dist, update_geometry):
            p, q = (x.detach().contiguous() for x in (positions, points))
            if update_geometry:
                renderer.update_geometry(p)
            res = renderer.closest_points(q, max_dist=None if max_dist is None else max_dist.detach().contiguous())
            ctx.renderer = renderer
            ctx.set_materialize_grads(False)              # an output the loss does not use arrives as None = zero, and is not read
            ctx.save_for_backward(p, q, res["group"], res["vertex0"])
            ctx.mark_non_differentiable(res["group"], res["vertex0"])
            return res["dist2"], res["point"], res["bw"], res["group"], res["vertex0"]

        @staticmethod
        def backward(ctx, g_dist2, g_point, g_bw, _g_group, _g_vertex0):
            p, q, group, vertex0 = ctx.saved_tensors
            names = ("positions", "points")
            want = tuple(n for n, needed in zip(names, ctx.needs_input_grad[1:3]) if needed)
            if not want:
                return (None,) * 5
            grads = [None if g is None else g.contiguous() for g in (g_dist2, g_point, g_bw)]
            res = ctx.renderer.closest_points_backward(q, group, vertex0, p, grad_dist2=grads[0], grad_point=grads[1], grad_bw=grads[2],
                                                       want=want)
            return (None,) + tuple(res.get(n) for n in names) + (None, None)

    _POINT_FUNCTION = ClosestPoints
    return _POINT_FUNCTION


def closest_points_differentiable(renderer, positions, points, *, max_dist=None, update_geometry: bool = True):
    """The nearest surface point of `points` on the renderer's scene with its vertices at `positions`.

    positions (P, 3) and points (n, 3): float32 torch tensors on the renderer's device; max_dist: None or float32 (n,) distances,
    as Renderer.closest_points takes them (not differentiated).  With update_geometry (the default) the scene's vertices are first
    moved to `positions` (Renderer.update_geometry: P must be the uploaded scene's count); without it `positions` must be what
    the scene holds already.  Returns (dist2, point, bw, group, vertex0) as Renderer.closest_points does; the first three are
    differentiable with respect to whichever of positions and points require a gradient, group and vertex0 are not.  A miss (a
    point with a non-finite component, or nothing within max_dist) has dist2 = FLT_MAX, point and bw zeros, and zero gradient."""
    return _point_function().apply(renderer, positions, points, max_dist, bool(update_geometry))


def signed_distance_differentiable(renderer, positions, points, *, max_dist=None, update_geometry: bool = True):
    """The signed distance of `points` to the renderer's scene with its vertices at `positions` (Renderer.signed_distance).

    positions, points, max_dist and update_geometry: as closest_points_differentiable takes them.  The signed query runs once
    without a graph - after moving the geometry when update_geometry is set - and gives the sign and the value; dist2 comes from
    closest_points_differentiable on the geometry already moved, and the result is sign x sqrt(dist2): the bits of
    Renderer.signed_distance's signed_distance (FLT_MAX on a miss), differentiable with respect to whichever of positions and
    points require a gradient.  The gradient with respect to the positions is closest_points_differentiable's.  The gradient
    with respect to a point is that of |p - q|^2 with the returned nearest point q held fixed, sign x (p - q) / dist: the
    distance to a nearest point does not change to first order when the nearest point moves along its feature, so the
    derivative of q through v and w - which the region's formula carries, and which in float32 is the tangential rounding noise of
    p - q rather than zero - is left out.  Where dist2 == 0, and on a miss, the gradient is zero (not inf or NaN)."""
    import torch
    with torch.no_grad():
        if update_geometry:
            renderer.update_geometry(positions.detach().contiguous())
        res = renderer.signed_distance(points.detach().contiguous(), max_dist=None if max_dist is None else max_dist.detach().contiguous(),
                                       fields=("signed_distance", "feature"))
    signed = res["signed_distance"].detach()
    dist2, point, _bw, group, _vertex0 = closest_points_differentiable(renderer, positions, points.detach(), max_dist=max_dist,
                                                                       update_geometry=False)
    live = (group >= 0) & (dist2 > 0)
    e = torch.where(live[:, None], points - point.detach(), torch.zeros_like(points))
    own = (e * e).sum(-1)
    dist2 = dist2 + (own - own.detach())                 # dist2's bits and gradient to the positions, 2 (p - q) to the points
    dist = torch.where(live, torch.where(live, dist2, torch.ones_like(dist2)).sqrt(), torch.zeros_like(dist2))
    g = torch.where(signed < 0, -dist, dist)
    return signed + (g - g.detach())                     # the library's bits, the gradient of sign x sqrt(dist2)


def _sample_function():
    global _SAMPLE_FUNCTION
    if _SAMPLE_FUNCTION is not None:
        return _SAMPLE_FUNCTION
    import torch

    class SampleSurface(torch.autograd.Function):
        @staticmethod
        def forward(ctx, renderer, positions, count, seed, first, update_geometry):
            p = positions.detach().contiguous()
            if update_geometry:
                renderer.update_geometry(p)
            res = renderer.sample_surface(count, seed=seed, first=first, out="torch")
            ctx.renderer = renderer
            ctx.set_materialize_grads(False)              # an output the loss does not use arrives as None = zero, and is not read
            ctx.save_for_backward(p, res["bw"], res["group"], res["vertex0"])
            ctx.mark_non_differentiable(res["bw"], res["group"], res["vertex0"])
            return res["point"], res["normal"], res["bw"], res["group"], res["vertex0"]

        @staticmethod
        def backward(ctx, g_point, g_normal, _g_bw, _g_group, _g_vertex0):
            p, bw, group, vertex0 = ctx.saved_tensors
            if not ctx.needs_input_grad[1]:
                return (None,) * 6
            grads = [None if g is None else g.contiguous() for g in (g_point, g_normal)]
            res = ctx.renderer.sample_surface_backward(group, vertex0, bw, p, grad_point=grads[0], grad_normal=grads[1])
            return (None, res["positions"], None, None, None, None)

    _SAMPLE_FUNCTION = SampleSurface
    return _SAMPLE_FUNCTION


def sample_surface_differentiable(renderer, positions, count, *, seed, first: int = 0, update_geometry: bool = True):
    """`count` points drawn uniformly by area on the renderer's scene with its vertices at `positions` (Renderer.sample_surface).

    positions (P, 3): a float32 torch tensor on the renderer's device.  With update_geometry (the default) the scene's vertices
    are first moved to `positions` (Renderer.update_geometry: P must be the uploaded scene's count); without it `positions` must
    be what the scene holds already.  Returns (point, normal, bw, group, vertex0) as Renderer.sample_surface(out="torch") does;
    point and normal are differentiable with respect to positions - each sample moves with its triangle, at fixed barycentrics -,
    bw, group and vertex0 are not.  The choice of the triangle is not differentiated: there is no gradient through the area
    weights.  A miss (a scene without area) has zeros and zero gradient."""
    return _sample_function().apply(renderer, positions, int(count), int(seed), int(first), bool(update_geometry))
