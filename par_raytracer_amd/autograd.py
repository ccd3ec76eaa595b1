"""Closest-hit queries as a differentiable torch operation.

`trace_rays_differentiable` ties Renderer.update_geometry, Renderer.trace_rays and Renderer.trace_rays_backward into one
torch.autograd.Function, so that a loss over t, bw, position and normal of a batch of rays can be back-propagated to the vertex
positions, the ray origins and the ray directions - the optimisation loop over vertex positions that prt_update_geometry and
prt_trace_rays were added for (include/prt.h).  The gradient is that of the hit arithmetic on the triangle each ray reported; changes
of visibility at silhouettes are not modelled.

torch is imported when the function is first called: importing the package stays torch-free.
"""
from __future__ import annotations

_FUNCTION = None


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
