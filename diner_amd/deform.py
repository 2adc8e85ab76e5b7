"""Nearest mesh vertex and the deformation the fork's NOVEL / NOVEL_PE renderers build on it (csrc/nearest_vertex.hip):

* :func:`nearest_vertex`     -- ``pytorch3d.ops.knn_points(points, vertices, K=1)``: index and squared distance of the nearest vertex
* :func:`deform_points`      -- ``NeRFRendererDGS.deform_points`` (reference ``src/models/novel/nerf_novel_renderer.py:40-50``) for one
  or two offset sets over the same vertices, in one pass
* :func:`deform_ray_points`  -- the same on the sample points of rays, formed in the kernel as ``composite`` forms them (:412, :441-442)

The arithmetic contract is in ``include/diner_hip.h``: ``d2 = ((px - vx)^2 + (py - vy)^2) + (pz - vz)^2`` in fp32 without contraction,
the vertex of smallest ``(d2, index)`` wins.  Two kernels return the same bits: brute force, and a search pruned by the bounding boxes of
clusters of 64 vertices in Morton order.  ``method="auto"`` chooses by ``V``; the choice affects time only.  Re-exported from
:mod:`diner_amd.glue`.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._lib import check

METHODS = ("auto", "brute", "clusters")
# V from which method="auto" takes the pruned kernel.  Measured on an MI355X (tools/bench_deform.py, profiles/deform_points.json,
# "threshold_sweep"): one search of a forward's 4096 x 1000 candidates plus one of its 4096 x 40 samples takes
# 0.30 ms brute force against 0.39 ms pruned at V = 256, 1.06 against 0.91 at 1024, 3.92 against 2.21 at 4096 and 25.2 against 4.9 at
# 26 317; the build (0.05 - 0.09 ms, once per mesh) does not move the crossing.  The samples alone, whose waves span whole rays, are
# faster brute force up to V of about 20 000 (0.92 against 1.18 ms at 16 384, 1.60 against 1.29 at 26 317): a caller that searches
# nothing but such points on a small mesh passes method="brute".
AUTO_CLUSTERS_MIN_V = 1024


def _f(t):
    return t.detach().to(torch.float32).contiguous()


def _st(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _check_method(method):
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS}, not {method!r}")


def _check_sets(points_shape, vertices, who, *offsets):
    if len(points_shape) != 3 or points_shape[2] != 3:
        raise ValueError(f"{who}: points must be [SB,N,3], not {tuple(points_shape)}")
    if vertices.dim() != 3 or vertices.shape[2] != 3 or vertices.shape[0] != points_shape[0] or vertices.shape[1] < 1:
        raise ValueError(f"{who}: target_vertices must be [SB = {points_shape[0]}, V >= 1, 3], not {tuple(vertices.shape)}")
    for o in offsets:
        if o is not None and tuple(o.shape) != tuple(vertices.shape):
            raise ValueError(f"{who}: offsets must have the vertices' shape {tuple(vertices.shape)}, not {tuple(o.shape)}")


def _no_grad_inputs(who, **tensors):
    for name, t in tensors.items():
        if isinstance(t, torch.Tensor) and t.requires_grad and torch.is_grad_enabled():
            raise NotImplementedError(f"{who}: {name} requires grad, but {name} is data here as in the reference (the nearest-vertex "
                                      f"gather has no backward to it); detach it")


# ---- the cluster structure, one entry ------------------------------------------------------------------------------------------------------
_cache = {"key": None, "workspace": None, "vertices": None}
cluster_builds = 0      # how many times the structure has been built (the tests watch it)


def _clusters(vertices, v32):
    """the workspace of diner_nearest_vertex_build for ``vertices`` (the caller's tensor; ``v32`` its fp32 contiguous form), kept in a
    single entry keyed on the caller's tensor: storage, ``_version`` and shape -- an in-place edit rebuilds it"""
    global cluster_builds
    key = (vertices.data_ptr(), vertices._version, tuple(vertices.shape), vertices.dtype, vertices.device, tuple(vertices.stride()))
    if _cache["key"] == key:
        return _cache["workspace"]
    L = _lib.lib()
    SB, V, dev = v32.shape[0], v32.shape[1], v32.device
    keys = torch.empty((SB, V), dtype=torch.int32, device=dev)
    check(L.diner_nearest_vertex_keys(v32.data_ptr(), SB, V, keys.data_ptr(), _st(dev)), "diner_nearest_vertex_keys")
    order = torch.sort(keys, dim=1, stable=True).indices.to(torch.int32).contiguous()
    n = int(L.diner_nearest_vertex_workspace_floats(SB, V))
    if n < 0:
        raise NotImplementedError(f"nearest_vertex: SB={SB}, V={V} beyond the envelope (V <= 2^24, SB <= 65535)")
    ws = torch.empty(max(n, 4), dtype=torch.float32, device=dev)
    check(L.diner_nearest_vertex_build(v32.data_ptr(), order.data_ptr(), SB, V, ws.data_ptr(), _st(dev)), "diner_nearest_vertex_build")
    cluster_builds += 1
    # the entry keeps the caller's tensor alive: its address cannot be handed to another tensor while the key stands
    _cache.update(key=key, workspace=ws, vertices=vertices)
    return ws


def clear_cache():
    _cache.update(key=None, workspace=None, vertices=None)


def _route(method, vertices, v32):
    """the workspace pointer of the route ``method`` selects (None: brute force) + what keeps it alive"""
    if method == "clusters" or (method == "auto" and v32.shape[1] >= AUTO_CLUSTERS_MIN_V):
        ws = _clusters(vertices, v32)
        return ws.data_ptr(), ws
    return None, None


def _gpu(t, who):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"diner_amd.glue.{who} runs on the GPU only")


# ---- the search ----------------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def nearest_vertex(points, vertices, method="auto"):
    """points [SB,N,3], vertices [SB,V,3] -> ``(idx [SB,N] int32, d2 [SB,N] fp32)``: for every point the vertex of its own scene with the
    smallest ``(d2, index)`` and that squared distance, by the contract of ``include/diner_hip.h``.  ``method``: ``"brute"``,
    ``"clusters"`` (the pruned search; the cluster structure of the vertices is built once and cached) or ``"auto"`` (by ``V``); the
    results are the same bits.  Carries no gradient."""
    _check_method(method)
    _gpu(points, "nearest_vertex")
    _check_sets(points.shape, vertices, "nearest_vertex")
    p, v = _f(points), _f(vertices).to(points.device)
    SB, N, V, dev = p.shape[0], p.shape[1], v.shape[1], p.device
    idx = torch.empty((SB, N), dtype=torch.int32, device=dev)
    d2 = torch.empty((SB, N), dtype=torch.float32, device=dev)
    if SB * N:
        ws, _keep = _route(method, vertices, v)
        check(_lib.lib().diner_nearest_vertex(p.data_ptr(), v.data_ptr(), ws, SB, N, V, idx.data_ptr(), d2.data_ptr(), _st(dev)),
              "diner_nearest_vertex")
    return idx, d2


# ---- the deformation -----------------------------------------------------------------------------------------------------------------------
def _deform(points, target_vertices, offsets, offsets2, method):
    p, v = _f(points), _f(target_vertices).to(points.device)
    o1 = _f(offsets).to(p.device)
    o2 = None if offsets2 is None else _f(offsets2).to(p.device)
    SB, N, V, dev = p.shape[0], p.shape[1], v.shape[1], p.device
    out = torch.empty_like(p)
    out2 = None if o2 is None else torch.empty_like(p)
    if SB * N:
        ws, _keep = _route(method, target_vertices, v)
        check(_lib.lib().diner_deform_points(p.data_ptr(), v.data_ptr(), ws, o1.data_ptr(), None if o2 is None else o2.data_ptr(), SB, N, V,
                                             out.data_ptr(), None if out2 is None else out2.data_ptr(), _st(dev)), "diner_deform_points")
    return out, out2


class _DeformFn(torch.autograd.Function):
    """d out / d points = identity for either output: the offsets are constants and the choice of vertex is piecewise constant"""

    @staticmethod
    def forward(ctx, points, target_vertices, offsets, offsets2, method):
        out, out2 = _deform(points, target_vertices, offsets, offsets2, method)
        ctx.dtype = points.dtype
        if out2 is None:
            return out
        return out, out2

    @staticmethod
    def backward(ctx, *grads):
        g = None
        for d in grads:
            if d is not None:
                g = d if g is None else g + d
        return (None if g is None else g.to(ctx.dtype)), None, None, None, None


def deform_points(points, target_vertices, offsets, offsets2=None, method="auto"):
    """``NeRFRendererDGS.deform_points`` of the NOVEL renderers (reference src/models/novel/nerf_novel_renderer.py:40-50): points [SB,B,3],
    target_vertices [SB,V,3], offsets [SB,V,3] -> ``points + offsets[nearest vertex]`` [SB,B,3] (fp32).  With ``offsets2`` (a second set
    over the same vertices, as ``composite`` uses, :441-442) it returns the pair of deformed point sets from ONE search.  Under autograd
    the gradient to ``points`` is the identity (the sum of both outputs' gradients); ``offsets`` / ``offsets2`` / ``target_vertices``
    that require grad raise ``NotImplementedError``: they are data in the reference."""
    _check_method(method)
    _gpu(points, "deform_points")
    _check_sets(points.shape, target_vertices, "deform_points", offsets, offsets2)
    _no_grad_inputs("deform_points", offsets=offsets, offsets2=offsets2, target_vertices=target_vertices)
    if points.requires_grad and torch.is_grad_enabled():
        return _DeformFn.apply(points, target_vertices, offsets, offsets2, method)
    with torch.no_grad():
        out, out2 = _deform(points, target_vertices, offsets, offsets2, method)
    return out if offsets2 is None else (out, out2)


def deform_ray_points(rays, z_samp, target_vertices, offsets, offsets2=None, return_points=False, method="auto"):
    """The sample points of rays [SB,B,8] at the depths z_samp [SB,B,K], formed in the kernel as the reference's ``composite`` forms
    them (``o + z d``: a multiplication, then an addition, :412) and deformed like :func:`deform_points` without ever being stored:
    -> ``deformed`` [SB,B*K,3], or ``(deformed, deformed2)`` with ``offsets2``; ``return_points=True`` appends the undeformed points
    [SB,B*K,3] (``NOVEL_PE``'s model takes them as a third argument).  Refuses any input that requires grad (``NotImplementedError``),
    as ``render_image(bounds=)`` does: differentiate :func:`deform_points` on points formed by torch instead."""
    _check_method(method)
    _gpu(rays, "deform_ray_points")
    if rays.dim() != 3 or rays.shape[2] != 8 or z_samp.dim() != 3 or tuple(z_samp.shape[:2]) != tuple(rays.shape[:2]):
        raise ValueError(f"deform_ray_points: rays must be [SB,B,8] and z_samp [SB,B,K], not {tuple(rays.shape)}, {tuple(z_samp.shape)}")
    SB, B, K = z_samp.shape
    _check_sets((SB, B * K, 3), target_vertices, "deform_ray_points", offsets, offsets2)
    if torch.is_grad_enabled():
        for name, t in dict(rays=rays, z_samp=z_samp, target_vertices=target_vertices, offsets=offsets, offsets2=offsets2).items():
            if isinstance(t, torch.Tensor) and t.requires_grad:
                raise NotImplementedError(f"deform_ray_points: {name} requires grad, but the ray form carries no gradient; form the "
                                          "points with torch and use deform_points (identity gradient to the points)")
    with torch.no_grad():
        dev = rays.device
        r, z, v = _f(rays), _f(z_samp).to(dev), _f(target_vertices).to(dev)
        o1 = _f(offsets).to(dev)
        o2 = None if offsets2 is None else _f(offsets2).to(dev)
        V = v.shape[1]
        out = torch.empty((SB, B * K, 3), dtype=torch.float32, device=dev)
        out2 = None if o2 is None else torch.empty_like(out)
        pts = torch.empty_like(out) if return_points else None
        if SB * B * K:
            ws, _keep = _route(method, target_vertices, v)
            check(_lib.lib().diner_deform_ray_points(r.data_ptr(), z.data_ptr(), v.data_ptr(), ws, o1.data_ptr(),
                                                     None if o2 is None else o2.data_ptr(), SB, B, K, V, out.data_ptr(),
                                                     None if out2 is None else out2.data_ptr(), None if pts is None else pts.data_ptr(),
                                                     _st(dev)), "diner_deform_ray_points")
    res = (out,) if out2 is None else (out, out2)
    if return_points:
        res = res + (pts,)
    return res[0] if len(res) == 1 else res
