"""Differentiable point model of the fork's NOVEL configuration (reference ``src/models/novel/novel_pixelnerf.py:143-242``) on the
shape-general training path: what ``diner_amd.novel.NeRFRendererDGS.composite()`` runs in place of the chunked PyTorch model when the
renderer was constructed with ``hip_point_model`` and ``train_hip_point_model`` and a parameter of the model requires grad.

The NOVEL model differs from the plain one (``diner_amd/training_gen.py``) in the first and the last stage of the staged schedule only:
the points are given, not formed from rays, the viewdirs are per point, and the learned ``gen_latent``, looked up at one general camera
per scene, is added to the encoder's lookup before ``lin_z`` (:196) -- ``diner_train_point_inputs_novel`` (csrc/train_novel.hip) -- and
autograd sends d(final_latent) to both maps: ``diner_train_bilinear_scatter`` into ``encoder.latent``'s gradient, unchanged, and
``diner_train_novel_gen_scatter`` (the sum over the views, then the same scatter) into ``gen_latent``'s.  Everything between is
``training_gen.schedule_forward`` / ``schedule_backward``: the same GEMMs, in exact fp32 or (``f16=True``) in f16x3 through the same
``WeightSplitCache``.  Gradients: every fusion-MLP parameter, ``encoder.latent`` and ``gen_latent``; the points and viewdirs are data.
PyTorch supplies buffers and the autograd hook -- no arithmetic of the path.
"""
from __future__ import annotations

import ctypes as C

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import check
from .training import _p, _st, check_versions, latent_grad_out, prepare_latent, remember_versions
from .training_gen import Act, _Layout, mlp_params, schedule_backward, schedule_forward


def _timed(renderer, name, launch):
    """profiling hook (tools/bench_novel_train.py): when ``renderer.novel_train_events`` is a list, the launch of one of the two new
    kernels is bracketed by device events and (name, ev0, ev1) appended; otherwise the launch alone"""
    events = getattr(renderer, "novel_train_events", None)
    if events is None:
        return launch()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    launch()
    e1.record()
    events.append((name, e0, e1))


class _RenderNovelFn(torch.autograd.Function):
    """(in_points, gen_points, viewdirs, encoder.latent, gen_latent, *mlp_params) -> rgbsigma [SB,P,4].  ``scene``: the DinerScene with
    C, h, w of the latent; ``ix``: the 4-tap lookup (None: bilinear / border); ``gen``: the DinerNovelGen of ``_novel_gen`` (its packed
    gen_latent); ``keep``: the tensors both point into."""

    @staticmethod
    def forward(ctx, renderer, scene, ix, gen, keep, shape, f16, xi, xg, vd, latent, gen_latent, *params):
        L = _lib.lib()
        dev = xi.device
        st = _st(dev)
        SB, P, _ = xi.shape
        NV = scene.NV
        R = NV * P
        lay, act = _Layout(shape), Act(shape.beta)
        H, F = shape.d_hidden, shape.num_freqs
        ld_in = 8 * (F + 1)
        f = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
        lat, lat_nhwc, ctx.lat_packed = prepare_latent(L, latent, dev, st)
        prm = [p.detach().to(torch.float32).contiguous() for p in params]
        remember_versions(ctx, tuple(params) + (gen_latent,), latent, ())
        w_in = torch.zeros((H, ld_in), dtype=torch.float32, device=dev)   # lin_in's weight, zero-padded to the input's ld_in columns
        w_in[:, :shape.d_in] = prm[0]

        def sw(i):   # f16x3: the pre-split planes of weight i (mlp_params order); None = the fp32 GEMM
            return renderer._weight_split_cache.get(params[i], w_in if i == 0 else prm[i], False) if f16 else None

        rgbsigma = f(SB, P, 4)
        ixp = C.byref(ix) if ix is not None else None
        saved = []
        for sb in range(SB):
            inp = f(R, ld_in)
            zl, taps, gtaps = (f(R, scene.C), f(R, 8), f(P, 8)) if lay.nlz else (None, None, None)   # combine_layer 0: no latent is read
            _timed(renderer, "point_inputs_novel", lambda: check(L.diner_train_point_inputs_novel(
                C.byref(scene), ixp, _p(lat_nhwc), C.byref(gen), _p(xi), _p(xg), _p(vd), P, sb, _p(inp), ld_in, _p(zl), _p(taps), _p(gtaps), st),
                "diner_train_point_inputs_novel"))
            blocks, x, out = schedule_forward(L, inp, zl, prm, w_in, lay, act, sw, NV, P, st)
            check(L.diner_train_head(_p(out), None, None, P * 4, _p(rgbsigma[sb]), 0, st), "diner_train_head")  # novel_pixelnerf.py:236-240
            saved.append((inp, zl, taps, gtaps, blocks, x, out))
        ctx.renderer, ctx.scene, ctx.rgbsigma = renderer, scene, rgbsigma
        ctx.saved_acts, ctx.prm, ctx.w_in, ctx.lat_shape = saved, prm, w_in, tuple(latent.shape)
        ctx.gen_shape = (int(gen.C), int(gen.h), int(gen.w))
        ctx.keep = (lat, lat_nhwc, keep)
        ctx.shape, ctx.f16, ctx.params, ctx.P = shape, bool(f16), params, P
        return rgbsigma

    @staticmethod
    @once_differentiable                       # the hand-written backward has no graph of its own: a double backward raises
    def backward(ctx, d_rgbsigma):
        L = _lib.lib()
        check_versions(ctx, "diner_amd.training_novel")
        scene, rgbsigma, prm, shape, P = ctx.scene, ctx.rgbsigma, ctx.prm, ctx.shape, ctx.P
        lay, act = _Layout(shape), Act(shape.beta)
        dev = rgbsigma.device
        st = _st(dev)
        SB, NV = rgbsigma.shape[0], scene.NV
        f = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
        d_rgbsigma = d_rgbsigma.detach().to(torch.float32).contiguous()
        want_lat, want_gen = ctx.needs_input_grad[10] and lay.nlz > 0, ctx.needs_input_grad[11] and lay.nlz > 0
        g = [torch.zeros_like(p) for p in prm]          # parameter gradients (fp32, accumulated atomically)
        g_in = torch.zeros_like(ctx.w_in)
        SBl, NVl, Cl, hl, wl = ctx.lat_shape
        Cg, hg, wg = ctx.gen_shape
        d_lat_nhwc = torch.zeros((SBl, NVl, hl, wl, Cl), dtype=torch.float32, device=dev) if ctx.needs_input_grad[10] else None
        d_gen_nhwc = torch.zeros((hg, wg, Cg), dtype=torch.float32, device=dev) if ctx.needs_input_grad[11] else None
        f16 = ctx.f16

        def swt(i):
            return ctx.renderer._weight_split_cache.get(ctx.params[i], ctx.w_in if i == 0 else prm[i], True) if f16 else None

        for sb in range(SB):
            inp, zl, taps, gtaps, blocks, x_last, out = ctx.saved_acts[sb]
            d_out = f(x_last.shape[0], 4)
            check(L.diner_train_head(_p(out), _p(rgbsigma[sb]), _p(d_rgbsigma[sb]), P * 4, _p(d_out), 1, st), "diner_train_head(bwd)")
            _d_x, _a_x, d_zl = schedule_backward(L, inp, zl, blocks, x_last, d_out, prm, g, g_in, lay, act, swt, f16, NV, P, scene.C, st)
            if want_lat:     # d(final_latent) goes to both maps (novel_pixelnerf.py:196)
                check(L.diner_train_bilinear_scatter(_p(d_zl), _p(taps), P, scene.C, scene.h, scene.w, NV, sb, _p(d_lat_nhwc), st),
                      "diner_train_bilinear_scatter")
            if want_gen:     # one map for every scene: all of them accumulate into it
                _timed(ctx.renderer, "novel_gen_scatter", lambda: check(L.diner_train_novel_gen_scatter(
                    _p(d_zl), _p(gtaps), P, Cg, hg, wg, NV, _p(d_gen_nhwc), st), "diner_train_novel_gen_scatter"))
        d_lat = latent_grad_out(L, d_lat_nhwc, ctx.lat_shape, ctx.lat_packed, st) if d_lat_nhwc is not None else None
        d_gen = None
        if d_gen_nhwc is not None:
            d_gen = f(Cg, hg, wg)
            check(L.diner_train_nhwc_to_nchw(_p(d_gen_nhwc), 1, Cg, hg, wg, _p(d_gen), st), "diner_train_nhwc_to_nchw")
        g[0] = g_in[:, :shape.d_in].contiguous()
        gp = tuple(gi if need else None for gi, need in zip(g, ctx.needs_input_grad[12:]))
        return (None,) * 10 + (d_lat, d_gen) + gp


def render_points_with_grad(renderer, model, in_points, gen_points, viewdirs, shape, f16=False):
    """rgbsigma [SB,P,4] of the NOVEL PixelNeRF at ``in_points`` / ``gen_points`` / ``viewdirs`` [SB,P,3], with gradients to every
    fusion-MLP parameter, ``encoder.latent`` and ``model.gen_latent``.  Any shape of the shape-general envelope, the standard one
    included; every 4-tap lookup mode.  ``f16``: the GEMMs in f16x3."""
    xi, xg, vd = [t.detach().to(torch.float32).contiguous() for t in (in_points, gen_points, viewdirs)]
    if not xi.is_cuda:
        raise RuntimeError("diner_amd.training_novel runs on the GPU only (points are on %s)" % xi.device)
    assert xi.dim() == 3 and xi.shape[-1] == 3 and xg.shape == xi.shape and vd.shape == xi.shape
    dev = xi.device
    with torch.no_grad():
        sc, keep = renderer._scene(model, need_latent=False)
        gen, gkeep = renderer._novel_gen(model, dev)     # gen_latent's NHWC pack, re-made after every in-place update, and the cameras
    if shape.combine_layer >= shape.n_blocks and sc.NV != 1:
        raise NotImplementedError(f"combine_layer={shape.combine_layer} >= n_blocks={shape.n_blocks} (no mean over views) with NV={sc.NV}: "
                                  "the reference supports it for one view only (novel_pixelnerf.py:234)")
    lat = model.encoder.latent
    assert xi.shape[0] == sc.SB and lat.shape[:2] == (sc.SB, sc.NV) and lat.shape[2] == shape.d_latent
    sc.C, sc.h, sc.w = int(lat.shape[2]), int(lat.shape[3]), int(lat.shape[4])
    if int(gen.C) != sc.C:
        raise ValueError(f"gen_latent has {int(gen.C)} channels, the encoder's latent {sc.C}")
    ix = renderer._latent_index(model)
    return _RenderNovelFn.apply(renderer, sc, ix, gen, (keep, gkeep), shape, bool(f16), xi, xg, vd, lat, model.gen_latent,
                                *mlp_params(model.mlp_fine))
