"""Differentiable render path for any fusion-MLP shape of the shape-general envelope (include/diner_hip.h): the training path of
``diner_amd/training.py`` for ResnetFC / PositionalEncoding shapes other than the standard one, in exact fp32 or (``renderer.train_f16x3_any_shape``) in f16x3.

The reference trains any model its constructors accept (``ResnetFC.from_conf`` reads d_hidden, n_blocks, combine_layer and beta from
``mlp_fine_conf``, num_freqs comes from ``poscode_conf``, d_latent from the encoder's ``num_layers``).  This module runs the layer
schedule of ResnetFC.forward (reference src/models/resnetfc.py:139-158) for any ``n_blocks`` / ``combine_layer`` on the HIP building
blocks of ``diner_amd/csrc/train_gen.hip`` (the fp32 MFMA GEMM with activation codes, the point inputs of any num_freqs and latent width
and their transpose) plus the shape-agnostic ones of ``train.hip`` (view mean, head, column sums, latent scatter, compositing
backward).  Gradients: every fusion-MLP parameter, ``encoder.latent``, and the rays, source cameras and depth maps when they require
grad.  PyTorch supplies buffers and the autograd hook -- no arithmetic of the path.

f16x3 mode (``f16=True``; csrc/train_gen_f16.hip): every GEMM of the graph runs in the split-fp16 arithmetic of the standard path
(``diner_amd/training.py``): activations scaled by 2^-4 and weights by 2^4, every gradient operand by its measured max|.|; forward and dX
read the weight pre-split (``WeightSplitCache``, made once per parameter version), dW streams and splits both operands.  Everything else
(point inputs, view mean, head, scatter, compositing backward, camera reductions) is the same fp32 kernels.
"""
from __future__ import annotations

import ctypes as C
import weakref

import torch

from . import _lib
from ._lib import check
from .training import (CAMERA_INPUTS, EXP_ACT, EXP_W, _p, _st, camera_grad_buffers, camera_grads_out, camera_inputs, camera_leaves,
                       check_versions, composite_backward, latent_grad_out, prepare_latent, remember_versions)

K_CHUNK = 4096  # rows per split of the weight-gradient GEMMs (multiple of 32)


class Act:
    """activation code + beta of a shape (DINER_ACT_*)"""
    __slots__ = ("code", "beta")

    def __init__(self, beta):
        self.code = _lib.ACT_SOFTPLUS if beta > 0 else _lib.ACT_RELU
        self.beta = float(beta) if beta > 0 else 1.0


def _gemm(A, B, bias, S, Cm, M, N, K, sam, sak, sbk, sbn, ldc, lds, act_a=0, act_b=0, act_s=0, beta=1.0, accumulate=0, atomic=0, k_chunk=0):
    check(_lib.lib().diner_train_gemm_act(_p(A), _p(B), _p(bias), _p(S), _p(Cm), M, N, K, sam, sak, sbk, sbn, ldc, lds, act_a, act_b, act_s,
                                          beta, accumulate, atomic, k_chunk, _st(Cm.device)), "diner_train_gemm_act")


class SplitWeight:
    """fp16 hi / lo planes of a weight operand (``diner_train_split_weight``) for ``diner_train_gemm_act_f16x3_w``"""
    __slots__ = ("hi", "lo")

    def __init__(self, W, transpose):
        n, k = (W.shape[1], W.shape[0]) if transpose else (W.shape[0], W.shape[1])
        halfs = int(_lib.lib().diner_train_split_weight_halfs(n, k))
        self.hi = torch.empty(halfs, dtype=torch.float16, device=W.device)
        self.lo = torch.empty(halfs, dtype=torch.float16, device=W.device)
        check(_lib.lib().diner_train_split_weight(_p(W), n, k, W.stride(0), int(transpose), EXP_W, _p(self.hi), _p(self.lo), _st(W.device)),
              "diner_train_split_weight")


class WeightSplitCache:
    """``SplitWeight``s of the MLP weights, kept per (parameter object, orientation) and valid for one ``_version`` like
    ``training.PanelCache``'s panels: re-split only after an in-place update of the parameter, and two models that share a renderer keep
    their own entries.  Weak references: no parameter is kept alive; entries of dead parameters go when a new one is made."""

    def __init__(self):
        self._e = {}

    def get(self, src, W, transpose):
        """planes of ``W`` (``src``'s fp32 contiguous copy, or lin_in's zero-padded one), B[k][n] = W[n][k] or (transpose) W[k][n]"""
        key = (id(src), bool(transpose))
        ent = self._e.get(key)
        if ent is not None and ent[0]() is src and ent[1] == src._version and ent[2] == tuple(W.shape):
            return ent[3]
        for k in [k for k, e in self._e.items() if e[0]() is None]:
            del self._e[k]
        sw = SplitWeight(W, transpose)
        self._e[key] = (weakref.ref(src), src._version, tuple(W.shape), sw)
        return sw


def _gemm_w(A, sw, bias, S, Cm, M, N, K, act_a=0, act_s=0, beta=1.0, accumulate=0, amax=None, exp_a=0):
    check(_lib.lib().diner_train_gemm_act_f16x3_w(_p(A), A.stride(0), _p(sw.hi), _p(sw.lo), _p(bias), _p(S), 0 if S is None else S.stride(0),
                                                  _p(Cm), Cm.stride(0), M, N, K, act_a, act_s, beta, accumulate, _p(amax), exp_a, EXP_W,
                                                  _st(Cm.device)), "diner_train_gemm_act_f16x3_w")


def linear_fwd(X, W, b, out, act=None, accumulate=False, sw=None):
    """out[M,N] (+)= act?(X[M,K]) W[N,K]^T + b   (sw: W's SplitWeight -> the f16x3 GEMM)"""
    M, K = X.shape
    N = W.shape[0]
    a = act.code if act is not None else _lib.ACT_NONE
    if sw is not None:
        return _gemm_w(X, sw, b, None, out, M, N, K, act_a=a, beta=act.beta if act else 1.0, accumulate=int(accumulate), exp_a=EXP_ACT)
    _gemm(X, W, b, None, out, M, N, K, X.stride(0), 1, 1, W.stride(0), out.stride(0), 0, act_a=a, beta=act.beta if act else 1.0,
          accumulate=int(accumulate))


def linear_bwd_x(dY, W, S, out, act=None, accumulate=False, sw=None, amax=None):
    """out[M,K] (+)= (dY[M,N] W[N,K]) * act'(S)   (S None: no derivative; sw: W's transposed SplitWeight, amax: max|dY| -> f16x3)"""
    M, N = dY.shape
    K = W.shape[1]
    a_s = act.code if (act is not None and S is not None) else _lib.ACT_NONE
    if sw is not None:
        return _gemm_w(dY, sw, None, S, out, M, K, N, act_s=a_s, beta=act.beta if act else 1.0, accumulate=int(accumulate), amax=amax)
    _gemm(dY, W, None, S, out, M, K, N, dY.stride(0), 1, W.stride(0), 1, out.stride(0), 0 if S is None else S.stride(0),
          act_s=a_s, beta=act.beta if act else 1.0, accumulate=int(accumulate))


def linear_bwd_w(dY, X, dW, db, act=None, amax=None):
    """dW[N,K] += dY[M,N]^T act?(X[M,K]);  db[N] += sum_m dY (its own column sums).  amax (the device word with max|dY|, from
    ``grad_reduce``, which has summed the columns into db already): the f16x3 GEMM"""
    M, N = dY.shape
    K = X.shape[1]
    if amax is not None:
        check(_lib.lib().diner_train_gemm_act_f16x3(_p(dY), _p(X), None, None, _p(dW), N, K, M, 1, dY.stride(0), X.stride(0), 1, dW.stride(0), 0,
                                                    _lib.ACT_NONE, act.code if act else _lib.ACT_NONE, _lib.ACT_NONE,
                                                    act.beta if act else 1.0, 0, 1, K_CHUNK, _p(amax), None, 0, EXP_ACT, _st(dW.device)),
              "diner_train_gemm_act_f16x3")
    else:
        _gemm(dY, X, None, None, dW, N, K, M, 1, dY.stride(0), X.stride(0), 1, dW.stride(0), 0, act_b=act.code if act else _lib.ACT_NONE,
              beta=act.beta if act else 1.0, atomic=1, k_chunk=K_CHUNK)
        check(_lib.lib().diner_train_colsum(_p(dY), M, N, dY.stride(0), _p(db), _st(dY.device)), "diner_train_colsum")


def grad_reduce(dY, db, f16):
    """f16x3 mode: db += column sums of dY (a bias gradient) and the device word with max|dY| that scales dY as a GEMM operand -- one
    pass (``diner_train_colsum_amax``) where the width allows it ((N / 4) | 256), else ``diner_train_amax`` + ``diner_train_colsum``.
    fp32 mode: nothing, None (``linear_bwd_w`` sums the columns after its GEMM, as before)."""
    if not f16:
        return None
    L = _lib.lib()
    M, N = dY.shape
    word = torch.empty(1, dtype=torch.int32, device=dY.device)
    st = _st(dY.device)
    if 256 % (N // 4) == 0:
        check(L.diner_train_colsum_amax(_p(dY), M, N, dY.stride(0), _p(db), _p(word), st), "diner_train_colsum_amax")
    else:
        assert dY.is_contiguous()
        check(L.diner_train_amax(_p(dY), dY.numel(), _p(word), st), "diner_train_amax")
        check(L.diner_train_colsum(_p(dY), M, N, dY.stride(0), _p(db), st), "diner_train_colsum")
    return word


def mlp_params(mlp):
    """The fusion MLP's parameters in the order of the autograd function's inputs: lin_in, lin_z[0 .. min(combine_layer, n_blocks) - 1],
    every block's fc_0 / fc_1, lin_out (weight, bias each)."""
    nlz = min(int(mlp.combine_layer), int(mlp.n_blocks))
    ps = [mlp.lin_in.weight, mlp.lin_in.bias]
    for b in range(nlz):
        ps += [mlp.lin_z[b].weight, mlp.lin_z[b].bias]
    for b in range(int(mlp.n_blocks)):
        ps += [mlp.blocks[b].fc_0.weight, mlp.blocks[b].fc_0.bias, mlp.blocks[b].fc_1.weight, mlp.blocks[b].fc_1.bias]
    ps += [mlp.lin_out.weight, mlp.lin_out.bias]
    return ps


class _Layout:
    """indices of a shape's parameters in ``mlp_params`` order"""

    def __init__(self, shape):
        self.nb, self.cl = shape.n_blocks, shape.combine_layer
        self.nlz = min(self.cl, self.nb)

    def lz(self, b):
        return 2 + 2 * b

    def blk(self, b):
        return 2 + 2 * self.nlz + 4 * b

    @property
    def out(self):
        return 2 + 2 * self.nlz + 4 * self.nb


# ---- the layer schedule of ResnetFC.forward and its transpose, for one scene's rows: what both autograd functions (_RenderGenFn here,
# training_novel._RenderNovelFn) run between their own point-input and latent-scatter stages

def schedule_forward(L, inp, zl, prm, w_in, lay, act, sw, NV, P, st):
    """in [R, ld_in], zlat [R, C] (None: no lin_z) -> blocks [(x, net) per block], the last block's output x, lin_out's output [P or R, 4].
    ``prm``: the fp32 parameters in ``mlp_params`` order, ``w_in``: lin_in's zero-padded weight, ``sw(i)``: weight i's SplitWeight (f16x3)
    or None."""
    dev = inp.device
    f = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
    H = w_in.shape[0]
    x = f(NV * P, H)
    linear_fwd(inp, w_in, prm[1], x, sw=sw(0))                                                # resnetfc.py:139
    blocks = []
    for b in range(lay.nb):
        if b == lay.cl:                                                                # :146-149 (mean over views)
            xbar = f(P, H)
            check(L.diner_train_view_mean(_p(x), P * H, NV, _p(xbar), 0, st), "diner_train_view_mean")
            x = xbar
        if b < lay.cl:                                                                 # :151-153, x += lin_z[b](z) in place
            linear_fwd(zl, prm[lay.lz(b)], prm[lay.lz(b) + 1], x, accumulate=True, sw=sw(lay.lz(b)))
        i = lay.blk(b)
        net = torch.empty_like(x)
        linear_fwd(x, prm[i], prm[i + 1], net, act=act, sw=sw(i))                             # :62
        y = x.clone()
        linear_fwd(net, prm[i + 2], prm[i + 3], y, act=act, accumulate=True, sw=sw(i + 2))         # :63, :69
        blocks.append((x, net))
        x = y
    out = f(x.shape[0], 4)
    linear_fwd(x, prm[lay.out], prm[lay.out + 1], out, act=act, sw=sw(lay.out))                    # :158
    return blocks, x, out


def schedule_backward(L, inp, zl, blocks, x_last, d_out, prm, g, g_in, lay, act, swt, f16, NV, P, Cl, st, zero_d_zl=False):
    """The transpose of ``schedule_forward`` from d_out (the head's backward) down to lin_in's weight gradient: adds every parameter's
    gradient into ``g`` (``g_in``: lin_in's padded weight) and returns d_x [R, H] (lin_in's output gradient), its amax word (f16x3, else
    None) and d_zlat [R, Cl] (None without lin_z, zeros under ``zero_d_zl``).  ``swt(i)``: weight i's transposed SplitWeight or None."""
    dev = inp.device
    f = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
    H, R = x_last.shape[1], NV * P
    a_out = grad_reduce(d_out, g[lay.out + 1], f16)
    linear_bwd_w(d_out, x_last, g[lay.out], g[lay.out + 1], act=act, amax=a_out)  # lin_out
    d_x = f(x_last.shape[0], H)
    linear_bwd_x(d_out, prm[lay.out], x_last, d_x, act=act, sw=swt(lay.out), amax=a_out)
    d_zl = torch.zeros((R, Cl), dtype=torch.float32, device=dev) if zero_d_zl else None
    for b in reversed(range(lay.nb)):
        xb, net = blocks[b]
        i = lay.blk(b)
        d_y = d_x                                                                      # gradient of the block's output
        a_y = grad_reduce(d_y, g[i + 3], f16)
        linear_bwd_w(d_y, net, g[i + 2], g[i + 3], act=act, amax=a_y)             # fc_1
        d_net = torch.empty_like(net)
        linear_bwd_x(d_y, prm[i + 2], net, d_net, act=act, sw=swt(i + 2), amax=a_y)
        a_net = grad_reduce(d_net, g[i + 1], f16)
        linear_bwd_w(d_net, xb, g[i], g[i + 1], act=act, amax=a_net)              # fc_0
        linear_bwd_x(d_net, prm[i], xb, d_y, act=act, accumulate=True, sw=swt(i), amax=a_net)  # d_xb = d_y + (d_net W0) act'(xb), in place
        d_xb = d_y
        if b < lay.cl:                                                                 # lin_z[b]: its own dY is d_xb
            j = lay.lz(b)
            a_xb = grad_reduce(d_xb, g[j + 1], f16)
            linear_bwd_w(d_xb, zl, g[j], g[j + 1], amax=a_xb)
            if d_zl is None:
                d_zl = f(R, Cl)
                linear_bwd_x(d_xb, prm[j], None, d_zl, sw=swt(j), amax=a_xb)
            else:
                linear_bwd_x(d_xb, prm[j], None, d_zl, accumulate=True, sw=swt(j), amax=a_xb)
        if b == lay.cl:                                                                # the mean's transpose: rows P -> R
            d_x = f(R, H)
            check(L.diner_train_view_mean(_p(d_xb), P * H, NV, _p(d_x), 1, st), "diner_train_view_mean(bwd)")
        else:
            d_x = d_xb
    a_x = grad_reduce(d_x, g[1], f16)
    linear_bwd_w(d_x, inp, g_in, g[1], amax=a_x)                                  # lin_in
    return d_x, a_x, d_zl


class _RenderGenFn(torch.autograd.Function):
    """(rays, latent, poses, focal, c, image_shape, depths, *mlp_params) -> (rgb, depth, weights) for fixed samples, any shape of the
    envelope.  Same contract as ``training._RenderFn`` (``cams``: the caller's leaves, whose versions backward() checks).
    ``ix``: the latent lookup -- None (bilinear / border), a DinerLatentIndex, or an int: the bicubic lookup with that DINER_INDEX_PAD_*
    (16-float tap records and the _bc entry points of csrc/train_gen_bc.hip)."""

    @staticmethod
    def forward(ctx, renderer, scene, ix, keep, cams, shape, f16, z, rays, latent, poses, focal, c_, image_shape, depths, *params):
        L = _lib.lib()
        rays = rays.detach()
        dev = rays.device
        st = _st(dev)
        SB, NR, K = z.shape
        NV, P = scene.NV, NR * K
        R = NV * P
        lay, act = _Layout(shape), Act(shape.beta)
        H, F = shape.d_hidden, shape.num_freqs
        ld_in = 8 * (F + 1)
        f = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
        lat, lat_nhwc, ctx.lat_packed = prepare_latent(L, latent, dev, st)
        prm = [p.detach().to(torch.float32).contiguous() for p in params]
        remember_versions(ctx, params, latent, cams)
        w_in = torch.zeros((H, ld_in), dtype=torch.float32, device=dev)   # lin_in's weight, zero-padded to the input's ld_in columns
        w_in[:, :shape.d_in] = prm[0]

        def sw(i):   # f16x3: the pre-split planes of weight i (mlp_params order); None = the fp32 GEMM
            return renderer._weight_split_cache.get(params[i], w_in if i == 0 else prm[i], False) if f16 else None

        rgbsigma = f(SB, NR, K, 4)
        bicubic = isinstance(ix, int)
        ixp = C.byref(ix) if ix is not None and not bicubic else None
        saved = []
        for sb in range(SB):
            inp, zl, taps = f(R, ld_in), f(R, scene.C), f(R, 16 if bicubic else 8)
            if bicubic:
                check(L.diner_train_point_inputs_gen_bc(C.byref(scene), ix, _p(lat_nhwc), _p(rays), _p(z), NR, K, sb, _p(inp), ld_in, _p(zl),
                                                        _p(taps), st), "diner_train_point_inputs_gen_bc")
            else:
                check(L.diner_train_point_inputs_gen(C.byref(scene), ixp, _p(lat_nhwc), _p(rays), _p(z), NR, K, sb, _p(inp), ld_in, _p(zl),
                                                     _p(taps), st), "diner_train_point_inputs_gen")
            blocks, x, out = schedule_forward(L, inp, zl, prm, w_in, lay, act, sw, NV, P, st)
            check(L.diner_train_head(_p(out), None, None, P * 4, _p(rgbsigma[sb]), 0, st), "diner_train_head")  # pixelnerf.py:139-143
            saved.append((inp, zl, taps, blocks, x, out))
        N = SB * NR
        rgb, depth, weights = f(SB, NR, 3), f(SB, NR), f(SB, NR, K)
        check(L.diner_composite(_p(rays), _p(z), _p(rgbsigma), N, K, int(bool(renderer.white_bkgd)), _p(rgb), _p(depth), _p(weights), None, st),
              "diner_composite")
        ctx.renderer, ctx.scene, ctx.rays, ctx.z, ctx.rgbsigma = renderer, scene, rays, z, rgbsigma
        ctx.saved_acts, ctx.prm, ctx.w_in, ctx.lat_shape = saved, prm, w_in, tuple(latent.shape)
        ctx.keep = (lat, lat_nhwc, keep)
        ctx.shape, ctx.ix = shape, ix
        ctx.f16, ctx.params = bool(f16), params
        ctx.cam_shapes = [tuple(t.shape) for t in (poses, focal, c_, image_shape, depths)]
        return rgb, depth, weights

    @staticmethod
    def backward(ctx, d_rgb, d_depth, d_weights):
        L = _lib.lib()
        check_versions(ctx, "diner_amd.training_gen")
        # which geometric leaves want a gradient (inputs 8 and 10..14: rays, poses, focal, c, image_shape, depths)
        want = dict(zip(CAMERA_INPUTS, (ctx.needs_input_grad[8],) + tuple(ctx.needs_input_grad[10:15])))
        cam_any = any(want.values())
        scene, rays, z, rgbsigma, prm, shape = ctx.scene, ctx.rays, ctx.z, ctx.rgbsigma, ctx.prm, ctx.shape
        lay, act = _Layout(shape), Act(shape.beta)
        H, ld_in = shape.d_hidden, ctx.w_in.shape[1]
        dev = rays.device
        st = _st(dev)
        SB, NR, K = z.shape
        NV, P = scene.NV, NR * K
        R = NV * P
        f = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
        d_rgbsigma, d_far = composite_backward(L, ctx, d_rgb, d_depth, d_weights, want["rays"], st)
        cam_bufs = None
        if cam_any:
            cam_bufs, ws = camera_grad_buffers(L, want, scene, SB, NR, K, dev)
        bicubic = isinstance(ctx.ix, int)
        ixp = C.byref(ctx.ix) if ctx.ix is not None and not bicubic else None
        lat_nhwc = ctx.keep[1]
        g = [torch.zeros_like(p) for p in prm]          # parameter gradients (fp32, accumulated atomically)
        g_in = torch.zeros_like(ctx.w_in)
        SBl, NVl, Cl, hl, wl = ctx.lat_shape
        d_lat_nhwc = torch.zeros((SBl, NVl, hl, wl, Cl), dtype=torch.float32, device=dev)
        f16 = ctx.f16   # f16x3: every gradient operand is scaled by its measured max|.| (grad_reduce), dX reads the transposed planes

        def swt(i):
            return ctx.renderer._weight_split_cache.get(ctx.params[i], ctx.w_in if i == 0 else prm[i], True) if f16 else None

        for sb in range(SB):
            inp, zl, taps, blocks, x_last, out = ctx.saved_acts[sb]
            d_out = f(x_last.shape[0], 4)
            check(L.diner_train_head(_p(out), _p(rgbsigma[sb]), _p(d_rgbsigma[sb]), P * 4, _p(d_out), 1, st), "diner_train_head(bwd)")
            d_x, a_x, d_zl = schedule_backward(L, inp, zl, blocks, x_last, d_out, prm, g, g_in, lay, act, swt, f16, NV, P, scene.C, st,
                                               zero_d_zl=lay.nlz == 0 and cam_any)
            if cam_any:   # lin_in's input gradient, then the transpose of the point inputs to the geometric leaves
                d_in = f(R, ld_in)
                linear_bwd_x(d_x, ctx.w_in, None, d_in, sw=swt(0), amax=a_x)
                bwd, name = ((L.diner_train_point_inputs_backward_gen_bc, "diner_train_point_inputs_backward_gen_bc") if bicubic else
                             (L.diner_train_point_inputs_backward_gen, "diner_train_point_inputs_backward_gen"))
                check(bwd(C.byref(scene), ctx.ix if bicubic else ixp, _p(lat_nhwc), _p(rays), _p(z), NR, K, sb, _p(d_in), ld_in, _p(d_zl),
                          _p(d_far), _p(ws), *map(_p, cam_bufs), st), name)
            if lay.nlz and bicubic:
                check(L.diner_train_bicubic_scatter(_p(d_zl), _p(taps), P, scene.C, scene.h, scene.w, NV, sb, _p(d_lat_nhwc), st),
                      "diner_train_bicubic_scatter")
            elif lay.nlz:
                check(L.diner_train_bilinear_scatter(_p(d_zl), _p(taps), P, scene.C, scene.h, scene.w, NV, sb, _p(d_lat_nhwc), st),
                      "diner_train_bilinear_scatter")
        d_lat = latent_grad_out(L, d_lat_nhwc, ctx.lat_shape, ctx.lat_packed, st)
        g[0] = g_in[:, :shape.d_in].contiguous()
        cam = camera_grads_out(cam_bufs, ctx.cam_shapes)
        return (None, None, None, None, None, None, None, None, cam[0], d_lat) + cam[1:] + tuple(g)


def render_with_grad(renderer, model, rays, z, scene, shape, keep=None, f16=False):
    """rgb, depth, weights = composite(model, rays, z) for a model of any shape of the envelope, with gradients to every fusion-MLP
    parameter, encoder.latent, and the rays, cameras and depth maps when they require grad.  ``f16``: the GEMMs in f16x3."""
    if shape.combine_layer >= shape.n_blocks and scene.NV != 1:
        raise NotImplementedError(f"combine_layer={shape.combine_layer} >= n_blocks={shape.n_blocks} (no mean over views) with NV={scene.NV}: "
                                  "the reference supports it for one view only (pixelnerf.py:137)")
    params = mlp_params(model.mlp_fine)
    # the encoder's lookup mode (None: bilinear / border; an int: bicubic with that padding, renderer.bicubic_index)
    pad = renderer._bicubic_pad(model)
    ix = int(pad) if pad is not None else renderer._latent_index(model)
    cams, f32 = camera_inputs(model, rays)
    return _RenderGenFn.apply(renderer, scene, ix, keep, cams, shape, bool(f16), z, *f32[:1], model.encoder.latent, *f32[1:], *params)

